#!/usr/bin/env python3
"""What each resize filter of the device augmentation costs per batch, and tiled against gather for the two tap filters.

    python tools/aug_probe.py [--batch 32] [--reps 30] [--warmup 5]

Input: --batch seeded 375x500 uint8 images, identity plans (no crop, canvas or mirror), every image of a launch on one
filter (0 linear, 1 nearest, 2 area through ct_preproc_augment; 3 bicubic, 4 Lanczos4 through
ct_preproc_augment_taps), distortion flags 0 and 15, output sizes 300 and 512.  Time: HIP events around the launch
alone (images, plans and tables are on the device before), --warmup launches first, median of --reps.

CTDET_AUG_TILED is read once per process, so the two forms are measured in fresh child processes, in the order
tiled, gather, tiled, gather; the two runs of one form give the spread a difference has to beat.  `ms` of a row is the
median per run in that order; filters 0..2 do not depend on the switch, their four runs are four repeats.
Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)

MEANS = (104, 117, 123)
FILTERS = ('linear', 'nearest', 'area', 'cubic', 'lanczos4')
ORDER = ('tiled', 'gather', 'tiled', 'gather')


def child(a):
    import numpy as np
    import torch
    from ctdet import ops
    from ctdet._lib import check, lib
    torch.cuda.set_device(0)
    rng = np.random.RandomState(0)
    n, H, W = a.batch, 375, 500
    per = (H * W * 3 + 15) // 16 * 16
    src_h = np.zeros(n * per, np.uint8)
    for i in range(n):
        src_h[i * per:i * per + H * W * 3] = rng.randint(0, 256, H * W * 3)
    src = torch.from_numpy(src_h).cuda()
    means = (C.c_float * 3)(*MEANS)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())        # noqa: E731
    rows = []
    for S in (300, 512):
        out = torch.empty(n, 3, S, S, device='cuda')
        for interp, name in enumerate(FILTERS):
            taps_d = None
            if interp >= 3:
                t = np.zeros((n, 2, S), dtype=ops.TAP_DTYPE)
                t[:, 0], t[:, 1] = ops.tap_records(W, S, name), ops.tap_records(H, S, name)
                taps_d = torch.from_numpy(t.reshape(-1).view(np.uint8)).cuda()
            for flags in (0, 15):
                recs = (ops.AugPlan * n)()
                for i, r in enumerate(recs):
                    r.src_off, r.H, r.W = i * per, H, W
                    r.crop_l, r.crop_t, r.crop_w, r.crop_h = 0, 0, W, H
                    r.exp_w, r.exp_h, r.exp_left, r.exp_top = W, H, 0, 0
                    r.mirror, r.interp, r.flags, r.hue_delta = 0, interp, flags, 7
                    r.beta, r.alpha, r.sat_alpha = 12.5, 1.2, 0.9
                    for c in range(3):
                        r.fill[c] = MEANS[c]
                plans = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).cuda()

                def launch():
                    if taps_d is None:
                        check(lib().ct_preproc_augment(ptr(src), ptr(plans), n, S, C.cast(means, C.c_void_p), ptr(out),
                                                       stream), 'ct_preproc_augment')
                    else:
                        check(lib().ct_preproc_augment_taps(ptr(src), ptr(plans), ptr(taps_d), n, S,
                                                            C.cast(means, C.c_void_p), ptr(out), stream),
                              'ct_preproc_augment_taps')
                for _ in range(a.warmup):
                    launch()
                torch.cuda.synchronize()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
                for e0, e1 in ev:
                    e0.record()
                    launch()
                    e1.record()
                torch.cuda.synchronize()
                ms = [e0.elapsed_time(e1) for e0, e1 in ev]
                rows.append({'S': S, 'filter': name, 'flags': flags, 'ms': round(statistics.median(ms), 4),
                             'min_ms': round(min(ms), 4), 'checksum': float(out.double().sum().item())})
    print(json.dumps({'device': torch.cuda.get_device_name(0), 'rows': rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for form in ORDER:                              # fresh processes: the switch is read once
        env = dict(os.environ, CTDET_AUG_TILED='0' if form == 'gather' else '1')
        cmd = [sys.executable, os.path.abspath(__file__), '--child', '--batch', str(a.batch), '--reps', str(a.reps),
               '--warmup', str(a.warmup)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit('aug_probe: the %s run exited with status %d' % (form, r.returncode))
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    rows = []
    for i, base in enumerate(runs[0]['rows']):
        ms = [run['rows'][i]['ms'] for run in runs]
        sums = {run['rows'][i]['checksum'] for run in runs}
        row = {'S': base['S'], 'filter': base['filter'], 'flags': base['flags'], 'order': list(ORDER), 'ms': ms,
               'same_output_in_all_runs': len(sums) == 1}
        if base['filter'] in ('cubic', 'lanczos4'):
            tiled, gather = [ms[0], ms[2]], [ms[1], ms[3]]
            row.update(tiled_ms=round(statistics.mean(tiled), 4), gather_ms=round(statistics.mean(gather), 4),
                       spread_ms=round(max(abs(tiled[0] - tiled[1]), abs(gather[0] - gather[1])), 4))
            row['tiled_faster_beyond_spread'] = row['gather_ms'] - row['tiled_ms'] > row['spread_ms']
        rows.append(row)
    linear = {(r['S'], r['flags']): statistics.median(r['ms']) for r in rows if r['filter'] == 'linear'}
    for r in rows:                                  # the tap filters as they run by default: the tiled runs
        r['over_linear'] = round(r.get('tiled_ms', statistics.median(r['ms'])) / linear[(r['S'], r['flags'])], 2)
    print(json.dumps({'probe': 'aug_filters', 'batch': a.batch, 'source': '375x500', 'reps': a.reps, 'warmup': a.warmup,
                      'device': runs[0]['device'], 'rows': rows}))


if __name__ == '__main__':
    main()
