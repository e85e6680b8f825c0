#!/usr/bin/env python3
"""What the random affine stage costs behind the plain and the mosaic path of the device input pipeline.

    python tools/affine_probe.py            # prints one JSON line, writes profiles/affine_probe.json

S = 300 and 512, batch 32, synthetic 500x375 images with 3 boxes each.  Two variants, as tools/mosaic_probe.py has
them: `plain` (32 samples, ct_aug_plan + ct_preproc_augment) and `mosaic` (128 samples, ct_aug_plan_mosaic +
ct_preproc_augment_mosaic).  The stage runs on what the variant rendered (ops.AffineWarp, default parameters, p = 1:
every image is resampled; the fallback's copies are counted in `copied`).  Per configuration, warm:
  step_ms       the input step WITHOUT the stage, plan + render between two events, median of --iters batches, with
                the minimum and maximum of those batches beside it: the spread the stage's time has to be read against
  plan_us       ct_aug_affine_plan, both launches  } --calls back-to-back raw C calls between two events, divided by
  warp_us       ct_preproc_warp_affine             } --calls; median of --iters such windows
  mixup_us      ct_mixup_blend on the same [B,3,S,S] shape, timed the same way: a streaming kernel over 1.5x the
                warp's bytes (two reads, one write), the yardstick
  warp_tbs      the warp's bytes (read + write, 2*B*3*S*S*4) over warp_us; warp_hbm_share = that over --hbm-tbs.  The
                batch (69 MB at S = 300, 201 MB at S = 512, both buffers) fits the 256 MiB Infinity Cache, so a rate
                above the HBM figure is possible and is a cache rate, not an HBM rate
  warp_over_mixup   warp_us / mixup_us; per byte: (warp_us / warp bytes) / (mixup_us / mixup bytes)
  plan_kernel_us, pack_kernel_us, warp_kernel_us   the library's own launch records (ct_profile_enable), medians
Every (variant, round) runs in a fresh process, the variants alternating, --rounds times (default 2): each figure is
the median over the rounds with the rounds' minimum and maximum beside it.  There is no pass threshold.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, MEANS, P, BOXES = 375, 500, (104.0, 117.0, 123.0), 0.6, 3
SIZES, VARIANTS = (300, 512), ('plain', 'mosaic')
KEYS = ('step_ms', 'plan_us', 'warp_us', 'mixup_us', 'plan_kernel_us', 'pack_kernel_us', 'warp_kernel_us')


def child(variant, batch, iters, calls, round_no):
    sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    from ctdet import ops
    from ctdet._lib import ProfileRecord, check, lib
    from data.data_augment import INTERP_OF_DRAW
    assert torch.cuda.is_available(), 'affine_probe needs a HIP device'
    L = lib()
    per = 4 if variant == 'mosaic' else 1
    m = batch * per
    r = np.random.RandomState(5)
    images = [r.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(m)]
    q = np.random.RandomState(7)
    x1, y1 = q.uniform(0, W * 0.7, m * BOXES), q.uniform(0, H * 0.7, m * BOXES)
    bw, bh = q.uniform(W * 0.08, W * 0.3, m * BOXES), q.uniform(H * 0.08, H * 0.3, m * BOXES)
    bx = np.stack([x1, y1, np.minimum(x1 + bw, W), np.minimum(y1 + bh, H), q.randint(1, 21, m * BOXES)], 1).astype(np.float32)
    border = [float(np.float32(int(v)) - np.float32(v)) for v in MEANS]
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731

    def window(fn):
        """microseconds per call of `calls` back-to-back calls, median of `iters` windows"""
        for _ in range(3):
            fn()
        got = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            got.append(e0.elapsed_time(e1) * 1e3 / calls)
        return statistics.median(got)

    rows = []
    for S in SIZES:
        aug = ops.Augmenter(S, MEANS, 'cuda', m)
        planner = ops.AugPlanner('cuda', 1234, P, INTERP_OF_DRAW, MEANS, m, m * BOXES)
        warp = ops.AffineWarp('cuda', 1234, ops.AffineParams())
        x = torch.empty(batch, 3, S, S, device='cuda')
        it = [round_no * 1000]

        def pack():
            s = np.zeros(m, dtype=ops.AUG_SAMPLE_DTYPE)
            s['src_off'], s['H'], s['W'], s['cls'], s['weight'] = aug.upload(images), H, W, -1, 1.0
            s['image'] = np.arange(m) // per
            s['box_begin'] = np.arange(m) * BOXES
            s['box_end'] = s['box_begin'] + BOXES
            s['sample_id'] = np.arange(m, dtype=np.uint64) + np.uint64(it[0] * m)
            it[0] += 1
            return s

        def step(s):
            if variant == 'mosaic':
                plans, tiles, packed = planner.mosaic(s, bx, batch, BOXES, S, S // 4)
                return aug.render_mosaic(plans, tiles, batch, x), packed
            plans, packed = planner(s, bx, batch, BOXES)
            return aug.render(plans, batch, x), packed

        for _ in range(5):
            _, packed = step(pack())
        planner.check()
        t_step = []
        for _ in range(iters):
            s = pack()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            _, packed = step(s)
            e1.record()
            torch.cuda.synchronize()
            t_step.append(e0.elapsed_time(e1))
        # the stage on that batch: raw C calls on buffers allocated once
        ids = list(range(9000 + 100 * round_no, 9000 + 100 * round_no + batch))
        records, packed_out = warp.plan(packed, ids, batch, S)
        st = warp.check()
        flags = records.view(batch, ops.AFFINE_BYTES).cpu().numpy().view(ops.AFFINE_DTYPE)['flags'].reshape(-1)
        n_rows = packed.truths.shape[0]
        ids_d = torch.tensor(ids, dtype=torch.int64, device='cuda')
        ws_bytes = L.ct_aug_affine_plan_workspace_bytes(batch, n_rows)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
        status = torch.empty(4, dtype=torch.int32, device='cuda')
        prm = warp.params.struct()
        y, x2 = torch.empty_like(x), torch.randn_like(x)
        lam = torch.full((batch,), 0.4, device='cuda')
        bd = (C.c_float * 3)(*border)

        def run_plan():
            check(L.ct_aug_affine_plan(packed.truths.data_ptr(), packed.gt_off.data_ptr(), ids_d.data_ptr(), batch, n_rows, S,
                                       1234, C.byref(prm), records.data_ptr(), packed_out.truths.data_ptr(),
                                       packed_out.gt_off.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes, stream()),
                  'ct_aug_affine_plan')

        def run_warp():
            check(L.ct_preproc_warp_affine(x.data_ptr(), records.data_ptr(), batch, S, bd, y.data_ptr(), stream()),
                  'ct_preproc_warp_affine')

        def run_mixup():
            check(L.ct_mixup_blend(x.data_ptr(), x2.data_ptr(), lam.data_ptr(), batch, 3 * S * S, y.data_ptr(), stream()),
                  'ct_mixup_blend')

        row = dict(size=S, samples=m, rows_in=int(packed.gt_off[-1]), rows_out=int(st[3]), fallback=int(st[2]),
                   copied=int((flags & 4 != 0).sum()), step_ms=statistics.median(t_step), step_ms_batches=[min(t_step), max(t_step)],
                   plan_us=window(run_plan), warp_us=window(run_warp), mixup_us=window(run_mixup))
        torch.cuda.synchronize()
        L.ct_profile_enable(1)
        for _ in range(iters):
            run_plan()
            run_warp()
        n = C.c_int(0)
        recs = (ProfileRecord * 4096)()
        check(L.ct_profile_collect(recs, 4096, C.byref(n)), 'ct_profile_collect')
        L.ct_profile_enable(0)
        for key, kernel in (('plan_kernel_us', b'affine_plan_kernel'), ('pack_kernel_us', b'affine_pack_kernel'),
                            ('warp_kernel_us', b'warp_affine_kernel')):
            row[key] = statistics.median([recs[i].ms for i in range(min(n.value, 4096)) if recs[i].name == kernel]) * 1e3
        rows.append(row)
    print(json.dumps(dict(variant=variant, device=torch.cuda.get_device_name(0), rows=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=15)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--hbm-tbs', type=float, default=4.85)
    ap.add_argument('--child', choices=VARIANTS)
    ap.add_argument('--round', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'affine_probe.json'))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.batch, a.iters, a.calls, a.round)
    got = {v: [] for v in VARIANTS}
    device = None
    for rnd in range(a.rounds):
        for v in VARIANTS:                                  # alternating; a failed child ends the probe
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', v, '--batch', str(a.batch),
                                '--iters', str(a.iters), '--calls', str(a.calls), '--round', str(rnd)],
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit('affine_probe: the %s child of round %d ended with %d' % (v, rnd, r.returncode))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            device = rec['device']
            got[v].append(rec['rows'])
            sys.stderr.write('round %d %s done\n' % (rnd, v))
            sys.stderr.flush()
    rows = []
    for v in VARIANTS:
        for k, first in enumerate(got[v][0]):
            S = first['size']
            row = dict(variant=v, size=S, samples=first['samples'], rows_in=first['rows_in'],
                       rows_out=[rnd[k]['rows_out'] for rnd in got[v]], copied=[rnd[k]['copied'] for rnd in got[v]],
                       step_ms_batches=[round(min(rnd[k]['step_ms_batches'][0] for rnd in got[v]), 4),
                                        round(max(rnd[k]['step_ms_batches'][1] for rnd in got[v]), 4)])
            for key in KEYS:
                vals = [rnd[k][key] for rnd in got[v]]
                row[key] = round(statistics.median(vals), 4)
                row[key + '_min_max'] = [round(min(vals), 4), round(max(vals), 4)]
            warp_bytes = 2 * a.batch * 3 * S * S * 4
            row['warp_bytes'] = warp_bytes
            row['warp_tbs'] = round(warp_bytes / (row['warp_us'] * 1e-6) / 1e12, 3)
            row['warp_hbm_share'] = round(row['warp_tbs'] / a.hbm_tbs, 3)
            row['warp_over_mixup'] = round(row['warp_us'] / row['mixup_us'], 3)
            row['warp_over_mixup_per_byte'] = round(row['warp_us'] / row['mixup_us'] * 1.5, 3)
            row['stage_over_step'] = round((row['plan_us'] + row['warp_us']) * 1e-3 / row['step_ms'], 3)
            rows.append(row)
    line = json.dumps(dict(tool='affine_probe', device=device, batch=a.batch, image='%dx%d' % (W, H), boxes=BOXES,
                           iters=a.iters, calls=a.calls, rounds=a.rounds, hbm_tbs=a.hbm_tbs, rows=rows))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
