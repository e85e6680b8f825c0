#!/usr/bin/env python3
"""What a four-image mosaic batch costs next to the plain device path of the input pipeline.

    python tools/mosaic_probe.py            # prints one JSON line, writes profiles/mosaic_probe.json

S = 300 and 512, batch 32, synthetic 500x375 images with 1 / 3 / 8 boxes.  Two variants:
  plain    32 samples: ops.AugPlanner (ct_aug_plan) + Augmenter.render (ct_preproc_augment), what
           preproc.batch_device runs
  mosaic   128 samples: AugPlanner.mosaic (ct_aug_plan_mosaic) + Augmenter.render_mosaic (ct_preproc_augment_mosaic),
           what preproc.mosaic_device runs
Per configuration, warm, median of --iters batches:
  dev_ms        plan + render between two events on the stream: the one H2D copy of the sample records and boxes,
                the planner's launches and the render launch (the image upload is enqueued before the first event)
  call_host_ms  host wall time of those two calls (packing the records into the staging buffer, enqueueing)
  pack_host_ms  host wall time of packing the inputs: staging the images into pinned memory and enqueueing their
                copy (Augmenter.upload), and building the ct_aug_sample records and the box table
  upload_bytes  images + sample records + boxes
Every (variant, round) runs in a fresh process, the variants alternating, so neither owes anything to the other's
warm caches and drift of the shared host shows as spread between rounds: each figure is the median over the rounds,
with the rounds' minimum and maximum beside it.  There is no pass threshold.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, MEANS, P = 375, 500, (104.0, 117.0, 123.0), 0.6
SIZES, BOXES, VARIANTS = (300, 512), (1, 3, 8), ('plain', 'mosaic')


def child(variant, batch, iters, round_no):
    sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    from ctdet import ops
    from data.data_augment import INTERP_OF_DRAW
    assert torch.cuda.is_available(), 'mosaic_probe needs a HIP device'
    per = 4 if variant == 'mosaic' else 1
    m = batch * per
    r = np.random.RandomState(5)
    images = [r.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(m)]

    def boxes(n, seed):
        q = np.random.RandomState(seed)
        x1, y1 = q.uniform(0, W * 0.7, n), q.uniform(0, H * 0.7, n)
        w, h = q.uniform(W * 0.08, W * 0.3, n), q.uniform(H * 0.08, H * 0.3, n)
        return np.stack([x1, y1, np.minimum(x1 + w, W), np.minimum(y1 + h, H), q.randint(1, 21, n)], 1).astype(np.float32)

    rows = []
    for S in SIZES:
        aug = ops.Augmenter(S, MEANS, 'cuda', m)
        planner = ops.AugPlanner('cuda', 1234, P, INTERP_OF_DRAW, MEANS, m, m * max(BOXES))
        out = torch.empty(batch, 3, S, S, device='cuda')
        for g in BOXES:
            tgs = [boxes(g, 100 * g + i) for i in range(m)]
            it = [round_no * 1000]

            def pack():
                offs = aug.upload(images)
                s = np.zeros(m, dtype=ops.AUG_SAMPLE_DTYPE)
                s['src_off'], s['H'], s['W'], s['cls'], s['weight'] = offs, H, W, -1, 1.0
                s['image'] = np.arange(m) // per
                s['box_begin'] = np.arange(m) * g
                s['box_end'] = s['box_begin'] + g
                s['sample_id'] = np.arange(m, dtype=np.uint64) + np.uint64(it[0] * m)
                it[0] += 1
                return s, np.concatenate(tgs, 0)

            def run(s, bx):
                if variant == 'mosaic':
                    plans, tiles, packed = planner.mosaic(s, bx, batch, g, S, S // 4)
                    return aug.render_mosaic(plans, tiles, batch, out), packed
                plans, packed = planner(s, bx, batch, g)
                return aug.render(plans, batch, out), packed

            for _ in range(5):
                run(*pack())
            st = planner.check()
            t_dev, t_call, t_pack = [], [], []
            for _ in range(iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s, bx = pack()
                t1 = time.perf_counter()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                e0.record()
                run(s, bx)
                e1.record()
                t3 = time.perf_counter()
                torch.cuda.synchronize()
                t_dev.append(e0.elapsed_time(e1)); t_call.append((t3 - t2) * 1e3); t_pack.append((t1 - t0) * 1e3)
            rows.append(dict(size=S, boxes=g, samples=m, dev_ms=statistics.median(t_dev),
                             call_host_ms=statistics.median(t_call), pack_host_ms=statistics.median(t_pack),
                             upload_bytes=int(sum((im.size + 15) // 16 * 16 for im in images) + planner.upload_bytes),
                             rows=int(st[3])))
    print(json.dumps(dict(variant=variant, device=torch.cuda.get_device_name(0), rows=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=15)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--child', choices=VARIANTS)
    ap.add_argument('--round', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mosaic_probe.json'))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.batch, a.iters, a.round)
    got = {v: [] for v in VARIANTS}
    device = None
    for rnd in range(a.rounds):
        for v in VARIANTS:                                  # alternating; a failed child ends the probe
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', v, '--batch', str(a.batch),
                                '--iters', str(a.iters), '--round', str(rnd)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit('mosaic_probe: the %s child of round %d ended with %d' % (v, rnd, r.returncode))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            device = rec['device']
            got[v].append(rec['rows'])
            sys.stderr.write('round %d %s done\n' % (rnd, v))
            sys.stderr.flush()
    rows = []
    for v in VARIANTS:
        for k, first in enumerate(got[v][0]):
            row = dict(variant=v, size=first['size'], boxes=first['boxes'], samples=first['samples'],
                       upload_bytes=first['upload_bytes'])
            for key in ('dev_ms', 'call_host_ms', 'pack_host_ms'):
                vals = [rnd[k][key] for rnd in got[v]]
                row[key] = round(statistics.median(vals), 4)
                row[key + '_min_max'] = [round(min(vals), 4), round(max(vals), 4)]
            rows.append(row)
    line = json.dumps(dict(tool='mosaic_probe', device=device, batch=a.batch, image='%dx%d' % (W, H), iters=a.iters,
                           rounds=a.rounds, rows=rows))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
