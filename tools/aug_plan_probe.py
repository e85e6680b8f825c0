#!/usr/bin/env python3
"""What the augmentation decisions of one batch cost: the host sampler against the device planner.

    python tools/aug_plan_probe.py > profiles/aug_plan_probe.json

Batch 32 at S = 300, synthetic 500x375 images with 1 / 3 / 8 / 20 boxes, with and without mixup (which doubles the
samples).  Per configuration, in one process:
  host_decide_ms   `preproc.decide` over the batch's samples: the scalar rejection sampler `preproc.batch` runs per
                   image before its one pixel launch (median of --rounds batches, host wall time)
  dev_ms           ops.AugPlanner between two events on the stream, warm, median: its one H2D copy of the samples
                   and boxes and ct_aug_plan's two launches; kernels_ms: the two launches alone, from the library's
                   per-launch event records
  planner_host_ms  host wall time of the AugPlanner call (packing the samples and boxes, one copy, two launches)
  launches         as the library's own launch records count them (ct_profile_enable)
  upload_before    bytes the host path uploads per batch besides the images: the plan records, and the truths /
                   offset table `ops.match_batched` builds and copies
  upload_after     bytes the device path uploads: the ct_aug_sample records and the pixel boxes
Prints one JSON line.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)

from ctdet import _lib, ops  # noqa: E402
from data.data_augment import INTERP_OF_DRAW, preproc  # noqa: E402

H, W, MEANS, P = 375, 500, (104.0, 117.0, 123.0), 0.6


def boxes(n, seed):
    r = np.random.RandomState(seed)
    x1, y1 = r.uniform(0, W * 0.7, n), r.uniform(0, H * 0.7, n)
    w, h = r.uniform(W * 0.08, W * 0.3, n), r.uniform(H * 0.08, H * 0.3, n)
    return np.stack([x1, y1, np.minimum(x1 + w, W), np.minimum(y1 + h, H), r.randint(1, 21, n)], 1).astype(np.float32)


def launches_of(fn):
    """(kernel names, their summed ms) of one call, from the library's own launch records."""
    lib = _lib.lib()
    torch.cuda.synchronize()
    lib.ct_profile_enable(1)
    fn()
    recs = (_lib.ProfileRecord * 64)()
    n = _lib.C.c_int(0)
    _lib.check(lib.ct_profile_collect(recs, 64, _lib.C.byref(n)), 'ct_profile_collect')
    lib.ct_profile_enable(0)
    k = min(n.value, 64)
    return [recs[i].name.decode() for i in range(k)], sum(recs[i].ms for i in range(k))


def probe(batch, g, mixup, rounds):
    m = batch * (2 if mixup else 1)
    tgs = [boxes(g, 100 * g + i) for i in range(m)]
    host = preproc.__new__(preproc)
    host.rng, host.p, host.interp_of_draw = random.Random(7), P, INTERP_OF_DRAW
    t_host, rows = [], 0
    for _ in range(rounds):
        t0 = time.perf_counter()
        out = [host.decide((H, W, 3), tg.astype(np.float64)) for tg in tgs]
        t_host.append((time.perf_counter() - t0) * 1e3)
        rows = sum(len(o[1]) for o in out)
    samples = np.zeros(m, dtype=ops.AUG_SAMPLE_DTYPE)
    samples['H'], samples['W'], samples['cls'], samples['weight'] = H, W, -1, 1.0
    samples['image'] = np.arange(m) // (2 if mixup else 1)
    samples['box_begin'] = np.arange(m) * g
    samples['box_end'] = samples['box_begin'] + g
    bx = np.concatenate(tgs, 0)
    planner = ops.AugPlanner('cuda', 1234, P, INTERP_OF_DRAW, MEANS, m, m * g)
    it = [0]

    def run():
        samples['sample_id'] = np.arange(m, dtype=np.uint64) + np.uint64(it[0] * m)
        it[0] += 1
        return planner(samples, bx, batch, g)

    for _ in range(5):
        run()
    planner.check()
    t_dev, t_call = [], []
    for _ in range(rounds):
        samples['sample_id'] = np.arange(m, dtype=np.uint64) + np.uint64(it[0] * m)
        it[0] += 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        planner(samples, bx, batch, g)
        e1.record()
        t_call.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t_dev.append(e0.elapsed_time(e1))
    names, kernels_ms = launches_of(run)
    return dict(boxes=g, mixup=mixup, samples=m, host_decide_ms=round(statistics.median(t_host), 3),
                dev_ms=round(statistics.median(t_dev), 4), planner_host_ms=round(statistics.median(t_call), 3),
                kernels_ms=round(kernels_ms, 4), launches=names,
                upload_before=m * ops.PLAN_BYTES + rows * 24 + (batch + 1) * 4, upload_after=planner.upload_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=21)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'aug_plan_probe needs a HIP device'
    rows = [probe(a.batch, g, mix, a.rounds) for mix in (False, True) for g in (1, 3, 8, 20)]
    name = torch.cuda.get_device_name(0)
    print(json.dumps(dict(tool='aug_plan_probe', device=name, batch=a.batch, size=300, image='%dx%d' % (W, H),
                          rounds=a.rounds, rows=rows)))


if __name__ == '__main__':
    main()
