#!/usr/bin/env python3
"""VOC evaluation of a VOC07-test-sized synthetic result: the host evaluate_detections against the device evaluator.

    python tools/voc_eval_probe.py [--images 4952] [--batch 32] [--step-ms 6.85] > profiles/voc_eval_probe.json

Synthetic set, fixed seed: --images images, 20 classes, 10 detections per class and image in descending score order
(half of them jittered ground-truth boxes), 1-4 ground-truth boxes per image.  Timed in this (fresh) process:
  host    evaluate.evaluate_detections(..., stable=True) on the host copy, wall clock;
  add     DeviceVOCEvaluator.add per batch of --batch images (one ct_voc_match launch), HIP events around each call of
          a second pass over the data set after a full warm-up pass; median and inter-quartile range;
  finish  DeviceVOCEvaluator.finish() (status read, key sort, ct_voc_pr, AP read-back), wall clock, second call.
--step-ms is the pipeline step the add is set against (README: RFBNet-300 bs 32).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ctdet import evaluate  # noqa: E402

T, PER_CLASS = 20, 10


def synthetic(n, seed=2007):
    rng = np.random.RandomState(seed)
    classes = ['__background__'] + ['c%02d' % j for j in range(1, T + 1)]
    ids = ['%06d' % (i + 1) for i in range(n)]
    gt = {c: {} for c in classes[1:]}
    dets = np.zeros((n, T, PER_CLASS, 5), np.float32)
    xy = rng.uniform(0, 400, (n, T, PER_CLASS, 2))
    dets[..., :2], dets[..., 2:4] = xy, xy + rng.uniform(10, 200, (n, T, PER_CLASS, 2))
    dets[..., 4] = -np.sort(-rng.beta(0.5, 2.0, (n, T, PER_CLASS)).clip(0.011, 1.0), axis=2)
    for i, iid in enumerate(ids):
        k = rng.randint(1, 5)
        labels = rng.randint(1, T + 1, k)
        p = rng.randint(0, 380, (k, 2))
        boxes = np.concatenate([p, p + rng.randint(20, 120, (k, 2))], 1)
        for j in np.unique(labels):
            bb = boxes[labels == j]
            gt[classes[j]][iid] = {'bbox': bb, 'difficult': rng.rand(len(bb)) < 0.1}
            rows = rng.choice(PER_CLASS, PER_CLASS // 2, replace=False)
            dets[i, j - 1, rows, :4] = bb[rng.randint(0, len(bb), len(rows))] - 1 + rng.uniform(-3, 3, (len(rows), 4))
    return classes, ids, gt, dets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=4952)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--step-ms', type=float, default=6.85)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'voc_eval_probe needs a HIP device'
    dev = 'cuda:0'
    n, B = a.images, a.batch
    classes, ids, gt, dets = synthetic(n)
    count = np.full((n, T), PER_CLASS, np.int32)

    all_boxes = [[[]] * n] + [[dets[i, c] for i in range(n)] for c in range(T)]
    t0 = time.perf_counter()
    host_aps, host_mean = evaluate.evaluate_detections(all_boxes, ids, gt, classes, stable=True)
    host_s = time.perf_counter() - t0

    ev = evaluate.DeviceVOCEvaluator(gt, classes, ids, dev)
    pad = (-n) % B
    d_dets = torch.from_numpy(np.concatenate([dets, np.zeros((pad,) + dets.shape[1:], np.float32)])).to(dev)
    d_count = torch.from_numpy(np.concatenate([count, np.zeros((pad, T), np.int32)])).to(dev)
    index = [[s + k if s + k < n else -1 for k in range(B)] for s in range(0, n, B)]
    samples = []
    for timed in (False, True):                     # a full warm-up pass, then the timed one
        ev.reset()
        for b, idx in enumerate(index):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ev.add(d_dets[b * B:(b + 1) * B], d_count[b * B:(b + 1) * B], idx)
            e1.record()
            if timed:
                samples.append((e0, e1))
        torch.cuda.synchronize()
    us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in samples]
    finish_ms = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aps, mean = ev.finish()
        finish_ms.append((time.perf_counter() - t0) * 1e3)
    q = statistics.quantiles(us, n=4)
    add_us = statistics.median(us)
    out = {'probe': 'VOC07 11-point evaluation, host evaluate_detections vs DeviceVOCEvaluator',
           'device': torch.cuda.get_device_name(0), 'images': n, 'classes': T, 'rows': int(count.sum()),
           'ground_truth_boxes': int(ev.G), 'batch': B, 'adds': len(us),
           'host_evaluate_detections_s': round(host_s, 2),
           'add_us_median': round(add_us, 1), 'add_us_iqr': round(q[2] - q[0], 1),
           'finish_ms_first': round(finish_ms[0], 2), 'finish_ms': round(finish_ms[1], 2),
           'device_total_ms': round(add_us * len(us) / 1e3 + finish_ms[1], 2),
           'pipeline_step_ms': a.step_ms, 'add_share_of_step': round(add_us / 1e3 / a.step_ms, 4),
           'mean_ap_host': host_mean, 'mean_ap_device': mean, 'aps_equal': aps == host_aps}
    print(json.dumps(out))
    assert aps == host_aps and mean == host_mean, 'device and host evaluation differ'


if __name__ == '__main__':
    main()
