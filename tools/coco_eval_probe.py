#!/usr/bin/env python3
"""COCO bbox evaluation of a val2017-sized synthetic result: the host twin against the device evaluator.

    python tools/coco_eval_probe.py [--images 5000] [--batch 32] [--step-ms 6.85] > profiles/coco_eval_probe.json

Synthetic set, fixed seed: --images images, 80 classes, about 7 ground-truth boxes per image over 1-4 of its classes
(a tenth of them crowds), 100 detection rows per image: 10 classes x 10 rows in descending score order, the image's own
classes among them with half of their rows jittered ground-truth boxes.  Timed in this (fresh) process:
  host    evaluate.coco_eval_arrays + coco_summarize on the host copy, wall clock (the reference's COCOeval runs the same
          Python loops; it is not timed here);
  add     DeviceCOCOEvaluator.add per batch of --batch images (one ct_coco_match launch), HIP events around each call
          of a second pass over the data set after a full warm-up pass; median and inter-quartile range;
  finish  DeviceCOCOEvaluator.finish() (status read, key sort, ct_coco_accumulate, read-back of the three arrays, the
          means on the host), wall clock, second call.
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

T, CLASSES_PER_IMAGE, PER_CLASS = 80, 10, 10


def synthetic(n, seed=2017):
    rng = np.random.RandomState(seed)
    category_ids = [0] + sorted(rng.choice(np.arange(1, 91), T, replace=False).tolist())
    image_ids = rng.choice(np.arange(1, 600000), n, replace=False).tolist()
    dets = np.zeros((n, T, PER_CLASS, 5), np.float32)
    count = np.zeros((n, T), np.int32)
    anns = []
    for i, img in enumerate(image_ids):
        own = rng.choice(T, rng.randint(1, 5), replace=False)
        rest = rng.choice(np.setdiff1d(np.arange(T), own), CLASSES_PER_IMAGE - len(own), replace=False)
        for c in np.concatenate([own, rest]):
            xy = rng.uniform(0, 400, (PER_CLASS, 2))
            dets[i, c, :, :2], dets[i, c, :, 2:4] = xy, xy + rng.uniform(8, 220, (PER_CLASS, 2))
            dets[i, c, :, 4] = -np.sort(-rng.beta(0.5, 2.0, PER_CLASS).clip(0.011, 1.0))
            count[i, c] = PER_CLASS
        per = np.maximum(1, rng.multinomial(7, np.ones(len(own)) / len(own)))
        for c, k in zip(own, per):
            p = np.round(rng.uniform(0, 380, (k, 2)), 2)
            wh = np.round(np.exp(rng.uniform(np.log(8), np.log(250), (k, 2))), 2)
            for b in range(k):
                anns.append({'id': len(anns) + 1, 'image_id': img, 'category_id': category_ids[c + 1],
                             'bbox': [float(p[b, 0]), float(p[b, 1]), float(wh[b, 0]), float(wh[b, 1])],
                             'area': float(np.round(wh[b, 0] * wh[b, 1] * rng.uniform(0.5, 1), 2)),
                             'iscrowd': int(rng.rand() < 0.1)})
            rows = rng.choice(PER_CLASS, PER_CLASS // 2, replace=False)
            pick = rng.randint(0, k, len(rows))
            jit = rng.uniform(-0.1, 0.1, (len(rows), 4)) * np.concatenate([wh[pick], wh[pick]], 1)
            dets[i, c, rows, :2] = p[pick] + jit[:, :2]
            dets[i, c, rows, 2:4] = p[pick] + wh[pick] - 1 + jit[:, 2:]
    gt = {'images': [{'id': i} for i in image_ids], 'annotations': anns,
          'categories': [{'id': c, 'name': 'c%02d' % c} for c in category_ids[1:]]}
    return gt, category_ids, image_ids, dets, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--step-ms', type=float, default=6.85)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'coco_eval_probe needs a HIP device'
    dev = 'cuda:0'
    n, B = a.images, a.batch
    gt, category_ids, image_ids, dets, count = synthetic(n)

    t0 = time.perf_counter()
    packed = evaluate.pack_coco_ground_truth(gt, category_ids, image_ids)
    pack_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = evaluate.coco_eval_arrays((dets, count), packed)
    host_stats = evaluate.coco_summarize(host[0], host[1], packed)[1]
    host_s = time.perf_counter() - t0

    ev = evaluate.DeviceCOCOEvaluator(gt, category_ids, dev, image_ids)
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
        results, stats = ev.finish()
        finish_ms.append((time.perf_counter() - t0) * 1e3)
    equal = all(np.array_equal(x, y) for x, y in zip(ev.arrays(), host)) and np.array_equal(stats, host_stats)
    q = statistics.quantiles(us, n=4)
    add_us = statistics.median(us)
    out = {'probe': 'COCO bbox AP/AR at IoU .50:.95, host coco_eval_arrays vs DeviceCOCOEvaluator',
           'device': torch.cuda.get_device_name(0), 'images': n, 'classes': T, 'rows': int(count.sum()),
           'ground_truth_boxes': int(ev.G), 'batch': B, 'adds': len(us),
           'host_pack_ground_truth_s': round(pack_s, 2), 'host_coco_eval_arrays_s': round(host_s, 2),
           'add_us_median': round(add_us, 1), 'add_us_iqr': round(q[2] - q[0], 1),
           'finish_ms_first': round(finish_ms[0], 2), 'finish_ms': round(finish_ms[1], 2),
           'device_total_ms': round(add_us * len(us) / 1e3 + finish_ms[1], 2),
           'pipeline_step_ms': a.step_ms, 'add_share_of_step': round(add_us / 1e3 / a.step_ms, 4),
           'stats_host': [float(s) for s in host_stats], 'stats_device': [float(s) for s in stats],
           'arrays_equal': bool(equal)}
    print(json.dumps(out))
    assert equal, 'device and host evaluation differ'


if __name__ == '__main__':
    main()
