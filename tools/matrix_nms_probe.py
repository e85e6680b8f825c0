#!/usr/bin/env python3
"""Device time of the batched post-processing with hard NMS, soft-NMS (linear, Gaussian) and Matrix NMS (linear, Gaussian),
bs 32, 20 classes.

    python tools/matrix_nms_probe.py [--batch 32] [--reps 10] [--out profiles/matrix_nms_probe.json]

The two inputs of tools/soft_nms_probe.py:
  clustered  'trained-like': RFBNet-300's prior count, the boxes of synth.clustered_dets; per (image, class) --per-class
             priors carry its tie-free scores, every other score is below conf_thresh;
  random     boxes and scores RFBNet-300 with synthetic weights produces for a random batch (thousands of candidates per
             class).
One process makes both inputs and writes them to a scratch directory; this process never opens the device.  Every method
is then measured in a fresh process of its own, the five methods one after the other, and the whole round a second time
(alternating: a drift of the machine shows as a difference between the two rounds of a method, not between methods).  Per
input, method and max_per_image (200 and 0): ops.PostProcessor.run between HIP events after 3 warm-up calls, --reps windows
of 20 back-to-back calls each (one call where a call takes more than 5 ms), per-call median / min / max over the windows,
with the rows it keeps and its overflow flag.  Matrix NMS runs with matrix_pre_top = ct_matrix_nms_max_rows().
Baseline a user has without the device path: the candidates of every segment on the host, in the pipeline's order, and a
loop of ct_cpu_matrix_nms over them (wall clock of the loop alone; on the random input over the first image's 20 segments,
scaled to the batch).  Writes one JSON line."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))

import numpy as np  # noqa: E402

T, CONF, NMS_T, SIGMA, THR = 20, 0.01, 0.45, 0.5, 0.001
METHODS = ('hard', 'linear', 'gaussian', 'matrix_linear', 'matrix_gaussian')
INPUTS = ('clustered', 'random')


def prepare(a):
    """Both inputs -> <dir>/<input>_boxes.npy, <dir>/<input>_scores.npy."""
    import torch
    import soft_nms_probe
    assert torch.cuda.is_available(), 'matrix_nms_probe needs a HIP device'
    rb, rs = soft_nms_probe.random_input(a.batch)
    cb, cs = soft_nms_probe.clustered_input(a.batch, rb.shape[1], a.per_class)
    for name, boxes, scores in (('clustered', cb, cs), ('random', rb, rs)):
        np.save(os.path.join(a.dir, name + '_boxes.npy'), boxes)
        np.save(os.path.join(a.dir, name + '_scores.npy'), scores)
    print(json.dumps({'device': torch.cuda.get_device_name(0)}))


def load(a, name):
    return np.load(os.path.join(a.dir, name + '_boxes.npy')), np.load(os.path.join(a.dir, name + '_scores.npy'))


def measure(a):
    """One method on both inputs in this (fresh) process -> one JSON line."""
    import torch
    from ctdet import ops
    assert torch.cuda.is_available(), 'matrix_nms_probe needs a HIP device'
    pre_top = int(ops.lib().ct_matrix_nms_max_rows())
    out = {}
    for name in INPUTS:
        boxes, scores = load(a, name)
        B, P = boxes.shape[:2]
        db, ds = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
        pp = ops.PostProcessor(B, P, T, 'cuda:0', out_cap=P)
        for mpi in (200, 0):
            def window(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    pp.run(db, ds, CONF, NMS_T, False, mpi, nms_method=a.method, soft_sigma=SIGMA, soft_score_threshold=THR,
                           matrix_pre_top=pre_top)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / calls
            warm = [window(1) for _ in range(3)]
            calls = 1 if warm[-1] > 5 else 20
            ms = [window(calls) for _ in range(3 if warm[-1] > 50 else a.reps)]
            out['%s_mpi%d' % (name, mpi)] = {'ms_median': round(statistics.median(ms), 4), 'ms_min': round(min(ms), 4),
                                             'ms_max': round(max(ms), 4), 'windows': len(ms), 'calls_per_window': calls,
                                             'rows_kept': int(pp.out_count.sum().item()),
                                             'overflow': int(pp.overflow.item())}
    print(json.dumps(out))


def host_loop(boxes, scores, images, pre_top):
    """ct_cpu_matrix_nms over the (image, class) segments of `images` -> {method: seconds}, candidates, longest segment."""
    from ctdet import ops
    segs = []
    for b in images:
        for c in range(T):
            inds = np.where(scores[b, :, 1 + c] > np.float32(CONF))[0]
            inds = inds[np.argsort(-scores[b, inds, 1 + c], kind='stable')]
            segs.append(np.hstack([boxes[b, inds], scores[b, inds, 1 + c][:, None]]).astype(np.float32))
    out = {}
    for name, method in (('matrix_linear', 1), ('matrix_gaussian', 2)):
        t0 = time.perf_counter()
        for s in segs:
            ops.cpu_matrix_nms(s, method, SIGMA, THR, pre_top, 0)
        out[name] = time.perf_counter() - t0
    return out, int(sum(len(s) for s in segs)), int(max(len(s) for s in segs))


def child(a, *args):
    cmd = [sys.executable, os.path.abspath(__file__), '--dir', a.dir, '--batch', str(a.batch), '--reps', str(a.reps),
           '--per-class', str(a.per_class)] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError('%s failed (%d):\n%s' % (' '.join(args), r.returncode, r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--per-class', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'matrix_nms_probe.json'))
    ap.add_argument('--dir', help=argparse.SUPPRESS)
    ap.add_argument('--prepare', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--method', choices=METHODS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.prepare:
        return prepare(a)
    if a.method:
        return measure(a)
    a.dir = tempfile.mkdtemp(prefix='matrix_nms_probe_')
    try:
        dev = child(a, '--prepare')
        rounds = [{m: child(a, '--method', m) for m in METHODS} for _ in range(a.rounds)]
        from ctdet import _lib
        pre_top = int(_lib.lib().ct_matrix_nms_max_rows())
        out = {'probe': 'post-processing per batch: hard NMS, soft-NMS and Matrix NMS (linear, Gaussian), device vs host loop',
               'device': dev['device'], 'batch': a.batch, 'classes': T, 'conf_thresh': CONF, 'nms_thresh': NMS_T,
               'soft_sigma': SIGMA, 'soft_score_threshold': THR, 'matrix_pre_top': pre_top,
               'processes': 'one fresh process per method and round, methods in turn, %d rounds' % a.rounds}
        for name in INPUTS:
            boxes, scores = load(a, name)
            images = range(a.batch) if name == 'clustered' else range(1)
            host, cand, longest = host_loop(boxes, scores, images, pre_top)
            scale = a.batch / len(images)
            out[name] = {'priors': int(boxes.shape[1]), 'host_images': len(images), 'host_candidates': cand,
                         'longest_host_segment': longest,
                         'host_loop_ms_per_batch': {k: round(v * 1e3 * scale, 1) for k, v in host.items()},
                         'host_loop_scaled_from_images': len(images) if len(images) != a.batch else None,
                         'device': {'%s_mpi%d' % (m, mpi): [r[m]['%s_mpi%d' % (name, mpi)] for r in rounds]
                                    for mpi in (200, 0) for m in METHODS}}
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    line = json.dumps(out)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
