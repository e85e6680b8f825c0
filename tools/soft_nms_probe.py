#!/usr/bin/env python3
"""Device time of the batched post-processing with hard NMS and with soft-NMS (linear, Gaussian), bs 32, 20 classes.

    python tools/soft_nms_probe.py [--batch 32] [--reps 10] > profiles/soft_nms_probe.json

Two inputs:
  clustered  'trained-like': RFBNet-300's prior count, the boxes of synth.clustered_dets; per (image, class) --per-class
             priors carry its tie-free scores, every other score is below conf_thresh;
  random     boxes and scores RFBNet-300 with synthetic weights produces for a random batch (thousands of candidates
             per class: the regime the top-k shortcuts of the hard path were built for).
Per input, method and max_per_image (200 and 0): ops.PostProcessor.run between HIP events, after 3 warm-up calls, median
of --reps calls (3 calls where one takes more than 50 ms), with the rows it keeps and its overflow flag.  max_per_image 0
with soft-NMS on thousands of candidates is slow by construction: one dependent trip per emitted row.
Baseline a user has without the device path: the candidates of every segment on the host, in the pipeline's order, and a
loop of ct_cpu_soft_nms over them (wall clock of the loop alone; on the random input over the first image's 20 segments,
reported per image and scaled to the batch).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ctdet import ops, synth  # noqa: E402

T, CONF, NMS_T = 20, 0.01, 0.45


def clustered_input(B, P, per_class):
    rng = np.random.RandomState(5)
    boxes = np.zeros((B, P, 4), np.float32)
    scores = np.zeros((B, P, T + 1), np.float32)
    for b in range(B):
        boxes[b] = synth.clustered_dets(P, seed=1000 + b)[:, :4]
        for c in range(T):
            where = rng.choice(P, per_class, replace=False)
            scores[b, where, 1 + c] = synth.clustered_dets(per_class, seed=7 * b + c)[:, 4]
    return boxes, scores


def random_input(B):
    from data import VOC_300
    from layers.functions import PriorBox
    from models.RFB_Net_vgg import build_net
    from ctdet.pipeline import DetectionPipeline
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), 300, T)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()), strict=True)
    net = net.eval().cuda()
    net.device = 'cuda'
    pipe = DetectionPipeline(net, PriorBox(VOC_300).forward(), B, T, image_wh=(500, 375), graph=False)
    pipe.run(synth.images(B, 300, 'randn', 2024).cuda())
    torch.cuda.synchronize()
    return pipe.boxes.cpu().numpy(), pipe.scores.cpu().numpy()


def device_times(boxes, scores, reps):
    B, P = boxes.shape[:2]
    db, ds = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    pp = ops.PostProcessor(B, P, T, 'cuda:0', out_cap=P)
    out = {}
    for mpi in (200, 0):
        for method in ('hard', 'linear', 'gaussian'):
            def once():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                pp.run(db, ds, CONF, NMS_T, False, mpi, nms_method=method)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)
            warm = [once() for _ in range(3)]
            ms = [once() for _ in range(3 if warm[-1] > 50 else reps)]
            out['%s_mpi%d' % (method, mpi)] = {'ms_median': round(statistics.median(ms), 3),
                                               'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3), 'calls': len(ms),
                                               'rows_kept': int(pp.out_count.sum().item()),
                                               'overflow': int(pp.overflow.item())}
    return out


def host_loop(boxes, scores, images):
    """ct_cpu_soft_nms over the (image, class) segments of `images` -> {method: seconds}, candidates, longest segment."""
    segs = []
    for b in images:
        for c in range(T):
            inds = np.where(scores[b, :, 1 + c] > np.float32(CONF))[0]
            inds = inds[np.argsort(-scores[b, inds, 1 + c], kind='stable')]
            segs.append(np.hstack([boxes[b, inds], scores[b, inds, 1 + c][:, None]]).astype(np.float32))
    out = {}
    for name, method in (('linear', 1), ('gaussian', 2)):
        work = [s.copy() for s in segs]
        t0 = time.perf_counter()
        for w in work:
            ops.cpu_soft_nms(w, 0.5, NMS_T, 0.001, method)
        out[name] = time.perf_counter() - t0
    return out, int(sum(len(s) for s in segs)), int(max(len(s) for s in segs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--per-class', type=int, default=300)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'soft_nms_probe needs a HIP device'
    B = a.batch
    out = {'probe': 'post-processing per batch: hard NMS vs soft-NMS (linear, Gaussian), device vs host loop',
           'device': torch.cuda.get_device_name(0), 'batch': B, 'classes': T, 'conf_thresh': CONF, 'nms_thresh': NMS_T,
           'soft_sigma': 0.5, 'soft_score_threshold': 0.001, 'lds_rows': int(ops.lib().ct_soft_nms_lds_rows())}
    rb, rs = random_input(B)
    cb, cs = clustered_input(B, rb.shape[1], a.per_class)
    for name, boxes, scores, images in (('clustered', cb, cs, range(B)), ('random', rb, rs, range(1))):
        host, cand, longest = host_loop(boxes, scores, images)
        scale = B / len(images)
        entry = {'priors': int(boxes.shape[1]), 'host_images': len(images), 'host_candidates': cand,
                 'longest_host_segment': longest,
                 'host_loop_ms_per_batch': {k: round(v * 1e3 * scale, 1) for k, v in host.items()},
                 'host_loop_scaled_from_images': len(images) if len(images) != B else None,
                 'device': device_times(boxes, scores, a.reps)}
        out[name] = entry
    print(json.dumps(out))


if __name__ == '__main__':
    main()
