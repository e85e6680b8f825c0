#!/usr/bin/env python3
"""The three target matchers of MultiBoxLoss side by side: ct_match_batched (IoU >= 0.5 plus one forced prior per box),
ct_atss_match_batched (adaptive training sample selection) and ct_detect_fused + ct_tal_match_batched (task-aligned assignment
from predictions, include/ctdet.h).

    python tools/tal_probe.py [--reps 30] [--warmup 5] [--calls 10] [--topk 13] [--alpha 1.0] [--beta 6] [--out profiles/tal_probe.json]

All C entries are called on preallocated buffers in the same process, alternating; a sample is the HIP-event time around
--calls back-to-back calls divided by --calls, so that the launch gaps of one call do not set the figure.  Medians over --reps
after --warmup, `spread_us` the inter-quartile range.  `tal` is the matching call alone, `tal_with_detect` what a training step
pays: the ct_detect_fused pass over the raw predictions and the matching call.  Shapes as tools/atss_probe.py: VOC_300 bs 32 and
VOC_512 bs 8 with synth.targets (1-8 boxes per image), and a crowded VOC_300 bs 32 with 64 boxes per image; the predictions are
seeded noise around the priors (loc ~ N(0, 1), conf ~ 3 N(0, 1), obj ~ N(0, 1)).  Also per shape: the kernels apart (the
library's launch records, events around each launch), the positives per box each matcher ends with (counted by giving every
box of an image its own label; TAL then ranks by 1 - background for the labels above the class count, the same work), and for
TAL the eligible candidates per box and the forced boxes.  Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ctdet import ops, synth  # noqa: E402
from ctdet._lib import ProfileRecord, check, lib  # noqa: E402
from layers.functions import PriorBox  # noqa: E402
import data as cfgs  # noqa: E402

sys.path.insert(0, os.path.join(REPO, 'tools'))
from atss_probe import crowded, per_box  # noqa: E402

KERNELS = ('atss_select', 'atss_assign', 'tal_select', 'tal_assign')


def probe(size, ncls, targets, a):
    dev = 'cuda'
    pb = PriorBox(cfgs.VOC_300 if size == 300 else cfgs.VOC_512)
    priors, off = pb.forward().to(dev), pb.level_offsets()
    B, P = len(targets), priors.shape[0]
    counts = [int(t.shape[0]) for t in targets]
    numbered = []
    for t in targets:                                   # every box its own label: the positives per box can be counted
        t = t.clone()
        t[:, 4] = torch.arange(1, t.shape[0] + 1)
        numbered.append(t.to(dev))
    var = (0.1, 0.2)
    g = torch.Generator().manual_seed(5)
    loc, conf, obj = (torch.randn(B, P, 4, generator=g).to(dev), (torch.randn(B, P, ncls - 1, generator=g) * 3).to(dev),
                      torch.randn(B, P, 2, generator=g).to(dev))
    boxes, scores = ops.detect_fused(loc, conf, obj, priors, var, apply_softmax=True)
    ssd = ops.match_batched(numbered, priors, 0.5, var)
    atss = ops.atss_match_batched(numbered, priors, off, 9, var)
    tal = ops.tal_match_batched(numbered, priors, boxes, scores, a.topk, a.alpha, a.beta, var, want_stats=True)
    stats = tal[3].cpu()
    live = stats[..., 1] > 0

    max_gt = max(counts)
    truths = torch.cat(numbered, 0).contiguous()
    gt_off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)
    loc_t, conf_t = torch.empty(B, P, 4, device=dev), torch.empty(B, P, 2, device=dev)
    obj_t = torch.empty(B, P, device=dev, dtype=torch.uint8)
    L = lib()
    sizes = (L.ct_match_workspace_bytes(B, P, max_gt), L.ct_atss_workspace_bytes(B, P, max_gt), L.ct_tal_workspace_bytes(B, P, max_gt))
    ws = torch.empty(max(sizes), device=dev, dtype=torch.uint8)
    levels = (C.c_int * len(off))(*off)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    topk, alpha2, beta = ops.check_tal(a.topk, a.alpha, a.beta)

    def run_ssd():
        check(L.ct_match_batched(ptr(truths), ptr(gt_off), B, max_gt, ptr(priors), P, 0.5, var[0], var[1], ptr(loc_t), ptr(conf_t),
                                 ptr(obj_t), None, ptr(ws), sizes[0], st), 'ct_match_batched')

    def run_atss():
        check(L.ct_atss_match_batched(ptr(truths), ptr(gt_off), B, max_gt, ptr(priors), P, levels, len(off) - 1, 9, var[0],
                                      var[1], ptr(loc_t), ptr(conf_t), ptr(obj_t), None, None, ptr(ws), sizes[1], st),
              'ct_atss_match_batched')

    def run_detect():
        check(L.ct_detect_fused(ptr(loc), ptr(conf), ptr(obj), ptr(priors), B, P, ncls - 1, var[0], var[1], 1, None, 0,
                                ptr(boxes), ptr(scores), st), 'ct_detect_fused')

    def run_tal():
        check(L.ct_tal_match_batched(ptr(truths), ptr(gt_off), B, max_gt, ptr(priors), P, ptr(boxes), ptr(scores), ncls, topk,
                                     alpha2, beta, var[0], var[1], ptr(loc_t), ptr(conf_t), ptr(obj_t), None, None, ptr(ws),
                                     sizes[2], st), 'ct_tal_match_batched')

    def run_tal_with_detect():
        run_detect()
        run_tal()

    forms = {'ssd': run_ssd, 'atss': run_atss, 'detect': run_detect, 'tal': run_tal, 'tal_with_detect': run_tal_with_detect}
    samples = {k: [] for k in forms}
    for it in range(a.warmup + a.reps):
        for name, fn in forms.items():                  # alternating: all see the same clocks and cache state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                samples[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    res = {'size': size, 'num_priors': P, 'batch': B, 'boxes': sum(counts), 'max_gt': max_gt, 'select_workgroups': B * max_gt,
           'score_cols': ncls, 'pred_bytes_read_by_detect': int(loc.numel() + conf.numel() + obj.numel()) * 4}
    for name, s in samples.items():
        q = statistics.quantiles(s, n=4)
        res[name + '_us'], res[name + '_spread_us'] = round(statistics.median(s), 1), round(q[2] - q[0], 1)
    res['tal_over_atss'] = round(res['tal_us'] / res['atss_us'], 2)
    res['tal_with_detect_over_ssd'] = round(res['tal_with_detect_us'] / res['ssd_us'], 2)
    # the kernels apart: the library's own launch records (ct_profile_enable), medians over `reps` calls
    torch.cuda.synchronize()
    L.ct_profile_enable(1)
    for _ in range(a.reps):
        run_atss()
        run_tal()
    n = C.c_int(0)
    recs = (ProfileRecord * 8192)()
    check(L.ct_profile_collect(recs, 8192, C.byref(n)), 'ct_profile_collect')
    L.ct_profile_enable(0)
    for kernel in KERNELS:
        ms = [recs[i].ms for i in range(min(n.value, 8192)) if recs[i].name == kernel.encode()]
        res[kernel + '_us'] = round(statistics.median(ms) * 1e3, 1)
    res['tal_select_over_atss_select'] = round(res['tal_select_us'] / res['atss_select_us'], 2)
    res['positives_per_box'] = {'ssd': per_box(ssd[1], counts), 'atss': per_box(atss[1], counts), 'tal': per_box(tal[1], counts)}
    elig = stats[..., 0][live]
    res['tal_eligible_per_box'] = {'min': int(elig.min()), 'median': float(elig.median()), 'max': int(elig.max())}
    res['tal_positives_before_conflicts'] = {'min': int(stats[..., 1][live].min()), 'max': int(stats[..., 1][live].max())}
    res['tal_forced_boxes'] = int(stats[..., 3].sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--topk', type=int, default=13)
    ap.add_argument('--alpha', type=float, default=1.0)
    ap.add_argument('--beta', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'tal_probe.json'))
    a = ap.parse_args()
    assert a.reps >= 20, 'medians of at least 20 samples'
    assert torch.cuda.is_available(), 'tal_probe needs a HIP device'
    shapes = (('rfb300_bs32', 300, 21, synth.targets(32, 21, 99)), ('rfb512_bs8', 512, 61, synth.targets(8, 61, 22)),
              ('rfb300_bs32_crowded64', 300, 21, crowded(32, 64)))
    out = {'probe': 'ct_match_batched vs ct_atss_match_batched vs ct_detect_fused + ct_tal_match_batched, HIP events over '
                    'back-to-back calls, median us per call',
           'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'calls': a.calls, 'atss_topk': 9, 'tal_topk': a.topk,
           'tal_alpha': a.alpha, 'tal_beta': a.beta, 'tal_lds_keys': lib().ct_tal_lds_keys(),
           'shapes': {name: probe(size, ncls, tg, a) for name, size, ncls, tg in shapes}}
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
