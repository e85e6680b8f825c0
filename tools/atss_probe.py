#!/usr/bin/env python3
"""The two target matchers of MultiBoxLoss side by side: ct_match_batched (IoU >= 0.5 plus one forced prior per box) and
ct_atss_match_batched (adaptive training sample selection, include/ctdet.h).

    python tools/atss_probe.py [--reps 30] [--warmup 5] [--calls 10] [--topk 9]

Both C entries are called on preallocated buffers in the same process, alternating; a sample is the HIP-event time around
--calls back-to-back calls divided by --calls, so that the launch gaps of one call do not set the figure.  Medians over --reps
after --warmup, `spread_us` the inter-quartile range.  Shapes: VOC_300 bs 32 and VOC_512 bs 8 with synth.targets (1-8 boxes per
image), and a crowded VOC_300 bs 32 with 64 boxes per image.  Also per shape: the positives per box each matcher ends with
(counted by giving every box of an image its own label), the two ATSS kernels apart (the library's launch records, events
around each launch), and for ATSS the candidates, the forced boxes and the boxes left
with no prior after conflicts.  Prints one JSON line."""
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


def crowded(batch, boxes, seed=7):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(batch):
        xy = rng.uniform(0, 0.7, (boxes, 2))
        wh = rng.uniform(0.05, 0.3, (boxes, 2))
        t = np.concatenate([xy, xy + wh, np.ones((boxes, 1)), np.ones((boxes, 1))], 1)
        out.append(torch.from_numpy(t.astype(np.float32)))
    return out


def per_box(conf_t, counts):
    """Positives per box from labels that number the boxes of each image 1..G."""
    lab = conf_t[..., 0].long().cpu()
    rows = [torch.bincount(lab[b], minlength=g + 1)[1:g + 1] for b, g in enumerate(counts)]
    n = torch.cat(rows).double()
    return {'min': int(n.min()), 'median': float(n.median()), 'mean': round(float(n.mean()), 2), 'max': int(n.max()),
            'boxes_without_prior': int((n == 0).sum())}


def probe(size, targets, topk, reps, warmup, calls):
    dev = 'cuda'
    pb = PriorBox(cfgs.VOC_300 if size == 300 else cfgs.VOC_512)
    priors, off = pb.forward().to(dev), pb.level_offsets()
    B, P = len(targets), priors.shape[0]
    counts = [int(t.shape[0]) for t in targets]
    numbered = []
    for t in targets:                                   # every box its own label: the matchers do not read it
        t = t.clone()
        t[:, 4] = torch.arange(1, t.shape[0] + 1)
        numbered.append(t.to(dev))
    var = (0.1, 0.2)
    ssd = ops.match_batched(numbered, priors, 0.5, var)
    atss = ops.atss_match_batched(numbered, priors, off, topk, var, want_stats=True)
    stats = atss[3].cpu()
    live = stats[..., 1] > 0

    max_gt = max(counts)
    truths = torch.cat(numbered, 0).contiguous()
    gt_off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)
    loc_t, conf_t = torch.empty(B, P, 4, device=dev), torch.empty(B, P, 2, device=dev)
    obj_t = torch.empty(B, P, device=dev, dtype=torch.uint8)
    L = lib()
    ws_s, ws_a = L.ct_match_workspace_bytes(B, P, max_gt), L.ct_atss_workspace_bytes(B, P, max_gt)
    ws = torch.empty(max(ws_s, ws_a), device=dev, dtype=torch.uint8)
    levels = (C.c_int * len(off))(*off)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run_ssd():
        check(L.ct_match_batched(ptr(truths), ptr(gt_off), B, max_gt, ptr(priors), P, 0.5, var[0], var[1], ptr(loc_t), ptr(conf_t),
                                 ptr(obj_t), None, ptr(ws), ws_s, st), 'ct_match_batched')

    def run_atss():
        check(L.ct_atss_match_batched(ptr(truths), ptr(gt_off), B, max_gt, ptr(priors), P, levels, len(off) - 1, topk, var[0],
                                      var[1], ptr(loc_t), ptr(conf_t), ptr(obj_t), None, None, ptr(ws), ws_a, st),
              'ct_atss_match_batched')

    forms = {'ssd': run_ssd, 'atss': run_atss}
    samples = {k: [] for k in forms}
    for it in range(warmup + reps):
        for name, fn in forms.items():                  # alternating: both see the same clocks and cache state
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                samples[name].append(a.elapsed_time(b) * 1e3 / calls)
    res = {'size': size, 'num_priors': P, 'batch': B, 'boxes': sum(counts), 'max_gt': max_gt, 'select_workgroups': B * max_gt}
    for name, s in samples.items():
        q = statistics.quantiles(s, n=4)
        res[name + '_us'], res[name + '_spread_us'] = round(statistics.median(s), 1), round(q[2] - q[0], 1)
    res['atss_over_ssd'] = round(res['atss_us'] / res['ssd_us'], 2)
    # the two ATSS kernels apart: the library's own launch records (ct_profile_enable), medians over `reps` calls
    torch.cuda.synchronize()
    L.ct_profile_enable(1)
    for _ in range(reps):
        run_atss()
    n = C.c_int(0)
    recs = (ProfileRecord * 4096)()
    check(L.ct_profile_collect(recs, 4096, C.byref(n)), 'ct_profile_collect')
    L.ct_profile_enable(0)
    for kernel in ('atss_select', 'atss_assign'):
        ms = [recs[i].ms for i in range(min(n.value, 4096)) if recs[i].name == kernel.encode()]
        res[kernel + '_us'] = round(statistics.median(ms) * 1e3, 1)
    res['positives_per_box'] = {'ssd': per_box(ssd[1], counts), 'atss': per_box(atss[1], counts)}
    res['atss_candidates'] = int(stats[..., 1][live].max())
    res['atss_positives_before_conflicts'] = {'min': int(stats[..., 2][live].min()), 'max': int(stats[..., 2][live].max())}
    res['atss_forced_boxes'] = int(stats[..., 3].sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--topk', type=int, default=9)
    a = ap.parse_args()
    assert a.reps >= 20, 'medians of at least 20 samples'
    assert torch.cuda.is_available(), 'atss_probe needs a HIP device'
    shapes = (('rfb300_bs32', 300, synth.targets(32, 21, 99)), ('rfb512_bs8', 512, synth.targets(8, 61, 22)),
              ('rfb300_bs32_crowded64', 300, crowded(32, 64)))
    out = {'probe': 'ct_match_batched vs ct_atss_match_batched, HIP events over back-to-back calls, median us per call',
           'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'calls': a.calls, 'topk': a.topk,
           'shapes': {name: probe(size, tg, a.topk, a.reps, a.warmup, a.calls) for name, size, tg in shapes}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
