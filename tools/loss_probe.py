#!/usr/bin/env python3
"""MultiBoxLoss forward + gradients w.r.t. the three predictions: the torch path against the fused HIP kernels.

    python tools/loss_probe.py [--reps 30] [--warmup 5]

Both forms run on the same prematched batch in the same process, alternating, with HIP events around
loss forward + torch.autograd.grad; medians over --reps after --warmup, at (300^2, bs 32), (300^2, bs 4) and
(512^2, bs 8, C = 61).  Prints one JSON line; `spread_us` is the inter-quartile range of each form's samples."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from ctdet import synth  # noqa: E402
from layers.functions import PriorBox  # noqa: E402
from layers.modules.multibox_loss_combined import MultiBoxLoss_combined  # noqa: E402
import data as cfgs  # noqa: E402

SHAPES = (('rfb300_bs32', 300, 32, 21), ('rfb300_bs4', 300, 4, 21), ('rfb512_bs8_c61', 512, 8, 61))


def probe(size, batch, ncls, reps, warmup):
    dev = 'cuda'
    priors = PriorBox(cfgs.VOC_300 if size == 300 else cfgs.VOC_512).forward().to(dev)
    P = priors.shape[0]
    g = torch.Generator().manual_seed(5)
    preds = [t.to(dev).requires_grad_(True) for t in (torch.randn(batch, P, 4, generator=g),
                                                      torch.randn(batch, P, ncls - 1, generator=g) * 3,
                                                      torch.randn(batch, P, 2, generator=g))]
    crits = {name: MultiBoxLoss_combined(ncls, 0.5, True, 0, True, 3, 0.5, False, fused=f)
             for name, f in (('torch', False), ('fused', True))}
    matched = crits['torch'].match(priors, [t.to(dev) for t in synth.targets(batch, ncls, 99)])

    def step(crit):
        out = crit(preds, priors, matched)
        return out, torch.autograd.grad(sum(out.values()), preds)

    values = {}
    for name, crit in crits.items():
        out, _ = step(crit)
        values[name] = {k: float(v.detach()) for k, v in out.items()}
    samples = {name: [] for name in crits}
    for it in range(warmup + reps):
        for name, crit in crits.items():            # alternating: both forms see the same clocks and cache state
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(crit)
            b.record()
            b.synchronize()
            if it >= warmup:
                samples[name].append(a.elapsed_time(b) * 1e3)
    res = {'num_priors': P, 'batch': batch, 'num_classes': ncls, 'loss': values}
    for name, s in samples.items():
        q = statistics.quantiles(s, n=4)
        res[name + '_us'] = round(statistics.median(s), 1)
        res[name + '_spread_us'] = round(q[2] - q[0], 1)
    res['speedup'] = round(res['torch_us'] / res['fused_us'], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    assert a.reps >= 20, 'medians of at least 20 samples'
    assert torch.cuda.is_available(), 'loss_probe needs a HIP device'
    out = {'probe': 'multibox_loss fwd + grad, HIP events, median us', 'device': torch.cuda.get_device_name(0),
           'reps': a.reps, 'shapes': {name: probe(size, b, c, a.reps, a.warmup) for name, size, b, c in SHAPES}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
