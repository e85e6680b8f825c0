#!/usr/bin/env python3
"""MultiBoxLoss forward + gradients w.r.t. the three predictions: the torch path against the fused HIP kernels.

    python tools/loss_probe.py [--reps 30] [--warmup 5] [--loc-loss NAME ...] [--conf-loss ce focal]

Both forms run on the same prematched batch in the same process, alternating, with HIP events around
loss forward + torch.autograd.grad; medians over --reps after --warmup, at (300^2, bs 32), (300^2, bs 4) and
(512^2, bs 8, C = 61).  Prints one JSON line; `spread_us` is the inter-quartile range of each form's samples.
--loc-loss: the IoU-family localisation terms to time next to the two smooth-L1 forms (default: all four); each adds a
`loc` row per shape with the fused and the torch form's medians and spreads (`--loc-loss none`: the smooth-L1 rows alone).
--conf-loss: the classification terms to time (default: ce alone, the rows above); with `focal` each shape gains a `conf` row with
the mining-free focal form (gamma 2, alpha 0.25) next to the cross-entropy one: fused and torch medians and spreads of the whole
step, and for both fused forms the forward and the backward part (a third event between the loss and torch.autograd.grad)."""
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
LOC_KINDS = ('iou', 'giou', 'diou', 'ciou')


def probe(size, batch, ncls, reps, warmup, kinds=(), focal=False):
    dev = 'cuda'
    priors = PriorBox(cfgs.VOC_300 if size == 300 else cfgs.VOC_512).forward().to(dev)
    P = priors.shape[0]
    g = torch.Generator().manual_seed(5)
    preds = [t.to(dev).requires_grad_(True) for t in (torch.randn(batch, P, 4, generator=g),
                                                      torch.randn(batch, P, ncls - 1, generator=g) * 3,
                                                      torch.randn(batch, P, 2, generator=g))]
    crits = {name: MultiBoxLoss_combined(ncls, 0.5, True, 0, True, 3, 0.5, False, fused=f)
             for name, f in (('torch', False), ('fused', True))}
    for kind in kinds:
        for name, f in (('torch', False), ('fused', True)):
            crits['%s_%s' % (name, kind)] = MultiBoxLoss_combined(ncls, 0.5, True, 0, True, 3, 0.5, False, fused=f,
                                                                  loc_loss=kind)
    if focal:
        for name, f in (('torch', False), ('fused', True)):
            crits[name + '_focal'] = MultiBoxLoss_combined(ncls, 0.5, True, 0, True, 3, 0.5, False, fused=f, conf_loss='focal',
                                                           focal_gamma=2.0, focal_alpha=0.25)
    matched = crits['torch'].match(priors, [t.to(dev) for t in synth.targets(batch, ncls, 99)])

    def step(crit):
        out = crit(preds, priors, matched)
        return out, torch.autograd.grad(sum(out.values()), preds)

    values = {}
    for name, crit in crits.items():
        out, _ = step(crit)
        values[name] = {k: float(v.detach()) for k, v in out.items()}
    samples = {name: [] for name in crits}
    parts = {name: ([], []) for name in crits}      # forward, backward
    for it in range(warmup + reps):
        for name, crit in crits.items():            # alternating: both forms see the same clocks and cache state
            a, m, b = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            a.record()
            out = crit(preds, priors, matched)
            m.record()
            torch.autograd.grad(sum(out.values()), preds)
            b.record()
            b.synchronize()
            if it >= warmup:
                samples[name].append(a.elapsed_time(b) * 1e3)
                parts[name][0].append(a.elapsed_time(m) * 1e3)
                parts[name][1].append(m.elapsed_time(b) * 1e3)
    res = {'num_priors': P, 'batch': batch, 'num_classes': ncls, 'positives': int((matched.conf_t[:, :, 0] > 0).sum()),
           'loss': {k: values[k] for k in ('torch', 'fused')}}
    stat = {}
    for name, s in samples.items():
        q = statistics.quantiles(s, n=4)
        stat[name] = (round(statistics.median(s), 1), round(q[2] - q[0], 1))
    for name in ('torch', 'fused'):
        res[name + '_us'], res[name + '_spread_us'] = stat[name]
    res['speedup'] = round(res['torch_us'] / res['fused_us'], 2)
    if kinds:       # one row per kind, next to the smooth-L1 figures above
        res['loc'] = {kind: {'fused_us': stat['fused_' + kind][0], 'fused_spread_us': stat['fused_' + kind][1],
                             'torch_us': stat['torch_' + kind][0], 'torch_spread_us': stat['torch_' + kind][1],
                             'fused_minus_smooth_l1_us': round(stat['fused_' + kind][0] - stat['fused'][0], 1),
                             'loss_box_reg': {f: values['%s_%s' % (f, kind)]['loss_box_reg'] for f in ('torch', 'fused')}}
                      for kind in kinds}
    if focal:       # the focal form next to the cross-entropy one, forward and backward apart for the fused forms
        med = lambda v: round(statistics.median(v), 1)
        res['conf'] = {'focal': {'fused_us': stat['fused_focal'][0], 'fused_spread_us': stat['fused_focal'][1],
                                 'torch_us': stat['torch_focal'][0], 'torch_spread_us': stat['torch_focal'][1],
                                 'fused_minus_ce_us': round(stat['fused_focal'][0] - stat['fused'][0], 1),
                                 'fused_fwd_us': med(parts['fused_focal'][0]), 'fused_bwd_us': med(parts['fused_focal'][1]),
                                 'loss': {f: values[f + '_focal'] for f in ('torch', 'fused')}},
                       'ce': {'fused_fwd_us': med(parts['fused'][0]), 'fused_bwd_us': med(parts['fused'][1])}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--loc-loss', nargs='+', default=list(LOC_KINDS), choices=LOC_KINDS + ('none',))
    ap.add_argument('--conf-loss', nargs='+', default=['ce'], choices=('ce', 'focal'))
    a = ap.parse_args()
    kinds = tuple(k for k in LOC_KINDS if k in a.loc_loss)
    assert a.reps >= 20, 'medians of at least 20 samples'
    assert torch.cuda.is_available(), 'loss_probe needs a HIP device'
    out = {'probe': 'multibox_loss fwd + grad, HIP events, median us', 'device': torch.cuda.get_device_name(0),
           'reps': a.reps, 'loc_loss': list(kinds), 'conf_loss': a.conf_loss,
           'shapes': {name: probe(size, b, c, a.reps, a.warmup, kinds, 'focal' in a.conf_loss) for name, size, b, c in SHAPES}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
