#!/usr/bin/env python3
"""What a weight average (EMA) costs next to the fused SGD step, on the parameter sets of tools/sgd_probe.py.

    python tools/ema_probe.py --hbm-tbs 4.85 [--hbm-source "tools/ubench/hbm_stream.hip, 1024 MB RW copy"]

Four ways to run one optimizer step over the same parameters and gradients (one parameter group):
  fused     FusedSGD.step()                                              ct_sgd_step: the yardstick, no average
  attached  FusedSGD(ema=WeightEMA(net)).step()                          ct_ema_begin + ct_sgd_step_ema + ct_ema_update
                                                                         (the update: buffers only)
  update    FusedSGD.step(); WeightEMA.update()                          ct_sgd_step, ct_ema_begin + ct_ema_update
  foreach   FusedSGD.step(); torch._foreach_mul_ / torch._foreach_add_   what a user bolts on without the feature
Every (variant, round) is a FRESH process that measures all three sets; the variants alternate inside a round, and the
medians over --rounds rounds are reported next to every round's value (dev_ms / host_ms / loop_ms as tools/sgd_probe.py
defines them).  Launches are the library's own launch records (ct_profile_enable) and, for `foreach`, the
aten::_foreach_* calls on top (each is at least one launch).  must_move_mb is what the variant has to read and write:
4 B * numel * passes, with 5 passes for the step (p, buf read and written, g read), 2 more per parameter when the
average rides in the step, 3 for an average updated on its own (ema read and written, source read) and 5 for the two
foreach calls (mul_: 2, add_: 3); gbs = must_move / dev time, hbm_frac = gbs against --hbm-tbs.
Prints one JSON line and writes it to profiles/ema_probe.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

VARIANTS = ('fused', 'attached', 'update', 'foreach')
DECAY = 0.9998


class Then:
    """opt.step() followed by `after()`."""

    def __init__(self, opt, after):
        self.opt, self.after = opt, after

    def step(self):
        self.opt.step()
        self.after()


def child(variant, steps, warmup):
    import torch
    from clip_probe import library_launches
    from ctdet.optim import FusedSGD, WeightEMA
    from models.RFB_Net_vgg import build_net
    from sgd_probe import SETS, timed
    torch.cuda.set_device(0)
    rows = []
    for tag, size, phase in SETS:
        args = types.SimpleNamespace(method='ours', phase=phase, setting='transfer')
        net = build_net(args, size, 20).cuda()
        gen = torch.Generator(device='cuda').manual_seed(1)
        prm = [p for p in net.parameters() if p.requires_grad]
        for p in prm:
            p.grad = torch.randn(p.shape, device='cuda', generator=gen) * 1e-2
        numel = sum(p.numel() for p in prm)
        opt = FusedSGD(prm, lr=4e-3, momentum=0.9, weight_decay=5e-4)
        rest, foreach_calls = 0, 0
        if variant == 'fused':
            way, passes = opt, 5 * numel
        else:
            ema = WeightEMA(net, DECAY)
            averaged = sum(s.numel() for s in ema.shadows())
            rest = averaged - numel                     # frozen parameters and floating-point buffers
            if variant == 'attached':
                way, passes = opt.attach_ema(ema), 7 * numel + 3 * rest
            elif variant == 'update':
                way, passes = Then(opt, ema.update), 5 * numel + 3 * averaged
            else:
                shadows = ema.shadows()
                live = [t for _, t in ema.pairs()]

                def bolt_on():
                    torch._foreach_mul_(shadows, DECAY)
                    torch._foreach_add_(shadows, live, alpha=1.0 - DECAY)

                way, passes = Then(opt, bolt_on), 5 * numel + 5 * averaged
                from torch.profiler import ProfilerActivity, profile
                with torch.no_grad(), profile(activities=[ProfilerActivity.CPU]) as prof:
                    bolt_on()
                foreach_calls = sum(e.count for e in prof.key_averages() if e.key.startswith('aten::_foreach'))
        with torch.no_grad():
            dev_ms, host_ms, loop_ms = timed(way, steps, warmup)
            launches = library_launches(way)
        rows.append({'set': tag, 'tensors': len(prm), 'numel': numel, 'other_averaged_numel': rest,
                     'dev_ms': dev_ms, 'host_ms': host_ms, 'loop_ms': loop_ms, 'must_move_mb': 4 * passes / 1e6,
                     'launches': {k: v[0] for k, v in launches.items()}, 'kernel_ms': {k: round(v[1], 4) for k, v in launches.items()},
                     'aten_foreach_calls': foreach_calls,
                     'ema_info': None if variant in ('fused', 'foreach') else ema.info()})
        del net, opt, way
        torch.cuda.empty_cache()
    print(json.dumps({'variant': variant, 'device': torch.cuda.get_device_name(0), 'rows': rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--hbm-tbs', type=float, required=True, help='HBM rate of this box in TB/s (tools/ubench/hbm_stream.hip)')
    ap.add_argument('--hbm-source', default='tools/ubench/hbm_stream.hip, 1024 MB RW copy, best grid')
    ap.add_argument('--timeout', type=float, default=240.0, help='seconds one measuring process may take')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'ema_probe.json'))
    ap.add_argument('--child', choices=VARIANTS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup)
    runs = {v: [] for v in VARIANTS}
    device = None
    for _ in range(a.rounds):
        for v in VARIANTS:                              # a fresh process each: no allocator or cache state carries over
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', v, '--steps', str(a.steps), '--warmup',
                                str(a.warmup), '--hbm-tbs', str(a.hbm_tbs)], capture_output=True, text=True,
                               timeout=a.timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit('ema_probe: the %s process ended with status %d; nothing more is started' % (v, r.returncode))
            got = json.loads(r.stdout.strip().splitlines()[-1])
            device = got['device']
            runs[v].append(got['rows'])
    rows = []
    for i, first in enumerate(runs['fused'][0]):
        row = {'set': first['set'], 'tensors': first['tensors'], 'numel': first['numel'],
               'other_averaged_numel': runs['attached'][0][i]['other_averaged_numel']}
        for v in VARIANTS:
            per_round = [r[i] for r in runs[v]]
            last = per_round[-1]
            dev = statistics.median(x['dev_ms'] for x in per_round)
            gbs = last['must_move_mb'] * 1e6 / (dev * 1e-3) / 1e9
            row[v] = {'dev_ms': round(dev, 4), 'host_ms': round(statistics.median(x['host_ms'] for x in per_round), 4),
                      'loop_ms': round(statistics.median(x['loop_ms'] for x in per_round), 4),
                      'all_rounds_dev_ms': [round(x['dev_ms'], 4) for x in per_round],
                      'launches': last['launches'], 'library_launches': sum(last['launches'].values()),
                      'aten_foreach_calls': last['aten_foreach_calls'], 'kernel_ms': last['kernel_ms'],
                      'must_move_mb': round(last['must_move_mb'], 1), 'gbs': round(gbs, 1),
                      'hbm_frac': round(gbs * 1e9 / (a.hbm_tbs * 1e12), 3), 'ema_info': last['ema_info']}
        base = row['fused']['dev_ms']
        for v in VARIANTS[1:]:
            row[v]['dev_ms_over_fused'] = round(row[v]['dev_ms'] / base, 3)
            row[v]['extra_dev_ms'] = round(row[v]['dev_ms'] - base, 4)
        rows.append(row)
    line = json.dumps({'probe': 'ema', 'decay': DECAY, 'steps': a.steps, 'warmup': a.warmup, 'rounds': a.rounds,
                       'hbm_tbs': a.hbm_tbs, 'hbm_source': a.hbm_source, 'device': device, 'rows': rows})
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
