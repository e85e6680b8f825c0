#!/usr/bin/env python3
"""What an AdamW step costs on the project's parameter sets: torch's own implementations against ctdet.optim.FusedAdamW.

    python tools/adamw_probe.py --hbm-tbs 4.85 [--hbm-source "tools/ubench/hbm_stream.hip, 1024 MB RW copy"]

Four ways to run one optimizer step over the same parameters and gradients (one parameter group, lr 1e-3, betas
0.9 / 0.999, eps 1e-8, weight decay 5e-4), on RFBNet-300 phase 1 and RFBNet-512 phase 2:
  foreach      torch.optim.AdamW(foreach=True)                      torch's multi-tensor path
  torch_fused  torch.optim.AdamW(fused=True)                        torch's fused kernel, if this torch runs it
  fused        FusedAdamW.step()                                    ct_adamw_begin + ct_adamw_step
  fused_full   FusedAdamW(max_grad_norm=1e30, ema=WeightEMA(net))   + ct_grad_norm_clip, ct_ema_begin, the average inside
                                                                    the step, ct_ema_update for the buffers
Every (variant, round) is a FRESH process that measures both sets; the variants alternate inside a round, and the
medians over --rounds rounds are reported next to every round's value (dev_ms / host_ms / loop_ms as tools/sgd_probe.py
defines them: device time from HIP events over back-to-back steps queued behind a blocker).  Launches are the library's
own launch records (ct_profile_enable) and, for torch, the aten::_foreach_* / aten::_fused_* calls of one step (each is
at least one launch).  must_move_mb is what the variant has to read and write: 28 B per element for the step (p, m, v
read and written, g read), 36 B with the average inside it, 4 B more for the norm's read of the gradients and 12 B per
element of what ct_ema_update averages; gbs = must_move / dev time, hbm_frac = gbs against --hbm-tbs.
Prints one JSON line and writes it to profiles/adamw_probe.json.
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

VARIANTS = ('foreach', 'torch_fused', 'fused', 'fused_full')
SETS = [('rfb300_phase1', 300, 1), ('rfb512_phase2', 512, 2)]
KW = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
MAX_NORM = 1e30                                 # the norm and the guard run, the coefficient stays 1
DECAY = 0.9998


def torch_calls(opt):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        opt.step()
    return sum(e.count for e in prof.key_averages() if e.key.startswith(('aten::_foreach', 'aten::_fused')))


def child(variant, steps, warmup):
    import torch
    from clip_probe import library_launches
    from ctdet.optim import FusedAdamW, WeightEMA
    from models.RFB_Net_vgg import build_net
    from sgd_probe import timed
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
        row = {'set': tag, 'tensors': len(prm), 'numel': numel, 'ran': True, 'other_averaged_numel': 0}
        launches, calls, ema = {}, 0, None
        try:
            if variant == 'foreach':
                opt, moved = torch.optim.AdamW(prm, foreach=True, **KW), 28 * numel
            elif variant == 'torch_fused':
                opt, moved = torch.optim.AdamW(prm, fused=True, **KW), 28 * numel
            elif variant == 'fused':
                opt, moved = FusedAdamW(prm, **KW), 28 * numel
            else:
                ema = WeightEMA(net, DECAY)
                rest = sum(s.numel() for s in ema.shadows()) - numel    # frozen parameters and floating-point buffers
                opt, moved = FusedAdamW(prm, max_grad_norm=MAX_NORM, ema=ema, **KW), (36 + 4) * numel + 12 * rest
                row['other_averaged_numel'] = rest
            with torch.no_grad():
                dev_ms, host_ms, loop_ms = timed(opt, steps, warmup)
                if variant in ('fused', 'fused_full'):
                    launches = library_launches(opt)
                else:
                    calls = torch_calls(opt)
        except (RuntimeError, ValueError) as e:
            if variant != 'torch_fused':
                raise
            rows.append(dict(row, ran=False, why=str(e)[:200]))         # this torch does not run its fused AdamW here
            continue
        row.update(dev_ms=dev_ms, host_ms=host_ms, loop_ms=loop_ms, must_move_mb=moved / 1e6,
                   launches={k: v[0] for k, v in launches.items()},
                   kernel_ms={k: round(v[1], 4) for k, v in launches.items()}, aten_calls=calls,
                   clip_info=opt.clip_info() if variant == 'fused_full' else None,
                   ema_info=ema.info() if ema is not None else None)
        rows.append(row)
        del net, opt
        torch.cuda.empty_cache()
    print(json.dumps({'variant': variant, 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--hbm-tbs', type=float, required=True, help='HBM rate of this box in TB/s (tools/ubench/hbm_stream.hip)')
    ap.add_argument('--hbm-source', default='tools/ubench/hbm_stream.hip, 1024 MB RW copy, best grid')
    ap.add_argument('--timeout', type=float, default=240.0, help='seconds one measuring process may take')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'adamw_probe.json'))
    ap.add_argument('--child', choices=VARIANTS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup)
    runs = {v: [] for v in VARIANTS}
    device = version = None
    for _ in range(a.rounds):
        for v in VARIANTS:                              # a fresh process each: no allocator or cache state carries over
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', v, '--steps', str(a.steps), '--warmup',
                                str(a.warmup), '--hbm-tbs', str(a.hbm_tbs)], capture_output=True, text=True,
                               timeout=a.timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit('adamw_probe: the %s process ended with status %d; nothing more is started' % (v, r.returncode))
            got = json.loads(r.stdout.strip().splitlines()[-1])
            device, version = got['device'], got['torch']
            runs[v].append(got['rows'])
    rows = []
    for i, first in enumerate(runs['fused'][0]):
        row = {'set': first['set'], 'tensors': first['tensors'], 'numel': first['numel'],
               'other_averaged_numel': runs['fused_full'][0][i]['other_averaged_numel']}
        for v in VARIANTS:
            per_round = [r[i] for r in runs[v]]
            last = per_round[-1]
            if not all(x['ran'] for x in per_round):
                row[v] = {'ran': False, 'why': next(x['why'] for x in per_round if not x['ran'])}
                continue
            dev = statistics.median(x['dev_ms'] for x in per_round)
            gbs = last['must_move_mb'] * 1e6 / (dev * 1e-3) / 1e9
            row[v] = {'ran': True, 'dev_ms': round(dev, 4),
                      'host_ms': round(statistics.median(x['host_ms'] for x in per_round), 4),
                      'loop_ms': round(statistics.median(x['loop_ms'] for x in per_round), 4),
                      'all_rounds_dev_ms': [round(x['dev_ms'], 4) for x in per_round],
                      'launches': last['launches'], 'library_launches': sum(last['launches'].values()),
                      'aten_calls': last['aten_calls'], 'kernel_ms': last['kernel_ms'],
                      'must_move_mb': round(last['must_move_mb'], 1), 'gbs': round(gbs, 1),
                      'hbm_frac': round(gbs * 1e9 / (a.hbm_tbs * 1e12), 3), 'clip_info': last['clip_info'],
                      'ema_info': last['ema_info']}
        base = row['fused']['dev_ms']
        for v in VARIANTS:
            if v != 'fused' and row[v]['ran']:
                row[v]['dev_ms_over_fused'] = round(row[v]['dev_ms'] / base, 3)
        rows.append(row)
    line = json.dumps({'probe': 'adamw', 'hyper': {k: list(v) if isinstance(v, tuple) else v for k, v in KW.items()},
                       'steps': a.steps, 'warmup': a.warmup, 'rounds': a.rounds, 'hbm_tbs': a.hbm_tbs,
                       'hbm_source': a.hbm_source, 'device': device, 'torch': version, 'rows': rows})
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
