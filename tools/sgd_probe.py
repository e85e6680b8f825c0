#!/usr/bin/env python3
"""torch.optim.SGD against ctdet.optim.FusedSGD on the project's parameter sets, same process, same gradients.

    python tools/sgd_probe.py --hbm-tbs 5.1 [--hbm-source "tools/ubench/hbm_stream.hip, 1024 MB RW copy"]

Parameter sets: RFBNet-300 phase 1, RFBNet-300 phase 2, RFBNet-512 phase 2.  Group layouts: `one` (a single group,
as bench.py --train and tools/train_bench.py build it) and `per_tensor` (utils/solver.py::build_optimizer: one group per
tensor, per-name learning rates).  Per combination, alternating torch / fused for --rounds rounds, medians:
  dev_ms    device time per step: HIP events around --steps steps after --warmup warm-up steps, queued behind a
            blocker (matrix products) long enough for the host to issue all of them before the first one starts
  host_ms   host wall time per step of the same loop without a blocker and with no synchronisation inside it
  loop_ms   HIP events around that second loop: what a loop that does nothing but step() sees (host-bound when
            it is close to host_ms)
  fused_kernel_ms   the step's sgd_multi_kernel launches alone, summed from the library's per-launch event records
  launches  fused: sgd_multi_kernel launches of one step as the library's own launch records count them
            (ct_profile_enable), next to what the rule of include/ctdet.h predicts;
            torch: the aten::_foreach_* calls of one step (each is at least one multi_tensor_apply launch)
  hbm_frac  fused only: (5 arrays * 4 B * numel / HBM rate) / dev_ms, the rate being --hbm-tbs (what
            tools/ubench/hbm_stream.hip reports on the same box; named in the output)
Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)

from ctdet import _lib  # noqa: E402
from ctdet.optim import FusedSGD  # noqa: E402
from models.RFB_Net_vgg import build_net  # noqa: E402
from utils import solver  # noqa: E402

SETS = [('rfb300_phase1', 300, 1), ('rfb300_phase2', 300, 2), ('rfb512_phase2', 512, 2)]


def make_opt(kind, layout, args, net):
    if layout == 'per_tensor':
        return solver.build_optimizer(args, net, fused=kind == 'fused')
    cls = FusedSGD if kind == 'fused' else torch.optim.SGD
    return cls([p for p in net.parameters() if p.requires_grad], lr=args.lr, momentum=args.momentum,
               weight_decay=args.weight_decay)


_BLOCK = {}


def blocker(ms):
    """Keep the device busy for about `ms` so that the host can queue the timed steps ahead of it: the events then
    bracket device time alone, not the host's launch rate."""
    if not _BLOCK:
        _BLOCK['x'] = torch.randn(8192, 8192, device='cuda')
        _BLOCK['y'] = torch.empty_like(_BLOCK['x'])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.mm(_BLOCK['x'], _BLOCK['x'], out=_BLOCK['y'])
        e0.record()
        for _ in range(3):
            torch.mm(_BLOCK['x'], _BLOCK['x'], out=_BLOCK['y'])
        e1.record()
        torch.cuda.synchronize()
        _BLOCK['ms'] = e0.elapsed_time(e1) / 3
    for _ in range(int(ms / _BLOCK['ms']) + 1):
        torch.mm(_BLOCK['x'], _BLOCK['x'], out=_BLOCK['y'])


def timed(opt, steps, warmup):
    """-> (device ms per step, host ms per step, ms per step of the loop as the device saw it without a head start)."""
    for _ in range(warmup):
        opt.step()
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    e[0].record()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.step()
    host = (time.perf_counter() - t0) / steps * 1e3
    e[1].record()
    torch.cuda.synchronize()
    blocker(1.5 * host * steps + 5.0)
    e[2].record()
    for _ in range(steps):
        opt.step()
    e[3].record()
    torch.cuda.synchronize()
    return e[2].elapsed_time(e[3]) / steps, host, e[0].elapsed_time(e[1]) / steps


def fused_launches(opt):
    lib = _lib.lib()
    torch.cuda.synchronize()
    lib.ct_profile_enable(1)
    opt.step()
    n = C.c_int(0)
    recs = (_lib.ProfileRecord * 4096)()
    _lib.check(lib.ct_profile_collect(recs, 4096, C.byref(n)), 'ct_profile_collect')
    lib.ct_profile_enable(0)
    mine = [recs[i].ms for i in range(min(n.value, 4096)) if recs[i].name == b'sgd_multi_kernel']
    return len(mine), sum(mine)


def torch_foreach_calls(opt):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        opt.step()
    return sum(e.count for e in prof.key_averages() if e.key.startswith('aten::_foreach'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--hbm-tbs', type=float, required=True, help='HBM rate of this box in TB/s (tools/ubench/hbm_stream.hip)')
    ap.add_argument('--hbm-source', default='tools/ubench/hbm_stream.hip, 1024 MB RW copy, best grid')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    per_launch = _lib.lib().ct_sgd_tensors_per_launch()
    rows = []
    for tag, size, phase in SETS:
        args = types.SimpleNamespace(method='ours', phase=phase, setting='transfer', lr=4e-3, weight_decay=5e-4, momentum=0.9)
        nets = {k: build_net(args, size, 20).cuda() for k in ('torch', 'fused')}
        nets['fused'].load_state_dict(nets['torch'].state_dict())
        gen = torch.Generator(device='cuda').manual_seed(1)
        for pt, pf in zip(nets['torch'].parameters(), nets['fused'].parameters()):
            if pt.requires_grad:
                pt.grad = pf.grad = torch.randn(pt.shape, device='cuda', generator=gen) * 1e-2     # ONE gradient tensor for both
        prm = [p for p in nets['fused'].parameters() if p.requires_grad]
        numel = sum(p.numel() for p in prm)
        floor_ms = 5 * 4 * numel / (a.hbm_tbs * 1e12) * 1e3
        for layout in ('one', 'per_tensor'):
            opts = {k: make_opt(k, layout, args, nets[k]) for k in ('torch', 'fused')}
            t = {k: [] for k in opts}
            for _ in range(a.rounds):
                for k in ('torch', 'fused'):
                    t[k].append(timed(opts[k], a.steps, a.warmup))
            med = {k: [statistics.median(v[i] for v in t[k]) for i in (0, 1, 2)] for k in t}
            launches, kernel_ms = fused_launches(opts['fused'])
            calls = len({(g['momentum'], g['dampening'], g['nesterov']) for g in opts['fused'].param_groups})
            rows.append({
                'set': tag, 'layout': layout, 'tensors': len(prm), 'groups': len(opts['fused'].param_groups), 'numel': numel,
                'torch_dev_ms': round(med['torch'][0], 4), 'torch_host_ms': round(med['torch'][1], 4),
                'fused_dev_ms': round(med['fused'][0], 4), 'fused_host_ms': round(med['fused'][1], 4),
                'torch_loop_ms': round(med['torch'][2], 4), 'fused_loop_ms': round(med['fused'][2], 4),
                'dev_ratio_torch_over_fused': round(med['torch'][0] / med['fused'][0], 3),
                'torch_foreach_calls': torch_foreach_calls(opts['torch']),
                'fused_launches': launches, 'fused_kernel_ms': round(kernel_ms, 4),
                'fused_launches_rule': calls * ((len(prm) + per_launch - 1) // per_launch),
                'hbm_floor_ms': round(floor_ms, 4), 'fused_hbm_frac': round(floor_ms / med['fused'][0], 3),
                'all_rounds_dev_ms': {k: [round(v[0], 4) for v in t[k]] for k in t},
            })
        del nets, opts
        torch.cuda.empty_cache()
    print(json.dumps({'probe': 'sgd', 'steps': a.steps, 'warmup': a.warmup, 'rounds': a.rounds, 'hbm_tbs': a.hbm_tbs,
                      'hbm_source': a.hbm_source, 'tensors_per_launch': per_launch, 'device': torch.cuda.get_device_name(0),
                      'rows': rows}))


if __name__ == '__main__':
    main()
