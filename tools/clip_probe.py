#!/usr/bin/env python3
"""What gradient-norm clipping costs in front of the fused SGD step, on the parameter sets of tools/sgd_probe.py.

    python tools/clip_probe.py --hbm-tbs 4.85 [--hbm-source "tools/ubench/hbm_stream.hip, 1024 MB RW copy"]

Three ways to run one optimizer step over the same parameters and gradients, in ONE process, alternating for --rounds
rounds, medians (dev_ms / host_ms / loop_ms as tools/sgd_probe.py defines them):
  a  FusedSGD.step()                                   ct_sgd_step: the yardstick
  b  FusedSGD(max_grad_norm=...).step()                ct_grad_norm_clip + ct_sgd_step_clipped
  c  torch.nn.utils.clip_grad_norm_ then a             what the option replaces
max_grad_norm is far above the norm, so the coefficient is 1 and all three leave the same parameters behind.
Launches: a and b as the library's own launch records count them (ct_profile_enable), beside the rule of
include/ctdet.h; c adds the aten calls clip_grad_norm_ makes (each is at least one launch, the foreach ones one per
chunk of tensors).  The norm pass alone (grad_norm_kernel + grad_norm_finish_kernel, from the same records) is given in
ms and in GB/s of gradient bytes read, against --hbm-tbs (what tools/ubench/hbm_stream.hip reports on the same box).
Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ctdet import _lib  # noqa: E402
from ctdet.optim import FusedSGD  # noqa: E402
from models.RFB_Net_vgg import build_net  # noqa: E402
from utils import solver  # noqa: E402
from sgd_probe import SETS, timed  # noqa: E402

MAX_NORM = 1e30


class TorchClipThenFused:
    def __init__(self, opt, params):
        self.opt, self.params = opt, params

    def step(self):
        torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
        self.opt.step()


def make_fused(layout, args, net, max_grad_norm):
    if layout == 'per_tensor':
        a = types.SimpleNamespace(**vars(args))
        if max_grad_norm is not None:
            a.max_grad_norm = max_grad_norm
        return solver.build_optimizer(a, net, fused=True)
    return FusedSGD([p for p in net.parameters() if p.requires_grad], lr=args.lr, momentum=args.momentum,
                    weight_decay=args.weight_decay, max_grad_norm=max_grad_norm)


def library_launches(opt):
    """-> {kernel name: (launches, ms)} of one step, from the library's per-launch event records."""
    lib = _lib.lib()
    torch.cuda.synchronize()
    lib.ct_profile_enable(1)
    opt.step()
    n = C.c_int(0)
    recs = (_lib.ProfileRecord * 4096)()
    _lib.check(lib.ct_profile_collect(recs, 4096, C.byref(n)), 'ct_profile_collect')
    lib.ct_profile_enable(0)
    out = {}
    for i in range(min(n.value, 4096)):
        k = recs[i].name.decode()
        c, ms = out.get(k, (0, 0.0))
        out[k] = (c + 1, ms + recs[i].ms)
    return out


def torch_clip_calls(params):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
    return {e.key: e.count for e in prof.key_averages() if e.key.startswith('aten::')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--hbm-tbs', type=float, required=True, help='HBM rate of this box in TB/s (tools/ubench/hbm_stream.hip)')
    ap.add_argument('--hbm-source', default='tools/ubench/hbm_stream.hip, 1024 MB RW copy, best grid')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _lib.lib()
    per_sgd, per_norm = lib.ct_sgd_tensors_per_launch(), lib.ct_grad_norm_tensors_per_launch()
    rows = []
    for tag, size, phase in SETS:
        args = types.SimpleNamespace(method='ours', phase=phase, setting='transfer', lr=4e-3, weight_decay=5e-4, momentum=0.9)
        net = build_net(args, size, 20).cuda()
        gen = torch.Generator(device='cuda').manual_seed(1)
        prm = [p for p in net.parameters() if p.requires_grad]
        for p in prm:
            p.grad = torch.randn(p.shape, device='cuda', generator=gen) * 1e-2
        numel = sum(p.numel() for p in prm)
        for layout in ('one', 'per_tensor'):
            plain = make_fused(layout, args, net, None)
            ways = {'a': plain, 'b': make_fused(layout, args, net, MAX_NORM), 'c': TorchClipThenFused(plain, prm)}
            t = {k: [] for k in ways}
            for _ in range(a.rounds):
                for k in ('a', 'b', 'c'):
                    t[k].append(timed(ways[k], a.steps, a.warmup))
            med = {k: [statistics.median(v[i] for v in t[k]) for i in (0, 1, 2)] for k in t}
            la, lb = library_launches(ways['a']), library_launches(ways['b'])
            info = ways['b'].clip_info()
            norm_ms = sum(lb.get(k, (0, 0.0))[1] for k in ('grad_norm_kernel', 'grad_norm_finish_kernel'))
            step_ms_b = lb.get('sgd_multi_kernel_clipped', (0, 0.0))[1]
            step_ms_a = la.get('sgd_multi_kernel', (0, 0.0))[1]
            calls = len({(g['momentum'], g['dampening'], g['nesterov']) for g in plain.param_groups})
            clip_calls = torch_clip_calls(prm)
            rows.append({
                'set': tag, 'layout': layout, 'tensors': len(prm), 'numel': numel,
                'a_dev_ms': round(med['a'][0], 4), 'b_dev_ms': round(med['b'][0], 4), 'c_dev_ms': round(med['c'][0], 4),
                'a_host_ms': round(med['a'][1], 4), 'b_host_ms': round(med['b'][1], 4), 'c_host_ms': round(med['c'][1], 4),
                'a_loop_ms': round(med['a'][2], 4), 'b_loop_ms': round(med['b'][2], 4), 'c_loop_ms': round(med['c'][2], 4),
                'b_over_a_dev': round(med['b'][0] / med['a'][0], 3), 'c_over_a_dev': round(med['c'][0] / med['a'][0], 3),
                'a_launches': {k: v[0] for k, v in la.items()}, 'b_launches': {k: v[0] for k, v in lb.items()},
                'a_launches_rule': calls * (-(-len(prm) // per_sgd)),
                'b_launches_rule': -(-len(prm) // per_norm) + 1 + calls * (-(-len(prm) // per_sgd)),
                'c_torch_clip_aten_calls': clip_calls,
                'c_torch_clip_foreach_calls': sum(v for k, v in clip_calls.items() if k.startswith('aten::_foreach')),
                'a_kernel_ms': round(step_ms_a, 4), 'b_step_kernel_ms': round(step_ms_b, 4),
                'norm_pass_ms': round(norm_ms, 4), 'norm_pass_over_a_kernel': round(norm_ms / step_ms_a, 3),
                'norm_pass_gbs': round(4 * numel / (norm_ms * 1e-3) / 1e9, 1),
                'norm_pass_hbm_frac': round(4 * numel / (norm_ms * 1e-3) / (a.hbm_tbs * 1e12), 3),
                'clip_info': info,
                'all_rounds_dev_ms': {k: [round(v[0], 4) for v in t[k]] for k in t},
            })
        del net, ways, plain
        torch.cuda.empty_cache()
    print(json.dumps({'probe': 'clip', 'steps': a.steps, 'warmup': a.warmup, 'rounds': a.rounds, 'hbm_tbs': a.hbm_tbs,
                      'hbm_source': a.hbm_source, 'sgd_tensors_per_launch': per_sgd,
                      'grad_norm_tensors_per_launch': per_norm, 'device': torch.cuda.get_device_name(0), 'rows': rows}))


if __name__ == '__main__':
    main()
