#!/usr/bin/env python3
"""Step time of the detection pipeline with flip test-time augmentation and box voting: RFBNet-300, bs 32, synthetic weights.

    python tools/tta_probe.py [--batch 32] [--rounds 3] [--steps 30] [--parent-tree DIR] > profiles/tta_probe.json

Variants: plain, hflip (tta='hflip'), hflip_vote (tta='hflip', box_vote=0.5), vote (box_vote=0.5) and, with --parent-tree (a
built checkout of the parent commit), plain_parent: the plain variant of this script run on that tree's package.  Every
measurement is a fresh process (`--child VARIANT`), the variants alternate inside each of --rounds rounds; a child builds the
pipeline, runs 5 steps (two eager, capture, replays), then times --steps graph replays between two HIP events and reports
ms per step.  The report holds every child's figure, the medians and the two differences to judge:
    hflip - 2 x plain          merging plus post-processing on 2P rows instead of twice on P
    hflip_vote - hflip         the voting kernel
One more child (`--child kernels`) runs hflip_vote eagerly under the library's launch records (ct_profile_enable) for the
device time of tta_merge_kernel, hflip_kernel, box_vote_kernel and the kernels of the 2P post-processing, and reports the
workspace sizes of the P and 2P post-processors and of voting.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 20
VARIANTS = {'plain': {}, 'hflip': {'tta': 'hflip'}, 'hflip_vote': {'tta': 'hflip', 'box_vote': 0.5}, 'vote': {'box_vote': 0.5}}
POST_KERNELS = ('select_sort_kernel', 'select_sort_redo', 'clamp_len_kernel', 'nms_segments_kernel', 'prefix_cut_kernel',
                'topk_kernel', 'gather_kernel')


def _pipeline(tree, batch, graph, **kw):
    sys.path.insert(0, os.path.join(tree, 'context-transformer_amd'))
    sys.path.insert(0, tree)
    import torch
    from ctdet import synth
    from ctdet.pipeline import DetectionPipeline
    from data import VOC_300
    from layers.functions import PriorBox
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), 300, T)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()), strict=True)
    net = net.eval().cuda()
    net.device = 'cuda'
    pipe = DetectionPipeline(net, PriorBox(VOC_300).forward(), batch, T, image_wh=(500, 375), graph=graph, **kw)
    return torch, pipe, synth.images(batch, 300, 'randn', 2024).cuda()


def child_step(tree, variant, batch, steps):
    torch, pipe, x = _pipeline(tree, batch, True, **VARIANTS[variant])
    for _ in range(5):
        pipe.run(x)
    torch.cuda.synchronize()
    assert pipe._graph is not None, 'the step was not captured'
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        pipe.run(x)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({'variant': variant, 'ms_per_step': round(e0.elapsed_time(e1) / steps, 4),
                      'rows_kept': int(pipe.post.out_count.sum().item()), 'overflow': int(pipe.post.overflow.item())}))


def child_kernels(tree, batch, steps):
    torch, pipe, x = _pipeline(tree, batch, False, **VARIANTS['hflip_vote'])
    from ctdet import _lib
    lib = _lib.lib()
    for _ in range(3):
        pipe.run(x)
    torch.cuda.synchronize()
    _lib.check(lib.ct_profile_enable(1), 'ct_profile_enable')
    for _ in range(steps):
        pipe.run(x)
    torch.cuda.synchronize()
    n = C.c_int(0)
    _lib.check(lib.ct_profile_collect(None, 0, C.byref(n)), 'ct_profile_collect')
    recs = (_lib.ProfileRecord * max(n.value, 1))()
    _lib.check(lib.ct_profile_collect(recs, n.value, C.byref(n)), 'ct_profile_collect')
    _lib.check(lib.ct_profile_enable(0), 'ct_profile_enable')
    agg = {}
    for i in range(n.value):
        agg[recs[i].name.decode()] = agg.get(recs[i].name.decode(), 0.0) + recs[i].ms
    want = ('hflip_kernel', 'tta_merge_kernel', 'box_vote_kernel') + POST_KERNELS
    per_step = {k: round(agg[k] / steps, 4) for k in want if k in agg}
    per_seg = (pipe.scores[:, :, 1:] > pipe.conf_thresh).sum(1)
    P = pipe.P
    print(json.dumps({
        'kernel_ms_per_step': per_step,
        'postprocess_2P_ms_per_step': round(sum(per_step.get(k, 0.0) for k in POST_KERNELS), 4),
        'candidates_per_segment': {'mean': round(float(per_seg.float().mean().item()), 1), 'max': int(per_seg.max().item())},
        'box_vote_lds_rows': int(lib.ct_box_vote_lds_rows()),
        'workspace_bytes': {'postprocess_P': int(lib.ct_postprocess_workspace_bytes(batch, P, T)),
                            'postprocess_2P': int(lib.ct_postprocess_workspace_bytes(batch, 2 * P, T)),
                            'box_vote_2P': int(lib.ct_box_vote_workspace_bytes(batch, 2 * P, T, pipe.post.cap)),
                            'extra_pipeline_buffers': int(2 * P * (4 + T + 1) * 4 * batch + pipe.x_flip.numel() * 4),
                            'postprocess_2P_rfb512': int(lib.ct_postprocess_workspace_bytes(batch, 2 * 32756, T))}}))


def run_child(tree, what, batch, steps):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', what, '--tree', tree, '--batch', str(batch), '--steps', str(steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError('child %s failed (%d):\n%s' % (what, r.returncode, r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--tree', default=REPO)
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child == 'kernels':
        return child_kernels(a.tree, a.batch, a.steps)
    if a.child:
        return child_step(a.tree, a.child, a.batch, a.steps)
    series = {}
    order = list(VARIANTS) + (['plain_parent'] if a.parent_tree else [])
    for _ in range(a.rounds):
        for v in order:
            tree, what = (a.parent_tree, 'plain') if v == 'plain_parent' else (REPO, v)
            series.setdefault(v, []).append(run_child(tree, what, a.batch, a.steps))
            print('%s: %s' % (v, series[v][-1]), file=sys.stderr, flush=True)
    ms = {v: [c['ms_per_step'] for c in s] for v, s in series.items()}
    med = {v: round(statistics.median(x), 4) for v, x in ms.items()}
    import torch
    out = {'probe': 'detection step with flip TTA and box voting, RFBNet-300 with synthetic weights, graph replay',
           'device': torch.cuda.get_device_name(0), 'batch': a.batch, 'classes': T, 'steps_per_child': a.steps,
           'vote_thresh': 0.5, 'ms_per_step_series': ms, 'ms_per_step_median': med,
           'rows_kept': {v: s[0]['rows_kept'] for v, s in series.items()},
           'hflip_minus_2x_plain_ms': round(med['hflip'] - 2 * med['plain'], 4),
           'hflip_vote_minus_hflip_ms': round(med['hflip_vote'] - med['hflip'], 4),
           'vote_minus_plain_ms': round(med['vote'] - med['plain'], 4)}
    out.update(run_child(REPO, 'kernels', a.batch, 5))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
