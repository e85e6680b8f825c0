#!/usr/bin/env python3
"""bench.py -- images/sec of forward + NMS for RFBNet-300 (BASELINE.json metric).

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --train [--gpus N]          data-parallel TRAINING step (BASELINE configs[3]), see below

A plain run sets up, warms up (W steps), times K steps, writes the outputs of the last timed step if --dump-outputs is
given, and prints one JSON line; `ms_per_step` is the wall time of the K timed steps / K.  Everything else the
benchmark measures (roofline, stage rooflines, other configurations, CPU baseline: "Extra objects" below) runs only
with --full.

`--gpus N` with N > 1 and no torchrun environment (no WORLD_SIZE): bench.py launches its own N ranks through
torch.distributed.run on 127.0.0.1, one per GPU, over RCCL (backend 'nccl'); it never prints a 1-GPU number for an
N-GPU request: N > visible devices exits non-zero (unless --share-devices rehearses the N-rank path on fewer GPUs
over gloo), and so does a process group whose size is not N.  The line carries `rccl_ranks`, the backend, and per
rank the device index / PCI bus id and its own ms/step.

One "step" = one pass of the whole hot path over one synthetic batch already resident in HBM:
RFBNet engine (fused HIP convs) -> fused softmax/decode/score fusion -> per (image, class)
threshold + sort + NMS(0.45) -> per-image top-200 (test.py:130-161 generalised to a batch).
Workload = BASELINE.json configs[1]: RFBNet-300 VGG16, bs=32 per GPU, fp32, 20 foreground
classes, name-seeded random weights (no checkpoints/datasets offline).  Images shard across
ranks with no data-path collective (inference).  `--scaling weak` (default): every rank owns
--batch images; `--scaling strong`: ONE batch of --batch images is split over the ranks, the
reference's DataParallel scatter (train.py:296-297).  value = all images / max-over-ranks time.

--dump-outputs DIR: after the timed steps, what a caller of the timed path receives from its last step, as DIR/<name>.npy
(float32; float64 for the training loss), at most 64 MB in all; inputs and weights are seeded, so two builds run with the
same arguments can be compared file by file.  Inference: detections [B, classes, cap, 5] (x1 y1 x2 y2 score; rows past
a class's count zeroed), detection_counts [B, classes], and fixed samples of the per-prior decoded boxes and fused scores.
--train: loss [1] and a fixed sample of the parameters after the last SGD update.  A tensor above its element budget is
replaced by the elements at sorted indices drawn without replacement by numpy's default_rng(0) (same sample every run).

Extra objects on the JSON line (--full, N=1, rank 0; null otherwise):
  roofline      dominant kernel = the conv kernel with the most accumulated time of its own, from HIP events recorded on
                the launch stream around every conv launch.  The timed region replays a hipGraph, inside which no
                per-launch events exist, so the same K steps run once more as eager launches right after it
                (`events_from` says which).  `achieved`/`frac` count the multiply-adds the kernel's algorithm
                executes on the matrix pipe it uses (Winograd F(4x4,3x3): 36/144 of the direct-convolution count,
                x 3 piece products on the f16x2 operand form, x 6 on bf16x3) against that pipe's dense peak;
                `algorithmic_*` is the direct-convolution FLOP count of SURVEY 8(d) over the same time (can exceed
                the fp32 peak -- that is the Winograd / operand-form saving, not a roofline fraction).
                `traffic` = HBM bytes per launch from the committed rocprofv3 --pmc passes (profiles/).
    .stages     context attention / score fusion / select+sort / NMS kernels: per-launch HIP events
                recorded by the library (ct_profile_enable) in a few extra steps after the timed region,
                against the roofline that bounds each, `traffic` from the same PMC passes.
  cpu_baseline  the CPU oracle (port of the reference path: stock torch-CPU fp32 ops + C NMS) on a bounded
                sample (BASELINE configs[0] shape): forward swept over thread counts, the whole pipeline at the best
                of them (`value`, `cores`) and at all physical cores (`value_all_cores`), split by stage.
  other_configs the other single-GPU configurations BASELINE.json names (512, +Context-Transformer, the
                bs-4 shard of a strong-scaled batch, the per-GPU shape of configs[4]: bf16 512x512 bs 16 with its own
                roofline block, the per-GPU training steps of configs[3]), a few steps each in the same process.

--train: one step = forward (batch-statistics BatchNorm) + MultiBoxLoss_combined + HIP backward with the bucketed
gradient all-reduce issued from inside it (ctdet.dist.GradBucketer, RCCL) + SGD update; default workload = the
per-GPU share of BASELINE configs[3] (RFBNet-512 + Context-Transformer, phase 2 transfer, bs 8 per GPU).  For N > 1
the line also reports the same step without the all-reduce, the all-reduce alone (bucket by bucket on the idle GPU)
and overlap = 1 - (step_with - step_without) / allreduce_alone.
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)

PEAK_F32_MFMA_TFLOPS = 157.3
PEAK_BF16_MFMA_TFLOPS = 2500.0      # dense bf16 MFMA (MI355X_MICROARCH.md), --dtype bf16 only
PEAK_HBM_GBS = 8000.0               # HBM3E spec (6.3 TB/s achievable, MI355X_MICROARCH.md)
# multiplications executed / direct-convolution multiplications: F(2x2,3x3) 16 per 4 outputs x 9, F(4x4,3x3) 36 per 16 x 9
# st.rt['wino'] code 23 is F(2x2,3x3) on the bf16 pipe (csrc/ct_wino_x3.hip): every
# transform-domain multiplication is six bf16 MFMA products (bf16x3), priced against the bf16 MFMA peak
WINOGRAD_MULT_RATIO = {2: 16.0 / 36.0, 4: 36.0 / 144.0, 23: 16.0 / 36.0, 44: 36.0 / 144.0,
                       46: 36.0 / 144.0, 47: 36.0 / 144.0, 48: 36.0 / 144.0}
# 44: one conv launch = three kernels (csrc/ct_wino4s.hip: wino4s_in, wino4s_gemm, wino4s_out); 47: the same on the
# f16x2 operand form (csrc/ct_f16x2.h: absmax pass, wino4s_in<h2>, wino4h_gemm, wino4s_out<h2>); 48: the fused kernel on f16x2
WINOGRAD_KERNEL = {2: 'wino_f2x2_3x3_f32', 4: 'wino_f4x4_3x3_f32', 23: 'wino_f2x2_3x3_x3',
                   44: 'wino4s(in+gemm+out)', 46: 'wino_f4x4_3x3_x3',
                   47: 'wino4s_h2(absmax+in+gemm+out)', 48: 'wino_f4x4_3x3_h2'}
WINOGRAD_X3 = (23, 44, 46, 47, 48)       # on the 16-bit matrix pipe; 46: F(4x4,3x3) fused on bf16x3 (csrc/ct_wino4f.hip)
WINOGRAD_F4 = (4, 44, 46, 47, 48)
WINOGRAD_H2 = (47, 48)                   # f16x2: two binary16 pieces, THREE piece products per multiply-add (bf16x3: six)


# what the matrix pipe of this part sustains in a loop of MFMAs without any memory traffic (the data sheet's 2.5 PFLOP/s is the
# all-zero-operand figure: with real data the chip lowers its clock)
SUSTAINED_PEAK = {'f16_mfma_tflops_gaussian_operands': 1689, 'f16_mfma_tflops_zero_operands': 2419,
                  'bf16_mfma_tflops_gaussian_operands': 1824, 'bf16_mfma_tflops_zero_operands': 2402,
                  'source': 'tools/ubench/f16x2_probe.hip, profiles/r06_f16x2_probe.txt (tools/ubench/mfma_power.hip, '
                            'profiles/r04_mfma_power.txt: 1722 / 2474 for bf16 on another box)'}


def piece_products(wino):
    return 3.0 if wino in WINOGRAD_H2 else 6.0


def _lib_config_name(cfg):
    from ctdet import _lib
    return _lib.lib().ct_conv_config_name(cfg - 1).decode() if cfg > 0 else 'auto'


def build_net(size, num_fg, phase, setting, device):
    from models.RFB_Net_vgg import build_net as bn
    from ctdet import synth
    args = types.SimpleNamespace(method='ours', phase=phase, setting=setting)
    net = bn(args, size, num_fg)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()), strict=True)
    net = net.eval().to(device)
    net.device = device
    return net


def physical_cores():
    try:
        import psutil
        n = psutil.cpu_count(logical=False)
        if n:
            return int(n), 'psutil physical cores'
    except Exception:
        pass
    return int(os.cpu_count() or 1), 'os.cpu_count() logical CPUs'


def cpu_baseline(size, num_fg, images=4, reps=2):
    """Oracle (port) timed on the host cores, SURVEY 8(d): forward / Detect / per-class NMS + top-200 timed
    separately and end to end.  torch-CPU convolutions do not scale to every core at 4 images, so the forward is
    first timed over a small sweep of thread counts (1, 16, 32, 64, all physical cores; one run after one warm-up
    each) and the whole pipeline is then timed at the BEST of them -- that is `value` / `cores`; the sweep and the
    one-thread figure are reported next to it.  Bounded: about 15-25 s of host time."""
    from ctdet import synth
    from oracle import box_ref, nms_ref, rfbnet_ref
    nms_ref.build_c()
    allc, src = physical_cores()
    forced = int(os.environ.get('CTDET_CPU_THREADS', 0))
    sd = synth.fill_state_dict(rfbnet_ref.param_shapes(size, num_fg, 1))
    priors = box_ref.prior_box(box_ref.ANCHOR_CFGS['VOC_%d' % size])
    x = synth.images(images, size, 'randn', 1234)

    def forward_only(n_threads):
        torch.set_num_threads(n_threads)
        with torch.no_grad():
            rfbnet_ref.forward(sd, x, size, num_fg)
            t0 = time.perf_counter()
            rfbnet_ref.forward(sd, x, size, num_fg)
            return time.perf_counter() - t0

    def run(n_threads, n_reps):
        torch.set_num_threads(n_threads)
        rows = []
        with torch.no_grad():
            for r in range(n_reps + 1):
                t0 = time.perf_counter()
                loc, conf, obj = rfbnet_ref.forward(sd, x, size, num_fg)
                t1 = time.perf_counter()
                boxes, scores = box_ref.detect(loc, conf, obj, priors)
                t2 = time.perf_counter()
                for i in range(images):
                    nms_ref.postprocess_image(boxes[i].numpy(), scores[i].numpy(), (500, 375), nms_fn=nms_ref.nms_c)
                t3 = time.perf_counter()
                if r > 0:
                    rows.append((t3 - t0, t1 - t0, t2 - t1, t3 - t2))
        med = np.median(np.array(rows), axis=0)
        return {'images_per_s': round(images / float(med[0]), 3),
                'ms_per_image': {'forward': round(float(med[1]) / images * 1e3, 2),
                                 'detect': round(float(med[2]) / images * 1e3, 2),
                                 'nms_top200': round(float(med[3]) / images * 1e3, 2)}}
    before = torch.get_num_threads()
    sweep = {}
    for n in ([forced] if forced > 0 else sorted({1, 16, 32, 64, allc})):
        if n <= allc or forced > 0:
            sweep[n] = forward_only(n)
    best = min(sweep, key=sweep.get)
    full = run(best, reps)
    full_all = full if best == allc else run(allc, 1)        # "n = all physical host cores" next to the best count
    torch.set_num_threads(before)
    return {'value': full['images_per_s'], 'unit': 'images/s', 'cores': best, 'kind': 'port',
            'value_all_cores': full_all['images_per_s'],
            'cores_available': allc, 'cores_source': src if forced <= 0 else 'CTDET_CPU_THREADS',
            'stages_ms_per_image': full['ms_per_image'],
            'thread_sweep_forward_ms_per_image': {str(n): round(t / images * 1e3, 1) for n, t in sorted(sweep.items())},
            'sample': '%d synthetic %dx%d images (BASELINE configs[0] shape): torch-CPU fp32 forward + Detect + per-class '
                      'C NMS + top-200; forward timed at %s threads (1 run after 1 warm-up each), the whole pipeline at '
                      'the best of them (%d), median of %d runs after 1 warm-up; value_all_cores = the same pipeline at all '
                      '%d physical cores (1 run after 1 warm-up)'
                      % (images, size, size, '/'.join(str(n) for n in sorted(sweep)), best, reps, allc)}


def load_pmc(workload):
    """{kernel name prefix: HBM bytes per launch} from the NEWEST committed rocprofv3 PMC passes recorded for THIS
    workload (profiles/*_pmc_traffic*.json: separate --pmc FETCH_SIZE / WRITE_SIZE runs, 2*FETCH+WRITE per
    MI355X_MICROARCH.md).  One file only: kernels change template signature between rounds and an older round's rows
    must not answer for this round's kernels."""
    import glob
    best = {}
    for path in sorted(glob.glob(os.path.join(REPO, 'profiles', '*_pmc_traffic*.json'))):
        try:
            table = json.load(open(path))
        except (OSError, ValueError):
            continue
        if table.get('__workload__', {'size': 300, 'batch': 32, 'phase': 1, 'classes': 20}) != workload:
            continue
        rows = {k: (v['hbm_bytes'], os.path.basename(path)) for k, v in table.items() if k != '__workload__'}
        if rows:
            best = rows
    return best


def pmc_lookup(pmc, name):
    """HBM bytes per launch of kernel `name` (bench naming) in the PMC table (rocprof naming: template arguments spelled out; the
    f16x2 instantiations are the ones whose LAST template argument is `true`)."""
    import re
    m = re.match(r'conv_igemm_f32<(\d+)x(\d+),(\d+)x(\d+)', name)
    x = re.match(r'conv_(x3|h2)_f32<\d+x\d+,(\d+)x(\d+)k(\d+)(d?)>', name)
    alias = {'wino_f4x4_3x3_h2': ('wino_f4x4_3x3_x3<', True), 'wino_f4x4_3x3_x3': ('wino_f4x4_3x3_x3<', False)}

    def targs(k):
        return [t.strip() for t in k[k.find('<') + 1:k.rfind('>')].split(',')] if '<' in k else []
    cands = []
    for k, (v, _) in pmc.items():
        if x:       # rocprof: conv_x3_f32<BM, BN, BK, dual, h2>; one instantiation serves every filter geometry
            f = targs(k)
            if k.startswith('conv_x3_f32') and len(f) >= 4 and tuple(f[:3]) == x.groups()[1:4] and \
                    (f[3] in ('true', '1')) == bool(x.group(5)) and ((f[4] in ('true', '1')) if len(f) > 4 else False) == (x.group(1) == 'h2'):
                return v
        elif m:
            f = targs(k)
            if k.startswith('conv_igemm_f32') and len(f) >= 5 and (f[0], f[1], f[3], f[4]) == m.groups():
                return v
        elif name in alias:
            pre, h2 = alias[name]
            f = targs(k)
            if k.startswith(pre) and (len(f) >= 3 and f[2] in ('true', '1')) == h2:    # <SEG, PLAIN, H2>
                return v
        elif name == 'wino4s_gemm' and (k.startswith('wino4h_gemm') or k.startswith('wino4s_gemm')):
            return v
        elif k.startswith(name):
            cands.append(v)
    # several instantiations share a bench name (select_sort_kernel<4096, true> and the near-empty re-sort launch <4096, false>):
    # the one that moves the bytes
    return max(cands, key=lambda t: t[0] if isinstance(t, tuple) else t) if cands else None


def conv_roofline(rt, batch, pmc, pick=None):
    """Per-instantiation totals from the HIP events the engine recorded around every conv launch
    of the timed region; reports the instantiation with the most accumulated time (or the one named `pick`)."""
    from ctdet import _lib
    lib = _lib.lib()
    agg = {}
    bf16 = getattr(rt.backend, 'load_input', None) is not None       # NHWC bf16 path (--dtype bf16, configs[4])
    x3_names = rt.backend.x3_names() if hasattr(rt.backend, 'x3_names') else []
    for st, e0, e1 in rt.event_log:
        cfg = st.rt['desc'].config
        wino = int(st.rt.get('wino') or 0)              # 0, 2 = F(2x2,3x3), 4 = F(4x4,3x3)
        x3 = st.rt.get('x3')
        if bf16:
            name, mult, pk = 'conv_bf16_nhwc', 1.0, PEAK_BF16_MFMA_TFLOPS
        elif wino in WINOGRAD_X3:
            name, mult, pk = WINOGRAD_KERNEL[wino], WINOGRAD_MULT_RATIO[wino] * piece_products(wino), PEAK_BF16_MFMA_TFLOPS
        elif wino:
            name, mult, pk = WINOGRAD_KERNEL[wino], WINOGRAD_MULT_RATIO[wino], PEAK_F32_MFMA_TFLOPS
        elif x3 is not None:
            # bf16x3: six bf16 MFMA products per fp32 multiply-add, on the bf16 pipe; f16x2 ('h2:' configurations): three f16 products
            h2 = x3_names[x3].startswith('h2:')
            name, mult, pk = 'conv_%s_f32<%dx%d,%s>' % ('h2' if h2 else 'x3', st.kh, st.kw, x3_names[x3][3:]), 3.0 if h2 else 6.0, \
                PEAK_BF16_MFMA_TFLOPS
        else:
            cname = lib.ct_conv_config_name(cfg - 1).decode() if cfg > 0 else 'auto'
            name = st.rt.get('kernel_name') or 'conv_igemm_f32<%dx%d,%s>' % (st.kh, st.kw, cname)
            mult, pk = 1.0, PEAK_F32_MFMA_TFLOPS
            if cname == 'valu' or (cfg == 0 and st.cin == 3 and (st.kh, st.kw) == (3, 3)):
                # the 3-channel image layer on the vector ALU (v_pk_fma_f32): 256 CUs x 4 SIMDs x 16 lanes x 2 (packed)
                # x 2 flop x 2.4 GHz = 157.3 TFLOP/s, numerically the fp32 MFMA peak; the kernel is bound by its
                # 8 KB-per-pixel-row output stream, not by either pipe
                name = 'conv_valu3x3_f32'
        a = agg.setdefault(name, [0.0, 0.0, 0, 0.0, pk])
        a[0] += e0.elapsed_time(e1) * 1e-3
        a[1] += st.flops(batch)                # direct-convolution flops
        a[2] += 1
        a[3] += st.flops(batch) * mult         # multiply-adds x2 sent to the matrix pipe the kernel uses
    tot_t = sum(a[0] for a in agg.values())
    tot_f = sum(a[1] for a in agg.values())
    tot_x = sum(a[3] for a in agg.values())
    tot_peak_s = sum(a[3] / (a[4] * 1e12) for a in agg.values())     # seconds the executed work needs at its pipe's peak
    name, (t, f, n, fx, peak) = max(agg.items(), key=lambda kv: kv[1][0]) if pick is None else (pick, agg[pick])
    wino = {v: k for k, v in WINOGRAD_KERNEL.items()}.get(name, 0)
    ach = fx / t / 1e12
    nlog, nconv = max(1, len(rt.event_log)), len(rt.conv_steps())
    return {
        'bound': 'mfma', 'achieved': round(ach, 2), 'peak': peak, 'unit': 'TFLOP/s',
        'frac': round(ach / peak, 4), 'traffic': pmc_lookup(pmc, name),
        # the same multiply-adds priced as bf16x3 would execute them (six piece products): an f16x2 kernel issues half the
        # products of its bf16x3 twin, so its `frac` halves while it gets faster -- this is the figure that compares across rounds
        'frac_bf16x3_equivalent': round(ach / peak * (2.0 if (wino in WINOGRAD_H2 or name.startswith('conv_h2')) else 1.0), 4),
        'kernel': name, 'launches': n, 'avg_launch_us': round(t / n * 1e6, 2),
        'flops_per_launch': round(fx / n),
        'flops_definition': 'multiply-adds x2 executed on the matrix pipe per launch' +
                            (' = direct-convolution flops x %s (Winograd F(%dx%d,3x3), output-tile padding not counted)%s'
                             % ('36/144' if wino in WINOGRAD_F4 else '16/36', 4 if wino in WINOGRAD_F4 else 2, 4 if wino in WINOGRAD_F4 else 2,
                                (' x 3 (f16x2 split, f16 MFMA pipe)' if wino in WINOGRAD_H2 else ' x 6 (bf16x3 split, bf16 MFMA pipe)' if wino in WINOGRAD_X3 else '')) if wino else
                             ' = direct-convolution flops x 6 (bf16x3 split, bf16 MFMA pipe)' if name.startswith('conv_x3') else ''),
        'algorithmic_flops_per_launch': round(f / n),
        'algorithmic_achieved': round(f / t / 1e12, 2),
        'algorithmic_frac': round(f / t / 1e12 / PEAK_F32_MFMA_TFLOPS, 4) if not bf16 else round(f / t / 1e12 / peak, 4),
        'winograd_mult_ratio': round(WINOGRAD_MULT_RATIO[wino], 4) if wino else 1.0,
        'peaks': {'f32_mfma_tflops': PEAK_F32_MFMA_TFLOPS, 'bf16_mfma_tflops': PEAK_BF16_MFMA_TFLOPS,
                  'note': 'executed_frac of a kernel is against the pipe it runs on (conv_x3_f32: bf16 MFMA, six bf16 '
                          'products per fp32 multiply-add; every other fp32 kernel: fp32 MFMA); algorithmic_frac is the '
                          'direct-convolution flop rate over the fp32 MFMA peak (can exceed 1: Winograd / bf16x3 savings)'},
        'by_kernel': {k: {'launches_per_step': round(v[2] / nlog * nconv, 1),
                          'ms_per_step': round(v[0] / nlog * nconv * 1e3, 3),
                          'executed_frac': round(v[3] / v[0] / 1e12 / v[4], 4),
                          'algorithmic_frac': round(v[1] / v[0] / 1e12 / (v[4] if bf16 else PEAK_F32_MFMA_TFLOPS), 4)}
                      for k, v in sorted(agg.items(), key=lambda kv: -kv[1][0])[:6]},
        'all_conv': {'achieved': round(tot_x / tot_t / 1e12, 2),
                     # time the executed work would need at the peak of the pipe it runs on / measured launch time
                     'frac': round(tot_peak_s / tot_t, 4),
                     'algorithmic_achieved': round(tot_f / tot_t / 1e12, 2),
                     'algorithmic_frac': round(tot_f / tot_t / 1e12 / (peak if bf16 else PEAK_F32_MFMA_TFLOPS), 4),
                     'time_share_of_dominant': round(t / tot_t, 3),
                     # sum of the launch durations; with the two-stream schedule launches overlap, so this
                     # can exceed the wall time of a step (and every duration includes the contention)
                     'sum_launch_ms_per_step': round(tot_t / nlog * nconv * 1e3, 3),
                     'launches_per_step': nconv,
                     'streams': 2 if getattr(rt, 'side', None) is not None else 1},
    }


def stage_rooflines(pipe, x, steps, pmc):
    """Per-launch HIP events from the library's own profile scopes (ct_profile_enable) over `steps` extra steps."""
    from ctdet import _lib
    lib = _lib.lib()
    B, P, T = pipe.batch, pipe.P, pipe.T
    torch.cuda.synchronize()
    graph_mode, pipe.use_graph = pipe.use_graph, False      # per-launch events need eager launches
    _lib.check(lib.ct_profile_enable(1), 'ct_profile_enable')
    for _ in range(steps):
        pipe.run(x)
    torch.cuda.synchronize()
    pipe.use_graph = graph_mode
    n = C.c_int(0)
    _lib.check(lib.ct_profile_collect(None, 0, C.byref(n)), 'ct_profile_collect')
    recs = (_lib.ProfileRecord * max(n.value, 1))()
    _lib.check(lib.ct_profile_collect(recs, n.value, C.byref(n)), 'ct_profile_collect')
    agg = {}
    for i in range(n.value):
        a = agg.setdefault(recs[i].name.decode(), [0.0, 0])
        a[0] += recs[i].ms * 1e-3
        a[1] += 1
    _lib.check(lib.ct_profile_enable(0), 'ct_profile_enable')
    per_seg = (pipe.scores[:, :, 1:] > pipe.conf_thresh).sum(1)               # candidates per (image, class)
    cand = int(per_seg.sum().item())
    sorted_rows = int(per_seg.clamp(max=1024).sum().item())
    net = pipe.net
    work = {
        # loc 16P + conf 4CP + obj 8P in, boxes 16P + scores 4(T+1)P out per image, priors 16P once
        'detect_kernel': ('hbm', B * P * (16 + 4 * pipe.scores_in_ch + 8 + 16 + 4 * (T + 1)) + 16 * P),
        # threshold scan of every score, an 8 B key per candidate written and read back, and a 20 B row + 4 B index for the
        # candidates that are sorted: the best >= 1024 of a class under the top-k rule (csrc/ct_post.hip, partial sort)
        'select_sort_kernel': ('hbm', B * P * (T + 1) * 4 + cand * 16 + sorted_rows * 24),
        # 20 B row in + 4 B kept index out per candidate (SURVEY 8d "20N in + 4N out"), both NMS passes share it
        'nms_segments_kernel': ('hbm', cand * 24),
    }
    w4s = [st for st in pipe.rt.conv_steps() if int(st.rt.get('wino') or 0) in (44, 47)]
    if w4s:
        # the three kernels of the F(4x4,3x3) / bf16x3 layers, summed over the layers of a step (csrc/ct_wino4s.hip):
        # tiles padded to 128, couts to 128; V = 36 points x 3 bf16 pieces, M = 36 points x fp32; dilated layers (pad = dilation)
        # have their tiles on the dilation sub-lattices
        gf = gfp = ib = ob = 0.0
        for st in w4s:
            dl = st.dil              # dilated layers: dl x dl sub-lattices of ceil(oh / dl) x ceil(ow / dl) pixels, tiled like images
            tiles = B * dl * dl * ((-(-st.oh // dl) + 3) // 4) * ((-(-st.ow // dl) + 3) // 4)
            tpad, mpad = -(-tiles // 128) * 128, -(-st.cout // 128) * 128
            pp = piece_products(int(st.rt['wino']))          # piece products per multiply-add (f16x2: 3, V = two 2-byte pieces; bf16x3: 6, three pieces)
            gf += 36.0 * tiles * st.cin * st.cout * 2 * pp         # useful work: the layer's own tiles and couts
            gfp += 36.0 * tpad * st.cin * mpad * 2 * pp            # what the 128 x 128 blocks execute
            ib += 4.0 * B * st.cin * st.h * st.w + (4.0 if pp == 3.0 else 6.0) * 36 * tpad * st.cin
            ob += 4.0 * 36 * tiles * st.cout + 4.0 * B * st.cout * st.oh * st.ow
        work['wino4s_gemm'] = ('mfma_bf16', gf)
        gemm_padded = gfp
        work['wino4s_in'] = ('hbm', ib)
        work['wino4s_out'] = ('hbm', ob)
    if net.method == 'ours' and net.phase == 2:
        d, M = net.num_classes, pipe.rt.plan.M
        work['ctx_attn_kernel'] = ('mfma', B * 4.0 * P * M * d)      # QK^T and PV contractions, 2 flop per multiply-add
        # read conf P*d*4 + pooled conf M*d*4, write P*T*4 per image (4.17 MB at 300 / transfer)
        work['ctx_attn_kernel.hbm'] = ('hbm', B * (P * d * 4 + M * d * 4 + P * pipe.scores_in_ch * 4))
    out = {}
    for key, (bound, amount) in work.items():
        kname = key.split('.')[0]
        if kname not in agg:
            continue
        t, cnt = agg[kname]
        per_launch = amount / (cnt / steps)
        avg = t / cnt
        if bound == 'mfma_bf16':
            ach, peak, unit, bound = per_launch / avg / 1e12, PEAK_BF16_MFMA_TFLOPS, 'TFLOP/s', 'mfma'
        elif bound == 'mfma':
            ach, peak, unit = per_launch / avg / 1e12, PEAK_F32_MFMA_TFLOPS, 'TFLOP/s'
        else:
            ach, peak, unit = per_launch / avg / 1e9, PEAK_HBM_GBS, 'GB/s'
        out[key] = {'bound': bound, 'achieved': round(ach, 2), 'peak': peak, 'unit': unit, 'frac': round(ach / peak, 4),
                    'launches_per_step': round(cnt / steps, 2), 'avg_launch_us': round(avg * 1e6, 2),
                    'algorithmic_per_launch': int(per_launch), 'traffic': pmc_lookup(pmc, kname)}
        if key == 'wino4s_gemm':
            # the MFMAs the 128 x 128 blocks issue, padding included (tiles and couts rounded up to 128)
            out[key]['executed_incl_padding_per_launch'] = int(gemm_padded / (cnt / steps))
            out[key]['executed_incl_padding_frac'] = round(gemm_padded / (cnt / steps) / avg / 1e12 / peak, 4)
    if 'ctx_attn_kernel' in out:
        from ctdet import _lib as _l
        # piece products per multiply-add of the attention's two contractions: 6 = bf16x3 (default), 3 = f16x2 (CTDET_ATTN_H2=1)
        out['ctx_attn_kernel']['piece_products'] = int(_l.lib().ct_ctx_attention_piece_products())
    out['other_kernels_us_per_step'] = {k: round(v[0] / steps * 1e6, 2) for k, v in sorted(agg.items())
                                        if k not in [w.split('.')[0] for w in work]}
    out['candidates_per_step'] = cand
    return out


def log(msg):
    if os.environ.get('CTDET_BENCH_VERBOSE', '1') != '0' and int(os.environ.get('RANK', 0)) == 0:
        sys.stderr.write('[bench %7.1fs] %s\n' % (time.perf_counter() - _T0, msg))
        sys.stderr.flush()


_T0 = time.perf_counter()

DUMP_LIMIT_BYTES = 64 * 1000 * 1000          # --dump-outputs: every file together
DUMP_SAMPLE_SEED = 0


def dump_outputs(out_dir, arrays):
    """--dump-outputs: each (name, tensor, max_elements) -> out_dir/<name>.npy, float32 (float64 stays float64).  A tensor
    with more elements than its max is replaced by a fixed sample: the flattened elements at sorted indices drawn without
    replacement by np.random.default_rng(DUMP_SAMPLE_SEED) -- the same indices for the same shape on every run."""
    os.makedirs(out_dir, exist_ok=True)
    total, shapes = 0, {}
    for name, t, max_elems in arrays:
        t = t.detach()
        if t.numel() > max_elems:
            idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(t.numel(), max_elems, replace=False))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        arr = t.cpu().numpy().astype(np.float64 if t.dtype == torch.float64 else np.float32)
        total += arr.nbytes
        if total > DUMP_LIMIT_BYTES:
            raise SystemExit('bench.py --dump-outputs: %s would take the files past %d bytes' % (name, DUMP_LIMIT_BYTES))
        np.save(os.path.join(out_dir, name + '.npy'), arr)
        shapes[name] = list(arr.shape)
    log('outputs written to %s: %s (%.1f MB)' % (out_dir, shapes, total / 1e6))


def inference_outputs(pipe):
    """What DetectionPipeline.run hands its caller (out_dets, out_count), plus samples of the per-prior boxes / scores it
    also leaves on the device, for --dump-outputs."""
    post = pipe.post
    if int(post.overflow.item()):
        raise SystemExit('bench.py --dump-outputs: postprocess output capacity %d exceeded' % post.cap)
    dets = post.out_dets.clone()
    rows = torch.arange(dets.shape[2], device=dets.device)
    dets[rows.view(1, 1, -1) >= post.out_count.unsqueeze(-1)] = 0.0      # only rows [0, count) are part of the result
    return [('detections', dets, 1 << 23), ('detection_counts', post.out_count, 1 << 23),
            ('boxes', pipe.boxes, 1 << 20), ('scores', pipe.scores, 1 << 20)]


def make_pipeline(size, num_fg, phase, setting, batch, dtype, dev):
    from ctdet.pipeline import DetectionPipeline
    from layers.functions import PriorBox
    import data as cfgs
    T = 20 if phase == 2 else num_fg
    net = build_net(size, num_fg, phase, setting, dev)
    net.conv_dtype = dtype
    priors = PriorBox(getattr(cfgs, 'VOC_%d' % size)).forward()
    pipe = DetectionPipeline(net, priors, batch, T, image_wh=(500, 375))
    pipe.scores_in_ch = T            # channels of the conf tensor the score-fusion kernel reads
    return pipe


def quick_config(size, num_fg, phase, setting, batch, dtype, dev, steps=5, warmup=4, roofline=False):
    """ms/step and images/s of another configuration, same step definition, in this process.  roofline=True adds the
    conv roofline block of that configuration (HIP events around every conv launch of an eager pass + the committed
    PMC traffic of that workload)."""
    from ctdet import synth
    pipe = make_pipeline(size, num_fg, phase, setting, batch, dtype, dev)
    x = synth.images(batch, size, 'randn', 4321).to(dev)
    for _ in range(warmup):
        pipe.run(x)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        pipe.run(x)
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / steps
    flops = pipe.rt.plan.conv_flops()
    res = {'ms_per_step': round(dt * 1e3, 3), 'images_per_s': round(batch / dt, 1), 'batch': batch, 'steps': steps,
           'dtype': dtype, 'launch_mode': 'hipGraph replay' if pipe._graph is not None else 'eager launches',
           'conv_gflop_per_image': round(flops / batch / 1e9, 2),
           'conv_algorithmic_tflops': round(flops / dt / 1e12, 1),
           'live_tuned_layers': len(getattr(pipe.rt, 'live_tuned', [])),
           'policy': pipe.rt.policy_record() if hasattr(pipe.rt, 'policy_record') else None,
           'operand_form': 'bf16' if dtype == 'bf16' else 'f16x2' if getattr(pipe.rt.backend, 'h2', False) else 'bf16x3'}
    if roofline:
        pipe.rt.event_log = []
        for _ in range(steps):
            pipe.run(x)
        torch.cuda.synchronize(dev)
        pmc = load_pmc({'size': size, 'batch': batch, 'phase': phase, 'classes': num_fg})    # kernel names tell the dtypes apart
        res['roofline'] = conv_roofline(pipe.rt, batch, pmc)
        res['roofline']['events_from'] = 'an eager pass of the same %d steps' % steps
        res['roofline']['traffic_source'] = sorted({v[1] for v in pmc.values()}) or None
        pipe.rt.event_log = None
    del pipe, x
    torch.cuda.empty_cache()
    return res


def train_config(size, num_fg, phase, setting, batch, dev, steps=4, warmup=2, rank=0, world=1, after_timed=None):
    """One data-parallel training step (train.py:222-229 on this rank's image shard): forward with batch-statistics
    BatchNorm, MultiBoxLoss_combined, HIP backward with the bucketed gradient all-reduce issued from inside it, SGD.
    Returns local timings; for world > 1 also the step without the all-reduce and the all-reduce alone.
    after_timed(net, loss): called right after the timed steps, before any further step changes the parameters."""
    import torch.distributed as tdist
    from ctdet import synth, dist as cdist
    from models.RFB_Net_vgg import build_net as bn
    from layers.functions import PriorBox
    from layers.modules.multibox_loss_combined import MultiBoxLoss_combined
    import data as cfgs
    net = bn(types.SimpleNamespace(method='ours', phase=phase, setting=setting), size, num_fg)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()))
    net = net.to(dev).train()
    net.device = dev
    priors = PriorBox(getattr(cfgs, 'VOC_%d' % size)).forward().to(dev)
    nout = num_fg if phase == 1 else net.OBJ_Target.weight.shape[0] + (num_fg if setting == 'incre' else 0)
    crit = MultiBoxLoss_combined(nout + 1, 0.5, True, 0, True, 3, 0.5, False)
    crit.sync_normalizer = world > 1
    opt = torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4)
    x = synth.images(batch, size, 'randn', 1234 + rank).to(dev)
    tg = [t.to(dev) for t in synth.targets(batch, nout + 1, 99 + rank)]
    trt = net.train_runtime(batch)
    bucketer = trt.enable_grad_sync() if world > 1 else None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def timed(n, split):
        tf = tl = tb = 0.0
        cdist.barrier(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            ev[0].record()
            out = net(x)
            ev[1].record()
            loss = sum(crit(out, priors, tg).values())
            ev[2].record()
            loss.backward()
            ev[3].record()
            opt.step()
            if split:
                torch.cuda.synchronize(dev)
                tf += ev[0].elapsed_time(ev[1])
                tl += ev[1].elapsed_time(ev[2])
                tb += ev[2].elapsed_time(ev[3])
        cdist.barrier(dev)
        return (time.perf_counter() - t0) / n, tf / n, tl / n, tb / n, float(loss)
    timed(warmup, False)
    dt, _, _, _, loss = timed(steps, False)              # the timed K steps: no host synchronisation inside
    if after_timed is not None:
        after_timed(net, loss)
    _, tf, tl, tb, _ = timed(max(2, steps // 2), True)   # stage split from HIP events, one sync per step
    res = {'ms_per_step': dt * 1e3, 'fwd_ms': tf, 'loss_ms': tl, 'bwd_ms': tb, 'loss': loss, 'batch': batch,
           'grad_bytes': int(trt.arena.numel()) * 4}
    if world > 1:
        trt.bucketer = None                              # the same step with every rank keeping its own gradients
        timed(1, False)
        res['ms_per_step_no_allreduce'] = timed(steps, False)[0] * 1e3
        trt.bucketer = bucketer
        spans = bucketer.bucket_span
        cdist.barrier(dev)
        t0 = time.perf_counter()
        reps = 5
        for _ in range(reps):
            hs = [tdist.all_reduce(bucketer.flat[a:b], async_op=True) for a, b in spans]
            for h in hs:
                h.wait()
            torch.cuda.synchronize(dev)
        cdist.barrier(dev)
        res['allreduce_ms_alone'] = (time.perf_counter() - t0) / reps * 1e3
        res['buckets'] = len(spans)
        res['bucket_bytes'] = max(b - a_ for a_, b in spans) * 4
    del net, trt, opt, x, tg
    torch.cuda.empty_cache()
    return res


XGMI_LINK_GBS = 153.0        # one xGMI link, one direction (MI355X_MICROARCH.md: 7 links x ~153 GB/s per GPU)


def allreduce_model(grad_bytes, bucket_bytes, world):
    """What the gradient all-reduce of a step should cost on an 8-GPU MI355X node, so that the first run on one can be read against a
    prediction: a ring all-reduce moves 2 (N - 1) / N of the buffer through every GPU; xGMI is point-to-point, so one ring is
    bound by ONE link per hop (153 GB/s), and RCCL can run up to seven rings (one per link) -- the two bounds below, per bucket and
    per step, at an assumed 70 % of link rate."""
    n = max(2, int(world))
    moved = 2.0 * (n - 1) / n
    eff = 0.7
    def ms(nbytes, links):
        return round(moved * nbytes / (links * XGMI_LINK_GBS * 1e9 * eff) * 1e3, 3)
    return {'ranks': n, 'bytes_through_each_gpu': int(moved * grad_bytes),
            'ms_per_step_one_ring': ms(grad_bytes, 1), 'ms_per_step_seven_rings': ms(grad_bytes, 7),
            'ms_per_bucket_one_ring': ms(bucket_bytes, 1), 'ms_per_bucket_seven_rings': ms(bucket_bytes, 7),
            'assumptions': 'ring all-reduce, xGMI %.0f GB/s per link and direction, %.0f %% of it achieved; one ring = one link per '
                           'hop, seven rings = every link of the fully connected node' % (XGMI_LINK_GBS, eff * 100)}


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def self_launch(a):
    """`python bench.py --gpus N` outside torchrun: start the N ranks ourselves (one per GPU, RCCL) and relay the
    JSON line.  Never degrades to fewer ranks: refuses N > visible GPUs unless --share-devices was asked for."""
    ndev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if ndev == 0:
        raise SystemExit('bench.py needs a HIP device (the product has no CPU path)')
    if a.gpus > ndev and not a.share_devices:
        raise SystemExit('bench.py --gpus %d: only %d HIP device(s) visible on this node -- refusing to report a '
                         'smaller run as %d GPUs (use --share-devices to REHEARSE the %d-rank path on %d device(s) '
                         'over gloo; such a line is marked devices_shared)' % (a.gpus, ndev, a.gpus, a.gpus, ndev))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(a.gpus),
           '--master-addr', '127.0.0.1', '--master-port', str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')       # dmabuf IPC: RCCL needs it on this driver
    env.setdefault('OMP_NUM_THREADS', '4')
    env['CTDET_BENCH_SELF_LAUNCHED'] = '1'
    rc = subprocess.call(cmd, env=env)
    raise SystemExit(rc)


def main():
    import faulthandler
    faulthandler.enable()
    if os.environ.get('CTDET_BENCH_WATCHDOG'):
        faulthandler.dump_traceback_later(int(os.environ['CTDET_BENCH_WATCHDOG']), exit=False)
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=None, help='default 20 (inference) / 5 (--train)')
    ap.add_argument('--warmup', type=int, default=None, help='default 5 (inference) / 2 (--train)')
    ap.add_argument('--train', action='store_true',
                    help='time the data-parallel TRAINING step (BASELINE configs[3]; default RFBNet-512 + '
                         'Context-Transformer phase 2, 60 classes, bs 8 per GPU) instead of forward + NMS')
    ap.add_argument('--size', type=int, default=None)
    ap.add_argument('--batch', type=int, default=None, help='images per GPU (weak scaling) / per job (strong scaling)')
    ap.add_argument('--classes', type=int, default=None)
    ap.add_argument('--phase', type=int, default=None)
    ap.add_argument('--setting', default='transfer')
    ap.add_argument('--scaling', default=os.environ.get('CTDET_BENCH_SCALING', 'weak'), choices=['weak', 'strong'],
                    help='strong: ONE batch of --batch images split over the ranks (train.py:296-297 DataParallel scatter)')
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'],
                    help="bf16: NHWC bf16 activations + bf16 MFMA convolutions (BASELINE configs[4]); NOT the "
                         "headline metric, which is fp32")
    ap.add_argument('--share-devices', action='store_true',
                    help='allow more ranks than GPUs (rehearsal of the N-rank path on a smaller box; gloo, since RCCL '
                         'refuses two ranks on one device); the line is marked devices_shared')
    ap.add_argument('--full', action='store_true',
                    help='also measure what the headline does not need (N=1 inference): conv roofline and stage rooflines '
                         '(extra eager passes), the other configurations, the CPU baseline')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the outputs of the last timed step to DIR/<name>.npy (see the module docstring)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: leave out the CPU baseline')
    ap.add_argument('--no-roofline', action='store_true', help='with --full: leave out the roofline passes')
    ap.add_argument('--no-other-configs', action='store_true', help='with --full: leave out the other configurations')
    a = ap.parse_args()
    if (a.steps is not None and a.steps < 1) or (a.warmup is not None and a.warmup < 0):
        raise SystemExit('bench.py: --steps must be >= 1 and --warmup >= 0')
    dflt = (512, 8, 60, 2, 5, 2) if a.train else (300, 32, 20, 1, 20, 5)
    explicit_workload = any(v is not None for v in (a.size, a.batch, a.classes, a.phase))
    for name, v in zip(('size', 'batch', 'classes', 'phase', 'steps', 'warmup'), dflt):
        if getattr(a, name) is None:
            setattr(a, name, v)

    from ctdet import dist as cdist
    rank, local, world = cdist.env_world()
    if 'WORLD_SIZE' not in os.environ and a.gpus > 1:
        self_launch(a)                      # does not return
    if world != a.gpus:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d: refusing to report a %d-rank run as %d GPUs'
                         % (a.gpus, world, world, a.gpus))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a HIP device (the product has no CPU path)')
    ndev = torch.cuda.device_count()
    shared = world > ndev
    if shared and not a.share_devices:
        raise SystemExit('%d ranks but %d HIP device(s): refusing to share devices without --share-devices' % (world, ndev))
    local = local % ndev
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    # RCCL (backend 'nccl').  Inference uses it only for the timing barrier / max-over-ranks; --train all-reduces the
    # gradients through it.  RCCL refuses two ranks on one device, so a --share-devices rehearsal uses gloo.
    backend = os.environ.get('CTDET_DIST_BACKEND') or ('gloo' if shared else 'nccl')
    cdist.init(backend)
    ranks_info = [{'rank': rank, 'device': local, 'pci_bus_id': getattr(torch.cuda.get_device_properties(local), 'pci_bus_id', None),
                   'name': torch.cuda.get_device_name(local)}]
    if world > 1:
        import torch.distributed as tdist
        if tdist.get_world_size() != a.gpus:
            raise SystemExit('process group has %d ranks, --gpus %d' % (tdist.get_world_size(), a.gpus))
        probe = torch.ones(1, device=dev)
        tdist.all_reduce(probe)             # every rank must answer through the data-path backend before anything is timed
        if int(probe.item()) != a.gpus:
            raise SystemExit('all-reduce over the process group saw %d ranks, --gpus %d' % (int(probe.item()), a.gpus))
        gathered = [None] * world
        tdist.all_gather_object(gathered, ranks_info[0])
        ranks_info = gathered
        if not shared and len({(r['device'], r['pci_bus_id']) for r in ranks_info}) != world:
            raise SystemExit('ranks do not sit on %d distinct devices: %r' % (world, ranks_info))

    from ctdet import synth
    num_fg = a.classes
    if a.scaling == 'strong':
        b0, b1 = cdist.shard(a.batch, rank, world)       # contiguous image shard of the one global batch
        batch, global_batch = b1 - b0, a.batch
        if batch == 0:
            raise SystemExit('--scaling strong: batch %d cannot be split over %d ranks' % (a.batch, world))
    else:
        batch, global_batch = a.batch, a.batch * world

    def per_rank(value):
        """value of every rank, in rank order (python floats)."""
        if world == 1:
            return [value]
        import torch.distributed as tdist
        out = [None] * world
        tdist.all_gather_object(out, value)
        return out

    dist_info = {'backend': backend if world > 1 else None,
                 'rccl_ranks': world if (world > 1 and backend == 'nccl') else (1 if world == 1 else 0),
                 'devices_shared': shared, 'self_launched': os.environ.get('CTDET_BENCH_SELF_LAUNCHED') == '1',
                 'ranks': ranks_info}

    if a.train:
        log('training step: building net + training runtime')

        def dump_train(net, loss):
            params = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
            dump_outputs(a.dump_outputs, [('loss', torch.tensor([loss], dtype=torch.float64), 1), ('parameters', params, 1 << 20)])
        r = train_config(a.size, num_fg, a.phase, a.setting, batch, dev, a.steps, a.warmup, rank, world,
                         after_timed=dump_train if a.dump_outputs and rank == 0 else None)
        dt = cdist.max_over_ranks(r['ms_per_step'] * 1e-3, dev)
        ms_rank = per_rank(round(r['ms_per_step'], 3))
        if rank == 0:
            line = {
                'metric': 'images/sec training step (fwd + loss + bwd + grad all-reduce + SGD)',
                'value': round(global_batch / dt, 2), 'unit': 'images/s', 'n_gpus': world, 'steps': a.steps,
                'warmup': a.warmup, 'ms_per_step': round(dt * 1e3, 3), 'higher_is_better': True, 'scaling': a.scaling,
                'launch_mode': 'eager launches', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
                'config': {'workload': 'RFBNet-%d VGG16 TRAINING step, bs=%d per GPU, %d fg classes, phase %d%s: forward '
                                       '(batch-stat BN) + MultiBoxLoss_combined + HIP backward + bucketed gradient '
                                       'all-reduce + SGD; name-seeded random weights, randn images, synthetic targets'
                                       % (a.size, batch, num_fg, a.phase, ' ' + a.setting if a.phase == 2 else ''),
                           'global_batch': global_batch,
                           'parallelism': 'dp%d (image shards, gradient all-reduce in 32 MiB buckets from inside the '
                                          'backward pass, %s scaling)' % (world, a.scaling)},
                'stages_ms': {'forward': round(r['fwd_ms'], 3), 'loss': round(r['loss_ms'], 3),
                              'backward_incl_allreduce': round(r['bwd_ms'], 3)},
                'loss': round(r['loss'], 5), 'grad_bytes': r['grad_bytes'],
                'per_rank_ms_per_step': ms_rank, 'dist': dist_info,
                # the prediction for the 8-GPU node this step is meant for (32 MiB buckets, ctdet.dist.GradBucketer)
                'allreduce_model_8gpu': allreduce_model(r['grad_bytes'], r.get('bucket_bytes', 32 << 20), 8),
            }
            if world > 1:
                t_with, t_wo, t_ar = r['ms_per_step'], r['ms_per_step_no_allreduce'], r['allreduce_ms_alone']
                line['allreduce'] = {
                    'ms_alone': round(t_ar, 3), 'buckets': r['buckets'], 'bucket_MiB': round(r['bucket_bytes'] / 2 ** 20, 2),
                    'algbw_GBs': round(r['grad_bytes'] / t_ar / 1e6, 1),
                    'busbw_GBs': round(r['grad_bytes'] / t_ar / 1e6 * 2 * (world - 1) / world, 1),
                    'step_ms_without_allreduce': round(t_wo, 3), 'exposed_ms': round(max(0.0, t_with - t_wo), 3),
                    'overlap_frac': round(min(1.0, max(0.0, 1.0 - (t_with - t_wo) / t_ar)), 3) if t_ar > 0 else None,
                    'note': 'rank 0 timings; alone = the same buckets all-reduced back to back on the idle GPUs'}
            print(json.dumps(line))
        if world > 1:
            import torch.distributed as tdist
            tdist.destroy_process_group()
        return

    log('building net + pipeline (plan, weight packing%s)' % (', conv autotune' if os.environ.get('CTDET_TUNE', '1') != '0' else ''))
    pipe = make_pipeline(a.size, num_fg, a.phase, a.setting, batch, a.dtype, dev)
    x = synth.images(global_batch if a.scaling == 'strong' else batch, a.size, 'randn', 1234 + (0 if a.scaling == 'strong' else rank))
    if a.scaling == 'strong':
        x = x[b0:b1]
    x = x.to(dev)

    def sync():
        cdist.barrier(dev)

    log('warm-up')
    for _ in range(a.warmup):
        pipe.run(x)
    torch.cuda.synchronize(dev)
    log('timed region')
    want_roof = a.full and not a.no_roofline and rank == 0 and world == 1      # N > 1 runs only report throughput
    graph_mode = bool(pipe.use_graph)
    if want_roof and not graph_mode:
        pipe.rt.event_log = []          # HIP events around every conv launch of the timed region
    sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        pipe.run(x)
    torch.cuda.synchronize(dev)
    dt_local = time.perf_counter() - t0
    sync()
    dt = time.perf_counter() - t0
    dt = cdist.max_over_ranks(dt, dev)
    ms_rank = per_rank(round(dt_local / a.steps * 1e3, 3))

    log('timed region done: %.2f ms/step' % (dt / a.steps * 1e3))
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, inference_outputs(pipe))
    graph_mode = pipe._graph is not None            # False if the capture failed and the steps were launched eagerly
    workload = {'size': a.size, 'batch': batch, 'phase': a.phase, 'classes': a.classes}
    roof = None
    events_from = 'the timed region'
    if want_roof and graph_mode:
        # the timed region replays a hipGraph, inside which no per-launch events can be recorded: the same K steps
        # again as eager launches with the events around every conv launch
        log('event pass (eager launches of the same steps)')
        pipe.rt.event_log = []
        for _ in range(a.steps):
            pipe.run(x)
        torch.cuda.synchronize(dev)
        events_from = 'an eager pass of the same %d steps right after the timed region (the timed region replays a ' \
                      'hipGraph)' % a.steps
    if pipe.rt.event_log:
        pmc = load_pmc(workload)
        roof = conv_roofline(pipe.rt, batch, pmc)
        ev_log, pipe.rt.event_log = pipe.rt.event_log, None
        log('stage rooflines (library profile scopes, 5 extra steps)')
        stages = stage_rooflines(pipe, x, 5, pmc)
        g = stages.get('wino4s_gemm')
        if roof['kernel'].startswith('wino4s') and g:
            # a three-kernel launch group leads by launch time; the line names ONE kernel, so the group's matrix kernel
            # competes with the single-kernel groups on its own time (rocprofv3 --stats ranks them the same way)
            gemm_ms = g['avg_launch_us'] * g['launches_per_step'] * 1e-3
            single = [(k, v['ms_per_step']) for k, v in roof['by_kernel'].items() if not k.startswith('wino4s')]
            if single and max(single, key=lambda kv: kv[1])[1] > gemm_ms:
                best = max(single, key=lambda kv: kv[1])
                pipe.rt.event_log = ev_log
                lead = {k: roof[k] for k in ('kernel', 'launches', 'avg_launch_us', 'achieved', 'frac')}
                roof = conv_roofline(pipe.rt, batch, pmc, pick=best[0])
                pipe.rt.event_log = None
                roof['dominant_selection'] = {
                    'rule': 'kernel with the most accumulated time of its own per step',
                    'this_kernel_ms_per_step': best[1], 'wino4s_gemm_ms_per_step': round(gemm_ms, 3),
                    'leading_launch_group': lead,
                    'note': 'the wino4s launch group (in + gemm + out, three kernels) has more launch time in total; none of '
                            'its kernels alone has more than this one (stages.wino4s_* have their rooflines)'}
        roof['events_from'] = events_from
        roof['stages'] = stages
        if roof['kernel'].startswith('wino4s') and g:
            # the dominant conv launch is a three-kernel one: the line's kernel-level fields describe its matrix kernel
            # (HIP events of the library's profile scopes on the launch stream, 5 eager steps), the launch-level numbers
            # (transform kernels included) stay in `dominant_launch`
            roof['dominant_launch'] = {k: roof[k] for k in ('kernel', 'launches', 'avg_launch_us', 'achieved', 'frac',
                                                            'flops_per_launch', 'flops_definition')}
            roof.update({'kernel': 'wino4s_gemm', 'bound': 'mfma', 'achieved': g['achieved'], 'peak': g['peak'],
                         'frac': g['frac'], 'traffic': g['traffic'], 'avg_launch_us': g['avg_launch_us'],
                         'launches': int(round(g['launches_per_step'] * 5)), 'flops_per_launch': g['algorithmic_per_launch'],
                         'flops_definition': 'USEFUL multiply-adds x2 on the 16-bit matrix pipe per launch: 36 transform points x the '
                                             'layer\'s tiles x cin x cout x the piece products of its operand form (f16x2: 3, bf16x3: 6), '
                                             'averaged over the layers that run this kernel; the padding of tiles and couts to 128 is '
                                             'not counted (stages.wino4s_gemm.executed_incl_padding_frac has it)',
                         'measured_sustained_peak': SUSTAINED_PEAK})
        roof['traffic_source'] = sorted({v[1] for v in pmc.values()}) or None
    counts = int(pipe.post.out_count.sum().item())
    def kind(st):
        w = int(st.rt.get('wino') or 0)
        if w:
            return 'winograd_h2' if w in WINOGRAD_H2 else 'winograd_x3' if w in WINOGRAD_X3 else 'winograd'
        if st.rt.get('x3') is not None:
            return 'h2' if pipe.rt.backend.x3_h2(st.rt['x3']) else 'bf16x3'
        cfg = st.rt['desc'].config
        name = _lib_config_name(cfg)
        return 'valu' if name == 'valu' or (cfg == 0 and st.cin == 3 and (st.kh, st.kw) == (3, 3)) else 'fp32_mfma'
    kinds = [kind(st) for st in pipe.rt.conv_steps()] if a.dtype != 'bf16' else []
    arith = ('bf16 MFMA, fp32 accumulate' if a.dtype == 'bf16' else
             'fp32 results: %d launches Winograd F(4x4,3x3) + %d launches direct on the f16x2 operand form (every fp32 operand = two '
             'binary16 pieces hi = rne16(x 2^e), lo = rne16(x 2^e - hi) with a per-image / per-layer power-of-two scale 2^e from the '
             'operand\'s maximum; three piece products on the f16 MFMA, fp32 accumulate; 22-24 significant bits per product like '
             'bf16x3\'s six, whole-network error vs fp64 below the fp32 CPU path\'s: profiles/r06_wino_accuracy.txt, per-layer gates '
             'tests/test_gpu_wino.py / tests/test_gpu_x3.py), %d + %d launches Winograd / direct on bf16x3 (three exact bfloat16 '
             'pieces, six products on the bf16 MFMA), %d launches Winograd on the fp32 MFMA, %d launches fp32 MFMA direct, %d '
             'launches fp32 vector ALU (the 3-channel image layer)'
             % (kinds.count('winograd_h2'), kinds.count('h2'), kinds.count('winograd_x3'), kinds.count('bf16x3'),
                kinds.count('winograd'), kinds.count('fp32_mfma'), kinds.count('valu')))
    conv_gflop = round(pipe.rt.plan.conv_flops() / batch / 1e9, 2)
    tuned = bool(pipe.rt.tuned)
    live_tuned = list(getattr(pipe.rt, 'live_tuned', []))
    operand_form = 'f16x2' if getattr(pipe.rt.backend, 'h2', False) else 'bf16x3'
    policy = pipe.rt.policy_record()
    if live_tuned and not explicit_workload and a.dtype == 'f32' and os.environ.get('CTDET_BENCH_ALLOW_LIVE_TUNE') != '1':
        # the tests pin CTDET_TUNE=0 and therefore only ever see table tiles: a headline must not run tiles chosen by a live timing
        raise SystemExit('bench.py: %d conv shape(s) of the headline workload are not in the committed tile table (%s ...): add them '
                         '(tools/tune_convs.py) with a parity test at that shape, or set CTDET_BENCH_ALLOW_LIVE_TUNE=1'
                         % (len(live_tuned), ', '.join(live_tuned[:3])))
    other = None
    if a.full and rank == 0 and world == 1 and not a.no_other_configs and a.dtype == 'f32' and not explicit_workload:
        del pipe
        torch.cuda.empty_cache()
        other = {}
        for key, cfg in (('rfb512_bs32', (512, 20, 1, 'transfer', 32)),
                         ('rfb300_ctx_bs32', (300, 60, 2, 'transfer', 32)),
                         ('rfb512_ctx_bs32', (512, 60, 2, 'transfer', 32)),
                         ('rfb300_bs4_strong_shard', (300, 20, 1, 'transfer', 4))):
            log('other config %s' % key)
            other[key] = quick_config(*cfg, 'f32', dev, steps=20 if cfg[4] == 4 else 5)
        for key in ('rfb300_ctx_bs32', 'rfb512_ctx_bs32'):
            other[key]['note'] = ('randn images; parity of the Context-Transformer block is claimed for randn inputs only (flat 1e-4 against '
                                  'the fp32 CPU path, tests/test_gpu_ctx_parity.py): on image-like u8 inputs (SURVEY 8d ii, |x| ~ 128) the '
                                  'un-scaled theta.phi^T logits make the block chaotic in fp32 -- the CPU path itself is 1e-3 .. 1e-1 '
                                  'from fp64 there -- and the tests hold the block\'s INPUT to 1e-4 instead'
                                  + ('; 512 + Context-Transformer is build-defined (the reference raises IndexError): parity unpinned'
                                     if key.startswith('rfb512') else ''))
        other['rfb300_bs4_strong_shard']['note'] = \
            'the per-GPU shard when ONE bs-32 batch is split over 8 GPUs (--scaling strong); no collective on the path'
        # BASELINE configs[4]: RFBNet-512 bf16 MFMA convs + fp32 NMS, bs 128 over 8 GPUs = bs 16 per GPU
        log('other config bf16_rfb512_bs16')
        other['bf16_rfb512_bs16'] = quick_config(512, 20, 1, 'transfer', 16, 'bf16', dev, steps=5, roofline=True)
        other['bf16_rfb512_bs16']['note'] = 'per-GPU shape of BASELINE configs[4] (bs 128 over 8 GPUs); NHWC bf16 ' \
                                            'activations, bf16 MFMA convs, fp32 softmax / decode / NMS'
        # BASELINE configs[3]: the training step; its per-GPU shape (512 + Context-Transformer, bs 64 over 8 GPUs) and
        # the RFBNet-300 bs-32 step
        for key, cfg in (('train_rfb300_bs32', (300, 20, 1, 'transfer', 32)),
                         ('train_rfb512ctx_bs8', (512, 60, 2, 'transfer', 8))):
            log('other config %s' % key)
            r = train_config(*cfg, dev, steps=4, warmup=2)
            other[key] = {'ms_per_step': round(r['ms_per_step'], 3), 'images_per_s': round(cfg[4] / r['ms_per_step'] * 1e3, 1),
                          'batch': cfg[4], 'steps': 4,
                          'stages_ms': {'forward': round(r['fwd_ms'], 3), 'loss': round(r['loss_ms'], 3),
                                        'backward': round(r['bwd_ms'], 3)},
                          'grad_bytes': r['grad_bytes'],
                          'step': 'forward (batch-stat BN) + MultiBoxLoss_combined + HIP backward + SGD, one GPU '
                                  '(no all-reduce); `bench.py --train --gpus N` times the data-parallel form'}
    cpu = None
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        log('cpu baseline (oracle on host cores)')
        cpu = cpu_baseline(a.size, num_fg)
        log('cpu baseline done')

    if rank == 0:
        total_images = global_batch * a.steps
        line = {
            'metric': 'images/sec fwd+NMS', 'value': round(total_images / dt, 2), 'unit': 'images/s',
            'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup,
            'ms_per_step': round(dt / a.steps * 1e3, 3), 'higher_is_better': True, 'scaling': a.scaling,
            'launch_mode': 'hipGraph replay' if graph_mode else 'eager launches',
            'vs_baseline': None, 'dtype': a.dtype, 'data': 'synthetic',
            'arith': arith,
            'config': {'workload': 'RFBNet-%d VGG16 inference, bs=%d per GPU, %d fg classes, phase %d%s: '
                                   'fwd + softmax/decode + per-class NMS(0.45) + top-200; name-seeded random '
                                   'weights, randn images' % (a.size, batch, num_fg, a.phase,
                                                              ' ' + a.setting if a.phase == 2 else ''),
                       'global_batch': global_batch,
                       'parallelism': 'dp%d (image shards, no collective, %s scaling)' % (world, a.scaling),
                       'conv_gflop_per_image': conv_gflop,
                       'detections_per_batch': counts, 'conv_autotuned': tuned,
                       # shapes whose tile came from a live timing instead of the committed table (0 for a headline run: refused above)
                       'live_tuned_layers': {'count': len(live_tuned), 'keys': live_tuned[:16]},
                       'operand_form': operand_form,
                       # every kernel-choice switch in force (engine.Runtime.policy_record)
                       'policy': policy},
            'per_rank_ms_per_step': ms_rank, 'dist': dist_info,
            'roofline': roof, 'cpu_baseline': cpu, 'other_configs': other,
        }
        print(json.dumps(line))
    if world > 1:
        import torch.distributed as tdist
        tdist.destroy_process_group()


if __name__ == '__main__':
    main()
