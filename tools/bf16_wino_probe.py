#!/usr/bin/env python3
"""ct_conv2d_bf16_fwd (direct bf16 MFMA kernel) against ct_conv2d_bf16_wino_fwd (Winograd F(4x4,3x3), binary16 operands in the
transform domain, csrc/ct_wino_bf16.hip) on every distinct 3x3 / stride 1 / dilation 1 layer shape with a plain bf16 output of
RFBNet-300 bs 32 and of RFBNet-512 bs 16 (the shapes ct_conv_bf16_wino_supported accepts).

    python tools/bf16_wino_probe.py [--iters 20] > profiles/bf16_wino_probe.txt

Per shape, on post-ReLU random activations and He-scaled weights:
  direct_us, wino_us      HIP-event medians of --iters launches (the route with in_absmax given, as between two routed layers)
  wino_null_us            the route with in_absmax NULL (its own ct_absmax_bf16_nhwc pass included)
  in_us, gemm_us, out_us  device time of the three kernels of the route (ct_profile_enable, medians)
  err_direct, err_wino    max |y - E| / max |E| on a 64 x 64 corner of image 0 and the first 64 output channels, E = the float64
                          convolution of the same bf16 activations with the unrounded fp32 weights
`step_us` sums direct_us, wino_us and min(direct, wino) over the layers of the step (shape count x time); `min_cin_rule` is the
smallest cin from which the route wins on EVERY shape of the network at or above it.
Each network runs in a child process of its own under `timeout -k 10`; the second one starts only if the first one succeeded.
Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import types
from collections import Counter

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)

NETS = {'rfb300_bs32': (300, 32), 'rfb512_bs16': (512, 16)}


def shapes(size, batch):
    from ctdet import engine
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), size, 20).eval()
    plan = engine.Plan(net, batch)
    return sorted(Counter((st.cin, st.cout, st.h, st.w) for st in plan.steps
                          if st.kind == 'conv' and (st.kh, st.kw, st.stride, st.dil, st.ph, st.pw) == (3, 3, 1, 1, 1, 1)
                          and not st.segs and st.res is None and st.cin % 8 == 0 and st.cin >= 16
                          and len({p.relu for p in st.parts}) == 1).items())


def run_net(tag, iters):
    import torch
    import torch.nn.functional as F
    from ctdet import _lib
    lib = _lib.lib()
    size, B = NETS[tag]
    dev = 'cuda:0'
    line = _lib.ABSMAX_LINE_BYTES // 4

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def median_us(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ts)

    def kernel_us(fn):
        _lib.check(lib.ct_profile_enable(1), 'profile')
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        recs = (_lib.ProfileRecord * (8 * iters))()
        n = C.c_int(0)
        _lib.check(lib.ct_profile_collect(recs, len(recs), C.byref(n)), 'collect')
        _lib.check(lib.ct_profile_enable(0), 'profile')
        by = {}
        for r in recs[:min(n.value, len(recs))]:
            by.setdefault(r.name.decode(), []).append(r.ms * 1e3)
        return {k: statistics.median(v) for k, v in by.items()}

    rows = []
    for (cin, cout, h, w), count in shapes(size, B):
        g = torch.Generator().manual_seed(cin + cout + h)
        x = torch.randn(B, h, w, cin, generator=g).relu_().bfloat16()
        wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
        xb, wd = x.to(dev), wt.to(dev)
        scale, shift = torch.ones(lib.ct_conv_mpad(cout), device=dev), torch.zeros(lib.ct_conv_mpad(cout), device=dev)
        ptrs, couts = (C.c_void_p * 1)(wd.data_ptr()), (C.c_int * 1)(cout)
        wp = torch.empty(lib.ct_conv_bf16_packed_elems(cin, cout, 3, 3), dtype=torch.int16, device=dev)
        _lib.check(lib.ct_conv_pack_weights_bf16(ptrs, couts, 1, cin, 3, 3, wp.data_ptr(), stream()), 'pack')
        up = torch.empty(lib.ct_conv_bf16_wino_packed_bytes(cin, cout), dtype=torch.uint8, device=dev)
        _lib.check(lib.ct_conv_pack_weights_bf16_wino(ptrs, couts, 1, cin, up.data_ptr(), stream()), 'pack wino')
        y_d = torch.zeros(B, h, w, cout, dtype=torch.bfloat16, device=dev)
        y_w = torch.zeros(B, h, w, cout, dtype=torch.bfloat16, device=dev)

        def desc(wpacked, out):
            d = _lib.ConvDesc()
            d.in_ = xb.data_ptr()
            d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = B, cin, h, w, cin, 0
            d.wpacked, d.scale, d.shift = wpacked.data_ptr(), scale.data_ptr(), shift.data_ptr()
            d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil, d.oh, d.ow = cout, 3, 3, 1, 1, 1, 1, h, w
            d.out, d.out_ctot, d.out_coff, d.relu = out.data_ptr(), cout, 0, 1
            return d
        dd, dw = desc(wp, y_d), desc(up, y_w)
        ksws = None
        if cout * B * h * w <= (2 << 20):               # the engine's split-K rule for the small maps
            ksws = torch.empty(16 * cout * B * h * w, device=dev)
            dd.ksplit, dd.ksplit_ws, dd.ksplit_ws_floats = -1, ksws.data_ptr(), ksws.numel()
        assert lib.ct_conv_bf16_wino_supported(C.byref(dw)) == 1
        need = lib.ct_conv_bf16_wino_workspace_bytes(C.byref(dw))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        lines = torch.zeros(B * line, dtype=torch.int32, device=dev)
        _lib.check(lib.ct_absmax_bf16_nhwc(xb.data_ptr(), B, h * w, cin, 0, cin, lines.data_ptr(), stream()), 'absmax')

        def direct():
            _lib.check(lib.ct_conv2d_bf16_fwd(C.byref(dd), stream()), 'direct')

        def wino(given):
            dw.in_absmax = lines.data_ptr() if given else None
            _lib.check(lib.ct_conv2d_bf16_wino_fwd(C.byref(dw), ws.data_ptr(), need, stream()), 'wino')
        t_d = median_us(direct)
        t_w = median_us(lambda: wino(True))
        t_n = median_us(lambda: wino(False))
        k = kernel_us(lambda: wino(True))
        # error on a corner of image 0: rows / columns 0 .. 63 need input rows / columns 0 .. 64
        ch, cw, cc = min(h, 64), min(w, 64), min(cout, 64)
        xc = x[0, :min(h, ch + 1), :min(w, cw + 1)].double().permute(2, 0, 1).unsqueeze(0)
        E = F.relu(F.conv2d(xc, wt[:cc].double(), None, 1, 1))[0, :, :ch, :cw]

        def err(y):
            got = y[0, :ch, :cw, :cc].double().permute(2, 0, 1).cpu()
            return float((got - E).abs().max() / E.abs().max())
        torch.cuda.synchronize()
        rows.append({'cin': cin, 'cout': cout, 'h': h, 'w': w, 'batch': B, 'layers': count,
                     'direct_us': round(t_d, 1), 'wino_us': round(t_w, 1), 'wino_null_us': round(t_n, 1),
                     'in_us': round(k.get('wbf_in', 0.0), 1), 'gemm_us': round(k.get('wbf_gemm', 0.0), 1),
                     'out_us': round(k.get('wbf_out', 0.0), 1), 'speedup': round(t_d / t_w, 3),
                     'err_direct': err(y_d), 'err_wino': err(y_w), 'workspace_mb': round(need / 2 ** 20, 1)})
        del xb, ws, y_d, y_w, ksws
        torch.cuda.empty_cache()
    step = {'direct_us': round(sum(r['direct_us'] * r['layers'] for r in rows), 1),
            'wino_us': round(sum(r['wino_us'] * r['layers'] for r in rows), 1),
            'best_us': round(sum(min(r['direct_us'], r['wino_us']) * r['layers'] for r in rows), 1)}
    rule = None
    for c in sorted({r['cin'] for r in rows}, reverse=True):
        if all(r['wino_us'] < r['direct_us'] for r in rows if r['cin'] >= c):
            rule = c
        else:
            break
    print(json.dumps({'net': tag, 'device': torch.cuda.get_device_name(0), 'rows': rows, 'step_us': step, 'min_cin_rule': rule}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--net', choices=sorted(NETS), help='(child mode) one network, one JSON line')
    ap.add_argument('--timeout', type=int, default=420, help='seconds per network')
    a = ap.parse_args()
    if a.net:
        run_net(a.net, a.iters)
        return 0
    out = {'probe': 'bf16_wino', 'iters': a.iters, 'nets': []}
    for tag in ('rfb300_bs32', 'rfb512_bs16'):
        r = subprocess.run(['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--net', tag,
                            '--iters', str(a.iters)], capture_output=True, text=True)
        if r.returncode != 0:           # nothing more is started on the device after a failure
            sys.stderr.write(r.stderr[-4000:])
            print(json.dumps(dict(out, failed=tag, returncode=r.returncode)))
            return 1
        out['nets'].append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
