#!/usr/bin/env python3
"""ct_conv2d_wgrad (fp32 MFMA, atomics, needs a zeroed dw) against ct_conv2d_wgrad_h2 (f16x2, slabs, deterministic) on every
distinct 1x1 layer shape of RFBNet-300 bs 32 and of RFBNet-512 + Context-Transformer bs 8.

    python tools/wgrad_h2_probe.py [--iters 30] > profiles/wgrad_h2_probe.txt

Per shape: HIP-event medians of --iters launches of
  old_us        hipMemsetAsync(dw) + ct_conv2d_wgrad
  h2_us         ct_conv2d_wgrad_h2 with both maxima given
  h2_null_us    ct_conv2d_wgrad_h2 with both maxima NULL (its own ct_absmax_f32 passes included)
and rel_err of each result against a float64 evaluation (max |a - b| / max |b|, the suite's measure) plus the Frobenius error
pair err_old / err_h2 the full-size test compares.  `step_us` sums each column over the layers of the step (shape count x time).
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

NETS = {'rfb300_bs32': (300, 1, 32), 'rfb512_ctx_bs8': (512, 2, 8)}


def shapes(size, phase, batch):
    from ctdet import engine
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=phase, setting='transfer'), size, 20).eval()
    plan = engine.Plan(net, batch)
    return sorted(Counter((st.cin, st.cout, st.h, st.w, st.stride) for st in plan.steps
                          if st.kind == 'conv' and (st.kh, st.kw) == (1, 1)).items())


def run_net(tag, iters):
    import torch
    from ctdet import _lib
    lib = _lib.lib()
    size, phase, B = NETS[tag]
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

    rows = []
    for (cin, cout, h, w, stride), count in shapes(size, phase, B):
        g = torch.Generator().manual_seed(cin + cout + h)
        oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
        x = torch.randn(B, cin, h, w, generator=g).to(dev)
        dz = torch.randn(B, cout, oh, ow, generator=g).to(dev)
        d = _lib.ConvDesc()
        d.in_ = x.data_ptr()
        d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = B, cin, h, w, cin, 0
        d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil, d.oh, d.ow = cout, 1, 1, stride, 0, 0, 1, oh, ow
        assert lib.ct_conv_wgrad_h2_supported(C.byref(d)) == 1
        need = lib.ct_conv_wgrad_h2_workspace_bytes(C.byref(d))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        xl = torch.zeros(B * line, dtype=torch.int32, device=dev)
        zl = torch.zeros(B * line, dtype=torch.int32, device=dev)
        _lib.check(lib.ct_absmax_f32(x.data_ptr(), B, cin * h * w, cin * h * w, xl.data_ptr(), stream()), 'absmax')
        _lib.check(lib.ct_absmax_f32(dz.data_ptr(), B, cout * oh * ow, cout * oh * ow, zl.data_ptr(), stream()), 'absmax')
        dw_old, dw_h2, dw_null = (torch.empty(cout, cin, device=dev) for _ in range(3))

        def old():
            dw_old.zero_()
            _lib.check(lib.ct_conv2d_wgrad(C.byref(d), dz.data_ptr(), cout, 0, dw_old.data_ptr(), stream()), 'wgrad')

        def h2(lines_x, lines_z, out):
            d.in_absmax = lines_x
            _lib.check(lib.ct_conv2d_wgrad_h2(C.byref(d), dz.data_ptr(), cout, 0, lines_z, out.data_ptr(), ws.data_ptr(), need,
                                              stream()), 'wgrad_h2')
            d.in_absmax = None
        t_old = median_us(old)
        t_h2 = median_us(lambda: h2(xl.data_ptr(), zl.data_ptr(), dw_h2))
        t_null = median_us(lambda: h2(None, None, dw_null))
        ref = torch.einsum('bop,bip->oi', dz.reshape(B, cout, -1).double(),
                           x[:, :, ::stride, ::stride].reshape(B, cin, -1).double())

        def errs(a):
            a = a.double()
            return float((a - ref).abs().max() / ref.abs().max()), float((a - ref).norm() / ref.norm())
        (r_old, f_old), (r_h2, f_h2), (r_null, _) = errs(dw_old), errs(dw_h2), errs(dw_null)
        rows.append({'cin': cin, 'cout': cout, 'h': h, 'w': w, 'stride': stride, 'batch': B, 'layers': count,
                     'old_us': round(t_old, 1), 'h2_us': round(t_h2, 1), 'h2_null_us': round(t_null, 1),
                     'rel_err_old': r_old, 'rel_err_h2': r_h2, 'rel_err_h2_null': r_null, 'err_old': f_old, 'err_h2': f_h2})
        del x, dz, ws, ref
    step = {k: round(sum(r[k] * r['layers'] for r in rows), 1) for k in ('old_us', 'h2_us', 'h2_null_us')}
    print(json.dumps({'net': tag, 'device': torch.cuda.get_device_name(0), 'rows': rows, 'step_us': step}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--net', choices=sorted(NETS), help='(child mode) one network, one JSON line')
    ap.add_argument('--timeout', type=int, default=420, help='seconds per network')
    a = ap.parse_args()
    if a.net:
        run_net(a.net, a.iters)
        return 0
    out = {'probe': 'wgrad_h2', 'iters': a.iters, 'nets': []}
    for tag in ('rfb300_bs32', 'rfb512_ctx_bs8'):
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
