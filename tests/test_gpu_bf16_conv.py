"""ct_conv2d_bf16_fwd, variant by variant and row by row (tests/conv_bf16_cases.py), against the float64 reference of the fused step
on bfloat16-rounded operands; then the kernels the path uses as plumbing (layout converters, weight packer, max-pool), bit for bit.

Every launch is built on the host: NHWC bf16 operands from torch.Tensor.bfloat16() (not from the device converters), weights packed
by ct_conv_pack_weights_bf16.  Poison: the input buffer holds the bf16 NaN pattern in every channel outside [coff, coff + cin) and
in one extra pixel row behind the last image.  That row is INSIDE the allocation and OUTSIDE in_bytes: the launcher derives the
byte count of its buffer descriptor from batch x h x w x in_ctot alone, so a read there must come back as the range check's zero
(the row only keeps a kernel that mistakes the range from touching memory the test does not own).  The output buffer, the head
buffers and the split-K workspace (the engine's size, 16 x cout x pixels floats) are NaN-filled.

Asserted per launch: the variant name, finite output, the bound per image (|g - r| <= h(r) + A; fp32 segments: rel_err <
max(8 e32, 2^-20) and < 1e-4), NaN bits kept outside the output slice / the head segments, a second launch bit-equal.  One BF16
line per launch in front of the asserts: row, variant, ksplit, worst (|g - r| - h) / max|r|, e32, that excess / e32, err / bound,
the share of outputs that differ from RNE(r).

Measured on an MI355X, 51 launches (largest over the launches of a variant; excess = (|g - r| - h) / max|r|, what the accumulation
term A / max|r| = max(8 e32, 2^-20) has to cover; err / bound = |g - r| / (h + A), which the rounding term alone brings to 1):
  variant            launches  largest excess (row)          excess / e32   err / bound   outputs != RNE(r)
  bf16:128x64k32s        5     2.96e-9 (img_3x3)                 0.02          1.000          2.6e-5
  bf16:128x128k32s       1     2.41e-8 (img_wide)                0.16          0.999          1.7e-5
  bf16:128x64k32        11     3.08e-8 (sk_64_96)                0.23          0.999          1.1e-4
      fp32 segments            rel_err 3.24e-7 (sk_heads)        1.95          0.244
  bf16:128x64k64        19     8.73e-8 (k64_200_dil5)            0.59          0.999          5.6e-4
  bf16:128x128k64        5     1.34e-7 (w_72of96)                0.89          0.999          5.5e-5
  bf16:256x256k32        6     7.02e-8 (big_256_dil6)            0.59          0.999          9.1e-5
  bf16:128x128k32        4     1.34e-7 (w_72of96_ring)           0.89          0.999          5.5e-5
Largest err / e32: 1.95, on the fp32 head segments without split-K.  The factor 8 was not needed beyond that and stays as first set.
Before the loader masked EVERY channel step that reaches past cin, the rows sk_24of40, sk_16_dil3, sk_32of72, big_72of104,
big_136_1x1, w_72of96_ring and w_136_1x1_ring came back all NaN (BK = 32, cin % 64 in (0, 32], another tensor's channels behind
the slice); every other row passed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO          # first: it puts the package on sys.path (the child process below has no pytest)
import conv_bf16_cases as T
from ctdet import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN16 = T.BF16_NAN


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    """fp32 tensor -> the int16 bit patterns of its bfloat16 rounding (torch.Tensor.bfloat16())."""
    return t.bfloat16().contiguous().view(torch.int16)


def _nhwc_poisoned(t, ctot, coff, extra_rows=0):
    """t [B, C, H, W] fp32 -> int16 [B * H * W + extra_rows * W, ctot], NaN everywhere but the channels [coff, coff + C)."""
    B, C_, H, W = t.shape
    buf = torch.full((B * H * W + extra_rows * W, ctot), NAN16, dtype=torch.int16)
    buf[:B * H * W, coff:coff + C_] = _bits(t.permute(0, 2, 3, 1).reshape(-1, C_))
    return buf


class _Operands:
    """The device buffers of a row (built once per row, shared by its launches)."""

    def __init__(self, case):
        lib = _lib.lib()
        inp = T.make_inputs(case)
        x = inp.x_buf[:, case.x_coff:case.x_coff + case.cin]
        self.x = _nhwc_poisoned(x, case.x_ctot, case.x_coff, extra_rows=1).to(DEV)
        wd = [w.to(DEV).contiguous() for w in inp.parts]
        self.w = torch.full((lib.ct_conv_bf16_packed_elems(case.cin, case.cout, case.k, case.k),), NAN16, dtype=torch.int16, device=DEV)
        ptrs = (C.c_void_p * len(wd))(*[w.data_ptr() for w in wd])
        couts = (C.c_int * len(wd))(*[w.shape[0] for w in wd])
        _lib.check(lib.ct_conv_pack_weights_bf16(ptrs, couts, len(wd), case.cin, case.k, case.k, self.w.data_ptr(), _s()), 'pack')
        self.scale, self.shift = inp.scale.to(DEV), inp.shift.to(DEV)
        self.lo = inp.lo.to(DEV) if inp.lo is not None else None
        self.res = None
        if case.res_slice:              # the whole residual buffer is finite: a wrong offset reads wrong VALUES
            self.res = _bits(inp.res_buf.permute(0, 2, 3, 1).reshape(-1, case.res_slice[0])).to(DEV)
        torch.cuda.synchronize()


def _launch(case, ops, ksplit):
    """-> (variant name, int16 [B, oh, ow, out_ctot] | None, [fp32 [B, size]] per segment)."""
    lib = _lib.lib()
    d = T.fill_geometry(case, _lib.ConvDesc())
    d.in_, d.wpacked, d.scale, d.shift = ops.x.data_ptr(), ops.w.data_ptr(), ops.scale.data_ptr(), ops.shift.data_ptr()
    if ops.lo is not None:
        d.lo = ops.lo.data_ptr()
    if ops.res is not None:
        d.res = ops.res.data_ptr()
    out, flats = None, []
    if case.segs:
        for g, (c0, c1, base, size) in enumerate(T.segments(case)):
            flats.append(torch.full((case.B, size), float('nan'), device=DEV))
            sg = d.seg[g]
            sg.ptr, sg.co_begin, sg.co_end, sg.pix_stride, sg.img_stride, sg.base = flats[g].data_ptr(), c0, c1, c1 - c0, size, base
    else:
        out = torch.full((case.B, case.oh, case.ow, case.out_ctot), NAN16, dtype=torch.int16, device=DEV)
        d.out = out.data_ptr()
    if ksplit:
        ws = torch.full((16 * case.cout * case.npix,), float('nan'), device=DEV)       # the engine's size; needs no initialisation
        d.ksplit, d.ksplit_ws, d.ksplit_ws_floats = ksplit, ws.data_ptr(), ws.numel()
    name = lib.ct_conv_bf16_variant_name(C.byref(d))
    assert name is not None, lib.ct_last_error_string()
    _lib.check(lib.ct_conv2d_bf16_fwd(C.byref(d), _s()), 'conv bf16')
    torch.cuda.synchronize()
    return name.decode(), (out.cpu() if out is not None else None), [f.cpu() for f in flats]


def _check_row(case):
    """Every launch of a row (one per ksplit value) under the environment that is already set."""
    ops = _Operands(case)
    r = T.ref64(case)
    for ks in case.ksplits:
        name, out, flats = _launch(case, ops, ks)
        _n2, out2, flats2 = _launch(case, ops, ks)
        if case.segs:
            got = torch.full((case.B, case.cout, case.oh, case.ow), float('nan'))
            outside_ok = True
            for flat, (c0, c1, base, size) in zip(flats, T.segments(case)):
                cnt = case.oh * case.ow * (c1 - c0)
                got[:, c0:c1] = flat[:, base:base + cnt].view(case.B, case.oh, case.ow, c1 - c0).permute(0, 3, 1, 2)
                outside_ok &= bool(torch.isnan(flat[:, :base]).all() and torch.isnan(flat[:, base + cnt:]).all())
            worst, err, ratio = T.judge_f32(case, got)
            print('BF16 %-18s %-16s ksplit %4d fp32 rel_err %.3g e32 %.3g err/e32 %.2f err/bound %.3f' %
                  (case.name, name, ks, err, max(T.e32(case)), ratio, worst))
            assert name == case.variant, (case.name, name)
            assert torch.isfinite(got).all(), (case.name, ks)
            assert worst < 1.0 and err < T.HARD, (case.name, ks, worst, err)
            assert outside_ok, (case.name, ks)
            for a, b in zip(flats, flats2):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (case.name, ks, 'a second launch differs')
            continue
        bits = out[..., case.out_coff:case.out_coff + case.cout]
        got = bits.contiguous().view(torch.bfloat16).float().permute(0, 3, 1, 2)
        j = T.judge(case, got)
        differ = float((got.double() != r.to(torch.bfloat16).double()).double().mean())
        print('BF16 %-18s %-16s ksplit %4d excess %.3g e32 %.3g excess/e32 %.2f err/bound %.3f violations %d not-RNE %.3g' %
              (case.name, name, ks, j.excess, max(T.e32(case)), j.err_over_e32, j.err_over_bound, j.violations, differ))
        assert name == case.variant, (case.name, name)
        assert torch.isfinite(got).all(), (case.name, ks, int((~torch.isfinite(got)).sum()))
        assert j.violations == 0, (case.name, ks, j)
        assert (out[..., :case.out_coff] == NAN16).all() and (out[..., case.out_coff + case.cout:] == NAN16).all(), (case.name, ks)
        assert torch.equal(out, out2), (case.name, ks, 'a second launch differs')


def _set_env(case, monkeypatch):
    for k in T.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env:
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize('case', [c for c in T.CASES if not c.child], ids=lambda c: c.name)
def test_conv_bf16_row(case, monkeypatch):
    _set_env(case, monkeypatch)
    _check_row(case)


@pytest.mark.parametrize('big,small', T.BIG_PAIRS, ids=[p[0] for p in T.BIG_PAIRS])
def test_256x256_tile_is_bit_equal_to_the_128_wide_tiles(big, small, monkeypatch):
    """Same products, same k order per accumulator: the 256 x 256 tile and the tile the launcher takes when it is forbidden."""
    outs = []
    for name in (big, small):
        case = T.BY_NAME[name]
        _set_env(case, monkeypatch)
        variant, out, _ = _launch(case, _Operands(case), 0)
        assert variant == case.variant, (name, variant)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


def _ring_child():
    """In a fresh process with CTDET_BF16_BK=32 (the library reads it once): the rows of the three-buffer ring."""
    assert os.environ.get('CTDET_BF16_BK') == '32'
    bad = 0
    for case in T.CASES:
        if not case.child:
            continue
        try:
            _check_row(case)
        except AssertionError as e:
            bad += 1
            print('FAILED %s: %s' % (case.name, e))
    return 1 if bad else 0


def test_ring_variant_in_a_child_process():
    rows = [c for c in T.CASES if c.child]
    assert rows and all(c.variant == 'bf16:128x128k32' for c in rows)
    env = {k: v for k, v in os.environ.items() if k not in T.SWITCHES}
    env['CTDET_BF16_BK'] = '32'
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--ring-child'], env=env, timeout=180, cwd=REPO,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.count('bf16:128x128k32 ') == sum(len(c.ksplits) for c in rows)


# ------------------------------------------------------------------------------------------------ converters, packer, pool
def _f32_from_bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


SPECIALS = _f32_from_bits([
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,     # exact ties: to even downwards, to even upwards, and negative
    0x3F808001, 0x3F807FFF, 0x3F7F8000,                 # just above / below a tie; a tie that carries into the exponent
    0x00000000, 0x80000000,                             # +-0
    0x00000001, 0x00008000, 0x00018000, 0x0000C000, 0x007FFFFF, 0x807FFFFF, 0x00010000,      # denormals (ties among them)
    0x7F800000, 0xFF800000,                             # +-inf
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,     # the largest finite values: round to inf from the tie up
    0x7FC00000, 0x7F800001,                             # NaN, quiet and with a payload in the low half only
])


@pytest.mark.parametrize('B,C_,HW,c_pad', [(2, 5, 37, 8), (3, 24, 50, 24), (1, 1, len(SPECIALS), 16), (2, 5, 366 * 366, 8)],
                         ids=['5to8', '24', 'specials', 'stride_loop'])
def test_nchw_f32_to_nhwc_bf16_is_torch_rounding(B, C_, HW, c_pad):
    lib = _lib.lib()
    g = torch.Generator().manual_seed(HW)
    x = torch.randn(B, C_, HW, generator=g) * torch.exp(torch.randn(B, C_, HW, generator=g) * 8)
    n = min(HW, len(SPECIALS))
    x[0, 0, :n] = SPECIALS[:n]
    assert B * HW * c_pad > 2 ** 21 or HW < 1000          # the last case runs the grid-stride loop (a launch is 2^21 threads at most)
    y = torch.full((B * HW * c_pad,), NAN16, dtype=torch.int16, device=DEV)
    _lib.check(lib.ct_nchw_f32_to_nhwc_bf16(x.to(DEV).data_ptr(), B, C_, HW, c_pad, y.data_ptr(), _s()), 'nhwc')
    torch.cuda.synchronize()
    got = y.cpu().view(B, HW, c_pad)
    want = _bits(x.permute(0, 2, 1))
    nan = torch.isnan(x.permute(0, 2, 1))
    assert torch.equal(got[..., :C_][~nan], want[~nan])
    assert torch.isnan(got[..., :C_].contiguous().view(torch.bfloat16).float()[nan]).all()      # NaN stays NaN
    assert (got[..., C_:] == 0).all()                     # padding channels are zero
    if n == len(SPECIALS):
        s = got[0, :n, 0].contiguous().view(torch.bfloat16).float()
        assert torch.isinf(s[SPECIALS == torch.finfo(torch.float32).max]).all()


@pytest.mark.parametrize('B,C_,HW,ctot,coff', [(2, 5, 37, 16, 3), (1, 24, 50, 24, 0), (2, 8, 366 * 366, 16, 8)],
                         ids=['5of16', 'whole', 'stride_loop'])
def test_nhwc_bf16_to_nchw_f32_is_exact_from_a_slice(B, C_, HW, ctot, coff):
    lib = _lib.lib()
    g = torch.Generator().manual_seed(HW + 1)
    bits = torch.randint(-32768, 32768, (B, HW, C_), generator=g, dtype=torch.int32).to(torch.int16)
    buf = torch.full((B, HW, ctot), NAN16, dtype=torch.int16)
    buf[..., coff:coff + C_] = bits
    assert B * HW * C_ > 2 ** 21 or HW < 1000
    x = torch.full((B, C_, HW), float('nan'), device=DEV)
    _lib.check(lib.ct_nhwc_bf16_to_nchw_f32(buf.to(DEV).data_ptr(), B, C_, HW, ctot, coff, x.data_ptr(), _s()), 'nchw')
    torch.cuda.synchronize()
    want = bits.view(torch.bfloat16).float().permute(0, 2, 1).contiguous()
    assert torch.equal(x.cpu().view(torch.int32), want.view(torch.int32))


def _pack_np(parts, cin, k):
    """[tap][cin_pad / 8][cout_pad][8] bf16 bit patterns of the concatenated parts [cout, cin, k, k], zero padded."""
    w = torch.cat(parts)
    cout = w.shape[0]
    cin_pad = 8 if cin <= 8 else (cin + 63) // 64 * 64
    cout_pad = (cout + 7) // 8 * 8
    full = np.zeros((k * k, cin_pad, cout_pad), dtype=np.int16)
    full[:, :cin, :cout] = _bits(w).numpy().reshape(cout, cin, k * k).transpose(2, 1, 0)
    return full.reshape(k * k, cin_pad // 8, 8, cout_pad).transpose(0, 1, 3, 2).copy(), cin_pad, cout_pad


@pytest.mark.parametrize('cin,k,couts', [(3, 3, (13,)), (8, 1, (16,)), (24, 3, (5, 12, 6)), (72, 1, (40, 24, 8, 3, 1, 7)),
                                         (72, 3, (600, 500, 400, 200, 100, 25))],
                         ids=['cin3', 'cin8', 'cin24_3parts', 'cin72_6parts', 'stride_loop'])
def test_pack_weights_bf16_layout(cin, k, couts):
    lib = _lib.lib()
    g = torch.Generator().manual_seed(cin + len(couts))
    parts = [torch.randn(c, cin, k, k, generator=g) for c in couts]
    want, cin_pad, cout_pad = _pack_np(parts, cin, k)
    assert (cin_pad, cout_pad) == (lib.ct_conv_bf16_cin_pad(cin), lib.ct_conv_bf16_cout_pad(sum(couts)))
    n = lib.ct_conv_bf16_packed_elems(cin, sum(couts), k, k)
    assert n == want.size and (n > 2 ** 21 or sum(couts) < 600)
    wd = [w.to(DEV).contiguous() for w in parts]
    out = torch.full((n + 64,), NAN16, dtype=torch.int16, device=DEV)           # poisoned, and 64 elements behind the end
    ptrs = (C.c_void_p * len(wd))(*[w.data_ptr() for w in wd])
    cs = (C.c_int * len(wd))(*couts)
    _lib.check(lib.ct_conv_pack_weights_bf16(ptrs, cs, len(wd), cin, k, k, out.data_ptr(), _s()), 'pack')
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:n].reshape(want.shape), want)        # the zeros of `want` are the padded entries
    assert (got[n:] == np.int16(NAN16)).all()


def _pool_out(n, k, s, p, ceil):
    o = (n + 2 * p - k + (s - 1 if ceil else 0)) // s + 1
    if ceil and (o - 1) * s >= n + p:
        o -= 1
    return o


POOLS = [  # B, C, H, W, k, stride, pad, ceil, sign
    (2, 12, 9, 7, 3, 1, 1, False, 0), (2, 5, 7, 9, 2, 2, 0, True, 0), (1, 3, 5, 5, 3, 2, 1, True, -1),      # scalar kernel (C % 8 != 0)
    (2, 16, 9, 7, 3, 1, 1, False, -1), (1, 8, 6, 6, 3, 2, 1, False, 0),                                       # v8 kernel, padded
    (9, 8, 485, 485, 2, 1, 0, False, 0),                                                                      # v8 above the grid cap
]


@pytest.mark.parametrize('cfg', POOLS, ids=['c12_k3p1', 'c5_ceil_odd', 'c3_negative_pad', 'c16_negative_pad', 'c8_k3s2p1', 'grid_cap'])
def test_maxpool_nhwc_bf16_edges(cfg):
    B, C_, H, W, k, s, p, ceil, sign = cfg
    lib = _lib.lib()
    g = torch.Generator().manual_seed(H * W + C_)
    x = torch.randn(B, C_, H, W, generator=g).bfloat16().float()
    if sign < 0:
        x = -x.abs() - 0.5                               # all negative: a padding that counted as 0 would win
        x = x.bfloat16().float()
    want = F.max_pool2d(x, k, s, p, ceil_mode=ceil)
    OH, OW = want.shape[2:]
    assert (OH, OW) == (_pool_out(H, k, s, p, ceil), _pool_out(W, k, s, p, ceil))
    if cfg is POOLS[-1]:
        assert B * OH * OW * (C_ // 8) > 2 ** 21
    xb = _bits(x.permute(0, 2, 3, 1)).to(DEV)
    yb = torch.full((B, OH, OW, C_), NAN16, dtype=torch.int16, device=DEV)
    _lib.check(lib.ct_maxpool2d_nhwc_bf16(xb.data_ptr(), yb.data_ptr(), B, C_, H, W, OH, OW, k, s, p, _s()), 'pool')
    torch.cuda.synchronize()
    assert torch.equal(yb.cpu(), _bits(want.permute(0, 2, 3, 1))), cfg


if __name__ == '__main__':
    if sys.argv[1:] == ['--ring-child']:
        sys.exit(_ring_child())
    sys.exit('usage: %s --ring-child' % sys.argv[0])
