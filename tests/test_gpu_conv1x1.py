"""conv_x3_f32_pw (csrc/ct_conv_x3.hip): the pointwise form of the f16x2 ("h2:") twins of ct_conv2d_x3_fwd -- forward 1x1 / stride 1 /
pad 0 layers as a plain GEMM, 32 input channels per barrier, weights by LDS-DMA.  Its contract is that every accumulator receives the
MFMA results of the generic kernel conv_x3_f32 in the same order, so each case here runs ONE descriptor twice, with
ct_conv_x3_pointwise_enable off and on, and compares the results with torch.equal; the launches outside the rule must not change
either.  Shapes: the smallest on which the kernel can still go wrong (one / three iterations, partial cout and pixel tiles, a pixel
tile across two images with different exponents, every epilogue input)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from ctdet import _lib, engine
from test_gpu_absmax import LW, _amax, _bits
from test_gpu_kernels import TOL, _bn, _cuda, _ref_conv

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H2_CFGS = (6, 7, 8, 9)          # h2:128x128k16d, h2:64x128k16d, h2:128x64k32d, h2:64x64k32d


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('the gpu tests need a HIP device; none visible')
    names = [_lib.lib().ct_conv_x3_config_name(i).decode() for i in H2_CFGS]
    assert names == ['h2:128x128k16d', 'h2:64x128k16d', 'h2:128x64k32d', 'h2:64x64k32d'], names


def _both(x, parts, stride=1, pad=0, dil=1, *, x3, res=None, res_scale=1.0, res_coff=0, cin_off=0, cin=None, out_ctot=None,
          out_coff=0, ksplit=None, segs=None, track=False, fill=float('nan')):
    """One conv step through engine.HipBackend, launched twice from the same descriptor: pointwise kernel off, then on.
    parts: (weight, bias, bn, relu); segs = [(name, co_begin, co_end, base, flat size)] -> the head buffers.
    -> [off, on], each dict(y, slot, flat)"""
    lib = _lib.lib()
    be = engine.HipBackend(DEV)
    cps = []
    for (w, b, bn, relu) in parts:
        bnm = None
        if bn is not None:
            bnm = torch.nn.BatchNorm2d(w.shape[0], eps=1e-5).to(DEV)
            bnm.weight.data.copy_(bn[0]); bnm.bias.data.copy_(bn[1])
            bnm.running_mean.copy_(bn[2]); bnm.running_var.copy_(bn[3])
        cps.append(engine.ConvPart(torch.nn.Parameter(_cuda(w), requires_grad=False),
                                   torch.nn.Parameter(_cuda(b), requires_grad=False) if b is not None else None, bnm, relu))
    kh, kw = parts[0][0].shape[2:]
    B, ctot, H, W = x.shape
    cin = cin if cin is not None else ctot - cin_off
    st = engine.ConvStep('t', cps, cin, kh, kw, stride, pad, pad, dil, 'x', cin_off, H, W, None if segs else 'y', out_coff)
    bufs = {'x': _cuda(x)}
    if segs:
        st.segs = [engine.Segment(n, c0, c1, c1 - c0, base) for (n, c0, c1, base, _) in segs]
        for (n, c0, c1, base, size) in segs:
            bufs[n] = torch.empty((B, size), device=DEV)
    else:
        bufs['y'] = torch.empty((B, out_ctot or st.cout, st.oh, st.ow), device=DEV)
    if res is not None:
        bufs['r'] = _cuda(res)
        st.res, st.res_coff, st.res_scale = 'r', res_coff, res_scale
    st.rt['config'] = 0
    be.prepare_conv(st, bufs, B)
    d = st.rt['desc']
    if ksplit is not None:
        d.ksplit = ksplit
    be.enable_x3(st, x3)
    slot = torch.zeros(B, LW, dtype=torch.int32, device=DEV)
    if track:
        d.out_absmax = slot.data_ptr()
    outs = []
    for on in (0, 1):
        for name in ([n for (n, *_r) in segs] if segs else ['y']):
            bufs[name].fill_(fill)
        if ksplit is not None:
            st.rt['ksws'].fill_(float('nan'))
        slot.zero_()
        prev = lib.ct_conv_x3_pointwise_enable(on)
        try:
            be.run_conv(st)
            torch.cuda.synchronize()
        finally:
            lib.ct_conv_x3_pointwise_enable(prev)
        outs.append(dict(y=None if segs else bufs['y'].cpu(), slot=slot.cpu(),
                         flat={n: bufs[n].cpu() for (n, *_r) in (segs or [])}))
    return outs


def _same(a, b):
    """bit equality, NaN included"""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_the_setter_returns_the_previous_value():
    lib = _lib.lib()
    first = lib.ct_conv_x3_pointwise_enable(0)
    assert first in (0, 1)
    assert lib.ct_conv_x3_pointwise_enable(1) == 0
    assert lib.ct_conv_x3_pointwise_enable(first) == 1


@pytest.mark.parametrize('cfg', H2_CFGS)
def test_one_iteration_partial_tiles_two_exponents(cfg):
    """B = 2, 32 -> 40, 5x7: one 32-channel iteration, a partial cout block, one partial pixel tile (70 pixels) that holds both
    images; image 1 is 2^10 times image 0, so the two halves of the tile are split with different exponents."""
    g = torch.Generator().manual_seed(100 + cfg)
    x = torch.randn(2, 32, 5, 7, generator=g)
    x[1] *= 1024.0
    w = torch.randn(40, 32, 1, 1, generator=g) * 0.2
    b = torch.rand(40, generator=g) - 0.5
    parts = [(w, b, None, False)]
    off, on = _both(x, parts, x3=cfg)
    assert not torch.isnan(on['y']).any()
    assert torch.equal(off['y'], on['y'])
    want = _ref_conv(x.double(), [(w.double(), b.double(), None, False)], 1, 0, 1)
    for n in range(2):
        assert rel_err(on['y'][n].double(), want[n]) < TOL, n


_CASE2 = {}


def _case2():
    """B = 3, 96 -> 160, 9x9 (243 pixels): three iterations (both LDS buffers, both peeled ends), two pixel tiles with the last one
    partial at BN = 128, two cout blocks with the last one partial at BM = 128.  Run once per configuration, with out_absmax."""
    if not _CASE2:
        g = torch.Generator().manual_seed(7)
        x = torch.randn(3, 96, 9, 9, generator=g)
        w = torch.randn(160, 96, 1, 1, generator=g) * 0.1
        b = torch.rand(160, generator=g) - 0.5
        _CASE2['x'], _CASE2['w'], _CASE2['b'] = x, w, b
        _CASE2['want64'] = F.conv2d(x.double(), w.double(), b.double())
        for cfg in H2_CFGS:
            _CASE2[cfg] = _both(x, [(w, b, None, False)], x3=cfg, track=True)
    return _CASE2


@pytest.mark.parametrize('cfg', H2_CFGS)
def test_odd_iteration_count(cfg):
    off, on = _case2()[cfg]
    assert not torch.isnan(on['y']).any()
    assert torch.equal(off['y'], on['y'])


@pytest.mark.parametrize('cfg', H2_CFGS)
def test_out_absmax(cfg):
    """the tracked per-image maxima are max |y| of each image, and the generic kernel's slots bit for bit"""
    off, on = _case2()[cfg]
    assert torch.equal(on['slot'][:, 0].contiguous(), _bits(_amax(on['y'])))
    assert torch.equal(on['slot'], off['slot'])
    assert (on['slot'][:, 1:] == 0).all()


@pytest.mark.parametrize('cfg', H2_CFGS)
def test_against_fp64(cfg):
    """case 2 against a float64 conv2d, within the bound tests/test_gpu_x3.py holds its f16x2 1x1 cases to (test_gpu_kernels.TOL)"""
    c = _case2()
    assert rel_err(c[cfg][1]['y'].double(), c['want64']) < TOL


@pytest.mark.parametrize('cfg', H2_CFGS)
def test_epilogue(cfg):
    """B = 2, 64 -> 48 (24 ReLU + 24 plain: folded scale / shift and a per-channel floor), 6x6; input channels 8..71 of an 80-channel
    buffer, residual x 0.6 from channels 5..52 of a 60-channel buffer, output into channels 3..50 of a 56-channel buffer pre-filled
    with 7, whose other channels stay 7."""
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, 80, 6, 6, generator=g)
    w1 = torch.randn(24, 64, 1, 1, generator=g) * 0.15
    w2 = torch.randn(24, 64, 1, 1, generator=g) * 0.15
    parts = [(w1, None, _bn(24, g), True), (w2, None, _bn(24, g), False)]
    res = torch.randn(2, 60, 6, 6, generator=g)
    off, on = _both(x, parts, x3=cfg, cin_off=8, cin=64, res=res, res_coff=5, res_scale=0.6, out_ctot=56, out_coff=3, fill=7.0)
    assert torch.equal(off['y'], on['y'])
    y = on['y']
    assert (y[:, :3] == 7).all() and (y[:, 51:] == 7).all()
    want = torch.cat([_ref_conv(x[:, 8:72], [p], 1, 0, 1, res=res[:, 5 + 24 * i:29 + 24 * i], res_scale=0.6)
                      for i, p in enumerate(parts)], 1)         # _ref_conv adds the residual part by part
    assert (want[:, :24] == 0).any() and (want[:, 24:] < 0).any()      # the ReLU part clamps, the plain part keeps negative values
    assert rel_err(y[:, 3:51], want) < TOL


def test_the_rule_keeps_the_generic_kernel_elsewhere():
    """A 3x3 layer, a stride-2 1x1 layer, Cin = 48 (no whole 32-channel iterations), a split-K launch and a head-scatter launch:
    identical with the setter off and on, and none refused."""
    g = torch.Generator().manual_seed(53)
    x = torch.randn(2, 64, 7, 7, generator=g)
    w3 = torch.randn(40, 64, 3, 3, generator=g) * 0.05
    w1 = torch.randn(40, 64, 1, 1, generator=g) * 0.1
    b = torch.rand(40, generator=g) - 0.5
    x48 = torch.randn(2, 48, 7, 7, generator=g)
    w48 = torch.randn(40, 48, 1, 1, generator=g) * 0.1
    for cfg in (6, 9):
        off, on = _both(x, [(w3, b, None, True)], 1, 1, 1, x3=cfg)
        assert _same(off['y'], on['y']) and rel_err(on['y'], _ref_conv(x, [(w3, b, None, True)], 1, 1, 1)) < TOL, ('3x3', cfg)
        off, on = _both(x, [(w1, b, None, True)], 2, 0, 1, x3=cfg)
        assert _same(off['y'], on['y']) and rel_err(on['y'], _ref_conv(x, [(w1, b, None, True)], 2, 0, 1)) < TOL, ('stride 2', cfg)
        off, on = _both(x, [(w1, b, None, True)], x3=cfg, ksplit=2)
        assert _same(off['y'], on['y']) and rel_err(on['y'], _ref_conv(x, [(w1, b, None, True)], 1, 0, 1)) < TOL, ('split-K', cfg)
        segs = [('loc', 0, 24, 5, 5 + 49 * 24 + 3), ('conf', 24, 40, 2, 2 + 49 * 16 + 4)]
        off, on = _both(x, [(w1, b, None, False)], x3=cfg, segs=segs)
        want = _ref_conv(x, [(w1, b, None, False)], 1, 0, 1)
        for (n, c0, c1, base, size) in segs:
            assert _same(off['flat'][n], on['flat'][n]), ('heads', cfg, n)
            got = on['flat'][n][:, base:base + 49 * (c1 - c0)]
            assert rel_err(got, want[:, c0:c1].permute(0, 2, 3, 1).reshape(2, -1)) < TOL, ('heads', cfg, n)
    off, on = _both(x48, [(w48, b, None, True)], x3=7)          # a k16 twin: 48 = 3 packed steps, not whole 32-channel iterations
    assert _same(off['y'], on['y']) and rel_err(on['y'], _ref_conv(x48, [(w48, b, None, True)], 1, 0, 1)) < TOL
