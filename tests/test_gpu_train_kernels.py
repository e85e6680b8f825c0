"""The non-convolution training kernels of csrc/ct_train.hip, one entry point at a time, against the float64 reference of
tests/train_ref.py (itself proved against autograd in tests/test_train_ref_cpu.py): BatchNorm statistics / apply / backward
(batch and frozen statistics, the per-channel `lo` clamp), bias + activation backward, the three max-pool backward kernels
and the fused pool + bias + ReLU backward, the head-gradient gather, ct_scratch_prezeroed(1) and non-default streams.
The cases (shapes, flags, data) are built in tests/train_cases.py; every sliced operand sits at a nonzero channel offset of a
wider buffer whose other channels must keep their sentinel.

Bounds.  Copies, masks and single additions are compared with torch.equal.  Reduced or rounded outputs are compared with
conftest.rel_err against float64: err < max(floor, 3 * e32), e32 being torch-CPU float32 on the same inputs, with the floors
test_gpu_train.py asserts for the same kernels (1e-5 statistics / y / dres / dbias, 1e-4 dz / dgamma / dbeta, 1e-6 overlapping
pool) and the factor 3 of test_ctx_block_backward_vs_float64_autograd; and, so that a noisy e32 cannot loosen it, by the same
expression over the e32 recorded in tests/golden/train_kernels_e32.npz.  The largest recorded e32 is 1.2e-6 (a dbias over
7220 terms), so every bound in force today IS its floor.

Not fed: NaN and -inf into the pools.  The kernels select with a strict `>` from -inf, so a window of NaN or -inf selects
nothing and passes no gradient, where torch propagates to the NaN resp. the first element; that difference is by design
and unspecified in include/ctdet.h.

The element-count guards of the grid-stride entry points are NOT run here: passing an oversized count to see the guard fire
would launch out of bounds if the guard were wrong.  They are checked by reading and by the host-side compile."""
import ctypes as C

import pytest
import torch

import train_cases as TC
import train_ref as R
from conftest import rel_err
from ctdet import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = torch.float32


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bound(tag, got, r64, r32, floor):
    e, e32, rec = rel_err(got.cpu(), r64), rel_err(r32, r64), TC.recorded_e32(tag)
    print('%-44s err %.3e  e32 %.3e  recorded e32 %.3e' % (tag, e, e32, rec))
    assert e < max(floor, 3 * e32), (tag, e, e32)
    assert e < max(floor, 3 * rec), (tag, e, rec)


def _outside(buf, off, width, sentinel):
    """The channels outside [off, off+width) still hold what they held."""
    keep = torch.ones(buf.shape[1], dtype=torch.bool)
    keep[off:off + width] = False
    want = sentinel[:, keep] if torch.is_tensor(sentinel) else torch.full_like(buf[:, keep].cpu(), sentinel)
    return torch.equal(buf[:, keep].cpu(), want)


def _amax_lines(B):
    return torch.zeros(B * _lib.ABSMAX_LINE_BYTES // 4, dtype=torch.int32, device=DEV)


def _amax_values(lines, B):
    return lines.view(B, -1)[:, 0].cpu().view(F32)


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn_splits(k):
    """include/ctdet.h: a call splits its reductions (and uses scratch) when batch*hw >= 4096 and channels < 1024."""
    return k.B * k.HW >= 4096 and k.C < 1024


def _bn_launch(k, st=None, zero_scratch=False):
    """The three launches of one case on stream `st`; every device buffer the entry points write, by name."""
    lib = _lib.lib()
    st = st or _s()
    B, C, HW = k.B, k.C, k.HW
    o = {}
    z, gamma, beta, lo, res = _d(k.z), _d(k.gamma), _d(k.beta), _d(k.lo_t), _d(k.res)
    meanin, varin, dy, yin = _d(k.mean), _d(k.var), _d(k.dy), _d(k.y_in)

    def scratch():
        if not k.scratch:
            return None
        return (torch.zeros if zero_scratch else lambda *a, **kw: torch.full(*a, fill_value=123.0, **kw))(
            (2 * C,), dtype=torch.float64, device=DEV)

    o['mean'], o['var'] = torch.full((C,), 3.0, device=DEV), torch.full((C,), 3.0, device=DEV)
    o['rmean'], o['rvar'] = (_d(k.rm0.clone()), _d(k.rv0.clone())) if k.running else (None, None)
    o['scratch_stats'] = scratch()
    torch.cuda.synchronize()
    _lib.check(lib.ct_bn_train_stats(z.data_ptr(), B, C + TC.ZP, TC.ZO, C, HW, o['mean'].data_ptr(), o['var'].data_ptr(),
                                     TC.MOMENTUM, _p(o['rmean']), _p(o['rvar']), _p(o['scratch_stats']), st), 'stats')
    o['y'] = _d(k.y0.clone())
    _lib.check(lib.ct_bn_train_apply(z.data_ptr(), meanin.data_ptr(), varin.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                     TC.EPS, k.relu, _p(lo), _p(res), C + TC.RP, TC.RO, k.rscale, o['y'].data_ptr(),
                                     C + TC.YP, TC.YO, C + TC.ZP, TC.ZO, B, C, HW, st), 'apply')
    o['dz'], o['dres'] = _d(k.dz0.clone()), _d(None if k.dres0 is None else k.dres0.clone())
    o['dgamma'], o['dbeta'] = torch.full((C,), 3.0, device=DEV), torch.full((C,), 3.0, device=DEV)
    o['scratch_bwd'] = scratch()
    torch.cuda.synchronize()
    fn = lib.ct_bn_eval_backward if k.frozen else lib.ct_bn_train_backward
    _lib.check(fn(dy.data_ptr(), C + TC.GP, TC.GO, _p(yin), C + TC.YP, TC.YO, z.data_ptr(), meanin.data_ptr(), varin.data_ptr(),
                  gamma.data_ptr(), TC.EPS, k.relu, _p(lo), k.rscale, _p(o['dres']), k.dres_ctot, k.dres_off, k.acc,
                  o['dz'].data_ptr(), o['dgamma'].data_ptr(), o['dbeta'].data_ptr(), C + TC.ZP, TC.ZO, B, C, HW,
                  _p(o['scratch_bwd']), st), 'bn backward')
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize('combo', list(TC.BN_COMBOS))
@pytest.mark.parametrize('shape', TC.BN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_batchnorm_kernels_vs_float64(shape, combo):
    k = TC.bn_case(shape, combo)
    want = TC.bn_expected(k)
    o = _bn_launch(k)
    C = k.C
    sl = dict(y=(TC.YO, 9.0), dz=(TC.ZO, 7.0), dres=(k.dres_off, k.dres0))
    for name, (r64, r32) in want.items():
        got = o[name]
        if name in sl:
            off, sentinel = sl[name]
            assert _outside(got, off, C, sentinel), name + ': channels outside the slice were written'
            got = got[:, off:off + C]
        assert bool(torch.isfinite(got).all()), name
        if name == 'dres' and not k.acc:
            assert torch.equal(got.cpu(), r64.float()), 'dres (set) is a masked copy of dy'
        _bound('bn/%s/%s' % (k.name, name), got, r64, r32, TC.BN_FLOORS[name])
    assert set(want) == {n for n in o if o[n] is not None and not n.startswith('scratch')}
    # y never falls below its clamp, and the gradient stops wherever the given y is <= 0 (+0.0 and -0.0 included)
    ys = o['y'][:, TC.YO:TC.YO + C].cpu()
    if k.lo_t is not None or k.relu:
        assert bool((ys >= (k.lo_t if k.lo_t is not None else torch.zeros(C))[None, :, None]).all())
    mask = R.bn_mask(k.y_in, TC.YO, C, k.relu, k.lo_t).expand(k.B, C, k.HW)
    if bool(mask.any()) and o['dres'] is not None and not k.acc:
        assert bool((o['dres'][:, k.dres_off:k.dres_off + C].cpu()[mask] == 0).all())
    # scratch after the call (include/ctdet.h): the two sums of a call that splits, untouched otherwise
    if k.scratch:
        ss, sb = o['scratch_stats'], o['scratch_bwd']
        if _bn_splits(k):
            assert torch.equal((ss[:C] / float(k.B * k.HW)).float(), o['mean'])
            assert torch.equal(sb[:C].float(), o['dbeta']) and torch.equal(sb[C:].float(), o['dgamma'])
        else:
            assert bool((ss == 123.0).all()) and bool((sb == 123.0).all())


# ------------------------------------------------------------------------------------------------ bias + activation
def _bias_launch(k, st=None, dbias_fill=float('nan'), amax=True):
    lib = _lib.lib()
    st = st or _s()
    dy, y, dz = _d(k.dy), _d(k.y), _d(k.dz0.clone())
    db = torch.full((k.C,), dbias_fill, device=DEV) if k.has_db else None
    lines = _amax_lines(k.B) if amax else None
    torch.cuda.synchronize()
    args = (dy.data_ptr(), k.C + 2, 1, _p(y), k.C + 3, 2, k.relu, k.B, k.C, k.HW, dz.data_ptr(), k.C + 4, 3, _p(db))
    if amax:
        _lib.check(lib.ct_bias_act_backward_amax(*args, lines.data_ptr(), st), 'bias bwd amax')
    else:
        _lib.check(lib.ct_bias_act_backward(*args, st), 'bias bwd')
    torch.cuda.synchronize()
    return dz, db, lines


@pytest.mark.parametrize('c', TC.BIAS_CASES, ids=TC.bias_id)
def test_bias_act_backward_vs_float64(c):
    k = TC.bias_case(c)
    (dz64, db64, _), (dz32, db32, am32) = TC.bias_expected(k)
    dz, db, lines = _bias_launch(k)
    assert torch.equal(dz.cpu(), dz32), 'dz is a masked copy of dy; the channels outside the slice keep their sentinel'
    assert torch.equal(_amax_values(lines, k.B), am32)
    if k.has_db:
        _bound('bias/%s/dbias' % k.name, db, db64, db32, 1e-5)
    dz2, db2, _ = _bias_launch(k, amax=False)               # the entry point without the maxima
    assert torch.equal(dz2, dz) and (db is None or rel_err(db2.cpu(), db64) < 1e-5)


@pytest.mark.parametrize('B,HW', [(5, 1444), (2, 25), (3, 1366)])
def test_bias_act_backward_in_place_on_adjacent_parts(B, HW):
    """The heads: dy and dz are the same slice of the same buffer, no activation, y == NULL; two parts side by side."""
    lib = _lib.lib()
    C0, C1 = 3, 5
    g = TC.gen('inplace-%d-%d' % (B, HW))
    orig = torch.randn(B, C0 + C1, HW, generator=g) * 3
    buf = _d(orig)
    for off, cw in ((0, C0), (C0, C1)):
        db, lines = torch.full((cw,), float('nan'), device=DEV), _amax_lines(B)
        _lib.check(lib.ct_bias_act_backward_amax(buf.data_ptr(), C0 + C1, off, None, 0, 0, 0, B, cw, HW, buf.data_ptr(), C0 + C1,
                                                 off, db.data_ptr(), lines.data_ptr(), _s()), 'bias bwd in place')
        torch.cuda.synchronize()
        assert torch.equal(buf.cpu(), orig), 'part at %d disturbed the buffer' % off
        part = orig[:, off:off + cw]
        assert rel_err(db.cpu(), part.double().sum((0, 2))) < 1e-5
        assert torch.equal(_amax_values(lines, B), part.abs().amax((1, 2)))


# ------------------------------------------------------------------------------------------------ pools
def _pool_launch(k, accumulate, st=None):
    lib = _lib.lib()
    st = st or _s()
    x, dy, dx = _d(k.x), _d(k.dy), _d(k.dx0.clone())
    torch.cuda.synchronize()
    _lib.check(lib.ct_maxpool2d_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), k.P, k.H, k.W, k.OH, k.OW, k.k, k.s, k.p,
                                    accumulate, st), 'pool bwd')
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize('c', TC.POOL_CASES, ids=TC.pool_id)
def test_maxpool_backward_vs_float64(c):
    k = TC.pool_case(c)
    for acc in (0, 1):
        r64, r32 = TC.pool_expected(k, acc)
        dx = _pool_launch(k, acc)
        if k.overlap:
            _bound('pool/%s/dx%d' % (k.name, acc), dx, r64, r32, 1e-6)
            if not acc:
                assert torch.equal(dx.cpu() != 0, r64 != 0), 'a gradient went to an element that is no first maximum'
        else:
            assert torch.equal(dx.cpu(), r32), 'one window per element: a copy of dy (plus at most one addition)'


def _fused_launch(k, st=None, dbias_fill=float('nan')):
    lib = _lib.lib()
    st = st or _s()
    y, dy, dz = _d(k.y), _d(k.dy), _d(k.dz0.clone())
    db, lines = torch.full((k.C,), dbias_fill, device=DEV), _amax_lines(k.B)
    torch.cuda.synchronize()
    _lib.check(lib.ct_maxpool2x2_bias_relu_bwd(y.data_ptr(), k.C + 3, 2, dy.data_ptr(), k.B, k.C, k.H, k.W, k.OH, k.OW,
                                               dz.data_ptr(), k.C + 2, 1, db.data_ptr(), lines.data_ptr(), st), 'fused pool bwd')
    torch.cuda.synchronize()
    return dz, db, lines


@pytest.mark.parametrize('c', TC.FUSED_CASES, ids=TC.fused_id)
def test_fused_pool_bias_relu_backward_vs_float64(c):
    k = TC.fused_case(c)
    (_, db64, _), (dz32, db32, am32) = TC.fused_expected(k)
    dz, db, lines = _fused_launch(k)
    assert torch.equal(dz.cpu(), dz32)
    assert torch.equal(_amax_values(lines, k.B), am32)
    _bound('fused/%s/dbias' % k.name, db, db64, db32, 1e-5)


# ------------------------------------------------------------------------------------------------ head gather
def _gather_launch(nseg, HW, st=None):
    lib = _lib.lib()
    st = st or _s()
    B, Cc = 2, TC.GATHER_C
    g = TC.gen('gather%d-%d' % (nseg, HW))
    segs = (_lib.OutSegment * nseg)()
    ref_segs, keep = [], []
    for i, (c0, c1, ps, istr, base) in enumerate(TC.gather_layout(nseg, HW)):
        flat = torch.randn(B * istr, generator=g)
        dev = _d(flat)
        keep.append(dev)
        segs[i].ptr, segs[i].co_begin, segs[i].co_end = dev.data_ptr(), c0, c1
        segs[i].pix_stride, segs[i].img_stride, segs[i].base = ps, istr, base
        ref_segs.append((flat, c0, c1, ps, istr, base))
    dz = torch.full((B, Cc, HW), float('nan'), device=DEV)
    torch.cuda.synchronize()
    _lib.check(lib.ct_head_grad_gather(segs, nseg, B, Cc, HW, dz.data_ptr(), st), 'head gather')
    torch.cuda.synchronize()
    return dz, R.head_grad_gather(ref_segs, B, Cc, HW)


@pytest.mark.parametrize('HW', [1, 9, 1444])
@pytest.mark.parametrize('nseg', [1, 2, 3])
def test_head_grad_gather_is_the_reference_copy(nseg, HW):
    dz, want = _gather_launch(nseg, HW)
    assert torch.equal(dz.cpu(), want)
    covered = sorted(c for (c0, c1, *_r) in TC.gather_layout(nseg, HW) for c in range(c0, c1))
    rest = [c for c in range(TC.GATHER_C) if c not in covered]
    assert len(rest) >= 3 and bool((dz[:, rest] == 0).all())


# ------------------------------------------------------------------------------------------------ prezeroed mode, streams
@pytest.fixture
def prezeroed(request):
    """Returns the switch of ct_scratch_prezeroed.  The restore to 0 is registered BEFORE the switch can be turned, so it
    does not depend on the test body: a leaked 1 would take the memsets away from every later test of the process."""
    lib = _lib.lib()
    request.addfinalizer(lambda: lib.ct_scratch_prezeroed(0))
    return lambda on: _lib.check(lib.ct_scratch_prezeroed(int(on)), 'ct_scratch_prezeroed')


# The equality tests below use cases whose accumulation meets at most two partial sums per output (two ranges per channel,
# one image per plane): a + b does not depend on the order the atomics land in, three terms would.
_EQ_BN = [((4, 10, 1200), 'racc'), ((4, 10, 1200), 'l0'), ((1, 7, 4097), 'lin')]
_EQ_BIAS = (3, 3, 1366, 1, 1, 1)
_EQ_FUSED = (1, 257, 9, 9, True)
_EQ_POOL = (6, 19, 19, 3, 1, 1, False, 'randn')


def _same(a, b):
    assert set(a) == set(b)
    for n in a:
        assert (a[n] is None and b[n] is None) or torch.equal(a[n], b[n]), n


@pytest.mark.parametrize('shape,combo', _EQ_BN, ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_prezeroed_batchnorm_equals_plain(prezeroed, shape, combo):
    k = TC.bn_case(shape, combo)
    assert _bn_splits(k) and k.scratch
    plain = _bn_launch(k)
    prezeroed(1)
    pre = _bn_launch(k, zero_scratch=True)
    prezeroed(0)
    _same(plain, pre)                       # scratch included: the sums stay behind in both modes
    assert bool((pre['scratch_stats'] != 0).any()) and bool((pre['scratch_bwd'] != 0).any())


def test_prezeroed_bias_gradients_equal_plain(prezeroed):
    kb, kf = TC.bias_case(_EQ_BIAS), TC.fused_case(_EQ_FUSED)
    plain_b, plain_f = _bias_launch(kb), _fused_launch(kf)
    prezeroed(1)
    pre_b, pre_f = _bias_launch(kb, dbias_fill=0.0), _fused_launch(kf, dbias_fill=0.0)
    prezeroed(0)
    for a, b in zip(plain_b + plain_f, pre_b + pre_f):
        assert torch.equal(a, b)
    # and the switch is what removes the memset: with it on, dbias accumulates into what the caller left there
    prezeroed(1)
    acc = _bias_launch(kb, dbias_fill=1.0)[1]
    prezeroed(0)
    assert rel_err(acc.cpu(), (plain_b[1] + 1).cpu()) < 1e-5


def test_side_stream_gives_the_bits_of_the_default_stream():
    """One case per entry point on a non-default stream while the default stream is idle."""
    side = torch.cuda.Stream()
    sp = C.c_void_p(side.cuda_stream)
    for shape, combo in _EQ_BN[:2]:                        # statistics, apply, train backward / eval backward
        k = TC.bn_case(shape, combo)
        _same(_bn_launch(k), _bn_launch(k, st=sp))
    kb, kf, kp = TC.bias_case(_EQ_BIAS), TC.fused_case(_EQ_FUSED), TC.pool_case(_EQ_POOL)
    for amax in (True, False):
        for a, b in zip(_bias_launch(kb, amax=amax), _bias_launch(kb, st=sp, amax=amax)):
            assert (a is None and b is None) or torch.equal(a, b)
    for a, b in zip(_fused_launch(kf), _fused_launch(kf, st=sp)):
        assert torch.equal(a, b)
    assert torch.equal(_pool_launch(kp, 1), _pool_launch(kp, 1, st=sp))
    assert torch.equal(_gather_launch(3, 1444)[0], _gather_launch(3, 1444, st=sp)[0])
