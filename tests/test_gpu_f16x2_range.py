"""The consumer side of the f16x2 operand form (csrc/ct_f16x2.h): tile 47 (its own maxima, and given ones), tile 48 and the
"h2:" configurations of ct_conv2d_x3_fwd must be right for ANY valid upper bound in ct_conv_desc.in_absmax, at any magnitude of
the operands, per image -- against an fp64 torch-CPU convolution (TOL = the project's 1e-4), exactly (torch.equal) where the
header's own argument makes the result exact, and never worse than the bf16x3 twin of the same kernel on non-finite inputs.
The producers' side of the contract: tests/test_gpu_absmax.py; the wiring: tests/test_absmax_wiring_cpu.py.

Every asserted number is exact, the project's 1e-4, or derived in the test from ct_f16x2.h; measured figures are in docstrings."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from ctdet import _lib, engine
from ctdet.wino_forms import FORMS
from test_gpu_kernels import _ref_conv, _run_conv

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4
LW = _lib.ABSMAX_LINE_BYTES // 4


def _x3(name):
    lib = _lib.lib()
    return [lib.ct_conv_x3_config_name(i).decode() for i in range(lib.ct_conv_x3_num_configs())].index(name)


def _h2_names():
    lib = _lib.lib()
    return [n for n in (lib.ct_conv_x3_config_name(i).decode() for i in range(lib.ct_conv_x3_num_configs())) if n.startswith('h2:')]


# consumer id -> (keyword arguments of _run_conv, takes in_absmax from the caller, the same kernel on bf16x3)
def _consumers():
    out = {'wino47_own': (dict(config=engine.WINO4H), False, dict(config=engine.WINO4S)),
           'wino47': (dict(config=engine.WINO4H), True, dict(config=engine.WINO4S)),
           'wino48': (dict(config=engine.WINO4FH), True, dict(config=engine.WINO4F))}
    for n in _h2_names():
        out[n] = (dict(x3=_x3(n)), True, dict(x3=_x3('x3:' + n[3:])))
    return out


CONSUMERS = ['wino47_own', 'wino47', 'wino48', 'h2:128x128k16d', 'h2:64x128k16d', 'h2:128x64k32d', 'h2:64x64k32d']


def test_consumer_list_is_complete():
    assert sorted(CONSUMERS) == sorted(_consumers())
    assert sorted(c for c, f in FORMS.items() if f.h2) == [47, 48]


def _lines(bounds):
    """in_absmax lines holding the given per-image bounds."""
    t = torch.zeros(len(bounds), LW, dtype=torch.int32)
    t[:, 0] = torch.as_tensor(bounds, dtype=torch.float32).view(torch.int32)
    return t.to(DEV)


def _run(cid, x, parts, bounds=None, **kw):
    kwargs, given, _ = _consumers()[cid]
    if given:
        b = x.abs().amax((1, 2, 3)) if bounds is None else bounds
        return _run_conv(x, parts, 1, 1, 1, in_absmax=_lines(b), **kwargs, **kw)
    return _run_conv(x, parts, 1, 1, 1, **kwargs, **kw)


def _ref64(x, parts):
    return _ref_conv(x.double(), [(w.double(), None if b is None else b.double(), bn, relu) for (w, b, bn, relu) in parts], 1, 1, 1)


def _data(seed, B=3, Cin=64, H=19, W=17, Cout=72):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g).relu()
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05
    return x, w, g


@pytest.mark.parametrize('cid', [c for c in CONSUMERS if c != 'wino47_own'])
def test_any_valid_bound_works(cid):
    """in_absmax = true maximum x 2^k, k in {0, 1, 5, 10}: every one within TOL of fp64.  ct_f16x2.h claims the error is unchanged
    with a scale 1024 x too small; the ratios err(k) / err(0) are printed (pytest -s), not asserted.
    Measured on an MI355X at the commit that added this test (parent 33b18fd), err(0) and err(10) / err(0): tile 47 7.7e-7, 0.93;
    tile 48 9.5e-7, 0.94; h2:128x128k16d / h2:64x128k16d 1.83e-7, 1.00; h2:128x64k32d / h2:64x64k32d 1.79e-7, 1.00 (ratio 1.00 at
    k = 1 and 5 for all): the header's claim holds."""
    x, w, g = _data(31)
    x = x * (4.0 ** torch.arange(3).view(3, 1, 1, 1))
    parts = [(w, torch.rand(72, generator=g) - 0.5, None, True)]
    want = _ref64(x, parts)
    true = x.abs().amax((1, 2, 3))
    errs = {}
    for k in (0, 1, 5, 10):
        got = _run(cid, x, parts, bounds=true * 2.0 ** k)
        errs[k] = max(rel_err(got[n], want[n]) for n in range(3))
    print('f16x2 bound sweep %s: ' % cid + ', '.join('k=%d err %.3g ratio %.2f' % (k, e, e / errs[0]) for k, e in errs.items()))
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize('cid', CONSUMERS)
def test_power_of_two_covariance_is_exact(cid):
    """No bias, no BatchNorm, ReLU: conv(x 2^a, w 2^b) == conv(x, w) 2^(a + b), bit for bit, with a different `a` per image of one
    batch.  Exact by the header's argument: the exponent follows the maximum, so the scaled binary16 pieces are the same bits, and
    the factor 2^-(eA + eB) is a power of two.  A failure = a scale applied inexactly, or an exponent taken from the wrong image
    or tensor.  |a|, |b| <= 30 with max |x| ~ 4, max |w| ~ 0.2: far inside exponent_for's clamp and fp32's range."""
    x, w, g = _data(32)
    base = _run(cid, x, [(w, None, None, True)])
    assert rel_err(base, _ref64(x, [(w, None, None, True)])) < TOL
    for a, b in (((30, -30, 7), 0), ((-30, 30, 0), 30), ((1, -13, 30), -30), ((-30, -30, -30), -30), ((30, 30, 30), 30), ((0, 5, -5), 11)):
        sa = 2.0 ** torch.tensor(a, dtype=torch.float32).view(3, 1, 1, 1)
        got = _run(cid, x * sa, [(w * 2.0 ** b, None, None, True)])
        assert torch.equal(got, base * sa * 2.0 ** b), (cid, a, b, rel_err(got, base * sa * 2.0 ** b))


@pytest.mark.parametrize('bad', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('cid', CONSUMERS)
def test_non_finite_input_stays_in_its_image(cid, bad):
    """One NaN / Inf in image 1 of 3 (its maximum becomes non-finite: exponent 0): images 0 and 2 are bit-identical to the clean
    run; image 1 is non-finite at least where the fp64 convolution is, and nowhere the bf16x3 twin of the same kernel is finite
    (the Winograd forms spread a NaN over the 6x6 input tiles it falls in -- both operand forms alike); its finite values are
    still within TOL.  Measured (same commit), non-finite outputs of image 1 for one NaN or one Inf: fp64 648 (9 positions x 72
    channels); the h2: direct configurations and their x3: twins 648; tiles 47 / 48 and their twins 44 / 46 1440 alike."""
    x, w, g = _data(33)
    parts = [(w, None, None, False)]
    clean = _run(cid, x, parts)
    xb = x.clone()
    xb[1, 5, 9, 8] = bad
    got = _run(cid, xb, parts)
    twin = _run_conv(xb, parts, 1, 1, 1, **_consumers()[cid][2])
    want = _ref64(xb, parts)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2]), cid
    nf, nf_want, nf_twin = ~torch.isfinite(got[1]), ~torch.isfinite(want[1]), ~torch.isfinite(twin[1])
    print('non-finite outputs of image 1, %s / %s: fp64 %d, f16x2 %d, bf16x3 twin %d' % (cid, bad, nf_want.sum(), nf.sum(), nf_twin.sum()))
    assert (nf | ~nf_want).all(), (cid, 'finite where fp64 is not')
    assert (nf_twin | ~nf).all(), (cid, 'non-finite where the bf16x3 twin is finite', int(nf.sum()), int(nf_twin.sum()))
    if not cid.startswith('wino'):                  # the direct kernel: exactly the receptive field (measured; a regression that
        assert torch.equal(nf, nf_want), cid        # spreads it is caught even if the twin regresses too)
    ok = ~nf
    assert rel_err(torch.where(ok, got[1].double(), 0.0), torch.where(ok, want[1], 0.0)) < TOL, cid


PRODUCERS = {'wino44': dict(tile=44), 'wino47': dict(tile=47), 'wino48': dict(tile=48), 'x3': dict(x3='x3:128x128k16d'), 'direct': dict()}
CHAINS = [(p, m) for p in ('wino44', 'wino47', 'wino48') for m in ('fused', 'fused_only', 'step')] + [('x3', 'step'), ('direct', 'step'),
                                                                                                      ('direct', 'none')]


def _chain(x, wp, bp, cparts, prod, mode, cid, own=False):
    """producer conv [+ MaxPool2d(2, 2): 'fused' into the producer's launch (full map written too), 'fused_only' (pooled map only),
    'step' (ct_maxpool2d_fwd), 'none'] -> f16x2 consumer on channels [16, 48) of the result, all on one backend and the same device
    buffers.  The consumer reads the PRODUCER's slot (own: its own ct_absmax_f32 pass over exactly its slice).
    -> (consumer input slice, consumer output), on the CPU"""
    be = engine.HipBackend(DEV)
    B, Cin, H, Wd = x.shape
    C = wp.shape[0]
    P = lambda t: torch.nn.Parameter(t.to(DEV).contiguous(), requires_grad=False)
    ps = engine.ConvStep('p', [engine.ConvPart(P(wp), P(bp), None, True)], Cin, 3, 3, 1, 1, 1, 1, 'x', 0, H, Wd, 'm', 0)
    ph, pw = (H // 2, Wd // 2) if mode != 'none' else (H, Wd)
    bufs = {'x': x.to(DEV), 'm': torch.full((B, C, H, Wd), float('nan'), device=DEV),
            'q': torch.full((B, C, ph, pw), float('nan'), device=DEV)}
    kw = PRODUCERS[prod]
    be.prepare_conv(ps, bufs, B)
    ps.rt['desc'].ksplit = 0
    if 'tile' in kw:
        be.enable_wino(ps, tile=kw['tile'])
    elif 'x3' in kw:
        be.enable_x3(ps, _x3(kw['x3']))
    else:
        ps.rt['desc'].config = 1
    if mode.startswith('fused'):
        ps.rt['pool'] = (bufs['q'], ph, pw, mode == 'fused')
    slot = torch.zeros(B, LW, dtype=torch.int32, device=DEV)
    ps.rt['desc'].out_absmax = slot.data_ptr()
    be.run_conv(ps)
    if mode == 'step':
        be.run_pool(engine.PoolStep('pool', 'm', 'q', C, H, Wd, 2, 2, 0, False), bufs, B)
    src = 'm' if mode == 'none' else 'q'
    cw, cb, _, relu = cparts[0]
    cs = engine.ConvStep('c', [engine.ConvPart(P(cw), P(cb), None, relu)], 32, 3, 3, 1, 1, 1, 1, src, 16, ph, pw, 'y', 0)
    bufs['y'] = torch.full((B, cw.shape[0], ph, pw), float('nan'), device=DEV)
    ckw = _consumers()[cid][0]
    cs.rt['config'] = ckw.get('config', 0)
    be.prepare_conv(cs, bufs, B)
    cs.rt['desc'].ksplit = 0
    if 'x3' in ckw:
        be.enable_x3(cs, ckw['x3'])
    if own:
        mid = bufs[src][:, 16:48]
        lines = _lines(mid.abs().amax((1, 2, 3)).cpu())
        cs.rt['desc'].in_absmax = lines.data_ptr()
    else:
        cs.rt['desc'].in_absmax = slot.data_ptr()
    be.run_conv(cs)
    torch.cuda.synchronize()
    return bufs[src][:, 16:48].cpu(), bufs['y'].cpu()


@pytest.mark.parametrize('prod,mode', CHAINS, ids=['%s-%s' % c for c in CHAINS])
@pytest.mark.parametrize('cid', [c for c in CONSUMERS if c != 'wino47_own'])
def test_chain_through_the_producers_slot(cid, prod, mode):
    """producer conv (tile 44 / 47 / 48, bf16x3 direct, fp32 direct; out_absmax slot) -> 2x2 max-pool fused into the producer's
    launch, as a ct_maxpool2d_fwd step, or none -> f16x2 consumer reading the PRODUCER's slot through a channel slice of the pooled
    buffer (what _wire_absmax sets up in the shipped plans), against the same consumer with maxima over exactly its slice: both
    within TOL of fp64 on the consumer's actual input; with the producer's slot, image n alone and inside a batch give the same
    bits (images at three scales, so a batch-wide or misplaced line shows)."""
    g = torch.Generator().manual_seed(34)
    B, Cin, H, Wd = 3, 32, 20, 18
    x = torch.randn(B, Cin, H, Wd, generator=g) * (64.0 ** torch.arange(B).view(B, 1, 1, 1))
    wp = torch.randn(64, Cin, 3, 3, generator=g) * 0.08
    bp = torch.rand(64, generator=g) - 0.5
    wc = torch.randn(40, 32, 3, 3, generator=g) * 0.05
    cparts = [(wc, torch.rand(40, generator=g) - 0.5, None, True)]
    mid, got = _chain(x, wp, bp, cparts, prod, mode, cid)
    mid2, own = _chain(x, wp, bp, cparts, prod, mode, cid, own=True)
    assert torch.equal(mid, mid2) and torch.isfinite(mid).all()
    want = _ref64(mid, cparts)
    for n in range(B):
        assert rel_err(got[n], want[n]) < TOL and rel_err(own[n], want[n]) < TOL, (cid, n)
        alone = _chain(x[n:n + 1], wp, bp, cparts, prod, mode, cid)[1]
        assert torch.equal(alone[0], got[n]), (cid, prod, mode, n)


# Exponents at the ends of fp32's range.  x and w on grids (multiples of 2^-6 / 2^-8), so that x 2^a and w 2^b are exact in fp32
# down to a = -120, b = -118.
def _grid_data(seed):
    x, w, g = _data(seed)
    return (x * 64).round() / 64, (w * 256).round() / 256


EDGE_EXACT = [((110, 110, 110), -100), ((118, -100, 0), 0), ((-100, -100, -100), 100), ((118, 118, 118), -105), ((60, 60, 60), 60),
              ((-100, 100, 0), -5), ((118, 118, 118), -110)]


@pytest.mark.parametrize('cid', CONSUMERS)
def test_covariance_up_to_the_ends_of_fp32(cid):
    """ADVICE round 6, finding 1, fixed in the kernels: exponent_for is clamped to +-126 (was +-100) and the consumers undo the two
    scales as two exact factors (h2::unscale_for; was one float 2^-(eU + eImg)).  So conv(x 2^a, w 2^b) == conv(x, w) 2^(a + b)
    bit for bit up to where fp32 itself ends: |x| < 5 here and a <= 118, max |x| 2^120 -- the Winograd input transform (gain
    32.35, in fp32 in every form, the bf16x3 twins included) reaches 2^125.4; max |w| down to 2^-108, per-image exponents 220 apart in one batch.  With the old clamp the first, fourth and last case
    gave Inf (hi pieces beyond 65504).  The upper clamp is reached only by maxima below 2^-112 (2^-106 for the Winograd forms'
    growth): there the pieces are no longer the same bits -- the second part asks for TOL against fp64 and the bf16x3 twin at
    a = -120 (the smallest normal inputs on this grid), one step beyond the exact range.  The bf16x3 twin is finite and within TOL
    of fp64 in every case."""
    x, w = _grid_data(36)
    parts = [(w, None, None, True)]
    base = _run(cid, x, parts)
    want = _ref64(x, parts)
    assert rel_err(base, want) < TOL
    twin_kw = _consumers()[cid][2]
    for a, b in EDGE_EXACT + [((-120, -120, -120), 110)]:
        sa = 2.0 ** torch.tensor(a, dtype=torch.float64).view(3, 1, 1, 1)
        xs, ws = (x.double() * sa).float(), (w.double() * 2.0 ** b).float()
        assert torch.isfinite(xs).all() and torch.equal(xs.double(), x.double() * sa) and torch.equal(ws.double(), w.double() * 2.0 ** b)
        got = _run(cid, xs, [(ws, None, None, True)])
        twin = _run_conv(xs, [(ws, None, None, True)], 1, 1, 1, **twin_kw)
        expect = (base.double() * sa * 2.0 ** b).float()
        assert torch.isfinite(got).all() and torch.isfinite(twin).all(), (cid, a, b)
        for n in range(3):
            ref = want[n] * float(sa[n]) * 2.0 ** b
            assert rel_err(got[n], ref) < TOL and rel_err(twin[n], ref) < TOL, (cid, a, b, n)
        if (a, b) in EDGE_EXACT:
            assert torch.equal(got, expect), (cid, a, b)


@pytest.mark.parametrize('m', [8, 14, 20])
@pytest.mark.parametrize('cid', CONSUMERS)
def test_heavy_tail(cid, m):
    """One image of relu(randn) activations and ONE value 2^m times their maximum in the corner (0, 0) of channel 0: the image's
    scale follows the outlier, so every ordinary value's lo piece is rounded on a grid that is 2^m coarser.  Checked on the
    outputs the outlier cannot reach -- outside its 3x3 receptive field for the direct kernel, outside the 4x4 output tile whose
    6x6 input tile holds it for the Winograd forms (inside, fp32's own rounding of the transforms of a 2^m value is what any
    Winograd kernel shows) -- normalised by THEIR maximum.  Admissible error, from csrc/ct_f16x2.h:13-19: the scaled maximum lies in
    [2^14, 2^15) and a subnormal lo piece has quantum 2^-24, so an operand is off by at most half of 2^-38 M = 2^-39 M absolute
    (M = growth x max |x|: the maximum the exponent was taken from), where its relative error 2^-23 |x| is smaller still:
        direct:    K max|w| 2^-39 M                                  + (K + 2) 2^-24 S      K = cin kh kw, S = max (|x| * |w|)
        Winograd:  A2 cin (2 max|w|) 2^-39 (64 M)                    + A2 (K + 2) 2^-24 S   A2 = 2^7 >= ||A^T||_inf^2 = 74
    (second terms: the split's 2^-23 and fp32 accumulation of K terms, as for any fp32 kernel; 64 and 2: kGrowthBtB, kGrowthGG).
    The bound is what is asserted; the measured error and the bf16x3 twin's are printed.  Measured on an MI355X at the commit that added this test, error of the
    outside outputs' maximum at m = 8 / 14 / 20: h2: direct tiles 1.8e-7 / 1.8e-7 / 5.3e-6 (x3: twins 1.9e-7 at every m; bound
    1.3e-4 / 1.4e-4 / 4.2e-4); tile 47 7.4e-7 / 8.2e-6 / 5.2e-4, tile 48 1.2e-6 / 8.2e-6 / 5.2e-4 (twins 44 / 46 5.3e-7 / 9.9e-7
    at every m; bound 0.017 / 0.025 / 0.55).  FINDING: inside the derived bound everywhere, but at m = 20 the Winograd forms are
    5x OUTSIDE the project's 1e-4 where their bf16x3 twins are not: a per-image scale cannot keep the low bits next to a 2^20
    outlier (include/ctdet.h states it)."""
    x, w, g = _data(37, B=1)
    M0 = float(x.max())
    x[0, 0, 0, 0] = M0 * 2.0 ** m
    parts = [(w, None, None, False)]
    got = _run(cid, x, parts)[0]
    twin = _run_conv(x, parts, 1, 1, 1, **_consumers()[cid][2])[0]
    want = _ref64(x, parts)[0]
    S = F.conv2d(x.double().abs(), w.double().abs(), None, 1, 1)[0]
    wino = cid.startswith('wino')
    out = torch.ones_like(want, dtype=torch.bool)
    out[:, :4, :4] = False if wino else True
    out[:, :2, :2] = False
    K, cin, wmax, M = 64 * 9, 64, float(w.abs().max()), M0 * 2.0 ** m
    Sm = float(S[out].max())
    bound = (128 * cin * 2 * wmax * 2.0 ** -39 * 64 * M + 128 * (K + 2) * 2.0 ** -24 * Sm) if wino else \
        (K * wmax * 2.0 ** -39 * M + (K + 2) * 2.0 ** -24 * Sm)
    scale = float(want[out].abs().max())
    err = float((got.double() - want)[out].abs().max())
    err_twin = float((twin.double() - want)[out].abs().max())
    print('heavy tail %s m=%d: err %.3g twin %.3g bound %.3g (of the outside outputs\' maximum %.3g)'
          % (cid, m, err / scale, err_twin / scale, bound / scale, scale))
    assert torch.isfinite(got).all()
    assert err <= bound, (cid, m, err / scale, bound / scale)


def test_tuner_does_not_leave_stale_maxima(monkeypatch):
    """HipBackend.tune_conv timed the f16x2 forms on frozen maxima and left them in the descriptor; run_conv on
    the same buffers refilled with data 4096 x larger then split by a stale exponent (hi pieces overflow binary16)."""
    monkeypatch.setenv('CTDET_WINO_TILES', '47,48')
    g = torch.Generator().manual_seed(35)
    B, Cin, H, Wd, Cout = 2, 64, 19, 19, 96
    x = torch.randn(B, Cin, H, Wd, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (Cin * 9)) ** 0.5
    b = torch.rand(Cout, generator=g) - 0.5
    be = engine.HipBackend(DEV)
    st = engine.ConvStep('t', [engine.ConvPart(torch.nn.Parameter(w.cuda(), requires_grad=False),
                                               torch.nn.Parameter(b.cuda(), requires_grad=False), None, True)],
                         Cin, 3, 3, 1, 1, 1, 1, 'x', 0, H, Wd, 'y', 0)
    bufs = {'x': x.cuda(), 'y': torch.full((B, Cout, H, Wd), float('nan'), device=DEV)}
    be.prepare_conv(st, bufs, B)
    be.tune_conv(st)
    assert set(engine.wino_tiles(be, st)) == {47, 48}
    for tile in (48, 48):                                   # after tune_conv, then after a single _time_conv
        be.enable_wino(st, tile=tile)
        big = x * 4096.0
        bufs['x'].copy_(big)
        bufs['y'].fill_(float('nan'))
        be.run_conv(st)
        torch.cuda.synchronize()
        got = bufs['y'].cpu()
        assert torch.isfinite(got).all(), tile
        assert rel_err(got, _ref64(big, [(w, b, None, True)])) < TOL, tile
        bufs['x'].copy_(x)
        be._time_conv(st)                                   # times on x; the next launch sees other data again
