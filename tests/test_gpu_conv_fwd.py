"""Every forward convolution path, row by row, against the float64 reference of the whole fused step (tests/conv_fwd_cases.py):

  D  ct_conv2d_fwd: the heuristic and every tile configuration ('valu' on the 3-channel row);
  X  ct_conv2d_x3_fwd, the bf16x3 configurations whose k-step divides cin (the others must refuse);
  H  its f16x2 twins -- on the rows the pointwise rule takes, once with ct_conv_x3_pointwise_enable(1) and once with (0);
  W  the Winograd forms 2, 4, 23, 44, 46, 47, 48 through Form.config (dilated rows: 44 and 47).

Every launch goes through engine.HipBackend (test_gpu_absmax._launch) into NaN-filled buffers and is checked for: the error of EACH
IMAGE on its own (rel_err of the slice or segment against that image's float64 reference) below the hard bound 1e-4 and the tight
bound of its family (conv_fwd_cases: max(8 e32, 2^-20) for D, the dual-accumulator X configurations and H; the form's deep-shape
bound scaled by ew32(row) / ew32_deep for W; the two single-accumulator X configurations, which the engine cannot select, get the
hard bound only); finite output; NaN left outside an output slice or head segment; the same bits from a second launch (the
forward has no atomics); and, for the fused pool, the pooled map equal to max_pool2d of the full one where that is written and held
to the same bounds against the pooled reference.  Every launch prints one `FWD` line before it asserts (`pytest -s`).

Measured on an MI355X: 564 launches over the 44 rows, none above its tight bound, every second launch bit-equal.  Per family the
largest per-image err and its row; the largest err / base (base = e32 for D / X / H, ew32(row, m_f) for W) and the largest
err / tight bound (DESIGN.md section 6 has the same table):

  family                                    launches  largest err             err / base              err / tight
  D   fp32 MFMA, heuristic + 8 tiles           195    1.34e-6 splitk, ks 0    7.38 same               0.92 same
      ... every other launch                           1.08e-6 slices          4.53 splitk, ks 2       0.56 splitk, ks 2
  D   valu                                       1    1.70e-7 img3            1.00                    0.12
  X   bf16x3, two accumulators (4 configs)      90    4.10e-7 splitk, ks 0    2.25 same               0.28 same
  X   bf16x3, one accumulator (2 configs)       46    8.62e-7 heads, ks 0     4.44 splitk, ks 0       hard bound only
  H   f16x2 (4 configs), pointwise on / off    102    3.23e-7 heads, ks 0     1.74 splitk, ks 0       0.22 same
  W2  F(2x2,3x3) fp32                           17    3.45e-7 b3_19x19        1.47 cin8               0.19 cin8
  W4  F(4x4,3x3) fp32, channel split 2 / 5 / -1 20    1.39e-6 b3_19x19        1.24 pool_b8_3x3        0.04 pool_b8_3x3
  W23 F(2x2,3x3) bf16x3                         15    2.48e-7 b3_19x19        1.12 pool_floor_only    0.25 pool_floor_only
  W44 three-kernel bf16x3                       21    7.79e-7 img1_small      1.06 pool_b8_3x3        0.29 pool_b8_3x3
  W46 fused bf16x3                              15    1.02e-6 b3_19x19        1.21 pool_b8_3x3        0.17 pool_b8_3x3
  W47 three-kernel f16x2                        24    1.12e-6 tiles300_cout136 1.26 d6                0.35 d6
  W48 fused f16x2                               18    1.01e-6 parts           1.77 pool_b8_3x3        0.25 pool_b8_3x3

e32 is 1.6-4.7e-7 over the direct rows, ew32(2) 1.6-3.9e-7 and ew32(4) 2.6e-7-1.7e-6 over the Winograd rows (ew32_deep 4.7e-7 /
1.9e-6).  The eight fp32 tiles give the same figures on every row (one sequential fp32 sum per output in the same k order whatever
the tile), and that sum is what brings D within 8 % of its bound on the one long row: splitk has 2016 terms, unsplit 1.34e-6 = 7.38
e32, and every split shortens it (ks 2: 8.2e-7, 3: 3.9e-7, 1000 and -1: 1.8-2.1e-7).  A CPU restatement with ONE float32 accumulator per
output over the 2016 products gives 1.46e-6 (channel-major order) / 1.13e-6 (tap-major): the level is that of the form, not of a
lost term, and it stays inside the factor 8.  The pointwise kernel gives the generic kernel's errors on all 12 (row, configuration)
pairs; in_absmax given / unset give the same per-image errors on forms 47 and 48, and lines 2^10 too large move image 0 by 2e-8.
Two mutations of a scratch copy of conv_x3_f32 were run on the device: the (mid, mid) piece product of bf16x3 dropped everywhere
(errors 0.7-1.9e-5, 28-106 e32) fails all 18 rows that run X here and, of the earlier tests, only the five large stride-1 rows of
test_gpu_x3.py's float64 gate; dropped at stride 2 only, it fails the rows s2 and 1x1s2 here and no earlier test."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err          # noqa: F401  (first: it puts the package on sys.path)
import conv_fwd_cases as G
from ctdet import _lib
from ctdet.wino_forms import FORMS
from test_gpu_absmax import LW, _kernels, _launch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('the gpu tests need a HIP device; none visible')


def _ids(cases):
    return [c.name for c in cases]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(case, **kernel):
    """One launch of a row -> what test_gpu_absmax._launch returns."""
    inp = G.make_inputs(case)
    return _launch(inp.x_buf, list(inp.parts), case.stride, (case.ph, case.pw), case.dil, res=inp.res,
                   res_scale=case.res_scale if case.res_scale is not None else 1.0, cin_off=case.x_coff, cin=case.cin,
                   out_ctot=case.out_ctot, out_coff=case.out_coff, pool=case.pool, segs=G.segments(case) if case.segs else None,
                   track=False, **kernel)


def _same_bits(a, b):
    for k in ('y', 'pooled'):
        if a[k] is not None and not torch.equal(_bits(a[k]), _bits(b[k])):
            return False
    return all(torch.equal(_bits(a['flat'][n]), _bits(b['flat'][n])) for n in a['flat'])


def _check(case, fam, cname, base, tight, variant='', **kernel):
    """Launch twice, print the figures, assert.  base: e32 or ew32 of the row; tight: None = hard bound only.  -> max error"""
    ref = G.ref64(case)
    got, again = _run(case, **kernel), _run(case, **kernel)
    who = (fam, cname, case.name, variant)
    problems = []
    if case.segs:
        errs = [0.0] * case.B
        for (n, c0, c1, sbase, size) in G.segments(case):
            flat, cnt = got['flat'][n], ref.flat[n].shape[1]
            assert flat.shape == (case.B, size), who
            if not (torch.isnan(flat[:, :sbase]).all() and torch.isnan(flat[:, sbase + cnt:]).all()):
                problems.append('floats outside segment %s were written' % n)
            seg = flat[:, sbase:sbase + cnt]
            if not torch.isfinite(seg).all():
                problems.append('segment %s is not finite' % n)
            errs = [max(a, b) for a, b in zip(errs, G.image_errors(torch.nan_to_num(seg), ref.flat[n]))]
        # the three segments of an image share one scale here (one conv, weights of one distribution): the worst of the three
    else:
        y = got['y']
        lo, hi = case.out_coff, case.out_coff + case.cout
        if not (torch.isnan(y[:, :lo]).all() and torch.isnan(y[:, hi:]).all()):
            problems.append('channels outside the slice were written')
        errs = None
        if case.pool is None or case.pool[1]:
            if not torch.isfinite(y[:, lo:hi]).all():
                problems.append('the output is not finite')
            errs = G.image_errors(torch.nan_to_num(y[:, lo:hi]), ref.y)
        elif not torch.isnan(y).all():
            problems.append('the full-resolution map was written')
        if case.pool is not None:
            p = got['pooled']
            assert p.shape == ref.pooled.shape, who
            if not torch.isfinite(p).all():
                problems.append('the pooled map is not finite')
            perrs = G.image_errors(torch.nan_to_num(p), ref.pooled)
            errs = perrs if errs is None else [max(a, b) for a, b in zip(errs, perrs)]
            if case.pool[1] and not torch.equal(F.max_pool2d(y, 2, 2, 0, ceil_mode=case.pool[0]), p):
                problems.append('pooled != max_pool2d(full)')
    worst = max(errs)
    print('FWD %s cfg=%s row=%s%s err %s base %.3g ratio %.2f tight %s' %
          (fam, cname, case.name, ' ' + variant if variant else '', ' '.join('%.3g' % e for e in errs), base, worst / base,
           '%.3g' % tight if tight is not None else '-'))
    assert not problems, who + (problems,)
    assert worst < G.HARD, who + (errs,)
    if tight is not None:
        assert worst < tight, who + (errs, base, tight)
    assert _same_bits(got, again), who + ('two launches differ',)
    return worst


# ------------------------------------------------------------------------------------------------ direct kernels
@pytest.fixture
def pointwise(request):
    """The switch of ct_conv_x3_pointwise_enable; the restore is registered BEFORE the switch can be turned (a leaked 0 would keep
    every later test of the process off the pointwise kernel)."""
    lib, prev = _lib.lib(), []
    request.addfinalizer(lambda: lib.ct_conv_x3_pointwise_enable(prev[0]) if prev else None)

    def turn(on):
        was = lib.ct_conv_x3_pointwise_enable(int(on))
        if not prev:
            prev.append(was)
    return turn


def _direct_launches(case):
    """(family, configuration name, keyword arguments of _launch, tight bound applies) of every D / X / H launch form that takes
    the row, split-K left to the caller."""
    out = []
    for tag, kw in _kernels(case.cin, case.kh, case.kw, case.stride, case.ph, case.dil, case.cout, splitk=False, wino=False):
        if tag.startswith('direct:'):
            fam, cname, tight = 'D', tag[len('direct:'):], True
        else:
            fam, cname, tight = ('H' if tag.startswith('h2:') else 'X'), tag, tag.endswith('d')
        if fam in case.forms:
            out.append((fam, cname, kw, tight))
    return out


@pytest.mark.parametrize('case', G.DIRECT, ids=_ids(G.DIRECT))
def test_direct_row_every_launch_form_vs_float64(case, pointwise):
    lib = _lib.lib()
    e32, tight = G.e32(case), G.tight_direct(case)
    launches = _direct_launches(case)
    fams = {f for f, *_r in launches}
    assert fams == set(case.forms), (case.name, fams)
    if case.cin == 3:
        assert any(c == 'valu' for _f, c, *_r in launches)
    for j in range(lib.ct_conv_x3_num_configs()) if 'X' in case.forms else ():
        if case.cin % lib.ct_conv_x3_config_bk(j):        # k-step must divide cin: refused loudly
            with pytest.raises(_lib.CtdetError, match='not a multiple'):
                _run(case, x3=j, ksplit=0)
    ran = 0
    for fam, cname, kw, tightens in launches:
        if case.ksplits and fam == 'D' and 'splitk' in case.props and not case.segs and kw['config'] not in G.KSPLIT_CONFIGS:
            continue
        for ks in case.ksplits or (0,):
            modes = (('pw=on', 1), ('pw=off', 0)) if fam == 'H' and case.pointwise else (('', None),)
            for mtag, on in modes:
                if on is not None:
                    pointwise(on)
                variant = ' '.join(t for t in ('ks=%d' % ks if case.ksplits else '', mtag) if t)
                _check(case, fam, cname, e32, tight if tightens else None, variant, ksplit=ks, **kw)
                ran += 1
    assert ran >= len(launches)


# ------------------------------------------------------------------------------------------------ Winograd forms
def _lines(case, loose):
    """The per-image maxima of |x| in the line layout of ct_conv_desc.in_absmax, from ct_absmax_f32; loose: every line x 2^10 (an
    upper bound is enough: csrc/ct_f16x2.h)."""
    import ctypes as C
    x = G.make_inputs(case).x(case).contiguous().to(DEV)
    lines = torch.zeros(case.B, LW, dtype=torch.int32, device=DEV)
    per = case.cin * case.H * case.W
    _lib.check(_lib.lib().ct_absmax_f32(x.data_ptr(), case.B, per, per, lines.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'ct_absmax_f32')
    torch.cuda.synchronize()
    assert torch.equal(lines[:, 0].contiguous().view(torch.float32), x.reshape(case.B, -1).abs().amax(1))
    if loose:
        lines[:, 0] = (lines[:, 0].contiguous().view(torch.float32) * 1024.0).view(torch.int32)
    return lines


@pytest.mark.parametrize('case', G.WINO, ids=_ids(G.WINO))
def test_wino_row_every_form_vs_float64(case):
    assert sorted(FORMS) == list(G.ALL_W)
    for code in case.forms:
        f = FORMS[code]
        base, tight = G.ew32(case, G.WINO_M[code]), G.tight_wino(case, code)
        for ks in case.ksplits or (None,):
            kw = dict(config=f.config) if ks is None else dict(config=f.config, ksplit=ks)
            _check(case, 'W%d' % code, f.name, base, tight, '' if ks is None else 'ks=%d' % ks, **kw)
        if f.h2:
            # where the maxima come from: the caller's exact lines, an upper bound 2^10 above them, or none (form 47 takes them
            # inside its launch, the engine runs ct_absmax_f32 in front of form 48)
            for amax in case.amax:
                lines = None if amax == 'unset' else _lines(case, amax == 'loose')
                kw = dict(config=f.config) if lines is None else dict(config=f.config, in_absmax=lines)
                _check(case, 'W%d' % code, f.name, base, tight, 'amax=' + amax, **kw)
