"""The reference side of tests/test_gpu_conv_fwd.py, checked without a GPU (tests/conv_fwd_cases.py): the row table holds every
property it is there for, for every kernel family; the float32 Winograd restatement, evaluated in float64, IS the reference
(padding, cropping, the sub-lattices of a dilated layer); float32 arithmetic itself stays far below the bounds; and the tight bound
of every direct row rejects an operand that lost its lowest bfloat16 piece.  `pytest -s` prints the figures of every row."""
import pytest
import torch

import conv_fwd_cases as G


def _ids(cases):
    return ['%s-%s' % (c.family, c.name) for c in cases]


def test_rows_are_unique_and_well_formed():
    assert len({(c.family, c.name) for c in G.CASES}) == len(G.CASES)
    for c in G.CASES:
        assert len(c.part_relus) == len(c.parts) and c.oh >= 1 and c.ow >= 1, c.name
        assert c.x_coff + c.cin <= c.x_ctot and c.out_coff + c.cout <= c.out_ctot, c.name
        if c.family == 'wino':
            assert (c.kh, c.kw, c.stride) == (3, 3, 1) and c.ph == c.pw == c.dil, c.name
            assert set(c.forms) <= set(G.ALL_W) and c.cin % (8 if set(c.forms) <= set(G.F32_W) else 16) == 0, c.name
            assert c.dil == 1 or set(c.forms) <= set(G.SPLIT_W), c.name
        else:
            assert set(c.forms) <= set(G.DIRECT_FAMILIES), c.name
            assert 'X' not in c.forms and 'H' not in c.forms or c.cin % 16 == 0, c.name
        assert set(c.props) <= set(G.REQUIRED), (c.name, c.props)
        assert ('pointwise' in c.props) == (c.family == 'direct' and 'H' in c.forms and c.pointwise), c.name
        assert not c.segs or not any(c.part_relus), c.name


@pytest.mark.parametrize('prop', sorted(G.REQUIRED))
def test_every_required_property_has_its_rows(prop):
    families, least = G.REQUIRED[prop]
    for fam in families:
        rows = G.rows_with(prop, fam)
        assert len(rows) >= least, (prop, fam, [c.name for c in rows])


def test_the_properties_are_what_the_shapes_say():
    for c in G.CASES:
        p = set(c.props)
        assert ('s2' in p) == (c.stride == 2) and ('dilated' in p) == (c.dil > 1) and ('nonsquare' in p) == (c.kh != c.kw), c.name
        assert ('bn' in p) == (c.epi == 'bn') and ('res' in p) == (c.res_scale is not None), c.name
        assert ('floor' in p) == (len(set(c.part_relus)) == 2) and ('segs' in p) == c.segs, c.name
        assert ('in_slice' in p) == (c.x_slice is not None) and ('out_slice' in p) == (c.out_slice is not None), c.name
        assert ('img_scale' in p) == (c.img1_scale is not None) and ('splitk' in p) == any(k != 0 for k in c.ksplits), c.name
        assert ('pool_ceil' in p) == bool(c.pool and c.pool[0]) and ('pool_floor' in p) == bool(c.pool and not c.pool[0]), c.name
        assert ('pooled_only' in p) == bool(c.pool and not c.pool[1]), c.name
        assert ('one_pixel' in p) == (c.oh * c.ow == 1), c.name
        if 'empty_sublattice' in p:
            assert c.dil > min(c.H, c.W), c.name
        for a in ('given', 'loose', 'unset'):
            assert ('amax_' + a in p) == (a in c.amax), c.name
    assert all(c.cout % 32 or c.cout % 64 for c in G.CASES if 'ragged_block' in c.props)


def test_bn_draw_is_the_one_of_the_gpu_tests():
    from test_gpu_kernels import _bn
    a, b = _bn(7, torch.Generator().manual_seed(3)), G._bn(7, torch.Generator().manual_seed(3))
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize('case', G.WINO, ids=_ids(G.WINO))
def test_wino_restatement_in_float64_is_the_reference(case):
    """Pins the zero-padding to a multiple of m, the crop and the sub-lattice restatement of the dilated rows."""
    ref = G.ref64(case).y
    for m in (2, 4):
        assert G.rel_err(G.wino32(case, m, torch.float64), ref) < 1e-10, (case.name, m)


@pytest.mark.parametrize('case', G.CASES, ids=_ids(G.CASES))
def test_float32_itself_is_far_below_the_bounds(case):
    ref = G.ref64(case)
    assert torch.isfinite(ref.y).all() and ref.y.shape == (case.B, case.cout, case.oh, case.ow)
    if case.pool:
        assert ref.pooled.shape[2:] == case.pooled_hw
    e32 = G.e32(case)
    line = 'ROW %s/%s terms %d e32 %.3g' % (case.family, case.name, case.terms, e32)
    assert 0 < e32 < 1e-5, (case.name, e32)
    if case.family == 'direct':
        line += ' tight %.3g' % G.tight_direct(case)
    else:
        for m in (2, 4):
            ew = G.ew32(case, m)
            assert 0 < ew < 1e-5, (case.name, m, ew)
            line += ' ew32(%d) %.3g' % (m, ew)
        line += ' tight ' + ' '.join('f%d %.3g' % (code, G.tight_wino(case, code)) for code in case.forms)
    print(line)


def test_deep_shape_of_the_winograd_bounds():
    for m in (2, 4):
        ew = G.ew32_deep(m)
        print('DEEP ew32_deep(%d) %.3g' % (m, ew))
        assert 1e-7 < ew < 1e-5, (m, ew)
    assert G.ew32_deep(4) > G.ew32_deep(2)          # F(4x4,3x3)'s transforms amplify more
    assert sorted(G.WINO_BOUND) == sorted(G.WINO_M) == list(G.ALL_W)


@pytest.mark.parametrize('case', G.DIRECT, ids=_ids(G.DIRECT))
@pytest.mark.parametrize('operand', ['x', 'w'])
def test_tight_bound_rejects_a_dropped_low_piece(case, operand):
    """One operand truncated to 16 significand bits (a bf16x3 value without its lowest piece), everything else in float64: the
    error of the worst image must exceed the row's tight bound, or the row is too forgiving to be in the table."""
    inp = G.make_inputs(case)
    x, parts = inp.x(case), inp.parts
    if operand == 'x':
        x = G.drop_low_piece(x)
    else:
        parts = tuple((G.drop_low_piece(w), b, bn, relu) for (w, b, bn, relu) in parts)
    got = G.fused_step(x, parts, case, inp.res, torch.float64)
    errs = G.image_errors(got, G.ref64(case).y)
    tight = G.tight_direct(case)
    print('DROP %s %s err %s tight %.3g ratio %.1f' % (case.name, operand, ' '.join('%.3g' % e for e in errs), tight, max(errs) / tight))
    assert tight < G.HARD
    assert max(errs) < G.HARD           # ... while the 1e-4 contract alone does not see it
    assert max(errs) > tight, (case.name, operand, errs, tight)
