"""tests/conv_grad_cases.py without a GPU: the float64 reference agrees with torch's fp32 autograd, the table still holds every
edge case tests/test_gpu_conv_grad.py is there for (per kernel class of the weight gradient, per tile height of the data
gradient), the reductions stay short, and a single dropped input pixel moves every row's reference by far more than the bounds
the GPU tests assert -- so those assertions cannot pass a kernel that loses one term."""
import functools

import pytest
import torch

import conv_grad_cases as G
from conftest import rel_err

ALL = G.WGRAD_CASES + G.DGRAD_CASES
IDS = ['%s-%s' % (c.kind, c.name) for c in ALL]


@functools.lru_cache(maxsize=None)
def _problem(case):
    inp = G.make_inputs(case)
    return inp, G.ref64(inp.x(case), inp.parts, inp.dz(case), case)


@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_reference_agrees_with_fp32_autograd(case):
    inp, (dw, dx) = _problem(case)
    dw32, dx32 = G.grad32(inp.x(case), inp.parts, inp.dz(case), case)
    assert dw.dtype == dx.dtype == torch.float64
    assert dw.shape == (case.cout, case.cin, case.kh, case.kw) and dx.shape == (case.B, case.cin, case.H, case.W)
    assert rel_err(dw32, dw) < 1e-5 and rel_err(dx32, dx) < 1e-5, (case.name, rel_err(dw32, dw), rel_err(dx32, dx))


@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_one_dropped_pixel_shows(case):
    """Corner pixel (0, 0) of image 0 zeroed in the kernel's gathered operand (x for the weight gradient: every dw element loses
    at most one term; dZ for the data gradient): the float64 result moves by more than 1e-3 of its maximum."""
    inp, (dw, dx) = _problem(case)
    if case.kind == 'w':
        x = inp.x(case).clone()
        x[0, :, 0, 0] = 0
        got = G.ref64(x, inp.parts, inp.dz(case), case)[0]
        assert rel_err(got, dw) > 1e-3, (case.name, rel_err(got, dw))
    else:
        dz = inp.dz(case).clone()
        dz[0, :, 0, 0] = 0
        got = G.ref64(inp.x(case), inp.parts, dz, case)[1]
        assert rel_err(got[0], dx[0]) > 1e-3, (case.name, rel_err(got[0], dx[0]))


def test_reduction_lengths():
    for c in ALL:
        if c.kind == 'w' and c.name.rsplit('_', 1)[0] in G.RED_CAP_EXEMPT:
            assert c.reduction == 4 * 38 * 38       # the many-splits row and nothing longer
            continue
        assert c.reduction <= G.RED_CAP, (c.kind, c.name, c.reduction)


def test_rows_are_launches_the_kernels_take():
    names = set()
    for c in ALL:
        assert (c.kind, c.name) not in names
        names.add((c.kind, c.name))
        assert c.kind in ('w', 'd') and c.B > 0 and c.oh > 0 and c.ow > 0
        assert (c.kh, c.kw) in ((3, 3), (1, 1), (1, 3), (3, 1), (4, 4)) and c.stride in (1, 2)
        assert 0 <= c.x_coff and c.x_coff + c.cin <= c.x_ctot
        assert 0 <= c.dz_coff and c.dz_coff + c.zc <= c.dz_ctot
        if c.kind == 'w':
            assert len(c.parts) == 1 and not (c.zero or c.sliced or c.acc or c.splitk)
            assert c.tapmajor or c.cin in G.GENERIC_CINS, c.name
        else:
            assert c.x_slice is None and c.cin in G.DGRAD_CINS and c.zc in G.DGRAD_ZCS + (32,), c.name
            assert 0 <= c.out_coff and c.out_coff + c.cin < c.out_ctot, c.name      # the buffer is wider than the slice
            if c.x3:                                                                 # both k-step lengths of ct_conv2d_x3_fwd
                assert c.zc % 32 == 0, c.name
    for cin in G.GENERIC_CINS:
        assert any(c.cin == cin for c in G.WGRAD_CASES), cin
    for cin in G.DGRAD_CINS:
        assert any(c.cin == cin for c in G.DGRAD_CASES), cin
    for zc in G.DGRAD_ZCS:
        assert any(c.zc == zc and not c.zero for c in G.DGRAD_CASES), zc


def _is(case, prop):
    """What a row IS, not what it is labelled."""
    c = case
    k33p1 = (c.kh, c.kw, c.ph, c.pw, c.dil) == (3, 3, 1, 1, 1)
    return {
        'pad1_19': k33p1 and c.stride == 1 and (c.H, c.W) == (19, 19),
        'b3_19x17': k33p1 and c.stride == 1 and (c.B, c.H, c.W) == (3, 19, 17) and
        (c.kind == 'd' or (c.cout == 70 and c.cin in (128, 72))),
        's2_odd': k33p1 and c.stride == 2 and (c.H, c.W) == (19, 19),
        's2_even': k33p1 and c.stride == 2 and (c.H, c.W) == (10, 10),
        'd6_19': (c.kh, c.kw, c.ph, c.pw, c.dil, c.stride, c.H, c.W) == (3, 3, 6, 6, 6, 1, 19, 19),
        'd6_5x5': (c.kh, c.kw, c.ph, c.pw, c.dil, c.stride, c.H, c.W) == (3, 3, 6, 6, 6, 1, 5, 5),
        'k1x3': (c.kh, c.kw, c.ph, c.pw, c.H, c.W) == (1, 3, 0, 1, 12, 11),
        'k3x1': (c.kh, c.kw, c.ph, c.pw, c.H, c.W) == (3, 1, 1, 0, 12, 11),
        'k4x4': (c.kh, c.kw, c.ph, c.pw, c.H, c.W, c.oh * c.ow) == (4, 4, 1, 1, 2, 2, 1),
        'k1x1_s1': (c.kh, c.kw, c.ph, c.pw, c.stride) == (1, 1, 0, 0, 1),
        'k1x1_s2': (c.kh, c.kw, c.ph, c.pw, c.stride) == (1, 1, 0, 0, 2),
        'pad0_5x5': (c.kh, c.kw, c.ph, c.pw, c.dil, c.H, c.W) == (3, 3, 0, 0, 1, 5, 5),
        'one_pixel': k33p1 and (c.H, c.W) == (1, 1),
        'slices': c.x_slice == (80, 9) and c.dz_slice == (64, 7) and c.cout == 48,
        'b4_38x38': (c.B, c.H, c.W, c.cout) == (4, 38, 38, 64),
        'tb2': c.tb2,
        'parts': len(c.parts) > 1,
        'zero_part': c.parts == (20, 6) and c.zero == 6,
        'slice': c.sliced and (c.out_coff, c.out_ctot) == (5, c.cin + 11),
        'acc': c.acc,
        'in_coff': c.kind == 'd' and c.dz_coff != 0,
        'splitk': c.splitk,
    }[prop]


def test_table_keeps_every_edge_case():
    for c in ALL:
        for prop in set(G.REQUIRED_W if c.kind == 'w' else G.REQUIRED_D):
            assert (prop in c.props) == bool(_is(c, prop)), (c.kind, c.name, prop)
    # weight gradient: every property once on the tap-major kernel and once on the generic one
    for prop, least in G.REQUIRED_W.items():
        for tm in (True, False):
            rows = [c.name for c in G.WGRAD_CASES if prop in c.props and c.tapmajor == tm]
            assert len(rows) >= least, (prop, 'tapmajor' if tm else 'generic', rows)
    tb = [c for c in G.WGRAD_CASES if c.tb2]
    assert any(c.cin % 128 == 0 for c in tb) and any(c.cin % 64 for c in tb)
    b3 = [c for c in G.WGRAD_CASES if 'b3_19x17' in c.props]
    assert all(c.reduction == 969 and 969 % 64 == 9 and c.cout % 64 == 6 for c in b3)
    # data gradient: over the table ...
    for prop, least in G.REQUIRED_D.items():
        rows = [c.name for c in G.DGRAD_CASES if prop in c.props]
        assert len(rows) >= least, (prop, rows)
    # ... and what depends on the tile height, for every height: a last tile with dead rows behind a full one, a single tile with
    # dead rows, and each of these with the epilogue forms that read or skip rows (slice, accumulate)
    for bm in G.TILE_ROWS:
        second = [c for c in G.DGRAD_CASES if c.cin > bm and c.cin % bm]
        single = [c for c in G.DGRAD_CASES if c.cin < bm]
        assert second and single, bm
        for prop in ('slice', 'acc', 'parts', 'splitk'):
            assert any(prop in c.props for c in second + single), (bm, prop)
        assert any('acc' in c.props and 'slice' in c.props for c in second), bm
    # pixel counts ragged against both tile widths; zc 34 leaves a k-step tail at every channels-per-step of 3x3, 1x3 / 3x1 and 1x1
    assert any(c.npix % 64 and c.npix % 128 and c.npix > 128 for c in G.DGRAD_CASES)
    assert any(c.zc == 34 for c in G.DGRAD_CASES if (c.kh, c.kw) == (3, 3))
    assert any(c.zc == 34 for c in G.DGRAD_CASES if c.kh * c.kw == 3)
    assert any(c.zc == 34 for c in G.DGRAD_CASES if c.kh * c.kw == 1)
    sk = {c.name for c in G.DGRAD_CASES if c.splitk}
    assert {'d6_5x5', 'k4x4', 'k1x1_s2'} <= sk and any(len(c.parts) > 1 for c in G.DGRAD_CASES if c.splitk)
    assert all(G.ksplit_floats(c) == 16 * c.cin * c.B * c.H * c.W for c in G.DGRAD_CASES)
    # the bf16x3 route gets the rows its own test lacks
    x3 = [c for c in G.DGRAD_CASES if c.x3]
    for prop in ('parts', 'zero_part', 's2_even', 'acc', 'slice'):
        assert any(prop in c.props for c in x3), prop


def test_descriptors_are_the_engines():
    buf = torch.zeros(1)
    for c in G.WGRAD_CASES:
        d = G.wgrad_desc(c, buf.expand(c.B, c.x_ctot, c.H, c.W))
        assert (d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff) == (c.B, c.cin, c.H, c.W, c.x_ctot, c.x_coff)
        assert (d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil, d.oh, d.ow) == \
            (c.cout, c.kh, c.kw, c.stride, c.ph, c.pw, c.dil, c.oh, c.ow)
        assert d.transposed == 0 and not d.out and not d.res
    for c in G.DGRAD_CASES:
        out = buf.expand(c.B, c.out_ctot, c.H, c.W)
        d = G.dgrad_desc(c, buf.expand(c.B, c.dz_ctot, c.oh, c.ow), out, buf, buf, mpad=32, kpad=64, ksplit=-1, ksplit_ws=buf)
        assert (d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff) == (c.B, c.zc, c.oh, c.ow, c.dz_ctot, c.dz_coff)
        assert (d.cout, d.oh, d.ow, d.transposed, d.m_pad, d.k_pad) == (c.cin, c.H, c.W, 1, 32, 64)
        assert (d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil) == (c.kh, c.kw, c.stride, c.ph, c.pw, c.dil)
        assert (d.out_ctot, d.out_coff, d.res_ctot, d.res_coff, d.res_scale) == (c.out_ctot, c.out_coff, c.out_ctot, c.out_coff, 1.0)
        assert (d.res == d.out) == c.acc and (d.ksplit, d.ksplit_ws_floats) == (-1, 1)
