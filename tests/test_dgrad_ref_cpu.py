"""tests/dgrad_ref.py without a GPU: the mirrored forward weight really computes the data gradient (so the GPU test's mirror
launch is the same convolution as its *_dgrad launch), every row of the case table is a launch TrainEngine could make, and the
table still holds every edge case tests/test_gpu_wino_dgrad.py is there for."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import dgrad_ref as R
from ctdet import _lib
from ctdet.wino_forms import FORMS


@pytest.mark.parametrize('B,parts,cin,H,W,dil', [
    (2, (16,), 24, 13, 10, 1), (2, (16,), 24, 7, 9, 2), (1, (16,), 32, 19, 19, 6), (1, (16,), 16, 5, 5, 6),
    (2, (40, 24), 40, 9, 11, 1), (2, (20, 12), 8, 19, 17, 6),
], ids=['d1', 'd2', 'd6', 'd6_5x5', 'two_parts_d1', 'two_parts_d6'])
def test_mirrored_forward_is_the_data_gradient(B, parts, cin, H, W, dil):
    g = torch.Generator().manual_seed(H * 100 + dil)
    ws = [torch.randn(c, cin, 3, 3, generator=g) for c in parts]
    dy = torch.randn(B, sum(parts), H, W, generator=g)
    want = R.ref_dgrad64(ws, dy, dil)
    wm = R.mirrored_weights(ws)
    assert wm.shape == (cin, sum(parts), 3, 3) and wm.is_contiguous()
    got = F.conv2d(dy.double(), wm.double(), None, 1, dil, dil)
    assert want.dtype == torch.float64 and got.shape == want.shape == (B, cin, H, W)
    assert float((got - want).abs().max()) <= 1e-11 * max(float(want.abs().max()), 1.0)
    # the parts are concatenated on dim 0: one part or two, the same gradient
    assert torch.equal(R.ref_dgrad64([torch.cat(ws, 0)], dy, dil), want)


def test_every_row_is_a_launch_the_engine_makes():
    """train_engine.py: zc % 8 == 0 (forms 2, 4), zc % 16 == 0 (44, 46, 47, 48), 3x3 / stride 1 / pad = dilation, dilated layers
    on the three-kernel forms only -- and FORMS has the entry points the GPU test goes through."""
    names = set()
    for c in R.CASES + R.DEEP:
        assert c.name not in names, c.name
        names.add(c.name)
        assert c.forms and set(c.forms) <= set(R.FORM_CODES), c.name
        assert all(p > 0 for p in c.parts) and c.cin > 0 and c.B > 0 and c.H > 0 and c.W > 0 and 1 <= c.dil <= 8, c.name
        assert 0 <= c.out_coff and c.out_coff + c.cin < c.out_ctot, c.name          # the buffer is wider than the slice
        assert c.amax in ('given', 'loose', 'null'), c.name
        assert c.img1_scale is None or c.B >= 2, c.name
        for code in c.forms:
            assert c.zc % (8 if code in R.F32_FORMS else 16) == 0, (c.name, code)
            assert FORMS[code].pack_dgrad and FORMS[code].split == (code in R.SPLIT_FORMS) and FORMS[code].h2 == (code in R.H2_FORMS)
            if c.dil > 1 and not c.acc:
                assert code in R.SPLIT_FORMS, (c.name, code)
            if c.amax != 'given':
                assert code in R.H2_FORMS, (c.name, code)
        dz = torch.zeros(c.B, c.zc, 1, 1).expand(c.B, c.zc, c.H, c.W)       # shapes only: nothing is launched
        out = torch.zeros(1)
        d = R.dgrad_desc(dz, c.cin, c.dil, torch.zeros(c.B, c.out_ctot, 1, 1).expand(c.B, c.out_ctot, c.H, c.W), c.out_coff, out, out,
                         acc=c.acc)
        assert (d.pad_h, d.pad_w, d.dil, d.stride, d.kh, d.kw, d.transposed) == (c.dil, c.dil, c.dil, 1, 3, 3, 0)
        assert (d.cin, d.in_ctot, d.in_coff, d.cout, d.oh, d.ow) == (c.zc, c.zc, 0, c.cin, d.h, d.w)
        assert (d.res_ctot, d.res_coff, d.res_scale) == (d.out_ctot, d.out_coff, 1.0) and (d.res == d.out) == c.acc


def test_library_predicates_agree_with_the_table():
    """ct_conv_*_supported (host code: no device needed) on every row's descriptor says what the GPU test expects of it."""
    lib = _lib.lib()
    buf = torch.zeros(1)
    for c in R.CASES + R.DEEP:
        dz = buf.expand(c.B, c.zc, c.H, c.W)
        out = buf.expand(c.B, c.out_ctot, c.H, c.W)
        d = R.dgrad_desc(dz, c.cin, c.dil, out, c.out_coff, buf, buf, acc=c.acc, lib=lib)
        for code in c.forms:
            for sym in R.SUPPORTED[code]:
                assert bool(getattr(lib, sym)(C.byref(d))) == R.expect_supported(c, code), (c.name, code, sym)


def test_table_keeps_every_edge_case():
    for prop, (forms, least) in R.REQUIRED.items():
        for code in forms:
            rows = [c.name for c in R.CASES + R.DEEP if prop in c.props and code in c.forms]
            assert len(rows) >= least, (prop, code, rows)
    by = {c.name: c for c in R.CASES + R.DEEP}
    # the properties are what the rows ARE, not only what they are labelled
    for c in by.values():
        P = set(c.props)
        assert ('slice' in P) == (c.sliced and c.dil == 1), c.name
        assert ('dilated_slice' in P) == (c.sliced and c.dil > 1 and not c.acc), c.name
        assert ('acc' in P) == (c.acc and c.dil == 1), c.name
        assert ('dilated' in P) == (c.dil > 1 and not c.acc), c.name
        assert ('refused' in P) == (c.dil > 1 and c.acc), c.name
        assert ('parts' in P or 'dilated_parts' in P) == (len(c.parts) > 1), c.name
        assert ('img_scale' in P) == (c.img1_scale is not None), c.name
        assert ('empty_sublattice' in P) == (c.dil > 1 and not c.acc and (c.H < c.dil or c.W < c.dil)), c.name
        assert ('acc_ragged_block' in P) == (c.acc and c.dil == 1 and c.cin % 64 != 0 and c.cin > 64), c.name
        if 'tiles300' in P:
            assert c.B * -(-c.H // 4) * -(-c.W // 4) == 300 and 128 < c.cin < 256
        if 'ragged_tiles' in P:
            assert c.H % 4 and c.W % 4 and c.H % 2 and c.cin < 64
        if 'deep' in P:
            assert (c.B, c.zc, c.cin, c.H, c.W) == (2, 512, 512, 19, 19)
    assert (by['one_tile'].H, by['one_tile'].W, by['one_pixel'].H, by['one_pixel'].W) == (4, 4, 1, 1)
    assert by['d6_5x5'].dil ** 2 - by['d6_5x5'].H * by['d6_5x5'].W == 11
    # parts whose boundaries fall inside a 16-channel k-group
    for c in by.values():
        if len(c.parts) > 1:
            assert any(sum(c.parts[:i]) % 16 for i in range(1, len(c.parts))), c.name
