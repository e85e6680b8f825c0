"""The two epilogues of the fused F(4x4,3x3) kernel's PLAIN launches (csrc/ct_wino4f.hip, csrc/ct_wino4_emit.h): the default one
works out a tile's geometry once per work item and runs a straight-line part per 16 output channels (plan_tile4 /
emit_tile4_plain), CTDET_W4F_LEAN_EPI=0 -- inside a process ct_wino4f_set_lean_epilogue(0) -- launches the twin that keeps
emit_tile4's per-row tests.  Both apply the same arithmetic to every stored value, so the full-resolution output, the pooled output and the per-image maxima line must agree BIT FOR BIT --
on maps whose tiles are all interior, on maps with partial tiles on the right and at the bottom, in work items with dead lanes,
with a partial second channel block, with and without the fused 2x2 pool (floor and ceil mode) and the full map.  Each path is
also held to an fp64 convolution at the bound tests/test_gpu_wino.py::test_wino_rounding_error_vs_fp64 sets for these tiles."""
import pytest
import torch
import torch.nn.functional as F

from ctdet import _lib, engine
from test_gpu_absmax import _launch, _ref

pytestmark = pytest.mark.gpu
BOUND = 1.2e-5          # test_wino_rounding_error_vs_fp64: WINO4F and WINO4FH, max error over the output range
CIN = 32
# H, W, batch: 32 tiles make a work item -- every batch gives one item that is all live and one with dead lanes
MAPS = [(8, 8, 10),     # 2 x 2 tiles per image, all interior: 40 tiles
        (12, 16, 4),    # 3 x 4, all interior: 48 tiles = one full item and one half-dead one
        (10, 10, 4),    # 3 x 3, the right column and the bottom row hold 2 of 4: 36 tiles
        (9, 13, 3),     # 3 x 4, 1 of 4 on both edges: 36 tiles
        (6, 6, 9)]      # 2 x 2, 2 of 4 on both edges: 36 tiles
TILES = [(engine.WINO4FH, 'tile48_f16x2'), (engine.WINO4F, 'tile46_bf16x3')]
# (pool, relu): pool = None or (ceil_mode, write_full)
FORMS = [(None, True), (None, False), ((False, 1), True), ((False, 0), True), ((True, 1), True), ((True, 0), True)]


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('the gpu tests need a HIP device; none visible')


def _layer(H, W, B, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, CIN, H, W, generator=g) * (3.0 ** torch.arange(B).view(B, 1, 1, 1) / 9.0)
    w = torch.randn(cout, CIN, 3, 3, generator=g) * (2.0 / (CIN * 9)) ** 0.5
    b = torch.rand(cout, generator=g) - 0.5
    return x, w, b


def _both(x, parts, config, pool):
    """The same launch through the lean epilogue and through the per-row one (what CTDET_W4F_LEAN_EPI=0 selects for a process)."""
    lib = _lib.lib()
    try:
        _lib.check(lib.ct_wino4f_set_lean_epilogue(1), 'set_lean_epilogue')
        lean = _launch(x, parts, 1, 1, 1, config=config, pool=pool, seed=1e-30)
        _lib.check(lib.ct_wino4f_set_lean_epilogue(0), 'set_lean_epilogue')
        old = _launch(x, parts, 1, 1, 1, config=config, pool=pool, seed=1e-30)
    finally:
        lib.ct_wino4f_set_lean_epilogue(-1)          # back to the environment's choice
    return lean, old


def _err(got, want64):
    return float((got.double() - want64).abs().max() / want64.abs().max())


@pytest.mark.parametrize('config,tid', TILES, ids=[t[1] for t in TILES])
@pytest.mark.parametrize('geo', MAPS, ids=['%dx%d' % (m[0], m[1]) for m in MAPS])
def test_lean_epilogue_matches_the_per_row_epilogue(geo, config, tid):
    H, W, B = geo
    for cout in (64, 96):                     # 96: the second block of 64 output channels is half empty
        x, w, b = _layer(H, W, B, cout, 100 * H + W + cout)
        want = {relu: _ref(x, [(w, b, None, relu)], 1, 1, 1) for relu in (True, False)}
        for pool, relu in FORMS:
            tag = (H, W, cout, tid, pool, relu)
            lean, old = _both(x, [(w, b, None, relu)], config, pool)
            full = pool is None or pool[1]
            for r in (lean, old):
                if full:
                    assert _err(r['y'], want[relu]) < BOUND, (tag, _err(r['y'], want[relu]))
                else:
                    assert torch.isnan(r['y']).all(), tag
                if pool is not None:
                    wp = F.max_pool2d(want[relu], 2, 2, 0, ceil_mode=pool[0])
                    assert r['pooled'].shape == wp.shape and _err(r['pooled'], wp) < BOUND, (tag, _err(r['pooled'], wp))
            if full:
                assert torch.equal(lean['y'], old['y']), tag
            if pool is not None:
                assert torch.equal(lean['pooled'], old['pooled']), tag
            assert torch.equal(lean['slot'], old['slot']), tag
            if config == engine.WINO4FH:      # the f16x2 form tracks: the line really was raised, to the same bits on both paths
                assert not torch.equal(lean['slot'], lean['seeded']), tag


@pytest.mark.parametrize('config,tid', TILES, ids=[t[1] for t in TILES])
def test_one_nan_in_the_input_lands_in_the_same_places(config, tid):
    """A single NaN in the input (image 1, an edge tile's patch): NaN at the same positions of the output and of the pooled output on
    both paths, the same bits everywhere else, the same maxima line (a NaN is skipped by the tracker)."""
    H, W, B, cout = 10, 10, 4, 96
    x, w, b = _layer(H, W, B, cout, 7)
    x[1, 5, 8, 9] = float('nan')
    lean, old = _both(x, [(w, b, None, True)], config, (True, 1))
    for k in ('y', 'pooled'):
        nl, no = torch.isnan(lean[k]), torch.isnan(old[k])
        assert torch.equal(nl, no), (tid, k)
        assert torch.equal(torch.where(nl, 0.0, lean[k]), torch.where(no, 0.0, old[k])), (tid, k)
    nan_y = torch.isnan(lean['y'])
    assert nan_y[1].any() and not nan_y[0].any() and not nan_y[2:].any(), tid
    assert torch.equal(lean['slot'], old['slot']), tid


@pytest.mark.parametrize('config,tid', TILES, ids=[t[1] for t in TILES])
def test_per_channel_scale_and_shift_of_a_batchnorm_layer(config, tid):
    """BatchNorm folded into the epilogue: scale and shift differ per channel (the layers above are bias-only, scale 1), so a
    quarter that took another channel's scale shows -- 96 channels = six quarters in two blocks, the last two empty; a map with
    partial tiles, ceil-mode pool, full map stored."""
    H, W, B, cout = 9, 13, 3, 96
    x, w, _ = _layer(H, W, B, cout, 11)
    g = torch.Generator().manual_seed(12)
    bn = (torch.rand(cout, generator=g) * 3.0 + 0.25, torch.rand(cout, generator=g) - 0.5,
          torch.rand(cout, generator=g) * 0.2 - 0.1, torch.rand(cout, generator=g) * 0.4 + 0.8)      # weight, bias, mean, var
    parts = [(w, None, bn, True)]
    want = _ref(x, parts, 1, 1, 1)
    scale = bn[0] / torch.sqrt(bn[3] + 1e-5)
    assert float(scale.max() / scale.min()) > 4.0
    lean, old = _both(x, parts, config, (True, 1))
    wp = F.max_pool2d(want, 2, 2, 0, ceil_mode=True)
    for r in (lean, old):
        assert _err(r['y'], want) < BOUND, (tid, _err(r['y'], want))
        assert _err(r['pooled'], wp) < BOUND, (tid, _err(r['pooled'], wp))
    assert torch.equal(lean['y'], old['y']) and torch.equal(lean['pooled'], old['pooled']) and torch.equal(lean['slot'], old['slot']), tid
