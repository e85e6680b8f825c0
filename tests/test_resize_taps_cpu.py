"""Host side of the bicubic / Lanczos4 augmentation filters: the C ABI surface, ops.resize_taps against the NumPy
definition (tests/resize_taps_ref.py) and its known answers, the definition against torch's bicubic, and the
`filters` switch of data.data_augment.preproc.  No device needed."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

import resize_taps_ref as ref
from conftest import REPO
from ctdet import _lib, ops
from data.data_augment import preproc

MEANS = (104, 117, 123)
KINDS = ('cubic', 'lanczos4')
# known answers of the definition: 11-bit coefficients of a fraction x
IC_OF_X = {
    0.0: ([0, 2048, 0, 0], [0, 0, 0, 2048, 0, 0, 0, 0]),
    0.25: ([-216, 1800, 536, -72], [-31, 114, -312, 1830, 579, -188, 64, -8]),
    0.5: ([-192, 1216, 1216, -192], [-26, 122, -340, 1267, 1267, -340, 122, -26]),
    0.8125: ([-44, 379, 1903, -190], [-5, 47, -139, 416, 1923, -262, 95, -27]),
}
# (n, S, kind) -> first rows: (source indices, coefficients)
ROWS = {
    (53, 24, 'cubic'): [([0, 0, 1, 2], [-145, 931, 1485, -222]),
                        ([1, 2, 3, 4], [-44, 379, 1903, -190]),
                        ([4, 5, 6, 7], [-31, 2046, 33, -1])],
    (5, 8, 'lanczos4'): [([0, 0, 0, 0, 0, 1, 2, 3], [-5, 47, -139, 416, 1923, -262, 95, -27]),
                         ([0, 0, 0, 0, 1, 2, 3, 4], [-29, 129, -355, 1429, 1097, -313, 112, -22])],
}


def test_abi_surface():
    """The library exports the entry, ctypes binds it, and the header's record is the 20 bytes the binding packs."""
    assert 'ct_preproc_augment_taps' in _lib.SIGNATURES
    fn = _lib.lib().ct_preproc_augment_taps
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    with open(os.path.join(REPO, 'include', 'ctdet.h')) as f:
        m = re.search(r'typedef\s+struct\s*\{\s*int\s+first;\s*short\s+c\[8\];\s*\}\s*ct_resize_tap;', f.read())
    assert m, 'ct_resize_tap is not declared in include/ctdet.h'
    assert C.sizeof(_lib.ResizeTap) == 20 and ops.TAP_DTYPE.itemsize == 20
    assert _lib.ResizeTap.first.offset == 0 and _lib.ResizeTap.c.offset == 4


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,S', [(53, 24), (5, 8), (24, 24), (500, 300), (2000, 300), (80, 512)])
def test_resize_taps_equal_the_definition(n, S, kind):
    first, ic = ops.resize_taps(n, S, kind)
    want_first, want_ic = ref.taps(n, S, kind)
    assert ic.dtype == np.int16 and ic.shape == (S, ref.K[kind])
    assert np.array_equal(first, want_first) and np.array_equal(ic, want_ic)
    rec = ops.tap_records(n, S, kind)               # what the device gets: first tap unclamped, 8 coefficient slots
    assert np.array_equal(rec['first'], want_first - (ref.K[kind] // 2 - 1))
    assert np.array_equal(rec['c'][:, :ref.K[kind]], want_ic) and not rec['c'][:, ref.K[kind]:].any()
    assert ops.resize_taps(n, S, kind)[1] is ic     # cached


def test_known_answers():
    for x, (cubic, lanczos) in IC_OF_X.items():
        for kind, want in (('cubic', cubic), ('lanczos4', lanczos)):
            assert ref.coeffs(x, kind).tolist() == want, (x, kind)
            assert ops.resize_coeffs(np.array([x], np.float32), kind)[0].tolist() == want, (x, kind)
    # the same fractions through resize_taps: x = 0 at n == S, 0.25 at 3 -> 2, 0.5 at 2 -> 1
    for (n, S), x in (((24, 24), 0.0), ((3, 2), 0.25), ((2, 1), 0.5)):
        for kind, want in zip(KINDS, IC_OF_X[x]):
            assert ops.resize_taps(n, S, kind)[1][0].tolist() == want, (n, S, kind)
    for (n, S, kind), rows in ROWS.items():
        k = ref.K[kind]
        for taps in (ops.resize_taps(n, S, kind), ref.taps(n, S, kind)):
            idx = ref.indices(np.asarray(taps[0], dtype=np.int64), n, k)
            for d, (want_idx, want_ic) in enumerate(rows):
                assert idx[d].tolist() == want_idx and taps[1][d].tolist() == want_ic, (n, S, kind, d)
    with pytest.raises(ValueError):
        ops.resize_taps(5, 8, 'linear')


@pytest.mark.parametrize('kind', KINDS)
def test_reference_resize_is_identity_at_equal_size(kind):
    img = np.random.RandomState(7).randint(0, 256, (24, 24, 3)).astype(np.uint8)
    assert np.array_equal(ref.resize(img, 24, kind), img)


@pytest.mark.parametrize('h,w,S', [(37, 53, 24), (90, 260, 300), (375, 500, 300)])
def test_reference_bicubic_against_torch(h, w, S):
    """Float bicubic (A = -0.75, half-pixel centres, clamped border) rounded and clipped differs from the 11-bit
    fixed-point path only where a value lands near a rounding boundary: by one grey level, on a few percent."""
    rng = np.random.RandomState(h)
    worst = 0.0
    for img in (rng.randint(0, 256, (h, w, 3)), 255 * rng.randint(0, 2, (h, w, 3))):
        img = img.astype(np.uint8)
        got = ref.resize(img, S, 'cubic').astype(np.int64)
        t = torch.from_numpy(img).permute(2, 0, 1)[None].double()
        want = torch.nn.functional.interpolate(t, size=(S, S), mode='bicubic', align_corners=False)
        want = want.round().clamp(0, 255)[0].permute(1, 2, 0).numpy().astype(np.int64)
        d = np.abs(got - want)
        print('bicubic %dx%d -> %d: max diff %d, share %.4f' % (h, w, S, d.max(), (d > 0).mean()))
        assert d.max() <= 1
        worst = max(worst, float((d > 0).mean()))
    assert worst <= 0.08


def _decide_all(filters, seed):
    random.seed(seed)
    pre = preproc(300, MEANS, 0.6, device='cpu', filters=filters)
    rng = np.random.RandomState(seed)
    plans = []
    for _ in range(3):
        h, w = int(rng.randint(90, 400)), int(rng.randint(90, 500))
        xy = rng.uniform(0, 0.6, (2, 2)) * (w, h)
        tg = np.hstack([xy, np.minimum(xy + rng.uniform(0.1, 0.4, (2, 2)) * (w, h), (w - 1, h - 1)),
                        rng.randint(0, 20, (2, 1)).astype(np.float64)])
        plans.append(pre.decide((h, w, 3), tg)[0])
    return plans, random.getstate()


def test_preproc_filters_switch(monkeypatch):
    monkeypatch.delenv('CTDET_AUG_FILTERS', raising=False)
    seen = set()
    for seed in range(200):
        fast, state_fast = _decide_all('fast', seed)
        cv2, state_cv2 = _decide_all('cv2', seed)
        assert state_fast == state_cv2                      # the same number of draws
        for a, b in zip(fast, cv2):
            assert {k: v for k, v in a.items() if k != 'interp'} == {k: v for k, v in b.items() if k != 'interp'}
            assert a['interp'] in (0, 1, 2)
            assert (a['interp'], b['interp']) in ((0, 0), (0, 3), (0, 4), (1, 1), (2, 2))
            seen.add(b['interp'])
    assert {3, 4} <= seen
    assert _decide_all(None, 5)[0] == _decide_all('fast', 5)[0]          # the default is today's mapping
    monkeypatch.setenv('CTDET_AUG_FILTERS', 'cv2')
    assert _decide_all(None, 5)[0] == _decide_all('cv2', 5)[0]
    with pytest.raises(ValueError):
        preproc(300, MEANS, 0.6, device='cpu', filters='bicubic')
    monkeypatch.setenv('CTDET_AUG_FILTERS', 'nope')
    with pytest.raises(ValueError):
        preproc(300, MEANS, 0.6, device='cpu')
