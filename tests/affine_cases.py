"""The case table of the random affine stage (ct_aug_affine_plan / ct_preproc_warp_affine), shared by
tests/test_affine_cpu.py and tests/test_gpu_affine.py.  It is built on tests/mosaic_cases.py: the rows and offsets the
mosaic twin gives its tables at expand probability 0.6 are this stage's input, S and the per-image ids are the
table's.  A96: 12 images at S = 96; A8: 16 images at S = 8, the smallest square at which the border, the clamp and the
one-pixel tile show.  Under P_ALL the twin gives A96 images that keep every row, image 3 that loses 5 of 12, and image
11 (the tiny boxes) that falls back; test_affine_cpu.py::test_the_table_covers_what_it_was_built_for asserts it."""
import numpy as np

import mosaic_cases
from ctdet import aug_plan_ref as ref

SEED = mosaic_cases.SEED
BORDER_MEANS = (104.5, 117.25, 123.0)               # of the raw-ABI pixel tests: a border that is not zero
BORDER = tuple(float(np.float32(int(m)) - np.float32(m)) for m in BORDER_MEANS)     # (float)(int)fill - mean
P_ALL = ref.AffineParams()
P_HALF = ref.AffineParams(p=0.5)
P_NONE = ref.AffineParams(p=0.0)
PARAMS = {'P_ALL': P_ALL, 'P_HALF': P_HALF, 'P_NONE': P_NONE}
CASES = {'A96': 'M96', 'A8': 'M8'}

_built, _twin, _pixels = {}, {}, {}


def build(name):
    """-> dict(truths float32 [rows,6], gt_off int32 [n+1], ids, S, n), read-only and shared."""
    if name not in _built:
        t, r = mosaic_cases.build(CASES[name]), mosaic_cases.twin(CASES[name], 0.6)
        _built[name] = dict(truths=r.truths, gt_off=r.gt_off, ids=list(t['ids']), S=t['S'], n=t['n'])
    return _built[name]


def twin(name, pname):
    """The twin's AffineResult for table `name` under parameter set `pname`, computed once and shared (read-only)."""
    if (name, pname) not in _twin:
        t = build(name)
        r = ref.affine_batch(t['truths'], t['gt_off'], t['ids'], t['S'], SEED, PARAMS[pname])
        for a in (r.records, r.truths, r.gt_off, r.status):
            a.setflags(write=False)
        _twin[name, pname] = r
    return _twin[name, pname]


def pixels(name):
    """float32 [n,3,S,S]: mosaic_cases.image patterns minus BORDER_MEANS, CHW; computed once and shared (read-only)."""
    if name not in _pixels:
        t = build(name)
        rng = np.random.RandomState(t['S'] + 1)
        x = np.stack([mosaic_cases.image(rng, t['S'], t['S']).astype(np.float32).transpose(2, 0, 1)
                      for _ in range(t['n'])])
        x = x - np.asarray(BORDER_MEANS, dtype=np.float32).reshape(1, 3, 1, 1)
        x.setflags(write=False)
        _pixels[name] = x
    return _pixels[name]
