"""The case table of the four-image mosaic (ct_aug_plan_mosaic / ct_preproc_augment_mosaic), shared by
tests/test_mosaic_cpu.py and tests/test_gpu_mosaic.py: one seeded table, the smallest shapes at which the composition
can go wrong.  The per-image sample ids were searched on the host twin until the table shows every situation
test_mosaic_cpu.py::test_the_table_covers_what_it_was_searched_for asserts; sample k of image i draws with id
(ids[i] + k * 2**61) mod 2**64, as data_augment.preproc.mosaic_device does."""
import numpy as np

from ctdet import aug_plan_ref as ref

SEED = 0x5EED0002BEEF
INTERP = (0, 0, 2, 1, 0)
FILL = (104.0, 117.0, 123.0)
P_VALUES = (0.6, 0.0, 1.0)

# M96: image 0 holds a tile with the nearest filter and no distortion, image 10 mixes tiny and large boxes (the
# filter drops some rows, not all), image 11 has tiny boxes only (the fallback fires).
M96 = dict(name='M96', S=96, margin=24, n=12, lo=30, hi=120, max_boxes=6, rng=96,
           ids=[7000001, 7001000, 7002000, 7003000, 7004000, 7005000, 7006000, 7007000, 7008000, 7009000,
                7010000, 7011000])
# M8: images 0..3 meet at cx = 1, cx = 7, cy = 1, cy = 7 (tiles of width / height 1, both ends of the range).
M8 = dict(name='M8', S=8, margin=1, n=16, lo=5, hi=20, max_boxes=3, rng=8,
          ids=[8000007, 8001006, 8002003, 8003000] + [8004000 + 1000 * i for i in range(12)])
CASES = {'M96': M96, 'M8': M8}
NO_BOXES, WITH_CLS = 5, 9                   # M96: a sample without boxes, a sample with a class constraint
MIXED_IMAGE, TINY_IMAGE = 10, 11            # M96


def image(rng, h, w):
    """A uint8 h x w x 3 image with gradients, wrap-around edges and noise (the pattern of tests/test_gpu_augment.py)."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 3 + yy) % 256, (xx + yy * 2) % 256, (xx * yy // 7) % 256], -1)
    return ((base + rng.randint(0, 64, (h, w, 3))) % 256).astype(np.uint8)


def _boxes(rng, n, H, W, lo=0.15, hi=0.6):
    """n boxes inside an H x W image with sides lo..hi of it, float32 [n,5], labels 1..20."""
    w, h = rng.uniform(lo, hi, n) * W, rng.uniform(lo, hi, n) * H
    x1, y1 = rng.uniform(0, 1, n) * (W - w), rng.uniform(0, 1, n) * (H - h)
    return np.stack([x1, y1, x1 + w, y1 + h, rng.randint(1, 21, n)], 1).astype(np.float32)


def sample_ids(ids):
    return np.array([(int(ids[s // 4]) + (s % 4) * 2 ** 61) % 2 ** 64 for s in range(4 * len(ids))], dtype=np.uint64)


_built, _twin = {}, {}


def build(name, ids=None):
    """-> dict(samples SAMPLE_DTYPE [4n], boxes float32 [total,5], images [4n] uint8, targets [4n], max_gt, S, margin,
    n, ids).  `ids` replaces the table's per-image ids (the search); the default is computed once and shared."""
    if ids is None and name in _built:
        return _built[name]
    case = CASES[name]
    rng = np.random.RandomState(case['rng'])
    n = case['n']
    shapes, targets, images, cls = [], [], [], []
    for s in range(4 * n):
        H, W = (int(v) for v in rng.randint(case['lo'], case['hi'] + 1, 2))
        g = int(rng.randint(0, case['max_boxes'] + 1))
        tg = _boxes(rng, g, H, W)
        c = -1
        if name == 'M96':
            if s == NO_BOXES:
                tg = tg[:0]
            elif s == WITH_CLS:
                tg = _boxes(rng, 3, H, W)
                c = int(tg[1, 4]) - 1
            elif s // 4 == MIXED_IMAGE:
                H = W = 120
                tg = np.concatenate([_boxes(rng, 2, H, W, 0.011, 0.013), _boxes(rng, 2, H, W, 0.3, 0.6)], 0)
            elif s // 4 == TINY_IMAGE:
                H = W = 120
                tg = _boxes(rng, 1 + s % 2, H, W, 0.011, 0.012)
        shapes.append((H, W)); targets.append(tg); cls.append(c)
        images.append(image(rng, H, W))
    use = case['ids'] if ids is None else ids
    samples, boxes = ref.make_samples(shapes, targets, images=np.arange(4 * n) // 4, sample_ids=sample_ids(use), cls=cls)
    out = dict(samples=samples, boxes=boxes, images=images, targets=targets, S=case['S'], margin=case['margin'], n=n,
               max_gt=max(max(len(t) for t in targets), 1), ids=list(use))
    if ids is None:
        samples.setflags(write=False); boxes.setflags(write=False)
        _built[name] = out
    return out


def run_twin(t, p, truths_cap=None):
    return ref.mosaic_batch(t['samples'], t['boxes'], t['n'], t['max_gt'], SEED, p, INTERP, FILL, t['S'], t['margin'],
                            truths_cap=truths_cap)


def twin(name, p):
    """The twin's result for the table `name` drawn with expand probability p, computed once and shared (read-only)."""
    if (name, p) not in _twin:
        r = run_twin(build(name), p)
        for a in (r.plans, r.tiles, r.truths, r.gt_off, r.status):
            a.setflags(write=False)
        _twin[name, p] = r
    return _twin[name, p]
