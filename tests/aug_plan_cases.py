"""The case table of the device augmentation planner (ct_aug_plan), shared by tests/test_aug_plan_ref_cpu.py and
tests/test_gpu_aug_plan.py.  It holds the smallest shapes at which the sampler can go wrong, not the workload's."""
import numpy as np

from ctdet import aug_plan_ref as ref

SEED = 0x5EED0001CAFE
MAX_GT = 20
IDS = 64                                    # sample ids per case
INTERP = (0, 0, 2, 1, 0)
FILL = (104.0, 117.0, 123.0)


def _boxes(n, W, H, seed):
    """n boxes inside a W x H image, float32 [n,5], labels 1..20."""
    r = np.random.RandomState(seed)
    x1, y1 = r.uniform(0, W * 0.7, n), r.uniform(0, H * 0.7, n)
    w, h = r.uniform(W * 0.08, W * 0.3, n), r.uniform(H * 0.08, H * 0.3, n)
    return np.stack([x1, y1, np.minimum(x1 + w, W), np.minimum(y1 + h, H), r.randint(1, 21, n)], 1).astype(np.float32)


B3 = np.array([[100, 100, 300, 250, 5], [10, 20, 80, 90, 3], [350, 200, 480, 360, 7]], dtype=np.float32)

# name -> dict(H, W, boxes[, cls, p, weight, flags]); p defaults to 0.6
CASES = [
    dict(name='voc_0', H=375, W=500, boxes=np.zeros((0, 5), np.float32)),
    dict(name='voc_1', H=375, W=500, boxes=_boxes(1, 500, 375, 1)),
    dict(name='voc_3', H=375, W=500, boxes=B3),
    dict(name='voc_20', H=375, W=500, boxes=_boxes(20, 500, 375, 2)),
    dict(name='voc_8', H=375, W=500, boxes=_boxes(8, 500, 375, 5)),
    dict(name='tall_2', H=500, W=333, boxes=_boxes(2, 333, 500, 6)),
    dict(name='tiny_9x7', H=7, W=9, boxes=np.array([[2, 1, 7, 6, 4]], np.float32)),
    dict(name='tiny_3x2', H=2, W=3, boxes=np.array([[0, 0, 3, 2, 4]], np.float32)),
    dict(name='whole', H=375, W=500, boxes=np.array([[0, 0, 500, 375, 9]], np.float32)),
    dict(name='one_px', H=375, W=500, boxes=np.array([[250, 180, 251, 181, 2]], np.float32)),
    dict(name='max_gt', H=375, W=500, boxes=_boxes(MAX_GT, 500, 375, 3)),
    dict(name='max_gt_plus3', H=375, W=500, boxes=_boxes(MAX_GT + 3, 500, 375, 4)),
    dict(name='cls_present', H=375, W=500, boxes=B3, cls=4),
    dict(name='cls_absent', H=375, W=500, boxes=B3, cls=10),
    dict(name='p0', H=375, W=500, boxes=B3, p=0.0),
    dict(name='p1', H=375, W=500, boxes=B3, p=1.0),
]
P_VALUES = (0.6, 0.0, 1.0)

# mixup pairs whose second target carries labels -1, under every flags value
MIX_A = np.array([[40, 30, 200, 220, 6], [220, 150, 400, 330, -1]], dtype=np.float32)
MIX_B = np.array([[60, 60, 300, 300, -1], [310, 40, 470, 200, 12], [20, 250, 150, 360, 8]], dtype=np.float32)


def case_samples(case, ids=IDS):
    """(shapes, targets, sample ids) of one case: `ids` samples of the same image, ids unique across the table."""
    k = [c['name'] for c in CASES].index(case['name'])
    return [(case['H'], case['W'])] * ids, [case['boxes']] * ids, np.arange(ids, dtype=np.uint64) + np.uint64(1000 * k)


def table(p):
    """One launch's inputs for the cases drawn with expand probability p: every case x IDS as one image each, then
    the mixup pairs (two samples per image, flags 0..3), then two samples of one image whose first keeps no row.
    -> (samples SAMPLE_DTYPE, boxes float32 [total,5], num_images)."""
    shapes, targets, ids, images, cls, weights, flags = [], [], [], [], [], [], []
    img = 0
    for case in CASES:
        if case.get('p', 0.6) != p:
            continue
        sh, tg, sid = case_samples(case)
        for j in range(len(sh)):
            shapes.append(sh[j]); targets.append(tg[j]); ids.append(sid[j]); images.append(img)
            cls.append(case.get('cls', -1)); weights.append(1.0); flags.append(0)
            img += 1
    if p == 0.6:
        for f in range(4):
            for j in range(16):
                lam = np.float32(0.25 + 0.03 * j)
                for tg, w, hi in ((MIX_A, lam, 0), (MIX_B, np.float32(1.0 - float(lam)), 1)):
                    shapes.append((375, 500)); targets.append(tg); images.append(img)
                    ids.append(np.uint64(500000 + 1000 * f + 2 * j + hi)); cls.append(-1); weights.append(w); flags.append(f)
                img += 1
        # an image whose first sample has no box (no row) and whose second has three
        for j in range(8):
            for tg in (np.zeros((0, 5), np.float32), B3):
                shapes.append((375, 500)); targets.append(tg); images.append(img)
                ids.append(np.uint64(600000 + 2 * j + len(tg))); cls.append(-1); weights.append(0.5); flags.append(0)
            img += 1
    s, b = ref.make_samples(shapes, targets, images=images, sample_ids=np.array(ids, dtype=np.uint64), cls=cls,
                            weights=weights, flags=flags)
    return s, b, img                   # p = 0.6: more samples than one chunk of the packing launch (1024)


_twin = {}


def twin(p):
    """The twin's result for table(p), computed once and shared (read-only)."""
    if p not in _twin:
        s, b, n_img = table(p)
        r = ref.plan_batch(s, b, n_img, MAX_GT, SEED, p, INTERP, FILL)
        for a in (s, b, r.plans, r.truths, r.gt_off):
            a.setflags(write=False)
        _twin[p] = (s, b, n_img, r)
    return _twin[p]
