"""Shared cases of the device VOC evaluator's tests (tests/test_voc_eval_device_cpu.py, tests/test_gpu_voc_eval.py):
the golden of data/voc_eval.py laid out as the post-processing's buffers, a randomised tie-heavy data set, the host
reference (evaluate.voc_eval_lines with stable=True) and a NumPy restatement of ct_voc_match's rule."""
import os

import numpy as np

from ctdet import evaluate

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'voc_eval.npz')


def golden_case():
    """14 images, T = 3, cap = 8: the golden's detections in its own (unsorted) row order."""
    g = np.load(GOLDEN)
    classes, ids = [str(c) for c in g['classes']], [str(i) for i in g['ids']]
    T, n, cap = len(classes) - 1, len(ids), 8
    dets, count = np.zeros((n, T, cap, 5), np.float32), np.zeros((n, T), np.int32)
    for ci in range(1, T + 1):
        for i in range(n):
            d = g['det_c%d_i%d' % (ci, i)]
            dets[i, ci - 1, :len(d)], count[i, ci - 1] = d, len(d)
    gt = {c: {} for c in classes[1:]}
    for iid in ids:
        a = g['gt_%s' % iid].reshape(-1, 6)
        for ci in range(1, T + 1):
            rows = a[a[:, 0] == ci]
            gt[classes[ci]][iid] = {'bbox': rows[:, 1:5], 'difficult': rows[:, 5].astype(bool)}
    return dict(dets=dets, count=count, gt=gt, classes=classes, ids=ids, golden=g)


def random_case(seed=11, n=70, cap=40):
    """70 images, T = 3, 0..40 rows per segment in descending score order.  Scores sit within 4e-4 of 50 three-decimal
    levels (ties abound, and rounding decides the level), coordinates on quarter pixels.  Class 'a': up to 70 boxes
    in one image (more than a 64-lane wave), one box five times over, difficult boxes, images without any; class 'b'
    has detections and no ground truth; class 'c' has ground truth and no detection."""
    rng = np.random.RandomState(seed)
    classes = ['__background__', 'a', 'b', 'c']
    ids = ['%06d' % (i + 1) for i in range(n)]
    T = 3
    gt = {'a': {}, 'c': {}}                                     # 'b' is missing from the mapping altogether
    for i, iid in enumerate(ids):
        k = 70 if i == 5 else 0 if i % 7 == 3 else rng.randint(1, 6)
        xy = rng.randint(0, 400, (k, 2))
        wh = rng.randint(8, 90, (k, 2))
        bb = np.concatenate([xy, xy + wh], 1)
        if i == 9:
            bb = np.concatenate([bb, np.repeat(bb[:1], 4, 0)])          # one box five times: the first takes the match
        if k or i == 9:
            gt['a'][iid] = {'bbox': bb, 'difficult': rng.rand(len(bb)) < 0.2}
        if i % 3 == 0:
            gt['c'][iid] = {'bbox': rng.randint(0, 300, (2, 4)) + np.array([0, 0, 300, 300]),
                            'difficult': np.array([False, i % 2 == 0])}
    levels = np.sort(rng.choice(np.arange(15, 1000), 50, replace=False))
    dets, count = np.zeros((n, T, cap, 5), np.float32), np.zeros((n, T), np.int32)
    for i, iid in enumerate(ids):
        for c in range(2):                                              # class 'c' (index 2) gets no detection
            k = cap if i == 5 else int(rng.choice([0, 1, 3, 17, cap, rng.randint(0, cap + 1)]))
            if i == 20:
                k = 0                                                   # an image without any detection
            rows = np.zeros((k, 5))
            xy = rng.randint(0, 1600, (k, 2)) / 4.0
            rows[:, :2], rows[:, 2:4] = xy, xy + rng.randint(32, 360, (k, 2)) / 4.0
            src = gt['a'].get(iid)
            if c == 0 and src is not None and k:                        # most rows are jittered ground-truth boxes
                pick = rng.randint(0, len(src['bbox']), k)
                near = src['bbox'][pick] - 1 + rng.randint(-24, 25, (k, 4)) / 4.0
                use = rng.rand(k) < 0.8
                rows[use, :4] = near[use]
            rows[:, 4] = levels[rng.randint(0, 50, k)] / 1000.0 + rng.randint(-4, 5, k) * 1e-4
            r32 = rows.astype(np.float32)
            r32 = r32[np.argsort(-r32[:, 4], kind='stable')]            # a segment as the post-processing leaves it
            dets[i, c, :k], count[i, c] = r32, k
    return dict(dets=dets, count=count, gt=gt, classes=classes, ids=ids)


def all_boxes_of(case):
    """The reference's all_boxes[cls][img] of a case's buffers."""
    n, T = case['count'].shape
    return [[np.empty((0, 5), np.float32)] * n] + [[case['dets'][i, c, :case['count'][i, c]].copy() for i in range(n)]
                                                    for c in range(T)]


def host_reference(case, ovthresh, use_07_metric):
    """{class: (rec, prec, ap)} from the host twin: results lines + voc_eval_lines(stable=True)."""
    ab = all_boxes_of(case)
    out = {}
    for ci, cls in enumerate(case['classes']):
        if ci:
            lines = evaluate.results_lines(ab[ci], case['ids'])
            with np.errstate(invalid='ignore', divide='ignore'):           # a class without positives: rec = 0 / 0
                out[cls] = evaluate.voc_eval_lines(lines, case['gt'].get(cls, {}), ovthresh, use_07_metric, stable=True)
    return out


def recall_steps(rec):
    """Change points of [0, rec, 1]: the number of terms of the area AP's sum."""
    m = np.concatenate(([0.], rec, [1.]))
    return int(np.sum(m[1:] != m[:-1]))


def restated_records(case, ovthresh):
    """ct_voc_match in NumPy (csrc/ct_eval.hip): per row the key (class, 2^20-1 - n, image, row) and the flag
    1 = tp / 2 = fp / 0 = neither, where a box goes to the row first in (n descending, row ascending) order among the
    rows of its segment that point at it.  -> (keys int64, flags uint8) in ascending key order."""
    boxes, label, difficult, off, _ = evaluate.pack_ground_truth(case['gt'], case['classes'], case['ids'])
    n, T = case['count'].shape
    keys, flags = [], []
    for i in range(n):
        gb, gl, gd = (a[off[i]:off[i + 1]] for a in (boxes.astype(np.float64), label, difficult))
        for c in range(T):
            rows = case['dets'][i, c, :case['count'][i, c]]
            bb, nn = evaluate.quantise_like_results_file(rows)
            sel = np.flatnonzero(gl == c + 1)
            best = np.full(len(rows), -1)
            for r in range(len(rows)):
                if len(sel):
                    g = gb[sel]
                    iw = np.maximum(np.minimum(g[:, 2], bb[r, 2]) - np.maximum(g[:, 0], bb[r, 0]) + 1., 0.)
                    ih = np.maximum(np.minimum(g[:, 3], bb[r, 3]) - np.maximum(g[:, 1], bb[r, 1]) + 1., 0.)
                    uni = ((bb[r, 2] - bb[r, 0] + 1.) * (bb[r, 3] - bb[r, 1] + 1.) +
                           (g[:, 2] - g[:, 0] + 1.) * (g[:, 3] - g[:, 1] + 1.) - iw * ih)
                    iou = iw * ih / uni
                    if iou.max() > ovthresh:
                        best[r] = sel[np.argmax(iou)]
            rank = (2 ** 20 - 1 - nn) * 4096 + np.arange(len(rows))
            for r in range(len(rows)):
                f = 2
                if best[r] >= 0:
                    mates = rank[best == best[r]]
                    f = 0 if gd[best[r]] else 1 if rank[r] == mates.min() else 2
                flags.append(f)
                keys.append((c << 53) | (int(2 ** 20 - 1 - nn[r]) << 33) | (i << 12) | r)
    keys, flags = np.asarray(keys, np.int64), np.asarray(flags, np.uint8)
    order = np.argsort(keys)
    return keys[order], flags[order]
