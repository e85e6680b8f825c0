"""Adaptive training sample selection (the ATSS matcher, include/ctdet.h at ct_atss_match_batched) restated in numpy: the
yardstick of tests/test_atss_cpu.py and tests/test_gpu_atss.py, never the code under test.  Every fp32 step is a numpy
float32 operation, rounded one at a time as the rule demands; the statistics are Python floats (float64) accumulated in
candidate order; boxes and levels are walked by plain loops with a stable sort on (d, index)."""
import math
import types

import numpy as np

F = np.float32


def iou_plain(gt, pf):
    """ct_box_math.h: iou_plain(gt [4], point-form priors [n,4]) -> [n], float32 operation by operation."""
    w = np.maximum(np.minimum(gt[2], pf[:, 2]) - np.maximum(gt[0], pf[:, 0]), F(0))
    h = np.maximum(np.minimum(gt[3], pf[:, 3]) - np.maximum(gt[1], pf[:, 1]), F(0))
    inter = w * h
    area_a = (gt[2] - gt[0]) * (gt[3] - gt[1])
    area_b = (pf[:, 2] - pf[:, 0]) * (pf[:, 3] - pf[:, 1])
    return inter / (area_a + area_b - inter)


def point_form(p):
    return np.stack([p[:, 0] - p[:, 2] / F(2), p[:, 1] - p[:, 3] / F(2), p[:, 0] + p[:, 2] / F(2),
                     p[:, 1] + p[:, 3] / F(2)], 1)


def encode(t, pr, v0, v1):
    """The encode expression of the matchers (ct_box_math.h: encode_box) for one box t [4] and priors pr [n,4]."""
    v0, v1 = F(v0), F(v1)
    return np.stack([((t[0] + t[2]) / F(2) - pr[:, 0]) / (v0 * pr[:, 2]), ((t[1] + t[3]) / F(2) - pr[:, 1]) / (v0 * pr[:, 3]),
                     np.log((t[2] - t[0]) / pr[:, 2]) / v1, np.log((t[3] - t[1]) / pr[:, 3]) / v1], 1).astype(F)


def box_candidates(t, priors, level_off, topk):
    """Rules 1-6 for one box t [6] -> None for a degenerate box, else a namespace: idx (candidate priors in candidate
    order), iou, t, positive (bool per candidate, the forced one included), forced (candidate position or -1), margin."""
    x1, y1, x2, y2 = t[0], t[1], t[2], t[3]
    if not (x2 > x1 and y2 > y1):
        return None
    gx, gy = (x1 + x2) / F(2), (y1 + y2) / F(2)
    dx, dy = priors[:, 0] - gx, priors[:, 1] - gy
    d = dx * dx + dy * dy
    assert d.dtype == F
    idx = []
    for l in range(len(level_off) - 1):
        lo, hi = level_off[l], level_off[l + 1]
        order = np.argsort(d[lo:hi], kind='stable')[:min(topk, hi - lo)]      # ties: the lower prior index
        idx.extend(int(lo + o) for o in order)
    idx = np.asarray(idx, dtype=np.int64)
    iou = iou_plain(t[:4], point_form(priors[idx]))
    assert iou.dtype == F
    n = len(idx)
    s = 0.0
    for v in iou:
        s += float(v)
    mean = s / n
    var = 0.0
    if n >= 2:
        for v in iou:
            var += (float(v) - mean) * (float(v) - mean)
        var /= n - 1
    thr = F(mean + math.sqrt(var))
    pcx, pcy = priors[idx, 0], priors[idx, 1]
    positive = (iou >= thr) & (x1 < pcx) & (pcx < x2) & (y1 < pcy) & (pcy < y2)
    forced = -1
    if not positive.any():
        forced = int(np.argmax(iou))                                           # the first maximum in candidate order
        positive[forced] = True
    margin = float(np.abs(iou.astype(np.float64) - float(thr)).min())
    return types.SimpleNamespace(idx=idx, iou=iou, t=thr, positive=positive, forced=forced, margin=margin)


def match_image(truths, priors, level_off, topk, variances, max_gt):
    """One image: truths [G,6] float32 -> loc_t [P,4], conf_t [P,2], obj_t [P] bool, overlap [P], gt_stats [max_gt,4],
    margins (one per box that is not skipped)."""
    truths = np.asarray(truths, dtype=F).reshape(-1, 6)
    P = priors.shape[0]
    loc_t, conf_t = np.zeros((P, 4), F), np.zeros((P, 2), F)
    conf_t[:, 1] = 1
    obj_t, overlap = np.zeros(P, bool), np.zeros(P, F)
    stats = np.zeros((max_gt, 4), F)
    owner = {}                                  # prior -> (forced, iou, box): rule 7
    margins = []
    for g in range(min(len(truths), max_gt)):
        c = box_candidates(truths[g], priors, level_off, topk)
        if c is None:
            continue
        margins.append(c.margin)
        stats[g] = (c.t, len(c.idx), int(c.positive.sum()), 1 if c.forced >= 0 else 0)
        for k in np.nonzero(c.positive)[0]:
            p, claim = int(c.idx[k]), (k == c.forced, float(c.iou[k]), g)
            old = owner.get(p)
            # a forced claim over an ordinary one, then the larger IoU, then the lower box index (g only ever grows here)
            if old is None or (claim[0], claim[1]) > (old[0], old[1]):
                owner[p] = claim
    for p, (_, iou, g) in owner.items():
        t = truths[g]
        loc_t[p] = encode(t[:4], priors[p:p + 1], variances[0], variances[1])[0]
        conf_t[p] = (t[4], t[5])
        obj_t[p] = t[4] != 0
        overlap[p] = iou
    return loc_t, conf_t, obj_t, overlap, stats, margins


def match(targets, priors, level_off, topk=9, variances=(0.1, 0.2), max_gt=None):
    """A batch: targets = list of [G,6] arrays or tensors -> a namespace of numpy arrays loc_t [B,P,4], conf_t [B,P,2],
    obj_t [B,P] bool, overlap [B,P], gt_stats [B,max_gt,4] and margins (list per image).  max_gt defaults to the largest
    box count (at least 1), as ops.atss_match_batched chooses it."""
    priors = np.ascontiguousarray(np.asarray(priors, dtype=F))
    level_off = [int(o) for o in level_off]
    assert level_off[0] == 0 and level_off[-1] == priors.shape[0]
    targets = [np.asarray(t, dtype=F).reshape(-1, 6) for t in targets]
    if max_gt is None:
        max_gt = max([len(t) for t in targets] + [1])
    with np.errstate(divide='ignore', invalid='ignore'):
        rows = [match_image(t, priors, level_off, topk, variances, max_gt) for t in targets]
    out = types.SimpleNamespace(margins=[r[5] for r in rows])
    for i, name in enumerate(('loc_t', 'conf_t', 'obj_t', 'overlap', 'gt_stats')):
        setattr(out, name, np.stack([r[i] for r in rows]))
    return out
