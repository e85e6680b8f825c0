"""Task-aligned assignment (the TAL matcher, include/ctdet.h at ct_tal_match_batched) restated in numpy: the yardstick of
tests/test_tal_cpu.py and tests/test_gpu_tal.py, never the code under test.  Every fp32 step is a numpy float32 operation,
rounded one at a time as the rule demands; boxes are walked by plain loops with a stable sort on (-m, index).  The predicted
boxes and scores come in as arrays: what ct_detect_fused wrote, or anything a test makes up."""
import types

import numpy as np

from atss_ref import encode, iou_plain, point_form

F = np.float32
FLT_MIN = np.finfo(np.float32).tiny


def metric(s, u, alpha2, beta):
    """Rule 3 from s and u (float32 arrays): 1 * [sqrt(s)] * s^(alpha2 // 2) * u^beta in this order, below FLT_MIN -> 0."""
    s, u = np.asarray(s, F), np.asarray(u, F)
    m = np.ones(np.broadcast(s, u).shape, F)
    if alpha2 & 1:
        m = m * np.sqrt(s)
    for _ in range(alpha2 // 2):
        m = m * s
    for _ in range(beta):
        m = m * u
    assert m.dtype == F
    return np.where(m >= FLT_MIN, m, F(0))


def box_select(t, priors, pred_boxes, pred_scores, topk, alpha2, beta):
    """Rules 1-5 for one box t [6] of an image with pred_boxes [P,4], pred_scores [P,C] -> None for a degenerate box, else a
    namespace: inside (bool [P]), m ([P], 0 outside the box), eligible (count), idx (the positives in the order chosen), u
    (the IoU each claim carries), last (m of the last positive, 0 if forced), forced (bool), gap (relative distance between the
    last chosen and the first rejected metric; None when nothing eligible is rejected)."""
    x1, y1, x2, y2 = t[0], t[1], t[2], t[3]
    if not (x2 > x1 and y2 > y1):
        return None
    pcx, pcy = priors[:, 0], priors[:, 1]
    inside = (x1 < pcx) & (pcx < x2) & (y1 < pcy) & (pcy < y2)
    u = iou_plain(t[:4], pred_boxes)
    u = np.where(u > 0, u, F(0)).astype(F)                       # NaN included
    label, cols = float(t[4]), pred_scores.shape[1]
    if label == int(label) and 1 <= int(label) <= cols - 1:
        s = pred_scores[:, int(label)]
    else:
        s = F(1) - pred_scores[:, 0]
    s = np.where(s > 0, s, F(0)).astype(F)
    m = np.where(inside, metric(s, u, alpha2, beta), F(0)).astype(F)
    eligible = int((m > 0).sum())
    if eligible == 0:                                            # rule 5: the best prior by its own IoU, over all priors
        pu = iou_plain(t[:4], point_form(priors))
        p = int(np.argmax(pu))                                   # the first maximum
        return types.SimpleNamespace(inside=inside, m=m, eligible=0, idx=np.array([p]), u=pu[p:p + 1], last=F(0), forced=True,
                                     gap=None)
    order = np.argsort(-m, kind='stable')[:eligible]             # ties: the lower prior index
    idx = order[:topk]
    gap = None
    if eligible > len(idx):
        last, nxt = float(m[idx[-1]]), float(m[order[len(idx)]])
        gap = (last - nxt) / last
    return types.SimpleNamespace(inside=inside, m=m, eligible=eligible, idx=idx, u=u[idx], last=m[idx[-1]], forced=False, gap=gap)


def match_image(truths, priors, pred_boxes, pred_scores, topk, alpha2, beta, variances, max_gt):
    """One image: truths [G,6] float32 -> loc_t [P,4], conf_t [P,2], obj_t [P] bool, overlap [P], gt_stats [max_gt,4], owner [P]
    (box index or -1), gaps (one per box that is not skipped)."""
    truths = np.asarray(truths, dtype=F).reshape(-1, 6)
    P = priors.shape[0]
    loc_t, conf_t = np.zeros((P, 4), F), np.zeros((P, 2), F)
    conf_t[:, 1] = 1
    obj_t, overlap = np.zeros(P, bool), np.zeros(P, F)
    stats = np.zeros((max_gt, 4), F)
    claims = {}                                 # prior -> (forced, u, box): rule 6
    gaps = []
    for g in range(min(len(truths), max_gt)):
        c = box_select(truths[g], priors, pred_boxes, pred_scores, topk, alpha2, beta)
        if c is None:
            continue
        gaps.append(c.gap)
        stats[g] = (c.eligible, len(c.idx), c.last, 1 if c.forced else 0)
        for p, u in zip(c.idx, c.u):
            claim, old = (c.forced, float(u), g), claims.get(int(p))
            # a forced claim over an ordinary one, then the larger u, then the lower box index (g only ever grows here)
            if old is None or (claim[0], claim[1]) > (old[0], old[1]):
                claims[int(p)] = claim
    owner = np.full(P, -1)
    for p, (_, u, g) in claims.items():
        t = truths[g]
        loc_t[p] = encode(t[:4], priors[p:p + 1], variances[0], variances[1])[0]
        conf_t[p] = (t[4], t[5])
        obj_t[p] = t[4] != 0
        overlap[p] = u
        owner[p] = g
    return loc_t, conf_t, obj_t, overlap, stats, owner, gaps


def match(targets, priors, pred_boxes, pred_scores, topk=13, alpha=1.0, beta=6, variances=(0.1, 0.2), max_gt=None):
    """A batch: targets = list of [G,6] arrays, pred_boxes [B,P,4], pred_scores [B,P,C] -> a namespace of numpy arrays loc_t
    [B,P,4], conf_t [B,P,2], obj_t [B,P] bool, overlap [B,P], gt_stats [B,max_gt,4], owner [B,P] and gaps (list per image).
    max_gt defaults to the largest box count (at least 1), as ops.tal_match_batched chooses it."""
    priors = np.ascontiguousarray(np.asarray(priors, dtype=F))
    pred_boxes, pred_scores = np.asarray(pred_boxes, dtype=F), np.asarray(pred_scores, dtype=F)
    targets = [np.asarray(t, dtype=F).reshape(-1, 6) for t in targets]
    alpha2 = int(2 * alpha)
    assert alpha2 == 2 * alpha and 0 <= alpha2 <= 4 and 0 <= beta <= 8 and 1 <= topk <= 16
    assert pred_boxes.shape == (len(targets), len(priors), 4) and pred_scores.shape[:2] == pred_boxes.shape[:2]
    if max_gt is None:
        max_gt = max([len(t) for t in targets] + [1])
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        rows = [match_image(t, priors, pred_boxes[b], pred_scores[b], topk, alpha2, beta, variances, max_gt)
                for b, t in enumerate(targets)]
    out = types.SimpleNamespace(gaps=[r[6] for r in rows])
    for i, name in enumerate(('loc_t', 'conf_t', 'obj_t', 'overlap', 'gt_stats', 'owner')):
        setattr(out, name, np.stack([r[i] for r in rows]))
    return out
