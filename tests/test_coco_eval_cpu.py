"""The host twin of the COCO bbox evaluator (ctdet.evaluate.pack_coco_ground_truth / coco_eval_arrays / coco_summarize)
against the golden of the reference's own COCOeval (tests/golden/coco_eval.npz) -- equality, no tolerance -- and, on a
random data set, against a deliberately naive scalar restatement of cocoeval.py written here."""
import copy
import functools

import numpy as np
import pytest

import coco_eval_cases as cases
from ctdet import evaluate


@functools.lru_cache(maxsize=None)
def _golden():
    return cases.golden_case()


@functools.lru_cache(maxsize=None)
def _golden_arrays():
    g = _golden()
    packed = evaluate.pack_coco_ground_truth(g['gt'], g['category_ids'], g['image_ids'])
    return packed, evaluate.coco_eval_arrays(cases.all_boxes_of(g['dets'], g['count']), packed)


def test_default_params_are_the_reference_expressions():
    iou, rec, area, md = evaluate.coco_default_params()
    assert len(iou) == 10 and len(rec) == 101 and md == (1, 10, 100)
    assert iou[0] == 0.5 and iou[-1] == 0.95 and rec[0] == 0. and rec[-1] == 1.
    assert area.tolist() == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]


def test_golden_arrays_equal_the_reference():
    g = _golden()
    _, (precision, recall, scores) = _golden_arrays()
    assert precision.dtype == recall.dtype == scores.dtype == np.float64
    assert precision.shape == (10, 101, 5, 4, 3) and recall.shape == (10, 5, 4, 3)
    assert np.array_equal(precision, g['precision'])
    assert np.array_equal(recall, g['recall'])
    assert np.array_equal(scores, g['scores'])


def test_golden_exercises_every_kind_of_entry():
    g = _golden()
    for a in range(4):
        for arr in (g['precision'][:, :, :, a], g['recall'][:, :, a]):
            assert (arr == -1).any() and (arr == 0).any() and ((arr > 0) & (arr < 1)).any()
    assert g['count'].max() > 100 and g['count'][g['never_fed']].sum() == 0


def test_packed_rows_and_all_boxes_are_the_same_input():
    g = _golden()
    packed, want = _golden_arrays()
    got = evaluate.coco_eval_arrays((g['dets'], g['count']), packed)
    assert all(np.array_equal(x, y) for x, y in zip(got, want))


def test_golden_stats_and_results():
    g = _golden()
    packed, (precision, recall, _) = _golden_arrays()
    results, stats = evaluate.coco_summarize(precision, recall, packed)
    assert stats.shape == (12,) and np.array_equal(stats, g['stats'])
    assert [results[m] for m in ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl')] == [float(s * 100) for s in stats[:6]]
    # per class: the class's own K position.  K is by ascending id: 3 car, 7 train, 18 dog, 44 bottle, 90 toothbrush
    assert packed.cat_ids == [3, 7, 18, 44, 90] and packed.cat_rank.tolist() == [-1, 2, 0, 4, 1, 3]
    for k, name in enumerate(packed.names):
        p = g['precision'][:, :, k, 0, -1]
        p = p[p > -1]
        want = float(np.mean(p) * 100) if p.size else float('nan')
        assert results['AP-' + name] == want or (np.isnan(want) and np.isnan(results['AP-' + name]))
    assert np.isnan(results['AP-toothbrush']) and np.isnan(results['AP-train']) and results['AP-bottle'] == 0.
    assert 0 < results['AP-dog'] < 100 and 0 < results['AP-car'] < 100
    empty = evaluate.coco_summarize(-np.ones_like(precision), -np.ones_like(recall))[1]
    assert np.array_equal(empty, -np.ones(12))


def test_packer_layout_order_and_npig():
    g = _golden()
    packed, _ = _golden_arrays()
    gt, ids = g['gt'], g['image_ids']
    assert packed.boxes.dtype == np.float64 and packed.area.dtype == np.float64
    assert packed.iscrowd.dtype == np.uint8 and packed.label.dtype == np.int32 and packed.off.dtype == np.int32
    assert packed.npig.dtype == np.int32 and packed.npig.shape == (5, 4)
    assert ids != sorted(ids)                            # the data set order is not the evaluation order
    assert [ids[i] for i in np.argsort(packed.image_rank)] == sorted(ids)
    area_rng = evaluate.coco_default_params()[2]
    want = np.zeros((5, 4), int)
    for ann in gt['annotations']:
        if not ann['iscrowd']:
            for a, (lo, hi) in enumerate(area_rng):
                want[packed.cat_ids.index(ann['category_id']), a] += lo <= ann['area'] <= hi
    assert np.array_equal(packed.npig, want) and want[4].sum() == 0 and want[1].sum() == 0
    assert any(ann['area'] == 1024 for ann in gt['annotations']) and (want[:, 1] + want[:, 2] + want[:, 3] > want[:, 0]).any()
    # per image (by rank) and class: annotation order
    for r, img in enumerate(sorted(ids)):
        a0, a1 = packed.off[r], packed.off[r + 1]
        assert np.all(np.diff(packed.label[a0:a1]) >= 0)
        for j in range(1, 6):
            mine = [ann for ann in gt['annotations'] if ann['image_id'] == img and ann['category_id'] == g['category_ids'][j]]
            sel = np.flatnonzero(packed.label[a0:a1] == j) + a0
            assert packed.boxes[sel].tolist() == [ann['bbox'] for ann in mine]
            assert packed.area[sel].tolist() == [ann['area'] for ann in mine]
            assert packed.iscrowd[sel].tolist() == [ann['iscrowd'] for ann in mine]
    assert packed.off[-1] == len(gt['annotations']) == len(packed.label)


def test_packer_subset_of_images_and_categories():
    g = _golden()
    ids = g['image_ids'][3:9]
    packed = evaluate.pack_coco_ground_truth(g['gt'], [0, 44, 3], ids)
    assert packed.cat_ids == [3, 7, 18, 44, 90] and packed.cat_rank.tolist() == [-1, 3, 0]
    inside = [ann for ann in g['gt']['annotations'] if ann['image_id'] in ids]
    assert len(packed.label) == sum(ann['category_id'] in (44, 3) for ann in inside)
    assert packed.npig[:, 0].sum() == sum(not ann['iscrowd'] for ann in inside)     # other categories keep their npig


def test_packer_refusals():
    g = _golden()
    gt = copy.deepcopy(g['gt'])
    gt['annotations'][5]['id'] = 0
    with pytest.raises(ValueError, match='id 0'):
        evaluate.pack_coco_ground_truth(gt, g['category_ids'], g['image_ids'])
    limit = evaluate.COCO_MAX_GT_PER_SEGMENT
    assert limit >= 128
    tiny = {'images': [{'id': 7}], 'categories': [{'id': 2, 'name': 'x'}],
            'annotations': [{'id': k + 1, 'image_id': 7, 'category_id': 2, 'bbox': [k, 0, 5, 5], 'area': 25., 'iscrowd': 0}
                            for k in range(limit + 1)]}
    with pytest.raises(ValueError, match='at most %d' % limit):
        evaluate.pack_coco_ground_truth(tiny, [0, 2])
    tiny['annotations'].pop()
    assert evaluate.pack_coco_ground_truth(tiny, [0, 2]).npig.tolist() == [[limit, limit, 0, 0]]
    with pytest.raises(ValueError):
        evaluate.pack_coco_ground_truth(g['gt'], [0, 18, 5], g['image_ids'])         # 5 is no category of the data set
    with pytest.raises(ValueError):
        evaluate.pack_coco_ground_truth(g['gt'], g['category_ids'], g['image_ids'] + [123456])
    packed, _ = _golden_arrays()
    with pytest.raises(ValueError, match='ascending'):
        evaluate.coco_eval_arrays((g['dets'], g['count']), packed, rec_thrs=[0.5, 0.1])


# ---------------------------------------------------------------- the naive restatement
def _naive_iou(d, g, crowd):
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.
    i = w * h
    u = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - i
    return i / u


def _naive_coco(case):
    """cocoeval.py evaluate() + accumulate(), scalar loops over dicts, nothing shared with the twin."""
    iou_thrs, rec_thrs, area_rng, max_dets = evaluate.coco_default_params()
    gt, ids, cat_of = case['gt'], case['image_ids'], case['category_ids']
    img_ids, cat_ids = sorted(ids), sorted(c['id'] for c in gt['categories'])
    gts, dts = {}, {}
    for ann in gt['annotations']:
        gts.setdefault((ann['image_id'], ann['category_id']), []).append(ann)
    did = 0
    for j in range(1, len(cat_of)):
        for pos, img in enumerate(ids):
            for row in case['dets'][pos, j - 1, :case['count'][pos, j - 1]].astype(np.float64):
                did += 1
                box = [row[0], row[1], row[2] - row[0] + 1, row[3] - row[1] + 1]
                dts.setdefault((img, cat_of[j]), []).append(
                    {'id': did, 'bbox': box, 'area': box[2] * box[3], 'score': row[4]})
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(cat_ids), len(area_rng), len(max_dets)
    precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
    for k, cat in enumerate(cat_ids):
        for a, (lo, hi) in enumerate(area_rng):
            per_image = []
            for img in img_ids:
                g_all, d_all = gts.get((img, cat), []), dts.get((img, cat), [])
                if not g_all and not d_all:
                    continue
                ign = [bool(g['iscrowd']) or g['area'] < lo or g['area'] > hi for g in g_all]
                gs = [g for g, i in zip(g_all, ign) if not i] + [g for g, i in zip(g_all, ign) if i]
                g_ig = sorted(ign)
                ds = sorted(d_all, key=lambda d: -d['score'])[:max_dets[-1]]         # sorted() is stable
                dtm, dt_ig = np.zeros((T, len(ds))), np.zeros((T, len(ds)), bool)
                gtm = np.zeros((T, len(gs)))
                for ti, t in enumerate(iou_thrs):
                    for di, d in enumerate(ds):
                        best, m = min(t, 1 - 1e-10), -1
                        for gi, g in enumerate(gs):
                            if gtm[ti, gi] > 0 and not g['iscrowd']:
                                continue
                            if m > -1 and not g_ig[m] and g_ig[gi]:
                                break
                            v = _naive_iou(d['bbox'], g['bbox'], g['iscrowd'])
                            if v < best:
                                continue
                            best, m = v, gi
                        if m == -1:
                            dt_ig[ti, di] = d['area'] < lo or d['area'] > hi
                            continue
                        dt_ig[ti, di], dtm[ti, di], gtm[ti, m] = g_ig[m], gs[m]['id'], d['id']
                per_image.append((ds, dtm, dt_ig, g_ig))
            npig = sum(1 for e in per_image for i in e[3] if not i)
            if npig == 0:
                continue
            for m, max_det in enumerate(max_dets):
                flat = [(d['score'], e[1][:, di], e[2][:, di]) for e in per_image for di, d in enumerate(e[0][:max_det])]
                flat.sort(key=lambda x: -x[0])
                nd = len(flat)
                for ti in range(T):
                    tp = fp = 0
                    rc, pr = [], []
                    for s, mt, ig in flat:
                        tp += bool(mt[ti]) and not ig[ti]
                        fp += not mt[ti] and not ig[ti]
                        rc.append(float(tp) / npig)
                        pr.append(float(tp) / (float(fp) + float(tp) + np.spacing(1)))
                    recall[ti, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q, ss = np.zeros(R), np.zeros(R)
                    for ri, thr in enumerate(rec_thrs):
                        pi = next((i for i in range(nd) if rc[i] >= thr), nd)
                        if pi == nd:
                            break
                        q[ri], ss[ri] = pr[pi], flat[pi][0]
                    precision[ti, :, k, a, m], scores[ti, :, k, a, m] = q, ss
    return precision, recall, scores


def test_random_case_against_the_naive_loop():
    case = cases.random_case()
    packed = evaluate.pack_coco_ground_truth(case['gt'], case['category_ids'], case['image_ids'])
    got = evaluate.coco_eval_arrays((case['dets'], case['count']), packed)
    want = _naive_coco(case)
    for name, x, y in zip(('precision', 'recall', 'scores'), got, want):
        assert np.array_equal(x, y), name
    p = got[0]
    assert ((p > 0) & (p < 1)).any() and (p == 0).any()
    stats = evaluate.coco_summarize(got[0], got[1], packed)[1]
    assert np.all((stats > 0) & (stats < 1))


def test_the_naive_loop_reproduces_the_golden_too():
    g = _golden()
    want = _naive_coco(g)
    assert np.array_equal(want[0], g['precision']) and np.array_equal(want[1], g['recall'])
    assert np.array_equal(want[2], g['scores'])


def test_golden_holds_the_hand_made_situations():
    """The places the issue names, found in the stored inputs themselves (tools/gen_coco_golden.py build_case)."""
    g = _golden()
    packed, _ = _golden_arrays()
    ids, cats = g['image_ids'], g['category_ids']
    thr = np.minimum(evaluate.coco_default_params()[0], 1 - 1e-10)
    area_rng = packed.area_rng

    def segment(img, cat):
        """-> (sorted xywh boxes, scores, matched, ignored [T,A,D], the segment's ground-truth rows)."""
        i, j = ids.index(img), cats.index(cat)
        row = g['dets'][i, j - 1, :g['count'][i, j - 1]].astype(np.float64)
        row = row[np.argsort(-row[:, 4], kind='stable')[:100]]
        box = np.stack([row[:, 0], row[:, 1], row[:, 2] - row[:, 0] + 1, row[:, 3] - row[:, 1] + 1], axis=1)
        r = packed.image_rank[i]
        sel = np.flatnonzero(packed.label[packed.off[r]:packed.off[r + 1]] == j) + packed.off[r]
        crowd, ga, da = packed.iscrowd[sel].astype(bool), packed.area[sel], box[:, 2] * box[:, 3]
        gt_ignore = crowd[None] | (ga[None] < area_rng[:, :1]) | (ga[None] > area_rng[:, 1:])
        det_out = (da[None] < area_rng[:, :1]) | (da[None] > area_rng[:, 1:])
        m, ig = evaluate._coco_match_segment(evaluate.coco_bbox_iou(box, packed.boxes[sel], crowd), crowd, gt_ignore,
                                             det_out, thr)
        return box, row[:, 4], m, ig, sel

    # an IoU of exactly 0.5 matches at t = 0.5 and not at 0.55; annotation areas of exactly 32^2 and 96^2 count in two
    # ranges; detection areas exactly on a bound are inside both ranges
    box, score, m, ig, sel = segment(139, 18)
    d = int(np.flatnonzero((box == [1000, 0, 10, 10]).all(1))[0])
    gsel = sel[(packed.boxes[sel] == [1000, 0, 10, 20]).all(1)]
    assert evaluate.coco_bbox_iou(box[d:d + 1], packed.boxes[gsel], [False])[0, 0] == 0.5
    assert m[0, 0, d] and not m[1, 0, d]
    for edge, (lo_rng, hi_rng) in ((32 ** 2, (1, 2)), (96 ** 2, (2, 3))):
        assert (packed.area[sel] == edge).any() and not (packed.boxes[sel][:, 2] * packed.boxes[sel][:, 3] == edge).any()
        on = np.flatnonzero(box[:, 2] * box[:, 3] == edge)
        assert len(on) == 1 and not m[:, :, on[0]].any() and not ig[:, [lo_rng, hi_rng], on[0]].any()
        assert ig[:, 3 if edge == 32 ** 2 else 1, on[0]].all()
    assert len(np.unique(score)) < len(score)                           # equal scores inside a segment
    # a detection that takes an ignored box only because the regular one is taken; a crowd takes any number
    box, score, m, ig, sel = segment(42, 3)
    first, second, third = (int(np.flatnonzero((box[:, :2] == xy).all(1))[0]) for xy in ([1000, 500], [1002, 502], [1004, 504]))
    assert first < second < third and score[second] == score[third]
    assert m[0, 0, first] and not ig[0, 0, first]
    assert m[0, 0, second] and ig[0, 0, second] and m[0, 0, third] and ig[0, 0, third]
    regular = sel[(packed.boxes[sel] == [1000, 500, 100, 100]).all(1)]
    assert evaluate.coco_bbox_iou(box[second:second + 1], packed.boxes[regular], [False])[0, 0] > 0.5
    # ... and a box ignored by its area alone is taken once: the third detection there is unmatched at t = 0.5
    a, b, c = (int(np.flatnonzero((box[:, :2] == xy).all(1))[0]) for xy in ([1300, 500], [1301, 501], [1301, 500]))
    # (area range 2, `medium`: the 50 x 50 box is regular there, the one with area 20000 is not)
    assert m[0, 2, a] and not ig[0, 2, a] and m[0, 2, b] and ig[0, 2, b] and not m[0, 2, c]
    # equal scores across images; a segment with more than 100 rows stored worst first; coordinates with two decimals
    per_image = [set(g['dets'][i, 0, :g['count'][i, 0], 4].tolist()) for i in range(len(ids))]
    assert per_image[0] & per_image[2]
    i, j = ids.index(57), cats.index(3)
    many = g['dets'][i, j - 1, :g['count'][i, j - 1], 4]
    assert len(many) > 130 and np.all(np.diff(many[-130:]) >= 0) and len(np.unique(many[-130:])) < 130
    assert any(round(v * 100) % 100 not in (0, 50) for ann in g['gt']['annotations'] for v in ann['bbox'])
    # an image without boxes (it has detections) and one that is never fed (it has boxes)
    counts = np.diff(packed.off)
    assert counts[packed.image_rank[ids.index(724)]] == 0 and g['count'][ids.index(724)].sum() > 0
    assert counts[packed.image_rank[g['never_fed']]] > 0
