"""The host twin of the device augmentation planner (ctdet/aug_plan_ref.py), without a GPU: the generator's known
answers, the sampler's invariants recomputed with utils.box_utils.matrix_iou and plain numpy, the round caps, the
distribution against the host sampler `preproc.decide`, and independence from the batch."""
import math
import random

import numpy as np
import pytest

import aug_plan_cases as cases
from ctdet import aug_plan_ref as ref
from data.data_augment import CROP_MODES, preproc
from utils.box_utils import matrix_iou


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in ref.philox4x32(*ctr, *key)) == want
    # vectorised over the lane word, and the counter layout of draws(): (sample_id lo, hi, slot, lane)
    sid, seed = 0x85a308d3243f6a88, 0x299f31d0a4093822
    got = ref.draws(seed, sid, 0x13198a2e, np.array([0x03707344, 5]))
    assert tuple(int(v) for v in got[0]) == kat[2][2]
    assert tuple(int(v) for v in got[1]) == tuple(int(v) for v in ref.philox4x32(0x243f6a88, 0x85a308d3, 0x13198a2e, 5,
                                                                                  0xa4093822, 0x299f31d0))


def _crop_trial(words, H, W, boxes, labels, mode, cls):
    """One trial of data_augment.py `_crop` on the draw-table words, in the reference's scalar form: the roi or None."""
    u = [int(w) * 2.0 ** -32 for w in words]
    scale = 0.3 + (1. - 0.3) * u[0]
    lo, hi = max(0.5, scale * scale), min(2, 1. / scale / scale)
    ratio = math.sqrt(lo + (hi - lo) * u[1])
    w, h = int(scale * ratio * W), int((scale / ratio) * H)
    if w < 1 or h < 1 or w >= W or h >= H:
        return None
    l, t = (int(words[2]) * (W - w)) >> 32, (int(words[3]) * (H - h)) >> 32
    roi = np.array((l, t, l + w, t + h))
    iou = matrix_iou(boxes, roi[np.newaxis])
    min_iou = float('-inf') if mode[0] is None else mode[0]
    max_iou = float('inf') if mode[1] is None else mode[1]
    if not (min_iou <= iou.min() and iou.max() <= max_iou):
        return None
    centers = (boxes[:, :2] + boxes[:, 2:]) / 2
    inside = np.logical_and(roi[:2] < centers, centers < roi[2:]).all(axis=1)
    if not inside.any() or (cls >= 0 and (labels[inside] != (cls + 1)).all()):
        return None
    return l, t, w, h


def _reference_rows(plan, boxes, labels, cropped):
    """The box arithmetic of `preproc._crop` / `_expand` / `decide` applied to a finished plan."""
    l, t, w, h = plan['crop']
    roi = np.array((l, t, l + w, t + h))
    bt, lt = boxes.copy(), labels.copy()
    if cropped:
        centers = (boxes[:, :2] + boxes[:, 2:]) / 2
        inside = np.logical_and(roi[:2] < centers, centers < roi[2:]).all(axis=1)
        bt, lt = boxes[inside].copy(), labels[inside].copy()
        bt[:, :2] = np.maximum(bt[:, :2], roi[:2]) - roi[:2]
        bt[:, 2:] = np.minimum(bt[:, 2:], roi[2:]) - roi[:2]
    ew, eh, left, top = plan['exp']
    if (ew, eh, left, top) != (w, h, 0, 0):
        bt[:, :2] += (left, top)
        bt[:, 2:] += (left, top)
    if plan['mirror']:
        bt[:, 0::2] = ew - bt[:, 2::-2]
    bt[:, 0::2] /= ew
    bt[:, 1::2] /= eh
    keep = np.minimum(bt[:, 2] - bt[:, 0], bt[:, 3] - bt[:, 1]) > 0.01
    return np.hstack((bt[keep], lt[keep][:, None]))


@pytest.mark.parametrize('p', cases.P_VALUES)
def test_twin_invariants(p):
    samples, boxes, n_img, res = cases.twin(p)
    assert res.status.tolist()[:3] == [0, 0, 0]
    checked = dict(cropped=0, lower=0, fallback=0, expanded=0)
    for i, s in enumerate(samples):
        info, plan = res.info[i], ref.plan_dict(res.plans[i])
        H, W, cls = int(s['H']), int(s['W']), int(s['cls'])
        tg = boxes[s['box_begin']:s['box_end']][:cases.MAX_GT].astype(np.float64)
        bx, lab = tg[:, :4], tg[:, 4]
        rows = res.sample_rows[i]
        l, t, w, h = plan['crop']
        ew, eh, left, top = plan['exp']
        if info['fallback']:
            checked['fallback'] += 1
            assert (l, t, w, h) == (0, 0, W, H) and plan['exp'] == (W, H, 0, 0)
            assert plan['mirror'] == 0 and plan['flags'] == 0
            want = tg.copy()
            want[:, 0:4:2] /= W
            want[:, 1:4:2] /= H
        else:
            if info['cropped']:
                checked['cropped'] += 1
                assert 1 <= w < W and 1 <= h < H and l >= 0 and t >= 0 and l + w <= W and t + h <= H
                r, lane, mode = info['crop_rounds'] - 1, info['crop_lane'], CROP_MODES[info['crop_mode']]
                d = ref.draws(cases.SEED, s['sample_id'], ref.SLOT_CROP + r, np.arange(64))
                assert CROP_MODES[(int(d[63, 0]) * 7) >> 32] == mode and mode is not None
                assert 0 <= lane < 50
                assert _crop_trial(d[lane], H, W, bx, lab, mode, cls) == (l, t, w, h)
                for k in range(lane):
                    assert _crop_trial(d[k], H, W, bx, lab, mode, cls) is None
                    checked['lower'] += 1
            else:
                assert (l, t, w, h) == (0, 0, W, H)
            assert ew >= w and eh >= h and 0 <= left <= ew - w and 0 <= top <= eh - h
            checked['expanded'] += (ew, eh) != (w, h)
            want = _reference_rows(plan, bx, lab, info['cropped'])
            assert len(want) > 0
        if s['flags'] & 2:                              # data/voc0712.py:237-238
            want[1:, 4] = -1
        assert np.array_equal(rows[:, :5], want.astype(np.float32))
        if s['flags'] == 0:
            assert (rows[:, 5] == s['weight']).all()
    if p == 0.6:
        assert checked['cropped'] > 300 and checked['lower'] > 300 and checked['fallback'] > 64
    assert (checked['expanded'] == 0) == (p == 0.0)


def test_flags_and_row_order():
    """Rows of an image are those of its samples in sample order; flags 1 and 2 as data/voc0712.py:237-238, 271-273."""
    samples, boxes, n_img, res = cases.twin(0.6)
    pos = 0
    for img in range(n_img):
        mine = np.flatnonzero(samples['image'] == img)
        want = np.concatenate([res.sample_rows[i] for i in mine], 0)
        assert res.gt_off[img] == pos and res.gt_off[img + 1] == pos + len(want)
        assert np.array_equal(res.truths[pos:pos + len(want)], want)
        pos += len(want)
    seen = set()
    for i, s in enumerate(samples):
        f, rows = int(s['flags']), res.sample_rows[i]
        if s['sample_id'] < 500000 or s['sample_id'] >= 600000:
            continue
        if f & 2:
            assert (rows[1:, 4] == -1).all()
        if f & 1:
            assert (rows[rows[:, 4] == -1, 5] == 0).all() and (rows[rows[:, 4] != -1, 5] == s['weight']).all()
        else:
            assert (rows[:, 5] == s['weight']).all()
        seen.add((f, bool((rows[:, 4] == -1).any())))
    assert {(0, True), (1, True), (2, True), (3, True)} <= seen


def test_round_caps_never_shape_a_result():
    for p in cases.P_VALUES:
        res = cases.twin(p)[3]
        assert res.crop_rounds.max() <= 128, res.crop_rounds.max()
        assert res.expand_rounds.max() <= 32, res.expand_rounds.max()


def _stats(plan, tout, H, W):
    l, t, w, h = plan['crop']
    return [float((l, t, w, h) == (0, 0, W, H)), float(tuple(plan['exp'][:2]) != (w, h)), float(plan['mirror']),
            float(plan['flags'] & 1), float(plan['flags'] >> 1 & 1), float(plan['flags'] >> 2 & 1),
            float(plan['flags'] >> 3 & 1), float(len(tout)), w * h / float(W * H)]


def test_same_distribution_as_the_host_sampler():
    """1500 twin samples against 1500 `preproc.decide` samples of one 500x375 image with three boxes: every statistic
    agrees within five standard errors of the two-sample difference, computed from the samples themselves."""
    n, H, W, p = 1500, 375, 500, 0.6
    names = ['no crop', 'expanded', 'mirrored', 'brightness', 'contrast', 'hue', 'saturation', 'kept rows', 'crop area']
    host = preproc.__new__(preproc)                 # the decision logic alone: no device objects
    host.rng, host.p, host.interp_of_draw = random.Random(20240607), p, cases.INTERP
    tg = cases.B3.astype(np.float64)
    a = np.array([_stats(*host.decide((H, W, 3), tg), H, W) for _ in range(n)])
    s, b = ref.make_samples([(H, W)] * n, [cases.B3] * n, sample_ids=np.arange(n, dtype=np.uint64) + np.uint64(77000))
    res = ref.plan_batch(s, b, n, 8, cases.SEED, p, cases.INTERP, cases.FILL)
    bb = np.array([_stats(ref.plan_dict(res.plans[i]), res.sample_rows[i], H, W) for i in range(n)])
    for k, name in enumerate(names):
        diff = abs(a[:, k].mean() - bb[:, k].mean())
        se = math.sqrt(a[:, k].var(ddof=1) / n + bb[:, k].var(ddof=1) / n)
        print('%-10s host %.4f twin %.4f diff %.4f 5se %.4f' % (name, a[:, k].mean(), bb[:, k].mean(), diff, 5 * se))
        assert diff <= 5 * se, (name, a[:, k].mean(), bb[:, k].mean(), se)


def test_preproc_decisions_argument():
    """'host' is the default and has no device entry; 'device' refuses the tap filters, whose tables are host work."""
    pre = preproc(300, cases.FILL, 0.6)
    assert pre.decisions == 'host'
    with pytest.raises(ValueError, match="decisions='device'"):
        pre.batch_device([], [], [])
    with pytest.raises(ValueError, match='cv2'):
        preproc(300, cases.FILL, 0.6, filters='cv2', decisions='device', seed=1)
    with pytest.raises(ValueError, match='decisions'):
        preproc(300, cases.FILL, 0.6, decisions='gpu')
    assert preproc(300, cases.FILL, 0.6, filters='fast', decisions='device', seed=5).seed == 5


def test_result_does_not_depend_on_the_batch():
    """(seed, sample_id, size, boxes, cls) decide a sample: not its batch mates, its position or the sample order."""
    samples, boxes, n_img, res = cases.twin(0.6)
    pick = np.arange(0, len(samples), 37)
    shapes = [(int(samples[i]['H']), int(samples[i]['W'])) for i in pick]
    tgs = [boxes[samples[i]['box_begin']:samples[i]['box_end']] for i in pick]

    def run(order):
        s, b = ref.make_samples([shapes[k] for k in order], [tgs[k] for k in order],
                                sample_ids=samples['sample_id'][pick[order]], cls=samples['cls'][pick[order]],
                                weights=samples['weight'][pick[order]], flags=samples['flags'][pick[order]])
        return ref.plan_batch(s, b, len(order), cases.MAX_GT, cases.SEED, 0.6, cases.INTERP, cases.FILL)

    order = np.random.RandomState(5).permutation(len(pick))
    shuffled = run(order)
    for j, k in enumerate(order):
        i = pick[k]
        alone = run(np.array([k]))
        for got in ((shuffled.plans[j], shuffled.sample_rows[j]), (alone.plans[0], alone.sample_rows[0])):
            assert got[0].tobytes() == res.plans[i].tobytes()
            assert np.array_equal(got[1], res.sample_rows[i])
