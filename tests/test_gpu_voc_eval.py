"""The device VOC evaluator (csrc/ct_eval.hip, ctdet.evaluate.DeviceVOCEvaluator) on the MI355X against the golden of
data/voc_eval.py and against the host twin evaluate.voc_eval_lines(stable=True): rec and prec bit for bit, the
11-point AP equal, the area AP within (recall steps) x 2^-52 (its terms are the host's; np.sum adds them pairwise, the
kernel per thread and then as a tree, and each addition of a partial sum <= 1 errs by at most 2^-53 either way)."""
import functools
import types

import numpy as np
import pytest
import torch

import voc_eval_cases as cases
from ctdet import evaluate, harness, ops, synth
from ctdet._lib import CtdetError

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def _case(name):
    return cases.golden_case() if name == 'golden' else cases.random_case()


@functools.lru_cache(maxsize=None)
def _reference(name, ovthresh, m07):
    return cases.host_reference(_case(name), ovthresh, m07)


def _evaluate(case, batches, ovthresh=0.5, per_image_cap=None, device_index=False):
    """Feed `batches` (lists of data set indices, -1 = padding image) -> {metric: (aps, mean, {cls: (rec, prec)})}."""
    ev = evaluate.DeviceVOCEvaluator(case['gt'], case['classes'], case['ids'], DEV, ovthresh=ovthresh,
                                     per_image_cap=per_image_cap)
    T, cap = case['dets'].shape[1], case['dets'].shape[2]
    for idx in batches:
        idx = np.asarray(idx)
        dets, count = np.zeros((len(idx), T, cap, 5), np.float32), np.zeros((len(idx), T), np.int32)
        dets[idx >= 0], count[idx >= 0] = case['dets'][idx[idx >= 0]], case['count'][idx[idx >= 0]]
        dets[idx < 0], count[idx < 0] = np.nan, cap                     # a padding image's rows must never be looked at
        index = torch.from_numpy(idx.astype(np.int32)).to(DEV) if device_index else idx.tolist()
        ev.add(torch.from_numpy(dets).to(DEV), torch.from_numpy(count).to(DEV), index)
    out = {}
    for m07 in (True, False):
        aps, mean = ev.finish(use_07_metric=m07)
        out[m07] = (aps, mean, {c: ev.curves(c) for c in case['classes'][1:]})
    return out


def _check(got, name, ovthresh):
    case = _case(name)
    for m07 in (True, False):
        want = _reference(name, ovthresh, m07)
        aps, mean, curves = got[m07]
        assert list(aps) == case['classes'][1:]
        for cls in case['classes'][1:]:
            rec, prec, ap = want[cls]
            assert curves[cls][0].dtype == np.float64 and len(curves[cls][0]) == len(rec)
            assert np.array_equal(curves[cls][0], rec, equal_nan=True), (cls, m07)
            assert np.array_equal(curves[cls][1], prec), (cls, m07)
            if m07:
                assert aps[cls] == float(ap), (cls, aps[cls], float(ap))
            elif np.isnan(ap):
                assert np.isnan(aps[cls]), cls
            else:
                k = cases.recall_steps(rec)
                print('%s %s area AP: device %.17g host %.17g, %d recall steps' % (name, cls, aps[cls], float(ap), k))
                assert abs(aps[cls] - float(ap)) <= k * 2.0 ** -52, (cls, aps[cls], float(ap), k)
        host_mean = float(np.mean([float(want[c][2]) for c in case['classes'][1:]]))
        assert mean == host_mean or (np.isnan(mean) and np.isnan(host_mean)) or not m07 and abs(mean - host_mean) <= 2.0 ** -40


@pytest.mark.parametrize('batches', [[list(range(14))],
                                     [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, -1, -1]]],
                         ids=['one_batch_of_14', 'batches_of_4_ragged'])
def test_golden_of_the_reference(batches):
    case, g = _case('golden'), _case('golden')['golden']
    got = _evaluate(case, batches)
    for m07 in (True, False):
        aps, _, curves = got[m07]
        for ci, cls in enumerate(case['classes'][1:], 1):
            tag = 'c%d_%s' % (ci, '07' if m07 else 'area')
            assert np.array_equal(curves[cls][0], g[tag + '_rec']) and np.array_equal(curves[cls][1], g[tag + '_prec'])
            if m07:
                assert aps[cls] == float(g[tag + '_ap'])
            else:
                assert abs(aps[cls] - float(g[tag + '_ap'])) <= cases.recall_steps(g[tag + '_rec']) * 2.0 ** -52
    _check(got, 'golden', 0.5)


@pytest.mark.parametrize('ovthresh', [0.5, 0.75])
def test_randomised_against_the_stable_host_twin(ovthresh):
    case = _case('random')
    n = len(case['ids'])
    in_order = [list(range(s, min(s + 16, n))) + [-1] * max(0, s + 16 - n) for s in range(0, n, 16)]      # 4 x 16 + 6
    got = _evaluate(case, in_order, ovthresh)
    _check(got, 'random', ovthresh)
    # any order of add calls, any position inside a batch, image_index already on the device
    perm = np.random.RandomState(1).permutation(n).tolist()
    shuffled = [perm[40:70] + [-1, -1], [-1] + perm[0:3], perm[3:40]]
    again = _evaluate(case, shuffled, ovthresh, device_index=True)
    for m07 in (True, False):
        assert again[m07][0] == got[m07][0] or not m07          # area: NaN != NaN for the class without ground truth
        for cls in case['classes'][1:]:
            assert np.array_equal(again[m07][2][cls][0], got[m07][2][cls][0], equal_nan=True)
            assert np.array_equal(again[m07][2][cls][1], got[m07][2][cls][1])
            a, b = again[m07][0][cls], got[m07][0][cls]
            assert a == b or (np.isnan(a) and np.isnan(b))


def test_overflow_raises_and_a_sufficient_capacity_changes_nothing():
    case = _case('random')
    most = int(case['count'].sum(1).max())
    assert most == 80                                                    # image 5: both classes full
    batches = [list(range(0, 35)), list(range(35, 70))]
    with pytest.raises(CtdetError, match='per_image_cap >= %d' % most):
        _evaluate(case, batches, per_image_cap=most - 1)
    exact = _evaluate(case, batches, per_image_cap=most)
    _check(exact, 'random', 0.5)
    roomy = _evaluate(case, batches, per_image_cap=3 * most + 5)
    assert exact[True][0] == roomy[True][0] and exact[True][1] == roomy[True][1]


def test_add_refuses_what_the_host_can_see():
    case = _case('golden')
    ev = evaluate.DeviceVOCEvaluator(case['gt'], case['classes'], case['ids'], DEV)
    dets, count = torch.from_numpy(case['dets'][:4]).to(DEV), torch.from_numpy(case['count'][:4]).to(DEV)
    ev.add(dets, count, [0, 1, 2, 3])
    with pytest.raises(CtdetError, match='twice'):
        ev.add(dets, count, [4, 5, 6, 3])
    with pytest.raises(CtdetError, match='twice'):
        ev.add(dets, count, [4, 4, 5, 6])
    with pytest.raises(CtdetError, match='outside'):
        ev.add(dets, count, [4, 5, 6, 14])
    with pytest.raises(ValueError):
        ev.add(dets, count, [4, 5, 6])
    with pytest.raises(CtdetError):
        ev.add(dets.cpu(), count, [4, 5, 6, 7])
    with pytest.raises(CtdetError):
        ev.curves('bird')                                                # no finish() yet
    # an index the host cannot see (device tensor) beyond the data set: reported by finish(), nothing written
    ev.add(dets, count, torch.tensor([4, 5, 6, 99], dtype=torch.int32, device=DEV))
    with pytest.raises(CtdetError, match='out of range'):
        ev.finish()
    ev.reset()
    ev.add(dets, count, [0, 1, 2, 3])
    assert all(np.isfinite(v) for v in ev.finish()[0].values())


@pytest.mark.parametrize('n', [1, 2047, 2048, 2049, 5000])
def test_pr_kernel_across_chunk_boundaries(n):
    """ct_voc_pr on flags of its own: three classes (n rows, none, 77 rows without positives) with the rows permuted
    in memory; a chunk of the scan is 2048 rows."""
    rng = np.random.RandomState(n)
    sizes, num_pos = [n, 0, 77], np.array([max(1, n // 3), 4, 0], np.int32)
    total = sum(sizes)
    flags_sorted = rng.choice([0, 1, 2], total, p=[0.1, 0.3, 0.6]).astype(np.uint8)
    tp_room = np.cumsum(flags_sorted[:n] == 1) <= num_pos[0]             # never more true positives than positives
    flags_sorted[:n][~tp_room & (flags_sorted[:n] == 1)] = 2
    flags_sorted[n:][flags_sorted[n:] == 1] = 2                          # and none at all without positives
    order = rng.permutation(total + 9)[:total]                           # the sort's permutation; 9 unused slots
    flags = np.zeros(total + 9, np.uint8)
    flags[order] = flags_sorted
    ev = types.SimpleNamespace(
        T=3, flags=torch.from_numpy(flags).to(DEV), num_pos=torch.from_numpy(num_pos).to(DEV),
        rec=torch.full((total + 9,), -1.0, dtype=torch.float64, device=DEV),
        prec=torch.full((total + 9,), -1.0, dtype=torch.float64, device=DEV),
        ap=torch.empty(3, dtype=torch.float64, device=DEV), pr_status=torch.empty(1, dtype=torch.int32, device=DEV))
    off = np.concatenate([[0], np.cumsum(sizes)])
    for m07 in (True, False):
        ops.voc_pr(ev, torch.from_numpy(order).to(DEV), torch.from_numpy(off).to(DEV),
                   np.arange(0., 1.1, 0.1) if m07 else None)
        ap, rec, prec = ev.ap.cpu().numpy(), ev.rec.cpu().numpy(), ev.prec.cpu().numpy()
        assert int(ev.pr_status.item()) == 0
        assert np.all(rec[total:] == -1.0) and np.all(prec[total:] == -1.0)
        for c in range(3):
            f = flags_sorted[off[c]:off[c + 1]]
            tp, fp = np.cumsum(f == 1).astype(np.float64), np.cumsum(f == 2).astype(np.float64)
            with np.errstate(invalid='ignore', divide='ignore'):
                want_rec = tp / float(num_pos[c])
            want_prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
            assert np.array_equal(rec[off[c]:off[c + 1]], want_rec, equal_nan=True)
            assert np.array_equal(prec[off[c]:off[c + 1]], want_prec)
            with np.errstate(invalid='ignore'):
                want = float(evaluate.voc_ap(want_rec, want_prec, m07))
            if m07:
                assert ap[c] == want, (c, ap[c], want)
            elif np.isnan(want):
                assert c == 2 and np.isnan(ap[c])
            else:
                assert abs(ap[c] - want) <= cases.recall_steps(want_rec) * 2.0 ** -52, (c, ap[c], want)
    # a permutation entry or an offset out of range is reported, not followed
    bad = order.copy()
    bad[0] = total + 9
    ops.voc_pr(ev, torch.from_numpy(bad).to(DEV), torch.from_numpy(off).to(DEV), None)
    assert int(ev.pr_status.item()) == 2
    ops.voc_pr(ev, torch.from_numpy(order).to(DEV), torch.from_numpy(off + 10).to(DEV), None)
    assert int(ev.pr_status.item()) == 2


# ---------------------------------------------------------------- harness
class _Dataset:
    def __init__(self, imgs):
        self.imgs = imgs

    def __len__(self):
        return len(self.imgs)

    def pull_image(self, i):
        return self.imgs[i]


def test_harness_feeds_the_evaluator(tmp_path):
    """6 images at batch 4 (one ragged batch): do_test with an evaluator returns the APs of the host twin on the boxes
    it also returns; with keep_boxes=False the same APs and no boxes."""
    from data import VOC_300, BaseTransform
    from layers.functions import PriorBox
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), 300, 20)
    sd = synth.fill_state_dict(net.state_dict())
    sd['base.0.weight'] = sd['base.0.weight'] / 64      # synthetic weights expect unit-scale inputs, images are +-128
    net.load_state_dict(sd, strict=True)
    net = net.eval().cuda()
    net.device = 'cuda'
    priors = PriorBox(VOC_300).forward().cuda()
    rng = np.random.RandomState(9)
    shapes = [(375, 500), (500, 333), (120, 77), (300, 300), (333, 500), (480, 364)]
    imgs = [np.kron(rng.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8), np.ones((8, 8, 1), np.uint8))[:h, :w]
            for h, w in shapes]
    imgs = [np.ascontiguousarray(im) for im in imgs]
    n = len(imgs)
    tf = BaseTransform(300, (104, 117, 123), (2, 0, 1), max_batch=4)
    ds = _Dataset(imgs)
    first = harness.detect_dataset(net, priors, ds, tf, 20, batch=4)
    # synthetic ground truth: a jittered subset of the detections, so that the AP is neither 0 nor 1
    classes = ['__background__'] + ['c%d' % j for j in range(1, 21)]
    ids = ['img%03d' % i for i in range(n)]
    gt = {c: {} for c in classes[1:]}
    for j in range(1, 21):
        for i in range(n):
            d = first[j][i]
            pick = d[:: max(1, len(d) // 3)][:3] if len(d) else d
            if len(pick):
                bb = np.round(pick[:, :4] + rng.uniform(-3, 3, (len(pick), 4))).astype(int)
                gt[classes[j]][ids[i]] = {'bbox': bb, 'difficult': rng.rand(len(bb)) < 0.2}
    ev = evaluate.DeviceVOCEvaluator(gt, classes, ids, 'cuda', per_image_cap=1024)
    all_boxes, (aps, mean) = harness.do_test(net, priors, ds, tf, 20, str(tmp_path), batch=4, evaluator=ev)
    assert all(np.array_equal(all_boxes[j][i], first[j][i]) for j in range(1, 21) for i in range(n))
    want_aps, want_mean = evaluate.evaluate_detections(all_boxes, ids, gt, classes, stable=True)
    assert aps == want_aps and mean == want_mean
    assert 0.05 < mean < 0.999 and (tmp_path / 'detections.pkl').exists()
    ev2 = evaluate.DeviceVOCEvaluator(gt, classes, ids, 'cuda', per_image_cap=1024)
    boxes2, (aps2, mean2) = harness.do_test(net, priors, ds, tf, 20, str(tmp_path / 'nb'), batch=4, evaluator=ev2,
                                            keep_boxes=False)
    assert boxes2 is None and aps2 == want_aps and mean2 == want_mean
    assert not (tmp_path / 'nb' / 'detections.pkl').exists()
    with pytest.raises(ValueError):
        harness.do_test(net, priors, ds, tf, 20, str(tmp_path), batch=4, keep_boxes=False)
