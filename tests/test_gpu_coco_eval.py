"""The device COCO bbox evaluator (csrc/ct_coco_eval.hip, ctdet.evaluate.DeviceCOCOEvaluator) on the MI355X against
the golden of the reference's own COCOeval and against the host twin evaluate.coco_eval_arrays.  Every double
expression of the kernels is the host's and the scans are integer, so equality is the criterion everywhere: there is no
tolerance in this file."""
import functools
import types

import numpy as np
import pytest
import torch

import coco_eval_cases as cases
from ctdet import evaluate, harness, ops, synth
from ctdet._lib import CtdetError

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def _case(name):
    return cases.golden_case() if name == 'golden' else cases.random_case()


@functools.lru_cache(maxsize=None)
def _host(name):
    case = _case(name)
    packed = evaluate.pack_coco_ground_truth(case['gt'], case['category_ids'], case['image_ids'])
    arrays = evaluate.coco_eval_arrays((case['dets'], case['count']), packed)
    return arrays, evaluate.coco_summarize(arrays[0], arrays[1], packed)


def _feed(ev, dets, count, batches, device_index=False):
    T, cap = dets.shape[1], dets.shape[2]
    for idx in batches:
        idx = np.asarray(idx)
        d, c = np.zeros((len(idx), T, cap, 5), np.float32), np.zeros((len(idx), T), np.int32)
        d[idx >= 0], c[idx >= 0] = dets[idx[idx >= 0]], count[idx[idx >= 0]]
        d[idx < 0], c[idx < 0] = np.nan, cap                            # a padding image's rows must never be looked at
        index = torch.from_numpy(idx.astype(np.int32)).to(DEV) if device_index else idx.tolist()
        ev.add(torch.from_numpy(d).to(DEV), torch.from_numpy(c).to(DEV), index)


def _evaluator(case, **kw):
    return evaluate.DeviceCOCOEvaluator(case['gt'], case['category_ids'], DEV, case['image_ids'], **kw)


def _same_results(got, want):
    return list(got) == list(want) and all(got[k] == v or (np.isnan(v) and np.isnan(got[k])) for k, v in want.items())


def _assert_equal(ev, got, want_arrays, want_summary):
    results, stats = got
    for name, x, y in zip(('precision', 'recall', 'scores'), ev.arrays(), want_arrays):
        assert x.dtype == np.float64 and x.shape == y.shape
        assert np.array_equal(x, y), (name, int((x != y).sum()))
    assert np.array_equal(stats, want_summary[1])
    assert _same_results(results, want_summary[0])


@pytest.mark.parametrize('batches', [[list(range(14))],
                                     [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, -1, -1]]],
                         ids=['one_batch_of_14', 'batches_of_4_ragged'])
def test_golden_of_the_reference(batches):
    case = _case('golden')
    batches = [[i if i != case['never_fed'] else -1 for i in b] for b in batches]      # one image is never fed
    ev = _evaluator(case)
    _feed(ev, case['dets'], case['count'], batches)
    got = ev.finish()
    golden = (case['precision'], case['recall'], case['scores'])
    _assert_equal(ev, got, golden, _host('golden')[1])
    assert np.array_equal(got[1], case['stats'])


@pytest.mark.parametrize('device_index', [False, True], ids=['host_index', 'device_index'])
def test_random_case_against_the_host_twin(device_index):
    case = _case('random')
    fed = case['fed']
    batches = [fed[i:i + 32] for i in range(0, len(fed), 32)]
    batches[-1] = batches[-1] + [-1] * (32 - len(batches[-1]))
    ev = _evaluator(case)
    _feed(ev, case['dets'], case['count'], batches, device_index)
    got = ev.finish()
    _assert_equal(ev, got, *_host('random'))
    assert np.all((got[1] > 0) & (got[1] < 1))
    # a second round after reset() gives the same
    ev.reset()
    _feed(ev, case['dets'], case['count'], batches[::-1], device_index)
    _assert_equal(ev, ev.finish(), *_host('random'))


def test_segments_in_ascending_score_order():
    """The rank by counting: every segment stored worst first (equal scores then keep their stored order, so the host
    twin on the same rows is the reference)."""
    case = _case('random')
    dets = case['dets'].copy()
    for i, j in zip(*np.nonzero(case['count'])):
        k = case['count'][i, j]
        dets[i, j, :k] = dets[i, j, :k][np.argsort(dets[i, j, :k, 4], kind='stable')]
    assert any(np.all(np.diff(dets[i, j, :case['count'][i, j], 4]) >= 0) and case['count'][i, j] > 5
               for i, j in zip(*np.nonzero(case['count'])))
    packed = evaluate.pack_coco_ground_truth(case['gt'], case['category_ids'], case['image_ids'])
    want = evaluate.coco_eval_arrays((dets, case['count']), packed)
    ev = _evaluator(case)
    _feed(ev, dets, case['count'], [list(range(len(case['image_ids'])))])
    got = ev.finish()
    _assert_equal(ev, got, want, evaluate.coco_summarize(want[0], want[1], packed))


def test_overflow_raises_and_a_sufficient_cap_changes_nothing():
    case = _case('golden')
    kept = np.minimum(case['count'], 100).sum(1).max()
    batches = [[i for i in range(14) if i != case['never_fed']]]
    ev = _evaluator(case, per_image_cap=int(kept) - 1)
    _feed(ev, case['dets'], case['count'], batches)
    with pytest.raises(CtdetError, match='per_image_cap >= %d' % kept):
        ev.finish()
    ev = _evaluator(case, per_image_cap=int(kept))
    _feed(ev, case['dets'], case['count'], batches)
    _assert_equal(ev, ev.finish(), (case['precision'], case['recall'], case['scores']), _host('golden')[1])


def test_host_side_refusals():
    case = _case('golden')
    ev = _evaluator(case)
    d = torch.zeros(2, 5, 4, 5, device=DEV)
    c = torch.zeros(2, 5, dtype=torch.int32, device=DEV)
    ev.add(d, c, [0, 1])
    with pytest.raises(CtdetError, match='twice'):
        ev.add(d, c, [1, 2])
    with pytest.raises(CtdetError, match='outside'):
        ev.add(d, c, [3, 14])
    with pytest.raises(ValueError):
        ev.add(d[:, :4].contiguous(), c[:, :4].contiguous(), [3, 4])
    with pytest.raises(CtdetError, match='finish'):
        ev.arrays()
    # a device index out of range and a NaN score are met by the kernel and reported by finish()
    ev.add(d, c, torch.tensor([5, 99], dtype=torch.int32, device=DEV))
    with pytest.raises(CtdetError, match='out of range'):
        ev.finish()
    ev.reset()
    d[0, 0, 0, 4], c[0, 0] = float('nan'), 1
    ev.add(d, c, [0, 1])
    with pytest.raises(CtdetError, match='NaN'):
        ev.finish()


# ---------------------------------------------------------------- the accumulate kernel alone
def _key(k, score, img, rank):
    u = int(np.float32(score).view(np.uint32))
    u = (~u & 0xFFFFFFFF) if u & 0x80000000 else u | 0x80000000
    return (k << 56) | ((~u & 0xFFFFFFFF) << 24) | (img << 7) | rank


def _host_accumulate(recs, npig, K, pair_bits, max_dets, rec_thrs):
    """accumulate() on hand-made records [(k, score, img, rank, matched mask, ignored mask)], A = 1."""
    T, R, M = len(pair_bits), len(rec_thrs), len(max_dets)
    precision, recall, scores = -np.ones((T, R, K, 1, M)), -np.ones((T, K, 1, M)), -np.ones((T, R, K, 1, M))
    for k in range(K):
        if npig[k] == 0:
            continue
        for m, md in enumerate(max_dets):
            rows = sorted((r for r in recs if r[0] == k and r[3] < md), key=lambda r: (-np.float32(r[1]), r[2], r[3]))
            sc = np.asarray([np.float32(r[1]) for r in rows], dtype=np.float64)
            for t, bit in enumerate(pair_bits):
                mt = np.asarray([(r[4] >> bit) & 1 for r in rows], dtype=bool)
                ig = np.asarray([(r[5] >> bit) & 1 for r in rows], dtype=bool)
                tp = np.cumsum(mt & ~ig).astype(np.float64)
                fp = np.cumsum(~mt & ~ig).astype(np.float64)
                rc, pr = tp / int(npig[k]), tp / (fp + tp + np.spacing(1))
                recall[t, k, 0, m] = rc[-1] if len(rows) else 0
                pr = np.maximum.accumulate(pr[::-1])[::-1]
                at = np.searchsorted(rc, rec_thrs, side='left')
                ok = at < len(rows)
                q, ss = np.zeros(R), np.zeros(R)
                q[ok], ss[ok] = pr[at[ok]], sc[at[ok]]
                precision[t, :, k, 0, m], scores[t, :, k, 0, m] = q, ss
    return precision, recall, scores


@pytest.mark.parametrize('sorted_input', [False, True], ids=['with_order', 'already_sorted'])
def test_accumulate_alone_around_its_chunk_size(sorted_input):
    """Categories with chunk - 1, chunk, chunk + 1 records, one with none, one with npig == 0, a last one that spans
    three chunks; three thresholds on the mask bits 0, 1, 2."""
    chunk = 512                                                          # CT_COCO_ACC_CHUNK
    rng = np.random.RandomState(5)
    sizes = [chunk - 1, chunk, chunk + 1, 0, 40, 2 * chunk + 7]
    npig = np.asarray([300, 280, 310, 5, 0, 900], dtype=np.int32)
    recs = []
    for k, n in enumerate(sizes):
        for e in range(n):
            img, rank = e // 16, e % 16
            matched = int(rng.randint(0, 8)) if rng.rand() < 0.55 else 0
            ignored = int(rng.randint(0, 8)) if rng.rand() < 0.2 else 0
            recs.append((k, rng.randint(1, 200) / 200., img, rank, matched, ignored))
    perm = rng.permutation(len(recs))
    keys = np.asarray([_key(*recs[i][:4]) for i in perm], dtype=np.int64)
    assert len(set(keys.tolist())) == len(keys)
    matched = np.asarray([recs[i][4] for i in perm], dtype=np.int64)
    ignored = np.asarray([recs[i][5] for i in perm], dtype=np.int64)
    order = np.argsort(keys, kind='stable')
    if sorted_input:
        keys, matched, ignored, order = keys[order], matched[order], ignored[order], None
    K, max_dets, rec_thrs = len(sizes), [1, 10, 100], evaluate.coco_default_params()[1]
    off = np.searchsorted(np.sort(keys), np.arange(K + 1, dtype=np.int64) << 56).astype(np.int64)
    assert np.diff(off).tolist() == sizes
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                             # noqa: E731
    precision = torch.full((3, len(rec_thrs), K, 1, 3), 7., dtype=torch.float64, device=DEV)
    scores, recall = torch.full_like(precision, 7.), torch.full((3, K, 1, 3), 7., dtype=torch.float64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.coco_accumulate(up(keys), up(matched), up(ignored), None if order is None else up(order), up(off),
                        up(npig.reshape(K, 1)), up(np.asarray(max_dets, np.int32)), 3, up(rec_thrs), precision, recall,
                        scores, status)
    want = _host_accumulate(recs, npig, K, [0, 1, 2], max_dets, rec_thrs)
    assert int(status.item()) == 0
    for name, x, y in zip(('precision', 'recall', 'scores'), (precision, recall, scores), want):
        assert np.array_equal(x.cpu().numpy(), y), name
    assert np.all(want[0][:, :, 4] == -1) and np.all(want[1][:, 3] == 0) and np.all(want[0][:, :, 3] == 0)
    # an offset outside the records is reported and never dereferenced
    ops.coco_accumulate(up(keys), up(matched), up(ignored), None if order is None else up(order), up(off + 5),
                        up(npig.reshape(K, 1)), up(np.asarray(max_dets, np.int32)), 3, up(rec_thrs), precision, recall,
                        scores, status)
    assert int(status.item()) == 2


# ---------------------------------------------------------------- harness
class _Dataset:
    def __init__(self, imgs):
        self.imgs = imgs

    def __len__(self):
        return len(self.imgs)

    def pull_image(self, i):
        return self.imgs[i]


def test_harness_feeds_the_evaluator(tmp_path):
    """The 6 synthetic images of test_gpu_voc_eval.py at batch 4 (one ragged batch) with COCO-style ground truth made
    from the detections: do_test with the evaluator returns the host twin's results on the boxes it also returns; with
    keep_boxes=False the same results and no boxes."""
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
    image_ids = [907, 12, 440, 31, 5, 268]
    category_ids = [0] + [int(c) for c in rng.permutation(np.arange(1, 91))[:20]]
    anns = []
    for j in range(1, 21):
        for i in range(n):
            d = first[j][i]
            pick = d[:: max(1, len(d) // 3)][:3] if len(d) else d
            for row in pick:
                x1, y1, x2, y2 = np.round(row[:4] + rng.uniform(-3, 3, 4), 2)
                w, h = float(max(x2 - x1, 1.)), float(max(y2 - y1, 1.))
                anns.append({'id': len(anns) + 1, 'image_id': image_ids[i], 'category_id': category_ids[j],
                             'bbox': [float(x1), float(y1), w, h], 'area': float(np.round(w * h * rng.uniform(0.6, 1), 2)),
                             'iscrowd': int(rng.rand() < 0.15)})
    gt = {'images': [{'id': i} for i in image_ids], 'annotations': anns,
          'categories': [{'id': c, 'name': 'c%d' % c} for c in sorted(category_ids[1:])]}
    ev = evaluate.DeviceCOCOEvaluator(gt, category_ids, 'cuda', image_ids, per_image_cap=1024)
    all_boxes, (results, stats) = harness.do_test(net, priors, ds, tf, 20, str(tmp_path), batch=4, evaluator=ev)
    assert all(np.array_equal(all_boxes[j][i], first[j][i]) for j in range(1, 21) for i in range(n))
    want = evaluate.coco_eval_arrays(all_boxes, ev.packed)
    want_results, want_stats = evaluate.coco_summarize(want[0], want[1], ev.packed)
    assert all(np.array_equal(x, y) for x, y in zip(ev.arrays(), want))
    assert np.array_equal(stats, want_stats) and _same_results(results, want_results)
    assert 0 < stats[0] < 1 and (tmp_path / 'detections.pkl').exists()
    ev2 = evaluate.DeviceCOCOEvaluator(gt, category_ids, 'cuda', image_ids, per_image_cap=1024)
    boxes2, (results2, stats2) = harness.do_test(net, priors, ds, tf, 20, str(tmp_path / 'nb'), batch=4, evaluator=ev2,
                                                 keep_boxes=False)
    assert boxes2 is None and np.array_equal(stats2, want_stats) and _same_results(results2, want_results)
    assert not (tmp_path / 'nb' / 'detections.pkl').exists()
