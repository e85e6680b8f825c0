"""The TAL matcher (matcher='tal', ct_tal_match_batched) as far as it can be checked without a GPU: the numpy twin against a
second, float64 brute-force formulation and against numbers worked out by hand, the criterion's arguments and environment, the
refusals of the C entry (all before any HIP call) and the header."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from ctdet import _lib, ops
from layers.modules.multibox_loss_combined import MultiBoxLoss_combined

import atss_cases
import tal_cases
import tal_ref

FLT_MIN = float(np.finfo(np.float32).tiny)


def _crit(**kw):
    return MultiBoxLoss_combined(21, 0.5, True, 0, True, 3, 0.5, False, **kw)


# ------------------------------------------------------------------------------------ 1: the twin
def brute_force(c):
    """The rule once more in float64 and in another shape: the metric is a direct score**alpha * iou**beta on the same fp32
    inputs, the positives of a box come from one lexsort, all claims of an image are listed first and the conflicts settled by
    one sort over the list.  -> per image: owner [P] (box index or -1), per box (eligible, positives, forced, gap, low) with
    low = a metric lies within a factor 2 of FLT_MIN, where float32 and float64 may disagree on eligibility."""
    pri, index = c.priors.numpy().astype(np.float64), np.arange(len(c.priors))
    out = []
    for b, t in enumerate(c.targets):
        t = t.numpy().astype(np.float64).reshape(-1, 6)
        pb, ps = c.boxes[b].numpy().astype(np.float64), c.scores[b].numpy().astype(np.float64)
        claims, boxes = [], {}
        for g, (x1, y1, x2, y2, label, _) in enumerate(t[:c.max_gt]):
            if not (x2 > x1 and y2 > y1):
                continue
            inside = (x1 < pri[:, 0]) & (pri[:, 0] < x2) & (y1 < pri[:, 1]) & (pri[:, 1] < y2)
            with np.errstate(invalid='ignore', over='ignore'):
                iw = np.clip(np.minimum(x2, pb[:, 2]) - np.maximum(x1, pb[:, 0]), 0, None)
                ih = np.clip(np.minimum(y2, pb[:, 3]) - np.maximum(y1, pb[:, 1]), 0, None)
                u = iw * ih / ((x2 - x1) * (y2 - y1) + (pb[:, 2] - pb[:, 0]) * (pb[:, 3] - pb[:, 1]) - iw * ih)
                u = np.where(u > 0, u, 0.0)
                s = ps[:, int(label)] if label == int(label) and 1 <= label <= ps.shape[1] - 1 else 1.0 - ps[:, 0]
                s = np.where(s > 0, s, 0.0)
                m = np.where(inside, s ** c.alpha * u ** c.beta, 0.0)
            low = bool(((m > FLT_MIN / 2) & (m < FLT_MIN * 2)).any())
            m = np.where(m >= FLT_MIN, m, 0.0)
            eligible = int((m > 0).sum())
            if eligible == 0:
                iw = np.clip(np.minimum(x2, pri[:, 0] + pri[:, 2] / 2) - np.maximum(x1, pri[:, 0] - pri[:, 2] / 2), 0, None)
                ih = np.clip(np.minimum(y2, pri[:, 1] + pri[:, 3] / 2) - np.maximum(y1, pri[:, 1] - pri[:, 3] / 2), 0, None)
                pu = iw * ih / ((x2 - x1) * (y2 - y1) + pri[:, 2] * pri[:, 3] - iw * ih)
                p = int(np.argmax(pu))
                claims.append((True, pu[p], -g, p))
                boxes[g] = (0, 1, True, None, low)
                continue
            order = np.lexsort((index, -m))[:eligible]
            pos = order[:c.topk]
            gap = (m[pos[-1]] - m[order[len(pos)]]) / m[pos[-1]] if eligible > len(pos) else None
            claims += [(False, u[p], -g, int(p)) for p in pos]
            boxes[g] = (eligible, len(pos), False, gap, low)
        owner = np.full(len(pri), -1)
        for _, _, g, p in sorted(claims):                   # the worst claim first, the winning one written last
            owner[p] = -g
        out.append((owner, boxes))
    return out


@pytest.mark.parametrize('topk,alpha,beta', tal_cases.PARAMS)
@pytest.mark.parametrize('name', ['small', 'A', 'B'])
def test_twin_against_the_float64_brute_force(name, topk, alpha, beta):
    c = tal_cases.case(name, topk, alpha, beta)
    ref = c.ref
    brute = brute_force(c)
    smallest = math.inf
    for b, (owner, boxes) in enumerate(brute):
        t = c.targets[b].numpy()
        assert len(boxes) == len(ref.gaps[b]) == len(t)         # no box of these cases is skipped
        for (g, (eligible, npos, forced, gap, low)), twin_gap in zip(sorted(boxes.items()), ref.gaps[b]):
            # the fp32 chain rounds at most 10 times (IoU 5, sqrt 1, the products): 10 * 2^-24 < 2^-20 relative, so a gap of
            # 2^-18 in both formulations cannot be crossed; an exact tie is decided by the index in both
            assert (gap is None) == (twin_gap is None), (b, g)
            if gap is not None:
                assert (gap == 0 and twin_gap == 0) or (gap >= 2.0 ** -18 and twin_gap >= 2.0 ** -18), (b, g, gap, twin_gap)
                smallest = min(smallest, gap if gap > 0 else math.inf)
            assert not low, (b, g)                              # nor does eligibility hang on the FLT_MIN clause
            assert tuple(ref.gt_stats[b, g, [0, 1, 3]]) == (eligible, npos, forced), (b, g)
        assert np.array_equal(owner, ref.owner[b])              # every positive set, and every conflict
        got = owner >= 0
        assert np.array_equal(ref.conf_t[b][got], t[owner[got]][:, 4:6])
        assert np.array_equal(ref.obj_t[b][got], t[owner[got], 4] != 0)
        # every other prior: zeros and (0, 1), exactly
        assert not ref.loc_t[b][~got].any() and not ref.overlap[b][~got].any() and not ref.obj_t[b][~got].any()
        assert (ref.conf_t[b][~got] == (0, 1)).all()
        # loc_t of the assigned priors against utils/box_utils.py::encode in float64
        m, p = t[owner[got]].astype(np.float64), c.priors.numpy()[got].astype(np.float64)
        want = np.stack([((m[:, 0] + m[:, 2]) / 2 - p[:, 0]) / (0.1 * p[:, 2]), ((m[:, 1] + m[:, 3]) / 2 - p[:, 1]) / (0.1 * p[:, 3]),
                         np.log((m[:, 2] - m[:, 0]) / p[:, 2]) / 0.2, np.log((m[:, 3] - m[:, 1]) / p[:, 3]) / 0.2], 1)
        assert np.allclose(ref.loc_t[b][got], want, rtol=1e-5, atol=2e-5) and np.isfinite(ref.loc_t[b]).all()
    print(name, (topk, alpha, beta), 'smallest non-zero gap %.3g' % smallest, 'positives',
          [int((ref.owner[b] >= 0).sum()) for b in range(len(c.targets))], 'eligible', sorted(set(ref.gt_stats[..., 0].ravel())))


def test_small_pyramid_box_0_by_hand():
    """Box 0 = (1/16, 1/16, 7/16, 7/16), label 1.  Prior centres strictly inside: level 0 (centres 1/8, 3/8, ...) cells (0,0),
    (0,1), (1,0), (1,1) = priors 0 1, 2 3, 8 9, 10 11; level 1 (centres 1/4, 3/4) cell (0,0) = priors 32 33; level 2 (centre
    1/2) none.  Predicted boxes with dyadic IoUs: the box itself (u = 1); its upper half (1/16, 1/16, 7/16, 1/4): inter = 9/128,
    union = 9/64, u = 1/2; its quarter (1/16, 1/16, 1/4, 1/4): u = 1/4.  With alpha = 1, beta = 2, m = s * u * u:
        prior   0     1     2     3     8     9        10    11    32    33
        s       1/2   1     1/4   1     0     1        1/8   1/2   1/2   1/16
        u       1     1/2   1     1/4   1     0 (off)  1/2   1/2   1/2   1
        m       1/2   1/4   1/4   1/16  0     0        1/32  1/8   1/8   1/16
    8 eligible.  Descending (m, then index): 0, 1, 2, 11, 32, 3, 33, 10.  Every other prior predicts the box itself with score
    1 (m = 1) and must not matter: its centre is outside."""
    pri = atss_cases.small_pyramid()[0].numpy()
    t = atss_cases.SMALL_BOXES[0].numpy()
    full, half, quarter, off = (1 / 16, 1 / 16, 7 / 16, 7 / 16), (1 / 16, 1 / 16, 7 / 16, 1 / 4), (1 / 16, 1 / 16, 1 / 4, 1 / 4), (2, 2, 3, 3)
    boxes = np.tile(np.array(full, np.float32), (41, 1))
    scores = np.zeros((41, 5), np.float32)
    scores[:, 1] = 1
    table = {0: (1 / 2, full), 1: (1, half), 2: (1 / 4, full), 3: (1, quarter), 8: (0, full), 9: (1, off), 10: (1 / 8, half),
             11: (1 / 2, half), 32: (1 / 2, half), 33: (1 / 16, full)}
    for p, (s, box) in table.items():
        scores[p, 1], boxes[p] = s, box
    sel = tal_ref.box_select(t, pri, boxes, scores, 3, 2, 2)
    assert sorted(np.nonzero(sel.inside)[0]) == sorted(table)
    assert {p: float(sel.m[p]) for p in table} == {0: 1 / 2, 1: 1 / 4, 2: 1 / 4, 3: 1 / 16, 8: 0, 9: 0, 10: 1 / 32, 11: 1 / 8,
                                                   32: 1 / 8, 33: 1 / 16}
    assert not sel.m[~sel.inside].any()
    assert (sel.eligible, list(sel.idx), list(sel.u), float(sel.last), sel.forced, sel.gap) == (8, [0, 1, 2], [1, 0.5, 1], 0.25, False, 0.5)
    for topk, want, last, gap in ((1, [0], 1 / 2, 0.5), (2, [0, 1], 1 / 4, 0.0), (4, [0, 1, 2, 11], 1 / 8, 0.0),
                                  (5, [0, 1, 2, 11, 32], 1 / 8, 0.5), (8, [0, 1, 2, 11, 32, 3, 33, 10], 1 / 32, None),
                                  (16, [0, 1, 2, 11, 32, 3, 33, 10], 1 / 32, None)):
        sel = tal_ref.box_select(t, pri, boxes, scores, topk, 2, 2)
        assert (list(sel.idx), float(sel.last), sel.gap) == (want, last, gap), topk
    # the metric's order of operations, on values where every step is exact: sqrt(1/4) = 1/2
    assert float(tal_ref.metric(0.25, 0.5, 1, 1)) == 0.25 and float(tal_ref.metric(0.25, 0.5, 3, 1)) == 1 / 16
    assert float(tal_ref.metric(0.25, 0.5, 0, 0)) == 1 and float(tal_ref.metric(0.25, 0.5, 4, 8)) == 2.0 ** -12
    assert float(tal_ref.metric(2.0 ** -60, 2.0 ** -20, 2, 4)) == 0 and float(tal_ref.metric(2.0 ** -60, 2.0 ** -16, 2, 4)) == 2.0 ** -124
    # the batch form on the same arrays: box 0 alone, label 1 and weight 1 on its three priors, stats = (8, 3, 1/4, 0)
    ref = tal_ref.match([t], pri, boxes[None], scores[None], 3, 1.0, 2)
    assert list(np.nonzero(ref.owner[0] >= 0)[0]) == [0, 1, 2] and tuple(ref.gt_stats[0, 0]) == (8, 3, 0.25, 0)
    assert (ref.conf_t[0, :3] == (1, 1)).all() and list(ref.overlap[0, :3]) == [1, 0.5, 1] and ref.obj_t[0, :3].all()
    # a label that names no score column (0, -1, 7, 1.5) ranks by 1 - background: scores[:, 0] is 0 here, so s = 1, m = u * u
    for label in (0, -1, 7, 1.5):
        sel = tal_ref.box_select(np.concatenate([t[:4], [label, 1]]).astype(np.float32), pri, boxes, scores, 3, 2, 2)
        assert (sel.eligible, list(sel.idx)) == (9, [0, 2, 8]), label


def test_edge_cases_on_the_twin():
    ref = tal_cases.edge('empty').ref
    assert not ref.loc_t.any() and not ref.obj_t.any() and (ref.conf_t == (0, 1)).all() and not ref.gt_stats.any()
    ref = tal_cases.edge('degenerate').ref
    assert not ref.gt_stats[0, 0].any() and ref.gt_stats[0, 1, 0] > 13 and set(np.unique(ref.conf_t[0, :, 0])) == {0.0, 4.0}
    for name in ('tiny', 'moved_off'):
        ref = tal_cases.edge(name).ref
        assert tuple(ref.gt_stats[0, 0]) == (0, 1, 0, 1) and int((ref.owner[0] >= 0).sum()) == 1, name
        assert 0 < ref.overlap[0].max() < 1
    c = tal_cases.edge('moved_off')
    x1, y1, x2, y2 = tal_cases.EDGE_BOX
    p = c.priors.numpy()
    assert ((x1 < p[:, 0]) & (p[:, 0] < x2) & (y1 < p[:, 1]) & (p[:, 1] < y2)).sum() > 1000      # centres inside, all at u = 0
    ref = tal_cases.edge('identical').ref
    assert np.array_equal(ref.gt_stats[0, 0], ref.gt_stats[0, 1]) and ref.gt_stats[0, 0, 1] == 13
    assert set(ref.owner[0]) == {-1, 0} and set(ref.conf_t[0, :, 1]) == {1.0}          # the lower index wins every prior
    ref = tal_cases.edge('nan_inf').ref
    assert np.isfinite(ref.loc_t).all() and np.isfinite(ref.overlap).all() and (ref.gt_stats[0, :, 1] == 13).all()
    ref = tal_cases.edge('ignored').ref
    assert set(map(tuple, ref.conf_t[0][ref.owner[0] >= 0])) == {(-1.0, np.float32(0.37))} and ref.gt_stats[0, 0, 1] == 13
    assert ref.obj_t[0][ref.owner[0] >= 0].all()
    full, cut = tal_cases.case('A').ref, tal_cases.case('A', 13, 1.0, 6, 'host', 2).ref
    assert cut.gt_stats.shape == (3, 2, 4) and np.array_equal(cut.gt_stats, full.gt_stats[:, :2]) and cut.owner.max() == 1


# ------------------------------------------------------------------------------------ 2: the criterion's switches
ENV = ('CTDET_MATCHER', 'CTDET_ATSS_TOPK', 'CTDET_TAL_TOPK', 'CTDET_TAL_ALPHA', 'CTDET_TAL_BETA')


def test_defaults_environment_and_arguments(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    crit = _crit()
    assert (crit.matcher, crit.tal_topk, crit.tal_alpha, crit.tal_beta) == ('ssd', 13, 1.0, 6)
    crit = _crit(matcher='tal')
    assert (crit.matcher, crit.tal_topk, crit.tal_alpha, crit.tal_beta) == ('tal', 13, 1.0, 6)
    for k in ENV:
        monkeypatch.setenv(k, '')
    crit = _crit()
    assert (crit.matcher, crit.tal_topk, crit.tal_alpha, crit.tal_beta) == ('ssd', 13, 1.0, 6)
    monkeypatch.setenv('CTDET_MATCHER', 'tal')
    monkeypatch.setenv('CTDET_TAL_TOPK', '10')
    monkeypatch.setenv('CTDET_TAL_ALPHA', '0.5')
    monkeypatch.setenv('CTDET_TAL_BETA', '4')
    crit = _crit()
    assert (crit.matcher, crit.tal_topk, crit.tal_alpha, crit.tal_beta) == ('tal', 10, 0.5, 4)
    crit = _crit(matcher='atss', tal_topk=16, tal_alpha=2, tal_beta=0)          # arguments win over the environment
    assert (crit.matcher, crit.tal_topk, crit.tal_alpha, crit.tal_beta) == ('atss', 16, 2.0, 0)
    assert _lib.MATCHERS == ('ssd', 'atss') and _lib.PRED_MATCHERS == ('tal',)
    # overlap_thresh and level_offsets are accepted and not read under tal
    assert MultiBoxLoss_combined(21, None, True, 0, True, 3, 0.5, False, matcher='tal').level_offsets is None


def test_bad_values_raise_value_error(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for kw in (dict(matcher='TAL'), dict(tal_topk=0), dict(tal_topk=17), dict(tal_topk=2.5), dict(tal_alpha=0.3),
               dict(tal_alpha=2.5), dict(tal_alpha=-0.5), dict(tal_beta=9), dict(tal_beta=-1), dict(tal_beta=1.5),
               dict(matcher='tal', tal_topk=0)):
        with pytest.raises(ValueError):
            _crit(**kw)
    for name, text in (('CTDET_MATCHER', 'Tal'), ('CTDET_TAL_TOPK', '0'), ('CTDET_TAL_TOPK', '17'), ('CTDET_TAL_TOPK', 'nine'),
                       ('CTDET_TAL_ALPHA', '0.3'), ('CTDET_TAL_ALPHA', 'one'), ('CTDET_TAL_BETA', '9'), ('CTDET_TAL_BETA', '1.5')):
        monkeypatch.setenv(name, text)
        with pytest.raises(ValueError):
            _crit()
        monkeypatch.delenv(name)
    for alpha in (0, 0.5, 1, 1.5, 2):
        assert ops.check_tal(13, alpha, 6) == (13, int(2 * alpha), 6)
    assert ops.check_tal(1, 0, 0) == (1, 0, 0) and ops.check_tal(16.0, 2.0, 8.0) == (16, 4, 8)
    for bad in ((0, 1, 6), (17, 1, 6), (13, 0.3, 6), (13, 1, 9), (13, 1, -1), (13, 1, 1.5), (True, 1, 6), (13, '1', 6)):
        with pytest.raises(ValueError):
            ops.check_tal(*bad)


def test_match_under_tal_needs_predictions():
    pri = atss_cases.small_pyramid()[0]
    targets = [atss_cases.SMALL_BOXES]
    crit = _crit(matcher='tal')
    with pytest.raises(ValueError, match='predictions'):
        crit.match(pri, targets)
    with pytest.raises(ValueError, match='predictions'):
        crit.match(pri, ops.PackedTargets(torch.zeros(4, 6), torch.zeros(2, dtype=torch.int32), 4))
    # with predictions the call reaches the library's wrappers, which have no CPU form
    pred = [torch.zeros(1, 41, 4), torch.zeros(1, 41, 20), torch.zeros(1, 41, 2)]
    with pytest.raises(_lib.CtdetError, match='HIP device'):
        crit.match(pri, targets, predictions=pred)
    with pytest.raises(_lib.CtdetError, match='HIP device'):
        crit(pred, pri, targets)


def test_ssd_and_atss_never_reach_the_tal_wrappers(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, 'match_batched', lambda *a, **k: calls.append('ssd') or (1, 2, 3))
    monkeypatch.setattr(ops, 'atss_match_batched', lambda *a, **k: calls.append('atss') or (1, 2, 3))
    for name in ('tal_match_batched', 'tal_match_packed', 'detect_fused'):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail('the TAL path was taken'))
    pri, off = atss_cases.small_pyramid()
    pred = [torch.zeros(1, 41, 4), torch.zeros(1, 41, 20), torch.zeros(1, 41, 2)]
    for matcher in ('ssd', 'atss'):
        crit = _crit(matcher=matcher, level_offsets=off, tal_topk=3)
        assert tuple(crit.match(pri, [atss_cases.SMALL_BOXES])) == (1, 2, 3)
        assert tuple(crit.match(pri, [atss_cases.SMALL_BOXES], predictions=pred)) == (1, 2, 3)      # given, and not read
        assert calls == [matcher] * 2
        del calls[:]
    assert _lib.MATCHERS == ('ssd', 'atss')


# ------------------------------------------------------------------------------------ 3: the C entry and the header
def test_c_abi_refuses_bad_arguments_without_a_device():
    """Every check of ct_tal_match_batched comes before any HIP call: host pointers stand in for the tensors."""
    lib = _lib.lib()
    buf = (C.c_float * 64)()
    host = C.cast(buf, C.c_void_p)

    def call(truths=host, gt_off=host, batch=2, max_gt=4, priors=host, P=41, boxes=host, scores=host, cols=5, topk=13, alpha2=2,
             beta=6, v0=0.1, v1=0.2, loc_t=host, conf_t=host, obj_t=host, ws=host, ws_bytes=1 << 20):
        return lib.ct_tal_match_batched(truths, gt_off, batch, max_gt, priors, P, boxes, scores, cols, topk, alpha2, beta, v0, v1,
                                        loc_t, conf_t, obj_t, None, None, ws, ws_bytes, None)

    need = lib.ct_tal_workspace_bytes(2, 41, 4)
    assert need >= 2 * 41 * 8 and lib.ct_tal_workspace_bytes(1, 41, 4) < need and lib.ct_tal_workspace_bytes(0, 41, 4) == 0
    assert lib.ct_tal_lds_keys() >= 16 + 256                # the survivors of a reduction plus at least one round
    bad = [(dict(truths=None), b'null'), (dict(gt_off=None), b'null'), (dict(priors=None), b'null'), (dict(boxes=None), b'null'),
           (dict(scores=None), b'null'), (dict(loc_t=None), b'null'), (dict(conf_t=None), b'null'), (dict(obj_t=None), b'null'),
           (dict(ws=None), b'null'),
           (dict(batch=0), b'batch=0'), (dict(P=0), b'num_priors=0'), (dict(max_gt=0), b'max_gt=0'),
           (dict(P=(1 << 30) + 1), b'num_priors='), (dict(batch=65536), b'batch=65536'),
           (dict(cols=1), b'score_cols=1'), (dict(cols=0), b'score_cols=0'),
           (dict(topk=0), b'topk=0'), (dict(topk=17), b'topk=17'), (dict(alpha2=-1), b'alpha2=-1'), (dict(alpha2=5), b'alpha2=5'),
           (dict(beta=-1), b'beta=-1'), (dict(beta=9), b'beta=9'),
           (dict(v0=0.0), b'variances'), (dict(v1=-0.2), b'variances'), (dict(v0=math.nan), b'variances'),
           (dict(v1=math.inf), b'variances'), (dict(ws_bytes=need - 1), b'workspace'),
           (dict(ws=C.c_void_p(host.value + 4)), b'aligned')]
    for kw, word in bad:
        assert call(**kw) == 1, kw                          # CT_ERR_INVALID
        msg = lib.ct_last_error_string()
        assert b'ct_tal_match_batched' in msg and word in msg, (kw, msg)


def test_header_documents_the_rule_and_the_binding_matches():
    hdr = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    declared = set(re.findall(r'\b(ct_[a-z0-9_]+)\s*\(', hdr))
    for s in ('ct_tal_match_batched', 'ct_tal_workspace_bytes', 'ct_tal_lds_keys'):
        assert s in declared and s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES['ct_tal_match_batched'][1]) == 22
    assert 'CTDET_ABI_VERSION 1' in hdr and _lib.lib().ct_abi_version() == 1
    text = re.sub(r'\s*\n \*\s*', ' ', hdr)
    for words in ('TASK-ALIGNED ASSIGNMENT', 'x1 < pcx < x2 && y1 < pcy < y2', 'u = 0 if !(u > 0)', 's = 1.f - pred_scores[b,p,0]',
                  'multiply by sqrtf(s) if alpha2 is odd', 'm = 0 if !(m >= FLT_MIN)', 'Ties go to the lower prior index',
                  'over ALL priors, lowest index on a tie', 'then the larger u (for a forced claim, its prior IoU), then the lower box index',
                  'm of the last positive chosen or 0 if forced', 'ct_tal_lds_keys() keys whatever P is'):
        assert words in text, words
    csrc = os.path.join(REPO, 'context-transformer_amd', 'csrc')
    for name in ('ct_atss.hip', 'ct_tal.hip'):              # the claim order and the assign body are shared, not copied
        src = open(os.path.join(csrc, name)).read()
        assert '#include "ct_claims.h"' in src and 'pack_claim(bool' not in src, name
    import importlib.util
    spec = importlib.util.spec_from_file_location('ctdet_build', os.path.join(REPO, 'context-transformer_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SOURCES['ct_tal.hip'] == ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt']
    assert mod.SOURCES['ct_atss.hip'] == ['-ffp-contract=off']
