"""The TAL matcher (ct_tal_match_batched, ops.tal_match_batched / tal_match_packed, MultiBoxLoss_combined(matcher='tal')) on the
MI355X.

Yardstick: tests/tal_ref.py, the numpy restatement of the rule in include/ctdet.h, fed the DEVICE's ct_detect_fused outputs
downloaded to the host (tests/tal_cases.py, detect='device'), so the softmaxes and exp are not part of the comparison;
tests/test_tal_cpu.py holds the twin against a float64 brute force.  conf_t, obj_t, overlap and gt_stats are compared with exact
equality; loc_t with rtol 1e-5, atol 2e-5, the existing matcher tolerance, because of logf.  Background rows are exact zeros."""
import numpy as np
import pytest
import torch

from ctdet import _lib, ops
from layers.modules.multibox_loss_combined import MatchedTargets, MultiBoxLoss_combined

import atss_cases
import iou_loss_cases as cases
import tal_cases
import tal_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VAR = tal_cases.VAR
tal_match_batched, tal_match_packed = ops.tal_match_batched, ops.tal_match_packed


def _run_list(c, images=None):
    sel = slice(None) if images is None else images
    return tal_match_batched([t.to(DEV) for t in c.targets[sel]], c.priors.to(DEV).contiguous(), c.boxes[sel].to(DEV).contiguous(),
                             c.scores[sel].to(DEV).contiguous(), c.topk, c.alpha, c.beta, VAR, want_overlap=True, want_stats=True)


def _run_packed(c):
    truths, gt_off = atss_cases.packed(c, DEV)
    return tal_match_packed(truths, gt_off, len(c.targets), c.max_gt, c.priors.to(DEV).contiguous(), c.boxes.to(DEV).contiguous(),
                            c.scores.to(DEV).contiguous(), c.topk, c.alpha, c.beta, VAR, want_overlap=True, want_stats=True)


def _check(got, ref, what):
    loc_t, conf_t, obj_t, overlap, stats = (t.cpu().numpy() for t in got)
    print(what, 'positives', [int(n) for n in (ref.owner >= 0).sum(1)], 'max |loc_t - twin| %.3g' % float(np.abs(loc_t - ref.loc_t).max()))
    assert np.array_equal(stats, ref.gt_stats), what          # first: a wrong selection shows here, before any conflict
    assert np.array_equal(conf_t, ref.conf_t), what
    assert obj_t.dtype == np.bool_ and np.array_equal(obj_t, ref.obj_t), what
    assert np.array_equal(overlap, ref.overlap), what
    assert np.isfinite(loc_t).all() and np.allclose(loc_t, ref.loc_t, rtol=1e-5, atol=2e-5), what
    assert not loc_t[ref.owner < 0].any() and (conf_t[ref.owner < 0] == (0, 1)).all()      # background rows are exact


# ------------------------------------------------------------------------------------ 1: against the twin
@pytest.mark.parametrize('form', ['list', 'packed'])
@pytest.mark.parametrize('name', ['A', 'A_mixup_ignored', 'B'])
def test_against_the_twin(name, form):
    """VOC_300 B = 3 and VOC_512 B = 2 with random predictions: boxes with 394 to 7304 eligible candidates (B: more than the LDS
    key buffer), mixup weights and label -1."""
    c = tal_cases.case(name, 13, 1.0, 6, 'device')
    _check(_run_list(c) if form == 'list' else _run_packed(c), c.ref, '%s/%s' % (name, form))
    want = {'A': [26, 52, 62], 'A_mixup_ignored': [25, 52, 62], 'B': [77, 101]}[name]
    assert [int(n) for n in (c.ref.owner >= 0).sum(1)] == want
    assert c.ref.gt_stats[..., 0].max() > _lib.lib().ct_tal_lds_keys() or name != 'B'


@pytest.mark.parametrize('topk,alpha,beta', [(10, 0.5, 6), (1, 0.0, 1), (16, 2.0, 8), (13, 1.5, 0)])
def test_other_exponents(topk, alpha, beta):
    """The sqrtf factor, alpha = 0, beta = 0 (u plays no part in m and a positive may carry u = 0) on case A."""
    c = tal_cases.case('A', topk, alpha, beta, 'device')
    _check(_run_list(c), c.ref, 'A/%s' % ((topk, alpha, beta),))


# ------------------------------------------------------------------------------------ 2: a pyramid to enumerate by hand
@pytest.mark.parametrize('topk', [1, 3, 16])
def test_small_pyramid(topk):
    """4x4 cells x 2 priors, 2x2 x 2, 1x1 x 1 (P = 41: less than one wave of work per round), four boxes."""
    c = tal_cases.case('small', topk, 1.0, 6, 'device')
    got = _run_list(c)
    _check(got, c.ref, 'small/k%d' % topk)
    assert got[4][0, :, 1].tolist() == [float(min(topk, e)) for e in got[4][0, :, 0].tolist()]


# ------------------------------------------------------------------------------------ 3: edge cases
@pytest.mark.parametrize('name', tal_cases.EDGE_NAMES)
def test_edge_cases(name):
    c = tal_cases.edge(name, 'device')
    got = _run_list(c)
    _check(got, c.ref, name)
    loc_t, conf_t, obj_t, overlap, stats = (t.cpu() for t in got)
    if name == 'empty':
        assert not loc_t.any() and not obj_t.any() and not overlap.any() and not stats.any()
        assert bool((conf_t == torch.tensor([0.0, 1.0])).all())
    if name == 'degenerate':
        assert not stats[0, 0].any() and bool(torch.isfinite(loc_t).all()) and set(conf_t[0, :, 0].tolist()) == {0.0, 4.0}
    if name in ('tiny', 'moved_off'):                       # forced: one prior, by the prior's own IoU
        assert stats[0, 0].tolist() == [0, 1, 0, 1] and int((conf_t[..., 0] != 0).sum()) == 1
        assert 0 < float(overlap.max()) < 1
    if name == 'identical':                                 # the lower index wins every prior
        assert stats[0, 0].tolist() == stats[0, 1].tolist() and int((conf_t[0, :, 0] == 2).sum()) == 13
        assert set(conf_t[0, :, 1].tolist()) == {1.0}
    if name == 'nan_inf':
        assert bool(torch.isfinite(loc_t).all()) and bool(torch.isfinite(overlap).all()) and stats[0, :, 1].tolist() == [13, 13]
    if name == 'ignored':
        rows = conf_t[0][conf_t[0, :, 0] != 0]
        assert len(rows) == 13 and bool((rows == torch.tensor([-1.0, 0.37])).all()) and int(obj_t.sum()) == 13


def test_more_boxes_than_max_gt_through_the_packed_form():
    c = tal_cases.case('A', 13, 1.0, 6, 'device', 2)
    assert max(int(t.shape[0]) for t in c.targets) > c.max_gt == 2
    got = _run_packed(c)
    _check(got, c.ref, 'A/max_gt=2')
    assert tuple(got[4].shape) == (3, 2, 4)


# ------------------------------------------------------------------------------------ 4: the selection paths
@pytest.mark.parametrize('order', ['rising', 'falling', 'constant'])
@pytest.mark.parametrize('topk', [13, 16])
def test_selection_paths_on_a_whole_image_box(order, topk):
    """One box over the whole image at VOC_512: all 32 756 priors are eligible, eight times what the LDS key buffer holds, and
    every predicted box is the box itself (u = 1, m = s).  Scores rising with the prior index put every key above the running
    threshold (the buffer refills and is reduced again and again), falling ones none after the first reduction, constant ones
    make all metrics equal so that the index alone decides."""
    pri = atss_cases.pyramid(512)[0]
    P = pri.shape[0]
    assert P == 32756 > 2 * _lib.lib().ct_tal_lds_keys()
    ramp = (torch.arange(P, dtype=torch.float32) + 1) / P
    scores = torch.zeros(1, P, 4)
    scores[0, :, 2] = {'rising': ramp, 'falling': ramp.flip(0), 'constant': torch.full((P,), 0.75)}[order]
    boxes = torch.tensor([0.0, 0.0, 1.0, 1.0]).expand(1, P, 4).contiguous()
    c = tal_cases.build([torch.tensor([[0.0, 0.0, 1.0, 1.0, 2, 1.0]])], pri, boxes, scores, topk, 1.0, 6)
    got = _run_list(c)
    _check(got, c.ref, '%s/k%d' % (order, topk))
    chosen = (got[1][0, :, 0] != 0).nonzero().view(-1).tolist()
    assert chosen == (list(range(P - topk, P)) if order == 'rising' else list(range(topk)))
    last = {'rising': float(ramp[P - topk]), 'falling': float(ramp[P - topk]), 'constant': 0.75}[order]
    assert got[4][0, 0].tolist() == [P, topk, last, 0]


# ------------------------------------------------------------------------------------ 5: independence, repeatability
def test_images_do_not_see_their_batch_mates_and_two_runs_give_equal_bits():
    c = tal_cases.case('A', 13, 1.0, 6, 'device')
    a, b = _run_list(c), _run_list(c)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for i, t in enumerate(c.targets):
        alone = _run_list(c, images=slice(i, i + 1))
        g = int(t.shape[0])
        for k, (x, y) in enumerate(zip(a, alone)):
            want = x[i:i + 1] if k < 4 else x[i:i + 1, :g]      # gt_stats has max_gt rows of the batch it came from
            assert torch.equal(want, y), (i, k)
        assert not a[4][i, g:].any()


# ------------------------------------------------------------------------------------ 6: end to end
def _losses_and_grads(crit, pred, priors, targets):
    dev = [p.clone().to(DEV).requires_grad_(True) for p in pred]
    out = crit(dev, priors, targets)
    sum(out.values()).backward()
    return [out[k].detach() for k in cases.KEYS] + [p.grad for p in dev]


@pytest.mark.parametrize('fused', [True, False])
def test_criterion_end_to_end(fused):
    c = tal_cases.case('A', 13, 1.0, 6, 'device')
    ncls = cases._targets('A')[1]
    priors = c.priors.to(DEV)
    targets = [t.to(DEV) for t in c.targets]
    crit = MultiBoxLoss_combined(ncls, 0.5, True, 0, True, 3, 0.5, False, fused=fused, matcher='tal', conf_loss='focal',
                                 loc_loss='giou')
    assert (crit.tal_topk, crit.tal_alpha, crit.tal_beta) == (13, 1.0, 6)
    # the criterion fed raw targets against the same criterion fed the wrapper's result on the same predictions
    boxes, scores = ops.detect_fused(*(p.to(DEV) for p in c.pred), priors.contiguous(), VAR, apply_softmax=True)
    direct = MatchedTargets(*tal_match_batched(targets, priors.contiguous(), boxes, scores, 13, 1.0, 6, VAR))
    raw = _losses_and_grads(crit, c.pred, priors, targets)
    fed = _losses_and_grads(crit, c.pred, priors, direct)
    for x, y in zip(raw, fed):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    assert float(raw[0]) > 0 and float(raw[1]) > 0 and float(raw[2]) > 0
    # those targets are the twin's
    assert np.array_equal(direct.conf_t.cpu().numpy(), c.ref.conf_t) and np.array_equal(direct.obj_t.cpu().numpy(), c.ref.obj_t)
    assert np.allclose(direct.loc_t.cpu().numpy(), c.ref.loc_t, rtol=1e-5, atol=2e-5)
    # nothing flows through the assignment: match() on clones of the predictions, with and without requires_grad
    live = [p.clone().to(DEV).requires_grad_(True) for p in c.pred]
    matched = crit.match(priors, targets, predictions=live)
    assert isinstance(matched, MatchedTargets) and not any(t.requires_grad for t in matched) and all(p.grad is None for p in live)
    for x, y in zip(matched, direct):
        assert torch.equal(x, y)
    cloned = _losses_and_grads(crit, c.pred, priors, crit.match(priors, targets, predictions=[p.clone().to(DEV) for p in c.pred]))
    for x, y in zip(raw, cloned):
        assert torch.equal(x, y)
    # out= form and the packed form of match()
    buf = MatchedTargets(*(torch.zeros_like(t) for t in matched))
    assert crit.match(priors, targets, out=buf, predictions=live) is buf
    truths, gt_off = atss_cases.packed(c, DEV)
    again = crit.match(priors, ops.PackedTargets(truths, gt_off, c.max_gt), predictions=live)
    for x, y, z in zip(matched, buf, again):
        assert torch.equal(x, y) and torch.equal(x, z)
    with pytest.raises(ValueError, match='predictions'):
        crit.match(priors, targets)


def test_ssd_and_atss_are_bit_equal_to_the_direct_calls():
    """matcher='ssd' and 'atss' with the tal arguments set: match() returns what ops.match_batched / ops.atss_match_batched
    return, predictions given or not."""
    c = tal_cases.case('A', 13, 1.0, 6, 'device')
    priors, off = c.priors.to(DEV).contiguous(), atss_cases.pyramid(300)[1]
    targets = [t.to(DEV) for t in c.targets]
    pred = [p.to(DEV) for p in c.pred]
    want = {'ssd': ops.match_batched(targets, priors, 0.5, [0.1, 0.2]), 'atss': ops.atss_match_batched(targets, priors, off, 9, [0.1, 0.2])}
    for matcher in ('ssd', 'atss'):
        crit = MultiBoxLoss_combined(21, 0.5, True, 0, True, 3, 0.5, False, matcher=matcher, level_offsets=off, tal_topk=3,
                                     tal_alpha=0.5, tal_beta=2)
        for got in (crit.match(priors, targets), crit.match(priors, targets, predictions=pred)):
            for x, y in zip(got, want[matcher]):
                assert torch.equal(x, y), matcher
    tal = MultiBoxLoss_combined(21, 0.5, True, 0, True, 3, 0.5, False, matcher='tal').match(priors, targets, predictions=pred)
    assert not torch.equal(tal.conf_t, want['ssd'][1]) and not torch.equal(tal.conf_t, want['atss'][1])
