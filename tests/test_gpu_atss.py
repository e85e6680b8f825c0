"""The ATSS matcher (ct_atss_match_batched, ops.atss_match_batched / atss_match_packed, MultiBoxLoss_combined(matcher='atss'))
on the MI355X.

Yardstick: tests/atss_ref.py, the numpy restatement of the rule in include/ctdet.h -- evaluated once per case in
tests/atss_cases.py; tests/test_atss_cpu.py holds it against a float64 brute force and shows that no decision of a case is
closer than 1e-5 to its threshold.  conf_t, obj_t, overlap and gt_stats are compared with exact equality (the IoU expression is
the one tests/test_gpu_kernels.py::test_jaccard_and_match_exact already holds bit for bit); loc_t with rtol 1e-5, atol 2e-5, the
tolerance of that test, because of logf.  The end-to-end losses follow the project's loss rule (tests/iou_loss_cases.py)."""
import numpy as np
import pytest
import torch

from ctdet import ops
from layers.modules.multibox_loss_combined import MatchedTargets, MultiBoxLoss_combined

import atss_cases
import focal_loss_ref
import iou_loss_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VAR = atss_cases.VAR


def _run_list(c, targets=None, priors=None):
    targets = c.targets if targets is None else targets
    return ops.atss_match_batched([t.to(DEV) for t in targets], (c.priors if priors is None else priors).to(DEV).contiguous(),
                                  c.off, c.topk, VAR, want_overlap=True, want_stats=True)


def _run_packed(c):
    truths, gt_off = atss_cases.packed(c, DEV)
    return ops.atss_match_packed(truths, gt_off, len(c.targets), c.max_gt, c.priors.to(DEV).contiguous(), c.off, c.topk, VAR,
                                 want_overlap=True, want_stats=True)


def _check(got, ref, what):
    loc_t, conf_t, obj_t, overlap, stats = (t.cpu().numpy() for t in got)
    print(what, 'positives', [int(n) for n in (conf_t[..., 0] != 0).sum(1)], 'max |loc_t - twin| %.3g'
          % float(np.abs(loc_t - ref.loc_t).max()))
    assert np.array_equal(stats, ref.gt_stats), what         # first: a wrong threshold shows here, before any conflict
    assert np.array_equal(conf_t, ref.conf_t), what
    assert obj_t.dtype == np.bool_ and np.array_equal(obj_t, ref.obj_t), what
    assert np.array_equal(overlap, ref.overlap), what
    assert np.isfinite(loc_t).all() and np.allclose(loc_t, ref.loc_t, rtol=1e-5, atol=2e-5), what
    assert not loc_t[conf_t[..., 0] == 0].any()              # background rows are exact zeros


# ------------------------------------------------------------------------------------ 1: against the twin
@pytest.mark.parametrize('form', ['list', 'packed'])
@pytest.mark.parametrize('name', ['A', 'A_mixup_ignored', 'B'])
def test_against_the_twin(name, form):
    """VOC_300 B = 3 and VOC_512 B = 2: all 6 and 7 levels, a level smaller than topk, mixup weights and label -1."""
    c = atss_cases.case(name)
    _check(_run_list(c) if form == 'list' else _run_packed(c), c.ref, '%s/%s' % (name, form))
    want = {'A': [19, 38, 37], 'A_mixup_ignored': [19, 38, 37], 'B': [60, 73]}[name]
    assert [int(n) for n in (c.ref.conf_t[..., 0] != 0).sum(1)] == want


# ------------------------------------------------------------------------------------ 2: a pyramid to enumerate by hand
@pytest.mark.parametrize('topk', [1, 3, 16])
def test_small_pyramid(topk):
    """4x4 cells x 2 priors, 2x2 x 2, 1x1 x 1 (P = 41), four boxes; tests/test_atss_cpu.py works box 0 out by hand."""
    c = atss_cases.case('small_k%d' % topk)
    got = _run_list(c)
    _check(got, c.ref, c.name)
    assert set(got[4][0, :, 1].tolist()) == {float(min(topk, 32) + min(topk, 8) + 1)}
    if topk == 1:
        conf_t = got[1][0].cpu()
        assert tuple(conf_t[32].tolist()) == (4.0, 1.0) and not (conf_t[:, 0] == 1).any()


# ------------------------------------------------------------------------------------ 3: edge cases
@pytest.mark.parametrize('name', atss_cases.EDGE_NAMES + ('edge_batch',))
def test_edge_cases(name):
    c = atss_cases.case(name)
    got = _run_list(c)
    _check(got, c.ref, name)
    loc_t, conf_t, obj_t, overlap, stats = (t.cpu() for t in got)
    if name == 'empty':
        assert not loc_t.any() and not obj_t.any() and not overlap.any() and not stats.any()
        assert bool((conf_t == torch.tensor([0.0, 1.0])).all())
    if name == 'tiny':
        assert int((conf_t[..., 0] != 0).sum()) == 1 and stats[0, 0, 3] == 1 and stats[0, 0, 2] == 1
    if name == 'degenerate':
        assert not stats[0, 0].any() and bool(torch.isfinite(loc_t).all()) and set(conf_t[0, :, 0].tolist()) == {0.0, 4.0}
    if name == 'identical':
        assert set(conf_t[0, :, 0].tolist()) == {0.0, 2.0}
    if name == 'corner_tie':
        first = (15 * 64 + 15) * 6                          # the lower prior indices of the four tied cells
        assigned = (conf_t[0, :, 0] != 0).nonzero().view(-1)
        level0 = assigned[assigned < c.off[1]]
        assert len(level0) == 0 or (int(level0.min()) >= first and int(level0.max()) < first + 9)
    if name == 'forced_vs_ordinary':
        assert stats[0, 1, 3] == 1 and stats[0, 0, 3] == 0
        forced_row = (conf_t[0, :, 0] == 5).nonzero().view(-1)
        assert len(forced_row) == 1 and float(overlap[0, forced_row[0]]) < 0.01      # the forced claim won with the smaller IoU


def test_more_boxes_than_max_gt_through_the_packed_form():
    c = atss_cases.case('A_max_gt_2')
    assert max(int(t.shape[0]) for t in c.targets) > c.max_gt == 2
    got = _run_packed(c)
    _check(got, c.ref, c.name)
    assert tuple(got[4].shape) == (3, 2, 4)


# ------------------------------------------------------------------------------------ 4: independence, repeatability
def test_images_do_not_see_their_batch_mates_and_two_runs_give_equal_bits():
    c = atss_cases.case('A')
    a, b = _run_list(c), _run_list(c)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for i, t in enumerate(c.targets):
        alone = _run_list(c, targets=[t])
        g = int(t.shape[0])
        for k, (x, y) in enumerate(zip(a, alone)):
            want = x[i:i + 1] if k < 4 else x[i:i + 1, :g]      # gt_stats has max_gt rows of the batch it came from
            assert torch.equal(want, y), (i, k)
        assert not a[4][i, g:].any()


# ------------------------------------------------------------------------------------ 5: end to end
def _criterion_reference(c, ncls, pred):
    """tests/focal_loss_ref.py and tests/iou_loss_ref.py on the TWIN's targets: the three losses and the three gradients."""
    loc_t, conf_t, obj_t = (torch.from_numpy(getattr(c.ref, k)) for k in ('loc_t', 'conf_t', 'obj_t'))
    n = focal_loss_ref.num_pos(conf_t)
    sums, grads = focal_loss_ref.sums_and_grads(pred, loc_t, conf_t, obj_t, 2.0, 0.25, (1.0 / n,) * 3)
    loc_want, loc_g = cases.loc_reference('giou', pred[0], loc_t, conf_t, c.priors, n)
    return {'loss_box_reg': loc_want, 'loss_cls': sums[1] / n, 'loss_obj': sums[2] / n}, [loc_g, grads[1], grads[2]]


@pytest.mark.parametrize('name', ['A', 'B'])
def test_criterion_end_to_end(name):
    c = atss_cases.case(name)
    size, ncls, _, seed = cases._targets(name)
    pred = cases.preds(len(c.targets), c.priors.shape[0], ncls, seed)
    want, want_g = _criterion_reference(c, ncls, pred)
    priors = c.priors.to(DEV)
    matched = None
    for fused in (True, False):
        crit = MultiBoxLoss_combined(ncls, 0.5, True, 0, True, 3, 0.5, False, fused=fused, matcher='atss', conf_loss='focal',
                                     loc_loss='giou', level_offsets=c.off)
        dev = [p.clone().to(DEV).requires_grad_(True) for p in pred]
        if matched is None:
            matched = crit.match(priors, [t.to(DEV) for t in c.targets])
            assert isinstance(matched, MatchedTargets)
            assert np.array_equal(matched.conf_t.cpu().numpy(), c.ref.conf_t)
            out = crit(dev, priors, [t.to(DEV) for t in c.targets])          # the raw targets: forward() matches itself
        else:
            out = crit(dev, priors, matched)                                 # the same device targets
        sum(out.values()).backward()
        for k in cases.KEYS:
            cases.check_loss('%s fused=%s' % (k, fused), out[k].detach(), want[k])
        for what, got, ref in zip(('loc', 'conf', 'obj'), dev, want_g):
            cases.check_grad(what, got.grad, ref)
    # out= form and the packed form of match()
    buf = MatchedTargets(*(torch.zeros_like(t) for t in matched))
    assert crit.match(priors, [t.to(DEV) for t in c.targets], out=buf) is buf
    truths, gt_off = atss_cases.packed(c, DEV)
    again = crit.match(priors, ops.PackedTargets(truths, gt_off, c.max_gt))
    for x, y, z in zip(matched, buf, again):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_ssd_matcher_is_bit_equal_to_the_calls_made_before():
    """matcher='ssd': the criterion's outputs equal those of the same criterion fed ops.match_batched's outputs as
    MatchedTargets, which is what the parent's criterion computes."""
    c = cases.case('A_mixup')
    priors = c.priors.to(DEV)
    targets = [t.to(DEV) for t in c.targets]
    mt = MatchedTargets(*ops.match_batched(targets, priors.contiguous(), 0.5, [0.1, 0.2]))
    for kw in (dict(fused=True), dict(fused=False), dict(fused=True, conf_loss='focal', loc_loss='giou')):
        outs = []
        for matcher_kw, tg in ((dict(matcher='ssd', level_offsets=atss_cases.pyramid(300)[1]), targets), ({}, mt)):
            crit = MultiBoxLoss_combined(c.ncls, 0.5, True, 0, True, 3, 0.5, False, **kw, **matcher_kw)
            assert crit.matcher == 'ssd'
            dev = [p.clone().to(DEV).requires_grad_(True) for p in c.pred]
            out = crit(dev, priors, tg)
            sum(out.values()).backward()
            outs.append([out[k].detach() for k in cases.KEYS] + [p.grad for p in dev])
        for x, y in zip(*outs):
            assert torch.equal(x, y), kw
        got = crit.match(priors, targets)
        for x, y in zip(got, mt):
            assert torch.equal(x, y)
