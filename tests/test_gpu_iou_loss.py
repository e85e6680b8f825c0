"""The IoU-family localisation terms of the fused MultiBoxLoss (ct_multibox_loss_fwd_loc / _bwd_loc,
MultiBoxLoss_combined(fused=True, loc_loss=...)) on the MI355X.

Yardsticks: tests/iou_loss_ref.py (float64, autograd) for the loc term, oracle.loss_ref on torch-CPU for the class and
objectness terms -- never the criterion's torch path or the kernels for each other.  Tolerances: the project's loss rule,
each loss within 2e-5 * max(1, |ref|), each gradient within 2e-5 * max|ref grad| + 1e-9 in max-norm, all gradients finite.
Every case is matched on the CPU once (tests/iou_loss_cases.py) and the same MatchedTargets go to the device.

Largest device errors observed on the MI355X over every comparison of this file (printed by the tests): see DESIGN.md, the
IoU-family subsection."""
import math
import types

import pytest
import torch

from ctdet import ops, synth
from layers.modules.multibox_loss_combined import MatchedTargets, MultiBoxLoss_combined

import iou_loss_cases as cases
import iou_loss_ref as twin

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = twin.KINDS


def _crit(ncls, loc_loss, **kw):
    return MultiBoxLoss_combined(ncls, 0.5, True, 0, True, 3, 0.5, False, fused=True, loc_loss=loc_loss, **kw)


def _mt(c):
    return MatchedTargets(c.loc_t.to(DEV), c.conf_t.to(DEV), c.obj_t.to(DEV))


def _criterion_vs_references(c, kind):
    dev = [p.clone().to(DEV).requires_grad_(True) for p in c.pred]
    out = _crit(c.ncls, kind)(dev, c.priors.to(DEV), _mt(c))
    sum(out.values()).backward()
    want, want_g = c.loc[kind]
    cases.check_loss(kind, out['loss_box_reg'].detach(), want)
    cases.check_loss('loss_cls', out['loss_cls'].detach(), c.loss_cls)
    cases.check_loss('loss_obj', out['loss_obj'].detach(), c.loss_obj)
    cases.check_grad('loc', dev[0].grad, want_g)
    cases.check_grad('conf', dev[1].grad, c.dconf)
    cases.check_grad('obj', dev[2].grad, c.dobj)
    return dev


def _raw(pred, loc_t, conf_t, obj_t, ncls, priors, kind, g=(0.01, 0.02, -0.005)):
    """The two ops alone -> sums, n, num_pos, w, dloc, dconf, dobj.  kind None: the entries without a loc_loss."""
    d = [t.to(DEV).contiguous() for t in (*pred, loc_t, conf_t)] + [obj_t.to(DEV)]
    kw = {} if kind is None else dict(priors=priors.to(DEV).contiguous(), loc_loss=kind)
    sums, n, num_pos, w = ops.multibox_loss(*d, ncls, 3, **kw)
    grads = ops.multibox_loss_backward(*d, w, torch.tensor(g, device=DEV), ncls, **kw)
    return (sums, n, num_pos, w) + tuple(grads)


def _raw_case(c, kind, **kw):
    return _raw(c.pred, c.loc_t, c.conf_t, c.obj_t, c.ncls, c.priors, kind, **kw)


# ------------------------------------------------------------------------------------ 1: against the twin
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['A', 'A_mixup', 'A_ignored', 'B'])
def test_values_and_gradients_against_the_twin(name, kind):
    """A: VOC_300, B = 3, C = 21 (group width 8); B: VOC_512, B = 2, C = 61 (group width 16)."""
    c = cases.case(name)
    if name == 'A_ignored':
        assert (c.conf_t[..., 0] < 0).any() and int(c.pos[1].sum()) == 0
    if name == 'A_mixup':
        assert set(c.conf_t[..., 1][c.pos].tolist()) == {0.37000000476837158, 0.62999999523162842}
    _criterion_vs_references(c, kind)


# ------------------------------------------------------------------------------------ 2: the non-overlap branch
@pytest.mark.parametrize('name', ['A', 'B'])
def test_the_non_overlap_branch(name):
    c, far = cases.case(name), cases.case(name, 10.0)
    # preconditions, on the twin alone -- a miss is a failure, not a skip
    npos, disjoint, kink = cases.overlap_stats(far)
    npos1, disjoint1, kink1 = cases.overlap_stats(c)
    print('positives %d, disjoint %.3f scaled / %.3f unscaled, kink distance %.3g / %.3g' % (npos, disjoint, disjoint1,
                                                                                              kink, kink1))
    assert npos >= 100 and npos1 == npos
    assert 0.3 <= disjoint <= 0.9
    assert 1 - disjoint1 >= 0.95
    assert kink > 1e-6 and kink1 > 1e-6
    pri = far.priors.expand(far.pred[0].shape[0], -1, -1)
    apart = torch.zeros_like(far.pos)
    apart[far.pos] = twin.terms(far.pred[0][far.pos].double(), far.loc_t[far.pos].double(),
                                pri[far.pos].double())['inter'] == 0
    for kind in KINDS:
        dev = _criterion_vs_references(far, kind)
        rows = dev[0].grad[apart.to(DEV)]
        if kind == 'iou':
            assert float(rows.abs().max()) == 0.0
        elif kind in ('giou', 'diou'):
            assert bool((rows.abs().sum(1) > 0).all()), kind


# ------------------------------------------------------------------------------------ 3: launch geometry
def _grid_case(P, B, ncls, seed):
    """Hand-built: priors on a regular grid, image 0 with every prior positive, then (B = 3) one without ground truth and
    one with every third prior positive.  Offsets of +-0.5: overlapping boxes, no ties (continuous draws)."""
    g = torch.Generator().manual_seed(seed)
    side = int(math.ceil(math.sqrt(P)))
    idx = torch.arange(P)
    pri = torch.stack([(idx % side + 0.5) / side, (idx // side + 0.5) / side, 0.08 + 0.01 * (idx % 7).float(),
                       0.06 + 0.02 * (idx % 5).float()], 1)
    pred = [torch.randn(B, P, 4, generator=g) * 0.5, torch.randn(B, P, ncls - 1, generator=g) * 3,
            torch.randn(B, P, 2, generator=g)]
    loc_t = torch.randn(B, P, 4, generator=g) * 0.5
    conf_t = torch.zeros(B, P, 2)
    conf_t[:, :, 1] = torch.rand(B, P, generator=g) * 0.5 + 0.5
    is_pos = torch.zeros(B, P, dtype=torch.bool)
    is_pos[0] = True
    if B == 3:
        is_pos[2, ::3] = True
    conf_t[:, :, 0] = torch.where(is_pos, torch.randint(1, ncls, (B, P), generator=g).float(), torch.zeros(B, P))
    return pri, pred, loc_t, conf_t, is_pos.clone()


@pytest.mark.parametrize('ncls', [2, 6, 21])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('P', [1, 63, 64, 65, 257])
def test_launch_geometry(P, B, ncls):
    """The loc term against the twin; the two other terms and their gradients are bit-equal to the smooth-L1 launch of the
    same inputs (item 4), which tests/test_gpu_loss_fused.py holds to its own references."""
    # seeds at which every case keeps off the kinks
    pri, pred, loc_t, conf_t, obj_t = _grid_case(P, B, ncls, 300000 + 1000 * P + 10 * B + ncls)
    pos = conf_t[..., 0] > 0
    assert bool(pos[0].all()) and (B == 1 or (int(pos[1].sum()) == 0 and 0 < int(pos[2].sum()) < P or P == 1))
    assert float(twin.kink_distance(pred[0][pos], loc_t[pos], pri.expand(B, -1, -1)[pos]).min()) > 1e-6
    g = (0.01, 0.02, -0.005)
    base = _raw(pred, loc_t, conf_t, obj_t, ncls, pri, None, g)
    for kind in KINDS:
        got = _raw(pred, loc_t, conf_t, obj_t, ncls, pri, kind, g)
        x = pred[0].double().requires_grad_(True)
        want = twin.loc_sum(kind, x, loc_t, conf_t, pri)
        want_g, = torch.autograd.grad(want * g[0], x)
        cases.check_loss(kind, got[0][0], float(want.detach()))
        cases.check_grad('loc', got[4], want_g)
        for i in (1, 2, 3, 5, 6):
            assert torch.equal(got[i], base[i]), (kind, i)
        assert torch.equal(got[0][1:], base[0][1:]), kind


# ------------------------------------------------------------------------------------ 4: nothing else moves
@pytest.mark.parametrize('name', ['A_mixup', 'B'])
def test_everything_but_the_loc_term_is_bit_equal_to_the_smooth_l1_call(name):
    c = cases.case(name)
    base = _raw_case(c, None)
    for kind in KINDS:
        got = _raw_case(c, kind)
        for i, what in ((1, 'n'), (2, 'num_pos'), (3, 'w'), (5, 'dconf'), (6, 'dobj')):
            assert torch.equal(got[i], base[i]), (kind, what)
        assert torch.equal(got[0][1:], base[0][1:]), kind
        assert not torch.equal(got[0][:1], base[0][:1]) and not torch.equal(got[4], base[4]), kind
    same = _raw_case(c, 'smooth_l1')                     # the _loc entries with loc_loss = 0: the old entries' bytes
    for a, b in zip(same, base):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------ 5: exact zeros
@pytest.mark.parametrize('kind', KINDS)
def test_rows_that_are_not_positive_are_never_read(kind):
    c = cases.case('A')
    clean = _raw_case(c, kind)
    loc = c.pred[0].clone()
    loc[~c.pos] = float('nan')
    loc[:, ::2][~c.pos[:, ::2]] = 1e30
    loc_t = c.loc_t.clone()
    loc_t[~c.pos] = float('nan')
    never = ~c.pos.any(0)
    assert int(never.sum()) > 10000 and int((~c.pos).sum()) > 30000
    pri = c.priors.clone()
    pri[never] = float('nan')
    got = _raw([loc, c.pred[1], c.pred[2]], loc_t, c.conf_t, c.obj_t, c.ncls, pri, kind)
    for t in got:
        assert torch.isfinite(t.float()).all()
    assert float(got[4][(~c.pos).to(DEV)].abs().max()) == 0.0
    for a, b in zip(got, clean):
        assert torch.equal(a, b)
    # a positive row of weight 0: exact zeros, not read either
    conf_t = c.conf_t.clone()
    first = c.pos.nonzero()[0]
    conf_t[first[0], first[1], 1] = 0.0
    loc[first[0], first[1]] = float('nan')
    got = _raw([loc, c.pred[1], c.pred[2]], loc_t, conf_t, c.obj_t, c.ncls, pri, kind)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[4]).all()
    assert float(got[4][first[0], first[1]].abs().max()) == 0.0


# ------------------------------------------------------------------------------------ 6: the minimum
@pytest.mark.parametrize('kind', KINDS)
def test_prediction_equal_to_the_target_on_every_positive(kind):
    """loc == loc_t is a kink (every min / max pair ties): values only.  L >= 0 for every row, so the weighted sum bounds
    each row's L."""
    c = cases.case('A_mixup')
    loc = c.pred[0].clone()
    loc[c.pos] = c.loc_t[c.pos]
    got = _raw([loc, c.pred[1], c.pred[2]], c.loc_t, c.conf_t, c.obj_t, c.ncls, c.priors, kind)
    total = float(got[0][0])
    print(kind, 'sum of L * weight over %d positives: %.3g' % (int(c.pos.sum()), total))
    assert -1e-6 * 0.37 <= total <= 1e-6 * 0.37
    for t in got[4:]:
        assert torch.isfinite(t).all()


# ------------------------------------------------------------------------------------ 7: repeatability, capture
def test_two_calls_are_bit_identical_and_images_do_not_see_their_batch_mates():
    c = cases.case('A_mixup')
    for kind in KINDS:
        a, b = _raw_case(c, kind), _raw_case(c, kind)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        alone = _raw([p[:1] for p in c.pred], c.loc_t[:1], c.conf_t[:1], c.obj_t[:1], c.ncls, c.priors, kind)
        for i in (2, 3, 4, 5, 6):                       # num_pos, w, dloc, dconf, dobj of image 0
            assert torch.equal(a[i][:1], alone[i]), (kind, i)


def test_forward_and_backward_replay_from_a_captured_graph():
    """tests/test_gpu_loss_fused.py::test_forward_and_backward_replay_from_a_captured_graph with loc_loss='ciou' and a
    loc_weight: one stream, matching outside the graph."""
    priors = cases.priors(300).to(DEV)
    P, ncls, B = priors.shape[0], 21, 4
    crit = _crit(ncls, 'ciou', loc_weight=2.0)
    tg1 = [t.to(DEV) for t in synth.targets(B, ncls, 5)]
    tg2 = [t.to(DEV) for t in synth.targets(B, ncls, 6)]
    p1, p2 = cases.preds(B, P, ncls, 1), cases.preds(B, P, ncls, 2)
    static = [p.clone().to(DEV).requires_grad_(True) for p in p1]
    mt = crit.match(priors, tg1)
    mt = MatchedTargets(mt.loc_t.clone(), mt.conf_t.clone(), mt.obj_t.clone())

    def region():
        out = crit(static, priors, mt)
        return out, torch.autograd.grad(sum(out.values()), static)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            region()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = region()
    torch.cuda.synchronize()
    with torch.no_grad():
        for a, b in zip(static, p2):
            a.copy_(b)
    crit.match(priors, tg2, out=mt)
    graph.replay()
    torch.cuda.synchronize()
    eager_in = [p.clone().to(DEV).requires_grad_(True) for p in p2]
    want = crit(eager_in, priors, crit.match(priors, tg2))
    want_g = torch.autograd.grad(sum(want.values()), eager_in)
    for k in cases.KEYS:
        assert torch.equal(out[k], want[k]), k
    for a, b in zip(grads, want_g):
        assert torch.equal(a, b)
    assert float(want["loss_box_reg"].detach()) > 0 and float(grads[0].abs().max()) > 0


# ------------------------------------------------------------------------------------ 8: end to end
def test_training_reduces_the_loss_with_the_fused_giou_criterion():
    """tests/test_gpu_loss_fused.py::test_training_reduces_the_loss_with_the_fused_criterion with loc_loss='giou'."""
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), 300, 20)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()), strict=True)
    net = net.cuda().train()
    net.device = 'cuda'
    priors = cases.priors(300).cuda()
    crit = _crit(21, 'giou')
    opt = torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4)
    x = synth.images(4, 300, 'randn', 77).cuda()
    tg = [t.cuda() for t in synth.targets(4, 21, 5)]
    losses = []
    for _ in range(15):
        opt.zero_grad(set_to_none=True)
        loss = sum(crit(net(x), priors, tg).values())
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(losses)
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
