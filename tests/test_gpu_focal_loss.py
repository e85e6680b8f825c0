"""The mining-free focal classification terms of the fused MultiBoxLoss (ct_multibox_loss_fwd_terms / _bwd_terms,
MultiBoxLoss_combined(fused=True, conf_loss='focal')) on the MI355X.

Yardstick: tests/focal_loss_ref.py (float64, autograd through the definition) -- never the criterion's torch path, which
has its own comparison in tests/test_focal_loss_cpu.py.  Tolerances: the project's loss rule (tests/iou_loss_cases.py),
each loss within 2e-5 * max(1, |ref|), each gradient within 2e-5 * max|ref grad| + 1e-9 in max-norm, all gradients finite.
Every case is matched on the CPU once and the same MatchedTargets go to the device.

Largest device errors observed on the MI355X over every comparison of this file (printed by the tests): see DESIGN.md, the
focal subsection."""
import ctypes as C
import math

import pytest
import torch
import torch.nn as nn

from ctdet import _lib, ops, synth
from layers.modules.multibox_loss_combined import MatchedTargets, MultiBoxLoss_combined, focal_prior_init

import focal_loss_ref as twin
import iou_loss_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = (0.01, 0.02, -0.005)


def _crit(ncls, gamma, alpha, **kw):
    return MultiBoxLoss_combined(ncls, 0.5, True, 0, True, 3, 0.5, False, fused=True, conf_loss='focal', focal_gamma=gamma,
                                 focal_alpha=alpha, **kw)


def _mt(c):
    return MatchedTargets(c.loc_t.to(DEV), c.conf_t.to(DEV), c.obj_t.to(DEV))


def _raw(pred, loc_t, conf_t, obj_t, ncls, focal=None, priors=None, kind=None, g=G):
    """The two ops alone -> sums, n, num_pos, w, dloc, dconf, dobj.  focal: (gamma, alpha), or None for cross-entropy."""
    d = [t.to(DEV).contiguous() for t in (*pred, loc_t, conf_t)] + [obj_t.to(DEV)]
    kw = {} if kind is None else dict(priors=priors.to(DEV).contiguous(), loc_loss=kind)
    if focal is not None:
        kw.update(conf_loss='focal', focal_gamma=focal[0], focal_alpha=focal[1])
    sums, n, num_pos, w = ops.multibox_loss(*d, ncls, 3, **kw)
    grads = ops.multibox_loss_backward(*d, w, torch.tensor(g, device=DEV), ncls, **kw)
    return (sums, n, num_pos, w) + tuple(grads)


def _raw_case(c, focal, **kw):
    return _raw(c.pred, c.loc_t, c.conf_t, c.obj_t, c.ncls, focal, priors=c.priors, **kw)


def _check_raw_against_the_twin(got, pred, loc_t, conf_t, obj_t, gamma, alpha, loc=True):
    want, want_g = twin.sums_and_grads(pred, loc_t, conf_t, obj_t, gamma, alpha, G)
    for i, name in ((0, 'sum_loc'), (1, 'sum_cls'), (2, 'sum_obj')):
        if i or loc:
            cases.check_loss(name, got[0][i], want[i])
    for i, name in ((4, 'loc'), (5, 'conf'), (6, 'obj')):
        if i > 4 or loc:
            cases.check_grad(name, got[i], want_g[i - 4])


# ------------------------------------------------------------------------------------ 1: against the twin
@pytest.mark.parametrize('gamma,alpha', twin.GAMMA_ALPHA)
@pytest.mark.parametrize('name', ['A', 'A_mixup', 'A_ignored', 'B'])
def test_values_and_gradients_against_the_twin(name, gamma, alpha):
    """A: VOC_300, B = 3, C = 21 (group width 8); B: VOC_512, B = 2, C = 61 (group width 16)."""
    c = cases.case(name)
    if name == 'A_ignored':
        assert (c.conf_t[..., 0] < 0).any() and int(c.pos[1].sum()) == 0
    dev = [p.clone().to(DEV).requires_grad_(True) for p in c.pred]
    out = _crit(c.ncls, gamma, alpha)(dev, c.priors.to(DEV), _mt(c))
    sum(out.values()).backward()
    want, want_g = twin.criterion_reference(name, gamma, alpha)
    for k in cases.KEYS:
        cases.check_loss(k, out[k].detach(), want[k])
    for what, got, ref in zip(('loc', 'conf', 'obj'), dev, want_g):
        cases.check_grad(what, got.grad, ref)


def test_combined_with_the_giou_term():
    c = cases.case('A_mixup')
    dev = [p.clone().to(DEV).requires_grad_(True) for p in c.pred]
    out = _crit(c.ncls, 2.0, 0.25, loc_loss='giou')(dev, c.priors.to(DEV), _mt(c))
    sum(out.values()).backward()
    want, want_g = twin.criterion_reference('A_mixup', 2.0, 0.25)
    loc_want, loc_g = c.loc['giou']
    cases.check_loss('giou', out['loss_box_reg'].detach(), loc_want)
    cases.check_loss('loss_cls', out['loss_cls'].detach(), want['loss_cls'])
    cases.check_loss('loss_obj', out['loss_obj'].detach(), want['loss_obj'])
    cases.check_grad('loc', dev[0].grad, loc_g)
    cases.check_grad('conf', dev[1].grad, want_g[1])
    cases.check_grad('obj', dev[2].grad, want_g[2])


# ------------------------------------------------------------------------------------ 2: launch geometry
def _geometry_case(P, B, ncls, seed):
    """Hand-built rows: every fifth row (over the flattened batch) foreground with a mixup weight, the next one ignored
    (label -1, whatever weight), the others background with weight 1 -- as the matcher writes them."""
    g = torch.Generator().manual_seed(seed)
    pred = [torch.randn(B, P, 4, generator=g) * 0.5, torch.randn(B, P, ncls - 1, generator=g) * 3,
            torch.randn(B, P, 2, generator=g) * 2]
    loc_t = torch.randn(B, P, 4, generator=g) * 0.5
    j = torch.arange(B * P).view(B, P)
    fg, ignored = j % 5 == 0, j % 5 == 1
    label = torch.where(fg, torch.randint(1, ncls, (B, P), generator=g).float(), torch.zeros(B, P))
    label = torch.where(ignored, -torch.ones(B, P), label)
    weight = torch.where(label == 0, torch.ones(B, P), torch.rand(B, P, generator=g) * 0.5 + 0.5)
    return pred, loc_t, torch.stack((label, weight), 2), label != 0


@pytest.mark.parametrize('ncls', [2, 6, 21, 61, 82])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('P', [1, 63, 64, 65, 257])
def test_launch_geometry(P, B, ncls):
    """Row lengths 1, 5 and 81 (scalar loads; 4, 8 and the looping 64 lanes per row) and 20, 60 (16-byte loads; 8 and 16
    lanes); row counts below, at and above a whole number of workgroups."""
    pred, loc_t, conf_t, obj_t = _geometry_case(P, B, ncls, 500000 + 1000 * P + 100 * B + ncls)
    label = conf_t[..., 0]
    assert (label > 0).any() and (B * P < 3 or ((label < 0).any() and (label == 0).any()))
    for gamma, alpha in ((2.0, 0.25), (0.5, -1.0)):
        got = _raw(pred, loc_t, conf_t, obj_t, ncls, (gamma, alpha))
        _check_raw_against_the_twin(got, pred, loc_t, conf_t, obj_t, gamma, alpha)
        assert torch.equal(got[3].cpu(), twin.row_weights(conf_t).float())


# ------------------------------------------------------------------------------------ 3: saturated logits
def _saturated_case():
    """64 rows of C = 21: objectness rows of (+-40, -+40) and (+-100, -+100) under both targets, conf rows with one logit at
    +60 (and +120) with the target on it and off it.  In float32 the other probabilities of the +-100 / +120 rows are
    exactly 0 (m = 0: 0^0 at gamma = 0, r = -1), those of the +-40 / +60 rows merely tiny."""
    g = torch.Generator().manual_seed(41)
    P, ncls = 64, 21
    pred = [torch.randn(1, P, 4, generator=g) * 0.5, torch.randn(1, P, ncls - 1, generator=g) * 3,
            torch.randn(1, P, 2, generator=g)]
    loc_t = torch.randn(1, P, 4, generator=g) * 0.5
    label = torch.zeros(1, P)
    label[0, ::2] = torch.randint(1, ncls, (P // 2,), generator=g).float()
    weight = torch.where(label == 0, torch.ones(1, P), torch.rand(1, P, generator=g) * 0.5 + 0.5)
    for k, big in ((0, 40.0), (16, 100.0)):
        for i, sign in enumerate((1.0, 1.0, -1.0, -1.0)):      # rows k .. k+3: both signs on a foreground and a background row
            pred[2][0, k + i] = torch.tensor([sign * big, -sign * big])
    for k, big in ((8, 60.0), (24, 120.0)):
        on, off = k, k + 2                                       # two foreground rows
        pred[1][0, on, int(label[0, on]) - 1] = big
        pred[1][0, off, int(label[0, off]) % (ncls - 1)] = big   # the column after the target's
        pred[1][0, k + 1, 3] = big                               # and a background row, whose conf is not read
    return pred, loc_t, torch.stack((label, weight), 2), label != 0


@pytest.mark.parametrize('gamma,alpha', twin.GAMMA_ALPHA)
def test_saturated_logits_stay_finite_and_inside_the_rule(gamma, alpha):
    pred, loc_t, conf_t, obj_t = _saturated_case()
    got = _raw(pred, loc_t, conf_t, obj_t, 21, (gamma, alpha))
    for t in got:
        assert torch.isfinite(t.float()).all()
    _check_raw_against_the_twin(got, pred, loc_t, conf_t, obj_t, gamma, alpha)
    # rows 17 and 18: the objectness target sits on the +100 logit, p = 1 and m = 0 in float32 -- its gradient is exactly 0 for
    # every gamma (c (p_j - [j = t]) with p_t = 1, p_other = 0) only if c is finite there
    for row in (17, 18):
        assert bool(obj_t[0, row]) == (row == 18) and float(pred[2][0, row, int(row == 18)]) == 100.0
    obj_only = _raw(pred, loc_t, conf_t, obj_t, 21, (gamma, alpha), g=(0.0, 0.0, 1.0))
    assert float(obj_only[6][0, 17].abs().max()) == 0.0 and float(obj_only[6][0, 18].abs().max()) == 0.0


# ------------------------------------------------------------------------------------ 4: the cross-entropy form
def _terms_entries(c, kind, conf_loss=0, gamma=2.0, alpha=0.25, g=G):
    """ct_multibox_loss_fwd_terms / _bwd_terms called directly (ops builds the struct for the focal form alone)."""
    lib = _lib.lib()
    d = [t.to(DEV).contiguous() for t in (*c.pred, c.loc_t, c.conf_t)] + [c.obj_t.to(DEV).view(torch.uint8)]
    pri = c.priors.to(DEV).contiguous()
    B, P = d[0].shape[:2]
    sums, n = torch.empty(3, device=DEV), torch.empty(1, device=DEV, dtype=torch.int64)
    num_pos, w = torch.empty(B, device=DEV, dtype=torch.int64), torch.empty(B, P, device=DEV)
    ws_bytes = lib.ct_multibox_loss_workspace_bytes(B, P, c.ncls)
    ws = torch.empty(ws_bytes, device=DEV, dtype=torch.uint8)
    terms = _lib.LossTerms(pri.data_ptr() if kind != 'smooth_l1' else None, _lib.LOC_LOSSES.index(kind), 0.1, 0.2, conf_loss,
                           gamma, alpha)
    ptr = [C.c_void_p(t.data_ptr()) for t in d]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.ct_multibox_loss_fwd_terms(*ptr, B, P, c.ncls, 3, sums.data_ptr(), num_pos.data_ptr(), n.data_ptr(),
                                              w.data_ptr(), ws.data_ptr(), ws_bytes, stream, C.byref(terms)), 'fwd_terms')
    gd = torch.tensor(g, device=DEV)
    grads = [torch.empty_like(t) for t in d[:3]]
    _lib.check(lib.ct_multibox_loss_bwd_terms(*ptr, w.data_ptr(), gd.data_ptr(), B, P, c.ncls,
                                              *[t.data_ptr() for t in grads], stream, C.byref(terms)), 'bwd_terms')
    torch.cuda.synchronize()
    return (sums, n, num_pos, w) + tuple(grads)


@pytest.mark.parametrize('kind', ['smooth_l1', 'giou'])
@pytest.mark.parametrize('name', ['A_mixup', 'B'])
def test_cross_entropy_through_the_terms_entries_is_bit_equal_to_the_loc_entries(name, kind):
    c = cases.case(name)
    base = _raw_case(c, None, kind=kind)                    # with priors given: ct_multibox_loss_fwd_loc / _bwd_loc
    got = _terms_entries(c, kind, conf_loss=0, gamma=-1.0, alpha=9.0)       # gamma and alpha are not read
    for a, b, what in zip(got, base, ('sums', 'n', 'num_pos', 'w', 'dloc', 'dconf', 'dobj')):
        assert torch.equal(a, b), what
    # and the struct reaches the focal form as ops hands it over
    focal = _terms_entries(c, kind, conf_loss=1)
    for a, b in zip(focal, _raw_case(c, (2.0, 0.25), kind=kind)):
        assert torch.equal(a, b)
    assert not torch.equal(focal[0][1:], base[0][1:])


# ------------------------------------------------------------------------------------ 5: exact zeros, rows not read
@pytest.mark.parametrize('gamma,alpha', [(0.5, 0.25), (2.0, -1.0)])
def test_rows_of_weight_0_and_background_conf_rows_are_never_read(gamma, alpha):
    c = cases.case('A_ignored')
    label = c.conf_t[..., 0]
    ignored, bg = label < 0, label == 0
    conf_t = c.conf_t.clone()
    first = (label > 0).nonzero()[0]
    conf_t[first[0], first[1], 1] = 0.0                     # and one foreground row of weight 0
    dead = ignored.clone()
    dead[first[0], first[1]] = True
    assert int(ignored.sum()) > 0 and int(bg.sum()) > 30000 and int((label > 0).sum()) > 1
    clean = _raw(c.pred, c.loc_t, conf_t, c.obj_t, c.ncls, (gamma, alpha))
    pred = [p.clone() for p in c.pred]
    pred[1][dead] = float('nan')
    pred[2][dead] = float('inf')
    pred[2][:, ::2][dead[:, ::2]] = float('nan')
    pred[1][bg] = float('nan')
    pred[1][:, ::2][bg[:, ::2]] = float('inf')
    got = _raw(pred, c.loc_t, conf_t, c.obj_t, c.ncls, (gamma, alpha))
    for t in got:
        assert torch.isfinite(t.float()).all()
    for a, b in zip(got, clean):
        assert torch.equal(a, b)
    dconf, dobj = got[5].cpu(), got[6].cpu()
    assert float(dconf[dead | bg].abs().max()) == 0.0 and float(dobj[dead].abs().max()) == 0.0
    assert float(dconf[~(dead | bg)].abs().max()) > 0 and float(dobj[~dead].abs().max()) > 0


# ------------------------------------------------------------------------------------ 6: w, num_pos, n, the loc term
@pytest.mark.parametrize('name', ['A_mixup', 'A_ignored'])
def test_w_is_the_row_weight_and_the_counts_and_the_loc_term_are_the_cross_entropy_calls(name):
    c = cases.case(name)
    ce, focal = _raw_case(c, None), _raw_case(c, (2.0, 0.25))
    assert torch.equal(focal[3].cpu(), twin.row_weights(c.conf_t).float())
    assert float(focal[3].cpu()[c.conf_t[..., 0] < 0].abs().sum()) == 0.0
    assert torch.equal(focal[1], ce[1]) and torch.equal(focal[2], ce[2]) and int(focal[1]) == c.n
    assert torch.equal(focal[0][:1], ce[0][:1]) and torch.equal(focal[4], ce[4])
    assert int((focal[3] != 0).sum()) > 4 * int((ce[3] != 0).sum())     # every row, not a 3:1 sample


# ------------------------------------------------------------------------------------ 7: repeatability, capture
def test_two_calls_are_bit_identical_and_images_do_not_see_their_batch_mates():
    c = cases.case('A_mixup')
    for kind in (None, 'ciou'):
        a, b = _raw_case(c, (2.0, 0.25), kind=kind), _raw_case(c, (2.0, 0.25), kind=kind)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        alone = _raw([p[:1] for p in c.pred], c.loc_t[:1], c.conf_t[:1], c.obj_t[:1], c.ncls, (2.0, 0.25), priors=c.priors,
                     kind=kind)
        for i in (2, 3, 4, 5, 6):                           # num_pos, w, dloc, dconf, dobj of image 0
            assert torch.equal(a[i][:1], alone[i]), (kind, i)


def test_forward_and_backward_replay_from_a_captured_graph():
    """tests/test_gpu_loss_fused.py::test_forward_and_backward_replay_from_a_captured_graph with the focal terms: one
    stream, matching outside the graph."""
    priors = cases.priors(300).to(DEV)
    P, ncls, B = priors.shape[0], 21, 4
    crit = _crit(ncls, 2.0, 0.25, loc_loss='giou')
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
    assert float(want['loss_cls'].detach()) > 0 and float(grads[1].abs().max()) > 0


# ------------------------------------------------------------------------------------ 8: end to end
class _TinyDetector(nn.Module):
    """A synthetic single-scale detector: a linear trunk over fixed per-cell features and three 1x1 heads in the channel order
    of the real heads ((anchor, 4), (anchor, C-1), (anchor, 2)), evaluated as matrix products."""

    def __init__(self, ch, anchors, nfg):
        super().__init__()
        self.nfg = nfg
        self.trunk = nn.Linear(ch, ch)
        self.loc = nn.ModuleList([nn.Conv2d(ch, anchors * 4, 1)])
        self.conf = nn.ModuleList([nn.Conv2d(ch, anchors * nfg, 1)])
        self.obj = nn.ModuleList([nn.Conv2d(ch, anchors * 2, 1)])

    def forward(self, x):                                   # x [B, cells, ch] -> loc [B,P,4], conf [B,P,C-1], obj [B,P,2]
        h = torch.tanh(self.trunk(x))
        return tuple((h @ m[0].weight.flatten(1).t() + m[0].bias).view(x.shape[0], -1, k)
                     for m, k in ((self.loc, 4), (self.conf, self.nfg), (self.obj, 2)))


def test_training_a_small_net_reduces_the_focal_loss():
    torch.manual_seed(11)
    side, anchors, ncls, B, ch = 12, 2, 21, 4, 32
    net = focal_prior_init(_TinyDetector(ch, anchors, ncls - 1)).to(DEV)
    assert abs(float(torch.softmax(net.obj[0].bias.detach().view(-1, 2), 1)[0, 1]) - 0.01) < 1e-6
    cell = (torch.arange(side).float() + 0.5) / side
    cy, cx = torch.meshgrid(cell, cell, indexing='ij')
    priors = torch.stack([torch.stack((cx, cy, torch.full_like(cx, s), torch.full_like(cx, s)), 2) for s in (0.2, 0.4)], 2)
    priors = priors.view(-1, 4).to(DEV)                     # cell-major, anchor-minor: the heads' order
    crit = _crit(ncls, 2.0, 0.25)
    x = torch.randn(B, side * side, ch, generator=torch.Generator().manual_seed(12)).to(DEV)
    mt = crit.match(priors, [t.to(DEV) for t in synth.targets(B, ncls, 5)])
    assert int((mt.conf_t[..., 0] > 0).sum()) >= B
    opt = torch.optim.SGD(net.parameters(), lr=0.05, momentum=0.9)
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        loss = sum(crit(net(x), priors, mt).values())
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(losses)
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
