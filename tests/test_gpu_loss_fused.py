"""The fused HIP MultiBoxLoss (ct_multibox_loss_fwd / _bwd, MultiBoxLoss_combined(fused=True)) on the MI355X.

Yardsticks: oracle.loss_ref.multibox_loss_combined on torch-CPU, and for hand-built MatchedTargets the existing torch
path of MultiBoxLoss_combined on CPU tensors (fused=False) -- never the fused code itself.  Tolerances are those of
tests/test_gpu_train.py::test_loss_with_ignored_boxes_labelled_minus_one: each loss within 2e-5 * max(1, |ref|), each
gradient within 2e-5 * max|ref grad| + 1e-9 in max-norm, all gradients finite."""
import ctypes as C
import math
import types

import pytest
import torch
import torch.nn.functional as F

from ctdet import _lib, ops, synth
from oracle import box_ref, loss_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEYS = ('loss_box_reg', 'loss_cls', 'loss_obj')


def _crit(C_=21, fused=True, ratio=3):
    from layers.modules.multibox_loss_combined import MultiBoxLoss_combined
    return MultiBoxLoss_combined(C_, 0.5, True, 0, True, ratio, 0.5, False, fused=fused)


def _priors(size):
    from layers.functions import PriorBox
    import data as cfgs
    return PriorBox(cfgs.VOC_300 if size == 300 else cfgs.VOC_512).forward()


def _preds(B, P, ncls, seed):
    """Exactly as the existing -1 test draws them: ONE generator, loc, conf * 3, obj in that order."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, P, 4, generator=g), torch.randn(B, P, ncls - 1, generator=g) * 3,
            torch.randn(B, P, 2, generator=g)]


def _check_losses(got, want):
    for k in KEYS:
        a, b = float(got[k].detach()), float(want[k].detach())
        print('loss %-12s fused %.8g ref %.8g' % (k, a, b))
        assert abs(a - b) < 2e-5 * max(1.0, abs(b)), (k, a, b)


def _check_grads(got, want):
    for a, b, n in zip(got, want, ('loc', 'conf', 'obj')):
        a = a.detach().cpu()
        assert torch.isfinite(a).all(), n
        err, ref = float((a - b).abs().max()), float(b.abs().max())
        print('grad %-5s max err %.3g of max %.3g' % (n, err, ref))
        assert err <= 2e-5 * ref + 1e-9, (n, err, ref)


# ------------------------------------------------------------------------------------ 1 + 2: the oracle cases
def _case(name):
    if name == 'b3':
        return 300, 21, synth.targets(3, 21, 99), 5
    if name == 'b8':
        return 300, 21, synth.targets(8, 21, 7), 11
    if name == 'b8_mixup':
        tg = synth.targets(8, 21, 7)
        for t in tg:
            t[::2, 5] = 0.37
            t[1::2, 5] = 0.63
        return 300, 21, tg, 11
    if name == 'ignored':
        tg = synth.targets(3, 21, 99)
        for t in tg:                            # every second box (and one whole image) ignored
            t[::2, 4] = -1
        tg[1][:, 4] = -1
        tg[0][0, 4] = 3
        return 300, 21, tg, 5
    if name == 'voc512':
        return 512, 21, synth.targets(4, 21, 21), 3
    if name == 'voc512_c61':
        return 512, 61, synth.targets(4, 61, 21), 3
    raise KeyError(name)


CASES = ('b3', 'b8', 'b8_mixup', 'ignored', 'voc512', 'voc512_c61')


def _oracle_selection(pred, priors, targets, negpos_ratio=3):
    """oracle/loss_ref.py:16-36 up to the mask: the CPU oracle's own selection, with the figures the precondition of
    the exact comparison needs.  -> w = weight * (pos | neg) [B,P], num_pos [B], num_neg [B], gaps, fractional parts."""
    num, P = pred[0].shape[0], priors.shape[0]
    conf_t = torch.zeros(num, P, 2)
    obj_t = torch.zeros(num, P, dtype=torch.bool)
    for i in range(num):
        t = targets[i]
        _, c, o, _ = box_ref.match(0.5, t[:, :-2], priors, [0.1, 0.2], t[:, -2:])
        conf_t[i], obj_t[i] = c, o
    pos = conf_t[:, :, 0] > 0
    num_pos = (conf_t[:, :, 1] * pos.float()).sum(1, keepdim=True).long()
    lo = F.cross_entropy(pred[2].reshape(-1, 2), obj_t.long().view(-1), reduction='none')
    lo[obj_t.view(-1)] = 0
    lo = lo.view(num, -1)
    _, loss_idx = lo.sort(1, descending=True)
    _, idx_rank = loss_idx.sort(1)
    num_neg = torch.clamp(negpos_ratio * num_pos, max=P - 1)
    neg = idx_rank < num_neg.expand_as(idx_rank)
    w = conf_t[:, :, 1] * (pos | neg).float()
    srt = lo.sort(1, descending=True)[0].double()
    gaps, fracs = [], []
    for i in range(num):
        k = int(num_neg[i])
        gaps.append(None if k == 0 else float((srt[i, k - 1] - srt[i, k]) / srt[i, k - 1]))
        pw = conf_t[i, :, 1][pos[i]].double()
        s = float(pw.sum())
        fracs.append(None if bool((pw == 1).all()) else abs(s - round(s)))
    return w, num_pos.view(-1), num_neg.view(-1), gaps, fracs


@pytest.mark.parametrize('name', CASES)
def test_values_gradients_and_selection_vs_oracle(name):
    """Losses and gradients against the CPU oracle, and w = weight * (pos | neg) equal to the oracle's element for
    element.  The exact comparison is legitimate only away from near-ties; that is asserted on the oracle first."""
    size, ncls, targets, seed = _case(name)
    priors = _priors(size)
    B, P = len(targets), priors.shape[0]
    pred = _preds(B, P, ncls, seed)
    want_w, want_np, want_nn, gaps, fracs = _oracle_selection(pred, priors, targets)
    print('num_pos', want_np.tolist(), 'num_neg', want_nn.tolist(), 'gaps', gaps, 'fracs', fracs)
    for i in range(B):      # precondition, on the oracle alone -- a failure here is a failure, not a skip
        assert gaps[i] is None or gaps[i] > 1e-5, 'precondition: image %d cut-off is a near-tie (gap %r)' % (i, gaps[i])
        assert fracs[i] is None or fracs[i] > 1e-3, 'precondition: image %d positive-weight sum near an integer' % i
    if name == 'ignored':
        assert int(want_np[1]) == 0 and float(want_w[1].abs().sum()) == 0.0    # the fully ignored image: nothing mined

    dev = [p.clone().to(DEV).requires_grad_(True) for p in pred]
    cpu = [p.clone().requires_grad_(True) for p in pred]
    crit = _crit(ncls, fused=True)
    mt = crit.match(priors.to(DEV), [t.to(DEV) for t in targets])
    ld = crit(dev, priors.to(DEV), mt)
    lo = loss_ref.multibox_loss_combined(cpu, priors, targets, ncls)
    sum(ld.values()).backward()
    sum(lo.values()).backward()
    _check_losses(ld, lo)
    _check_grads([p.grad for p in dev], [p.grad for p in cpu])

    sums, n, num_pos, w = ops.multibox_loss(dev[0].detach(), dev[1].detach(), dev[2].detach(), mt.loc_t, mt.conf_t,
                                            mt.obj_t, ncls, 3)
    assert torch.equal(num_pos.cpu(), want_np)
    assert int(n) == int(want_np.sum())
    diff = (w.cpu() != want_w)
    assert not diff.any(), '%d of %d loss weights differ from the oracle' % (int(diff.sum()), diff.numel())


# ------------------------------------------------------------------------------------ 3: the tie rule
def _pairs():
    """48 fixed (o0, o1) pairs: CE(label 0) = log(1 + exp(o1 - o0)) takes 48 values at least 1e-2 apart."""
    d = torch.arange(48, dtype=torch.float32) * 0.25 - 3.0
    return torch.stack([torch.full((48,), 0.5), 0.5 + d], 1)


def _stable_w(obj, conf_t, obj_t, ratio):
    """The torch path's selection (multibox_loss_combined.py:58-79) on CPU with sort(stable=True)."""
    B, P = obj_t.shape
    labels, weights = conf_t[:, :, 0], conf_t[:, :, 1]
    pos = labels > 0
    num_pos = (weights * pos.float()).sum(1, keepdim=True).long()
    ce = F.cross_entropy(obj.reshape(-1, 2), obj_t.long().view(-1), reduction='none')
    ce = ce.masked_fill(obj_t.view(-1), 0.0).view(B, -1)
    rank = ce.sort(dim=1, descending=True, stable=True)[1].sort(dim=1, stable=True)[1]
    num_neg = torch.clamp(ratio * num_pos, max=P - 1)
    neg = rank < num_neg.expand_as(rank)
    return weights * (pos | neg).float(), num_pos.view(-1), num_neg.view(-1), ce


def _tied_batch(B, P, ncls, pos_frac, seed, ignore_frac):
    g = torch.Generator().manual_seed(seed)
    pairs = _pairs()
    obj = pairs[torch.randint(0, 48, (B, P), generator=g)]
    loc, conf = torch.randn(B, P, 4, generator=g), torch.randn(B, P, ncls - 1, generator=g) * 3
    conf_t = torch.zeros(B, P, 2)
    conf_t[:, :, 1] = 1.0
    is_pos = torch.rand(B, P, generator=g) < pos_frac
    conf_t[:, :, 0] = torch.where(is_pos, torch.randint(1, ncls, (B, P), generator=g).float(), torch.zeros(B, P))
    obj_t = is_pos.clone() if ignore_frac is None else torch.rand(B, P, generator=g) < ignore_frac
    loc_t = torch.randn(B, P, 4, generator=g)
    return [loc, conf, obj], loc_t, conf_t, obj_t


def _fused_w(pred, loc_t, conf_t, obj_t, ncls, ratio):
    d = [t.to(DEV).contiguous() for t in (*pred, loc_t, conf_t)]
    return ops.multibox_loss(*d, obj_t.to(DEV), ncls, ratio)


def test_tie_rule_cutoff_inside_a_tie_group():
    B, P, ncls = 3, 3000, 21
    pred, loc_t, conf_t, obj_t = _tied_batch(B, P, ncls, 0.02, 17, None)
    want_w, want_np, want_nn, ce = _stable_w(pred[2], conf_t, obj_t, 3)
    srt = ce.sort(1, descending=True)[0]
    for i in range(B):      # precondition: the cut-off really falls inside a group of equal keys
        k = int(want_nn[i])
        assert k > 0 and srt[i, k - 1] == srt[i, k], (i, k)
    vals = torch.unique(ce[ce > 0])
    assert float((vals[1:] - vals[:-1]).min()) >= 1e-2
    sums, n, num_pos, w = _fused_w(pred, loc_t, conf_t, obj_t, ncls, 3)
    assert torch.equal(num_pos.cpu(), want_np)
    assert torch.equal(w.cpu(), want_w)
    # equal keys carry equal objectness losses and weight 1 here, so loss_obj does not depend on WHICH tied priors a sort draws
    ref = _crit(ncls, fused=False)
    from layers.modules.multibox_loss_combined import MatchedTargets
    lo = ref(pred, torch.zeros(P, 4), MatchedTargets(loc_t, conf_t, obj_t))
    got = float(sums[2]) / int(n)
    assert abs(got - float(lo['loss_obj'])) < 2e-5 * max(1.0, abs(float(lo['loss_obj'])))


def test_tie_rule_clamp_takes_zero_key_priors_by_index():
    """40 % positives: 3 * num_pos > P - 1, so all priors but one are drawn -- the zero-key prior of highest index is left."""
    B, P, ncls = 2, 2500, 21
    pred, loc_t, conf_t, obj_t = _tied_batch(B, P, ncls, 0.4, 23, 0.3)
    conf_t[:, -1, 0] = 0            # the last prior: not positive, zero key -> the one prior left out
    obj_t[:, -1] = True
    assert not (conf_t[:, :, 0] < 0).any()
    want_w, want_np, want_nn, ce = _stable_w(pred[2], conf_t, obj_t, 3)
    assert (want_nn == P - 1).all() and ((ce == 0).sum(1) > 1).all()
    assert (want_w[:, -1] == 0).all() and (want_w[:, :-1] == 1).all()
    sums, n, num_pos, w = _fused_w(pred, loc_t, conf_t, obj_t, ncls, 3)
    assert torch.equal(num_pos.cpu(), want_np)
    assert torch.equal(w.cpu(), want_w)


# ------------------------------------------------------------------------------------ 4: edge cases
def _hand_built(B, P, ncls, seed, pos_every=37, extreme=False):
    """Random predictions and hand-built targets; no ties (continuous logits).  extreme: +-1e4 logits on rows that
    are ignored (obj_t set, label -1 or 0), i.e. never positive and never mined."""
    g = torch.Generator().manual_seed(seed)
    pred = _preds(B, P, ncls, seed + 1000)
    conf_t = torch.zeros(B, P, 2)
    conf_t[:, :, 1] = torch.rand(B, P, generator=g) * 0.5 + 0.5
    idx = torch.arange(P)
    is_pos = (idx % pos_every == 0).expand(B, P).clone()
    conf_t[:, :, 0] = torch.where(is_pos, torch.randint(1, ncls, (B, P), generator=g).float(), torch.zeros(B, P))
    obj_t = is_pos.clone()
    loc_t = torch.randn(B, P, 4, generator=g)
    rows = None
    if extreme:
        rows = (idx % 11 == 5) & (idx % pos_every != 0)
        obj_t[:, rows] = True
        conf_t[:, rows, 0] = torch.where(idx[rows] % 2 == 0, -1.0, 0.0)
        sign = torch.where(torch.rand(B, int(rows.sum()), 1, generator=g) < 0.5, -1.0, 1.0)
        for p in pred:
            p[:, rows] = 1e4 * sign * torch.where(torch.arange(p.shape[2]) % 2 == 0, 1.0, -1.0)
    return pred, loc_t, conf_t, obj_t, rows


def _assert_away_from_ties(pred, conf_t, obj_t, ratio):
    """The precondition of the oracle cases for a hand-built batch: the cut-off is no near-tie (relative gap > 1e-5) and
    the positive-weight sum is > 1e-3 from an integer unless all weights are 1 -- asserted on CPU figures alone."""
    _, _, num_neg, ce = _stable_w(pred[2], conf_t, obj_t, ratio)
    srt = ce.sort(1, descending=True)[0].double()
    for i in range(ce.shape[0]):
        k = int(num_neg[i])
        if k > 0 and float(srt[i, k - 1]) > 0:
            gap = float((srt[i, k - 1] - srt[i, k]) / srt[i, k - 1])
            assert gap > 1e-5, 'precondition: image %d cut-off is a near-tie (gap %r)' % (i, gap)
        pw = conf_t[i, :, 1][conf_t[i, :, 0] > 0].double()
        if pw.numel() and not bool((pw == 1).all()):
            sm = float(pw.sum())
            assert abs(sm - round(sm)) > 1e-3, 'precondition: image %d positive-weight sum %r near an integer' % (i, sm)


def _fused_vs_torch_cpu(pred, loc_t, conf_t, obj_t, ncls, ratio=3, combine=None, ref_dtype=torch.float32):
    from layers.modules.multibox_loss_combined import MatchedTargets
    P = pred[0].shape[1]
    _assert_away_from_ties(pred, conf_t, obj_t, ratio)
    combine = combine or (lambda d: sum(d.values()))
    dev = [p.clone().to(DEV).requires_grad_(True) for p in pred]
    cpu = [p.clone().to(ref_dtype).requires_grad_(True) for p in pred]
    ld = _crit(ncls, True, ratio)(dev, torch.zeros(P, 4, device=DEV),
                                  MatchedTargets(loc_t.to(DEV), conf_t.to(DEV), obj_t.to(DEV)))
    lo = _crit(ncls, False, ratio)(cpu, torch.zeros(P, 4), MatchedTargets(loc_t, conf_t, obj_t))
    combine(ld).backward()
    combine(lo).backward()
    _check_losses(ld, lo)
    _check_grads([p.grad for p in dev], [p.grad for p in cpu])
    return dev, cpu


def test_image_without_ground_truth_next_to_one_with_300_boxes():
    from layers.modules.multibox_loss_combined import MatchedTargets
    priors = _priors(300)
    P, ncls = priors.shape[0], 21
    rng = torch.Generator().manual_seed(41)
    xy = torch.rand(300, 2, generator=rng) * 0.7
    wh = torch.rand(300, 2, generator=rng) * 0.25 + 0.05
    many = torch.cat([xy, xy + wh, torch.randint(1, ncls, (300, 1), generator=rng).float(), torch.ones(300, 1)], 1)
    targets = [torch.zeros(0, 6), many]
    mt = _crit(ncls).match(priors.to(DEV), [t.to(DEV) for t in targets])
    mt = MatchedTargets(*(t.cpu() for t in mt))
    assert int((mt.conf_t[0, :, 0] > 0).sum()) == 0 and int((mt.conf_t[1, :, 0] > 0).sum()) >= 300
    pred = _preds(2, P, ncls, 8)
    _fused_vs_torch_cpu(pred, mt.loc_t, mt.conf_t, mt.obj_t, ncls)
    _, _, num_pos, w = _fused_w(pred, mt.loc_t, mt.conf_t, mt.obj_t, ncls, 3)
    assert int(num_pos[0]) == 0 and float(w[0].abs().sum()) == 0.0


@pytest.mark.parametrize('P', [63, 40000])
def test_prior_counts_beside_and_past_the_lds_budget(P):
    pred, loc_t, conf_t, obj_t, _ = _hand_built(2, P, 21, P)
    _fused_vs_torch_cpu(pred, loc_t, conf_t, obj_t, 21)
    want_w = _stable_w(pred[2], conf_t, obj_t, 3)[0]
    assert torch.equal(_fused_w(pred, loc_t, conf_t, obj_t, 21, 3)[3].cpu(), want_w)


def test_single_prior():
    """P = 1: num_neg = min(3 * num_pos, 0) = 0; one image's prior is positive, the other's is not (w = 0)."""
    pred, loc_t, conf_t, obj_t, _ = _hand_built(2, 1, 21, 3)
    conf_t[:, :, 1] = 1
    conf_t[1, 0, 0] = 0
    obj_t[1, 0] = False
    _fused_vs_torch_cpu(pred, loc_t, conf_t, obj_t, 21)
    w = _fused_w(pred, loc_t, conf_t, obj_t, 21, 3)[3].cpu()
    assert float(w[0, 0]) == float(conf_t[0, 0, 1]) and float(w[1, 0]) == 0.0


@pytest.mark.parametrize('ncls', [2, 4, 8])
def test_small_and_unaligned_class_counts(ncls):
    """C = 2 (one foreground logit), and row lengths that are not a multiple of four floats.

    With C = 2 the softmax over the single class logit is identically 1, so the true conf gradient is exactly 0 and the
    fused kernel writes exactly 0.  The fp32 torch path returns rounding noise there (max |grad| 3.7e-9, measured on
    the MI355X run of this test), and `2e-5 * max|ref grad| + 1e-9` of pure noise bounds nothing an exact result can
    meet; for that one case the same torch path is therefore evaluated on fp64 CPU tensors (noise ~1e-17) -- the same
    reference computed more exactly, under the same bound."""
    pred, loc_t, conf_t, obj_t, _ = _hand_built(2, 777, ncls, 50 + ncls)
    _fused_vs_torch_cpu(pred, loc_t, conf_t, obj_t, ncls, ref_dtype=torch.float64 if ncls == 2 else torch.float32)


def test_huge_logits_on_unselected_rows_give_exact_zero_gradients():
    pred, loc_t, conf_t, obj_t, rows = _hand_built(2, 1500, 21, 61, extreme=True)
    dev, cpu = _fused_vs_torch_cpu(pred, loc_t, conf_t, obj_t, 21)
    assert int(rows.sum()) > 100
    for p in dev:
        assert torch.isfinite(p.grad).all()
        assert float(p.grad[:, rows.to(DEV)].abs().max()) == 0.0
    w = _fused_w(pred, loc_t, conf_t, obj_t, 21, 3)[3].cpu()
    assert float(w[:, rows].abs().max()) == 0.0


def test_negpos_ratio_zero_keeps_positives_only():
    pred, loc_t, conf_t, obj_t, _ = _hand_built(2, 900, 21, 71)
    _fused_vs_torch_cpu(pred, loc_t, conf_t, obj_t, 21, ratio=0)
    w = _fused_w(pred, loc_t, conf_t, obj_t, 21, 0)[3].cpu()
    assert torch.equal(w, conf_t[:, :, 1] * (conf_t[:, :, 0] > 0).float())


# ------------------------------------------------------------------------------------ 5: upstream gradients, normaliser
def test_weighted_combination_of_the_three_losses():
    pred, loc_t, conf_t, obj_t, _ = _hand_built(3, 2000, 21, 81)
    _fused_vs_torch_cpu(pred, loc_t, conf_t, obj_t, 21,
                        combine=lambda d: 2 * d['loss_box_reg'] + 0.5 * d['loss_cls'] - d['loss_obj'])


def test_float_normaliser_as_sync_normalizer_uses_it(monkeypatch):
    """ctdet.dist.global_normalizer returns a float quotient (7 positives over 2 ranks = 3.5); both forms must scale by it."""
    from layers.modules.multibox_loss_combined import MatchedTargets
    import ctdet.dist
    monkeypatch.setattr(ctdet.dist, 'global_normalizer',
                        lambda n, dev: torch.tensor(3.5, dtype=torch.float64, device=dev))
    pred, loc_t, conf_t, obj_t, _ = _hand_built(2, 1200, 21, 91)
    dev = [p.clone().to(DEV).requires_grad_(True) for p in pred]
    cpu = [p.clone().requires_grad_(True) for p in pred]
    cf, ct = _crit(21, True), _crit(21, False)
    cf.sync_normalizer = ct.sync_normalizer = True
    ld = cf(dev, torch.zeros(1200, 4, device=DEV), MatchedTargets(loc_t.to(DEV), conf_t.to(DEV), obj_t.to(DEV)))
    lo = ct(cpu, torch.zeros(1200, 4), MatchedTargets(loc_t, conf_t, obj_t))
    sum(ld.values()).backward()
    sum(lo.values()).backward()
    _check_losses(ld, lo)
    _check_grads([p.grad for p in dev], [p.grad for p in cpu])
    sums, n, _, _ = _fused_w(pred, loc_t, conf_t, obj_t, 21, 3)
    assert abs(float(ld['loss_obj']) - float(sums[2]) / 3.5) < 1e-6 * max(1.0, float(sums[2]))


# ------------------------------------------------------------------------------------ 6: reproducibility
def _run_raw(pred, loc_t, conf_t, obj_t, ncls, g):
    d = [t.to(DEV).contiguous() for t in (*pred, loc_t, conf_t)] + [obj_t.to(DEV)]
    sums, n, num_pos, w = ops.multibox_loss(*d, ncls, 3)
    grads = ops.multibox_loss_backward(*d, w, g.to(DEV), ncls)
    return (sums, num_pos, w) + tuple(grads)


def test_two_calls_are_bit_identical_and_images_do_not_see_their_batch_mates():
    priors = _priors(300)
    P, ncls = priors.shape[0], 21
    targets = synth.targets(8, ncls, 7)
    for t in targets:
        t[::2, 5] = 0.37
        t[1::2, 5] = 0.63
    mt = _crit(ncls).match(priors.to(DEV), [t.to(DEV) for t in targets])
    pred = _preds(8, P, ncls, 11)
    g = torch.tensor([0.01, 0.02, -0.005])
    a = _run_raw(pred, mt.loc_t, mt.conf_t, mt.obj_t, ncls, g)
    b = _run_raw(pred, mt.loc_t, mt.conf_t, mt.obj_t, ncls, g)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = _run_raw([p[:4] for p in pred], mt.loc_t[:4], mt.conf_t[:4], mt.obj_t[:4], ncls, g)
    for x, y in zip(a[1:], c[1:]):                   # num_pos, w, dloc, dconf, dobj of images 0-3
        assert torch.equal(x[:4], y)


# ------------------------------------------------------------------------------------ 7: capture
def test_forward_and_backward_replay_from_a_captured_graph():
    from layers.modules.multibox_loss_combined import MatchedTargets
    priors = _priors(300).to(DEV)
    P, ncls, B = priors.shape[0], 21, 4
    crit = _crit(ncls)
    tg1 = [t.to(DEV) for t in synth.targets(B, ncls, 5)]
    tg2 = [t.to(DEV) for t in synth.targets(B, ncls, 6)]
    p1, p2 = _preds(B, P, ncls, 1), _preds(B, P, ncls, 2)
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
    for k in KEYS:
        assert torch.equal(out[k], want[k]), k
    for a, b in zip(grads, want_g):
        assert torch.equal(a, b)
    assert float(want['loss_cls']) > 0


# ------------------------------------------------------------------------------------ 8: end to end
def _net(size, C_):
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), size, C_)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()), strict=True)
    net = net.cuda()
    net.device = 'cuda'
    return net


def test_training_reduces_the_loss_with_the_fused_criterion():
    """tests/test_gpu_train.py::test_training_reduces_the_loss_on_a_fixed_batch with fused=True, same criterion."""
    net = _net(300, 20).train()
    priors = _priors(300).cuda()
    crit = _crit(21, fused=True)
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
    assert losses[-1] < 0.5 * losses[0], losses


def test_head_bias_gradients_agree_between_the_two_forms():
    net = _net(300, 20).train()
    priors = _priors(300).cuda()
    x = synth.images(2, 300, 'randn', 31).cuda()
    tg = [t.cuda() for t in synth.targets(2, 21, 13)]
    grads = {}
    for fused in (False, True):
        net.zero_grad(set_to_none=True)
        sum(_crit(21, fused=fused)(net(x), priors, tg).values()).backward()
        grads[fused] = {n: p.grad.detach().clone() for n, p in net.named_parameters()
                        if n.split('.')[0] in ('loc', 'conf', 'obj') and n.endswith('.bias')}
    assert len(grads[True]) >= 18
    # one gradient per prediction, as in the tolerance's own test: the biases of all six scales of a head family side by
    # side (a scale without positives has a conf gradient of exactly 0, where the torch path leaves 2e-8 of rounding noise)
    for fam in ('loc', 'conf', 'obj'):
        names = sorted(n for n in grads[False] if n.split('.')[0] == fam)
        assert len(names) >= 6, names
        ref = torch.cat([grads[False][n].flatten() for n in names])
        got = torch.cat([grads[True][n].flatten() for n in names])
        assert torch.isfinite(got).all(), fam
        err, top = float((got - ref).abs().max()), float(ref.abs().max())
        print('bias grad %-5s max err %.3g of max %.3g' % (fam, err, top))
        assert err <= 2e-5 * top + 1e-9, (fam, err, top)


# ------------------------------------------------------------------------------------ 9: C ABI
def test_c_abi_refuses_bad_arguments_and_short_workspaces():
    lib = _lib.lib()
    B, P, ncls = 2, 100, 21
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)
    loc, conf, obj, loc_t, conf_t = z(B, P, 4), z(B, P, ncls - 1), z(B, P, 2), z(B, P, 4), z(B, P, 2)
    obj_t, sums, num_pos, n, w = z(B, P, dt=torch.uint8), z(3), z(B, dt=torch.int64), z(1, dt=torch.int64), z(B, P)
    need = lib.ct_multibox_loss_workspace_bytes(B, P, ncls)
    assert need >= B * P * 16
    ws = z(need, dt=torch.uint8)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def fwd(loc_=loc, batch=B, npri=P, nc=ncls, ratio=3, ws_bytes=need):
        return lib.ct_multibox_loss_fwd(ptr(loc_) if loc_ is not None else None, ptr(conf), ptr(obj), ptr(loc_t),
                                        ptr(conf_t), ptr(obj_t), batch, npri, nc, ratio, ptr(sums), ptr(num_pos),
                                        ptr(n), ptr(w), ptr(ws), ws_bytes, st)

    assert fwd() == _lib.CT_OK
    for kw, status in (({'loc_': None}, 1), ({'nc': 1}, 1), ({'batch': 0}, 1), ({'npri': -3}, 1), ({'ratio': -1}, 1),
                       ({'ws_bytes': need - 1}, 3)):
        assert fwd(**kw) == status, kw
        assert b'ct_multibox_loss_fwd' in lib.ct_last_error_string(), kw
    g, dloc, dconf, dobj = z(3), z(B, P, 4), z(B, P, ncls - 1), z(B, P, 2)

    def bwd(g_=g, nc=ncls, npri=P):
        return lib.ct_multibox_loss_bwd(ptr(loc), ptr(conf), ptr(obj), ptr(loc_t), ptr(conf_t), ptr(obj_t), ptr(w),
                                        ptr(g_) if g_ is not None else None, B, npri, nc, ptr(dloc), ptr(dconf),
                                        ptr(dobj), st)

    assert bwd() == _lib.CT_OK
    for kw in ({'g_': None}, {'nc': 0}, {'npri': 0}):
        assert bwd(**kw) == 1, kw
        assert b'ct_multibox_loss_bwd' in lib.ct_last_error_string(), kw
    torch.cuda.synchronize()
    with pytest.raises(_lib.CtdetError):
        ops.multibox_loss(loc.cpu(), conf, obj, loc_t, conf_t, obj_t, ncls, 3)


def test_switch_shows_in_the_policy_record(monkeypatch):
    """CTDET_LOSS_FUSED is reported like every other set CTDET_* variable (bench.py prints it as config.policy.env)."""
    monkeypatch.setenv('CTDET_LOSS_FUSED', '1')
    from ctdet.pipeline import DetectionPipeline
    pipe = DetectionPipeline(_net(300, 20).eval(), _priors(300), 1, 20)
    assert pipe.rt.policy_record()['env'].get('CTDET_LOSS_FUSED') == '1'
