"""Shared inputs and float64 references of tests/test_iou_loss_cpu.py and tests/test_gpu_iou_loss.py: every case is
matched ONCE on the CPU (oracle.box_ref.match), its reference computed once and handed out unchanged.  The loc term's
reference is tests/iou_loss_ref.py, the class and objectness terms' is oracle.loss_ref; never the code under test."""
import functools
import types

import torch

from ctdet import synth
from oracle import box_ref, loss_ref

import iou_loss_ref as twin

KINDS = twin.KINDS
KEYS = ('loss_box_reg', 'loss_cls', 'loss_obj')


@functools.lru_cache(None)
def priors(size):
    from layers.functions import PriorBox
    import data as cfgs
    return PriorBox(cfgs.VOC_300 if size == 300 else cfgs.VOC_512).forward()


def preds(B, P, ncls, seed):
    """As tests/test_gpu_loss_fused.py::_preds: ONE generator; loc, conf * 3, obj in that order."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, P, 4, generator=g), torch.randn(B, P, ncls - 1, generator=g) * 3,
            torch.randn(B, P, 2, generator=g)]


def _targets(name):
    """-> size, num_classes, targets, prediction seed"""
    if name == 'A':
        return 300, 21, synth.targets(3, 21, 99), 5
    if name == 'A_mixup':
        tg = synth.targets(3, 21, 99)
        for t in tg:
            t[::2, 5] = 0.37
            t[1::2, 5] = 0.63
        return 300, 21, tg, 5
    if name == 'A_ignored':                     # as tests/test_gpu_loss_fused.py::_case('ignored')
        tg = synth.targets(3, 21, 99)
        for t in tg:
            t[::2, 4] = -1
        tg[1][:, 4] = -1
        tg[0][0, 4] = 3
        return 300, 21, tg, 5
    if name == 'A_mixup_ignored':               # mixup weights and one ignored box per image
        tg = synth.targets(3, 21, 99)
        for t in tg:
            t[::2, 5] = 0.37
            t[1::2, 5] = 0.63
            t[-1, 4] = -1
        return 300, 21, tg, 5
    if name == 'B':
        return 512, 61, synth.targets(2, 61, 22), 3      # seed 22: 203 positives (seed 21 gives 99)
    raise KeyError(name)


def match_cpu(pri, targets):
    """oracle.box_ref.match per image -> loc_t [B,P,4], conf_t [B,P,2], obj_t [B,P] bool"""
    B, P = len(targets), pri.shape[0]
    loc_t, conf_t, obj_t = torch.zeros(B, P, 4), torch.zeros(B, P, 2), torch.zeros(B, P, dtype=torch.bool)
    for i, t in enumerate(targets):
        loc_t[i], conf_t[i], obj_t[i], _ = box_ref.match(0.5, t[:, :-2], pri, [0.1, 0.2], t[:, -2:])
    return loc_t, conf_t, obj_t


def loc_reference(kind, loc, loc_t, conf_t, pri, n):
    """The twin's loss_box_reg = sum / n and its gradient w.r.t. loc, float64."""
    x = loc.double().requires_grad_(True)
    val = twin.loc_sum(kind, x, loc_t, conf_t, pri) / n
    g, = torch.autograd.grad(val, x)
    return float(val.detach()), g


@functools.lru_cache(None)
def case(name, xy_scale=1.0):
    """One case with everything the comparisons need.  xy_scale multiplies loc[..., :2] (10: the non-overlap branch)."""
    size, ncls, targets, seed = _targets(name)
    pri = priors(size)
    B, P = len(targets), pri.shape[0]
    pred = preds(B, P, ncls, seed)
    pred[0][..., :2] *= xy_scale
    loc_t, conf_t, obj_t = match_cpu(pri, targets)
    cpu = [p.clone().requires_grad_(True) for p in pred]
    lo = loss_ref.multibox_loss_combined(cpu, pri, targets, ncls)
    (lo['loss_cls'] + lo['loss_obj']).backward()
    pos = conf_t[..., 0] > 0
    n = int((conf_t[..., 1] * pos.float()).sum(1).long().sum())
    c = types.SimpleNamespace(name=name, size=size, ncls=ncls, targets=targets, priors=pri, pred=pred, loc_t=loc_t,
                              conf_t=conf_t, obj_t=obj_t, n=n, pos=pos, loss_cls=float(lo['loss_cls'].detach()),
                              loss_obj=float(lo['loss_obj'].detach()), dconf=cpu[1].grad, dobj=cpu[2].grad, loc={})
    for kind in KINDS:
        c.loc[kind] = loc_reference(kind, pred[0], loc_t, conf_t, pri, n)
    return c


def check_loss(name, got, want):
    got = float(got.detach()) if isinstance(got, torch.Tensor) else float(got)
    print('loss %-12s got %.8g ref %.8g rel %.3g' % (name, got, want, abs(got - want) / max(1.0, abs(want))))
    assert abs(got - want) < 2e-5 * max(1.0, abs(want)), (name, got, want)
    return abs(got - want) / max(1.0, abs(want))


def check_grad(name, got, want):
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), name
    err, ref = float((got - want.double()).abs().max()), float(want.abs().max())
    print('grad %-5s max err %.3g of max %.3g (%.3g of the bound)' % (name, err, ref, err / (2e-5 * ref + 1e-9)))
    assert err <= 2e-5 * ref + 1e-9, (name, err, ref)
    return err / ref if ref else 0.0


def overlap_stats(c):
    """On the twin alone: positives, the fraction with inter == 0, the smallest kink distance over the positives."""
    pri = c.priors.expand(c.pred[0].shape[0], -1, -1)
    loc, loc_t, p = c.pred[0][c.pos], c.loc_t[c.pos], pri[c.pos]
    t = twin.terms(loc.double(), loc_t.double(), p.double())
    return int(c.pos.sum()), float((t['inter'] == 0).double().mean()), float(twin.kink_distance(loc, loc_t, p).min())
