"""The IoU-family localisation terms (loc_loss = iou / giou / diou / ciou) as far as they can be checked without a GPU:
the float64 twin itself, the criterion's torch path against the twin, and the surface (header, binding, switch, C ABI
refusals).  Tolerances are the project's loss rule: 2e-5 * max(1, |ref|) for a loss, 2e-5 * max|ref grad| + 1e-9 for a
gradient."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import REPO
from ctdet import _lib
from layers.modules.multibox_loss_combined import MatchedTargets, MultiBoxLoss_combined

import iou_loss_cases as cases
import iou_loss_ref as twin

KINDS = twin.KINDS


def _crit(**kw):
    return MultiBoxLoss_combined(21, 0.5, True, 0, True, 3, 0.5, False, **kw)


# ------------------------------------------------------------------------------------ 1: the twin
def _hand_rows():
    """16 rows placed by hand: (prior, loc, loc_t) -- shifted, nested, partly overlapping and disjoint boxes of several
    aspect ratios, none near a kink."""
    pri = torch.tensor([[0.50, 0.50, 0.20, 0.30], [0.30, 0.60, 0.40, 0.15], [0.70, 0.25, 0.10, 0.10],
                        [0.45, 0.55, 0.60, 0.50]], dtype=torch.float64).repeat(4, 1)
    loc = torch.tensor([[0.9, -0.6, 0.5, -0.3], [-1.2, 0.8, -0.7, 0.9], [0.3, 0.4, 1.1, 0.6], [-0.5, -0.9, -0.4, -1.0],
                        [2.1, 1.7, 0.2, 0.3], [-1.9, 2.2, -0.3, 0.1], [0.2, -0.1, 1.9, 1.6], [0.1, 0.3, -1.8, -2.0],
                        [14.0, 0.5, 0.3, -0.2], [0.4, -16.0, -0.5, 0.4], [-13.0, 12.0, 0.6, 0.2], [15.0, 17.0, -0.1, -0.6],
                        [1.1, 0.2, 0.8, -0.9], [-0.3, 1.3, -1.1, 0.7], [0.6, 0.7, 0.4, 1.2], [-0.8, -0.2, 1.3, -0.5]],
                       dtype=torch.float64)
    loc_t = torch.tensor([[0.1, 0.2, -0.2, 0.4], [0.3, -0.4, 0.1, 0.2], [-0.6, 0.1, 0.3, -0.5], [0.2, 0.5, 0.6, -0.1]],
                         dtype=torch.float64).repeat_interleave(4, 0).roll(1, 0)
    return pri, loc, loc_t


def test_twin_gradcheck_away_from_kinks():
    pri, loc, loc_t = _hand_rows()
    # gradcheck moves an offset by 1e-6, i.e. a coordinate by less than 1e-6 image units
    assert float(twin.kink_distance(loc, loc_t, pri).min()) > 1e-4
    inter = twin.terms(loc, loc_t, pri)['inter']
    assert int((inter == 0).sum()) == 4 and int((inter > 0).sum()) == 12       # rows 8-11 are disjoint
    x = loc.clone().requires_grad_(True)
    for kind in ('iou', 'giou', 'diou'):
        assert torch.autograd.gradcheck(lambda l: twin.loss_rows(kind, l, loc_t, pri), (x,), eps=1e-6, atol=1e-7)
    alpha = twin.alpha_of(twin.terms(loc, loc_t, pri))
    assert float(alpha.min()) >= 0 and float(alpha.max()) > 1e-3
    assert torch.autograd.gradcheck(lambda l, a: twin.loss_rows('ciou', l, loc_t, pri, alpha=a), (x, alpha), eps=1e-6,
                                    atol=1e-7)
    # the detached alpha gives the gradient of "alpha supplied as a constant"
    g1, = torch.autograd.grad(twin.loss_rows('ciou', x, loc_t, pri).sum(), x)
    g2, = torch.autograd.grad(twin.loss_rows('ciou', x, loc_t, pri, alpha=alpha).sum(), x)
    assert torch.equal(g1, g2)


def test_twin_values():
    pri, loc, loc_t = _hand_rows()
    for kind in KINDS:                                  # identical boxes
        assert float(twin.loss_rows(kind, loc, loc, pri).abs().max()) < 1e-12, kind
    dis = slice(8, 12)                                  # disjoint boxes
    assert torch.equal(twin.loss_rows('iou', loc[dis], loc_t[dis], pri[dis]), torch.ones(4, dtype=torch.float64))
    assert float(twin.loss_rows('giou', loc[dis], loc_t[dis], pri[dis]).min()) > 1.0
    t = twin.terms(loc, loc_t, pri)
    extra = twin.loss_rows('ciou', loc, loc_t, pri) - twin.loss_rows('diou', loc, loc_t, pri)
    assert float(extra.min()) >= 0 and float(extra.max()) > 1e-4
    assert float((extra - twin.alpha_of(t) * t['v']).abs().max()) < 1e-15
    same = loc.clone()
    same[:, 2:] = loc_t[:, 2:]                          # equal aspect ratios: v = 0, alpha = 0
    assert float((twin.loss_rows('ciou', same, loc_t, pri) - twin.loss_rows('diou', same, loc_t, pri)).abs().max()) == 0.0
    assert float(twin.alpha_of(twin.terms(same, loc_t, pri)).abs().max()) == 0.0


# ------------------------------------------------------------------------------------ 2: the criterion's torch path
def _run_torch_path(c, loc_loss, loc_weight=1.0):
    pred = [p.clone().requires_grad_(True) for p in c.pred]
    crit = MultiBoxLoss_combined(c.ncls, 0.5, True, 0, True, 3, 0.5, False, fused=False, loc_loss=loc_loss,
                                 loc_weight=loc_weight)
    out = crit(pred, c.priors, MatchedTargets(c.loc_t, c.conf_t, c.obj_t))
    sum(out.values()).backward()
    return out, [p.grad for p in pred]


@pytest.mark.parametrize('name', ['A', 'A_mixup_ignored'])
def test_torch_path_against_the_twin(name):
    c = cases.case(name)
    assert (c.conf_t[..., 0] < 0).any() == (name == 'A_mixup_ignored')
    base, base_g = _run_torch_path(c, 'smooth_l1')
    for kind in KINDS:
        out, grads = _run_torch_path(c, kind)
        want, want_g = c.loc[kind]
        cases.check_loss(kind, out['loss_box_reg'], want)
        cases.check_grad('loc', grads[0], want_g)
        assert torch.equal(out['loss_cls'], base['loss_cls']) and torch.equal(out['loss_obj'], base['loss_obj'])
        assert torch.equal(grads[1], base_g[1]) and torch.equal(grads[2], base_g[2])
        cases.check_loss('loss_cls', out['loss_cls'], c.loss_cls)
        cases.check_loss('loss_obj', out['loss_obj'], c.loss_obj)


def test_torch_path_ignores_whatever_a_row_that_is_not_positive_holds():
    c = cases.case('A')
    crit = _crit(fused=False, loc_loss='ciou')
    pred = [p.clone() for p in c.pred]
    pred[0][~c.pos] = float('nan')
    pred[0][:, ::2][~c.pos[:, ::2]] = 1e30
    pred = [p.requires_grad_(True) for p in pred]
    out = crit(pred, c.priors, MatchedTargets(c.loc_t, c.conf_t, c.obj_t))
    out['loss_box_reg'].backward()
    cases.check_loss('ciou', out['loss_box_reg'], c.loc['ciou'][0])
    assert torch.isfinite(pred[0].grad).all() and float(pred[0].grad[~c.pos].abs().max()) == 0.0


def test_loc_weight_scales_value_and_gradient():
    c = cases.case('A')
    eps = 2.0 ** -23                                    # one fp32 rounding
    for kind in ('smooth_l1', 'giou'):
        one, one_g = _run_torch_path(c, kind, 1.0)
        out, grads = _run_torch_path(c, kind, 2.5)
        a, b = float(out['loss_box_reg']), 2.5 * float(one['loss_box_reg'])
        assert abs(a - b) <= eps * abs(b), (kind, a, b)
        d = (grads[0].double() - 2.5 * one_g[0].double()).abs()
        assert bool((d <= eps * (2.5 * one_g[0].double()).abs()).all()), kind
        assert float(one_g[0].abs().max()) > 0
        for k in ('loss_cls', 'loss_obj'):
            assert torch.equal(out[k], one[k])
        assert torch.equal(grads[1], one_g[1]) and torch.equal(grads[2], one_g[2])


# ------------------------------------------------------------------------------------ 3: the surface
def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    declared = set(re.findall(r'\b(ct_[a-z0-9_]+)\s*\(', hdr))
    for s in ('ct_multibox_loss_fwd_loc', 'ct_multibox_loss_bwd_loc'):
        assert s in declared and s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES['ct_multibox_loss_fwd_loc'][1]) == 17 + 4
    assert len(_lib.SIGNATURES['ct_multibox_loss_bwd_loc'][1]) == 15 + 4
    for i, name in enumerate(('CT_LOC_SMOOTH_L1', 'CT_LOC_IOU', 'CT_LOC_GIOU', 'CT_LOC_DIOU', 'CT_LOC_CIOU')):
        assert re.search(r'\b%s = %d\b' % (name, i), hdr), name
        assert _lib.LOC_LOSSES[i] == name[len('CT_LOC_'):].lower()
    assert 'CTDET_ABI_VERSION 1' in hdr and _lib.lib().ct_abi_version() == 1
    assert 'alpha is a CONSTANT in the backward pass' in hdr


def test_loc_loss_follows_the_environment_and_refuses_unknown_names(monkeypatch):
    monkeypatch.delenv('CTDET_LOC_LOSS', raising=False)
    assert _crit().loc_loss == 'smooth_l1' and _crit().loc_weight == 1.0
    monkeypatch.setenv('CTDET_LOC_LOSS', '')
    assert _crit().loc_loss == 'smooth_l1'
    monkeypatch.setenv('CTDET_LOC_LOSS', 'giou')
    assert _crit().loc_loss == 'giou'
    assert _crit(loc_loss='ciou').loc_loss == 'ciou'
    assert _crit(loc_loss='smooth_l1').loc_loss == 'smooth_l1'
    for make in (lambda: _crit(loc_loss='l2'), lambda: (monkeypatch.setenv('CTDET_LOC_LOSS', 'GIoU'), _crit())):
        with pytest.raises(ValueError) as e:
            make()
        for name in ('smooth_l1', 'iou', 'giou', 'diou', 'ciou'):
            assert name in str(e.value)


def test_fused_with_an_iou_term_still_refuses_cpu_tensors():
    c = cases.case('A')
    crit = MultiBoxLoss_combined(c.ncls, 0.5, True, 0, True, 3, 0.5, False, fused=True, loc_loss='giou')
    with pytest.raises(_lib.CtdetError, match='HIP device'):
        crit(c.pred, c.priors, MatchedTargets(c.loc_t, c.conf_t, c.obj_t))


def test_c_abi_refuses_bad_loc_arguments_without_a_device():
    """The checks of the _loc entries come before any HIP call and before the pointers are looked at."""
    lib = _lib.lib()
    buf = (C.c_float * 16)()
    host = C.cast(buf, C.c_void_p)

    def fwd(priors, kind, v0, v1):
        return lib.ct_multibox_loss_fwd_loc(None, None, None, None, None, None, 2, 100, 21, 3, None, None, None, None,
                                            None, 0, None, priors, kind, v0, v1)

    def bwd(priors, kind, v0, v1):
        return lib.ct_multibox_loss_bwd_loc(None, None, None, None, None, None, None, None, 2, 100, 21, None, None, None,
                                            None, priors, kind, v0, v1)

    for fn, name in ((fwd, b'ct_multibox_loss_fwd_loc'), (bwd, b'ct_multibox_loss_bwd_loc')):
        for args, word in (((host, 5, 0.1, 0.2), b'loc_loss=5'), ((host, -1, 0.1, 0.2), b'loc_loss=-1'),
                           ((None, 2, 0.1, 0.2), b'priors'), ((None, 4, 0.1, 0.2), b'priors'),
                           ((host, 2, 0.0, 0.2), b'variances'), ((host, 2, 0.1, -0.2), b'variances'),
                           ((host, 0, math.nan, 0.2), b'variances'), ((host, 3, 0.1, math.inf), b'variances'),
                           ((None, 0, 0.1, 0.2), b'null pointer')):      # smooth-L1 needs no priors: the old checks answer
            assert fn(*args) == 1, (name, args)
            msg = lib.ct_last_error_string()
            assert name in msg and word in msg, (args, msg)
