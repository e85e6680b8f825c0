"""The fused MultiBoxLoss switch and its C ABI surface, as far as they can be checked without a GPU."""
import os
import re

import pytest
import torch

from conftest import REPO
from ctdet import _lib
from layers.modules.multibox_loss_combined import MatchedTargets, MultiBoxLoss_combined

SYMBOLS = ('ct_multibox_loss_workspace_bytes', 'ct_multibox_loss_fwd', 'ct_multibox_loss_bwd')


def _crit(**kw):
    return MultiBoxLoss_combined(21, 0.5, True, 0, True, 3, 0.5, False, **kw)


def _batch(B=2, P=40, C=21, seed=0):
    g = torch.Generator().manual_seed(seed)
    preds = [torch.randn(B, P, 4, generator=g), torch.randn(B, P, C - 1, generator=g), torch.randn(B, P, 2, generator=g)]
    conf_t = torch.zeros(B, P, 2)
    conf_t[:, :, 1] = 1
    conf_t[:, :3, 0] = torch.tensor([1., 7., 20.])
    obj_t = conf_t[:, :, 0] > 0
    return preds, MatchedTargets(torch.randn(B, P, 4, generator=g), conf_t, obj_t)


def test_loss_symbols_are_declared_and_bound():
    hdr = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    declared = set(re.findall(r'\b(ct_[a-z0-9_]+)\s*\(', hdr))
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES['ct_multibox_loss_fwd'][1]) == 17
    assert len(_lib.SIGNATURES['ct_multibox_loss_bwd'][1]) == 15
    lib = _lib.lib()
    assert lib.ct_multibox_loss_workspace_bytes(2, 100, 21) >= 2 * 100 * 16
    # the header states the two rules that are part of the contract
    text = hdr[hdr.index('ct_multibox_loss_workspace_bytes') - 2500:hdr.index('ct_multibox_loss_workspace_bytes')]
    assert 'multibox_loss_combined.py:76-122' in text
    assert 'ascending prior index' in text and 'num_pos rule' in text


def test_fused_true_constructs_and_refuses_cpu_tensors():
    crit = _crit(fused=True)
    assert crit.fused is True
    preds, mt = _batch()
    with pytest.raises(_lib.CtdetError, match='HIP device'):
        crit(preds, torch.zeros(40, 4), mt)


def test_fused_none_follows_the_environment(monkeypatch):
    monkeypatch.delenv('CTDET_LOSS_FUSED', raising=False)
    assert _crit().fused is False
    assert _crit(fused=None).fused is False
    monkeypatch.setenv('CTDET_LOSS_FUSED', '1')
    assert _crit().fused is True
    assert _crit(fused=False).fused is False
    monkeypatch.setenv('CTDET_LOSS_FUSED', '0')
    assert _crit().fused is False
    assert _crit(fused=True).fused is True


def test_default_takes_the_torch_path_on_cpu_tensors(monkeypatch):
    monkeypatch.delenv('CTDET_LOSS_FUSED', raising=False)
    crit = _crit()
    assert crit.fused is False
    preds, mt = _batch()
    preds = [p.requires_grad_(True) for p in preds]
    out = crit(preds, torch.zeros(40, 4), mt)
    assert set(out) == {'loss_box_reg', 'loss_cls', 'loss_obj'}
    sum(out.values()).backward()
    assert all(torch.isfinite(v) for v in out.values())
    assert all(torch.isfinite(p.grad).all() for p in preds)
