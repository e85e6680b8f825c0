"""The fused SGD step without a device: the NumPy restatement of the recurrence (tests/sgd_ref.py) against
torch.optim.SGD on the CPU, the C ABI surface (export, binding, host-side argument errors), the opt-in switch of
utils/solver.py::build_optimizer and the refusals of ctdet.optim.FusedSGD."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import sgd_ref
from models.RFB_Net_vgg import build_net
from utils import solver

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, 'context-transformer_amd', 'lib', 'libctdet.so')
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'solver.npz'))


@pytest.mark.parametrize('momentum,dampening,nesterov', [(0.0, 0.0, False), (0.9, 0.0, False), (0.9, 0.1, False),
                                                         (0.9, 0.0, True)])
@pytest.mark.parametrize('wd', [0.0, 5e-4])
def test_restatement_is_close_to_torch_cpu_sgd(momentum, dampening, nesterov, wd):
    """6 steps over 100 003 elements: the fp32 restatement and torch's CPU SGD against the fp64 restatement.  torch
    is the yardstick and its own error the tolerance (2 x own + one ulp of the largest parameter)."""
    rng = np.random.RandomState(7)
    n, lr = 100003, 0.05
    p0 = rng.randn(n).astype(np.float32)
    grads = [(rng.randn(n) * 1e-1).astype(np.float32) for _ in range(6)]
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([tp], lr, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    p32, b32, p64, b64 = p0.copy(), None, p0.astype(np.float64), None
    for i, g in enumerate(grads):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p32, b32 = sgd_ref.step(p32, g, b32, lr, wd, momentum, dampening, nesterov, first_step=i == 0)
        p64, b64 = sgd_ref.step(p64, g, b64, lr, wd, momentum, dampening, nesterov, first_step=i == 0,
                                dtype=np.float64)
        assert p32.dtype == np.float32 and p64.dtype == np.float64
        if i == 0:
            first_equal = sgd_ref.bits_equal(p32, tp.detach().numpy())
    ok, e_ref, e_torch, bound = sgd_ref.close_to_torch(p32, tp.detach().numpy(), p64)
    differ = int((p32.view(np.uint32) != tp.detach().numpy().view(np.uint32)).sum())
    print('restatement %.3e  torch %.3e  bound %.3e  | %d of %d elements differ from torch, step 1 bit-equal: %s'
          % (e_ref, e_torch, bound, differ, n, first_equal))
    assert ok, (e_ref, e_torch, bound)
    if momentum != 0:
        assert b32 is not None and b32.dtype == np.float32
        ok, e_ref, e_torch, bound = sgd_ref.close_to_torch(b32, opt.state[tp]['momentum_buffer'].numpy(), b64)
        print('momentum buffer: restatement %.3e  torch %.3e  bound %.3e' % (e_ref, e_torch, bound))
        assert ok, (e_ref, e_torch, bound)
    else:
        assert b32 is None


def test_library_exports_and_binds_ct_sgd_step():
    assert os.path.exists(LIB), 'build the library first (context-transformer_amd/build.py)'
    r = subprocess.run(['nm', '-D', '--defined-only', LIB], capture_output=True, text=True)
    assert r.returncode == 0 and ' T ct_sgd_step' in r.stdout and ' T ct_sgd_tensors_per_launch' in r.stdout
    from ctdet import _lib
    assert 'ct_sgd_step' in _lib.SIGNATURES
    fn = _lib.lib().ct_sgd_step
    assert fn.restype is C.c_int and len(fn.argtypes) == 7
    assert C.sizeof(_lib.SgdTensor) == 48                     # 3 pointers, int64, 2 floats, int, tail padding
    assert _lib.lib().ct_sgd_tensors_per_launch() == 80       # the launch rule include/ctdet.h states
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    assert 'int ct_sgd_step(const ct_sgd_tensor* items_host, int n, float momentum, float dampening,' in header


def _args(method, phase, setting):
    return types.SimpleNamespace(method=method, phase=phase, setting=setting, lr=4e-3, weight_decay=5e-4,
                                 momentum=0.9, steps=[30, 50], warmup_iter=10)


@pytest.mark.parametrize('env', [None, '0'])
def test_build_optimizer_default_is_torch_sgd(monkeypatch, env):
    if env is None:
        monkeypatch.delenv('CTDET_SGD_FUSED', raising=False)
    else:
        monkeypatch.setenv('CTDET_SGD_FUSED', env)
    args = _args('ours', 2, 'transfer')
    net = build_net(args, 300, 20)
    opt = solver.build_optimizer(args, net)
    assert type(opt) is torch.optim.SGD
    assert [g['params'][0].numel() for g in opt.param_groups] == G['p2ours_numel'].tolist()
    assert np.array_equal(np.array([g['lr'] for g in opt.param_groups]), G['p2ours_lr'])
    assert np.array_equal(np.array([g['weight_decay'] for g in opt.param_groups]), G['p2ours_wd'])
    assert opt.defaults['momentum'] == 0.9


def test_build_optimizer_switch_gives_fused_over_the_same_groups(monkeypatch):
    from ctdet.optim import FusedSGD
    args = _args('ours', 2, 'transfer')
    net = build_net(args, 300, 20)
    monkeypatch.setenv('CTDET_SGD_FUSED', '1')
    for opt in (solver.build_optimizer(args, net), solver.build_optimizer(args, net, fused=True)):
        assert type(opt) is FusedSGD and isinstance(opt, torch.optim.Optimizer)
        assert [g['params'][0].numel() for g in opt.param_groups] == G['p2ours_numel'].tolist()
        assert np.array_equal(np.array([g['lr'] for g in opt.param_groups]), G['p2ours_lr'])
        assert np.array_equal(np.array([g['weight_decay'] for g in opt.param_groups]), G['p2ours_wd'])
        assert opt.defaults['momentum'] == 0.9 and opt.grad_scale == 1.0
    assert type(solver.build_optimizer(args, net, fused=False)) is torch.optim.SGD      # the argument beats the variable
    # the schedule drives the fused class as it drives torch's: same lr rows as the golden of the reference
    opt = solver.build_optimizer(args, net, fused=True)
    sched = solver.build_lr_scheduler(args, opt)
    rows = []
    for it in range(60):
        rows.append([opt.param_groups[0]['lr'], opt.param_groups[-1]['lr']])
        opt.step()                                            # no gradients: nothing to launch
        sched.step()
    assert np.array_equal(np.array(rows), G['p2ours_sched'])


def test_fused_sgd_refuses_cpu_parameters_and_unsupported_modes():
    from ctdet._lib import CtdetError
    from ctdet.optim import FusedSGD
    p = torch.nn.Parameter(torch.zeros(5))
    before = p.detach().clone()
    for momentum in (0.0, 0.9):
        opt = FusedSGD([p], 0.1, momentum=momentum)
        p.grad = torch.ones(5)
        with pytest.raises(CtdetError):
            opt.step()
        assert torch.equal(p.detach(), before) and 'momentum_buffer' not in opt.state.get(p, {})
    for kw in ({'maximize': True}, {'foreach': True}, {'fused': True}, {'differentiable': True},
               {'nesterov': True}, {'nesterov': True, 'momentum': 0.9, 'dampening': 0.1},
               {'momentum': -0.1}, {'weight_decay': -1.0}):
        with pytest.raises(ValueError):
            FusedSGD([p], 0.1, **kw)
    with pytest.raises(ValueError):
        FusedSGD([p], -0.1)
    FusedSGD([p], 0.1, maximize=False, foreach=None, fused=None, differentiable=False)
    FusedSGD([p], 0.1, momentum=0.9, nesterov=True)


def test_state_dict_layout_is_torchs():
    """Group keys and defaults as torch.optim.SGD has them, so state dicts move between the classes (the tensors'
    side of the interchange runs on the device: tests/test_gpu_sgd_fused.py)."""
    from ctdet.optim import FusedSGD
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))]
    groups = [{'params': [ps[0]], 'lr': 0.5}, {'params': [ps[1]], 'weight_decay': 1e-3}]
    a = torch.optim.SGD(groups, 0.1, momentum=0.9)
    b = FusedSGD([{'params': [ps[0]], 'lr': 0.5}, {'params': [ps[1]], 'weight_decay': 1e-3}], 0.1, momentum=0.9)
    assert a.state_dict()['param_groups'] == b.state_dict()['param_groups']
    ps[0].grad = torch.ones(3)
    a.step()
    b.load_state_dict(a.state_dict())
    assert torch.equal(b.state[ps[0]]['momentum_buffer'], a.state[ps[0]]['momentum_buffer']) and ps[1] not in b.state
    a2 = torch.optim.SGD(groups, 0.1, momentum=0.9)
    a2.load_state_dict(b.state_dict())
    assert a2.state_dict()['param_groups'] == a.state_dict()['param_groups']


def test_ct_sgd_step_argument_errors():
    """Host-side checks: they return before anything touches a device (the library loads without one, as
    tests/test_c_abi_cpu.py relies on)."""
    from ctdet import _lib
    try:
        lib = _lib.lib()
    except _lib.CtdetError as e:                              # pragma: no cover
        pytest.skip('libctdet cannot be loaded on this box: %s' % e)
    T = _lib.SgdTensor
    ok = dict(param=0x1000, grad=0x2000, momentum_buf=0x3000, numel=16, lr=0.1, weight_decay=0.0, first_step=1)

    def call(items, n=None, momentum=0.9, dampening=0.0, nesterov=0):
        arr = (T * max(len(items), 1))(*[T(**it) for it in items])
        return lib.ct_sgd_step(arr, len(items) if n is None else n, momentum, dampening, nesterov, 1.0, None)

    assert call([], n=0) == 0                                                   # n == 0: valid no-op
    assert lib.ct_sgd_step(None, 0, 0.9, 0.0, 0, 1.0, None) == 0
    assert call([dict(ok, numel=0)]) == 0                                       # numel == 0: valid no-op
    assert call([dict(ok, numel=0, momentum_buf=None)], momentum=0.0) == 0
    bad = [
        (dict(items=[ok], n=-1), 'negative'),
        (dict(items=[dict(ok, param=None)]), 'param'),
        (dict(items=[dict(ok, numel=0), dict(ok, grad=None)]), 'grad'),
        (dict(items=[dict(ok, momentum_buf=None)]), 'momentum_buf'),
        (dict(items=[dict(ok, numel=-1)]), 'numel'),
        (dict(items=[dict(ok, numel=2 ** 31)]), 'numel'),
        (dict(items=[dict(ok, param=0x1002)]), 'aligned'),
        (dict(items=[ok], momentum=0.0, nesterov=1), 'nesterov'),
        (dict(items=[ok], momentum=0.9, dampening=0.1, nesterov=1), 'nesterov'),
    ]
    for kw, word in bad:
        assert call(**kw) == 1, kw                                              # CT_ERR_INVALID
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith('ct_sgd_step') and word in msg, (kw, msg)
        with pytest.raises(_lib.CtdetError):
            _lib.check(1, 'ct_sgd_step')
