"""Gradient-norm clipping and the non-finite guard without a device: the restatement of ct_grad_norm_clip
(tests/clip_ref.py) against torch.nn.utils.clip_grad_norm_ on the CPU, the C ABI surface (exports, bindings, struct
sizes, header text, host-side argument errors), FusedSGD(max_grad_norm=...)'s refusals and state_dict() layout, and the
args.max_grad_norm switch of utils/solver.py::build_optimizer."""
import ctypes as C
import math
import os
import pickle
import subprocess
import types

import numpy as np
import pytest
import torch

import clip_ref
import sgd_ref
from models.RFB_Net_vgg import build_net
from utils import solver

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, 'context-transformer_amd', 'lib', 'libctdet.so')
SYMBOLS = ['ct_grad_norm_tensors_per_launch', 'ct_grad_norm_workspace_bytes', 'ct_grad_norm_clip', 'ct_sgd_step_clipped']


# --------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('max_ratio', [0.5, 10.0])
def test_restatement_against_torch_clip_grad_norm(dtype, max_ratio):
    """Five fp32 gradient tensors, the norm and the coefficient of the restatement against what clip_grad_norm_
    returns and does on the CPU, computing in fp32 and in fp64 (on the same fp32 values).  Tolerances: torch in fp64
    sums ~1e5 positive terms within 1e5 * 2^-53 of the exact sum, so the two fp64 norms agree to 1e-10 relative; torch
    in fp32 rounds every partial sum to fp32 (relative 2^-24 each, at most log2-many of them in its blocked sums plus
    the final sqrt): 1e-5 relative.  The scaled gradients follow with one more fp32 rounding of the product."""
    rng = np.random.RandomState(31)
    grads = [(rng.randn(n) * s).astype(np.float32) for n, s in ((1, 1.0), (1000, 0.1), (33333, 1e-3), (70001, 3.0), (5, 1e2))]
    n64 = clip_ref.norm64(grads)
    direct = math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads))
    assert abs(n64 - direct) <= 1e-12 * direct
    max_norm = max_ratio * n64
    ps = [torch.nn.Parameter(torch.zeros(g.size, dtype=dtype)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(g.copy()).to(dtype)
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    rel = 1e-10 if dtype == torch.float64 else 1e-5
    print('norm: restatement %.17g  torch(%s) %.17g  rel %.3e' % (n64, dtype, total, abs(total - n64) / n64))
    assert abs(total - n64) <= rel * n64
    n32 = clip_ref.norm32(grads)
    assert n32.dtype == np.float32 and abs(float(n32) - n64) <= 0.5 * sgd_ref.ulp(n64) * (1 + 1e-9)
    c, finite = clip_ref.coef(n32, max_norm)
    assert finite == 1 and c.dtype == np.float32
    if max_ratio > 1:
        assert c == np.float32(1.0)
    else:
        assert abs(float(c) - 0.5) < 1e-6
    for p, g in zip(ps, grads):
        want = g.astype(np.float64) * float(c)
        got = p.grad.double().numpy()
        # the restatement's coef is an fp32 number (two roundings, 2^-24 each), torch's is of `dtype`
        assert np.abs(got - want).max() <= (2 * rel + 2.0 ** -23) * np.abs(want).max() + 1e-45


def test_restatement_special_values():
    f32 = np.float32
    assert clip_ref.norm64([]) == 0.0 and clip_ref.norm64([np.zeros(0, f32)]) == 0.0
    assert clip_ref.coef(f32(0.0), 1.0) == (f32(1.0), 1)
    assert clip_ref.coef(f32(3.0), math.inf) == (f32(1.0), 1)                   # guard only
    assert clip_ref.coef(f32(np.inf), 1.0) == (f32(0.0), 0)
    assert clip_ref.coef(f32(np.nan), math.inf) == (f32(0.0), 0)
    for bad in (np.inf, -np.inf, np.nan):
        assert not np.isfinite(clip_ref.norm32([np.ones(7, f32), np.array([1.0, bad], f32)]))
    big = np.full(4, 3e38, f32)                                                  # squares overflow fp32, not fp64
    assert clip_ref.norm32([big]) == f32(np.inf)                                 # 6e38: the NORM overflows fp32
    assert clip_ref.norm32([big[:1]]) == f32(3e38) and clip_ref.norm32([big], 2.0 ** -10) == f32(6e38 / 1024)
    assert clip_ref.norm64([np.full(4, 1e38, f32)]) == 2.0 * float(f32(1e38))
    assert clip_ref.norm64([np.full(4, 1e-30, f32)]) == pytest.approx(2.0 * float(f32(1e-30)), rel=1e-15)
    assert clip_ref.norm64([np.full(4, 1.0, f32)], -0.125) == 0.25                # |grad_scale|
    c, _ = clip_ref.coef(f32(4.0), 2.0)
    assert c == f32(2.0) / (f32(4.0) + f32(1e-6))
    assert clip_ref.ulps_apart(f32(1.0), np.nextafter(f32(1.0), f32(2.0))) == 1


# --------------------------------------------------------------------------------------------------------- C ABI
def test_library_exports_binds_and_documents_the_entry_points():
    assert os.path.exists(LIB), 'build the library first (context-transformer_amd/build.py)'
    r = subprocess.run(['nm', '-D', '--defined-only', LIB], capture_output=True, text=True)
    assert r.returncode == 0
    for sym in SYMBOLS:
        assert ' T %s\n' % sym in r.stdout, sym
    from ctdet import _lib
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.ct_abi_version() == 1
    assert C.sizeof(_lib.GradTensor) == 16 and C.sizeof(_lib.ClipState) == 16
    assert [f[0] for f in _lib.ClipState._fields_] == ['norm', 'coef', 'finite', 'nonfinite']
    assert lib.ct_grad_norm_clip.restype is C.c_int and len(lib.ct_grad_norm_clip.argtypes) == 8
    assert lib.ct_sgd_step_clipped.restype is C.c_int and len(lib.ct_sgd_step_clipped.argtypes) == 8
    assert lib.ct_grad_norm_workspace_bytes.restype is C.c_size_t
    per = lib.ct_grad_norm_tensors_per_launch()
    assert per >= 1 and per * 12 + (per + 1) * 4 <= 4096            # pointer + numel + prefix sum per tensor, in 4 KiB
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    for text in ('typedef struct ct_grad_tensor {', 'typedef struct ct_clip_state {',
                 'int ct_grad_norm_tensors_per_launch(void);',
                 'size_t ct_grad_norm_workspace_bytes(const ct_grad_tensor* items_host, int n);',
                 'int ct_grad_norm_clip(const ct_grad_tensor* items_host, int n, float grad_scale, float max_norm,',
                 'int ct_sgd_step_clipped(const ct_sgd_tensor* items_host, int n, float momentum, float dampening, int nesterov,',
                 'norm   = (float)( sqrt(S) * (double)|grad_scale| )',
                 'coef   = finite ? min(1.0f, max_norm / (norm + 1e-6f)) : 0.0f',
                 'A norm\n * that overflows fp32 counts as non-finite',
                 'only\n *       when dampening != 0'):
        assert text in header, text


def _lib_or_skip():
    from ctdet import _lib
    try:
        return _lib, _lib.lib()
    except _lib.CtdetError as e:                              # pragma: no cover
        pytest.skip('libctdet cannot be loaded on this box: %s' % e)


def _grad_items(_lib, items):
    T = _lib.GradTensor
    return (T * max(len(items), 1))(*[T(g, n) for g, n in items])


def test_workspace_bytes_grows_with_the_table():
    _lib, lib = _lib_or_skip()

    def ws(items):
        return lib.ct_grad_norm_workspace_bytes(_grad_items(_lib, items), len(items))

    one = ws([(0x1000, 1)])
    assert one >= 8 and one % 8 == 0
    assert ws([]) >= 8 and ws([(None, 0)]) == ws([])            # the finish needs no slot, the entry a valid pointer
    assert ws([(0x1000, 1)] * 2) == 2 * one                     # one slot per chunk, one chunk per small tensor
    assert ws([(0x1000, 1)] * 500) == 500 * one                 # beyond one launch's table
    sizes = [8192 * k for k in (1, 2, 5, 100)]
    got = [ws([(0x1000, n)]) for n in sizes]
    assert got == sorted(got) and len(set(got)) == 4 and got[3] == 100 * got[0]
    assert ws([(0x1004, 8192)]) == 2 * ws([(0x1000, 8192)])     # chunks are counted from the 16-byte line
    assert ws([(0x1000, 8192), (None, 0), (0x2000, 8193)]) == ws([(0x1000, 8192)]) + ws([(0x2000, 8193)])
    assert ws([(None, 5)]) == 0 and ws([(0x1000, -1)]) == 0     # a table the call refuses


def test_ct_grad_norm_clip_argument_errors():
    """Host-side checks: they return before anything touches a device."""
    _lib, lib = _lib_or_skip()
    ok = [(0x1000, 16), (None, 0), (0x2004, 9000)]
    need = lib.ct_grad_norm_workspace_bytes(_grad_items(_lib, ok), len(ok))
    assert need == 3 * 8

    def call(items=ok, n=None, max_norm=1.0, ws=0x10000, ws_bytes=None, state=0x20000):
        return lib.ct_grad_norm_clip(_grad_items(_lib, items), len(items) if n is None else n, 1.0, max_norm, ws,
                                     need if ws_bytes is None else ws_bytes, state, None)

    bad = [
        (dict(n=-1), 'negative'),
        (dict(items=[(None, 4)]), 'NULL grad'),
        (dict(items=[(0x1000, 4), (0x1002, 4)]), 'aligned'),
        (dict(items=[(0x1000, -1)]), 'numel'),
        (dict(items=[(0x1000, 2 ** 31)]), 'numel'),
        (dict(max_norm=0.0), 'max_norm'),
        (dict(max_norm=-1.0), 'max_norm'),
        (dict(max_norm=math.nan), 'max_norm'),
        (dict(max_norm=-math.inf), 'max_norm'),
        (dict(state=None), 'state_dev'),
        (dict(ws=None), 'workspace'),
        (dict(ws_bytes=need - 1), 'workspace'),
        (dict(ws_bytes=0), 'workspace'),
        (dict(items=[], ws=None), 'workspace'),
    ]
    for kw, word in bad:
        assert call(**kw) == 1, kw                                              # CT_ERR_INVALID
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith('ct_grad_norm_clip') and word in msg, (kw, msg)
    assert lib.ct_grad_norm_clip(None, 3, 1.0, 1.0, 0x10000, 64, 0x20000, None) == 1
    assert 'items is NULL' in lib.ct_last_error_string().decode()


def test_ct_sgd_step_clipped_argument_errors():
    """The argument errors of ct_sgd_step, and a NULL state."""
    _lib, lib = _lib_or_skip()
    T = _lib.SgdTensor
    ok = dict(param=0x1000, grad=0x2000, momentum_buf=0x3000, numel=16, lr=0.1, weight_decay=0.0, first_step=1)

    def call(items, n=None, momentum=0.9, dampening=0.0, nesterov=0, state=0x20000):
        arr = (T * max(len(items), 1))(*[T(**it) for it in items])
        return lib.ct_sgd_step_clipped(arr, len(items) if n is None else n, momentum, dampening, nesterov, 1.0, state,
                                       None)

    assert call([], n=0) == 0                                                   # n == 0: valid no-op
    assert call([dict(ok, numel=0)]) == 0                                       # numel == 0: valid no-op
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
        (dict(items=[ok], state=None), 'state_dev'),
        (dict(items=[], n=0, state=None), 'state_dev'),
    ]
    for kw, word in bad:
        assert call(**kw) == 1, kw
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith('ct_sgd_step_clipped') and word in msg, (kw, msg)


# ------------------------------------------------------------------------------------------------------ FusedSGD
def test_fused_sgd_max_grad_norm_validation_and_layout():
    from ctdet._lib import CtdetError
    from ctdet.optim import FusedSGD
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))]
    for bad in (0, 0.0, -1, -1.0, math.nan, -math.inf, '1.0', torch.tensor(1.0), True):
        with pytest.raises(ValueError):
            FusedSGD(ps, 0.1, momentum=0.9, max_grad_norm=bad)
    plain = FusedSGD(ps, 0.1, momentum=0.9)
    assert plain.max_grad_norm is None and plain.clip_state is None and plain.clip_info() is None
    for good in (1, 2.5, math.inf):
        opt = FusedSGD(ps, 0.1, momentum=0.9, max_grad_norm=good)
        assert opt.max_grad_norm == float(good) and opt.clip_state is None
        # an attribute, not a key: defaults, groups and the state dict are what they are without it
        assert opt.defaults == plain.defaults
        assert opt.state_dict() == plain.state_dict()
        assert all('max_grad_norm' not in g for g in opt.param_groups)
    ref = torch.optim.SGD(ps, 0.1, momentum=0.9)
    assert opt.state_dict()['param_groups'] == ref.state_dict()['param_groups']
    # __setstate__ defaults the option to None (an optimizer pickled before the option existed)
    old = pickle.loads(pickle.dumps(plain))
    for k in ('max_grad_norm', 'clip_state', '_clip_workspace'):
        old.__dict__.pop(k, None)
    old.__setstate__(old.__getstate__())
    assert old.max_grad_norm is None and old.clip_state is None and old.clip_info() is None
    # no gradients: nothing to launch, with or without the option
    opt.step()
    assert opt.last_calls == 0 and opt.clip_state is None
    # a CPU parameter stays an error, and nothing is written
    before = ps[0].detach().clone()
    ps[0].grad = torch.ones(3)
    with pytest.raises(CtdetError):
        opt.step()
    assert torch.equal(ps[0].detach(), before) and 'momentum_buffer' not in opt.state.get(ps[0], {})
    # a value set later is checked when it is used
    opt.max_grad_norm = -2.0
    with pytest.raises(ValueError):
        opt.step()


def _args(**kw):
    d = dict(method='ours', phase=2, setting='transfer', lr=4e-3, weight_decay=5e-4, momentum=0.9, steps=[30, 50],
             warmup_iter=10)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_build_optimizer_passes_max_grad_norm_on(monkeypatch):
    from ctdet.optim import FusedSGD
    monkeypatch.delenv('CTDET_SGD_FUSED', raising=False)
    net = build_net(_args(), 300, 20)
    # without the attribute (or with None): unchanged
    assert type(solver.build_optimizer(_args(), net)) is torch.optim.SGD
    assert type(solver.build_optimizer(_args(max_grad_norm=None), net)) is torch.optim.SGD
    plain = solver.build_optimizer(_args(), net, fused=True)
    assert type(plain) is FusedSGD and plain.max_grad_norm is None
    opt = solver.build_optimizer(_args(max_grad_norm=10.0), net, fused=True)
    assert type(opt) is FusedSGD and opt.max_grad_norm == 10.0
    assert opt.state_dict() == plain.state_dict()
    assert [g['lr'] for g in opt.param_groups] == [g['lr'] for g in plain.param_groups]
    monkeypatch.setenv('CTDET_SGD_FUSED', '1')
    assert solver.build_optimizer(_args(max_grad_norm=math.inf), net).max_grad_norm == math.inf
    # a value without the fused optimizer: an error, no silent torch path
    monkeypatch.setenv('CTDET_SGD_FUSED', '0')
    with pytest.raises(ValueError, match='max_grad_norm'):
        solver.build_optimizer(_args(max_grad_norm=10.0), net)
    with pytest.raises(ValueError, match='max_grad_norm'):
        solver.build_optimizer(_args(max_grad_norm=10.0), net, fused=False)
    with pytest.raises(ValueError):
        solver.build_optimizer(_args(max_grad_norm=0.0), net, fused=True)
