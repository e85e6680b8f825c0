"""The fused AdamW step without a device: the NumPy restatement (tests/adamw_ref.py) and torch's CPU AdamW against the
float64 definition, the C ABI surface of ct_adamw_begin / ct_adamw_step (exports, bindings, struct sizes, header text,
host-side argument errors), the args.optimizer switch of utils/solver.py::build_optimizer, and what
ctdet.optim.FusedAdamW decides on the host: its state-dict layout, its refusals and the betas-change error."""
import copy
import ctypes as C
import functools
import math
import os
import pickle
import subprocess
import types

import numpy as np
import pytest
import torch

import adamw_ref
import sgd_ref
from models.RFB_Net_vgg import build_net
from utils import solver

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, 'context-transformer_amd', 'lib', 'libctdet.so')
SYMBOLS = ['ct_adamw_begin_indices_per_launch', 'ct_adamw_begin', 'ct_adamw_tensors_per_launch', 'ct_adamw_step']
F32 = np.float32
BETAS, EPS = (0.9, 0.999), 1e-8


# --------------------------------------------------------------------------------------------------- restatement
@functools.lru_cache(maxsize=None)
def _inputs():
    return adamw_ref.accuracy_inputs()


@pytest.mark.parametrize('lr,wd', adamw_ref.ACCURACY_SETTINGS)
def test_restatement_and_torch_cpu_against_the_definition(lr, wd):
    """40 steps over 20 000 weights of magnitude up to 1, gradients of magnitude 1e-4 .. 1 with exact zeros: the fp32
    restatement and torch's CPU AdamW against the float64 definition (Python-double hyperparameters, beta ** t) under
    the project's rule e <= 2 * e_torch_cpu + ulp(max|p|).  Measured here: the restatement 3.0e-7 .. 1.4e-6, torch
    3.3e-7 .. 1.9e-6 (the larger figures are the settings with weight decay, one more rounding of p per step)."""
    p0, grads = _inputs()
    assert len(grads) == 40 and p0.size == 20000 and any((g == 0).any() for g in grads)
    run = adamw_ref.Run(p0, BETAS, EPS)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([tp], lr=lr, betas=BETAS, eps=EPS, weight_decay=wd)
    for g in grads:
        run.step(g, lr, wd)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
    want, m64, v64, t = adamw_ref.definition(p0, grads, lr, BETAS, EPS, wd)
    assert t == 40 and run.state.step == 40 and run.p.dtype == np.float32
    ok, e_ref, e_torch, bound = sgd_ref.close_to_torch(run.p, tp.detach().numpy(), want)
    print('lr %g wd %g: restatement %.3e  torch %.3e  bound %.3e' % (lr, wd, e_ref, e_torch, bound))
    assert ok, (e_ref, e_torch, bound)
    assert not run.flag, 'a subnormal intermediate on the accuracy inputs'
    # The moments are those of beta' = fp32(beta), which the C ABI takes: 1 - fp32(0.9) is 2.4e-7 of its value away from
    # 0.1 and 1 - fp32(0.999) 1.3e-5 from 0.001, a difference in the hyperparameter, not in the arithmetic.  Against the
    # definition run with beta' the bound is that of tests/ema_ref.py: every step rounds R times (beta * m, (1 - beta) * g,
    # their sum, and the rounding of 1 - beta' itself: R = 4; one more product for g * g: R = 5), each by at most
    # 2^-24 * M with M the largest element, and earlier errors shrink by beta per step: R * 2^-24 * M * min(40, 1 / (1 - beta)).
    m64, v64 = adamw_ref.definition(p0, grads, lr, [adamw_ref.widened(b) for b in BETAS], EPS, wd)[1:3]
    for name, got, ref, rounds, beta in (('exp_avg', run.m, m64, 4, BETAS[0]), ('exp_avg_sq', run.v, v64, 5, BETAS[1])):
        err = float(np.abs(got - ref).max())
        tol = rounds * 2.0 ** -24 * float(np.abs(ref).max()) * min(40.0, 1.0 / (1.0 - beta))
        print('  %s: restatement %.3e from the definition at fp32(beta), bound %.3e' % (name, err, tol))
        assert err <= tol, (name, err, tol)


def test_restatement_of_begin():
    s = adamw_ref.State()
    b1p = b2p = 1.0
    for n in range(1, 6):
        adamw_ref.begin(s, 0.9, 0.999)
        b1p, b2p = b1p * 0.9, b2p * 0.999                       # Python doubles: the same running products
        assert (s.step, s.applied) == (n, 1) and float(s.beta1_pow) == b1p and float(s.beta2_pow) == b2p
        assert s.bc1 == F32(1.0 - b1p) and s.rs2 == np.sqrt(F32(1.0 - b2p))
        assert s.bc1.dtype == np.float32 and s.rs2.dtype == np.float32 and s.beta1_pow.dtype == np.float64
    assert abs(float(s.beta2_pow) - 0.999 ** 5) <= 5e-16
    before = s.record()
    adamw_ref.begin(s, 0.9, 0.999, finite=0)                    # a skipped step: only `applied` changes
    assert s.applied == 0 and s.record()[:3] == before[:3] and s.record()[4:] == before[4:]
    adamw_ref.begin(s, 0.9, 0.999, finite=1)
    assert (s.step, s.applied) == (6, 1)
    s = adamw_ref.State(step=adamw_ref.INT_MAX, beta1_pow=0.0, beta2_pow=0.0)
    adamw_ref.begin(s, 0.9, 0.999)
    assert s.step == adamw_ref.INT_MAX and s.bc1 == F32(1.0)   # saturates
    s = adamw_ref.State(step=0, beta1_pow=123.0, beta2_pow=-4.0)   # not read while step == 0
    adamw_ref.begin(s, 0.5, 0.25)
    assert (float(s.beta1_pow), float(s.beta2_pow)) == (0.5, 0.25)
    assert adamw_ref.loaded(7, BETAS).record()[:3] == \
        (np.float64(float(F32(0.9)) ** 7).view(np.uint64), np.float64(float(F32(0.999)) ** 7).view(np.uint64), 7)


def test_restatement_reports_subnormal_intermediates():
    s = adamw_ref.begin(adamw_ref.State(), 0.9, 0.999)
    z = np.zeros(4, F32)
    g = np.array([1e-30, -1e-30, 1e20, np.inf], F32)            # (om2 * g) * g: exactly zero, 1e37 or inf, no subnormal
    p, m, v, flag = adamw_ref.step(np.ones(4, F32), g, z, z, s, 1e-3, 5e-4, 0.9, 0.999, 1e-8)
    assert not flag and v[0] == 0 and v[1] == 0 and np.isfinite(v[2]) and np.isinf(v[3])
    assert np.isfinite(p[:3]).all() and np.isnan(p[3])
    g = np.array([1e-20, 0.0, 0.0, 0.0], F32)                   # (om2 * g) * g = 1e-43: subnormal
    assert adamw_ref.step(np.ones(4, F32), g, z, z, s, 1e-3, 0.0, 0.9, 0.999, 1e-8)[3]
    out = adamw_ref.step(np.ones(4, F32), g, z, z, s, 1e-3, 0.0, 0.9, 0.999, 1e-8, dtype=np.float64)
    assert out[0].dtype == np.float64 and not out[3]


# --------------------------------------------------------------------------------------------------------- C ABI
def test_library_exports_binds_and_documents_the_entry_points():
    assert os.path.exists(LIB), 'build the library first (context-transformer_amd/build.py)'
    r = subprocess.run(['nm', '-D', '--defined-only', LIB], capture_output=True, text=True)
    assert r.returncode == 0
    from ctdet import _lib, ops
    for sym in SYMBOLS:
        assert ' T %s\n' % sym in r.stdout, sym
        assert sym in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.ct_abi_version() == 1
    assert C.sizeof(_lib.AdamState) == 32 and ops.ADAM_STATE_BYTES == 32 and ops.ADAM_STATE_DTYPE.itemsize == 32
    assert [(f[0], getattr(_lib.AdamState, f[0]).offset) for f in _lib.AdamState._fields_] == \
        [('beta1_pow', 0), ('beta2_pow', 8), ('step', 16), ('applied', 20), ('bc1', 24), ('rs2', 28)]
    assert [(n, ops.ADAM_STATE_DTYPE.fields[n][1]) for n in ops.ADAM_STATE_DTYPE.names] == \
        [(f[0], getattr(_lib.AdamState, f[0]).offset) for f in _lib.AdamState._fields_]
    assert C.sizeof(_lib.AdamwTensor) == 64
    assert [f[0] for f in _lib.AdamwTensor._fields_] == ['param', 'grad', 'exp_avg', 'exp_avg_sq', 'ema', 'state', 'numel',
                                                         'lr', 'weight_decay']
    for sym, nargs, args in (('ct_adamw_begin', 7, None), ('ct_adamw_step', 9, None),
                             ('ct_adamw_begin_indices_per_launch', 0, None), ('ct_adamw_tensors_per_launch', 0, None)):
        fn = getattr(lib, sym)
        assert fn.restype is C.c_int and len(fn.argtypes or []) == nargs, sym
    assert lib.ct_adamw_begin.argtypes[3] is C.c_double and lib.ct_adamw_begin.argtypes[4] is C.c_double
    per, idx = lib.ct_adamw_tensors_per_launch(), lib.ct_adamw_begin_indices_per_launch()
    # six pointers, numel, lr, lr * weight_decay, flags and a prefix sum per tensor, the scalars of the launch: in 4 KiB
    assert 50 <= per <= 63 and per * 64 + (per + 1) * 4 + 48 <= 4096
    assert idx >= 256 and idx * 4 + 40 <= 4096
    assert lib.ct_sgd_tensors_per_launch() == 80 and lib.ct_sgd_ema_tensors_per_launch() == 77      # untouched
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    for text in ('typedef struct ct_adam_state {', 'typedef struct ct_adamw_tensor {',
                 'int ct_adamw_begin_indices_per_launch(void);', 'int ct_adamw_tensors_per_launch(void);',
                 'int ct_adamw_begin(ct_adam_state* states_dev, const int* index_host, int n, double beta1, double beta2,',
                 'int ct_adamw_step(const ct_adamw_tensor* items_host, int n, float beta1, float beta2, float eps, '
                 'float grad_scale,',
                 'm   = beta1 * m + om1 * g', 'v   = beta2 * v + (om2 * g) * g', 'p   = p - a * (m / den)',
                 'ct_adamw_tensors_per_launch() (%d) tensors per' % per,
                 'ct_adamw_begin_indices_per_launch() (%d) per launch' % idx):
        assert text in header, text
    build = open(os.path.join(REPO, 'context-transformer_amd', 'build.py')).read()
    assert "'ct_adamw.hip': ['-ffp-contract=off'," in build


def _lib_or_skip():
    from ctdet import _lib
    try:
        return _lib, _lib.lib()
    except _lib.CtdetError as e:                              # pragma: no cover
        pytest.skip('libctdet cannot be loaded on this box: %s' % e)


def _check(lib, who, call, bad):
    for kw, word in bad:
        assert call(**kw) == 1, kw                                              # CT_ERR_INVALID
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith(who) and word in msg, (kw, msg)


def test_ct_adamw_begin_argument_errors():
    """Host-side checks: they return before anything touches a device (the pointers are made up)."""
    _lib, lib = _lib_or_skip()

    def call(states=0x20000, index=(0, 1, 2), n=None, beta1=0.9, beta2=0.999, clip=None):
        arr = None if index is None else (C.c_int * max(len(index), 1))(*index)
        return lib.ct_adamw_begin(states, arr, (len(index) if index is not None else 3) if n is None else n, beta1, beta2,
                                  clip, None)

    assert call(index=(), n=0) == 0 and call(states=None, index=None, n=0) == 0     # n == 0: valid no-ops
    many = tuple(range(3000))
    _check(lib, 'ct_adamw_begin', call, [
        (dict(n=-1), 'negative'),
        (dict(states=None), 'states_dev is NULL'),
        (dict(states=0x20004), '8-byte'),
        (dict(index=None), 'index_host is NULL'),
        (dict(index=(0, -1, 2)), 'negative'),
        (dict(index=(4, 1, 4)), 'twice'),
        (dict(index=many + (2999,)), 'twice'),
        (dict(index=many[::-1] + (-7,)), 'negative'),
        (dict(beta1=1.0), 'betas'),
        (dict(beta1=-0.1), 'betas'),
        (dict(beta1=math.nan), 'betas'),
        (dict(beta2=1.0), 'betas'),
        (dict(beta2=1.5), 'betas'),
        (dict(beta2=math.nan), 'betas'),
        (dict(clip=0x30002), 'clip'),
    ])


def test_ct_adamw_step_argument_errors():
    _lib, lib = _lib_or_skip()
    T = _lib.AdamwTensor
    ok = dict(param=0x1000, grad=0x2000, exp_avg=0x3000, exp_avg_sq=0x4000, ema=None, state=0x20000, numel=16, lr=0.1,
              weight_decay=0.0)

    def call(items, n=None, beta1=0.9, beta2=0.999, eps=1e-8, clip=None, ema=None):
        arr = (T * max(len(items), 1))(*[T(**it) for it in items])
        return lib.ct_adamw_step(arr, len(items) if n is None else n, beta1, beta2, eps, 1.0, clip, ema, None)

    assert call([], n=0) == 0                                                   # n == 0: valid no-op
    assert call([dict(ok, numel=0)]) == 0 and call([dict(ok, numel=0)], ema=0x50000) == 0
    nothing = dict(param=None, grad=None, exp_avg=None, exp_avg_sq=None, ema=None, state=None, numel=0, lr=0.1,
                   weight_decay=0.0)
    assert call([nothing] * 200) == 0 and call([dict(nothing, ema=0x7)] * 3) == 0      # ... with any pointers, any count
    with_ema = dict(ok, ema=0x5000)
    _check(lib, 'ct_adamw_step', call, [
        (dict(items=[ok], n=-1), 'negative'),
        (dict(items=[dict(ok, param=None)]), 'param'),
        (dict(items=[dict(ok, numel=0), dict(ok, grad=None)]), 'grad'),
        (dict(items=[dict(ok, exp_avg=None)]), 'NULL exp_avg'),
        (dict(items=[dict(ok, exp_avg_sq=None)]), 'NULL exp_avg_sq'),
        (dict(items=[dict(ok, state=None)]), 'NULL state'),
        (dict(items=[dict(ok, state=0x20004)]), '8-byte'),
        (dict(items=[dict(ok, numel=-1)]), 'numel'),
        (dict(items=[dict(ok, numel=2 ** 31)]), 'numel'),
        (dict(items=[dict(ok, param=0x1002)]), 'aligned'),
        (dict(items=[dict(ok, exp_avg_sq=0x4001)]), 'aligned'),
        (dict(items=[with_ema]), 'ema'),                                        # an ema without ema_dev
        (dict(items=[with_ema, ok], ema=0x50000), 'ema'),                       # a mix of NULL and non-NULL
        (dict(items=[dict(with_ema, ema=0x5002)], ema=0x50000), 'aligned'),
        (dict(items=[with_ema], ema=0x50001), 'ema state'),
        (dict(items=[ok], clip=0x30002), 'clip'),
        (dict(items=[ok], eps=-1e-8), 'eps'),
        (dict(items=[ok], eps=math.nan), 'eps'),
        (dict(items=[ok], beta1=1.0), 'betas'),
        (dict(items=[ok], beta1=math.nan), 'betas'),
        (dict(items=[ok], beta2=-0.5), 'betas'),
        (dict(items=[ok], beta2=1.0), 'betas'),
        (dict(items=[], n=0, eps=-1.0), 'eps'),
    ])
    assert lib.ct_adamw_step(None, 3, 0.9, 0.999, 1e-8, 1.0, None, None, None) == 1
    assert 'items is NULL' in lib.ct_last_error_string().decode()


# ---------------------------------------------------------------------------------------------- build_optimizer
def _args(**kw):
    d = dict(method='ours', phase=2, setting='transfer', lr=4e-3, weight_decay=5e-4, momentum=0.9, steps=[30, 50],
             warmup_iter=10)
    d.update(kw)
    return types.SimpleNamespace(**d)


@functools.lru_cache(maxsize=None)
def _net():
    return build_net(_args(), 300, 20)


def _group_view(opt):
    return [(len(g['params']), id(g['params'][0]), g['lr'], g['weight_decay']) for g in opt.param_groups]


def test_build_optimizer_switch(monkeypatch):
    from ctdet.optim import FusedAdamW, FusedSGD
    monkeypatch.delenv('CTDET_SGD_FUSED', raising=False)
    net = _net()
    # the default path: what it returned before there was a switch, with and without the attribute
    sgd = solver.build_optimizer(_args(), net)
    assert type(sgd) is torch.optim.SGD and type(solver.build_optimizer(_args(optimizer='sgd'), net)) is torch.optim.SGD
    assert all(g['momentum'] == 0.9 for g in sgd.param_groups)
    assert type(solver.build_optimizer(_args(optimizer='sgd'), net, fused=True)) is FusedSGD
    for bad in ('adam', 'AdamW', '', None):
        with pytest.raises(ValueError, match='optimizer'):
            solver.build_optimizer(_args(optimizer=bad), net)
    # 'adamw' without and with `fused`: the same per-tensor groups as the SGD path
    plain = solver.build_optimizer(_args(optimizer='adamw'), net)
    fused = solver.build_optimizer(_args(optimizer='adamw'), net, fused=True)
    assert type(plain) is torch.optim.AdamW and type(fused) is FusedAdamW
    assert _group_view(plain) == _group_view(sgd) == _group_view(fused)
    assert {g['lr'] for g in fused.param_groups} == {4e-3, 4e-3 * 0.1, 4e-3 * 0.5}
    for opt in (plain, fused):
        assert all(g['betas'] == (0.9, 0.999) and g['eps'] == 1e-8 and g['weight_decay'] == 5e-4 for g in opt.param_groups)
    for opt in (solver.build_optimizer(_args(optimizer='adamw', betas=[0.8, 0.99], eps=1e-6), net),
                solver.build_optimizer(_args(optimizer='adamw', betas=(0.8, 0.99), eps=1e-6), net, fused=True)):
        assert all(g['betas'] == (0.8, 0.99) and g['eps'] == 1e-6 for g in opt.param_groups)
    monkeypatch.setenv('CTDET_SGD_FUSED', '1')
    assert type(solver.build_optimizer(_args(optimizer='adamw'), net)) is FusedAdamW
    monkeypatch.setenv('CTDET_SGD_FUSED', '0')
    # max_grad_norm and ema_decay still need the fused class
    with pytest.raises(ValueError, match='max_grad_norm'):
        solver.build_optimizer(_args(optimizer='adamw', max_grad_norm=1.0), net)
    with pytest.raises(ValueError, match='ema_decay'):
        solver.build_optimizer(_args(optimizer='adamw', ema_decay=0.9998), net, fused=False)
    clipped = solver.build_optimizer(_args(optimizer='adamw', max_grad_norm=math.inf), net, fused=True)
    assert type(clipped) is FusedAdamW and clipped.max_grad_norm == math.inf and clipped.ema is None
    from ctdet._lib import CtdetError
    with pytest.raises(CtdetError, match='no CPU path'):        # the average is built first: the model is on the CPU
        solver.build_optimizer(_args(optimizer='adamw', ema_decay=0.9998), net, fused=True)


# --------------------------------------------------------------------------------------------------- FusedAdamW
def _stepped_torch(sizes, steps, **kw):
    gen = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(n, generator=gen)) for n in sizes]
    opt = torch.optim.AdamW([dict(params=ps[:1], lr=2e-3), dict(params=ps[1:])], **kw)
    for it in range(steps):
        for i, p in enumerate(ps):
            p.grad = None if (i == 2 and it == 0) else torch.randn(p.shape, generator=gen)
        opt.step()
    return ps, opt


def _same_state_dict(a, b):
    assert a['param_groups'] == b['param_groups'] and [list(g) for g in a['param_groups']] == \
        [list(g) for g in b['param_groups']]
    assert list(a['state']) == list(b['state'])
    for k in a['state']:
        assert list(a['state'][k]) == list(b['state'][k]) == ['step', 'exp_avg', 'exp_avg_sq'], k
        for name in a['state'][k]:
            x, y = a['state'][k][name], b['state'][k][name]
            assert type(x) is type(y) and x.dtype == y.dtype and x.device == y.device and x.shape == y.shape, (k, name)
            assert torch.equal(x, y), (k, name)
    return True


def test_state_dict_layout_is_torchs():
    from ctdet.optim import FusedAdamW
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (3, 2, 5)]
    fresh, ref = FusedAdamW(ps, 2e-3), torch.optim.AdamW(ps, 2e-3)
    assert fresh.defaults == ref.defaults and list(fresh.defaults) == list(ref.defaults)
    assert _same_state_dict(fresh.state_dict(), ref.state_dict()) and fresh.state_dict()['state'] == {}
    ref.load_state_dict(fresh.state_dict())
    assert fresh.max_grad_norm is None and fresh.ema is None and fresh.grad_scale == 1.0 and fresh.clip_info() is None
    assert all('max_grad_norm' not in g and 'ema' not in g for g in fresh.param_groups)
    # torch -> fused -> state_dict(): torch's own, steps included (the third tensor has taken one step fewer)
    tps, topt = _stepped_torch((3, 2, 5), 4, lr=1e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1)
    want = topt.state_dict()
    assert [int(want['state'][k]['step']) for k in (0, 1, 2)] == [4, 4, 3]
    fused = FusedAdamW([dict(params=ps[:1]), dict(params=ps[1:])], 5e-2)
    fused.load_state_dict(copy.deepcopy(want))
    assert _same_state_dict(fused.state_dict(), want)
    assert [g['lr'] for g in fused.param_groups] == [2e-3, 1e-3]
    # ... and back into a fresh torch optimizer
    back = torch.optim.AdamW([dict(params=ps[:1]), dict(params=ps[1:])], 7.0)
    back.load_state_dict(fused.state_dict())
    assert _same_state_dict(back.state_dict(), want)
    # pickling and deepcopy carry the step counts, which otherwise live in the records
    for clone in (pickle.loads(pickle.dumps(fused)), copy.deepcopy(fused)):
        assert type(clone) is FusedAdamW and _same_state_dict(clone.state_dict(), want)
        assert clone.max_grad_norm is None and clone.ema is None and clone.grad_scale == 1.0
    with pytest.raises(ValueError, match='step count'):
        bad = copy.deepcopy(want)
        bad['state'][1]['step'] = torch.tensor(-2.0)
        fused.load_state_dict(bad)


def test_refusals():
    from ctdet._lib import CtdetError
    from ctdet.optim import FusedAdamW
    ps = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(foreach=True), dict(capturable=True), dict(differentiable=True),
               dict(fused=True)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            FusedAdamW(ps, **kw)
    ok = FusedAdamW(ps, amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(betas=(math.nan, 0.9)),
               dict(weight_decay=-1.0), dict(lr=torch.tensor(1e-3)), dict(max_grad_norm=0.0), dict(max_grad_norm='1')):
        with pytest.raises(ValueError):
            FusedAdamW(ps, **kw)
    with pytest.raises(TypeError):
        FusedAdamW(ps, ema='ema')
    with pytest.raises(TypeError):                              # positional amsgrad is not part of the signature
        FusedAdamW(ps, 1e-3, (0.9, 0.999), 1e-8, 1e-2, True)
    ok.step()                                                   # no gradients: nothing to do, no device needed
    assert ok.last_calls == 0 and ok.state_dict()['state'] == {}
    ps[0].grad = torch.ones(3)
    with pytest.raises(CtdetError, match='no CPU fallback'):    # a CPU parameter: an error, not a torch path
        ok.step()
    assert torch.equal(ps[0].detach(), torch.zeros(3)) and ok.state_dict()['state'] == {}
    for key in ('amsgrad', 'maximize', 'foreach', 'capturable', 'differentiable', 'fused'):
        ok.param_groups[0][key] = True                          # a group key set behind the constructor's back
        with pytest.raises(ValueError, match=key):
            ok.step()
        ok.param_groups[0][key] = ok.defaults[key]
    ps[0].grad = torch.ones(3).to_sparse()
    with pytest.raises(CtdetError, match='sparse'):
        ok.step()
    with pytest.raises(ValueError, match='decoupled'):
        sd = torch.optim.Adam(ps, weight_decay=0.1).state_dict()
        sd['param_groups'][0]['decoupled_weight_decay'] = False
        ok.load_state_dict(sd)


def test_betas_cannot_change_after_a_step():
    from ctdet._lib import CtdetError
    from ctdet.optim import FusedAdamW
    tps, topt = _stepped_torch((3, 2, 5), 2, lr=1e-3)
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (3, 2, 5)]
    opt = FusedAdamW([dict(params=ps[:1]), dict(params=ps[1:])], 1e-3)
    opt.load_state_dict(topt.state_dict())
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.param_groups[1]['betas'] = (0.9, 0.99)
    with pytest.raises(ValueError, match='betas changed'):      # host-side, before the CPU parameters are looked at
        opt.step()
    opt.param_groups[1]['betas'] = (0.9, 0.999)
    with pytest.raises(CtdetError):                             # the same betas: the step goes on, to the device
        opt.step()
    # a tensor that has not stepped yet may still change its betas
    fresh = FusedAdamW(ps, 1e-3)
    fresh.param_groups[0]['betas'] = (0.5, 0.5)
    fresh.load_state_dict(fresh.state_dict())
    assert fresh.param_groups[0]['betas'] == (0.5, 0.5)
