"""The weight average without a device: the C ABI surface of ct_ema_begin, ct_sgd_step_ema, ct_ema_update and
ct_tensor_swap (exports, bindings, struct sizes, header text, host-side argument errors), the refusals of WeightEMA,
FusedSGD.attach_ema and the args.ema_decay switch of utils/solver.py::build_optimizer, FusedSGD.state_dict()'s layout
with an average attached, and a rehearsal of the accuracy tolerance of tests/test_gpu_ema.py on the restatement
(tests/ema_ref.py)."""
import ctypes as C
import math
import os
import pickle
import subprocess
import types

import numpy as np
import pytest
import torch

import ema_ref
from models.RFB_Net_vgg import build_net
from utils import solver

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, 'context-transformer_amd', 'lib', 'libctdet.so')
SYMBOLS = ['ct_ema_begin', 'ct_sgd_ema_tensors_per_launch', 'ct_sgd_step_ema', 'ct_ema_update', 'ct_tensor_swap']
F32 = np.float32


# --------------------------------------------------------------------------------------------------- restatement
def test_restatement_schedule_and_special_values():
    s = ema_ref.State()
    want = [F32(1 + n) / F32(10 + n) for n in range(6)]
    for n in range(6):
        ema_ref.begin(s, 0.9998, 10.0)
        assert s.updates == n + 1 and s.applied == 1
        assert s.decay == want[n] and s.decay.dtype == np.float32
        assert s.one_minus == F32(1.0) - want[n]
    assert want[0] == F32(0.1)
    s = ema_ref.State(updates=10 ** 6)                          # past the warm-up: the constant decay
    ema_ref.begin(s, 0.9998, 10.0)
    assert s.decay == F32(0.9998) and s.updates == 10 ** 6 + 1
    s = ema_ref.State()
    ema_ref.begin(s, 0.5, 0.0)                                  # warmup 0: constant from the first update
    assert s.decay == F32(0.5) and s.one_minus == F32(0.5)
    ema_ref.begin(s, 0.5, 1.0)                                  # warmup 1: (1 + n) / (1 + n) = 1 never wins
    assert s.decay == F32(0.5) and s.updates == 2
    before = (s.updates, s.decay, s.one_minus)
    ema_ref.begin(s, 0.25, 10.0, finite=0)                      # a skipped step: only `applied` changes
    assert (s.updates, s.decay, s.one_minus) == before and s.applied == 0
    e = np.arange(4, dtype=F32)
    assert ema_ref.update(e, e + 1, s) is e                     # ... and the average stays
    ema_ref.begin(s, 0.25, 10.0, finite=1)
    assert s.applied == 1 and s.updates == 3 and s.decay == F32(3.0) / F32(12.0)
    s = ema_ref.State(updates=ema_ref.INT_MAX)
    ema_ref.begin(s, 0.9, 10.0)
    assert s.updates == ema_ref.INT_MAX and s.decay == F32(0.9)  # saturates
    s = ema_ref.State()
    ema_ref.begin(s, 0.0, 0.0)                                  # decay 0: the average IS the source
    x = np.array([1.5, -0.0, 3e38, 1e-45], F32)
    assert np.array_equal(ema_ref.update(np.ones(4, F32), x, s).view(np.uint32) & 0x7fffffff,
                          x.view(np.uint32) & 0x7fffffff)
    out = ema_ref.update(np.ones(3, F32), np.zeros(3, F32), ema_ref.begin(ema_ref.State(), 0.75, 0.0), np.float64)
    assert out.dtype == np.float64 and np.all(out == 0.75)


@pytest.mark.parametrize('decay', [0.9, 0.9998])
def test_restatement_in_fp32_stays_inside_the_fp64_bound(decay):
    """The tolerance of tests/test_gpu_ema.py::test_accuracy rehearsed on the CPU: 50 updates in float32 against the
    same updates in float64 with the fp32 d and (1 - d); warmup 0, so that `decay` is the decay of every update (the
    warm-up of 10 would stay below 0.9 for all 50).  Three roundings per step, each at most 2^-24 * M (half an
    ulp of a value of magnitude <= M), contracted by d per step: 3 * 2^-24 * M * min(50, 1 / (1 - decay))."""
    start, seq = ema_ref.accuracy_inputs()
    assert len(seq) == 50 and 1e-3 > np.abs(start).min() and np.abs(start).max() > 1e2
    e32, _ = ema_ref.accuracy_run(start, seq, decay, 0.0, np.float32)
    e64, m = ema_ref.accuracy_run(start, seq, decay, 0.0, np.float64)
    assert e32.dtype == np.float32 and e64.dtype == np.float64
    err = float(np.abs(e32.astype(np.float64) - e64).max())
    tol = ema_ref.bound(decay, 50, m)
    print('decay %g: max|fp32 - fp64| %.3e, bound %.3e (%.3f of it), M %.3e' % (decay, err, tol, err / tol, m))
    assert tol == 3 * 2.0 ** -24 * m * min(50, 1 / (1 - decay))
    assert 0 < err <= tol


# --------------------------------------------------------------------------------------------------------- C ABI
def test_library_exports_binds_and_documents_the_entry_points():
    assert os.path.exists(LIB), 'build the library first (context-transformer_amd/build.py)'
    r = subprocess.run(['nm', '-D', '--defined-only', LIB], capture_output=True, text=True)
    assert r.returncode == 0
    from ctdet import _lib
    for sym in SYMBOLS:
        assert ' T %s\n' % sym in r.stdout, sym
        assert sym in _lib.SIGNATURES
    lib = _lib.lib()
    assert C.sizeof(_lib.EmaState) == 16
    assert [f[0] for f in _lib.EmaState._fields_] == ['updates', 'decay', 'one_minus', 'applied']
    assert C.sizeof(_lib.EmaTensor) == 24 and C.sizeof(_lib.SwapTensor) == 24
    assert [f[0] for f in _lib.SgdEmaTensor._fields_] == [f[0] for f in _lib.SgdTensor._fields_] + ['ema']
    assert [getattr(_lib.SgdEmaTensor, f[0]).offset for f in _lib.SgdTensor._fields_] == \
        [getattr(_lib.SgdTensor, f[0]).offset for f in _lib.SgdTensor._fields_]
    assert C.sizeof(_lib.SgdEmaTensor) == 56 and _lib.SgdEmaTensor.ema.offset == 48
    from ctdet import ops
    assert ops.EMA_STATE_BYTES == 16
    for sym, nargs in (('ct_ema_begin', 5), ('ct_sgd_step_ema', 9), ('ct_ema_update', 4), ('ct_tensor_swap', 3),
                       ('ct_sgd_ema_tensors_per_launch', 0)):
        fn = getattr(lib, sym)
        assert fn.restype is C.c_int and len(fn.argtypes or []) == nargs, sym
    per = lib.ct_sgd_ema_tensors_per_launch()
    # four pointers, numel, lr, weight_decay, flags and a prefix sum per tensor, the scalars of the launch: in 4 KiB
    assert 70 <= per <= 77 and per * 48 + (per + 1) * 4 + 40 <= 4096
    assert lib.ct_sgd_tensors_per_launch() == 80                # the plain step keeps its table
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    for text in ('typedef struct ct_ema_state {', 'typedef struct ct_sgd_ema_tensor {', 'typedef struct ct_ema_tensor {',
                 'typedef struct ct_swap_tensor {',
                 'int ct_ema_begin(ct_ema_state* state_dev, float decay, float warmup, const ct_clip_state* clip_dev_or_null,',
                 'int ct_sgd_ema_tensors_per_launch(void);',
                 'int ct_sgd_step_ema(const ct_sgd_ema_tensor* items_host, int n, float momentum, float dampening, int nesterov,',
                 'int ct_ema_update(const ct_ema_tensor* items_host, int n, const ct_ema_state* ema_dev, ct_stream_t stream);',
                 'int ct_tensor_swap(const ct_swap_tensor* items_host, int n, ct_stream_t stream);',
                 'applied = clip ? clip->finite : 1',
                 'a   = 1.0f + nf', 'b   = warmup + nf', 'q   = a / b',
                 'd   = (warmup == 0) ? decay : min(decay, q)', 'om  = 1.0f - d',
                 't   = d * ema', 'u   = om * p', 'ema = t + u',
                 'writes nothing to ema'):
        assert text in header, text
    assert '(%d) tensors per launch, no limit on n' % per in header
    build = open(os.path.join(REPO, 'context-transformer_amd', 'build.py')).read()
    assert "'ct_ema.hip': ['-ffp-contract=off']," in build


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


def test_ct_ema_begin_argument_errors():
    """Host-side checks: they return before anything touches a device (the pointers are made up)."""
    _lib, lib = _lib_or_skip()

    def call(state=0x20000, decay=0.9998, warmup=10.0, clip=None):
        return lib.ct_ema_begin(state, decay, warmup, clip, None)

    _check(lib, 'ct_ema_begin', call, [
        (dict(state=None), 'NULL'),
        (dict(state=0x20002), 'aligned'),
        (dict(decay=1.0), 'decay'),
        (dict(decay=-0.1), 'decay'),
        (dict(decay=1.5), 'decay'),
        (dict(decay=math.nan), 'decay'),
        (dict(warmup=0.5), 'warmup'),
        (dict(warmup=-1.0), 'warmup'),
        (dict(warmup=math.nan), 'warmup'),
        (dict(warmup=math.inf), 'warmup'),
        (dict(clip=0x30001), 'clip'),
    ])


def test_ct_sgd_step_ema_argument_errors():
    _lib, lib = _lib_or_skip()
    T = _lib.SgdEmaTensor
    ok = dict(param=0x1000, grad=0x2000, momentum_buf=0x3000, numel=16, lr=0.1, weight_decay=0.0, first_step=1,
              ema=0x4000)

    def call(items, n=None, momentum=0.9, dampening=0.0, nesterov=0, clip=None, state=0x20000):
        arr = (T * max(len(items), 1))(*[T(**it) for it in items])
        return lib.ct_sgd_step_ema(arr, len(items) if n is None else n, momentum, dampening, nesterov, 1.0, clip, state,
                                   None)

    assert call([], n=0) == 0                                                   # n == 0: valid no-op
    assert call([dict(ok, numel=0)]) == 0                                       # numel == 0: valid no-op
    assert call([dict(param=None, grad=None, momentum_buf=None, numel=0, lr=0.1, weight_decay=0.0, first_step=0,
                      ema=None)] * 200) == 0                                    # ... with any pointers, any count
    _check(lib, 'ct_sgd_step_ema', call, [
        (dict(items=[ok], n=-1), 'negative'),
        (dict(items=[dict(ok, param=None)]), 'param'),
        (dict(items=[dict(ok, numel=0), dict(ok, grad=None)]), 'grad'),
        (dict(items=[dict(ok, momentum_buf=None)]), 'momentum_buf'),
        (dict(items=[dict(ok, ema=None)]), 'ema'),
        (dict(items=[dict(ok, numel=-1)]), 'numel'),
        (dict(items=[dict(ok, numel=2 ** 31)]), 'numel'),
        (dict(items=[dict(ok, param=0x1002)]), 'aligned'),
        (dict(items=[dict(ok, ema=0x4001)]), 'aligned'),
        (dict(items=[ok], momentum=0.0, nesterov=1), 'nesterov'),
        (dict(items=[ok], momentum=0.9, dampening=0.1, nesterov=1), 'nesterov'),
        (dict(items=[ok], state=None), 'ema state'),
        (dict(items=[ok], state=0x20001), 'ema state'),
        (dict(items=[], n=0, state=None), 'ema state'),
        (dict(items=[ok], clip=0x30002), 'clip'),
    ])
    assert lib.ct_sgd_step_ema(None, 3, 0.9, 0.0, 0, 1.0, None, 0x20000, None) == 1
    assert 'items is NULL' in lib.ct_last_error_string().decode()


def test_ct_ema_update_and_ct_tensor_swap_argument_errors():
    _lib, lib = _lib_or_skip()
    E, S = _lib.EmaTensor, _lib.SwapTensor

    def upd(items, n=None, state=0x20000):
        arr = (E * max(len(items), 1))(*[E(*it) for it in items])
        return lib.ct_ema_update(arr, len(items) if n is None else n, state, None)

    def swap(items, n=None):
        arr = (S * max(len(items), 1))(*[S(*it) for it in items])
        return lib.ct_tensor_swap(arr, len(items) if n is None else n, None)

    assert upd([], n=0) == 0 and upd([(None, None, 0), (0x1001, 0x7, 0)]) == 0
    assert swap([], n=0) == 0 and swap([(None, None, 0), (0x1000, 0x1000, 0)] * 150) == 0
    _check(lib, 'ct_ema_update', upd, [
        (dict(items=[(0x1000, 0x2000, 4)], n=-1), 'negative'),
        (dict(items=[(None, 0x2000, 4)]), 'NULL ema'),
        (dict(items=[(0x1000, 0x2000, 0), (0x1000, None, 4)]), 'NULL src'),
        (dict(items=[(0x1002, 0x2000, 4)]), 'aligned'),
        (dict(items=[(0x1000, 0x2001, 4)]), 'aligned'),
        (dict(items=[(0x1000, 0x2000, -1)]), 'numel'),
        (dict(items=[(0x1000, 0x2000, 2 ** 31)]), 'numel'),
        (dict(items=[(0x1000, 0x2000, 4)], state=None), 'ema state'),
        (dict(items=[(0x1000, 0x2000, 4)], state=0x20003), 'ema state'),
    ])
    assert lib.ct_ema_update(None, 2, 0x20000, None) == 1
    assert 'items is NULL' in lib.ct_last_error_string().decode()
    _check(lib, 'ct_tensor_swap', swap, [
        (dict(items=[(0x1000, 0x2000, 4)], n=-1), 'negative'),
        (dict(items=[(None, 0x2000, 4)]), 'NULL a'),
        (dict(items=[(0x1000, None, 4)]), 'NULL b'),
        (dict(items=[(0x1000, 0x2002, 4)]), 'aligned'),
        (dict(items=[(0x1000, 0x2000, -1)]), 'numel'),
        (dict(items=[(0x1000, 0x2000, 2 ** 31)]), 'numel'),
        (dict(items=[(0x1000, 0x1000, 4)]), 'a == b'),
        (dict(items=[(0x1000, 0x100c, 4)]), 'overlap'),
        (dict(items=[(0x100c, 0x1000, 4)]), 'overlap'),
        (dict(items=[(0x1000, 0x2000, 8), (0x3000, 0x3004, 2)]), 'overlap'),
    ])
    assert lib.ct_tensor_swap(None, 1, None) == 1
    assert 'items is NULL' in lib.ct_last_error_string().decode()


# ------------------------------------------------------------------------------------------ WeightEMA / FusedSGD
def test_weight_ema_refusals():
    from ctdet._lib import CtdetError
    from ctdet.optim import WeightEMA
    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    for bad in (1.0, -0.1, 1.5, math.nan, '0.9', torch.tensor(0.9), True, None):
        with pytest.raises(ValueError):                         # before any device work: the model is on the CPU
            WeightEMA(model, decay=bad)
    for bad in (0.5, -1.0, math.nan, math.inf, '10', True):
        with pytest.raises(ValueError):
            WeightEMA(model, warmup=bad)
    with pytest.raises(CtdetError, match='no CPU path'):        # valid settings: the CPU model is the error
        WeightEMA(model)
    with pytest.raises(CtdetError, match='no CPU path'):
        WeightEMA(model, decay=0.0, warmup=0.0, buffers=False)


def _host_ema(tensors):
    """A WeightEMA over CPU tensors, put together by hand: enough for the host-side rules of attach_ema."""
    from ctdet.optim import WeightEMA
    ema = WeightEMA.__new__(WeightEMA)
    ema.decay, ema.warmup = 0.9998, 10.0
    ema._live = {str(i): t for i, t in enumerate(tensors)}
    ema.shadow = {str(i): t.detach().clone() for i, t in enumerate(tensors)}
    ema._by_id = {id(t): ema.shadow[str(i)] for i, t in enumerate(tensors)}
    ema.state = torch.zeros(16, dtype=torch.uint8)
    return ema


def test_attach_ema_rules_and_state_dict_layout():
    from ctdet.optim import FusedSGD
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))]
    plain = FusedSGD(ps, 0.1, momentum=0.9)
    assert plain.ema is None
    for bad in ('ema', 0.9998, object(), torch.zeros(3)):
        with pytest.raises(TypeError):
            plain.attach_ema(bad)
        with pytest.raises(TypeError):
            FusedSGD(ps, 0.1, momentum=0.9, ema=bad)
    with pytest.raises(ValueError, match='no shadow'):          # a parameter of the optimizer the average lacks
        plain.attach_ema(_host_ema(ps[:1]))
    assert plain.ema is None
    ema = _host_ema(ps)
    opt = FusedSGD(ps, 0.1, momentum=0.9, ema=ema)
    assert opt.ema is ema and plain.attach_ema(ema) is plain and plain.ema is ema
    assert plain.attach_ema(None).ema is None
    # an attribute, not a key: defaults, groups and the state dict are what they are without it -- and torch's
    assert opt.defaults == plain.defaults and opt.state_dict() == plain.state_dict()
    assert all('ema' not in g for g in opt.param_groups)
    ref = torch.optim.SGD(ps, 0.1, momentum=0.9)
    assert opt.state_dict()['param_groups'] == ref.state_dict()['param_groups']
    assert set(opt.state_dict()) == set(ref.state_dict())
    ref.load_state_dict(opt.state_dict())
    # __setstate__ defaults the attribute to None (an optimizer pickled before it existed)
    old = pickle.loads(pickle.dumps(plain))
    old.__dict__.pop('ema', None)
    old.__setstate__(old.__getstate__())
    assert old.ema is None
    # no gradients, no device: with an average attached the step has to reach the device and says so
    from ctdet._lib import CtdetError
    with pytest.raises(CtdetError):
        opt.step()


def _args(**kw):
    d = dict(method='ours', phase=2, setting='transfer', lr=4e-3, weight_decay=5e-4, momentum=0.9, steps=[30, 50],
             warmup_iter=10)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_build_optimizer_ema_switch(monkeypatch):
    from ctdet._lib import CtdetError
    from ctdet.optim import FusedSGD
    monkeypatch.delenv('CTDET_SGD_FUSED', raising=False)
    net = build_net(_args(), 300, 20)
    # without the attribute (or with None): unchanged
    assert type(solver.build_optimizer(_args(), net)) is torch.optim.SGD
    assert type(solver.build_optimizer(_args(ema_decay=None), net)) is torch.optim.SGD
    plain = solver.build_optimizer(_args(ema_decay=None, ema_warmup=5.0), net, fused=True)
    assert type(plain) is FusedSGD and plain.ema is None
    # a value without the fused optimizer: an error, no silent torch path
    with pytest.raises(ValueError, match='ema_decay'):
        solver.build_optimizer(_args(ema_decay=0.9998), net)
    with pytest.raises(ValueError, match='ema_decay'):
        solver.build_optimizer(_args(ema_decay=0.9998), net, fused=False)
    monkeypatch.setenv('CTDET_SGD_FUSED', '0')
    with pytest.raises(ValueError, match='ema_decay'):
        solver.build_optimizer(_args(ema_decay=0.9998), net)
    # fused: the values are checked first, then the model has to be on the device
    with pytest.raises(ValueError, match='decay'):
        solver.build_optimizer(_args(ema_decay=1.0), net, fused=True)
    with pytest.raises(ValueError, match='warmup'):
        solver.build_optimizer(_args(ema_decay=0.9998, ema_warmup=0.5), net, fused=True)
    monkeypatch.setenv('CTDET_SGD_FUSED', '1')
    with pytest.raises(CtdetError, match='no CPU path'):
        solver.build_optimizer(_args(ema_decay=0.9998), net)
