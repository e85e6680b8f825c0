"""ct_conv2d_wgrad_h2 (the f16x2 weight gradient of the 1x1 convolutions, csrc/ct_wgrad_h2.hip) without a device: exports,
the geometry table over the four shipped plans, the workspace size, the argument checks that return before any device work, and
which layers of a training runtime call it under CTDET_WGRAD_H2 (library proxy as in tests/test_wino_dispatch_cpu.py: host
queries go to the real libctdet, every other call is recorded instead of run)."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

from ctdet import _lib, engine, train_engine
from ctdet.engine import ConvPart, ConvStep, HipBackend
from test_wino_dispatch_cpu import _Train

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ct_conv_wgrad_h2_supported', 'ct_conv_wgrad_h2_workspace_bytes', 'ct_conv2d_wgrad_h2')


def _desc(cin=64, cout=96, h=19, w=19, k=1, stride=1, pad=0, dil=1, batch=2, in_=0x10000):
    d = _lib.ConvDesc()
    d.in_ = in_
    d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = batch, cin, h, w, cin, 0
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = cout, k, k, stride, pad, pad, dil
    d.oh = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1
    d.ow = (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return d


# ------------------------------------------------------------------ exports
def test_exports():
    out = subprocess.run(['nm', '-D', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == 'T'}
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    for n in NAMES:
        assert n in exported, n
        assert n in _lib.SIGNATURES, n
        assert re.search(r'\b(int|size_t)\s+%s\s*\(\s*const ct_conv_desc\s*\*' % n, header), n
    assert len(_lib.SIGNATURES['ct_conv2d_wgrad_h2'][1]) == 9


# ------------------------------------------------------------------ geometry
def _net(size, phase):
    from models.RFB_Net_vgg import build_net
    return build_net(types.SimpleNamespace(method='ours', phase=phase, setting='transfer'), size, 20).eval()


@pytest.mark.parametrize('size,phase', [(300, 1), (300, 2), (512, 1), (512, 2)])
def test_every_1x1_step_of_the_shipped_plans_is_supported(size, phase):
    lib = _lib.lib()
    plan = engine.Plan(_net(size, phase), 8)
    seen = 0
    for st in plan.steps:
        if st.kind != 'conv' or (st.kh, st.kw) != (1, 1):
            continue
        d = _desc(st.cin, st.cout, st.h, st.w, 1, st.stride, st.ph, st.dil, batch=8)
        assert (d.oh, d.ow) == (st.oh, st.ow), st.name
        assert lib.ct_conv_wgrad_h2_supported(C.byref(d)) == 1, (st.name, st.cin, st.cout, st.h, st.stride)
        assert lib.ct_conv_wgrad_h2_workspace_bytes(C.byref(d)) > 0, st.name
        seen += 1
    assert seen >= 10, seen
    assert any(st.kind == 'conv' and (st.kh, st.kw) == (1, 1) and st.stride == 2 for st in plan.steps)


@pytest.mark.parametrize('kw', [dict(k=3, pad=1), dict(k=4, pad=1), dict(pad=1), dict(dil=2), dict(stride=3)],
                         ids=['3x3', '4x4', 'pad', 'dil', 'stride3'])
def test_other_geometries_are_not_supported(kw):
    lib = _lib.lib()
    d = _desc(**kw)
    assert lib.ct_conv_wgrad_h2_supported(C.byref(d)) == 0
    assert lib.ct_conv_wgrad_h2_workspace_bytes(C.byref(d)) == 0
    assert lib.ct_conv_wgrad_h2_supported(C.byref(_desc())) == 1
    assert lib.ct_conv_wgrad_h2_supported(C.byref(_desc(stride=2))) == 1


def test_workspace_bytes_positive_and_monotone():
    lib = _lib.lib()
    for hw, batch in ((19, 32), (38, 32), (10, 8), (1, 8)):
        sizes = [(16, 16), (33, 20), (64, 64), (128, 512), (256, 1024), (1024, 1024), (2048, 2048), (4096, 4096)]
        got = [lib.ct_conv_wgrad_h2_workspace_bytes(C.byref(_desc(ci, co, hw, hw, batch=batch))) for co, ci in sizes]
        assert all(g > 2 * batch * _lib.ABSMAX_LINE_BYTES for g in got), got
        assert all(a <= b for a, b in zip(got, got[1:])), (hw, got)
        assert got[-1] >= 4096 * 4096 * 4 and got[-1] > got[0]


# ------------------------------------------------------------------ argument errors
def test_argument_errors_before_any_device_work():
    """Host-side checks: they return before anything touches a device (the library loads without one)."""
    lib = _lib.lib()
    ok = _desc()
    need = lib.ct_conv_wgrad_h2_workspace_bytes(C.byref(ok))

    def call(d=ok, dz=0x20000, ctot=96, coff=0, amax=None, dw=0x30000, ws=0x40000, nbytes=need):
        return lib.ct_conv2d_wgrad_h2(C.byref(d) if d is not None else None, dz, ctot, coff, amax, dw, ws, nbytes, None)

    mismatch = _desc()
    mismatch.oh = 18
    bad = [
        (dict(d=None), 'd is null'),
        (dict(d=_desc(in_=None)), 'd->in'),
        (dict(dz=None), 'dz'),
        (dict(dw=None), 'dw'),
        (dict(ws=None), 'workspace'),
        (dict(ctot=95), 'dz slice'),
        (dict(coff=-1), 'dz slice'),
        (dict(ctot=100, coff=5), 'dz slice'),
        (dict(d=mismatch), 'oh/ow'),
        (dict(nbytes=need - 1), 'workspace_bytes'),
        (dict(nbytes=0), 'workspace_bytes'),
        (dict(d=_desc(k=3, pad=1)), 'geometry'),
        (dict(d=_desc(stride=3)), 'geometry'),
        (dict(d=_desc(dil=2)), 'geometry'),
    ]
    for kw, word in bad:
        assert call(**kw) != 0, kw
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith('ct_conv2d_wgrad_h2') and word in msg, (kw, msg)
    assert call(d=_desc(k=3, pad=1)) == 4           # CT_ERR_UNSUPPORTED
    assert call(nbytes=need - 1) == 3               # CT_ERR_WORKSPACE


# ------------------------------------------------------------------ dispatch
HOST_QUERIES = ('ct_conv_kpad', 'ct_conv_mpad', 'ct_conv_x3_config_', 'ct_conv_config_name', 'ct_conv_num_configs',
                'ct_conv_x3_num_configs')


class _Lib:
    def __init__(self, log, names):
        self._real, self._log, self._names = _lib.lib(), log, names

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.endswith(('_supported', '_bytes', '_floats')) or name.startswith(HOST_QUERIES):
            if name.startswith('ct_conv_wgrad_h2'):
                self._log.append(('query', name))
            return fn

        def call(*args):
            names = self._names()
            self._log.append((name,) + tuple(self._arg(a, t, names) for a, t in zip(args, fn.argtypes)))
            return 0
        return call

    @staticmethod
    def _arg(a, t, names):
        if a is None or isinstance(a, (int, float)) and t is not _lib._P:
            return a
        if isinstance(a, int):
            return names.get(a, 'ptr')
        if isinstance(a, C.Array):
            return list(a) if a._type_ is C.c_int else 'ptrs'
        d = a._obj
        return 'desc', names.get(d.in_, 'ptr'), bool(d.in_absmax)


class _Backend(HipBackend):
    """HipBackend on the CPU: no device check, CPU buffers, no stream."""

    def __init__(self, log, names):
        self.device = torch.device('cpu')
        self.lib = _Lib(log, names)
        self.ws_pool, self.ws_generation = {}, 0
        self.slot_pool, self.slots_used = None, 0
        self.kernel_epoch = 0

    def _stream(self):
        return None

    def prepare_conv(self, st, bufs, batch):
        d = _lib.ConvDesc()
        d.batch, d.cin, d.h, d.w, d.in_ctot = batch, st.cin, st.h, st.w, st.cin
        d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = st.cout, st.kh, st.kw, st.stride, st.ph, st.pw, st.dil
        d.oh, d.ow, d.out_ctot = st.oh, st.ow, st.cout
        d.in_, d.out = bufs[st.src].data_ptr(), bufs[st.dst].data_ptr()
        st.rt['desc'] = d
        plain = st.dil == 1
        st.rt.update(wino_ok=plain, winox_ok=plain, wino4s_ok=True, wino4f_ok=plain)


def _conv(name, src, dst, hw, cin, cout, k=1, stride=1, bn=False):
    w = torch.nn.Parameter(torch.zeros(cout, cin, k, k))
    bnm = torch.nn.BatchNorm2d(cout) if bn else None
    b = None if bn else torch.nn.Parameter(torch.zeros(cout))
    return ConvStep(name, [ConvPart(w, b, bnm, True)], cin, k, k, stride, k // 2, k // 2, 1, src, 0, hw, hw, dst, 0)


def _plan():
    """3x3 'A' -> 1x1 bias+ReLU 'P1' -> 1x1 BatchNorm 'P2' -> 1x1 BatchNorm 'P3' -> 1x1 stride-2 BatchNorm 'S' -> 3x3 'C' -> 1x1
    'T' on a 10x10 map.  Every 1x1 layer has a supported geometry; the selection rule (profiles/wgrad_h2_probe.txt) keeps the
    stride-2 layer and the small map on ct_conv2d_wgrad, where the new kernel measured slower."""
    steps = [_conv('A', 'x', 'a', 38, 64, 64, k=3), _conv('P1', 'a', 'b', 38, 64, 96), _conv('P2', 'b', 'c', 38, 96, 48, bn=True),
             _conv('P3', 'c', 'c2', 38, 48, 48, bn=True), _conv('S', 'c2', 'd', 38, 48, 64, stride=2, bn=True),
             _conv('C', 'd', 'e', 19, 64, 64, k=3), _conv('T', 'f', 'g', 10, 64, 32, bn=True)]
    shapes = {'x': (64, 38, 38), 'a': (64, 38, 38), 'b': (96, 38, 38), 'c': (48, 38, 38), 'c2': (48, 38, 38), 'd': (64, 19, 19),
              'e': (64, 19, 19), 'f': (64, 10, 10), 'g': (32, 10, 10)}
    return types.SimpleNamespace(steps=steps, buf_shapes=shapes, ctx=False)


def _backward_log(monkeypatch, value):
    if value is None:
        monkeypatch.delenv('CTDET_WGRAD_H2', raising=False)
    else:
        monkeypatch.setenv('CTDET_WGRAD_H2', value)
    monkeypatch.setenv('CTDET_TRAIN_H2', '1')
    monkeypatch.setenv('CTDET_H2', '2')
    monkeypatch.setenv('CTDET_TRAIN_STREAMS', '1')
    monkeypatch.setenv('CTDET_STREAMS', '1')
    plan = _plan()
    monkeypatch.setattr(train_engine, 'Plan', lambda net, batch: plan)
    monkeypatch.setattr(train_engine, 'apply_tuned', lambda be, s, batch, wino4=True: True)
    log, box = [], {}

    def names():
        if 'rt' not in box:
            return {}
        rt = box['rt']
        out = {t.data_ptr(): 'buf.' + k for k, t in rt.bufs.items()}
        out.update({s.dz.data_ptr(): 'dz.' + k for k, s in rt.state.items()})
        out.update({s.dw.data_ptr(): 'dw.' + k for k, s in rt.state.items()})
        for k in ('wgrad_wsh2', 'wgrad_ws4s'):
            if getattr(rt, k, None) is not None:
                out[getattr(rt, k).data_ptr()] = k
        return out
    rt = _Train(types.SimpleNamespace(size=300), 2, _Backend(log, names))
    box['rt'] = rt
    built = list(log)
    for s in rt.state.values():
        s.frozen = [False]
    del log[:]
    written = {}
    rt._backward_steps({}, written, lambda n, c0, c1: any(a < c1 and c0 < b for a, b in written.get(n, [])),
                       lambda prm, g: None, None, None)
    return rt, built, list(log)


def _wgrad_calls(log):
    return [e for e in log if 'wgrad' in e[0]]


def test_switch_off_launches_what_the_parent_launched(monkeypatch):
    logs = {}
    for value in (None, '0', ''):
        rt, built, log = _backward_log(monkeypatch, value)
        assert not rt.wgrad_h2 and rt.wgrad_wsh2 is None
        assert not [e for e in built + log if 'wgrad_h2' in ''.join(map(str, e[:2]))], value       # not even a host query
        logs[value] = log
    assert logs['0'] == logs[None] and logs[''] == logs[None]
    calls = _wgrad_calls(logs[None])
    assert [e[0] for e in calls].count('ct_conv2d_wgrad') == 5           # T, S, P3, P2, P1
    assert all(e[0] != 'ct_conv2d_wgrad_h2' for e in calls)


def test_switch_on_moves_exactly_the_selected_1x1_layers(monkeypatch):
    _, _, off = _backward_log(monkeypatch, None)
    rt, built, on = _backward_log(monkeypatch, '1')
    assert rt.wgrad_h2 and rt.h2
    lib = _lib.lib()
    need = max(lib.ct_conv_wgrad_h2_workspace_bytes(C.byref(rt.state[n].wgrad)) for n in ('P1', 'P2', 'P3'))
    assert rt.wgrad_wsh2.numel() == need
    assert {n for n, s in rt.state.items() if s.wgrad_route.name == 'h2'} == {'P1', 'P2', 'P3'}
    calls_on, calls_off = _wgrad_calls(on), _wgrad_calls(off)
    assert len(calls_on) == len(calls_off) == 7
    assert all(lib.ct_conv_wgrad_h2_supported(C.byref(rt.state[n].wgrad)) == 1 for n in ('P1', 'P2', 'P3', 'S', 'T'))
    moved = [e for e in calls_on if e[0] == 'ct_conv2d_wgrad_h2']
    # (name, desc, dz, dz_ctot, dz_coff, dz_absmax, dw, workspace, workspace_bytes, stream): reverse plan order
    assert [(e[2], e[3], e[4], e[6], e[7], e[8], e[9]) for e in moved] == [
        ('dz.P3', 48, 0, 'dw.P3', 'wgrad_wsh2', need, None),
        ('dz.P2', 48, 0, 'dw.P2', 'wgrad_wsh2', need, None),
        ('dz.P1', 96, 0, 'dw.P1', 'wgrad_wsh2', need, None)]
    assert [e[1][1] for e in moved] == ['buf.c', 'buf.b', 'buf.a']
    kept = [e[2] for e in calls_on if e[0] == 'ct_conv2d_wgrad']
    assert kept == ['dz.T', 'dz.S'], kept          # small map, stride 2: slower there, left on the fp32 kernel
    # dZ's maxima only where ct_bias_act_backward_amax wrote dZ (P1: bias + ReLU); the BatchNorm backward does not track
    assert [e[5] is not None for e in moved] == [False, False, True]
    amax = [e for e in on if e[0] == 'ct_bias_act_backward_amax']
    p1 = [e for e in amax if e[11] == 'dz.P1']
    assert len(p1) == 1 and p1[0][-2] is not None
    # the 3x3 layers keep their entry, and everything that is no weight gradient is launched as before
    for a, b in zip(calls_on, calls_off):
        if a[0] != 'ct_conv2d_wgrad_h2':
            assert a == b
        else:
            assert b[0] == 'ct_conv2d_wgrad'
    assert [e[0] for e in on if 'wgrad' not in e[0]] == [e[0] for e in off if 'wgrad' not in e[0]]
