"""Which libctdet entry points the Winograd forward and data-gradient launches call, with which scalar arguments (no device).

HipBackend.enable_wino + run_conv and the training runtime's data-gradient pack + launch run against a library proxy: pure host
queries (sizes, geometry checks, configs) go to the real libctdet, every other call is recorded instead of run.  Pointer
arguments are recorded by the name of the buffer they point into (the st.rt key of the packed weights, 'ws', 'pool', ...).
"""
import ctypes as C
import types

import pytest
import torch

from ctdet import _lib, train_engine
from ctdet.engine import ConvPart, ConvStep, HipBackend

HOST_QUERIES = ('ct_conv_kpad', 'ct_conv_mpad', 'ct_conv_x3_config_', 'ct_conv_config_name', 'ct_conv_num_configs',
                'ct_conv_x3_num_configs')
KEPT = ('ct_conv_pack_', 'ct_conv2d_', 'ct_absmax_f32')


class _Lib:
    def __init__(self, log, names):
        self._real, self._log, self._names = _lib.lib(), log, names

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.endswith(('_supported', '_bytes', '_floats')) or name.startswith(HOST_QUERIES):
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
        d = a._obj                      # C.byref(ConvDesc): where it writes and whether it accumulates
        return 'desc', names.get(d.in_, 'ptr'), names.get(d.out, 'ptr'), d.res and names.get(d.res, 'ptr')


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


def _step(dil=1, cin=64, cout=64, hw=38, bias=True):
    w = torch.nn.Parameter(torch.zeros(cout, cin, 3, 3))
    b = torch.nn.Parameter(torch.zeros(cout)) if bias else None
    return ConvStep('c', [ConvPart(w, b, None, True)], cin, 3, 3, 1, dil, dil, dil, 'a', 0, hw, hw, 'b')


def _names(*groups):
    def names():
        out = {}
        for prefix, d in groups:
            for k, v in d().items():
                if isinstance(v, torch.Tensor) and v.numel():
                    out[v.data_ptr()] = prefix + k
        return out
    return names


def _forward(tile, pool, dil):
    log = []
    st = _step(dil)
    bufs = {'a': torch.zeros(2, 64, 38, 38), 'b': torch.zeros(2, 64, 38, 38), 'pool': torch.zeros(2, 64, 19, 19)}
    be = None
    be = _Backend(log, _names(('', lambda: st.rt), ('', lambda: bufs),
                              ('ws', lambda: {str(k): v for k, v in be.ws_pool.items() if v is not None})))
    be.prepare_conv(st, bufs, 2)
    if pool:
        st.rt['pool'] = (bufs['pool'], 19, 19, False)
    before = set(st.rt)
    be.enable_wino(st, tile=tile)
    allocs = sorted((k, st.rt[k].numel() * st.rt[k].element_size()) for k in set(st.rt) - before
                    if isinstance(st.rt[k], torch.Tensor))
    be.run_conv(st)
    return allocs, [e for e in log if e[0].startswith(KEPT)]


FORWARD = {
    (2, False, 1): ([('U', 262144)], [
        ('ct_conv_pack_weights_wino', 'ptrs', [64], 1, 64, 'U', None),
        ('ct_conv2d_wino_fwd', ('desc', 'a', 'b', None), 'U', None),
    ]),
    (2, True, 1): ([('U', 262144)], [
        ('ct_conv_pack_weights_wino', 'ptrs', [64], 1, 64, 'U', None),
        ('ct_conv2d_wino_pool_fwd', ('desc', 'a', 'b', None), 'U', 'pool', 64, 0, 19, 19, 0, None),
    ]),
    (4, False, 1): ([('U4', 589824)], [
        ('ct_conv_pack_weights_wino4', 'ptrs', [64], 1, 64, 'U4', None),
        ('ct_conv2d_wino4_fwd', ('desc', 'a', 'b', None), 'U4', None),
    ]),
    (4, True, 1): ([('U4', 589824)], [
        ('ct_conv_pack_weights_wino4', 'ptrs', [64], 1, 64, 'U4', None),
        ('ct_conv2d_wino4_pool_fwd', ('desc', 'a', 'b', None), 'U4', 'pool', 64, 0, 19, 19, 0, None),
    ]),
    (23, False, 1): ([('UX', 393216)], [
        ('ct_conv_pack_weights_wino_x3', 'ptrs', [64], 1, 64, 'UX', None),
        ('ct_conv2d_wino_x3_fwd', ('desc', 'a', 'b', None), 'UX', 1, None),
    ]),
    (23, True, 1): ([('UX', 393216)], [
        ('ct_conv_pack_weights_wino_x3', 'ptrs', [64], 1, 64, 'UX', None),
        ('ct_conv2d_wino_x3_pool_fwd', ('desc', 'a', 'b', None), 'UX', 1, 'pool', 64, 0, 19, 19, 0, None),
    ]),
    (44, False, 1): ([('U4S', 1769472)], [
        ('ct_conv_pack_weights_wino4s', 'ptrs', [64], 1, 64, 'U4S', None),
        ('ct_conv2d_wino4s_fwd', ('desc', 'a', 'b', None), 'U4S', 'ws0', 8257792, 1, None),
    ]),
    (44, True, 1): ([('U4S', 1769472)], [
        ('ct_conv_pack_weights_wino4s', 'ptrs', [64], 1, 64, 'U4S', None),
        ('ct_conv2d_wino4s_pool_fwd', ('desc', 'a', 'b', None), 'U4S', 'ws0', 8257792, 1, 'pool', 64, 0, 19, 19, 0, None),
    ]),
    (46, False, 1): ([('U4F', 884736)], [
        ('ct_conv_pack_weights_wino4f', 'ptrs', [64], 1, 64, 'U4F', None),
        ('ct_conv2d_wino4f_pool_fwd_v', ('desc', 'a', 'b', None), 'U4F', 1, None, 0, 0, 0, 0, 1, None),
    ]),
    (46, True, 1): ([('U4F', 884736)], [
        ('ct_conv_pack_weights_wino4f', 'ptrs', [64], 1, 64, 'U4F', None),
        ('ct_conv2d_wino4f_pool_fwd_v', ('desc', 'a', 'b', None), 'U4F', 1, 'pool', 64, 0, 19, 19, 0, None),
    ]),
    (47, False, 1): ([('U4H', 1179904)], [
        ('ct_conv_pack_weights_wino4s_h2', 'ptrs', [64], 1, 64, 'U4H', None),
        ('ct_conv2d_wino4s_fwd', ('desc', 'a', 'b', None), 'U4H', 'ws0', 8257792, 3, None),
    ]),
    (47, True, 1): ([('U4H', 1179904)], [
        ('ct_conv_pack_weights_wino4s_h2', 'ptrs', [64], 1, 64, 'U4H', None),
        ('ct_conv2d_wino4s_pool_fwd', ('desc', 'a', 'b', None), 'U4H', 'ws0', 8257792, 3, 'pool', 64, 0, 19, 19, 0, None),
    ]),
    (48, False, 1): ([('U4FH', 590080)], [
        ('ct_conv_pack_weights_wino4f_h2', 'ptrs', [64], 1, 64, 'U4FH', None),
        ('ct_absmax_f32', 'a', 2, 92416, 92416, 'amax_own', None),
        ('ct_conv2d_wino4f_pool_fwd_v', ('desc', 'a', 'b', None), 'U4FH', 2, None, 0, 0, 0, 0, 1, None),
    ]),
    (48, True, 1): ([('U4FH', 590080)], [
        ('ct_conv_pack_weights_wino4f_h2', 'ptrs', [64], 1, 64, 'U4FH', None),
        ('ct_absmax_f32', 'a', 2, 92416, 92416, 'amax_own', None),
        ('ct_conv2d_wino4f_pool_fwd_v', ('desc', 'a', 'b', None), 'U4FH', 2, 'pool', 64, 0, 19, 19, 0, None),
    ]),
    (44, False, 2): ([('U4S', 1769472)], [
        ('ct_conv_pack_weights_wino4s', 'ptrs', [64], 1, 64, 'U4S', None),
        ('ct_conv2d_wino4s_fwd', ('desc', 'a', 'b', None), 'U4S', 'ws0', 8257792, 1, None),
    ]),
    (47, False, 2): ([('U4H', 1179904)], [
        ('ct_conv_pack_weights_wino4s_h2', 'ptrs', [64], 1, 64, 'U4H', None),
        ('ct_conv2d_wino4s_fwd', ('desc', 'a', 'b', None), 'U4H', 'ws0', 8257792, 3, None),
    ]),
}


def _forward_cases():
    for tile in (2, 4, 23, 44, 46, 47, 48):
        for pool in (False, True):
            yield tile, pool, 1
    for tile in (44, 47):
        yield tile, False, 2


@pytest.mark.parametrize('tile,pool,dil', list(_forward_cases()))
def test_forward_dispatch(tile, pool, dil):
    got = _forward(tile, pool, dil)
    assert got == FORWARD[(tile, pool, dil)]


class _Train(train_engine.TrainRuntime):
    def _s(self):
        return None


def _dgrad(fwd_tile, h2, dil, acc, monkeypatch):
    """One training layer 'c' (src 'a' -> dst 'b', bias + ReLU) whose forward launch runs `fwd_tile`: the allocation of its
    data-gradient weights, their pack and the data-gradient launch."""
    monkeypatch.setenv('CTDET_TRAIN_H2', '1' if h2 else '0')
    monkeypatch.setenv('CTDET_H2', '2')
    monkeypatch.setenv('CTDET_TRAIN_STREAMS', '1')
    monkeypatch.setenv('CTDET_STREAMS', '1')
    st = _step(dil)
    plan = types.SimpleNamespace(steps=[st], buf_shapes={'x': (3, 4, 4), 'a': (64, 38, 38), 'b': (64, 38, 38)}, ctx=False)
    monkeypatch.setattr(train_engine, 'Plan', lambda net, batch: plan)
    monkeypatch.setattr(train_engine, 'apply_tuned', lambda be, s, batch, wino4=True: be.enable_wino(s, tile=fwd_tile))
    log, box = [], {}
    be = _Backend(log, _names(('', lambda: {'U_d': box['s'].U_d, 'dz': box['s'].dz} if 's' in box else {}),
                              ('', lambda: {'ws': box['rt'].dgrad_ws4s} if 'rt' in box else {}),
                              ('grad.', lambda: box['rt'].grads if 'rt' in box else {}),
                              ('', lambda: box['rt'].bufs if 'rt' in box else {})))
    rt = _Train(types.SimpleNamespace(size=300), 2, be)
    s = rt.state['c']
    box.update(s=s, rt=rt)
    if s.dgrad_wino is None:
        return None
    alloc = ('U_d', s.U_d.numel() * s.U_d.element_size())
    del log[:]
    rt._pack_dgrad(st, s)
    written = {'a': [(0, 64)]} if acc else {}
    rt._backward_steps({}, written, lambda n, c0, c1: any(a < c1 and c0 < b for a, b in written.get(n, [])),
                       lambda prm, g: None, None, None)
    return s.dgrad_tile, alloc, [e for e in log if e[0].startswith(KEPT) and 'wgrad' not in e[0]]


DGRAD_CASES = [(2, False, 1, False), (4, False, 1, False), (44, False, 1, False), (44, False, 1, True), (46, False, 1, False),
               (47, True, 1, False), (48, True, 1, False), (44, False, 2, False), (44, False, 2, True),
               (47, True, 2, False), (47, True, 2, True)]
DGRAD = {
    (2, False, 1, False): (2, ('U_d', 262144), [
        ('ct_conv_pack_weights_wino_dgrad', 'ptrs', [64], 1, 64, 'U_d', None),
        ('ct_conv2d_wino_fwd', ('desc', 'dz', 'grad.a', None), 'U_d', None),
    ]),
    (4, False, 1, False): (4, ('U_d', 589824), [
        ('ct_conv_pack_weights_wino4_dgrad', 'ptrs', [64], 1, 64, 'U_d', None),
        ('ct_conv2d_wino4_fwd', ('desc', 'dz', 'grad.a', None), 'U_d', None),
    ]),
    (44, False, 1, False): (44, ('U_d', 1769472), [
        ('ct_conv_pack_weights_wino4s_dgrad', 'ptrs', [64], 1, 64, 'U_d', None),
        ('ct_conv2d_wino4s_fwd', ('desc', 'dz', 'grad.a', None), 'U_d', 'ws', 8257792, 1, None),
    ]),
    (44, False, 1, True): (44, ('U_d', 1769472), [
        ('ct_conv_pack_weights_wino4s_dgrad', 'ptrs', [64], 1, 64, 'U_d', None),
        ('ct_conv2d_wino4s_fwd', ('desc', 'dz', 'grad.a', 'grad.a'), 'U_d', 'ws', 8257792, 1, None),
    ]),
    (46, False, 1, False): (46, ('U_d', 884736), [
        ('ct_conv_pack_weights_wino4f_dgrad', 'ptrs', [64], 1, 64, 'U_d', None),
        ('ct_conv2d_wino4f_pool_fwd_v', ('desc', 'dz', 'grad.a', None), 'U_d', 1, None, 0, 0, 0, 0, 1, None),
    ]),
    (47, True, 1, False): (47, ('U_d', 1179904), [
        ('ct_conv_pack_weights_wino4s_h2_dgrad', 'ptrs', [64], 1, 64, 'U_d', None),
        ('ct_conv2d_wino4s_fwd', ('desc', 'dz', 'grad.a', None), 'U_d', 'ws', 8257792, 3, None),
    ]),
    (48, True, 1, False): (48, ('U_d', 590080), [
        ('ct_conv_pack_weights_wino4f_h2_dgrad', 'ptrs', [64], 1, 64, 'U_d', None),
        ('ct_conv2d_wino4f_pool_fwd_v', ('desc', 'dz', 'grad.a', None), 'U_d', 2, None, 0, 0, 0, 0, 1, None),
    ]),
    (44, False, 2, False): (44, ('U_d', 1769472), [
        ('ct_conv_pack_weights_wino4s_dgrad', 'ptrs', [64], 1, 64, 'U_d', None),
        ('ct_conv2d_wino4s_fwd', ('desc', 'dz', 'grad.a', None), 'U_d', 'ws', 8257792, 1, None),
    ]),
    (44, False, 2, True): (44, ('U_d', 1769472), [
        ('ct_conv_pack_weights_wino4s_dgrad', 'ptrs', [64], 1, 64, 'U_d', None),
        ('ct_conv2d_wino4s_fwd', ('desc', 'dz', 'ptr', None), 'U_d', 'ws', 8257792, 1, None),
    ]),
    (47, True, 2, False): (47, ('U_d', 1179904), [
        ('ct_conv_pack_weights_wino4s_h2_dgrad', 'ptrs', [64], 1, 64, 'U_d', None),
        ('ct_conv2d_wino4s_fwd', ('desc', 'dz', 'grad.a', None), 'U_d', 'ws', 8257792, 3, None),
    ]),
    (47, True, 2, True): (47, ('U_d', 1179904), [
        ('ct_conv_pack_weights_wino4s_h2_dgrad', 'ptrs', [64], 1, 64, 'U_d', None),
        ('ct_conv2d_wino4s_fwd', ('desc', 'dz', 'ptr', None), 'U_d', 'ws', 8257792, 3, None),
    ]),
}


@pytest.mark.parametrize('fwd_tile,h2,dil,acc', DGRAD_CASES)
def test_dgrad_dispatch(fwd_tile, h2, dil, acc, monkeypatch):
    got = _dgrad(fwd_tile, h2, dil, acc, monkeypatch)
    assert got == DGRAD[(fwd_tile, h2, dil, acc)]
