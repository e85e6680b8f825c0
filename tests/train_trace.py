"""A launch trace of one whole training step of a shipped plan, without a device (tests/test_train_trace_cpu.py checks it against
tests/golden/train_trace.json, tools/gen_train_trace.py writes that file and dumps full traces).

The real TrainRuntime is built on a HipBackend with CPU buffers and a library proxy, as in tests/test_wino_dispatch_cpu.py: host
queries go to the real libctdet, every other call is recorded -- entry point and EVERY argument -- and returns 0.  Pointers are
recorded as (name of the tensor they fall in, byte offset); a descriptor as all of its fields.  The item builders of the two batched
pack lists (ct_conv_x3_pack_item, ct_conv_wino_h2_pack_item) are host functions: they run, and the item they fill is recorded field
by field.  ct_pack_record_end copies the recorded table to the device and cannot run here: it is stubbed to count the pack calls
that the proxy logged since ct_pack_record_begin, which ARE the first table's items.
"""
import contextlib
import ctypes as C
import functools
import hashlib
import json
import os
import struct
import types

import torch

from ctdet import _lib
from ctdet.engine import HipBackend
from test_wino_dispatch_cpu import _Train as TraceTrain

HOST_QUERIES = ('ct_conv_kpad', 'ct_conv_mpad', 'ct_conv_x3_config_', 'ct_conv_config_name', 'ct_conv_num_configs',
                'ct_conv_x3_num_configs')
UNNAMED = 'UNNAMED'
# host-side layouts of the two pack items (csrc/ct_conv_x3.hip X3PackArgs, csrc/ct_wino4s.hip WinoH2Item): P = pointer
ITEMS = {
    'ct_conv_x3_pack_item': ('<6Q14i2Q', ['P'] * 6 + ['mbeg%d' % i for i in range(7)] +
                             ['nparts', 'cin', 'khw', 'bk', 'm_pad', 'cgroups', 'dgrad', 'P', 'P']),
    'ct_conv_wino_h2_pack_item': ('<6Q15i4x2Q', ['P'] * 6 + ['mbeg%d' % i for i in range(7)] +
                                  ['nparts', 'cin', 'cout', 'chunks', 'kblocks', 'dgrad', 'cin_fwd', 'tile', 'P', 'P']),
}
DESC_POINTERS = ('in_', 'out', 'res', 'wpacked', 'scale', 'shift', 'lo', 'ksplit_ws', 'in_absmax', 'out_absmax')

ENVS = {
    'default': {'CTDET_H2': '2', 'CTDET_TRAIN_H2': '1'},
    'train_h2_0': {'CTDET_TRAIN_H2': '0'},
    'pack_batch_0': {'CTDET_PACK_BATCH': '0'},
    'prezero_0': {'CTDET_PREZERO': '0'},
    'fuse_pool_bwd_0': {'CTDET_TRAIN_FUSE_POOL_BWD': '0'},
    'ksplit_0': {'CTDET_KSPLIT': '0'},
    'wgrad_h2_1': {'CTDET_WGRAD_H2': '1'},
}
NETS = {'300p1': (300, 1), '300p2': (300, 2), '512p1': (512, 1)}
# (case id, net, environment, what runs): 'step' = forward + reverse walk; 'again' = that, then a second forward (traced alone);
# 'retile' = that, then be.enable_wino moves one layer to another tile and a forward follows (traced alone)
CASES = [('%s-%s' % (n, e), n, e, 'step') for n in NETS for e in ENVS] + \
    [('300p2-default-again', '300p2', 'default', 'again'), ('300p2-default-retile', '300p2', 'default', 'retile')]
BATCH = 2


class Namer:
    """pointer -> (name, byte offset) of the smallest named tensor that holds it."""

    def __init__(self, tensors, fixed):
        self.tensors, self.pointers, self.unnamed = tensors, 0, []
        self.fixed = self._spans(fixed)         # the network's parameters and buffers: they do not move during a trace

    @staticmethod
    def _spans(tensors):
        return [(t.numel() * t.element_size(), name, t.data_ptr()) for name, t in tensors
                if isinstance(t, torch.Tensor) and t.numel()]

    def table(self):
        return sorted(self.fixed + self._spans(self.tensors()))

    def name(self, p, spans, where):
        if not p:
            return None
        self.pointers += 1
        for size, name, base in spans:
            if base <= p < base + size:
                return [name, p - base]
        self.unnamed.append(where)
        return UNNAMED


class TraceLib:
    def __init__(self, log, namer):
        self._real, self._log, self._namer = _lib.lib(), log, namer
        self._rec_from = 0

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.endswith(('_supported', '_bytes', '_floats')) or name.startswith(HOST_QUERIES):
            return fn

        def call(*args):
            spans = self._namer.table()
            entry = [name] + [self._arg(a, t, spans, name) for a, t in zip(args, fn.argtypes)]
            assert len(args) == len(fn.argtypes), name
            if name in ITEMS:                   # a host function: fills the item, which is recorded by field
                rc = fn(*args)
                assert rc == 0, (name, self._real.ct_last_error_string())
                fmt, fields = ITEMS[name]
                raw = bytes(args[-1])
                assert len(raw) == struct.calcsize(fmt), (name, len(raw))
                entry[-1] = [self._namer.name(v, spans, name + ' item') if f == 'P' else [f, v]
                             for f, v in zip(fields, struct.unpack(fmt, raw))]
            elif name == 'ct_pack_record_begin':
                self._rec_from = len(self._log) + 1
            elif name == 'ct_pack_record_end':
                packs = [e[0] for e in self._log[self._rec_from:] if e[0].startswith('ct_conv_pack_weights')]
                nw = sum('wino' in n for n in packs)
                args[2]._obj.value, args[3]._obj.value = len(packs) - nw, nw
                entry[3:5] = [len(packs) - nw, nw]
            self._log.append(entry)
            return 0
        return call

    def _arg(self, a, t, spans, where):
        nm = self._namer
        if a is None:
            return None
        if isinstance(a, C.c_void_p):
            return nm.name(a.value, spans, where)
        if isinstance(a, (int, float)):
            return nm.name(a, spans, where) if t is _lib._P else a
        if isinstance(a, C.Array):
            if a._type_ is C.c_int:
                return list(a)
            if a._type_ is C.c_void_p:
                return [nm.name(p, spans, where) for p in a]
            if a._type_ is C.c_ubyte:
                return 'item'
            assert a._type_ is _lib.OutSegment, (where, a._type_)
            return [self._segment(sg, spans, where) for sg in a]
        d = a._obj
        if isinstance(d, C.c_int):
            return d.value
        assert isinstance(d, _lib.ConvDesc), (where, type(d))
        out = {}
        for f, _ in _lib.ConvDesc._fields_:
            v = getattr(d, f)
            out[f] = [self._segment(sg, spans, where) for sg in v] if f == 'seg' else \
                nm.name(v, spans, where + ' desc.' + f) if f in DESC_POINTERS else v
        return out

    def _segment(self, sg, spans, where):
        return {'ptr': self._namer.name(sg.ptr, spans, where + ' segment'), 'co_begin': sg.co_begin, 'co_end': sg.co_end,
                'pix_stride': sg.pix_stride, 'img_stride': sg.img_stride, 'base': sg.base}


class TraceBackend(HipBackend):
    """HipBackend on the CPU: no device check, CPU buffers, no stream; the real prepare_conv / pack_conv / run_conv."""

    def __init__(self, log, namer):
        self.device = torch.device('cpu')
        self.lib = TraceLib(log, namer)
        self.ws_pool, self.ws_generation = {}, 0
        self.slot_pool, self.slots_used = None, 0
        self.kernel_epoch = 0

    def _stream(self):
        return None

    def _ws_drop(self, key):                    # HipBackend's waits for the device first
        if self.ws_pool.get(key) is not None:
            self.ws_generation += 1
        self.ws_pool[key] = None


def _named(prefix, v):
    if isinstance(v, torch.Tensor):
        yield prefix, v
    elif isinstance(v, (list, tuple)):
        for i, t in enumerate(v):
            yield from _named('%s[%d]' % (prefix, i), t)
    elif isinstance(v, dict):
        for k, t in v.items():
            yield from _named('%s[%s]' % (prefix, k), t)


def _tensors(box):
    """Every tensor the step may hand to the library, by name (looked up at each call: buffers appear and move)."""
    for k, t in box.get('extra', {}).items():
        yield k, t
    be = box.get('be')
    if be is not None:
        for k, t in be.ws_pool.items():
            yield 'ws_pool[%s]' % k, t
        if be.slot_pool is not None:
            for i in range(be.slot_pool.shape[0]):
                yield 'slot[%d]' % i, be.slot_pool[i]
    rt = box.get('rt')
    if rt is None:
        return
    for k, t in rt.bufs.items():
        yield 'buf.' + k, t
    for k, t in rt.grads.items():
        yield 'grad.' + k, t
    for k in ('wgrad_ws', 'dgrad_ws4s', 'wgrad_ws4s', 'wgrad_wsh2', 'bn_scratch', 'wgrad_ws_all', 'arena', '_pack_table'):
        yield k, getattr(rt, k, None)
    for k in ('_x3_list', '_h2_list'):          # (table, count, key), or an object with a .table
        lst = getattr(rt, k, None)
        yield k, lst[0] if isinstance(lst, tuple) else getattr(lst, 'table', None)
    if rt.ctx is not None:
        for k, t in vars(rt.ctx).items():
            yield 'ctx.' + k, t
    for name, s in rt.state.items():
        for k, v in vars(s).items():
            if k in ('fwd', 'zstep'):
                continue
            yield from _named('%s.%s' % (name, k), v)
        if getattr(s, 'fwd', None) is not None:
            for k, v in s.fwd.rt.items():
                yield from _named('%s.rt.%s' % (name, k), v)


@contextlib.contextmanager
def _host_parameters():
    """HipBackend.pack_conv refuses parameters that are not on the HIP device; on the recording backend they are CPU tensors."""
    assert 'is_cuda' not in vars(torch.Tensor)      # inherited from the C base class: deleting the override restores it
    torch.Tensor.is_cuda = property(lambda self: True)
    try:
        yield
    finally:
        del torch.Tensor.is_cuda


@functools.lru_cache(maxsize=None)
def _net(size, phase):
    from models.RFB_Net_vgg import build_net
    torch.manual_seed(0)
    return build_net(types.SimpleNamespace(method='ours', phase=phase, setting='transfer'), size, 20).train()


def _walk(rt, extra):
    flat = {k: torch.zeros_like(rt.bufs[k]).view(rt.batch, -1) for k in ('loc', 'conf', 'obj')}
    extra.update({'flat.' + k: t for k, t in flat.items()})
    written = {}
    rt._backward_steps(flat, written, lambda n, c0, c1: any(a < c1 and c0 < b for a, b in written.get(n, [])),
                       lambda prm, g: None, None, None)


def trace(net_key, env_key, mode, setenv, delenv):
    """-> (trace, number of pointer arguments, places of unnamed pointers).  setenv / delenv: monkeypatch's, or os.environ's."""
    for k in [k for k in os.environ if k.startswith('CTDET_') and k != 'CTDET_LIB']:
        delenv(k)
    for k, v in dict(ENVS[env_key], CTDET_STREAMS='1', CTDET_TRAIN_STREAMS='1', CTDET_TUNE='0').items():
        setenv(k, v)
    size, phase = NETS[net_key]
    log, box = [], {}
    net = _net(size, phase)
    namer = Namer(lambda: _tensors(box), [('net.' + k, t) for k, t in list(net.named_parameters()) + list(net.named_buffers())])
    with _host_parameters():
        be = TraceBackend(log, namer)
        box['be'] = be
        rt = TraceTrain(net, BATCH, be)
        box['rt'] = rt
        x = torch.zeros((BATCH,) + tuple(rt.plan.buf_shapes['x']))
        box['extra'] = {'x': x}
        del log[:]
        namer.pointers, namer.unnamed = 0, []
        rt.forward(x, use_ctx=False)
        _walk(rt, box['extra'])
        if mode != 'step':
            if mode == 'retile':
                st = next(s.fwd for s in rt.state.values() if s.fwd.rt.get('wino') == 48 and s.fwd.rt.get('wino4s_ok'))
                be.enable_wino(st, tile=47)
            del log[:]
            namer.pointers, namer.unnamed = 0, []
            rt.forward(x, use_ctx=False)
    return log, namer.pointers, namer.unnamed


def canonical(log):
    return json.dumps(log, sort_keys=True, separators=(',', ':'), allow_nan=False)


def summary(log, pointers):
    calls = {}
    for e in log:
        calls[e[0]] = calls.get(e[0], 0) + 1
    return {'sha256': hashlib.sha256(canonical(log).encode()).hexdigest(), 'calls': dict(sorted(calls.items())),
            'pointers': pointers}
