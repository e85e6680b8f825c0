"""The bf16 Winograd route (csrc/ct_wino_bf16.hip, CTDET_BF16_WINO) without a device: exported symbols, the pure-host queries of
the C ABI, and which entry points HipBackendBF16 calls with the switch unset and set (a library proxy records every call that
would launch, as tests/test_wino_dispatch_cpu.py does)."""
import ctypes as C
import os
import re

import pytest
import torch

from ctdet import _lib
from ctdet.engine import ConvPart, ConvStep
from ctdet.engine_bf16 import HipBackendBF16

NEW = ('ct_conv_bf16_wino_supported', 'ct_conv_bf16_wino_packed_bytes', 'ct_conv_pack_weights_bf16_wino',
       'ct_conv_bf16_wino_workspace_bytes', 'ct_conv2d_bf16_wino_fwd', 'ct_absmax_bf16_nhwc')
LAUNCHES = ('ct_conv_pack_weights_bf16_wino', 'ct_conv2d_bf16_wino_fwd', 'ct_absmax_bf16_nhwc')


def test_symbols_exported_and_declared():
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'ctdet.h')).read()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
        assert re.search(r'\b%s\(' % name, header), name
    assert lib.ct_abi_version() == 1


def _desc(cin=64, cout=64, k=3, stride=1, pad=1, dil=1, hw=20, batch=2):
    d = _lib.ConvDesc()
    d.batch, d.cin, d.h, d.w, d.in_ctot = batch, cin, hw, hw, cin
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = cout, k, k, stride, pad, pad, dil
    d.oh = d.ow = (hw + 2 * pad - dil * (k - 1) - 1) // stride + 1
    d.out_ctot = cout
    return d


def test_supported_accepts_and_refuses():
    ok = _lib.lib().ct_conv_bf16_wino_supported
    assert ok(C.byref(_desc())) == 1
    assert ok(C.byref(_desc(cin=40, cout=130))) == 1
    assert ok(C.byref(_desc(stride=2))) == 0
    assert ok(C.byref(_desc(pad=3, dil=3))) == 0
    assert ok(C.byref(_desc(k=1, pad=0))) == 0
    assert ok(C.byref(_desc(cin=3))) == 0
    assert ok(C.byref(_desc(cin=8))) == 0            # below 16
    assert ok(C.byref(_desc(cin=20))) == 0           # no multiple of 8
    keep = torch.zeros(4)
    for field in ('res', 'lo'):
        d = _desc()
        setattr(d, field, keep.data_ptr())
        assert ok(C.byref(d)) == 0, field
    d = _desc()
    d.nseg = 1
    assert ok(C.byref(d)) == 0
    assert ok(None) == 0


def test_sizes_positive_and_monotonic():
    lib = _lib.lib()
    chans = (16, 24, 64, 72, 256, 520)
    for c in chans:
        sizes = [lib.ct_conv_bf16_wino_packed_bytes(c, m) for m in (1, 8, 33, 64, 130, 512)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0], (c, sizes)
        sizes = [lib.ct_conv_bf16_wino_packed_bytes(k, c) for k in chans]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0], (c, sizes)
        ws = [lib.ct_conv_bf16_wino_workspace_bytes(C.byref(_desc(cin=c, cout=m))) for m in (1, 8, 33, 64, 130, 512)]
        assert ws[0] > 0 and ws == sorted(ws) and ws[-1] > ws[0], (c, ws)
        ws = [lib.ct_conv_bf16_wino_workspace_bytes(C.byref(_desc(cin=k, cout=c))) for k in chans]
        assert ws[0] > 0 and ws == sorted(ws) and ws[-1] > ws[0], (c, ws)
    # V (2 bytes) and M (4 bytes) of every (tile, point), and the maxima lines
    d = _desc(cin=64, cout=64, hw=20, batch=2)
    tiles = 2 * 5 * 5
    assert lib.ct_conv_bf16_wino_workspace_bytes(C.byref(d)) >= 36 * tiles * 64 * (2 + 4) + 2 * _lib.ABSMAX_LINE_BYTES
    assert lib.ct_conv_bf16_wino_workspace_bytes(C.byref(_desc(stride=2))) == 0


class _Lib:
    """Pure host queries go to the real library; everything that would launch is logged."""

    def __init__(self, log):
        self._real, self._log = _lib.lib(), log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.endswith(('_supported', '_bytes', '_elems')) or name in ('ct_conv_mpad',):
            return fn

        def call(*args):
            self._log.append(name)
            return 0
        return call


class _Backend(HipBackendBF16):
    def __init__(self, log):
        self.device = torch.device('cpu')
        self.lib = _Lib(log)
        self.ws_pool, self.ws_generation = {}, 0
        self.slot_pool, self.slots_used = None, 0
        self.kernel_epoch = 0
        self._read_switches()

    def _stream(self):
        return None


def _step(cin, cout=64, stride=1, dil=1, hw=12):
    w = torch.nn.Parameter(torch.zeros(cout, cin, 3, 3))
    b = torch.nn.Parameter(torch.zeros(cout))
    st = ConvStep('c', [ConvPart(w, b, None, True)], cin, 3, 3, stride, dil, dil, dil, 'a', 0, hw, hw, 'b')
    bufs = {'a': torch.zeros(2, hw, hw, cin, dtype=torch.bfloat16),
            'b': torch.zeros(2, st.oh, st.ow, cout, dtype=torch.bfloat16)}
    return st, bufs


def test_switch_unset_is_todays_dispatch(monkeypatch):
    monkeypatch.delenv('CTDET_BF16_WINO', raising=False)
    monkeypatch.delenv('CTDET_BF16_WINO_MIN_CIN', raising=False)
    log = []
    be = _Backend(log)
    st, bufs = _step(512)
    be.prepare_conv(st, bufs, 2)
    assert st.rt['wino_ok'] is False
    with pytest.raises(_lib.CtdetError, match='no Winograd routing'):
        be.enable_wino(st, True)
    be.enable_wino(st, False)
    be.run_conv(st)
    assert log[-1] == 'ct_conv2d_bf16_fwd'
    assert not [n for n in log if n in NEW]
    assert be.ws_pool == {}
    assert be.policy_extra([st])['bf16_wino'] == {'switch': 'CTDET_BF16_WINO', 'on': False, 'min_cin': 512, 'max_tiles': 3200,
                                                  'layers': 0}


def test_switch_set_routes_supported_steps(monkeypatch):
    monkeypatch.setenv('CTDET_BF16_WINO', '1')
    monkeypatch.delenv('CTDET_BF16_WINO_MIN_CIN', raising=False)
    log = []
    be = _Backend(log)
    wide, wb = _step(512)
    narrow, nb = _step(256)                  # supported, below the default rule
    strided, sb = _step(512, stride=2)
    dilated, db = _step(512, dil=3)
    large, lb = _step(512, cout=8, hw=164)   # supported, more tiles (2 x 41 x 41) than the default rule takes
    for st, bufs in ((wide, wb), (narrow, nb), (strided, sb), (dilated, db), (large, lb)):
        be.prepare_conv(st, bufs, 2)
    assert [st.rt['wino_ok'] for st in (wide, narrow, strided, dilated, large)] == [True, True, False, False, True]
    assert not large.rt.get('bf16_wino')
    assert 'ct_conv_pack_weights_bf16_wino' in log
    del log[:]
    for st in (wide, narrow, strided, dilated):
        be.run_conv(st)
    assert log == ['ct_conv2d_bf16_wino_fwd', 'ct_conv2d_bf16_fwd', 'ct_conv2d_bf16_fwd', 'ct_conv2d_bf16_fwd']
    # one workspace for the route, as large as the library asks for
    assert be.ws_pool[0].numel() == be.lib.ct_conv_bf16_wino_workspace_bytes(C.byref(wide.rt['desc_w']))
    assert be.policy_extra([wide, narrow, strided, dilated])['bf16_wino']['layers'] == 1
    # by hand: onto the route, and back; an unsupported layer is refused
    be.enable_wino(narrow, True)
    be.enable_wino(wide, False)
    with pytest.raises(_lib.CtdetError, match='no bf16 Winograd path'):
        be.enable_wino(strided, True)
    del log[:]
    be.run_conv(wide)
    be.run_conv(narrow)
    assert log == ['ct_conv2d_bf16_fwd', 'ct_conv2d_bf16_wino_fwd']
    # a new parameter version re-packs both layouts of a routed layer
    with torch.no_grad():
        narrow.parts[0].weight.add_(1.0)
    assert narrow.rt['versions'] != be.param_versions(narrow)
    del log[:]
    be.pack_conv(narrow)
    assert 'ct_conv_pack_weights_bf16' in log and 'ct_conv_pack_weights_bf16_wino' in log
    assert narrow.rt['versions'] == be.param_versions(narrow)


def test_min_cin_override(monkeypatch):
    monkeypatch.setenv('CTDET_BF16_WINO', '1')
    monkeypatch.setenv('CTDET_BF16_WINO_MIN_CIN', '16')
    log = []
    be = _Backend(log)
    st, bufs = _step(40, cout=24)
    be.prepare_conv(st, bufs, 2)
    be.run_conv(st)
    assert log[-1] == 'ct_conv2d_bf16_wino_fwd'
