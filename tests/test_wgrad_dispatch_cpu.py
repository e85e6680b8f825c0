"""Which weight-gradient entry point a TrainRuntime launches for each layer (ctdet/wgrad_routes.py), without a device: the
recording library of tests/test_wgrad_h2_cpu.py (host queries go to the real libctdet, every other call is recorded instead of
run) under a hand-made plan with one layer per route, for the default environment and for each selection knob flipped once.
Per launch, in launch order: entry point, dZ, dz_ctot, dw, workspace, workspace bytes.  The lists were recorded with this
harness before the routes moved into a table; the one difference since is that a three-kernel layer no longer owns a 64-float
slice of the pre-zeroed arena (wgrad_ws_all), which it never passed to its launch."""
import types

import pytest
import torch

from ctdet import train_engine
from ctdet.engine import ConvPart, ConvStep
from test_wgrad_h2_cpu import _Backend, _Train

KNOBS = ('CTDET_WGRAD_WINO', 'CTDET_WGRAD_WINO4', 'CTDET_WGRAD_W4S_MIN_CIN', 'CTDET_TRAIN_W4S_DIL', 'CTDET_WGRAD_H2', 'CTDET_PREZERO',
         'CTDET_WGRAD_W4S_DIL_PROD', 'CTDET_WGRAD_W4S_DIL_CIN')


def _conv(name, src, dst, hw, cin, cout, k=3, stride=1, dil=1):
    w = torch.nn.Parameter(torch.zeros(cout, cin, k, k))
    b = torch.nn.Parameter(torch.zeros(cout))
    pad = dil * (k // 2)
    return ConvStep(name, [ConvPart(w, b, None, True)], cin, k, k, stride, pad, pad, dil, src, 0, hw, hw, dst, 0)


def _plan():
    """A 3x3 64 -> 64 @38 | P 1x1 64 -> 96 @38 | S 1x1 stride 2 96 -> 256 @38 | W 3x3 256 -> 512 @19 | D 3x3 dilation 2 256 -> 256
    @19 | M 3x3 64 -> 64 @10 | T 3x3 64 -> 32 @5 (M and T on inputs of their own)."""
    steps = [_conv('A', 'x', 'a', 38, 64, 64), _conv('P', 'a', 'b', 38, 64, 96, k=1), _conv('S', 'b', 'c', 38, 96, 256, k=1, stride=2),
             _conv('W', 'c', 'd', 19, 256, 512), _conv('D', 'c', 'e', 19, 256, 256, dil=2), _conv('M', 'f', 'g', 10, 64, 64),
             _conv('T', 'h', 'i', 5, 64, 32)]
    shapes = {'x': (64, 38, 38), 'a': (64, 38, 38), 'b': (96, 38, 38), 'c': (256, 19, 19), 'd': (512, 19, 19), 'e': (256, 19, 19),
              'f': (64, 10, 10), 'g': (64, 10, 10), 'h': (64, 5, 5), 'i': (32, 5, 5)}
    return types.SimpleNamespace(steps=steps, buf_shapes=shapes, ctx=False)


def _launches(monkeypatch, env):
    """(runtime, [(entry point, dz, dz_ctot, dw, workspace, workspace bytes)] in launch order) under `env`."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('CTDET_TRAIN_H2', '1')
    monkeypatch.setenv('CTDET_H2', '2')
    monkeypatch.setenv('CTDET_TRAIN_STREAMS', '1')
    monkeypatch.setenv('CTDET_STREAMS', '1')
    plan = _plan()
    monkeypatch.setattr(train_engine, 'Plan', lambda net, batch: plan)
    monkeypatch.setattr(train_engine, 'apply_tuned', lambda be, s, batch, wino4=True: True)
    log, box = [], {}

    def tensors():
        rt = box['rt']
        out = {k: getattr(rt, k) for k in ('wgrad_wsh2', 'wgrad_ws4s', 'wgrad_ws') if getattr(rt, k, None) is not None}
        out.update({'wgrad_ws.' + k: s.wgrad_ws for k, s in rt.state.items() if getattr(s, 'wgrad_ws', None) is not None})
        return out

    def names():
        if 'rt' not in box:
            return {}
        rt = box['rt']
        out = {s.dz.data_ptr(): 'dz.' + k for k, s in rt.state.items()}
        out.update({s.dw.data_ptr(): 'dw.' + k for k, s in rt.state.items()})
        out.update({t.data_ptr(): k for k, t in tensors().items()})
        return out
    rt = _Train(types.SimpleNamespace(size=300), 2, _Backend(log, names))
    box['rt'] = rt
    for s in rt.state.values():
        s.frozen = [False]
    del log[:]
    written = {}
    rt._backward_steps({}, written, lambda n, c0, c1: any(a < c1 and c0 < b for a, b in written.get(n, [])),
                       lambda prm, g: None, None, None)
    out = []
    for e in log:
        if not e[0].startswith('ct_conv2d_wgrad'):
            continue
        rest = e[6:] if e[0] == 'ct_conv2d_wgrad_h2' else e[5:]         # past dz_absmax: dw, [workspace, [bytes]], stream
        ws = rest[1] if len(rest) > 2 else None
        size = rest[2] if len(rest) > 3 else (tensors()[ws].numel() * tensors()[ws].element_size() if ws else None)
        out.append((e[0], e[2], e[3], rest[0], ws, size))
    return rt, out


DIRECT, WINO2, WINO4, WINO4S, H2 = ('ct_conv2d_wgrad', 'ct_conv2d_wgrad_wino', 'ct_conv2d_wgrad_wino4', 'ct_conv2d_wgrad_wino4s',
                                    'ct_conv2d_wgrad_h2')
WS4S, WS4S_D = 29491200, 20054016       # the three-kernel workspaces of W (the larger: shared) and of D
# backward order = reverse plan order
DEFAULT = [
    (DIRECT, 'dz.T', 32, 'dw.T', None, None),
    (WINO2, 'dz.M', 64, 'dw.M', 'wgrad_ws.M', 262144),
    (WINO4S, 'dz.D', 256, 'dw.D', 'wgrad_ws4s', WS4S),
    (WINO4S, 'dz.W', 512, 'dw.W', 'wgrad_ws4s', WS4S),
    (DIRECT, 'dz.S', 256, 'dw.S', None, None),
    (DIRECT, 'dz.P', 96, 'dw.P', None, None),
    (WINO4, 'dz.A', 64, 'dw.A', 'wgrad_ws.A', 589824),
]


def _with(base, **rows):
    return [rows.get(e[1][3:], e) for e in base]


EXPECTED = {
    '': DEFAULT,
    'CTDET_WGRAD_WINO=0': _with(DEFAULT, M=(DIRECT, 'dz.M', 64, 'dw.M', None, None), W=(DIRECT, 'dz.W', 512, 'dw.W', None, None),
                                A=(DIRECT, 'dz.A', 64, 'dw.A', None, None), D=(WINO4S, 'dz.D', 256, 'dw.D', 'wgrad_ws4s', WS4S_D)),
    'CTDET_WGRAD_WINO4=0': _with(DEFAULT, W=(WINO2, 'dz.W', 512, 'dw.W', 'wgrad_ws.W', 8388608),
                                 A=(WINO2, 'dz.A', 64, 'dw.A', 'wgrad_ws.A', 262144), D=(WINO4S, 'dz.D', 256, 'dw.D', 'wgrad_ws4s', WS4S_D)),
    'CTDET_WGRAD_W4S_MIN_CIN=0': _with(DEFAULT, D=(DIRECT, 'dz.D', 256, 'dw.D', None, None),
                                       W=(WINO4, 'dz.W', 512, 'dw.W', 'wgrad_ws.W', 18874368)),
    'CTDET_TRAIN_W4S_DIL=0': _with(DEFAULT, D=(DIRECT, 'dz.D', 256, 'dw.D', None, None),
                                   W=(WINO4S, 'dz.W', 512, 'dw.W', 'wgrad_ws4s', WS4S)),
    'CTDET_WGRAD_H2=1': _with(DEFAULT, P=(H2, 'dz.P', 96, 'dw.P', 'wgrad_wsh2', 565760)),
    'CTDET_PREZERO=0': _with(DEFAULT, M=(WINO2, 'dz.M', 64, 'dw.M', 'wgrad_ws', 589824),
                             A=(WINO4, 'dz.A', 64, 'dw.A', 'wgrad_ws', 589824)),
}
# floats of the pre-zeroed arena: every dU workspace rounded up to 64 floats
ARENA = {'': 65536 + 147456, 'CTDET_WGRAD_WINO=0': 1, 'CTDET_WGRAD_WINO4=0': 2 * 65536 + 2097152,
         'CTDET_WGRAD_W4S_MIN_CIN=0': 65536 + 147456 + 4718592, 'CTDET_TRAIN_W4S_DIL=0': 65536 + 147456,
         'CTDET_WGRAD_H2=1': 65536 + 147456}


@pytest.mark.parametrize('knob', list(EXPECTED), ids=[k or 'default' for k in EXPECTED])
def test_every_route_launches_its_entry_point(monkeypatch, knob):
    rt, got = _launches(monkeypatch, dict([knob.split('=')]) if knob else {})
    assert got == EXPECTED[knob], got
    assert {n: s.wgrad_route.name for n, s in rt.state.items()} == {
        e[1][3:]: {DIRECT: 'direct', WINO2: 'wino2', WINO4: 'wino4', WINO4S: 'wino4s', H2: 'h2'}[e[0]] for e in EXPECTED[knob]}
    if knob in ARENA:
        assert rt.wgrad_ws_all.numel() == ARENA[knob]
    else:
        assert rt.wgrad_ws_all is None
