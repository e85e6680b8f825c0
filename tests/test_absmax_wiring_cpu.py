"""Which buffers get a slot of per-image maxima (ct_conv_desc.in_absmax / out_absmax, csrc/ct_f16x2.h) and who fills it -- host
side, no device: Runtime._wire_absmax and TrainRuntime._wire_absmax (one shared rule, engine.absmax_source) against a
restatement written here, on every shipped plan and on synthetic plans that break the rule.

A slot handed to an f16x2 consumer must be an UPPER BOUND of |x| over everything the consumer reads: every step that stores into
the consumer's buffer, or into a buffer that buffer was max-pooled from, is either that pool or a convolution whose kernel
folds max |y| into the slot (FORMS[tile].tracks / the direct kernels).  Anything else and the binary16 hi pieces may overflow
silently.  The kernels' side of the promise is tests/test_gpu_absmax.py."""
import types

import pytest
import torch

from ctdet import engine, train_engine
from ctdet.engine import ConvPart, ConvStep, PoolStep
from ctdet.wino_forms import FORMS
from test_wino_dispatch_cpu import _Backend, _Train


class _Host(_Backend):
    """HipBackend without a device: the real prepare_conv (descriptors, geometry flags from the real library), CPU buffers, every
    launch and pack recorded instead of run."""
    prepare_conv = engine.HipBackend.prepare_conv

    def pack_conv(self, st, weights=True):
        pass

    def _ws_drop(self, key):
        self.ws_pool[key] = None


def _writers(steps, buf):
    """Every step that stores into `buf`, the fused pools included (a pool step stays in the plan when its producer runs it)."""
    out = []
    for st in steps:
        dsts = [sg.dst for sg in st.segs] if st.kind == 'conv' and st.segs else [st.dst]
        if buf in dsts:
            out.append(st)
    return out


def _tracks(st, is_bn=lambda st: False):
    if st.kind != 'conv' or st.segs or is_bn(st):
        return False
    f = FORMS.get(st.rt.get('wino'))
    return f.tracks if f is not None else True


def _check_wiring(steps, be, is_bn=lambda st: False):
    """-> number of consumers that read a slot.  The restatement of the rule, walked from each consumer backwards."""
    wired = 0
    convs = [st for st in steps if st.kind == 'conv']
    for st in convs:
        slot = st.rt['desc'].in_absmax
        if not be.reads_max(st):
            assert not slot, (st.name, 'a kernel that reads no maxima has a slot')
            continue
        own = getattr(FORMS.get(st.rt.get('wino')), 'own_max', False)
        assert slot or own, (st.name, 'an f16x2 kernel that cannot take the maxima itself was left without a slot')
        if not slot:
            continue
        wired += 1
        buf, chain = st.src, []
        while True:
            ws = _writers(steps, buf)
            assert ws, (st.name, buf, 'slot for a buffer nobody writes')
            chain.append(buf)
            pools = [w for w in ws if w.kind == 'pool']
            if pools:
                assert len(ws) == 1, (st.name, buf, [w.name for w in ws], 'a pooled buffer on the chain has another writer')
                buf = pools[0].src
                assert buf not in chain
                continue
            for w in ws:
                assert _tracks(w, is_bn), (st.name, buf, w.name, w.rt.get('wino'), 'writer does not fold its maxima')
                assert w.rt['desc'].out_absmax == slot, (st.name, buf, w.name, 'writer fills another slot')
            break
    slots = {}
    for st in convs:                       # the other direction: nobody fills a slot it should not, no slot serves two buffers
        out = st.rt['desc'].out_absmax
        if out:
            assert _tracks(st, is_bn), st.name
            assert slots.setdefault(out, st.dst) == st.dst, (st.name, 'one slot, two buffers')
    return wired


def _net(size, phase):
    from models.RFB_Net_vgg import build_net
    return build_net(types.SimpleNamespace(method='ours', phase=phase, setting='transfer'), size, 20).eval()


@pytest.mark.parametrize('batch', [1, 8])
@pytest.mark.parametrize('size,phase', [(300, 1), (300, 2), (512, 1), (512, 2)],
                         ids=['rfb300', 'rfb300_ctx', 'rfb512', 'rfb512_ctx'])
def test_shipped_plans_give_slots_only_to_fully_tracked_buffers(size, phase, batch, monkeypatch):
    monkeypatch.setenv('CTDET_H2', '2')                 # the f16x2 form at every batch size
    be = _Host([], lambda: {})
    rt = engine.Runtime(_net(size, phase), batch, be, tune=False)
    assert be.h2
    wired = _check_wiring(rt.plan.steps, be)
    assert wired >= 5 and len(rt.amax_slots) >= 5, (wired, len(rt.amax_slots))
    assert any(getattr(ps, 'fused_into', None) for ps in rt.plan.steps if ps.kind == 'pool')     # fused pools are on the chains


# ---- synthetic plans: conv A -> 'b' -> MaxPool2d(2, 2) -> 'p' -> f16x2 consumer C; optionally a second writer of 'p' or of 'b'
def _conv(name, src, dst, hw, cin=64, cout=64, k=3, coff=0, bn=False):
    w = torch.nn.Parameter(torch.zeros(cout, cin, k, k))
    bnm = torch.nn.BatchNorm2d(cout) if bn else None
    b = None if bn else torch.nn.Parameter(torch.zeros(cout))
    return ConvStep(name, [ConvPart(w, b, bnm, True)], cin, k, k, 1, k // 2, k // 2, 1, src, 0, hw, hw, dst, coff)


def _plan(extra):
    steps = [_conv('A', 'x', 'b', 38), PoolStep('pool', 'b', 'p', 64, 38, 38, 2, 2, 0, False)]
    if extra == 'pooled':               # a concat slice: another conv stores into the POOLED buffer
        steps.append(_conv('X', 'x2', 'p', 19, k=1))
    elif extra == 'pooled_fused':       # ... a fused F(4x4,3x3) / fp32 kernel, which does not fold its maxima
        steps.append(_conv('X4', 'x2', 'p', 19))
    elif extra == 'source':             # a non-tracking kernel stores into the pool's INPUT
        steps.append(_conv('X4', 'x', 'b', 38))
    steps.append(_conv('C', 'p', 'c', 19))
    shapes = {'x': (64, 38, 38), 'x2': (64, 19, 19), 'b': (64, 38, 38), 'p': (64, 19, 19), 'c': (64, 19, 19)}
    return types.SimpleNamespace(steps=steps, buf_shapes=shapes, ctx=False)


TILES = {'A': 44, 'C': 48, 'X4': 4}


def _tuned(be, st, batch, wino4=True):
    if st.name in TILES:
        be.enable_wino(st, tile=TILES[st.name])
    return True


@pytest.mark.parametrize('extra,wired', [(None, True), ('pooled', False), ('pooled_fused', False), ('source', False)])
def test_second_writer_on_the_pool_chain_leaves_the_consumer_without_a_slot(extra, wired, monkeypatch):
    """the wiring looked at the writers of the pool's source only.  'pooled': the other writer is a direct
    kernel that DOES track -- but into no slot of this chain, and the pooled buffer is no longer a subset of the source."""
    monkeypatch.setenv('CTDET_H2', '2')
    monkeypatch.setenv('CTDET_FUSE_POOL', '0' if extra == 'source' else '1')
    plan = _plan(extra)
    monkeypatch.setattr(engine, 'Plan', lambda net, batch: plan)
    monkeypatch.setattr(engine, 'apply_tuned', _tuned)
    be = _Host([], lambda: {})
    rt = engine.Runtime(types.SimpleNamespace(size=300), 2, be, tune=False)
    a, c = plan.steps[0], plan.steps[-1]
    if wired:
        assert c.rt['wino'] == 48 and c.rt['desc'].in_absmax and c.rt['desc'].in_absmax == a.rt['desc'].out_absmax
        assert a.rt.get('pool') is not None            # the pool runs inside A: 'p' still shares A's slot
    else:
        assert c.rt['wino'] == 46 and not c.rt['desc'].in_absmax            # the bf16x3 twin, no maxima
        assert not rt.amax_slots
    _check_wiring(plan.steps, be)


@pytest.mark.parametrize('extra,wired', [(None, True), ('pooled', False), ('pooled_fused', False), ('source', False)])
def test_training_runtime_applies_the_same_rule(extra, wired, monkeypatch):
    monkeypatch.setenv('CTDET_TRAIN_H2', '1')
    monkeypatch.setenv('CTDET_H2', '2')
    monkeypatch.setenv('CTDET_TRAIN_STREAMS', '1')
    monkeypatch.setenv('CTDET_STREAMS', '1')
    plan = _plan(extra)
    monkeypatch.setattr(train_engine, 'Plan', lambda net, batch: plan)
    monkeypatch.setattr(train_engine, 'apply_tuned', _tuned)
    be = _Backend([], lambda: {})
    rt = _Train(types.SimpleNamespace(size=300), 2, be)
    assert rt.h2
    a, c = rt.state['A'].fwd, rt.state['C'].fwd
    if wired:
        assert c.rt['wino'] == 48 and c.rt['desc'].in_absmax and c.rt['desc'].in_absmax == a.rt['desc'].out_absmax
    else:
        assert c.rt['wino'] == 46 and not c.rt['desc'].in_absmax
        assert not rt.amax_slots


def test_training_runtime_gives_no_slot_behind_a_batchnorm_layer(monkeypatch):
    """The output of a BatchNorm layer is written by ct_bn_train_apply, which folds no maxima."""
    monkeypatch.setenv('CTDET_TRAIN_H2', '1')
    monkeypatch.setenv('CTDET_H2', '2')
    monkeypatch.setenv('CTDET_TRAIN_STREAMS', '1')
    monkeypatch.setenv('CTDET_STREAMS', '1')
    plan = _plan(None)
    plan.steps[0] = _conv('A', 'x', 'b', 38, bn=True)
    monkeypatch.setattr(train_engine, 'Plan', lambda net, batch: plan)
    monkeypatch.setattr(train_engine, 'apply_tuned', _tuned)
    rt = _Train(types.SimpleNamespace(size=300), 2, _Backend([], lambda: {}))
    c = rt.state['C'].fwd
    assert c.rt['wino'] == 46 and not c.rt['desc'].in_absmax and not rt.amax_slots


def test_tuner_leaves_no_frozen_maxima_behind():
    """_time_conv froze the maxima of the data it timed on (amax_frozen) and left desc.in_absmax on them; a later
    run_conv on other data split its input by a stale exponent.  After timing, the next launch takes the maxima again.  (The
    numbers: tests/test_gpu_f16x2_range.py::test_tuner_does_not_leave_stale_maxima.)"""
    log = []
    st = _conv('c', 'a', 'b', 38)
    bufs = {'a': torch.zeros(2, 64, 38, 38), 'b': torch.zeros(2, 64, 38, 38)}
    be = _Backend(log, lambda: {})
    be.prepare_conv(st, bufs, 2)
    be.enable_wino(st, tile=48)

    class _Ev:
        def __init__(self, enable_timing=True): pass
        def record(self): pass
        def elapsed_time(self, other): return 1.0
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
        mp.setattr(torch.cuda, 'Event', _Ev)
        be._time_conv(st, iters=2, rounds=1)
    finally:
        mp.undo()
    timed = [e[0] for e in log]
    assert timed.count('ct_absmax_f32') == 1 and timed.count('ct_conv2d_wino4f_pool_fwd_v') >= 3      # one pass for all the bursts
    assert not st.rt.get('amax_frozen')
    del log[:]
    be.run_conv(st)
    assert [e[0] for e in log] == ['ct_absmax_f32', 'ct_conv2d_wino4f_pool_fwd_v']
