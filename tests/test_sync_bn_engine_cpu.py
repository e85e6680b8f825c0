"""The training engine's dispatch with synchronized BatchNorm, without a device: the shipped RFBNet-300 plan through the recording
backend of tests/train_trace.py, once as it is and once after enable_bn_sync() (a group of one rank: the collectives are no-ops,
the launches are the real sequence).  Off, nothing changes; on, every unfrozen BatchNorm part runs local -> finish -> the SAME
ct_bn_train_apply call, and local -> apply in the backward, in deterministic mode too; frozen parts keep their path."""
import os

import pytest
import torch

import train_trace as TT
from ctdet import _lib

FWD = {'ct_bn_train_stats', 'ct_bn_train_stats_det', 'ct_bn_sync_stats_local', 'ct_bn_sync_stats_finish'}
BWD = {'ct_bn_train_backward', 'ct_bn_train_backward_det', 'ct_bn_sync_backward_local', 'ct_bn_sync_backward_apply'}
GROUP = object()            # any group: torch.distributed is not initialised here, so the syncer's world is one


def _step_log(monkeypatch, sync, env=(), before=None):
    for k in [k for k in os.environ if k.startswith('CTDET_') and k != 'CTDET_LIB']:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(TT.ENVS['default'], CTDET_STREAMS='1', CTDET_TRAIN_STREAMS='1', CTDET_TUNE='0', **dict(env)).items():
        monkeypatch.setenv(k, v)
    log, box = [], {}
    net = TT._net(*TT.NETS['300p1'])
    namer = TT.Namer(lambda: TT._tensors(box), [])
    with TT._host_parameters():
        be = TT.TraceBackend(log, namer)
        box['be'] = be
        rt = TT.TraceTrain(net, TT.BATCH, be)
        box['rt'] = rt
        if sync == 'bn':
            rt.enable_bn_sync(GROUP)
        elif sync == 'grad':
            rt.enable_grad_sync()
        if before:
            before(rt)
        x = torch.zeros((TT.BATCH,) + tuple(rt.plan.buf_shapes['x']))
        del log[:]
        rt.forward(x, use_ctx=False)
        TT._walk(rt, {})
    return rt, log


def _names(log, drop=()):
    return [e[0] for e in log if e[0] not in drop]


@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'deterministic'])
def test_sync_replaces_the_statistics_and_the_backward_of_every_batchnorm_part(monkeypatch, det):
    env = {'CTDET_TRAIN_DETERMINISTIC': '1'} if det else {}
    _, off = _step_log(monkeypatch, None, env)
    rt, on = _step_log(monkeypatch, 'bn', env)
    sfx = '_det' if det else ''
    parts = sum(len(st.parts) for st, s in rt._convs() if s.is_bn)
    stages = [st for st, s in rt._convs() if s.is_bn]
    assert parts > len(stages) > 10
    n_off, n_on = _names(off), _names(on)
    assert n_off.count('ct_bn_train_stats' + sfx) == n_off.count('ct_bn_train_backward' + sfx) == parts
    assert not {n for n in n_off if 'sync' in n}
    assert not (set(n_on) & {'ct_bn_train_stats', 'ct_bn_train_stats_det', 'ct_bn_train_backward', 'ct_bn_train_backward_det'})
    for n in ('ct_bn_sync_stats_local', 'ct_bn_sync_stats_finish', 'ct_bn_sync_backward_local', 'ct_bn_sync_backward_apply'):
        assert n_on.count(n) == parts, n
    # everything else, ct_bn_train_apply included, is the same call with the same arguments in the same order
    rest = lambda log: [e for e in log if e[0] not in FWD | BWD]
    assert rest(on) == rest(off)
    # per stage: the local launches of all parts, then (the collective, then) their finish / apply launches
    assert len(rt.bn_sync.stages) == len(stages) and rt.bn_sync.arena.numel() == 4 * sum(p.cout for st in stages for p in st.parts)
    seq = [n for n in n_on if n in FWD | BWD]
    i = 0
    for st in stages:
        k = len(st.parts)
        assert seq[i:i + 2 * k] == ['ct_bn_sync_stats_local'] * k + ['ct_bn_sync_stats_finish'] * k, st.name
        i += 2 * k
    for st in reversed(stages):
        k = len(st.parts)
        assert seq[i:i + 2 * k] == ['ct_bn_sync_backward_local'] * k + ['ct_bn_sync_backward_apply'] * k, st.name
        i += 2 * k
    assert i == len(seq)
    # the count every finish / apply is given is the global batch times the map
    hw = {st.name: st.oh * st.ow for st in stages}
    counts = [e[2] for e in on if e[0] == 'ct_bn_sync_stats_finish'] + [e[-2] for e in on if e[0] == 'ct_bn_sync_backward_apply']
    want = [float(TT.BATCH * hw[st.name]) for st in stages for _ in st.parts]
    assert counts == want + [float(TT.BATCH * hw[st.name]) for st in reversed(stages) for _ in st.parts]
    # the scratch a local entry is handed is as large as the library's query asks
    lib = _lib.lib()
    for st, s in rt._convs():
        if s.is_bn:
            assert len(s.sync_scratch) == len(st.parts) and (det or not s.det_scratch)
            for p, t in zip(st.parts, s.sync_scratch):
                assert t.numel() * 8 >= lib.ct_bn_det_scratch_bytes(TT.BATCH, p.cout, st.oh * st.ow, None) > 0 and t.data_ptr() % 16 == 0


def test_world_of_one_without_a_group_is_a_no_op(monkeypatch):
    _, off = _step_log(monkeypatch, None)
    rt, on = _step_log(monkeypatch, None, before=lambda rt: rt.enable_bn_sync())
    assert rt.bn_sync is None and rt.bn_sync_scratch is None and on == off


def test_environment_switch_rides_on_enable_grad_sync(monkeypatch):
    rt, _ = _step_log(monkeypatch, 'grad')
    assert rt.bucketer is not None and rt.bn_sync is None
    calls = []
    monkeypatch.setattr(type(rt), 'enable_bn_sync', lambda self, group=None: calls.append(group))
    _step_log(monkeypatch, 'grad', {'CTDET_SYNC_BN': '1'})
    assert calls == [None]


def test_frozen_parts_keep_their_path_and_a_change_asks_for_enable_again(monkeypatch):
    net = TT._net(*TT.NETS['300p1'])
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    frozen = bns[::3]
    try:
        for m in frozen:
            m.eval()
        rt, on = _step_log(monkeypatch, 'bn')
        n_on = _names(on)
        live = len(bns) - len(frozen)
        assert n_on.count('ct_bn_eval_backward') == len(frozen)
        assert n_on.count('ct_bn_sync_stats_local') == n_on.count('ct_bn_sync_backward_apply') == live
        assert sum(len(cs) for _, cs in rt.bn_sync.stages) == live
        frozen[0].train()
        with TT._host_parameters(), pytest.raises(_lib.CtdetError, match='enable_bn_sync'):
            rt.forward(torch.zeros((TT.BATCH,) + tuple(rt.plan.buf_shapes['x'])), use_ctx=False)
    finally:
        for m in bns:
            m.train()
