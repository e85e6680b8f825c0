"""Which kernel every forward and data-gradient convolution of the shipped networks runs, under the default switches and under
each CTDET_* selection switch alone (no device): the real Runtime / TrainRuntime on a host backend (the real prepare_conv and
geometry queries of libctdet, launches recorded instead of run, tests/test_absmax_wiring_cpu.py) against
tests/golden/conv_policy.json, and the pure rules of ctdet/conv_policy.py on hand-made layer records.

The fixture was recorded from the code BEFORE the rules moved into ctdet/conv_policy.py (`python tests/test_conv_policy_cpu.py
--record`, which refuses to overwrite an existing file) and is not regenerated for a refactor: a changed entry is a changed
kernel choice."""
import dataclasses
import json
import os
import sys
import types

import pytest

if __name__ == '__main__':
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
    import conftest  # noqa: F401

from ctdet import engine, train_engine
from test_absmax_wiring_cpu import _Host, _Train

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_policy.json')
# every switch that takes part in the choice (and the few that shape the descriptors it is made on): cleared before each case
SELECTION = ('CTDET_WINO', 'CTDET_X3', 'CTDET_WINO_TILES', 'CTDET_WINO_FORCE', 'CTDET_H2', 'CTDET_H2_X3', 'CTDET_CTX_TILES',
             'CTDET_CTX_F4_MAX_CIN', 'CTDET_CTX_F4_TILE', 'CTDET_CTX_W4S_MIN_CIN', 'CTDET_CTX_DIL_W4S', 'CTDET_CTX_W4F_MAX_CIN',
             'CTDET_TRAIN_H2', 'CTDET_TRAIN_WINO4', 'CTDET_TRAIN_W4S', 'CTDET_TRAIN_W4F', 'CTDET_TRAIN_W4S_DIL',
             'CTDET_TRAIN_CTX_W4F_MAX_CIN', 'CTDET_KSPLIT', 'CTDET_FORCE_KSPLIT', 'CTDET_FUSE_POOL', 'CTDET_W4_STREAMK',
             'CTDET_WGRAD_H2')
NETS = {'300p1': (300, 1), '300p2': (300, 2), '512p1': (512, 1), '512p2': (512, 2)}
# the batches the committed table serves
BATCHES = {'300p1': (2, 4, 8, 32), '300p2': (2, 4, 8, 32), '512p1': (1, 4, 32), '512p2': (1, 8, 32)}
INFER = ('', 'CTDET_H2=0', 'CTDET_H2=2', 'CTDET_H2_X3=0', 'CTDET_WINO_TILES=2,4', 'CTDET_WINO_TILES=2,4,23,44', 'CTDET_X3=0',
         'CTDET_WINO=0', 'CTDET_WINO_FORCE=23')
INFER_CTX = ('CTDET_CTX_TILES=2,23', 'CTDET_CTX_TILES=2', 'CTDET_CTX_TILES=any',
             'CTDET_CTX_TILES=2,23 CTDET_CTX_W4S_MIN_CIN=128 CTDET_CTX_F4_MAX_CIN=128',
             'CTDET_CTX_TILES=2,23 CTDET_CTX_W4S_MIN_CIN=128 CTDET_CTX_F4_MAX_CIN=128 CTDET_CTX_DIL_W4S=0',
             'CTDET_CTX_TILES=2,23 CTDET_CTX_F4_TILE=46 CTDET_CTX_F4_MAX_CIN=256', 'CTDET_CTX_W4F_MAX_CIN=128')
TRAIN = ('', 'CTDET_TRAIN_H2=0', 'CTDET_TRAIN_WINO4=0', 'CTDET_TRAIN_W4S=0', 'CTDET_TRAIN_W4F=0', 'CTDET_TRAIN_W4S_DIL=0',
         'CTDET_TRAIN_CTX_W4F_MAX_CIN=512', 'CTDET_X3=0', 'CTDET_CTX_TILES=2,23')


def _cases():
    for net in NETS:
        for batch in BATCHES[net]:
            for knobs in INFER + (INFER_CTX if net.endswith('p2') else ()):
                yield 'infer', net, batch, knobs
    for net in ('300p1', '300p2'):
        for batch in (2, 32):
            for knobs in TRAIN:
                yield 'train', net, batch, knobs


CASES = list(_cases())


def _id(case):
    return '%s-%s-b%d-%s' % (case[0], case[1], case[2], case[3] or 'default')


_nets = {}


def _net(name):
    if name not in _nets:
        from models.RFB_Net_vgg import build_net
        size, phase = NETS[name]
        _nets[name] = build_net(types.SimpleNamespace(method='ours', phase=phase, setting='transfer'), size, 20).eval()
    return _nets[name]


def _choice(be, rt):
    """What a prepared conv step launches: w<tile>, the bf16x3 / f16x2 tile name, the fp32 config name, or 'auto'."""
    if rt.get('wino'):
        return 'w%d' % rt['wino']
    if rt.get('x3') is not None:
        return be.x3_names()[rt['x3']]
    cfg = rt['desc'].config
    return be.lib.ct_conv_config_name(cfg - 1).decode() if cfg > 0 else 'auto'


def _dgrad_choice(s):
    if s.dgrad is None:
        return None
    if s.dgrad_wino is not None:
        return 'w%d' % s.dgrad_tile
    return 'x3cfg%d' % s.dgrad_x3 if s.dgrad_x3 is not None else 'direct'


def observe(case, setenv, delenv):
    """The record of one case, from what the runtimes expose: st.rt, s.dgrad_*, live_tuned, policy_record()."""
    mode, name, batch, knobs = case
    for k in SELECTION:
        delenv(k, raising=False)
    setenv('CTDET_STREAMS', '1')
    setenv('CTDET_TRAIN_STREAMS', '1')
    for kv in knobs.split():
        setenv(*kv.split('=', 1))
    be = _Host([], lambda: {})
    if mode == 'infer':
        rt = engine.Runtime(_net(name), batch, be, tune=False)
        policy = rt.policy_record()
        del policy['env']
        return {'fwd': [_choice(be, st.rt) for st in rt.conv_steps()], 'live_tuned': rt.live_tuned, 'policy': policy}
    rt = _Train(_net(name), batch, be)
    convs = [st for st in rt.plan.steps if st.kind == 'conv']
    ts = getattr(be, 'wino_tile_set', None)
    return {'fwd': [_choice(be, rt.state[st.name].fwd.rt) for st in convs],
            'dgrad': [_dgrad_choice(rt.state[st.name]) for st in convs],
            'policy': {'h2': bool(rt.h2), 'be_h2': bool(be.h2), 'h2_direct': bool(be.h2_direct),
                       'wino_tile_set': sorted(ts) if ts is not None else None}}


# ---- the fixture: {'lists': [per-layer choices in plan order, space-joined, '-' for none; each list stored once],
# 'policies': [each record stored once], 'cases': {id: record with indices into the two}}
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with open(FIXTURE) as f:
            _fixture = json.load(f)
    return _fixture


def expected(case):
    fx = fixture()
    rec = dict(fx['cases'][_id(case)])
    for k in ('fwd', 'dgrad', 'live_tuned'):
        if k in rec:
            rec[k] = [None if v == '-' else v for v in fx['lists'][rec[k]].split()]
    rec['policy'] = fx['policies'][rec['policy']]
    return rec


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_choice_matches_the_recorded_one(case, monkeypatch):
    got = observe(case, monkeypatch.setenv, monkeypatch.delenv)
    want = expected(case)
    names = [st.name for st in engine.Plan(_net(case[1]), case[2]).steps if st.kind == 'conv']
    for k in ('fwd', 'dgrad'):
        if k in want:
            assert len(got[k]) == len(want[k]) == len(names)
            diff = {n: (g, w) for n, g, w in zip(names, got[k], want[k]) if g != w}
            assert not diff, (k, '(got, recorded) per layer', diff)
    assert got == want


def test_the_fixture_holds_every_case_and_every_kernel_family():
    """So the fixture cannot pass while testing nothing: all the cases are there, and between them the recorded choices hold
    every Winograd code, a bf16x3, an f16x2 and an fp32 tile, the vector-ALU kernel, a dilated layer on its '|alt' entry, and
    among the data gradients tile 2 and the three bf16x3 configs.  A case the table serves no layer of is not counted."""
    fx = fixture()
    assert sorted(fx['cases']) == sorted(_id(c) for c in CASES)
    table = engine.tune_table()
    fwd, dgrad, alt = set(), set(), 0
    for case in CASES:
        rec = expected(case)
        steps = [st for st in engine.Plan(_net(case[1]), case[2]).steps if st.kind == 'conv']
        if case[0] == 'infer':
            assert len(rec['live_tuned']) < len(steps), _id(case)          # (every listed batch is one the table serves)
        fwd |= set(rec['fwd'])
        dgrad |= set(rec.get('dgrad', ()))
        for st, got in zip(steps, rec['fwd']):
            key = st.tune_key(case[2])
            if st.dil > 1 and table.get(key) in engine.WINO_NAME.values() and not got.startswith('w'):
                want = table[key + '|alt']
                assert got in (want, 'x3:' + want[3:], table.get(key + '|f32')), (_id(case), st.name, got, want)
                alt += got == want
    assert {'w%d' % t for t in (2, 4, 23, 44, 46, 47, 48)} <= fwd
    fp32 = {n for n in fwd if n[0].isdigit()}
    assert any(n.startswith('x3:') for n in fwd) and any(n.startswith('h2:') for n in fwd) and fp32 and 'valu' in fwd
    assert alt
    assert {'w2', 'x3cfg0', 'x3cfg1', 'x3cfg3', 'direct'} <= dgrad


def record():
    if os.path.exists(FIXTURE):
        sys.exit('%s exists: the recorded choices are not regenerated' % FIXTURE)
    lists, policies, cases = [], [], {}
    saved = dict(os.environ)

    def setenv(k, v):
        os.environ[k] = v

    def delenv(k, raising=False):
        os.environ.pop(k, None)
    for case in CASES:
        rec = observe(case, setenv, delenv)
        for k in ('fwd', 'dgrad', 'live_tuned'):
            if k in rec:
                joined = ' '.join('-' if v is None else v for v in rec[k])
                if joined not in lists:
                    lists.append(joined)
                rec[k] = lists.index(joined)
        if rec['policy'] not in policies:
            policies.append(rec['policy'])
        rec['policy'] = policies.index(rec['policy'])
        cases[_id(case)] = rec
        os.environ.clear()
        os.environ.update(saved)
    with open(FIXTURE, 'w') as f:
        def rows(items):
            return ',\n'.join(json.dumps(v, separators=(',', ':')) for v in items)
        f.write('{"lists": [\n%s\n],\n"policies": [\n%s\n],\n"cases": {\n%s\n}}\n' % (
            rows(lists), rows(policies), ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':')))
                                                    for k, v in cases.items())))


if __name__ == '__main__':
    if sys.argv[1:] == ['--record']:
        record()


# ---- the pure rules on hand-made records: no backend, no network, no library
from ctdet import conv_policy  # noqa: E402
from ctdet.conv_policy import Choice, ConvPolicy, Kernels, Layer, choose_dgrad, choose_forward, resolve  # noqa: E402

KERNELS = Kernels(direct=('64x64', '32x128', 'valu'), x3=('x3:128x128d', 'x3:64x64k32d', 'h2:128x128d'), x3_bk=(16, 32, 16),
                  x3_h2=(False, False, True))
PLAIN = dict(wino_ok=True, winox_ok=True, wino4s_ok=True, wino4f_ok=True)
NO16 = dict(wino_ok=True, winox_ok=False, wino4s_ok=False, wino4f_ok=False)       # a 3x3 layer without 16-channel chunks
DILATED = dict(wino_ok=False, winox_ok=False, wino4s_ok=True, wino4f_ok=False)
CTX = ConvPolicy(ctx_tiles='2,23', tile_set=(2, 23), f4_max_cin=128)               # round 5's accuracy policy


def _fwd(entry, policy=ConvPolicy(), cin=64, geo=PLAIN, **more):
    """choose_forward for a layer whose table entry is `entry`; more: further table entries by suffix ('|alt': ...) and Layer fields."""
    table = {'k' + k: more.pop(k) for k in [k for k in more if k.startswith('|')]}
    if entry is not None:
        table['k'] = entry
    return choose_forward(policy, table, KERNELS, Layer(key='k', cin=cin, geo=geo, **more))


def test_choose_forward_winograd_entries():
    assert _fwd(None) is None
    assert _fwd('wino4s') == Choice('wino', 44) and _fwd('wino4f') == Choice('wino', 46) and _fwd('wino') == Choice('wino', 2)
    # the f16x2 runtime: the twins of the bf16x3 forms, and the family recorded under '|h2'
    h2 = ConvPolicy(h2=True, h2_direct=True)
    assert _fwd('wino4s', h2) == Choice('wino', 47) and _fwd('wino4f', h2) == Choice('wino', 48) and _fwd('wino4', h2) == Choice('wino', 4)
    assert _fwd('wino4f', h2, **{'|h2': 'wino4s'}) == Choice('wino', 47) and _fwd('wino4f', **{'|h2': 'wino4s'}) == Choice('wino', 46)
    assert _fwd('wino4s', ConvPolicy(h2=True, tiles_env=(2, 4, 44))) == Choice('wino', 44)      # an explicit list names its twins
    # CTDET_WINO_TILES without the entry's tile: the fused fp32 F(4x4), then F(2x2)
    assert _fwd('wino4s', ConvPolicy(tiles_env=(2, 4))) == Choice('wino', 4) == _fwd('wino4f', ConvPolicy(tiles_env=(2, 4)))
    assert _fwd('wino4s', ConvPolicy(tiles_env=(2,))) == Choice('wino', 2) == _fwd('wino4', ConvPolicy(tiles_env=(2,)))
    assert _fwd('wino4s', ConvPolicy(tiles_env=(23, 44)), geo=NO16) == Choice('wino', 2)        # nothing allowed fits: F(2x2) / fp32
    # wino4=False: every F(4x4,3x3) entry runs F(2x2,3x3)
    for entry in ('wino4', 'wino4s', 'wino4f'):
        assert _fwd(entry, ConvPolicy(wino4=False)) == Choice('wino', 2)
    # CTDET_WINO=0 / a geometry without the form: the '|alt' entry, else nothing
    off = ConvPolicy(wino=False)
    assert _fwd('wino4s', off) is None and _fwd('wino4s', off, **{'|alt': '64x64'}) == Choice('direct', 1, ('wino4s',))
    assert _fwd('wino4', geo=dict(PLAIN, wino_ok=False, wino4s_ok=False), **{'|alt': '32x128'}) == Choice('direct', 2, ('wino4',))


def test_choose_forward_accuracy_policies():
    # the tile set: the most accurate allowed variant, a fused F(4x4) only on the short channel sums
    assert _fwd('wino4s', CTX, cin=256) == Choice('wino', 23) == _fwd('wino4f', CTX, cin=256) == _fwd('wino', CTX, cin=256)
    assert _fwd('wino4f', CTX, cin=128) == Choice('wino', 4) == _fwd('wino4', CTX, cin=64)
    assert _fwd('wino4s', CTX, cin=64) == Choice('wino', 23)                # a three-kernel entry is no fused one
    assert _fwd('wino4', CTX, cin=48, geo=NO16) == Choice('wino', 4) and _fwd('wino4', CTX, cin=200, geo=NO16) == Choice('wino', 2)
    f46 = dataclasses.replace(CTX, f4_tile=46, f4_max_cin=256)
    assert _fwd('wino4f', f46, cin=256) == Choice('wino', 46) == _fwd('wino4', f46, cin=64)
    assert _fwd('wino4', f46, cin=48, geo=NO16) == Choice('wino', 4)        # tile 46 needs 16-channel chunks
    assert _fwd('wino4f', dataclasses.replace(CTX, tile_set=(2,)), cin=256) == Choice('wino', 2)
    assert _fwd('wino4f', dataclasses.replace(CTX, tiles_env=(2, 23)), cin=64) == Choice('wino', 23)     # the list narrows f4 away
    w4s = dataclasses.replace(CTX, w4s_min_cin=128)
    assert _fwd('wino4f', w4s, cin=128) == Choice('wino', 44) == _fwd('wino4', w4s, cin=512)
    assert _fwd('wino', w4s, cin=512) == Choice('wino', 23)
    assert _fwd('wino4f', w4s, cin=64) == Choice('wino', 4)
    # a tile set never runs the f16x2 twins (resolve gives it h2 = False; and they are not in the set)
    assert _fwd('wino4s', dataclasses.replace(w4s, h2=True), cin=512) == Choice('wino', 44)
    # the training runtime of a network with the block: the one-accumulator fused kernel only up to w4f_max_cin channels
    cap = ConvPolicy(w4f_max_cin=128, h2=True)
    assert _fwd('wino4f', cap, cin=128) == Choice('wino', 48) and _fwd('wino4f', cap, cin=256) == Choice('wino', 47)
    assert _fwd('wino4f', dataclasses.replace(cap, h2=False), cin=256, geo=dict(PLAIN, wino4s_ok=False)) == Choice('wino', 4)
    assert _fwd('wino4f', ConvPolicy(w4f_max_cin=128, tiles_env=(2, 46)), cin=256) == Choice('wino', 2)
    assert _fwd('wino4s', cap, cin=256) == Choice('wino', 47) and _fwd('wino4f', ConvPolicy(w4f_max_cin=0), cin=512) == Choice('wino', 46)


def test_choose_forward_dilated_layers():
    """Only the three-kernel form takes them; where it may not run, the table's previous choice ('|alt')."""
    alt = {'|alt': 'x3:128x128d', '|f32': '32x128', 'dil': 2, 'geo': DILATED, 'cin': 256}
    back = Choice('x3', 0, ('wino4s',))
    assert _fwd('wino4s', **alt) == Choice('wino', 44) and _fwd('wino4s', ConvPolicy(h2=True), **alt) == Choice('wino', 47)
    assert _fwd('wino4s', ConvPolicy(tiles_env=(2, 4)), **alt) == back              # tile 44 not allowed
    assert _fwd('wino4s', ConvPolicy(wino4=False), **alt) == back                   # no F(4x4)
    assert _fwd('wino4s', ConvPolicy(wino=False), **alt) == back
    assert _fwd('wino4s', ConvPolicy(wino=False, x3=False), **alt) == Choice('direct', 2, ('wino4s', 'x3:128x128d'))
    assert _fwd('wino4s', CTX, **alt) == back                                       # an accuracy policy: from w4s_min_cin channels up
    w4s = dataclasses.replace(CTX, w4s_min_cin=128)
    assert _fwd('wino4s', w4s, **alt) == Choice('wino', 44) and _fwd('wino4s', w4s, **dict(alt, cin=64)) == back
    assert _fwd('wino4s', dataclasses.replace(w4s, dil_w4s=False), **alt) == back
    assert _fwd('wino4s', geo=dict(DILATED, wino4s_ok=False), dil=2, cin=256) is None


def test_choose_forward_direct_entries():
    h2 = ConvPolicy(h2=True, h2_direct=True)
    twin = {'|h2': 'h2:128x128d', '|f32': '64x64'}
    assert _fwd('x3:128x128d') == Choice('x3', 0) == _fwd('x3:128x128d', **twin)            # '|h2' is the f16x2 runtime's
    assert _fwd('x3:128x128d', h2, **twin) == Choice('x3', 2)
    # the h2: -> x3: -> |f32 chain
    assert _fwd('x3:128x128d', ConvPolicy(h2=True), **twin) == Choice('x3', 0, ('h2:128x128d',))
    assert _fwd('x3:128x128d', dataclasses.replace(h2, x3=False), **twin) == Choice('direct', 1, ('h2:128x128d', 'x3:128x128d'))
    assert _fwd('x3:128x128d', ConvPolicy(x3=False)) is None
    assert _fwd('x3:64x64k32d', cin=48, **{'|f32': '32x128'}) == Choice('direct', 2, ('x3:64x64k32d',))     # the k-step must divide cin
    assert _fwd('x3:64x64k32d', cin=96) == Choice('x3', 1) and _fwd('x3:128x128d', cin=8, **twin) == Choice('direct', 1, ('x3:128x128d',))
    assert _fwd('x3:256x256d') is None and _fwd('h2:64x64d', h2, **{'|f32': '64x64'}) == Choice('direct', 1, ('h2:64x64d', 'x3:64x64d'))
    assert _fwd('32x128') == Choice('direct', 2) and _fwd('96x96') is None
    # the vector-ALU kernel: the 3-channel 3x3 image layer only
    assert _fwd('valu', cin=3) == Choice('direct', 3)
    assert _fwd('valu', cin=64) is None and _fwd('valu', cin=3, kh=1, kw=1) is None and _fwd('valu', cin=3, has_res=True) is None


def _dgrad(fwd_tile, policy=ConvPolicy(), missing=(), **kw):
    kw = dict(dict(cin=64, zc=64, h=38, w=38, oh=38, ow=38, batch=2), **kw)
    asked = []

    def supported(form):
        asked.append(form)
        return form not in missing
    got = choose_dgrad(policy, Layer(**kw), fwd_tile, supported)
    assert set(asked) <= {'wino', 'wino4', 'wino4s', 'wino4f'}
    return got


def test_choose_dgrad_rungs():
    h2 = ConvPolicy(h2=True)
    # 3x3 / stride 1 / pad 1 from 19x19 maps up: F(2x2), F(4x4) where the forward launch runs one, and on the heads
    assert _dgrad(None) == (2, None) == _dgrad(2) == _dgrad(23) and _dgrad(4) == (4, None)
    assert _dgrad(4, missing=('wino4',)) == (2, None) and _dgrad(4, missing=('wino',)) == (None, 3)
    assert _dgrad(None, segs=True) == (4, None) and _dgrad(None, ConvPolicy(wino4=False), segs=True) == (2, None)
    assert _dgrad(None, segs=True, h=19, w=19, oh=19, ow=19) == (4, None)
    assert _dgrad(4, h=10, w=10, oh=10, ow=10) == (None, 3) and _dgrad(4, zc=36) == (None, None)
    # the three-kernel form where the forward launch runs it
    assert _dgrad(44) == (44, None) == _dgrad(47) and _dgrad(44, h2) == (47, None) == _dgrad(47, h2, is_bn=True)
    assert _dgrad(44, ConvPolicy(dgrad_w4s=False)) == (4, None) == _dgrad(44, missing=('wino4s',))
    # the fused bf16x3 kernel; f16x2 only where dZ's maxima exist (no BatchNorm, no head)
    assert _dgrad(46) == (46, None) == _dgrad(48) and _dgrad(46, h2) == (48, None)
    assert _dgrad(46, h2, is_bn=True) == (46, None) == _dgrad(46, h2, segs=True)
    assert _dgrad(46, ConvPolicy(dgrad_w4f=False)) == (4, None) == _dgrad(46, missing=('wino4f',))
    cap = ConvPolicy(w4f_max_cin=128)
    assert _dgrad(46, cap, zc=256) == (4, None) and _dgrad(46, cap, zc=128) == (46, None)
    # dilated layers: only behind a three-kernel forward launch
    dil = dict(dil=2, ph=2, pw=2, cin=256, zc=256)
    assert _dgrad(44, **dil) == (44, None) and _dgrad(47, h2, **dil) == (47, None)
    for pol in (ConvPolicy(dgrad_w4s=False), ConvPolicy(dgrad_w4s_dil=False)):
        assert _dgrad(44, pol, **dil) == (None, 3)
    assert _dgrad(None, **dil) == (None, 3) == _dgrad(44, missing=('wino4s',), **dil) == _dgrad(44, **dict(dil, ph=1, pw=1))
    assert _dgrad(44, **dict(dil, zc=40)) == (None, None)
    # no Winograd data gradient: bf16x3 by the size of the GEMM, the fp32 kernel where the channels do not fit
    one = dict(kh=1, kw=1, ph=0, pw=0)
    assert _dgrad(None, cin=512, batch=32, **one) == (None, 0)              # 4 x 361 tiles of 128 x 128
    assert _dgrad(None, cin=128, h=19, w=19, **one) == (None, 3) and _dgrad(None, cin=128, h=19, w=19, zc=48, **one) == (None, 1)
    assert _dgrad(None, cin=512, batch=32, h=19, w=19, **one) == (None, 1)          # 4 x 91 tiles of 128 x 128, 8 x 91 of 64 x 128
    assert _dgrad(None, ConvPolicy(x3=False), **one) == (None, None) == _dgrad(None, zc=16, **one) == _dgrad(None, zc=40, **one)
    assert _dgrad(None, stride=2, **one) == (None, 3) and _dgrad(None, stride=4, **one) == (None, None)


def test_resolve_inference_and_training():
    plain = types.SimpleNamespace(method='ours', phase=1, size=300)
    plain512 = types.SimpleNamespace(method='ours', phase=1, size=512)
    ctx = types.SimpleNamespace(method='ours', phase=2, size=300)
    assert resolve(None, None, {}) == ConvPolicy()                          # a backend no runtime has bound
    assert resolve(None, 32, {'CTDET_H2': '2'}) == ConvPolicy()
    big = ConvPolicy(h2=True, h2_direct=True)
    assert resolve(plain, 4, {}) == ConvPolicy() and resolve(plain, 8, {}) == big == resolve(plain512, 4, {}) == resolve(plain, None, {})
    assert resolve(plain, 2, {'CTDET_H2': '2'}) == big and resolve(plain, 32, {'CTDET_H2': '0'}) == ConvPolicy()
    assert resolve(plain, 32, {'CTDET_H2_X3': '0'}) == ConvPolicy(h2=True)
    env = {'CTDET_WINO': '0', 'CTDET_X3': '0', 'CTDET_WINO_TILES': '2,4,', 'CTDET_WINO_FORCE': '23', 'CTDET_CTX_TILES': '2,23',
           'CTDET_CTX_W4F_MAX_CIN': '64', 'CTDET_CTX_F4_TILE': '46', 'CTDET_CTX_DIL_W4S': '0', 'CTDET_TRAIN_H2': '0',
           'CTDET_TRAIN_WINO4': '0', 'CTDET_TRAIN_CTX_W4F_MAX_CIN': '64'}
    assert resolve(plain, 2, env) == ConvPolicy(wino=False, x3=False, tiles_env=(2, 4), force_tile=23, f4_tile=46, dil_w4s=False)
    assert resolve(plain, 2, {'CTDET_WINO_TILES': '', 'CTDET_WINO_FORCE': ''}) == ConvPolicy(tiles_env=())
    # a network with the block: the shipped 'h2', a tile set with its caps, 'any' = like every other network
    shipped = ConvPolicy(h2=True, ctx_tiles='h2')
    assert resolve(ctx, 2, {}) == shipped == resolve(ctx, 32, {'CTDET_H2_X3': '0', 'CTDET_CTX_F4_MAX_CIN': '64'})
    assert resolve(ctx, 32, {'CTDET_H2': '0'}) == ConvPolicy(ctx_tiles='h2')
    assert resolve(ctx, 32, {'CTDET_CTX_TILES': '2,23'}) == CTX
    assert resolve(ctx, 32, {'CTDET_CTX_TILES': '2', 'CTDET_CTX_F4_MAX_CIN': '0', 'CTDET_CTX_W4S_MIN_CIN': '128', 'CTDET_H2': '2'}) == \
        ConvPolicy(ctx_tiles='2', tile_set=(2,), w4s_min_cin=128)
    assert resolve(ctx, 32, {'CTDET_CTX_TILES': 'any'}) == dataclasses.replace(big, ctx_tiles='any')
    assert resolve(ctx, 2, {'CTDET_CTX_TILES': 'any'}) == ConvPolicy(ctx_tiles='any')
    assert resolve(ctx, 2, {'CTDET_CTX_W4F_MAX_CIN': '128'}) == dataclasses.replace(shipped, w4f_max_cin=128)
    assert resolve(ctx, 2, {'CTDET_CTX_W4F_MAX_CIN': ''}) == shipped
    # training: the inference batch rule for h2 and never the direct twins; no tile set whatever CTDET_CTX_TILES says; the cap
    # on the fused one-accumulator kernel only with the block
    assert resolve(plain, 32, {}, training=True) == ConvPolicy(h2=True) and resolve(plain, 2, {}, training=True) == ConvPolicy()
    for off in ('CTDET_TRAIN_H2', 'CTDET_H2'):
        assert resolve(plain, 32, {off: '0'}, training=True) == ConvPolicy()
    assert resolve(ctx, 2, {}, training=True) == ConvPolicy(h2=True, ctx_tiles='h2', w4f_max_cin=128)
    assert resolve(ctx, 32, {'CTDET_CTX_TILES': '2,23', 'CTDET_CTX_W4S_MIN_CIN': '128', 'CTDET_CTX_W4F_MAX_CIN': '64'}, training=True) == \
        ConvPolicy(ctx_tiles='2,23', w4f_max_cin=128)
    assert resolve(ctx, 32, env, training=True) == ConvPolicy(wino=False, x3=False, tiles_env=(2, 4), force_tile=23, f4_tile=46,
                                                              dil_w4s=False, ctx_tiles='2,23', w4f_max_cin=64, wino4=False)
    flags = {'CTDET_TRAIN_W4S': '0', 'CTDET_TRAIN_W4F': '0', 'CTDET_TRAIN_W4S_DIL': '0'}
    assert resolve(plain, 2, flags, training=True) == ConvPolicy(dgrad_w4s=False, dgrad_w4f=False, dgrad_w4s_dil=False)
    assert resolve(plain, 2, dict(flags, CTDET_TRAIN_WINO4='0')) == ConvPolicy()    # ... which an inference runtime does not read


def test_a_bound_backend_keeps_its_policy_and_an_unbound_one_follows_the_environment(monkeypatch):
    for k in SELECTION:
        monkeypatch.delenv(k, raising=False)
    be = _Host([], lambda: {})                      # (a test backend that does not run HipBackend.__init__)
    assert be.policy == ConvPolicy() and not be.h2 and not be.h2_direct and be.wino_tile_set is None
    monkeypatch.setenv('CTDET_WINO_TILES', '47,48')
    assert be.policy.tiles_env == (47, 48) and engine.wino_tiles(be) == (47, 48) == engine.wino_tiles()
    be.policy = CTX
    assert be.policy is CTX and be.wino_tile_set == (2, 23) == engine.wino_tiles(be)     # ... and no longer CTDET_WINO_TILES
    monkeypatch.setenv('CTDET_CTX_TILES', '2,23')
    assert engine.ctx_tile_set(types.SimpleNamespace(method='ours', phase=2)) == (2, 23) and engine.ctx_f4_tile() == 4
    assert _Host([], lambda: {}).policy.tile_set is None


def test_the_engines_read_no_selection_variable_themselves():
    """resolve() is the only reader: a switch read in the middle of a decision is how the training runtime came to ignore
    CTDET_CTX_TILES by a missing assignment."""
    names = SELECTION[:SELECTION.index('CTDET_KSPLIT')]
    for mod in (engine, train_engine):
        with open(mod.__file__) as f:
            src = f.read()
        assert not [k for k in names if "'%s'" % k in src], mod.__name__
    with open(conv_policy.__file__) as f:
        src = f.read()
    assert all("'%s'" % k in src for k in names) and 'environ' not in src
