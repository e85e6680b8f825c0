"""The deterministic training mode (CTDET_TRAIN_DETERMINISTIC=1) without a device: the `_det` entries of include/ctdet.h are
exported and bound, their size queries follow the formulas of the header comment (worked out again here), their argument
checks return before any device work, and a TrainRuntime under the switch calls them -- and none of them with the switch unset
(recording library as in tests/test_wgrad_dispatch_cpu.py and tests/train_trace.py: host queries go to the real libctdet, every
other call is recorded instead of run)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import test_wgrad_dispatch_cpu as WD
import train_trace as TT
from ctdet import _lib, train_engine, wgrad_routes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = ('ct_conv_wgrad_det_workspace_bytes', 'ct_conv_wgrad_wino_det_workspace_bytes', 'ct_conv_wgrad_wino4_det_workspace_bytes',
           'ct_bn_det_scratch_bytes', 'ct_bias_det_scratch_bytes', 'ct_maxpool2x2_bias_relu_bwd_det_scratch_bytes')
LAUNCHES = ('ct_conv2d_wgrad_det', 'ct_conv2d_wgrad_wino_det', 'ct_conv2d_wgrad_wino4_det', 'ct_bn_train_stats_det',
            'ct_bn_train_backward_det', 'ct_bn_eval_backward_det', 'ct_bias_act_backward_det', 'ct_maxpool2x2_bias_relu_bwd_det')
CONV = {'direct': ('ct_conv_wgrad_det_workspace_bytes', 'ct_conv2d_wgrad_det'),
        'wino2': ('ct_conv_wgrad_wino_det_workspace_bytes', 'ct_conv2d_wgrad_wino_det'),
        'wino4': ('ct_conv_wgrad_wino4_det_workspace_bytes', 'ct_conv2d_wgrad_wino4_det')}
CT_ERR_INVALID, CT_ERR_WORKSPACE, CT_ERR_UNSUPPORTED = 1, 3, 4
GIB2 = 1 << 31


def _desc(cin=64, cout=64, h=38, w=38, k=3, stride=1, pad=None, dil=1, batch=2, in_=0x10000, in_ctot=None, kw=None):
    kh, kw = k, (k if kw is None else kw)
    ph, pw = (dil * (kh // 2), dil * (kw // 2)) if pad is None else (pad, pad)
    d = _lib.ConvDesc()
    d.in_ = in_
    d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = batch, cin, h, w, in_ctot or cin, 0
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = cout, kh, kw, stride, ph, pw, dil
    d.oh = (h + 2 * ph - dil * (kh - 1) - 1) // stride + 1
    d.ow = (w + 2 * pw - dil * (kw - 1) - 1) // stride + 1
    return d


def _query(name, *args):
    n = C.c_int(-7)
    return int(getattr(_lib.lib(), name)(*args, C.byref(n))), n.value


# ------------------------------------------------------------------ exports
def test_exports_signatures_and_header():
    out = subprocess.run(['nm', '-D', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == 'T'}
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    for n in QUERIES + LAUNCHES:
        assert n in exported, n
        assert n in _lib.SIGNATURES, n
        assert re.search(r'\b(int|size_t)\s+%s\s*\(' % n, header), n
    for n in QUERIES:
        assert _lib.SIGNATURES[n][0] is C.c_size_t and _lib.SIGNATURES[n][1][-1] is C.POINTER(C.c_int), n
    # the arguments of the plain entry, with the workspace / scratch followed by its size
    for plain, det, extra in (('ct_conv2d_wgrad', 'ct_conv2d_wgrad_det', 2), ('ct_conv2d_wgrad_wino', 'ct_conv2d_wgrad_wino_det', 1),
                              ('ct_conv2d_wgrad_wino4', 'ct_conv2d_wgrad_wino4_det', 1), ('ct_bn_train_stats', 'ct_bn_train_stats_det', 1),
                              ('ct_bn_train_backward', 'ct_bn_train_backward_det', 1), ('ct_bn_eval_backward', 'ct_bn_eval_backward_det', 1),
                              ('ct_bias_act_backward_amax', 'ct_bias_act_backward_det', 2),
                              ('ct_maxpool2x2_bias_relu_bwd', 'ct_maxpool2x2_bias_relu_bwd_det', 2)):
        a, b = _lib.SIGNATURES[plain][1], _lib.SIGNATURES[det][1]
        assert len(b) == len(a) + extra and b[-1] is _lib._P and b[-2] is _lib._Z and b[-3] is _lib._P, det
    assert _lib.lib().ct_abi_version() == 1


# ------------------------------------------------------------------ the split rules of include/ctdet.h, worked out again
def _ceil(a, b):
    return -(-a // b)


def _chunks(d, launch_max):
    """Images per launch: X and dZ (dense) of one launch stay below launch_max bytes."""
    img = max(d.in_ctot * d.h * d.w * 4, d.cout * d.oh * d.ow * 4, 1)
    step = max(1, launch_max // img)
    return [min(step, d.batch - b0) for b0 in range(0, d.batch, step)]


def _direct_splits(d, nb, slots=512):
    npix, ncols = nb * d.oh * d.ow, d.cin * d.kh * d.kw
    tiles = _ceil(d.cout, 64) * _ceil(ncols, 64)
    smax = max(1, min(_ceil(npix, 256), 4 * slots // tiles))
    want, best = 1, 0.0
    for sp in range(1, smax + 1):
        fill = tiles * sp / (_ceil(tiles * sp, slots) * slots)
        if fill > best + 1e-9:
            best, want = fill, sp
        if fill >= 0.92:
            break
    blocks = _ceil(npix, 64)
    return _ceil(blocks, _ceil(blocks, want))


def _wino_splits(d, nb, tile, block, wgs):
    chunks = _ceil(nb * _ceil(d.h, tile) * _ceil(d.w, tile), 8)
    blocks = _ceil(d.cout, block) * _ceil(d.cin, block)
    want = min(65535, max(1, min(chunks, wgs // blocks)))
    return _ceil(chunks, _ceil(chunks, want))


def _expected(route, d):
    if route == 'direct':
        n = sum(_direct_splits(d, nb) for nb in _chunks(d, GIB2 - 1))
        return n, n * d.cout * d.cin * d.kh * d.kw * 4
    tile, points, block, wgs = (2, 16, 64, 256) if route == 'wino2' else (4, 36, 32, 512)
    n = sum(_wino_splits(d, nb, tile, block, wgs) for nb in _chunks(d, GIB2))
    return n, n * points * d.cout * d.cin * 4


DIRECT_DESCS = {
    'k1x1_38': dict(k=1), 'k1x1_s2': dict(k=1, stride=2, h=19, w=19), 's2': dict(stride=2, h=19, w=19, cout=40),
    'k1x3': dict(k=1, kw=3, h=12, w=11, cout=24), 'k3x1': dict(k=3, kw=1, h=12, w=11, cout=24), 'd6': dict(dil=6, h=19, w=19, cout=24),
    'generic': dict(cin=72, cout=70, h=19, w=17, batch=3), 'b4_38': dict(batch=4), 'k4x4': dict(k=4, pad=1, h=2, w=2, cout=32, batch=3),
    'wide': dict(cin=512, cout=512, h=38, w=38, batch=32), 'first': dict(cin=3, cout=64, h=300, w=300, batch=32),
    'above_2gib': dict(cin=8, cout=16, h=512, w=512, batch=3, in_ctot=704, dil=2),
}


@pytest.mark.parametrize('name', list(DIRECT_DESCS))
def test_direct_query_counts_the_launchers_splits(name, monkeypatch):
    for k in ('CTDET_WGRAD_WGS', 'CTDET_WGRAD_TB'):
        assert k not in os.environ              # read once by the library: the formulas here are the defaults'
    d = _desc(**DIRECT_DESCS[name])
    size, partials = _query(CONV['direct'][0], C.byref(d))
    assert (partials, size) == _expected('direct', d)
    assert size > 0
    if name == 'k1x1_38':
        assert partials == 12               # B 2, 64 -> 64, 1x1, 38x38: 46 blocks of 64 pixels, 4 per split
    if name == 'above_2gib':
        assert _chunks(d, GIB2 - 1) == [2, 1]       # 738 MB per image: two launches, the second appends its slabs


WINO_DESCS = {
    '64x64_19': dict(h=19, w=19), '72x130_19x17': dict(cin=72, cout=130, h=19, w=17), '32x64_38': dict(cin=32, in_ctot=48),
    'first': dict(cin=3, cout=64, h=300, w=300, batch=32), 'wide': dict(cin=512, cout=512, batch=32), 'tiny': dict(cin=8, cout=8, h=1, w=1),
    'above_2gib': dict(cin=8, cout=8, h=512, w=512, batch=3, in_ctot=704),
}


@pytest.mark.parametrize('route', ['wino2', 'wino4'])
@pytest.mark.parametrize('name', list(WINO_DESCS))
def test_wino_queries_count_the_launchers_splits(name, route):
    for k in ('CTDET_WW_WGS', 'CTDET_W4W_WGS'):
        assert k not in os.environ
    d = _desc(**WINO_DESCS[name])
    size, partials = _query(CONV[route][0], C.byref(d))
    assert (partials, size) == _expected(route, d)
    assert size > 0 and partials >= 1
    if name == 'above_2gib':
        assert _chunks(d, GIB2) == [2, 1]


@pytest.mark.parametrize('route', list(CONV))
def test_conv_queries_grow_with_batch_and_channels(route):
    k = 1 if route == 'direct' else 3
    by_batch = [_query(CONV[route][0], C.byref(_desc(batch=b, k=k)))[0] for b in (1, 2, 3, 4, 8, 16, 32, 64)]
    assert all(v > 0 for v in by_batch) and all(a <= b for a, b in zip(by_batch, by_batch[1:])) and by_batch[-1] > by_batch[0]
    by_ch = [_query(CONV[route][0], C.byref(_desc(cin=c, cout=c, k=k, batch=32, h=19, w=19)))[0] for c in (8, 16, 32, 64, 128, 256, 512, 1024)]
    assert all(v > 0 for v in by_ch) and all(a <= b for a, b in zip(by_ch, by_ch[1:])) and by_ch[-1] > by_ch[0]


def test_conv_queries_refuse_what_the_plain_entries_refuse():
    lib = _lib.lib()
    n = C.c_int(-7)
    for q, _ in CONV.values():
        assert getattr(lib, q)(None, C.byref(n)) == 0 and n.value == 0
        assert getattr(lib, q)(C.byref(_desc(batch=0)), None) == 0
    mismatch = _desc(k=1)
    mismatch.oh = 37
    for d in (_desc(k=5, pad=2), _desc(k=2, pad=0), mismatch):
        assert _query(CONV['direct'][0], C.byref(d)) == (0, 0)
    for kw in (dict(stride=2), dict(dil=2), dict(k=1), dict(pad=0)):
        d = _desc(**kw)
        assert lib.ct_conv_wgrad_wino_supported(C.byref(d)) == 0
        for route in ('wino2', 'wino4'):
            assert _query(CONV[route][0], C.byref(d)) == (0, 0), kw
    assert _query(CONV['direct'][0], C.byref(_desc(stride=2)))[0] > 0
    assert getattr(lib, CONV['direct'][0])(C.byref(_desc()), None) > 0           # partials may be NULL


def _bn_slices(b, c, hw):
    return max(1, min(_ceil(1024, c), b * hw // 2048))


def _bias_slices(b, c, hw):
    s0 = min(65535, max(1, min(_ceil(2048, c), _ceil(b * hw, 4096))))
    per = _ceil(_ceil(b * hw, s0), 4) * 4
    return _ceil(b * hw, per)


def test_reduction_queries():
    assert _query('ct_bn_det_scratch_bytes', 32, 8, 361)[1] == 5 and _query('ct_bn_det_scratch_bytes', 8, 64, 5625)[1] == 16
    shapes = [(b, c, hw) for b in (1, 2, 8, 32) for c in (1, 3, 8, 64, 126, 512, 513, 1023, 1024, 1030, 2049) for hw in (1, 25, 361, 4097, 5625)]
    for b, c, hw in shapes:
        size, partials = _query('ct_bn_det_scratch_bytes', b, c, hw)
        assert partials == _bn_slices(b, c, hw)
        assert size == 16 * max(c, min(1023 + c, c * max(1, b * hw // 2048))) and size >= partials * 2 * c * 8 > 0
        size, partials = _query('ct_bias_det_scratch_bytes', b, c, hw)
        assert partials == _bias_slices(b, c, hw)
        assert size == 8 * max(c, min(2047 + c, c * _ceil(b * hw, 4096))) and size >= partials * c * 8 > 0
        assert _query('ct_maxpool2x2_bias_relu_bwd_det_scratch_bytes', b, c) == (b * c * 8, b)
    for q in ('ct_bn_det_scratch_bytes', 'ct_bias_det_scratch_bytes'):
        for hw in (361, 5625):
            by_batch = [_query(q, b, 64, hw)[0] for b in range(1, 66)]
            by_ch = [_query(q, 8, c, hw)[0] for c in range(1, 2100)]
            assert all(a <= b for a, b in zip(by_batch, by_batch[1:])) and all(a <= b for a, b in zip(by_ch, by_ch[1:]))
            assert by_batch[0] > 0 and by_ch[0] > 0 and by_ch[-1] > by_ch[0]
        assert _query(q, 0, 8, 361) == (0, 0) and _query(q, 2, 0, 361) == (0, 0) and _query(q, 2, 8, 0) == (0, 0)
        assert getattr(_lib.lib(), q)(8, 64, 5625, None) > 0
    assert _query('ct_maxpool2x2_bias_relu_bwd_det_scratch_bytes', 0, 5) == (0, 0)


# ------------------------------------------------------------------ refusals, before any device work
@pytest.mark.parametrize('route', list(CONV))
def test_conv_entries_refuse_like_the_plain_entries(route):
    lib = _lib.lib()
    q, run = CONV[route]
    ok = _desc(k=1 if route == 'direct' else 3)
    need = _query(q, C.byref(ok))[0]

    def call(d=ok, dz=0x20000, ctot=64, coff=0, dw=0x30000, ws=0x40000, nbytes=need):
        return getattr(lib, run)(C.byref(d) if d is not None else None, dz, ctot, coff, dw, ws, nbytes, None)

    mismatch = _desc(k=1 if route == 'direct' else 3)
    mismatch.oh = 37
    bad = [
        (dict(d=None), 'd is null', CT_ERR_INVALID),
        (dict(d=_desc(in_=None)), 'd->in', CT_ERR_INVALID),
        (dict(dz=None), 'dz is null', CT_ERR_INVALID),
        (dict(dw=None), 'dw is null', CT_ERR_INVALID),
        (dict(ws=None), 'workspace is null', CT_ERR_INVALID),
        (dict(ws=0x40004), 'aligned', CT_ERR_INVALID),
        (dict(ctot=63), 'dz slice', CT_ERR_INVALID),
        (dict(nbytes=need - 1), 'workspace_bytes', CT_ERR_WORKSPACE),
        (dict(nbytes=0), 'workspace_bytes', CT_ERR_WORKSPACE),
        (dict(d=mismatch), 'oh/ow' if route == 'direct' else 'needs 3x3', CT_ERR_INVALID if route == 'direct' else CT_ERR_UNSUPPORTED),
    ]
    if route == 'direct':
        bad.append((dict(d=_desc(k=5, pad=2)), 'filters not built', CT_ERR_UNSUPPORTED))
    else:
        bad += [(dict(d=_desc(stride=2)), 'needs 3x3', CT_ERR_UNSUPPORTED), (dict(d=_desc(dil=2)), 'needs 3x3', CT_ERR_UNSUPPORTED)]
    for kw, word, code in bad:
        assert call(**kw) == code, kw
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith(run + ':') and word in msg, (kw, msg)
    # the plain entry refuses the same geometry with the same code
    plain = {'direct': None, 'wino2': lib.ct_conv2d_wgrad_wino, 'wino4': lib.ct_conv2d_wgrad_wino4}[route]
    if plain is not None:
        assert plain(C.byref(_desc(stride=2)), 0x20000, 64, 0, 0x30000, 0x40000, None) == CT_ERR_UNSUPPORTED
    else:
        assert lib.ct_conv2d_wgrad(C.byref(mismatch), 0x20000, 64, 0, 0x30000, None) == CT_ERR_INVALID


def test_reduction_entries_refuse_a_short_or_missing_scratch():
    lib = _lib.lib()
    B, Cc, HW = 8, 64, 5625
    need = _query('ct_bn_det_scratch_bytes', B, Cc, HW)[0]
    exact = 16 * 2 * Cc * 8             # 16 slices of two sums per channel
    assert need >= exact
    p = 0x10000

    def stats(scratch=p, nbytes=need, z=p):
        return lib.ct_bn_train_stats_det(z, B, Cc, 0, Cc, HW, p, p, 0.01, None, None, scratch, nbytes, None)

    def bwd(fn, scratch=p, nbytes=need):
        return fn(p, Cc, 0, p, Cc, 0, p, p, p, p, 1e-5, 1, None, 1.0, None, 0, 0, 0, p, p, p, Cc, 0, B, Cc, HW, scratch, nbytes, None)

    for name, call in (('ct_bn_train_stats_det', stats), ('ct_bn_train_backward_det', lambda **kw: bwd(lib.ct_bn_train_backward_det, **kw)),
                       ('ct_bn_eval_backward_det', lambda **kw: bwd(lib.ct_bn_eval_backward_det, **kw))):
        for kw, word, code in ((dict(scratch=None), 'scratch is null', CT_ERR_INVALID), (dict(scratch=p + 4), 'aligned', CT_ERR_INVALID),
                               (dict(nbytes=exact - 1), 'scratch_bytes', CT_ERR_WORKSPACE)):
            assert call(**kw) == code, (name, kw)
            msg = lib.ct_last_error_string().decode()
            assert msg.startswith(name + ':') and word in msg, msg
    assert stats(z=None) == CT_ERR_INVALID and lib.ct_last_error_string().decode().startswith('ct_bn_train_stats_det:')

    B, Cc, HW = 8, 3, 5625
    need = _query('ct_bias_det_scratch_bytes', B, Cc, HW)[0]

    def bias(scratch=p, nbytes=need, dy=p):
        return lib.ct_bias_act_backward_det(dy, Cc, 0, p, Cc, 0, 1, B, Cc, HW, p, Cc, 0, p, None, scratch, nbytes, None)

    def pool(scratch=p, nbytes=B * Cc * 8, oh=32):
        return lib.ct_maxpool2x2_bias_relu_bwd_det(p, Cc, 0, p, B, Cc, 64, 64, oh, 32, p, Cc, 0, p, None, scratch, nbytes, None)

    for name, call, short in (('ct_bias_act_backward_det', bias, 11 * Cc * 8 - 1), ('ct_maxpool2x2_bias_relu_bwd_det', pool, B * Cc * 8 - 1)):
        for kw, word, code in ((dict(scratch=None), 'scratch is null', CT_ERR_INVALID), (dict(nbytes=short), 'scratch_bytes', CT_ERR_WORKSPACE)):
            assert call(**kw) == code, (name, kw)
            msg = lib.ct_last_error_string().decode()
            assert msg.startswith(name + ':') and word in msg, msg
    assert bias(dy=None) == CT_ERR_INVALID and lib.ct_last_error_string().decode().startswith('ct_bias_act_backward_det:')
    assert pool(oh=40) == CT_ERR_INVALID and lib.ct_last_error_string().decode().startswith('ct_maxpool2x2_bias_relu_bwd_det:')


def test_plain_reduction_entries_report_under_their_own_name():
    """One refused call per plain entry (a null required pointer, refused before any device work): the message names the entry
    that was called.  The one exception: ct_bias_act_backward_amax reports as ct_bias_act_backward, the entry it extends."""
    lib = _lib.lib()
    B, Cc, HW, p = 8, 64, 5625, 0x10000

    def bwd(fn):
        return fn(None, Cc, 0, p, Cc, 0, p, p, p, p, 1e-5, 1, None, 1.0, None, 0, 0, 0, p, p, p, Cc, 0, B, Cc, HW, p, None)

    calls = (('ct_bn_train_stats', 'ct_bn_train_stats', lambda: lib.ct_bn_train_stats(None, B, Cc, 0, Cc, HW, p, p, 0.01, None, None, p, None)),
             ('ct_bn_train_backward', 'ct_bn_train_backward', lambda: bwd(lib.ct_bn_train_backward)),
             ('ct_bn_eval_backward', 'ct_bn_eval_backward', lambda: bwd(lib.ct_bn_eval_backward)),
             ('ct_bias_act_backward', 'ct_bias_act_backward',
              lambda: lib.ct_bias_act_backward(None, Cc, 0, p, Cc, 0, 1, B, Cc, HW, p, Cc, 0, p, None)),
             ('ct_bias_act_backward_amax', 'ct_bias_act_backward',
              lambda: lib.ct_bias_act_backward_amax(None, Cc, 0, p, Cc, 0, 1, B, Cc, HW, p, Cc, 0, p, None, None)),
             ('ct_maxpool2x2_bias_relu_bwd', 'ct_maxpool2x2_bias_relu_bwd',
              lambda: lib.ct_maxpool2x2_bias_relu_bwd(None, Cc, 0, p, B, Cc, 64, 64, 32, 32, p, Cc, 0, p, None, None)))
    for entry, name, call in calls:
        assert call() == CT_ERR_INVALID, entry
        msg = lib.ct_last_error_string().decode()
        assert msg.split(':')[0] == name, (entry, msg)


# ------------------------------------------------------------------ dispatch: the routes
TWIN = {WD.DIRECT: 'ct_conv2d_wgrad_det', WD.WINO2: 'ct_conv2d_wgrad_wino_det', WD.WINO4: 'ct_conv2d_wgrad_wino4_det'}


def test_switches_read_the_variable_once_and_default_to_off():
    of = train_engine.TrainSwitches.of
    assert of({}).deterministic is False and of({'CTDET_TRAIN_DETERMINISTIC': '0'}).deterministic is False
    assert of({'CTDET_TRAIN_DETERMINISTIC': ''}).deterministic is False and of({'CTDET_TRAIN_DETERMINISTIC': '1'}).deterministic is True
    assert set(wgrad_routes.DET_ROUTES) == {'direct', 'wino2', 'wino4'}
    assert {r.ws for r in wgrad_routes.DET_ROUTES.values()} == {'wgrad_wsdet'}
    assert not any(r.zeroed or r.dz_amax for r in wgrad_routes.DET_ROUTES.values())
    assert {r.launch for r in wgrad_routes.DET_ROUTES.values()} == set(TWIN.values())


@pytest.mark.parametrize('knob', list(WD.EXPECTED), ids=[k or 'default' for k in WD.EXPECTED])
def test_switch_maps_direct_wino2_wino4_to_their_twins(monkeypatch, knob):
    env = dict([knob.split('=')]) if knob else {}
    monkeypatch.delenv('CTDET_TRAIN_DETERMINISTIC', raising=False)
    rt_off, off = WD._launches(monkeypatch, env)
    assert off == WD.EXPECTED[knob] and not rt_off.det and rt_off.wgrad_wsdet is None and rt_off.det_scratch is None
    monkeypatch.setenv('CTDET_TRAIN_DETERMINISTIC', '1')
    rt, on = WD._launches(monkeypatch, env)
    assert rt.det and rt.policy_record()['deterministic'] is True and rt_off.policy_record()['deterministic'] is False
    lib = _lib.lib()
    needs = [int(getattr(lib, s.wgrad_route.size)(C.byref(s.wgrad), None)) for s in rt.state.values() if s.wgrad_route.name.endswith('_det')]
    assert needs and rt.wgrad_wsdet.numel() == max(needs)
    for s_on, s_off in zip(rt.state.values(), rt_off.state.values()):
        name = s_off.wgrad_route.name
        assert s_on.wgrad_route.name == (name + '_det' if name in ('direct', 'wino2', 'wino4') else name)
    assert len(on) == len(off)
    for a, b in zip(on, off):
        if b[0] in TWIN:
            assert a[:4] == (TWIN[b[0]],) + b[1:4] and a[5] == rt.wgrad_wsdet.numel(), (a, b)
        else:
            assert a == b               # wino4s and h2 have no atomics: untouched
    if rt.wgrad_ws_all is not None:     # no dU workspace is zeroed for a layer that sums slabs
        assert rt.wgrad_ws_all.numel() == 1


# ------------------------------------------------------------------ dispatch: the whole step of a shipped plan
def _step_log(net_key, deterministic, monkeypatch, use_ctx=False):
    """(runtime, names of the entries one forward + reverse walk of the shipped plan calls), as tests/train_trace.py runs it."""
    for k in [k for k in os.environ if k.startswith('CTDET_') and k != 'CTDET_LIB']:
        monkeypatch.delenv(k, raising=False)
    env = dict(TT.ENVS['default'], CTDET_STREAMS='1', CTDET_TRAIN_STREAMS='1', CTDET_TUNE='0')
    if deterministic:
        env['CTDET_TRAIN_DETERMINISTIC'] = '1'
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    log, box = [], {}
    net = TT._net(*TT.NETS[net_key])
    namer = TT.Namer(lambda: TT._tensors(box), [])
    with TT._host_parameters():
        be = TT.TraceBackend(log, namer)
        box['be'] = be
        rt = TT.TraceTrain(net, TT.BATCH, be)
        box['rt'] = rt
        x = torch.zeros((TT.BATCH,) + tuple(rt.plan.buf_shapes['x']))
        del log[:]
        rt.forward(x, use_ctx=use_ctx)
        TT._walk(rt, {})
    return rt, log


def test_step_without_the_switch_calls_no_det_entry(monkeypatch):
    rt, log = _step_log('300p1', False, monkeypatch)
    assert not [e[0] for e in log if '_det' in e[0]]
    assert rt.policy_record()['deterministic'] is False and rt.wgrad_wsdet is None and rt.det_scratch is None
    assert all(not s.det_scratch for s in rt.state.values())


def test_step_under_the_switch_calls_the_det_entries(monkeypatch):
    _, off = _step_log('300p1', False, monkeypatch)
    rt, on = _step_log('300p1', True, monkeypatch)
    assert rt.policy_record()['deterministic'] is True
    swap = {'ct_conv2d_wgrad': 'ct_conv2d_wgrad_det', 'ct_conv2d_wgrad_wino': 'ct_conv2d_wgrad_wino_det',
            'ct_conv2d_wgrad_wino4': 'ct_conv2d_wgrad_wino4_det', 'ct_bn_train_stats': 'ct_bn_train_stats_det',
            'ct_bn_train_backward': 'ct_bn_train_backward_det', 'ct_bn_eval_backward': 'ct_bn_eval_backward_det',
            'ct_bias_act_backward': 'ct_bias_act_backward_det', 'ct_bias_act_backward_amax': 'ct_bias_act_backward_det',
            'ct_maxpool2x2_bias_relu_bwd': 'ct_maxpool2x2_bias_relu_bwd_det'}
    # the same calls in the same order, each atomic site replaced by its twin
    assert [e[0] for e in on] == [swap.get(e[0], e[0]) for e in off]
    called = {e[0] for e in on}
    assert not called & set(swap), sorted(called & set(swap))
    assert called >= {'ct_conv2d_wgrad_det', 'ct_conv2d_wgrad_wino4_det', 'ct_bn_train_stats_det', 'ct_bn_train_backward_det',
                      'ct_bias_act_backward_det', 'ct_maxpool2x2_bias_relu_bwd_det', 'ct_conv2d_wgrad_wino4s'}
    # every reduction got a slice of the ONE arena, as large as its query asks, and passes its size
    lib, B = _lib.lib(), TT.BATCH
    base, end = rt.det_scratch.data_ptr(), rt.det_scratch.data_ptr() + rt.det_scratch.numel() * 8
    seen = []
    for st, s in rt._convs():
        assert len(s.det_scratch) == len(st.parts)
        for p, t in zip(st.parts, s.det_scratch):
            q = 'ct_bn_det_scratch_bytes' if s.is_bn else 'ct_bias_det_scratch_bytes'
            assert t.numel() * 8 >= getattr(lib, q)(B, p.cout, st.oh * st.ow, None) > 0
            assert base <= t.data_ptr() and t.data_ptr() + t.numel() * 8 <= end and t.data_ptr() % 16 == 0
            seen.append((t.data_ptr(), t.data_ptr() + t.numel() * 8))
    seen.sort()
    assert all(a[1] <= b[0] for a, b in zip(seen, seen[1:])), 'two reductions share scratch'
    for pr in rt._pool_bwd.values():
        assert rt.state[pr.name].det_scratch[0].numel() * 8 >= lib.ct_maxpool2x2_bias_relu_bwd_det_scratch_bytes(B, pr.cout, None)
    sizes = {(e[-3][0], e[-2]) for e in on if e[0] in ('ct_bn_train_stats_det', 'ct_bn_train_backward_det', 'ct_bias_act_backward_det',
                                                      'ct_maxpool2x2_bias_relu_bwd_det')}
    by_name = {'%s.det_scratch[%d]' % (n, i): t.numel() * 8 for n, s in rt.state.items() for i, t in enumerate(s.det_scratch)}
    assert sizes and all(by_name[n] == b for n, b in sizes), sorted(sizes)[:4]
    needs = [int(getattr(lib, s.wgrad_route.size)(C.byref(s.wgrad), None)) for s in rt.state.values() if s.wgrad_route.name.endswith('_det')]
    assert rt.wgrad_wsdet.numel() == max(needs)
    assert all(e[-2] == rt.wgrad_wsdet.numel() for e in on if e[0] in TWIN.values())


def test_context_transformer_block_is_refused_under_the_switch(monkeypatch):
    rt, _ = _step_log('300p2', True, monkeypatch)            # without the block the phase-2 plan runs
    assert rt.ctx is not None
    with pytest.raises(_lib.CtdetError, match='ct_ctx_attention_bwd'):
        rt.forward(torch.zeros((TT.BATCH,) + tuple(rt.plan.buf_shapes['x'])), use_ctx=True)
