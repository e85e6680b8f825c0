"""ct_ctx_attention_bwd_det without a device: the entry and its size query are exported and bound, the query follows the formulas
of include/ctdet.h (worked out again here), the entry's argument checks return before any device work, and
CTDET_TRAIN_DETERMINISTIC has two levels (1: the convolutional step, the Context-Transformer block refused; 2: the block too)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from ctdet import _lib, train_engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CT_ERR_INVALID, CT_ERR_WORKSPACE = 1, 3
QUERY, ENTRY = 'ct_ctx_attention_bwd_det_workspace_bytes', 'ct_ctx_attention_bwd_det'

# B, P, M, d, T, incre: the tables of tests/test_gpu_ctx_train.py and tests/test_gpu_ctx_det.py, the two training configurations
# (RFBNet-300 bs 32: 11 620 priors, 1 890 pooled; RFBNet-512 bs 8: 32 756 priors, 4 964 pooled), sizes on both sides of every rounding
CASES = [(2, 300, 70, 60, 20, False), (2, 257, 129, 60, 20, True), (1, 640, 33, 20, 15, False), (3, 130, 260, 64, 32, True),
         (1, 1, 1, 5, 3, False), (2, 641, 257, 21, 20, False), (3, 700, 300, 64, 32, True),
         (32, 11620, 1890, 60, 20, False), (8, 32756, 4964, 60, 20, False), (8, 32756, 4964, 15, 20, True),
         (1, 128, 128, 1, 1, False), (1, 129, 129, 64, 32, True), (1, 256, 256, 64, 1, False), (1, 257, 257, 1, 32, True),
         (64, 1024, 2048, 33, 17, False), (5, 100000, 3, 60, 20, True)]


def _ceil(a, b):
    return -(-a // b)


def _up(n, a=256):
    return _ceil(n, a) * a


def _query(*args):
    out = (C.c_int * 4)(-7, -7, -7, -7)
    return int(getattr(_lib.lib(), QUERY)(*args, out)), list(out)


def _expected(B, P, M, d, T, incre):
    """(partials, slab bytes) by the header's formulas."""
    P_pad, M_pad = _up(P, 128), _up(M, 128)
    partials = [_ceil(P_pad, 256) * B, max(1, min(P_pad // 256, _ceil(1024, (M_pad // 128) * B))), _ceil(P, 256) * B, _ceil(M, 256) * B]
    kv = partials[1] * B * M_pad * 64 * 4 if partials[1] > 1 else 0
    out = partials[0] * (T + 1) * d * 4
    lin_q, lin_k = partials[2] * (d + 1) * d * 4, partials[3] * (d + 1) * d * 4
    return partials, _up(kv) + _up(out) + (2 if incre else 1) * _up(lin_q) + 2 * _up(lin_k)


def test_exports_signatures_and_header():
    out = subprocess.run(['nm', '-D', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == 'T'}
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    for n in (QUERY, ENTRY):
        assert n in exported and n in _lib.SIGNATURES, n
        assert re.search(r'\b(int|size_t)\s+%s\s*\(' % n, header), n
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES['ct_ctx_attention_bwd']        # the arguments of the plain entry
    assert _lib.SIGNATURES[QUERY][0] is C.c_size_t and _lib.SIGNATURES[QUERY][1][-1] is C.POINTER(C.c_int)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(str(int(v)) for v in c))
def test_query_follows_the_formulas_of_the_header(case):
    B, P, M, d, T, incre = case
    size, partials = _query(B, P, M, d, T, int(incre))
    want_partials, slabs = _expected(*case)
    assert partials == want_partials
    plain = _lib.lib().ct_ctx_attention_bwd_workspace_bytes(B, P, M)
    assert plain > 0 and size == plain + slabs
    assert getattr(_lib.lib(), QUERY)(B, P, M, d, T, int(incre), None) == size         # partials may be NULL


def test_query_worked_by_hand():
    assert _query(2, 641, 257, 21, 20, 0)[1] == [6, 3, 6, 4]
    assert _query(3, 700, 300, 64, 32, 1)[1] == [9, 3, 9, 6]
    assert _query(2, 640, 257, 21, 20, 0)[1][1] == 2                # 641 is the smallest P with three key-side partials
    assert _query(1, 1, 1, 5, 3, 0)[1] == [1, 1, 1, 1]
    # the two training configurations: 46 x 32 workgroups in the output pass, kv_split 3 and 4, the ONE key-side slab area
    p300, p512 = _query(32, 11620, 1890, 60, 20, 0)[1], _query(8, 32756, 4964, 60, 20, 0)[1]
    assert p300 == [1472, 3, 1472, 256] and p512 == [1024, 4, 1024, 160]
    assert 3 * 32 * 1920 * 64 * 4 == 47185920 and 4 * 8 * 4992 * 64 * 4 == 40894464           # 47.2 MB and 40.9 MB


def test_query_refuses_sizes_the_entry_refuses():
    ok = (2, 300, 70, 60, 20, 0)
    assert _query(*ok)[0] > 0
    for i, bad in ((0, 0), (0, -1), (1, 0), (1, -5), (2, 0), (2, -1), (3, 0), (3, 65), (4, 0), (4, 33)):
        args = list(ok)
        args[i] = bad
        assert _query(*args) == (0, [0, 0, 0, 0]), args


def test_entry_refuses_before_any_device_work():
    lib = _lib.lib()
    B, P, M, d, T = 2, 641, 257, 21, 20
    need = _query(B, P, M, d, T, 0)[0]
    p = 0x10000
    prm = _lib.CtxParams()
    for f in ('theta_w', 'theta_b', 'phi_w', 'phi_b', 'g_w', 'g_b', 'wz', 'obj_w'):
        setattr(prm, f, p)
    prm.scale, prm.d, prm.t = 5.0, d, T
    g = _lib.CtxGrads()
    for f in ('theta_w', 'theta_b', 'phi_w', 'phi_b', 'g_w', 'g_b', 'wz', 'obj_w'):
        setattr(g, f, p)

    def call(conf=p, ws=p, nbytes=need, batch=B, grads=g):
        return lib.ct_ctx_attention_bwd_det(conf, p, batch, P, M, C.byref(prm), p, p, p, p, C.byref(grads), ws, nbytes, None)

    no_wz = _lib.CtxGrads()
    for f in ('theta_w', 'theta_b', 'phi_w', 'phi_b', 'g_w', 'g_b', 'obj_w'):
        setattr(no_wz, f, p)
    for kw, word, code in ((dict(ws=None), 'workspace is null', CT_ERR_INVALID), (dict(ws=p + 4), 'aligned', CT_ERR_INVALID),
                           (dict(ws=p + 8), 'aligned', CT_ERR_INVALID), (dict(nbytes=need - 1), 'workspace_bytes', CT_ERR_WORKSPACE),
                           (dict(nbytes=0), 'workspace_bytes', CT_ERR_WORKSPACE), (dict(conf=None), 'null pointer', CT_ERR_INVALID),
                           (dict(batch=0), 'bad sizes', CT_ERR_INVALID), (dict(grads=no_wz), 'null gradient buffer', CT_ERR_INVALID)):
        assert call(**kw) == code, kw
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith(ENTRY + ':') and word in msg, (kw, msg)
    # the plain entry's workspace is too small for the twin, and the plain entry names itself
    plain = lib.ct_ctx_attention_bwd_workspace_bytes(B, P, M)
    assert plain < need and call(nbytes=plain) == CT_ERR_WORKSPACE
    assert lib.ct_ctx_attention_bwd(p, p, B, P, M, C.byref(prm), p, p, p, p, C.byref(g), p, plain - 1, None) == CT_ERR_WORKSPACE
    assert lib.ct_last_error_string().decode().startswith('ct_ctx_attention_bwd:')


def test_switch_levels():
    of = train_engine.TrainSwitches.of
    for env, det, ctx in (({}, False, False), ({'CTDET_TRAIN_DETERMINISTIC': ''}, False, False),
                          ({'CTDET_TRAIN_DETERMINISTIC': '0'}, False, False), ({'CTDET_TRAIN_DETERMINISTIC': '1'}, True, False),
                          ({'CTDET_TRAIN_DETERMINISTIC': '2'}, True, True), ({'CTDET_TRAIN_DETERMINISTIC': 'yes'}, True, False)):
        s = of(env)
        assert (s.deterministic, s.deterministic_ctx) == (det, ctx), env


def _runtime(level, monkeypatch):
    """The phase-2 RFBNet-300 training runtime on the recording backend of tests/train_trace.py under the given level."""
    import train_trace as TT
    for k in [k for k in os.environ if k.startswith('CTDET_') and k != 'CTDET_LIB']:
        monkeypatch.delenv(k, raising=False)
    env = dict(TT.ENVS['default'], CTDET_STREAMS='1', CTDET_TRAIN_STREAMS='1', CTDET_TUNE='0')
    if level:
        env['CTDET_TRAIN_DETERMINISTIC'] = level
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    log, box = [], {}
    net = TT._net(*TT.NETS['300p2'])
    with TT._host_parameters():
        be = TT.TraceBackend(log, TT.Namer(lambda: TT._tensors(box), []))
        box['be'] = be
        return TT.TraceTrain(net, TT.BATCH, be)


@pytest.mark.parametrize('level', ['', '1', '2'])
def test_runtime_builds_the_block_trainer_by_level(level, monkeypatch):
    rt = _runtime(level, monkeypatch)
    ctx, rec = rt.ctx, rt.policy_record()
    assert ctx is not None
    assert rec['deterministic'] is (level != '') and rec['deterministic_ctx'] is (level == '2')
    assert ctx.deterministic is (level == '2') and ctx.bwd_entry == (ENTRY if level == '2' else 'ct_ctx_attention_bwd')
    lib = _lib.lib()
    plain = lib.ct_ctx_attention_bwd_workspace_bytes(ctx.B, ctx.P, ctx.M)
    if level == '2':
        need = _query(ctx.B, ctx.P, ctx.M, ctx.d, ctx.T, int(ctx.incre))[0]
        assert ctx.ws_bytes >= need > plain and ctx.ws.numel() == ctx.ws_bytes
        assert rec['det_workspace_bytes']['ctx_slabs'] == ctx.slab_bytes == need - plain
        assert set(rec['det_workspace_bytes']) == {'wgrad_wsdet', 'det_scratch', 'ctx_slabs'}
    else:
        assert ctx.slab_bytes == 0 and ctx.ws_bytes == max(plain, lib.ct_ctx_attention_workspace_bytes(ctx.B, ctx.P, ctx.M, ctx.d))
        assert rec['det_workspace_bytes'] is None if level == '' else set(rec['det_workspace_bytes']) == {'wgrad_wsdet', 'det_scratch'}
