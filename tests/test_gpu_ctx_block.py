"""The Context-Transformer block's kernels (csrc/ct_attn.hip, ct_attn_bwd.hip: ct_ctx_attention_fwd / _fwd_train / _bwd) against
float64 -- oracle.rfbnet_ref.context_block and float64 autograd over it -- on the case table of tests/ctx_block_cases.py: the
regimes where EVERY key carries weight (diffuse, mixed), a few peaked rows, and rows whose maximum is tied between the first and
the last key tile; both operand forms of the forward.  tests/test_ctx_block_ref_cpu.py shows on the reference alone that an
unmasked padding key, a masked valid key or a dropped query tile would move these rows by 3 ... 10 000 times the bound.

The bound is the project's flat 1e-4 on conftest.rel_err (ctx_cases.verdict, TOL of tests/test_gpu_kernels.py); the error of torch's
float32 autograd on the same inputs (e32) is reported next to every figure and bounds nothing."""
import ctypes as C

import pytest
import torch

import ctx_block_cases as cc
from conftest import rel_err
from ctdet import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4
FORMS = ['bf16x3', 'f16x2']


def _set_form(monkeypatch, form):
    monkeypatch.setenv('CTDET_ATTN_H2', '1' if form == 'f16x2' else '0')
    assert ops.lib().ct_ctx_attention_piece_products() == (3 if form == 'f16x2' else 6)


def _device_inputs(case):
    inp = cc.inputs(case)
    pd = {k: v.to(DEV) for k, v in inp.p.items()}
    pd['scale'] = 5.0
    return inp, inp.conf.to(DEV), inp.pool.to(DEV), pd


def _poison(*tensors):
    for t in tensors:
        t.view(torch.uint8).fill_(0xFF)


def _judge(case, form, key, got, want, e32):
    """One output against float64 at the flat 1e-4; prints the figure first (the table of DESIGN.md section 2 is collected from
    these lines)."""
    assert got.shape == want.shape, (case.name, form, key, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), (case.name, form, key, 'not finite')
    e = rel_err(got, want.float())
    print('CTXBLOCK %s %s %s %.3e %.3e' % (case.name, form, key, e, e32))
    assert e < TOL, (case.name, form, key, e, e32)


def _run(case, form, monkeypatch):
    """Forward and backward of one case through ops.CtxTrainer with every buffer the kernels own filled with 0xFF bytes first
    -> (out, {conf, pool, parameter names: gradient}) on the CPU ({} for a forward-only case)."""
    _set_form(monkeypatch, form)
    inp, conf, pool, pd = _device_inputs(case)
    tr = ops.CtxTrainer(case.B, case.P, case.M, case.d, case.T, case.incre, DEV)
    _poison(tr.ws, tr.saved, tr.dconf, tr.dpool)
    out = tr.forward(conf, pool, pd)
    # the training forward and the inference forward are the same kernel
    assert torch.equal(out, ops.ctx_attention(conf, pool, pd, case.incre)), (case.name, form)
    if case.fwd_only:
        return out.cpu(), {}
    # the backward may read `saved` and what it writes into its own workspace, nothing the forward left behind (include/ctdet.h)
    _poison(tr.ws, tr.dconf, tr.dpool)
    dconf, dpool, grads = tr.backward(conf, pool, pd, inp.R.to(DEV))
    return out.cpu(), dict(conf=dconf.cpu(), pool=dpool.cpu(), **{k: v.cpu() for k, v in grads.items()})


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('case', cc.by_regime('diffuse', 'mixed', 'peaked'), ids=[c.name for c in cc.by_regime('diffuse', 'mixed', 'peaked')])
def test_ctx_block_forward_and_backward_vs_float64(case, form, monkeypatch):
    ref = cc.reference(case)
    out, got = _run(case, form, monkeypatch)
    _judge(case, form, 'out', out, ref.out, ref.e32['out'])
    assert set(got) == set(ref.grads)
    for k in ref.zero if got else ():
        # exactly zero in exact arithmetic (phi_b: the rows of dS sum to 0; theta / phi with one key: the softmax is constant):
        # judged on the scale of dphi_w, or of dg_w where dphi_w is itself zero
        scale = float(ref.grads['g_w' if case.M == 1 else 'phi_w'].abs().max())
        worst = float(got[k].abs().max())
        print('CTXBLOCK %s %s %s(zero) %.3e of %.3e' % (case.name, form, k, worst, scale))
        assert bool(torch.isfinite(got[k]).all()) and worst <= TOL * scale, (case.name, form, k, worst, scale)
    for k in got:
        if k not in ref.zero:
            _judge(case, form, k, got[k], ref.grads[k], ref.e32[k])


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('case', cc.by_regime('tie'), ids=[c.name for c in cc.by_regime('tie')])
def test_ctx_block_with_the_row_maximum_tied_across_key_tiles(case, form, monkeypatch):
    ref = cc.reference(case)
    out, got = _run(case, form, monkeypatch)
    _judge(case, form, 'out', out, ref.out, ref.e32['out'])
    _judge(case, form, 'phi_w', got['phi_w'], ref.grads['phi_w'], ref.e32['phi_w'])
    _judge(case, form, 'pool', got['pool'], ref.grads['pool'], ref.e32['pool'])
    for b, pair in enumerate(ref.inp.tie):      # the two tied rows on their own scale
        rows = list(pair)
        e32 = cc.moved(cc.block(case, ref.inp.conf, ref.inp.pool, ref.inp.p, ref.inp.R, torch.float32)[1]['pool'][b, rows],
                       ref.grads['pool'][b, rows])
        _judge(case, form, 'pool[%d,%s]' % (b, rows), got['pool'][b, rows], ref.grads['pool'][b, rows], e32)


@pytest.mark.parametrize('form', FORMS)
def test_forward_of_an_image_does_not_depend_on_its_batch_mates(form, monkeypatch):
    """include/ctdet.h: the f16x2 form scales phi and g by one power of two PER IMAGE; bf16x3 has no scales at all."""
    case = next(c for c in cc.by_regime('diffuse') if c.B == 3 and c.M % 32 and c.P % 32 and c.d == 64)
    _set_form(monkeypatch, form)
    inp, conf, pool, pd = _device_inputs(case)
    pool = pool.clone()
    pool[1] *= 37.0                              # a batch-mate with another exponent
    batch = ops.ctx_attention(conf, pool, pd, case.incre)
    assert bool(torch.isfinite(batch).all())
    for i in range(case.B):
        alone = ops.ctx_attention(conf[i:i + 1].contiguous(), pool[i:i + 1].contiguous(), pd, case.incre)
        assert torch.equal(alone[0], batch[i]), (case.name, form, i, rel_err(alone[0].cpu(), batch[i].cpu()))


# ---- refusals: a non-zero status and nothing written ----
_R = cc.Case('diffuse', 2, 130, 70, 60, 20, True)
SENTINEL = -12345.0


def _refusal_setup(case=_R):
    inp, conf, pool, pd = _device_inputs(case)
    tr = ops.CtxTrainer(case.B, case.P, case.M, case.d, case.T, case.incre, DEV)
    out = torch.full((case.B, case.P, (case.d if case.incre else 0) + case.T), SENTINEL, device=DEV)
    tr.dconf.fill_(SENTINEL)
    tr.dpool.fill_(SENTINEL)
    return inp, conf, pool, pd, tr, out


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _fwd(case, prm, conf, pool, out, tr, ws_bytes=None):
    return ops.lib().ct_ctx_attention_fwd(_ptr(conf), _ptr(pool), case.B, case.P, case.M, C.byref(prm), _ptr(out), _ptr(tr.ws),
                                          tr.ws_bytes if ws_bytes is None else ws_bytes, ops._stream())


def _fwd_train(case, prm, conf, pool, out, tr, ws_bytes=None, saved_bytes=None):
    return ops.lib().ct_ctx_attention_fwd_train(_ptr(conf), _ptr(pool), case.B, case.P, case.M, C.byref(prm), _ptr(out),
                                                _ptr(tr.saved), tr.saved_bytes if saved_bytes is None else saved_bytes,
                                                _ptr(tr.ws), tr.ws_bytes if ws_bytes is None else ws_bytes, ops._stream())


def _bwd(case, prm, conf, pool, dout, tr, grads, ws_bytes=None, fc=True):
    g = _lib.CtxGrads()
    for k in tr.keys:
        if fc or k not in ('fc_w', 'fc_b'):
            setattr(g, k, grads[k].data_ptr())
    return ops.lib().ct_ctx_attention_bwd(_ptr(conf), _ptr(pool), case.B, case.P, case.M, C.byref(prm), _ptr(tr.saved), _ptr(dout),
                                          _ptr(tr.dconf), _ptr(tr.dpool), C.byref(g), _ptr(tr.ws),
                                          tr.ws_bytes if ws_bytes is None else ws_bytes, ops._stream())


def _untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool((t == SENTINEL).all()) for t in tensors)


@pytest.mark.parametrize('d,T', [(65, 20), (0, 20), (60, 33), (60, 0)])
def test_sizes_outside_the_kernels_range_are_refused(d, T):
    case = _R
    inp, conf, pool, pd, tr, out = _refusal_setup()
    prm = ops._ctx_prm(pd, d, T, case.incre)            # the real buffers, the refused sizes
    grads = {k: torch.full_like(pd[k], SENTINEL) for k in tr.keys}
    assert _fwd(case, prm, conf, pool, out, tr) != 0
    assert _fwd_train(case, prm, conf, pool, out, tr) != 0
    assert _bwd(case, prm, conf, pool, inp.R.to(DEV), tr, grads) != 0
    assert _untouched(out, tr.dconf, tr.dpool, *grads.values())


def test_buffers_one_byte_short_and_missing_fc_gradients_are_refused():
    case = _R
    inp, conf, pool, pd, tr, out = _refusal_setup()
    prm = ops._ctx_prm(pd, case.d, case.T, case.incre)
    L = ops.lib()
    fwd_need = L.ct_ctx_attention_workspace_bytes(case.B, case.P, case.M, case.d)
    bwd_need = L.ct_ctx_attention_bwd_workspace_bytes(case.B, case.P, case.M)
    grads = {k: torch.full_like(pd[k], SENTINEL) for k in tr.keys}
    assert _fwd(case, prm, conf, pool, out, tr, ws_bytes=fwd_need - 1) != 0
    assert _fwd_train(case, prm, conf, pool, out, tr, ws_bytes=fwd_need - 1) != 0
    assert _fwd_train(case, prm, conf, pool, out, tr, saved_bytes=tr.saved_bytes - 1) != 0
    assert _untouched(out)
    assert _bwd(case, prm, conf, pool, inp.R.to(DEV), tr, grads, ws_bytes=bwd_need - 1) != 0
    assert _bwd(case, prm, conf, pool, inp.R.to(DEV), tr, grads, fc=False) != 0        # 'incre' without fc_w / fc_b gradients
    assert _untouched(tr.dconf, tr.dpool, *grads.values())
    # the exact sizes are accepted
    assert _fwd_train(case, prm, conf, pool, out, tr, ws_bytes=fwd_need) == 0
    assert _bwd(case, prm, conf, pool, inp.R.to(DEV), tr, grads, ws_bytes=bwd_need) == 0
    assert not _untouched(out) and not _untouched(tr.dconf)
