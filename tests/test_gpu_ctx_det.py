"""ct_ctx_attention_bwd_det on the MI355X: the deterministic twin of the Context-Transformer block's backward, and the whole
phase-2 training step under CTDET_TRAIN_DETERMINISTIC=2.

  1. same numbers: every case against float64 autograd over the oracle's context_block, by the rule of
     test_gpu_ctx_train.py::test_ctx_block_backward_vs_float64_autograd (max(1e-4, 3 e32) per tensor, phi_b on the scale of dphi_w),
     under both forward operand forms;
  2. repeat equality where at least three partial sums meet at EVERY site (asserted from the size query: two terms commute): three
     calls, and a fourth beside a busy second stream, give the same bits;
  3. the workspace is not state: NaN-filled, zero-filled, and left as the previous call left it -- the same finite bits; the bytes
     behind the queried size are not touched;
  4. a NULL, misaligned or short workspace is refused;
  5. the whole step of RFBNet-300 phase 2 (bs 2) twice from the same state under level 2: every parameter gradient, the block's
     included, and every BatchNorm running statistic bit for bit; against the step with the switch unset inside the rules the
     existing tests hold a training step to.

Measured: the largest error over the tensors of all cases is 0.21 of its bound max(1e-4, 3 e32) (max|got - f64| / max|f64| =
2.1e-5: dpool of (3, 130, 260, 64, 32, True) behind the f16x2 forward; 5.6e-6 behind bf16x3).  Whole step: the block's parameters
under level 2 lie within 3.4e-7 (max|on - off| / max|off|) of the step without the switch, max|dphi.bias| / max|dphi.weight| 1e-6.

The repeat tests compare outputs only: nothing is run over and over to look for a difference, and nothing is asserted about the
plain (atomic) entry."""
import ctypes as C
import functools
import zlib

import pytest
import torch

from conftest import rel_err
import test_gpu_ctx_train as CT
import test_gpu_train_det as TD
from ctdet import _lib, engine, ops, synth, train_engine
from oracle import rfbnet_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NEW = [(2, 641, 257, 21, 20, False), (3, 700, 300, 64, 32, True)]      # B, P, M, d, T, incre; partials 6/3/6/4 and 9/3/9/6
CASES = list(CT.CASES) + NEW
CT_ERR_INVALID, CT_ERR_WORKSPACE = 1, 3


def _id(case):
    return 'x'.join(str(int(v)) for v in case)


def _query(case):
    B, P, M, d, T, incre = case
    out = (C.c_int * 4)()
    size = _lib.lib().ct_ctx_attention_bwd_det_workspace_bytes(B, P, M, d, T, int(incre), out)
    return int(size), list(out)


@functools.lru_cache(maxsize=None)
def _problem(case):
    """Inputs as test_ctx_block_backward_vs_float64_autograd draws them, the float64 gradients and the float32 autograd ones
    (computed once per case; nobody writes to them)."""
    B, P, M, d, T, incre = case
    seed = zlib.crc32(repr(case).encode()) % 10007
    g = torch.Generator().manual_seed(seed)
    conf = torch.randn(B, P, d, generator=g) * 1.5
    pool = torch.randn(B, M, d, generator=g) * 1.5
    p = CT._params(d, T, incre, seed + 1)
    R = torch.randn(B, P, (d if incre else 0) + T, generator=g)
    setting = 'incre' if incre else 'transfer'
    leaves = {k: v.double().requires_grad_(True) for k, v in p.items()}
    c64, p64 = conf.double().requires_grad_(True), pool.double().requires_grad_(True)
    (rfbnet_ref.context_block(CT._oracle_sd(leaves, incre), c64, p64, setting) * R.double()).sum().backward()
    l32 = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    c32, p32 = conf.clone().requires_grad_(True), pool.clone().requires_grad_(True)
    sd32 = CT._oracle_sd(l32, incre)
    sd32['scale'] = torch.tensor([5.0])
    (rfbnet_ref.context_block(sd32, c32, p32, setting) * R).sum().backward()
    want = dict(conf=c64.grad, pool=p64.grad, **{k: v.grad for k, v in leaves.items()})
    w32 = dict(conf=c32.grad, pool=p32.grad, **{k: v.grad for k, v in l32.items()})
    return conf, pool, p, R, want, w32


def _device_inputs(case):
    conf, pool, p, R, _, _ = _problem(case)
    pd = {k: v.to(DEV) for k, v in p.items()}
    pd['scale'] = 5.0
    return conf.to(DEV), pool.to(DEV), pd, R.to(DEV)


def _trainer(case):
    """A deterministic CtxTrainer after its forward (the backward reads the rows the forward saved)."""
    B, P, M, d, T, incre = case
    conf, pool, pd, R = _device_inputs(case)
    tr = ops.CtxTrainer(B, P, M, d, T, incre, DEV, deterministic=True)
    assert tr.bwd_entry == 'ct_ctx_attention_bwd_det' and tr.ws_bytes >= _query(case)[0]
    tr.forward(conf, pool, pd)
    return tr, conf, pool, pd, R


def _backward(tr, conf, pool, pd, R):
    dconf, dpool, grads = tr.backward(conf, pool, pd, R)
    return dict(conf=dconf.clone(), pool=dpool.clone(), **grads)


# ------------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize('fwd_form', ['f16x2', 'bf16x3'])
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_det_backward_vs_float64_autograd(case, fwd_form, monkeypatch):
    monkeypatch.setenv('CTDET_ATTN_H2', '1' if fwd_form == 'f16x2' else '0')
    want, w32 = _problem(case)[4:]
    got = {k: v.cpu() for k, v in _backward(*_trainer(case)).items()}
    assert set(got) == set(want)
    worst = (0.0, 0.0, None)
    checks = []
    for k in want:
        assert bool(torch.isfinite(got[k]).all()), k
        if k == 'phi_b':      # exactly zero in exact arithmetic (rows of dS sum to 0): judge on the scale of dphi_w
            checks.append((k, float(got[k].abs().max()), 1e-4 * float(want['phi_w'].abs().max())))
            continue
        e, e32 = rel_err(got[k], want[k].float()), rel_err(w32[k], want[k].float())
        checks.append((k, e, max(1e-4, 3 * e32)))
        worst = max(worst, (e / max(1e-4, 3 * e32), e, k))
    print('CTX-DET %s %s partials %s largest err / bound %.3g (err %.3g, %s)' % (_id(case), fwd_form, _query(case)[1], *worst))
    for k, e, bound in checks:
        assert (e <= bound) if k == 'phi_b' else (e < bound), (k, e, bound)


# ------------------------------------------------------------------------------------------------ 2. repeat equality
@pytest.mark.parametrize('case', NEW, ids=_id)
def test_det_backward_repeats_bit_for_bit(case):
    partials = _query(case)[1]
    assert partials == {NEW[0]: [6, 3, 6, 4], NEW[1]: [9, 3, 9, 6]}[case]
    assert min(partials) >= 3, partials
    args = _trainer(case)
    got = TD._repeat(lambda: _backward(*args))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert set(got) == {'conf', 'pool'} | set(args[0].keys)


# ------------------------------------------------------------------------------------------------ 3. / 4. the workspace
def _direct(tr, conf, pool, pd, R, ws_ptr, ws_bytes):
    """ct_ctx_attention_bwd_det on a caller's workspace, every output NaN before the call -> (status, outputs)."""
    prm = ops._ctx_prm(pd, tr.d, tr.T, tr.incre)
    out = dict(conf=torch.full_like(conf, TD.NAN), pool=torch.full_like(pool, TD.NAN),
               **{k: torch.full_like(pd[k], TD.NAN) for k in tr.keys})
    g = _lib.CtxGrads()
    for k in tr.keys:
        setattr(g, k, out[k].data_ptr())
    rc = _lib.lib().ct_ctx_attention_bwd_det(conf.data_ptr(), pool.data_ptr(), tr.B, tr.P, tr.M, C.byref(prm), tr.saved.data_ptr(),
                                            R.data_ptr(), out['conf'].data_ptr(), out['pool'].data_ptr(), C.byref(g), ws_ptr, ws_bytes,
                                            TD._s())
    torch.cuda.synchronize()
    return rc, out


def test_det_workspace_is_not_state():
    case = NEW[1]
    need, partials = _query(case)
    assert min(partials) >= 3
    args = _trainer(case)
    nan_ws, zero_ws = TD.Workspace(need, 0xFF), TD.Workspace(need, 0x00)
    results = []
    for ws in (nan_ws, zero_ws, zero_ws):           # the third call finds what the second left behind
        rc, out = _direct(*args, *ws.args())
        _lib.check(rc, 'ct_ctx_attention_bwd_det')
        assert ws.tail_untouched()
        results.append(out)
    for out in results:
        assert all(bool(torch.isfinite(v).all()) for v in out.values())
        TD.TK._same(results[0], out)
    TD.TK._same(results[0], _backward(*args))       # and the trainer's own (larger, uninitialised) workspace


def test_det_refuses_a_missing_misaligned_or_short_workspace():
    case = NEW[0]
    need = _query(case)[0]
    args = _trainer(case)
    ws = TD.Workspace(need + 16)
    ptr = ws.t.data_ptr()
    lib = _lib.lib()
    for ws_ptr, nbytes, word, code in ((None, need, 'workspace is null', CT_ERR_INVALID), (ptr + 4, need, 'aligned', CT_ERR_INVALID),
                                       (ptr, need - 1, 'workspace_bytes', CT_ERR_WORKSPACE)):
        rc, out = _direct(*args, ws_ptr, nbytes)
        assert rc == code, (word, rc)
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith('ct_ctx_attention_bwd_det:') and word in msg, msg
        assert all(bool(torch.isnan(v).all()) for v in out.values()), 'a refused call wrote an output'
    assert bool((ws.t[:need] == 0xFF).all()), 'a refused call wrote the workspace'
    rc, out = _direct(*args, ptr, need)
    assert rc == 0 and all(bool(torch.isfinite(v).all()) for v in out.values())


# ------------------------------------------------------------------------------------------------ 5. the whole phase-2 step
CTX_NAMES = ['theta.weight', 'theta.bias', 'phi.weight', 'phi.bias', 'g.weight', 'g.bias', 'Wz', 'OBJ_Target.weight']


def _step(net, state, x, level, monkeypatch):
    """test_gpu_train_det._step for the phase-2 network with its block: a fresh TrainRuntime on `net` restored to `state`, forward
    (use_ctx=True) + backward with fixed (seeded) upstream gradients -> (gradients by name, running statistics, policy, entries)."""
    if level:
        monkeypatch.setenv('CTDET_TRAIN_DETERMINISTIC', level)
    else:
        monkeypatch.delenv('CTDET_TRAIN_DETERMINISTIC', raising=False)
    net.load_state_dict(state)
    be = engine.HipBackend(torch.device(DEV))
    calls = be.lib = TD._Calls(be.lib)
    monkeypatch.setattr(ops, 'lib', lambda: calls)          # ops.CtxTrainer fetches its entries through ops.lib()
    rt = train_engine.TrainRuntime(net, 2, be)
    assert rt.lib is calls and rt.ctx is not None
    outs = rt.forward(x, use_ctx=True)
    g = torch.Generator().manual_seed(7)
    ups = tuple((torch.randn(o.shape, generator=g) * 1e-3).to(DEV) for o in outs)
    grads = rt.backward(*ups)
    torch.cuda.synchronize()
    names = {id(p): n for n, p in net.named_parameters()}
    out = {names[id(p)]: g.clone() for p, g in zip(rt.params, grads)}
    running = {n: b.clone() for n, b in net.named_buffers() if 'running' in n}
    return out, running, rt.policy_record(), set(calls.names)


def test_whole_phase2_step_repeats_bit_for_bit_under_level_2(monkeypatch):
    net = CT._net(300, 60, 'transfer').train()          # 60 base classes: the width the block's parameters are built for
    state = {k: v.clone() for k, v in net.state_dict().items()}
    x = synth.images(2, 300, 'randn', 1234).cuda()
    a, ra, pa, ca = _step(net, state, x, '2', monkeypatch)
    b, rb, pb, cb = _step(net, state, x, '2', monkeypatch)
    for rec in (pa, pb):
        assert rec['deterministic'] is True and rec['deterministic_ctx'] is True and rec['det_workspace_bytes']['ctx_slabs'] > 0
    for called in (ca, cb):
        assert 'ct_ctx_attention_bwd_det' in called and 'ct_ctx_attention_bwd' not in called
        assert 'ct_ctx_attention_fwd_train' in called and 'ct_ctx_pool_bwd' in called and 'ct_conv2d_wgrad_det' in called
    assert set(a) == set(b) >= {n for n, _ in net.named_parameters() if n != 'scale'}      # `scale` is not trained
    assert set(CTX_NAMES) <= set(a)
    for n in a:
        assert torch.isfinite(a[n]).all(), n
        assert torch.equal(a[n], b[n]), n
    assert ra and set(ra) == set(rb)
    for n in ra:
        assert torch.equal(ra[n], rb[n]), n
        assert not torch.equal(ra[n], state[n]), n + ' was not updated'
    # against the same step with the switch unset
    off, _, poff, coff = _step(net, state, x, None, monkeypatch)
    assert poff['deterministic'] is False and poff['deterministic_ctx'] is False
    assert 'ct_ctx_attention_bwd' in coff and not [n for n in coff if '_det' in n]
    conv = [n for n in off if n not in CTX_NAMES]
    bad = TD._outside_train_test_tolerance({n: a[n] for n in conv}, {n: off[n] for n in conv})
    errs = {n: rel_err(a[n].cpu(), off[n].cpu()) for n in CTX_NAMES if n != 'phi.bias'}
    phi_b = float(a['phi.bias'].abs().max()) / float(off['phi.weight'].abs().max())
    print('CTX-DET-STEP block parameters, max|on - off| / max|off|: %s; max|dphi.bias| / max|dphi.weight| %.3g'
          % (' '.join('%s %.3g' % kv for kv in sorted(errs.items())), phi_b))
    assert not bad, sorted(bad.items())[:12]
    for n, e in errs.items():
        assert e < 2e-3, (n, e)
    assert phi_b < 1e-3
