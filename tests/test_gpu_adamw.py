"""The fused AdamW step on the MI355X: ct_adamw_begin, ct_adamw_step and ctdet.optim.FusedAdamW.

Yardsticks, never the code under test: tests/adamw_ref.py (the two entries in NumPy float32, bit for bit, and AdamW's
definition in float64 for the accuracy rule of tests/sgd_ref.py::close_to_torch), tests/ema_ref.py (the averaging
line) and tests/clip_ref.py (the clipping coefficient, evaluated from the device's own norm as in
tests/test_gpu_grad_clip.py).  Tensors are views into flat buffers with NaN between the views, and whole buffers are
compared, so an access outside a view shows."""
import copy
import ctypes as C
import types

import numpy as np
import pytest
import torch

import adamw_ref
import clip_ref
import ema_ref
import sgd_ref
from ctdet import _lib, ops, synth
from ctdet.optim import FusedAdamW, WeightEMA

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
GAP = 9                                      # sentinel elements between two views (and before the first, after the last)
P, G, M, V, E = range(5)                     # the five arrays of a step: param, grad, exp_avg, exp_avg_sq, average
B1, B2, EPS = 0.9, 0.999, 1e-8


def layout(sizes, offs):
    """First element of each view in a flat buffer: `off` elements past a 16-byte line, GAP or more apart."""
    starts, cur = [], 0
    for n, off in zip(sizes, offs):
        s = (cur + GAP + 3) // 4 * 4 + off
        starts.append(s)
        cur = s + n
    return starts, cur + GAP + 4


class Arena:
    """(param, grad, exp_avg, exp_avg_sq, ema) views into five flat device buffers, NaN sentinels between the views, one
    ct_adam_state per tensor, and the host's expected image of each WHOLE buffer and of every record.
    offs[i] = the five line offsets of tensor i."""

    def __init__(self, sizes, offs, seed, steps=None):
        self.sizes = list(sizes)
        n = len(self.sizes)
        self.rng = rng = np.random.RandomState(seed)
        self.starts, totals = zip(*[layout(sizes, [o[r] for o in offs]) for r in range(5)])
        self.host = [np.full(t, np.nan, F32) for t in totals]
        for i, k in enumerate(sizes):
            self.view(P, i, False)[:] = (rng.randn(k) * 0.25).astype(F32)
            self.view(G, i, False)[:] = adamw_ref.grads_like(rng, k)
            self.view(M, i, False)[:] = 0.0
            self.view(V, i, False)[:] = 0.0
            self.view(E, i, False)[:] = rng.randn(k).astype(F32)
        self.dev = [torch.from_numpy(h).to(DEV) for h in self.host]
        assert all(d.data_ptr() % 16 == 0 for d in self.dev)
        self.ref = [adamw_ref.loaded(s, (B1, B2)) for s in (steps or [0] * n)]
        self.states = torch.zeros(n * ops.ADAM_STATE_BYTES, device=DEV, dtype=torch.uint8)
        if steps:
            ops.adam_states_write(self.states, records_of(self.ref))
        self.flag = False

    def view(self, r, i, dev=True):
        s = self.starts[r][i]
        return (self.dev[r] if dev else self.host[r])[s:s + self.sizes[i]]

    def set_grads(self, make):
        for i, k in enumerate(self.sizes):
            self.view(G, i, False)[:] = make(self.rng, k)
        self.dev[G].copy_(torch.from_numpy(self.host[G]))

    def items(self, lrs, wds, ema=False, which=None):
        idx = range(len(self.sizes)) if which is None else which
        return [(self.view(P, i), self.view(G, i), self.view(M, i), self.view(V, i), i, lrs[i], wds[i]) +
                ((self.view(E, i),) if ema else ()) for i in idx]

    def run(self, lrs, wds, grad_scale=1.0, ema_state=None, clip=None, which=None, betas=(B1, B2)):
        """ops.adamw_begin + ops.adamw_step over `which` (all)."""
        idx = list(range(len(self.sizes)) if which is None else which)
        ops.adamw_begin(self.states, idx, betas[0], betas[1], clip_state=clip)
        ops.adamw_step(self.items(lrs, wds, ema_state is not None, idx), betas[0], betas[1], EPS, grad_scale, self.states,
                       ema_state=ema_state, clip_state=clip)

    def expect(self, lrs, wds, grad_scale=1.0, ema_ref_state=None, which=None, betas=(B1, B2)):
        """The restatement of run(), written into the host images."""
        for i in (range(len(self.sizes)) if which is None else which):
            adamw_ref.begin(self.ref[i], betas[0], betas[1])
            p, m, v, flag = adamw_ref.step(self.view(P, i, False), self.view(G, i, False), self.view(M, i, False),
                                           self.view(V, i, False), self.ref[i], lrs[i], wds[i], betas[0], betas[1], EPS,
                                           grad_scale)
            self.flag = self.flag or flag
            self.view(P, i, False)[:], self.view(M, i, False)[:], self.view(V, i, False)[:] = p, m, v
            if ema_ref_state is not None:
                self.view(E, i, False)[:] = ema_ref.update(self.view(E, i, False), p, ema_ref_state)

    def same_bits(self, other=None):
        want = self.host if other is None else [d.cpu().numpy() for d in other.dev]
        return [sgd_ref.bits_equal(self.dev[r].cpu().numpy(), want[r]) for r in range(5)]

    def same_records(self, other=None):
        want = records_of(self.ref) if other is None else ops.adam_states_read(other.states)
        return ops.adam_states_read(self.states).tobytes() == want.tobytes()


def records_of(refs):
    """adamw_ref.State objects -> the packed array ops.adam_states_write takes."""
    out = np.zeros(len(refs), ops.ADAM_STATE_DTYPE)
    for k, s in enumerate(refs):
        out[k] = (s.beta1_pow, s.beta2_pow, s.step, s.applied, s.bc1, s.rs2)
    return out


def new_ema_state():
    return torch.zeros(ops.EMA_STATE_BYTES, device=DEV, dtype=torch.uint8)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _launch_names(fn):
    lib = _lib.lib()
    torch.cuda.synchronize()
    lib.ct_profile_enable(1)
    try:
        fn()
        n = C.c_int(0)
        recs = (_lib.ProfileRecord * 256)()
        _lib.check(lib.ct_profile_collect(recs, 256, C.byref(n)), 'ct_profile_collect')
    finally:
        lib.ct_profile_enable(0)
    return [recs[i].name.decode() for i in range(min(n.value, 256))]


# 1 -----------------------------------------------------------------------------------------------------------------
# Around the chunk of 8192 elements a workgroup owns: one chunk at any offset (8188), one that its shift pushes into a
# second chunk (8189 at 3, 8192 at 1..3), a last chunk of one element (8193 at 0), a whole middle chunk (16391 at 1..3).
SIZES = [1, 3, 4, 5, 1023, 8188, 8189, 8192, 8193, 16391]


def _walk_arena(seed):
    """Every size with all five arrays at the line offsets 0..3 (the vector walk, partial first and last group), and
    once more with one of the arrays one element further (the dword walk): 50 tensors."""
    sizes = [n for n in SIZES for _ in range(5)]
    offs = []
    for k, _ in enumerate(SIZES):
        odd = [k % 4] * 5
        odd[k % 5] = (k + 1) % 4
        offs += [(o,) * 5 for o in range(4)] + [tuple(odd)]
    return Arena(sizes, offs, seed)


@pytest.mark.parametrize('ema', [False, True])
@pytest.mark.parametrize('grad_scale', [1.0, 0.125])
@pytest.mark.parametrize('wd', [0.0, 5e-4])
def test_bit_exact_against_the_restatement(wd, grad_scale, ema):
    a = _walk_arena(41)
    n = len(a.sizes)
    lrs = [1e-3 * (1 + i % 7) for i in range(n)]
    wds = [0.0 if i % 3 == 0 else wd for i in range(n)]
    state, ref = (new_ema_state(), ema_ref.State()) if ema else (None, None)
    for it in range(4):
        if it:
            a.set_grads(adamw_ref.grads_like)
        assert any((a.view(G, i, False) == 0).any() for i in range(n))
        if ema:
            ops.ema_begin(state, 0.9998, 10.0)
            ema_ref.begin(ref, 0.9998, 10.0)
        if it == 2:                                     # one call per tensor
            for i in range(n):
                a.run(lrs, wds, grad_scale, state, which=[i])
        else:
            a.run(lrs, wds, grad_scale, state)
        a.expect(lrs, wds, grad_scale, ref)
        assert not a.flag, 'a subnormal intermediate: the inputs are outside the bit-for-bit claim'
        assert a.same_records(), 'step %d: records' % it
        got = a.same_bits()
        assert got[:4] == [True] * 4, 'step %d: (param, grad, exp_avg, exp_avg_sq) %s, sentinels included' % (it, got)
        assert got[E], 'step %d: the average (without ema: untouched)' % it
    assert all(s.step == 4 for s in a.ref)


# 2 -----------------------------------------------------------------------------------------------------------------
EXTREMES = np.array([1e-30, -1e-30, 1e20, -1e20, np.inf, np.nan], F32)


def _extreme_grads(rng, k):
    g = adamw_ref.grads_like(rng, k)
    hit = rng.rand(k) < 0.5
    g[hit] = EXTREMES[rng.randint(0, len(EXTREMES), int(hit.sum()))]
    return g


@pytest.mark.parametrize('ema', [False, True])
def test_extreme_gradients_are_bit_exact_too(ema):
    """Without the guard non-finite gradients propagate as the lines say.  (om2 * g) * g of +-1e-30 is exactly zero and
    of +-1e20 about 1e37: no intermediate is subnormal, so the bit-for-bit claim covers these inputs."""
    sizes = [6, 61, 4099, 8193]
    a = Arena(sizes, [(i % 4,) * 5 for i in range(4)], 43)
    lrs, wds = [1e-3, 2e-3, 4e-3, 1e-3], [5e-4, 0.0, 1e-2, 5e-4]
    state, ref = (new_ema_state(), ema_ref.State()) if ema else (None, None)
    for it in range(3):
        a.set_grads(_extreme_grads)
        if it == 0:
            a.view(G, 0, False)[:] = EXTREMES                   # each of them at least once
            a.dev[G].copy_(torch.from_numpy(a.host[G]))
        if ema:
            ops.ema_begin(state, 0.9, 0.0)
            ema_ref.begin(ref, 0.9, 0.0)
        a.run(lrs, wds, 1.0, state)
        a.expect(lrs, wds, 1.0, ref)
        assert not a.flag
        assert a.same_bits() == [True] * 5 and a.same_records(), 'step %d' % it
    p = a.view(P, 3, False)
    assert np.isnan(p).any() and np.isfinite(p).any()


# 3 -----------------------------------------------------------------------------------------------------------------
LIMITS = [(1, -1), (1, 0), (1, 1), (2, 1)]       # cap - 1, cap, cap + 1 and 2 cap + 1 entries


def _cap():
    return _lib.lib().ct_adamw_tensors_per_launch()


@pytest.mark.parametrize('caps,more', LIMITS)
@pytest.mark.parametrize('ema', [False, True])
def test_table_limits(caps, more, ema):
    cap = _cap()
    assert 50 <= cap <= 63
    count = caps * cap + more
    sizes = [1 + i % 7 for i in range(count)]
    a = Arena(sizes, [(i % 4,) * 5 for i in range(count)], 47, steps=[(3 * i) % 11 for i in range(count)])
    lrs, wds = [1e-3 * (1 + i % 3) for i in range(count)], [5e-4] * count
    state, ref = (new_ema_state(), ema_ref.State()) if ema else (None, None)
    empty = (torch.empty(0, device=DEV),) * 4 + (0, 1e-3, 0.0) + ((torch.empty(0, device=DEV),) if ema else ())
    for it in range(3):
        which = [i for i in range(count) if it == 0 or i % 5 != it]        # a subset gets no gradient in some steps
        a.set_grads(adamw_ref.grads_like)
        if ema:
            ops.ema_begin(state, 0.9998, 10.0)
            ema_ref.begin(ref, 0.9998, 10.0)
        ops.adamw_begin(a.states, which, B1, B2)
        items = a.items(lrs, wds, ema, which)
        items.insert(len(items) // 2, empty)                                # empty tensors take no slot of a launch
        items.append(empty)
        names = _launch_names(lambda: ops.adamw_step(items, B1, B2, EPS, 1.0, a.states, ema_state=state))
        assert names == ['adamw_multi_kernel_ema' if ema else 'adamw_multi_kernel'] * -(-len(which) // cap), (it, names)
        a.expect(lrs, wds, 1.0, ref, which)
        assert a.same_bits() == [True] * 5 and a.same_records(), 'step %d' % it
    assert not a.flag
    assert sorted({s.step for s in a.ref})[0] >= 2 and len({s.step for s in a.ref}) > 3


@pytest.mark.parametrize('caps,more', LIMITS)
def test_begin_capacity(caps, more):
    cap = _lib.lib().ct_adamw_begin_indices_per_launch()
    assert cap >= 256
    count = caps * cap + more
    rng = np.random.RandomState(53)
    total = count + 5
    refs = [adamw_ref.loaded(int(s), (B1, B2)) for s in rng.randint(0, 50, total)]
    refs[3] = adamw_ref.State(step=adamw_ref.INT_MAX, beta1_pow=0.0, beta2_pow=1e-300)     # saturates
    states = torch.zeros(total * ops.ADAM_STATE_BYTES, device=DEV, dtype=torch.uint8)
    ops.adam_states_write(states, records_of(refs))
    which = [int(i) for i in rng.permutation(total)[:count]]                # any order; five records stay out
    if 3 not in which:
        which[0] = 3
    names = _launch_names(lambda: ops.adamw_begin(states, which, B1, B2))
    assert names == ['adamw_begin_kernel'] * -(-count // cap), names
    for i in which:
        adamw_ref.begin(refs[i], B1, B2)
    assert ops.adam_states_read(states).tobytes() == records_of(refs).tobytes()
    assert refs[3].step == adamw_ref.INT_MAX and refs[3].applied == 1
    # a skipped step: `applied` of the listed records goes to 0, nothing else moves; then the count goes on
    clip = torch.zeros(ops.CLIP_STATE_BYTES, device=DEV, dtype=torch.uint8)     # finite == 0
    ops.adamw_begin(states, which[:count // 2], B1, B2, clip_state=clip)
    for i in which[:count // 2]:
        adamw_ref.begin(refs[i], B1, B2, finite=0)
    assert ops.adam_states_read(states).tobytes() == records_of(refs).tobytes()
    with pytest.raises(_lib.CtdetError, match='twice'):
        ops.adamw_begin(states, which + which[:1], B1, B2)
    with pytest.raises(_lib.CtdetError, match='record'):                    # past the buffer: refused on the host
        ops.adamw_begin(states, [total], B1, B2)
    assert ops.adam_states_read(states).tobytes() == records_of(refs).tobytes()


# 4 -----------------------------------------------------------------------------------------------------------------
def test_empty_calls_and_empty_tensors_launch_nothing():
    a = Arena([5, 9], [(0,) * 5, (1,) * 5], 59)
    lib = _lib.lib()
    none = torch.empty(0, device=DEV)
    empty = (none, none, none, none, 1, 1e-3, 5e-4)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def calls():
        ops.adamw_begin(a.states, [], B1, B2)
        ops.adamw_step([], B1, B2, EPS, 1.0, a.states)
        ops.adamw_step([empty] * 3, B1, B2, EPS, 1.0, a.states)
        ops.adamw_step([empty + (none,)] * 70, B1, B2, EPS, 1.0, a.states, ema_state=new_ema_state())
        assert lib.ct_adamw_step(None, 0, B1, B2, EPS, 1.0, None, None, stream) == 0
        assert lib.ct_adamw_begin(None, None, 0, B1, B2, None, stream) == 0

    assert _launch_names(calls) == []
    assert a.same_bits() == [True] * 5 and a.same_records()
    with pytest.raises(_lib.CtdetError):                                    # no CPU path
        ops.adamw_step([(torch.zeros(4),) * 4 + (0, 1e-3, 0.0)], B1, B2, EPS, 1.0, a.states)
    with pytest.raises(_lib.CtdetError, match='average'):                   # an average without an ema state
        ops.adamw_step(a.items([1e-3] * 2, [0.0] * 2, ema=True), B1, B2, EPS, 1.0, a.states)
    assert a.same_bits() == [True] * 5


# 5 -----------------------------------------------------------------------------------------------------------------
class Toy(torch.nn.Module):
    """Parameters of given sizes in a ParameterList and one floating-point buffer, as a model has them."""

    def __init__(self, sizes, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.w = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=gen) * 0.25) for n in sizes])
        self.register_buffer('stat', torch.randn(33, generator=gen))


class Restated:
    """A FusedAdamW run restated: one adamw_ref.Run per parameter, the shadows and the average's schedule."""

    def __init__(self, model, ema=None, betas=(B1, B2), eps=EPS):
        self.runs = [adamw_ref.Run(p.detach().cpu().numpy(), betas, eps) for p in model.parameters()]
        self.e = None if ema is None else {k: v.cpu().numpy().copy() for k, v in ema.shadow.items()}
        self.ref = ema_ref.State()

    def step(self, grads, hyper, grad_scale=1.0, ema=None, stat=None):
        if ema is not None:
            ema_ref.begin(self.ref, ema.decay, ema.warmup)
        for i, (run, g) in enumerate(zip(self.runs, grads)):
            if g is not None:
                run.step(g, hyper[i]['lr'], hyper[i]['weight_decay'], grad_scale)
            if ema is not None:
                self.e['w.%d' % i] = ema_ref.update(self.e['w.%d' % i], run.p, self.ref)
        if ema is not None:
            self.e['stat'] = ema_ref.update(self.e['stat'], stat, self.ref)

    def check(self, model, opt, tag, ema=None):
        for i, (p, run) in enumerate(zip(model.parameters(), self.runs)):
            assert not run.flag
            assert sgd_ref.bits_equal(p.detach().cpu().numpy(), run.p), (tag, 'param', i)
            if run.state.step:
                assert sgd_ref.bits_equal(opt.state[p]['exp_avg'].cpu().numpy(), run.m), (tag, 'exp_avg', i)
                assert sgd_ref.bits_equal(opt.state[p]['exp_avg_sq'].cpu().numpy(), run.v), (tag, 'exp_avg_sq', i)
        if ema is not None:
            for k, v in self.e.items():
                assert sgd_ref.bits_equal(ema.shadow[k].cpu().numpy(), v), (tag, 'shadow', k)
        rec = ops.adam_states_read(opt._records)
        assert rec[:len(self.runs)].tobytes() == records_of([r.state for r in self.runs]).tobytes(), (tag, 'records')


OPT_SIZES = [1, 7, 255, 4099, 8193, 20000]
NO_GRAD = 2                                  # this parameter never gets a gradient
HYPER = [dict(lr=2e-3, weight_decay=5e-4), dict(lr=1e-3, weight_decay=0.0)]


def _groups(model):
    ps = list(model.parameters())
    return [dict(params=ps[:3], **HYPER[0]), dict(params=ps[3:], **HYPER[1])]


def _hyper():
    return [HYPER[0 if i < 3 else 1] for i in range(len(OPT_SIZES))]


def _set_grads(model, rng, nan_at=None):
    grads = [None if i == NO_GRAD else adamw_ref.grads_like(rng, n) for i, n in enumerate(OPT_SIZES)]
    if nan_at is not None:
        grads[nan_at][-1] = np.nan
    for p, g in zip(model.parameters(), grads):
        p.grad = None if g is None else torch.from_numpy(g).to(DEV)
    return grads


def test_a_skipped_step_writes_nothing():
    model = Toy(OPT_SIZES, 1).to(DEV)
    ema = WeightEMA(model, 0.9998, 10.0)
    opt = FusedAdamW(_groups(model), max_grad_norm=float('inf'), ema=ema)
    restated = Restated(model, ema)
    rng = np.random.RandomState(3)
    ps = list(model.parameters())

    def snapshot():
        """Everything a step may write.  Of the records everything but `applied`, which ct_adamw_begin sets to 0 on a
        skipped step by definition (include/ctdet.h) and which is checked on its own."""
        moments = [bits(opt.state[p][k]) for p in ps if p in opt.state for k in ('exp_avg', 'exp_avg_sq')]
        rec = ops.adam_states_read(opt._records)
        rec['applied'] = 0
        return [bits(p) for p in ps] + moments + [bits(s) for s in ema.shadows()] + [rec.tobytes()]

    for it in range(3):
        grads = _set_grads(model, rng, nan_at=4 if it == 1 else None)
        model.stat.add_(1.0)
        if it == 1:
            before, count = snapshot(), ema.info()['updates']
            opt.step()
            after = snapshot()
            assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(before, after)), \
                'a skipped step moved something'
            assert ema.info()['updates'] == count == 1 and ema.info()['applied'] is False
            applied = ops.adam_states_read(opt._records)['applied']
            assert [int(x) for x in applied] == [0] * len(ps)   # the listed records say "skipped"; NO_GRAD's never ran
            info = opt.clip_info()
            assert info['nonfinite'] == 1 and info['finite'] is False and info['coef'] == 0.0
            assert opt.state_dict()['state'][0]['step'] == 1    # the skipped step does not count
            ema_ref.begin(restated.ref, ema.decay, ema.warmup, finite=0)
            continue
        opt.step()
        assert opt.last_calls == 1 and opt.clip_info()['coef'] == 1.0
        # the following finite step equals a restatement that never saw the skipped one
        restated.step(grads, _hyper(), 1.0, ema, model.stat.cpu().numpy())
        restated.check(model, opt, 'step %d' % it, ema)
    assert opt.clip_info()['nonfinite'] == 1 and ema.info()['updates'] == 2
    assert [int(s['step']) for s in opt.state_dict()['state'].values()] == [2] * (len(OPT_SIZES) - 1)
    assert NO_GRAD not in opt.state_dict()['state']


# 6 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grad_scale', [1.0, 0.5])
def test_clipping(grad_scale):
    model = Toy(OPT_SIZES, 5).to(DEV)
    opt = FusedAdamW(_groups(model), max_grad_norm=0.5)
    opt.grad_scale = grad_scale
    restated = Restated(model)
    rng = np.random.RandomState(7)
    for it in range(3):
        grads = _set_grads(model, rng)
        opt.step()
        info = opt.clip_info()
        want = clip_ref.norm32([g for g in grads if g is not None], grad_scale)
        assert clip_ref.ulps_apart(F32(info['norm']), want) <= 1               # as tests/test_gpu_grad_clip.py
        coef, finite = clip_ref.coef(F32(info['norm']), 0.5)                    # from the device's own norm
        assert finite == 1 and info['finite'] and coef < 1 and F32(info['coef']) == coef
        restated.step(grads, _hyper(), F32(grad_scale) * coef)
        restated.check(model, opt, 'step %d' % it)


# 7 -----------------------------------------------------------------------------------------------------------------
def _rfb(train=False):
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), 300, 20)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()))
    net = (net.train() if train else net.eval()).cuda()
    net.device = 'cuda'
    return net


def _report(tag, rows):
    """rows of (name, ok, e_fused, e_torch, bound): prints the two errors before asserting, as the rule's callers do."""
    worst = max(rows, key=lambda r: r[2] / r[4] if r[4] else 0.0)
    print('%s: %d tensors; largest e_fused %.3e, largest e_torch_cpu %.3e; closest to its bound: %s e_fused %.3e '
          'e_torch_cpu %.3e bound %.3e' % (tag, len(rows), max(r[2] for r in rows), max(r[3] for r in rows), worst[0],
                                           worst[2], worst[3], worst[4]))
    bad = [r for r in rows if not r[1]]
    assert not bad, bad[:5]


def test_against_torch_on_the_rfbnet_parameters():
    """The parameter list of RFBNet-300 (20 foreground classes + background), random gradients, 3 steps:
    FusedAdamW and torch.optim.AdamW on the CPU against the float64 definition, e_fused <= 2 * e_torch_cpu + ulp(max|p|)
    per tensor."""
    net = _rfb()
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    kw = dict(lr=1e-3, betas=(B1, B2), eps=EPS, weight_decay=5e-4)
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for _, p in named]
    p0 = [c.detach().numpy().copy() for c in cpu]
    topt, fopt = torch.optim.AdamW(cpu, **kw), FusedAdamW([p for _, p in named], **kw)
    gen = torch.Generator().manual_seed(11)
    grads = []
    for _ in range(3):
        step = [torch.randn(c.shape, generator=gen) * 1e-2 for c in cpu]
        grads.append([g.numpy() for g in step])
        for c, (_, p), g in zip(cpu, named, step):
            c.grad, p.grad = g, g.to(DEV)
        topt.step()
        fopt.step()
    assert fopt.last_calls == 1
    rows = []
    for i, ((n, p), c) in enumerate(zip(named, cpu)):
        ref = adamw_ref.definition(p0[i], [g[i] for g in grads], kw['lr'], kw['betas'], kw['eps'], kw['weight_decay'])[0]
        rows.append((n,) + sgd_ref.close_to_torch(p.detach().cpu().numpy(), c.detach().numpy(), ref))
    _report('RFBNet-300 parameters, 3 steps', rows)
    steps = {int(s['step']) for s in fopt.state_dict()['state'].values()}
    assert steps == {3}


# 8 -----------------------------------------------------------------------------------------------------------------
def test_checkpoints_move_between_fused_and_torch():
    sizes = [3, 255, 8193, 20000]
    kw = dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-2)
    rng = np.random.RandomState(13)
    p0 = [(rng.randn(n) * 0.25).astype(F32) for n in sizes]
    grads = [[adamw_ref.grads_like(rng, n) for n in sizes] for _ in range(4)]
    want = [adamw_ref.definition(p0[i], [g[i] for g in grads], kw['lr'], kw['betas'], kw['eps'], kw['weight_decay'])[0]
            for i in range(len(sizes))]

    def make(device):
        return [torch.nn.Parameter(torch.from_numpy(p.copy()).to(device)) for p in p0]

    def drive(opt, ps, which):
        for it in which:
            for p, g in zip(ps, grads[it]):
                p.grad = torch.from_numpy(g).to(p.device)
            opt.step()

    # the yardstick of both directions: torch on the CPU, all four steps
    cpu = make('cpu')
    topt = torch.optim.AdamW(cpu, **kw)
    drive(topt, cpu, range(3))
    sd_torch = copy.deepcopy(topt.state_dict())
    drive(topt, cpu, [3])
    # torch -> fused: three steps on the CPU, the fourth on the device
    dev = [torch.nn.Parameter(c.detach().to(DEV)) for c in make('cpu')]
    half = torch.optim.AdamW([torch.nn.Parameter(p.detach().cpu()) for p in dev], **kw)
    drive(half, half.param_groups[0]['params'], range(3))
    for p, h in zip(dev, half.param_groups[0]['params']):
        p.data.copy_(h.detach())
    fopt = FusedAdamW(dev, lr=7.0)
    fopt.load_state_dict(half.state_dict())
    assert fopt.param_groups[0]['betas'] == (0.8, 0.99) and fopt.param_groups[0]['lr'] == 2e-3
    assert all(fopt.state[p]['exp_avg'].is_cuda for p in dev)
    assert [int(s['step']) for s in fopt.state_dict()['state'].values()] == [3] * 4
    drive(fopt, dev, [3])
    assert [int(s['step']) for s in fopt.state_dict()['state'].values()] == [4] * 4
    rec = ops.adam_states_read(fopt._records)
    assert rec['beta1_pow'][0] == (float(F32(0.8)) ** 3) * float(F32(0.8)) and list(rec['step']) == [4] * 4
    rows = [('torch->fused %d' % i,) + sgd_ref.close_to_torch(p.detach().cpu().numpy(), c.detach().numpy(), w)
            for i, (p, c, w) in enumerate(zip(dev, cpu, want))]
    _report('torch -> FusedAdamW, then one more step', rows)
    # fused -> torch: three steps on the device, the fourth on the CPU (and on the device)
    dev2 = make(DEV)
    fopt2 = FusedAdamW(dev2, **kw)
    drive(fopt2, dev2, range(3))
    sd = fopt2.state_dict()
    assert list(sd) == list(sd_torch) and sd['param_groups'] == sd_torch['param_groups']
    for k in sd_torch['state']:
        assert list(sd['state'][k]) == list(sd_torch['state'][k])
        assert torch.equal(sd['state'][k]['step'], sd_torch['state'][k]['step'])
        assert sd['state'][k]['step'].dtype == sd_torch['state'][k]['step'].dtype and not sd['state'][k]['step'].is_cuda
    cpu2 = [torch.nn.Parameter(p.detach().cpu()) for p in dev2]
    topt2 = torch.optim.AdamW(cpu2, lr=7.0)
    topt2.load_state_dict(sd)
    drive(topt2, cpu2, [3])
    drive(fopt2, dev2, [3])
    rows = [('fused->torch %d' % i,) + sgd_ref.close_to_torch(p.detach().cpu().numpy(), c.detach().numpy(), w)
            for i, (p, c, w) in enumerate(zip(dev2, cpu2, want))]
    _report('FusedAdamW -> torch, then one more step on each side', rows)
    # a fused optimizer continues its own checkpoint bit for bit
    dev3 = make(DEV)
    fopt3 = FusedAdamW(dev3, lr=7.0)
    for p, q in zip(dev3, dev2):
        p.data.copy_(q.detach())
    fopt3.load_state_dict(copy.deepcopy(fopt2.state_dict()))
    for it in (0, 1):
        drive(fopt2, dev2, [it])
        drive(fopt3, dev3, [it])
    for p, q in zip(dev3, dev2):
        got, ref = p.detach().cpu().numpy(), q.detach().cpu().numpy()
        # beta ** 4 against four running products: the records differ by a few 1e-16, far below what fp32 shows
        assert sgd_ref.bits_equal(got, ref) or float(np.abs(got - ref).max()) <= sgd_ref.ulp(np.abs(ref).max())


# 9 -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_are_real_steps():
    """begin + step captured once, no parallel branches; three replays against three eager steps on a copy.  The step
    count lives in the records, so every replay advances it."""
    sizes, offs = [5, 1023, 8193, 16391], [(0,) * 5, (1,) * 5, (2,) * 5, (0, 0, 1, 0, 0)]
    a, eager = Arena(sizes, offs, 61), Arena(sizes, offs, 61)
    lrs, wds = [1e-3, 2e-3, 3e-3, 4e-3], [5e-4, 0.0, 5e-4, 1e-2]
    sa, se = new_ema_state(), new_ema_state()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ema_begin(sa, 0.9998, 10.0)
        a.run(lrs, wds, 0.5, sa)
    torch.cuda.synchronize()
    assert a.same_bits(eager) == [True] * 5 and a.same_records(eager), 'capturing ran something'
    for it in range(3):
        for arena in (a, eager):
            arena.set_grads(adamw_ref.grads_like)
        assert torch.equal(a.dev[G].view(torch.int32), eager.dev[G].view(torch.int32))
        graph.replay()
        ops.ema_begin(se, 0.9998, 10.0)
        eager.run(lrs, wds, 0.5, se)
        torch.cuda.synchronize()
        assert a.same_bits(eager) == [True] * 5 and a.same_records(eager), 'replay %d' % it
        assert torch.equal(sa, se)
    assert list(ops.adam_states_read(a.states)['step']) == [3] * 4 and ops.ema_info(sa)['updates'] == 3
    # ... and the eager side is the restatement's
    ref = ema_ref.State()
    b = Arena(sizes, offs, 61)
    for it in range(3):
        b.set_grads(adamw_ref.grads_like)
        ema_ref.begin(ref, 0.9998, 10.0)
        b.expect(lrs, wds, 0.5, ref)
    assert [sgd_ref.bits_equal(d.cpu().numpy(), h) for d, h in zip(a.dev, b.host)] == [True] * 5


# 10 ----------------------------------------------------------------------------------------------------------------
def test_side_stream_and_repeat_give_the_same_bits():
    sizes, offs = [3, 4099, 8193], [(0,) * 5, (3,) * 5, (1, 1, 1, 2, 1)]
    arenas = [Arena(sizes, offs, 67) for _ in range(3)]
    lrs, wds = [1e-3, 2e-3, 4e-3], [5e-4, 0.0, 1e-2]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for it in range(3):
        for a in arenas:
            a.set_grads(adamw_ref.grads_like)
        torch.cuda.synchronize()
        arenas[0].run(lrs, wds)
        arenas[1].run(lrs, wds)                                 # a second run from the same state
        with torch.cuda.stream(side):
            arenas[2].run(lrs, wds)
        torch.cuda.synchronize()
        arenas[0].expect(lrs, wds)
        for a in arenas[1:]:
            assert a.same_bits(arenas[0]) == [True] * 5 and a.same_records(arenas[0]), it
    assert arenas[0].same_bits() == [True] * 5 and arenas[0].same_records()


def test_version_counters_move():
    ps = [torch.nn.Parameter(torch.randn(100, device=DEV)) for _ in range(3)]
    opt = FusedAdamW(ps, 1e-3)
    for rnd in range(2):
        ps[0].grad, ps[1].grad, ps[2].grad = torch.ones(100, device=DEV), None, torch.ones(100, device=DEV)
        v = [p._version for p in ps]
        mv = [opt.state[p][k]._version for p in (ps[0], ps[2]) for k in ('exp_avg', 'exp_avg_sq')] if rnd else None
        opt.step()
        assert ps[0]._version > v[0] and ps[2]._version > v[2] and ps[1]._version == v[1]
        if rnd:
            now = [opt.state[p][k]._version for p in (ps[0], ps[2]) for k in ('exp_avg', 'exp_avg_sq')]
            assert all(x > y for x, y in zip(now, mv))
    assert ps[1] not in opt.state and opt.last_calls == 1
    # betas are fixed once a tensor has stepped
    opt.param_groups[0]['betas'] = (0.5, 0.999)
    with pytest.raises(ValueError, match='betas changed'):
        opt.step()


def test_in_the_training_step():
    """FusedAdamW inside one TrainRuntime step of RFBNet-300, batch 2: every parameter that has a gradient moves."""
    from layers.functions import PriorBox
    from layers.modules.multibox_loss_combined import MultiBoxLoss_combined
    from data import VOC_300
    net = _rfb(train=True)
    assert net.train_runtime(2) is not None
    priors = PriorBox(VOC_300).forward().cuda()
    crit = MultiBoxLoss_combined(21, 0.5, True, 0, True, 3, 0.5, False)
    x = synth.images(2, 300, 'randn', 1234).cuda()
    tg = [t.cuda() for t in synth.targets(2, 21, 99)]
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    opt = FusedAdamW([p for _, p in named], lr=1e-3, weight_decay=1e-2)
    opt.zero_grad(set_to_none=True)
    sum(crit(net(x), priors, tg).values()).backward()
    assert all(p.grad is not None for _, p in named)
    before = [bits(p) for _, p in named]
    versions = [p._version for _, p in named]
    # the first update of an element is lr * sign(g), and the decay lr * wd * p = 1e-5 * p is above fp32's resolution: only
    # a tensor of zeros with a gradient of zeros can stay
    stays = [not bool((p.grad != 0).any() or (p != 0).any()) for _, p in named]
    opt.step()
    print('%d parameters, %d of them all zero with an all-zero gradient' % (len(named), sum(stays)))
    assert opt.last_calls == 1 and sum(stays) < len(named) // 10
    for (n, p), b, v, st in zip(named, before, versions, stays):
        assert p._version > v, n
        assert st or not np.array_equal(bits(p), b), n
    loss = sum(crit(net(x), priors, tg).values())
    assert bool(torch.isfinite(loss)), float(loss)
