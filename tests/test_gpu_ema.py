"""The weight average on the MI355X: ct_ema_begin, ct_sgd_step_ema, ct_ema_update, ct_tensor_swap, WeightEMA and
FusedSGD with an average attached.

Yardsticks, never the code under test: tests/ema_ref.py (the schedule and the averaging line in NumPy float32, bit for
bit; in float64 from the same fp32 decay for the accuracy bound), tests/sgd_ref.py (the SGD recurrence) and
tests/clip_ref.py (the clipping coefficient, evaluated from the device's own norm as in tests/test_gpu_grad_clip.py).
Tensors are views into flat buffers whose every other element is NaN, and whole buffers are compared, so an access
outside a view shows."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import clip_ref
import ema_ref
import sgd_ref
from ctdet import _lib, ops, synth
from ctdet.optim import FusedSGD, WeightEMA

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
GAP = 9                                      # elements between two views (and before the first, after the last)
TRIPLES = [(0.0, 0.0, 0), (0.9, 0.0, 0), (0.9, 0.1, 0), (0.9, 0.0, 1)]
P, G, B, E = range(4)                        # the four arrays of a step: param, grad, momentum buffer, average


def layout(sizes, offs):
    """First element of each view in a flat buffer: `off` elements past a 16-byte line, GAP or more apart."""
    starts, cur = [], 0
    for n, off in zip(sizes, offs):
        s = (cur + GAP + 3) // 4 * 4 + off
        starts.append(s)
        cur = s + n
    return starts, cur + GAP + 4


class Arena:
    """(param, grad, buf, ema) views into four flat device buffers, NaN between the views, and the host's expected
    image of each WHOLE buffer.  offs[i] = the four line offsets of tensor i."""

    def __init__(self, sizes, offs, seed):
        self.sizes = list(sizes)
        rng = np.random.RandomState(seed)
        self.starts, totals = zip(*[layout(sizes, [o[r] for o in offs]) for r in range(4)])
        self.host = [np.full(t, np.nan, F32) for t in totals]
        for r in range(4):
            for i, n in enumerate(sizes):
                scale = 0.1 if r in (G, B) else 1.0
                self.view(r, i, False)[:] = (rng.randn(n) * scale).astype(F32)
        self.dev = [torch.from_numpy(h).to(DEV) for h in self.host]
        assert all(d.data_ptr() % 16 == 0 for d in self.dev)
        self.rng = rng

    def view(self, r, i, dev=True):
        s = self.starts[r][i]
        return (self.dev[r] if dev else self.host[r])[s:s + self.sizes[i]]

    def new_grads(self, scale=0.1):
        for i, n in enumerate(self.sizes):
            self.view(G, i, False)[:] = (self.rng.randn(n) * scale).astype(F32)
        self.dev[G].copy_(torch.from_numpy(self.host[G]))

    def items(self, lrs, wds, has_buf, first, ema=True, which=None):
        idx = range(len(self.sizes)) if which is None else which
        return [(self.view(P, i), self.view(G, i), self.view(B, i) if has_buf else None, lrs[i], wds[i], first) +
                ((self.view(E, i),) if ema else ()) for i in idx]

    def expect_step(self, i, lr, wd, triple, state, grad_scale=1.0, first=False):
        """The restatement of one fused step of tensor i, written into the host image."""
        m, damp, nest = triple
        p, b = sgd_ref.step(self.view(P, i, False), self.view(G, i, False), self.view(B, i, False) if m else None, lr, wd,
                            m, damp, bool(nest), grad_scale=grad_scale, first_step=first)
        self.view(P, i, False)[:] = p
        if m:
            self.view(B, i, False)[:] = b
        self.view(E, i, False)[:] = ema_ref.update(self.view(E, i, False), p, state)

    def same_bits(self, other=None, rows=(P, G, B, E)):
        want = self.host if other is None else [d.cpu().numpy() for d in other.dev]
        return [sgd_ref.bits_equal(self.dev[r].cpu().numpy(), want[r]) for r in rows]


def read(state):
    """The 16 bytes of a ct_ema_state -> (updates, decay f32, one_minus f32, applied); synchronises."""
    raw = state.cpu().numpy()
    assert raw.dtype == np.uint8 and raw.size == 16
    f, i = raw.view(F32), raw.view(np.int32)
    return int(i[0]), f[1], f[2], int(i[3])


def new_state():
    return torch.zeros(ops.EMA_STATE_BYTES, device=DEV, dtype=torch.uint8)


def same_state(state, ref):
    n, d, om, applied = read(state)
    return (n, d.view(np.uint32), om.view(np.uint32), applied) == \
        (ref.updates, ref.decay.view(np.uint32), ref.one_minus.view(np.uint32), ref.applied)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


# 1 -----------------------------------------------------------------------------------------------------------------
LOAD_SIZES = [1, 3, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 5]


def _load_arena(seed):
    """Every size with all four pointers at the line offsets 0..3, and once more with only the average's pointer one
    element further (the dword path): 45 tensors."""
    sizes = [n for n in LOAD_SIZES for _ in range(5)]
    offs = []
    for k, _ in enumerate(LOAD_SIZES):
        offs += [(o, o, o, o) for o in range(4)] + [(k % 4, k % 4, k % 4, (k + 1) % 4)]
    return Arena(sizes, offs, seed)


def test_every_load_path_of_the_fused_step():
    a = _load_arena(41)
    n = len(a.sizes)
    lrs = [0.01 * (1 + i % 7) for i in range(n)]
    wds = [0.0 if i % 3 == 0 else 5e-4 for i in range(n)]
    triple = (0.9, 0.0, 0)
    state, ref = new_state(), ema_ref.State()
    # one call over all tensors
    ops.ema_begin(state, 0.9998, 10.0)
    ema_ref.begin(ref, 0.9998, 10.0)
    ops.sgd_step_ema(a.items(lrs, wds, True, False), *triple, 1.0, state)
    for i in range(n):
        a.expect_step(i, lrs[i], wds[i], triple, ref)
    assert same_state(state, ref) and ref.decay == F32(0.1)
    assert a.same_bits() == [True] * 4, 'one call: (param, grad, buf, ema) against the restatement, NaN gaps intact'
    # one call per tensor, new gradients, the second decay of the warm-up
    a.new_grads()
    ops.ema_begin(state, 0.9998, 10.0)
    ema_ref.begin(ref, 0.9998, 10.0)
    for i in range(n):
        ops.sgd_step_ema(a.items(lrs, wds, True, False, which=[i]), *triple, 1.0, state)
        a.expect_step(i, lrs[i], wds[i], triple, ref)
    assert same_state(state, ref) and ref.updates == 2
    assert a.same_bits() == [True] * 4, 'one call per tensor'
    # without momentum the buffer pointer is NULL and does not take part in the offset rule
    a.new_grads()
    ops.ema_begin(state, 0.9998, 10.0)
    ema_ref.begin(ref, 0.9998, 10.0)
    ops.sgd_step_ema(a.items(lrs, wds, False, False), 0.0, 0.0, False, 0.5, state)
    for i in range(n):
        a.expect_step(i, lrs[i], wds[i], (0.0, 0.0, 0), ref, grad_scale=0.5)
    assert a.same_bits() == [True] * 4, 'momentum 0'


def test_every_load_path_of_update_and_swap():
    a = _load_arena(43)
    n = len(a.sizes)
    state, ref = new_state(), ema_ref.State()
    pairs = [(a.view(E, i), a.view(P, i)) for i in range(n)]
    for per_tensor in (False, True):
        ops.ema_begin(state, 0.9, 0.0)
        ema_ref.begin(ref, 0.9, 0.0)
        if per_tensor:
            for pr in pairs:
                ops.ema_update([pr], state)
        else:
            ops.ema_update(pairs, state)
        for i in range(n):
            a.view(E, i, False)[:] = ema_ref.update(a.view(E, i, False), a.view(P, i, False), ref)
        assert a.same_bits() == [True] * 4, 'ct_ema_update, per tensor: %s' % per_tensor
    # a step that was not opened: nothing moves
    clip = torch.zeros(ops.CLIP_STATE_BYTES, device=DEV, dtype=torch.uint8)     # finite == 0
    ops.ema_begin(state, 0.9, 0.0, clip_state=clip)
    assert read(state)[3] == 0 and read(state)[0] == 2
    ops.ema_update(pairs, state)
    assert a.same_bits() == [True] * 4, 'applied == 0'
    # the exchange: (param, ema) once -> swapped images, twice -> the bits are back
    before = [h.copy() for h in a.host]
    for per_tensor in (False, True):
        for rounds in (1, 2):
            if per_tensor:
                for e, p in pairs:
                    ops.tensor_swap([(p, e)])
            else:
                ops.tensor_swap([(p, e) for e, p in pairs])
            if rounds == 1:
                for i in range(n):
                    tmp = a.view(P, i, False).copy()
                    a.view(P, i, False)[:] = a.view(E, i, False)
                    a.view(E, i, False)[:] = tmp
                assert not np.array_equal(a.host[P], before[P], equal_nan=True)
            else:
                a.host = [h.copy() for h in before]
            assert a.same_bits() == [True] * 4, 'ct_tensor_swap x%d, per tensor: %s' % (rounds, per_tensor)
    with pytest.raises(_lib.CtdetError, match='overlap'):
        ops.tensor_swap([(a.dev[P][8:24], a.dev[P][16:32])])
    with pytest.raises(_lib.CtdetError, match='a == b'):
        ops.tensor_swap([(a.view(P, 3), a.view(P, 3))])
    with pytest.raises(_lib.CtdetError):                        # no CPU path
        ops.ema_update([(torch.zeros(4), torch.zeros(4))], state)
    assert a.same_bits() == [True] * 4


# 2 -----------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize('clipped', [False, True])
def test_launch_boundary_and_empty_tensors(clipped):
    per = _lib.lib().ct_sgd_ema_tensors_per_launch()
    assert 70 <= per <= 77
    count = 2 * per + 3
    a = Arena([5] * count, [(i % 4,) * 4 for i in range(count)], seed=47)
    lrs, wds = [0.1] * count, [5e-4] * count
    empty = (torch.empty(0, device=DEV),) * 3 + (0.1, 0.0, False, torch.empty(0, device=DEV))
    items = a.items(lrs, wds, True, False)
    items.insert(count // 2, empty)
    items.append(empty)
    state, ref = new_state(), ema_ref.State()
    clip, gs = None, F32(1.0)
    if clipped:
        gh = [a.view(G, i, False) for i in range(count)]
        max_norm = 0.5 * clip_ref.norm64(gh)
        clip = ops.grad_norm_clip([a.view(G, i) for i in range(count)], max_norm)
        coef, finite = clip_ref.coef(F32(ops.clip_info(clip)['norm']), max_norm)
        assert finite == 1 and coef < 1
        gs = F32(1.0) * coef
    ops.ema_begin(state, 0.9998, 10.0, clip_state=clip)
    ema_ref.begin(ref, 0.9998, 10.0, finite=1 if clipped else None)
    names = _launch_names(lambda: ops.sgd_step_ema(items, 0.9, 0.0, False, 1.0, state, clip_state=clip))
    kernel = 'sgd_multi_kernel_ema_clipped' if clipped else 'sgd_multi_kernel_ema'
    assert names == [kernel] * 3 and 3 == -(-count // per), names
    for i in range(count):
        a.expect_step(i, lrs[i], wds[i], (0.9, 0.0, 0), ref, grad_scale=gs)
    assert a.same_bits() == [True] * 4
    if clipped:
        return
    # exactly `per` and `per + 1` tensors; the other two entries at their own boundary; a call of empty tensors only
    for k, want in ((per, 1), (per + 1, 2)):
        names = _launch_names(lambda: ops.sgd_step_ema(a.items(lrs, wds, True, False)[:k], 0.9, 0.0, False, 0.0, state))
        assert names == ['sgd_multi_kernel_ema'] * want, (k, names)
    assert _launch_names(lambda: ops.sgd_step_ema([empty] * 3, 0.9, 0.0, False, 1.0, state)) == []
    pairs = [(a.view(E, i), a.view(P, i)) for i in range(count)] + \
        [(a.view(B, i), a.view(G, i)) for i in range(2 * 140 + 3 - count)]         # 283 pairs, no array twice
    pairs.insert(7, (torch.empty(0, device=DEV), torch.empty(0, device=DEV)))
    assert _launch_names(lambda: ops.ema_update(pairs, state)) == ['ema_multi_kernel'] * 3
    swaps = [(a.view(E, i), a.view(P, i)) for i in range(141)] + [(torch.empty(0, device=DEV),) * 2]
    assert _launch_names(lambda: ops.tensor_swap(swaps)) == ['tensor_swap_kernel'] * 2
    assert _launch_names(lambda: ops.ema_begin(state, 0.5, 0.0)) == ['ema_begin_kernel']


# 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('warmup', [10.0, 0.0])
def test_schedule(warmup):
    rng = np.random.RandomState(53)
    p_h = rng.randn(1000).astype(F32)
    e_h = rng.randn(1000).astype(F32)
    p, e = torch.from_numpy(p_h).to(DEV), torch.from_numpy(e_h).to(DEV)
    state, ref = new_state(), ema_ref.State()
    seen = []
    for it in range(30):
        ops.ema_begin(state, 0.9998, warmup)
        ops.ema_update([(e, p)], state)
        ema_ref.begin(ref, 0.9998, warmup)
        e_h = ema_ref.update(e_h, p_h, ref)
        assert same_state(state, ref), (it, read(state), ref)
        seen.append(float(ref.decay))
        p_h = (p_h + F32(0.01) * rng.randn(1000).astype(F32)).astype(F32)
        p.copy_(torch.from_numpy(p_h))
    assert sgd_ref.bits_equal(e.cpu().numpy(), e_h)
    assert ops.ema_info(state) == {'updates': 30, 'decay': float(ref.decay), 'applied': True}
    if warmup:
        assert seen == sorted(seen) and seen[0] == float(F32(0.1)) and seen[-1] == float(F32(30.0) / F32(39.0))
    else:
        assert set(seen) == {float(F32(0.9998))}


def test_decay_zero_copies_the_source_bit_for_bit():
    rng = np.random.RandomState(59)
    p_h = (rng.randn(8195) * 10.0 ** rng.uniform(-20, 20, 8195)).astype(F32)
    p, e = torch.from_numpy(p_h).to(DEV), torch.from_numpy(rng.randn(8195).astype(F32)).to(DEV)
    state = new_state()
    ops.ema_begin(state, 0.0, 0.0)
    ops.ema_update([(e, p)], state)
    assert np.array_equal(bits(e), p_h.view(np.uint32))
    assert read(state) == (1, F32(0.0), F32(1.0), 1)


# 4 -----------------------------------------------------------------------------------------------------------------
STEP_SIZES = [1, 3, 63, 4097, 8193]
STEP_OFFS = [(0, 0, 0, 0), (1, 1, 1, 1), (2, 3, 2, 2), (3, 3, 3, 3), (0, 0, 0, 2)]


@pytest.mark.parametrize('clipped', [False, True])
@pytest.mark.parametrize('wd', [0.0, 5e-4])
@pytest.mark.parametrize('momentum,dampening,nesterov', TRIPLES)
def test_param_and_buffer_bits_are_those_of_the_plain_step(momentum, dampening, nesterov, wd, clipped):
    """Three steps, the first one a first step: ct_sgd_step_ema against ct_sgd_step / ct_sgd_step_clipped on a copy."""
    a, plain = Arena(STEP_SIZES, STEP_OFFS, 61), Arena(STEP_SIZES, STEP_OFFS, 61)
    n = len(STEP_SIZES)
    lrs = [0.01 * (1 + i) for i in range(n)]
    wds = [0.0 if i == 2 else wd for i in range(n)]
    has_buf = momentum != 0
    state, ref = new_state(), ema_ref.State()
    for it in range(3):
        for arena in (a, plain):
            arena.new_grads(10.0 ** (it - 1))
        clip = None
        if clipped:
            max_norm = 0.5 * clip_ref.norm64([a.view(G, i, False) for i in range(n)])
            clip = ops.grad_norm_clip([a.view(G, i) for i in range(n)], max_norm)
        p_before = [a.view(P, i, False).copy() for i in range(n)]
        ops.ema_begin(state, 0.9998, 10.0, clip_state=clip)
        ema_ref.begin(ref, 0.9998, 10.0, finite=1 if clipped else None)
        ops.sgd_step_ema(a.items(lrs, wds, has_buf, it == 0), momentum, dampening, nesterov, 1.0, state, clip_state=clip)
        ops.sgd_step(plain.items(lrs, wds, has_buf, it == 0, ema=False), momentum, dampening, nesterov, 1.0,
                     clip_state=clip)
        assert a.same_bits(plain, rows=(P, G, B)) == [True] * 3, 'step %d' % it
        # ... and the average followed the NEW parameter values
        got_p = a.dev[P].cpu().numpy()
        for i in range(n):
            s = a.starts[P][i]
            new_p = got_p[s:s + STEP_SIZES[i]]
            assert not np.array_equal(new_p, p_before[i])
            a.view(P, i, False)[:] = new_p
            a.view(E, i, False)[:] = ema_ref.update(a.view(E, i, False), new_p, ref)
        assert a.same_bits(rows=(E,)) == [True], 'step %d: ema' % it


# 5 -----------------------------------------------------------------------------------------------------------------
class Toy(torch.nn.Module):
    """Parameters of given sizes in a ParameterList and one floating-point buffer, as a model has them."""

    def __init__(self, sizes, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.w = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=gen)) for n in sizes])
        self.register_buffer('stat', torch.randn(33, generator=gen))
        self.register_buffer('count', torch.zeros((), dtype=torch.long))        # not floating point: no shadow


def test_a_skipped_step_skips_the_average():
    sizes = [5, 300, 8195]
    model = Toy(sizes, 1).to(DEV)
    ema = WeightEMA(model, 0.9998, 10.0)
    assert sorted(ema.shadow) == ['stat', 'w.0', 'w.1', 'w.2']
    opt = FusedSGD(model.parameters(), 0.1, momentum=0.9, weight_decay=5e-4, max_grad_norm=1.0).attach_ema(ema)
    ps = list(model.parameters())
    host_p = [p.detach().cpu().numpy().copy() for p in ps]
    host_b = [None] * 3
    host_e = {k: v.cpu().numpy().copy() for k, v in ema.shadow.items()}
    ref = ema_ref.State()
    rng = np.random.RandomState(3)
    for it in range(3):
        grads = [rng.randn(n).astype(F32) for n in sizes]
        if it == 1:
            grads[2][8191] = np.nan
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(g).to(DEV)
        model.stat.add_(1.0)
        stat_h = model.stat.cpu().numpy()
        snap = [bits(p) for p in ps] + [bits(opt.state[p]['momentum_buffer']) for p in ps if it] + \
            [bits(s) for s in ema.shadows()]
        opt.step()
        info, cinfo = ema.info(), opt.clip_info()
        if it == 1:
            after = [bits(p) for p in ps] + [bits(opt.state[p]['momentum_buffer']) for p in ps] + \
                [bits(s) for s in ema.shadows()]
            assert all(np.array_equal(x, y) for x, y in zip(snap, after)), 'a skipped step moved something'
            assert info['applied'] is False and info['updates'] == 1 and cinfo['finite'] is False
            ema_ref.begin(ref, 0.9998, 10.0, finite=0)
            continue
        coef, finite = clip_ref.coef(F32(cinfo['norm']), 1.0)
        assert finite == 1 and coef < 1
        ema_ref.begin(ref, 0.9998, 10.0, finite=1)
        assert same_state(ema.state, ref)
        for i in range(3):
            host_p[i], host_b[i] = sgd_ref.step(host_p[i], grads[i], host_b[i], 0.1, 5e-4, 0.9, 0.0, False,
                                                grad_scale=F32(1.0) * coef, first_step=host_b[i] is None)
            host_e['w.%d' % i] = ema_ref.update(host_e['w.%d' % i], host_p[i], ref)
            assert sgd_ref.bits_equal(ps[i].detach().cpu().numpy(), host_p[i]), (it, i)
            assert sgd_ref.bits_equal(opt.state[ps[i]]['momentum_buffer'].cpu().numpy(), host_b[i]), (it, i)
        host_e['stat'] = ema_ref.update(host_e['stat'], stat_h, ref)
        for k in host_e:
            assert sgd_ref.bits_equal(ema.shadow[k].cpu().numpy(), host_e[k]), (it, k)
    # the third step used the warm-up decay of n = 1, not of n = 2
    assert ref.updates == 2 and ref.decay == F32(2.0) / F32(11.0) and info == {'updates': 2, 'decay': float(ref.decay),
                                                                               'applied': True}
    assert cinfo['nonfinite'] == 1 and opt.last_calls == 1


# 6 -----------------------------------------------------------------------------------------------------------------
OPT_SIZES = [1, 2, 7, 64, 255, 1000, 4099, 8192, 8193, 20000, 33333, 70000]
NO_GRAD = 4                                  # this parameter never gets a gradient
HYPER = [dict(momentum=0.9, nesterov=False, lr=0.05, weight_decay=5e-4),
         dict(momentum=0.5, nesterov=True, lr=0.02, weight_decay=0.0)]


def _groups(model):
    ps = list(model.parameters())
    return [dict(params=ps[:6], **HYPER[0]), dict(params=ps[6:], **HYPER[1])]


class Restated:
    """The restatement of the optimizer-level runs: parameters, momentum buffers, the buffer and all shadows."""

    def __init__(self, model, ema):
        self.p = [p.detach().cpu().numpy().copy() for p in model.parameters()]
        self.b = [None] * len(self.p)
        self.e = {k: v.cpu().numpy().copy() for k, v in ema.shadow.items()}
        self.ref = ema_ref.State()

    def step(self, grads, stat, decay, warmup):
        ema_ref.begin(self.ref, decay, warmup)
        for i, g in enumerate(grads):
            if g is not None:
                h = HYPER[0 if i < 6 else 1]
                self.p[i], self.b[i] = sgd_ref.step(self.p[i], g, self.b[i], h['lr'], h['weight_decay'], h['momentum'], 0.0,
                                                    h['nesterov'], first_step=self.b[i] is None)
            self.e['w.%d' % i] = ema_ref.update(self.e['w.%d' % i], self.p[i], self.ref)
        self.e['stat'] = ema_ref.update(self.e['stat'], stat, self.ref)

    def check(self, model, ema, tag):
        for i, p in enumerate(model.parameters()):
            assert sgd_ref.bits_equal(p.detach().cpu().numpy(), self.p[i]), (tag, 'param', i)
        for k, v in self.e.items():
            assert sgd_ref.bits_equal(ema.shadow[k].cpu().numpy(), v), (tag, 'shadow', k)
        assert same_state(ema.state, self.ref), tag


def _drive(model, opt, rng, restated, ema, steps, tag):
    ps = list(model.parameters())
    for it in range(steps):
        grads = [None if i == NO_GRAD else (rng.randn(n) * 0.1).astype(F32) for i, n in enumerate(OPT_SIZES)]
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.from_numpy(g).to(DEV)
        model.stat.mul_(0.9).add_(0.1)                           # what a BatchNorm layer does to its statistics
        opt.step()
        assert opt.last_calls == 2                              # one ct_sgd_step_ema per momentum triple
        restated.step(grads, model.stat.cpu().numpy(), ema.decay, ema.warmup)
        restated.check(model, ema, '%s step %d' % (tag, it))


def test_fused_sgd_with_an_attached_average():
    model = Toy(OPT_SIZES, 7).to(DEV)
    ema = WeightEMA(model, 0.999, 4.0)
    with pytest.raises(ValueError, match='no shadow'):          # an optimizer parameter the average does not hold
        FusedSGD([torch.nn.Parameter(torch.zeros(3, device=DEV))], 0.1, ema=ema)
    opt = FusedSGD(_groups(model), 0.1, ema=ema)
    assert opt.ema is ema and ema.info() == {'updates': 0, 'decay': 0.0, 'applied': False}
    restated = Restated(model, ema)
    rng = np.random.RandomState(11)
    no_grad_start = restated.e['w.%d' % NO_GRAD].copy()
    _drive(model, opt, rng, restated, ema, 8, 'first run')
    assert ema.info()['updates'] == 8 and ema.info()['decay'] == float(F32(8.0) / F32(11.0))
    # the grad-less parameter's shadow moved by the same rule: towards the value it already had, so only by the
    # three roundings of each of the 8 updates
    assert np.array_equal(model.w[NO_GRAD].detach().cpu().numpy(), restated.p[NO_GRAD])
    assert np.abs(restated.e['w.%d' % NO_GRAD] - no_grad_start).max() <= 8 * 3 * 2.0 ** -24 * np.abs(no_grad_start).max()
    assert not np.array_equal(restated.e['stat'], model.stat.cpu().numpy())
    assert 'count' not in ema.shadow
    # state_dict() -> fresh objects -> load_state_dict(): the run continues bit for bit
    sd_model, sd_opt, sd_ema = model.state_dict(), opt.state_dict(), ema.state_dict()
    assert set(sd_ema) == {'decay', 'warmup', 'updates', 'shadow'} and sd_ema['updates'] == 8
    assert set(sd_opt) == {'state', 'param_groups'}
    sd_ema = {k: ({n: t.cpu() for n, t in v.items()} if k == 'shadow' else v) for k, v in sd_ema.items()}
    model2 = Toy(OPT_SIZES, 99).to(DEV)
    model2.load_state_dict(sd_model)
    ema2 = WeightEMA(model2, 0.5, 0.0)
    ema2.load_state_dict(sd_ema)
    assert (ema2.decay, ema2.warmup) == (0.999, 4.0) and ema2.info()['updates'] == 8
    opt2 = FusedSGD(_groups(model2), 0.1, ema=ema2)
    opt2.load_state_dict(sd_opt)
    _drive(model2, opt2, rng, restated, ema2, 3, 'after the round trip')
    assert ema2.info() == {'updates': 11, 'decay': float(F32(11.0) / F32(14.0)), 'applied': True}
    # copy_to: another model takes the shadows, parameters and the floating-point buffer
    model3 = Toy(OPT_SIZES, 5).to(DEV)
    ema2.copy_to(model3)
    for k, v in restated.e.items():
        t = dict(model3.named_parameters()).get(k, dict(model3.named_buffers()).get(k))
        assert sgd_ref.bits_equal(t.detach().cpu().numpy(), v), k


def test_weight_ema_update_after_torch_sgd():
    model = Toy(OPT_SIZES, 13).to(DEV)
    ema = WeightEMA(model, 0.9998, 10.0)
    opt = torch.optim.SGD(_groups(model), 0.1)
    shadows = {k: v.cpu().numpy().copy() for k, v in ema.shadow.items()}
    ref = ema_ref.State()
    gen = torch.Generator().manual_seed(17)
    for it in range(4):
        for i, p in enumerate(model.parameters()):
            p.grad = None if i == NO_GRAD else (torch.randn(p.shape, generator=gen) * 0.1).to(DEV)
        opt.step()
        ema.update()
        ema_ref.begin(ref, 0.9998, 10.0)
        live = dict(model.named_parameters())
        live['stat'] = model.stat
        for k in shadows:
            shadows[k] = ema_ref.update(shadows[k], live[k].detach().cpu().numpy(), ref)
            assert sgd_ref.bits_equal(ema.shadow[k].cpu().numpy(), shadows[k]), (it, k)
        assert same_state(ema.state, ref)


# 7 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('decay', [0.9, 0.9998])
def test_accuracy(decay):
    """50 updates on the device against the same updates in float64 (from the fp32 d and 1 - d), parameters spread over
    1e-3 .. 1e2; warmup 0, so that `decay` is the decay of every update.
    Tolerance, derived: each update rounds three times (d * ema, (1 - d) * p, their sum; the rounding of 1 - d is in
    the fp32 value both sides use), each by at most half an ulp <= 2^-24 * M, where M is the largest |ema| or |p| of
    the float64 run; the error of earlier updates is multiplied by d <= 1 per update, so after 50 updates it is at most
    3 * 2^-24 * M * min(50, 1 / (1 - decay)).  On these inputs the float32 restatement uses 0.07 of this bound at
    decay 0.9 and 0.18 of it at 0.9998 (tests/test_ema_cpu.py), and the device reproduces the restatement's bits."""
    start, seq = ema_ref.accuracy_inputs()
    e64, m = ema_ref.accuracy_run(start, seq, decay, 0.0, np.float64)
    e32, _ = ema_ref.accuracy_run(start, seq, decay, 0.0, np.float32)
    p, e = torch.from_numpy(start.copy()).to(DEV), torch.from_numpy(start.copy()).to(DEV)
    state = new_state()
    for x in seq:
        p.copy_(torch.from_numpy(x))
        ops.ema_begin(state, decay, 0.0)
        ops.ema_update([(e, p)], state)
    got = e.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - e64).max())
    tol = 3 * 2.0 ** -24 * m * min(50, 1 / (1 - decay))
    print('decay %g: max|ema_gpu - ema_fp64| %.3e  bound %.3e  (M %.3e; the fp32 restatement: %.3e)'
          % (decay, err, tol, m, float(np.abs(e32.astype(np.float64) - e64).max())))
    assert err <= tol
    assert sgd_ref.bits_equal(got, e32)


# 8 -----------------------------------------------------------------------------------------------------------------
def _rfb(sd=None):
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), 300, 20)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()) if sd is None else sd)
    net = net.eval().cuda()
    net.device = 'cuda'
    return net


def test_pipeline_runs_on_the_averaged_weights_inside_swapped():
    from data import VOC_300
    from ctdet.pipeline import DetectionPipeline
    from layers.functions import PriorBox
    priors = PriorBox(VOC_300).forward()
    x = synth.images(2, 300, 'randn', 1234).cuda()

    def run(pipe):
        """(out_dets, out_count) of one run.  Only the rows r < out_count[b, c] of out_dets [B,T,cap,5] belong to the
        result: the buffer is not cleared between runs, so a pipeline that has run on other weights before keeps its
        older rows behind them.  They are zeroed here, and everything else is compared with torch.equal."""
        dets, count = pipe.run(x)
        rows = torch.arange(dets.shape[2], device=dets.device)
        valid = rows[None, None, :] < count[:, :, None]
        return torch.where(valid[..., None], dets, torch.zeros_like(dets)), count.clone()

    net = _rfb()
    pipe = DetectionPipeline(net, priors, 2, 20, graph=True)
    first = [run(pipe) for _ in range(3)]                       # two eager steps and the captured one
    assert pipe._graph is not None, 'the graph path did not capture'
    graph = pipe._graph
    assert all(torch.equal(a, b) for r in first[1:] for a, b in zip(first[0], r))
    ema = WeightEMA(net, 0.9998, 10.0)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    opt = FusedSGD([p for _, p in named], 0.1, momentum=0.9, weight_decay=5e-4, ema=ema)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(3):
        for _, p in named:
            p.grad = torch.randn(p.shape, generator=gen, device=DEV) * 1e-3
        opt.step()
    assert ema.info() == {'updates': 3, 'decay': float(F32(3.0) / F32(12.0)), 'applied': True}
    live_bits = {n: bits(p) for n, p in net.named_parameters()}
    live_sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    # a second network and pipeline built from copy_to, a third that holds the live weights
    net_avg = ema.copy_to(_rfb(live_sd))
    want_avg = run(DetectionPipeline(net_avg, priors, 2, 20, graph=False))
    want_live = run(DetectionPipeline(_rfb(live_sd), priors, 2, 20, graph=False))
    assert int(want_avg[1].sum()) > 0 and int(want_live[1].sum()) > 0, 'degenerate case: no detections'
    with ema.swapped():
        got_avg = run(pipe)
        assert any(not np.array_equal(bits(p), live_bits[n]) for n, p in net.named_parameters())
    assert pipe._graph is graph, 'the swap made the pipeline capture again'
    assert torch.equal(got_avg[0], want_avg[0]) and torch.equal(got_avg[1], want_avg[1])
    for n, p in net.named_parameters():
        assert np.array_equal(bits(p), live_bits[n]), n
    got_live = run(pipe)
    assert pipe._graph is graph
    assert torch.equal(got_live[0], want_live[0]) and torch.equal(got_live[1], want_live[1])
    # the test cannot pass on a swap that does nothing
    assert not (torch.equal(got_avg[0], got_live[0]) and torch.equal(got_avg[1], got_live[1]))
    assert not (torch.equal(got_live[0], first[0][0]) and torch.equal(got_live[1], first[0][1]))


# 9 -----------------------------------------------------------------------------------------------------------------
# Around the chunk of 8192 elements a workgroup owns, where "whole chunk" flips to "first / last chunk": with the line
# offsets 0..3 these give a one-chunk tensor (8188 and 8189 at any offset, 8191 at 0 and 1, 8192 at 0: the chunk is
# whole), a tensor its shift pushes into a second chunk (8191 at 2 and 3, 8192 at 1..3), a whole middle chunk (16384 at
# 1..3, 16387: at 3 it is 8189 + 8192 + 6 elements), a whole last chunk (16381 at 3) and a last chunk of one element
# (8193 at 0, 8192 and 16384 at 1).
EDGE_SIZES = [8188, 8189, 8191, 8192, 8193, 16381, 16384, 16387]
EDGE_KERNELS = ['step', 'step_clipped', 'step_skipped', 'step_ema', 'ema_update', 'tensor_swap']


@pytest.mark.parametrize('kernel', EDGE_KERNELS)
def test_chunk_boundaries_of_every_walked_kernel(kernel):
    """Every size at the four common line offsets and once with four disagreeing ones (the dword path), 40 tensors in
    ONE call of the kernel: all four whole buffers against the restatement bit for bit, NaN gaps included."""
    sizes = [n for n in EDGE_SIZES for _ in range(5)]
    offs = []
    for k, _ in enumerate(EDGE_SIZES):
        offs += [(o, o, o, o) for o in range(4)] + [tuple((k + r) % 4 for r in range(4))]
    a = Arena(sizes, offs, 83)
    n = len(sizes)
    lrs = [0.01 * (1 + i % 7) for i in range(n)]
    wds = [0.0 if i % 3 == 0 else 5e-4 for i in range(n)]
    triple = (0.9, 0.0, 0)
    state, ref = new_state(), ema_ref.State()
    if kernel in ('ema_update', 'tensor_swap'):
        if kernel == 'ema_update':
            ops.ema_begin(state, 0.9, 0.0)
            ema_ref.begin(ref, 0.9, 0.0)
            ops.ema_update([(a.view(E, i), a.view(P, i)) for i in range(n)], state)
            for i in range(n):
                a.view(E, i, False)[:] = ema_ref.update(a.view(E, i, False), a.view(P, i, False), ref)
        else:
            ops.tensor_swap([(a.view(P, i), a.view(E, i)) for i in range(n)])
            for i in range(n):
                tmp = a.view(P, i, False).copy()
                a.view(P, i, False)[:] = a.view(E, i, False)
                a.view(E, i, False)[:] = tmp
        assert a.same_bits() == [True] * 4, kernel
        return
    first = [kernel == 'step_skipped' and i % 2 == 0 for i in range(n)]
    clip, gs = None, F32(1.0)
    if kernel == 'step_skipped':
        for i in range(n):
            if first[i]:
                a.view(B, i, False)[:] = np.nan                 # "uninitialised": the skip must leave +0 here
        a.view(G, n - 1, False)[sizes[-1] - 1] = np.inf
        for r in (G, B):
            a.dev[r].copy_(torch.from_numpy(a.host[r]))
    if kernel in ('step_clipped', 'step_skipped'):
        gh = [a.view(G, i, False) for i in range(n)]
        max_norm = 0.5 * clip_ref.norm64(gh) if kernel == 'step_clipped' else 1.0
        clip = ops.grad_norm_clip([a.view(G, i) for i in range(n)], max_norm)
        info = ops.clip_info(clip)
        if kernel == 'step_clipped':
            assert clip_ref.ulps_apart(F32(info['norm']), clip_ref.norm32(gh)) <= 1     # as tests/test_gpu_grad_clip.py
            coef, finite = clip_ref.coef(F32(info['norm']), max_norm)
            assert finite == 1 and info['finite'] and coef < 1 and F32(info['coef']) == coef
            gs = F32(1.0) * coef
        else:
            assert not info['finite'] and info['coef'] == 0.0
    items = [(a.view(P, i), a.view(G, i), a.view(B, i), lrs[i], wds[i], first[i]) +
             ((a.view(E, i),) if kernel == 'step_ema' else ()) for i in range(n)]
    if kernel == 'step_ema':
        ops.ema_begin(state, 0.9998, 10.0)
        ema_ref.begin(ref, 0.9998, 10.0)
        ops.sgd_step_ema(items, *triple, 1.0, state)
    else:
        ops.sgd_step(items, *triple, 1.0, clip_state=clip)
    for i in range(n):
        if kernel == 'step_skipped':
            if first[i]:
                a.view(B, i, False)[:] = 0.0                    # nothing else is written
        else:
            a.expect_step(i, lrs[i], wds[i], triple, ref, grad_scale=gs)       # ref not applied: the average stays
    assert a.same_bits() == [True] * 4, kernel
