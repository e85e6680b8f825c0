"""Gradient-norm clipping and the non-finite guard on the MI355X (ct_grad_norm_clip, ct_sgd_step_clipped,
FusedSGD(max_grad_norm=...)).

Yardsticks, never the code under test: tests/clip_ref.py (the norm in binary64 with an exactly rounded sum, the
coefficient in NumPy float32), tests/sgd_ref.py (the recurrence) and torch on the CPU (clip_grad_norm_ followed by
torch.optim.SGD) with torch's own distance from an fp64 evaluation as the tolerance.

Tolerances.  The device `norm` is at most 1 fp32 ulp from np.float32(norm64): all terms are positive, so a binary64
sum of N <= 3.8e7 terms in any order is within N * 2^-53 < 4.2e-9 relative of the exact sum, the square root halves
that, and 2.1e-9 is far inside half an fp32 ulp (>= 2.9e-8 relative) -- the result is the same or the adjacent float.
`coef` is bit-equal to the restatement evaluated from the device's own norm; parameters and momentum buffers are
bit-equal to sgd_ref.step(..., grad_scale=np.float32(gs) * coef)."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import clip_ref
import sgd_ref
from ctdet import _lib, ops, synth
from ctdet.optim import FusedSGD

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
GAP = 9                                      # elements between two views (and before the first, after the last)
CHUNK = 8192                                 # elements a workgroup owns (include/ctdet.h)
TRIPLES = [(0.0, 0.0, 0), (0.9, 0.0, 0), (0.9, 0.1, 0), (0.9, 0.0, 1)]


def layout(sizes, offs):
    """First element of each view in a flat buffer: `off` elements past a 16-byte line, GAP or more apart."""
    starts, cur = [], 0
    for n, off in zip(sizes, offs):
        s = (cur + GAP + 3) // 4 * 4 + off
        starts.append(s)
        cur = s + n
    return starts, cur + GAP + 4


class GradArena:
    """Gradient tensors as views into ONE flat device buffer whose every other element is NaN: a read outside a
    tensor turns the norm non-finite."""

    def __init__(self, sizes, offs, seed, fill=None):
        self.sizes = list(sizes)
        self.starts, total = layout(sizes, offs)
        rng = np.random.RandomState(seed)
        self.host = np.full(total, np.nan, F32)
        for s, n in zip(self.starts, sizes):
            self.host[s:s + n] = fill(rng, n) if fill else (rng.randn(n) * 10.0 ** rng.uniform(-3, 2)).astype(F32)
        self.upload()

    def upload(self):
        self.dev = torch.from_numpy(self.host).to(DEV)
        assert self.dev.data_ptr() % 16 == 0

    def views(self, dev=True):
        b = self.dev if dev else self.host
        return [b[s:s + n] for s, n in zip(self.starts, self.sizes)]


def read(state):
    """The 16 state bytes -> (norm f32, coef f32, finite, nonfinite); synchronises."""
    raw = state.cpu().numpy()
    assert raw.dtype == np.uint8 and raw.size == 16
    f, i = raw.view(F32), raw.view(np.int32)
    return f[0], f[1], int(i[2]), int(i[3])


def check_state(state, grads_host, max_norm, grad_scale=1.0, nonfinite=0, tag=''):
    """Asserts the finite case: norm within 1 ulp of the restatement, coef bit-equal from the device's norm."""
    norm, coef, finite, bad = read(state)
    want = clip_ref.norm32(grads_host, grad_scale)
    assert np.isfinite(want), (tag, want)
    assert np.isfinite(norm) and norm >= 0, (tag, norm)
    d = clip_ref.ulps_apart(norm, want)
    wc, wf = clip_ref.coef(norm, max_norm)
    print('%s norm %.9g want %.9g (%d ulp)  coef %.9g want %.9g  finite %d nonfinite %d'
          % (tag, norm, want, d, coef, wc, finite, bad))
    assert d <= 1, (tag, norm, want)
    assert finite == 1 and wf == 1 and bad == nonfinite, (tag, finite, bad)
    assert coef.view(np.uint32) == wc.view(np.uint32), (tag, coef, wc)
    return norm, coef


# 1 -----------------------------------------------------------------------------------------------------------------
LOAD_SIZES = [1, 3, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 5]


def test_every_load_path_reads_nothing_outside_the_tensors():
    """Every size at element offsets 0..3 past a 16-byte boundary, NaN everywhere between the views: one call over
    all 36 tensors, and one call per tensor."""
    sizes = [n for n in LOAD_SIZES for _ in range(4)]
    offs = [o for _ in LOAD_SIZES for o in range(4)]
    a = GradArena(sizes, offs, seed=41)
    gd, gh = a.views(), a.views(False)
    max_norm = 0.5 * clip_ref.norm64(gh)
    state = ops.grad_norm_clip(gd, max_norm)
    _, coef = check_state(state, gh, max_norm, tag='all 36')
    assert coef < 1
    for i in range(len(sizes)):
        one = 10.0 * clip_ref.norm64(gh[i:i + 1])
        st = ops.grad_norm_clip(gd[i:i + 1], one, 0.125)
        _, coef = check_state(st, gh[i:i + 1], one, 0.125, tag='numel %d offset %d' % (sizes[i], offs[i]))
        assert coef == 1
    assert np.array_equal(a.dev.cpu().numpy().view(np.uint32), a.host.view(np.uint32)), 'gradients were written'


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


def test_launch_boundary_empty_tensor_and_empty_call():
    per = _lib.lib().ct_grad_norm_tensors_per_launch()
    count = 2 * per + 3
    sizes = [7] * count
    offs = [i % 4 for i in range(count)]
    a = GradArena(sizes, offs, seed=43)
    gd, gh = a.views(), a.views(False)
    mid = count // 2
    gd.insert(mid, torch.empty(0, device=DEV))                  # passes a NULL pointer (ops.grad_table)
    assert ops.grad_table(gd)[mid].grad is None and ops.grad_table(gd)[mid].numel == 0
    got = {}
    names = _launch_names(lambda: got.update(state=ops.grad_norm_clip(gd, 1.0)))
    check_state(got['state'], gh, 1.0, tag='%d tensors of 7' % count)
    assert names.count('grad_norm_kernel') == 3 == -(-count // per)
    assert names.count('grad_norm_finish_kernel') == 1 and len(names) == 4
    # exactly `per` and `per + 1` tensors: one and two launches before the finish
    for k, want in ((per, 1), (per + 1, 2)):
        names = _launch_names(lambda: ops.grad_norm_clip(gd[:k], 1.0))
        assert names.count('grad_norm_kernel') == want and len(names) == want + 1, (k, names)
    # n == 0, and a call of empty tensors only: norm 0, finite, coef 1 -- one launch, the finish
    for grads in ([], [torch.empty(0, device=DEV)] * 3):
        names = _launch_names(lambda: got.update(state=ops.grad_norm_clip(grads, 1.0)))
        norm, coef, finite, bad = read(got['state'])
        assert (float(norm), float(coef), finite, bad) == (0.0, 1.0, 1, 0) and names == ['grad_norm_finish_kernel']
        assert norm.view(np.uint32) == 0


# 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['huge_one', 'huge_scaled', 'tiny', 'mixed', 'overflow'])
def test_range(case):
    """Squares that overflow or underflow fp32 are summed in binary64; only a NORM beyond fp32 counts as non-finite."""
    sizes, offs = [1, 1000, 8195], [0, 1, 3]
    gs = 1.0
    if case == 'huge_one':                                      # one element of 3e38, the rest small: norm 3e38
        def fill(rng, n):
            return np.full(n, 3e38, F32) if n == 1 else rng.randn(n).astype(F32)
    elif case in ('huge_scaled', 'overflow'):                   # 9 196 elements of 3e38: 2.9e40, finite only scaled
        gs = 2.0 ** -10 if case == 'huge_scaled' else 1.0

        def fill(rng, n):
            return np.full(n, 3e38, F32) * rng.choice([-1, 1], n).astype(F32)
    elif case == 'tiny':                                        # squares of 1e-30 are 0 in fp32
        def fill(rng, n):
            return np.full(n, 1e-30, F32) * rng.choice([-1, 1], n).astype(F32)
    else:
        gs = 2.0 ** -10

        def fill(rng, n):
            return np.where(rng.rand(n) < 0.01, 3e38, 1e-30).astype(F32)
    a = GradArena(sizes, offs, seed=47, fill=fill)
    gd, gh = a.views(), a.views(False)
    max_norm = 1e3                                              # keeps 1e3 / 3e38 a normal fp32 number
    state = ops.grad_norm_clip(gd, max_norm, gs)
    if case == 'overflow':
        norm, coef, finite, bad = read(state)
        assert np.isinf(norm) and norm > 0 and coef == 0 and finite == 0 and bad == 1
        assert np.isinf(clip_ref.norm32(gh, gs))
        return
    norm, coef = check_state(state, gh, max_norm, gs, tag=case)
    if case == 'tiny':
        assert 9e-29 < norm < 1e-28 and coef == 1               # sqrt(9196) * 1e-30
    else:
        assert norm > 1e35 and 1e-37 < coef < 1e-32


# 4 -----------------------------------------------------------------------------------------------------------------
NF_SIZES = [100, 8200, 8195, 3 * 8192 + 5]
NF_OFFS = [(0, 0, 0), (1, 1, 1), (0, 1, 2), (2, 2, 2)]          # (param, grad, buf); tensor 2 takes the dword path
NF_FIRST = [False, True, True, False]                           # tensors 1 and 2 have no momentum state yet
# the last tensor's grad sits 2 elements past a line: chunk c holds elements [c * 8192 - 2, (c + 1) * 8192 - 2)
NF_POS = {'first_of_tensor': 0, 'last_of_chunk0': CHUNK - 3, 'first_of_chunk1': CHUNK - 2,
          'last_of_chunk2': 3 * CHUNK - 3, 'first_of_last_chunk': 3 * CHUNK - 2, 'last_of_tensor': 3 * CHUNK + 4}


@pytest.mark.parametrize('where', sorted(NF_POS))
@pytest.mark.parametrize('value', [np.inf, -np.inf, np.nan])
def test_non_finite_gradient_skips_the_step(value, where):
    rng = np.random.RandomState(53)
    starts, totals = zip(*[layout(NF_SIZES, [o[r] for o in NF_OFFS]) for r in range(3)])
    host = [rng.randn(t).astype(F32) for t in totals]           # param, grad, buf: canaries are random numbers
    host[1] *= F32(0.1)

    def view(buf, r, i):
        return buf[r][starts[r][i]:starts[r][i] + NF_SIZES[i]]

    for i, first in enumerate(NF_FIRST):
        if first:
            view(host, 2, i)[:] = np.nan                        # "uninitialised": the skip must leave +0 here
    good = view(host, 1, 3)[NF_POS[where]]
    view(host, 1, 3)[NF_POS[where]] = value
    dev = [torch.from_numpy(h).to(DEV) for h in host]
    assert all(d.data_ptr() % 16 == 0 for d in dev)
    grads = [view(dev, 1, i) for i in range(4)]
    lrs, wds = [0.1, 0.2, 0.05, 0.3], [0.0, 5e-4, 5e-4, 0.0]
    items = [(view(dev, 0, i), grads[i], view(dev, 2, i), lrs[i], wds[i], NF_FIRST[i]) for i in range(4)]
    state = None
    for call in (1, 2):
        state = ops.grad_norm_clip(grads, 1.0, state=state)
        norm, coef, finite, bad = read(state)
        assert not np.isfinite(norm) and finite == 0 and bad == call, (norm, finite, bad)
        assert coef.view(np.uint32) == 0                        # +0.0
    ops.sgd_step(items, 0.9, 0.0, False, 1.0, clip_state=state)
    got = [d.cpu().numpy() for d in dev]
    assert np.array_equal(got[1].view(np.uint32), host[1].view(np.uint32)), 'gradients were written'
    assert np.array_equal(got[0].view(np.uint32), host[0].view(np.uint32)), 'parameters moved in a skipped step'
    want_buf = host[2].copy()
    for i, first in enumerate(NF_FIRST):
        if first:
            view([None, None, want_buf], 2, i)[:] = 0.0
    assert np.array_equal(got[2].view(np.uint32), want_buf.view(np.uint32)), \
        'momentum buffers: existing ones keep their bits, first-step ones are +0, canaries stay'
    # the next step, finite again, continues from that state: no tensor is a first step any more
    host[2] = want_buf
    view(host, 1, 3)[NF_POS[where]] = good
    dev[1].copy_(torch.from_numpy(host[1]))
    gh = [view(host, 1, i) for i in range(4)]
    max_norm = 0.5 * clip_ref.norm64(gh)
    state = ops.grad_norm_clip(grads, max_norm, state=state)
    _, coef = check_state(state, gh, max_norm, nonfinite=2, tag='after the skip')
    items = [it[:5] + (False,) for it in items]
    ops.sgd_step(items, 0.9, 0.0, False, 1.0, clip_state=state)
    for i in range(4):
        p, b = sgd_ref.step(view(host, 0, i), gh[i], view(host, 2, i), lrs[i], wds[i], 0.9, 0.0, False,
                            grad_scale=F32(1.0) * coef, first_step=False)
        view(host, 0, i)[:] = p
        view(host, 2, i)[:] = b
    got = [d.cpu().numpy() for d in dev]
    assert sgd_ref.bits_equal(got[0], host[0]) and sgd_ref.bits_equal(got[2], host[2])
    assert np.array_equal(got[1].view(np.uint32), host[1].view(np.uint32))


# 5 -----------------------------------------------------------------------------------------------------------------
STEP_SIZES = [1, 3, 63, 4097, 8193]
STEP_OFFS = [(0, 0, 0), (1, 1, 1), (2, 3, 2), (3, 3, 3), (0, 1, 2)]


class StepArena:
    """(param, grad, buf) views into three flat device buffers with random canaries, and the host's expected image
    of each WHOLE buffer."""

    def __init__(self, seed):
        rng = np.random.RandomState(seed)
        self.starts, totals = zip(*[layout(STEP_SIZES, [o[r] for o in STEP_OFFS]) for r in range(3)])
        self.host = [rng.randn(t).astype(F32) for t in totals]
        self.dev = [torch.from_numpy(h).to(DEV) for h in self.host]
        self.rng = rng

    def view(self, r, i, dev=True):
        s = self.starts[r][i]
        return (self.dev[r] if dev else self.host[r])[s:s + STEP_SIZES[i]]

    def new_grads(self, scale):
        for i in range(len(STEP_SIZES)):
            self.view(1, i, False)[:] = (self.rng.randn(STEP_SIZES[i]) * scale).astype(F32)
        self.dev[1].copy_(torch.from_numpy(self.host[1]))

    def items(self, lrs, wds, has_buf, first):
        return [(self.view(0, i), self.view(1, i), self.view(2, i) if has_buf else None, lrs[i], wds[i], first)
                for i in range(len(STEP_SIZES))]

    def same_bits(self, other=None):
        got = [d.cpu().numpy() for d in self.dev]
        want = self.host if other is None else [d.cpu().numpy() for d in other.dev]
        return [sgd_ref.bits_equal(g, w) for g, w in zip(got, want)]


@pytest.mark.parametrize('ratio', [0.5, 10.0])
@pytest.mark.parametrize('grad_scale', [1.0, 0.125])
@pytest.mark.parametrize('wd', [0.0, 5e-4])
@pytest.mark.parametrize('momentum,dampening,nesterov', TRIPLES)
def test_clipped_step_bit_for_bit(momentum, dampening, nesterov, wd, grad_scale, ratio):
    """Three steps with fresh gradients each, max_norm at `ratio` times that step's norm: params and momentum buffers
    equal sgd_ref.step(grad_scale = f32(gs) * coef) bit for bit, canaries and gradients keep their bits; at ratio 10
    (coef == 1) a second arena driven by plain ops.sgd_step holds the same bits."""
    a, plain = StepArena(61), StepArena(61)
    n = len(STEP_SIZES)
    lrs = [0.01 * (1 + i) for i in range(n)]
    wds = [0.0 if i == 2 else wd for i in range(n)]
    has_buf = momentum != 0
    state = ws = None
    for it in range(3):
        for arena in (a, plain):
            arena.new_grads(10.0 ** (it - 1))
        gh = [a.view(1, i, False) for i in range(n)]
        gd = [a.view(1, i) for i in range(n)]
        max_norm = ratio * clip_ref.norm64(gh, grad_scale)
        if ws is None:
            ws = torch.empty(ops.grad_norm_workspace_bytes(gd), device=DEV, dtype=torch.uint8)
        state = ops.grad_norm_clip(gd, max_norm, grad_scale, state=state, workspace=ws)
        _, coef = check_state(state, gh, max_norm, grad_scale, tag='step %d' % it)
        assert (coef == 1) == (ratio > 1)
        ops.sgd_step(a.items(lrs, wds, has_buf, it == 0), momentum, dampening, nesterov, grad_scale, clip_state=state)
        for i in range(n):
            p, b = sgd_ref.step(a.view(0, i, False), gh[i], a.view(2, i, False) if has_buf else None, lrs[i], wds[i],
                                momentum, dampening, nesterov, grad_scale=F32(grad_scale) * coef, first_step=it == 0)
            a.view(0, i, False)[:] = p
            if has_buf:
                a.view(2, i, False)[:] = b
        assert a.same_bits() == [True, True, True], 'step %d: (param, grad, buf) against the restatement' % it
        if ratio > 1:
            ops.sgd_step(plain.items(lrs, wds, has_buf, it == 0), momentum, dampening, nesterov, grad_scale)
            assert a.same_bits(plain) == [True, True, True], 'step %d: coef == 1 against plain sgd_step' % it


# 6 -----------------------------------------------------------------------------------------------------------------
def test_determinism_and_a_dirty_workspace():
    sizes = [3 * 8192 + 5, 257, 8192, 70001, 1]
    a = GradArena(sizes, [1, 0, 0, 3, 2], seed=67)
    gd = a.views()
    need = ops.grad_norm_workspace_bytes(gd)
    assert need == 8 * sum(-(-(n + o) // CHUNK) for n, o in zip(sizes, [1, 0, 0, 3, 2]))
    out = []
    for fill in (0x00, 0xFF, None, None):
        ws = torch.empty(need, device=DEV, dtype=torch.uint8) if fill is None else \
            torch.full((need,), fill, device=DEV, dtype=torch.uint8)
        out.append(ops.grad_norm_clip(gd, 3.0, workspace=ws).cpu().numpy().tobytes())
    again = ops.grad_norm_clip(gd, 3.0)
    out.append(again.cpu().numpy().tobytes())
    assert len(set(out)) == 1, out
    check_state(again, a.views(False), 3.0, tag='determinism')
    with pytest.raises(_lib.CtdetError):                        # one byte short: refused, nothing launched
        ops.grad_norm_clip(gd, 3.0, workspace=torch.empty(need - 1, device=DEV, dtype=torch.uint8))
    with pytest.raises(_lib.CtdetError):
        ops.grad_norm_clip(gd, 0.0)
    with pytest.raises(_lib.CtdetError):                        # no CPU path
        ops.grad_norm_clip([torch.ones(4)], 1.0, state=again)


# 7 -----------------------------------------------------------------------------------------------------------------
def _report(tag, rows):
    worst = max(rows, key=lambda r: r[2] / r[4])
    print('%s: %d tensors, max|fused - fp64| %.3e, max|torch_cpu - fp64| %.3e, worst %s: fused %.3e torch %.3e bound %.3e'
          % (tag, len(rows), max(r[2] for r in rows), max(r[3] for r in rows), worst[0], worst[2], worst[3], worst[4]))
    assert all(r[1] for r in rows), [r for r in rows if not r[1]][:5]


def _coef64(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


def test_fused_sgd_with_max_grad_norm_against_torch_cpu():
    """Four parameters in two groups with different momenta, one without a gradient, four steps of which the third
    holds an Inf: FusedSGD(max_grad_norm=0.5) against clip_grad_norm_ + torch.optim.SGD on the CPU, which skips that
    step by hand, both measured against the fp64 evaluation."""
    torch.manual_seed(1)
    shapes = (1000, 77, 4099, 5)
    start = [torch.randn(n) for n in shapes]
    grads = [[torch.randn(n) * 1e-2 for n in shapes] for _ in range(4)]
    grads[1] = [g * 0.1 for g in grads[1]]                      # one step under the threshold: coef == 1
    grads[2][3][2] = math.inf
    max_norm = 0.5
    hyper = [(0.1, 5e-4, 0.9), (0.1, 5e-4, 0.9), (0.2, 0.0, 0.5), (0.2, 0.0, 0.5)]

    def groups(ps):
        return [{'params': ps[:2], 'momentum': 0.9}, {'params': ps[2:], 'momentum': 0.5, 'lr': 0.2, 'weight_decay': 0.0}]

    pd = [torch.nn.Parameter(s.clone().to(DEV)) for s in start]
    pc = [torch.nn.Parameter(s.clone()) for s in start]
    opt_d = FusedSGD(groups(pd), 0.1, momentum=0.9, weight_decay=5e-4, max_grad_norm=max_norm)
    opt_c = torch.optim.SGD(groups(pc), 0.1, momentum=0.9, weight_decay=5e-4)
    plain = FusedSGD(groups([torch.nn.Parameter(s.clone().to(DEV)) for s in start]), 0.1, momentum=0.9, weight_decay=5e-4)
    p64, b64 = [s.numpy().astype(np.float64) for s in start], [None] * 4
    coefs = []
    for it in range(4):
        live = [i for i in range(4) if i != 1]
        for i in range(4):
            pd[i].grad = None if i == 1 else grads[it][i].to(DEV)
            pc[i].grad = None if i == 1 else grads[it][i].clone()
            plain.param_groups[i // 2]['params'][i % 2].grad = None if i == 1 else torch.zeros(shapes[i], device=DEV)
        opt_d.step()
        plain.step()
        assert opt_d.last_calls == plain.last_calls == 2        # one step call per momentum triple, as without clipping
        n64 = clip_ref.norm64([grads[it][i].numpy() for i in live])
        if not math.isfinite(n64):
            assert it == 2
            continue                                            # the torch side skips the step by hand
        total = torch.nn.utils.clip_grad_norm_([pc[i] for i in live], max_norm)
        assert abs(float(total) - n64) <= 1e-5 * n64
        opt_c.step()
        c64 = _coef64(n64, max_norm)
        coefs.append(c64)
        for i in live:
            lr, wd, m = hyper[i]
            p64[i], b64[i] = sgd_ref.step(p64[i], grads[it][i].numpy().astype(np.float64) * c64, b64[i], lr, wd, m, 0.0,
                                          False, first_step=b64[i] is None, dtype=np.float64)
    assert coefs[1] == 1.0 and coefs[0] < 1.0 and coefs[2] < 1.0
    info = opt_d.clip_info()
    assert set(info) == {'norm', 'coef', 'finite', 'nonfinite'}
    assert info['nonfinite'] == 1 and info['finite'] is True and info['coef'] == float(F32(info['coef'])) < 1.0
    assert clip_ref.ulps_apart(F32(info['norm']), clip_ref.norm32([grads[3][i].numpy() for i in (0, 2, 3)])) <= 1
    assert opt_d.clip_state.numel() == 16 and opt_d.clip_state.is_cuda
    rows = []
    for i in (0, 2, 3):
        rows.append(('param %d' % i,) + sgd_ref.close_to_torch(pd[i].detach().cpu().numpy(), pc[i].detach().numpy(), p64[i]))
    _report('FusedSGD(max_grad_norm), 4 steps', rows)
    assert torch.equal(pd[1].detach().cpu(), start[1]) and pd[1] not in opt_d.state
    assert set(opt_d.state_dict()['param_groups'][0]) == set(opt_c.state_dict()['param_groups'][0])


def test_fused_sgd_guard_only_matches_the_plain_optimizer_bit_for_bit():
    """max_grad_norm = inf: coef is 1 in every finite step, so the bits are those of FusedSGD without the option; an
    Inf step is skipped and counted."""
    torch.manual_seed(3)
    start = [torch.randn(n) for n in (513, 8195)]
    out = {}
    for tag, kw in (('plain', {}), ('guard', {'max_grad_norm': math.inf})):
        ps = [torch.nn.Parameter(s.clone().to(DEV)) for s in start]
        opt = FusedSGD(ps, 0.1, momentum=0.9, weight_decay=5e-4, **kw)
        opt.grad_scale = 0.5
        gen = torch.Generator().manual_seed(9)
        for it in range(4):
            gs = [torch.randn(s.shape, generator=gen) for s in start]
            if it == 2:
                if tag == 'plain':
                    continue
                gs[1][-1] = math.nan
            for p, g in zip(ps, gs):
                p.grad = g.to(DEV)
            opt.step()
        out[tag] = [p.detach().cpu().numpy() for p in ps] + [opt.state[p]['momentum_buffer'].cpu().numpy() for p in ps]
        if kw:
            assert opt.clip_info()['nonfinite'] == 1 and opt.clip_info()['coef'] == 1.0
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(out['plain'], out['guard']))


# 8 -----------------------------------------------------------------------------------------------------------------
def test_in_the_training_step():
    """RFBNet-300 bs 2 as in tests/test_gpu_sgd_fused.py::test_in_the_training_step: one backward, then
    FusedSGD(max_grad_norm = half of the fp64 norm of those gradients)."""
    from data import VOC_300
    from layers.functions import PriorBox
    from layers.modules.multibox_loss_combined import MultiBoxLoss_combined
    from models.RFB_Net_vgg import build_net
    args = types.SimpleNamespace(method='ours', phase=1, setting='transfer')
    net = build_net(args, 300, 20)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()), strict=True)
    net = net.cuda()
    net.device = 'cuda'
    net.train()
    assert net.train_runtime(2) is not None
    priors = PriorBox(VOC_300).forward().cuda()
    crit = MultiBoxLoss_combined(21, 0.5, True, 0, True, 3, 0.5, False)
    x = synth.images(2, 300, 'randn', 1234).cuda()
    tg = [t.cuda() for t in synth.targets(2, 21, 99)]
    sum(crit(net(x), priors, tg).values()).backward()
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    assert all(p.grad is not None for _, p in named)
    grads = [p.grad.detach().clone() for _, p in named]
    gh = [g.cpu().numpy() for g in grads]
    n64 = clip_ref.norm64(gh)
    assert math.isfinite(n64) and n64 > 0
    max_norm = 0.5 * n64
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for _, p in named]
    p64 = [c.detach().numpy().astype(np.float64) for c in cpu]
    for c, g in zip(cpu, gh):
        c.grad = torch.from_numpy(g.copy())
    kw = dict(lr=1e-3, momentum=0.9, weight_decay=5e-4)
    torch.nn.utils.clip_grad_norm_(cpu, max_norm)
    torch.optim.SGD(cpu, **kw).step()
    for (_, p), g in zip(named, grads):
        p.grad = g
    opt = FusedSGD([p for _, p in named], max_grad_norm=max_norm, **kw)
    opt.step()
    assert opt.last_calls == 1
    norm, coef = check_state(opt.clip_state, gh, max_norm, tag='training step, %d tensors' % len(gh))
    assert 0.49 < coef < 0.51
    c64 = _coef64(n64, max_norm)
    rows = []
    for (n, p), c, r, g in zip(named, cpu, p64, gh):
        ref, _ = sgd_ref.step(r, g.astype(np.float64) * c64, None, kw['lr'], kw['weight_decay'], 0.9, 0.0, False,
                              first_step=True, dtype=np.float64)
        rows.append((n,) + sgd_ref.close_to_torch(p.detach().cpu().numpy(), c.detach().numpy(), ref))
    _report('clipped training step', rows)
    loss = sum(crit(net(x), priors, tg).values())
    assert bool(torch.isfinite(loss)), float(loss)


# 9 -----------------------------------------------------------------------------------------------------------------
def test_side_stream_gives_the_same_bits():
    out = []
    for stream in (None, torch.cuda.Stream()):
        a = StepArena(71)
        n = len(STEP_SIZES)
        lrs, wds = [0.01 * (1 + i) for i in range(n)], [5e-4] * n
        states = []
        state = None
        for it in range(3):
            a.new_grads(0.1)
            gd = [a.view(1, i) for i in range(n)]
            max_norm = 0.5 * clip_ref.norm64([a.view(1, i, False) for i in range(n)])
            if stream is None:
                state = ops.grad_norm_clip(gd, max_norm, state=state)
                ops.sgd_step(a.items(lrs, wds, True, it == 0), 0.9, 0.0, False, 1.0, clip_state=state)
            else:
                done = torch.cuda.Event()
                stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    state = ops.grad_norm_clip(gd, max_norm, state=state)
                    ops.sgd_step(a.items(lrs, wds, True, it == 0), 0.9, 0.0, False, 1.0, clip_state=state)
                    done.record()
                torch.cuda.current_stream().wait_event(done)
            states.append(state.cpu().numpy().tobytes())
        torch.cuda.synchronize()
        out.append([d.cpu().numpy() for d in a.dev] + [np.frombuffer(b''.join(states), np.uint8)])
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(*out))
    assert np.isfinite(out[0][0]).all()
