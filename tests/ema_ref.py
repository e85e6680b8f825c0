"""ct_ema_begin and the averaging line of ct_sgd_step_ema / ct_ema_update (include/ctdet.h) restated in NumPy, one
operation per line, so that every operation is rounded once.  The schedule (begin) is fp32 arithmetic whatever `dtype`
is; update(dtype=float32) is what the kernels must reproduce bit for bit, update(dtype=float64) evaluates the same
line in binary64 from the SAME fp32 d and fp32 (1 - d) and is the accuracy yardstick.

Only data and arithmetic live here; nothing of the code under test is imported.  The SGD and clipping parts of a step
come from tests/sgd_ref.py and tests/clip_ref.py.
"""
import numpy as np

F32 = np.float32
INT_MAX = 2 ** 31 - 1


class State:
    """The 16 bytes of ct_ema_state."""

    def __init__(self, updates=0):
        self.updates = int(updates)
        self.decay = F32(0.0)
        self.one_minus = F32(0.0)
        self.applied = 0

    def __repr__(self):
        return 'State(updates=%d, decay=%r, one_minus=%r, applied=%d)' % (self.updates, self.decay, self.one_minus,
                                                                          self.applied)


def begin(state, decay, warmup=0.0, finite=None):
    """ct_ema_begin; `finite` is clip->finite, None without a clip state.  Changes and returns `state`."""
    n = state.updates
    applied = 1 if finite is None else int(bool(finite))
    if not applied:
        state.applied = 0
        return state
    decay, warmup = F32(decay), F32(warmup)
    d = decay
    if warmup != 0:
        nf = F32(n)
        a = F32(1.0) + nf
        b = warmup + nf
        q = a / b
        d = min(decay, q)
    om = F32(1.0) - d
    assert all(isinstance(v, np.float32) for v in (d, om))
    state.updates = n if n == INT_MAX else n + 1
    state.decay = d
    state.one_minus = om
    state.applied = 1
    return state


def update(ema, x, state, dtype=np.float32):
    """The averaging line with the d / (1 - d) of `state` -> a new array of `dtype`; `ema` itself when the update was
    not applied."""
    if not state.applied:
        return ema
    d, om = dtype(state.decay), dtype(state.one_minus)
    ema = np.asarray(ema).astype(dtype)
    x = np.asarray(x).astype(dtype)
    with np.errstate(all='ignore'):
        t = d * ema
        u = om * x
        out = t + u
    return out


def accuracy_inputs(steps=50, n=20011, seed=5):
    """The parameter values of the accuracy tests: `steps` fp32 arrays whose magnitudes spread over 1e-3 .. 1e2 and
    that drift by about a percent per step, as a parameter under SGD does, and the starting average (= the start)."""
    rng = np.random.RandomState(seed)
    p = (rng.randn(n) * 10.0 ** rng.uniform(-3, 2, n)).astype(F32)
    start = p.copy()
    seq = []
    for _ in range(steps):
        p = (p - F32(0.01) * (rng.randn(n).astype(F32) * np.abs(p))).astype(F32)
        seq.append(p)
    return start, seq


def accuracy_run(start, seq, decay, warmup, dtype):
    """The average after len(seq) updates in `dtype` -> (ema, largest |ema| or |p| seen)."""
    state = State()
    ema = start.astype(dtype)
    m = float(np.abs(start).max())
    for p in seq:
        begin(state, decay, warmup)
        ema = update(ema, p, state, dtype)
        m = max(m, float(np.abs(ema).max()), float(np.abs(p).max()))
    return ema, m


def bound(decay, steps, m):
    """The accuracy bound of the feature's issue: three roundings per step of at most 2^-24 * m each, contracted by d
    per step, so the sum over the steps is at most 3 * 2^-24 * m * min(steps, 1 / (1 - decay))."""
    return 3.0 * 2.0 ** -24 * m * min(float(steps), 1.0 / (1.0 - float(decay)))
