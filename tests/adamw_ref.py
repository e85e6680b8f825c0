"""ct_adamw_begin and ct_adamw_step (include/ctdet.h) restated in NumPy, one operation per line, so that every operation
is rounded once to `dtype`.  dtype=float32 is what the kernels must reproduce bit for bit; dtype=float64 runs the same
lines on the same fp32 inputs.  step() also reports whether any fp32 intermediate was subnormal: the bit-for-bit claim
is made for inputs on which none is.

Separately, definition() is AdamW as torch documents it (decoupled weight decay, amsgrad=False), in float64 with
Python-double hyperparameters and beta ** t: the yardstick the restatement, the kernels and torch's CPU AdamW are all
measured against (tests/sgd_ref.py::close_to_torch is the rule).

Only data and arithmetic live here; nothing of the code under test is imported.  The averaging line of a step with a
weight average comes from tests/ema_ref.py, the clipping coefficient from tests/clip_ref.py.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
INT_MAX = 2 ** 31 - 1
TINY = np.finfo(np.float32).tiny                # the smallest normal fp32


class State:
    """The 32 bytes of ct_adam_state."""

    def __init__(self, step=0, beta1_pow=0.0, beta2_pow=0.0):
        self.beta1_pow = F64(beta1_pow)
        self.beta2_pow = F64(beta2_pow)
        self.step = int(step)
        self.applied = 0
        self.bc1 = F32(0.0)
        self.rs2 = F32(0.0)

    def __repr__(self):
        return 'State(step=%d, beta1_pow=%r, beta2_pow=%r, applied=%d, bc1=%r, rs2=%r)' % (
            self.step, self.beta1_pow, self.beta2_pow, self.applied, self.bc1, self.rs2)

    def record(self):
        """(beta1_pow, beta2_pow, step, applied, bc1, rs2) with the floats as their bit patterns."""
        return (self.beta1_pow.view(np.uint64), self.beta2_pow.view(np.uint64), self.step, self.applied,
                self.bc1.view(np.uint32), self.rs2.view(np.uint32))


def begin(state, beta1, beta2, finite=None):
    """ct_adamw_begin on one record; `finite` is clip->finite, None without a clip state.  Changes and returns it."""
    ok = 1 if finite is None else int(bool(finite))
    if not ok:
        state.applied = 0
        return state
    beta1, beta2 = F64(beta1), F64(beta2)
    b1p = (F64(1.0) if state.step == 0 else state.beta1_pow) * beta1
    b2p = (F64(1.0) if state.step == 0 else state.beta2_pow) * beta2
    d1 = F64(1.0) - b1p
    d2 = F64(1.0) - b2p
    bc1 = F32(d1)
    bc2 = F32(d2)
    rs2 = np.sqrt(bc2)
    assert all(isinstance(v, np.float64) for v in (b1p, b2p)) and all(isinstance(v, np.float32) for v in (bc1, rs2))
    state.beta1_pow, state.beta2_pow = b1p, b2p
    state.step = state.step if state.step == INT_MAX else state.step + 1
    state.applied = 1
    state.bc1, state.rs2 = bc1, rs2
    return state


def _subnormal(*arrays):
    return any(bool(((np.abs(a) > 0) & (np.abs(a) < TINY)).any()) for a in arrays)


def step(p, g, m, v, state, lr, weight_decay, beta1, beta2, eps, grad_scale=1.0, dtype=np.float32):
    """One update with the bias corrections begin() left in `state`.  p, g, m, v: arrays -> (new p, new m, new v,
    flag), new arrays of `dtype`; flag: some intermediate was a subnormal fp32 value (always False for float64)."""
    lr32, wd32, b1_32, b2_32 = F32(lr), F32(weight_decay), F32(beta1), F32(beta2)
    om1 = F32(1.0 - float(b1_32))                       # (1 - beta): in binary64 from the fp32 beta, rounded once
    om2 = F32(1.0 - float(b2_32))
    lw = lr32 * wd32                                    # one fp32 rounding
    a = lr32 / state.bc1                                # one fp32 division
    assert all(isinstance(x, np.float32) for x in (om1, om2, lw, a))
    b1, b2, om1, om2, lw, a, rs2, eps, gs = (dtype(x) for x in (b1_32, b2_32, om1, om2, lw, a, state.rs2, F32(eps),
                                                                F32(grad_scale)))
    p = np.asarray(p).astype(dtype)
    g = np.asarray(g).astype(dtype)
    m = np.asarray(m).astype(dtype)
    v = np.asarray(v).astype(dtype)
    seen = []
    with np.errstate(all='ignore'):
        g = g * gs
        seen.append(g)
        if wd32 != 0:
            t = lw * p
            p = p - t
            seen += [t, p]
        t1 = b1 * m
        t2 = om1 * g
        m = t1 + t2
        u1 = b2 * v
        u2 = om2 * g
        u3 = u2 * g
        v = u1 + u3
        s = np.sqrt(v)
        q = s / rs2
        den = q + eps
        r = m / den
        w = a * r
        p = p - w
        seen += [t1, t2, m, u1, u2, u3, v, s, q, den, r, w, p]
    flag = dtype == np.float32 and _subnormal(a, lw, *seen)
    return p, m, v, bool(flag)


def definition(p, grads, lr, betas, eps, weight_decay, grad_scale=1.0, t0=0, m=None, v=None):
    """AdamW itself, float64, Python-double hyperparameters, beta ** t: `grads` is the list of one gradient per step
    (None: the tensor has no gradient in that step and does not count it), steps t0 + 1 ...  -> (p, m, v, steps)."""
    b1, b2 = float(betas[0]), float(betas[1])
    lr, eps, wd, gs = float(lr), float(eps), float(weight_decay), float(grad_scale)
    p = np.asarray(p, dtype=F64).copy()
    m = np.zeros_like(p) if m is None else np.asarray(m, dtype=F64).copy()
    v = np.zeros_like(p) if v is None else np.asarray(v, dtype=F64).copy()
    t = int(t0)
    with np.errstate(all='ignore'):
        for g in grads:
            if g is None:
                continue
            t += 1
            g = np.asarray(g, dtype=F64) * gs
            p = p * (1.0 - lr * wd)
            m = b1 * m + (1.0 - b1) * g
            v = b2 * v + (1.0 - b2) * g * g
            bc1 = 1.0 - b1 ** t
            bc2 = 1.0 - b2 ** t
            p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    return p, m, v, t


def widened(beta):
    """The fp32 value of `beta` as a double: what the step's recurrence runs with, handed to begin() as well so that
    the bias corrections belong to the same beta (FusedAdamW does this; with the unrounded 0.999 in begin(), 1 - beta2
    there and in the recurrence differ by 1.3e-5 of their value)."""
    return float(F32(beta))


def loaded(step, betas):
    """The record FusedAdamW.load_state_dict() builds for a tensor that took `step` steps: beta ** step in Python
    double."""
    return State(step, widened(betas[0]) ** step, widened(betas[1]) ** step) if step else State()


class Run:
    """One tensor under the restatement, driven the way FusedAdamW drives the two entries: p, m, v and its record,
    begin() with the widened fp32 betas, then step()."""

    def __init__(self, p, betas=(0.9, 0.999), eps=1e-8, dtype=np.float32, m=None, v=None, state=None):
        self.dtype = dtype
        self.p = np.asarray(p).astype(dtype)
        self.m = np.zeros_like(self.p) if m is None else np.asarray(m).astype(dtype)
        self.v = np.zeros_like(self.p) if v is None else np.asarray(v).astype(dtype)
        self.betas, self.eps = betas, eps
        self.state = State() if state is None else state
        self.flag = False

    def step(self, g, lr, weight_decay, grad_scale=1.0, finite=None):
        begin(self.state, widened(self.betas[0]), widened(self.betas[1]), finite)
        if not self.state.applied:
            return self
        self.p, self.m, self.v, flag = step(self.p, g, self.m, self.v, self.state, lr, weight_decay, self.betas[0],
                                            self.betas[1], self.eps, grad_scale, self.dtype)
        self.flag = self.flag or flag
        return self


def grads_like(rng, n, zeros=0.1):
    """One gradient: magnitudes spread log-uniformly over 1e-4 .. 1, a share of exact zeros."""
    g = (rng.randn(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(F32)
    g[rng.rand(n) < zeros] = 0.0
    return g


ACCURACY_SETTINGS = [(lr, wd) for lr in (1e-3, 4e-3) for wd in (0.0, 5e-4, 1e-2)]


def accuracy_inputs(steps=40, n=20000, seed=7):
    """The parameters (weights of magnitude up to about 1) and per-step gradients of the accuracy checks."""
    rng = np.random.RandomState(seed)
    p = (rng.randn(n) * 0.25).astype(F32)
    return p, [grads_like(rng, n) for _ in range(steps)]
