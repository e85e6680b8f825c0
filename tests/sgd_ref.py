"""The recurrence of ct_sgd_step (include/ctdet.h) restated in NumPy, one operation per line, so that every operation
is rounded once to `dtype`.  dtype=float32 is what the kernel must reproduce bit for bit; dtype=float64 on the same
fp32 inputs (tensors AND the fp32-rounded scalars the C ABI takes) is the yardstick both the kernel and torch's CPU
SGD are measured against (torch is not bit-equal to the fp32 restatement: its vectorised CPU loops contract some
multiply-adds).

Only data and arithmetic live here; nothing of the code under test is imported.
"""
import numpy as np


def step(p, g, buf, lr, weight_decay, momentum, dampening, nesterov, grad_scale=1.0, first_step=False,
         dtype=np.float32):
    """One update.  p, g, buf: arrays (buf None iff momentum == 0) -> (new p, new buf), new arrays of `dtype`."""
    f32 = np.float32
    lr, wd, m, gs = (dtype(f32(v)) for v in (lr, weight_decay, momentum, grad_scale))
    omd = dtype(f32(1.0) - f32(dampening))              # (1 - dampening): once, in fp32
    p = np.asarray(p).astype(dtype)
    g = np.asarray(g).astype(dtype)
    with np.errstate(all='ignore'):
        g = g * gs
        d = g
        if wd != 0:
            t = wd * p
            d = g + t
        if m == 0:
            stp = d
            new_buf = None
        else:
            if first_step:
                new_buf = d.copy()
            else:
                a = m * np.asarray(buf).astype(dtype)
                b = omd * d
                new_buf = a + b
            if nesterov:
                t = m * new_buf
                stp = d + t
            else:
                stp = new_buf
        u = lr * stp
        p = p - u
    return p, new_buf


def bits_equal(a, b):
    """np.array_equal on the raw bits; NaN positions are compared as masks (their payload is not part of the claim)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def ulp(x):
    """Spacing of fp32 at |x|."""
    return float(np.spacing(np.float32(abs(float(x)))))


def close_to_torch(fused, torch_cpu, ref64, p_for_ulp=None):
    """The issue's tolerance: max|fused - fp64| <= 2 * max|torch_cpu - fp64| + ulp(max|p|).  -> (ok, e_fused, e_torch,
    bound); callers print the two errors before they assert."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    e_f = float(np.abs(np.asarray(fused, dtype=np.float64) - ref64).max()) if ref64.size else 0.0
    e_t = float(np.abs(np.asarray(torch_cpu, dtype=np.float64) - ref64).max()) if ref64.size else 0.0
    pm = np.abs(ref64 if p_for_ulp is None else np.asarray(p_for_ulp, dtype=np.float64))
    bound = 2.0 * e_t + ulp(pm.max() if pm.size else 0.0)
    return e_f <= bound, e_f, e_t, bound
