"""ct_grad_norm_clip (include/ctdet.h) restated: the norm in binary64 with an exactly rounded sum (math.fsum), and the
clipping coefficient in NumPy float32, one operation per line, so that every operation is rounded once.

Only data and arithmetic live here; nothing of the code under test is imported.
"""
import itertools
import math

import numpy as np

F32 = np.float32
EPS = F32(1e-6)


def norm64(grads, grad_scale=1.0):
    """sqrt(exactly rounded sum of float(g)^2 over every element of every array) * |f32(grad_scale)|, in binary64.
    Each square of an fp32 value is exact in binary64."""
    flats = [np.asarray(g, dtype=np.float32).ravel() for g in grads]
    if any(np.isnan(f).any() for f in flats):
        return float('nan')
    if any(np.isinf(f).any() for f in flats):
        return float('inf')

    def squares():                          # ONE fsum over all elements, a million at a time to bound the memory
        for f in flats:
            for i in range(0, f.size, 1 << 20):
                c = f[i:i + (1 << 20)].astype(np.float64)
                yield (c * c).tolist()

    return math.sqrt(math.fsum(itertools.chain.from_iterable(squares()))) * abs(float(F32(grad_scale)))


def norm32(grads, grad_scale=1.0):
    """What the device's `norm` is measured against: norm64 rounded once to fp32 (overflow gives inf)."""
    with np.errstate(all='ignore'):
        return F32(norm64(grads, grad_scale))


def coef(norm, max_norm):
    """The fp32 lines of the header from a given fp32 norm -> (coef, finite)."""
    norm, max_norm = F32(norm), F32(max_norm)
    if not np.isfinite(norm):
        return F32(0.0), 0
    with np.errstate(all='ignore'):
        t = norm + EPS
        q = max_norm / t
        c = min(F32(1.0), q)
    return F32(c), 1


def ulps_apart(a, b):
    """Distance of two finite non-negative fp32 values in units of the last place."""
    a, b = F32(a), F32(b)
    assert np.isfinite(a) and np.isfinite(b) and a >= 0 and b >= 0, (a, b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))
