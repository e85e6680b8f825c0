"""The bicubic and Lanczos4 resize filters of ct_preproc_augment_taps (include/ctdet.h) restated in NumPy, one
operation per line and one output coordinate at a time, so that every operation is rounded once to the type named
on its line.  This is the project's definition of the two filters: OpenCV's 8-bit `resize` path (imgproc/resize.cpp)
as two fixed-point separable passes.

    taps(n, S, kind)        -> (first [S] int64, ic [S, k] int16): floor(f) and the 11-bit coefficients per output index
    coeffs(x, kind)         -> ic [k] int16 of one fraction x
    resize(img_u8, S, kind) -> uint8 [S, S, C] of an [H, W, C] uint8 image

kind: 'cubic' (k = 4) or 'lanczos4' (k = 8).  Where the definition leaves the type of an intermediate open this
file follows OpenCV's source: `x + 3 - i` is float32 arithmetic (x is a float), everything that touches pi is double.

Only data and arithmetic live here; nothing of the code under test is imported.
"""
import numpy as np

K = {'cubic': 4, 'lanczos4': 8}
f32 = np.float32
f64 = np.float64


def cubic_weights(x):
    x = f32(x)
    A = f32(-0.75)
    one = f32(1)
    xp = x + one
    c0 = A * xp
    c0 = c0 - f32(5) * A
    c0 = c0 * xp
    c0 = c0 + f32(8) * A
    c0 = c0 * xp
    c0 = c0 - f32(4) * A
    c1 = (A + f32(2)) * x
    c1 = c1 - (A + f32(3))
    c1 = c1 * x
    c1 = c1 * x
    c1 = c1 + one
    xm = one - x
    c2 = (A + f32(2)) * xm
    c2 = c2 - (A + f32(3))
    c2 = c2 * xm
    c2 = c2 * xm
    c2 = c2 + one
    c3 = one - c0
    c3 = c3 - c1
    c3 = c3 - c2
    return [c0, c1, c2, c3]


def lanczos4_weights(x):
    x = f32(x)
    s = 0.70710678118654752440084436210485
    cs = [(1, 0), (-s, -s), (0, 1), (s, -s), (-1, 0), (s, s), (0, -1), (-s, s)]
    y0 = -(f64(x) + 3.0)
    y0 = y0 * np.pi
    y0 = y0 * 0.25
    s0 = np.sin(y0)
    c0 = np.cos(y0)
    c = []
    total = f32(0)
    for i in range(8):
        t = x + f32(3)
        t = t - f32(i)
        if abs(t) >= f32(1e-6):
            y = -f64(t)
            y = y * np.pi
            y = y * 0.25
            num = cs[i][0] * s0 + cs[i][1] * c0
            ci = f32(num / (y * y))
        else:
            ci = f32(1e30)
        c.append(ci)
        total = total + ci
    inv = f32(1) / total
    return [ci * inv for ci in c]


def coeffs(x, kind):
    w = cubic_weights(x) if kind == 'cubic' else lanczos4_weights(x)
    assert len(w) == K[kind] and all(isinstance(v, np.float32) for v in w)
    ic = []
    for v in w:
        q = np.rint(v * f32(2048))                    # round half to even
        ic.append(int(min(max(q, -32768), 32767)))
    return np.array(ic, dtype=np.int16)


def taps(n, S, kind):
    k = K[kind]
    scale = 1.0 / (S / float(n))
    first = np.zeros(S, dtype=np.int64)
    ic = np.zeros((S, k), dtype=np.int16)
    for d in range(S):
        f = f32((d + 0.5) * scale - 0.5)
        fl = int(np.floor(f))
        x = f - f32(fl)
        first[d] = fl
        ic[d] = coeffs(x, kind)
    return first, ic


def indices(first, n, k):
    """Source index of every tap: clamp(first - (k/2 - 1) + j, 0, n - 1) -> [S, k]."""
    return np.clip(first[:, None] - (k // 2 - 1) + np.arange(k)[None, :], 0, n - 1)


def resize(img_u8, S, kind):
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8 and img.ndim == 3
    H, W = img.shape[:2]
    k = K[kind]
    fx, icx = taps(W, S, kind)
    fy, icy = taps(H, S, kind)
    ix, iy = indices(fx, W, k), indices(fy, H, k)
    P = img.astype(np.int64)
    h = np.zeros((H, S, img.shape[2]), dtype=np.int64)
    for j in range(k):
        h += icx[:, j].astype(np.int64)[None, :, None] * P[:, ix[:, j], :]
    v = np.zeros((S, S, img.shape[2]), dtype=np.int64)
    for j in range(k):
        v += icy[:, j].astype(np.int64)[:, None, None] * h[iy[:, j], :, :]
    assert np.abs(h).max() < 2 ** 31 and np.abs(v).max() < 2 ** 31 - 2 ** 21       # the int32 of the definition holds them
    return np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
