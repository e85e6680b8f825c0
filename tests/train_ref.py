"""Plain reference of the non-convolution training kernels (csrc/ct_train.hip), written from the mathematics in
include/ctdet.h and the kernel comments: torch-CPU tensor arithmetic, no autograd, no device.

Every function takes the arguments of its C entry point: FULL buffers (NCHW with `ctot` channels) plus the channel
offset of the slice, the flags, `accumulate`.  Every output buffer the entry point writes is passed in with its
previous contents and returned as an updated COPY, so a caller can check the channels outside the slice too.

`dtype` is the arithmetic: torch.float64 is the reference; torch.float32 evaluates the same formula the way a float32
machine would, which is what the tests use to judge how exact a float32 kernel can be on an input (`e32`).
tests/test_train_ref_cpu.py proves the float64 form against torch autograd."""
import torch

F64 = torch.float64


def _t(a, dtype):
    return None if a is None else torch.as_tensor(a).to(dtype)


def _sl(t, coff, C):
    return t[:, coff:coff + C]


def bn_stats(z, coff, C, momentum=0.0, running_mean=None, running_var=None, dtype=F64):
    """Biased mean / variance over (batch, hw) of channels [coff, coff+C) of z [B][ctot][HW]; the running statistics
    of nn.BatchNorm2d: r = (1-momentum)*r + momentum*stat, the variance scaled by n/(n-1) (by 1 where n == 1, the
    convention of ct_bn_train_stats).  Returns (mean, var, running_mean, running_var); the last two None if not given."""
    zs = _sl(_t(z, dtype), coff, C)
    B, _, HW = zs.shape
    n = B * HW
    mean = zs.sum((0, 2)) / n
    var = ((zs - mean[None, :, None]) ** 2).sum((0, 2)) / n
    rm = rv = None
    if running_mean is not None and running_var is not None:
        unbias = n / (n - 1.0) if n > 1 else 1.0
        rm = (1 - momentum) * _t(running_mean, dtype) + momentum * mean
        rv = (1 - momentum) * _t(running_var, dtype) + momentum * (var * unbias)
    return mean, var, rm, rv


def bn_apply(z, z_coff, mean, var, gamma, beta, eps, relu, lo, res, res_coff, res_scale, y, y_coff, dtype=F64):
    """y[:, y_coff:+C] = act(((z - mean) / sqrt(var + eps)) * gamma + beta [* res_scale + res]);
    act = max(., lo[c]) when lo is given, else ReLU when relu, else nothing."""
    mean, var, gamma, beta = (_t(a, dtype) for a in (mean, var, gamma, beta))
    C = mean.numel()
    b = lambda a: a[None, :, None]
    v = (_sl(_t(z, dtype), z_coff, C) - b(mean)) / torch.sqrt(b(var) + eps) * b(gamma) + b(beta)
    if res is not None:
        v = v * res_scale + _sl(_t(res, dtype), res_coff, C)
    if lo is not None:
        v = torch.maximum(v, b(_t(lo, dtype)))
    elif relu:
        v = torch.clamp_min(v, 0)
    out = _t(y, dtype).clone()
    out[:, y_coff:y_coff + C] = v
    return out


def bn_mask(y, y_coff, C, relu, lo):
    """Where the activation stops the gradient: y <= 0 on the channels that have a ReLU (lo[c] == 0 where lo is given
    -- a channel with lo == -inf has none -- else every channel when relu).  Bool [B][C][HW]."""
    if lo is not None:
        act = torch.as_tensor(lo) == 0
    else:
        act = torch.full((C,), bool(relu))
    if not bool(act.any()):
        return torch.zeros((y.shape[0] if y is not None else 1, C, 1), dtype=torch.bool)
    return (_sl(torch.as_tensor(y), y_coff, C) <= 0) & act[None, :, None]


def bn_backward(frozen, dy, dy_coff, y, y_coff, z, z_coff, mean, var, gamma, eps, relu, lo, res_scale,
                dres, dres_coff, dres_accumulate, dz, dtype=F64):
    """Backward of bn_apply.  gm = dy where the mask lets it through (else 0) is the residual branch's gradient (set
    into or added to dres[:, dres_coff:+C]); g = gm * res_scale; dbeta = sum g, dgamma = sum g * xhat;
    dz = gamma/sqrt(var+eps) * (g - dbeta/n - xhat*dgamma/n), without the two statistics terms when `frozen`.
    Returns (dz, dgamma, dbeta, dres) with dz / dres the updated full buffers (dres None if not given)."""
    mean, var, gamma = (_t(a, dtype) for a in (mean, var, gamma))
    C = mean.numel()
    b = lambda a: a[None, :, None]
    gm = _sl(_t(dy, dtype), dy_coff, C).clone()
    B, _, HW = gm.shape
    n = B * HW
    gm = torch.where(bn_mask(y, y_coff, C, relu, lo).expand_as(gm), torch.zeros((), dtype=dtype), gm)
    inv = 1 / torch.sqrt(var + eps)
    xh = (_sl(_t(z, dtype), z_coff, C) - b(mean)) * b(inv)
    g = gm * res_scale
    dbeta = g.sum((0, 2))
    dgamma = (g * xh).sum((0, 2))
    d = b(gamma * inv) * (g if frozen else g - b(dbeta) / n - xh * b(dgamma) / n)
    dz_out = _t(dz, dtype).clone()
    dz_out[:, z_coff:z_coff + C] = d
    dres_out = None
    if dres is not None:
        dres_out = _t(dres, dtype).clone()
        if dres_accumulate:
            dres_out[:, dres_coff:dres_coff + C] += gm
        else:
            dres_out[:, dres_coff:dres_coff + C] = gm
    return dz_out, dgamma, dbeta, dres_out


def bias_act_backward(dy, dy_coff, y, y_coff, relu, C, dz, dz_coff, dtype=F64):
    """y = act(conv + bias): dz[:, dz_coff:+C] = dy * (y > 0 if relu), dbias[c] = sum dz, amax[n] = max |dz| of image n.
    dy and dz may be the same buffer (the heads' in-place form).  Returns (dz, dbias, amax)."""
    g = _sl(_t(dy, dtype), dy_coff, C).clone()
    if relu:
        g = torch.where(_sl(torch.as_tensor(y), y_coff, C) <= 0, torch.zeros((), dtype=dtype), g)
    out = _t(dz, dtype).clone()
    out[:, dz_coff:dz_coff + C] = g
    return out, g.sum((0, 2)), g.abs().amax((1, 2))


def maxpool_bwd(x, dy, k, stride, pad, dx, accumulate, dtype=F64):
    """max_pool2d backward on planes x [P][H][W], dy [P][OH][OW]: every window (clipped to the plane) sends its dy to
    its FIRST maximum in row-major order; an element sums what it receives in row-major window order, then is set into
    or added to dx.  Windows are compared in the dtype of x (exact)."""
    x = torch.as_tensor(x)
    P, H, W = x.shape
    dy = _t(dy, dtype)
    OH, OW = dy.shape[1:]
    g = torch.zeros((P, H * W), dtype=dtype)
    pl = torch.arange(P)
    for oh in range(OH):
        h0, h1 = max(oh * stride - pad, 0), min(oh * stride - pad + k, H)
        for ow in range(OW):
            w0, w1 = max(ow * stride - pad, 0), min(ow * stride - pad + k, W)
            if h1 <= h0 or w1 <= w0:
                continue
            win = x[:, h0:h1, w0:w1].reshape(P, -1)
            m = win.max(1, keepdim=True).values
            first = (win == m).to(torch.uint8).argmax(1)           # first index holding the maximum (-0.0 == +0.0)
            hh, ww = h0 + first // (w1 - w0), w0 + first % (w1 - w0)
            g[pl, hh * W + ww] += dy[:, oh, ow]
    g = g.view(P, H, W)
    return _t(dx, dtype) + g if accumulate else g


def maxpool2x2_bias_relu_bwd(y, y_coff, C, dy, dz, dz_coff, dtype=F64):
    """MaxPool2d(2, 2) backward (floor or ceil mode, from the shape of dy [B][C][OH][OW]) through the ReLU of the
    convolution under it: dz = (y > 0) * [first maximum of its window] * dy over the whole slice (elements no window
    covers get 0), dbias[c] = sum dz, amax[n] = max |dz| of image n.  y, dz: [B][ctot][H][W].  Returns (dz, dbias, amax)."""
    ys = _sl(torch.as_tensor(y), y_coff, C)
    B, _, H, W = ys.shape
    yp = ys.reshape(B * C, H, W)
    g = maxpool_bwd(yp, torch.as_tensor(dy).reshape(B * C, *dy.shape[2:]), 2, 2, 0, None, 0, dtype)
    g = torch.where(yp <= 0, torch.zeros((), dtype=dtype), g).view(B, C, H, W)
    out = _t(dz, dtype).clone()
    out[:, dz_coff:dz_coff + C] = g
    return out, g.sum((0, 2, 3)), g.abs().amax((1, 2, 3))


def head_grad_gather(segs, B, C, HW):
    """Gradient of the channels-last head scatter: dz[n][c][i] = flat[n*img_stride + base + i*pix_stride + (c - co_begin)]
    for the segment (flat, co_begin, co_end, pix_stride, img_stride, base) that holds channel c (the last one if several
    do); channels outside every segment give 0.  A pure copy: the dtype of the first segment is kept."""
    dz = torch.zeros((B, C, HW), dtype=torch.as_tensor(segs[0][0]).dtype)
    n = torch.arange(B)[:, None, None]
    i = torch.arange(HW)[None, None, :]
    for flat, c0, c1, ps, istr, base in segs:
        c = torch.arange(c1 - c0)[None, :, None]
        dz[:, c0:c1] = torch.as_tensor(flat).reshape(-1)[n * istr + base + i * ps + c]
    return dz
