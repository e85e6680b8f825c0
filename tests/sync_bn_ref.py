"""Synchronized BatchNorm in torch, step by step as the four ct_bn_sync_* entries (include/ctdet.h) split it, at a chosen dtype:
local sums -> (the caller's SUM over the ranks) -> finish / apply.  Dense [B][C][HW] tensors; the channel slicing of the device
entries is covered by tests/train_cases.py.  tests/test_sync_bn_ref_cpu.py proves the split against float64 autograd of
F.batch_norm over the concatenated batch."""
import torch

F64 = torch.float64


def _b(a):
    return a[None, :, None]


def stats_local(z, dtype=F64):
    """[2][C]: sum z, then sum z^2, over the shard."""
    z = z.to(dtype)
    return torch.stack([z.sum((0, 2)), (z * z).sum((0, 2))])


def stats_finish(sums, count, momentum=0.0, running_mean=None, running_var=None, dtype=F64):
    """mean, biased var (clamped at 0), and the running statistics (unbiased: count / (count - 1), 1 for count <= 1)."""
    s = sums.to(dtype)
    m = s[0] / count
    var = torch.clamp_min(s[1] / count - m * m, 0)
    rm = rv = None
    if running_mean is not None and running_var is not None:
        unbias = count / (count - 1.0) if count > 1 else 1.0
        rm = (1 - momentum) * running_mean.to(dtype) + momentum * m
        rv = (1 - momentum) * running_var.to(dtype) + momentum * (var * unbias)
    return m, var, rm, rv


def apply(z, mean, var, gamma, beta, eps, relu, lo, res, res_scale, dtype=F64):
    """ct_bn_train_apply: act(((z - mean) / sqrt(var + eps)) * gamma + beta [* res_scale + res])."""
    v = (z.to(dtype) - _b(mean.to(dtype))) / torch.sqrt(_b(var.to(dtype)) + eps) * _b(gamma.to(dtype)) + _b(beta.to(dtype))
    if res is not None:
        v = v * res_scale + res.to(dtype)
    if lo is not None:
        v = torch.maximum(v, _b(lo.to(dtype)))
    elif relu:
        v = torch.clamp_min(v, 0)
    return v


def _masked(dy, y, relu, lo, dtype):
    C = dy.shape[1]
    act = (lo == 0) if lo is not None else torch.full((C,), bool(relu))
    stop = (y <= 0) & act[None, :, None] if bool(act.any()) else torch.zeros_like(dy, dtype=torch.bool)
    return torch.where(stop, torch.zeros((), dtype=dtype), dy.to(dtype))


def backward_local(dy, y, z, mean, var, eps, relu, lo, res_scale, dtype=F64):
    """([2][C]: sum g, then sum g*xhat; dgamma; dbeta) of the shard, xhat from the GLOBAL mean / var."""
    g = _masked(dy, y, relu, lo, dtype) * res_scale
    xh = (z.to(dtype) - _b(mean.to(dtype))) / torch.sqrt(_b(var.to(dtype)) + eps)
    sums = torch.stack([g.sum((0, 2)), (g * xh).sum((0, 2))])
    return sums, sums[1].clone(), sums[0].clone()


def backward_apply(dy, y, z, mean, var, gamma, eps, relu, lo, res_scale, sums, count, dtype=F64):
    """(dz, the residual branch's gradient) of the shard from the REDUCED sums and the global count."""
    gm = _masked(dy, y, relu, lo, dtype)
    g = gm * res_scale
    inv = 1 / torch.sqrt(var.to(dtype) + eps)
    xh = (z.to(dtype) - _b(mean.to(dtype))) * _b(inv)
    s = sums.to(dtype)
    return _b(gamma.to(dtype) * inv) * (g - _b(s[0]) / count - xh * _b(s[1]) / count), gm
