"""tests/train_ref.py (the float64 reference the device sweep of the training kernels is held to) against torch
float64 autograd over F.batch_norm / F.relu / F.max_pool2d and the channels-last permute / reshape scatter of the heads,
with every flag combination tests/test_gpu_train_kernels.py uses.  No device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_cases as TC
import train_ref as R
from conftest import rel_err

F64 = torch.float64
# Both sides evaluate the same real formula in float64; they differ in the order of the sums and in a few elementwise
# roundings.  A float64 sum of n terms is off by at most n * eps64 * sum|t_i|; the terms here are O(1) (unit-variance
# activations and gradients, gamma in [0.5, 1.5]) and rel_err divides by the largest reference value, which is O(1) or
# larger, so one reduction costs at most ~n * eps64.  dz passes two chained reductions (the statistics, then dbeta /
# dgamma) and is scaled by gamma / sqrt(var + eps) <= ~2 on these inputs: 2 * 2 * n * eps64, and a factor 4 for the
# elementwise operations around them gives 16 * n * eps64.  (Observed errors are near sqrt(n) * eps64.)
EPS64 = 2.0 ** -52


def tol(n):
    return 16 * n * EPS64


BN_CPU_SHAPES = [(2, 5, 9), (3, 4, 50), (1, 7, 300), (4, 1030, 3)]


@pytest.mark.parametrize('combo', list(TC.BN_COMBOS))
@pytest.mark.parametrize('shape', BN_CPU_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_batchnorm_reference_vs_autograd(shape, combo):
    B, C, HW = shape
    k = TC.BN_COMBOS[combo]
    g = TC.gen('cpu' + TC.bn_id(shape, combo))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    n = B * HW
    z = rn(B, C + 3, HW) * 2 + 0.5
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).requires_grad_(True)
    beta = (torch.rand(C, generator=g, dtype=F64) - 0.5).requires_grad_(True)
    lo = {None: None, 'zero': torch.zeros(C, dtype=F64), 'ninf': torch.full((C,), TC.NINF, dtype=F64),
          'mixed': torch.where(torch.arange(C) % 2 == 0, 0.0, TC.NINF).to(F64)}[k['lo']]
    res = rn(B, C + 4, HW) if k['rs'] is not None else None
    rscale = k['rs'] if k['rs'] is not None else 1.0
    rm0, rv0 = rn(C) * 0.1, torch.rand(C, generator=g, dtype=F64) + 0.5
    zs = z[:, 2:2 + C].clone().requires_grad_(True)
    # statistics
    mean, var, rm, rv = R.bn_stats(z, 2, C, 0.01, rm0, rv0)
    assert rel_err(mean, zs.detach().mean((0, 2))) < tol(n) and rel_err(var, zs.detach().var((0, 2), unbiased=False)) < tol(n)
    trm, trv = rm0.clone(), rv0.clone()
    F.batch_norm(zs.detach(), trm, trv, None, None, True, 0.01, 1e-5)
    assert rel_err(rm, trm) < tol(n) and rel_err(rv, trv) < tol(n)
    assert R.bn_stats(z, 2, C)[2] is None
    if k['frozen']:
        mean, var = rn(C) * 0.3, torch.rand(C, generator=g, dtype=F64) + 0.5
    # forward
    rs = res[:, 3:3 + C].clone().requires_grad_(True) if res is not None else None
    v = F.batch_norm(zs, mean.clone() if k['frozen'] else None, var.clone() if k['frozen'] else None, gamma, beta,
                     not k['frozen'], 0.0, 1e-5)
    if rs is not None:
        v = v * rscale + rs
    if lo is not None:
        want_y = torch.maximum(v, lo[None, :, None])
    else:
        want_y = F.relu(v) if k['relu'] else v
    y0 = torch.full((B, C + 2, HW), 9.0, dtype=F64)
    y = R.bn_apply(z, 2, mean, var, gamma.detach(), beta.detach(), 1e-5, k['relu'], lo, res, 3, rscale, y0, 1)
    assert rel_err(y[:, 1:1 + C], want_y.detach()) < tol(n)
    assert bool((y[:, :1] == 9).all()) and bool((y[:, 1 + C:] == 9).all())
    # the mask, from autograd's own forward: equal, not close
    act = (lo == 0) if lo is not None else torch.full((C,), bool(k['relu']))
    yy = y0.clone()
    yy[:, 1:1 + C] = want_y.detach()
    assert torch.equal(R.bn_mask(yy, 1, C, k['relu'], lo).expand(B, C, HW), (want_y.detach() <= 0) & act[None, :, None])
    # backward
    dy = rn(B, C + 4, HW)
    (want_y * dy[:, 1:1 + C]).sum().backward()
    dres_ctot, dres_off = {None: (0, 0), 'dense': (C, 0), 'slice': (C + 5, 4)}[k['dres']]
    dres0 = rn(B, dres_ctot, HW) if k['dres'] else None
    dz0 = torch.full((B, C + 3, HW), 7.0, dtype=F64)
    dz, dg, db, dres = R.bn_backward(k['frozen'], dy, 1, yy if (k['relu'] or lo is not None) else None, 1, z, 2, mean, var,
                                     gamma.detach(), 1e-5, k['relu'], lo, rscale, dres0, dres_off, k['acc'], dz0)
    assert rel_err(dz[:, 2:2 + C], zs.grad) < tol(n)
    assert rel_err(dg, gamma.grad) < tol(n) and rel_err(db, beta.grad) < tol(n)
    assert bool((dz[:, :2] == 7).all()) and bool((dz[:, 2 + C:] == 7).all())
    if k['dres']:
        want = dres0.clone()
        want[:, dres_off:dres_off + C] = (dres0[:, dres_off:dres_off + C] if k['acc'] else 0) + rs.grad
        assert torch.equal(dres, want)          # a copy of dy or 0, plus at most one addition: no rounding to differ in
    else:
        assert dres is None


def test_running_statistics_of_a_single_sample():
    """n == 1: torch refuses to train on one value per channel; ct_bn_train_stats scales the (zero) variance by 1."""
    z = torch.tensor([[[3.0], [-2.0]]])
    mean, var, rm, rv = R.bn_stats(z, 0, 2, 0.25, torch.tensor([1.0, 1.0]), torch.tensor([2.0, 4.0]))
    assert torch.equal(mean, torch.tensor([3.0, -2.0], dtype=F64)) and torch.equal(var, torch.zeros(2, dtype=F64))
    assert torch.equal(rm, torch.tensor([1.5, 0.25], dtype=F64)) and torch.equal(rv, torch.tensor([1.5, 3.0], dtype=F64))


@pytest.mark.parametrize('relu,has_y', [(1, 1), (0, 1), (0, 0)])
@pytest.mark.parametrize('shape', [(2, 3, 25), (3, 1, 64), (1, 5, 7)], ids=lambda s: 'x'.join(map(str, s)))
def test_bias_act_reference_vs_autograd(shape, relu, has_y):
    B, C, HW = shape
    g = TC.gen('cpu-bias%s%d%d' % (shape, relu, has_y))
    zin = torch.randn(B, C, HW, generator=g, dtype=F64).requires_grad_(True)
    bias = torch.randn(C, generator=g, dtype=F64).requires_grad_(True)
    v = zin + bias[None, :, None]
    y = F.relu(v) if relu else v
    dy = torch.randn(B, C + 2, HW, generator=g, dtype=F64)
    (y * dy[:, 1:1 + C]).sum().backward()
    yfull = torch.zeros(B, C + 3, HW, dtype=F64)
    yfull[:, 2:2 + C] = y.detach()
    dz0 = torch.full((B, C + 4, HW), 7.0, dtype=F64)
    dz, db, amax = R.bias_act_backward(dy, 1, yfull if has_y else None, 2, relu, C, dz0, 3)
    assert torch.equal(dz[:, 3:3 + C], zin.grad)
    assert bool((dz[:, :3] == 7).all()) and bool((dz[:, 3 + C:] == 7).all())
    assert rel_err(db, bias.grad) < tol(B * HW)
    assert torch.equal(amax, zin.grad.abs().amax((1, 2)))
    # the in-place form of the heads: dy and dz the same buffer, two adjacent parts
    buf = torch.randn(B, 2 * C, HW, generator=g, dtype=F64)
    got, _, _ = R.bias_act_backward(buf, 0, None, 0, 0, C, buf, 0)
    assert torch.equal(got, buf)


CPU_POOL = [c for c in TC.POOL_CASES if c[0] == 6] + [(1, 30, 30, 2, 2, 0, False, 'randn'), (257, 9, 9, 3, 1, 1, False, 'randn')]


@pytest.mark.parametrize('c', CPU_POOL, ids=TC.pool_id)
def test_maxpool_reference_vs_autograd(c):
    k = TC.pool_case(c)
    x = k.x.double().requires_grad_(True)
    y = F.max_pool2d(x[None], k.k, k.s, k.p, ceil_mode=c[6])[0]
    assert tuple(y.shape[1:]) == (k.OH, k.OW)
    y.backward(k.dy.double())
    got = R.maxpool_bwd(k.x, k.dy, k.k, k.s, k.p, k.dx0, 0)
    acc = R.maxpool_bwd(k.x, k.dy, k.k, k.s, k.p, k.dx0, 1)
    if not k.overlap:
        assert torch.equal(got, x.grad)             # one contribution per element: which element is the whole question
        assert torch.equal(acc, k.dx0.double() + x.grad)
    else:
        assert rel_err(got, x.grad) < tol(k.k * k.k) and rel_err(acc, k.dx0.double() + x.grad) < tol(k.k * k.k)
        assert torch.equal(got != 0, x.grad != 0)


@pytest.mark.parametrize('c', TC.FUSED_CASES, ids=TC.fused_id)
def test_fused_pool_bias_relu_reference_vs_autograd(c):
    k = TC.fused_case(c)
    zin = k.y[:, 2:2 + k.C].double().requires_grad_(True)
    bias = torch.zeros(k.C, dtype=F64, requires_grad=True)
    p = F.max_pool2d(F.relu(zin + bias[None, :, None, None]), 2, 2, ceil_mode=c[4])
    assert tuple(p.shape[2:]) == (k.OH, k.OW)
    p.backward(k.dy.double())
    dz, db, amax = R.maxpool2x2_bias_relu_bwd(k.y, 2, k.C, k.dy, k.dz0, 1)
    assert torch.equal(dz[:, 1:1 + k.C], zin.grad)
    assert bool((dz[:, :1] == 7).all()) and bool((dz[:, 1 + k.C:] == 7).all())
    assert rel_err(db, bias.grad) < tol(k.B * k.H * k.W)
    assert torch.equal(amax, zin.grad.abs().amax((1, 2, 3)))


@pytest.mark.parametrize('HW', [1, 9, 1444])
@pytest.mark.parametrize('nseg', [1, 2, 3])
def test_head_gather_reference_vs_autograd(nseg, HW):
    B, C = 2, 12
    layout = TC.gather_layout(nseg, HW)
    g = TC.gen('cpu-gather%d-%d' % (nseg, HW))
    z = torch.randn(B, C, HW, generator=g, dtype=F64, requires_grad=True)
    loss = 0
    segs = []
    for (c0, c1, ps, istr, base) in layout:
        # the forward scatter of models/RFB_Net_vgg.py: permute to channels-last, flatten, cat into the image's row
        rows = torch.zeros(B, HW, ps, dtype=F64)
        rows = torch.cat([z[:, c0:c1].permute(0, 2, 1), rows[:, :, c1 - c0:]], 2).reshape(B, HW * ps)
        flat = torch.cat([torch.zeros(B, base, dtype=F64), rows, torch.zeros(B, istr - base - HW * ps, dtype=F64)], 1)
        dflat = torch.randn(B, istr, generator=g, dtype=F64)
        loss = loss + (flat * dflat).sum()
        segs.append((dflat, c0, c1, ps, istr, base))
    loss.backward()
    assert torch.equal(R.head_grad_gather(segs, B, C, HW), z.grad)
    covered = torch.zeros(C, dtype=torch.bool)
    for (c0, c1, *_r) in layout:
        covered[c0:c1] = True
    assert bool((z.grad[:, ~covered] == 0).all()) and int((~covered).sum()) >= 3


def test_recorded_e32_table_matches_the_cases():
    """tests/golden/train_kernels_e32.npz names exactly the reduced outputs of today's cases (the table is stale
    otherwise: python tests/train_cases.py) and float32 has an answer for every one of them (e32 <= 1e-2)."""
    t = np.load(TC.E32_TABLE, allow_pickle=False)
    names = set()
    for sh in TC.BN_SHAPES:
        for cb, k in TC.BN_COMBOS.items():
            outs = ['mean', 'var', 'y', 'dz', 'dgamma', 'dbeta'] + (['rmean', 'rvar'] if k['running'] else []) + \
                   (['dres'] if k['dres'] else [])
            names |= {'bn/%s/%s' % (TC.bn_id(sh, cb), o) for o in outs}
    names |= {'bias/%s/dbias' % TC.bias_id(c) for c in TC.BIAS_CASES}
    names |= {'pool/%s/dx%d' % (TC.pool_id(c), a) for c in TC.POOL_CASES if c[4] < c[3] for a in (0, 1)}
    names |= {'fused/%s/dbias' % TC.fused_id(c) for c in TC.FUSED_CASES}
    assert set(t['names'].tolist()) == names
    assert float(t['e32'].max()) <= 1e-2 and float(t['e32'].min()) >= 0


def test_recorded_e32_is_reproduced_for_a_sample():
    """A few rows recomputed here: within a factor 3 of the record or below float32's own resolution (the torch-CPU sums
    split by thread count, so equality is not expected)."""
    for sh, cb in (((2, 5, 9), 'lin'), ((2, 3, 1), 'plain'), ((4, 10, 1200), 'l1')):
        k = TC.bn_case(sh, cb)
        for n, (r64, r32) in TC.bn_expected(k).items():
            e = TC.rel_err(r32, r64)
            assert e <= max(3 * TC.recorded_e32('bn/%s/%s' % (k.name, n)), 2.0 ** -21), (k.name, n, e)
