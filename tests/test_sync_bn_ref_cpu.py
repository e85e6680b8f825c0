"""tests/sync_bn_ref.py (the four steps of synchronized BatchNorm) against float64 autograd of F.batch_norm over the concatenated
batch: two ranks with uneven shards, each rank's loss scaled by `world` as ctdet.dist.global_normalizer scales it, SUM-reduced
pairs, dz from the global sums and the global count.  Then the mean over the ranks of every downstream gradient, and of the local
dgamma / dbeta, is the full-batch gradient.

Bound: everything is float64; a sum over n <= 45000 terms carries at most n * 2^-53 ~ 5e-12 relative error, and the autograd
reference sums in another order, so the outputs are held to 1e-11 of their largest magnitude (conftest.rel_err)."""
import pytest
import torch
import torch.nn.functional as F

import sync_bn_ref as S
import train_cases as TC
from conftest import rel_err

F64 = torch.float64
TOL = 1e-11
SHAPES = [s for s in TC.BN_SHAPES if s[0] >= 2]
SPLIT = {2: 1, 4: 3, 3: 1, 32: 5, 8: 3}         # images of rank 0; the other rank holds the rest (uneven wherever B > 2)
MASKS = {'relu': dict(relu=1, lo=None, rs=None), 'linear-res': dict(relu=0, lo=None, rs=0.7), 'lo-mixed-res': dict(relu=0, lo='mixed', rs=0.7),
         'lo-ninf': dict(relu=1, lo='ninf', rs=1.0)}


def _case(shape, mask):
    B, C, HW = shape
    g = TC.gen('sync-%dx%dx%d-%s' % (shape + (mask,)))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    k = dict(MASKS[mask])
    k['z'] = rn(B, C, HW) * 2 + 0.5
    if B * HW < 8:
        # as train_cases.bn_case: over n = 2 samples dz cancels down to eps / var of its terms (1e-6 at var ~ 4), which would
        # leave six digits fewer than the bound assumes; a spread comparable to sqrt(eps) keeps dz of the order of its terms
        k['z'] = k['z'] * 0.004
    k['gamma'], k['beta'] = torch.rand(C, generator=g, dtype=F64) + 0.5, torch.rand(C, generator=g, dtype=F64) - 0.5
    k['lo_t'] = {None: None, 'ninf': torch.full((C,), TC.NINF, dtype=F64),
                 'mixed': torch.where(torch.arange(C) % 2 == 0, torch.tensor(0.0, dtype=F64), torch.tensor(TC.NINF, dtype=F64))}[k['lo']]
    k['res'] = rn(B, C, HW) if k['rs'] is not None else None
    k['rscale'] = k['rs'] if k['rs'] is not None else 1.0
    k['rm0'], k['rv0'] = rn(C) * 0.1, torch.rand(C, generator=g, dtype=F64) + 0.5
    k['w'] = rn(B, C, HW)                   # the loss: sum(y * w), so dy = w
    return k


def _autograd(k):
    z, gamma, beta = (k[n].clone().requires_grad_(True) for n in ('z', 'gamma', 'beta'))
    res = k['res'].clone().requires_grad_(True) if k['res'] is not None else None
    rm, rv = k['rm0'].clone(), k['rv0'].clone()
    v = F.batch_norm(z.unsqueeze(-1), rm, rv, gamma, beta, True, TC.MOMENTUM, TC.EPS).squeeze(-1)
    if res is not None:
        v = v * k['rscale'] + res
    if k['lo_t'] is not None:
        v = torch.maximum(v, k['lo_t'][None, :, None])
    elif k['relu']:
        v = torch.clamp_min(v, 0)
    (v * k['w']).sum().backward()
    return dict(y=v.detach(), dz=z.grad, dgamma=gamma.grad, dbeta=beta.grad, dres=None if res is None else res.grad, rmean=rm, rvar=rv)


@pytest.mark.parametrize('mask', list(MASKS))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_shard_sums_equal_full_batch_autograd(shape, mask):
    B, C, HW = shape
    k = _case(shape, mask)
    want = _autograd(k)
    a = SPLIT[B]
    shards, world = [(0, a), (a, B)], 2
    assert a != B - a or B == 2
    count = float(B * HW)
    cut = lambda t, r: None if t is None else t[shards[r][0]:shards[r][1]]
    # forward: local pairs, SUM, finish, apply
    fsum = sum(S.stats_local(cut(k['z'], r)) for r in range(world))
    mean, var, rm, rv = S.stats_finish(fsum, count, TC.MOMENTUM, k['rm0'], k['rv0'])
    y = [S.apply(cut(k['z'], r), mean, var, k['gamma'], k['beta'], TC.EPS, k['relu'], k['lo_t'], cut(k['res'], r), k['rscale'])
         for r in range(world)]
    assert rel_err(torch.cat(y), want['y']) < TOL
    assert rel_err(rm, want['rmean']) < TOL and rel_err(rv, want['rvar']) < TOL
    # backward: every rank's loss is scaled by `world` (its normaliser is N_global / world), the gradient all-reduce takes the mean
    dy = [cut(k['w'], r) * world for r in range(world)]
    loc = [S.backward_local(dy[r], y[r], cut(k['z'], r), mean, var, TC.EPS, k['relu'], k['lo_t'], k['rscale']) for r in range(world)]
    bsum = sum(l[0] for l in loc)
    out = [S.backward_apply(dy[r], y[r], cut(k['z'], r), mean, var, k['gamma'], TC.EPS, k['relu'], k['lo_t'], k['rscale'], bsum, count)
           for r in range(world)]
    assert rel_err(sum(l[1] for l in loc) / world, want['dgamma']) < TOL
    assert rel_err(sum(l[2] for l in loc) / world, want['dbeta']) < TOL
    # a downstream gradient is linear in dz: a rank holds world * (its rows of the full-batch dz), the mean over the ranks undoes it
    assert rel_err(torch.cat([o[0] for o in out]) / world, want['dz']) < TOL
    if want['dres'] is not None:
        assert rel_err(torch.cat([o[1] for o in out]) / world, want['dres']) < TOL
    # per-shard statistics are NOT the answer: with them the same steps miss the reference (the test can fail)
    m0, v0, _, _ = S.stats_finish(S.stats_local(cut(k['z'], 0)), float(a * HW))
    assert rel_err(m0, mean) > 1e3 * TOL


def test_the_steps_run_at_float32_too():
    k = _case((4, 10, 1200), 'relu')
    s32 = S.stats_local(k['z'], torch.float32)
    m32, v32, _, _ = S.stats_finish(s32, 4800.0, dtype=torch.float32)
    m64, v64, _, _ = S.stats_finish(S.stats_local(k['z']), 4800.0)
    assert s32.dtype == torch.float32 and m32.dtype == torch.float32
    # a float32 sum of n = 4800 terms is within n * 2^-24 = 2.9e-4 of the exact one in ANY order of summation; the variance as
    # E[x^2] - E[x]^2 loses nothing more to cancellation here (E[x^2] / var = 4.25 / 4)
    bound = 4800 * 2.0 ** -24
    assert rel_err(m32, m64) < bound and rel_err(v32, v64) < bound
