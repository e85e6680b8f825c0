"""The cases of tests/test_gpu_train_kernels.py, built without a device: inputs (seeded by the case name), the float64
reference of every output (train_ref.py) and e32 -- how far torch-CPU float32 arithmetic on the same inputs lands from
that float64 reference.  tests/golden/train_kernels_e32.npz records e32 of every reduced or rounded output:

    python tests/train_cases.py          # rewrites the table

The device test bounds an error by max(floor, 3 * e32) with e32 measured in the run AND by the same expression over the
recorded table, so a noisy float32 evaluation on another machine cannot loosen the bound.
tests/test_train_ref_cpu.py checks that the table names exactly the outputs of today's cases and that no recorded
e32 exceeds 1e-2 (above that float32 has no answer and the input would have to be replaced)."""
import os
import types
import zlib

import numpy as np
import torch

import train_ref as R

F32, F64 = torch.float32, torch.float64
E32_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_kernels_e32.npz')
NINF = float('-inf')


def rel_err(a, b):          # conftest.rel_err (a plain module cannot import conftest outside pytest)
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    d = np.abs(b).max()
    return float(np.abs(a - b).max() / (d if d > 0 else 1.0))


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------------------ BatchNorm
# (B, C, HW).  The host splits a channel's B*HW elements in min(ceil(1024 / C), B*HW / 2048) ranges: one below 4096
# elements, exactly two at (1,7,4097) and at (4,10,1200) (2400 = two whole images each), several that end inside an image at
# (32,8,361) (11552 / 5 -> 2311) and (8,64,5625) (45000 / 16 -> 2813); more than 1024 channels; a one-pixel map.
BN_SHAPES = [(2, 3, 1), (2, 5, 9), (1, 7, 4097), (4, 10, 1200), (3, 1030, 40), (32, 8, 361), (8, 64, 5625)]
# relu, lo (None / 'zero' / 'ninf' / 'mixed'), residual (None / 1.0 / 0.7), dres (None / 'dense' / 'slice'), accumulate,
# scratch given, frozen, running statistics given, data.  Every value of every axis occurs; relu disagrees with the lo rule
# in l0 (relu 0, lo 0: masked), l1 (relu 1, lo -inf: not masked) and both mixed rows.  The one combination
# test_gpu_train.py::test_batchnorm_train_forward_backward holds (ReLU, 0.7, dense dres, set) is not repeated.
BN_COMBOS = {
    'plain':  dict(relu=1, lo=None,    rs=None, dres=None,    acc=0, scratch=1, frozen=0, running=1, data='randn'),
    'lin':    dict(relu=0, lo=None,    rs=1.0,  dres='dense', acc=1, scratch=1, frozen=0, running=0, data='bigmean'),
    'l0':     dict(relu=0, lo='zero',  rs=0.7,  dres='slice', acc=0, scratch=1, frozen=1, running=1, data='randn'),
    'l1':     dict(relu=1, lo='ninf',  rs=1.0,  dres='slice', acc=1, scratch=0, frozen=0, running=1, data='const'),
    'mix0':   dict(relu=0, lo='mixed', rs=0.7,  dres='dense', acc=0, scratch=1, frozen=0, running=1, data='zeros'),
    'mix1':   dict(relu=1, lo='mixed', rs=None, dres=None,    acc=0, scratch=0, frozen=1, running=0, data='randn'),
    'racc':   dict(relu=1, lo=None,    rs=0.7,  dres='slice', acc=1, scratch=1, frozen=0, running=1, data='zeros'),
    'frz':    dict(relu=0, lo=None,    rs=None, dres=None,    acc=0, scratch=1, frozen=1, running=1, data='bigmean'),
}
EPS, MOMENTUM = 1e-5, 0.01
ZP, ZO = 3, 2           # every sliced operand: (extra channels, offset)
YP, YO = 2, 1
RP, RO = 4, 3
GP, GO = 4, 1
DP, DO = 5, 4


def bn_id(shape, combo):
    return '%dx%dx%d-%s' % (shape + (combo,))


def bn_case(shape, combo):
    """Inputs of one BatchNorm case, as float32 CPU tensors.  mean / var for apply and backward are the float32 rounding
    of the float64 batch statistics (frozen: running statistics unrelated to the batch), NOT the output of the statistics
    kernel: each entry point is judged on its own inputs."""
    B, C, HW = shape
    k = types.SimpleNamespace(**BN_COMBOS[combo])
    k.B, k.C, k.HW, k.name = B, C, HW, bn_id(shape, combo)
    g = gen(k.name)
    rn = lambda *s: torch.randn(*s, generator=g)
    z = rn(B, C + ZP, HW) * 2 + 0.5
    if B * HW < 8:
        # Batch statistics over n = 2 samples cancel dz down to the order of eps / var of what goes in: with var ~ 4 that is
        # 1e-6 of the terms, where float32 has no digit left (e32 ~ 1).  A spread comparable to sqrt(eps) keeps dz of the
        # order of its terms, so that the comparison says something about the kernel.
        z = z * 0.004
    if k.data == 'bigmean':                 # mean / std ~ 1e3: the variance as E[x^2] - E[x]^2 needs the f64 accumulators
        z[:, ZO] = 1000 + rn(B, HW)
    if k.data == 'const':                   # var == 0: the result is governed by eps
        z[:, ZO] = 3.25
    k.z = z
    k.gamma, k.beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    k.lo_t = {None: None, 'zero': torch.zeros(C), 'ninf': torch.full((C,), NINF),
              'mixed': torch.where(torch.arange(C) % 2 == 0, torch.tensor(0.0), torch.tensor(NINF))}[k.lo]
    k.res = rn(B, C + RP, HW) if k.rs is not None else None
    k.rscale = k.rs if k.rs is not None else 1.0
    k.rm0, k.rv0 = rn(C) * 0.1, torch.rand(C, generator=g) + 0.5
    k.y0 = torch.full((B, C + YP, HW), 9.0)
    k.dy = rn(B, C + GP, HW)
    k.dz0 = torch.full((B, C + ZP, HW), 7.0)
    k.dres_ctot, k.dres_off = {None: (0, 0), 'dense': (C, 0), 'slice': (C + DP, DO)}[k.dres]
    k.dres0 = None
    if k.dres:
        k.dres0 = rn(B, k.dres_ctot, HW) if k.acc else torch.full((B, k.dres_ctot, HW), 5.0)
    m, v, _, _ = R.bn_stats(z, ZO, C)
    if k.frozen:
        k.mean, k.var = (m + rn(C).double() * 0.3).float(), (v * (torch.rand(C, generator=g).double() + 0.5) + 0.01).float()
    else:
        k.mean, k.var = m.float(), v.float()
    # the forward output the backward masks with: float32 of the reference (clamped activations are exactly 0)
    y = R.bn_apply(z, ZO, k.mean, k.var, k.gamma, k.beta, EPS, k.relu, k.lo_t, k.res, RO, k.rscale, k.y0, YO).float()
    if k.data == 'zeros':                   # +0.0 and -0.0 where the activation was positive: the mask is y <= 0
        ys, idx = y[:, YO:YO + C], torch.arange(B * C * HW).view(B, C, HW)
        ys[idx % 5 == 0] = 0.0
        ys[idx % 7 == 2] = -0.0
    k.y_in = y if (k.relu or k.lo) else None
    return k


def _both(fn):
    return fn(F64), fn(F32)


def bn_expected(k):
    """name -> (float64 reference, float32 evaluation) of every output of the three entry points (y, dz, dres: the slice)."""
    C = k.C
    out = {}
    run = (k.rm0, k.rv0) if k.running else (None, None)
    for (m, v, rm, rv), tag in zip(_both(lambda d: R.bn_stats(k.z, ZO, C, MOMENTUM, run[0], run[1], d)), (0, 1)):
        for n, t in (('mean', m), ('var', v), ('rmean', rm), ('rvar', rv)):
            if t is not None:
                out.setdefault(n, [None, None])[tag] = t
    for y, tag in zip(_both(lambda d: R.bn_apply(k.z, ZO, k.mean, k.var, k.gamma, k.beta, EPS, k.relu, k.lo_t, k.res, RO,
                                                 k.rscale, k.y0, YO, d)), (0, 1)):
        out.setdefault('y', [None, None])[tag] = y[:, YO:YO + C]
    for (dz, dg, db, dres), tag in zip(_both(lambda d: R.bn_backward(
            k.frozen, k.dy, GO, k.y_in, YO, k.z, ZO, k.mean, k.var, k.gamma, EPS, k.relu, k.lo_t, k.rscale, k.dres0,
            k.dres_off, k.acc, k.dz0, d)), (0, 1)):
        dz = dz[:, ZO:ZO + C]
        dres = None if dres is None else dres[:, k.dres_off:k.dres_off + C]
        for n, t in (('dz', dz), ('dgamma', dg), ('dbeta', db), ('dres', dres)):
            if t is not None:
                out.setdefault(n, [None, None])[tag] = t
    return {n: tuple(v) for n, v in out.items()}


BN_FLOORS = dict(mean=1e-5, var=1e-5, rmean=1e-5, rvar=1e-5, y=1e-5, dres=1e-5, dz=1e-4, dgamma=1e-4, dbeta=1e-4)

# ------------------------------------------------------------------------------------------------ bias + activation
# (B, C, HW, relu, dbias given, y given).  HW % 4 in {0,1,2,3}; B*HW below / at / above 4096 (the host splits a channel in
# ceil(B*HW / 4096) ranges, rounded up to 4 elements, that cross images); C in {1, 3, 126, 2049}.
BIAS_CASES = [
    (2, 3, 25, 1, 1, 1), (2, 126, 2048, 1, 1, 1), (3, 3, 1366, 1, 1, 1), (5, 1, 1444, 1, 1, 1), (2, 2049, 7, 0, 1, 0),
    (4, 3, 1027, 0, 1, 1), (1, 126, 4096, 1, 0, 1), (8, 3, 5625, 1, 1, 1), (2, 1, 4100, 1, 1, 1), (3, 3, 1368, 0, 0, 0),
    (1, 3, 4096, 1, 1, 1), (1, 3, 4097, 1, 1, 1),
]


def bias_id(c):
    return '%dx%dx%d-r%d-b%d-y%d' % c


def bias_case(c):
    B, C, HW, relu, has_db, has_y = c
    k = types.SimpleNamespace(B=B, C=C, HW=HW, relu=relu, has_db=has_db, name=bias_id(c))
    g = gen(k.name)
    k.dy = torch.randn(B, C + 2, HW, generator=g) * 3
    y = torch.relu(torch.randn(B, C + 3, HW, generator=g))
    y.view(-1)[3::11] = -0.0
    k.y = y if has_y else None
    k.dz0 = torch.full((B, C + 4, HW), 7.0)
    return k


def bias_expected(k):
    return _both(lambda d: R.bias_act_backward(k.dy, 1, k.y, 2, k.relu, k.C, k.dz0, 3, d))


# ------------------------------------------------------------------------------------------------ pool backward
# (planes, H, W, k, stride, pad, ceil, data).  The first nine geometries are those of test_gpu_train.py::
# test_pool_and_bias_backward; k=2/s=2/p=0 takes the 2x2 kernel, planes of at most 4096 elements the LDS kernel, larger ones
# the gather kernel.  64x64 = 4096 and 17x241 = 4097 sit on that boundary.
_POOL_GEOMS = [(30, 30, 2, 2, 0, False), (15, 15, 2, 2, 0, True), (15, 13, 2, 2, 0, False), (75, 75, 2, 2, 0, True),
               (9, 9, 3, 1, 1, False), (19, 19, 3, 1, 1, False), (32, 32, 3, 1, 1, False), (19, 19, 3, 3, 0, True),
               (70, 66, 3, 1, 1, False)]
_POOL_3K = [(30, 30, 2, 2, 0, False), (19, 19, 3, 1, 1, False), (70, 66, 3, 1, 1, False)]        # one per kernel
POOL_CASES = ([(6,) + g + ('randn',) for g in _POOL_GEOMS]
              + [(p,) + g + ('randn',) for g in _POOL_3K for p in (1, 257)]
              + [(6, 64, 64, 3, 1, 1, False, 'randn'), (6, 17, 241, 3, 1, 1, False, 'randn'),
                 (6, 64, 64, 2, 2, 0, False, 'randn'), (6, 17, 241, 2, 2, 0, True, 'randn'),
                 (6, 33, 31, 3, 2, 1, False, 'randn'), (6, 64, 64, 3, 2, 1, False, 'randn'), (6, 70, 66, 3, 2, 1, False, 'randn')]
              + [(6,) + g + (d,) for g in _POOL_3K for d in ('negative', 'equal', 'zeros')])


def pool_id(c):
    return 'p%d-%dx%d-k%ds%dp%d-%s-%s' % (c[:6] + ('ceil' if c[6] else 'floor', c[7]))


def pool_out(n, k, s, p, ceil):
    o = -((n + 2 * p - k) // -s) + 1 if ceil else (n + 2 * p - k) // s + 1
    if ceil and (o - 1) * s >= n + p:       # torch: the last window must start inside the input or its left padding
        o -= 1
    return o


def pool_data(g, kind, shape):
    x = torch.randn(*shape, generator=g)
    if kind == 'randn':
        x.view(-1, shape[-2], shape[-1])[0, :4, :4] = 1.5           # ties inside windows
    elif kind == 'negative':
        x = -x.abs() - 1
    elif kind == 'equal':
        x = torch.full(shape, 2.0)
    elif kind == 'zeros':
        x = torch.where(x > 0, torch.tensor(0.0), torch.tensor(-0.0))
    return x


def pool_case(c):
    P, H, W, kk, s, p, ceil, data = c
    k = types.SimpleNamespace(P=P, H=H, W=W, k=kk, s=s, p=p, OH=pool_out(H, kk, s, p, ceil), OW=pool_out(W, kk, s, p, ceil),
                              name=pool_id(c), overlap=s < kk)
    g = gen(k.name)
    k.x = pool_data(g, data, (P, H, W))
    k.dy = torch.randn(P, k.OH, k.OW, generator=g)
    k.dx0 = torch.randn(P, H, W, generator=g)
    return k


def pool_expected(k, accumulate):
    return _both(lambda d: R.maxpool_bwd(k.x, k.dy, k.k, k.s, k.p, k.dx0, accumulate, d))


# fused 2x2 pool + bias + ReLU backward: (B, C, H, W, ceil)
FUSED_CASES = [(3, 5, 64, 64, False), (3, 5, 17, 241, False), (3, 5, 17, 241, True), (3, 5, 15, 13, False), (3, 5, 15, 13, True),
               (1, 1, 30, 30, False), (1, 257, 9, 9, True)]


def fused_id(c):
    return '%dx%dx%dx%d-%s' % (c[:4] + ('ceil' if c[4] else 'floor',))


def fused_case(c):
    B, C, H, W, ceil = c
    k = types.SimpleNamespace(B=B, C=C, H=H, W=W, OH=pool_out(H, 2, 2, 0, ceil), OW=pool_out(W, 2, 2, 0, ceil), name=fused_id(c))
    g = gen(k.name)
    y = torch.relu(torch.randn(B, C + 3, H, W, generator=g))
    y[0, 2, :4, :4] = 1.5                       # ties
    y[B - 1, 2, :6, :6] = 0.0                   # dead windows
    y[0, 2, 6:8, :] = -0.0
    k.y = y
    k.dy = torch.randn(B, C, k.OH, k.OW, generator=g) * 3
    k.dz0 = torch.full((B, C + 2, H, W), 7.0)
    return k


def fused_expected(k):
    return _both(lambda d: R.maxpool2x2_bias_relu_bwd(k.y, 2, k.C, k.dy, k.dz0, 1, d))


# ------------------------------------------------------------------------------------------------ head gather
GATHER_C = 12


def gather_layout(nseg, HW):
    """(co_begin, co_end, pix_stride, img_stride, base) of the first nseg segments over GATHER_C channels: a pixel stride equal
    to and larger than the segment's width, a gap (channels 4, 5), an uncovered tail (11; from 4 resp. 9 on with fewer
    segments), nonzero bases and image strides larger than the payload."""
    segs = [(0, 4, 4, 3), (6, 9, 5, 5), (9, 11, 2, 1)][:nseg]
    return [(c0, c1, ps, base + HW * ps + 6, base) for c0, c1, ps, base in segs]


# ------------------------------------------------------------------------------------------------ e32 table
def e32_entries():
    """name -> e32 of every reduced or rounded output of every case."""
    out = {}
    for sh in BN_SHAPES:
        for cb in BN_COMBOS:
            k = bn_case(sh, cb)
            for n, (r64, r32) in bn_expected(k).items():
                out['bn/%s/%s' % (k.name, n)] = rel_err(r32, r64)
    for c in BIAS_CASES:
        k = bias_case(c)
        (_, db64, _), (_, db32, _) = bias_expected(k)
        out['bias/%s/dbias' % k.name] = rel_err(db32, db64)
    for c in POOL_CASES:
        k = pool_case(c)
        if k.overlap:
            for acc in (0, 1):
                r64, r32 = pool_expected(k, acc)
                out['pool/%s/dx%d' % (k.name, acc)] = rel_err(r32, r64)
    for c in FUSED_CASES:
        k = fused_case(c)
        (_, db64, _), (_, db32, _) = fused_expected(k)
        out['fused/%s/dbias' % k.name] = rel_err(db32, db64)
    return out


_table = None


def recorded_e32(name):
    global _table
    if _table is None:
        t = np.load(E32_TABLE, allow_pickle=False)
        _table = dict(zip(t['names'].tolist(), t['e32'].tolist()))
    return _table[name]


if __name__ == '__main__':
    torch.set_num_threads(8)
    e = e32_entries()
    names = sorted(e)
    np.savez(E32_TABLE, names=np.array(names), e32=np.array([e[n] for n in names], dtype=np.float64))
    worst = sorted(e.items(), key=lambda kv: -kv[1])[:12]
    print('%d entries; largest:' % len(e))
    for n, v in worst:
        print('  %-48s %.3e' % (n, v))
