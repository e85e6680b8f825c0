"""Synchronized BatchNorm on the device: the four ct_bn_sync_* entries (csrc/ct_train.hip) and the two-rank training step.

  1. emulated ranks in one process: the local entries per shard, the two `sums` arrays added with torch (what the SUM
     all-reduce does), finish / apply with the global count -- every output against the float64 reference of the FULL batch
     (train_cases.bn_expected) under the rule of test_gpu_train_kernels._bound, with the floors and recorded e32 of the same cases;
  2. a world of one: torch.equal with ct_bn_train_stats_det / ct_bn_train_backward_det on all seven shapes;
  3. sensitivity: a shard whose z is shifted -- a shard's own statistics miss the full-batch reference by far more than the
     floor, the synchronized ones do not;
  4. two ranks (distinct devices over RCCL where the box has two, else one device over gloo): RFBNet-300 with BatchNorm in train
     mode, gradient and BatchNorm syncs on, against float64 autograd over the full batch.
"""
import os

import pytest
import torch
import torch.multiprocessing as mp

import sync_bn_ref as S
import train_cases as TC
import train_ref as R
from conftest import rel_err
from ctdet import _lib, synth
from test_gpu_train_kernels import _bound, _d, _outside, _p, _s

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64

SYNC_SHAPES = [(2, 3, 1), (2, 5, 9), (4, 10, 1200), (3, 1030, 40), (32, 8, 361), (8, 64, 5625)]
SPLITS = {(2, 3, 1): (1, 1), (2, 5, 9): (1, 1), (4, 10, 1200): (3, 1), (3, 1030, 40): (1, 2), (32, 8, 361): (5, 27),
          (8, 64, 5625): (4, 4)}
UNFROZEN = ['plain', 'lin', 'l1', 'mix0']       # of train_cases.BN_COMBOS; a frozen layer has no statistics to synchronize


def _scratch(B, Cn, HW):
    """The scratch of one local entry, filled with a value no sum may pick up."""
    n = _lib.lib().ct_bn_det_scratch_bytes(B, Cn, HW, None)
    return torch.full((max(int(n) // 8, 1),), 123.0, dtype=F64, device=DEV), int(n)


def _stats_local(z, B, Cn, HW, sums):
    sc, nb = _scratch(B, Cn, HW)
    _lib.check(_lib.lib().ct_bn_sync_stats_local(z.data_ptr(), B, Cn + TC.ZP, TC.ZO, Cn, HW, sums.data_ptr(), sc.data_ptr(), nb,
                                                 _s()), 'sync stats local')


def _sync_launch(k, shards):
    """The synchronized passes of case k over the batch ranges `shards`; every device buffer they write, by name (dz / dres /
    y: the shards' buffers concatenated along the batch)."""
    lib = _lib.lib()
    Cn, HW = k.C, k.HW
    count = float(k.B * HW)
    o = {}
    gamma, beta, lo = _d(k.gamma), _d(k.beta), _d(k.lo_t)
    meanin, varin = _d(k.mean), _d(k.var)
    parts = []
    for b0, b1 in shards:
        p = dict(B=b1 - b0, z=_d(k.z[b0:b1]), dy=_d(k.dy[b0:b1]), yin=_d(None if k.y_in is None else k.y_in[b0:b1]),
                 res=_d(None if k.res is None else k.res[b0:b1]), y=_d(k.y0[b0:b1].clone()), dz=_d(k.dz0[b0:b1].clone()),
                 dres=_d(None if k.dres0 is None else k.dres0[b0:b1].clone()))
        parts.append(p)
    # forward: local sums per shard, their sum, finish
    fsum = torch.zeros(2 * Cn, dtype=F64, device=DEV)
    for p in parts:
        p['fs'] = torch.full((2 * Cn,), 7.0, dtype=F64, device=DEV)
        _stats_local(p['z'], p['B'], Cn, HW, p['fs'])
        fsum += p['fs']
    o['mean'], o['var'] = torch.full((Cn,), 3.0, device=DEV), torch.full((Cn,), 3.0, device=DEV)
    o['rmean'], o['rvar'] = (_d(k.rm0.clone()), _d(k.rv0.clone())) if k.running else (None, None)
    _lib.check(lib.ct_bn_sync_stats_finish(fsum.data_ptr(), count, Cn, o['mean'].data_ptr(), o['var'].data_ptr(), TC.MOMENTUM,
                                           _p(o['rmean']), _p(o['rvar']), _s()), 'sync stats finish')
    # apply and backward on the case's own mean / var (train_cases.bn_case: each entry is judged on its own inputs)
    bsum = torch.zeros(2 * Cn, dtype=F64, device=DEV)
    for p in parts:
        _lib.check(lib.ct_bn_train_apply(p['z'].data_ptr(), meanin.data_ptr(), varin.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                         TC.EPS, k.relu, _p(lo), _p(p['res']), Cn + TC.RP, TC.RO, k.rscale, p['y'].data_ptr(),
                                         Cn + TC.YP, TC.YO, Cn + TC.ZP, TC.ZO, p['B'], Cn, HW, _s()), 'apply')
        p['bs'] = torch.full((2 * Cn,), 7.0, dtype=F64, device=DEV)
        p['dgamma'], p['dbeta'] = torch.full((Cn,), 3.0, device=DEV), torch.full((Cn,), 3.0, device=DEV)
        sc, nb = _scratch(p['B'], Cn, HW)
        _lib.check(lib.ct_bn_sync_backward_local(
            p['dy'].data_ptr(), Cn + TC.GP, TC.GO, _p(p['yin']), Cn + TC.YP, TC.YO, p['z'].data_ptr(), meanin.data_ptr(),
            varin.data_ptr(), TC.EPS, k.relu, _p(lo), k.rscale, Cn + TC.ZP, TC.ZO, p['B'], Cn, HW, p['bs'].data_ptr(),
            p['dgamma'].data_ptr(), p['dbeta'].data_ptr(), sc.data_ptr(), nb, _s()), 'sync backward local')
        bsum += p['bs']
    for p in parts:
        _lib.check(lib.ct_bn_sync_backward_apply(
            p['dy'].data_ptr(), Cn + TC.GP, TC.GO, _p(p['yin']), Cn + TC.YP, TC.YO, p['z'].data_ptr(), meanin.data_ptr(),
            varin.data_ptr(), gamma.data_ptr(), TC.EPS, k.relu, _p(lo), k.rscale, _p(p['dres']), k.dres_ctot, k.dres_off, k.acc,
            p['dz'].data_ptr(), Cn + TC.ZP, TC.ZO, p['B'], Cn, HW, bsum.data_ptr(), count, _s()), 'sync backward apply')
    torch.cuda.synchronize()
    o['y'] = torch.cat([p['y'] for p in parts])
    o['dz'] = torch.cat([p['dz'] for p in parts])
    o['dres'] = torch.cat([p['dres'] for p in parts]) if k.dres0 is not None else None
    # the parameter gradients: per-shard sums (what the gradient all-reduce adds), and the local floats of every shard
    o['dbeta'], o['dgamma'] = bsum[:Cn].float(), bsum[Cn:].float()
    o['local'] = [(p['dgamma'], p['dbeta'], p['bs']) for p in parts]
    o['fsums'] = [p['fs'] for p in parts]
    return o


def _check_shard_sums(k, shards, o):
    """What a rank hands to the collective -- the float64 pairs of every shard -- against tests/sync_bn_ref.py in float64.
    Bounds, per channel, from the arithmetic: the kernel adds n float32 values (their squares are exact in float64) in float64,
    so a forward sum is within n * 2^-53 of the sum of the magnitudes of its terms, and so is the reference: 2 n 2^-53 sum|t|.
    A backward term g = dy * res_scale, and g * xhat with xhat = (z - mean) * inv, is formed in float32 before it is added, the
    reference forms it in float64.  Roundings of 2^-24 each, to first order: two for g (res_scale as a float, the product), five
    for xhat (the subtraction, var + eps, the square root, the reciprocal, the product): 7, taken as 8 * 2^-24 sum|t| on top."""
    Cn, u64, u32 = k.C, 2.0 ** -53, 2.0 ** -24
    ch = lambda t, off: None if t is None else t[:, off:off + Cn].double()
    for (b0, b1), fs, (_, _, bs) in zip(shards, o['fsums'], o['local']):
        n = (b1 - b0) * k.HW
        z, dy, y = ch(k.z[b0:b1], TC.ZO), ch(k.dy[b0:b1], TC.GO), ch(None if k.y_in is None else k.y_in[b0:b1], TC.YO)
        want = S.stats_local(z)
        mag = torch.stack([z.abs().sum((0, 2)), (z * z).sum((0, 2))])
        err = (fs.cpu().view(2, Cn) - want).abs()
        assert bool((err <= 2 * n * u64 * mag).all()), ('forward sums', float((err / mag.clamp_min(1e-300)).max()))
        want, _, _ = S.backward_local(dy, y, z, k.mean, k.var, TC.EPS, k.relu, k.lo_t, k.rscale)
        g = S._masked(dy, y, k.relu, k.lo_t, F64) * k.rscale
        xh = (z - k.mean.double()[None, :, None]) / torch.sqrt(k.var.double()[None, :, None] + TC.EPS)
        mag = torch.stack([g.abs().sum((0, 2)), (g * xh).abs().sum((0, 2))])
        err = (bs.cpu().view(2, Cn) - want).abs()
        assert bool((err <= (2 * n * u64 + 8 * u32) * mag).all()), ('backward sums', float((err / mag.clamp_min(1e-300)).max()))


@pytest.mark.parametrize('combo', UNFROZEN)
@pytest.mark.parametrize('shape', SYNC_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_emulated_ranks_vs_float64_full_batch(shape, combo):
    k = TC.bn_case(shape, combo)
    want = TC.bn_expected(k)
    a, b = SPLITS[shape]
    assert a + b == k.B
    shards = [(0, a), (a, k.B)]
    o = _sync_launch(k, shards)
    Cn = k.C
    sl = dict(y=(TC.YO, 9.0), dz=(TC.ZO, 7.0), dres=(k.dres_off, k.dres0))
    for name, (r64, r32) in want.items():
        got = o[name]
        if name in sl:
            off, sentinel = sl[name]
            assert _outside(got, off, Cn, sentinel), name + ': channels outside the slice were written'
            got = got[:, off:off + Cn]
        assert bool(torch.isfinite(got).all()), name
        if name == 'dres' and not k.acc:
            assert torch.equal(got.cpu(), r64.float()), 'dres (set) is a masked copy of dy'
        _bound('bn/%s/%s' % (k.name, name), got, r64, r32, TC.BN_FLOORS[name])
    assert set(want) == {n for n in o if o[n] is not None and n not in ('local', 'fsums')}
    _check_shard_sums(k, shards, o)
    # a shard's dgamma / dbeta are the float roundings of its own sums
    for dg, db, bs in o['local']:
        assert torch.equal(db, bs[:Cn].float()) and torch.equal(dg, bs[Cn:].float())
    # ordered sums: a second run gives the same bits
    o2 = _sync_launch(k, shards)
    for name in want:
        assert torch.equal(o[name], o2[name]), name
    for (dg, db, bs), (dg2, db2, bs2) in zip(o['local'], o2['local']):
        assert torch.equal(bs, bs2) and torch.equal(dg, dg2) and torch.equal(db, db2)


@pytest.mark.parametrize('shape', TC.BN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_world_of_one_reproduces_the_det_twins(shape):
    lib = _lib.lib()
    k = TC.bn_case(shape, 'racc')           # ReLU mask, res_scale 0.7, dres slice accumulated, running statistics
    B, Cn, HW = shape
    o = _sync_launch(k, [(0, B)])
    z, gamma, lo = _d(k.z), _d(k.gamma), _d(k.lo_t)
    meanin, varin, dy, yin = _d(k.mean), _d(k.var), _d(k.dy), _d(k.y_in)
    mean, var = torch.full((Cn,), 3.0, device=DEV), torch.full((Cn,), 3.0, device=DEV)
    rm, rv = _d(k.rm0.clone()), _d(k.rv0.clone())
    sc, nb = _scratch(B, Cn, HW)
    _lib.check(lib.ct_bn_train_stats_det(z.data_ptr(), B, Cn + TC.ZP, TC.ZO, Cn, HW, mean.data_ptr(), var.data_ptr(), TC.MOMENTUM,
                                         rm.data_ptr(), rv.data_ptr(), sc.data_ptr(), nb, _s()), 'stats det')
    dz, dres = _d(k.dz0.clone()), _d(k.dres0.clone())
    dg, db = torch.full((Cn,), 3.0, device=DEV), torch.full((Cn,), 3.0, device=DEV)
    sc2, nb2 = _scratch(B, Cn, HW)
    _lib.check(lib.ct_bn_train_backward_det(
        dy.data_ptr(), Cn + TC.GP, TC.GO, _p(yin), Cn + TC.YP, TC.YO, z.data_ptr(), meanin.data_ptr(), varin.data_ptr(),
        gamma.data_ptr(), TC.EPS, k.relu, _p(lo), k.rscale, dres.data_ptr(), k.dres_ctot, k.dres_off, k.acc, dz.data_ptr(),
        dg.data_ptr(), db.data_ptr(), Cn + TC.ZP, TC.ZO, B, Cn, HW, sc2.data_ptr(), nb2, _s()), 'backward det')
    torch.cuda.synchronize()
    ldg, ldb, _ = o['local'][0]
    for name, got, twin in (('mean', o['mean'], mean), ('var', o['var'], var), ('rmean', o['rmean'], rm), ('rvar', o['rvar'], rv),
                            ('dgamma', ldg, dg), ('dbeta', ldb, db), ('dgamma of the sums', o['dgamma'], dg),
                            ('dbeta of the sums', o['dbeta'], db), ('dz', o['dz'], dz), ('dres', o['dres'], dres)):
        assert torch.equal(got, twin), name


def test_a_shifted_shard_needs_the_global_statistics():
    """(4,10,1200) as 3 + 1 images with +1 on the second shard's z: the first shard's own statistics are not the batch's."""
    lib = _lib.lib()
    k = TC.bn_case((4, 10, 1200), 'plain')
    B, Cn, HW = 4, 10, 1200
    zc = k.z.clone()
    zc[3:] += 1.0
    m64, v64, _, _ = R.bn_stats(zc, TC.ZO, Cn)
    m32, v32, _, _ = R.bn_stats(zc, TC.ZO, Cn, dtype=F32)
    z0, z1 = _d(zc[:3]), _d(zc[3:])
    own_m, own_v = torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    sc, nb = _scratch(3, Cn, HW)
    _lib.check(lib.ct_bn_train_stats_det(z0.data_ptr(), 3, Cn + TC.ZP, TC.ZO, Cn, HW, own_m.data_ptr(), own_v.data_ptr(), 0.0, None,
                                         None, sc.data_ptr(), nb, _s()), 'stats det')
    s0, s1 = torch.zeros(2 * Cn, dtype=F64, device=DEV), torch.zeros(2 * Cn, dtype=F64, device=DEV)
    _stats_local(z0, 3, Cn, HW, s0)
    _stats_local(z1, 1, Cn, HW, s1)
    tot = s0 + s1
    mean, var = torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    _lib.check(lib.ct_bn_sync_stats_finish(tot.data_ptr(), float(B * HW), Cn, mean.data_ptr(), var.data_ptr(), 0.0, None, None, _s()),
               'finish')
    torch.cuda.synchronize()
    for name, own, got, r64, r32 in (('mean', own_m, mean, m64, m32), ('var', own_v, var, v64, v32)):
        floor = TC.BN_FLOORS[name]
        e_own, e, e32 = rel_err(own.cpu(), r64), rel_err(got.cpu(), r64), rel_err(r32, r64)
        print('%s: shard alone %.3e  synchronized %.3e  e32 %.3e' % (name, e_own, e, e32))
        assert e_own > 100 * floor, (name, e_own)
        assert e < max(floor, 3 * e32), (name, e, e32)


# ------------------------------------------------------------------ two ranks
SMALL = ('extras.3.', 'extras.4.', 'extras.5.', 'extras.6.', 'loc.4.', 'conf.4.', 'obj.4.', 'loc.5.', 'conf.5.', 'obj.5.', 'extras.2.')


def _sync_worker(rank, world, port, q):
    """One rank of test_two_ranks_match_float64_autograd_of_the_full_batch; rank 0 does the float64 replay and the comparisons."""
    try:
        import datetime
        import torch.distributed as dist
        from emu_backend import replay_plan_autograd
        from test_gpu_dp_train import _net
        two = torch.cuda.device_count() >= world
        torch.cuda.set_device(rank if two else 0)
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        dist.init_process_group('nccl' if two else 'gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=world,
                                timeout=datetime.timedelta(seconds=600))
        Bg = 8
        B = Bg // world
        net = _net(300, 20).train()
        sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
        X = synth.images(Bg, 300, 'randn', 2024)
        trt = net.train_runtime(B)
        trt.enable_grad_sync()
        sy = trt.enable_bn_sync()
        assert sy is not None and sy.global_batch == Bg and sy.world == world
        out = net(X[rank * B:(rank + 1) * B].cuda())
        g = torch.Generator().manual_seed(5)
        R = [torch.randn((Bg,) + tuple(t.shape[1:]), generator=g) / (t.numel() * world) ** 0.5 for t in out]
        # a rank's loss is scaled by `world` (as ctdet.dist.global_normalizer scales it): the MEAN of the ranks' gradients is then
        # the gradient of the full-batch functional
        (sum((t * r[rank * B:(rank + 1) * B].cuda()).sum() for t, r in zip(out, R)) * world).backward()
        torch.cuda.synchronize()
        stages = len(sy.stages)
        assert sy.collectives == 2 * stages, (sy.collectives, stages)

        def gather(t):
            t = t.contiguous() if two else t.cpu().contiguous()         # gloo gathers host tensors only
            parts = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(parts, t)
            return [p.cpu() for p in parts]
        need = sorted({st.dst for st in trt.plan.steps if st.kind == 'conv' and not st.segs}
                      | {st.src for st in trt.plan.steps if st.kind == 'pool'})
        bufs = {n: torch.cat(gather(trt.bufs[n])) for n in need}
        outs = [torch.cat(gather(t.detach().reshape(B, -1))) for t in out]
        flat = torch.cat([p.grad.flatten() for p in net.parameters()])
        flats = gather(flat)
        stats = torch.cat([t.flatten().float() for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)
                           for t in (m.running_mean, m.running_var, m.num_batches_tracked)])
        statss = gather(stats)
        info = {'backend': dist.get_backend(), 'device': torch.cuda.current_device(), 'stages': stages}
        if rank != 0:
            q.put((rank, None, info))
            dist.destroy_process_group()
            return
        assert all(torch.equal(flats[0], f) for f in flats[1:]), 'the ranks hold different averaged gradients'
        assert all(torch.equal(statss[0], s) for s in statss[1:]), 'the ranks hold different running statistics'
        assert not torch.equal(statss[0], torch.cat([t.flatten().float() for k, t in sd.items() if 'running' in k or 'tracked' in k]))
        names = {id(p): n for n, p in net.named_parameters()}
        leaf = {i: sd[n].double().requires_grad_(True) for i, n in names.items()}

        def masks(st, off, cout):
            return bufs[st.dst][:, st.dst_coff + off:st.dst_coff + off + cout] > 0
        got64 = replay_plan_autograd(trt.plan, leaf, X, masks, pool_inputs=lambda st: bufs[st.src], batch_stats=True)
        report = {}
        for a, b, n in zip(outs, got64, ('loc', 'conf', 'obj')):
            report['out ' + n] = rel_err(a, b.detach().float())
            assert report['out ' + n] < 1e-4, (n, report)
        sum((t * r.double().reshape(Bg, -1)).sum() for t, r in zip(got64, R)).backward()
        worst, loose = {}, {}
        gmax = max(float(v.grad.abs().max()) for v in leaf.values())
        for name, prm in net.named_parameters():
            assert prm.grad is not None, name
            ref = leaf[id(prm)].grad
            if float(ref.abs().max()) < 1e-9 * gmax:
                # exactly cancelled by a following batch normalisation: the true gradient is 0, the device's is rounding
                assert float(prm.grad.abs().max()) < 1e-5 * gmax, (name, float(prm.grad.abs().max()), gmax)
                continue
            e = rel_err(prm.grad.cpu().double(), ref)
            report['grad ' + name] = e
            if name.startswith(SMALL):
                if e >= 5e-2:
                    loose[name] = e
            elif e >= 1e-4:
                worst[name] = e
        info['report'] = {k: v for k, v in sorted(report.items(), key=lambda kv: -kv[1])[:12]}
        assert not worst, ' '.join('%s:%.1e' % kv for kv in sorted(worst.items(), key=lambda kv: -kv[1])[:12])
        assert not loose, ' '.join('%s:%.1e' % kv for kv in loose.items())
        q.put((rank, None, info))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc(), None))
        raise


def test_two_ranks_match_float64_autograd_of_the_full_batch():
    """RFBNet-300, BatchNorm in train mode, gradient and BatchNorm syncs on; each rank holds half of the bs-8 batch of
    test_batch_stat_bn_network_gradients_match_fp64_autograd and that test's loss (a fixed random linear functional).  The ranks
    gather their activations; rank 0 replays the plan in float64 over the FULL batch with the gathered ReLU masks and pool inputs,
    BatchNorm differentiated through the statistics of all eight images.  Outputs within 1e-4; parameter gradients by that test's
    rule (1e-4, 5e-2 for its `small` list, its cancelled-bias clause); both ranks hold equal averaged gradients and equal running
    statistics of every BatchNorm layer."""
    from test_gpu_dp_train import _free_port
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    ps = [ctx.Process(target=_sync_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    try:
        res = sorted([q.get(timeout=900) for _ in range(world)], key=lambda t: t[0])
        for r in res:
            assert r[1] is None, r[1]
        for p in ps:
            p.join(120)
            assert p.exitcode == 0
    finally:
        for p in ps:
            if p.is_alive():
                p.kill()
    print(res[0][2])
    want = 'nccl' if torch.cuda.device_count() >= world else 'gloo'
    assert [r[2]['backend'] for r in res] == [want] * world
    if want == 'nccl':
        assert len({r[2]['device'] for r in res}) == world
    assert res[0][2]['stages'] > 10
