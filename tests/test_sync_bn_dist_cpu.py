"""ctdet.dist.BnStatSyncer over two gloo ranks on the CPU: the arena layout, one collective per stage and pass, the global batch
of uneven shards (3 + 1), and a layout mismatch that raises on BOTH ranks instead of hanging.  Every rank's process group has a
finite timeout; the parent waits with a timeout and kills whatever is left on any failure."""
import datetime
import socket

import torch
import torch.multiprocessing as mp

from ctdet import _lib
from ctdet import dist as cdist

STAGES = [('Norm.branch0.0', [3, 5]), ('extras.0', [4])]         # 2 * (8 + 4) doubles forward, as many backward


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, mismatch):
    try:
        import torch.distributed as dist
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=world,
                                timeout=datetime.timedelta(seconds=60))
        calls = []
        real = dist.all_reduce
        dist.all_reduce = lambda t, *a, **k: (calls.append(t.numel()), real(t, *a, **k))[1]
        stages = [(n, list(cs)) for n, cs in STAGES]
        if mismatch and rank == 1:
            stages[1] = ('extras.0', [6])
        try:
            sy = cdist.BnStatSyncer(stages, 3 if rank == 0 else 1, 'cpu')
        except _lib.CtdetError as e:
            q.put((rank, 'raised', str(e)))
            dist.destroy_process_group()
            return
        built = len(calls)
        out = {'built': built, 'world': sy.world, 'global_batch': sy.global_batch, 'numel': sy.arena.numel(),
               'dtype': str(sy.arena.dtype)}
        base = sy.arena.data_ptr()
        off = lambda t: (t.data_ptr() - base) // 8
        out['views'] = [(off(sy.forward_view(n)), sy.forward_view(n).numel(), off(sy.backward_view(n)), sy.backward_view(n).numel())
                        for n, _ in STAGES]
        out['parts'] = [(off(sy.part(sy.forward_view(n), n, k)), sy.part(sy.forward_view(n), n, k).numel(),
                         off(sy.part(sy.backward_view(n), n, k)))
                        for n, cs in STAGES for k in range(len(cs))]
        sy.arena.fill_(float(rank + 1))
        sy.reduce_forward('Norm.branch0.0')
        out['after_fwd'] = (sy.arena.clone(), calls[built:])
        sy.reduce_backward('extras.0')
        out['after_bwd'] = (sy.arena.clone(), calls[built:])
        out['collectives'] = sy.collectives
        q.put((rank, 'ok', out))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, 'error', traceback.format_exc()))
        raise


def _run(mismatch):
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q, mismatch)) for r in range(world)]
    for p in ps:
        p.start()
    try:
        res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
        for p in ps:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in ps:
            if p.is_alive():
                p.kill()
    return res


def test_layout_collectives_and_global_batch():
    res = _run(False)
    for rank, status, o in res:
        assert status == 'ok', o
        assert o['world'] == 2 and o['global_batch'] == 4           # 3 + 1 images
        assert o['built'] == 2                                      # the layout checksum and ONE reduction of the batch sizes
        assert o['numel'] == 48 and o['dtype'] == 'torch.float64'
        assert o['views'] == [(0, 16, 16, 16), (32, 8, 40, 8)]
        assert o['parts'] == [(0, 6, 16), (6, 10, 22), (32, 8, 40)]
        arena, calls = o['after_fwd']
        assert calls == [16]                                        # one collective, the stage's forward view
        assert bool((arena[:16] == 3).all()) and bool((arena[16:] == rank + 1).all())
        arena, calls = o['after_bwd']
        assert calls == [16, 8]
        assert bool((arena[40:48] == 3).all()) and bool((arena[16:40] == rank + 1).all())
        assert o['collectives'] == 2


def test_a_layout_mismatch_raises_on_every_rank():
    res = _run(True)
    assert [r[1] for r in res] == ['raised', 'raised'], res
    for _, _, msg in res:
        assert 'disagree' in msg


def test_world_of_one_needs_no_process_group():
    sy = cdist.BnStatSyncer(STAGES, 5, 'cpu')
    assert sy.world == 1 and sy.global_batch == 5 and sy.arena.numel() == 48
    sy.arena.fill_(2.0)
    sy.reduce_forward('extras.0')
    assert sy.collectives == 0 and bool((sy.arena == 2).all())
