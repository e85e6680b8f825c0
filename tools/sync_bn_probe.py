#!/usr/bin/env python3
"""What synchronized BatchNorm (TrainRuntime.enable_bn_sync) costs on the data-parallel training step.

    python tools/sync_bn_probe.py [--steps 20 --warmup 5 --rounds 2 --timeout 600]

Two configurations at their per-rank shapes -- RFBNet-300 with 4 images per rank (bs 32 over 8 GPUs) and RFBNet-512 +
Context-Transformer block (phase 2) with 1 image per rank -- over N = min(8, visible GPUs) ranks, with the sync off and on,
alternating `--rounds` times, every (configuration, variant, round) in FRESH processes (one per rank, never more than 8 with a
GPU open).  Every child runs under its own time limit, and the first child that fails ends the run.  With one visible GPU the
group has one rank: the collectives are skipped and the numbers are the cost of the split launches alone (`collectives_per_step`
0); the all-reduce cost needs two or more GPUs.

Per run: ms per step (max over ranks), forward and backward ms (HIP events, rank 0), collectives per step, and -- from a
torch.profiler pass over three more steps -- the launches and the summed device time per step of the new kernels (`bn_sync_*`:
the local reductions, the finish, the backward apply) next to the kernels they replace (`bn_stats_*`, `bn_bwd_*`).
Prints one JSON line and writes it to profiles/sync_bn_probe.json.
"""
import argparse
import json
import os
import signal
import socket
import statistics
import subprocess
import sys
import tempfile
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))
sys.path.insert(0, REPO)

CONFIGS = [('rfb300_phase1_b4', 300, 1, 4), ('rfb512_phase2_b1', 512, 2, 1)]
NEW, OLD = 'bn_sync_', ('bn_stats_', 'bn_bwd_')


def worker(a):
    import torch
    import torch.distributed as dist
    import datetime
    from ctdet import synth
    from models.RFB_Net_vgg import build_net, _CTX_DIMS
    from layers.functions import PriorBox
    from layers.modules.multibox_loss_combined import MultiBoxLoss_combined
    import data as cfgs
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(int(os.environ['LOCAL_RANK']))
    dist.init_process_group('nccl' if world > 1 else 'gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=a.timeout))
    classes = _CTX_DIMS['transfer'][0] if a.phase == 2 else 20
    net = build_net(types.SimpleNamespace(method='ours', phase=a.phase, setting='transfer'), a.size, classes)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()))
    net = net.cuda().train()
    net.device = 'cuda'
    prior_box = PriorBox(getattr(cfgs, 'VOC_%d' % a.size))
    priors = prior_box.forward().cuda()
    nout = classes if a.phase == 1 else net.OBJ_Target.weight.shape[0]
    crit = MultiBoxLoss_combined(nout + 1, 0.5, True, 0, True, 3, 0.5, False)
    crit.sync_normalizer = world > 1
    opt = torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4)
    x = synth.images(a.batch, a.size, 'randn', 1234 + rank).cuda()
    tg = [t.cuda() for t in synth.targets(a.batch, nout + 1, 99 + rank)]
    trt = net.train_runtime(a.batch)
    trt.enable_grad_sync()
    if a.variant == 'on':
        trt.enable_bn_sync(dist.group.WORLD)        # with the group given a world of one runs the split launches too
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def step(timed=False):
        opt.zero_grad(set_to_none=True)
        ev[0].record()
        out = net(x)
        ev[1].record()
        loss = sum(crit(out, priors, tg).values())
        ev[2].record()
        loss.backward()
        ev[3].record()
        opt.step()
        if timed:
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    dist.barrier()
    c0 = trt.bn_sync.collectives if trt.bn_sync is not None else 0
    tf = tb = 0.0
    t0 = time.perf_counter()
    for _ in range(a.steps):
        f, b = step(True)
        tf, tb = tf + f, tb + b
    dt = torch.tensor([(time.perf_counter() - t0) / a.steps], dtype=torch.float64, device='cuda' if world > 1 else 'cpu')
    dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    coll = ((trt.bn_sync.collectives - c0) / a.steps) if trt.bn_sync is not None else 0.0
    kern, psteps = {}, 3
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(psteps):
                step()
            torch.cuda.synchronize()
        for e in prof.key_averages():
            key = 'new' if NEW in e.key else 'old' if any(o in e.key for o in OLD) else None
            if key:
                us = getattr(e, 'device_time_total', None)
                us = e.cuda_time_total if us is None else us
                n, ms = kern.get(key, (0, 0.0))
                kern[key] = (n + e.count, ms + us / 1e3)
        kern = {k: {'launches_per_step': n / psteps, 'device_ms_per_step': round(ms / psteps, 4)} for k, (n, ms) in kern.items()}
    except Exception as e:              # the timing above stands without the kernel breakdown
        kern = {'error': repr(e)}
    if rank == 0:
        print('SYNC_BN_PROBE ' + json.dumps({
            'ms_per_step': round(float(dt) * 1e3, 3), 'fwd_ms': round(tf / a.steps, 3), 'bwd_ms': round(tb / a.steps, 3),
            'collectives_per_step': coll, 'stages': len(trt.bn_sync.stages) if trt.bn_sync is not None else 0,
            'global_batch': trt.bn_sync.global_batch if trt.bn_sync is not None else a.batch * world, 'bn_kernels': kern}), flush=True)
    dist.destroy_process_group()


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


WORKER = [sys.executable, os.path.abspath(__file__), '--worker']


def end_ranks(procs):
    """End every rank that still runs, wrapper and worker alike: each rank is the leader of a process group of its own, so the
    signal reaches the `timeout` wrapper AND the python under it.  SIGTERM first, SIGKILL after 10 s; returns once all are gone."""
    live = [p for p in procs if p.poll() is None]
    for sig in (signal.SIGTERM, signal.SIGKILL):
        for p in live:
            try:
                os.killpg(p.pid, sig)
            except ProcessLookupError:
                pass
        deadline = time.monotonic() + 10
        for p in live:
            try:
                p.wait(timeout=max(0.1, deadline - time.monotonic()))
            except subprocess.TimeoutExpired:
                pass
        live = [p for p in live if p.poll() is None]
        if not live:
            break
    for p in procs:
        p.wait()
        try:                        # a worker that outlived its wrapper
            os.killpg(p.pid, signal.SIGKILL)
        except (ProcessLookupError, PermissionError):
            pass


def run_ranks(argv, world, timeout, cmd=None):
    """One child per rank, each under `timeout` (its own `timeout -k 10` wrapper, its own process group).  All ranks are polled:
    the first one that ends with a non-zero status -- its time limit included -- ends the others at once (end_ranks), and the
    run stops only after every child is gone."""
    port = free_port()
    procs, failed = [], None
    with tempfile.TemporaryFile('w+') as out0:
        try:
            for r in range(world):
                env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                           MASTER_PORT=str(port))
                procs.append(subprocess.Popen(['timeout', '-k', '10', str(timeout)] + (cmd or WORKER) + argv, env=env,
                                              stdout=out0 if r == 0 else subprocess.DEVNULL, start_new_session=True))
            limit = time.monotonic() + timeout + 30
            while failed is None and any(p.poll() is None for p in procs):
                for r, p in enumerate(procs):
                    if p.poll() not in (None, 0):
                        failed = (r, p.returncode)
                        break
                else:
                    if time.monotonic() > limit:
                        failed = (-1, 124)
                    else:
                        time.sleep(0.05)
            if failed is None:
                failed = next(((r, p.returncode) for r, p in enumerate(procs) if p.returncode != 0), None)
        finally:
            end_ranks(procs)
        out0.seek(0)
        out = out0.read()
    if failed:
        sys.exit('sync_bn_probe: rank %d of `%s` ended with status %d; the other ranks were ended and nothing more is started'
                 % (failed[0], ' '.join(argv), failed[1]))
    line = [ln for ln in out.splitlines() if ln.startswith('SYNC_BN_PROBE ')]
    if not line:
        sys.exit('sync_bn_probe: no result line from `%s`' % ' '.join(argv))
    return json.loads(line[-1][len('SYNC_BN_PROBE '):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=600)
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--size', type=int)
    ap.add_argument('--phase', type=int)
    ap.add_argument('--batch', type=int)
    ap.add_argument('--variant', choices=('off', 'on'))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    # the GPU count from a child: this process never opens a device
    n = subprocess.run(['timeout', '-k', '10', '120', sys.executable, '-c', 'import torch; print(torch.cuda.device_count())'],
                       capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1]
    world = min(8, int(n))
    if world < 1:
        sys.exit('sync_bn_probe: no HIP device visible')
    report = {'sync_bn_probe': 1, 'ranks': world, 'steps': a.steps, 'warmup': a.warmup, 'rounds': a.rounds, 'configs': {}}
    for tag, size, phase, batch in CONFIGS:
        runs = {'off': [], 'on': []}
        for _ in range(a.rounds):
            for variant in ('off', 'on'):
                argv = ['--size', str(size), '--phase', str(phase), '--batch', str(batch), '--variant', variant,
                        '--steps', str(a.steps), '--warmup', str(a.warmup), '--timeout', str(a.timeout)]
                runs[variant].append(run_ranks(argv, world, a.timeout))
        med = {v: statistics.median(r['ms_per_step'] for r in runs[v]) for v in runs}
        report['configs'][tag] = {'size': size, 'phase': phase, 'images_per_rank': batch, 'runs': runs, 'median_ms_per_step': med}
    line = json.dumps(report)
    print(line)
    os.makedirs(os.path.join(REPO, 'profiles'), exist_ok=True)
    with open(os.path.join(REPO, 'profiles', 'sync_bn_probe.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
