"""The fused multi-tensor SGD step on the MI355X (ct_sgd_step, ctdet.optim.FusedSGD).

Yardsticks: the recurrence include/ctdet.h states, restated in NumPy float32 (tests/sgd_ref.py) -- bit for bit -- and
torch.optim.SGD on the CPU with torch's own distance from an fp64 evaluation as the tolerance ("close to torch":
max|fused - fp64| <= 2 * max|torch_cpu - fp64| + ulp(max|p|) per tensor).  Never the fused code itself."""
import copy
import types

import numpy as np
import pytest
import torch

import sgd_ref
from conftest import rel_err
from ctdet import _lib, ops, synth
from ctdet.optim import FusedSGD
from utils import checkpointer as ck
from utils import solver

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CANARY = 64
SIZES = [1, 3, 8, 63, 64, 65, 126, 1023, 4096, 4097, 2 ** 20 + 3, 4718592]
TRIPLES = [(0.0, 0.0, 0), (0.9, 0.0, 0), (0.9, 0.1, 0), (0.9, 0.0, 1)]
ALL_OFFSETS = [(a, b, c) for a in range(4) for b in range(4) for c in range(4)]
# the two large sizes: every shift of the 16-byte path, and mixed offsets that take the dword path
BIG_OFFSETS = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 2), (3, 0, 0), (1, 1, 2), (2, 3, 2)]


class Arena:
    """Tensors as views into three flat device buffers (param, grad, momentum) at chosen element offsets past a
    16-byte boundary, a 64-element canary on both sides of every view.  The host keeps the expected image of each
    WHOLE buffer, so one comparison covers the tensors, the canaries and everything in between."""

    def __init__(self, sizes, offsets, seed, grad_std=0.1):
        assert len(sizes) == len(offsets)
        self.sizes = list(sizes)
        self.start = []                                      # per tensor: (param, grad, buf) first element
        cur = [0, 0, 0]
        for n, off in zip(sizes, offsets):
            st = []
            for r in range(3):
                s = (cur[r] + CANARY + 3) // 4 * 4 + off[r]
                st.append(s)
                cur[r] = s + n + CANARY
            self.start.append(tuple(st))
        rng = np.random.RandomState(seed)
        self.host = [rng.randn(c + 4).astype(np.float32) for c in cur]
        self.host[1] *= np.float32(grad_std)
        self.rng = rng

    def upload(self):
        self.dev = [torch.from_numpy(h).to(DEV) for h in self.host]
        assert all(d.data_ptr() % 16 == 0 for d in self.dev)

    def view(self, r, i, dev=True):
        s, n = self.start[i][r], self.sizes[i]
        return (self.dev[r] if dev else self.host[r])[s:s + n]

    def run(self, lrs, wds, momentum, dampening, nesterov, grad_scale=1.0, steps=5, stream=None):
        """`steps` calls of ops.sgd_step over all tensors; after every step the three buffers must equal the NumPy
        restatement applied to the views and NOTHING else (canaries, gradients)."""
        has_buf = momentum != 0
        grad0 = self.host[1].copy()
        for it in range(steps):
            items = [(self.view(0, i), self.view(1, i), self.view(2, i) if has_buf else None, lrs[i], wds[i], it == 0)
                     for i in range(len(self.sizes))]
            if stream is None:
                ops.sgd_step(items, momentum, dampening, nesterov, grad_scale)
            else:
                done = torch.cuda.Event()
                stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    ops.sgd_step(items, momentum, dampening, nesterov, grad_scale)
                    done.record()
                torch.cuda.current_stream().wait_event(done)
            for i in range(len(self.sizes)):
                p, g = self.view(0, i, False), self.view(1, i, False)
                b = self.view(2, i, False) if has_buf else None
                newp, newb = sgd_ref.step(p, g, b, lrs[i], wds[i], momentum, dampening, nesterov, grad_scale, it == 0)
                p[:] = newp
                if has_buf:
                    b[:] = newb
            got = [d.cpu().numpy() for d in self.dev]
            assert np.array_equal(got[1].view(np.uint32), grad0.view(np.uint32)), 'gradients were written (step %d)' % it
            for r, name in ((0, 'param'), (2, 'momentum_buf')):
                if not sgd_ref.bits_equal(got[r], self.host[r]):
                    self._explain(got[r], r, name, it)
        return self

    def _explain(self, got, r, name, it):
        want = self.host[r]
        bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))[0]
        first = int(bad[0])
        owner = 'canary / gap'
        for i, st in enumerate(self.start):
            if st[r] <= first < st[r] + self.sizes[i]:
                owner = 'tensor %d (numel %d, offsets %s) element %d' % (i, self.sizes[i], [s % 4 for s in st], first - st[r])
        raise AssertionError('%s differs from the restatement after step %d at %d of %d positions; first: flat %d = %s, '
                             'got %r want %r' % (name, it + 1, bad.size, got.size, first, owner, got[first], want[first]))


def _hyper(n, wd):
    lrs = [0.01 * (1 + i % 7) for i in range(n)]
    wds = [0.0 if (wd == 0 or i % 5 == 4) else wd * (1 + i % 3) for i in range(n)]      # wd == 0 beside wd != 0 in one call
    return lrs, wds


def _sweep_layout():
    sizes, offs = [], []
    for n in SIZES:
        for o in (ALL_OFFSETS if n <= 4097 else BIG_OFFSETS):
            sizes.append(n)
            offs.append(o)
    return sizes, offs


# 1 + 2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grad_scale', [1.0, 0.125])
@pytest.mark.parametrize('wd', [0.0, 5e-4])
@pytest.mark.parametrize('momentum,dampening,nesterov', TRIPLES)
def test_bit_exact_sweep_and_nothing_else_touched(momentum, dampening, nesterov, wd, grad_scale):
    """Every size at every (param, grad, buf) offset combination (the two large sizes at eight of them), five steps,
    a different lr and weight decay per tensor inside ONE call: params and momentum buffers equal the restatement
    bit for bit after every step, canaries and gradients keep their bits; momentum 0 passes momentum_buf = NULL."""
    sizes, offs = _sweep_layout()
    a = Arena(sizes, offs, seed=11)
    a.upload()
    lrs, wds = _hyper(len(sizes), wd)
    a.run(lrs, wds, momentum, dampening, nesterov, grad_scale, steps=5)


# 3 -----------------------------------------------------------------------------------------------------------------
def _rfb512_phase2_shapes():
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=2, setting='transfer'), 512, 20)
    return [p.numel() for _, p in net.named_parameters() if p.requires_grad]


@pytest.mark.parametrize('case', ['one', 'thousand', 'rfb512'])
def test_table_limits(case):
    rng = np.random.RandomState(3)
    if case == 'one':
        sizes = [70001]
    elif case == 'thousand':                                  # more than a kernel-argument table holds (80)
        sizes = [int(v) for v in rng.randint(8, 301, 1000)]
    else:
        sizes = _rfb512_phase2_shapes()
        assert len(sizes) == 293
    offs = [tuple(int(v) for v in rng.randint(0, 4, 3)) if i % 2 else (int(rng.randint(0, 4)),) * 3
            for i in range(len(sizes))]
    a = Arena(sizes, offs, seed=5, grad_std=0.01)
    a.upload()
    lrs, wds = _hyper(len(sizes), 5e-4)
    a.run(lrs, wds, 0.9, 0.0, 0, 1.0, steps=3)
    per = _lib.lib().ct_sgd_tensors_per_launch()
    assert per == 80 and (len(sizes) + per - 1) // per == {'one': 1, 'thousand': 13, 'rfb512': 4}[case]


def test_empty_calls_and_empty_tensors_are_no_ops():
    ops.sgd_step([], 0.9, 0.0, False)
    a = Arena([0, 17, 0], [(1, 2, 3), (1, 1, 1), (0, 0, 0)], seed=2)
    a.upload()
    a.run([0.1] * 3, [5e-4] * 3, 0.9, 0.0, 0, steps=2)
    z = torch.empty(0, device=DEV)
    ops.sgd_step([(z, z.clone(), z.clone(), 0.1, 0.0, True)], 0.9, 0.0, False)
    torch.cuda.synchronize()


# 4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('momentum,nesterov', [(0.0, 0), (0.9, 0), (0.9, 1)])
def test_non_finite_gradients_propagate_as_the_recurrence_says(momentum, nesterov):
    sizes, offs = [4099, 4099, 257], [(0, 0, 0), (1, 2, 3), (3, 3, 3)]
    a = Arena(sizes, offs, seed=9)
    special = {5: np.nan, 64: np.inf, 65: -np.inf, 130: -0.0, 255: np.nan, 256: np.inf}
    for i in range(3):
        g = a.view(1, i, False)
        for pos, v in special.items():
            g[pos] = v
        a.view(0, i, False)[131] = 0.0                       # p = +0 and g = -0 side by side
        g[131] = -0.0
    a.upload()
    before = [a.view(0, i, False).copy() for i in range(3)]
    a.run([0.1, 0.2, 0.3], [0.0, 5e-4, 0.0], momentum, 0.0, nesterov, steps=2)
    for i in range(3):
        p = a.view(0, i).cpu().numpy()
        bad = sorted(np.nonzero(~np.isfinite(p))[0].tolist())
        assert bad == [5, 64, 65, 255, 256], (i, bad)          # the neighbours stayed finite
        assert np.isnan(p[5]) and np.isnan(p[255])
        if momentum == 0 and i != 1:                         # p - lr * (+-inf); momentum or weight decay make inf - inf
            assert p[64] == -np.inf and p[65] == np.inf and p[256] == -np.inf
        else:
            assert not np.isfinite(p[[64, 65, 256]]).any()
        if i != 1:                                           # no weight decay: a -0.0 gradient leaves p's bits alone
            assert p[130] == before[i][130] and p[131] == 0.0


# 5 -----------------------------------------------------------------------------------------------------------------
def _args(phase=2, **kw):
    d = dict(method='ours', phase=phase, setting='transfer', lr=4e-3, weight_decay=5e-4, momentum=0.9, steps=[3, 6],
             warmup_iter=4)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _net(size, C, phase, device):
    from models.RFB_Net_vgg import build_net
    net = build_net(_args(phase), size, C)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()), strict=True)
    if device == 'cuda':
        net = net.cuda()
        net.device = 'cuda'
    return net


def _report(tag, rows):
    """rows: (name, ok, e_fused, e_torch, bound).  Prints the worst ratio and asserts every tensor."""
    worst = max(rows, key=lambda r: r[2] / r[4])
    print('%s: %d tensors, max|fused - fp64| %.3e, max|torch_cpu - fp64| %.3e, worst tensor %s: fused %.3e torch %.3e '
          'bound %.3e' % (tag, len(rows), max(r[2] for r in rows), max(r[3] for r in rows), worst[0], worst[2], worst[3],
                          worst[4]))
    assert all(r[1] for r in rows), [r for r in rows if not r[1]][:5]


def test_fused_sgd_against_torch_cpu_on_the_network():
    """RFBNet-300 phase 2, the groups of build_optimizer ('ours': x0.1 / x0.5 multipliers), WarmupMultiStepLR with
    milestones [3, 6] and 4 warm-up iterations, 10 steps of seeded gradients (std 1e-2): FusedSGD on the device
    against torch.optim.SGD on the CPU (close to torch) and against the restatement driven by the same per-step lr
    list (bit for bit)."""
    args = _args(2)
    net_d, net_c = _net(300, 20, 2, 'cuda'), _net(300, 20, 2, 'cpu')
    opt_d = solver.build_optimizer(args, net_d, fused=True)
    opt_c = solver.build_optimizer(args, net_c, fused=False)
    assert type(opt_d) is FusedSGD and type(opt_c) is torch.optim.SGD and len(opt_d.param_groups) == 227
    assert sorted(set(round(g['lr'] / args.lr, 6) for g in opt_d.param_groups)) == [0.1, 0.5, 1.0]
    sch_d, sch_c = solver.build_lr_scheduler(args, opt_d), solver.build_lr_scheduler(args, opt_c)
    names = [n for n, p in net_c.named_parameters() if p.requires_grad]
    prm_d = [g['params'][0] for g in opt_d.param_groups]
    prm_c = [g['params'][0] for g in opt_c.param_groups]
    p32 = [p.detach().numpy().copy() for p in prm_c]
    p64 = [p.astype(np.float64) for p in p32]
    b32, b64 = [None] * len(p32), [None] * len(p32)
    gen = torch.Generator().manual_seed(2024)
    seen_lr = set()
    for it in range(10):
        lrs = [g['lr'] for g in opt_c.param_groups]
        assert lrs == [g['lr'] for g in opt_d.param_groups]
        seen_lr.add(lrs[-1])
        for i, (pd, pc) in enumerate(zip(prm_d, prm_c)):
            g = torch.randn(pc.shape, generator=gen) * 1e-2
            pc.grad = g
            pd.grad = g.to(DEV)
            gn = g.numpy()
            p32[i], b32[i] = sgd_ref.step(p32[i], gn, b32[i], lrs[i], 5e-4, 0.9, 0.0, False, first_step=it == 0)
            p64[i], b64[i] = sgd_ref.step(p64[i], gn, b64[i], lrs[i], 5e-4, 0.9, 0.0, False, first_step=it == 0,
                                          dtype=np.float64)
        opt_d.step()
        opt_c.step()
        sch_d.step()
        sch_c.step()
        assert opt_d.last_calls == 1
    assert len(seen_lr) >= 6                                  # warm-up and both milestones were crossed
    rows = []
    for i, name in enumerate(names):
        got = prm_d[i].detach().cpu().numpy()
        assert sgd_ref.bits_equal(got, p32[i]), name
        assert sgd_ref.bits_equal(opt_d.state[prm_d[i]]['momentum_buffer'].cpu().numpy(), b32[i]), name
        rows.append((name,) + sgd_ref.close_to_torch(got, prm_c[i].detach().numpy(), p64[i]))
    _report('network, 10 steps', rows)


# 6 -----------------------------------------------------------------------------------------------------------------
def _toy(device):
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Conv2d(4, 37, 5),
                            torch.nn.Linear(211, 307))
    return m.to(device)


def _toy_grads(model, it):
    gen = torch.Generator().manual_seed(100 + it)
    return [torch.randn(p.shape, generator=gen) * 1e-2 for p in model.parameters()]


def _drive(model, opt, its):
    for it in its:
        for p, g in zip(model.parameters(), _toy_grads(model, it)):
            p.grad = g.to(p.device)
        opt.step()


KW = dict(lr=0.05, momentum=0.9, weight_decay=5e-4)


def test_checkpoint_interchange_with_torch_sgd(tmp_path):
    base = _toy('cpu')
    # the yardsticks: torch on the CPU for 8 steps, and the fp64 restatement
    m_cpu = copy.deepcopy(base)
    _drive(m_cpu, torch.optim.SGD(m_cpu.parameters(), **KW), range(8))
    p64 = [p.detach().numpy().astype(np.float64) for p in base.parameters()]
    b64 = [None] * len(p64)
    for it in range(8):
        for i, g in enumerate(_toy_grads(base, it)):
            p64[i], b64[i] = sgd_ref.step(p64[i], g.numpy(), b64[i], KW['lr'], KW['weight_decay'], KW['momentum'], 0.0,
                                          False, first_step=it == 0, dtype=np.float64)
    # uninterrupted fused run
    m_full = copy.deepcopy(base).to(DEV)
    _drive(m_full, FusedSGD(m_full.parameters(), **KW), range(8))
    # fused -> (state_dict through DetectionCheckpointer.save / load) -> fused
    m_a = copy.deepcopy(base).to(DEV)
    opt_a = FusedSGD(m_a.parameters(), **KW)
    _drive(m_a, opt_a, range(4))
    cargs = types.SimpleNamespace(phase=1, save_folder=str(tmp_path), method='ours', setting='transfer')
    ck.DetectionCheckpointer(m_a, cargs, optimizer=opt_a).save('model_0000003', iteration=3)
    m_b = _toy(DEV)
    for p in m_b.parameters():
        p.data.add_(1.0)                                      # really loaded, not inherited from the seed
    opt_b = FusedSGD(m_b.parameters(), **KW)
    c = ck.DetectionCheckpointer(m_b, cargs, optimizer=opt_b)
    assert c.resume_or_load('', resume=True) == {'iteration': 3}
    assert all(opt_b.state[p]['momentum_buffer'].is_cuda for p in m_b.parameters())
    _drive(m_b, opt_b, range(4, 8))
    for (n, a), b in zip(m_full.named_parameters(), m_b.parameters()):
        assert torch.equal(a.detach(), b.detach()), 'fused resumed from fused differs from the uninterrupted run: ' + n
    # torch (device) -> fused, and fused -> torch (device)
    mixed = {}
    for tag, first, second in (('torch->fused', torch.optim.SGD, FusedSGD), ('fused->torch', FusedSGD, torch.optim.SGD)):
        m = copy.deepcopy(base).to(DEV)
        o1 = first(m.parameters(), **KW)
        _drive(m, o1, range(4))
        sd = copy.deepcopy(o1.state_dict())
        o2 = second(m.parameters(), **KW)
        o2.load_state_dict(sd)
        assert sorted(o2.state_dict()['state']) == sorted(sd['state'])
        assert all(set(v) == {'momentum_buffer'} for v in o2.state_dict()['state'].values())
        _drive(m, o2, range(4, 8))
        mixed[tag] = m
    for tag, m in list(mixed.items()) + [('fused', m_full)]:
        rows = [(n,) + sgd_ref.close_to_torch(p.detach().cpu().numpy(), q.detach().numpy(), r)
                for (n, p), q, r in zip(m.named_parameters(), m_cpu.parameters(), p64)]
        _report(tag + ', 8 steps', rows)


# 7 -----------------------------------------------------------------------------------------------------------------
def test_skipped_parameters_groups_and_grad_scale():
    torch.manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (1000, 77, 4099, 5)]
    start = [p.detach().cpu().numpy().copy() for p in ps]
    grads = [[torch.randn(p.shape) * 1e-2 for p in ps] for _ in range(3)]
    groups = [{'params': ps[:2], 'momentum': 0.9}, {'params': ps[2:], 'momentum': 0.5, 'lr': 0.2, 'weight_decay': 0.0}]
    opt = FusedSGD(groups, 0.1, momentum=0.9, weight_decay=5e-4)
    hyper = [(0.1, 5e-4, 0.9), (0.1, 5e-4, 0.9), (0.2, 0.0, 0.5), (0.2, 0.0, 0.5)]
    want, bufs = [s.copy() for s in start], [None] * 4
    for it in range(3):
        for i, p in enumerate(ps):
            p.grad = None if i == 1 else grads[it][i].to(DEV)
            if i != 1:
                lr, wd, m = hyper[i]
                want[i], bufs[i] = sgd_ref.step(want[i], grads[it][i].numpy(), bufs[i], lr, wd, m, 0.0, False,
                                                first_step=it == 0)
        opt.step()
        assert opt.last_calls == 2                            # one ct_sgd_step call per distinct momentum triple
    for i, p in enumerate(ps):
        assert sgd_ref.bits_equal(p.detach().cpu().numpy(), want[i]), i
    assert ps[1] not in opt.state and ps[1]._version == 0     # grad None: bits kept (checked above), no state
    assert sgd_ref.bits_equal(opt.state[ps[2]]['momentum_buffer'].cpu().numpy(), bufs[2])
    # grad_scale = 1/8 against gradients divided by 8 beforehand (exact: a power of two)
    res = []
    for scale in (0.125, None):
        qs = [torch.nn.Parameter(torch.from_numpy(s.copy()).to(DEV)) for s in start]
        o = FusedSGD(qs, 0.1, momentum=0.9, weight_decay=5e-4)
        assert o.grad_scale == 1.0
        if scale:
            o.grad_scale = scale
        for it in range(3):
            for q, g in zip(qs, grads[it]):
                q.grad = (g if scale else g / 8).to(DEV)
            o.step()
        res.append([q.detach().cpu().numpy() for q in qs] + [o.state[q]['momentum_buffer'].cpu().numpy() for q in qs])
    assert all(sgd_ref.bits_equal(a, b) for a, b in zip(*res))
    # closure contract
    assert float(FusedSGD(ps, 0.1).step(lambda: torch.tensor(3.5))) == 3.5
    # not contiguous fp32: an error, no fallback
    bad = torch.nn.Parameter(torch.randn(8, 8, device=DEV).t())
    bad.grad = torch.randn(8, 8, device=DEV)
    with pytest.raises(_lib.CtdetError):
        FusedSGD([bad], 0.1).step()
    half = torch.nn.Parameter(torch.randn(8, device=DEV).half())
    half.grad = torch.randn(8, device=DEV).half()
    with pytest.raises(_lib.CtdetError):
        FusedSGD([half], 0.1).step()


# 8 -----------------------------------------------------------------------------------------------------------------
def test_in_the_training_step():
    from layers.functions import PriorBox
    from layers.modules.multibox_loss_combined import MultiBoxLoss_combined
    from data import VOC_300
    net = _net(300, 20, 1, 'cuda').train()
    assert net.train_runtime(2) is not None
    priors = PriorBox(VOC_300).forward().cuda()
    crit = MultiBoxLoss_combined(21, 0.5, True, 0, True, 3, 0.5, False)
    x = synth.images(2, 300, 'randn', 1234).cuda()
    tg = [t.cuda() for t in synth.targets(2, 21, 99)]
    sum(crit(net(x), priors, tg).values()).backward()
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    assert all(p.grad is not None for _, p in named)
    grads = [p.grad.detach().clone() for _, p in named]
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for _, p in named]
    p64 = [c.detach().numpy().astype(np.float64) for c in cpu]
    for c, g in zip(cpu, grads):
        c.grad = g.cpu()
    kw = dict(lr=1e-3, momentum=0.9, weight_decay=5e-4)
    torch.optim.SGD(cpu, **kw).step()
    for (_, p), g in zip(named, grads):
        p.grad = g
    FusedSGD([p for _, p in named], **kw).step()
    rows = []
    for (n, p), c, r, g in zip(named, cpu, p64, grads):
        ref, _ = sgd_ref.step(r, g.cpu().numpy(), None, kw['lr'], kw['weight_decay'], 0.9, 0.0, False, first_step=True,
                              dtype=np.float64)
        rows.append((n,) + sgd_ref.close_to_torch(p.detach().cpu().numpy(), c.detach().numpy(), ref))
    _report('training step', rows)
    loss = sum(crit(net(x), priors, tg).values())
    assert bool(torch.isfinite(loss)), float(loss)


# 9 -----------------------------------------------------------------------------------------------------------------
def test_version_counters_and_the_inference_cache_see_the_update():
    ps = [torch.nn.Parameter(torch.randn(100, device=DEV)) for _ in range(3)]
    opt = FusedSGD(ps, 0.1, momentum=0.9)
    for rnd in range(2):
        ps[0].grad, ps[1].grad, ps[2].grad = torch.ones(100, device=DEV), None, torch.ones(100, device=DEV)
        v = [p._version for p in ps]
        bv = [opt.state[p]['momentum_buffer']._version for p in (ps[0], ps[2])] if rnd else None
        opt.step()
        assert ps[0]._version > v[0] and ps[2]._version > v[2] and ps[1]._version == v[1]
        if rnd:
            assert all(opt.state[p]['momentum_buffer']._version > b for p, b in zip((ps[0], ps[2]), bv))
    # the eval runtime packs weights once and re-packs when (data_ptr, _version) of a parameter moves
    x = synth.images(1, 300, 'randn', 7).cuda()
    nets = [_net(300, 20, 1, 'cuda').eval() for _ in range(2)]
    before = [[t.cpu().numpy() for t in n(x)] for n in nets]
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(p.shape, generator=gen) * 0.02 * float(p.detach().abs().mean()) for p in nets[0].parameters()]
    for n, cls in zip(nets, (FusedSGD, torch.optim.SGD)):
        prm = [p for p in n.parameters() if p.requires_grad]
        for p, g in zip(n.parameters(), grads):
            if p.requires_grad:
                p.grad = g.to(DEV)
        cls(prm, 1.0, momentum=0.9, weight_decay=5e-4).step()
    after = [[t.cpu().numpy() for t in n(x)] for n in nets]
    for k, name in enumerate(('loc', 'conf', 'obj')):
        assert np.isfinite(after[0][k]).all() and np.isfinite(after[1][k]).all()
        e = rel_err(after[0][k], after[1][k])
        moved = [rel_err(after[j][k], before[j][k]) for j in range(2)]
        print('%s: fused vs torch after the step %.3e; moved by the step: fused %.3e torch %.3e' % (name, e, *moved))
        assert e < 1e-4, (name, e)
        assert min(moved) > 1e-3, (name, moved)             # stale packed weights would leave the output where it was


# 10 ----------------------------------------------------------------------------------------------------------------
def test_side_stream_gives_the_same_bits():
    sizes = [1, 65, 4097, 2 ** 20 + 3, 300000]
    offs = [(0, 0, 0), (1, 2, 3), (2, 2, 2), (3, 3, 3), (0, 1, 0)]
    lrs, wds = _hyper(len(sizes), 5e-4)
    out = []
    for stream in (None, torch.cuda.Stream()):
        a = Arena(sizes, offs, seed=21)
        a.upload()
        a.run(lrs, wds, 0.9, 0.0, 0, steps=3, stream=stream)
        torch.cuda.synchronize()
        out.append([d.cpu().numpy() for d in a.dev])
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(*out))
