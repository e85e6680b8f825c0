#!/usr/bin/env python3
"""One-GPU training-step timing: RFBNet forward (batch-stat BN) + MultiBoxLoss + HIP backward + SGD.
   python tools/train_bench.py [--size 300 --batch 32 --classes 20 --steps 5] [--fused-sgd] [--per-tensor-groups] [--wgrad-h2]
                               [--optimizer sgd|adamw] [--clip-norm X] [--ema DECAY] [--deterministic] [--loc-loss NAME] [--loc-weight X]
                               [--conf-loss focal [--focal-gamma X --focal-alpha X]] [--matcher ssd|atss|tal [--atss-topk K] [--tal-topk K --tal-alpha A --tal-beta B]] [--json]
                               [--sync-bn]
   --classes: classes of the conf head; default 20, with --phase 2 the width of the Context-Transformer block (60 for 'transfer',
   15 for 'incre': the head feeds the block);
   --fused-sgd: ctdet.optim.FusedSGD (one multi-tensor HIP update) instead of torch.optim.SGD;
   --optimizer adamw: ctdet.optim.FusedAdamW (lr 1e-4, betas 0.9 / 0.999, eps 1e-8, weight decay 5e-4; the fused multi-tensor HIP AdamW
   update) in place of SGD; --clip-norm and --ema then go to it; the JSON line is always printed;
   --wgrad-h2: CTDET_WGRAD_H2=1 for this run (the 1x1 weight gradients on ct_conv2d_wgrad_h2);
   --clip-norm X: FusedSGD(max_grad_norm=X) (implies --fused-sgd; `inf` is the non-finite guard alone): the norm and the
   clipping coefficient are computed on the device in front of the update, a non-finite step is skipped;
   --ema DECAY: FusedSGD(ema=WeightEMA(net, DECAY)) (implies --fused-sgd): the weights are averaged inside the fused update and
   the JSON line (always printed) carries the average's device state (`ema_info`: updates, decay, applied);
   --deterministic: CTDET_TRAIN_DETERMINISTIC=1 for this run (ordered slab sums in place of the floating-point atomics of the
   convolutional training step; with --phase 2 level 2, which adds the Context-Transformer block's backward);
   after the timing line it prints `deterministic_repeat`: whether two runs of the same step from the same state gave the same
   gradient bits (every parameter of the network, at phase 2 the block's included), and with --fused-sgd under CTDET_LOSS_FUSED=1
   the same for the parameters after two steps (reported, not asserted);
   --loc-loss NAME, --loc-weight X: the criterion's localisation term (smooth_l1, iou, giou, diou, ciou; default: what CTDET_LOC_LOSS
   says, else smooth_l1) and the factor on loss_box_reg; both are reported on the JSON line, which is then always printed;
   --conf-loss NAME [--focal-gamma X --focal-alpha X]: the criterion's classification terms (ce, focal; default: what CTDET_CONF_LOSS
   says, else ce) and the focal constants (default: CTDET_FOCAL_GAMMA / CTDET_FOCAL_ALPHA, else 2.0 / 0.25); a focal run starts from
   focal_prior_init(net) (objectness prior 0.01); all three are reported on the JSON line, which is then always printed;
   --matcher NAME [--atss-topk K]: the criterion's target assignment (ssd, atss; default: what CTDET_MATCHER says, else ssd) and the
   ATSS candidates per level (default: CTDET_ATSS_TOPK, else 9); both are reported on the JSON line, which is then always printed;
   --matcher tal [--tal-topk K --tal-alpha A --tal-beta B]: task-aligned assignment from the step's own predictions (one more
   ct_detect_fused pass inside the loss time; defaults: CTDET_TAL_TOPK / _ALPHA / _BETA, else 13 / 1.0 / 6), reported likewise;
   --sync-bn: under torchrun, TrainRuntime.enable_bn_sync(): BatchNorm statistics over the global batch (two small all-reduces per
   BatchNorm stage and step); the JSON line (then always printed) carries `sync_bn`: the global batch, the
   stages and the collectives per step;
   --json: one more line, JSON, with the step time, the optimizer's device time and the training runtime's `policy` record
   (always with --clip-norm and --deterministic; with --clip-norm it
   also carries the last norm, coef and the number of skipped steps);
   --per-tensor-groups: the groups of utils/solver.py::build_optimizer (one per tensor) instead of a single group."""
import argparse, json, os, sys, time, types
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd')); sys.path.insert(0, REPO)
ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=300); ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--classes', type=int, default=None); ap.add_argument('--steps', type=int, default=5)
ap.add_argument('--sync', type=int, default=0)
ap.add_argument('--phase', type=int, default=1); ap.add_argument('--setting', default='transfer')
ap.add_argument('--fused-sgd', action='store_true'); ap.add_argument('--per-tensor-groups', action='store_true')
ap.add_argument('--wgrad-h2', action='store_true'); ap.add_argument('--deterministic', action='store_true')
ap.add_argument('--clip-norm', type=float, default=None); ap.add_argument('--json', action='store_true')
ap.add_argument('--ema', type=float, default=None); ap.add_argument('--optimizer', choices=('sgd', 'adamw'), default='sgd')
ap.add_argument('--loc-loss', default=None); ap.add_argument('--loc-weight', type=float, default=1.0)
ap.add_argument('--conf-loss', default=None); ap.add_argument('--focal-gamma', type=float, default=None)
ap.add_argument('--focal-alpha', type=float, default=None)
ap.add_argument('--matcher', default=None); ap.add_argument('--atss-topk', type=int, default=None)
ap.add_argument('--tal-topk', type=int, default=None); ap.add_argument('--tal-alpha', type=float, default=None)
ap.add_argument('--tal-beta', type=int, default=None)
ap.add_argument('--sync-bn', action='store_true')
a = ap.parse_args()
if a.clip_norm is not None or a.ema is not None:
    a.fused_sgd = True
if a.wgrad_h2:
    os.environ['CTDET_WGRAD_H2'] = '1'         # read once, when the TrainRuntime is built
if a.deterministic:
    os.environ['CTDET_TRAIN_DETERMINISTIC'] = '2' if a.phase == 2 else '1'      # the same; 2 = the Context-Transformer block too
from ctdet import synth, dist as cdist
from models.RFB_Net_vgg import build_net, _CTX_DIMS
from layers.functions import PriorBox
from layers.modules.multibox_loss_combined import MultiBoxLoss_combined, focal_prior_init
import data as cfgs
rank, local, world = cdist.init('nccl')
torch.cuda.set_device(local)
if a.classes is None:
    # phase 2: the width the Context-Transformer block's parameters are built for (60 base classes for 'transfer').  With any
    # other width the block's gradient tensors are only partly written, and their tails are whatever the allocator left there
    a.classes = _CTX_DIMS[a.setting][0] if a.phase == 2 else 20
net = build_net(types.SimpleNamespace(method='ours', phase=a.phase, setting=a.setting), a.size, a.classes)
net.load_state_dict(synth.fill_state_dict(net.state_dict()))
net = net.cuda().train(); net.device = 'cuda'
prior_box = PriorBox(getattr(cfgs, 'VOC_%d' % a.size))
priors = prior_box.forward().cuda()
nout = a.classes if a.phase == 1 else net.OBJ_Target.weight.shape[0] + (a.classes if a.setting == 'incre' else 0)
crit = MultiBoxLoss_combined(nout + 1, 0.5, True, 0, True, 3, 0.5, False, loc_loss=a.loc_loss, loc_weight=a.loc_weight,
                             conf_loss=a.conf_loss, focal_gamma=a.focal_gamma, focal_alpha=a.focal_alpha, matcher=a.matcher,
                             atss_topk=a.atss_topk, level_offsets=prior_box.level_offsets(), tal_topk=a.tal_topk,
                             tal_alpha=a.tal_alpha, tal_beta=a.tal_beta)
if crit.conf_loss == 'focal':
    focal_prior_init(net)       # every prior starts at objectness 0.01 instead of 0.5 (the biases; set before the runtime is built)
crit.sync_normalizer = world > 1
def make_opt():
    if a.per_tensor_groups:
        from utils import solver
        return solver.build_optimizer(types.SimpleNamespace(method='ours', phase=a.phase, lr=1e-4, momentum=0.9, weight_decay=5e-4,
                                                            max_grad_norm=a.clip_norm, ema_decay=a.ema, optimizer=a.optimizer),
                                      net, fused=a.fused_sgd or a.optimizer == 'adamw')
    if a.optimizer == 'adamw':
        from ctdet.optim import FusedAdamW, WeightEMA
        return FusedAdamW(net.parameters(), lr=1e-4, weight_decay=5e-4, max_grad_norm=a.clip_norm,
                          ema=None if a.ema is None else WeightEMA(net, a.ema))
    if a.fused_sgd:
        from ctdet.optim import FusedSGD, WeightEMA
        return FusedSGD(net.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4, max_grad_norm=a.clip_norm,
                        ema=None if a.ema is None else WeightEMA(net, a.ema))
    return torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4)
opt = make_opt()
x = synth.images(a.batch, a.size, 'randn', 1234 + rank).cuda()
tg = [t.cuda() for t in synth.targets(a.batch, nout + 1, 99 + rank)]
trt = net.train_runtime(a.batch)
if a.sync or world > 1:
    trt.enable_grad_sync()
if a.sync_bn:
    trt.enable_bn_sync()                        # a no-op for one rank; CTDET_SYNC_BN=1 has enable_grad_sync() do the same
def step():
    opt.zero_grad(set_to_none=True)
    out = net(x)
    ld = crit(out, priors, tg)
    loss = sum(ld.values())
    loss.backward()
    opt.step()
    return loss
for _ in range(2):
    l = step()
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
tf = tl = tb = to = 0.0
cdist.barrier('cuda')
t0 = time.perf_counter()
for _ in range(a.steps):
    opt.zero_grad(set_to_none=True)
    ev[0].record(); out = net(x); ev[1].record()
    ld = crit(out, priors, tg); loss = sum(ld.values()); ev[2].record()
    loss.backward(); ev[3].record()
    opt.step(); ev[4].record()
    torch.cuda.synchronize()
    to += ev[3].elapsed_time(ev[4])
    tf += ev[0].elapsed_time(ev[1]); tl += ev[1].elapsed_time(ev[2]); tb += ev[2].elapsed_time(ev[3])
cdist.barrier('cuda')
dt = cdist.max_over_ranks((time.perf_counter() - t0) / a.steps, 'cuda')
if rank == 0:
    n = a.steps
    print('RFBNet-%d phase %d bs=%d x %d GPU(s)%s: %.1f ms/step = %.1f img/s | fwd %.1f  loss %.1f  bwd %.1f ms | loss %.4f'
          % (a.size, a.phase, a.batch, world, ' [%s, %d groups]' % (type(opt).__name__, len(opt.param_groups))
             if a.fused_sgd or a.per_tensor_groups or a.optimizer != 'sgd' else '', dt * 1e3, a.batch * world / dt, tf / n, tl / n, tb / n, float(loss)))
    if a.json or a.clip_norm is not None or a.ema is not None or a.deterministic or a.loc_loss is not None or a.loc_weight != 1.0 \
            or a.conf_loss is not None or a.matcher is not None or a.optimizer != 'sgd' or a.sync_bn:
        row = {'train_bench': 'RFBNet-%d phase %d' % (a.size, a.phase), 'batch': a.batch, 'gpus': world, 'steps': n,
               'optimizer': type(opt).__name__, 'groups': len(opt.param_groups), 'ms_per_step': round(dt * 1e3, 3),
               'fwd_ms': round(tf / n, 3), 'loss_ms': round(tl / n, 3), 'bwd_ms': round(tb / n, 3), 'opt_ms': round(to / n, 3),
               'clip_norm': a.clip_norm, 'loss': float(loss), 'loc_loss': crit.loc_loss, 'loc_weight': crit.loc_weight,
               'loss_fused': crit.fused, 'conf_loss': crit.conf_loss, 'focal_gamma': crit.focal_gamma,
               'focal_alpha': crit.focal_alpha, 'matcher': crit.matcher, 'atss_topk': crit.atss_topk, 'tal_topk': crit.tal_topk,
               'tal_alpha': crit.tal_alpha, 'tal_beta': crit.tal_beta}
        if a.clip_norm is not None:
            row.update(opt.clip_info())                 # norm, coef, finite, nonfinite of the last step
        if a.ema is not None:
            row.update(ema_decay=a.ema, ema_info=opt.ema.info())
        if trt.bn_sync is not None:
            sy = trt.bn_sync
            row['sync_bn'] = {'global_batch': sy.global_batch, 'stages': len(sy.stages),
                              'collectives_per_step': sy.collectives / float(n + 2)}
        row['policy'] = trt.policy_record()             # deterministic: true / false, the weight-gradient routes
        print(json.dumps(row))
if a.deterministic:
    # two runs of the same step from the same state: parameters, BatchNorm buffers and a fresh optimizer each time
    state0 = {k: v.clone() for k, v in net.state_dict().items()}
    def rerun(steps):
        global opt
        net.load_state_dict(state0)
        opt = make_opt()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return [None if p.grad is None else p.grad.clone() for p in net.parameters()], [p.detach().clone() for p in net.parameters()]
    def same(u, v):
        return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(u, v))
    (g1, _), (g2, _) = rerun(1), rerun(1)
    rep = {'deterministic_repeat': same(g1, g2)}
    if a.fused_sgd and os.environ.get('CTDET_LOSS_FUSED', '0') not in ('', '0'):
        (_, p1), (_, p2) = rerun(2), rerun(2)
        rep['deterministic_repeat_params_2_steps'] = same(p1, p2)
    if rank == 0:
        print(json.dumps(rep))
