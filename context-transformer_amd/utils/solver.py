"""Optimizer / LR-schedule glue with the reference's entry points (utils/solver.py).

build_optimizer (:6-33): SGD with one parameter group per tensor; in phase 2 with method 'ours'
the groups are scaled by NAME — `base` in the key: lr x 0.1; `extras` or `Norm`: lr x 0.5 —
which is why the state-dict prefixes are part of the contract.  WarmupMultiStepLR (:49-111):
lr = base_lr * warmup(iter) * gamma ** (#milestones <= iter), linear warmup from `warmup_factor`.

build_optimizer(..., fused=True), or CTDET_SGD_FUSED=1 in the environment, returns ctdet.optim.FusedSGD over the same
groups: the whole update in one multi-tensor HIP call instead of three foreach launches per group.  Off by default.
args.max_grad_norm (optional; a positive float, or math.inf for the non-finite guard alone) is FusedSGD's max_grad_norm:
gradient-norm clipping and the skip of non-finite steps on the device.  Only the fused optimizer has it.
args.ema_decay (optional, with args.ema_warmup) attaches a ctdet.optim.WeightEMA of the model as `optimizer.ema`: the
weights are averaged inside the fused update; evaluate under `with optimizer.ema.swapped():`.  Fused only as well.
args.optimizer (optional; 'sgd' when absent) = 'adamw' builds AdamW over the same per-tensor groups, with args.betas and
args.eps when given: ctdet.optim.FusedAdamW when fused, torch.optim.AdamW otherwise; max_grad_norm and ema_decay need
the fused class here too.  Any other name is an error.
"""
import os
from bisect import bisect_right

import torch


def lr_multiplier(args, key):
    if args.phase == 2 and args.method == 'ours':
        if 'base' in key:
            return 0.1
        if 'extras' in key or 'Norm' in key:
            return 0.5
    return 1.0


def build_optimizer(args, model, fused=None):
    groups = [{'params': [p], 'lr': args.lr * lr_multiplier(args, name), 'weight_decay': args.weight_decay}
              for name, p in model.named_parameters() if p.requires_grad]
    if fused is None:
        fused = os.environ.get('CTDET_SGD_FUSED', '0') == '1'
    max_grad_norm = getattr(args, 'max_grad_norm', None)
    ema_decay = getattr(args, 'ema_decay', None)
    name = getattr(args, 'optimizer', 'sgd')
    if name == 'adamw':
        return _build_adamw(args, model, groups, fused, max_grad_norm, ema_decay)
    if name != 'sgd':
        raise ValueError("args.optimizer = %r: 'sgd' or 'adamw'" % (name,))
    if ema_decay is not None:
        if not fused:
            raise ValueError('args.ema_decay = %r needs the fused optimizer (fused=True or CTDET_SGD_FUSED=1): with '
                             'torch.optim.SGD call ctdet.optim.WeightEMA(model).update() after step()' % (ema_decay,))
        from ctdet.optim import FusedSGD, WeightEMA
        warmup = getattr(args, 'ema_warmup', None)
        ema = WeightEMA(model, ema_decay) if warmup is None else WeightEMA(model, ema_decay, warmup)
        return FusedSGD(groups, args.lr, momentum=args.momentum, max_grad_norm=max_grad_norm, ema=ema)
    if fused:
        from ctdet.optim import FusedSGD
        if max_grad_norm is None:
            return FusedSGD(groups, args.lr, momentum=args.momentum)
        return FusedSGD(groups, args.lr, momentum=args.momentum, max_grad_norm=max_grad_norm)
    if max_grad_norm is not None:
        raise ValueError('args.max_grad_norm = %r needs the fused optimizer (fused=True or CTDET_SGD_FUSED=1): there is '
                         'no torch path for it' % (max_grad_norm,))
    return torch.optim.SGD(groups, args.lr, momentum=args.momentum)


def _build_adamw(args, model, groups, fused, max_grad_norm, ema_decay):
    """args.optimizer == 'adamw': ctdet.optim.FusedAdamW when fused, else torch.optim.AdamW, over the same groups."""
    kw = {}
    if getattr(args, 'betas', None) is not None:
        kw['betas'] = tuple(args.betas)
    if getattr(args, 'eps', None) is not None:
        kw['eps'] = args.eps
    if not fused:
        for name, v in (('max_grad_norm', max_grad_norm), ('ema_decay', ema_decay)):
            if v is not None:
                raise ValueError('args.%s = %r needs the fused optimizer (fused=True or CTDET_SGD_FUSED=1): there is no '
                                 'torch path for it' % (name, v))
        return torch.optim.AdamW(groups, args.lr, **kw)
    from ctdet.optim import FusedAdamW, WeightEMA
    if max_grad_norm is not None:
        kw['max_grad_norm'] = max_grad_norm
    if ema_decay is not None:
        warmup = getattr(args, 'ema_warmup', None)
        kw['ema'] = WeightEMA(model, ema_decay) if warmup is None else WeightEMA(model, ema_decay, warmup)
    return FusedAdamW(groups, args.lr, **kw)


def _get_warmup_factor_at_iter(method, iter, warmup_iters, warmup_factor):
    if iter >= warmup_iters:
        return 1.0
    if method == 'constant':
        return warmup_factor
    if method == 'linear':
        alpha = iter / warmup_iters
        return warmup_factor * (1 - alpha) + alpha
    raise ValueError('Unknown warmup method: {}'.format(method))


class WarmupMultiStepLR(torch.optim.lr_scheduler._LRScheduler):
    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=1e-6, warmup_iters=1000,
                 warmup_method='linear', last_epoch=-1):
        if list(milestones) != sorted(milestones):
            raise ValueError('Milestones should be a list of increasing integers. Got {}'.format(milestones))
        self.milestones, self.gamma = milestones, gamma
        self.warmup_factor, self.warmup_iters, self.warmup_method = warmup_factor, warmup_iters, warmup_method
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        w = _get_warmup_factor_at_iter(self.warmup_method, self.last_epoch, self.warmup_iters, self.warmup_factor)
        decay = self.gamma ** bisect_right(self.milestones, self.last_epoch)
        return [base * w * decay for base in self.base_lrs]

    def _compute_values(self):
        return self.get_lr()


def build_lr_scheduler(args, optimizer):
    return WarmupMultiStepLR(optimizer, args.steps, warmup_iters=args.warmup_iter)
