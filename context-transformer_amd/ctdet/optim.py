"""FusedSGD: torch.optim.SGD's interface over the fused multi-tensor HIP update (ct_sgd_step, csrc/ct_optim.hip).

Drop-in for the optimizer utils/solver.py:6-33 builds (one parameter group per tensor, per-name learning rates that
WarmupMultiStepLR rewrites every iteration): `param_groups`, `state[p]['momentum_buffer']` and `state_dict()` have
torch's layout, so checkpoints move between the two classes in both directions.  One ct_sgd_step call per distinct
(momentum, dampening, nesterov) among the groups -- one for the reference's layout -- instead of three foreach
launches per group.  There is no CPU path: a parameter that is not contiguous fp32 on the HIP device is an error.
"""
import torch

from . import ops
from ._lib import CtdetError


def _check_group(momentum, dampening, weight_decay, nesterov, lr):
    if lr < 0.0:
        raise ValueError('Invalid learning rate: {}'.format(lr))
    if momentum < 0.0:
        raise ValueError('Invalid momentum value: {}'.format(momentum))
    if weight_decay < 0.0:
        raise ValueError('Invalid weight_decay value: {}'.format(weight_decay))
    if nesterov and (momentum <= 0 or dampening != 0):
        raise ValueError('Nesterov momentum requires a momentum and zero dampening')


class FusedSGD(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *,
                 maximize=False, foreach=None, differentiable=False, fused=None):
        if isinstance(lr, torch.Tensor) or isinstance(weight_decay, torch.Tensor):
            raise ValueError('FusedSGD takes lr and weight_decay as Python floats')
        if maximize or foreach or fused or differentiable:
            raise ValueError('FusedSGD implements maximize=False, foreach=None, fused=None, differentiable=False only')
        _check_group(momentum, dampening, weight_decay, nesterov, lr)
        # the off-valued torch keys are kept so that a state_dict() loads into torch.optim.SGD as it stands
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults)
        self.grad_scale = 1.0
        self.last_calls = 0         # ct_sgd_step calls of the last step() (one per distinct momentum triple)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault('grad_scale', 1.0)
        self.__dict__.setdefault('last_calls', 0)
        for group in self.param_groups:
            for key, off in (('nesterov', False), ('maximize', False), ('foreach', None), ('differentiable', False),
                             ('fused', None)):
                group.setdefault(key, off)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        calls = {}                  # (momentum, dampening, nesterov) -> items of ops.sgd_step, in group order
        touched = []
        for group in self.param_groups:
            if group.get('maximize') or group.get('foreach') or group.get('fused') or group.get('differentiable'):
                raise ValueError('FusedSGD: a parameter group asks for maximize / foreach / fused / differentiable')
            momentum, dampening, nesterov = group['momentum'], group['dampening'], group['nesterov']
            lr, wd = group['lr'], group['weight_decay']
            _check_group(momentum, dampening, wd, nesterov, lr)
            items = None
            for p in group['params']:
                grad = p.grad
                if grad is None:
                    continue
                if grad.is_sparse:
                    raise CtdetError('FusedSGD does not take sparse gradients')
                if items is None:
                    items = calls.setdefault((float(momentum), float(dampening), bool(nesterov)), [])
                buf, first = None, False
                if momentum != 0:
                    state = self.state[p]
                    buf = state.get('momentum_buffer')
                    if buf is None:
                        if not p.is_cuda:       # before the allocation, so that the error names the parameter
                            raise CtdetError('FusedSGD: parameter on %s; the fused update has no CPU fallback'
                                             % p.device)
                        buf = torch.empty_like(p, memory_format=torch.contiguous_format)
                        first = True
                    touched.append(buf)
                touched.append(p)
                items.append((p, grad, buf, lr, wd, first))
        for (momentum, dampening, nesterov), items in calls.items():
            ops.sgd_step(items, momentum, dampening, nesterov, self.grad_scale)
            for p, _, buf, _, _, first in items:
                if first:                       # only a buffer the kernel has filled becomes state
                    self.state[p]['momentum_buffer'] = buf
        self.last_calls = len(calls)
        # The kernel writes through raw pointers; the weight caches (HipBackend.param_versions, the `scale` read of
        # models/RFB_Net_vgg.py) are keyed on tensor._version, so the update has to show there.
        if touched:
            torch.autograd.graph.increment_version(touched)
        return loss
