"""FusedSGD: torch.optim.SGD's interface over the fused multi-tensor HIP update (ct_sgd_step, csrc/ct_optim.hip).

Drop-in for the optimizer utils/solver.py:6-33 builds (one parameter group per tensor, per-name learning rates that
WarmupMultiStepLR rewrites every iteration): `param_groups`, `state[p]['momentum_buffer']` and `state_dict()` have
torch's layout, so checkpoints move between the two classes in both directions.  One ct_sgd_step call per distinct
(momentum, dampening, nesterov) among the groups -- one for the reference's layout -- instead of three foreach
launches per group.  There is no CPU path: a parameter that is not contiguous fp32 on the HIP device is an error.

max_grad_norm (None = off; a positive float, or math.inf for the non-finite guard alone) puts ONE ct_grad_norm_clip over
the gradients of all groups in front of those calls: torch.nn.utils.clip_grad_norm_'s coefficient is computed on the
device and multiplied into grad_scale there, and a step whose norm is not finite is skipped -- no pass that rewrites the
gradients, no host synchronisation.  clip_info() reads the last norm / coef / skip count back for logging.
"""
import math

import torch

from . import ops
from ._lib import CtdetError


def _check_max_grad_norm(v):
    if v is None:
        return None
    if isinstance(v, torch.Tensor) or isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError('FusedSGD takes max_grad_norm as a Python float or None')
    v = float(v)
    if math.isnan(v) or v <= 0.0:
        raise ValueError('Invalid max_grad_norm: {} (a positive float, math.inf for the guard alone, or None)'.format(v))
    return v


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
                 maximize=False, foreach=None, differentiable=False, fused=None, max_grad_norm=None):
        if isinstance(lr, torch.Tensor) or isinstance(weight_decay, torch.Tensor):
            raise ValueError('FusedSGD takes lr and weight_decay as Python floats')
        if maximize or foreach or fused or differentiable:
            raise ValueError('FusedSGD implements maximize=False, foreach=None, fused=None, differentiable=False only')
        _check_group(momentum, dampening, weight_decay, nesterov, lr)
        max_grad_norm = _check_max_grad_norm(max_grad_norm)
        # the off-valued torch keys are kept so that a state_dict() loads into torch.optim.SGD as it stands
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults)
        self.grad_scale = 1.0
        self.last_calls = 0         # ct_sgd_step calls of the last step() (one per distinct momentum triple)
        # an attribute, not a group key: state_dict() keeps torch's layout
        self.max_grad_norm = max_grad_norm
        self.clip_state = None      # 16-byte device tensor (ct_clip_state), allocated zeroed by the first clipped step
        self._clip_workspace = None

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault('grad_scale', 1.0)
        self.__dict__.setdefault('last_calls', 0)
        self.__dict__.setdefault('max_grad_norm', None)
        self.__dict__.setdefault('clip_state', None)
        self.__dict__.setdefault('_clip_workspace', None)
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
        max_norm = _check_max_grad_norm(self.max_grad_norm)     # the attribute may have been set since __init__
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
        clip = None
        if max_norm is not None and calls:
            clip = self._grad_norm_clip([it[1] for items in calls.values() for it in items], max_norm)
        for (momentum, dampening, nesterov), items in calls.items():
            ops.sgd_step(items, momentum, dampening, nesterov, self.grad_scale, clip_state=clip)
            for p, _, buf, _, _, first in items:
                if first:                       # only a buffer the kernel has filled becomes state
                    self.state[p]['momentum_buffer'] = buf
        self.last_calls = len(calls)
        # The kernel writes through raw pointers; the weight caches (HipBackend.param_versions, the `scale` read of
        # models/RFB_Net_vgg.py) are keyed on tensor._version, so the update has to show there.
        if touched:
            torch.autograd.graph.increment_version(touched)
        return loss

    def _grad_norm_clip(self, grads, max_norm):
        """One ct_grad_norm_clip over `grads` into the optimizer's own state and workspace tensors."""
        dev = grads[0].device
        if not grads[0].is_cuda:
            raise CtdetError('FusedSGD: gradient on %s; the fused update has no CPU fallback' % dev)
        if self.clip_state is None or self.clip_state.device != dev:
            self.clip_state = torch.zeros(ops.CLIP_STATE_BYTES, device=dev, dtype=torch.uint8)
        table = ops.grad_table(grads)
        need = ops.grad_norm_workspace_bytes(grads, table)
        if self._clip_workspace is None or self._clip_workspace.numel() < need or self._clip_workspace.device != dev:
            self._clip_workspace = torch.empty(max(need, 8), device=dev, dtype=torch.uint8)
        return ops.grad_norm_clip(grads, max_norm, self.grad_scale, self.clip_state, self._clip_workspace, table)

    def clip_info(self):
        """{'norm', 'coef', 'finite', 'nonfinite'} of the last clipped step; synchronises, so call it every N
        iterations for logging, not every step.  None before the first clipped step."""
        return None if self.clip_state is None else ops.clip_info(self.clip_state)
