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

WeightEMA keeps an exponential moving average of a model's weights on the device; FusedSGD(ema=...) or attach_ema()
updates it inside the same pass (ct_sgd_step_ema replaces ct_sgd_step call for call, plus one ct_ema_begin and one
ct_ema_update for what the optimizer does not touch), and a step the guard skips leaves the average and its warm-up
count alone.  Like max_grad_norm it is an attribute, not a group key.

FusedAdamW is torch.optim.AdamW's interface over ct_adamw_begin + ct_adamw_step (csrc/ct_adamw.hip) with the same
grad_scale, max_grad_norm, clip_info() and attach_ema(); what the two classes share lives in _FusedOptimizer.
"""
import contextlib
import math

import numpy as np
import torch

from . import ops
from ._lib import CtdetError
from ._lib import EmaState as _EmaState


def _check_max_grad_norm(v, who='FusedSGD'):
    if v is None:
        return None
    if isinstance(v, torch.Tensor) or isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError('%s takes max_grad_norm as a Python float or None' % who)
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


class _FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share around their update call: grad_scale, the gradient-norm clip with its device state
    and workspace, the attached weight average, and the version counters of everything a step wrote.  All of it lives
    in attributes, not group keys, so state_dict() keeps torch's layout."""

    def _init_fused(self, max_grad_norm, ema):
        self.grad_scale = 1.0
        self.last_calls = 0         # update calls of the last step() (one per distinct set of call-wide hyperparameters)
        # an attribute, not a group key: state_dict() keeps torch's layout
        self.max_grad_norm = max_grad_norm
        self.clip_state = None      # 16-byte device tensor (ct_clip_state), allocated zeroed by the first clipped step
        self._clip_workspace = None
        self.ema = None             # a WeightEMA averaged inside the update (attach_ema); an attribute as well
        if ema is not None:
            self.attach_ema(ema)

    def _setstate_fused(self):
        self.__dict__.setdefault('grad_scale', 1.0)
        self.__dict__.setdefault('last_calls', 0)
        self.__dict__.setdefault('max_grad_norm', None)
        self.__dict__.setdefault('clip_state', None)
        self.__dict__.setdefault('_clip_workspace', None)
        self.__dict__.setdefault('ema', None)

    def _begin_ema(self, clip):
        """Opens one update of the attached average, skipped on the device with the step -> (ema, set of the shadows the
        update calls are about to move), or (None, None)."""
        ema = self.ema
        if ema is None:
            return None, None
        ops.ema_begin(ema.state, ema.decay, ema.warmup, clip_state=clip)
        return ema, set()

    def _finish(self, ema, averaged, touched):
        """The shadows the update calls did not move (parameters without a gradient this step, and the buffers), then the
        version counters."""
        if ema is not None:
            ops.ema_update([(sh, live) for sh, live in ema.pairs() if id(sh) not in averaged], ema.state)
            touched += ema.shadows()
        # The kernel writes through raw pointers; the weight caches (HipBackend.param_versions, the `scale` read of
        # models/RFB_Net_vgg.py) are keyed on tensor._version, so the update has to show there.
        if touched:
            torch.autograd.graph.increment_version(touched)

    def _grad_norm_clip(self, grads, max_norm):
        """One ct_grad_norm_clip over `grads` into the optimizer's own state and workspace tensors."""
        dev = grads[0].device
        if not grads[0].is_cuda:
            raise CtdetError('%s: gradient on %s; the fused update has no CPU fallback' % (type(self).__name__, dev))
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

    def attach_ema(self, ema):
        """Average the weights in the pass that updates them: `ema` (a WeightEMA, or None to detach) must hold a shadow
        for every parameter of every group.  step() then opens one update on the device (skipped with the step when
        max_grad_norm's guard skips it), moves the shadows of the parameters it updates inside the update call itself
        (ct_sgd_step_ema, ct_adamw_step) and the remaining ones (no gradient this step, buffers) with one ct_ema_update."""
        who = type(self).__name__
        if ema is not None:
            if not isinstance(ema, WeightEMA):
                raise TypeError('%s.attach_ema takes a ctdet.optim.WeightEMA, got %s' % (who, type(ema).__name__))
            for gi, group in enumerate(self.param_groups):
                for pi, p in enumerate(group['params']):
                    if ema.shadow_of(p) is None:
                        raise ValueError('%s.attach_ema: parameter %d of group %d (shape %s) has no shadow in the '
                                         'WeightEMA' % (who, pi, gi, tuple(p.shape)))
        self.ema = ema
        return self


class FusedSGD(_FusedOptimizer):
    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *,
                 maximize=False, foreach=None, differentiable=False, fused=None, max_grad_norm=None, ema=None):
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
        self._init_fused(max_grad_norm, ema)    # last_calls: ct_sgd_step calls, one per distinct momentum triple

    def __setstate__(self, state):
        super().__setstate__(state)
        self._setstate_fused()
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
        ema, averaged = self._begin_ema(clip)    # one update of the average, skipped on the device with the step
        for (momentum, dampening, nesterov), items in calls.items():
            if ema is None:
                ops.sgd_step(items, momentum, dampening, nesterov, self.grad_scale, clip_state=clip)
            else:
                items_ema = [it + (ema.shadow_of(it[0], required=True),) for it in items]
                averaged.update(id(it[6]) for it in items_ema)
                ops.sgd_step_ema(items_ema, momentum, dampening, nesterov, self.grad_scale, ema.state, clip_state=clip)
            for p, _, buf, _, _, first in items:
                if first:                       # only a buffer the kernel has filled becomes state
                    self.state[p]['momentum_buffer'] = buf
        self.last_calls = len(calls)
        self._finish(ema, averaged, touched)
        return loss


_ADAMW_OFF = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)


def _adamw_defaults():
    """The group keys of the installed torch's AdamW with their off values, in torch's order (newer versions add keys,
    e.g. decoupled_weight_decay), so that a state_dict() loads into torch.optim.AdamW as it stands."""
    return dict(torch.optim.AdamW([torch.zeros(1)]).defaults)


def _check_adamw_group(lr, betas, eps, weight_decay):
    if any(isinstance(v, torch.Tensor) for v in (lr, eps, weight_decay) + tuple(betas)):
        raise ValueError('FusedAdamW takes lr, betas, eps and weight_decay as Python floats')
    if not 0.0 <= lr:
        raise ValueError('Invalid learning rate: {}'.format(lr))
    if not 0.0 <= eps:
        raise ValueError('Invalid epsilon value: {}'.format(eps))
    for i in (0, 1):
        if not 0.0 <= betas[i] < 1.0:
            raise ValueError('Invalid beta parameter at index {}: {}'.format(i, betas[i]))
    if not 0.0 <= weight_decay:
        raise ValueError('Invalid weight_decay value: {}'.format(weight_decay))


def _as_f32(beta):
    """The value ct_adamw_step's recurrence runs with (its betas are fp32), as a Python double for ct_adamw_begin: the
    bias corrections then belong to the same beta as the moments.  With the unrounded 0.999 there, 1 - beta2 (0.001) and
    the recurrence's 1 - fp32(0.999) would differ by 1.3e-5 of their value, which is 6e-6 of every early update."""
    return float(np.float32(beta))


def _check_adamw_off(keys, who):
    """torch's other AdamW keywords: accepted at their off values only."""
    bad = [k for k in _ADAMW_OFF if keys.get(k)]
    if not keys.get('decoupled_weight_decay', True):
        bad.append('decoupled_weight_decay=False')
    if bad:
        raise ValueError('%s implements amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, '
                         'fused=None and decoupled weight decay only (got %s)' % (who, ', '.join(bad)))


class FusedAdamW(_FusedOptimizer):
    """torch.optim.AdamW's interface (amsgrad=False, maximize=False) over the fused multi-tensor HIP update
    (ct_adamw_begin + ct_adamw_step, csrc/ct_adamw.hip): one pair of calls per distinct (beta1, beta2, eps) among the
    groups.  grad_scale, max_grad_norm, clip_info() and attach_ema() are FusedSGD's.

    The step count of every parameter lives on the device, in one optimizer-owned buffer of 32-byte records
    (ct_adam_state, one slot per parameter): a step the non-finite guard skips does not count, without a host
    synchronisation, and a captured step() replays as a real step.  state[p] holds exp_avg and exp_avg_sq in torch's
    layout; state[p]['step'] is refreshed from the records by state_dict() (one device-to-host copy) and is otherwise as
    old as the last state_dict() or load_state_dict().  Checkpoints move between this class and torch.optim.AdamW in
    both directions; loading sets the records' beta powers to beta ** step in Python double, with beta the fp32 value
    the update runs with (_as_f32).

    The one departure from torch: changing a group's betas after one of its tensors has taken part in a step is a
    ValueError, because the running products beta^step belong to the old betas.  There is no CPU path: a parameter that
    is not contiguous fp32 on the HIP device is an error, and so is a sparse gradient."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, amsgrad=False, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, max_grad_norm=None, ema=None):
        _check_adamw_off(dict(amsgrad=amsgrad, maximize=maximize, foreach=foreach, capturable=capturable,
                              differentiable=differentiable, fused=fused), 'FusedAdamW')
        _check_adamw_group(lr, betas, eps, weight_decay)
        max_grad_norm = _check_max_grad_norm(max_grad_norm, 'FusedAdamW')
        defaults = _adamw_defaults()
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._init_fused(max_grad_norm, ema)    # last_calls: ct_adamw_step calls, one per distinct (beta1, beta2, eps)
        self._init_records()

    def _init_records(self):
        self._slots = {}            # id(parameter) -> its record's position in the buffer, in order of first use
        self._records = None        # uint8 device tensor, ops.ADAM_STATE_BYTES per slot
        self._pending = {}          # slot -> step count load_state_dict() read, not yet on the device
        self._betas_of = {}         # slot -> the (beta1, beta2) its running products were built from

    def __setstate__(self, state):
        super().__setstate__(state)
        self._setstate_fused()
        for group in self.param_groups:
            for key, off in _adamw_defaults().items():
                group.setdefault(key, off)
        if '_slots' not in self.__dict__:       # unpickled: the records are rebuilt from the step counts
            self._adopt_steps('FusedAdamW')

    def _slot(self, p):
        return self._slots.setdefault(id(p), len(self._slots))

    def _records_for(self, device):
        """The record buffer with a slot for every parameter seen so far, and what load_state_dict() left for it."""
        need = len(self._slots) * ops.ADAM_STATE_BYTES
        if self._records is None or self._records.numel() < need or self._records.device != device:
            grown = torch.zeros(max(need, ops.ADAM_STATE_BYTES), device=device, dtype=torch.uint8)
            if self._records is not None:
                grown[:self._records.numel()].copy_(self._records)
            self._records = grown
        if self._pending:           # only ever in front of the first step after a load: the buffer is new and all zero
            host = np.zeros(self._records.numel() // ops.ADAM_STATE_BYTES, ops.ADAM_STATE_DTYPE)
            for slot, step in self._pending.items():
                if step:
                    b1, b2 = (_as_f32(b) for b in self._betas_of[slot])
                    b1p, b2p = b1 ** step, b2 ** step           # Python doubles
                    host[slot] = (b1p, b2p, step, 0, np.float32(1.0 - b1p), np.sqrt(np.float32(1.0 - b2p)))
            ops.adam_states_write(self._records, host)
            self._pending = {}
        return self._records

    def _steps(self):
        """slot -> applied steps, from the device records (one device-to-host copy) and what is still pending."""
        steps = {}
        if self._records is not None:
            steps.update(enumerate(int(s) for s in ops.adam_states_read(self._records)['step']))
        steps.update(self._pending)
        return steps

    def _refresh_steps(self):
        """state[p]['step'] of every parameter that has state, as torch keeps it (a float32 scalar on the host)."""
        steps = self._steps()
        for group in self.param_groups:
            for p in group['params']:
                if p in self.state:
                    self.state[p]['step'] = torch.tensor(float(steps.get(self._slots.get(id(p)), 0)))

    def state_dict(self):
        self._refresh_steps()
        return super().state_dict()

    def __getstate__(self):         # pickling and deepcopy carry the step counts the way a checkpoint does
        self._refresh_steps()
        return super().__getstate__()

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._adopt_steps('FusedAdamW.load_state_dict')

    def _adopt_steps(self, who):
        """New records from state[p]['step']: beta*_pow = beta ** step, written to the device by the next step()."""
        self._init_records()
        for group in self.param_groups:
            _check_adamw_off(group, who)
            betas = (float(group['betas'][0]), float(group['betas'][1]))
            for p in group['params']:
                slot = self._slot(p)
                state = self.state.get(p)
                if not state:
                    continue
                step = int(round(float(state['step'])))
                if not 0 <= step <= 2 ** 31 - 1:
                    raise ValueError('%s: invalid step count %r' % (who, state['step']))
                state['step'] = torch.tensor(float(step))
                self._pending[slot] = step
                if step:
                    self._betas_of[slot] = betas

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        max_norm = _check_max_grad_norm(self.max_grad_norm, 'FusedAdamW')
        calls = {}                  # (beta1, beta2, eps) -> items of ops.adamw_step, in group order
        touched = []
        for group in self.param_groups:
            _check_adamw_off(group, 'FusedAdamW: a parameter group')
            lr, betas, eps, wd = group['lr'], group['betas'], group['eps'], group['weight_decay']
            _check_adamw_group(lr, betas, eps, wd)
            betas = (float(betas[0]), float(betas[1]))
            items = None
            for p in group['params']:
                slot = self._slot(p)                            # every parameter, so the slots follow the group order
                grad = p.grad
                if grad is None:
                    continue
                if grad.is_sparse:
                    raise CtdetError('FusedAdamW does not take sparse gradients')
                if self._betas_of.get(slot, betas) != betas:
                    raise ValueError('FusedAdamW: betas changed from %s to %s after a step; the running products beta^step on '
                                     'the device belong to the old ones' % (self._betas_of[slot], betas))
                state = self.state.get(p)
                if not state:
                    if not p.is_cuda:           # before the allocation, so that the error names the parameter
                        raise CtdetError('FusedAdamW: parameter on %s; the fused update has no CPU fallback' % p.device)
                    state = self.state[p]
                    state['step'] = torch.tensor(0.0)
                    state['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if items is None:
                    items = calls.setdefault(betas + (float(eps),), [])
                self._betas_of[slot] = betas
                touched += [p, state['exp_avg'], state['exp_avg_sq']]
                items.append((p, grad, state['exp_avg'], state['exp_avg_sq'], slot, lr, wd))
        clip = None
        if max_norm is not None and calls:
            clip = self._grad_norm_clip([it[1] for items in calls.values() for it in items], max_norm)
        ema, averaged = self._begin_ema(clip)    # one update of the average, skipped on the device with the step
        for (beta1, beta2, eps), items in calls.items():
            if not items[0][0].is_cuda:
                raise CtdetError('FusedAdamW: parameter on %s; the fused update has no CPU fallback' % items[0][0].device)
            records = self._records_for(items[0][0].device)
            if ema is not None:
                items = [it + (ema.shadow_of(it[0], required=True),) for it in items]
                averaged.update(id(it[7]) for it in items)
            ops.adamw_begin(records, [it[4] for it in items], _as_f32(beta1), _as_f32(beta2), clip_state=clip)
            ops.adamw_step(items, beta1, beta2, eps, self.grad_scale, records, ema_state=None if ema is None else ema.state,
                           clip_state=clip)
        self.last_calls = len(calls)
        self._finish(ema, averaged, touched)
        return loss


def _check_ema(decay, warmup):
    for name, v in (('decay', decay), ('warmup', warmup)):
        if isinstance(v, torch.Tensor) or isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError('WeightEMA takes %s as a Python float' % name)
    decay, warmup = float(decay), float(warmup)
    if not 0.0 <= decay < 1.0:                      # NaN fails both comparisons
        raise ValueError('Invalid EMA decay: {} (0 <= decay < 1)'.format(decay))
    if not (warmup == 0.0 or 1.0 <= warmup < math.inf):
        raise ValueError('Invalid EMA warmup: {} (0 for a constant decay, or a finite value >= 1)'.format(warmup))
    return decay, warmup


class WeightEMA:
    """Exponential moving average of a model's weights, kept on the device (csrc/ct_ema.hip).

    One contiguous fp32 shadow per named parameter -- and, with buffers=True, per floating-point named buffer, i.e. the
    BatchNorm running statistics but not num_batches_tracked -- initialised to the tensor's value.  Every update is
        d      = min(decay, (1 + n) / (warmup + n))       n = updates so far; warmup = 0: d = decay
        shadow = d * shadow + (1 - d) * weight
    in fp32, one rounding per operation (include/ctdet.h).  n, d and the decision whether a step counts live in a
    16-byte device tensor (`state`), so nothing here synchronises except info() and state_dict().

    Two ways to drive it: FusedSGD.attach_ema(ema) averages inside the optimizer's own pass and skips the update when
    the non-finite guard skips the step; update() after any other optimizer's step() does one pass over everything.

    `with ema.swapped():` exchanges weights and shadows in place for the duration of the block and bumps the version
    counters of both, so the runtimes re-pack from the same tensors and a captured DetectionPipeline graph stays valid;
    on exit they are exchanged back.  Whatever the block writes into the model in place is therefore written into the
    averaged values and ends up in the shadows: net.normalize() inside the block normalises the AVERAGED weights and
    they stay normalised in the shadows, the live weights are not touched by it; call it before entering for those.
    There is no CPU path: a model that is not on the HIP device is an error."""

    def __init__(self, model, decay=0.9998, warmup=10.0, buffers=True):
        self.decay, self.warmup = _check_ema(decay, warmup)
        named = [(n, p) for n, p in model.named_parameters()]
        if buffers:
            named += [(n, b) for n, b in model.named_buffers() if b.is_floating_point()]
        if not named:
            raise ValueError('WeightEMA: the model has no parameters')
        self._live = {}
        self.shadow = {}
        for name, t in named:
            if not t.is_cuda:
                raise CtdetError('WeightEMA: %s is on %s; the average is kept on the HIP device and has no CPU path'
                                 % (name, t.device))
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise CtdetError('WeightEMA: %s must be contiguous float32, got %s' % (name, t.dtype))
            self._live[name] = t
            self.shadow[name] = t.detach().clone(memory_format=torch.contiguous_format)
        self._by_id = {id(t): self.shadow[name] for name, t in self._live.items()}
        self.state = torch.zeros(ops.EMA_STATE_BYTES, device=named[0][1].device, dtype=torch.uint8)

    def shadow_of(self, tensor, required=False):
        """The shadow of one of the model's tensors (by identity), or None."""
        sh = self._by_id.get(id(tensor))
        if sh is None and required:
            raise ValueError('WeightEMA holds no shadow for a tensor of shape %s' % (tuple(tensor.shape),))
        return sh

    def pairs(self):
        """[(shadow, live tensor)] in the model's order."""
        return [(self.shadow[name], t.detach()) for name, t in self._live.items()]

    def shadows(self):
        return list(self.shadow.values())

    @torch.no_grad()
    def update(self):
        """One update of every shadow from the model's current values: ct_ema_begin and one ct_ema_update."""
        ops.ema_begin(self.state, self.decay, self.warmup)
        ops.ema_update(self.pairs(), self.state)
        torch.autograd.graph.increment_version(self.shadows())

    @contextlib.contextmanager
    def swapped(self):
        """The model holds the averaged weights inside the block, and its own again after it."""
        self._swap()
        try:
            yield self
        finally:
            self._swap()

    @torch.no_grad()
    def _swap(self):
        ops.tensor_swap(self.pairs())
        # raw-pointer writes: the weight caches are keyed on tensor._version (see FusedSGD.step)
        torch.autograd.graph.increment_version(list(self._live.values()) + self.shadows())

    @torch.no_grad()
    def copy_to(self, model):
        """Copies the shadows into `model` (this one or another of the same architecture), by name."""
        own = dict(model.named_parameters())
        own.update(dict(model.named_buffers()))
        for name, sh in self.shadow.items():
            if name not in own:
                raise KeyError('WeightEMA.copy_to: the model has no tensor named %s' % name)
            own[name].copy_(sh)
        return model

    def info(self):
        """{'updates', 'decay', 'applied'} from the device; synchronises."""
        return ops.ema_info(self.state)

    def state_dict(self):
        return {'decay': self.decay, 'warmup': self.warmup, 'updates': self.info()['updates'],
                'shadow': {name: sh.clone() for name, sh in self.shadow.items()}}

    @torch.no_grad()
    def load_state_dict(self, sd):
        decay, warmup = _check_ema(sd['decay'], sd['warmup'])
        updates = int(sd['updates'])
        if updates < 0 or updates > 2 ** 31 - 1:
            raise ValueError('WeightEMA: invalid update count %d' % updates)
        missing = [n for n in self.shadow if n not in sd['shadow']]
        extra = [n for n in sd['shadow'] if n not in self.shadow]
        if missing or extra:
            raise KeyError('WeightEMA.load_state_dict: missing %s, unexpected %s' % (missing, extra))
        for name, sh in self.shadow.items():
            src = sd['shadow'][name]
            if tuple(src.shape) != tuple(sh.shape):
                raise ValueError('WeightEMA.load_state_dict: %s has shape %s, expected %s'
                                 % (name, tuple(src.shape), tuple(sh.shape)))
            sh.copy_(src)
        self.decay, self.warmup = decay, warmup
        host = bytes(_EmaState(updates, 0.0, 0.0, 0))      # decay and applied are rewritten by the next update
        self.state.copy_(torch.frombuffer(bytearray(host), dtype=torch.uint8))
