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
"""
import contextlib
import math

import torch

from . import ops
from ._lib import CtdetError
from ._lib import EmaState as _EmaState


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
        self.grad_scale = 1.0
        self.last_calls = 0         # ct_sgd_step calls of the last step() (one per distinct momentum triple)
        # an attribute, not a group key: state_dict() keeps torch's layout
        self.max_grad_norm = max_grad_norm
        self.clip_state = None      # 16-byte device tensor (ct_clip_state), allocated zeroed by the first clipped step
        self._clip_workspace = None
        self.ema = None             # a WeightEMA averaged inside the update (attach_ema); an attribute as well
        if ema is not None:
            self.attach_ema(ema)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault('grad_scale', 1.0)
        self.__dict__.setdefault('last_calls', 0)
        self.__dict__.setdefault('max_grad_norm', None)
        self.__dict__.setdefault('clip_state', None)
        self.__dict__.setdefault('_clip_workspace', None)
        self.__dict__.setdefault('ema', None)
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
        ema = self.ema
        if ema is not None:                     # one update of the average, skipped on the device with the step
            ops.ema_begin(ema.state, ema.decay, ema.warmup, clip_state=clip)
            averaged = set()
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
        if ema is not None:                     # parameters without a gradient this step, and the buffers
            ops.ema_update([(sh, live) for sh, live in ema.pairs() if id(sh) not in averaged], ema.state)
            touched += ema.shadows()
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

    def attach_ema(self, ema):
        """Average the weights in the pass that updates them: `ema` (a WeightEMA, or None to detach) must hold a shadow
        for every parameter of every group.  step() then opens one update on the device (skipped with the step when
        max_grad_norm's guard skips it), moves the shadows of the parameters it updates inside ct_sgd_step_ema and the
        remaining ones (no gradient this step, buffers) with one ct_ema_update."""
        if ema is not None:
            if not isinstance(ema, WeightEMA):
                raise TypeError('FusedSGD.attach_ema takes a ctdet.optim.WeightEMA, got %s' % type(ema).__name__)
            for gi, group in enumerate(self.param_groups):
                for pi, p in enumerate(group['params']):
                    if ema.shadow_of(p) is None:
                        raise ValueError('FusedSGD.attach_ema: parameter %d of group %d (shape %s) has no shadow in the '
                                         'WeightEMA' % (pi, gi, tuple(p.shape)))
        self.ema = ema
        return self


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
