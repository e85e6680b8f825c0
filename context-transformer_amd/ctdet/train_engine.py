"""Training engine: forward with batch-statistics BatchNorm + the full backward pass of the RFBNet
backbone and heads as HIP launches, exposed to autograd as ONE function.

What the reference gets from autograd + cuDNN in `train.py:222-229` (`model(data)` ...
`losses.backward()`) is rebuilt on the same fused launch plan as inference (ctdet.engine.Plan):

  forward   conv (identity epilogue) -> ct_bn_train_stats (batch mean / biased var, running-stat
            update with momentum 0.01) -> ct_bn_train_apply (+ReLU, + `out*scale + shortcut`) for
            BasicConv layers; the fused bias+ReLU conv for the VGG trunk and the heads.
  backward  reverse walk: ct_bn_train_backward / ct_bias_act_backward -> dZ, then per fused conv ONE
            weight-gradient launch (ct_conv2d_wgrad) and ONE data-gradient launch (ct_conv2d_fwd,
            transposed mode, accumulating into the producer's gradient buffer through the residual
            input), ct_maxpool2d_bwd for the pools, ct_head_grad_gather for the head scatter.

  phase 2   the Context-Transformer block on top of the conf head: ct_ctx_pool_fwd +
            ct_ctx_attention_fwd_train forward, ct_ctx_attention_bwd + ct_ctx_pool_bwd backward
            (ops.CtxTrainer), producing the gradient of the raw conf logits the head backward consumes.

Buffers are owned by the runtime and reused every step (call backward before the next forward).

CTDET_TRAIN_DETERMINISTIC=1 (opt-in): the weight gradients, BatchNorm reductions and bias sums run their `_det` twins (one slab
per split, added in order, in place of floating-point atomics: include/ctdet.h), so the convolutional step repeats bit for bit;
the Context-Transformer block is refused under it.  CTDET_TRAIN_DETERMINISTIC=2: all of that, and the block's backward runs
ct_ctx_attention_bwd_det (ops.CtxTrainer(deterministic=True)), so forward(use_ctx=True) is accepted and a whole phase-2 step
repeats bit for bit.

enable_bn_sync() (opt-in; CTDET_SYNC_BN=1 has enable_grad_sync() call it): data-parallel ranks normalise with the statistics of the
GLOBAL batch.  Per BatchNorm stage the forward runs ct_bn_sync_stats_local for every unfrozen part, ONE all-reduce of the stage's
float64 sums (ctdet.dist.BnStatSyncer), ct_bn_sync_stats_finish, then the unchanged ct_bn_train_apply; the backward runs
ct_bn_sync_backward_local, one all-reduce, ct_bn_sync_backward_apply.  The local reductions are the ordered form in either mode.
"""
import ctypes as C
import os
from dataclasses import dataclass, field

import torch

from . import _lib, conv_policy, ops, wgrad_routes
from .engine import ConvPart, ConvStep, Plan, Runtime, apply_tuned, run_on_streams, weight_parts, wire_absmax
from .wino_forms import FORMS


@dataclass
class LayerState:
    """What a training step keeps for one fused conv (TrainRuntime.state[name]); None / empty where the layer has no use for it."""
    # forward: what run_conv launches -- the plan step, or a BatchNorm layer's identity-epilogue conv into 'z.<name>'
    fwd: object = None
    is_bn: bool = False
    # BatchNorm, per part: batch statistics, fp64 reduction scratch, the parts the last forward found in eval() mode
    mean: list = field(default_factory=list)
    var: list = field(default_factory=list)
    scratch: list = field(default_factory=list)
    frozen: list = field(default_factory=list)
    # synchronized BatchNorm: the parts enable_bn_sync() found in train mode, and per part the slice sums of the sync entries'
    # ordered reductions (a view of TrainRuntime.bn_sync_scratch; in deterministic mode the part's det_scratch slice itself)
    sync_parts: list = field(default_factory=list)
    sync_scratch: list = field(default_factory=list)
    # epilogue gradients: dZ of zc channels (cout; the heads' padded with zero channels, whose weights are zero_w), per-part
    # parameter gradients (views of the gradient arena); dz_from_pool: the fused pool backward wrote dZ in this pass
    zc: int = 0
    zero_w: object = None
    dz: object = None
    dgamma: list = field(default_factory=list)
    dbeta: list = field(default_factory=list)
    dbias: list = field(default_factory=list)
    dz_from_pool: bool = False
    ev_dz: object = field(default_factory=torch.cuda.Event)     # dZ ready -> the weight-gradient stream
    # data gradient (none for the image): transposed descriptor with fp32 weights wpk_d [kpad, mpad], unit epilogue and split-K
    # slabs; its forward-convolution twin for the Winograd kernels (tile, weights U_d); the bf16x3 config (weights wx3_d)
    dgrad: object = None
    wpk_d: object = None
    ones: object = None
    zeros: object = None
    ksws_d: object = None
    dgrad_wino: object = None
    dgrad_tile: object = None
    U_d: object = None
    dgrad_x3: object = None
    wx3_d: object = None
    # weight gradient: descriptor (forward geometry on the forward input), route, dense dw (a view of the gradient arena) and,
    # under CTDET_PREZERO, the layer's own slice of the zeroed workspace
    wgrad: object = None
    wgrad_route: object = None
    wgrad_ws_bytes: int = 0
    wgrad_ws: object = None
    dw: object = None
    dz_amax: object = None      # maxima of |dZ|: the slot ct_bias_act_backward_amax fills (_wire_absmax)
    # deterministic mode, per part: the slice of TrainRuntime.det_scratch its BatchNorm reductions (both passes) resp. its dbias
    # sum (the fused pool backward's included) store their partial sums in
    det_scratch: list = field(default_factory=list)


@dataclass(frozen=True)
class TrainSwitches:
    """The training runtime's own environment switches, read once (kernel choice: self.policy, wgrad_routes)."""
    pack_batch: bool        # CTDET_PACK_BATCH=0: per-layer pack launches instead of the recorded lists
    prezero: bool           # CTDET_PREZERO=0: the library's per-launch memsets instead of the arenas
    fuse_pool_bwd: bool     # CTDET_TRAIN_FUSE_POOL_BWD=0: pool backward and bias / ReLU backward as two kernels
    streams: int            # CTDET_TRAIN_STREAMS=1: weight gradients on the caller's stream
    ksplit: int             # CTDET_KSPLIT=0: no split-K slabs for the data gradients
    deterministic: bool = False     # CTDET_TRAIN_DETERMINISTIC=1 or 2: ordered slab sums in place of the floating-point atomics
    deterministic_ctx: bool = False     # CTDET_TRAIN_DETERMINISTIC=2: the Context-Transformer block's backward too
    sync_bn: bool = False           # CTDET_SYNC_BN=1: enable_grad_sync() also synchronizes the BatchNorm statistics (enable_bn_sync)

    @classmethod
    def of(cls, env):
        det = env.get('CTDET_TRAIN_DETERMINISTIC', '0')
        return cls(env.get('CTDET_PACK_BATCH', '1') != '0', env.get('CTDET_PREZERO', '1') != '0',
                   env.get('CTDET_TRAIN_FUSE_POOL_BWD', '1') != '0', int(env.get('CTDET_TRAIN_STREAMS', '2')),
                   int(env.get('CTDET_KSPLIT', '1')), det not in ('', '0'), det == '2',
                   env.get('CTDET_SYNC_BN', '0') not in ('', '0'))


class PackList:
    """A list of fixed-size pack items: built once for a key (host items from the `item` entry point, item_bytes() each), uploaded,
    replayed as ONE `run` launch per step."""

    def __init__(self, lib, name):
        self.name, self.table, self.n, self.key = name, None, 0, None
        self.item_bytes, self.item, self.run = (getattr(lib, name + sfx) for sfx in ('_item_bytes', '_item', '_run'))

    def replay(self, key, entries, device, stream):
        """entries() yields (parts, zero_w, the item arguments between the weight parts and the item) per layer, in order."""
        if self.key is None or self.key != key:
            nbytes, items = self.item_bytes(), []
            for parts, zero_w, args in entries():
                buf = (C.c_ubyte * nbytes)()
                _lib.check(self.item(*weight_parts(parts, zero_w), *args, buf), self.name + '_item')
                items.append(bytes(buf))
            self.table = torch.frombuffer(bytearray(b''.join(items)), dtype=torch.uint8).to(device) if items else None
            self.n, self.key = len(items), key
        if self.n:
            _lib.check(self.run(self.table.data_ptr(), self.n, stream), self.name + '_run')


class TrainRuntime:
    def __init__(self, net, batch, backend):
        self.net, self.batch, self.be, self.backend, self.lib = net, batch, backend, backend, backend.lib
        self.plan = Plan(net, batch)
        al = backend.alloc
        self.bufs = {n: al((batch,) + tuple(s)) for n, s in self.plan.buf_shapes.items()}
        self.grads = {n: al((batch,) + tuple(s)) for n, s in self.plan.buf_shapes.items() if n != 'x'}
        self.state = {}
        self.switches = TrainSwitches.of(os.environ)
        self.prezero = self.switches.prezero
        self._pack_table, self._pack_ptrs, self._pack_counts, self._recording = None, None, (0, 0), False
        self._x3_list, self._h2_list = PackList(self.lib, 'ct_conv_x3_pack'), PackList(self.lib, 'ct_conv_wino_h2_pack')
        self.bucketer, self.generation, self.used_ctx, self.amax_slots, self._wired_epoch = None, 0, False, {}, None
        self.bn_sync_scratch = None
        self.bn_sync = None                     # ctdet.dist.BnStatSyncer once enable_bn_sync() found more than one rank
        self.wgrad_wsh2 = self.wgrad_ws_all = self.bn_scratch = self.wgrad_wsdet = self.det_scratch = None
        self.det, self.det_ctx = self.switches.deterministic, self.switches.deterministic_ctx
        self.params, self._pindex, self.ctx = [], {}, None      # params: ordered parameters that receive gradients
        if self.plan.ctx:
            C_ = net.num_classes
            self.P = self.bufs['conf'].shape[1] // C_
            self.ctx = ops.CtxTrainer(batch, self.P, self.plan.M, C_, net.OBJ_Target.weight.shape[0],
                                      net.setting == 'incre', backend.device, deterministic=self.det_ctx)
            self.ctx_params = dict(obj_w=net.OBJ_Target.weight, wz=net.Wz, theta_w=net.theta.weight, theta_b=net.theta.bias,
                                   phi_w=net.phi.weight, phi_b=net.phi.bias, g_w=net.g.weight, g_b=net.g.bias)
            if net.setting == 'incre':
                self.ctx_params.update(fc_w=net.fc_base.weight, fc_b=net.fc_base.bias)
            for prm in self.ctx_params.values():
                self._reg(prm)
        self._ws_need = {'dgrad_ws4s': 0}       # bytes of the workspaces all layers share, by the runtime attribute that holds them
        self.wgrad_h2 = wgrad_routes.h2_enabled(os.environ)         # opt-in, resolved once here
        # the kernel policy of the step (ctdet/conv_policy.py): forward and data-gradient launches; h2 = its Winograd launches run
        # on the f16x2 operand form (csrc/ct_f16x2.h)
        self.policy = backend.policy = conv_policy.resolve(net, batch, os.environ, training=True)
        self.h2 = self.policy.h2
        for st in self.plan.steps:
            if st.kind == 'conv':
                self._build_layer(st)
        self._alloc_workspaces()
        Runtime._build_schedule(self)           # forward: Norm branch / heads on a side stream (CTDET_STREAMS)
        # the forward launches of the three-kernel Winograd form share ONE V / M workspace per stream of that schedule
        # (HipBackend.ws_pool); the launch object of a BatchNorm layer is its zstep, not the plan step
        for i, st in enumerate(self.plan.steps):
            if st.kind == 'conv':
                self.state[st.name].fwd.rt['ws_key'] = self.sid[i] if self.side is not None else 0
        backend.ws_rebuild([self.state[st.name].fwd for st in self.plan.steps if st.kind == 'conv'])
        self._wire_absmax()
        self._pool_bwd = self._find_fused_pool_bwd() if self.switches.fuse_pool_bwd else {}
        if self.det:
            self._alloc_det_scratch()
        # weight gradients beside the data-gradient chain (CTDET_TRAIN_STREAMS=1 keeps everything on the caller's stream).  The
        # stream is the forward pass's side stream: the two are never busy at the same time, and a training step with ONE side
        # stream can be captured as a hipGraph (a second one crashes hipStreamEndCapture on ROCm 7.2)
        self.wg_stream = (self.side if self.side is not None else torch.cuda.Stream(backend.device)) \
            if self.switches.streams > 1 else None
        self._bns = [p.bn for st in self.plan.steps if st.kind == 'conv' for p in st.parts if p.bn is not None]
        self._nbt = [bn.num_batches_tracked for bn in self._bns]
        self._build_gradient_arena()

    # ------------------------------------------------------------------ construction, one thing per method
    def _build_layer(self, st):
        s = self.state[st.name] = LayerState(is_bn=st.parts[0].bn is not None, frozen=[False] * len(st.parts))
        assert all((p.bn is not None) == s.is_bn for p in st.parts), st.name
        ctot, al = st.cout, self.be.alloc
        # channel count of the dZ buffer.  A multibox head has 4 k + C k + k output channels (156 for six anchors and 20
        # classes): not a multiple of 8 / 16, so its data gradient (a 3x3 convolution WITH dZ's channels as input) fitted
        # neither the Winograd nor the bf16x3 kernel and ran on the fp32 implicit GEMM (2 x 450-770 us per step).  dZ
        # is padded with zero channels instead (ct_head_grad_gather writes 0 outside its segments; the packed
        # data-gradient weights get a zero part of as many rows).
        s.zc = (ctot + 15) // 16 * 16 if (st.segs and st.src != 'x' and (st.kh, st.kw, st.stride, st.dil) == (3, 3, 1, 1)) else ctot
        s.zero_w = torch.zeros(s.zc - ctot, st.cin, st.kh, st.kw, device=self.be.device) if s.zc > ctot else None
        s.dz = al((self.batch, s.zc, st.oh, st.ow))
        s.dw = al((ctot, st.cin, st.kh, st.kw))
        self._build_forward(st, s)
        if st.src != 'x':                       # (the image needs no data gradient)
            self._build_dgrad(st, s)
        self._build_wgrad(st, s)
        for p in st.parts:
            for q in (p.weight,) + ((p.bn.weight, p.bn.bias) if p.bn is not None else (p.bias,) if p.bias is not None else ()):
                self._reg(q)

    def _build_forward(self, st, s):
        """The forward launch object and the per-part buffers of its epilogue."""
        al, batch = self.be.alloc, self.batch
        if s.is_bn:                             # conv with identity epilogue into a dense Z buffer
            zname = 'z.' + st.name
            self.bufs[zname] = al((batch, st.cout, st.oh, st.ow))
            s.fwd = ConvStep(zname, [ConvPart(p.weight, None, None, False) for p in st.parts], st.cin, st.kh, st.kw, st.stride,
                             st.ph, st.pw, st.dil, st.src, st.src_coff, st.h, st.w, zname, 0)
        else:
            s.fwd = st
        self.be.prepare_conv(s.fwd, self.bufs, batch)
        apply_tuned(self.be, s.fwd, batch, wino4=self.policy.wino4)
        if s.is_bn:
            s.mean, s.var, s.dgamma, s.dbeta = ([al((p.cout,)) for p in st.parts] for _ in range(4))
            s.scratch = [al((2 * p.cout,), torch.float64) for p in st.parts]     # sliced BN reductions
        else:
            s.dbias = [al((p.cout,)) for p in st.parts]

    def _build_dgrad(self, st, s):
        """The data-gradient descriptor, its Winograd / bf16x3 form (conv_policy.choose_dgrad) and their weight buffers."""
        al, batch, zc = self.be.alloc, self.batch, s.zc
        kpad = self.lib.ct_conv_kpad(zc, st.kh, st.kw)
        mpad = self.lib.ct_conv_mpad(st.cin)
        s.wpk_d = al((kpad, mpad))
        s.ones = torch.ones(mpad, device=self.be.device)
        s.zeros = torch.zeros(mpad, device=self.be.device)
        d = _lib.ConvDesc()
        d.in_ = s.dz.data_ptr()
        d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = batch, zc, st.oh, st.ow, zc, 0
        d.wpacked, d.scale, d.shift = s.wpk_d.data_ptr(), s.ones.data_ptr(), s.zeros.data_ptr()
        d.cout, d.m_pad, d.k_pad = st.cin, mpad, kpad
        d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = st.kh, st.kw, st.stride, st.ph, st.pw, st.dil
        d.oh, d.ow = st.h, st.w
        g = self.grads[st.src]
        d.out, d.out_ctot, d.out_coff = g.data_ptr(), g.shape[1], st.src_coff
        d.res_ctot, d.res_coff, d.res_scale = g.shape[1], st.src_coff, 1.0
        d.transposed = 1
        if self.switches.ksplit and st.cin * batch * st.h * st.w <= (2 << 20):
            s.ksws_d = al((16 * st.cin * batch * st.h * st.w,))      # split-K slabs (small maps)
            d.ksplit, d.ksplit_ws, d.ksplit_ws_floats = -1, s.ksws_d.data_ptr(), s.ksws_d.numel()
        s.dgrad = d
        # the data gradient written as a forward convolution on dZ (channels swapped, taps rotated: the packed weights):
        # what the Winograd kernels launch on, and what their geometry checks are asked about.  The dilated output
        # transform has no accumulate, so a source gradient that was already written goes through a scratch tensor
        # (does not happen in these networks)
        w2 = _lib.ConvDesc.from_buffer_copy(d)
        w2.transposed = 0
        if st.dil > 1:
            w2.ksplit, w2.ksplit_ws, w2.ksplit_ws_floats = 0, None, 0
        s.dgrad_tile, s.dgrad_x3 = conv_policy.choose_dgrad(
            self.policy, conv_policy.Layer.of(st, batch, zc, s.is_bn), s.fwd.rt.get('wino'),
            lambda form: bool(getattr(self.lib, 'ct_conv_%s_supported' % form)(C.byref(w2))))
        if s.dgrad_tile is not None:
            s.dgrad_wino = w2
            f = FORMS[s.dgrad_tile]
            s.U_d = f.alloc(self.lib, al, zc, st.cin, dgrad=True)
            if f.split:                 # V / M workspace shared by all data gradients
                self._ws_need['dgrad_ws4s'] = max(self._ws_need['dgrad_ws4s'], self.lib.ct_conv_wino4s_workspace_bytes(C.byref(w2)))
        if s.dgrad_x3 is not None:
            s.wx3_d = al((self.lib.ct_conv_x3_packed_bytes(zc, st.cin, st.kh, st.kw, self.lib.ct_conv_x3_config_bk(s.dgrad_x3)),),
                         torch.uint8)

    def _build_wgrad(self, st, s):
        """The weight-gradient descriptor = forward geometry on the forward input; its entry point (ctdet/wgrad_routes.py) and
        what that asks of the route's workspace: one per route, shared by all layers (weight gradients run in stream order)."""
        w = s.wgrad = _lib.ConvDesc()
        src = self.bufs[st.src]
        w.in_ = src.data_ptr()
        w.batch, w.cin, w.h, w.w, w.in_ctot, w.in_coff = self.batch, st.cin, st.h, st.w, src.shape[1], st.src_coff
        w.cout = st.cout
        w.kh, w.kw, w.stride, w.pad_h, w.pad_w, w.dil = st.kh, st.kw, st.stride, st.ph, st.pw, st.dil
        w.oh, w.ow = st.oh, st.ow
        r = s.wgrad_route = wgrad_routes.choose(self.lib, st, w, st.cout, os.environ, deterministic=self.det)
        s.wgrad_ws_bytes = r.workspace_bytes(self.lib, w)
        self._ws_need[r.ws] = max(self._ws_need.get(r.ws, 0), s.wgrad_ws_bytes)

    def _alloc_workspaces(self):
        """The workspaces all layers share, and under CTDET_PREZERO the arenas of the accumulation buffers the library would
        otherwise zero with one small memset per launch (~150 per step): the BatchNorm reduction scratch (both passes), the
        Winograd weight-gradient workspaces (one per layer instead of a shared one) and -- through the gradient arena -- the
        bias / split weight gradients."""
        need, dev = self._ws_need, self.be.device
        self.wgrad_ws = self.be.alloc((max(need.get('wgrad_ws', 0) // 4, 1),))
        self.dgrad_ws4s = torch.empty(max(need['dgrad_ws4s'], 1), device=dev, dtype=torch.uint8)
        self.wgrad_ws4s = torch.empty(max(need.get('wgrad_ws4s', 0), 1), device=dev, dtype=torch.uint8)
        if self.wgrad_h2:
            self.wgrad_wsh2 = torch.empty(max(need.get('wgrad_wsh2', 0), 1), device=dev, dtype=torch.uint8)
        if self.det:                            # the slabs of the largest deterministic weight gradient
            self.wgrad_wsdet = torch.empty(max(need.get('wgrad_wsdet', 0), 1), device=dev, dtype=torch.uint8)
        if not self.prezero:
            return
        al, states = self.be.alloc, list(self.state.values())
        self.bn_scratch = al((max(sum(t.numel() for s in states for t in s.scratch), 1),), torch.float64)
        o = 0
        for s in states:
            for i, t in enumerate(s.scratch):
                s.scratch[i] = self.bn_scratch[o:o + t.numel()]
                o += t.numel()
        sizes = [(s, s.wgrad_ws_bytes // 4) for s in states if s.wgrad_route.zeroed]
        self.wgrad_ws_all = al((max(sum((n + 63) // 64 * 64 for _, n in sizes), 1),))
        o = 0
        for s, n in sizes:
            s.wgrad_ws = self.wgrad_ws_all[o:o + n]
            o += (n + 63) // 64 * 64

    def _alloc_det_scratch(self):
        """Deterministic mode: ONE float64 arena; every BatchNorm part and every bias sum owns a slice of it, sized by the library's
        queries (a fused pool producer's slice also holds that launch's per-image sums).  Nothing zeroes it: the reductions store
        every partial sum they later add."""
        lib, B = self.lib, self.batch
        fused = {pr.name for pr in self._pool_bwd.values()}
        sizes = []
        for st, s in self._convs():
            for p in st.parts:
                hw = st.oh * st.ow
                if s.is_bn:
                    n = lib.ct_bn_det_scratch_bytes(B, p.cout, hw, None)
                else:
                    n = lib.ct_bias_det_scratch_bytes(B, p.cout, hw, None)
                    if st.name in fused:
                        n = max(n, lib.ct_maxpool2x2_bias_relu_bwd_det_scratch_bytes(B, p.cout, None))
                sizes.append((s, (int(n) + 15) // 16 * 2))          # doubles, slices 16-byte aligned
        self.det_scratch = self.be.alloc((max(sum(n for _, n in sizes), 1),), torch.float64)
        o = 0
        for s, n in sizes:
            s.det_scratch.append(self.det_scratch[o:o + n])
            o += n

    def _find_fused_pool_bwd(self):
        """MaxPool2d(2, 2) whose input only the pool reads, under a convolution with bias + ReLU and no BatchNorm (conv1_2, conv2_2,
        conv3_3): the pool's backward and the convolution's bias / ReLU backward are ONE pass (ct_maxpool2x2_bias_relu_bwd) -- the
        gradient of the pool's input is never materialised.  -> {pool step name: the convolution}"""
        steps, found = self.plan.steps, {}
        for ps in steps:
            if ps.kind != 'pool' or (ps.k, ps.stride, ps.pad) != (2, 2, 0):
                continue
            prods = [st for st in steps if st.kind == 'conv' and st.dst == ps.src and not st.segs]
            others = [st for st in steps if st is not ps and (getattr(st, 'src', None) == ps.src or getattr(st, 'res', None) == ps.src)]
            if len(prods) != 1 or others:
                continue
            pr = prods[0]
            s = self.state[pr.name]
            if not s.is_bn and len(pr.parts) == 1 and pr.parts[0].relu and pr.parts[0].bias is not None and pr.dst_coff == 0 and \
                    pr.cout == ps.ch and s.zc == pr.cout and pr.res is None and self.grads[ps.dst].shape[1] == ps.ch:
                found[ps.name] = pr
        return found

    def _build_gradient_arena(self):
        """ONE flat fp32 buffer in production order.  The weight / bias / BatchNorm gradient kernels write straight into their
        slice (no per-parameter copies), the bucketed all-reduce runs on slices of it, and backward() hands autograd views of
        a single snapshot."""
        order = self.production_order()
        assert len({id(q) for q in order}) == len(order) == len(self.params), 'parameter used by two plan steps'
        self._prod_index = {id(q): i for i, q in enumerate(order)}
        self._arena_off = [0]
        for q in order:
            self._arena_off.append(self._arena_off[-1] + q.numel())
        self.arena = self.be.alloc((max(self._arena_off[-1], 1),))
        for st in self.plan.steps:
            if st.kind != 'conv':
                continue
            s = self.state[st.name]
            for i, p in enumerate(st.parts):
                if s.is_bn:
                    s.dgamma[i], s.dbeta[i] = self._arena_view(p.bn.weight), self._arena_view(p.bn.bias)
                elif p.bias is not None:
                    s.dbias[i] = self._arena_view(p.bias)
            i0 = self._prod_index[id(st.parts[0].weight)]
            assert all(self._prod_index[id(p.weight)] == i0 + k for k, p in enumerate(st.parts))
            a0 = self._arena_off[i0]
            s.dw = self.arena[a0:a0 + s.dw.numel()].view(s.dw.shape)

    def _wire_absmax(self):
        """Maxima of |activation| / |dZ| for the f16x2 launches of the step (engine.wire_absmax is the loop, shared with inference).
        Forward: a buffer has a slot when every step that writes it is a convolution WITHOUT BatchNorm on a tracking kernel (the
        BatchNorm layers' outputs are written by ct_bn_train_apply, which does not track); a pooled buffer shares its source's.
        A fused f16x2 launch (tile 48) without a slot becomes its bf16x3 twin; the three-kernel form (47) takes the maxima
        inside its launch.  Backward: the dZ of a layer without BatchNorm is written by ct_bias_act_backward_amax into a slot of
        its own (s.dz_amax), read by that layer's data-gradient launch."""
        be = self.be
        if not self.h2:
            return
        convs = [st for st in self.plan.steps if st.kind == 'conv']

        def fwd(st):
            return self.state[st.name].fwd

        def form(st):
            return FORMS.get(fwd(st).rt.get('wino'))

        def tracks(st):
            if st.kind != 'conv' or st.segs or self.state[st.name].is_bn:
                return False
            return form(st).tracks if form(st) is not None else True

        def to_plain(st):
            if form(st).own_max:
                return False
            be.enable_wino(fwd(st), tile=form(st).plain)
            return True
        self.amax_slots = wire_absmax(be, self.batch, self.plan.steps, convs, lambda st: fwd(st).rt['desc'],
                                      lambda st: form(st) is not None and form(st).h2, tracks, to_plain)
        for st in convs:
            s = self.state[st.name]
            s.dz_amax = None
            if s.dgrad_wino is not None and FORMS[s.dgrad_tile].h2 and not s.is_bn and not st.segs:
                s.dz_amax = be.new_slot(self.batch)
                s.dgrad_wino.in_absmax = s.dz_amax
            elif s.wgrad_route.dz_amax and not s.is_bn and not st.segs:
                s.dz_amax = be.new_slot(self.batch)     # ct_bias_act_backward_amax leaves dZ's maxima for ct_conv2d_wgrad_h2
        self._wired_epoch = be.kernel_epoch

    def _arena_view(self, prm, flat=None):
        i = self._prod_index[id(prm)]
        return (self.arena if flat is None else flat)[self._arena_off[i]:self._arena_off[i + 1]].view(prm.shape)

    def _reg(self, prm):
        if id(prm) not in self._pindex:
            self._pindex[id(prm)] = len(self.params)
            self.params.append(prm)

    def production_order(self):
        """Parameters in the order backward() produces their gradients (heads first)."""
        order = list(self.ctx_params.values()) if self.ctx is not None else []
        for st in reversed(self.plan.steps):
            if st.kind != 'conv':
                continue
            for p in st.parts:
                if p.bn is not None:
                    order += [p.bn.weight, p.bn.bias]
                elif p.bias is not None:
                    order.append(p.bias)
            order += [p.weight for p in st.parts]
        return order

    def enable_grad_sync(self, bucket_bytes=32 << 20, group=None):
        """Data-parallel training: all-reduce (mean) the gradients over the process group in
        large buckets, overlapped with the rest of the backward pass (ctdet.dist.GradBucketer)."""
        from .dist import GradBucketer
        self.bucketer = GradBucketer([p.numel() for p in self.production_order()], self.be.device, bucket_bytes, group, flat=self.arena)
        if self.switches.sync_bn:
            self.enable_bn_sync(group)
        return self.bucketer

    def enable_bn_sync(self, group=None):
        """Data-parallel training: every BatchNorm layer in train mode normalises with the statistics of the GLOBAL batch, and its
        backward uses the global sums (ctdet.dist.BnStatSyncer; the ct_bn_sync_* entries).  Per stage and pass: the local sums of
        every unfrozen part, ONE all-reduce, finish / apply.  Independent of enable_grad_sync(); a no-op for a world of one
        without a group.  Call it again after moving BatchNorm layers between train() and eval()."""
        import torch.distributed as dist
        from .dist import BnStatSyncer
        if group is None and (not dist.is_initialized() or dist.get_world_size() == 1):
            self.bn_sync = None
            return None
        stages = []
        for st, s in self._convs():
            if s.is_bn:
                s.sync_parts = [i for i, p in enumerate(st.parts) if p.bn.training]
                if s.sync_parts:
                    stages.append((st.name, [st.parts[i].cout for i in s.sync_parts]))
        if self.det:
            for _, s in self._convs():
                if s.is_bn:
                    s.sync_scratch = list(s.det_scratch)
        elif self.bn_sync_scratch is None:
            self._alloc_bn_sync_scratch()
        self.bn_sync = BnStatSyncer(stages, self.batch, self.be.device, group)
        return self.bn_sync

    def _alloc_bn_sync_scratch(self):
        """The ordered reductions of the sync entries store their slice sums like the `_det` twins: outside deterministic mode
        (which has these slices already) every BatchNorm part gets its own slice of one float64 arena."""
        sizes = []
        for st, s in self._convs():
            if s.is_bn:
                for p in st.parts:
                    n = self.lib.ct_bn_det_scratch_bytes(self.batch, p.cout, st.oh * st.ow, None)
                    sizes.append((s, (int(n) + 15) // 16 * 2))
        self.bn_sync_scratch = self.be.alloc((max(sum(n for _, n in sizes), 1),), torch.float64)
        o = 0
        for s, n in sizes:
            s.sync_scratch.append(self.bn_sync_scratch[o:o + n])
            o += n

    def _s(self):
        return C.c_void_p(torch.cuda.current_stream(self.be.device).cuda_stream)

    def _convs(self):
        return [(st, self.state[st.name]) for st in self.plan.steps if st.kind == 'conv']

    # ------------------------------------------------------------------ weight packing
    def _pack_dgrad(self, st, s):
        """The data-gradient layout of one fused conv from the current weights (with the zero channels dZ is padded with)."""
        ptrs, couts, n = weight_parts(st.parts, s.zero_w)
        if s.dgrad_wino is not None:
            f = FORMS[s.dgrad_tile]
            if f.h2 and self._recording:
                return                  # takes the layer's maximum first: not recordable, batched by the f16x2 list of _repack_all
            _lib.check(f.pack_weights(self.lib, ptrs, couts, n, st.cin, s.U_d.data_ptr(), self._s(), dgrad=True),
                       st.name + ' pack dgrad (%s)' % f.name)
        elif s.dgrad_x3 is not None:
            if self._recording:
                return                  # not a recordable pack kind: re-issued every step by _repack_all
            _lib.check(self.lib.ct_conv_pack_weights_x3_dgrad(ptrs, couts, n, st.cin, st.kh, st.kw, self.lib.ct_conv_x3_config_bk(s.dgrad_x3),
                                                              s.wx3_d.data_ptr(), self._s()), st.name + ' pack dgrad (bf16x3)')
        else:
            _lib.check(self.lib.ct_conv_pack_weights_dgrad(ptrs, couts, n, st.cin, st.kh, st.kw, s.wpk_d.data_ptr(),
                                                           s.wpk_d.shape[1], s.wpk_d.shape[0], self._s()), st.name + ' pack dgrad')

    def _pack_key(self):
        """Cache key of the recorded lists: the parameter storage AND what each layer's launch reads (kernel choice and
        packed-weight buffer can change after the first step: enable_x3 / enable_wino / apply_tuned on the shared backend)."""
        ptrs = [p.data_ptr() for p in self.params]
        for st, s in self._convs():
            rt = s.fwd.rt
            x3 = rt.get('x3')
            f = FORMS.get(rt.get('wino'))
            ptrs.append((st.name, rt.get('wino') or 0, -1 if x3 is None else x3,
                         tuple((k, rt[k].data_ptr()) for k in ((f.key,) if f is not None else ()) + ('wpk',)
                               if rt.get(k) is not None),
                         tuple(sorted((bk, t.data_ptr()) for bk, t in rt.get('wx3', {}).items()))))
        return ptrs

    def _record_packs(self):
        """Record the recordable pack launches of every layer (ct_pack_record_*) into self._pack_table.  Skipped while recording,
        each batched by a list of its own in _repack_all: a bf16x3 layer's weight split (ct_conv_pack_weights_x3 is not
        recordable and would launch right here; only its epilogue is folded) and the f16x2 Winograd layouts, forward and data
        gradient (they take the layer's maximum first)."""
        lib = self.lib
        _lib.check(lib.ct_pack_record_begin(), 'ct_pack_record_begin')
        self._recording = True
        try:
            for st, s in self._convs():
                f = FORMS.get(s.fwd.rt.get('wino'))
                self.be.pack_conv(s.fwd, weights=s.fwd.rt.get('x3') is None and not (f is not None and f.h2))
                if s.dgrad is not None:
                    self._pack_dgrad(st, s)
        finally:
            self._recording = False
            nbytes = lib.ct_pack_record_bytes()
            self._pack_table = torch.empty(nbytes, dtype=torch.uint8, device=self.be.device)
            nd, nw = C.c_int(0), C.c_int(0)
            _lib.check(lib.ct_pack_record_end(self._pack_table.data_ptr(), nbytes, C.byref(nd), C.byref(nw), self._s()),
                       'ct_pack_record_end')
        self._pack_counts = (nd.value, nw.value)

    def _x3_entries(self):
        """The bf16x3 weight splits, forward then data gradient per layer (the direct layers of a training step run bf16x3)."""
        for st, s in self._convs():
            if s.fwd.rt.get('x3') is not None:
                bk = self.be.x3_bk(s.fwd.rt['x3'])
                yield s.fwd.parts, None, (s.fwd.cin, s.fwd.kh, s.fwd.kw, bk, s.fwd.rt['wx3'][(bk, False)].data_ptr(), 0)
            if s.dgrad is not None and s.dgrad_x3 is not None:
                yield st.parts, s.zero_w, (st.cin, st.kh, st.kw, self.lib.ct_conv_x3_config_bk(s.dgrad_x3), s.wx3_d.data_ptr(), 1)

    def _h2_entries(self):
        """The f16x2 Winograd layouts, forward then data gradient per layer."""
        for st, s in self._convs():
            f = FORMS.get(s.fwd.rt.get('wino'))
            if f is not None and f.h2:
                yield s.fwd.parts, None, (s.fwd.cin, 0, f.code, s.fwd.rt[f.key].data_ptr())
            if s.dgrad_wino is not None and FORMS[s.dgrad_tile].h2:
                yield st.parts, s.zero_w, (st.cin, 1, s.dgrad_tile, s.U_d.data_ptr())

    def _repack_all(self):
        """Every optimizer step changes every weight, and every fused conv needs its forward and its data-gradient
        layout: ~130 small pack launches per step.  They are recorded ONCE (ct_pack_record_*) and replayed as two
        batched launches at the start of each forward (the backward pass of the same step reads the same weights); the
        bf16x3 weight splits are one more launch (PackList: the arguments never change between steps) and the f16x2 Winograd
        layouts three -- maxima of the weights, then the split -- for the whole list.  CTDET_PACK_BATCH=0 keeps the per-layer launches."""
        if not self.switches.pack_batch:
            return
        key = self._pack_key()                  # (what the recording skips and leaves to the two lists, and why: _record_packs)
        if self._pack_table is None or key != self._pack_ptrs:
            self._record_packs()
            self._pack_ptrs = key
        _lib.check(self.lib.ct_pack_run(self._pack_table.data_ptr(), self._pack_counts[0], self._pack_counts[1], self._s()),
                   'ct_pack_run')
        self._x3_list.replay(key, self._x3_entries, self.be.device, self._s())
        if self.h2:
            self._h2_list.replay(key, self._h2_entries, self.be.device, self._s())

    # ------------------------------------------------------------------ forward
    def _ctx_tensors(self):
        p = {k: v.detach() for k, v in self.ctx_params.items()}
        p['scale'] = self.net._scale_value()
        return p

    def forward(self, x, use_ctx=True):
        lib, B = self.lib, self.batch
        if self.det and not self.det_ctx and use_ctx and self.ctx is not None:
            raise _lib.CtdetError('CTDET_TRAIN_DETERMINISTIC=1 does not cover the Context-Transformer block: ct_ctx_attention_bwd '
                                  'sums through floating-point atomics (csrc/ct_attn_bwd.hip); set the switch to 2 '
                                  "(ct_ctx_attention_bwd_det) or unset it for a phase-2 'ours' network")
        self.generation += 1                        # saved activations belong to THIS forward
        self.used_ctx = bool(use_ctx and self.ctx is not None)
        if tuple(x.shape) != tuple(self.bufs['x'].shape):
            raise _lib.CtdetError('training plan was built for input %s, got %s' % (tuple(self.bufs['x'].shape), tuple(x.shape)))
        self.bufs['x'].copy_(x)
        self._repack_all()
        if self.h2:
            if self._wired_epoch != self.be.kernel_epoch:     # a step changed kernels since the slots were wired
                self._wire_absmax()
            self.be.zero_slots()                    # maxima of |activation| and |dZ| of this step (_wire_absmax)
        if self.prezero:
            self.bn_scratch.zero_()                 # one memset instead of one per BatchNorm statistics launch
        _lib.check(lib.ct_scratch_prezeroed(int(self.prezero)), 'ct_scratch_prezeroed')
        # Norm branch and heads on the side stream, like the inference runtime (same schedule builder)
        try:
            run_on_streams(self, self._forward_step)
        finally:
            lib.ct_scratch_prezeroed(0)
        nbt = [t for t, bn in zip(self._nbt, self._bns) if bn.training]
        if nbt:
            torch._foreach_add_(nbt, 1)             # nn.BatchNorm2d's num_batches_tracked, one launch for all layers
        conf, d = self.bufs['conf'], self.net.num_classes
        if self.used_ctx:
            conf = self.ctx.forward(conf.view(B, self.P, d), self.bufs['pool'].view(B, self.plan.M, d), self._ctx_tensors())
        return self.bufs['loc'], conf, self.bufs['obj']

    def _forward_step(self, st):
        if st.kind == 'pool':
            self.be.run_pool(st, self.bufs, self.batch)
        elif st.kind == 'ctxpool':
            if self.used_ctx:
                self.be.run_ctxpool(st, self.bufs, self.batch)
        elif st.kind != 'conv':
            raise _lib.CtdetError('step %s has no training implementation' % st.name)
        else:
            s = self.state[st.name]
            self.be.pack_conv(s.fwd, weights=not self.switches.pack_batch)       # epilogue vectors (bias fold)
            self.be.run_conv(s.fwd)
            if s.is_bn:
                self._bn_forward(st, s)

    def _bn_forward(self, st, s):
        """Batch statistics (running-statistics update included) and normalisation + ReLU + shortcut of a BatchNorm layer's Z."""
        lib, B = self.lib, self.batch
        z, dst, hw = self.bufs[s.fwd.dst], self.bufs[st.dst], st.oh * st.ow
        off = 0
        s.frozen = [not p.bn.training for p in st.parts]
        sync = self.bn_sync is not None
        if sync:
            self._bn_sync_stats(st, s, z, hw)
        for i, p in enumerate(st.parts):
            bn = p.bn
            if s.frozen[i]:
                # nn.BatchNorm2d in eval() mode inside a training net: running statistics, no update
                mean_t, var_t = bn.running_mean, bn.running_var
            else:
                mean_t, var_t = s.mean[i], s.var[i]
                if not sync:
                    self._reduce('ct_bn_train_stats', 'ct_bn_train_stats_det',
                                 (z.data_ptr(), B, z.shape[1], off, p.cout, hw, mean_t.data_ptr(), var_t.data_ptr(), float(bn.momentum),
                                  bn.running_mean.data_ptr(), bn.running_var.data_ptr()), s, i, st.name + ' bn stats')
            res = self.bufs[st.res] if st.res is not None else None
            _lib.check(lib.ct_bn_train_apply(
                z.data_ptr(), mean_t.data_ptr(), var_t.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), float(bn.eps),
                int(p.relu), None, res.data_ptr() if res is not None else None, res.shape[1] if res is not None else 0,
                st.res_coff, float(st.res_scale), dst.data_ptr(), dst.shape[1], st.dst_coff + off, z.shape[1], off, B, p.cout, hw,
                self._s()), st.name + ' bn apply')
            off += p.cout

    def _sync_parts(self, st, s):
        """(k, part index, part, channel offset) of the unfrozen parts of a synchronized stage, k counting them."""
        live = [i for i, f in enumerate(s.frozen) if not f]
        if live != s.sync_parts:
            raise _lib.CtdetError('%s: BatchNorm layers moved between train() and eval() since enable_bn_sync(); call it again '
                                  '(on every rank)' % st.name)
        offs = [sum(p.cout for p in st.parts[:i]) for i in live]
        return [(k, i, st.parts[i], offs[k]) for k, i in enumerate(live)]

    def _bn_sync_stats(self, st, s, z, hw):
        """Forward statistics of a synchronized stage: local sums of every unfrozen part, one all-reduce, finish with the global
        count (mean / var / running statistics as ct_bn_train_stats writes them)."""
        lib, B, sy = self.lib, self.batch, self.bn_sync
        parts = self._sync_parts(st, s)
        if not parts:
            return
        view = sy.forward_view(st.name)
        for k, i, p, off in parts:
            t = s.sync_scratch[i]
            _lib.check(lib.ct_bn_sync_stats_local(z.data_ptr(), B, z.shape[1], off, p.cout, hw, sy.part(view, st.name, k).data_ptr(),
                                                  t.data_ptr(), t.numel() * 8, self._s()), st.name + ' bn sync stats')
        sy.reduce_forward(st.name)
        count = float(sy.global_batch * hw)
        for k, i, p, off in parts:
            bn = p.bn
            _lib.check(lib.ct_bn_sync_stats_finish(sy.part(view, st.name, k).data_ptr(), count, p.cout, s.mean[i].data_ptr(),
                                                   s.var[i].data_ptr(), float(bn.momentum), bn.running_mean.data_ptr(),
                                                   bn.running_var.data_ptr(), self._s()), st.name + ' bn sync finish')

    def _scratch(self, s, i):
        """The scratch arguments of part i's reduction: the BatchNorm scratch, or in deterministic mode the part's slab slice and
        its size in bytes."""
        if not self.det:
            return (s.scratch[i].data_ptr(),)
        t = s.det_scratch[i]
        return t.data_ptr(), t.numel() * 8

    def _reduce(self, plain, det, args, s, i, what, det_args=()):
        """Call the reduction entry `plain`, or in deterministic mode its twin `det`, for part i of state s.
        Both take `args` first and the stream last.  Between them:
          det entry:               `det_args`, then the slab pointer and its bytes
          plain BatchNorm entry:   the scratch pointer
          plain bias entry:        nothing
        `det_args` is what only the twin takes ahead of the slab (the heads' null dz_absmax)."""
        if self.det:
            name, tail = det, det_args + self._scratch(s, i)
        else:
            name, tail = plain, self._scratch(s, i) if s.is_bn else ()
        _lib.check(getattr(self.lib, name)(*args, *tail, self._s()), what)

    def policy_record(self):
        """What shaped this runtime's training launches, resolved to what is in force (tools/train_bench.py prints it as `policy`):
        the deterministic mode, the weight-gradient routes by layer count, the bytes of the mode's workspaces."""
        routes = {}
        for s in self.state.values():
            routes[s.wgrad_route.name] = routes.get(s.wgrad_route.name, 0) + 1
        det_bytes = None
        if self.det:
            det_bytes = {'wgrad_wsdet': self.wgrad_wsdet.numel(), 'det_scratch': self.det_scratch.numel() * 8}
            if self.det_ctx and self.ctx is not None:
                det_bytes['ctx_slabs'] = self.ctx.slab_bytes        # behind the plain carve of the block's workspace
        return {
            'deterministic': self.det,
            'deterministic_ctx': self.det_ctx,
            'wgrad_routes': dict(sorted(routes.items())),
            'det_workspace_bytes': det_bytes,
        }

    # ------------------------------------------------------------------ backward
    def backward(self, dloc, dconf, dobj):
        lib, B = self.lib, self.batch
        ctx_grads = None
        if self.used_ctx:
            # Context-Transformer block: gradient of its output -> gradient of the raw conf logits
            d = self.net.num_classes
            conf3 = self.bufs['conf'].view(B, self.P, d)
            dc, dpool, ctx_grads = self.ctx.backward(conf3, self.bufs['pool'].view(B, self.plan.M, d), self._ctx_tensors(),
                                                     dconf.contiguous().view(B, self.P, -1))
            dconf = dc.view(B, -1)
            dpool = dpool.view(B, -1)
            for st in self.plan.steps:
                if st.kind == 'ctxpool':
                    ops.ctx_pool_bwd(self.bufs['conf'], st.src_base, dpool, st.dst_base, dconf, B, st.h, st.w, st.ch, st.k)
        flat = {'loc': dloc.contiguous().view(B, -1), 'conf': dconf.contiguous().view(B, -1), 'obj': dobj.contiguous().view(B, -1)}
        written = {}

        def overlaps(name, c0, c1):
            return any(a < c1 and c0 < b for a, b in written.get(name, []))

        grads_out = [None] * len(self.params)
        main = torch.cuda.current_stream(self.be.device)
        side = self.wg_stream
        if self.prezero:
            # three memsets for the whole pass: gradient arena (bias / split weight gradients accumulate into it),
            # BatchNorm reduction scratch, Winograd weight-gradient workspaces
            self.arena.zero_()
            self.bn_scratch.zero_()
            self.wgrad_ws_all.zero_()
        if side is not None:
            side.wait_stream(main)
        join = (lambda: main.wait_stream(side)) if side is not None else None
        bk = self.bucketer
        if bk is not None:
            bk.begin()

        def put(prm, g):
            i = self._prod_index[id(prm)]
            v = self._arena_view(prm)
            if g.data_ptr() != v.data_ptr():        # produced elsewhere (Context-Transformer block): stage it
                v.copy_(g.reshape(v.shape))
            if bk is not None:                      # all-reduce per bucket as soon as its last gradient exists;
                bk.ready(i, join)                   # the collective is ordered after BOTH streams

        if ctx_grads is not None:
            for k, prm in self.ctx_params.items():
                put(prm, ctx_grads[k])
        _lib.check(lib.ct_scratch_prezeroed(int(self.prezero)), 'ct_scratch_prezeroed')
        try:
            self._backward_steps(flat, written, overlaps, put, main, side)
        finally:
            lib.ct_scratch_prezeroed(0)
        if side is not None:
            main.wait_stream(side)
        if bk is not None:
            bk.finish()
        snap = self.arena.clone()                   # the arena is rewritten by the next backward
        for prm in self.params:
            grads_out[self._pindex[id(prm)]] = self._arena_view(prm, snap)
        return grads_out

    def _backward_steps(self, flat, written, overlaps, put, main, side):
        """Reverse walk over the plan: the pools; per fused conv the epilogue gradient, the weight gradient (side stream) and the
        data gradient."""
        for st in reversed(self.plan.steps):
            if st.kind == 'pool':
                self._pool_backward(st, written, overlaps)
            elif st.kind == 'conv':
                s = self.state[st.name]
                self._epilogue_backward(st, s, flat, written, overlaps, put)
                self._launch_wgrad(st, s, put, main, side)
                if s.dgrad is not None:
                    self._launch_dgrad(st, s, written, overlaps)

    def _pool_backward(self, st, written, overlaps):
        lib, B = self.lib, self.batch
        acc = overlaps(st.src, 0, st.ch)
        if st.name in self._pool_bwd and not acc:       # fused with its producer's bias / ReLU backward (_find_fused_pool_bwd)
            pr = self._pool_bwd[st.name]
            sp = self.state[pr.name]
            y = self.bufs[pr.dst]
            self._reduce('ct_maxpool2x2_bias_relu_bwd', 'ct_maxpool2x2_bias_relu_bwd_det',
                         (y.data_ptr(), y.shape[1], pr.dst_coff, self.grads[st.dst].data_ptr(), B, st.ch, st.h, st.w, st.oh, st.ow,
                          sp.dz.data_ptr(), sp.zc, 0, sp.dbias[0].data_ptr(), sp.dz_amax), sp, 0, st.name + ' + ' + pr.name + ' bias bwd')
            sp.dz_from_pool = True
            return
        _lib.check(lib.ct_maxpool2d_bwd(self.bufs[st.src].data_ptr(), self.grads[st.dst].data_ptr(), self.grads[st.src].data_ptr(),
                                        B * st.ch, st.h, st.w, st.oh, st.ow, st.k, st.stride, st.pad, int(acc), self._s()), st.name)
        written.setdefault(st.src, []).append((0, st.ch))

    def _epilogue_backward(self, st, s, flat, written, overlaps, put):
        """dZ of the fused conv and the gradients of its epilogue parameters: the heads gather the flattened gradients, the others
        go through the BatchNorm or the bias / ReLU backward."""
        lib, B = self.lib, self.batch
        hw, ctot = st.oh * st.ow, s.zc          # channel stride of dZ (st.cout, padded for the heads)
        if st.segs:
            segs = (_lib.OutSegment * 3)()
            for g, sg in enumerate(st.segs):
                t = flat[sg.dst]
                segs[g].ptr = t.data_ptr()
                segs[g].co_begin, segs[g].co_end, segs[g].pix_stride = sg.co_begin, sg.co_end, sg.pix_stride
                segs[g].img_stride, segs[g].base = t.shape[1], sg.base
            _lib.check(lib.ct_head_grad_gather(segs, len(st.segs), B, ctot, hw, s.dz.data_ptr(), self._s()),
                       st.name + ' head gather')
            off = 0
            for i, p in enumerate(st.parts):
                # no maxima wanted: the plain entry is the one without dz_absmax, the twin takes a null one
                self._reduce('ct_bias_act_backward', 'ct_bias_act_backward_det',
                             (s.dz.data_ptr(), ctot, off, None, 0, 0, 0, B, p.cout, hw, s.dz.data_ptr(), ctot, off, s.dbias[i].data_ptr()),
                             s, i, st.name + ' bias bwd', det_args=(None,))
                put(p.bias, s.dbias[i])
                off += p.cout
            return
        gy, y = self.grads[st.dst], self.bufs[st.dst]
        off = 0
        sync = s.is_bn and self.bn_sync is not None
        if sync:
            self._bn_sync_backward_sums(st, s, gy, y, hw, ctot)
        for i, p in enumerate(st.parts):
            if s.is_bn:
                z = self.bufs[s.fwd.dst]
                dres, dres_ctot, dres_acc = None, 0, 0
                if st.res is not None:
                    dr = self.grads[st.res]
                    dres, dres_ctot = dr.data_ptr(), dr.shape[1]
                    dres_acc = int(overlaps(st.res, st.res_coff, st.res_coff + p.cout))
                    written.setdefault(st.res, []).append((st.res_coff, st.res_coff + p.cout))
                frozen = s.frozen[i]
                mean_t, var_t = (p.bn.running_mean, p.bn.running_var) if frozen else (s.mean[i], s.var[i])
                fn = 'ct_bn_eval_backward' if frozen else 'ct_bn_train_backward'
                args = (gy.data_ptr(), gy.shape[1], st.dst_coff + off, y.data_ptr(), y.shape[1], st.dst_coff + off, z.data_ptr(),
                        mean_t.data_ptr(), var_t.data_ptr(), p.bn.weight.data_ptr(), float(p.bn.eps), int(p.relu), None,
                        float(st.res_scale), dres, dres_ctot, st.res_coff, dres_acc, s.dz.data_ptr())
                if sync and not frozen:             # dgamma / dbeta: the local sums (_bn_sync_backward_sums); dz from the global ones
                    sy = self.bn_sync
                    sums = sy.part(sy.backward_view(st.name), st.name, s.sync_parts.index(i))
                    _lib.check(lib.ct_bn_sync_backward_apply(*args, ctot, off, B, p.cout, hw, sums.data_ptr(),
                                                             float(sy.global_batch * hw), self._s()), st.name + ' bn sync bwd')
                else:
                    self._reduce(fn, fn + '_det', args + (s.dgamma[i].data_ptr(), s.dbeta[i].data_ptr(), ctot, off, B, p.cout, hw),
                                 s, i, st.name + ' bn bwd')
                put(p.bn.weight, s.dgamma[i])
                put(p.bn.bias, s.dbeta[i])
            else:
                if s.dz_from_pool:
                    s.dz_from_pool = False          # dZ and dbias came from the pool's fused backward (_pool_backward)
                else:
                    self._reduce('ct_bias_act_backward_amax', 'ct_bias_act_backward_det',
                                 (gy.data_ptr(), gy.shape[1], st.dst_coff + off, y.data_ptr(), y.shape[1], st.dst_coff + off, int(p.relu), B,
                                  p.cout, hw, s.dz.data_ptr(), ctot, off, s.dbias[i].data_ptr() if p.bias is not None else None, s.dz_amax),
                                 s, i, st.name + ' bias bwd')
                if p.bias is not None:
                    put(p.bias, s.dbias[i])
            off += p.cout

    def _bn_sync_backward_sums(self, st, s, gy, y, hw, ctot):
        """Backward sums of a synchronized stage: per unfrozen part the local sum g / sum g*xhat (with the global mean / var) and
        the local dgamma / dbeta, then one all-reduce of the stage's view."""
        lib, B, sy = self.lib, self.batch, self.bn_sync
        parts = self._sync_parts(st, s)
        if not parts:
            return
        z, view = self.bufs[s.fwd.dst], sy.backward_view(st.name)
        for k, i, p, off in parts:
            t = s.sync_scratch[i]
            _lib.check(lib.ct_bn_sync_backward_local(
                gy.data_ptr(), gy.shape[1], st.dst_coff + off, y.data_ptr(), y.shape[1], st.dst_coff + off, z.data_ptr(),
                s.mean[i].data_ptr(), s.var[i].data_ptr(), float(p.bn.eps), int(p.relu), None, float(st.res_scale), ctot, off, B,
                p.cout, hw, sy.part(view, st.name, k).data_ptr(), s.dgamma[i].data_ptr(), s.dbeta[i].data_ptr(), t.data_ptr(),
                t.numel() * 8, self._s()), st.name + ' bn sync bwd sums')
        sy.reduce_backward(st.name)

    def _launch_wgrad(self, st, s, put, main, side):
        """Weight gradient of the fused conv, split back to its parts.  Nothing downstream in this backward pass reads it, so it
        runs on the side stream next to the data-gradient chain (dz ready -> side stream)."""
        if side is not None:
            s.ev_dz.record(main)
            side.wait_event(s.ev_dz)
        with torch.cuda.stream(side if side is not None else main):
            r = s.wgrad_route
            ws = None if r.ws is None else s.wgrad_ws if r.zeroed and self.prezero else getattr(self, r.ws)
            if r.dz_amax:
                # X's maxima where the forward wired a slot for this layer's input, dZ's where ct_bias_act_backward_amax
                # wrote them (a BatchNorm backward does not track: NULL, the entry point takes the maximum itself)
                s.wgrad.in_absmax = s.fwd.rt['desc'].in_absmax
            _lib.check(r.run(self.lib, s.wgrad, s.dz, s.zc, s.dw, ws, None if s.is_bn or st.segs else s.dz_amax, self._s()),
                       st.name + r.label)
        off = 0
        for p in st.parts:
            put(p.weight, s.dw[off:off + p.cout])
            off += p.cout

    def _launch_dgrad(self, st, s, written, overlaps):
        """Data gradient into the producer's gradient buffer (accumulate, through the residual input, if already written)."""
        lib = self.lib
        acc = overlaps(st.src, st.src_coff, st.src_coff + st.cin)
        if not self.switches.pack_batch:
            self._pack_dgrad(st, s)
        res = self.grads[st.src].data_ptr() if acc else None
        if s.dgrad_wino is not None:
            s.dgrad_wino.res = res
            f = FORMS[s.dgrad_tile]
            d = s.dgrad_wino
            if f.split and st.dil > 1 and acc:      # the dilated output transform has no accumulate: through a scratch tensor
                g = self.grads[st.src]
                tmp = torch.empty((g.shape[0], st.cin, st.h, st.w), device=g.device)
                d = _lib.ConvDesc.from_buffer_copy(s.dgrad_wino)
                d.res, d.out, d.out_ctot, d.out_coff = None, tmp.data_ptr(), st.cin, 0
            _lib.check(f.run(lib, C.byref(d), s.U_d.data_ptr(), self.dgrad_ws4s, None, self._s()),
                       st.name + ' dgrad (%s)' % f.name)
            if d is not s.dgrad_wino:
                g[:, st.src_coff:st.src_coff + st.cin] += tmp
        else:
            s.dgrad.res = res
            if s.dgrad_x3 is not None:
                _lib.check(lib.ct_conv2d_x3_fwd(C.byref(s.dgrad), s.wx3_d.data_ptr(), s.dgrad_x3, self._s()),
                           st.name + ' dgrad (bf16x3)')
            else:
                _lib.check(lib.ct_conv2d_fwd(C.byref(s.dgrad), self._s()), st.name + ' dgrad')
        written.setdefault(st.src, []).append((st.src_coff, st.src_coff + st.cin))


class BackboneFunction(torch.autograd.Function):
    """(x, *params) -> (loc, conf, obj) flattened head outputs, differentiable w.r.t. the parameters."""

    @staticmethod
    def forward(ctx, rt, x, use_ctx, *params):
        ctx.rt = rt
        loc, conf, obj = rt.forward(x, use_ctx)
        ctx.generation = rt.generation
        return loc.clone(), conf.clone(), obj.clone()

    @staticmethod
    def backward(ctx, dloc, dconf, dobj):
        if ctx.rt.generation != ctx.generation:
            # the activations / BatchNorm statistics this backward needs live in buffers the runtime reuses
            raise _lib.CtdetError(
                'RFBNet training runtime: backward() of forward #%d called after forward #%d overwrote its saved '
                'activations; run loss.backward() before the next model(x) of the same batch size (the engine keeps '
                'one set of activation buffers per batch size)' % (ctx.generation, ctx.rt.generation))
        grads = ctx.rt.backward(dloc, dconf, dobj)
        return (None, None, None) + tuple(grads)
