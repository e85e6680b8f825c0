"""Inference engine: turns an RFBNet module tree into a flat list of fused HIP launches.

The plan is built once per (network, batch size): every launch owns pre-packed weights,
folded epilogue vectors and pre-allocated activation buffers, so a forward pass is a
straight sequence of `ct_conv2d_fwd` / `ct_maxpool2d_fwd` / ... calls on the current HIP
stream with no allocation and no host synchronisation (and can be captured in a hipGraph).

Fusions relative to the reference's op-by-op PyTorch execution (models/RFB_Net_vgg.py):
  * Conv2d + bias/BatchNorm(eval) + ReLU                      -> one launch (:7-22, :332-336)
  * the parallel 1x1 "reduce" convs of an RFB block + shortcut -> one launch, per-channel ReLU
    mask (:33-50, :75-97)
  * torch.cat of the branches                                  -> branch convs write channel
    slices of one buffer (:58, :106)
  * ConvLinear + `out*scale + short` + ReLU                    -> one launch (:59-62, :107-110)
  * loc/conf/obj head convs + permute + view + cat             -> one launch per source writing
    the flattened [B,P*4] / [B,P*C] / [B,P*2] buffers directly (:238-248)
  * the conf head is evaluated once (the reference runs it twice in phase 2, :240/:243).

The `backend` indirection exists so tests can replay a plan with a torch-CPU emulation of the
launch descriptors (tests/emu_backend.py) and check the wiring without a GPU; the product
ships exactly one backend, the HIP one, and `RFBNet.forward` refuses non-HIP devices.
"""
import ctypes as C
import dataclasses
import json
import math
import os
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from . import _lib, conv_policy
from .conv_policy import (CTX_DIL_W4S_DEFAULT, CTX_F4_MAX_CIN_DEFAULT, CTX_F4_TILE_DEFAULT, CTX_TILES_DEFAULT,  # noqa: F401
                          CTX_W4S_MIN_CIN_DEFAULT, F4_TILES, H2_MIN_PIXELS, H2_OF_TILE, WINO4F_TILES, WINO4S_TILES, WINO_NAME)
from .wino_forms import FORMS, geometry_ok

# CTDET_TUNE_TABLE: another table file (A/B measurements of a re-tuned table against the committed one)
TUNE_TABLE = os.environ.get('CTDET_TUNE_TABLE') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_tune_gfx950.json')
_tune_table = None


def tune_table():
    """Committed per-shape tile choices measured on an MI355X by tools/tune_convs.py."""
    global _tune_table
    if _tune_table is None:
        try:
            with open(TUNE_TABLE) as f:
                _tune_table = json.load(f)
        except (OSError, ValueError):
            _tune_table = {}
    return _tune_table


CTX_POOL = {300: [3, 2, 2, 2, 1, 1],           # models/RFB_Net_vgg.py:235-236
            512: [3, 2, 2, 2, 2, 1, 1]}        # build-defined: the reference crashes at 512 (:243)


def conv_out(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def pool_out(n, k, s, p, ceil_mode):
    num = n + 2 * p - k
    o = (-(-num // s) if ceil_mode else num // s) + 1
    if ceil_mode and (o - 1) * s >= n + p:
        o -= 1
    return o


@dataclass
class ConvPart:
    """One torch conv folded into a fused launch: weight [cout,cin,kh,kw] + its epilogue source."""
    weight: torch.nn.Parameter
    bias: Optional[torch.nn.Parameter] = None
    bn: Optional[torch.nn.Module] = None
    relu: bool = False

    @property
    def cout(self):
        return self.weight.shape[0]


@dataclass
class Segment:
    dst: str            # flat buffer name [B, img_stride]
    co_begin: int
    co_end: int
    pix_stride: int
    base: int


@dataclass
class ConvStep:
    name: str
    parts: List[ConvPart]
    cin: int
    kh: int
    kw: int
    stride: int
    ph: int
    pw: int
    dil: int
    src: str
    src_coff: int
    h: int
    w: int
    dst: Optional[str] = None
    dst_coff: int = 0
    res: Optional[str] = None
    res_coff: int = 0
    res_scale: float = 1.0
    segs: Optional[List[Segment]] = None
    kind: str = 'conv'
    rt: dict = field(default_factory=dict)      # backend-private runtime state

    @property
    def cout(self):
        return sum(p.cout for p in self.parts)

    @property
    def oh(self):
        return conv_out(self.h, self.kh, self.stride, self.ph, self.dil)

    @property
    def ow(self):
        return conv_out(self.w, self.kw, self.stride, self.pw, self.dil)

    def flops(self, batch):
        return 2.0 * batch * self.cout * self.oh * self.ow * self.cin * self.kh * self.kw

    def tune_key(self, batch):
        return '%dx%d_s%d_d%d_c%d_m%d_%dx%d_b%d%s' % (self.kh, self.kw, self.stride, self.dil, self.cin,
                                                    self.cout, self.h, self.w, batch, '_seg' if self.segs else '')


@dataclass
class PoolStep:
    name: str
    src: str
    dst: str
    ch: int
    h: int
    w: int
    k: int
    stride: int
    pad: int
    ceil_mode: bool
    kind: str = 'pool'

    @property
    def oh(self):
        return pool_out(self.h, self.k, self.stride, self.pad, self.ceil_mode)

    @property
    def ow(self):
        return pool_out(self.w, self.k, self.stride, self.pad, self.ceil_mode)


@dataclass
class CtxPoolStep:
    name: str
    src: str            # flat conf buffer
    src_base: int
    dst: str            # flat pooled buffer
    dst_base: int
    h: int
    w: int
    ch: int
    k: int
    kind: str = 'ctxpool'


class Plan:
    """Flat launch list + buffer table for one (network, batch)."""

    def __init__(self, net, batch):
        self.net = net
        self.batch = batch
        self.size = net.size
        self.C = net.num_classes
        self.ctx = (net.method == 'ours' and net.phase == 2)
        self.steps = []
        self.buf_shapes = {}          # name -> shape tuple (without batch for 4D: (C,H,W); flat: (n,))
        self._build()

    # -- buffer helpers
    def _buf4(self, name, c, h, w):
        self.buf_shapes[name] = (c, h, w)
        return name

    def _flat(self, name, n):
        self.buf_shapes[name] = (n,)
        return name

    def _conv(self, name, parts, src, src_c, h, w, k, stride=1, pad=0, dil=1, src_coff=0, cin=None,
              dst=None, dst_c=None, dst_coff=0, res=None, res_coff=0, res_scale=1.0):
        kh, kw = (k, k) if isinstance(k, int) else k
        ph, pw = (pad, pad) if isinstance(pad, int) else pad
        st = ConvStep(name, parts, cin if cin is not None else src_c, kh, kw, stride, ph, pw, dil,
                      src, src_coff, h, w, dst, dst_coff, res, res_coff, res_scale)
        if dst is not None and dst not in self.buf_shapes:
            self._buf4(dst, dst_c if dst_c is not None else st.cout, st.oh, st.ow)
        self.steps.append(st)
        return st

    @staticmethod
    def _bc(m, relu=None):
        """ConvPart of a BasicConv module (conv without bias + BN [+ ReLU])."""
        return ConvPart(m.conv.weight, None, m.bn, m.relu if relu is None else relu)

    # -- network walk (models/RFB_Net_vgg.py:219-248)
    def _build(self):
        net, S = self.net, self.size
        self._buf4('x', 3, S, S)
        cur, c, h, w = 'x', 3, S, S
        sources = []
        k = 0
        nbase = len(net.base)
        while k < nbase:
            m = net.base[k]
            if isinstance(m, torch.nn.Conv2d):
                relu = k + 1 < nbase and isinstance(net.base[k + 1], torch.nn.ReLU)
                st = self._conv('base.%d' % k, [ConvPart(m.weight, m.bias, None, relu)], cur, c, h, w,
                                m.kernel_size, m.stride[0], m.padding, m.dilation[0], dst='a_base%d' % k)
                cur, c, h, w = st.dst, st.cout, st.oh, st.ow
                k += 2 if relu else 1
                if k == 23:
                    sources.append(self._rfb_a('Norm', net.Norm, cur, c, h, w))
            elif isinstance(m, torch.nn.MaxPool2d):
                ps = PoolStep('base.%d' % k, cur, 'a_base%d' % k, c, h, w, m.kernel_size, m.stride, m.padding,
                              m.ceil_mode)
                self._buf4(ps.dst, c, ps.oh, ps.ow)
                self.steps.append(ps)
                cur, h, w = ps.dst, ps.oh, ps.ow
                k += 1
            else:
                raise TypeError('unexpected module in base: %r' % m)
        indicator = net.indicator
        for i, m in enumerate(net.extras):
            name = 'extras.%d' % i
            if hasattr(m, 'branch0'):
                cur, c, h, w = self._rfb(name, m, cur, c, h, w)
            else:
                st = self._conv(name, [self._bc(m)], cur, c, h, w, m.conv.kernel_size, m.conv.stride[0],
                                m.conv.padding, m.conv.dilation[0], dst='a_' + name)
                cur, c, h, w = st.dst, st.cout, st.oh, st.ow
            if i < indicator or i % 2 == 0:
                sources.append((cur, c, h, w))
        # heads
        mbox = [l.out_channels // 4 for l in net.loc]
        assert len(mbox) == len(sources)
        C = self.C
        self.P = sum(hh * ww * mb for (_, _, hh, ww), mb in zip(sources, mbox))
        self._flat('loc', self.P * 4)
        self._flat('conf', self.P * C)
        self._flat('obj', self.P * 2)
        self.src_info = []
        pbase = 0
        for i, ((sname, sc, sh, sw), mb) in enumerate(zip(sources, mbox)):
            parts = [ConvPart(net.loc[i].weight, net.loc[i].bias), ConvPart(net.conf[i].weight, net.conf[i].bias),
                     ConvPart(net.obj[i].weight, net.obj[i].bias)]
            st = self._conv('head.%d' % i, parts, sname, sc, sh, sw, 3, 1, 1, 1)
            st.segs = [Segment('loc', 0, mb * 4, mb * 4, pbase * 4),
                       Segment('conf', mb * 4, mb * 4 + mb * C, mb * C, pbase * C),
                       Segment('obj', mb * (4 + C), mb * (6 + C), mb * 2, pbase * 2)]
            self.src_info.append((sh, sw, mb, pbase))
            pbase += sh * sw * mb
        if self.ctx:
            kk = CTX_POOL[S]
            assert len(kk) == len(sources)
            self.M = sum(-(-sh // kv) * -(-sw // kv) * mb for (sh, sw, mb, _), kv in zip(self.src_info, kk))
            self._flat('pool', self.M * C)
            mbase = 0
            for i, ((sh, sw, mb, pb), kv) in enumerate(zip(self.src_info, kk)):
                self.steps.append(CtxPoolStep('ctxpool.%d' % i, 'conf', pb * C, 'pool', mbase * C, sh, sw, mb * C, kv))
                mbase += -(-sh // kv) * -(-sw // kv) * mb

    def _rfb_a(self, name, m, src, c, h, w):
        """BasicRFB_a (models/RFB_Net_vgg.py:68-112)."""
        b0, b1, b2, b3 = m.branch0, m.branch1, m.branch2, m.branch3
        i0, i1, i2, i3 = b0[0].out_channels, b1[0].out_channels, b2[0].out_channels, b3[0].out_channels
        co = m.shortcut.out_channels
        t0 = name + '.t0'
        self._conv(name + '.reduce', [self._bc(b0[0]), self._bc(b1[0]), self._bc(b2[0]), self._bc(b3[0]),
                                      self._bc(m.shortcut)], src, c, h, w, 1, dst=t0)
        cat = name + '.cat'
        ccat = b0[1].out_channels + b1[2].out_channels + b2[2].out_channels + b3[3].out_channels
        self._buf4(cat, ccat, h, w)
        off = 0
        self._conv(name + '.b0.1', [self._bc(b0[1])], t0, i0, h, w, 3, 1, 1, 1, src_coff=0, dst=cat, dst_coff=off)
        off += b0[1].out_channels
        self._conv(name + '.b1.1', [self._bc(b1[1])], t0, i1, h, w, (3, 1), 1, (1, 0), 1, src_coff=i0, dst=name + '.t1')
        self._conv(name + '.b1.2', [self._bc(b1[2])], name + '.t1', b1[1].out_channels, h, w, 3, 1, 3, 3, dst=cat, dst_coff=off)
        off += b1[2].out_channels
        self._conv(name + '.b2.1', [self._bc(b2[1])], t0, i2, h, w, (1, 3), 1, (0, 1), 1, src_coff=i0 + i1, dst=name + '.t2')
        self._conv(name + '.b2.2', [self._bc(b2[2])], name + '.t2', b2[1].out_channels, h, w, 3, 1, 3, 3, dst=cat, dst_coff=off)
        off += b2[2].out_channels
        self._conv(name + '.b3.1', [self._bc(b3[1])], t0, i3, h, w, (1, 3), 1, (0, 1), 1, src_coff=i0 + i1 + i2, dst=name + '.t3a')
        self._conv(name + '.b3.2', [self._bc(b3[2])], name + '.t3a', b3[1].out_channels, h, w, (3, 1), 1, (1, 0), 1, dst=name + '.t3b')
        self._conv(name + '.b3.3', [self._bc(b3[3])], name + '.t3b', b3[2].out_channels, h, w, 3, 1, 5, 5, dst=cat, dst_coff=off)
        out = name + '.out'
        # out = relu(ConvLinear(cat)*scale + shortcut(x))   (:107-110)
        self._conv(name + '.linear', [self._bc(m.ConvLinear, relu=True)], cat, ccat, h, w, 1, dst=out,
                   res=t0, res_coff=i0 + i1 + i2 + i3, res_scale=float(m.scale))
        return out, co, h, w

    def _rfb(self, name, m, src, c, h, w):
        """BasicRFB (models/RFB_Net_vgg.py:26-64)."""
        b0, b1, b2 = m.branch0, m.branch1, m.branch2
        s = b0[0].conv.stride[0]
        c0, c1, c2 = b0[0].out_channels, b1[0].out_channels, b2[0].out_channels
        co = m.shortcut.out_channels
        v0, v1, v2 = b0[1].conv.dilation[0], b1[2].conv.dilation[0], b2[3].conv.dilation[0]
        if s == 1:
            t0 = name + '.t0'
            self._conv(name + '.reduce', [self._bc(b0[0]), self._bc(b1[0]), self._bc(b2[0]), self._bc(m.shortcut)],
                       src, c, h, w, 1, dst=t0)
            b0src, b0off, b12src, b1off, b2off = t0, 0, t0, c0, c0 + c1
            shsrc, shoff = t0, c0 + c1 + c2
            ho, wo = h, w
        else:
            ta, tb = name + '.ta', name + '.tb'
            self._conv(name + '.reduce1', [self._bc(b1[0]), self._bc(b2[0])], src, c, h, w, 1, dst=ta)
            st = self._conv(name + '.reduce2', [self._bc(b0[0]), self._bc(m.shortcut)], src, c, h, w, 1, s, dst=tb)
            b0src, b0off, b12src, b1off, b2off = tb, 0, ta, 0, c1
            shsrc, shoff = tb, c0
            ho, wo = st.oh, st.ow
        cat = name + '.cat'
        ccat = b0[1].out_channels + b1[2].out_channels + b2[3].out_channels
        self._buf4(cat, ccat, ho, wo)
        off = 0
        self._conv(name + '.b0.1', [self._bc(b0[1])], b0src, c0, ho, wo, 3, 1, v0, v0, src_coff=b0off, dst=cat, dst_coff=off)
        off += b0[1].out_channels
        self._conv(name + '.b1.1', [self._bc(b1[1])], b12src, c1, h, w, 3, s, 1, 1, src_coff=b1off, dst=name + '.t1')
        self._conv(name + '.b1.2', [self._bc(b1[2])], name + '.t1', b1[1].out_channels, ho, wo, 3, 1, v1, v1, dst=cat, dst_coff=off)
        off += b1[2].out_channels
        self._conv(name + '.b2.1', [self._bc(b2[1])], b12src, c2, h, w, 3, 1, 1, 1, src_coff=b2off, dst=name + '.t2a')
        self._conv(name + '.b2.2', [self._bc(b2[2])], name + '.t2a', b2[1].out_channels, h, w, 3, s, 1, 1, dst=name + '.t2b')
        self._conv(name + '.b2.3', [self._bc(b2[3])], name + '.t2b', b2[2].out_channels, ho, wo, 3, 1, v2, v2, dst=cat, dst_coff=off)
        out = name + '.out'
        self._conv(name + '.linear', [self._bc(m.ConvLinear, relu=True)], cat, ccat, ho, wo, 1, dst=out,
                   res=shsrc, res_coff=shoff, res_scale=float(m.scale))
        return out, co, ho, wo

    def conv_flops(self):
        return sum(s.flops(self.batch) for s in self.steps if s.kind == 'conv')


# ======================================================================================
# ConvStep.rt['config'] values selecting a Winograd kernel, and the st.rt['wino'] codes they select (wino_forms.FORMS)
WINO, WINO4, WINOX, WINO4S, WINO4F, WINO4H, WINO4FH = (FORMS[c].config for c in (2, 4, 23, 44, 46, 47, 48))
WINO_TILE = {f.config: c for c, f in FORMS.items()}
H2_TILES = tuple(c for c, f in FORMS.items() if f.h2)


def weight_parts(parts, zero_w=None):
    """The weights of a fused conv as the pack entry points take them: (pointer array, cout array, n) over its parts, plus the rows
    of zero_w where a data gradient pads dZ's channels with zeros."""
    wts = [(p.weight.detach().data_ptr(), p.cout) for p in parts]
    if zero_w is not None:
        wts.append((zero_w.data_ptr(), zero_w.shape[0]))
    return (C.c_void_p * len(wts))(*[w for w, _ in wts]), (C.c_int * len(wts))(*[c for _, c in wts]), len(wts)


class HipBackend:
    """Executes plan steps through libctdet (the only backend the product ships)."""
    # The kernel policy (ctdet/conv_policy.py).  A Runtime / TrainRuntime assigns the one it resolved for its network and batch
    # before it prepares the first layer; a backend no runtime has bound (kernel tests, tools/) resolves the default from the
    # environment at each use.
    _policy = None
    _kernels = None

    @property
    def policy(self):
        return self._policy if self._policy is not None else conv_policy.resolve(None, None, os.environ)

    @policy.setter
    def policy(self, p):
        self._policy = p

    h2 = property(lambda self: self.policy.h2)
    h2_direct = property(lambda self: self.policy.h2_direct)
    wino_tile_set = property(lambda self: self.policy.tile_set)

    @property
    def kernels(self):
        """The library's kernel lists (conv_policy.Kernels), asked once."""
        if self._kernels is None:
            self._kernels = conv_policy.Kernels.of(self.lib)
        return self._kernels

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.CtdetError('HipBackend needs a HIP device, got %s' % device)
        self.lib = _lib.lib()
        # V / M workspace of the three-kernel Winograd form (csrc/ct_wino4s.hip): ONE buffer per stream of the schedule,
        # sized for the largest layer on it -- launches of a stream run one after another (st.rt['ws_key'] = the stream
        # index the Runtime gave the step, 0 before there is a schedule).  Per-layer buffers were ~6 GB per RFBNet-300
        # runtime at bs 32 and > 10 GB for RFBNet-512.
        self.ws_pool = {}
        self.ws_generation = 0
        # "slots" for the per-image maxima of |activation| (ct_conv_desc.in_absmax / out_absmax, include/ctdet.h: one line per
        # image): rows of one tensor that a runtime zeroes once per step (zero_slots)
        self.slot_pool = None
        self.slots_used = 0
        self.kernel_epoch = 0          # bumped whenever a step changes kernels (enable_wino / enable_x3): a Runtime re-wires its slots

    def new_slot(self, batch):
        """Device pointer of a fresh slot of `batch` lines of CT_ABSMAX_LINE_BYTES."""
        words = batch * _lib.ABSMAX_LINE_BYTES // 4
        if self.slot_pool is None or self.slot_pool.shape[1] < words:
            if self.slots_used:
                raise _lib.CtdetError('absmax slots were handed out for a smaller batch')
            self.slot_pool = torch.zeros((128, words), device=self.device, dtype=torch.int32)
        if self.slots_used >= self.slot_pool.shape[0]:
            raise _lib.CtdetError('out of absmax slots')
        self.slots_used += 1
        return self.slot_pool[self.slots_used - 1].data_ptr()

    def zero_slots(self):
        if self.slot_pool is not None and self.slots_used:
            self.slot_pool[:self.slots_used].zero_()

    def _ws_drop(self, key):
        """Give a workspace back.  Launches on the side streams may still be using it (it was allocated on the caller's stream,
        so the caching allocator would hand the block out again at once), and a captured hipGraph holds its raw pointer: wait
        for the device, and bump the generation a DetectionPipeline keys its graph on."""
        if self.ws_pool.get(key) is not None:
            torch.cuda.synchronize(self.device)
            self.ws_generation += 1
        self.ws_pool[key] = None

    def ws_reserve(self, key, nbytes):
        t = self.ws_pool.get(key)
        if t is None or t.numel() < nbytes:
            self._ws_drop(key)                  # drop the old buffer before allocating the larger one
            self.ws_pool[key] = self.alloc((nbytes,), torch.uint8)

    def ws_rebuild(self, steps):
        """(Re)size the pool to what the given conv steps need, per key; called once the schedule is known."""
        need = {}
        for st in steps:
            if self.uses_ws(st):
                k = st.rt.get('ws_key', 0)
                need[k] = max(need.get(k, 0), st.rt.get('ws4s_bytes', 0))
        for k in list(self.ws_pool):
            if k not in need or self.ws_pool[k] is None or self.ws_pool[k].numel() != need[k]:
                self._ws_drop(k)
        for k, n in need.items():
            if self.ws_pool.get(k) is None:
                self.ws_pool[k] = self.alloc((n,), torch.uint8)

    @staticmethod
    def uses_ws(st):
        """Whether the step's launch takes the shared V / M workspace of its stream."""
        f = FORMS.get(st.rt.get('wino'))
        return f is not None and f.split

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def alloc(self, shape, dtype=torch.float32):
        return torch.empty(shape, device=self.device, dtype=dtype)

    # ---- conv
    def prepare_conv(self, st, bufs, batch):
        lib = self.lib
        kpad = lib.ct_conv_kpad(st.cin, st.kh, st.kw)
        if kpad < 0:
            raise _lib.CtdetError('%s: %dx%d filters are not built' % (st.name, st.kh, st.kw))
        mpad = lib.ct_conv_mpad(st.cout)
        rt = st.rt
        rt['wpk'] = self.alloc((kpad, mpad))
        rt['scale'] = torch.ones(mpad, device=self.device)       # entries past cout stay (1, 0)
        rt['shift'] = torch.zeros(mpad, device=self.device)
        relus = [p.relu for p in st.parts]
        rt['lo'] = self._relu_floor(st, mpad)
        rt['kpad'], rt['mpad'] = kpad, mpad
        self.pack_conv(st)
        d = _lib.ConvDesc()
        src = bufs[st.src]
        d.in_ = src.data_ptr()
        d.batch, d.cin, d.h, d.w = batch, st.cin, st.h, st.w
        d.in_ctot, d.in_coff = src.shape[1], st.src_coff
        d.wpacked, d.scale, d.shift = rt['wpk'].data_ptr(), rt['scale'].data_ptr(), rt['shift'].data_ptr()
        d.cout, d.m_pad, d.k_pad = st.cout, mpad, kpad
        d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = st.kh, st.kw, st.stride, st.ph, st.pw, st.dil
        d.oh, d.ow = st.oh, st.ow
        if st.segs:
            d.nseg = len(st.segs)
            for g, sg in enumerate(st.segs):
                t = bufs[sg.dst]
                d.seg[g].ptr = t.data_ptr()
                d.seg[g].co_begin, d.seg[g].co_end = sg.co_begin, sg.co_end
                d.seg[g].pix_stride = sg.pix_stride
                d.seg[g].img_stride = t.shape[1]
                d.seg[g].base = sg.base
        else:
            dst = bufs[st.dst]
            assert dst.shape[2] == st.oh and dst.shape[3] == st.ow, (st.name, dst.shape, st.oh, st.ow)
            d.out, d.out_ctot, d.out_coff = dst.data_ptr(), dst.shape[1], st.dst_coff
        if st.res is not None:
            r = bufs[st.res]
            d.res, d.res_ctot, d.res_coff, d.res_scale = r.data_ptr(), r.shape[1], st.res_coff, st.res_scale
        d.relu = int(all(relus))
        d.lo = rt['lo'].data_ptr() if rt['lo'] is not None else None
        d.config = max(rt.get('config', 0), 0)
        # split-K workspace for maps that cannot fill the chip (the library decides per launch whether to use it)
        npix = batch * st.oh * st.ow
        if int(os.environ.get('CTDET_KSPLIT', '1')):
            # 16 slabs for the small maps; 4 for the mid-sized 3x3 layers, where only the F(4x4,3x3) kernel splits
            # (over input channels: a 32-tile x 64-cout workgroup grid is 16x coarser than the direct kernel's)
            slabs = 16 if st.cout * npix <= (2 << 20) else \
                4 if st.cout * npix <= (8 << 20) and (st.kh, st.kw, st.stride, st.dil) == (3, 3, 1, 1) else 0
            force = int(os.environ.get('CTDET_FORCE_KSPLIT', '0'))      # accuracy experiments (tools/ctx_parity.py)
            if force > 1:
                slabs = force
            if slabs:
                rt['ksws'] = torch.empty(slabs * st.cout * npix, device=self.device)
                d.ksplit, d.ksplit_ws, d.ksplit_ws_floats = (force if force > 1 else -1), rt['ksws'].data_ptr(), \
                    rt['ksws'].numel()
        rt['desc'] = d
        rt['wino_ok'] = bool(lib.ct_conv_wino_supported(C.byref(d)))
        rt['winox_ok'] = bool(lib.ct_conv_wino_x3_supported(C.byref(d)))
        rt['wino4s_ok'] = bool(lib.ct_conv_wino4s_supported(C.byref(d)))
        rt['wino4f_ok'] = bool(lib.ct_conv_wino4f_supported(C.byref(d)))
        if rt.get('config', 0) in WINO_TILE:
            self.enable_wino(st, tile=WINO_TILE[rt['config']])

    def _relu_floor(self, st, mpad):
        """Per-channel lower clamp of a fused conv whose parts do not agree on ReLU (0 / -inf; None where they do)."""
        relus = [p.relu for p in st.parts]
        if all(relus) or not any(relus):
            return None
        lo = torch.zeros(mpad, device=self.device)
        off = 0
        for p in st.parts:
            lo[off:off + p.cout] = 0.0 if p.relu else -float('inf')
            off += p.cout
        return lo

    def enable_wino(self, st, on=True, tile=None):
        """Route this conv through a Winograd kernel (3x3 s1 d1 p1 layers only): tile 2 = F(2x2,3x3),
        tile 4 = F(4x4,3x3), 23 = F(2x2,3x3) on the bf16 matrix pipe (cin % 16 == 0), 44 / 46 / 47 / 48 = the F(4x4,3x3) forms on the
        16-bit pipe.  st.rt['wino'] holds the code in use."""
        rt = st.rt
        self.kernel_epoch += 1
        if not on:
            rt['wino'] = False
            rt.pop('ws4s_bytes', None)      # the three-kernel form's V / M workspace need (ws_rebuild shrinks the pool)
            if rt.get('wpk_stale'):
                self.pack_conv(st)
            return
        tile = int(tile or 2)
        # the three-kernel form also takes dilated 3x3 layers (pad = dilation: tiles on the sub-lattices), which the fused
        # kernels do not
        if not geometry_ok(rt, tile):
            raise _lib.CtdetError('%s: geometry has no Winograd path' % st.name)
        rt['x3'] = None
        f = FORMS.get(tile)
        if f is None:
            raise _lib.CtdetError('%s: Winograd tile %r (2, 4, 23, 44, 46, 47 or 48)' % (st.name, tile))
        if not f.split:
            rt.pop('ws4s_bytes', None)
        if not rt.get(f.ok):
            raise _lib.CtdetError('%s: geometry has no %s' % (st.name, f.path))
        if f.key not in rt:
            rt[f.key] = f.alloc(self.lib, self.alloc, st.cin, st.cout)
        if f.split:
            rt['ws4s_bytes'] = self.lib.ct_conv_wino4s_workspace_bytes(C.byref(rt['desc']))
            self.ws_reserve(rt.get('ws_key', 0), rt['ws4s_bytes'])
        rt['wino'] = tile
        self._pack_wino(st)

    def _pack_wino(self, st):
        f = FORMS[st.rt['wino']]
        _lib.check(f.pack_weights(self.lib, *weight_parts(st.parts), st.cin, st.rt[f.key].data_ptr(), self._stream()), f.pack)

    def pack_conv(self, st, weights=True):
        """(Re)pack weights and fold the epilogue from the CURRENT parameter values.  weights=False: only the epilogue
        (the training engine re-packs all weights of a step in one batched launch, ct_pack_run)."""
        rt, lib = st.rt, self.lib
        for wt in [p.weight.detach() for p in st.parts]:
            if not (wt.is_cuda and wt.is_contiguous() and wt.dtype == torch.float32):
                raise _lib.CtdetError('%s: parameters must be contiguous fp32 on the HIP device' % st.name)
        if not weights:
            pass
        elif rt.get('wino'):                    # only the layout the launch reads; the other one is packed on demand
            self._pack_wino(st)
            rt['wpk_stale'] = True
        elif rt.get('x3') is not None:
            self._pack_x3(st)
            rt['wpk_stale'] = True
        else:
            _lib.check(lib.ct_conv_pack_weights(*weight_parts(st.parts), st.cin, st.kh, st.kw, rt['wpk'].data_ptr(),
                                                rt['mpad'], rt['kpad'], self._stream()), 'ct_conv_pack_weights')
            rt['wpk_stale'] = False
        self._fold_epilogue(st, first=not rt.get('folded'))
        rt['folded'] = True
        rt['versions'] = self.param_versions(st)

    def _fold_epilogue(self, st, first=True):
        """Fold bias / BatchNorm of every part into the scale / shift vectors (first=False: skip the constant ones)."""
        rt, lib = st.rt, self.lib
        off = 0
        for p in st.parts:
            if not first and p.bn is None and p.bias is None:
                off += p.cout                   # identity epilogue: constant, written by the first call
                continue
            if p.bn is not None:
                bn = p.bn
                args = (bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                        bn.running_var.data_ptr(), float(bn.eps), None)
            else:
                args = (None, None, None, None, 0.0, p.bias.data_ptr() if p.bias is not None else None)
            _lib.check(lib.ct_conv_fold_epilogue(*args, p.cout, off, rt['scale'].data_ptr(),
                                                 rt['shift'].data_ptr(), self._stream()), 'ct_conv_fold_epilogue')
            off += p.cout

    @staticmethod
    def param_versions(st):
        v = []
        for p in st.parts:
            v.append((p.weight.data_ptr(), p.weight._version))
            if p.bias is not None:
                v.append((p.bias.data_ptr(), p.bias._version))
            if p.bn is not None:
                # num_batches_tracked stands in for the running statistics: the training engine updates
                # running_mean / running_var through raw pointers (no version bump) but bumps this counter
                # once per training forward, so an eval runtime re-folds its epilogue after any train step
                for t in (p.bn.weight, p.bn.bias, p.bn.running_mean, p.bn.running_var, p.bn.num_batches_tracked):
                    if t is not None:
                        v.append((t.data_ptr(), t._version))
        return v

    def _own_absmax(self, st):
        """A consumer of ct_conv_desc.in_absmax whose input has no producer-side maximum (a layer run on its own, an input some
        other kernel wrote): a private slot, zeroed and filled by ct_absmax_f32 in front of the launch."""
        rt, d = st.rt, st.rt['desc']
        if rt.get('amax_own') is None:
            rt['amax_own'] = torch.zeros(d.batch * _lib.ABSMAX_LINE_BYTES // 4, device=self.device, dtype=torch.int32)
            d.in_absmax = rt['amax_own'].data_ptr()
        rt['amax_own'].zero_()
        hw = d.h * d.w
        base = d.in_ + 4 * d.in_coff * hw
        _lib.check(self.lib.ct_absmax_f32(base, d.batch, d.cin * hw, d.in_ctot * hw, rt['amax_own'].data_ptr(), self._stream()),
                   'ct_absmax_f32')

    def reads_max(self, st):
        """Whether the launch of this conv reads maxima of |input| (ct_conv_desc.in_absmax): the f16x2 operand form."""
        f = FORMS.get(st.rt.get('wino'))
        return f.h2 if f is not None else st.rt.get('x3') is not None and self.x3_h2(st.rt['x3'])

    def run_conv(self, st):
        f = FORMS.get(st.rt.get('wino'))
        needs_max = (f.h2 and not f.own_max) if f is not None else st.rt.get('x3') is not None and self.x3_h2(st.rt['x3'])
        if needs_max and (not st.rt['desc'].in_absmax or (st.rt.get('amax_own') is not None and not st.rt.get('amax_frozen'))):
            self._own_absmax(st)
        if f is not None:
            _lib.check(f.run(self.lib, C.byref(st.rt['desc']), st.rt[f.key].data_ptr(),
                             self.ws_pool[st.rt.get('ws_key', 0)] if f.split else None, st.rt.get('pool'), self._stream()), st.name)
            return
        x3 = st.rt.get('x3')
        if x3 is not None:               # fp32 convolution on the bf16 matrix pipe (bf16x3 split, csrc/ct_conv_x3.hip)
            _lib.check(self.lib.ct_conv2d_x3_fwd(C.byref(st.rt['desc']), st.rt['wx3'][(self.x3_bk(x3), self.x3_h2(x3))].data_ptr(), x3,
                                                 self._stream()), st.name)
            return
        _lib.check(self.lib.ct_conv2d_fwd(C.byref(st.rt['desc']), self._stream()), st.name)

    # ---- bf16x3 (ct_conv2d_x3_fwd): config index, or None for the fp32 MFMA kernel
    def x3_bk(self, cfg):
        return self.lib.ct_conv_x3_config_bk(cfg)

    def x3_h2(self, cfg):
        """Whether bf16x3-kernel config `cfg` is one of the f16x2 twins ('h2:<tile>', csrc/ct_f16x2.h)."""
        return bool(self.lib.ct_conv_x3_config_h2(cfg))

    def x3_names(self):
        return [self.lib.ct_conv_x3_config_name(i).decode() for i in range(self.lib.ct_conv_x3_num_configs())]

    def enable_x3(self, st, cfg):
        """Route this conv through the bf16x3 kernel with tile config `cfg` (None = back to ct_conv2d_fwd)."""
        rt = st.rt
        self.kernel_epoch += 1
        if cfg is None:
            rt['x3'] = None
            if rt.get('wpk_stale'):
                self.pack_conv(st)
            return
        self.enable_wino(st, False)
        bk = self.x3_bk(cfg)
        if bk <= 0:
            raise _lib.CtdetError('%s: bf16x3 config %r' % (st.name, cfg))
        rt.setdefault('wx3', {})
        h2 = self.x3_h2(cfg)
        if (bk, h2) not in rt['wx3']:
            size = self.lib.ct_conv_x3h_packed_bytes if h2 else self.lib.ct_conv_x3_packed_bytes
            rt['wx3'][(bk, h2)] = self.alloc((size(st.cin, st.cout, st.kh, st.kw, bk),), torch.uint8)
        rt['x3'] = cfg
        self._pack_x3(st)

    def _pack_x3(self, st):
        bk, h2 = self.x3_bk(st.rt['x3']), self.x3_h2(st.rt['x3'])
        pack = self.lib.ct_conv_pack_weights_x3h if h2 else self.lib.ct_conv_pack_weights_x3
        _lib.check(pack(*weight_parts(st.parts), st.cin, st.kh, st.kw, bk, st.rt['wx3'][(bk, h2)].data_ptr(), self._stream()),
                   'ct_conv_pack_weights_x3h' if h2 else 'ct_conv_pack_weights_x3')

    def run_pool(self, st, bufs, batch):
        _lib.check(self.lib.ct_maxpool2d_fwd(bufs[st.src].data_ptr(), bufs[st.dst].data_ptr(), batch * st.ch,
                                             st.h, st.w, st.oh, st.ow, st.k, st.stride, st.pad, self._stream()),
                   st.name)

    def run_ctxpool(self, st, bufs, batch):
        src, dst = bufs[st.src], bufs[st.dst]
        _lib.check(self.lib.ct_ctx_pool_fwd(src.data_ptr() + 4 * st.src_base, src.shape[1],
                                            dst.data_ptr() + 4 * st.dst_base, dst.shape[1], batch, st.h, st.w,
                                            st.ch, st.k, self._stream()), st.name)

    # ---- autotune: time every tile config of a conv step on its real buffers
    def _time_conv(self, st, iters=3, rounds=2):
        """ms per launch: the better of `rounds` timed bursts of `iters` launches after one warm-up launch.  Short
        launches get longer bursts (>= ~1 ms of device time): three 30 us launches are inside the timer's noise, and a
        flipped choice lands in the committed table.  A kernel on the f16x2 operand form is timed with the maxima of |input| in
        place (taken once here, as its producer would have left them in a network), not with an absmax pass per launch."""
        if self.reads_max(st):
            if not st.rt['desc'].in_absmax or st.rt.get('amax_own') is not None:
                st.rt['amax_frozen'] = False
                self._own_absmax(st)
                st.rt['amax_frozen'] = True
        try:
            self.run_conv(st)
            torch.cuda.synchronize(self.device)
            best = float('inf')
            for r in range(rounds + 1):
                if r == 1 and best < 1.0 / 3:             # the first burst was the estimate: size the others from it
                    iters = min(64, max(iters, int(1.0 / max(best, 1e-3)) + 1))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    self.run_conv(st)
                e1.record()
                torch.cuda.synchronize(self.device)
                best = min(best, e0.elapsed_time(e1) / iters)
        finally:
            self._thaw_absmax(st)
        return best

    def tune_conv(self, st, iters=3):
        ncfg = self.lib.ct_conv_num_configs()
        best, best_t = 0, float('inf')
        times = []
        self.enable_wino(st, False)
        self.enable_x3(st, None)
        for cfg in range(ncfg):
            st.rt['desc'].config = cfg + 1
            try:
                t = self._time_conv(st, iters)
            except _lib.CtdetError:
                times.append(float('inf'))
                continue
            times.append(t)
            if t < best_t:
                best, best_t = cfg, t
        st.rt['desc'].config = best + 1
        st.rt['config'] = best + 1
        best_x3 = None
        policy = self.policy
        if conv_policy.x3_allowed(policy, st):
            for cfg in range(self.lib.ct_conv_x3_num_configs()):
                if st.cin % self.x3_bk(cfg) or not self.x3_names()[cfg].endswith('d') or self.x3_h2(cfg):   # (the table holds the bf16x3 names)
                    times.append(float('inf'))      # k-step does not divide cin / single accumulator (accuracy gate)
                    continue
                self.enable_x3(st, cfg)
                t = self._time_conv(st, iters)
                times.append(t)
                if t < best_t:
                    best_x3, best_t = cfg, t
            self.enable_x3(st, best_x3)
        if (st.rt.get('wino_ok') or st.rt.get('wino4s_ok')) and policy.wino:
            best_tile = 0
            for tile in wino_tiles(self, st):
                self.enable_wino(st, tile=tile)
                t = self._time_conv(st, iters)
                times.append(t)
                if t < best_t:
                    best_tile, best_t = tile, t
            # what the layer would run without a Winograd kernel: recorded next to a dilated layer's 'wino4s' entry ('|alt')
            st.rt['alt'] = self.x3_names()[best_x3] if best_x3 is not None else self.lib.ct_conv_config_name(best).decode()
            if best_tile:
                self.enable_wino(st, tile=best_tile)
            else:
                self.enable_wino(st, False)
                if best_x3 is not None:
                    self.enable_x3(st, best_x3)
        st.rt['tune_ms'] = times
        return best, times

    @staticmethod
    def _thaw_absmax(st):
        """Unfreeze the maxima _time_conv took for its bursts: they belong to the data the tuner saw, and run_conv on a standalone
        backend takes them again, into the same private slot, from whatever the buffers hold then (a Runtime wires its own
        slots afterwards)."""
        st.rt.pop('amax_frozen', None)


def absmax_source(steps, tracks):
    """Whose per-image maxima bound a buffer (ct_conv_desc.in_absmax / out_absmax), for the inference and the training wiring:
    -> f(buffer) = (root buffer, its writers) or (None, []).  A buffer whose ONLY writer is a max-pool step is bounded by the
    pool's input (pooled values are a subset of it), and so on along the chain; the root's writers must all satisfy
    tracks(step).  Any other writer of a buffer on the chain -- a second step storing into the pooled buffer, a kernel that
    does not fold its maxima -- leaves the buffer without a source: its consumer gets no slot."""
    writers = {}
    for st in steps:
        for b in ([sg.dst for sg in st.segs] if st.kind == 'conv' and st.segs else [st.dst]):
            writers.setdefault(b, []).append(st)

    def source(b):
        seen = set()
        while True:
            ws = writers.get(b, [])
            if len(ws) == 1 and ws[0].kind == 'pool' and b not in seen:
                seen.add(b)
                b = ws[0].src
                continue
            return (b, ws) if ws and all(tracks(w) for w in ws) else (None, [])
    return source


def wire_absmax(be, batch, steps, consumers, desc, reads, tracks, fallback=None):
    """Hand out the maxima slots of a plan (the ONE wiring loop of Runtime, TrainRuntime and the bf16 backend) -> {buffer: slot}.
    consumers: the conv steps in launch order; desc(st): the descriptor its launch reads (None: it has none); reads(st): whether
    that launch reads maxima of its input; tracks(st): whether a writer folds the maxima of what it stores (absmax_source).  A
    reader whose buffer has a source shares the buffer's slot: handed out at the first reader, out_absmax of the buffer's writers.
    Readers left without one go to fallback(st), which moves the layer to a kernel that needs none and says so -- then everything
    is wired again (the moved layer may have stopped tracking); fallback=None leaves them to measure their own input."""
    source = absmax_source(steps, tracks)
    while True:
        for st in consumers:
            if desc(st) is not None:
                desc(st).in_absmax = desc(st).out_absmax = None
        slots, left = {}, []
        be.slots_used = 0
        for st in consumers:
            if not reads(st):
                continue
            b, ws = source(st.src)
            if b is None:
                left.append(st)
                continue
            if b not in slots:
                slots[b] = be.new_slot(batch)
                for w in ws:
                    desc(w).out_absmax = slots[b]
            desc(st).in_absmax = slots[b]
        if fallback is None or not [st for st in left if fallback(st)]:
            return slots


# ---- the kernel policy as seen from here: thin views of ctdet/conv_policy.py on the process environment
def _env_policy(net=None, batch=None):
    return conv_policy.resolve(net, batch, os.environ)


def wino_tiles(backend=None, st=None):
    """Winograd variants the tuner / the table may use under the backend's policy (conv_policy.wino_tiles), on step st if given."""
    return conv_policy.wino_tiles(backend.policy if backend is not None else _env_policy(),
                                  conv_policy.Layer(cin=st.cin, geo=st.rt) if st is not None else None)


def operand_form_h2(net, batch=None):
    """(winograd, direct) of an inference runtime: ConvPolicy.h2 / h2_direct."""
    p = _env_policy(net, batch)
    return p.h2, p.h2_direct


def ctx_policy(net):
    return _env_policy(net).ctx_tiles


def ctx_tile_set(net):
    return _env_policy(net).tile_set


def ctx_f4_max_cin(net):
    return _env_policy(net).f4_max_cin


def ctx_f4_tile():
    return _env_policy().f4_tile


def ctx_w4s_min_cin(net):
    return _env_policy(net).w4s_min_cin


def apply_tuned(backend, st, batch, wino4=True):
    """Give a prepared conv step the committed tile choice for its shape under the backend's policy (conv_policy.choose_forward);
    False if the table has none.  wino4=False maps a 'wino4' entry to 'wino'."""
    policy = backend.policy if wino4 else dataclasses.replace(backend.policy, wino4=False)
    c = conv_policy.choose_forward(policy, tune_table(), backend.kernels, conv_policy.Layer.of(st, batch))
    if c is None:
        return False
    if c.kind == 'wino':
        backend.enable_wino(st, tile=c.value)
    elif c.kind == 'x3':
        backend.enable_x3(st, c.value)
    else:
        st.rt['config'] = st.rt['desc'].config = c.value
    return True


SIDE_AFTER_DEFAULT = ''


def run_on_streams(rt, run_step):
    """Walk the plan's steps in launch order (rt.order: plan order, side-stream steps possibly deferred, see
    Runtime._build_schedule), each step on the stream the schedule gave it (rt.sid), cross-stream producer -> consumer
    edges as events (rt.xdeps / rt.signal / rt.ev); everything joins the caller's stream."""
    steps = rt.plan.steps
    if rt.side is None:
        for st in steps:
            run_step(st)
        return
    main = torch.cuda.current_stream(rt.backend.device)
    for sd in rt.sides:
        sd.wait_stream(main)
    streams = [main] + rt.sides
    order = getattr(rt, 'order', None) or list(range(len(steps)))
    pos, n = 0, len(order)
    while pos < n:
        k = rt.sid[order[pos]]
        with torch.cuda.stream(streams[k]):
            while pos < n and rt.sid[order[pos]] == k:
                i = order[pos]
                for j in rt.xdeps[i]:
                    streams[k].wait_event(rt.ev[j])
                run_step(steps[i])
                if i in rt.signal:
                    rt.ev[i].record(streams[k])
                pos += 1
    for sd in rt.sides:
        main.wait_stream(sd)


class Runtime:
    """A Plan bound to a backend: buffers, packed weights, and the forward entry points."""

    def __init__(self, net, batch, backend, tune=None):
        self.plan = Plan(net, batch)
        self.backend = backend
        self.batch = batch
        self.net = net
        bufs = {}
        for name, shp in self.plan.buf_shapes.items():
            bufs[name] = backend.alloc((batch,) + tuple(shp))
        self.bufs = bufs
        self.policy = backend.policy = conv_policy.resolve(net, batch, os.environ)
        for st in self.plan.steps:
            if st.kind == 'conv':
                backend.prepare_conv(st, bufs, batch)
        # tile config per conv: committed table first (names, so it survives config reordering),
        # live autotune only for shapes the table does not know (CTDET_TUNE=0 disables, =2 forces)
        mode = os.environ.get('CTDET_TUNE', '1') if tune is None else ('1' if tune else '0')
        self.tuned = False
        self.live_tuned = []
        self.event_log = None        # set to a list to collect (step, start_event, end_event) per conv
        if getattr(backend, 'tune_conv', None) is not None:
            missing = [st for st in self.conv_steps() if mode == '2' or not apply_tuned(backend, st, batch)]
            if missing and mode != '0':
                self.autotune(missing)
            self.tuned = not missing or mode != '0'
            # shapes the committed table does not serve: timed live (mode 1 / 2) or left to the library's heuristic (mode 0) --
            # either way a tile choice no parity test pinned at that shape (bench.py refuses a headline with any)
            self.live_tuned = [st.tune_key(batch) for st in missing]
            # ConvPolicy.force_tile: every layer that runs on a Winograd kernel and has the geometry for it is moved to that variant
            force = self.policy.force_tile
            for st in (self.conv_steps() if force else ()):
                # dilated layers only exist on the three-kernel form: they keep it unless that is what is being forced
                geo = st.rt.get('wino4s_ok') if force in WINO4S_TILES else st.rt.get('wino4f_ok') if force in WINO4F_TILES else \
                    st.rt.get('wino_ok')
                if st.rt.get('wino') and geo and (st.rt.get('winox_ok') or force in (2, 4) + WINO4S_TILES + WINO4F_TILES):
                    backend.enable_wino(st, tile=force)
        self._fuse_pools()
        self._mark_exclusive()
        self._build_schedule()
        self._share_workspaces()
        self._wire_absmax()

    def _fuse_pools(self):
        """MaxPool2d(2, 2) directly behind a Winograd conv: the 2x2 output tile is the pooling window, so
        the conv writes the pooled map itself (and skips its full-resolution output if nothing else reads it)."""
        steps = self.plan.steps
        fuse = os.environ.get('CTDET_FUSE_POOL', '1') != '0'
        for pi, ps in enumerate(steps):
            if ps.kind != 'pool' or (ps.k, ps.stride, ps.pad) != (2, 2, 0):
                continue
            prod = [st for st in steps if st.kind == 'conv' and not st.segs and st.dst == ps.src]
            if len(prod) != 1 or not prod[0].rt.get('wino') or prod[0].dst_coff != 0 or prod[0].cout != ps.ch \
                    or prod[0].res is not None:
                continue
            # a fusable producer never splits its channel sum (the fused form cannot): CTDET_FUSE_POOL=0 then
            # changes the launches, not the arithmetic
            prod[0].rt['desc'].ksplit = 0
            if not fuse:
                continue
            others = [st for st in steps if st is not ps and (getattr(st, 'src', None) == ps.src or
                                                              getattr(st, 'res', None) == ps.src)]
            prod[0].rt['pool'] = (self.bufs[ps.dst], ps.oh, ps.ow, bool(others))
            ps.fused_into = prod[0].name

    def _mark_exclusive(self):
        """Opt-in (CTDET_W4_STREAMK=1): F(4x4,3x3) launches of the trunk up to the first branch point (conv1_1 ..
        conv4_3) have the device to themselves in every schedule -- nothing the side stream runs exists before the
        first Norm / head source -- so they may use the kernel's stream-K form (desc.ksplit = -2: a persistent grid
        whose last, partial round is cut by input-channel chunks; 67 MB of slab workspace shared by those launches,
        they run one after another).  +1.3 .. 2.5 % images/s at bs 32 (three layers with 3.1 rounds of workgroups).
        Off by default: the cut items are the LAST tiles of the batch, so an image's last bits would depend on its
        position in the batch (tests/test_gpu_harness.py and test_full_size_pipeline_properties check that they do not).
        The marking does not depend on CTDET_STREAMS or CTDET_FUSE_POOL."""
        if os.environ.get('CTDET_W4_STREAMK', '0') != '1' or not hasattr(self.backend, 'lib'):
            return
        steps = self.plan.steps
        first_side = next((i for i, st in enumerate(steps)
                           if st.name.startswith(('Norm.', 'head.')) or st.kind == 'ctxpool'), len(steps))
        ws = None
        for st in steps[:first_side]:
            if st.kind != 'conv' or st.rt.get('wino') != 4:
                continue
            if ws is None:
                ws = self.bufs.setdefault('__streamk_ws', self.backend.alloc((256 * 2 * 64 * 32 * 16,)))
            d = st.rt['desc']
            d.ksplit, d.ksplit_ws, d.ksplit_ws_floats = -2, ws.data_ptr(), ws.numel()

    # ---- two-stream schedule: the Norm branch and the multibox heads are independent of the trunk that
    # follows their source (base.23.., extras..), and the small 19x19 .. 1x1 kernels of that trunk cannot fill
    # 256 CUs on their own; running the side work on a second HIP stream lets it soak up the idle CUs.
    def _build_schedule(self):
        self.side = None
        steps = self.plan.steps
        if os.environ.get('CTDET_STREAMS', '2') == '1' or self.backend.device.type != 'cuda':
            return
        nstreams = int(os.environ.get('CTDET_STREAMS', '2'))

        def stream_of(st):
            side = st.name.startswith(('Norm.', 'head.')) or st.kind == 'ctxpool'
            sid = 1 if side else 0
            if nstreams > 2:                     # the independent branches of an RFB block on their own streams
                for b, tag in enumerate(('.b1.', '.b2.', '.b3.')):
                    if tag in st.name:
                        sid = 2 + (3 if side else 0) + b
            return sid
        sid = [stream_of(st) for st in steps]
        if not any(sid):
            return

        def reads(st):
            r = [st.src]
            if getattr(st, 'res', None) is not None:
                r.append(st.res)
            return r

        def writes(st):
            if st.kind == 'conv' and st.segs:
                return [sg.dst for sg in st.segs]
            if st.kind == 'conv' and st.rt.get('pool') is not None:
                return [st.dst] + [p.dst for p in steps if getattr(p, 'fused_into', None) == st.name]
            return [st.dst]
        writers = {}
        self.xdeps, self.signal = [[] for _ in steps], set()
        for i, st in enumerate(steps):
            for b in reads(st):
                for j in writers.get(b, []):
                    if sid[j] != sid[i]:
                        self.xdeps[i].append(j)
                        self.signal.add(j)
            for b in writes(st):
                writers.setdefault(b, []).append(i)
        self.sid = sid
        # Launch order.  The side work (Norm branch, heads: 38x38 / 19x19 layers that fill the chip) only depends on
        # conv4_3 / conv7, while the END of the trunk (extras.1 .. extras.6 and their heads: 10x10 .. 1x1 maps, ~30 launches
        # of 25 .. 80 workgroups) cannot fill 256 CUs.  CTDET_SIDE_AFTER = name of a trunk step: the side-stream steps that
        # precede it in plan order are launched right after it instead, so they run beside the small layers rather than
        # beside conv5 .. conv7, which fill the chip on their own.
        self.order = list(range(len(steps)))
        after = os.environ.get('CTDET_SIDE_AFTER', SIDE_AFTER_DEFAULT)
        names = [st.name for st in steps]
        if after and after in names:
            k = names.index(after)
            # only the side stream proper (Norm / heads / context pooling) is deferred: with CTDET_STREAMS > 2 the RFB branch
            # streams feed main-stream steps at or before the anchor, whose waits must see this pass's events
            early = [i for i in range(k) if sid[i] == 1]
            self.order = [i for i in range(k + 1) if sid[i] != 1] + early + list(range(k + 1, len(steps)))
        self.sides = [torch.cuda.Stream(self.backend.device) for _ in range(max(sid))]
        self.side = self.sides[0]
        self.ev = {j: torch.cuda.Event() for j in self.signal}

    def _wire_absmax(self):
        """Per-image maxima of |activation| for the f16x2 kernels (ct_conv_desc.in_absmax / out_absmax, csrc/ct_f16x2.h).  A buffer
        that an f16x2 layer reads gets a slot (one line per image) when EVERY step that writes it folds the maxima of what it
        stores into one: every forward convolution kernel does, except the fused Winograd kernels on fp32 / bf16x3; a max-pool's
        output shares the slot of its input (pooled values are a subset), whether the pool runs as a step or inside its producer.
        An f16x2 consumer whose buffer has no slot runs the bf16x3 twin of its kernel (tile 47 takes the maxima itself, inside its
        launch).  The slots are zeroed once per step (run_loaded)."""
        be = self.backend
        if not hasattr(be, 'new_slot'):
            return
        if hasattr(be, 'wire_absmax'):          # a backend with rules of its own (the bf16 path: ctdet/engine_bf16.py)
            self.amax_slots = be.wire_absmax(self)
            self._wired_epoch = be.kernel_epoch
            return
        def tracks(st):
            if st.kind != 'conv' or st.segs:
                return False
            f = FORMS.get(st.rt.get('wino'))
            return f.tracks if f is not None else True

        def to_plain(st):                   # the bf16x3 twin; tile 47 takes the maxima itself, inside its launch
            if getattr(FORMS.get(st.rt.get('wino')), 'own_max', False):
                return False
            if st.rt.get('wino'):
                be.enable_wino(st, tile=FORMS[st.rt['wino']].plain)
            else:
                xn = be.x3_names()
                be.enable_x3(st, xn.index('x3:' + xn[st.rt['x3']][3:]))
            return True
        for st in self.conv_steps():
            st.rt.pop('amax_own', None)
            st.rt.pop('amax_frozen', None)
        self.amax_slots = wire_absmax(be, self.batch, self.plan.steps, self.conv_steps(), lambda st: st.rt['desc'], be.reads_max,
                                      tracks, to_plain)
        self._wired_epoch = be.kernel_epoch

    def _share_workspaces(self):
        """One three-kernel-Winograd workspace per stream of the schedule (HipBackend.ws_pool) instead of one per layer."""
        if not hasattr(self.backend, 'ws_rebuild'):
            return
        for i, st in enumerate(self.plan.steps):
            if st.kind == 'conv':
                st.rt['ws_key'] = self.sid[i] if self.side is not None else 0
        self.backend.ws_rebuild(self.conv_steps())

    def autotune(self, steps=None):
        self.bufs['x'].normal_()
        for st in self.plan.steps:            # run once so every buffer holds realistic data
            self._run_step(st)
        for st in (steps if steps is not None else self.conv_steps()):
            self.backend.tune_conv(st)

    def tuned_configs(self):
        lib = self.backend.lib
        out = {}
        xn = self.backend.x3_names()
        for st in self.conv_steps():
            if not (st.rt['desc'].config > 0 or st.rt.get('wino') or st.rt.get('x3') is not None):
                continue
            key = st.tune_key(self.batch)
            f32 = lib.ct_conv_config_name(st.rt['desc'].config - 1).decode() if st.rt['desc'].config > 0 else None
            if st.rt.get('wino'):
                out[key] = WINO_NAME[st.rt['wino']]
                if st.dil > 1 and st.rt.get('alt'):       # apply_tuned's fallback where tile 44 may not be used on a dilated layer
                    out[key + '|alt'] = st.rt['alt']
                    if f32 and st.rt['alt'].startswith('x3:'):
                        out[key + '|f32'] = f32
            elif st.rt.get('x3') is not None:
                out[key] = xn[st.rt['x3']]
                if f32:
                    out[key + '|f32'] = f32        # fallback tile when CTDET_X3=0
            else:
                out[key] = f32
        return out

    def refresh_weights(self):
        """Re-pack any fused conv whose parameters changed since the last pack."""
        for st in self.plan.steps:
            if st.kind == 'conv' and st.rt.get('versions') != self.backend.param_versions(st):
                self.backend.pack_conv(st)

    def _run_step(self, st):
        if st.kind == 'conv':
            if self.event_log is not None:      # HIP events on the launch stream (bench roofline)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                self.backend.run_conv(st)
                e1.record()
                self.event_log.append((st, e0, e1))
                return
            self.backend.run_conv(st)
        elif st.kind == 'pool':
            if getattr(st, 'fused_into', None) is None:
                self.backend.run_pool(st, self.bufs, self.batch)
        elif st.kind == 'ctxpool':
            self.backend.run_ctxpool(st, self.bufs, self.batch)
        else:
            raise ValueError(st.kind)

    def load_input(self, x):
        """Shape check, re-pack of changed weights, copy of x [B,3,S,S] into the plan's input buffer."""
        want = (self.batch,) + tuple(self.plan.buf_shapes['x'])
        if tuple(x.shape) != want:
            raise _lib.CtdetError('plan was built for input %s, got %s' % (want, tuple(x.shape)))
        self.refresh_weights()
        self.copy_input(x)

    def copy_input(self, x):
        """The copy of load_input alone (x already checked, weights already fresh): one launch, capturable -- a
        DetectionPipeline's second test-time-augmentation pass loads its mirrored batch with it inside the step."""
        if hasattr(self.backend, 'load_input'):       # bf16 path: NCHW fp32 image -> NHWC bf16
            self.backend.load_input(self.bufs['x'], x)
        else:
            self.bufs['x'].copy_(x)

    def run_loaded(self):
        """The launches of the backbone on the input buffer (no allocation, no host synchronisation: capturable)."""
        if getattr(self.backend, 'zero_slots', None) is not None:
            self.ensure_wired()
            self.backend.zero_slots()       # the maxima of |activation| the f16x2 layers take their scales from (_wire_absmax)
        run_on_streams(self, self._run_step)
        return self.bufs['loc'], self.bufs['conf'], self.bufs['obj']

    def ensure_wired(self):
        """Re-wire the maxima slots when a step changed kernels since they were wired (tuner, tools): a producer may have stopped
        tracking.  Allocates: a DetectionPipeline calls it before it captures or replays a hipGraph."""
        if getattr(self.backend, 'new_slot', None) is not None and getattr(self, '_wired_epoch', None) != self.backend.kernel_epoch:
            self._wire_absmax()

    def run_backbone(self, x):
        """x [B,3,S,S] on the device -> raw (loc [B,P*4], conf [B,P*C], obj [B,P*2]) buffers (views)."""
        self.load_input(x)
        return self.run_loaded()

    def policy_record(self):
        """Every switch that shaped this runtime's kernel choice, resolved to what is in force (bench.py prints it as
        `config.policy`; a line measured under a non-default switch says so).  `env` lists the CTDET_* variables that are set --
        the library reads a few of its own (launch geometry experiments), so they are named even where Python ignores them."""
        b, p = self.backend, self.policy
        tiles = {}
        for st in self.conv_steps():
            w = st.rt.get('wino')
            if w:
                tiles[int(w)] = tiles.get(int(w), 0) + 1
        rec = b.policy_extra(self.conv_steps()) if hasattr(b, 'policy_extra') else {}
        return {
            **rec,
            'operand_form': 'f16x2' if p.h2 else 'bf16x3',
            'direct_twins_f16x2': p.h2_direct,
            'ctx_tiles': p.ctx_tiles,
            'wino_tile_set': sorted(p.tile_set) if p.tile_set is not None else None,
            'winograd_layers_by_tile': {str(k): v for k, v in sorted(tiles.items())},
            'tune_table': os.path.basename(TUNE_TABLE),
            'live_tuned_layers': len(self.live_tuned),
            'env': {k: v for k, v in sorted(os.environ.items()) if k.startswith('CTDET_')},
        }

    def conv_steps(self):
        return [s for s in self.plan.steps if s.kind == 'conv']
