"""Shared by tests/test_conv_grad_ref_cpu.py and tests/test_gpu_conv_grad.py: the float64 reference of a convolution's weight and
data gradient, the seeded inputs, the ct_conv_desc of the two direct gradient launches as ctdet/train_engine.py fills them
(s.wgrad for ct_conv2d_wgrad, s.dgrad for ct_conv2d_fwd / ct_conv2d_x3_fwd with transposed = 1) and ONE case table for both
kernels.  Importable without a GPU (nothing here loads libctdet.so).

Reduction lengths.  A weight gradient sums B*OH*OW products per element, a data gradient at most zc*kh*kw.  The rows keep both
at or below RED_CAP = 4300 terms: measured on the CPU, one dropped term then moves the result by >= 3e-3 of its maximum (4e-2 at
722 terms), three orders above the bounds the GPU tests assert, while torch's own fp32 path sits 0.7-12e-7 from float64.  The one
exception is the row the table needs for MANY pixel splits of the weight gradient (B 4 on 38x38: 5776 terms, 23 splits); the
sensitivity check of test_conv_grad_ref_cpu.py holds for it like for every other row."""
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from ctdet import _lib

RED_CAP = 4300
RED_CAP_EXEMPT = ('b4_38x38',)              # see the module docstring
TILE_ROWS = (32, 64, 96, 128, 160)          # heights of ct_conv2d_fwd's implicit-GEMM tiles (M = cin_fwd in a data gradient)
GENERIC_CINS = (3, 20, 34, 72)
DGRAD_CINS = (24, 40, 70, 130, 168)
DGRAD_ZCS = (16, 34, 64)


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                       # 'w': a ct_conv2d_wgrad row, 'd': a data-gradient row
    B: int
    cin: int                        # input channels of the forward layer (channels of x and of dX)
    H: int
    W: int                          # the forward layer's input map
    parts: Tuple[int, ...]          # couts of the forward layer's weight parts ('w' rows: one part = cout)
    kh: int = 3
    kw: int = 3
    stride: int = 1
    ph: int = 1
    pw: int = 1
    dil: int = 1
    zero: int = 0                   # 'd': rows of an extra all-zero weight part (the heads' padding of zc); dZ there is random
    x_slice: Optional[Tuple[int, int]] = None       # 'w': (in_ctot, in_coff) of x inside a wider buffer
    dz_slice: Optional[Tuple[int, int]] = None      # (ctot, coff) of the live dZ channels inside a wider buffer
    sliced: bool = False            # 'd': out_coff 5 of out_ctot = cin + 11 (else offset 0 of cin + 3: still wider than the slice)
    acc: bool = False               # 'd': res == out, res_scale 1: accumulate into what the slice holds
    splitk: bool = False            # 'd': member of the split-K subset
    props: Tuple[str, ...] = ()

    @property
    def cout(self):
        return sum(self.parts)

    @property
    def zc(self):
        """Channels of the data-gradient launch's input = live couts + the zero part."""
        return sum(self.parts) + self.zero

    @property
    def oh(self):
        return (self.H + 2 * self.ph - self.dil * (self.kh - 1) - 1) // self.stride + 1

    @property
    def ow(self):
        return (self.W + 2 * self.pw - self.dil * (self.kw - 1) - 1) // self.stride + 1

    @property
    def x_ctot(self):
        return self.x_slice[0] if self.x_slice else self.cin

    @property
    def x_coff(self):
        return self.x_slice[1] if self.x_slice else 0

    @property
    def dz_ctot(self):
        return self.dz_slice[0] if self.dz_slice else self.zc

    @property
    def dz_coff(self):
        return self.dz_slice[1] if self.dz_slice else 0

    @property
    def out_ctot(self):
        return self.cin + (11 if self.sliced else 3)

    @property
    def out_coff(self):
        return 5 if self.sliced else 0

    @property
    def tapmajor(self):
        """wgrad_impl's choice at the default 64x64 tile (csrc/ct_wgrad.hip)."""
        return self.cin % 64 == 0

    @property
    def reduction(self):
        return self.B * self.oh * self.ow if self.kind == 'w' else self.zc * self.kh * self.kw

    @property
    def npix(self):
        """GEMM columns of the data-gradient launch."""
        return self.B * self.H * self.W

    @property
    def x3(self):
        """TrainEngine's rule for the bf16x3 data gradient (s.dgrad_x3)."""
        return self.kind == 'd' and self.zc % 16 == 0 and self.zc >= 32 and self.stride <= 2

    @property
    def tb2(self):
        """wgrad_impl runs the 128x128 variant under CTDET_WGRAD_TB=2."""
        return self.kind == 'w' and self.cout >= 96 and self.cin * self.kh * self.kw >= 96


def _w(name, B, cin, H, W, cout, props, **kw):
    return Case(name, 'w', B, cin, H, W, (cout,), props=tuple(props), **kw)


def _pair(name, B, H, W, cout, tm_cin, g_cin, props, **kw):
    """The same weight-gradient row once for the tap-major kernel (cin % 64 == 0) and once for the generic one."""
    return (_w(name + '_tm', B, tm_cin, H, W, cout, props, **kw), _w(name + '_g', B, g_cin, H, W, cout, props, **kw))


WGRAD_CASES = (
    *_pair('pad1_19', 2, 19, 19, 40, 64, 3, ('pad1_19',)),
    # two channel tiles per tap, a second cout tile with 6 live rows, Npix 969: the last 64-pixel chunk holds 9 pixels and
    # chunks straddle images
    *_pair('b3_19x17', 3, 19, 17, 70, 128, 72, ('b3_19x17',)),
    *_pair('s2_odd', 2, 19, 19, 40, 64, 20, ('s2_odd',), stride=2),
    *_pair('s2_even', 2, 10, 10, 40, 64, 34, ('s2_even',), stride=2),
    *_pair('d6_19', 2, 19, 19, 24, 64, 20, ('d6_19',), ph=6, pw=6, dil=6),
    *_pair('d6_5x5', 2, 5, 5, 24, 64, 34, ('d6_5x5',), ph=6, pw=6, dil=6),          # only the centre tap is in bounds
    *_pair('k1x3', 2, 12, 11, 24, 64, 20, ('k1x3',), kh=1, kw=3, ph=0, pw=1),
    *_pair('k3x1', 2, 12, 11, 24, 64, 20, ('k3x1',), kh=3, kw=1, ph=1, pw=0),
    *_pair('k4x4', 3, 2, 2, 32, 64, 72, ('k4x4',), kh=4, kw=4),                      # 1x1 output: Npix = B
    *_pair('k1x1_s1', 2, 19, 19, 40, 64, 34, ('k1x1_s1',), kh=1, kw=1, ph=0, pw=0),
    *_pair('k1x1_s2', 2, 19, 19, 40, 64, 34, ('k1x1_s2',), kh=1, kw=1, ph=0, pw=0, stride=2),
    *_pair('pad0_5x5', 2, 5, 5, 32, 64, 3, ('pad0_5x5',), ph=0, pw=0),
    *_pair('one_pixel', 2, 1, 1, 24, 64, 20, ('one_pixel',)),
    *_pair('slices', 2, 13, 10, 48, 64, 34, ('slices',), x_slice=(80, 9), dz_slice=(64, 7)),
    *_pair('b4_38x38', 4, 38, 38, 64, 64, 20, ('b4_38x38',)),                        # the largest row: 23 pixel splits
    # cout >= 96 and cin*kh*kw >= 96: the rows the 128x128 variant (CTDET_WGRAD_TB=2) takes; tap-major there needs cin % 128 == 0
    *_pair('tb2', 2, 10, 9, 100, 128, 72, ('tb2',)),
)


def _d(name, B, parts, cin, H, W, props, **kw):
    return Case(name, 'd', B, cin, H, W, tuple(parts), props=tuple(props), **kw)


DGRAD_CASES = (
    _d('pad1_19', 2, (64,), 40, 19, 19, ('pad1_19',)),                               # Npix 722 = 5 x 128 + 82 = 11 x 64 + 18
    _d('b3_19x17', 3, (34,), 70, 19, 17, ('b3_19x17', 'slice'), sliced=True),        # Npix 969
    _d('s2_odd', 2, (16,), 130, 19, 19, ('s2_odd',), stride=2),
    _d('s2_even', 2, (64,), 24, 10, 10, ('s2_even',), stride=2),                     # last row / column of dX: fewer taps
    _d('s2_even_acc', 2, (64,), 24, 10, 10, ('s2_even', 'acc'), stride=2, acc=True),
    _d('d6_19', 1, (34,), 168, 19, 19, ('d6_19',), ph=6, pw=6, dil=6),
    _d('d6_5x5', 2, (64,), 40, 5, 5, ('d6_5x5', 'splitk'), ph=6, pw=6, dil=6, splitk=True),
    _d('k1x3', 2, (34,), 24, 12, 11, ('k1x3', 'in_coff'), kh=1, kw=3, ph=0, pw=1, dz_slice=(39, 3)),
    _d('k3x1', 2, (16,), 70, 12, 11, ('k3x1',), kh=3, kw=1, ph=1, pw=0),
    _d('k4x4', 3, (64,), 130, 2, 2, ('k4x4', 'splitk'), kh=4, kw=4, splitk=True),
    _d('k1x1_s1', 2, (34,), 168, 19, 19, ('k1x1_s1',), kh=1, kw=1, ph=0, pw=0),
    _d('k1x1_s1_slice_acc', 2, (64,), 168, 19, 19, ('k1x1_s1', 'slice', 'acc'), kh=1, kw=1, ph=0, pw=0, sliced=True, acc=True),
    _d('k1x1_s2', 2, (64,), 40, 19, 19, ('k1x1_s2', 'splitk'), kh=1, kw=1, ph=0, pw=0, stride=2, splitk=True),
    _d('pad0_5x5', 2, (16,), 24, 5, 5, ('pad0_5x5',), ph=0, pw=0),
    _d('one_pixel', 2, (34,), 40, 1, 1, ('one_pixel',)),
    # multi-part packing: part boundaries inside a k-step; the heads' form: (20, 6) + 6 all-zero rows -> zc 32, dZ random there too
    _d('parts_40_24', 2, (40, 24), 70, 13, 10, ('parts', 'splitk'), splitk=True),
    _d('parts_40_24_slice_acc', 2, (40, 24), 70, 13, 10, ('parts', 'slice', 'acc'), sliced=True, acc=True),
    _d('heads_20_6_zero6', 2, (20, 6), 130, 10, 10, ('parts', 'zero_part'), zero=6),
    _d('heads_20_6_zero6_slice_acc', 2, (20, 6), 130, 10, 10, ('parts', 'zero_part', 'slice', 'acc'), zero=6, sliced=True, acc=True),
)

GEOMETRY = ('pad1_19', 'b3_19x17', 's2_odd', 's2_even', 'd6_19', 'd6_5x5', 'k1x3', 'k3x1', 'k4x4', 'k1x1_s1', 'k1x1_s2', 'pad0_5x5',
            'one_pixel')
# property -> least number of rows.  Weight gradient: per class (tap-major AND generic).  Data gradient: over the table.
REQUIRED_W = {**{p: 1 for p in GEOMETRY}, 'slices': 1, 'b4_38x38': 1, 'tb2': 1}
REQUIRED_D = {**{p: 1 for p in GEOMETRY}, 'parts': 2, 'zero_part': 1, 'slice': 2, 'acc': 2, 'in_coff': 1, 'splitk': 4}


def ref64(x, w_parts, dz, case):
    """(dw, dx) of F.conv2d(x, cat(w_parts)) for the upstream gradient dz: float64 autograd on the float32 values.  The only
    reference of the direct-gradient tests."""
    xd = x.detach().double().requires_grad_(True)
    wd = torch.cat([p.detach() for p in w_parts], 0).double().requires_grad_(True)
    F.conv2d(xd, wd, None, case.stride, (case.ph, case.pw), case.dil).backward(dz.detach().double())
    return wd.grad.detach(), xd.grad.detach()


def grad32(x, w_parts, dz, case):
    """The same through torch's fp32 autograd: what the earlier tests compared with; its distance from ref64 is `e32`."""
    xd = x.detach().clone().requires_grad_(True)
    wd = torch.cat([p.detach() for p in w_parts], 0).clone().requires_grad_(True)
    F.conv2d(xd, wd, None, case.stride, (case.ph, case.pw), case.dil).backward(dz.detach())
    return wd.grad.detach(), xd.grad.detach()


@dataclass(frozen=True)
class Inputs:
    x_buf: torch.Tensor             # [B, x_ctot, H, W]; x = channels [x_coff, x_coff + cin)
    parts: Tuple[torch.Tensor, ...]         # the live weight parts [cout_i, cin, kh, kw]
    dz_buf: torch.Tensor            # [B, dz_ctot, OH, OW]; live dZ = channels [dz_coff, dz_coff + cout), then `zero` padded channels
    g0: torch.Tensor                # finite prefill of the output: 'w' [cout, cin, kh, kw], 'd' [B, out_ctot, H, W]

    def x(self, case):
        return self.x_buf[:, case.x_coff:case.x_coff + case.cin]

    def dz(self, case):
        return self.dz_buf[:, case.dz_coff:case.dz_coff + case.cout]


def make_inputs(case):
    """Seeded float32 inputs of a row: x and dZ randn (every channel of the wider buffers, the zero part's dZ included), the weight
    parts randn * (2 / (cin kh kw))^0.5 and G0."""
    g = torch.Generator().manual_seed(zlib.crc32(('%s/%s' % (case.kind, case.name)).encode()) % 100000)
    x_buf = torch.randn(case.B, case.x_ctot, case.H, case.W, generator=g)
    dz_buf = torch.randn(case.B, case.dz_ctot, case.oh, case.ow, generator=g)
    sc = (2.0 / (case.cin * case.kh * case.kw)) ** 0.5
    parts = tuple(torch.randn(c, case.cin, case.kh, case.kw, generator=g) * sc for c in case.parts)
    shape = (case.cout, case.cin, case.kh, case.kw) if case.kind == 'w' else (case.B, case.out_ctot, case.H, case.W)
    return Inputs(x_buf, parts, dz_buf, torch.randn(shape, generator=g))


def wgrad_desc(case, x_buf):
    """The ct_conv_desc of a weight-gradient launch, field by field what TrainEngine builds as s.wgrad: the forward geometry on
    the forward input (a channel slice of the source buffer); the call passes dZ, its channel total and offset, and dw."""
    w = _lib.ConvDesc()
    w.in_ = x_buf.data_ptr()
    w.batch, w.cin, w.h, w.w, w.in_ctot, w.in_coff = case.B, case.cin, case.H, case.W, x_buf.shape[1], case.x_coff
    w.cout = case.cout
    w.kh, w.kw, w.stride, w.pad_h, w.pad_w, w.dil = case.kh, case.kw, case.stride, case.ph, case.pw, case.dil
    w.oh, w.ow = case.oh, case.ow
    return w


def ksplit_floats(case):
    """Floats of the split-K slab workspace TrainEngine gives a data gradient (small maps only), else 0."""
    n = case.cin * case.B * case.H * case.W
    return 16 * n if n <= (2 << 20) else 0


def dgrad_desc(case, dz_buf, out, ones, zeros, *, wpacked=None, mpad=0, kpad=0, config=0, ksplit=0, ksplit_ws=None):
    """The ct_conv_desc of a direct data-gradient launch, field by field what TrainEngine builds as s.dgrad: in_ = dZ (zc channels
    at in_coff of its buffer), cout = the forward layer's input channels, (oh, ow) = the forward INPUT map, stride / pad / dil the
    forward layer's, identity epilogue, out = a channel slice of the source's gradient buffer, res_ctot / res_coff / res_scale =
    that slice with scale 1 -- and res = the SAME pointer as out when the slice was already written (case.acc) --, transposed = 1.
    ksplit_ws: the slab tensor (the engine passes ksplit = -1 with it)."""
    d = _lib.ConvDesc()
    d.in_ = dz_buf.data_ptr()
    d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = case.B, case.zc, case.oh, case.ow, dz_buf.shape[1], case.dz_coff
    d.wpacked = wpacked.data_ptr() if wpacked is not None else None
    d.scale, d.shift = ones.data_ptr(), zeros.data_ptr()
    d.cout, d.m_pad, d.k_pad = case.cin, mpad, kpad
    d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = case.kh, case.kw, case.stride, case.ph, case.pw, case.dil
    d.oh, d.ow = case.H, case.W
    d.out, d.out_ctot, d.out_coff = out.data_ptr(), out.shape[1], case.out_coff
    d.res_ctot, d.res_coff, d.res_scale = out.shape[1], case.out_coff, 1.0
    d.res = out.data_ptr() if case.acc else None
    d.transposed = 1
    d.config = config
    if ksplit_ws is not None:
        d.ksplit, d.ksplit_ws, d.ksplit_ws_floats = ksplit, ksplit_ws.data_ptr(), ksplit_ws.numel()
    return d
