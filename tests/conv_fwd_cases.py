"""Shared by tests/test_conv_fwd_ref_cpu.py and tests/test_gpu_conv_fwd.py: ONE row table for every forward convolution path
(ct_conv2d_fwd, ct_conv2d_x3_fwd as bf16x3 and f16x2, the seven Winograd forms of ctdet.wino_forms.FORMS), the seeded inputs of a
row, the float64 reference of the whole fused step (conv, bias or eval-BatchNorm, * res_scale + res, ReLU per part; the pooled map
and the head-segment layout where the row has them), what float32 arithmetic itself loses on the row (e32: torch-CPU fp32;
ew32: the Winograd transforms restated in float32) and the bounds the GPU tests assert.  Importable without a GPU (nothing here
loads libctdet.so).

Families.  'D' ct_conv2d_fwd (fp32 MFMA; 'valu' on the 3-channel rows), 'X' ct_conv2d_x3_fwd bf16x3 configurations, 'H' its f16x2
("h2:") twins -- the direct rows; 2, 4, 23, 44, 46, 47, 48 -- the Winograd rows (3x3, stride 1, pad = dilation).

Bounds.  None is fitted to the kernels under test.
  hard   1e-4 for every launch: the library's contract.
  tight, direct (D, the dual-accumulator X configurations, H):  max(8 * e32(row), 2^-20) -- factor and floor of
         tests/test_gpu_conv_grad.py: 8 for another accumulation order and the noise of a max statistic, 2^-20 = 16 fp32 roundoffs
         for the rows with a handful of terms.
  tight, Winograd form f:  max(WINO_BOUND[f] * ew32(row, m_f) / ew32_deep(m_f), 2^-20) -- the form's own bound on the deep shape of
         test_gpu_wino.py::test_wino_rounding_error_vs_fp64, scaled by how much easier the float32 restatement of F(m_f x m_f, 3x3)
         finds the row than that deep shape (m_f = 2 for forms 2 and 23, 4 for the others).
All errors are rel_err (max|a-b| / max|b|) of ONE image against the float64 reference of that image."""
import functools
import zlib
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from test_winograd_algebra_cpu import _wino_forward

HARD = 1e-4
TIGHT_FACTOR = 8.0
TIGHT_FLOOR = 2.0 ** -20
# the bounds of test_gpu_wino.py::test_wino_rounding_error_vs_fp64 (512 -> 512 channels on 38x38, post-ReLU input), per form
WINO_BOUND = {2: 3e-6, 4: 5e-5, 23: 1e-6, 44: 6e-6, 46: 1.2e-5, 47: 6e-6, 48: 1.2e-5}
WINO_M = {2: 2, 23: 2, 4: 4, 44: 4, 46: 4, 47: 4, 48: 4}

DIRECT_FAMILIES = ('D', 'X', 'H')
ALL_W = (2, 4, 23, 44, 46, 47, 48)
F32_W = (2, 4)                  # 8-channel chunks
SPLIT_W = (44, 47)              # three-kernel forms: dilated layers too
H2_W = (47, 48)                 # f16x2: read desc.in_absmax
KSPLITS = (0, 2, 3, 1000, -1)
KSPLIT_CONFIGS = (0, 5, 7)      # D configurations of the split-K row: heuristic, 32x128, 128x128k2


@dataclass(frozen=True)
class Case:
    name: str
    family: str                     # 'direct' or 'wino'
    forms: Tuple                    # direct: subset of ('D', 'X', 'H'); wino: form codes
    B: int
    cin: int
    H: int
    W: int
    parts: Tuple[int, ...]          # couts of the weight parts of the fused launch
    kh: int = 3
    kw: int = 3
    stride: int = 1
    ph: int = 1
    pw: int = 1
    dil: int = 1
    epi: str = 'bias'               # 'bias', 'bn' (eval BatchNorm, the tuple of test_gpu_kernels._bn) or 'none'
    relus: Optional[Tuple[bool, ...]] = None        # per part; None: ReLU everywhere
    img1_scale: Optional[float] = None      # x of image 1 multiplied by this
    res_scale: Optional[float] = None       # a residual [B, cout, oh, ow]: y * res_scale + res in front of the ReLU
    x_slice: Optional[Tuple[int, int]] = None       # (in_ctot, in_coff) of x inside a wider buffer
    out_slice: Optional[Tuple[int, int]] = None     # (out_ctot, out_coff)
    ksplits: Tuple[int, ...] = ()   # desc.ksplit values the row is launched with (direct rows: () = split-K off)
    segs: bool = False              # head scatter: every part is one segment of a flattened channels-last buffer
    pool: Optional[Tuple[bool, bool]] = None        # fused MaxPool2d(2, 2): (ceil_mode, write the full map too)
    amax: Tuple[str, ...] = ()      # forms 47 / 48: besides the default launch, in_absmax 'given' / 'loose' (x 2^10) / 'unset'
    props: Tuple[str, ...] = ()

    @property
    def cout(self):
        return sum(self.parts)

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
    def out_ctot(self):
        return self.out_slice[0] if self.out_slice else self.cout

    @property
    def out_coff(self):
        return self.out_slice[1] if self.out_slice else 0

    @property
    def part_relus(self):
        return self.relus if self.relus is not None else (True,) * len(self.parts)

    @property
    def terms(self):
        return self.cin * self.kh * self.kw

    @property
    def pointwise(self):
        """The rule of conv_x3_f32_pw (include/ctdet.h, ct_conv_x3_pointwise_enable) for a launch with split-K off."""
        return (self.kh, self.kw, self.stride, self.ph, self.pw, self.dil) == (1, 1, 1, 0, 0, 1) and self.cin % 32 == 0 and \
            not self.segs and not self.ksplits

    @property
    def pooled_hw(self):
        ceil = self.pool[0]
        return (-(-self.oh // 2), -(-self.ow // 2)) if ceil else (self.oh // 2, self.ow // 2)


def _d(name, forms, B, cin, H, W, parts, props, k=3, stride=1, pad=1, dil=1, **kw):
    kh, kw_ = (k, k) if isinstance(k, int) else k
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    return Case(name, 'direct', tuple(forms), B, cin, H, W, tuple(parts), kh, kw_, stride, ph, pw, dil, props=tuple(props), **kw)


def _w(name, forms, B, cin, H, W, parts, props, dil=1, **kw):
    return Case(name, 'wino', tuple(forms), B, cin, H, W, tuple(parts), 3, 3, 1, dil, dil, dil, props=tuple(props), **kw)


DXH = DIRECT_FAMILIES
DIRECT = (
    # the image layer: 27 terms, 143 pixels per image (a 128-pixel tile straddles the images); 'valu' and the fp32 tiles
    _d('img3', 'D', 2, 3, 13, 11, (16,), ('bn', 'k_tail', 'tile_across_images'), epi='bn'),
    # cout 37: a ragged 32-row block; cin 24: 216 terms, a k tail of every k-step; 63 pixels per image; mixed ReLU / no-ReLU
    _d('k_ragged', 'D', 3, 24, 9, 7, (24, 13), ('ragged_block', 'k_tail', 'tile_across_images', 'floor'), relus=(True, False)),
    _d('k3', DXH, 2, 32, 9, 7, (40,), ('bn', 'ragged_block', 'tile_across_images'), epi='bn'),
    # the second 128-row block has 8 live rows; image 1 at 2^-12 of image 0
    _d('two_blocks', DXH, 2, 64, 10, 10, (136,), ('ragged_block', 'img_scale'), img1_scale=2.0 ** -12),
    # ... and without a bias, so that image 1's own sums are what its error is measured against
    _d('img1_small', DXH, 2, 32, 9, 7, (40,), ('img_scale',), epi='none', relus=(False,), img1_scale=2.0 ** -12),
    _d('s2', DXH, 2, 32, 19, 17, (40,), ('s2',), stride=2),
    _d('p0', DXH, 2, 32, 5, 5, (33,), ('ragged_block',), pad=0),
    _d('4x4', DXH, 2, 32, 2, 2, (24,), ('one_pixel',), k=4),                          # 1x1 output: Npix = B
    _d('1x1', DXH, 3, 96, 10, 10, (70,), ('pointwise', 'ragged_block', 'tile_across_images'), k=1, pad=0),  # three 32-channel iterations
    _d('1x1_one_iter', DXH, 2, 32, 7, 9, (24, 8), ('pointwise', 'k_tail', 'floor', 'tile_across_images'), k=1, pad=0,
       relus=(True, False)),
    _d('1x1_tiny', DXH, 2, 64, 1, 1, (24,), ('pointwise', 'one_pixel'), k=1, pad=0),
    _d('1x1s2', DXH, 2, 32, 19, 19, (96,), ('s2', 'k_tail'), k=1, stride=2, pad=0),
    _d('1x3', DXH, 2, 32, 12, 11, (24,), ('nonsquare',), k=(1, 3), pad=(0, 1)),
    _d('3x1', DXH, 2, 32, 12, 11, (24,), ('nonsquare',), k=(3, 1), pad=(1, 0)),
    _d('dil3', DXH, 2, 32, 19, 19, (40,), ('dilated',), pad=3, dil=3),
    _d('dil6_small', DXH, 1, 32, 5, 5, (16,), ('dilated', 'k_tail'), pad=6, dil=6),               # only the centre tap is in bounds
    _d('res', DXH, 2, 32, 9, 7, (40,), ('bn', 'res'), epi='bn', res_scale=0.5),
    # input channels [32:80) of 96, output at offset 8 of 100, no ReLU: cin 48 -- the k32 configurations refuse it
    _d('slices', DXH, 2, 48, 9, 7, (64,), ('bn', 'in_slice', 'out_slice', 'k_tail'), epi='bn', relus=(False,), x_slice=(96, 32),
       out_slice=(100, 8)),
    _d('splitk', DXH, 2, 224, 5, 5, (72,), ('bn', 'res', 'splitk', 'ragged_block'), epi='bn', res_scale=0.7, ksplits=KSPLITS),
    # three head segments of 24 + 12 + 6 channels: a ragged last 32-row block, segment boundaries inside and across the blocks
    _d('heads', DXH, 2, 64, 5, 5, (24, 12, 6), ('segs', 'splitk'), relus=(False,) * 3, segs=True, ksplits=(0, 3)),
)

WINO = (
    _w('ragged_tiles', ALL_W, 2, 16, 13, 10, (24,), ('k_tail',)),                                 # 2x2 and 4x4 tilings ragged both ways
    _w('one_tile', ALL_W, 1, 16, 4, 4, (64,), ('k_tail',)),
    _w('block2_8rows', ALL_W, 2, 32, 5, 3, (72,), ('ragged_block',)),                             # a second 64-channel block with 8 live rows
    _w('one_pixel', ALL_W, 1, 48, 1, 1, (16,), ('one_pixel',)),
    _w('row', ALL_W, 2, 16, 1, 9, (33,), ('ragged_block',)),
    _w('col', ALL_W, 2, 16, 7, 1, (33,), ('ragged_block',)),
    _w('b3_19x19', ALL_W, 3, 64, 19, 19, (40,), ('tile_across_images',)),                         # 25 / 100 tiles per image
    _w('parts', ALL_W, 3, 48, 19, 19, (40, 24), ('bn', 'floor', 'tile_across_images'), epi='bn', relus=(True, False)),
    _w('res', ALL_W, 3, 64, 19, 19, (40,), ('bn', 'res'), epi='bn', res_scale=0.5),
    _w('slices', ALL_W, 2, 48, 13, 10, (40,), ('bn', 'in_slice', 'out_slice'), epi='bn', relus=(False,), x_slice=(80, 16),
       out_slice=(51, 5)),
    # ragged_tiles with image 1 at 2^-12 and no bias, so that image 1's own sums are what its error is measured against
    _w('img1_small', ALL_W, 2, 16, 13, 10, (24,), ('img_scale', 'amax_given', 'amax_loose', 'amax_unset'), epi='none', relus=(False,),
       img1_scale=2.0 ** -12, amax=('given', 'loose', 'unset')),
    _w('cin8', F32_W, 2, 8, 13, 10, (24,), ('k_tail',)),
    _w('cin24', F32_W, 2, 24, 5, 3, (72,), ('k_tail', 'ragged_block')),
    # 300 tiles (a ragged third 128-tile block), a ragged second 128-channel block
    _w('tiles300_cout136', SPLIT_W, 3, 32, 38, 37, (136,), ('ragged_block', 'tile_across_images')),
    _w('d2', SPLIT_W, 2, 16, 7, 9, (24,), ('dilated',), dil=2),
    _w('d3', SPLIT_W, 1, 64, 10, 10, (16,), ('dilated',), dil=3),
    _w('d5', SPLIT_W, 2, 32, 19, 17, (48,), ('dilated', 'bn', 'out_slice'), dil=5, epi='bn', out_slice=(59, 5)),
    _w('d6', SPLIT_W, 1, 16, 19, 19, (32,), ('dilated',), dil=6),
    _w('d6_5x5', SPLIT_W, 1, 16, 5, 5, (16,), ('dilated', 'empty_sublattice'), dil=6),            # 11 of 36 sub-lattices hold no pixel
    _w('pool_ceil_full', ALL_W, 2, 16, 19, 17, (9,), ('pool_ceil',), pool=(True, True)),
    _w('pool_floor_only', ALL_W, 1, 16, 23, 18, (33,), ('pool_floor', 'pooled_only'), pool=(False, False)),
    _w('pool_b8_3x3', ALL_W, 8, 16, 3, 3, (8,), ('pool_ceil', 'tile_across_images'), pool=(True, True)),
    _w('heads', ALL_W, 2, 32, 10, 9, (24, 42, 12), ('segs',), relus=(False,) * 3, segs=True),
    # F(4x4,3x3) fp32: the split over input channels (desc.ksplit); the stream-K path keeps its large-shape test
    _w('parts_ksplit', (4,), 3, 48, 19, 19, (40, 24), ('bn', 'floor', 'splitk'), epi='bn', relus=(True, False), ksplits=(2, 5, -1)),
)

CASES = DIRECT + WINO

# property -> (families that must have a row with it, least number of rows per family)
_EVERY = DIRECT_FAMILIES + ALL_W
REQUIRED = {
    'ragged_block': (_EVERY, 1), 'tile_across_images': (_EVERY, 1), 'one_pixel': (_EVERY, 1), 'k_tail': (_EVERY, 1),
    's2': (DIRECT_FAMILIES, 2), 'nonsquare': (DIRECT_FAMILIES, 2), 'dilated': (DIRECT_FAMILIES + SPLIT_W, 2),
    'empty_sublattice': (SPLIT_W, 1),
    'bn': (_EVERY, 2), 'floor': (_EVERY, 1), 'res': (_EVERY, 1), 'in_slice': (_EVERY, 1), 'out_slice': (_EVERY, 1),
    'img_scale': (_EVERY, 1), 'splitk': (DIRECT_FAMILIES + (4,), 1), 'segs': (_EVERY, 1),
    'pool_ceil': (ALL_W, 2), 'pool_floor': (ALL_W, 1), 'pooled_only': (ALL_W, 1),
    'pointwise': (('H',), 3),
    'amax_given': (H2_W, 1), 'amax_loose': (H2_W, 1), 'amax_unset': (H2_W, 1),
}


def rows_with(prop, family):
    return [c for c in CASES if prop in c.props and family in c.forms]


def segments(case):
    """[(name, co_begin, co_end, base, floats per image)] of a head row: part i is segment i, written channels-last at `base` of a
    longer row -- direct rows as test_gpu_kernels.check_split_k_head_segments lays them out, Winograd rows as
    test_gpu_wino.py::test_head_scatter_output (6 anchors, 11 priors in front, 5 behind)."""
    out, c0 = [], 0
    for name, c in zip(('loc', 'conf', 'obj'), case.parts):
        hw = case.oh * case.ow
        if case.family == 'direct':
            base, size = 7 * c, 7 * c + hw * c + 5 * c
        else:
            n = c // 6
            base, size = 11 * n, (11 + hw * 6 + 5) * n
        out.append((name, c0, c0 + c, base, size))
        c0 += c
    return out


def _bn(c, g):
    """The draw of test_gpu_kernels._bn: (weight, bias, running_mean, running_var)."""
    return (torch.rand(c, generator=g) * 0.4 + 0.8, torch.rand(c, generator=g) * 0.2 - 0.1,
            torch.rand(c, generator=g) * 0.2 - 0.1, torch.rand(c, generator=g) * 0.4 + 0.8)


@dataclass(frozen=True)
class Inputs:
    x_buf: torch.Tensor             # [B, x_ctot, H, W]; x = channels [x_coff, x_coff + cin)
    parts: Tuple                    # (weight [cout_i, cin, kh, kw], bias | None, bn tuple | None, relu) per part
    res: Optional[torch.Tensor]     # [B, cout, oh, ow]

    def x(self, case):
        return self.x_buf[:, case.x_coff:case.x_coff + case.cin]


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """Seeded float32 inputs of a row (computed once, never written): x randn -- every channel of the wider buffer --, image 1
    scaled where flagged; the weight parts randn * (2 / (cin kh kw))^0.5; a bias in [-0.5, 0.5) or the
    BatchNorm tuple; the residual randn."""
    g = torch.Generator().manual_seed(zlib.crc32(('%s/%s' % (case.family, case.name)).encode()) % 100000)
    x_buf = torch.randn(case.B, case.x_ctot, case.H, case.W, generator=g)
    if case.img1_scale is not None:
        x_buf[1] *= case.img1_scale
    sc = (2.0 / (case.cin * case.kh * case.kw)) ** 0.5
    parts = []
    for c, relu in zip(case.parts, case.part_relus):
        w = torch.randn(c, case.cin, case.kh, case.kw, generator=g) * sc
        b = torch.rand(c, generator=g) - 0.5 if case.epi == 'bias' else None
        bn = _bn(c, g) if case.epi == 'bn' else None
        parts.append((w, b, bn, relu))
    res = torch.randn(case.B, case.cout, case.oh, case.ow, generator=g) if case.res_scale is not None else None
    return Inputs(x_buf, tuple(parts), res)


def _epilogue(conv, parts, res, res_scale, dtype):
    """conv: [B, cout, oh, ow], the plain convolution of the concatenated parts in `dtype` -> the fused step's output: bias or
    eval-BatchNorm, * res_scale + res, ReLU, part by part (what test_gpu_absmax._ref does, the residual sliced per part)."""
    outs, c0 = [], 0
    for (w, b, bn, relu) in parts:
        c = w.shape[0]
        y = conv[:, c0:c0 + c]
        if b is not None:
            y = y + b.to(dtype).view(1, -1, 1, 1)
        if bn is not None:
            y = F.batch_norm(y, bn[2].to(dtype), bn[3].to(dtype), bn[0].to(dtype), bn[1].to(dtype), False, 0.0, 1e-5)
        if res is not None:
            y = y * res_scale + res[:, c0:c0 + c].to(dtype)
        outs.append(F.relu(y) if relu else y)
        c0 += c
    return torch.cat(outs, 1)


def fused_step(x, parts, case, res, dtype):
    """The whole fused step of a row on the operand values x / parts, evaluated in `dtype`."""
    w = torch.cat([p[0] for p in parts], 0).to(dtype)
    conv = F.conv2d(x.to(dtype), w, None, case.stride, (case.ph, case.pw), case.dil)
    return _epilogue(conv, parts, res, case.res_scale, dtype)


@dataclass(frozen=True)
class Ref:
    y: torch.Tensor                         # [B, cout, oh, ow] float64
    pooled: Optional[torch.Tensor]          # F.max_pool2d(y, 2, 2, ceil_mode=...) where the row pools
    flat: Optional[Dict[str, torch.Tensor]]         # segment name -> [B, oh * ow * channels], channels last


@functools.lru_cache(maxsize=None)
def ref64(case):
    """The fused step in float64 on the float32 values: the ONLY reference of the forward tests."""
    inp = make_inputs(case)
    y = fused_step(inp.x(case), inp.parts, case, inp.res, torch.float64)
    pooled = F.max_pool2d(y, 2, 2, 0, ceil_mode=case.pool[0]) if case.pool else None
    flat = {n: y[:, c0:c1].permute(0, 2, 3, 1).reshape(case.B, -1) for (n, c0, c1, _b, _s) in segments(case)} if case.segs else None
    return Ref(y, pooled, flat)


@functools.lru_cache(maxsize=None)
def cpu32(case):
    """The same step in torch-CPU float32."""
    inp = make_inputs(case)
    return fused_step(inp.x(case), inp.parts, case, inp.res, torch.float32)


def rel_err(a, b):
    """max|a-b| / max|b| (tests/conftest.py), on tensors."""
    d = float(b.abs().max())
    return float((a.double() - b.double()).abs().max()) / (d if d > 0 else 1.0)


def image_errors(got, want):
    """rel_err of each image on its own."""
    return [rel_err(got[n], want[n]) for n in range(want.shape[0])]


@functools.lru_cache(maxsize=None)
def e32(case):
    return max(image_errors(cpu32(case), ref64(case).y))


def wino_conv(x, w, m, dil, dtype):
    """A 3x3, stride-1, pad = dilation convolution as F(m x m, 3x3) in `dtype`: on each of the d x d sub-lattices of the pixel grid
    (test_winograd_algebra_cpu.py, test_dilated_layer_is_d2_pad1_layers_on_its_sublattices...) the sub-image is zero-padded to a
    multiple of m, transformed (test_winograd_algebra_cpu._wino_forward with the matrices cast to `dtype`) and cropped."""
    x, w = x.to(dtype), w.to(dtype)
    B, _, H, W = x.shape
    out = torch.zeros(B, w.shape[0], H, W, dtype=dtype)
    for sy in range(dil):
        for sx in range(dil):
            sub = x[:, :, sy::dil, sx::dil]
            if sub.numel() == 0:
                continue
            h, wd = sub.shape[2:]
            hp, wp = -(-h // m) * m, -(-wd // m) * m
            y = _wino_forward(F.pad(sub, (0, wp - wd, 0, hp - h)).contiguous(), w, m, dtype)
            out[:, :, sy::dil, sx::dil] = y[:, :, :h, :wd]
    return out


@functools.lru_cache(maxsize=None)
def wino32(case, m, dtype=torch.float32):
    """The fused step of a Winograd row with the convolution restated as F(m x m, 3x3) in float32 (dtype = float64: the same
    restatement without rounding, which must reproduce ref64)."""
    assert case.family == 'wino'
    inp = make_inputs(case)
    w = torch.cat([p[0] for p in inp.parts], 0)
    return _epilogue(wino_conv(inp.x(case), w, m, case.dil, dtype), inp.parts, inp.res, case.res_scale, dtype)


@functools.lru_cache(maxsize=None)
def ew32(case, m):
    return max(image_errors(wino32(case, m), ref64(case).y))


@functools.lru_cache(maxsize=None)
def ew32_deep(m):
    """ew32 on the shape of test_gpu_wino.py::test_wino_rounding_error_vs_fp64 (seed 5: x = randn(2, 512, 38, 38).relu(), weights
    randn * (2 / (512 * 9))^0.5, bias, ReLU), restricted to the first 64 output channels."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 512, 38, 38, generator=g).relu()
    w = (torch.randn(512, 512, 3, 3, generator=g) * (2.0 / (512 * 9)) ** 0.5)[:64].contiguous()
    b = (torch.rand(512, generator=g) - 0.5)[:64]
    want = F.relu(F.conv2d(x.double(), w.double(), b.double(), 1, 1))
    got = F.relu(wino_conv(x, w, m, 1, torch.float32) + b.view(1, -1, 1, 1))
    return max(image_errors(got, want))


def tight_direct(case):
    return max(TIGHT_FACTOR * e32(case), TIGHT_FLOOR)


def tight_wino(case, code):
    m = WINO_M[code]
    return max(WINO_BOUND[code] * ew32(case, m) / ew32_deep(m), TIGHT_FLOOR)


def drop_low_piece(t):
    """t with every value truncated to 16 significand bits: what a bf16x3 operand is without its lowest piece."""
    return (t.contiguous().view(torch.int32) & -256).view(torch.float32)
