"""Shared by tests/test_dgrad_ref_cpu.py and tests/test_gpu_wino_dgrad.py: the float64 reference of a convolution's data
gradient, the forward weight whose forward pass IS that data gradient, the ct_conv_desc of a data-gradient launch as
ctdet/train_engine.py fills it, and the case table of the Winograd data-gradient forms (ctdet.wino_forms.FORMS).  Importable
without a GPU (nothing here loads libctdet.so)."""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from ctdet import _lib

FORM_CODES = (2, 4, 44, 46, 47, 48)         # every FORMS entry with a *_dgrad packer (23 has none)
F32_FORMS = (2, 4)                          # 8-channel chunks: zc % 8 == 0
X3_FORMS = (44, 46, 47, 48)                 # 16-channel k-groups: zc % 16 == 0
SPLIT_FORMS = (44, 47)                      # three-kernel: 128 couts x 128 tiles per GEMM workgroup; dilated layers too
H2_FORMS = (47, 48)                         # f16x2: read the per-image maxima of dZ (desc.in_absmax)
# the geometry predicates TrainEngine asks before it selects a form (F(4x4,3x3) fp32: both)
SUPPORTED = {2: ('ct_conv_wino_supported',), 4: ('ct_conv_wino_supported', 'ct_conv_wino4_supported'),
             44: ('ct_conv_wino4s_supported',), 47: ('ct_conv_wino4s_supported',),
             46: ('ct_conv_wino4f_supported',), 48: ('ct_conv_wino4f_supported',)}


def ref_dgrad64(w_parts, dy, dil):
    """x.grad of F.conv2d(x, cat(w_parts), None, 1, dil, dil) for the upstream gradient dy: float64 autograd on the float32
    values.  The only reference of the data-gradient tests."""
    w = torch.cat([p.detach() for p in w_parts], 0).double()
    B, _, H, W = dy.shape
    x = torch.zeros(B, w.shape[1], H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, 1, dil, dil).backward(dy.detach().double())
    return x.grad.detach()


def mirrored_weights(w_parts):
    """The forward-convolution weight [cin_fwd, zc, 3, 3] whose forward pass (stride 1, pad = dilation) on dZ is the data
    gradient: channels swapped, taps rotated by 180 degrees."""
    return torch.cat(list(w_parts), 0).flip(2, 3).transpose(0, 1).contiguous()


def dgrad_desc(dz, cin_fwd, dil, out, out_coff, ones, zeros, *, acc=False, in_absmax=None, lib=None, ksplit_ws=None):
    """The ct_conv_desc of a Winograd data-gradient launch, field by field what TrainEngine builds (the direct descriptor `d` of a
    layer, copied into `w2` with transposed = 0): in_ = dZ [B, zc, H, W] (its own buffer: in_ctot = zc, in_coff = 0), cout = the
    forward layer's input channels, the source map as large as dZ (3x3, stride 1, pad = dilation), identity epilogue (scale = ones,
    shift = zeros), out = a channel slice of the source's gradient buffer, res_ctot / res_coff / res_scale = that slice with
    scale 1 -- and res = the SAME pointer as out when the slice was already written (acc).  lib: fills m_pad / k_pad (the direct
    kernel's paddings, which the copy carries along).  ksplit_ws: the split-K slab tensor the dilation-1 copy inherits (ksplit = -1:
    the library's choice; the F(4x4,3x3) fp32 kernel honours it); the engine's dilated copy resets it."""
    B, zc, H, W = dz.shape
    d = _lib.ConvDesc()
    d.in_ = dz.data_ptr()
    d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = B, zc, H, W, zc, 0
    d.scale, d.shift = ones.data_ptr(), zeros.data_ptr()
    d.cout = cin_fwd
    if lib is not None:
        d.m_pad, d.k_pad = lib.ct_conv_mpad(cin_fwd), lib.ct_conv_kpad(zc, 3, 3)
    d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = 3, 3, 1, dil, dil, dil
    d.oh, d.ow = H, W
    d.out, d.out_ctot, d.out_coff = out.data_ptr(), out.shape[1], out_coff
    d.res_ctot, d.res_coff, d.res_scale = out.shape[1], out_coff, 1.0
    d.res = out.data_ptr() if acc else None
    d.transposed = 0
    if ksplit_ws is not None and dil == 1:
        d.ksplit, d.ksplit_ws, d.ksplit_ws_floats = -1, ksplit_ws.data_ptr(), ksplit_ws.numel()
    if in_absmax is not None:
        d.in_absmax = in_absmax.data_ptr()
    return d


def ksplit_floats(B, cin_fwd, H, W):
    """Floats of the split-K slab workspace TrainEngine gives a data gradient (small maps only), else 0."""
    n = cin_fwd * B * H * W
    return 16 * n if n <= (2 << 20) else 0


@dataclass(frozen=True)
class Case:
    name: str
    forms: Tuple[int, ...]
    B: int
    parts: Tuple[int, ...]          # couts of the forward layer's weight parts; their sum = zc, the channels of dZ
    cin: int                        # input channels of the forward layer = channels of dX
    H: int
    W: int
    dil: int = 1
    sliced: bool = False            # out_coff 5 of out_ctot = cin + 11 (else offset 0 of cin + 3: still wider than the slice)
    acc: bool = False               # res == out: accumulate into what the slice holds
    amax: str = 'given'             # forms 47 / 48: 'given' (ct_absmax_f32), 'loose' (x 2^10), 'null' (desc.in_absmax unset)
    img1_scale: Optional[float] = None      # dZ of image 1 multiplied by this
    twice: bool = False             # a second launch must give the same bits
    props: Tuple[str, ...] = ()     # what the row is in the table for (test_dgrad_ref_cpu.py counts these per form)

    @property
    def zc(self):
        return sum(self.parts)

    @property
    def out_ctot(self):
        return self.cin + (11 if self.sliced else 3)

    @property
    def out_coff(self):
        return 5 if self.sliced else 0


def expect_supported(case, code):
    """What ct_conv_*_supported must say for the row's descriptor: the fused forms take dilation 1 only, the three-kernel form
    dilated layers without a residual (wino4s_ok)."""
    if case.dil == 1:
        return True
    return code in SPLIT_FORMS and not case.acc


def expect_error(case, code):
    """The launch must raise CtdetError and leave the buffer alone: an unsupported geometry, or the fused f16x2 form without
    the maxima of dZ (it has no pass of its own)."""
    return not expect_supported(case, code) or (code == 48 and case.amax == 'null')


ALL = FORM_CODES
CASES = (
    # ---- every form, dilation 1: B, parts (zc), cin_fwd, H, W
    Case('ragged_tiles', ALL, 2, (16,), 24, 13, 10, props=('ragged_tiles',)),           # 2x2 and 4x4 tilings ragged both ways, < 64 couts
    Case('one_tile', ALL, 1, (16,), 64, 4, 4, props=('one_tile',)),
    Case('block2_8rows', ALL, 2, (32,), 72, 5, 3, props=('ragged_block',)),             # a second 64-channel block with 8 live rows
    Case('one_pixel', ALL, 1, (48,), 16, 1, 1, props=('one_pixel',)),                   # all padding
    Case('b3_19x19', ALL, 3, (64,), 40, 19, 19, twice=True, props=('b3_19x19', 'twice')),
    # ---- multi-part packing: the parts' couts are THIS convolution's input channels, boundaries inside a 16-channel k-group
    Case('parts_40_24', ALL, 3, (40, 24), 40, 19, 19, props=('parts',)),
    Case('parts_100_28_acc', ALL, 2, (100, 28), 24, 13, 10, acc=True, props=('parts', 'acc')),
    # ---- output slice / in-place accumulate
    Case('ragged_tiles_slice', ALL, 2, (16,), 24, 13, 10, sliced=True, props=('slice',)),
    Case('ragged_tiles_slice_acc', ALL, 2, (16,), 24, 13, 10, sliced=True, acc=True, props=('slice', 'acc')),
    Case('block2_8rows_acc', ALL, 2, (32,), 72, 5, 3, acc=True, props=('acc', 'acc_ragged_block')),
    Case('block2_8rows_slice_acc', ALL, 2, (32,), 72, 5, 3, sliced=True, acc=True, props=('slice', 'acc', 'acc_ragged_block')),
    # ---- per-image scale: image 1 at 2^-12 of image 0 (the per-image metric must hold for both)
    Case('img1_small', ALL, 2, (16,), 24, 13, 10, img1_scale=2.0 ** -12, props=('img_scale',)),
    # ---- fp32 forms: zc a multiple of their 8-channel chunk and not of 16
    Case('zc8', F32_FORMS, 2, (8,), 24, 13, 10, props=('zc8',)),
    Case('zc24', F32_FORMS, 2, (24,), 72, 5, 3, props=('zc24',)),
    Case('zc24_parts_7_17', F32_FORMS, 3, (7, 17), 40, 19, 19, props=('zc24', 'parts')),
    # ---- three-kernel forms: 300 tiles (ragged third 128-tile block), ragged second 128-channel block
    Case('tiles300_cout136', SPLIT_FORMS, 3, (32,), 136, 38, 37, props=('tiles300',)),
    Case('tiles300_cout136_acc', SPLIT_FORMS, 3, (32,), 136, 38, 37, acc=True, props=('tiles300', 'acc', 'acc_ragged_block')),
    # ---- ... dilated (pad = dilation)
    Case('d5', SPLIT_FORMS, 2, (32,), 48, 19, 17, 5, twice=True, props=('dilated', 'twice_dilated')),
    Case('d6', SPLIT_FORMS, 1, (16,), 32, 19, 19, 6, props=('dilated',)),
    Case('d2', SPLIT_FORMS, 2, (16,), 24, 7, 9, 2, props=('dilated',)),
    Case('d3', SPLIT_FORMS, 1, (64,), 16, 10, 10, 3, props=('dilated',)),
    Case('d6_5x5', SPLIT_FORMS, 1, (16,), 16, 5, 5, 6, props=('dilated', 'empty_sublattice')),      # 11 of 36 sub-lattices hold no pixel
    Case('d2_slice', SPLIT_FORMS, 2, (16,), 24, 7, 9, 2, sliced=True, props=('dilated', 'dilated_slice')),
    Case('d5_parts_20_12_slice', SPLIT_FORMS, 2, (20, 12), 48, 19, 17, 5, sliced=True, props=('dilated', 'dilated_slice', 'dilated_parts')),
    Case('d6_5x5_slice', SPLIT_FORMS, 1, (16,), 16, 5, 5, 6, sliced=True, props=('dilated', 'dilated_slice', 'empty_sublattice')),
    # ... with a residual: wino4s_ok refuses (the dilated output transform has no accumulate)
    Case('d2_acc_refused', ALL, 2, (16,), 24, 7, 9, 2, acc=True, props=('refused',)),
    Case('d6_5x5_slice_acc_refused', SPLIT_FORMS, 1, (16,), 16, 5, 5, 6, sliced=True, acc=True, props=('refused',)),
    # ---- f16x2 forms: where the maxima of dZ come from
    Case('amax_loose', H2_FORMS, 3, (64,), 40, 19, 19, amax='loose', props=('amax_loose',)),
    Case('amax_null', H2_FORMS, 3, (64,), 40, 19, 19, amax='null', props=('amax_null',)),
    Case('amax_null_ragged_acc', H2_FORMS, 2, (32,), 72, 5, 3, acc=True, amax='null', props=('amax_null', 'acc', 'acc_ragged_block')),
    Case('amax_loose_img1_small', H2_FORMS, 2, (16,), 24, 13, 10, amax='loose', img1_scale=2.0 ** -12, props=('amax_loose', 'img_scale')),
    Case('amax_null_img1_small', H2_FORMS, 2, (16,), 24, 13, 10, amax='null', img1_scale=2.0 ** -12, props=('amax_null', 'img_scale')),
    Case('d5_amax_null', (47,), 2, (32,), 48, 19, 17, 5, amax='null', props=('dilated', 'amax_null_dilated')),
    Case('d6_5x5_amax_loose', (47,), 1, (16,), 16, 5, 5, 6, amax='loose', props=('dilated', 'empty_sublattice', 'amax_loose')),
)

# the deepest shape of the network (512 -> 512 @19x19), post-ReLU-like dZ (half zeros): rounding against float64
DEEP = (
    Case('deep', ALL, 2, (512,), 512, 19, 19, props=('deep',)),
    Case('deep_d6', SPLIT_FORMS, 2, (512,), 512, 19, 19, 6, props=('deep', 'deep_dilated', 'dilated')),
)

# property -> (forms that must have a row with it, least number of rows per form)
REQUIRED = {
    'ragged_tiles': (ALL, 1), 'one_tile': (ALL, 1), 'ragged_block': (ALL, 1), 'one_pixel': (ALL, 1), 'b3_19x19': (ALL, 1),
    'parts': (ALL, 2), 'slice': (ALL, 1), 'acc': (ALL, 2), 'acc_ragged_block': (ALL, 1), 'img_scale': (ALL, 1), 'twice': (ALL, 1),
    'refused': (ALL, 1),
    'zc8': (F32_FORMS, 1), 'zc24': (F32_FORMS, 1),
    'tiles300': (SPLIT_FORMS, 1), 'dilated': (SPLIT_FORMS, 5), 'empty_sublattice': (SPLIT_FORMS, 1), 'dilated_slice': (SPLIT_FORMS, 1),
    'dilated_parts': (SPLIT_FORMS, 1), 'twice_dilated': (SPLIT_FORMS, 1),
    'amax_loose': (H2_FORMS, 1), 'amax_null': (H2_FORMS, 1), 'amax_null_dilated': ((47,), 1),
    'deep': (ALL, 1), 'deep_dilated': (SPLIT_FORMS, 1),
}


def case_ids(cases):
    return [(c, code) for c in cases for code in c.forms]


def make_inputs(case, relu_like=False):
    """Seeded float32 inputs of a row: dZ [B, zc, H, W], the forward weight parts [cout_i, cin, 3, 3] scaled by
    (2 / (9 zc))^0.5, and G0, the finite pattern the output buffer [B, out_ctot, H, W] is pre-filled with."""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) % 100000)
    dz = torch.randn(case.B, case.zc, case.H, case.W, generator=g)
    if relu_like:
        dz = dz.relu()
    if case.img1_scale is not None:
        dz[1] *= case.img1_scale
    parts = [torch.randn(c, case.cin, 3, 3, generator=g) * (2.0 / (9 * case.zc)) ** 0.5 for c in case.parts]
    g0 = torch.randn(case.B, case.out_ctot, case.H, case.W, generator=g)
    return dz, parts, g0
