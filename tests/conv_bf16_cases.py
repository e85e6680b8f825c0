"""Shared by tests/test_conv_bf16_ref_cpu.py and tests/test_gpu_bf16_conv.py: ONE row table for the bf16 channels-last convolution
(ct_conv2d_bf16_fwd, csrc/ct_conv_bf16.hip), the seeded inputs of a row, the float64 reference of the whole fused step, what
torch-CPU float32 loses on the row (e32) and the bound the GPU test asserts.  Importable without a GPU (nothing here loads
libctdet.so).

Variants.  The launcher picks one of seven instantiations of conv_bf16_nhwc (ct_conv_bf16_variant_name); every row names the one
it is there for and the environment that forces it (CTDET_BF16_BIG_MIN, CTDET_BF16_SHORTK: read per call; CTDET_BF16_BK: read once
per process, so the rows that set it run in a child process).  A switch a row does not name is unset.

Reference.  Activations, weights and residual rounded to bfloat16 by torch.Tensor.bfloat16(); the convolution in float64; the
epilogue in float64 in the kernel's order: * scale + shift, then * res_scale + res, then the floor (lo[c] where the row has one,
else 0 with ReLU, else none).

Bound for a bf16 output g against the float64 value r, elementwise and per image:   |g - r| <= h(r) + A
  h(r) = 2^(floor(log2|r|) - 8), half a bf16 ulp of r (0 for r = 0): the one correct rounding;
  A    = max(8 * e32, 2^-20) * max|r| over the image: fp32 accumulation in another order -- e32 is the rel_err of torch-CPU fp32 on
         the same rounded operands against the reference, for that image; factor and floor are TIGHT_FACTOR / TIGHT_FLOOR of
         tests/conv_fwd_cases.py.
fp32 head segments have no rounding term: rel_err < max(8 * e32, 2^-20), and the library's hard bound 1e-4.
Nothing here is fitted to the kernel under test."""
import functools
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

HARD = 1e-4
TIGHT_FACTOR = 8.0              # largest err / e32 measured on the device: 1.95 (the table in tests/test_gpu_bf16_conv.py)
TIGHT_FLOOR = 2.0 ** -20
KSPLITS = (0, 2, 3, 1000, -1)
SWITCHES = ('CTDET_BF16_BIG_MIN', 'CTDET_BF16_SHORTK', 'CTDET_BF16_BK')
VARIANTS = ('bf16:128x64k32s', 'bf16:128x128k32s', 'bf16:256x256k32', 'bf16:128x64k32', 'bf16:128x64k64', 'bf16:128x128k32',
            'bf16:128x128k64')
BK = {'bf16:128x64k32s': 32, 'bf16:128x128k32s': 32, 'bf16:256x256k32': 32, 'bf16:128x64k32': 32, 'bf16:128x64k64': 64,
      'bf16:128x128k32': 32, 'bf16:128x128k64': 64}
BM = {v: (256 if v.startswith('bf16:256') else 128) for v in VARIANTS}
BF16_NAN = 0x7FC0
BIG_ON, BIG_OFF = (('CTDET_BF16_BIG_MIN', '1'),), (('CTDET_BF16_BIG_MIN', '1000000000'),)


@dataclass(frozen=True)
class Case:
    name: str
    variant: str                    # what ct_conv_bf16_variant_name answers under `env`
    B: int
    cin: int
    H: int
    W: int
    parts: Tuple[int, ...]          # couts of the weight parts of the fused launch
    k: int = 3
    stride: int = 1
    pad: int = 1
    dil: int = 1
    x_slice: Optional[Tuple[int, int]] = None       # (in_ctot, in_coff) of x inside a wider buffer
    out_slice: Optional[Tuple[int, int]] = None     # (out_ctot, out_coff)
    res_slice: Optional[Tuple[int, int]] = None     # (res_ctot, res_coff): the row has a residual
    res_scale: float = 1.0
    relu: bool = True
    lo: bool = False                # a per-channel floor: 0 / -inf alternating, one positive floor (channel 2)
    segs: bool = False              # head scatter: every part is one fp32 segment of a flattened channels-last buffer
    ksplits: Tuple[int, ...] = (0,)
    env: Tuple[Tuple[str, str], ...] = ()
    inputs_of: Optional[str] = None                 # the row whose inputs (and reference) this one shares

    @property
    def cout(self):
        return sum(self.parts)

    @property
    def oh(self):
        return (self.H + 2 * self.pad - self.dil * (self.k - 1) - 1) // self.stride + 1

    @property
    def ow(self):
        return (self.W + 2 * self.pad - self.dil * (self.k - 1) - 1) // self.stride + 1

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
    def npix(self):
        return self.B * self.oh * self.ow

    @property
    def tail(self):
        """The step in front of the last one holds segments at or past cin too (cin_pad is a multiple of 64)."""
        return BK[self.variant] == 32 and self.cin > 8 and 0 < self.cin % 64 < 32

    @property
    def child(self):
        return 'CTDET_BF16_BK' in dict(self.env)


def _c(name, variant, B, cin, H, W, parts, **kw):
    return Case(name, 'bf16:' + variant, B, cin, H, W, tuple(parts), **kw)


def _twin(case, name, variant, env):
    kw = dict(case.__dict__, name=name, variant='bf16:' + variant, env=env, inputs_of=case.inputs_of or case.name)
    return Case(**kw)


_IMG = (
    # the image layer (cin_pad == 8, a k-step is four taps of 8 channels): 9 taps = a last step of one tap; one tap; four taps
    # exactly; 49 taps = 13 steps, stride 2; the 8 channels at offset 8 of a 24-channel buffer
    _c('img_3x3', '128x64k32s', 2, 8, 30, 30, (64,)),
    _c('img_1x1', '128x64k32s', 2, 8, 13, 11, (40,), k=1, pad=0, relu=False),
    _c('img_2x2', '128x64k32s', 2, 8, 10, 9, (24,), k=2, pad=0),
    _c('img_7x7s2', '128x64k32s', 2, 8, 37, 41, (24,), k=7, stride=2, pad=3),
    _c('img_8of24', '128x64k32s', 2, 8, 11, 10, (16,), x_slice=(24, 8), out_slice=(40, 16)),
    # 16 562 pixels: 130 pixel tiles (the last ragged) x 2 cout tiles (the last with two channels) = 260 >= 256
    _c('img_wide', '128x128k32s', 2, 8, 91, 91, (130,)),
)
_SHORTK = (
    _c('sk_64_96', '128x64k32', 2, 64, 19, 19, (96,)),
    _c('sk_48of96', '128x64k32', 2, 48, 19, 19, (64,), pad=2, dil=2, x_slice=(96, 32), out_slice=(104, 16), res_slice=(64, 0),
       res_scale=0.5, relu=False),
    # (split-K 1000: every split owns one step, so a split starts ON the step that lies past cin altogether)
    _c('sk_24of40', '128x64k32', 2, 24, 10, 11, (40,), x_slice=(40, 8), res_slice=(64, 8), res_scale=0.7, lo=True,
       ksplits=(0, 3, 1000)),
    _c('sk_16_dil3', '128x64k32', 2, 16, 19, 19, (40,), pad=3, dil=3, x_slice=(32, 16)),
    _c('sk_32_1x1s2', '128x64k32', 2, 32, 19, 19, (96,), k=1, stride=2, pad=0),
    _c('sk_32of72', '128x64k32', 2, 32, 9, 7, (24,), x_slice=(72, 8), ksplits=(0, 1000)),       # a whole 32-channel step past cin
    _c('sk_heads', '128x64k32', 2, 64, 5, 5, (24, 12, 6), relu=False, segs=True, ksplits=(0, 3)),
)
_K64 = (
    _c('k64_72_parts', '128x64k64', 3, 72, 5, 5, (40, 24, 8), k=1, stride=2, pad=0),
    _c('k64_200_dil5', '128x64k64', 1, 200, 38, 38, (128,), pad=5, dil=5),
    _c('k64_4x4_on_2x2', '128x64k64', 2, 128, 2, 2, (256,), k=4),
    _c('k64_3x3_on_3x3', '128x64k64', 2, 128, 3, 3, (256,), pad=0),
    _c('k64_136of160', '128x64k64', 2, 136, 10, 11, (130,), stride=2, x_slice=(160, 16)),
    _c('splitk_256', '128x64k64', 2, 256, 5, 5, (72,), res_slice=(72, 0), res_scale=0.7, ksplits=KSPLITS),
    # two k-steps: a split owns a single step; the epilogue fields through conv_bf16_splitk_epilogue
    _c('splitk_1x1', '128x64k64', 2, 128, 5, 5, (40,), k=1, pad=0, res_slice=(64, 8), res_scale=0.7, lo=True,
       out_slice=(56, 8), ksplits=(0, 2, 1000)),
)
_WIDE = (
    _c('w_72of96', '128x128k64', 2, 72, 91, 91, (130,), x_slice=(96, 8)),
    _c('w_16', '128x128k64', 2, 16, 91, 91, (130,), relu=False),
    _c('w_136_1x1', '128x128k64', 2, 136, 64, 64, (512,), k=1, pad=0, x_slice=(152, 8), res_slice=(536, 8), res_scale=0.5, lo=True,
       out_slice=(536, 8)),
    _c('w_64_1x1', '128x128k64', 2, 64, 64, 64, (392,), k=1, pad=0),             # tail-free; a last cout tile of 8 channels
)
# the rows of test_gpu_bf16.BIG_CASES (residual * 0.5, output at offset 8 of cout + 24), one of them in a wider input buffer
_BIG_BASE = (
    _c('big_128', '256x256k32', 2, 128, 19, 19, (256,), res_slice=(256, 0), res_scale=0.5, out_slice=(280, 8), env=BIG_ON),
    _c('big_192_1x1', '256x256k32', 1, 192, 27, 21, (512,), k=1, pad=0, res_slice=(512, 0), res_scale=0.5, out_slice=(536, 8),
       env=BIG_ON),
    _c('big_72s2', '256x256k32', 3, 72, 13, 13, (256,), stride=2, res_slice=(256, 0), res_scale=0.5, out_slice=(280, 8), env=BIG_ON),
    _c('big_72of104', '256x256k32', 3, 72, 13, 13, (256,), stride=2, x_slice=(104, 16), env=BIG_ON),
    _c('big_256_dil6', '256x256k32', 1, 256, 20, 20, (768,), pad=6, dil=6, res_slice=(768, 0), res_scale=0.5, out_slice=(792, 8),
       env=BIG_ON),
    _twin(_WIDE[2], 'big_136_1x1', '256x256k32', BIG_ON),
)
BIG_PAIRS = tuple((b.name, b.name + '_small') for b in _BIG_BASE)
_BIG = _BIG_BASE + tuple(_twin(b, b.name + '_small', '128x128k64' if b.cin == 136 else '128x64k64', BIG_OFF) for b in _BIG_BASE)
_OTHER = (
    _twin(_SHORTK[0], 'sk_64_96_k64', '128x64k64', (('CTDET_BF16_SHORTK', '0'),)),
) + tuple(_twin(w, w.name + '_ring', '128x128k32', (('CTDET_BF16_BK', '32'),)) for w in _WIDE)

CASES = _IMG + _SHORTK + _K64 + _WIDE + _BIG + _OTHER
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def segments(case):
    """[(co_begin, co_end, base, floats per image)] of a head row, as test_gpu_bf16.py lays them out: part i is segment i, written
    channels-last at `base` of a longer row."""
    out, c0 = [], 0
    for c in case.parts:
        out.append((c0, c0 + c, 7 * c, 7 * c + case.oh * case.ow * c + 5 * c))
        c0 += c
    return out


def fill_geometry(case, d):
    """The shape, slice and epilogue-flag fields of a ct_conv_desc (ctdet._lib.ConvDesc) for the row; the pointers, the segments
    and the split-K fields are the caller's."""
    d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = case.B, case.cin, case.H, case.W, case.x_ctot, case.x_coff
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = case.cout, case.k, case.k, case.stride, case.pad, case.pad, case.dil
    d.oh, d.ow, d.out_ctot, d.out_coff, d.relu = case.oh, case.ow, case.out_ctot, case.out_coff, int(case.relu)
    d.nseg = len(case.parts) if case.segs else 0
    if case.res_slice:
        d.res_ctot, d.res_coff, d.res_scale = case.res_slice[0], case.res_slice[1], case.res_scale
    return d


@dataclass(frozen=True)
class Inputs:
    x_buf: torch.Tensor             # [B, x_ctot, H, W] fp32, finite everywhere; x = channels [x_coff, x_coff + cin)
    parts: Tuple                    # weight [cout_i, cin, k, k] fp32 per part
    scale: torch.Tensor
    shift: torch.Tensor
    lo: Optional[torch.Tensor]
    res_buf: Optional[torch.Tensor]         # [B, res_ctot, oh, ow] fp32; the residual = channels [res_coff, res_coff + cout)


def _base(case):
    return BY_NAME[case.inputs_of] if case.inputs_of else case


@functools.lru_cache(maxsize=None)
def _make_inputs(case):
    g = torch.Generator().manual_seed(zlib.crc32(('bf16/' + case.name).encode()) % 100000)
    x_buf = torch.randn(case.B, case.x_ctot, case.H, case.W, generator=g)
    sc = (2.0 / (case.cin * case.k * case.k)) ** 0.5
    parts = tuple(torch.randn(c, case.cin, case.k, case.k, generator=g) * sc for c in case.parts)
    scale = torch.rand(case.cout, generator=g) * 0.5 + 0.75
    shift = torch.rand(case.cout, generator=g) - 0.5
    lo = None
    if case.lo:
        lo = torch.zeros(case.cout)
        lo[1::2] = float('-inf')
        lo[2] = 0.25
    res_buf = torch.randn(case.B, case.res_slice[0], case.oh, case.ow, generator=g) if case.res_slice else None
    return Inputs(x_buf, parts, scale, shift, lo, res_buf)


def make_inputs(case):
    """Seeded float32 inputs of a row (computed once, never written)."""
    return _make_inputs(_base(case))


def trunc_bf16(t):
    """t with every value truncated (rounded toward zero) to a bfloat16 value."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def rne_bf16(t):
    return t.bfloat16().float()


def fused_step(case, dtype, x=None, w=None, res=None, lo='row', acc=None):
    """The fused step of a row in `dtype` on bfloat16-rounded operands -> [B, cout, oh, ow].  The keyword arguments replace an
    operand (already rounded, fp32) or a stage, for the mutated references: x, w, res (the residual itself), lo (None: the floor
    of the ReLU flag alone), acc (a function applied to the plain convolution in front of the epilogue)."""
    inp = make_inputs(case)
    if x is None:
        x = rne_bf16(inp.x_buf[:, case.x_coff:case.x_coff + case.cin])
    if w is None:
        w = rne_bf16(torch.cat(inp.parts))
    if res is None and case.res_slice:
        res = rne_bf16(inp.res_buf[:, case.res_slice[1]:case.res_slice[1] + case.cout])
    z = F.conv2d(x.to(dtype), w.to(dtype), None, case.stride, case.pad, case.dil)
    if acc is not None:
        z = acc(z)
    v = lambda t: t.to(dtype).view(1, -1, 1, 1)
    y = z * v(inp.scale) + v(inp.shift)
    if res is not None:
        y = y * torch.tensor(case.res_scale, dtype=torch.float32).to(dtype) + res.to(dtype)
    floor = inp.lo if (isinstance(lo, str) and inp.lo is not None) else None
    if floor is not None:
        return torch.maximum(y, v(floor))
    return F.relu(y) if case.relu else y


@functools.lru_cache(maxsize=None)
def _ref64(case):
    return fused_step(case, torch.float64)


def ref64(case):
    """The fused step in float64: the ONLY reference of the bf16 convolution tests."""
    return _ref64(_base(case))


@functools.lru_cache(maxsize=None)
def _cpu32(case):
    return fused_step(case, torch.float32)


def cpu32(case):
    return _cpu32(_base(case))


def e32(case):
    """Per image: max|cpu32 - ref| / max|ref|."""
    r, y = ref64(case), cpu32(case)
    return [float((y[n].double() - r[n]).abs().max()) / (float(r[n].abs().max()) or 1.0) for n in range(case.B)]


def half_ulp(r):
    """2^(floor(log2|r|) - 8) of a float64 tensor, 0 where r = 0 (exponents below bfloat16's normal range count as its lowest)."""
    _m, e = torch.frexp(r.abs())            # |r| = m 2^e, m in [0.5, 1)
    h = torch.ldexp(torch.ones_like(r), (e - 1).clamp_min(-126) - 8)
    return torch.where(r == 0, torch.zeros_like(r), h)


def accum_term_of(r, y32):
    """A of the bound for ONE image: r its float64 reference, y32 the torch-CPU fp32 evaluation of the same step."""
    m = float(r.abs().max())
    e = float((y32.double() - r).abs().max()) / (m or 1.0)
    return max(TIGHT_FACTOR * e, TIGHT_FLOOR) * m


def accum_term(case):
    """A of the bound, per image."""
    r = ref64(case)
    return [max(TIGHT_FACTOR * e, TIGHT_FLOOR) * float(r[n].abs().max()) for n, e in enumerate(e32(case))]


@dataclass(frozen=True)
class Judged:
    violations: int                 # elements outside the bound
    share: float                    # ... as a share of the outputs
    excess: float                   # largest (|g - r| - h) / max|r| of an image
    err_over_e32: float             # ... over e32 of that image (floored at 2^-20 / 8)
    err_over_bound: float           # largest |g - r| / (h + A)


def judge(case, got):
    """got [B, cout, oh, ow] (bf16 values as fp32 or float64) against the row's reference under the bf16 bound."""
    r, A, e = ref64(case), accum_term(case), e32(case)
    g = got.double()
    bad, excess, ratio, ob = 0, 0.0, 0.0, 0.0
    for n in range(case.B):
        d, h = (g[n] - r[n]).abs(), half_ulp(r[n])
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
        bad += int((~(d <= h + A[n])).sum())
        m = float(r[n].abs().max()) or 1.0
        x = float((d - h).max()) / m
        excess = max(excess, x)
        ratio = max(ratio, x / max(e[n], TIGHT_FLOOR / TIGHT_FACTOR))
        ob = max(ob, float((d / (h + A[n])).max()))
    return Judged(bad, bad / r.numel(), excess, ratio, ob)


def judge_f32(case, got):
    """fp32 head-segment values [B, cout, oh, ow] -> (largest rel_err / bound over the images, largest rel_err, largest
    rel_err / e32): the tight bound max(8 e32, 2^-20) per image."""
    r, e = ref64(case), e32(case)
    worst, err, ratio = 0.0, 0.0, 0.0
    for n in range(case.B):
        d = (got[n].double() - r[n]).abs()
        x = float(torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf'))).max()) / (float(r[n].abs().max()) or 1.0)
        worst = max(worst, x / max(TIGHT_FACTOR * e[n], TIGHT_FLOOR))
        err = max(err, x)
        ratio = max(ratio, x / max(e[n], TIGHT_FLOOR / TIGHT_FACTOR))
    return worst, err, ratio


def old_close(got, want32):
    """The criterion tests/test_gpu_bf16.py used before this table: against the bf16-rounded torch-CPU fp32 result."""
    want = rne_bf16(want32)
    return bool(((got.float() - want).abs() <= want.abs() * 2 ** -7 + 2e-5 * want.abs().max()).all())
