"""bf16 channels-last path (BASELINE.json configs[4]): ct_conv2d_bf16_fwd against float64 convolutions of the bf16-rounded
operands under the bound of tests/conv_bf16_cases.py (the row table itself runs in tests/test_gpu_bf16_conv.py), and the whole
RFBNet through HipBackendBF16 against the fp32 path on the same weights."""
import ctypes as C
import types

import pytest
import torch
import torch.nn.functional as F

import conv_bf16_cases as T
from ctdet import _lib, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Want:
    """The float64 reference of a launch on the bf16-rounded operands and the accumulation term of the bound, per image."""

    def __init__(self, r, y32, bf16=True):
        self.r, self.y32, self.bf16 = r, y32, bf16
        self.A = torch.tensor([T.accum_term_of(r[n], y32[n]) for n in range(r.shape[0])], dtype=torch.float64)

    def seg(self, c0, c1):
        """Channels [c0, c1) as the head buffers hold them: [B, oh * ow * channels], channels last."""
        w = _Want.__new__(_Want)
        B = self.r.shape[0]
        w.r, w.y32, w.bf16, w.A = (self.r[:, c0:c1].permute(0, 2, 3, 1).reshape(B, -1), None, self.bf16, self.A)
        return w


def _close(got, want):
    """The bound of tests/conv_bf16_cases.py: |g - r| <= h(r) + A per image against the float64 value r -- h half a bf16 ulp of r
    (the one correct rounding; none for the fp32 head segments), A = max(8 e32, 2^-20) max|r| (fp32 accumulation in another
    order; e32: torch-CPU fp32 against r on that image)."""
    r = want.r
    A = want.A.view(-1, *([1] * (r.dim() - 1)))
    h = T.half_ulp(r) if want.bf16 else 0.0
    return bool(((got.double() - r).abs() <= h + A).all())


def _close_pair(got, want):
    """Two device results of the same sums in another order: one bf16 ulp plus the accumulation noise near zero."""
    return ((got - want).abs() <= want.abs() * 2 ** -7 + 2e-5 * want.abs().max()).all()


def _conv_bf16(x, parts, stride, pad, dil, relu, res=None, res_scale=1.0, out_ctot=None, out_coff=0, cin_off=0, cin=None,
               ksplit=0, segs=None):
    """x [B,ctot,H,W] fp32, parts = [w [Cout_i,Cin,k,k]]; -> [B, sum Cout, OH, OW] fp32 of the bf16 result.
    segs = [(co_begin, co_end, base, size)]: the multibox head form (fp32, channels-last per segment, rows of `size` floats per
    image, NaN-filled) -> the list of [B, size] buffers instead, and the reference before any rounding to bf16."""
    lib = _lib.lib()
    B, ctot, H, W = x.shape
    cin = cin if cin is not None else ctot - cin_off
    cpad = (ctot + 7) // 8 * 8
    kh, kw = parts[0].shape[2:]
    cout = sum(w.shape[0] for w in parts)
    OH = (H + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    xd = x.to(DEV).contiguous()
    xb = torch.empty(B * H * W * cpad, dtype=torch.int16, device=DEV)
    _lib.check(lib.ct_nchw_f32_to_nhwc_bf16(xd.data_ptr(), B, ctot, H * W, cpad, xb.data_ptr(), _s()), 'nhwc')
    wd = [w.to(DEV).contiguous() for w in parts]
    wp = torch.empty(lib.ct_conv_bf16_packed_elems(cin, cout, kh, kw), dtype=torch.int16, device=DEV)
    ptrs = (C.c_void_p * len(wd))(*[w.data_ptr() for w in wd])
    couts = (C.c_int * len(wd))(*[w.shape[0] for w in wd])
    _lib.check(lib.ct_conv_pack_weights_bf16(ptrs, couts, len(wd), cin, kh, kw, wp.data_ptr(), _s()), 'pack')
    gs = torch.Generator().manual_seed(1000 + cout)
    scale = (torch.rand(cout, generator=gs) * 0.5 + 0.75).to(DEV)
    shift = (torch.rand(cout, generator=gs) - 0.5).to(DEV)
    octot = out_ctot or cout
    yb = torch.full((B * OH * OW * octot,), 0x7FC0, dtype=torch.int16, device=DEV)       # bf16 NaN
    d = _lib.ConvDesc()
    d.in_ = xb.data_ptr()
    d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = B, (cpad if cin == ctot else cin), H, W, cpad, cin_off
    d.wpacked, d.scale, d.shift = wp.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil, d.oh, d.ow = cout, kh, kw, stride, pad, pad, dil, OH, OW
    d.out, d.out_ctot, d.out_coff, d.relu = yb.data_ptr(), octot, out_coff, int(relu)
    flats = [torch.full((B, size), float('nan'), device=DEV) for (_c0, _c1, _base, size) in segs or []]
    for g_, (c0, c1, base, size) in enumerate(segs or []):
        d.out, d.nseg = None, len(segs)
        sg = d.seg[g_]
        sg.ptr, sg.co_begin, sg.co_end, sg.pix_stride, sg.img_stride, sg.base = flats[g_].data_ptr(), c0, c1, c1 - c0, size, base
    rb = None
    if res is not None:
        rd = res.to(DEV).contiguous()
        rb = torch.empty(B * OH * OW * cout, dtype=torch.int16, device=DEV)
        _lib.check(lib.ct_nchw_f32_to_nhwc_bf16(rd.data_ptr(), B, cout, OH * OW, cout, rb.data_ptr(), _s()), 'res')
        d.res, d.res_ctot, d.res_coff, d.res_scale = rb.data_ptr(), cout, 0, res_scale
    if ksplit:
        ws = torch.full((16 * cout * B * OH * OW,), float('nan'), device=DEV)      # needs no initialisation
        d.ksplit, d.ksplit_ws, d.ksplit_ws_floats = ksplit, ws.data_ptr(), ws.numel()
    _lib.check(lib.ct_conv2d_bf16_fwd(C.byref(d), _s()), 'conv bf16')
    y = torch.empty(B, cout, OH, OW, device=DEV)
    _lib.check(lib.ct_nhwc_bf16_to_nchw_f32(yb.data_ptr(), B, cout, OH * OW, octot, out_coff, y.data_ptr(), _s()), 'back')
    torch.cuda.synchronize()
    xr, wr = x[:, cin_off:cin_off + cin].bfloat16().float(), torch.cat(parts).bfloat16().float()

    def ref(dt):
        y = F.conv2d(xr.to(dt), wr.to(dt), None, stride, pad, dil) * scale.cpu().to(dt).view(1, -1, 1, 1) + \
            shift.cpu().to(dt).view(1, -1, 1, 1)
        if res is not None:
            y = y * torch.tensor(res_scale, dtype=torch.float32).to(dt) + res.bfloat16().to(dt)
        return F.relu(y) if relu else y
    want = _Want(ref(torch.float64), ref(torch.float32), bf16=not segs)
    if segs:
        return [f.cpu() for f in flats], want, yb
    return y.cpu(), want, yb


CASES = [  # B, ctot, H, W, couts, k, stride, pad, dil
    (2, 64, 19, 19, (96,), 3, 1, 1, 1), (2, 40, 10, 11, (130,), 3, 2, 1, 1), (1, 128, 19, 19, (64,), 3, 1, 3, 3),
    (2, 256, 10, 10, (72,), 1, 1, 0, 1), (2, 3, 30, 30, (64,), 3, 1, 1, 1), (3, 96, 5, 5, (40, 24, 8), 1, 2, 0, 1),
    (2, 128, 2, 2, (256,), 4, 1, 1, 1), (2, 128, 3, 3, (256,), 3, 1, 0, 1), (1, 200, 38, 38, (128,), 3, 1, 5, 5),
]


@pytest.mark.parametrize('case', CASES, ids=[str(i) for i in range(len(CASES))])
def test_conv_bf16_vs_cpu(case):
    B, ctot, H, W, couts, k, stride, pad, dil = case
    g = torch.Generator().manual_seed(31 + ctot + H)
    x = torch.randn(B, ctot, H, W, generator=g)
    parts = [torch.randn(c, ctot, k, k, generator=g) * (2.0 / (ctot * k * k)) ** 0.5 for c in couts]
    got, want, _ = _conv_bf16(x, parts, stride, pad, dil, True)
    # same products, fp32 accumulation in another order, one final rounding to bf16: at most one bf16 ulp apart
    assert _close(got, want), (got - want.r).abs().max()


def test_conv_bf16_slices_and_residual():
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 96, 19, 19, generator=g)
    w = torch.randn(64, 48, 3, 3, generator=g) * 0.05
    res = torch.randn(2, 64, 19, 19, generator=g)
    got, want, yb = _conv_bf16(x, [w], 1, 2, 2, False, res=res, res_scale=0.5, out_ctot=104, out_coff=16, cin_off=32,
                               cin=48)
    assert _close(got, want)
    full = yb.view(2, 19, 19, 104)
    assert (full[..., :16] == 0x7FC0).all() and (full[..., 80:] == 0x7FC0).all()      # untouched channel slices


BIG_CASES = [  # B, ctot, H, W, cout, k, stride, pad, dil -- ragged pixel counts, several 256-wide cout tiles, a channel tail
    (2, 128, 19, 19, 256, 3, 1, 1, 1), (1, 192, 27, 21, 512, 1, 1, 0, 1), (3, 72, 13, 13, 256, 3, 2, 1, 1),
    (1, 256, 20, 20, 768, 3, 1, 6, 6),
]


@pytest.mark.parametrize('case', BIG_CASES, ids=[str(i) for i in range(len(BIG_CASES))])
def test_conv_bf16_256x256_tile(case, monkeypatch):
    """The 256 x 256 workgroup tile (eight waves of 128 x 64, epilogue staged in four row passes) forced on small
    geometries (CTDET_BF16_BIG_MIN=1: the launch rule normally wants a workgroup per CU): against the torch reference,
    and bit-identical to the 128-wide tiles on the same operands (same products, same k order per accumulator)."""
    B, ctot, H, W, cout, k, stride, pad, dil = case
    g = torch.Generator().manual_seed(11 + ctot + H)
    x = torch.randn(B, ctot, H, W, generator=g)
    w = torch.randn(cout, ctot, k, k, generator=g) * (2.0 / (ctot * k * k)) ** 0.5
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    res = torch.randn(B, cout, OH, OW, generator=g)
    monkeypatch.setenv('CTDET_BF16_BIG_MIN', '1')
    got, want, yb = _conv_bf16(x, [w], stride, pad, dil, True, res=res, res_scale=0.5, out_ctot=cout + 24, out_coff=8)
    assert _close(got, want), (got - want.r).abs().max()
    full = yb.view(B, OH, OW, cout + 24)
    assert (full[..., :8] == 0x7FC0).all() and (full[..., 8 + cout:] == 0x7FC0).all()      # untouched channel slices
    monkeypatch.setenv('CTDET_BF16_BIG_MIN', '1000000000')
    small, _, _ = _conv_bf16(x, [w], stride, pad, dil, True, res=res, res_scale=0.5, out_ctot=cout + 24, out_coff=8)
    assert torch.equal(got, small)


def test_conv_bf16_split_k():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 256, 5, 5, generator=g)
    w = torch.randn(72, 256, 3, 3, generator=g) * 0.03
    res = torch.randn(2, 72, 5, 5, generator=g)
    base, want, _ = _conv_bf16(x, [w], 1, 1, 1, True, res=res, res_scale=0.7)
    assert _close(base, want)
    for ks in (2, 5, 1000, -1):
        got, _, _ = _conv_bf16(x, [w], 1, 1, 1, True, res=res, res_scale=0.7, ksplit=ks)
        assert _close(got, want), ks
        again, _, _ = _conv_bf16(x, [w], 1, 1, 1, True, res=res, res_scale=0.7, ksplit=ks)
        assert torch.equal(got, again), 'split-K must be run-to-run deterministic'


def test_conv_bf16_split_k_into_head_segments():
    """nseg > 0 through conv_bf16_splitk_epilogue: batch 2, 64 channels, 5x5 map, 3x3 pad 1, segments of 24 + 12 + 6 = 42 output
    channels (a ragged last 32-channel block, segment boundaries inside and across the blocks), ksplit 3 against the unsplit launch
    and the torch reference; outside the segments nothing is written, and a second run is bit-equal."""
    g = torch.Generator().manual_seed(42)
    B, H, W, couts = 2, 5, 5, (24, 12, 6)
    x = torch.randn(B, 64, H, W, generator=g)
    parts = [torch.randn(c, 64, 3, 3, generator=g) * 0.06 for c in couts]
    segs, c0 = [], 0
    for c in couts:
        segs.append((c0, c0 + c, 7 * c, 7 * c + H * W * c + 5 * c))
        c0 += c
    unsplit, want, _ = _conv_bf16(x, parts, 1, 1, 1, False, segs=segs)
    split, _, _ = _conv_bf16(x, parts, 1, 1, 1, False, segs=segs, ksplit=3)
    again, _, _ = _conv_bf16(x, parts, 1, 1, 1, False, segs=segs, ksplit=3)
    assert (want.r < 0).any()
    for g_, (c0, c1, base, size) in enumerate(segs):
        cnt = H * W * (c1 - c0)
        ref = want.seg(c0, c1)
        for tag, flat in (('unsplit', unsplit[g_]), ('ksplit3', split[g_])):
            assert torch.isnan(flat[:, :base]).all() and torch.isnan(flat[:, base + cnt:]).all(), (tag, g_)
            assert _close(flat[:, base:base + cnt], ref), (tag, g_, (flat[:, base:base + cnt] - ref.r).abs().max())
        assert _close_pair(split[g_][:, base:base + cnt], unsplit[g_][:, base:base + cnt]), g_
        assert torch.equal(split[g_].view(torch.int32), again[g_].view(torch.int32)), 'split-K must be run-to-run deterministic'


def test_maxpool_nhwc_bf16():
    lib = _lib.lib()
    g = torch.Generator().manual_seed(8)
    for (C_, H, W, k, s, p, ceil) in [(64, 30, 30, 2, 2, 0, False), (16, 15, 13, 2, 2, 0, True), (24, 9, 9, 3, 1, 1, False),
                                      (12, 7, 7, 2, 2, 0, True)]:
        x = torch.randn(2, C_, H, W, generator=g).bfloat16().float()
        want = F.max_pool2d(x, k, s, p, ceil_mode=ceil)
        OH, OW = want.shape[2:]
        xd = x.to(DEV)
        xb = torch.empty(2 * H * W * C_, dtype=torch.int16, device=DEV)
        _lib.check(lib.ct_nchw_f32_to_nhwc_bf16(xd.data_ptr(), 2, C_, H * W, C_, xb.data_ptr(), _s()), 'nhwc')
        yb = torch.empty(2 * OH * OW * C_, dtype=torch.int16, device=DEV)
        _lib.check(lib.ct_maxpool2d_nhwc_bf16(xb.data_ptr(), yb.data_ptr(), 2, C_, H, W, OH, OW, k, s, p, _s()), 'pool')
        y = torch.empty(2, C_, OH, OW, device=DEV)
        _lib.check(lib.ct_nhwc_bf16_to_nchw_f32(yb.data_ptr(), 2, C_, OH * OW, C_, 0, y.data_ptr(), _s()), 'back')
        torch.cuda.synchronize()
        assert torch.equal(y.cpu(), want), (C_, H, W, k, s, p, ceil)


@pytest.mark.parametrize('size,phase,C', [(300, 1, 20), (300, 2, 60), (512, 1, 20)])
def test_rfbnet_bf16_vs_fp32(size, phase, C):
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=phase, setting='transfer'), size, C)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()))
    net = net.cuda().eval()
    net.device = 'cuda'
    x = synth.images(2, size, 'randn', 4321).to(DEV)
    def outputs():
        loc, conf, obj = net.forward_raw(x)
        if phase == 2:
            # with random weights the Context-Transformer softmax is near-argmax: a 1 % change of its logits flips
            # winners, so its output is not a meaningful bf16-vs-fp32 comparison; the conv stack is compared on the
            # raw conf logits the block consumes (forward(x, init=True), models/RFB_Net_vgg.py:250-251)
            conf = net.forward_raw(x, init=True)
        return [t.clone() for t in (loc, conf, obj)]
    with torch.no_grad():
        ref = outputs()
        net.conv_dtype = 'bf16'
        got = outputs()
    torch.cuda.synchronize()
    for name, a, b in zip(('loc', 'conf', 'obj'), got, ref):
        err = (a - b).abs().max().item() / b.abs().max().item()
        assert err < 3e-2, (name, err)          # bf16 activations through ~25 layers (measured 0.9e-2 .. 1.8e-2)
        assert err > 0, name                    # really the other path
    assert got[0].dtype == torch.float32


class _RoundedF:
    """torch.nn.functional with conv2d evaluated on bfloat16-ROUNDED activations and weights (fp32 arithmetic): what
    the bf16 engine stores between its fused launches.  Max-pooling commutes with the (monotonic) rounding, the
    epilogues run in fp32 on the fp32 accumulator in both."""

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def conv2d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        return F.conv2d(x.bfloat16().float(), w.bfloat16().float(), b, stride, padding, dilation, groups)


@pytest.mark.parametrize('size', [300, 512])
def test_rfbnet_bf16_vs_oracle_on_bf16_rounded_activations(size, monkeypatch):
    """the bf16 network against the ORACLE (not against the repo's own fp32 path).  Two oracle
    evaluations: exact fp32, and with every convolution input and weight rounded to bfloat16 -- the rounding points
    of the engine's NHWC bf16 storage.  Raw loc / conf / obj."""
    from models.RFB_Net_vgg import build_net
    from oracle import rfbnet_ref
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), size, 20)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()))
    net = net.cuda().eval()
    net.device = 'cuda'
    net.conv_dtype = 'bf16'
    x = synth.images(1, size, 'randn', 4321)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    with torch.no_grad():
        got = [t.cpu() for t in net.forward_raw(x.to(DEV))]
        exact = rfbnet_ref.forward(sd, x, size, 20, raw=True)
        monkeypatch.setattr(rfbnet_ref, 'F', _RoundedF())
        want = rfbnet_ref.forward(sd, x, size, 20, raw=True)
    for name, a, b, c in zip(('loc', 'conf', 'obj'), got, want, exact):
        dev = float((a.reshape(c.shape) - c).abs().max() / c.abs().max())     # device bf16 path vs the exact fp32 oracle
        own = float((b - c).abs().max() / c.abs().max())                      # rounded oracle vs the exact oracle
        # Rounding decisions decorrelate after a few layers (a last-bit difference of an accumulator flips a bf16
        # rounding), so the device and the rounded oracle are two samples of the same noise rather than close to
        # each other (measured: 7e-3 apart, each 7e-3 from exact).  The check that means something: the device is no
        # further from the EXACT oracle than bf16 storage itself puts the oracle, and far inside the 3e-2 budget.
        assert dev < 2.0 * own and dev < 3e-2, (name, dev, own)      # measured ratios 0.9 .. 1.6 (max-norm of 1e5..1e6 values)
        assert dev > 1e-4, name                     # really the bf16 path


def test_rfbnet512_bf16_at_the_benched_batch_vs_oracle(monkeypatch):
    """the bf16 engine at the shape bench.py times for BASELINE configs[4] (RFBNet-512, bs 16 per GPU -- the
    batch selects the 256 x 256 tile, csrc/ct_conv_bf16.hip) against the oracle on the first and the last image: exact
    fp32 and with every convolution operand rounded to bfloat16 (the criterion of the bs-1 test above)."""
    from models.RFB_Net_vgg import build_net
    from oracle import rfbnet_ref
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), 512, 20)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()))
    net = net.cuda().eval()
    net.device = 'cuda'
    net.conv_dtype = 'bf16'
    B = 16
    x = synth.images(B, 512, 'randn', 4321)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    pick = [0, B - 1]
    with torch.no_grad():
        got = [t.cpu()[pick] for t in net.forward_raw(x.to(DEV))]
        exact = rfbnet_ref.forward(sd, x[pick], 512, 20, raw=True)
        monkeypatch.setattr(rfbnet_ref, 'F', _RoundedF())
        want = rfbnet_ref.forward(sd, x[pick], 512, 20, raw=True)
    for name, a, b, c in zip(('loc', 'conf', 'obj'), got, want, exact):
        for i in range(2):
            dev = float((a[i].reshape(c[i].shape) - c[i]).abs().max() / c[i].abs().max())
            own = float((b[i] - c[i]).abs().max() / c[i].abs().max())
            assert dev < 2.0 * own and dev < 3e-2, (name, pick[i], dev, own)
            assert dev > 1e-4, (name, pick[i])
