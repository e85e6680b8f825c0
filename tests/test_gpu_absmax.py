"""The producer side of the f16x2 operand form's per-image maxima (ct_conv_desc.out_absmax, ct_absmax_f32; include/ctdet.h,
csrc/ct_f16x2.h): every kernel the header lists as honouring out_absmax leaves, in word 0 of image n's line,

    max(seed[n], max |y[n, out_coff : out_coff + cout]|)        y = what the launch itself stored, NaN skipped

BIT FOR BIT (an exact consistency property of one launch, not a tolerance; y itself is held to an fp64 torch-CPU convolution at
TOL), touches no other word of the line and no channel outside its slice; every kernel listed as ignoring it leaves the
slot as seeded.  A consumer scales its binary16 pieces by these values with a factor 2 of headroom, so a tracker that misses a
lane, an image, the negative side or a chunk of the batch goes unnoticed on randn data end to end -- and overflows on real ones.

Not covered: CTDET_VALU_PPT=1 (the switch is read once per process; the default form of the 'valu' kernel is tested)."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from ctdet import _lib, engine
from ctdet.wino_forms import FORMS
from test_gpu_kernels import _bn, _cuda

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4
LW = _lib.ABSMAX_LINE_BYTES // 4
SENTINEL = 0x5A5A0000


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('the gpu tests need a HIP device; none visible')


def _bits(v):
    return torch.as_tensor(v, dtype=torch.float32).reshape(-1).view(torch.int32)


def _slot(B, seed=0.0):
    """B lines; word 0 = the bit pattern of seed[n] (a scalar or one value per image), words 1..31 = a sentinel per word."""
    s = (SENTINEL + torch.arange(B * LW, dtype=torch.int32)).view(B, LW).clone()
    s[:, 0] = _bits(torch.as_tensor(seed, dtype=torch.float32).expand(B).contiguous())
    return s


def _launch(x, parts, stride, pad, dil, *, config=0, x3=None, ksplit=None, seed=0.0, res=None, res_scale=1.0, cin_off=0, cin=None,
            out_ctot=None, out_coff=0, pool=None, segs=None, transposed=False, track=True, in_absmax=None):
    """One conv step through engine.HipBackend with a caller-owned slot in desc.out_absmax.  parts: (weight, bias, bn, relu).
    pool = (ceil, write_full); segs = [(name, co_begin, co_end, base)] + flat sizes -> the three head buffers; in_absmax: caller-owned
    device lines for desc.in_absmax (else the engine's own: HipBackend.run_conv).
    -> dict(y, slot, seeded, pooled, flat)"""
    be = engine.HipBackend(DEV)
    cps = []
    for (w, b, bn, relu) in parts:
        bnm = None
        if bn is not None:
            bnm = torch.nn.BatchNorm2d(w.shape[0], eps=1e-5).to(DEV)
            bnm.weight.data.copy_(bn[0]); bnm.bias.data.copy_(bn[1])
            bnm.running_mean.copy_(bn[2]); bnm.running_var.copy_(bn[3])
        cps.append(engine.ConvPart(torch.nn.Parameter(_cuda(w), requires_grad=False),
                                   torch.nn.Parameter(_cuda(b), requires_grad=False) if b is not None else None, bnm, relu))
    kh, kw = parts[0][0].shape[2:]
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    B, ctot, H, W = x.shape
    cin = cin if cin is not None else ctot - cin_off
    st = engine.ConvStep('t', cps, cin, kh, kw, stride, ph, pw, dil, 'x', cin_off, H, W, None if segs else 'y', out_coff)
    bufs = {'x': _cuda(x)}
    if segs:
        st.segs = [engine.Segment(n, c0, c1, c1 - c0, base) for (n, c0, c1, base, _) in segs]
        for (n, c0, c1, base, size) in segs:
            bufs[n] = torch.full((B, size), float('nan'), device=DEV)
    else:
        bufs['y'] = torch.full((B, out_ctot or st.cout, st.oh, st.ow), float('nan'), device=DEV)
    if res is not None:
        bufs['r'] = _cuda(res)
        st.res, st.res_coff, st.res_scale = 'r', 0, res_scale
    st.rt['config'] = config
    be.prepare_conv(st, bufs, B)
    d = st.rt['desc']
    if ksplit is not None:
        d.ksplit = ksplit
        st.rt['ksws'].fill_(float('nan'))
    if x3 is not None:
        be.enable_x3(st, x3)
    pooled = None
    if pool is not None:
        ceil, full = pool
        poh, pow_ = (-(-H // 2), -(-W // 2)) if ceil else (H // 2, W // 2)
        pooled = torch.full((B, st.cout, poh, pow_), float('nan'), device=DEV)
        st.rt['pool'] = (pooled, poh, pow_, bool(full))
    if transposed:
        d.transposed = 1
    if in_absmax is not None:
        d.in_absmax = in_absmax.data_ptr()
    seeded = _slot(B, seed)
    slot = seeded.to(DEV)
    if track:
        d.out_absmax = slot.data_ptr()
    be.run_conv(st)
    torch.cuda.synchronize()
    return dict(y=None if segs else bufs['y'].cpu(), slot=slot.cpu(), seeded=seeded, pooled=None if pooled is None else pooled.cpu(),
                flat={n: bufs[n].cpu() for (n, *_r) in (segs or [])}, cout=st.cout)


def _amax(t):
    """per-image max |t| with NaN skipped (ct_f16x2.h, track_absmax), as float32 [B]"""
    a = t.reshape(t.shape[0], -1).abs()
    return torch.where(torch.isnan(a), torch.zeros_like(a), a).amax(1)


def _check_slot(r, stored, tag):
    """slot[n] == max(seed[n], max |stored[n]|) bit for bit; words 1..31 untouched."""
    seed = r['seeded'][:, 0].contiguous().view(torch.float32)
    want = torch.maximum(seed, _amax(stored))
    got = r['slot'][:, 0].contiguous()
    assert torch.equal(got, _bits(want)), (tag, got.view(torch.float32).tolist(), want.tolist())
    assert torch.equal(r['slot'][:, 1:], r['seeded'][:, 1:]), (tag, 'words 1..31 of a line were written')


def _check(r, want64, tag, out_coff=0):
    y, c = r['y'], r['cout']
    sl = y[:, out_coff:out_coff + c]
    assert torch.isnan(y[:, :out_coff]).all() and torch.isnan(y[:, out_coff + c:]).all(), (tag, 'channels outside the slice')
    fin = torch.isfinite(want64)
    assert torch.equal(torch.isfinite(sl), fin), tag
    assert rel_err(torch.where(fin, sl.double(), 0.0), torch.where(fin, want64, 0.0)) < TOL, tag
    _check_slot(r, sl, tag)


def _ref(x, parts, stride, pad, dil, res=None, res_scale=1.0):
    outs = []
    for (w, b, bn, relu) in parts:
        y = F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride, pad, dil)
        if bn is not None:
            y = F.batch_norm(y, bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.0, 1e-5)
        if res is not None:
            y = y * res_scale + res.double()
        outs.append(F.relu(y) if relu else y)
    return torch.cat(outs, 1)


def _names():
    lib = _lib.lib()
    return ([lib.ct_conv_config_name(i).decode() for i in range(lib.ct_conv_num_configs())],
            [lib.ct_conv_x3_config_name(i).decode() for i in range(lib.ct_conv_x3_num_configs())])


def _kernels(cin, kh, kw, stride, pad, dil, cout, splitk=True, wino=True):
    """Every launch form that honours out_absmax and takes this geometry: (tag, keyword arguments of _launch)."""
    lib = _lib.lib()
    direct, x3 = _names()
    out = [('direct:heuristic', dict(config=0))]
    for i, n in enumerate(direct):
        if n == 'valu' and not (cin == 3 and (kh, kw) == (3, 3) and cout % 8 == 0):
            continue
        out.append(('direct:' + n, dict(config=i + 1)))
        if splitk and n != 'valu':
            out.append(('direct:%s/ksplit3' % n, dict(config=i + 1, ksplit=3)))          # the finishing kernel tracks
    for j, n in enumerate(x3):
        if cin % lib.ct_conv_x3_config_bk(j):
            continue
        out.append((n, dict(x3=j)))
        if splitk:
            out.append((n + '/ksplit3', dict(x3=j, ksplit=3)))
    plain = (kh, kw, stride) == (3, 3, 1) and pad == dil and cin % 16 == 0
    if wino and plain:
        out += [('wino44', dict(config=engine.WINO4S)), ('wino47', dict(config=engine.WINO4H))]
        if dil == 1:
            out.append(('wino48', dict(config=engine.WINO4FH)))
    return out


GEOS = [  # name, B, Cin, H, W, Cout, k, stride, pad, dil -- the ragged shapes of tests/test_gpu_wino.py CASES and the other layer kinds
    ('one_pixel', 2, 32, 1, 1, 5, 3, 1, 1, 1), ('row', 2, 32, 1, 9, 33, 3, 1, 1, 1), ('col', 2, 32, 7, 1, 33, 3, 1, 1, 1),
    ('odd_hw', 3, 32, 19, 17, 70, 3, 1, 1, 1), ('many_tiles', 4, 32, 150, 150, 8, 3, 1, 1, 1),
    ('cout_156', 2, 32, 10, 10, 156, 3, 1, 1, 1), ('tiny_b8', 8, 32, 3, 3, 24, 3, 1, 1, 1), ('tiny_b8_2x2', 8, 64, 2, 2, 70, 3, 1, 1, 1),
    ('s2', 2, 32, 19, 19, 40, 3, 2, 1, 1), ('1x1', 3, 64, 10, 10, 70, 1, 1, 0, 1), ('1x1s2', 2, 32, 19, 19, 96, 1, 2, 0, 1),
    ('1x3', 2, 32, 12, 11, 24, (1, 3), 1, (0, 1), 1), ('3x1', 2, 32, 12, 11, 24, (3, 1), 1, (1, 0), 1),
    ('dil3', 2, 32, 19, 19, 40, 3, 1, 3, 3), ('dil6_odd', 3, 32, 19, 17, 70, 3, 1, 6, 6),
    ('one_image_many_wgs', 1, 32, 75, 75, 64, 3, 1, 1, 1),
]


@pytest.mark.parametrize('geo', GEOS, ids=[g[0] for g in GEOS])
def test_every_tracking_kernel_every_geometry(geo):
    """No ReLU, signed outputs, images at different scales (a maximum landing in the wrong line shows), lines seeded with a
    different tiny value per image (always raised), into a channel slice of a NaN-filled buffer."""
    name, B, Cin, H, W, Cout, k, stride, pad, dil = geo
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 1000)
    kh, kw = (k, k) if isinstance(k, int) else k
    x = torch.randn(B, Cin, H, W, generator=g) * (3.0 ** torch.arange(B).view(B, 1, 1, 1))
    w = torch.randn(Cout, Cin, kh, kw, generator=g) * (2.0 / (Cin * kh * kw)) ** 0.5
    b = torch.rand(Cout, generator=g) - 0.5
    parts = [(w, b, None, False)]
    want = _ref(x, parts, stride, pad, dil)
    seed = [1e-30 * (n + 1) for n in range(B)]
    ks = _kernels(Cin, kh, kw, stride, pad, dil, Cout)
    assert len(ks) >= 20
    for tag, kwargs in ks:
        r = _launch(x, parts, stride, pad, dil, seed=seed, out_ctot=Cout + 7, out_coff=3, **kwargs)
        _check(r, want, (name, tag), out_coff=3)


def test_valu_image_layer():
    direct, _ = _names()
    valu = 1 + direct.index('valu')
    g = torch.Generator().manual_seed(3)
    for (B, H, W, Cout, stride, pad, dil) in ((2, 37, 41, 24, 1, 1, 1), (3, 37, 41, 24, 2, 1, 1), (8, 5, 5, 8, 1, 1, 1), (1, 75, 75, 64, 1, 2, 2)):
        x = torch.randn(B, 3, H, W, generator=g) * (3.0 ** torch.arange(B).view(B, 1, 1, 1))
        w = torch.randn(Cout, 3, 3, 3, generator=g) * 0.2
        parts = [(w[:Cout // 2], None, _bn(Cout // 2, g), True), (w[Cout // 2:], torch.rand(Cout - Cout // 2, generator=g) - 2.0, None, False)]
        r = _launch(x, parts, stride, pad, dil, config=valu, seed=[1e-30 * (n + 1) for n in range(B)], out_ctot=Cout + 5, out_coff=2)
        _check(r, _ref(x, parts, stride, pad, dil), ('valu', B, H, W), out_coff=2)


def test_negative_winner_in_every_corner():
    """No ReLU and the extreme value NEGATIVE (|.| forgotten), at a different channel and position per image: the four corners of
    (pixel, channel) space, the last image among them.  The winner comes in through the residual, so its place is exact."""
    B, Cin, H, W, Cout = 4, 32, 10, 7, 70
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05
    parts = [(w, None, None, False)]
    spots = [(0, 0, 0), (Cout - 1, H - 1, W - 1), (0, H - 1, W - 1), (Cout - 1, 0, 0)]       # image n: (channel, row, column)
    res = torch.randn(B, Cout, H, W, generator=g)
    for n, (c, py, px) in enumerate(spots):
        res[n, c, py, px] = -1000.0 * (n + 1)
    want = _ref(x, parts, 1, 1, 1, res=res, res_scale=0.5)
    for tag, kwargs in _kernels(Cin, 3, 3, 1, 1, 1, Cout):
        r = _launch(x, parts, 1, 1, 1, res=res, res_scale=0.5, **kwargs)
        _check(r, want, tag)
        got = r['slot'][:, 0].contiguous().view(torch.float32)
        for n, (c, py, px) in enumerate(spots):
            v = float(r['y'][n, c, py, px])
            assert v < -900.0 * (n + 1) and float(got[n]) == -v, (tag, n, v, float(got[n]))


def test_seeded_lines():
    """A line holding more than any output survives, one holding less is raised, and each image has its own."""
    B, Cin, H, W, Cout = 4, 32, 9, 9, 40
    g = torch.Generator().manual_seed(10)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05
    parts = [(w, None, _bn(Cout, g), False)]
    want = _ref(x, parts, 1, 1, 1)
    lim = float(want.abs().max())
    seed = [1e30, 0.0, 1e-30, lim * 0.5]
    for tag, kwargs in _kernels(Cin, 3, 3, 1, 1, 1, Cout):
        r = _launch(x, parts, 1, 1, 1, seed=seed, **kwargs)
        _check(r, want, tag)
        got = r['slot'][:, 0].contiguous().view(torch.float32)
        assert float(got[0]) == float(torch.tensor(1e30)) and 0 < float(got[1]) <= lim * 1.001 and float(got[2]) > 1e-3, (tag, got)


def test_multi_part_epilogues_and_residual():
    g = torch.Generator().manual_seed(11)
    B, Cin, H, W = 3, 32, 11, 13
    x = torch.randn(B, Cin, H, W, generator=g) * (3.0 ** torch.arange(B).view(B, 1, 1, 1))
    w1, w2, w3 = (torch.randn(c, Cin, 3, 3, generator=g) * 0.05 for c in (40, 24, 6))
    parts = [(w1, None, _bn(40, g), True), (w2, torch.rand(24, generator=g) - 3.0, None, False), (w3, None, _bn(6, g), True)]
    want = _ref(x, parts, 1, 1, 1)
    res = torch.randn(B, 70, H, W, generator=g) * 4
    one = [(torch.cat([w1, w2, w3]), None, _bn(70, g), True)]
    want_res = _ref(x, one, 1, 1, 1, res=res, res_scale=0.3)
    for tag, kwargs in _kernels(Cin, 3, 3, 1, 1, 1, 70):
        _check(_launch(x, parts, 1, 1, 1, seed=1e-30, **kwargs), want, (tag, 'mixed'))
        _check(_launch(x, one, 1, 1, 1, res=res, res_scale=0.3, out_ctot=80, out_coff=10, **kwargs), want_res, (tag, 'res'), out_coff=10)


def test_head_scatter_segments():
    """nseg > 0: the slot bounds what went into the three flattened head buffers."""
    g = torch.Generator().manual_seed(21)
    B, Cin, H, W, A, Cc = 3, 32, 10, 9, 6, 7
    x = torch.randn(B, Cin, H, W, generator=g) * (3.0 ** torch.arange(B).view(B, 1, 1, 1))
    ws = [torch.randn(A * n, Cin, 3, 3, generator=g) * 0.06 for n in (4, Cc, 2)]
    bs = [torch.rand(A * n, generator=g) - 0.5 for n in (4, Cc, 2)]
    parts = [(w, b, None, False) for w, b in zip(ws, bs)]
    pbase, P = 11, 11 + H * W * A + 5
    segs = [('loc', 0, A * 4, pbase * 4, P * 4), ('conf', A * 4, A * (4 + Cc), pbase * Cc, P * Cc),
            ('obj', A * (4 + Cc), A * (6 + Cc), pbase * 2, P * 2)]
    want = _ref(x, parts, 1, 1, 1)
    for tag, kwargs in _kernels(Cin, 3, 3, 1, 1, 1, A * (6 + Cc), splitk=False):
        r = _launch(x, parts, 1, 1, 1, segs=segs, seed=1e-30, **kwargs)
        stored = []
        for (n, c0, c1, base, size) in segs:
            flat, cnt = r['flat'][n], H * W * (c1 - c0)
            assert torch.isnan(flat[:, :base]).all() and torch.isnan(flat[:, base + cnt:]).all(), (tag, n)
            assert rel_err(flat[:, base:base + cnt], want[:, c0:c1].permute(0, 2, 3, 1).reshape(B, -1)) < TOL, (tag, n)
            stored.append(flat[:, base:base + cnt])
        _check_slot(r, torch.cat(stored, 1), tag)


@pytest.mark.parametrize('W', [engine.WINO4S, engine.WINO4H, engine.WINO4FH], ids=['wino44', 'wino47', 'wino48'])
@pytest.mark.parametrize('case', [(2, 32, 19, 17, 70, False), (3, 16, 23, 18, 33, True), (8, 16, 3, 3, 8, True), (1, 32, 38, 38, 24, False)])
def test_fused_pool_slot_bounds_the_full_resolution_output(case, W):
    """rt['pool']: _wire_absmax lets the pooled buffer share the producer's slot, so the slot must bound the FULL-resolution map
    (floor-mode pooling drops the last row / column of an odd map) -- also when that map is not written (write_full = 0)."""
    B, Cin, H, Wd, Cout, ceil = case
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, Cin, H, Wd, generator=g) * (3.0 ** torch.arange(B).view(B, 1, 1, 1))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.08
    parts = [(w, torch.rand(Cout, generator=g) - 0.5, None, True)]
    want = _ref(x, parts, 1, 1, 1)
    full = _launch(x, parts, 1, 1, 1, config=W, pool=(ceil, 1), seed=1e-30)
    _check(full, want, 'full')
    assert torch.equal(F.max_pool2d(full['y'], 2, 2, 0, ceil_mode=ceil), full['pooled'])
    skip = _launch(x, parts, 1, 1, 1, config=W, pool=(ceil, 0), seed=1e-30)
    assert torch.isnan(skip['y']).all() and torch.equal(skip['pooled'], full['pooled'])
    assert torch.equal(skip['slot'], full['slot'])


def test_nan_inf_and_all_zero_images():
    """ct_f16x2.h: a NaN is skipped (the line holds the maximum of the image's other values), an Inf becomes the maximum, an
    all-zero image leaves its line as seeded -- and none of it touches the neighbours' lines."""
    B, Cin, H, W, Cout = 5, 32, 9, 9, 40
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, Cin, H, W, generator=g)
    x[2] = 0.0
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05
    parts = [(w, None, None, False)]
    res = torch.zeros(B, Cout, H, W)
    res[1, Cout - 1, H - 1, W - 1] = float('nan')
    res[3, 0, 4, 4] = float('-inf')
    want = _ref(x, parts, 1, 1, 1, res=res)
    seed = [0.0, 0.0, 1e-30, 0.0, 1e-30]
    inf_bits = int(_bits(float('inf'))[0])
    for tag, kwargs in _kernels(Cin, 3, 3, 1, 1, 1, Cout):
        r = _launch(x, parts, 1, 1, 1, res=res, seed=seed, **kwargs)
        _check(r, want, tag)
        got = r['slot'][:, 0]
        assert int(got[3]) == inf_bits and int(got[2]) == int(_bits(1e-30)[0]), (tag, got)
        assert torch.isnan(r['y'][1, Cout - 1, H - 1, W - 1]) and 0 < float(got[1:2].contiguous().view(torch.float32)) < 10.0, tag


def test_kernels_that_ignore_out_absmax_leave_the_slot_alone():
    """The negative side of include/ctdet.h, which _wire_absmax's tracks() relies on: FORMS[c].tracks against what every Winograd
    form does with a slot, and a data-gradient launch of the direct kernel."""
    B, Cin, H, W, Cout = 2, 32, 12, 12, 32
    g = torch.Generator().manual_seed(13)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05
    parts = [(w, None, None, True)]
    want = _ref(x, parts, 1, 1, 1)
    assert sorted(FORMS) == [2, 4, 23, 44, 46, 47, 48]
    for code, f in FORMS.items():
        r = _launch(x, parts, 1, 1, 1, config=f.config, seed=[1e-30, 2e-30])
        assert rel_err(r['y'], want) < TOL, code
        wrote = not torch.equal(r['slot'], r['seeded'])
        assert wrote == f.tracks, (code, 'FORMS[%d].tracks = %s, the kernel %s the slot' % (code, f.tracks, 'wrote' if wrote else 'left'))
        if f.tracks:
            _check(r, want, code)
    r = _launch(x, parts, 1, 1, 1, config=1, ksplit=0, transposed=True, seed=[1e-30, 2e-30])          # some convolution of x: only the slot matters
    assert torch.isfinite(r['y']).all() and torch.equal(r['slot'], r['seeded'])


CHUNKED = [('direct', dict(config=0)), ('x3', dict(x3='x3:128x128k16d')), ('h2', dict(x3='h2:128x128k16d')), ('wino44', dict(config=engine.WINO4S)),
           ('wino47', dict(config=engine.WINO4H)), ('wino48', dict(config=engine.WINO4FH))]


@pytest.mark.parametrize('tag,kwargs', CHUNKED, ids=[c[0] for c in CHUNKED])
def test_chunked_batch_fills_every_image_line(tag, kwargs):
    """The launchers split a batch whose input exceeds the 32-bit buffer descriptors (kMaxBufBytes = 0x7FFFFF00) and offset the
    slot by b0 lines per chunk (ct_conv.hip, ct_conv_x3.hip, ct_wino4s.hip, ct_wino4f.hip).  img_in_bytes counts the whole
    in_ctot-channel buffer: a 16-channel slice of a [3, 262160, 32, 32] device buffer is 1 073 807 360 bytes per image, more than
    half the limit -> max_chunk = 1, THREE chunks of one image.  Only the slice is initialised and referenced."""
    B, ctot, H, Cin, coff, Cout = 3, 262160, 32, 16, 131072, 24
    assert ctot * H * H * 4 > 0x7FFFFF00 // 2 and ctot * H * H * 4 < 0x7FFFFF00
    if 'x3' in kwargs:
        kwargs = dict(x3=_names()[1].index(kwargs['x3']))
    g = torch.Generator().manual_seed(14)
    xs = torch.randn(B, Cin, H, H, generator=g) * (5.0 ** torch.arange(B).view(B, 1, 1, 1))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1
    parts = [(w, None, None, False)]
    xd = torch.empty((B, ctot, H, H), device=DEV)
    xd[:, coff:coff + Cin] = xs.to(DEV)
    r = _launch(xd, parts, 1, 1, 1, cin_off=coff, cin=Cin, seed=[1e-30, 2e-30, 3e-30], **kwargs)
    del xd
    torch.cuda.empty_cache()
    _check(r, _ref(xs, parts, 1, 1, 1), tag)
    got = r['slot'][:, 0].contiguous().view(torch.float32)
    assert float(got[0]) < float(got[1]) < float(got[2]), got


# ------------------------------------------------------------------ ct_absmax_f32
def _absmax(buf, base_off, batch, per_image, img_stride, seed=0.0):
    """buf: flat device fp32 tensor; the slice of image n starts at base_off + n * img_stride."""
    seeded = _slot(batch, seed)
    slot = seeded.to(DEV)
    _lib.check(_lib.lib().ct_absmax_f32(buf.data_ptr() + 4 * base_off, batch, per_image, img_stride, slot.data_ptr(), None), 'ct_absmax_f32')
    torch.cuda.synchronize()
    return slot.cpu(), seeded


def _want_lines(flat, base_off, batch, per_image, img_stride, seed=0.0):
    idx = base_off + torch.arange(batch).view(-1, 1) * img_stride + torch.arange(per_image).view(1, -1)
    m = flat[idx].abs().amax(1)
    return torch.maximum(m, torch.as_tensor(seed, dtype=torch.float32).expand(batch))


@pytest.mark.parametrize('per_image', [1, 3, 4, 4095, 4096, 4097, 3 * 4096 + 5])
@pytest.mark.parametrize('layout', ['packed', 'slice', 'unaligned'])
def test_absmax_f32_sizes_and_layouts(per_image, layout):
    """packed: img_stride = per_image; slice: a channel slice of a wider buffer (the vector path where everything is a multiple
    of 4); unaligned: base pointer 4 bytes off a 16-byte boundary and a stride that is not a multiple of 4 (vec_ok == 0)."""
    B = 3
    g = torch.Generator().manual_seed(per_image)
    stride = per_image if layout == 'packed' else (per_image + 3) // 4 * 4 + 8 if layout == 'slice' else per_image + 7 + (per_image % 2)
    off = 0 if layout == 'packed' else 4 if layout == 'slice' else 1
    if layout == 'unaligned' and stride % 4 == 0:
        stride += 1
    flat = torch.randn(off + B * stride + 8, generator=g)
    flat[:off] = 1e6                                  # what lies outside the slices is larger than anything inside
    for n in range(B):
        flat[off + n * stride + per_image: off + (n + 1) * stride] = 1e6
    flat[off + B * stride:] = 1e6
    pos = [0, per_image - 1, per_image // 2]          # winner first / last / middle, negative in images 0 and 1
    for n in range(B):
        flat[off + n * stride + pos[n]] = (-50.0 - n) if n < 2 else 70.0
    seed = [1e-30, 60.0, 0.0]                         # raised / survives (51 < 60) / zero
    got, seeded = _absmax(flat.to(DEV), off, B, per_image, stride, seed)
    want = _want_lines(flat, off, B, per_image, stride, seed)
    assert want.tolist() == [50.0, 60.0, 70.0]
    assert torch.equal(got[:, 0].contiguous(), _bits(want)), (got[:, 0].contiguous().view(torch.float32), want)
    assert torch.equal(got[:, 1:], seeded[:, 1:])


def test_absmax_f32_grid_stride_and_special_values():
    """items > 2048 (the grid-stride loop): 2100 images of 5 floats, and 3 images of 40 000 floats at 600 images; then the values
    around the sign bit and the exponent's ends: -0.0 (stays zero), a subnormal maximum, FLT_MAX, negative FLT_MAX."""
    g = torch.Generator().manual_seed(2)
    for (B, per, stride) in ((2100, 5, 5), (2100, 8, 12), (600, 40000, 40000)):
        flat = torch.randn(B * stride, generator=g) * (torch.arange(B * stride) % 97 + 1)
        got, seeded = _absmax(flat.to(DEV), 0, B, per, stride)
        assert torch.equal(got[:, 0].contiguous(), _bits(_want_lines(flat, 0, B, per, stride))), (B, per)
        assert torch.equal(got[:, 1:], seeded[:, 1:])
    sub, fmax = 2.0 ** -140, torch.finfo(torch.float32).max
    rows = torch.zeros(5, 16)
    rows[0, :] = -0.0
    rows[1, 3], rows[1, 15] = sub, -sub / 2
    rows[2, 0], rows[2, 7] = 1.0, fmax
    rows[3, 15], rows[3, 2] = -fmax, 3e38
    rows[4, 5], rows[4, 6] = -(2.0 ** -126), sub
    got, seeded = _absmax(rows.reshape(-1).to(DEV), 0, 5, 16, 16)
    want = torch.tensor([0.0, sub, fmax, fmax, 2.0 ** -126])
    assert torch.equal(got[:, 0].contiguous(), _bits(want)), got[:, 0]
    assert int(got[0, 0]) == 0 and torch.equal(got[:, 1:], seeded[:, 1:])
