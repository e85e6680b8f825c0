"""ct_conv2d_wgrad_h2 on the MI355X: the f16x2 weight gradient of the 1x1 convolutions against float64 autograd and against the
fp32 kernel it stands beside (ct_conv2d_wgrad), its determinism, its scaling rule, and the training step under CTDET_WGRAD_H2=1."""
import ctypes as C
import types

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from ctdet import _lib, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LINE = _lib.ABSMAX_LINE_BYTES // 4
GUARD = 4096            # floats / bytes of sentinel around dw and the workspace


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('the gpu tests need a HIP device; none visible')


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _desc(xbuf, B, cin, H, W, in_ctot, in_coff, cout, stride):
    d = _lib.ConvDesc()
    d.in_ = xbuf.data_ptr()
    d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = B, cin, H, W, in_ctot, in_coff
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = cout, 1, 1, stride, 0, 0, 1
    d.oh, d.ow = (H - 1) // stride + 1, (W - 1) // stride + 1
    return d


def _lines(t, B, per_image, img_stride, scale_log2=0):
    """The `batch` maxima lines of a channel slice (ct_absmax_f32), optionally made 2^scale_log2 too large."""
    lines = torch.zeros(B * LINE, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().ct_absmax_f32(t.data_ptr(), B, per_image, img_stride, lines.data_ptr(), _s()), 'absmax')
    if scale_log2:
        lines = (lines.view(torch.float32) * 2.0 ** scale_log2).view(torch.int32).contiguous()
    return lines


def _run(x, dz, stride=1, maxima='given', xs=(0, 0), zs=(0, 0), ws_fill=None, check_guards=False):
    """dw of the 1x1 convolution with input x [B, cin, H, W] and output gradient dz; xs / zs = (channels in front, behind) of the
    wider NCHW buffers the operands are slices of."""
    lib = _lib.lib()
    B, cin, H, W = x.shape
    cout = dz.shape[1]
    xb = torch.randn(B, xs[0] + cin + xs[1], H, W, device=DEV) * 50
    xb[:, xs[0]:xs[0] + cin] = x
    zb = torch.randn(B, zs[0] + cout + zs[1], dz.shape[2], dz.shape[3], device=DEV) * 50
    zb[:, zs[0]:zs[0] + cout] = dz
    d = _desc(xb, B, cin, H, W, xb.shape[1], xs[0], cout, stride)
    assert (d.oh, d.ow) == tuple(dz.shape[2:])
    assert lib.ct_conv_wgrad_h2_supported(C.byref(d)) == 1
    need = lib.ct_conv_wgrad_h2_workspace_bytes(C.byref(d))
    wsb = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    if ws_fill is not None:
        wsb[GUARD:GUARD + need] = ws_fill
    dwb = torch.full((cout * cin + GUARD,), -777.0, device=DEV)
    zl = None
    if maxima != 'null':
        up = 10 if maxima == 'loose' else 0
        hw, ohw = H * W, d.oh * d.ow
        xl = _lines(xb.view(-1)[xs[0] * hw:], B, cin * hw, xb.shape[1] * hw, up)
        zl = _lines(zb.view(-1)[zs[0] * ohw:], B, cout * ohw, zb.shape[1] * ohw, up)
        d.in_absmax = xl.data_ptr()
    _lib.check(lib.ct_conv2d_wgrad_h2(C.byref(d), zb.data_ptr(), zb.shape[1], zs[0], zl.data_ptr() if zl is not None else None,
                                      dwb.data_ptr(), wsb[GUARD:].data_ptr(), need, _s()), 'wgrad_h2')
    torch.cuda.synchronize()
    if check_guards:
        assert (dwb[cout * cin:] == -777.0).all(), 'wrote behind dw'
        assert (wsb[:GUARD] == 0xA5).all() and (wsb[GUARD + need:] == 0xA5).all(), 'wrote outside the workspace'
    return dwb[:cout * cin].view(cout, cin).clone()


def _ref64(x, dz, stride):
    w = torch.zeros(dz.shape[1], x.shape[1], 1, 1, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().cpu(), w, None, stride).backward(dz.double().cpu())
    return w.grad[:, :, 0, 0]


def _old(x, dz, stride):
    B, cin, H, W = x.shape
    d = _desc(x, B, cin, H, W, cin, 0, dz.shape[1], stride)
    dw = torch.empty(dz.shape[1], cin, device=DEV)
    _lib.check(_lib.lib().ct_conv2d_wgrad(C.byref(d), dz.data_ptr(), dz.shape[1], 0, dw.data_ptr(), _s()), 'wgrad')
    torch.cuda.synchronize()
    return dw


def _data(B, cin, H, W, cout, stride, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + B + cin + 7 * H + cout)
    x = torch.randn(B, cin, H, W, generator=g).to(DEV)
    dz = torch.randn(B, cout, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=g).to(DEV)
    return x, dz


# B, cin, H, W, cout, stride, x slice (front, behind), dz slice
CASES = [
    (2, 64, 19, 19, 96, 1, (0, 0), (0, 0)),         # the two 1x1 rows of tests/test_gpu_train.py GEOMS
    (2, 64, 19, 19, 96, 2, (0, 0), (0, 0)),
    (2, 20, 19, 19, 33, 1, (0, 0), (0, 0)),         # cout / cin no multiple of 32 / 16
    (5, 20, 1, 1, 33, 1, (0, 0), (0, 0)),
    (5, 40, 3, 3, 24, 1, (0, 0), (0, 0)),
    (1, 48, 5, 5, 130, 1, (0, 0), (0, 0)),
    (5, 136, 10, 10, 64, 1, (0, 0), (0, 0)),
    (1, 33, 38, 38, 20, 1, (0, 0), (0, 0)),
    (5, 32, 19, 19, 40, 2, (3, 5), (2, 1)),         # stride 2 on an odd map, inner channel slices
    (1, 20, 5, 5, 33, 2, (0, 0), (0, 0)),
    (5, 64, 19, 17, 96, 1, (7, 2), (1, 6)),         # inner channel slices, batch 5
    (2, 24, 38, 38, 160, 2, (1, 0), (0, 3)),
]


@pytest.mark.parametrize('maxima', ['given', 'null', 'loose'])
@pytest.mark.parametrize('case', CASES, ids=[str(i) for i in range(len(CASES))])
def test_against_fp64_autograd(case, maxima):
    B, cin, H, W, cout, stride, xs, zs = case
    x, dz = _data(B, cin, H, W, cout, stride)
    dw = _run(x, dz, stride, maxima, xs, zs, check_guards=True)
    assert torch.isfinite(dw).all() and not (dw == -777.0).any()
    e = rel_err(dw.cpu(), _ref64(x, dz, stride).float())
    print('case', case, maxima, 'rel_err %.3e' % e)
    assert e < 1e-4


FULL = [(32, 1024, 19, 19, 1024, 1), (32, 512, 38, 38, 128, 1), (32, 1024, 19, 19, 256, 2)]


@pytest.mark.parametrize('shape', FULL, ids=['1024-1024@19', '512-128@38', '1024-256@19s2'])
def test_full_size_error_within_twice_the_fp32_kernel(shape):
    """err_new <= 2 err_old against float64 (the reference is the parent's kernel; 2 x own error is the criterion of
    tests/test_gpu_bf16.py).  Measured pairs: profiles/wgrad_h2_probe.txt."""
    B, cin, H, W, cout, stride = shape
    x, dz = _data(B, cin, H, W, cout, stride, seed=3)
    ohw = dz.shape[2] * dz.shape[3]
    xs_ = x[:, :, ::stride, ::stride].reshape(B, cin, ohw).double()
    ref = torch.einsum('bop,bip->oi', dz.reshape(B, cout, ohw).double(), xs_).cpu()
    new = _run(x, dz, stride, 'given').double().cpu()
    old = _old(x, dz, stride).double().cpu()

    def err(a):
        return float((a - ref).norm() / ref.norm())
    err_new, err_old = err(new), err(old)
    print('shape', shape, 'err_new %.3e err_old %.3e' % (err_new, err_old))
    assert rel_err(new.float(), ref.float()) < 1e-4
    assert err_new <= 2 * err_old, (err_new, err_old)


def test_bit_reproducible():
    x, dz = _data(5, 136, 19, 19, 200, 1, seed=1)
    a = _run(x, dz, 1, 'null', ws_fill=0)
    b = _run(x, dz, 1, 'null', ws_fill=0)
    c = _run(x, dz, 1, 'null', ws_fill=0xFF)           # all-ones bytes: every float of the workspace is a NaN
    assert torch.equal(a, b) and torch.equal(a, c)
    g = _run(x, dz, 1, 'given', ws_fill=0xFF)
    assert torch.equal(a, g)                            # the entry point's own maxima are the ones ct_absmax_f32 gives


@pytest.mark.parametrize('a,b', [(7, -9), (-30, 40)])
def test_scale_covariance(a, b):
    x, dz = _data(2, 64, 19, 19, 96, 1, seed=2)
    base = _run(x, dz, 1, 'null')
    got = _run(x * 2.0 ** a, dz * 2.0 ** b, 1, 'null')
    assert torch.equal(got, base * 2.0 ** (a + b))


def test_uneven_images():
    """One exponent per launch: an image whose dZ is 2^12 times the others' must not cost the others their precision."""
    x, dz = _data(5, 64, 19, 19, 96, 1, seed=4)
    dz[3] *= 4096.0
    for maxima in ('given', 'null'):
        dw = _run(x, dz, 1, maxima)
        assert rel_err(dw.cpu(), _ref64(x, dz, 1).float()) < 1e-4
    # and the small images alone are still resolved: their own sum against float64, with the big image's maximum as bound
    keep = [0, 1, 2, 4]
    lib = _lib.lib()
    xk, zk = x[keep].contiguous(), dz[keep].contiguous()
    d = _desc(xk, 4, 64, 19, 19, 64, 0, 96, 1)
    zl = _lines(dz[3:4].contiguous(), 1, 96 * 361, 96 * 361).view(1, LINE).repeat(4, 1).contiguous()
    need = lib.ct_conv_wgrad_h2_workspace_bytes(C.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    dw = torch.empty(96, 64, device=DEV)
    _lib.check(lib.ct_conv2d_wgrad_h2(C.byref(d), zk.data_ptr(), 96, 0, zl.data_ptr(), dw.data_ptr(), ws.data_ptr(), need, _s()),
               'wgrad_h2')
    assert rel_err(dw.cpu(), _ref64(xk, zk, 1).float()) < 1e-4


# ------------------------------------------------------------------ the training step
def _net(size, C_):
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), size, C_)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()), strict=True)
    net = net.cuda()
    net.device = 'cuda'
    return net


def _freeze_bn(net):
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    return net


def test_step_gradients_match_fp64_autograd_with_the_switch(monkeypatch):
    """tests/test_gpu_dp_train.py::test_frozen_bn_network_gradients_match_fp64_autograd with CTDET_WGRAD_H2=1: every parameter
    gradient of RFBNet-300 (bs 8, BatchNorm in eval mode) against float64 autograd over the replayed plan with the device's
    activation pattern, at that test's 1e-4; and the gradients of the layers that moved are bit-equal across two backward
    passes (no atomics)."""
    from emu_backend import replay_plan_autograd
    monkeypatch.setenv('CTDET_WGRAD_H2', '1')
    B = 8
    net = _freeze_bn(_net(300, 20).train())
    x = synth.images(B, 300, 'randn', 2024)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}

    def step():
        net.zero_grad(set_to_none=True)
        out = net(x.cuda())
        R = [torch.randn(t.shape, generator=torch.Generator().manual_seed(5 + i)) / t.numel() ** 0.5 for i, t in enumerate(out)]
        sum((t * r.cuda()).sum() for t, r in zip(out, R)).backward()
        torch.cuda.synchronize()
        return out, R
    out, R = step()
    trt = net.train_runtime(B)
    assert trt.wgrad_h2
    moved = [n for n, s_ in trt.state.items() if s_.wgrad_route.name == 'h2']
    assert len(moved) >= 5, moved           # stride 1 from 19x19 up (the selection rule of train_engine.py)
    steps = {st.name: st for st in trt.plan.steps if st.kind == 'conv'}
    assert all((steps[n].kh, steps[n].kw) == (1, 1) for n in moved)
    moved_w = [p.weight for n in moved for p in steps[n].parts]
    first = [p.grad.clone() for p in moved_w]
    names = {id(p): n for n, p in net.named_parameters()}
    leaf = {i: sd[n].double().requires_grad_(True) for i, n in names.items()}

    def masks(st, off, cout):
        return (trt.bufs[st.dst][:, st.dst_coff + off:st.dst_coff + off + cout] > 0).cpu()
    got64 = replay_plan_autograd(trt.plan, leaf, x, masks, pool_inputs=lambda st: trt.bufs[st.src].cpu())
    for a, b, n in zip(out, got64, ('loc', 'conf', 'obj')):
        assert rel_err(a.detach().cpu().reshape(B, -1), b.detach().float()) < 1e-4, n
    sum((t * r.double().reshape(B, -1)).sum() for t, r in zip(got64, R)).backward()
    worst = {}
    for name, prm in net.named_parameters():
        assert prm.grad is not None, name
        e = rel_err(prm.grad.cpu().double(), leaf[id(prm)].grad)
        if e >= 1e-4:
            worst[name] = e
    assert not worst, ' '.join('%s:%.1e' % kv for kv in worst.items())
    step()
    for p, f in zip(moved_w, first):
        assert torch.equal(p.grad, f)
