"""The deterministic training mode (CTDET_TRAIN_DETERMINISTIC=1, include/ctdet.h `_det` entries) on the MI355X: every site that
otherwise sums through floating-point atomics stores one slab per split and adds the slabs in order.

  1. same numbers: every row of the existing tables through the `_det` entry, against the SAME float64 reference and the SAME bound
     the row's existing test asserts (imported: WGRAD_TOL of test_gpu_conv_grad.py, the tolerances of test_gpu_wino_wgrad.py, _bound
     and the floors of test_gpu_train_kernels.py);
  2. repeat equality: three launches from the same inputs give the same bits, and a fourth issued while a second stream is busy
     with a large elementwise kernel gives them again -- only at shapes where at least three partial sums meet per output (asserted
     from the size query before the launch: two terms commute);
  3. the workspace is not state: NaN-filled and zero-filled workspaces give the same finite bits, bytes past the queried size are
     not touched;
  4. the whole step of RFBNet-300 (bs 2) twice from the same state under the switch: every parameter gradient and every BatchNorm
     running statistic bit for bit; against the runtime without the switch inside the per-name rule test_gpu_train.py holds the
     parameter gradients to (heads 1e-3, the rest direction and norm); the policy record; no `_det` entry called with the switch unset;
  5. the phase-2 network with the Context-Transformer block is refused under the switch.

The repeat tests compare outputs only: nothing is run over and over to look for a difference, and nothing is asserted about the
default (atomic) path."""
import ctypes as C
import dataclasses
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
import conv_grad_cases as G
import train_cases as TC
import test_gpu_conv_grad as TG
import test_gpu_train_kernels as TK
import test_gpu_wino_wgrad as TW
from ctdet import _lib, engine, synth, train_engine

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
TAIL = 256              # sentinel bytes behind every workspace
WINO = {'f2': ('ct_conv_wgrad_wino_det_workspace_bytes', 'ct_conv2d_wgrad_wino_det'),
        'f4': ('ct_conv_wgrad_wino4_det_workspace_bytes', 'ct_conv2d_wgrad_wino4_det')}


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


class Workspace:
    """`need` bytes filled with `fill` (a byte value; 0xFF = NaN bit patterns in floats and doubles) and a sentinel tail."""

    def __init__(self, need, fill=0xFF):
        self.need = int(need)
        self.t = torch.empty(self.need + TAIL, dtype=torch.uint8, device=DEV)
        self.t[:self.need].fill_(fill)
        self.t[self.need:].fill_(0xA5)

    def args(self):
        return self.t.data_ptr(), self.need

    def tail_untouched(self):
        return bool((self.t[self.need:] == 0xA5).all())


def _busy(side):
    """Keeps `side` busy with large elementwise kernels while the caller launches on the current stream."""
    big = torch.empty(1 << 28, device=DEV)          # 1 GiB: a pass takes about half a millisecond of the whole chip's bandwidth,
    with torch.cuda.stream(side):                   # 60 of them outlast the upload of the inputs and the launch under test
        big.fill_(1.0)
        for _ in range(60):
            big.mul_(1.0001)
    return big


def _repeat(launch):
    """launch() -> dict of output tensors.  Three launches, then one beside a busy second stream: all the same bits."""
    torch.cuda.synchronize()
    first = launch()
    for _ in range(2):
        TK._same(first, launch())
    side = torch.cuda.Stream()
    keep = _busy(side)
    other = launch()
    torch.cuda.synchronize()
    del keep
    TK._same(first, other)
    return first


# ------------------------------------------------------------------------------------------------ direct weight gradient
def _partials(query, *args):
    n = C.c_int(-1)
    size = getattr(_lib.lib(), query)(*args, C.byref(n))
    return int(size), n.value


def _direct_query(case):
    d = G.wgrad_desc(case, torch.empty(1, case.x_ctot, 1, 1))       # geometry only: the query does not look at the pointer
    return _partials('ct_conv_wgrad_det_workspace_bytes', C.byref(d))


def _direct(case, fill=0xFF, inputs=None):
    """One ct_conv2d_wgrad_det launch into a NaN-filled dw -> (dw on the device, the workspace)."""
    inp = inputs if inputs is not None else TG._problem(case)[0]
    xd, dzd = inp.x_buf.to(DEV), inp.dz_buf.to(DEV)
    d = G.wgrad_desc(case, xd)
    ws = Workspace(_direct_query(case)[0], fill)
    dw = torch.full((case.cout, case.cin, case.kh, case.kw), NAN, device=DEV)
    _lib.check(_lib.lib().ct_conv2d_wgrad_det(C.byref(d), dzd.data_ptr(), case.dz_ctot, case.dz_coff, dw.data_ptr(), *ws.args(), _s()),
               'wgrad det ' + case.name)
    torch.cuda.synchronize()
    return dw, ws


@pytest.mark.parametrize('case', G.WGRAD_CASES, ids=TG._ids(G.WGRAD_CASES))
def test_direct_det_meets_the_bound_of_the_plain_entry(case, monkeypatch):
    monkeypatch.delenv('CTDET_WGRAD_GENERIC', raising=False)
    _, (ref, _dx), _ = TG._problem(case)
    size, partials = _direct_query(case)
    assert size > 0 and partials >= 1
    dw, ws = _direct(case)
    err = rel_err(dw.cpu().double(), ref)
    print('WGRAD-DET %s path=%s partials %d err %.3g' % (case.name, TG._path(case), partials, err))
    assert torch.isfinite(dw).all() and ws.tail_untouched(), case.name
    assert err < TG.WGRAD_TOL, (case.name, err)


def _row(name):
    return next(c for c in G.WGRAD_CASES if c.name == name)


def _three_partials(case, query):
    """The row with B raised until at least three partial sums meet per output (a host query; the kernel's rule decides)."""
    for B in range(case.B, 65):
        c = dataclasses.replace(case, B=B, name='%s_B%d' % (case.name, B)) if B != case.B else case
        if query(c)[1] >= 3:
            return c
    raise AssertionError('no batch up to 64 gives three partial sums for ' + case.name)


# 1x1 stride 1 (the issue's shape: 12 pixel splits) and stride 2; 3x3 stride 2; 1x3 and 3x1; dilation 6; the generic (cin % 64 != 0)
# instantiation; channel slices; ragged cout 40 and cin 72
REPEAT_DIRECT = [G.Case('k1x1_38', 'w', 2, 64, 38, 38, (64,), kh=1, kw=1, ph=0, pw=0), _row('k1x1_s1_tm'), _row('k1x1_s2_tm'),
                 _row('s2_odd_tm'), _row('k1x3_tm'), _row('k3x1_tm'), _row('d6_19_tm'), _row('s2_odd_g'), _row('slices_tm'),
                 _row('slices_g'), _row('pad1_19_tm'), _row('b3_19x17_g')]


@pytest.mark.parametrize('case', REPEAT_DIRECT, ids=TG._ids(REPEAT_DIRECT))
def test_direct_det_repeats_bit_for_bit(case, monkeypatch):
    monkeypatch.delenv('CTDET_WGRAD_GENERIC', raising=False)
    case = _three_partials(case, _direct_query)
    size, partials = _direct_query(case)
    if case.name == 'k1x1_38':
        assert partials == 12           # the rule of include/ctdet.h worked by hand: 46 blocks of 64 pixels, 4 per split
    assert partials >= 3, (case.name, partials)
    inp = G.make_inputs(case)
    got = _repeat(lambda: {'dw': _direct(case, inputs=inp)[0]})
    ref = G.ref64(inp.x(case), inp.parts, inp.dz(case), case)[0]
    assert rel_err(got['dw'].cpu().double(), ref) < TG.WGRAD_TOL


def test_direct_det_workspace_is_not_state():
    case = _three_partials(_row('b3_19x17_g'), _direct_query)
    (a, wa), (b, wb) = _direct(case, 0xFF), _direct(case, 0x00)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert wa.tail_untouched() and wb.tail_untouched()


# ------------------------------------------------------------------------------------------------ Winograd twins
@functools.lru_cache(maxsize=None)
def _wino_problem(g):
    """(x buffer, dZ buffer, float64 dw) of a row of test_gpu_wino_wgrad.GEOMS, built as that test builds it."""
    B, Cin, H, W, Cout, xs, zs = g
    gen = torch.Generator().manual_seed(11 + Cin + H)
    xctot, xcoff = xs or (Cin, 0)
    zctot, zcoff = zs or (Cout, 0)
    xfull = torch.randn(B, xctot, H, W, generator=gen)
    dzfull = torch.randn(B, zctot, H, W, generator=gen)
    x = xfull[:, xcoff:xcoff + Cin].double().requires_grad_(True)
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, 1, 1).backward(dzfull[:, zcoff:zcoff + Cout].double())
    return xfull, dzfull, w.grad


def _wino_query(g, variant):
    B, Cin, H, W, Cout, xs, zs = g
    xctot, xcoff = xs or (Cin, 0)
    d = TW._desc(torch.empty(0), B, Cin, H, W, xctot, xcoff, Cout)
    return _partials(WINO[variant][0], C.byref(d))


def _wino(g, variant, fill=0xFF):
    B, Cin, H, W, Cout, xs, zs = g
    xctot, xcoff = xs or (Cin, 0)
    zctot, zcoff = zs or (Cout, 0)
    xfull, dzfull, _ = _wino_problem(g)
    xd, dzd = xfull.to(DEV), dzfull.to(DEV)
    d = TW._desc(xd, B, Cin, H, W, xctot, xcoff, Cout)
    ws = Workspace(_wino_query(g, variant)[0], fill)
    dw = torch.full((Cout, Cin, 3, 3), NAN, device=DEV)
    _lib.check(getattr(_lib.lib(), WINO[variant][1])(C.byref(d), dzd.data_ptr(), zctot, zcoff, dw.data_ptr(), *ws.args(), _s()),
               'wgrad wino det')
    torch.cuda.synchronize()
    return dw, ws


@pytest.mark.parametrize('variant', ['f2', 'f4'])
@pytest.mark.parametrize('g', TW.GEOMS, ids=[str(i) for i in range(len(TW.GEOMS))])
def test_wino_det_meets_the_bound_of_the_plain_entry(g, variant):
    tol = TW.VARIANTS[variant][3]
    size, partials = _wino_query(g, variant)
    assert size > 0 and partials >= 1
    dw, ws = _wino(g, variant)
    err = rel_err(dw.cpu().double(), _wino_problem(g)[2])
    print('WINO-DET %s %s partials %d err %.3g' % (variant, g[:5], partials, err))
    assert torch.isfinite(dw).all() and ws.tail_untouched()
    assert err < tol, (g, err)


REPEAT_WINO = [TW.GEOMS[0], TW.GEOMS[2], TW.GEOMS[8]]      # 64 -> 64 @19x19, 72 -> 130 @19x17, the sliced 32 -> 64 @38x38


@pytest.mark.parametrize('variant', ['f2', 'f4'])
@pytest.mark.parametrize('g', REPEAT_WINO, ids=['64x64_19', '72x130_19x17', 'sliced_38'])
def test_wino_det_repeats_bit_for_bit(g, variant):
    for B in range(g[0], 65):           # raise B until three slabs meet (holds at the table's B today)
        gb = (B,) + g[1:]
        if _wino_query(gb, variant)[1] >= 3:
            break
    assert _wino_query(gb, variant)[1] >= 3, gb
    got = _repeat(lambda: {'dw': _wino(gb, variant)[0]})
    assert rel_err(got['dw'].cpu().double(), _wino_problem(gb)[2]) < TW.VARIANTS[variant][3]


@pytest.mark.parametrize('variant', ['f2', 'f4'])
def test_wino_det_workspace_is_not_state(variant):
    g = TW.GEOMS[2]
    assert _wino_query(g, variant)[1] >= 3
    (a, wa), (b, wb) = _wino(g, variant, 0xFF), _wino(g, variant, 0x00)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert wa.tail_untouched() and wb.tail_untouched()


# ------------------------------------------------------------------------------------------------ above 2 GiB: batch chunks
@pytest.mark.parametrize('route', ['direct', 'f2', 'f4'])
def test_det_above_2gib_appends_the_slabs_of_its_batch_chunks(route):
    """The shapes of test_direct_wgrad_above_2gib / test_wino_wgrad_above_2gib (an input buffer of 2.2 GB: two launches, two
    images and one): the second launch's slabs follow the first's and the finish adds them all; same bounds."""
    dil = 2 if route == 'direct' else 1
    B, ctot, coff, Cin, Cout, S = 3, 704, 100, 8, 16 if route == 'direct' else 8, 512
    gen = torch.Generator(device=DEV).manual_seed(9)
    xfull = torch.randn(B, ctot, S, S, device=DEV, generator=gen)
    dz = torch.randn(B, Cout, S, S, device=DEV, generator=gen)
    x = xfull[:, coff:coff + Cin].cpu().double().requires_grad_(True)
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, 1, dil, dil).backward(dz.cpu().double())
    d = TW._desc(xfull, B, Cin, S, S, ctot, coff, Cout, pad=dil, dil=dil)
    query, run = ('ct_conv_wgrad_det_workspace_bytes', 'ct_conv2d_wgrad_det') if route == 'direct' else WINO[route]
    size, partials = _partials(query, C.byref(d))
    one = C.c_int(0)                    # the same layer with one image less fits one launch: fewer slabs than the two launches
    d1 = TW._desc(xfull, B - 1, Cin, S, S, ctot, coff, Cout, pad=dil, dil=dil)
    getattr(_lib.lib(), query)(C.byref(d1), C.byref(one))
    assert partials > one.value >= 3
    ws = Workspace(size)
    dw = torch.full((Cout, Cin, 3, 3), NAN, device=DEV)
    _lib.check(getattr(_lib.lib(), run)(C.byref(d), dz.data_ptr(), Cout, 0, dw.data_ptr(), *ws.args(), _s()), run + ' > 2 GiB')
    torch.cuda.synchronize()
    assert ws.tail_untouched()
    assert rel_err(dw.cpu().double(), w.grad) < (TG.WGRAD_TOL if route == 'direct' else TW.VARIANTS[route][3])


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn_det(k, fill=0xFF):
    """The statistics and the backward launch of a case through the `_det` entries (the apply launch has no reduction); every
    buffer they write, by name, as test_gpu_train_kernels._bn_launch returns them."""
    lib, st = _lib.lib(), _s()
    B, Cc, HW = k.B, k.C, k.HW
    o = {}
    z, gamma, lo = _d(k.z), _d(k.gamma), _d(k.lo_t)
    meanin, varin, dy, yin = _d(k.mean), _d(k.var), _d(k.dy), _d(k.y_in)
    need = _partials('ct_bn_det_scratch_bytes', B, Cc, HW)[0]
    o['mean'], o['var'] = torch.full((Cc,), 3.0, device=DEV), torch.full((Cc,), 3.0, device=DEV)
    o['rmean'], o['rvar'] = (_d(k.rm0.clone()), _d(k.rv0.clone())) if k.running else (None, None)
    ws1 = Workspace(need, fill)
    _lib.check(lib.ct_bn_train_stats_det(z.data_ptr(), B, Cc + TC.ZP, TC.ZO, Cc, HW, o['mean'].data_ptr(), o['var'].data_ptr(),
                                         TC.MOMENTUM, _p(o['rmean']), _p(o['rvar']), *ws1.args(), st), 'stats det')
    o['dz'], o['dres'] = _d(k.dz0.clone()), _d(None if k.dres0 is None else k.dres0.clone())
    o['dgamma'], o['dbeta'] = torch.full((Cc,), 3.0, device=DEV), torch.full((Cc,), 3.0, device=DEV)
    ws2 = Workspace(need, fill)
    fn = lib.ct_bn_eval_backward_det if k.frozen else lib.ct_bn_train_backward_det
    _lib.check(fn(dy.data_ptr(), Cc + TC.GP, TC.GO, _p(yin), Cc + TC.YP, TC.YO, z.data_ptr(), meanin.data_ptr(), varin.data_ptr(),
                  gamma.data_ptr(), TC.EPS, k.relu, _p(lo), k.rscale, _p(o['dres']), k.dres_ctot, k.dres_off, k.acc,
                  o['dz'].data_ptr(), o['dgamma'].data_ptr(), o['dbeta'].data_ptr(), Cc + TC.ZP, TC.ZO, B, Cc, HW, *ws2.args(), st),
               'bn backward det')
    torch.cuda.synchronize()
    assert ws1.tail_untouched() and ws2.tail_untouched()
    return o


@pytest.mark.parametrize('combo', list(TC.BN_COMBOS))
@pytest.mark.parametrize('shape', TC.BN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_batchnorm_det_meets_the_bounds_of_the_plain_entries(shape, combo):
    k = TC.bn_case(shape, combo)
    want = TC.bn_expected(k)
    o = _bn_det(k)
    sl = dict(dz=(TC.ZO, 7.0), dres=(k.dres_off, k.dres0))
    for name, (r64, r32) in want.items():
        if name == 'y':
            continue                    # ct_bn_train_apply: no reduction, no twin
        got = o[name]
        if name in sl:
            off, sentinel = sl[name]
            assert TK._outside(got, off, k.C, sentinel), name + ': channels outside the slice were written'
            got = got[:, off:off + k.C]
        assert bool(torch.isfinite(got).all()), name
        TK._bound('bn/%s/%s' % (k.name, name), got, r64, r32, TC.BN_FLOORS[name])


@pytest.mark.parametrize('combo', ['plain', 'l0', 'racc'])
@pytest.mark.parametrize('shape', [(32, 8, 361), (8, 64, 5625)], ids=lambda s: 'x'.join(map(str, s)))
def test_batchnorm_det_repeats_bit_for_bit(shape, combo):
    partials = _partials('ct_bn_det_scratch_bytes', *shape)[1]
    assert partials == {(32, 8, 361): 5, (8, 64, 5625): 16}[shape] and partials >= 3
    k = TC.bn_case(shape, combo)
    _repeat(lambda: _bn_det(k))
    TK._same(_bn_det(k, 0xFF), _bn_det(k, 0x00))           # the scratch is not state


# ------------------------------------------------------------------------------------------------ bias sums
def _bias_det(k, fill=0xFF):
    lib = _lib.lib()
    dy, y, dz = _d(k.dy), _d(k.y), _d(k.dz0.clone())
    db = torch.full((k.C,), NAN, device=DEV) if k.has_db else None
    lines = TK._amax_lines(k.B)
    ws = Workspace(_partials('ct_bias_det_scratch_bytes', k.B, k.C, k.HW)[0], fill)
    _lib.check(lib.ct_bias_act_backward_det(dy.data_ptr(), k.C + 2, 1, _p(y), k.C + 3, 2, k.relu, k.B, k.C, k.HW, dz.data_ptr(), k.C + 4,
                                            3, _p(db), lines.data_ptr(), *ws.args(), _s()), 'bias bwd det')
    torch.cuda.synchronize()
    assert ws.tail_untouched()
    return {'dz': dz, 'dbias': db, 'amax': lines}


@pytest.mark.parametrize('c', TC.BIAS_CASES, ids=TC.bias_id)
def test_bias_det_meets_the_bound_of_the_plain_entry(c):
    k = TC.bias_case(c)
    (_, db64, _), (dz32, db32, am32) = TC.bias_expected(k)
    o = _bias_det(k)
    assert torch.equal(o['dz'].cpu(), dz32)
    assert torch.equal(TK._amax_values(o['amax'], k.B), am32)
    if k.has_db:
        assert bool(torch.isfinite(o['dbias']).all())
        TK._bound('bias/%s/dbias' % k.name, o['dbias'], db64, db32, 1e-5)


@pytest.mark.parametrize('c', [(8, 3, 5625, 1, 1, 1), (2, 1, 4100, 1, 1, 1)], ids=TC.bias_id)
def test_bias_det_repeats_bit_for_bit(c):
    assert c in TC.BIAS_CASES
    assert _partials('ct_bias_det_scratch_bytes', *c[:3])[1] >= 3
    k = TC.bias_case(c)
    _repeat(lambda: _bias_det(k))
    TK._same(_bias_det(k, 0xFF), _bias_det(k, 0x00))


def _fused_det(k, fill=0xFF):
    lib = _lib.lib()
    y, dy, dz = _d(k.y), _d(k.dy), _d(k.dz0.clone())
    db, lines = torch.full((k.C,), NAN, device=DEV), TK._amax_lines(k.B)
    ws = Workspace(_partials('ct_maxpool2x2_bias_relu_bwd_det_scratch_bytes', k.B, k.C)[0], fill)
    _lib.check(lib.ct_maxpool2x2_bias_relu_bwd_det(y.data_ptr(), k.C + 3, 2, dy.data_ptr(), k.B, k.C, k.H, k.W, k.OH, k.OW,
                                                   dz.data_ptr(), k.C + 2, 1, db.data_ptr(), lines.data_ptr(), *ws.args(), _s()),
               'fused pool bwd det')
    torch.cuda.synchronize()
    assert ws.tail_untouched()
    return {'dz': dz, 'dbias': db, 'amax': lines}


@pytest.mark.parametrize('c', TC.FUSED_CASES, ids=TC.fused_id)
def test_fused_pool_det_meets_the_bound_of_the_plain_entry(c):
    k = TC.fused_case(c)
    (_, db64, _), (dz32, db32, am32) = TC.fused_expected(k)
    o = _fused_det(k)
    assert torch.equal(o['dz'].cpu(), dz32)
    assert torch.equal(TK._amax_values(o['amax'], k.B), am32)
    assert bool(torch.isfinite(o['dbias']).all())
    TK._bound('fused/%s/dbias' % k.name, o['dbias'], db64, db32, 1e-5)


@pytest.mark.parametrize('c', [(3, 5, 64, 64, False), (3, 5, 17, 241, True)], ids=TC.fused_id)
def test_fused_pool_det_repeats_bit_for_bit(c):
    assert c in TC.FUSED_CASES
    assert _partials('ct_maxpool2x2_bias_relu_bwd_det_scratch_bytes', c[0], c[1])[1] >= 3        # one partial sum per image
    k = TC.fused_case(c)
    _repeat(lambda: _fused_det(k))
    TK._same(_fused_det(k, 0xFF), _fused_det(k, 0x00))


# ------------------------------------------------------------------------------------------------ the whole step
class _Calls:
    """The library of a backend, with the name of every entry fetched from it.  Installed on the backend BEFORE the runtime is
    built, so it is the one library object the runtime, its pack lists and the backend's own launches all go through: the set
    holds every entry any of them calls (and the few that are bound ahead of their first call)."""

    def __init__(self, lib):
        self._lib, self.names = lib, set()

    def __getattr__(self, name):
        self.names.add(name)
        return getattr(self._lib, name)


def _net(phase=1):
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=phase, setting='transfer'), 300, 20)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()), strict=True)
    net = net.cuda().train()
    net.device = 'cuda'
    return net


def _step(net, state, x, deterministic, monkeypatch):
    """A fresh TrainRuntime on `net` restored to `state`: forward + backward with fixed (seeded) upstream gradients ->
    (gradients by parameter name, BatchNorm running statistics by name, policy record, entries called)."""
    if deterministic:
        monkeypatch.setenv('CTDET_TRAIN_DETERMINISTIC', '1')
    else:
        monkeypatch.delenv('CTDET_TRAIN_DETERMINISTIC', raising=False)
    net.load_state_dict(state)
    be = engine.HipBackend(torch.device(DEV))
    calls = be.lib = _Calls(be.lib)
    rt = train_engine.TrainRuntime(net, 2, be)
    assert rt.lib is calls
    g = torch.Generator().manual_seed(7)
    ups = tuple((torch.randn(rt.bufs[k].shape, generator=g) * 1e-3).to(DEV) for k in ('loc', 'conf', 'obj'))
    rt.forward(x, use_ctx=False)
    grads = rt.backward(*ups)
    torch.cuda.synchronize()
    names = {id(p): n for n, p in net.named_parameters()}
    out = {names[id(p)]: g.clone() for p, g in zip(rt.params, grads)}
    running = {n: b.clone() for n, b in net.named_buffers() if 'running' in n}
    return out, running, rt.policy_record(), calls.names


def test_whole_step_repeats_bit_for_bit_under_the_switch(monkeypatch):
    net = _net()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    x = synth.images(2, 300, 'randn', 1234).cuda()
    a, ra, pa, ca = _step(net, state, x, True, monkeypatch)
    b, rb, pb, cb = _step(net, state, x, True, monkeypatch)
    assert pa['deterministic'] is True and pb['deterministic'] is True
    assert {n for n in ca if n.endswith('_det')} >= {'ct_conv2d_wgrad_det', 'ct_conv2d_wgrad_wino4_det', 'ct_bn_train_stats_det',
                                                     'ct_bn_train_backward_det', 'ct_bias_act_backward_det',
                                                     'ct_maxpool2x2_bias_relu_bwd_det'}
    assert set(a) == set(b) == {n for n, _ in net.named_parameters()}
    for n in a:
        assert torch.isfinite(a[n]).all(), n
        assert torch.equal(a[n], b[n]), n
    assert ra and set(ra) == set(rb)
    for n in ra:
        assert torch.equal(ra[n], rb[n]), n
        assert not torch.equal(ra[n], state[n]), n + ' was not updated'
    # against the runtime without the switch: the per-name rule test_gpu_train.py::test_train_forward_and_backward_vs_oracle_autograd
    # holds every parameter gradient to, with the switch-off gradients in the place of the oracle's
    off, _, poff, coff = _step(net, state, x, False, monkeypatch)
    assert poff['deterministic'] is False
    assert not [n for n in coff if '_det' in n], sorted(n for n in coff if '_det' in n)
    worst = max((float((a[n] - off[n]).abs().max()) / max(float(off[n].abs().max()), 1e-30), n) for n in off)
    print('DET-STEP largest max|on - off| / max|off| over the parameters: %.3g (%s)' % worst)
    bad = _outside_train_test_tolerance(a, off)
    assert not bad, sorted(bad.items())[:12]


def _outside_train_test_tolerance(got, ref):
    """The acceptance rule of tests/test_gpu_train.py (its lines 233-248), name by name: a reference gradient of negligible norm
    wants a negligible one; the heads (loc / conf / obj except the `.5` entries) max|a - b| <= 1e-3 max|b|; every other parameter
    cos >= 0.995 and a norm within 5 %.  -> {name: what it missed}"""
    gmax = max(float(v.abs().max()) for v in ref.values())
    bad = {}
    for name in ref:
        a, b = got[name].cpu().double().flatten(), ref[name].cpu().double().flatten()
        na, nb = float(a.norm()), float(b.norm())
        if nb < 1e-5 * gmax * max(1.0, b.numel() ** 0.5):
            assert na < 1e-3 * gmax * max(1.0, b.numel() ** 0.5), name       # both ~0 (BN-cancelled terms)
            continue
        cos = float(a @ b) / (na * nb)
        if name.split('.')[0] in ('loc', 'conf', 'obj') and not name.startswith(('loc.5', 'conf.5', 'obj.5')):
            if float((a - b).abs().max()) > 1e-3 * float(b.abs().max()):
                bad[name] = ('head', float((a - b).abs().max()) / float(b.abs().max()))
        elif cos < 0.995 or abs(na / nb - 1) > 0.05:
            bad[name] = (cos, na / nb)
    return bad


def test_context_transformer_block_is_refused_under_the_switch(monkeypatch):
    monkeypatch.setenv('CTDET_TRAIN_DETERMINISTIC', '1')
    net = _net(phase=2)
    rt = train_engine.TrainRuntime(net, 2, engine.HipBackend(torch.device(DEV)))
    assert rt.ctx is not None and rt.policy_record()['deterministic'] is True
    x = synth.images(2, 300, 'randn', 5).cuda()
    with pytest.raises(_lib.CtdetError, match='ct_ctx_attention_bwd'):
        rt.forward(x, use_ctx=True)
    rt.forward(x, use_ctx=False)            # the convolutional part alone is covered
    torch.cuda.synchronize()
