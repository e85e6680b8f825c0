"""The two direct gradient kernels of training, path by path, against float64 autograd (tests/conv_grad_cases.py):

  * ct_conv2d_wgrad (csrc/ct_wgrad.hip, conv_wgrad_f32): every row once on the tap-major, software-pipelined kernel
    (cin % 64 == 0) and once on the generic one, dw NaN on entry, rel_err (max|a-b| / max|b|) below WGRAD_TOL = 1e-5 -- the bound
    test_gpu_train.py::test_direct_wgrad_above_2gib already holds this kernel to; the tap-major rows again with
    CTDET_WGRAD_GENERIC=1 (read per call), which must agree with the tap-major result to the same bound; the accumulate contract
    of ct_scratch_prezeroed(1); and the 128x128 variant behind CTDET_WGRAD_TB=2 (read once) in one fresh child process.
    No bit-equality between runs: the pixel splits meet in fp32 atomics.
  * ct_conv2d_fwd with desc.transposed = 1 (csrc/ct_conv.hip): every row x the heuristic (config 0) and every implicit-GEMM
    tile configuration, into a channel slice of a wider buffer pre-filled with a finite pattern G0: channels outside the slice
    keep G0's bits, the slice is checked per image (G0 + dX where res == out), two launches give the same bits; on the split-K
    subset also ksplit 0 / 2 / 3 / 1000 / -1 with a NaN-filled workspace of the engine's size.
  * the same rows through ct_conv2d_x3_fwd (bf16x3) where TrainEngine would take that route, every non-f16x2 configuration.

Bounds of the data gradient.  Hard: 1e-4, the library's contract.  Tight, fp32 kernel only: max(TIGHT_FACTOR * e32, 2^-20), e32
= the error of torch-CPU fp32 autograd against the same float64 reference on the same row; the factor 8 allows for another
accumulation order and the noise of a max statistic, 2^-20 is 16 fp32 roundoffs for the rows with a handful of terms.

Every launch prints its figures before it asserts (`pytest -s`): lines `WGRAD`, `WGRAD-TB2`, `DGRAD-DIRECT`, `DGRAD-X3`.
Measured on an MI355X (largest err over the table, row; DESIGN.md section 6 has the same table):
  WGRAD tap-major 3.46e-7 (d6_19_tm), err / e32 at most 1.39; generic 3.55e-7 (tb2_g), err / e32 at most 1.44; tap-major rows forced
  generic 3.46e-7, 2.0e-7 from the tap-major result; prezeroed G0 + dw 3.69e-7, caller-zeroed 3.55e-7; WGRAD-TB2 2.49e-7 / 3.55e-7.
  DGRAD-DIRECT 9.33e-7 (parts_40_24, e32 2.87e-7: err / e32 3.25, the largest ratio too; 0.41 of the tight bound) -- the same for
  all eight tiles (the k order does not depend on the tile), lower with split-K (down to 2.06e-7 on that row).  DGRAD-X3 2.35e-7.
  e32 itself: 0.45-17e-7 over the rows.  The factor 8 was not needed beyond 3.25 and stays as first set."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch

from conftest import rel_err          # first: it puts the package on sys.path (the child process below has no pytest)
import conv_grad_cases as G
from ctdet import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WGRAD_TOL = 1e-5
HARD = 1e-4
TIGHT_FACTOR = 8.0
TIGHT_FLOOR = 2.0 ** -20
KSPLITS = (0, 2, 3, 1000, -1)
KSPLIT_CONFIGS = (0, 5, 7)


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('the gpu tests need a HIP device; none visible')


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _problem(case):
    """(inputs, float64 (dw, dx), torch-CPU fp32 (dw, dx)) of a row: computed once, shared by the tests, never written."""
    inp = G.make_inputs(case)
    args = (inp.x(case), inp.parts, inp.dz(case), case)
    return inp, G.ref64(*args), G.grad32(*args)


def _ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad(case, fill):
    """One ct_conv2d_wgrad launch into dw pre-filled with `fill` (a float or a tensor) -> dw on the CPU."""
    inp = _problem(case)[0]
    xd, dzd = inp.x_buf.to(DEV), inp.dz_buf.to(DEV)
    dw = torch.empty(case.cout, case.cin, case.kh, case.kw, device=DEV)
    if isinstance(fill, torch.Tensor):
        dw.copy_(fill)
    else:
        dw.fill_(fill)
    d = G.wgrad_desc(case, xd)
    _lib.check(_lib.lib().ct_conv2d_wgrad(C.byref(d), dzd.data_ptr(), case.dz_ctot, case.dz_coff, dw.data_ptr(), _s()),
               'wgrad ' + case.name)
    torch.cuda.synchronize()
    return dw.cpu()


def _path(case, forced_generic=False):
    return 'tapmajor' if case.tapmajor and not forced_generic else 'generic'


@pytest.mark.parametrize('case', G.WGRAD_CASES, ids=_ids(G.WGRAD_CASES))
def test_wgrad_vs_float64(case, monkeypatch):
    _, (ref, _dx), (cpu32, _dx32) = _problem(case)
    e32 = rel_err(cpu32, ref)
    monkeypatch.delenv('CTDET_WGRAD_GENERIC', raising=False)
    got = _wgrad(case, float('nan'))
    err = rel_err(got.double(), ref)
    print('WGRAD %s path=%s err %.3g e32 %.3g terms %d' % (case.name, _path(case), err, e32, case.reduction))
    assert torch.isfinite(got).all(), case.name
    assert err < WGRAD_TOL, (case.name, _path(case), err)
    if case.tapmajor:
        monkeypatch.setenv('CTDET_WGRAD_GENERIC', '1')
        gen = _wgrad(case, float('nan'))
        monkeypatch.delenv('CTDET_WGRAD_GENERIC')
        e_gen, e_both = rel_err(gen.double(), ref), rel_err(gen.double(), got.double())
        print('WGRAD %s path=%s err %.3g e32 %.3g vs tapmajor %.3g' % (case.name, _path(case, True), e_gen, e32, e_both))
        assert torch.isfinite(gen).all(), case.name
        assert e_gen < WGRAD_TOL and e_both < WGRAD_TOL, (case.name, 'forced generic', e_gen, e_both)


@pytest.fixture
def prezeroed(request):
    """The switch of ct_scratch_prezeroed; the restore to 0 is registered BEFORE it can be turned (a leaked 1 would take the
    memsets away from every later test of the process)."""
    lib = _lib.lib()
    request.addfinalizer(lambda: lib.ct_scratch_prezeroed(0))
    return lambda on: _lib.check(lib.ct_scratch_prezeroed(int(on)), 'ct_scratch_prezeroed')


@pytest.mark.parametrize('case', G.WGRAD_CASES, ids=_ids(G.WGRAD_CASES))
def test_wgrad_prezeroed_accumulates(case, prezeroed, monkeypatch):
    """ct_scratch_prezeroed(1): the entry point leaves the memset to the caller, so dw comes back as what it held + the gradient."""
    inp, (ref, _dx), _ = _problem(case)
    monkeypatch.delenv('CTDET_WGRAD_GENERIC', raising=False)
    prezeroed(1)
    acc = _wgrad(case, inp.g0)
    zeroed = _wgrad(case, 0.0)
    prezeroed(0)
    e_acc, e_zero = rel_err(acc.double(), inp.g0.double() + ref), rel_err(zeroed.double(), ref)
    print('WGRAD %s path=%s prezeroed: G0 + dw err %.3g, zeroed err %.3g' % (case.name, _path(case), e_acc, e_zero))
    assert e_acc < WGRAD_TOL and e_zero < WGRAD_TOL, (case.name, e_acc, e_zero)


def _tb2_child():
    """Runs in a fresh process with CTDET_WGRAD_TB=2 (the library reads it once): the rows the 128x128 variant takes."""
    assert os.environ.get('CTDET_WGRAD_TB') == '2'
    bad = 0
    for case in G.WGRAD_CASES:
        if not case.tb2:
            continue
        ref = _problem(case)[1][0]
        got = _wgrad(case, float('nan'))
        err = rel_err(got.double(), ref)
        path = 'tapmajor' if case.cin % 128 == 0 else 'generic'
        print('WGRAD-TB2 %s path=%s err %.3g' % (case.name, path, err))
        bad += not (bool(torch.isfinite(got).all()) and err < WGRAD_TOL)
    return 1 if bad else 0


def test_wgrad_tb2_variant_in_a_child_process():
    rows = [c for c in G.WGRAD_CASES if c.tb2]
    assert any(c.cin % 128 == 0 for c in rows) and any(c.cin % 64 for c in rows)
    env = dict(os.environ, CTDET_WGRAD_TB='2')
    env.pop('CTDET_WGRAD_GENERIC', None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--tb2-child'], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.count('WGRAD-TB2') == len(rows)


# ------------------------------------------------------------------------------------------------ data gradient
def _configs():
    """(desc.config, name) of the heuristic and of every implicit-GEMM tile configuration."""
    lib = _lib.lib()
    out = [(0, 'auto')]
    for i in range(lib.ct_conv_num_configs()):
        name = lib.ct_conv_config_name(i).decode()
        if name != 'valu':
            out.append((i + 1, name))
    return out


def _dz_and_weights(case):
    """dZ on the device and the weight parts as the engine lists them: the live parts, then the all-zero part."""
    inp = _problem(case)[0]
    ws = [p.to(DEV) for p in inp.parts]
    if case.zero:
        ws.append(torch.zeros(case.zero, case.cin, case.kh, case.kw, device=DEV))
    n = len(ws)
    ptrs = (C.c_void_p * n)(*[w.data_ptr() for w in ws])
    couts = (C.c_int * n)(*[w.shape[0] for w in ws])
    return inp.dz_buf.to(DEV), ws, ptrs, couts, n


def _dgrad_direct(case, config, ksplit=None):
    """One ct_conv2d_fwd(transposed) launch into a fresh copy of G0 -> the buffer on the CPU.  ksplit: None = no workspace."""
    lib = _lib.lib()
    inp = _problem(case)[0]
    dz_d, ws, ptrs, couts, n = _dz_and_weights(case)
    kpad, mpad = lib.ct_conv_kpad(case.zc, case.kh, case.kw), lib.ct_conv_mpad(case.cin)
    wpk = torch.full((kpad, mpad), float('nan'), device=DEV)
    _lib.check(lib.ct_conv_pack_weights_dgrad(ptrs, couts, n, case.cin, case.kh, case.kw, wpk.data_ptr(), mpad, kpad, _s()), 'pack')
    ones, zeros = torch.ones(mpad, device=DEV), torch.zeros(mpad, device=DEV)
    out = torch.empty(inp.g0.shape, device=DEV).copy_(inp.g0)
    ksws = None if ksplit is None else torch.full((G.ksplit_floats(case),), float('nan'), device=DEV)
    d = G.dgrad_desc(case, dz_d, out, ones, zeros, wpacked=wpk, mpad=mpad, kpad=kpad, config=config, ksplit=ksplit or 0,
                     ksplit_ws=ksws)
    _lib.check(lib.ct_conv2d_fwd(C.byref(d), _s()), 'dgrad %s config %d' % (case.name, config))
    torch.cuda.synchronize()
    return out.cpu()


def _dgrad_x3(case, cfg):
    """The same launch through ct_conv2d_x3_fwd with the engine's descriptor (ksplit = -1 and its slab workspace)."""
    lib = _lib.lib()
    inp = _problem(case)[0]
    dz_d, ws, ptrs, couts, n = _dz_and_weights(case)
    bk = lib.ct_conv_x3_config_bk(cfg)
    wx3 = torch.empty(lib.ct_conv_x3_packed_bytes(case.zc, case.cin, case.kh, case.kw, bk), dtype=torch.uint8, device=DEV)
    wx3.fill_(0xFF)
    _lib.check(lib.ct_conv_pack_weights_x3_dgrad(ptrs, couts, n, case.cin, case.kh, case.kw, bk, wx3.data_ptr(), _s()), 'pack x3')
    mpad = lib.ct_conv_mpad(case.cin)
    ones, zeros = torch.ones(mpad, device=DEV), torch.zeros(mpad, device=DEV)
    out = torch.empty(inp.g0.shape, device=DEV).copy_(inp.g0)
    ksws = torch.full((G.ksplit_floats(case),), float('nan'), device=DEV)
    d = G.dgrad_desc(case, dz_d, out, ones, zeros, mpad=mpad, kpad=lib.ct_conv_kpad(case.zc, case.kh, case.kw), ksplit=-1,
                     ksplit_ws=ksws)
    _lib.check(lib.ct_conv2d_x3_fwd(C.byref(d), wx3.data_ptr(), cfg, _s()), 'dgrad x3 %s config %d' % (case.name, cfg))
    torch.cuda.synchronize()
    return out.cpu()


def _slice_errors(case, got, ref):
    """per-image rel_err of the slice against `ref` (+ G0 where the launch accumulates)"""
    g0 = _problem(case)[0].g0
    lo, hi = case.out_coff, case.out_coff + case.cin
    want = ref.double() + g0[:, lo:hi].double() if case.acc else ref.double()
    return [rel_err(got[n, lo:hi].double(), want[n]) for n in range(case.B)]


def _outside_untouched(case, got):
    g0 = _problem(case)[0].g0
    lo, hi = case.out_coff, case.out_coff + case.cin
    return torch.equal(_bits(got[:, :lo]), _bits(g0[:, :lo])) and torch.equal(_bits(got[:, hi:]), _bits(g0[:, hi:]))


def _check_direct(case, config, cname, ksplit):
    _, (_dw, ref), (_dw32, cpu32) = _problem(case)
    e32 = max(rel_err(cpu32[n].double(), ref[n]) for n in range(case.B))
    got = _dgrad_direct(case, config, ksplit)
    again = _dgrad_direct(case, config, ksplit)
    errs = _slice_errors(case, got, ref)
    tight = max(TIGHT_FACTOR * e32, TIGHT_FLOOR)
    print('DGRAD-DIRECT %s cfg=%s ks=%s err %s e32 %.3g err/e32 %.2f tight %.3g' %
          (case.name, cname, 'off' if ksplit is None else ksplit, ' '.join('%.3g' % e for e in errs), e32, max(errs) / e32, tight))
    who = (case.name, cname, ksplit)
    assert torch.isfinite(got).all(), who
    assert _outside_untouched(case, got), who + ('channels outside the slice were written',)
    assert max(errs) < HARD, who + (errs,)
    assert max(errs) < tight, who + (errs, e32)
    assert torch.equal(_bits(got), _bits(again)), who + ('two launches differ',)


@pytest.mark.parametrize('case', G.DGRAD_CASES, ids=_ids(G.DGRAD_CASES))
def test_dgrad_direct_every_config_vs_float64(case):
    for config, cname in _configs():
        _check_direct(case, config, cname, None)


SPLITK = tuple(c for c in G.DGRAD_CASES if c.splitk)


@pytest.mark.parametrize('case', SPLITK, ids=_ids(SPLITK))
def test_dgrad_direct_split_k_vs_float64(case):
    names = dict(_configs())
    for config in KSPLIT_CONFIGS:
        for ks in KSPLITS:
            _check_direct(case, config, names[config], ks)


X3 = tuple(c for c in G.DGRAD_CASES if c.x3)


@pytest.mark.parametrize('case', X3, ids=_ids(X3))
def test_dgrad_x3_every_config_vs_float64(case):
    lib = _lib.lib()
    ref = _problem(case)[1][1]
    ran = 0
    for cfg in range(lib.ct_conv_x3_num_configs()):
        if lib.ct_conv_x3_config_h2(cfg):           # the f16x2 configurations are forward-only
            continue
        cname = lib.ct_conv_x3_config_name(cfg).decode()
        got = _dgrad_x3(case, cfg)
        errs = _slice_errors(case, got, ref)
        print('DGRAD-X3 %s cfg=%s err %s' % (case.name, cname, ' '.join('%.3g' % e for e in errs)))
        assert torch.isfinite(got).all(), (case.name, cname)
        assert _outside_untouched(case, got), (case.name, cname, 'channels outside the slice were written')
        assert max(errs) < HARD, (case.name, cname, errs)
        ran += 1
    assert ran >= 1


if __name__ == '__main__':
    if sys.argv[1:] == ['--tb2-child']:
        sys.exit(_tb2_child())
    sys.exit('usage: %s --tb2-child' % sys.argv[0])
