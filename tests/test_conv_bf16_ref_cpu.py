"""The row table of the bf16 channels-last convolution (tests/conv_bf16_cases.py) and its bound, proved without a device:
  coverage   under each row's environment ct_conv_bf16_variant_name (pure host code) answers the variant the row claims, the rows
             reach all seven, every BK = 32 variant has a row whose step in front of the last one runs past cin, every variant a
             tail-free row, and the split-K / epilogue / slice edges are there;
  reference  torch-CPU float32 on the bfloat16-rounded operands, rounded once, meets the bound on every row with no violation;
  mutations  eight wrong ways to compute the step fail the bound on every row they touch; each line says whether the criterion
             tests/test_gpu_bf16.py used before (_close) would have passed the mutant."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO          # first: it puts the package on sys.path (the child process below has no pytest)
import conv_bf16_cases as T
from ctdet import _lib


def _desc(case):
    """A descriptor of the row the launcher would accept; the pointers are dummies (the query never follows them)."""
    d = T.fill_geometry(case, _lib.ConvDesc())
    d.in_ = d.wpacked = d.scale = d.shift = d.out = 64
    if case.res_slice:
        d.res = 64
    for g, (c0, c1, base, size) in enumerate(T.segments(case) if case.segs else []):
        d.out = None
        sg = d.seg[g]
        sg.ptr, sg.co_begin, sg.co_end, sg.pix_stride, sg.img_stride, sg.base = 64, c0, c1, c1 - c0, size, base
    return d


def _variant(case):
    name = _lib.lib().ct_conv_bf16_variant_name(C.byref(_desc(case)))
    assert name is not None, (case.name, _lib.lib().ct_last_error_string())
    return name.decode()


def _set_env(case, monkeypatch):
    for k in T.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env:
        monkeypatch.setenv(k, v)


def test_rows_name_the_variant_the_launcher_picks(monkeypatch):
    seen = set()
    for case in T.CASES:
        if case.child:
            continue
        _set_env(case, monkeypatch)
        assert _variant(case) == case.variant, case.name
        seen.add(case.variant)
    assert seen == set(T.VARIANTS) - {'bf16:128x128k32'}


def _ring_child():
    """In a fresh process with CTDET_BF16_BK=32 (read once): the variant of every row that sets it."""
    assert os.environ.get('CTDET_BF16_BK') == '32'
    for case in T.CASES:
        if case.child:
            print('VARIANT %s %s' % (case.name, _variant(case)))
    return 0


def test_ring_rows_name_their_variant_in_a_child_process():
    rows = [c for c in T.CASES if c.child]
    assert len(rows) >= 4 and all(dict(c.env) == {'CTDET_BF16_BK': '32'} and c.variant == 'bf16:128x128k32' for c in rows)
    env = {k: v for k, v in os.environ.items() if k not in T.SWITCHES}
    env['CTDET_BF16_BK'] = '32'
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--ring-child'], env=env, timeout=120, cwd=REPO,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    for c in rows:
        assert 'VARIANT %s %s\n' % (c.name, c.variant) in r.stdout, (c.name, r.stdout[-2000:])


def test_query_refuses_what_the_launcher_refuses():
    lib = _lib.lib()
    d = _desc(T.BY_NAME['sk_64_96'])
    d.cin = 60
    assert lib.ct_conv_bf16_variant_name(C.byref(d)) is None
    msg = lib.ct_last_error_string().decode()
    assert msg.startswith('ct_conv_bf16_variant_name:') and 'multiples of 8' in msg, msg
    assert lib.ct_conv_bf16_variant_name(None) is None
    assert 'null tensor' in lib.ct_last_error_string().decode()


def test_table_covers_the_edges():
    rows = T.CASES
    of = lambda v: [c for c in rows if c.variant == v]
    for v in T.VARIANTS:
        assert of(v), v
    for v in ('bf16:128x64k32', 'bf16:128x128k32', 'bf16:256x256k32'):
        tails = [c for c in of(v) if c.tail]
        assert tails, v
        assert any(c.x_ctot > c.x_coff + c.cin for c in tails), v       # ... with channels of another tensor behind the slice
    for v in T.VARIANTS:
        if v.endswith('s'):
            assert all(c.cin == 8 for c in of(v)), v
        else:       # both instantiations of the variant: channels that fill their steps, and a tail
            assert any(c.cin % 64 == 0 for c in of(v)) and any(c.cin % 64 for c in of(v)), v
    # a ragged pixel tile, a ragged cout tile and more than one tile of each on the wide variants
    for v in ('bf16:128x128k32s', 'bf16:128x128k64', 'bf16:128x128k32', 'bf16:256x256k32'):
        assert any(c.npix % T.BM[v] and c.npix > T.BM[v] and c.cout > 128 for c in of(v)), v
    assert any(c.cout % 128 == 2 for c in of('bf16:128x128k32s')) and any(c.cout % 8 for c in rows)
    img = of('bf16:128x64k32s')
    assert {c.k * c.k % 4 for c in img} >= {0, 1} and any(c.k == 1 for c in img) and any(c.x_slice for c in img)
    assert any(c.k == 7 and c.stride == 2 for c in img)
    # split-K: a split that owns a single k-step, the engine's workspace, head segments
    sk = [c for c in rows if len(c.ksplits) > 1]
    assert any(set(c.ksplits) == set(T.KSPLITS) for c in sk)
    assert any(c.k == 1 and c.cin == 128 and c.variant == 'bf16:128x64k64' and 2 in c.ksplits for c in sk)
    assert any(c.segs and len(c.parts) == 3 for c in sk)
    assert any(c.lo and c.res_slice and c.res_slice[1] for c in sk)
    # epilogue fields
    assert any(c.lo for c in rows) and any(c.res_slice and c.res_slice[1] == 8 and c.res_slice[0] == c.cout + 24 for c in rows)
    assert any(c.res_slice and c.res_scale != 1.0 for c in rows)
    assert any(not c.relu and not c.lo and bool((T.ref64(c) < 0).any()) for c in rows if not c.segs)
    for c in rows:
        if c.lo:
            lo = T.make_inputs(c).lo
            assert (lo == 0).any() and torch.isinf(lo).any() and int((lo > 0).sum()) == 1, c.name
            r = T.ref64(c)
            assert bool((r < 0).any()) and bool((r[:, 2] == 0.25).any()), c.name       # every kind of floor acts or lets through
    # the pairs that must be bit-equal share inputs
    for a, b in T.BIG_PAIRS:
        assert T.make_inputs(T.BY_NAME[a]) is T.make_inputs(T.BY_NAME[b])
        assert T.BY_NAME[a].variant == 'bf16:256x256k32' != T.BY_NAME[b].variant


@pytest.mark.parametrize('case', [c for c in T.CASES if not c.inputs_of], ids=lambda c: c.name)
def test_cpu_fp32_meets_the_bound(case):
    y = T.cpu32(case)
    assert torch.isfinite(T.ref64(case)).all()
    if case.segs:
        worst, err, _ = T.judge_f32(case, y)
        assert worst <= 1.0 / T.TIGHT_FACTOR + 1e-12 and err < T.HARD, (case.name, worst, err)
        return
    j = T.judge(case, T.rne_bf16(y))
    assert j.violations == 0, (case.name, j)


# ---------------------------------------------------------------------------------------------------------------- mutated references
def _x(case):
    inp = T.make_inputs(case)
    return inp.x_buf[:, case.x_coff:case.x_coff + case.cin]


def _w(case):
    return torch.cat(T.make_inputs(case).parts)


def _m_out_trunc(case):
    return None if case.segs else T.trunc_bf16(T.cpu32(case))


def _m_operands_trunc(case):
    return T.fused_step(case, torch.float32, x=T.trunc_bf16(_x(case)), w=T.trunc_bf16(_w(case)))


def _m_acc_bf16(case):
    return T.fused_step(case, torch.float32, acc=T.rne_bf16)


def _m_group_dropped(case):
    w = T.rne_bf16(_w(case)).clone()
    w[:, case.cin - 8:, case.k // 2, case.k // 2] = 0         # the last 8-channel group at the centre tap (in bounds on every row)
    return T.fused_step(case, torch.float32, w=w)


def _m_last_step_dropped(case):
    if case.cin == 8:
        return None
    w = T.rne_bf16(_w(case)).clone()
    bk = T.BK[case.variant]
    w[:, (case.cin - 1) // bk * bk:] = 0                       # the last channel step that holds a channel, at every tap
    return T.fused_step(case, torch.float32, w=w)


def _m_tile_row_from_neighbour(case):
    bm = T.BM[case.variant]
    if case.npix <= bm:
        return None
    y = T.cpu32(case).permute(0, 2, 3, 1).reshape(case.npix, case.cout).clone()
    y[bm - 1] = y[bm]                                           # the first tile's last pixel row <- the next tile's first
    return y.view(case.B, case.oh, case.ow, case.cout).permute(0, 3, 1, 2)


def _m_res_offset_0(case):
    if not (case.res_slice and case.res_slice[1]):
        return None
    return T.fused_step(case, torch.float32, res=T.rne_bf16(T.make_inputs(case).res_buf[:, :case.cout]))


def _m_lo_ignored(case):
    return T.fused_step(case, torch.float32, lo=None) if case.lo else None


MUTANTS = [('output rounded toward zero', _m_out_trunc), ('operands truncated', _m_operands_trunc),
           ('accumulator rounded to bf16', _m_acc_bf16), ('8-channel group dropped at one tap', _m_group_dropped),
           ('last channel step dropped', _m_last_step_dropped), ("tile's last row from its neighbour", _m_tile_row_from_neighbour),
           ('residual read at offset 0', _m_res_offset_0), ('lo ignored', _m_lo_ignored)]


@pytest.mark.parametrize('what,mutant', MUTANTS, ids=[m[0].replace(' ', '_') for m in MUTANTS])
def test_mutated_reference_fails_the_bound(what, mutant):
    touched = 0
    for case in T.CASES:
        if case.inputs_of:
            continue
        y = mutant(case)
        if y is None:
            continue
        touched += 1
        if case.segs:
            worst, _err, _ = T.judge_f32(case, y)
            old = T.old_close(y, T.cpu32(case))       # (the old criterion judged the fp32 segments too)
            print('MUTANT %-36s %-16s fp32 rel_err / bound %.3g   old _close passes: %s' % (what, case.name, worst, old))
            assert worst > 1.0, (what, case.name, worst)
            continue
        y = y if mutant is _m_out_trunc else T.rne_bf16(y)
        j = T.judge(case, y)
        old = T.old_close(y, T.cpu32(case))
        print('MUTANT %-36s %-16s violations %6d (%.3g %%)   old _close passes: %s' % (what, case.name, j.violations, 100 * j.share,
                                                                                       old))
        assert j.violations > 0, (what, case.name, j)
    assert touched >= 2, what


if __name__ == '__main__':
    if sys.argv[1:] == ['--ring-child']:
        sys.exit(_ring_child())
    sys.exit('usage: %s --ring-child' % sys.argv[0])
