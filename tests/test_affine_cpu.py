"""The random affine stage on the host: the twin of ct_aug_affine_plan / ct_preproc_warp_affine
(ctdet/aug_plan_ref.py affine_matrix, affine_batch, warp_affine) against the properties include/ctdet.h RANDOM AFFINE
states, the coverage of tests/affine_cases.py, the layout of ct_affine_record as gcc sees the header, and the Python
surface's refusals.  No device."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import affine_cases as cases
import mosaic_cases
from ctdet import aug_plan_ref as ref
from ctdet import aug_records

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _rows_of(t, i):
    return t['truths'][t['gt_off'][i]:t['gt_off'][i + 1]]


# ---------------------------------------------------------------------------------------------------------- the table
def test_the_table_covers_what_it_was_built_for():
    t, r = cases.build('A96'), cases.twin('A96', 'P_ALL')
    before, after = np.diff(t['gt_off']), np.diff(r.gt_off)
    assert (before > 0).all() and r.status.tolist() == [0, 0, int(r.fallback.sum()), int(after.sum())]
    kept_all = (after == before) & ~r.fallback
    partial = (after < before) & (after > 0)
    assert kept_all.any() and partial.any() and r.fallback.any()
    assert (before[3], after[3]) == (12, 7) and r.fallback.nonzero()[0].tolist() == [mosaic_cases.TINY_IMAGE]
    assert (r.records['flags'][~r.fallback] == 1).all() and (r.records['flags'][r.fallback] == 6).all()
    r8 = cases.twin('A8', 'P_ALL')
    b8, a8 = np.diff(cases.build('A8')['gt_off']), np.diff(r8.gt_off)
    assert ((a8 < b8) & (a8 > 0)).sum() >= 2
    for name in ('A96', 'A8'):
        flags = cases.twin(name, 'P_HALF').records['flags']
        assert (flags == 4).any() and (flags & 1).any(), name       # both gate outcomes
        assert (cases.twin(name, 'P_NONE').records['flags'] == 4).all()


# --------------------------------------------------------------------------------------------------------- the matrix
def test_inverse_maps_the_corners_back_and_the_determinant_is_bounded():
    for S in (8, 96, 300):
        for i in range(200):
            rec = ref.affine_matrix(cases.SEED, 5000 + i, S, cases.P_ALL)
            f, v = rec['fwd'], rec['inv']
            for u, w in ((0, 0), (S, 0), (0, S), (S, S)):
                x, y = f[0] * u + f[1] * w + f[2], f[3] * u + f[4] * w + f[5]
                assert abs(v[0] * x + v[1] * y + v[2] - u) < 1e-9 and abs(v[3] * x + v[4] * y + v[5] - w) < 1e-9
            s = ref.affine_draws(cases.SEED, 5000 + i, S, cases.P_ALL)['s']
            assert f[0] * f[4] - f[1] * f[3] >= 0.75 * s * s * (1 - 1e-12)


def test_draws_lie_inside_their_bounds():
    P, S = cases.P_ALL, 96
    ids = np.arange(10000, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(17)
    d0 = ref.draws(cases.SEED, 0, ref.SLOT_AFFINE, 0)       # shape check of the scalar form
    assert d0.shape == (4,)
    lo = ids & np.uint64(0xFFFFFFFF)
    hi = ids >> np.uint64(32)
    k0, k1 = cases.SEED & 0xFFFFFFFF, cases.SEED >> 32
    w0 = ref.philox4x32(lo, hi, ref.SLOT_AFFINE, 0, k0, k1)
    w1 = ref.philox4x32(lo, hi, ref.SLOT_AFFINE, 1, k0, k1)
    t = ref.uniform(-P.rot_half_tan, P.rot_half_tan, w0[:, 0])
    s = ref.uniform(P.scale_lo, P.scale_hi, w0[:, 1])
    kx, ky = ref.uniform(-P.shear_tan, P.shear_tan, w0[:, 2]), ref.uniform(-P.shear_tan, P.shear_tan, w0[:, 3])
    tx = ref.uniform(0.5 - P.translate, 0.5 + P.translate, w1[:, 0]) * S
    angle = np.degrees(2 * np.arctan(t))
    assert np.abs(angle).max() <= 10.0 + 1e-9 and np.abs(angle).max() > 9.9
    assert s.min() >= 0.5 and s.max() <= 1.5 and s.max() - s.min() > 0.99
    for k in (kx, ky):
        assert np.degrees(np.arctan(np.abs(k))).max() <= 2.0 + 1e-9
    assert tx.min() >= 0.4 * S - 1e-9 and tx.max() <= 0.6 * S + 1e-9
    # the vector form above is the scalar form affine_draws uses
    for i in (0, 77, 9999):
        w = ref.affine_draws(cases.SEED, int(ids[i]), S, P)
        assert (w['t'], w['s'], w['kx'], w['ky'], w['tx']) == (t[i], s[i], kx[i], ky[i], tx[i])
    assert P.rot_half_tan == math.tan(math.radians(10) / 2) and P.shear_tan == math.tan(math.radians(2))


# ----------------------------------------------------------------------------------------------------------- the rows
def test_identity_gate_and_fallback_keep_the_rows_bytes():
    t = cases.build('A96')
    none = cases.twin('A96', 'P_NONE')
    assert none.truths.tobytes() == t['truths'].tobytes() and none.gt_off.tobytes() == t['gt_off'].tobytes()
    assert all(tuple(r['fwd']) == IDENTITY and tuple(r['inv']) == IDENTITY for r in none.records)
    for pname in ('P_ALL', 'P_HALF'):
        r = cases.twin('A96', pname)
        same = np.flatnonzero((r.records['flags'] & 4) != 0)
        assert len(same)
        for i in same:
            assert r.image_rows[i].tobytes() == _rows_of(t, i).tobytes()
            assert tuple(r.records[i]['fwd']) == IDENTITY and tuple(r.records[i]['inv']) == IDENTITY
    # a mapped row is the clipped bounding box of its corners, label and weight untouched
    r = cases.twin('A96', 'P_ALL')
    mapped, keep = ref.affine_rows(_rows_of(t, 3), r.records[3]['fwd'], t['S'], cases.P_ALL.min_side, cases.P_ALL.min_visible)
    assert mapped[keep].tobytes() == r.image_rows[3].tobytes()
    assert (mapped[:, 4:] == _rows_of(t, 3)[:, 4:]).all() and (mapped[:, :4] >= 0).all() and (mapped[:, :4] <= 1).all()


def test_safety_rule_of_the_twin():
    t = cases.build('A96')
    rows = len(t['truths'])
    off = t['gt_off'].astype(np.int64).copy()
    off[2] = -4                     # image 1 ends below its begin: refused; image 2 begins at 0, below image 0's end
    off[6] = off[5] - 3             # a decreasing pair: image 5 refused, image 6 begins below image 4's end
    off[12] = rows + 50             # past truths_rows: clamped
    r = ref.affine_batch(t['truths'], off, t['ids'], t['S'], cases.SEED, cases.P_NONE)
    refused = [1, 2, 5, 6]
    assert r.status[:2].tolist() == [ref.STATUS_BAD_IMAGE, len(refused)]
    assert [i for i in range(t['n']) if len(r.image_rows[i]) == 0] == refused
    c = np.clip(off, 0, rows)
    for i in range(t['n']):
        if i not in refused:
            assert r.image_rows[i].tobytes() == t['truths'][c[i]:c[i + 1]].tobytes(), i
    assert (r.records['flags'] == 4).all() and r.gt_off[-1] == sum(len(x) for x in r.image_rows) <= rows
    # a capacity below the table clamps every offset to it
    r = ref.affine_batch(t['truths'], t['gt_off'], t['ids'], t['S'], cases.SEED, cases.P_NONE, truths_rows=20)
    assert r.status[:2].tolist() == [0, 0] and r.gt_off[-1] == 20 and r.truths.tobytes() == t['truths'][:20].tobytes()


# --------------------------------------------------------------------------------------------------------- the pixels
def _warp64(x, records, border):
    """The pixel rule of include/ctdet.h evaluated wholly in float64."""
    x = x.astype(np.float64)
    B, _, S, _ = x.shape
    out = np.empty_like(x)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    pad = np.empty((3, S + 2, S + 2))
    for n in range(B):
        v = records[n]['inv']
        X, Y = v[0] * xx + v[1] * yy + v[2], v[3] * xx + v[4] * yy + v[5]
        inside = (-1 < X) & (X < S) & (-1 < Y) & (Y < S)
        X, Y = np.where(inside, X, 0), np.where(inside, Y, 0)
        ix, iy = np.floor(X).astype(int), np.floor(Y).astype(int)
        fx, fy = X - ix, Y - iy
        for c in range(3):
            pad[c] = border[c]
            pad[c, 1:-1, 1:-1] = x[n, c]
            p = pad[c]
            top = p[iy + 1, ix + 1] * (1 - fx) + p[iy + 1, ix + 2] * fx
            bot = p[iy + 2, ix + 1] * (1 - fx) + p[iy + 2, ix + 2] * fx
            out[n, c] = np.where(inside, top * (1 - fy) + bot * fy, border[c])
    return out


def test_warp_with_identity_records_returns_its_input():
    x = cases.pixels('A8')
    n = len(x)
    flagged = np.array([ref.affine_identity()] * n)
    general = np.array([ref.affine_identity(0)] * n)          # the identity matrix through the general path
    assert ref.warp_affine(x, flagged, cases.BORDER).tobytes() == x.tobytes()
    assert ref.warp_affine(x, general, cases.BORDER).tobytes() == x.tobytes()


def test_warp_against_the_rule_in_float64():
    """Nine fp32 roundings of values <= 510 and three weight roundings: < 3.3e-4; the bound is 5e-4."""
    x, r = cases.pixels('A96'), cases.twin('A96', 'P_ALL')
    got = ref.warp_affine(x, r.records, cases.BORDER)
    assert got.dtype == np.float32 and np.abs(x).max() <= 255
    worst = float(np.abs(got.astype(np.float64) - _warp64(x, r.records, cases.BORDER)).max())
    print('warp_affine against float64: worst %.3g' % worst)
    assert worst <= 5e-4
    border = np.asarray(cases.BORDER, dtype=np.float32).reshape(1, 3, 1, 1)
    share = float((got == border).all(1).mean())
    assert 0.02 < share < 0.9           # the warps bring border in and keep image


def test_warp_of_non_finite_records_is_border():
    x = cases.pixels('A8')[:4]
    recs = np.array([ref.affine_identity(0)] * 4)
    recs[0]['inv'][:] = np.nan
    recs[1]['inv'][:] = (np.inf, 0, 0, 0, -np.inf, 0)
    recs[2]['inv'][:] = (1e300, 1e300, 1e300, -1e300, 1e300, 1e300)
    recs[3]['inv'][:] = (1, 0, np.nan, 0, 1, 0)
    got = ref.warp_affine(x, recs, cases.BORDER)
    assert (got == np.asarray(cases.BORDER, dtype=np.float32).reshape(1, 3, 1, 1)).all()


# ------------------------------------------------------------------------------------------------------------ layout
RECORD = [('fwd', 'double', 6), ('inv', 'double', 6), ('flags', 'int', 0), ('pad', 'int', 0)]
PARAMS = [('rot_half_tan', 'double'), ('scale_lo', 'double'), ('scale_hi', 'double'), ('shear_tan', 'double'),
          ('translate', 'double'), ('p', 'float'), ('min_side', 'float'), ('min_visible', 'float')]


@pytest.fixture(scope='module')
def c_layout(tmp_path_factory):
    """{struct.field: (offsetof, sizeof)} and {struct: sizeof} as gcc lays out include/ctdet.h, C99 -pedantic."""
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    tmp = tmp_path_factory.mktemp('affine_records')
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ctdet.h"', 'int main(void) {',
             '    ct_affine_record r; ct_affine_params q;',
             '    printf("ct_affine_record %zu\\nct_affine_params %zu\\n", sizeof r, sizeof q);']
    for f, ctype, count in RECORD:
        lines.append('    { const %s* p = %sr.%s; (void)p; printf("ct_affine_record.%s %%zu %%zu\\n", '
                     'offsetof(ct_affine_record, %s), sizeof r.%s); }' % (ctype, '' if count else '&', f, f, f, f))
    for f, ctype in PARAMS:
        lines.append('    { const %s* p = &q.%s; (void)p; printf("ct_affine_params.%s %%zu %%zu\\n", '
                     'offsetof(ct_affine_params, %s), sizeof q.%s); }' % (ctype, f, f, f, f))
    lines += ['    return 0;', '}']
    src, exe = tmp / 'layout.c', str(tmp / 'layout')
    src.write_text('\n'.join(lines) + '\n')
    r = subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(REPO, 'include'),
                        str(src), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = {}
    for line in r.stdout.strip().split('\n'):
        w = line.split()
        got[w[0]] = tuple(int(v) for v in w[1:])
    return got


def test_record_layout_matches_the_header(c_layout):
    assert c_layout['ct_affine_record'] == (104,) == (aug_records.AFFINE_BYTES,)
    assert C.sizeof(aug_records.AffineRecord) == 104 and aug_records.AFFINE_DTYPE.itemsize == 104
    dt, ct = aug_records.AFFINE_DTYPE, np.dtype(aug_records.AffineRecord)
    assert dt.names == ct.names == tuple(f for f, _, _ in RECORD)
    for f, _, _ in RECORD:
        want = c_layout['ct_affine_record.' + f]
        assert (dt.fields[f][1], dt.fields[f][0].itemsize) == want == (ct.fields[f][1], ct.fields[f][0].itemsize), f
    assert aug_records._same_layout(aug_records.AffineRecord, aug_records.AFFINE_DTYPE)
    assert ref.AFFINE_DTYPE is aug_records.AFFINE_DTYPE


def test_params_struct_matches_the_header(c_layout):
    st = aug_records.AffineParamsRecord
    assert c_layout['ct_affine_params'] == (C.sizeof(st),)
    assert [n for n, _ in st._fields_] == [f for f, _ in PARAMS] == list(ref.AffineParams.FIELDS)
    for f, _ in PARAMS:
        d = getattr(st, f)
        assert (d.offset, d.size) == c_layout['ct_affine_params.' + f], f
    s = cases.P_ALL.struct()
    assert [getattr(s, f) for f in ref.AffineParams.FIELDS] == [getattr(cases.P_ALL, f) for f in ref.AffineParams.FIELDS]


# ------------------------------------------------------------------------------------------------- the Python surface
@pytest.mark.parametrize('kw', [dict(degrees=-1), dict(degrees=91), dict(degrees=float('nan')), dict(scale=(0.0, 1.0)),
                                dict(scale=(1.2, 1.1)), dict(scale=(0.5, 4.5)), dict(shear=-0.1), dict(shear=27),
                                dict(translate=-0.01), dict(translate=0.51), dict(p=-0.1), dict(p=1.1),
                                dict(min_side=-1), dict(min_side=1.5), dict(min_visible=-0.1), dict(min_visible=1.01),
                                dict(p=float('inf')), dict(scale=(0.5, float('nan')))])
def test_parameters_out_of_range_are_refused(kw):
    with pytest.raises(ValueError):
        ref.AffineParams(**kw)


def test_parameters_at_their_limits_are_accepted():
    P = ref.AffineParams(degrees=90, scale=(4, 4), shear=math.degrees(math.atan(0.5)), translate=0.5, p=0, min_side=1,
                         min_visible=1)
    assert P.rot_half_tan <= 1.0 and P.shear_tan <= 0.5 and P.scale_lo == P.scale_hi == 4.0
    Z = ref.AffineParams(degrees=0, scale=(1, 1), shear=0, translate=0)
    rec = ref.affine_matrix(cases.SEED, 3, 96, Z)
    assert rec['flags'] == 1 and tuple(rec['fwd']) == IDENTITY and tuple(rec['inv']) == IDENTITY


def test_affine_needs_device_decisions():
    from data.data_augment import preproc
    with pytest.raises(ValueError, match='affine'):
        preproc(96, mosaic_cases.FILL, 0.6, device='cpu', decisions='host', affine=cases.P_ALL)
    with pytest.raises(ValueError, match='affine'):
        preproc(96, mosaic_cases.FILL, 0.6, device='cpu', affine=dict(degrees=5))
    with pytest.raises(ValueError):
        preproc(96, mosaic_cases.FILL, 0.6, device='cpu', decisions='device', seed=1, affine=dict(degrees=500))
    pre = preproc(96, mosaic_cases.FILL, 0.6, device='cpu', decisions='device', seed=1, affine=dict(degrees=5))
    assert pre.affine.rot_half_tan == math.tan(math.radians(5) / 2)
    assert preproc(96, mosaic_cases.FILL, 0.6, device='cpu', decisions='device', seed=1).affine is None
