"""The four records of the device input pipeline have ONE layout: a C program that includes only include/ctdet.h prints
sizeof and offsetof of every field, and the numpy dtypes and ctypes structures of ctdet/aug_records.py must say the
same, field by field.  The table below restates the header; the program also takes a typed pointer to every field, so
a field whose C type differs from the table does not compile."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from ctdet import _lib, aug_plan_ref, aug_records, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_OF_C = {'long long': '<i8', 'unsigned long long': '<u8', 'int': '<i4', 'float': '<f4', 'short': '<i2'}


def _fields(ctype, names):
    return [(n.split('[')[0], ctype, int(n.split('[')[1][:-1]) if '[' in n else 0) for n in names.split()]


RECORDS = {     # record -> [(field, C type, array length or 0)] in declaration order
    'ct_aug_plan_record': (_fields('long long', 'src_off')
                           + _fields('int', 'H W crop_l crop_t crop_w crop_h exp_w exp_h exp_left exp_top mirror interp '
                                            'flags hue_delta')
                           + _fields('float', 'beta alpha sat_alpha fill[3] pad0 pad1')),
    'ct_aug_sample': (_fields('long long', 'src_off') + _fields('unsigned long long', 'sample_id')
                      + _fields('int', 'H W box_begin box_end image cls') + _fields('float', 'weight')
                      + _fields('int', 'flags')),
    'ct_mosaic_tile': _fields('int', 'x0 y0 w h'),
    'ct_resize_tap': _fields('int', 'first') + _fields('short', 'c[8]'),
}
DTYPES = {'ct_aug_plan_record': aug_records.PLAN_DTYPE, 'ct_aug_sample': aug_records.SAMPLE_DTYPE,
          'ct_mosaic_tile': aug_records.TILE_DTYPE, 'ct_resize_tap': aug_records.TAP_DTYPE}
STRUCTS = {'ct_aug_plan_record': ops.AugPlan, 'ct_resize_tap': _lib.ResizeTap}
PLAN_NAMES = ('src_off', 'H', 'W', 'crop', 'exp', 'mirror', 'interp', 'flags', 'hue', 'beta', 'alpha', 'sat', 'fill', 'pad')


def _leaves(dtype):
    """[(byte offset, scalar type)] of a numpy record, sub-arrays spelled out."""
    out = []
    for name in dtype.names:
        ft, off = dtype.fields[name][:2]
        base, shape = ft.subdtype or (ft, ())
        out += [(off + k * base.itemsize, base.str) for k in range(int(np.prod(shape, dtype=np.int64)))]
    return out


@pytest.fixture(scope='module')
def c_layout(tmp_path_factory):
    """{record: (sizeof, {field: (offsetof, sizeof)})} as gcc lays out include/ctdet.h."""
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    tmp = tmp_path_factory.mktemp('aug_records')
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ctdet.h"', 'int main(void) {']
    for rec, fields in RECORDS.items():
        lines.append('    { %s r; printf("%s %%zu\\n", sizeof r);' % (rec, rec))
        for f, ctype, count in fields:
            lines.append('      { const %s* p = %sr.%s; (void)p; printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof r.%s); }'
                         % (ctype, '' if count else '&', f, rec, f, rec, f, f))
        lines.append('    }')
    lines += ['    return 0;', '}']
    src, exe = tmp / 'layout.c', str(tmp / 'layout')
    src.write_text('\n'.join(lines) + '\n')
    r = subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(REPO, 'include'),
                        str(src), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = {}
    for line in r.stdout.split('\n'):
        w = line.split()
        if len(w) == 2:
            got[w[0]] = (int(w[1]), {})
        elif len(w) == 3:
            rec, f = w[0].split('.')
            got[rec][1][f] = (int(w[1]), int(w[2]))
    return got


@pytest.mark.parametrize('rec', sorted(RECORDS))
def test_numpy_dtype_matches_the_header(c_layout, rec):
    size, fields = c_layout[rec]
    assert [f for f, _, _ in RECORDS[rec]] == list(fields)
    dt = DTYPES[rec]
    assert dt.itemsize == size == {'ct_aug_plan_record': 96, 'ct_aug_sample': 48, 'ct_mosaic_tile': 16, 'ct_resize_tap': 20}[rec]
    want = []
    for f, ctype, count in RECORDS[rec]:
        elem = np.dtype(NP_OF_C[ctype])
        assert fields[f][1] == elem.itemsize * max(count, 1), (rec, f)
        want += [(fields[f][0] + k * elem.itemsize, elem.str) for k in range(max(count, 1))]
    assert _leaves(dt) == want
    if rec == 'ct_aug_plan_record':         # the plan dict's names: crop = crop_l.., exp = exp_w.., hue, sat, pad
        assert dt.names == PLAN_NAMES
        at = {off: f for f, (off, _) in fields.items()}
        assert all(at[dt.fields[n][1]].startswith(n) for n in dt.names)
    else:
        assert dt.names == tuple(f for f, _, _ in RECORDS[rec])


@pytest.mark.parametrize('rec', sorted(STRUCTS))
def test_ctypes_struct_matches_the_header(c_layout, rec):
    size, fields = c_layout[rec]
    dt = np.dtype(STRUCTS[rec])
    assert dt.itemsize == size and _leaves(dt) == _leaves(DTYPES[rec])
    assert {n: (dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names} == fields
    assert list(dt.names) == [f for f, _, _ in RECORDS[rec]]


def test_one_definition_many_names():
    assert ops.AugPlan is aug_records.AugPlan and _lib.ResizeTap is aug_records.ResizeTap
    assert ops.TAP_DTYPE is aug_records.TAP_DTYPE
    assert ops.AUG_SAMPLE_DTYPE is aug_plan_ref.SAMPLE_DTYPE is aug_records.SAMPLE_DTYPE
    assert aug_plan_ref.PLAN_DTYPE is aug_records.PLAN_DTYPE and aug_plan_ref.TILE_DTYPE is aug_records.TILE_DTYPE
    assert aug_plan_ref.plan_dict is aug_records.plan_dict
    assert (aug_records.PLAN_BYTES, aug_records.SAMPLE_BYTES, aug_records.TILE_BYTES, aug_records.TAP_BYTES) == (96, 48, 16, 20)


def test_plan_dict_and_record_are_inverse():
    plan = dict(H=7, W=9, crop=(1, 2, 3, 4), exp=(5, 6, 1, 0), mirror=1, interp=2, flags=5, hue=-3, beta=0.5, alpha=1.25,
                sat=0.75)
    recs = np.zeros(2, dtype=aug_records.PLAN_DTYPE)
    aug_records.plan_records(recs[1:], [plan])
    assert aug_records.plan_dict(recs[1]) == plan and tuple(aug_records.PLAN_KEYS) == tuple(plan)
    assert not recs[0].tobytes().strip(b'\0') and recs[1]['src_off'] == 0 and not recs[1]['fill'].any()
    c = ops.AugPlan.from_buffer_copy(recs[1].tobytes())
    assert (c.crop_l, c.crop_t, c.crop_w, c.crop_h, c.exp_w, c.exp_h, c.exp_left, c.exp_top) == (1, 2, 3, 4, 5, 6, 1, 0)
    assert (c.H, c.W, c.mirror, c.interp, c.flags, c.hue_delta, c.beta, c.alpha, c.sat_alpha) == (7, 9, 1, 2, 5, -3, 0.5, 1.25, 0.75)
