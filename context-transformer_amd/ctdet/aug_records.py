"""The records of the device input pipeline (include/ctdet.h), each laid out once for Python: the numpy dtypes
host code fills and reads, the ctypes twins callers fill by field name, and their sizes.  numpy and ctypes only: the
host twin (ctdet/aug_plan_ref.py) imports this without torch or the library.  tests/test_aug_records_cpu.py compiles
the header and compares every offset (tests/test_affine_cpu.py does for the two affine structs), so a layout edited
in one place fails at import, at compile time or there."""
import ctypes as C

import numpy as np


class AugPlan(C.Structure):
    """ct_aug_plan_record: one image's augmentation decisions."""
    _fields_ = [('src_off', C.c_longlong), ('H', C.c_int), ('W', C.c_int),
                ('crop_l', C.c_int), ('crop_t', C.c_int), ('crop_w', C.c_int), ('crop_h', C.c_int),
                ('exp_w', C.c_int), ('exp_h', C.c_int), ('exp_left', C.c_int), ('exp_top', C.c_int),
                ('mirror', C.c_int), ('interp', C.c_int), ('flags', C.c_int), ('hue_delta', C.c_int),
                ('beta', C.c_float), ('alpha', C.c_float), ('sat_alpha', C.c_float), ('fill', C.c_float * 3),
                ('pad0', C.c_float), ('pad1', C.c_float)]


class ResizeTap(C.Structure):
    """ct_resize_tap: first source index (unclamped) and the 11-bit coefficients of one output coordinate."""
    _fields_ = [('first', C.c_int), ('c', C.c_short * 8)]


class AffineRecord(C.Structure):
    """ct_affine_record: one image's random affine map, both directions."""
    _fields_ = [('fwd', C.c_double * 6), ('inv', C.c_double * 6), ('flags', C.c_int), ('pad', C.c_int)]


class AffineParamsRecord(C.Structure):
    """ct_affine_params: the host struct ct_aug_affine_plan takes (ctdet/aug_plan_ref.py AffineParams fills it)."""
    _fields_ = [('rot_half_tan', C.c_double), ('scale_lo', C.c_double), ('scale_hi', C.c_double),
                ('shear_tan', C.c_double), ('translate', C.c_double), ('p', C.c_float), ('min_side', C.c_float),
                ('min_visible', C.c_float)]


# ct_aug_plan_record with the field names of the plan dict ops.Augmenter takes: crop = (l, t, w, h), exp = (w, h, left, top)
PLAN_DTYPE = np.dtype([('src_off', '<i8'), ('H', '<i4'), ('W', '<i4'), ('crop', '<i4', (4,)), ('exp', '<i4', (4,)),
                       ('mirror', '<i4'), ('interp', '<i4'), ('flags', '<i4'), ('hue', '<i4'), ('beta', '<f4'),
                       ('alpha', '<f4'), ('sat', '<f4'), ('fill', '<f4', (3,)), ('pad', '<f4', (2,))])
SAMPLE_DTYPE = np.dtype([('src_off', '<i8'), ('sample_id', '<u8'), ('H', '<i4'), ('W', '<i4'), ('box_begin', '<i4'),
                         ('box_end', '<i4'), ('image', '<i4'), ('cls', '<i4'), ('weight', '<f4'), ('flags', '<i4')])    # ct_aug_sample
TILE_DTYPE = np.dtype([('x0', '<i4'), ('y0', '<i4'), ('w', '<i4'), ('h', '<i4')])       # ct_mosaic_tile
TAP_DTYPE = np.dtype([('first', '<i4'), ('c', '<i2', (8,))])                            # ct_resize_tap
AFFINE_DTYPE = np.dtype([('fwd', '<f8', (6,)), ('inv', '<f8', (6,)), ('flags', '<i4'), ('pad', '<i4')])   # ct_affine_record

PLAN_BYTES, SAMPLE_BYTES = PLAN_DTYPE.itemsize, SAMPLE_DTYPE.itemsize
TILE_BYTES, TAP_BYTES = TILE_DTYPE.itemsize, TAP_DTYPE.itemsize
AFFINE_BYTES = AFFINE_DTYPE.itemsize


def scalars(dtype):
    """[(byte offset, scalar type)] of a record's scalars in field order, sub-arrays spelled out."""
    out = []
    for name in dtype.names:
        ft, off = dtype.fields[name][:2]
        base, shape = ft.subdtype or (ft, ())
        out += [(off + k * base.itemsize, base.str) for k in range(int(np.prod(shape, dtype=np.int64)))]
    return out


def _same_layout(struct, dtype):
    """The ctypes struct and the numpy dtype put the same scalars at the same offsets, and a numpy field's name
    begins the name of the struct field at its offset (crop: crop_l, hue: hue_delta, pad: pad0)."""
    c = np.dtype(struct)
    at = {c.fields[n][1]: n for n in c.names}
    return (c.itemsize == dtype.itemsize == C.sizeof(struct) and scalars(c) == scalars(dtype)
            and all(at.get(dtype.fields[n][1], '').startswith(n) for n in dtype.names))


assert _same_layout(AugPlan, PLAN_DTYPE) and _same_layout(ResizeTap, TAP_DTYPE) and _same_layout(AffineRecord, AFFINE_DTYPE)

PLAN_KEYS = ('H', 'W', 'crop', 'exp', 'mirror', 'interp', 'flags', 'hue', 'beta', 'alpha', 'sat')


def plan_dict(rec):
    """A PLAN_DTYPE record as the dict `ops.Augmenter` takes (data_augment.py `_plan`)."""
    return {k: tuple(rec[k].tolist()) if rec[k].ndim else rec[k].item() for k in PLAN_KEYS}


def plan_records(recs, plans):
    """The reverse: plan dicts into a PLAN_DTYPE array of as many records, one assignment per field (src_off and fill
    are the caller's)."""
    for k in PLAN_KEYS:
        recs[k] = [p[k] for p in plans]
