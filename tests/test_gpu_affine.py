"""The random affine stage on the device: ct_aug_affine_plan against its host twin (ctdet/aug_plan_ref.py affine_batch)
byte for byte over the table of tests/affine_cases.py, its independence and safety rule, ct_preproc_warp_affine against
warp_affine bit for bit, and the stage end to end behind preproc.mosaic_device and preproc.batch_device."""
import ctypes as C

import numpy as np
import pytest
import torch

import affine_cases as cases
import mosaic_cases
from ctdet import aug_plan_ref as ref
from ctdet import ops
from ctdet._lib import lib, check

pytestmark = pytest.mark.gpu
TAIL = 64                                    # poisoned elements behind every output
CT_ERR_INVALID = 1                           # include/ctdet.h
DEV = 'cuda'
REC = ref.AFFINE_DTYPE.itemsize


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(truths, gt_off, ids, S, params, truths_rows=None):
    """ct_aug_affine_plan through the raw C ABI on poisoned buffers -> dict of host arrays (whole buffers, tails
    included) and the device records."""
    truths = np.ascontiguousarray(truths, dtype=np.float32).reshape(-1, 6)
    n = len(ids)
    rows = len(truths) if truths_rows is None else truths_rows
    t_d = torch.from_numpy(np.concatenate([truths, np.zeros((1, 6), np.float32)], 0).copy()).to(DEV)
    o_d = torch.from_numpy(np.asarray(gt_off, dtype=np.int32).copy()).to(DEV)
    i_d = torch.from_numpy(np.asarray(ids, dtype=np.uint64).view(np.int64).copy()).to(DEV)
    records = torch.full((n * REC + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((rows + TAIL, 6), float('nan'), device=DEV)
    off = torch.full((n + 1 + TAIL,), -1, dtype=torch.int32, device=DEV)
    status = torch.full((4 + TAIL,), -1, dtype=torch.int32, device=DEV)
    ws_bytes = lib().ct_aug_affine_plan_workspace_bytes(n, rows)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
    prm = params.struct()
    check(lib().ct_aug_affine_plan(t_d.data_ptr(), o_d.data_ptr(), i_d.data_ptr(), n, rows, S, cases.SEED, C.byref(prm),
                                   records.data_ptr(), out.data_ptr(), off.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                   ws_bytes, _stream()), 'ct_aug_affine_plan')
    torch.cuda.synchronize()
    return dict(records=records.cpu().numpy(), truths=out.cpu().numpy(), gt_off=off.cpu().numpy(),
                status=status.cpu().numpy(), ws_tail=ws[ws_bytes:].cpu().numpy(), n=n, records_d=records)


def assert_equals_twin(got, res):
    n = got['n']
    assert got['records'][:n * REC].tobytes() == res.records.tobytes()
    assert got['gt_off'][:n + 1].tobytes() == res.gt_off.tobytes()
    rows = int(res.gt_off[-1])
    assert rows == len(res.truths)
    assert got['truths'][:rows].tobytes() == res.truths.tobytes()
    assert got['status'][:4].tolist() == res.status.tolist()
    # poison: nothing behind the rows, the records, the offsets, the status words or the workspace was written
    assert np.isnan(got['truths'][rows:]).all()
    assert (got['records'][n * REC:] == 0xFF).all() and (got['ws_tail'] == 0xFF).all()
    assert (got['gt_off'][n + 1:] == -1).all() and (got['status'][4:] == -1).all()


# ------------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize('name', ['A96', 'A8'])
@pytest.mark.parametrize('pname', ['P_ALL', 'P_HALF', 'P_NONE'])
def test_table_equals_the_twin_byte_for_byte(name, pname):
    t, res = cases.build(name), cases.twin(name, pname)
    got = launch(t['truths'], t['gt_off'], t['ids'], t['S'], cases.PARAMS[pname])
    assert got['status'][:2].tolist() == [0, 0]
    assert_equals_twin(got, res)
    again = launch(t['truths'], t['gt_off'], t['ids'], t['S'], cases.PARAMS[pname])
    for k in ('records', 'truths', 'gt_off', 'status'):
        assert got[k].tobytes() == again[k].tobytes(), k


def test_shuffled_and_split_gives_the_same_bytes():
    """The images of A96 in another order, in two launches: every image's record and rows are the bytes of the
    one-launch result."""
    t, res = cases.build('A96'), cases.twin('A96', 'P_ALL')
    order = np.random.RandomState(11).permutation(t['n'])
    for part in (order[:t['n'] // 3], order[t['n'] // 3:]):
        rows = [t['truths'][t['gt_off'][i]:t['gt_off'][i + 1]] for i in part]
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        got = launch(np.concatenate(rows, 0), off, [t['ids'][i] for i in part], t['S'], cases.P_ALL)
        assert got['status'][:2].tolist() == [0, 0]
        assert got['records'][:len(part) * REC].tobytes() == res.records[part].tobytes()
        for j, i in enumerate(part):
            a, b = got['gt_off'][j], got['gt_off'][j + 1]
            assert got['truths'][a:b].tobytes() == res.image_rows[i].tobytes()


def test_more_rows_than_lanes():
    """One image of 150 rows between two small ones: the mapping takes three strides of the wave and the compaction
    carries across them, with rows dropped in more than one stride."""
    r = np.random.RandomState(5)
    g = 150
    kind = r.randint(0, 3, g)               # 0 large, 1 tiny, 2 crossing an edge
    w = np.where(kind == 1, r.uniform(0.002, 0.006, g), r.uniform(0.1, 0.4, g))
    h = np.where(kind == 1, r.uniform(0.002, 0.006, g), r.uniform(0.1, 0.4, g))
    x1 = np.where(kind == 2, r.uniform(0.8, 0.98, g), r.uniform(0.05, 0.55, g))
    y1 = r.uniform(0.05, 0.55, g)
    big = np.stack([x1, y1, np.minimum(x1 + w, 1.0), y1 + h, r.randint(1, 21, g), r.uniform(0.2, 1.0, g)], 1).astype(np.float32)
    small = np.array([[0.2, 0.2, 0.7, 0.8, 3, 1.0]], dtype=np.float32)
    truths, off, ids = np.concatenate([small, big, small], 0), [0, 1, 1 + g, 2 + g], [41000, 41001, 41002]
    res = ref.affine_batch(truths, off, ids, 300, cases.SEED, cases.P_ALL)
    kept = np.zeros(g, dtype=bool)
    _, keep = ref.affine_rows(big, res.records[1]['fwd'], 300, cases.P_ALL.min_side, cases.P_ALL.min_visible)
    kept[:] = keep
    dropped_in = [int((~kept[s:s + 64]).sum()) for s in (0, 64, 128)]
    assert res.records[1]['flags'] == 1 and len(res.image_rows[1]) > 64 and sum(d > 0 for d in dropped_in) >= 2
    assert_equals_twin(launch(truths, off, ids, 300, cases.P_ALL), res)


def test_safety_rule_on_a_foreign_offset_table():
    """An offset table built to be foreign but harmless: every access stays inside the allocations by the rule itself."""
    t = cases.build('A96')
    rows = len(t['truths'])
    off = t['gt_off'].astype(np.int64).copy()
    off[2] = -4                     # negative: image 1 ends below its begin, image 2 begins below image 0's end
    off[6] = off[5] - 3             # a decreasing pair
    off[12] = rows + 50             # beyond truths_rows: clamped
    for pname in ('P_ALL', 'P_NONE'):
        res = ref.affine_batch(t['truths'], off, t['ids'], t['S'], cases.SEED, cases.PARAMS[pname])
        got = launch(t['truths'], off, t['ids'], t['S'], cases.PARAMS[pname])
        assert_equals_twin(got, res)
        assert got['status'][:2].tolist() == [ref.STATUS_BAD_IMAGE, 4]
        recs = got['records'][:t['n'] * REC].view(ref.AFFINE_DTYPE)
        for i in (1, 2, 5, 6):
            assert recs[i]['flags'] == 4 and got['gt_off'][i] == got['gt_off'][i + 1]
    # a capacity below the table's rows
    res = ref.affine_batch(t['truths'], t['gt_off'], t['ids'], t['S'], cases.SEED, cases.P_ALL, truths_rows=20)
    assert_equals_twin(launch(t['truths'], t['gt_off'], t['ids'], t['S'], cases.P_ALL, truths_rows=20), res)


def test_invalid_arguments_are_refused_before_any_device_work():
    t = cases.build('A8')
    n, rows = t['n'], len(t['truths'])
    buf = torch.zeros(4096, dtype=torch.float32, device=DEV)
    p = buf.data_ptr()
    ws_bytes = lib().ct_aug_affine_plan_workspace_bytes(n, rows)
    assert lib().ct_aug_affine_plan_workspace_bytes(0, rows) == 0 and lib().ct_aug_affine_plan_workspace_bytes(n, -1) == 0
    ws = torch.zeros(ws_bytes + 64, dtype=torch.uint8, device=DEV)

    def call(prm=cases.P_ALL.struct(), n=n, rows=rows, S=8, tin=p, tout=p + 8192, ws_ptr=ws.data_ptr(), ws_bytes=ws_bytes,
             ids=p + 4096):
        return lib().ct_aug_affine_plan(tin, p + 2048, ids, n, rows, S, 1, C.byref(prm), p + 12288, tout, p + 3072,
                                        p + 3584, ws_ptr, ws_bytes, _stream())

    def with_field(name, v):
        s = cases.P_ALL.struct()
        setattr(s, name, v)
        return s

    assert call(n=0) == CT_ERR_INVALID and call(S=1) == CT_ERR_INVALID and call(rows=-1) == CT_ERR_INVALID
    assert call(tin=None) == CT_ERR_INVALID and call(ids=None) == CT_ERR_INVALID and call(ws_ptr=None) == CT_ERR_INVALID
    assert call(tout=p + 8) == CT_ERR_INVALID                                   # the row buffers overlap
    assert call(ws_bytes=ws_bytes - 1) == CT_ERR_INVALID and call(ws_ptr=ws.data_ptr() + 4) == CT_ERR_INVALID
    for name, bad in (('rot_half_tan', (-0.1, 1.5, float('nan'))), ('scale_lo', (0.0, 2.0)), ('scale_hi', (4.5, float('inf'))),
                      ('shear_tan', (-0.1, 0.6)), ('translate', (-0.1, 0.6)), ('p', (-0.1, 1.1)),
                      ('min_side', (-0.1, float('nan'))), ('min_visible', (-0.1, 1.5))):
        for v in bad:
            assert call(prm=with_field(name, v)) == CT_ERR_INVALID, (name, v)
    torch.cuda.synchronize()
    assert not buf.any()                                                        # nothing was launched


# ------------------------------------------------------------------------------------------------------ the pixels
def _warp(x_d, records_d, n, S, border=cases.BORDER):
    """ct_preproc_warp_affine through the raw C ABI on a poisoned output -> float32 [n,3,S,S] (tail checked)."""
    out = torch.full((n * 3 * S * S + TAIL,), float('nan'), device=DEV)
    check(lib().ct_preproc_warp_affine(x_d.data_ptr(), records_d.data_ptr(), n, S, (C.c_float * 3)(*border), out.data_ptr(),
                                       _stream()), 'ct_preproc_warp_affine')
    torch.cuda.synchronize()
    assert torch.isnan(out[n * 3 * S * S:]).all()
    return out[:n * 3 * S * S].view(n, 3, S, S)


def _records_d(recs):
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy()).to(DEV)


@pytest.mark.parametrize('name', ['A96', 'A8'])
def test_pixels_equal_the_twin_bit_for_bit(name):
    t, x = cases.build(name), cases.pixels(name)
    n, S = t['n'], t['S']
    x_d = torch.from_numpy(x.copy()).to(DEV)
    border = torch.tensor(cases.BORDER, device=DEV).view(1, 3, 1, 1)
    for pname in ('P_ALL', 'P_HALF'):
        got = launch(t['truths'], t['gt_off'], t['ids'], S, cases.PARAMS[pname])
        recs = got['records'][:n * REC].view(ref.AFFINE_DTYPE)
        assert recs.tobytes() == cases.twin(name, pname).records.tobytes()
        y = _warp(x_d, got['records_d'], n, S)
        assert torch.equal(y.cpu(), torch.from_numpy(ref.warp_affine(x, recs, cases.BORDER)))
        assert not torch.equal(y, x_d) and (y == border).all(1).any()
    # the identity: flag 4 (the copy) and flags 0 (the general path) both return the input bit for bit
    for flags in (4, 0):
        y = _warp(x_d, _records_d(np.array([ref.affine_identity(flags)] * n)), n, S)
        assert torch.equal(y, x_d), flags
    # a record table of NaN, infinities and huge entries: border everywhere
    bad = np.array([ref.affine_identity(0)] * n)
    for i, v in enumerate((np.nan, np.inf, -np.inf, 1e300, -1e300)):
        bad[i]['inv'][:] = v
    bad[5]['inv'][:] = (1, 0, np.nan, 0, 1, 0)
    bad[6]['inv'][:] = (np.inf, -np.inf, 0, 1e300, -1e300, np.nan)
    bad[7]['inv'][:] = (1, 0, 1e300, 0, 1, -1e300)
    y = _warp(x_d[:8], _records_d(bad[:8]), 8, S)
    assert torch.equal(y, border.expand(8, 3, S, S))


@pytest.mark.parametrize('S,n', [(6, 3), (7, 2)])
def test_copy_of_planes_that_are_no_multiple_of_16_bytes(S, n):
    """3*S*S floats per image with S = 7 leaves images 1.. off the 16-byte grid: the flag-4 copy takes a scalar head
    and tail there; a misaligned base pointer takes the scalar copy throughout."""
    x = torch.arange(1 + n * 3 * S * S + TAIL, dtype=torch.float32, device=DEV)
    recs = _records_d(np.array([ref.affine_identity()] * n))
    for shift in (0, 1):
        x_d = x[shift:shift + n * 3 * S * S]
        out = torch.full((1 + n * 3 * S * S + TAIL,), float('nan'), device=DEV)
        o_d = out[shift:]
        check(lib().ct_preproc_warp_affine(x_d.data_ptr(), recs.data_ptr(), n, S, (C.c_float * 3)(*cases.BORDER),
                                           o_d.data_ptr(), _stream()), 'ct_preproc_warp_affine')
        assert torch.equal(o_d[:n * 3 * S * S], x_d) and torch.isnan(o_d[n * 3 * S * S:]).all() and torch.isnan(out[:shift]).all()


def test_overlapping_buffers_are_refused():
    S, n = 8, 2
    x = torch.zeros(2 * n * 3 * S * S, device=DEV)
    recs = _records_d(np.array([ref.affine_identity()] * n))
    border = (C.c_float * 3)(*cases.BORDER)
    for shift in (0, 4, n * 3 * S * S * 4 - 4):
        assert lib().ct_preproc_warp_affine(x.data_ptr(), recs.data_ptr(), n, S, border, x.data_ptr() + shift,
                                            _stream()) == CT_ERR_INVALID
        assert lib().ct_preproc_warp_affine(x.data_ptr() + shift, recs.data_ptr(), n, S, border, x.data_ptr(),
                                            _stream()) == CT_ERR_INVALID
    assert lib().ct_preproc_warp_affine(x.data_ptr(), recs.data_ptr(), n, S, border, x.data_ptr() + n * 3 * S * S * 4,
                                        _stream()) == 0
    assert lib().ct_preproc_warp_affine(x.data_ptr(), recs.data_ptr(), 0, S, border, x.data_ptr() + n * 3 * S * S * 4,
                                        _stream()) == CT_ERR_INVALID
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ end to end
def _check_stage(pre, plain, ids, x, packed, x0, packed0, n, S):
    """(x, packed) of a call with affine=P_ALL against (x0, packed0) of the same call with affine=None."""
    assert pre._affine.check()[:2].tolist() == [0, 0]
    rows0 = int(packed0.gt_off[-1])
    res = ref.affine_batch(packed0.truths[:rows0].cpu().numpy(), packed0.gt_off.cpu().numpy(), ids, S, cases.SEED, cases.P_ALL)
    border = [float(np.float32(int(m)) - np.float32(m)) for m in mosaic_cases.FILL]
    assert x.shape == (n, 3, S, S) and x.dtype == torch.float32
    assert torch.equal(x.cpu(), torch.from_numpy(ref.warp_affine(x0.cpu().numpy(), res.records, border)))
    rows = int(res.gt_off[-1])
    assert packed.gt_off.cpu().numpy().tobytes() == res.gt_off.tobytes()
    assert packed.truths[:rows].cpu().numpy().tobytes() == res.truths.tobytes()
    assert packed.max_gt >= int(np.diff(res.gt_off).max()) and (res.records['flags'] == 1).any() and not torch.equal(x, x0)
    return res


def _check_matchers(packed, res, n):
    from data import VOC_300
    from layers.functions import PriorBox
    pb = PriorBox(VOC_300)
    priors = pb.forward().to(DEV).contiguous()
    has_rows = torch.from_numpy(np.diff(res.gt_off) > 0).to(DEV)
    assert has_rows.any()
    for out in (ops.match_packed(packed.truths, packed.gt_off, n, packed.max_gt, priors, 0.5, (0.1, 0.2)),
                ops.atss_match_packed(packed.truths, packed.gt_off, n, packed.max_gt, priors, pb.level_offsets(), 9,
                                      (0.1, 0.2))):
        loc_t, conf_t = out[0], out[1]
        assert torch.isfinite(loc_t).all() and torch.isfinite(conf_t).all()
        assert ((conf_t[:, :, 0] > 0).any(1) | ~has_rows).all()


def test_mosaic_device_end_to_end():
    from data.data_augment import preproc
    t = mosaic_cases.build('M96')
    S, n, p = t['S'], t['n'], 0.6
    kw = dict(device=DEV, max_batch=n, filters='fast', decisions='device', seed=cases.SEED)
    plain, pre = preproc(S, mosaic_cases.FILL, p, **kw), preproc(S, mosaic_cases.FILL, p, affine=cases.P_ALL, **kw)
    x0, packed0 = plain.mosaic_device(t['images'], t['targets'], t['ids'], margin=t['margin'])
    x, packed = pre.mosaic_device(t['images'], t['targets'], t['ids'], margin=t['margin'])
    # affine=None is today's path: the rows of the mosaic twin for that call (no class constraint);
    # test_gpu_mosaic.py holds its pixels to the renderer
    s = t['samples'].copy()
    s['cls'] = -1
    res0 = ref.mosaic_batch(s, t['boxes'], n, t['max_gt'], cases.SEED, p, mosaic_cases.INTERP, mosaic_cases.FILL, S,
                            t['margin'])
    assert packed0.gt_off.cpu().numpy().tobytes() == res0.gt_off.tobytes() and plain._affine is None
    assert packed0.truths[:len(res0.truths)].cpu().numpy().tobytes() == res0.truths.tobytes()
    res = _check_stage(pre, plain, t['ids'], x, packed, x0, packed0, n, S)
    assert res.fallback.any() and (np.diff(res.gt_off) < np.diff(res0.gt_off)).any()
    _check_matchers(packed, res, n)


def test_batch_device_with_a_mixup_pair_end_to_end():
    from data.data_augment import preproc
    t = mosaic_cases.build('M96')
    S, n, p = t['S'], 8, 0.6
    first = [i for i in range(4 * t['n']) if len(t['targets'][i])][:n]       # every first sample has boxes
    second = list(range(first[-1] + 1, first[-1] + 1 + n))
    imgs, tgs = [t['images'][i] for i in first], [t['targets'][i] for i in first]
    mix = ([t['images'][i] for i in second], [t['targets'][i] for i in second], [0.3, 1.0, 0.65, 0.5, 1.0, 0.8, 0.25, 0.9])
    ids = [9100 + 7 * i for i in range(n)]
    kw = dict(device=DEV, max_batch=n, filters='fast', decisions='device', seed=cases.SEED)
    plain, pre = preproc(S, mosaic_cases.FILL, p, **kw), preproc(S, mosaic_cases.FILL, p, affine=cases.P_ALL, **kw)
    for m in (mix, None):
        x0, packed0 = plain.batch_device(imgs, tgs, ids, mix=m)
        x, packed = pre.batch_device(imgs, tgs, ids, mix=m)
        res = _check_stage(pre, plain, ids, x, packed, x0, packed0, n, S)
        # affine=None is today's path: a second preproc without the argument gives the same bytes
        x1, packed1 = preproc(S, mosaic_cases.FILL, p, **kw).batch_device(imgs, tgs, ids, mix=m)
        assert torch.equal(x1, x0) and torch.equal(packed1.gt_off, packed0.gt_off)
        assert torch.equal(packed1.truths[:int(packed0.gt_off[-1])], packed0.truths[:int(packed0.gt_off[-1])])
    _check_matchers(packed, res, n)
