"""The four-image mosaic without a device: the host twin's invariants (ctdet/aug_plan_ref.py mosaic_batch) over the
table of tests/mosaic_cases.py, that the table covers what its ids were searched for, the float64 pixel restatement
(tests/mosaic_ref.py) against the oracle, and the C ABI surface (exports, header, bindings, argument errors before any
launch)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mosaic_cases as cases
import mosaic_ref
from ctdet import _lib
from ctdet import aug_plan_ref as ref
from oracle import augment_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, 'context-transformer_amd', 'lib', 'libctdet.so')
CT_ERR_INVALID = 1
NAMES = ('M96', 'M8')


def _plain(t, p):
    """plan_batch over the table's samples: what every sample gets before the composition."""
    return ref.plan_batch(t['samples'], t['boxes'], t['n'], t['max_gt'], cases.SEED, p, cases.INTERP, cases.FILL)


# ------------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('p', cases.P_VALUES)
def test_tiles_partition_the_square_with_sides_of_at_least_margin(name, p):
    t, r = cases.build(name), cases.twin(name, p)
    S, m = t['S'], t['margin']
    assert r.tiles.dtype == ref.TILE_DTYPE and len(r.tiles) == 4 * t['n']
    for i in range(t['n']):
        owner = np.zeros((S, S), dtype=int)
        for k in range(4):
            x0, y0, w, h = (int(v) for v in r.tiles[4 * i + k].tolist())
            assert w >= m and h >= m and x0 >= 0 and y0 >= 0 and x0 + w <= S and y0 + h <= S
            owner[y0:y0 + h, x0:x0 + w] += 1
        assert (owner == 1).all()
        cx, cy = int(r.tiles[4 * i + 3]['x0']), int(r.tiles[4 * i + 3]['y0'])
        assert [tuple(v) for v in r.tiles[4 * i:4 * i + 4].tolist()] == [
            (0, 0, cx, cy), (cx, 0, S - cx, cy), (0, cy, cx, S - cy), (cx, cy, S - cx, S - cy)]
        w = ref.draws(cases.SEED, t['samples'][4 * i]['sample_id'], 0x300, 0)
        assert cx == m + (int(w[0]) * (S - 2 * m + 1) >> 32) and cy == m + (int(w[1]) * (S - 2 * m + 1) >> 32)


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('p', cases.P_VALUES)
def test_plans_and_rows_are_plan_batchs_mapped_filtered_and_packed(name, p):
    """The plans are plan_batch's; the rows are its float32 rows through the affine map into the tile, recomputed here
    in float64, filtered at 0.01 of the output image, all kept when none of an image passes; slot order; gt_off and
    status count them."""
    t, r = cases.build(name), cases.twin(name, p)
    base = _plain(t, p)
    assert r.plans.tobytes() == base.plans.tobytes()
    S = float(t['S'])
    rows, counts = [], []
    for i in range(t['n']):
        mapped, keep = [], []
        for k in range(4):
            s = 4 * i + k
            x0, y0, w, h = (float(v) for v in r.tiles[s].tolist())
            q = base.sample_rows[s]
            o = q.copy()
            for c, (a, b) in enumerate(((x0, w), (y0, h), (x0, w), (y0, h))):
                o[:, c] = (a + q[:, c].astype(np.float64) * b) / S
            X1, Y1, X2, Y2 = [(a + q[:, c].astype(np.float64) * b) / S
                              for c, (a, b) in enumerate(((x0, w), (y0, h), (x0, w), (y0, h)))]
            mapped.append(o)
            keep.append(np.minimum(X2 - X1, Y2 - Y1) > 0.01)
        n_rows, n_kept = sum(len(m) for m in mapped), sum(int(k.sum()) for k in keep)
        fired = n_rows > 0 and n_kept == 0
        assert bool(r.fallback[i]) == fired
        mine = [m if fired else m[k] for m, k in zip(mapped, keep)]
        for k in range(4):
            assert r.sample_rows[4 * i + k].tobytes() == mine[k].tobytes()
        rows += mine
        counts.append(sum(len(m) for m in mine))
        assert counts[-1] > 0 or n_rows == 0            # an image loses its targets only when it had none
    want = np.concatenate(rows, 0)
    assert r.truths.dtype == np.float32 and r.truths.tobytes() == want.tobytes()
    assert r.gt_off.dtype == np.int32 and r.gt_off.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert r.status.tolist() == [0, 0, 0, len(want)]
    assert (want[:, 2] > want[:, 0]).all() and (want[:, :4] >= 0).all() and (want[:, :4] <= 1).all()


def test_the_table_covers_what_it_was_searched_for():
    t, r = cases.build('M96'), cases.twin('M96', 0.6)
    base = _plain(t, 0.6)
    before = [sum(len(base.sample_rows[4 * i + k]) for k in range(4)) for i in range(t['n'])]
    after = np.diff(r.gt_off).tolist()
    i = cases.MIXED_IMAGE
    assert 0 < after[i] < before[i] and not r.fallback[i]           # the filter drops some rows, not all
    i = cases.TINY_IMAGE
    assert r.fallback[i] and after[i] == before[i] > 0              # the fallback fires
    assert len(t['targets'][cases.NO_BOXES]) == 0 and t['samples'][cases.WITH_CLS]['cls'] >= 0
    assert set(int(v) for v in r.plans['interp']) == {0, 1, 2}
    info = [x for x in r.info if x is not None and not x['fallback']]
    assert any(x['mirror'] for x in info) and any(x['cropped'] for x in info) and any(x['expanded'] for x in info)
    assert any(int(pl['interp']) == 1 and int(pl['flags']) == 0 for pl in r.plans[:4])     # exact pixels on the device
    assert min(t['images'][s].shape[0] for s in range(48)) >= 30 and max(t['images'][s].shape[1] for s in range(48)) <= 120
    assert max(len(x) for x in t['targets']) <= 6 and t['S'] == 96 and t['margin'] == 24 and t['n'] == 12
    t8, r8 = cases.build('M8'), cases.twin('M8', 0.6)
    assert t8['S'] == 8 and t8['margin'] == 1 and t8['n'] == 16
    cx, cy = r8.tiles['x0'][3::4], r8.tiles['y0'][3::4]
    assert cx.min() == 1 and cx.max() == 7 and cy.min() == 1 and cy.max() == 7     # both ends of the range
    assert (r8.tiles['w'] == 1).any() and (r8.tiles['h'] == 1).any()
    assert set(int(v) for v in r8.plans['interp']) == {0, 1, 2}


@pytest.mark.parametrize('name', NAMES)
def test_an_image_alone_equals_the_image_inside_the_batch(name):
    t, r = cases.build(name), cases.twin(name, 0.6)
    for i in (0, 3, t['n'] - 2, t['n'] - 1):
        s = t['samples'][4 * i:4 * i + 4].copy()
        s['image'] = 0
        one = ref.mosaic_batch(s, t['boxes'], 1, t['max_gt'], cases.SEED, 0.6, cases.INTERP, cases.FILL, t['S'], t['margin'])
        assert one.plans.tobytes() == r.plans[4 * i:4 * i + 4].tobytes()
        assert one.tiles.tobytes() == r.tiles[4 * i:4 * i + 4].tobytes()
        assert one.truths.tobytes() == r.truths[r.gt_off[i]:r.gt_off[i + 1]].tobytes()


def test_refusal_and_truths_cap_rules():
    t = cases.build('M96')
    s = t['samples'].copy()
    s['image'][6] = 2                               # sample 6 belongs to image 1: refused, though 2 is a valid image
    s['image'][13] = -1
    s['H'][20] = 0
    s['box_end'][47] = len(t['boxes']) + 9          # clamped: the sample keeps its boxes
    full = cases.twin('M96', 0.6)
    r = ref.mosaic_batch(s, t['boxes'], t['n'], t['max_gt'], cases.SEED, 0.6, cases.INTERP, cases.FILL, t['S'], t['margin'])
    assert r.status.tolist()[:3] == [ref.STATUS_BAD_SAMPLE, 3, 0]
    for k, (H, W) in ((6, t['images'][6].shape[:2]), (13, t['images'][13].shape[:2]), (20, (1, t['images'][20].shape[1]))):
        pl = r.plans[k]
        assert (pl['H'], pl['W'], tuple(pl['crop']), tuple(pl['exp']), pl['mirror'], pl['interp'], pl['flags']) == \
            (H, W, (0, 0, W, H), (W, H, 0, 0), 0, 0, 0)
        assert len(r.sample_rows[k]) == 0 and r.info[k] is None
    assert r.tiles.tobytes() == full.tiles.tobytes()        # the tiles do not depend on the refusals
    for i in range(t['n']):                                 # the other images are untouched by their neighbours' refusals
        if i not in (1, 3, 5):
            assert r.truths[r.gt_off[i]:r.gt_off[i + 1]].tobytes() == full.truths[full.gt_off[i]:full.gt_off[i + 1]].tobytes()
            assert r.plans[4 * i:4 * i + 4].tobytes() == full.plans[4 * i:4 * i + 4].tobytes()
    rows = int(full.status[3])
    cap = rows - 5
    c = cases.run_twin(t, 0.6, truths_cap=cap)
    assert c.status.tolist() == [ref.STATUS_ROWS_DROPPED, 0, 5, rows]
    assert c.truths.tobytes() == full.truths[:cap].tobytes() and c.gt_off.tolist() == np.minimum(full.gt_off, cap).tolist()
    with pytest.raises(ValueError):
        ref.mosaic_batch(t['samples'][:7], t['boxes'], 2, 6, 1, 0.5, cases.INTERP, cases.FILL, 96, 24)
    with pytest.raises(ValueError):
        ref.mosaic_batch(t['samples'][:8], t['boxes'], 2, 6, 1, 0.5, cases.INTERP, cases.FILL, 96, 49)


# ------------------------------------------------------------------------------------------------------ pixels
def _mosaic_images(t, r, dtype):
    out = []
    for i in range(t['n']):
        sl = slice(4 * i, 4 * i + 4)
        out.append(mosaic_ref.mosaic(t['images'][sl], [ref.plan_dict(pl) for pl in r.plans[sl]], r.tiles[sl].tolist(),
                                     t['S'], cases.FILL, dtype=dtype))
    return np.stack(out)


def test_mosaic_ref_with_one_whole_tile_is_the_oracle_exactly():
    t, r = cases.build('M96'), cases.twin('M96', 0.6)
    S, seen = 40, set()
    for s in range(24):
        plan = ref.plan_dict(r.plans[s])
        got = mosaic_ref.mosaic([t['images'][s]] * 4, [plan] * 4, [(0, 0, S, S), (S, 0, 0, S), (0, S, S, 0), (S, S, 0, 0)],
                                S, cases.FILL)
        assert got.tobytes() == augment_ref.augment(t['images'][s], plan, S, cases.FILL).tobytes()
        seen.add(plan['interp'])
    assert seen == {0, 1, 2}
    # a strip no tile holds gets the canvas fill
    got = mosaic_ref.mosaic([t['images'][0]] * 4, [ref.plan_dict(r.plans[0])] * 4,
                            [(0, 0, S - 6, S), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)], S, cases.FILL)
    assert (got[:, :, S - 6:] == 0).all()


def test_float32_and_float64_evaluations_differ_in_few_pixels():
    """The share of pixels on which a float32 evaluation of the resize differs from the float64 one stays under the cap
    the device test uses (0.05, tests/test_gpu_augment.py's rule), and never by more than one grey level."""
    t, r = cases.build('M96'), cases.twin('M96', 0.6)
    a, b = _mosaic_images(t, r, np.float64), _mosaic_images(t, r, np.float32)
    d = np.abs(a - b)
    print('float32 vs float64 on M96: share %.5f, worst %.1f' % ((d > 0).mean(), d.max()))
    assert (d > 0).mean() < 0.05 and d.max() <= 1.0


# ------------------------------------------------------------------------------------------------------ C ABI
def test_library_exports_declares_and_binds_the_entry_points():
    assert os.path.exists(LIB), 'build the library first (context-transformer_amd/build.py)'
    out = subprocess.run(['nm', '-D', '--defined-only', LIB], capture_output=True, text=True)
    assert out.returncode == 0
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    lib = _lib.lib()
    for sym, nargs in (('ct_aug_plan_mosaic_workspace_bytes', 2), ('ct_aug_plan_mosaic', 20), ('ct_preproc_augment_mosaic', 8)):
        assert ' T %s\n' % sym in out.stdout, sym
        assert len(_lib.SIGNATURES[sym][1]) == nargs and len(getattr(lib, sym).argtypes) == nargs
        assert sym + '(' in header
    assert 'typedef struct { int x0, y0, w, h; } ct_mosaic_tile;' in header
    assert 'int ct_aug_plan_mosaic(const ct_aug_sample* samples /* dev [4*num_images] */, int num_images,' in header
    assert lib.ct_aug_plan_mosaic_workspace_bytes.restype is C.c_size_t and lib.ct_aug_plan_mosaic.restype is C.c_int
    assert lib.ct_abi_version() == 1
    assert ref.TILE_DTYPE.itemsize == 16 and ref.TILE_DTYPE.names == ('x0', 'y0', 'w', 'h')
    ws = lib.ct_aug_plan_mosaic_workspace_bytes(3, 7)
    assert ws >= lib.ct_aug_plan_workspace_bytes(12, 7) + 12 * 48
    assert lib.ct_aug_plan_mosaic_workspace_bytes(0, 7) == 0 and lib.ct_aug_plan_mosaic_workspace_bytes(3, 0) == 0
    from ctdet import ops
    from data.data_augment import preproc
    assert callable(ops.AugPlanner.mosaic) and callable(ops.Augmenter.render_mosaic) and callable(preproc.mosaic_device)


def _plan_args(**over):
    """A valid argument list of ct_aug_plan_mosaic on host memory (never launched: every case below breaks one rule)."""
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    base = (p.value + 255) // 256 * 256
    a = dict(samples=p, num_images=1, boxes=p, total_boxes=3, max_gt=4, seed=7, p_expand=0.5,
             interp=(C.c_int * 5)(*cases.INTERP), fill=(C.c_float * 3)(*cases.FILL), size=96, margin=24, plans=p, tiles=p,
             truths=p, truths_cap=3, gt_off=p, status=p, workspace=C.c_void_p(base), workspace_bytes=2048, stream=None)
    a.update(over)
    return list(a.values()), buf


@pytest.mark.parametrize('over', [
    dict(samples=None), dict(interp=None), dict(fill=None), dict(plans=None), dict(tiles=None), dict(truths=None),
    dict(gt_off=None), dict(status=None), dict(workspace=None), dict(boxes=None),
    dict(num_images=0), dict(num_images=-3), dict(max_gt=0), dict(size=1), dict(size=0),
    dict(margin=0), dict(margin=49), dict(margin=-1), dict(size=3, margin=2),
    dict(workspace_bytes=64), dict(workspace='misaligned')])
def test_plan_mosaic_refuses_bad_arguments_before_any_launch(over):
    if over.get('workspace') == 'misaligned':
        args, keep = _plan_args()
        args[17] = C.c_void_p(args[17].value + 4)
    else:
        args, keep = _plan_args(**over)
    lib = _lib.lib()
    assert lib.ct_aug_plan_mosaic_workspace_bytes(1, 4) <= 2048 - 4
    assert lib.ct_aug_plan_mosaic(*args) == CT_ERR_INVALID, over
    assert b'ct_aug_plan_mosaic' in lib.ct_last_error_string()


@pytest.mark.parametrize('over', [dict(src=None), dict(plans=None), dict(tiles=None), dict(means=None), dict(out=None),
                                  dict(num_images=0), dict(num_images=-1), dict(size=1), dict(size=0)])
def test_render_mosaic_refuses_bad_arguments_before_any_launch(over):
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    a = dict(src=p, plans=p, tiles=p, num_images=2, size=96, means=p, out=p, stream=None)
    a.update(over)
    lib = _lib.lib()
    assert lib.ct_preproc_augment_mosaic(*a.values()) == CT_ERR_INVALID, over
    assert b'ct_preproc_augment_mosaic' in lib.ct_last_error_string()


def test_mosaic_device_needs_device_decisions():
    from data.data_augment import preproc
    pre = preproc(96, cases.FILL, 0.6, device='cuda', decisions='host')
    with pytest.raises(ValueError, match="decisions='device'"):
        pre.mosaic_device([None] * 4, [None] * 4, [1])
    pre = preproc(96, cases.FILL, 0.6, device='cuda', decisions='device', seed=1)
    with pytest.raises(ValueError, match='4 images per id'):
        pre.mosaic_device([None] * 3, [None] * 3, [1])
    with pytest.raises(ValueError, match='margin'):
        pre.mosaic_device([None] * 4, [None] * 4, [1], margin=49)
