"""The four-image mosaic on the device: ct_aug_plan_mosaic against its host twin (ctdet/aug_plan_ref.py mosaic_batch)
byte for byte over the table of tests/mosaic_cases.py, the safety rule on foreign tables, ct_preproc_augment_mosaic
against ct_preproc_augment (bit-exact on degenerate tiles) and against the float64 restatement of tests/mosaic_ref.py,
and the path end to end (preproc.mosaic_device, then both matchers)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mosaic_cases as cases
import mosaic_ref
from ctdet import aug_plan_ref as ref
from ctdet import ops
from ctdet._lib import lib, check

pytestmark = pytest.mark.gpu
TAIL = 64                                    # poisoned elements behind every output
DEV = 'cuda'


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(samples, boxes, n_img, max_gt, p, S, margin, truths_cap=None):
    """ct_aug_plan_mosaic through the raw C ABI on poisoned buffers -> dict of host arrays (whole buffers, tails
    included) and the device plans / tiles."""
    n, total = 4 * n_img, len(boxes)
    assert len(samples) == n
    cap = max(total, 1) if truths_cap is None else truths_cap
    s_d = torch.from_numpy(np.ascontiguousarray(samples).view(np.uint8).reshape(-1).copy()).to(DEV)
    b_d = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1).copy()).to(DEV)
    if total == 0:
        b_d = torch.zeros(5, device=DEV)
    plans = torch.full((n * 96 + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
    tiles = torch.full((n * 4 + TAIL,), -7, dtype=torch.int32, device=DEV)
    truths = torch.full((max(cap, 1) + TAIL, 6), float('nan'), device=DEV)
    gt_off = torch.full((n_img + 1 + TAIL,), -1, dtype=torch.int32, device=DEV)
    status = torch.full((4 + TAIL,), -1, dtype=torch.int32, device=DEV)
    ws_bytes = lib().ct_aug_plan_mosaic_workspace_bytes(n_img, max_gt)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
    interp, fill = (C.c_int * 5)(*cases.INTERP), (C.c_float * 3)(*cases.FILL)
    check(lib().ct_aug_plan_mosaic(s_d.data_ptr(), n_img, b_d.data_ptr(), total, max_gt, cases.SEED, p, interp, fill, S,
                                   margin, plans.data_ptr(), tiles.data_ptr(), truths.data_ptr(), cap, gt_off.data_ptr(),
                                   status.data_ptr(), ws.data_ptr(), ws_bytes, _stream()), 'ct_aug_plan_mosaic')
    torch.cuda.synchronize()
    return dict(plans=plans.cpu().numpy(), tiles=tiles.cpu().numpy(), truths=truths.cpu().numpy(),
                gt_off=gt_off.cpu().numpy(), status=status.cpu().numpy(), ws_tail=ws[ws_bytes:].cpu().numpy(), n=n,
                n_img=n_img, plans_d=plans, tiles_d=tiles)


def launch_table(t, p, samples=None, truths_cap=None):
    return launch(t['samples'] if samples is None else samples, t['boxes'], t['n'], t['max_gt'], p, t['S'], t['margin'],
                  truths_cap)


def assert_equals_twin(got, res):
    n, n_img = got['n'], got['n_img']
    assert got['tiles'][:n * 4].tobytes() == res.tiles.tobytes()
    assert got['gt_off'][:n_img + 1].tobytes() == res.gt_off.tobytes()
    assert got['plans'][:n * 96].tobytes() == res.plans.tobytes()
    rows = int(res.gt_off[-1])
    assert rows == len(res.truths)
    assert got['truths'][:rows].tobytes() == res.truths.tobytes()
    assert got['status'][:4].tolist() == res.status.tolist()
    # poison: nothing behind the rows, the plans, the tiles, the offsets, the status words or the workspace was written
    assert np.isnan(got['truths'][rows:]).all()
    assert (got['plans'][n * 96:] == 0xFF).all() and (got['ws_tail'] == 0xFF).all() and (got['tiles'][n * 4:] == -7).all()
    assert (got['gt_off'][n_img + 1:] == -1).all() and (got['status'][4:] == -1).all()


# ------------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize('name', ['M96', 'M8'])
@pytest.mark.parametrize('p', cases.P_VALUES)
def test_table_equals_the_twin_byte_for_byte(name, p):
    t, res = cases.build(name), cases.twin(name, p)
    got = launch_table(t, p)
    assert got['status'][:3].tolist() == [0, 0, 0]
    assert_equals_twin(got, res)
    again = launch_table(t, p)
    for k in ('plans', 'tiles', 'truths', 'gt_off', 'status'):
        assert got[k].tobytes() == again[k].tobytes(), k


def test_shuffled_and_split_gives_the_same_bytes():
    """The images of M96 in another order, in two launches: every image's plans, tiles and rows are the bytes of the
    one-launch result."""
    t, res = cases.build('M96'), cases.twin('M96', 0.6)
    order = np.random.RandomState(11).permutation(t['n'])
    for part in (order[:t['n'] // 3], order[t['n'] // 3:]):
        idx = np.concatenate([np.arange(4 * i, 4 * i + 4) for i in part])
        sub = t['samples'][idx].copy()
        sub['image'] = np.arange(len(idx)) // 4
        got = launch(sub, t['boxes'], len(part), t['max_gt'], 0.6, t['S'], t['margin'])
        assert got['status'][:3].tolist() == [0, 0, 0]
        assert got['plans'][:len(idx) * 96].tobytes() == res.plans[idx].tobytes()
        assert got['tiles'][:len(idx) * 4].tobytes() == res.tiles[idx].tobytes()
        for j, i in enumerate(part):
            a, b = got['gt_off'][j], got['gt_off'][j + 1]
            assert got['truths'][a:b].tobytes() == res.truths[res.gt_off[i]:res.gt_off[i + 1]].tobytes()


def test_more_rows_than_lanes():
    """One group of 4 x 100 boxes: the mapping passes take two strides of the wave and the in-place compaction
    carries across them, with rows dropped in both strides."""
    g = 100
    r = np.random.RandomState(9)
    tgs = []
    for _ in range(4):
        x1, y1 = r.uniform(0, 400, g), r.uniform(0, 300, g)
        tgs.append(np.stack([x1, y1, x1 + r.uniform(6, 90, g), y1 + r.uniform(6, 70, g), r.randint(1, 21, g)],
                            1).astype(np.float32))
    s, b = ref.make_samples([(375, 500)] * 4, tgs, images=[0] * 4, sample_ids=cases.sample_ids([31001]), weights=0.5)
    res = ref.mosaic_batch(s, b, 1, g, cases.SEED, 0.0, cases.INTERP, cases.FILL, 300, 75)
    plain = ref.plan_batch(s, b, 1, g, cases.SEED, 0.0, cases.INTERP, cases.FILL)
    kept, before = [len(x) for x in res.sample_rows], [len(x) for x in plain.sample_rows]
    assert max(kept) > 64 and any(0 < k < n and n > 64 for k, n in zip(kept, before)) and not res.fallback[0]
    assert_equals_twin(launch(s, b, 1, g, 0.0, 300, 75), res)


def test_safety_rule_on_foreign_tables():
    """Tables built to be foreign but harmless: every access stays inside the allocations by the rule itself."""
    t = cases.build('M96')
    s = t['samples'].copy()
    s['image'][6] = 2                               # a valid image, but not this sample's group
    s['image'][13] = -1
    s['image'][30] = 1 << 30
    s['H'][20] = 0
    s['box_end'][47] = len(t['boxes']) + 9          # past total_boxes: clamped, the sample keeps its boxes
    s['box_begin'][40] = -5                         # clamped to 0: the sample looks at the first boxes of the table
    res = ref.mosaic_batch(s, t['boxes'], t['n'], t['max_gt'], cases.SEED, 0.6, cases.INTERP, cases.FILL, t['S'], t['margin'])
    got = launch_table(t, 0.6, samples=s)
    assert_equals_twin(got, res)
    assert got['status'][:2].tolist() == [ops.AUG_STATUS_BAD_SAMPLE, 4]
    plans = got['plans'][:48 * 96].view(ref.PLAN_DTYPE)
    for k in (6, 13, 30, 20):
        H, W = max(int(s['H'][k]), 1), int(s['W'][k])
        assert (plans[k]['H'], plans[k]['W'], tuple(plans[k]['crop']), tuple(plans[k]['exp']), plans[k]['interp'],
                plans[k]['flags']) == (H, W, (0, 0, W, H), (W, H, 0, 0), 0, 0), k
        assert len(res.sample_rows[k]) == 0
    # truths_cap below the row count: the first rows, capped offsets, the status bit, and nothing behind the cap
    rows = int(res.status[3])
    cap = rows - 7
    capped = ref.mosaic_batch(s, t['boxes'], t['n'], t['max_gt'], cases.SEED, 0.6, cases.INTERP, cases.FILL, t['S'],
                              t['margin'], truths_cap=cap)
    got = launch_table(t, 0.6, samples=s, truths_cap=cap)
    assert_equals_twin(got, capped)
    assert got['status'][:4].tolist() == [ops.AUG_STATUS_BAD_SAMPLE | ops.AUG_STATUS_ROWS_DROPPED, 4, 7, rows]
    assert got['truths'][:cap].tobytes() == res.truths[:cap].tobytes() and got['gt_off'][t['n']] == cap


# ------------------------------------------------------------------------------------------------------ the pixels
def _render(aug, plans_d, tiles_d, n, S, means):
    """ct_preproc_augment_mosaic through the raw C ABI on a poisoned output -> float32 [n,3,S,S] (tail checked)."""
    out = torch.full((n * 3 * S * S + TAIL,), float('nan'), device=DEV)
    check(lib().ct_preproc_augment_mosaic(aug.dev.data_ptr(), plans_d.data_ptr(), tiles_d.data_ptr(), n, S,
                                          (C.c_float * 3)(*means), out.data_ptr(), _stream()), 'ct_preproc_augment_mosaic')
    torch.cuda.synchronize()
    assert torch.isnan(out[n * 3 * S * S:]).all()
    return out[:n * 3 * S * S].view(n, 3, S, S)


def _uploaded(t, samples=None):
    """The table's images in an Augmenter's source buffer and its samples pointing at them."""
    aug = ops.Augmenter(t['S'], cases.FILL, DEV, max_batch=len(t['images']), max_pixels=128 * 128)
    offs = aug.upload(t['images'])
    s = (t['samples'] if samples is None else samples).copy()
    s['src_off'] = offs
    return aug, s


def test_degenerate_tiles_equal_the_plain_renderer_bit_for_bit():
    """Slot 0 = the whole square, slots 1..3 of zero width: the bytes of ct_preproc_augment on the same plans.  A strip
    no tile holds gets slot 0's canvas fill."""
    t = cases.build('M96')
    S, n = t['S'], 8
    aug, s = _uploaded(t)
    s = s[:n].copy()
    s['image'] = np.arange(n)
    plain = ops.AugPlanner(DEV, cases.SEED, 0.6, cases.INTERP, cases.FILL)
    plans_d, _ = plain(s, t['boxes'].copy(), n, t['max_gt'])
    assert plain.check()[:3].tolist() == [0, 0, 0]
    assert len(set(plans_d.view(n, 96).cpu().numpy().view(ref.PLAN_DTYPE)['interp'].reshape(-1).tolist())) >= 2
    means = (100.5, 110.25, 120.0)
    want = torch.empty(n, 3, S, S, device=DEV)
    check(lib().ct_preproc_augment(aug.dev.data_ptr(), plans_d.data_ptr(), n, S, (C.c_float * 3)(*means), want.data_ptr(),
                                   _stream()), 'ct_preproc_augment')
    plans4 = plans_d.view(n, 1, 96).expand(n, 4, 96).contiguous().view(-1)
    tiles = torch.tensor([[0, 0, S, S], [S, 0, 0, S], [S, 0, 0, S], [S, 0, 0, S]] * n, dtype=torch.int32, device=DEV)
    got = _render(aug, plans4, tiles, n, S, means)
    assert torch.equal(got, want)
    # an uncovered strip of 6 columns, a tile of negative size and one far outside
    tiles = torch.tensor([[0, 0, S - 6, S], [S - 6, 0, -3, S], [0, 0, S, 0], [5 * S, 5 * S, S, S]] * n, dtype=torch.int32,
                         device=DEV)
    got = _render(aug, plans4, tiles, n, S, means)
    fill = torch.tensor([float(int(f)) - m for f, m in zip(cases.FILL, means)], device=DEV)
    assert torch.equal(got[:, :, :, S - 6:], fill.view(1, 3, 1, 1).expand(n, 3, S, 6))
    assert not torch.equal(got[:, :, :, :S - 6], fill.view(1, 3, 1, 1).expand(n, 3, S, S - 6))


@pytest.mark.parametrize('name', ['M96', 'M8'])
def test_pixels_against_the_float64_restatement(name):
    """The device's own plans and tiles, rendered, against tests/mosaic_ref.py: every pixel within 2 grey levels, and
    on M96 fewer than 5 % of the pixels differ at all (tests/test_gpu_augment.py's rule).  Measured on an MI355X:
    M96 worst 1.0, share 0.00174; M8 worst 1.0, share 0.00195."""
    t = cases.build(name)
    S, n = t['S'], t['n']
    aug, s = _uploaded(t)
    got = launch_table(t, 0.6, samples=s)
    assert got['status'][:3].tolist() == [0, 0, 0]
    plans = got['plans'][:4 * n * 96].view(ref.PLAN_DTYPE)
    tiles = got['tiles'][:16 * n].reshape(4 * n, 4)
    x = _render(aug, got['plans_d'], got['tiles_d'], n, S, cases.FILL).cpu().numpy()
    worst, differing, exact = 0.0, 0, 0
    for i in range(n):
        sl = slice(4 * i, 4 * i + 4)
        want = mosaic_ref.mosaic(t['images'][sl], [ref.plan_dict(pl) for pl in plans[sl]], tiles[sl].tolist(), S, cases.FILL)
        d = np.abs(x[i] - want)
        worst, differing = max(worst, float(d.max())), differing + int((d > 0).sum())
        for k in range(4):
            if int(plans[4 * i + k]['interp']) == 1 and int(plans[4 * i + k]['flags']) == 0:       # pure gather: exact
                x0, y0, w, h = tiles[4 * i + k].tolist()
                assert d[:, y0:y0 + h, x0:x0 + w].max() == 0.0, (i, k)
                exact += 1
    share = differing / x.size
    print('%s: worst deviation %.1f grey levels, share of differing pixels %.5f' % (name, worst, share))
    assert worst <= 2.0
    if name == 'M96':
        assert share < 0.05 and exact >= 1


# ------------------------------------------------------------------------------------------------------ end to end
def test_mosaic_device_end_to_end():
    """preproc(decisions='device').mosaic_device on M96's images: the pixels are render_mosaic of the twin's plans and
    tiles, the packed targets are the twin's, and both matchers take them."""
    from data import VOC_300
    from data.data_augment import preproc
    from layers.functions import PriorBox
    t = cases.build('M96')
    S, n, p = t['S'], t['n'], 0.6
    pre = preproc(S, cases.FILL, p, device=DEV, max_batch=n, filters='fast', decisions='device', seed=cases.SEED)
    x, packed = pre.mosaic_device(t['images'], t['targets'], t['ids'], margin=t['margin'])
    assert pre._planner.check()[:3].tolist() == [0, 0, 0]
    # the twin of that call: no class constraint, the source offsets of the staging buffer
    aug, s = _uploaded(t)
    s['cls'] = -1
    res = ref.mosaic_batch(s, t['boxes'], n, t['max_gt'], cases.SEED, p, cases.INTERP, cases.FILL, S, t['margin'])
    plans_d = torch.from_numpy(res.plans.view(np.uint8).reshape(-1).copy()).to(DEV)
    tiles_d = torch.from_numpy(res.tiles.view(np.uint8).reshape(-1).copy()).to(DEV)
    want = aug.render_mosaic(plans_d, tiles_d, n)
    assert x.shape == (n, 3, S, S) and x.dtype == torch.float32 and torch.equal(x, want)
    rows = int(res.gt_off[-1])
    assert packed.gt_off.cpu().numpy().tobytes() == res.gt_off.tobytes()
    assert packed.truths[:rows].cpu().numpy().tobytes() == res.truths.tobytes()
    assert packed.max_gt >= int(np.diff(res.gt_off).max())
    # default margin: S // 4
    x2, packed2 = pre.mosaic_device(t['images'], t['targets'], t['ids'])
    assert torch.equal(x2, x) and torch.equal(packed2.truths[:rows], packed.truths[:rows])
    pb = PriorBox(VOC_300)
    priors = pb.forward().to(DEV).contiguous()
    has_rows = torch.from_numpy(np.diff(res.gt_off) > 0).to(DEV)
    assert has_rows.all()
    for out in (ops.match_packed(packed.truths, packed.gt_off, n, packed.max_gt, priors, 0.5, (0.1, 0.2)),
                ops.atss_match_packed(packed.truths, packed.gt_off, n, packed.max_gt, priors, pb.level_offsets(), 9,
                                      (0.1, 0.2))):
        loc_t, conf_t = out[0], out[1]
        assert torch.isfinite(loc_t).all() and torch.isfinite(conf_t).all()
        assert ((conf_t[:, :, 0] > 0).any(1) | ~has_rows).all()
