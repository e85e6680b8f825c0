"""ct_aug_plan on the device against its host twin (ctdet/aug_plan_ref.py): byte for byte, over the case table of
tests/aug_plan_cases.py; the safety rule on foreign tables; and the path end to end (pixels, matching)."""
import ctypes as C

import numpy as np
import pytest
import torch

import aug_plan_cases as cases
from ctdet import aug_plan_ref as ref
from ctdet import ops
from ctdet._lib import lib, check

pytestmark = pytest.mark.gpu
TAIL = 64                                    # poisoned elements behind every output


def launch(samples, boxes, n_img, max_gt, p, truths_cap=None):
    """ct_aug_plan through the raw C ABI on poisoned buffers -> dict of host arrays (whole buffers, tails included)."""
    dev = torch.device('cuda')
    n, total = len(samples), len(boxes)
    cap = max(total, 1) if truths_cap is None else truths_cap
    s_d = torch.from_numpy(np.ascontiguousarray(samples).view(np.uint8).reshape(-1).copy()).to(dev)
    b_d = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1).copy()).to(dev)
    if total == 0:
        b_d = torch.zeros(5, device=dev)
    plans = torch.full((n * 96 + TAIL,), 0xFF, dtype=torch.uint8, device=dev)
    truths = torch.full((max(cap, 1) + TAIL, 6), float('nan'), device=dev)
    gt_off = torch.full((n_img + 1 + TAIL,), -1, dtype=torch.int32, device=dev)
    status = torch.full((4 + TAIL,), -1, dtype=torch.int32, device=dev)
    ws_bytes = lib().ct_aug_plan_workspace_bytes(n, max_gt)
    ws = torch.full((ws_bytes + TAIL,), 0xFF, dtype=torch.uint8, device=dev)
    interp, fill = (C.c_int * 5)(*cases.INTERP), (C.c_float * 3)(*cases.FILL)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib().ct_aug_plan(s_d.data_ptr(), n, b_d.data_ptr(), total, n_img, max_gt, cases.SEED, p, interp, fill,
                            plans.data_ptr(), truths.data_ptr(), cap, gt_off.data_ptr(), status.data_ptr(),
                            ws.data_ptr(), ws_bytes, st), 'ct_aug_plan')
    torch.cuda.synchronize()
    return dict(plans=plans.cpu().numpy(), truths=truths.cpu().numpy(), gt_off=gt_off.cpu().numpy(),
                status=status.cpu().numpy(), ws_tail=ws[ws_bytes:].cpu().numpy(), n=n, n_img=n_img)


def assert_equals_twin(got, res):
    n, n_img = got['n'], got['n_img']
    assert got['gt_off'][:n_img + 1].tobytes() == res.gt_off.tobytes()
    assert got['plans'][:n * 96].tobytes() == res.plans.tobytes()
    rows = int(res.gt_off[-1])
    assert rows == len(res.truths)
    assert got['truths'][:rows].tobytes() == res.truths.tobytes()
    assert got['status'][:4].tolist() == res.status.tolist()
    # poison: nothing behind the rows, the plans, the offsets, the status words or the workspace was written
    assert np.isnan(got['truths'][rows:]).all()
    assert (got['plans'][n * 96:] == 0xFF).all() and (got['ws_tail'] == 0xFF).all()
    assert (got['gt_off'][n_img + 1:] == -1).all() and (got['status'][4:] == -1).all()


@pytest.mark.parametrize('p', cases.P_VALUES)
def test_table_equals_the_twin_byte_for_byte(p):
    samples, boxes, n_img, res = cases.twin(p)
    got = launch(samples, boxes, n_img, cases.MAX_GT, p)
    assert got['status'][:3].tolist() == [0, 0, 0]
    assert_equals_twin(got, res)
    again = launch(samples, boxes, n_img, cases.MAX_GT, p)
    for k in ('plans', 'truths', 'gt_off', 'status'):
        assert got[k].tobytes() == again[k].tobytes(), k


def test_shuffled_and_split_gives_the_same_bytes():
    """The images of the table in another order, in two launches: every sample's plan and every image's rows are the
    bytes of the one-launch result."""
    samples, boxes, n_img, res = cases.twin(0.6)
    order = np.random.RandomState(11).permutation(n_img)
    for part in (order[:n_img // 3], order[n_img // 3:]):
        idx = np.concatenate([np.flatnonzero(samples['image'] == img) for img in part])
        sub = samples[idx].copy()
        sub['image'] = np.repeat(np.arange(len(part)), [int((samples['image'] == img).sum()) for img in part])
        got = launch(sub, boxes, len(part), cases.MAX_GT, 0.6)
        assert got['status'][:4].tolist()[:3] == [0, 0, 0]
        plans = got['plans'][:len(idx) * 96].reshape(len(idx), 96)
        for j, i in enumerate(idx):
            assert plans[j].tobytes() == res.plans[i].tobytes()
        for j, img in enumerate(part):
            a, b = got['gt_off'][j], got['gt_off'][j + 1]
            assert got['truths'][a:b].tobytes() == res.truths[res.gt_off[img]:res.gt_off[img + 1]].tobytes()


def test_more_boxes_than_lanes():
    """150 boxes per sample: the row passes take three strides of the wave, the compaction carries across them."""
    g, n = 150, 24
    r = np.random.RandomState(9)
    tgs = []
    for _ in range(n):
        x1, y1 = r.uniform(0, 400, g), r.uniform(0, 300, g)
        tgs.append(np.stack([x1, y1, x1 + r.uniform(2, 90, g), y1 + r.uniform(2, 70, g), r.randint(1, 21, g)],
                            1).astype(np.float32))
    s, b = ref.make_samples([(375, 500)] * n, tgs, images=np.arange(n) // 2, sample_ids=np.arange(n) + 31000,
                            flags=np.arange(n) % 4, weights=0.5)
    res = ref.plan_batch(s, b, n // 2, g, cases.SEED, 0.6, cases.INTERP, cases.FILL)
    assert max(len(x) for x in res.sample_rows) > 64 and any(i is not None and i['cropped'] for i in res.info)
    assert_equals_twin(launch(s, b, n // 2, g, 0.6), res)


def _identity(plan, H, W):
    return (plan['H'], plan['W'], tuple(plan['crop']), tuple(plan['exp']), plan['mirror'], plan['interp'], plan['flags'],
            plan['hue'], plan['beta'], plan['alpha'], plan['sat']) == (H, W, (0, 0, W, H), (W, H, 0, 0), 0, 0, 0, 0, 0.0,
                                                                        1.0, 1.0)


def test_safety_rule_on_foreign_tables():
    """Tables built to be foreign but harmless: every access stays inside the allocations by the rule itself."""
    n_img = 4
    tgs = [cases.B3] * 7
    s, b = ref.make_samples([(375, 500)] * 7, tgs, images=[0, 2, 1, 7, 2, 3, -1], sample_ids=np.arange(7) + 900)
    s['H'][4] = 0                                   # image 2 again, but no height
    s['box_end'][5] = len(b) + 5                    # past total_boxes: clamped, the sample keeps its three boxes
    res = ref.plan_batch(s, b, n_img, cases.MAX_GT, cases.SEED, 0.6, cases.INTERP, cases.FILL)
    got = launch(s, b, n_img, cases.MAX_GT, 0.6)
    assert_equals_twin(got, res)
    assert got['status'][:2].tolist() == [ops.AUG_STATUS_BAD_SAMPLE, 4]
    plans = got['plans'][:7 * 96].view(ref.PLAN_DTYPE)
    for i, (H, W) in ((2, (375, 500)), (3, (375, 500)), (4, (1, 500)), (6, (375, 500))):
        assert _identity(plans[i], H, W), i
        assert len(res.sample_rows[i]) == 0
    assert len(res.sample_rows[5]) > 0 and res.info[5] is not None
    assert got['gt_off'][:n_img + 1].tolist() == np.concatenate(
        [[0], np.cumsum([len(res.sample_rows[0]), 0, len(res.sample_rows[1]), len(res.sample_rows[5])])]).tolist()
    # truths_cap smaller than the rows: the first rows, capped offsets, the status bit, and nothing behind the cap
    rows = int(res.gt_off[-1])
    assert rows >= 3
    cap = rows - 2
    capped = ref.plan_batch(s, b, n_img, cases.MAX_GT, cases.SEED, 0.6, cases.INTERP, cases.FILL, truths_cap=cap)
    got = launch(s, b, n_img, cases.MAX_GT, 0.6, truths_cap=cap)
    assert_equals_twin(got, capped)
    assert got['status'][:4].tolist() == [ops.AUG_STATUS_BAD_SAMPLE | ops.AUG_STATUS_ROWS_DROPPED, 4, 2, rows]
    assert got['truths'][:cap].tobytes() == res.truths[:cap].tobytes() and got['gt_off'][n_img] == cap


def _small_batch():
    r = np.random.RandomState(3)
    images = [r.randint(0, 256, (48, 64, 3)).astype(np.uint8) for _ in range(16)]
    targets = []
    for i in range(16):
        g = 1 + i % 3
        x1, y1 = r.uniform(0, 30, g), r.uniform(0, 20, g)
        targets.append(np.stack([x1, y1, x1 + r.uniform(10, 30, g), y1 + r.uniform(10, 25, g), r.randint(1, 21, g)],
                                1).astype(np.float32))
    return images, targets


def _twin_of_batch(images, targets, ids, seed, p, lam, mix):
    """The twin's samples of preproc.batch_device: image order, first then second where lambda < 1."""
    shapes, tgs, img_of, sid, w, src = [], [], [], [], [], []
    for i in range(len(images)):
        two = mix is not None and lam[i] < 1
        shapes.append(images[i].shape[:2]); tgs.append(targets[i]); img_of.append(i); sid.append(int(ids[i]))
        w.append(np.float32(lam[i]) if two else np.float32(1)); src.append(images[i])
        if two:
            shapes.append(mix[0][i].shape[:2]); tgs.append(mix[1][i]); img_of.append(i)
            sid.append((int(ids[i]) + 2 ** 63) % 2 ** 64); w.append(np.float32(1. - lam[i])); src.append(mix[0][i])
    s, b = ref.make_samples(shapes, tgs, images=img_of, sample_ids=np.array(sid, dtype=np.uint64), weights=w)
    max_gt = max(len(t) for t in tgs)
    return s, src, ref.plan_batch(s, b, len(images), max_gt, seed, p, cases.INTERP, cases.FILL)


@pytest.mark.parametrize('mixed', [False, True])
def test_batch_device_end_to_end(mixed):
    """preproc(decisions='device').batch_device: the pixels are those of ops.Augmenter fed the twin's plans, and
    MultiBoxLoss_combined.match(PackedTargets) assigns what match() assigns on the twin's target list -- bit for bit."""
    from data import VOC_300
    from data.data_augment import preproc
    from layers.functions import PriorBox
    from layers.modules.multibox_loss_combined import MultiBoxLoss_combined
    S, seed, p, n = 32, 4242, 0.6, 8
    images, targets = _small_batch()
    ids = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(2 ** 40)
    lam = [0.3, 1.0, 0.55, 0.7, 1.5, 0.2, 0.9, 0.45] if mixed else [1.0] * n
    mix = (images[n:], targets[n:], lam) if mixed else None
    pre = preproc(S, cases.FILL, p, device='cuda', max_batch=n, filters='fast', decisions='device', seed=seed)
    x, packed = pre.batch_device(images[:n], targets[:n], ids, mix=mix)
    assert pre._planner.check()[:3].tolist() == [0, 0, 0]
    s, src, res = _twin_of_batch(images[:n], targets[:n], ids, seed, p, lam, mix)
    # pixels
    aug = ops.Augmenter(S, cases.FILL, 'cuda', max_batch=2 * n)
    first = [int(np.flatnonzero(s['image'] == i)[0]) for i in range(n)]
    second = [int(np.flatnonzero(s['image'] == i)[-1]) for i in range(n)]
    x1 = aug([src[k] for k in first], [ref.plan_dict(res.plans[k]) for k in first]).clone()
    if mixed:
        x2 = aug([src[k] for k in second], [ref.plan_dict(res.plans[k]) for k in second])
        want = ops.mixup_blend(x1, x2, torch.tensor(lam).clamp(max=1.0).cuda())
    else:
        want = x1
    assert x.shape == (n, 3, S, S) and torch.equal(x, want)
    # packed targets, and the matching on them
    rows = int(res.gt_off[-1])
    assert packed.gt_off.cpu().numpy().tobytes() == res.gt_off.tobytes()
    assert packed.truths[:rows].cpu().numpy().tobytes() == res.truths.tobytes()
    priors = PriorBox(VOC_300).forward().cuda()
    crit = MultiBoxLoss_combined(21, 0.5, True, 0, True, 3, 0.5, False)
    tlist = [torch.from_numpy(res.truths[res.gt_off[i]:res.gt_off[i + 1]].copy()) for i in range(n)]
    assert packed.max_gt >= max(len(t) for t in tlist)
    a, b = crit.match(priors, packed), crit.match(priors, tlist)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert (a.conf_t[:, :, 0] > 0).any()
