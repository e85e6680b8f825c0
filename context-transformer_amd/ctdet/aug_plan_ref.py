"""Host twin of csrc/ct_aug_plan.hip (`ct_aug_plan`): the augmentation DECISIONS and the box targets of
data/data_augment.py `preproc.decide`, drawn from a counter-based generator instead of `random`.

numpy, fp64, no device, no `random`.  The draw table below is the one include/ctdet.h documents; the device kernel
evaluates the same expressions in the same order with contraction off, so both give the same bytes.

Generator: Philox4x32-10, key = (seed lo, seed hi), counter = (sample_id lo, sample_id hi, slot, lane); one
evaluation gives four 32-bit words w0..w3.  uniform(a, b) = a + (b - a) * (w * 2^-32), randrange(n) = (w * n) >> 32,
coin = w >> 31.

    slot           lane     w0                 w1                w2                  w3
    0 (misc)       0        brightness coin    contrast coin     hue coin            saturation coin
    0              1        beta U(-32,32)     alpha U(.5,1.5)   hue -18+rr(37)      sat U(.5,1.5)
    0              2        expand u (> p: no) mirror coin       interp rr(5)        fallback interp rr(5)
    0x100 + r      63       crop mode rr(7)
    0x100 + r      0..49    scale U(.3,1)      ratio u           left rr(W - w)      top rr(H - h)
    0x200 + r      0..63    scale U(1,4)       ratio u           left rr(w - cw + 1) top rr(h - ch + 1)
    0x300 (mosaic) 0        cx margin+rr(S-2m+1) cy likewise     (of a group's first sample; `mosaic_batch` below)
    0x400 (affine) 0        t U(-rot,rot)      s U(lo,hi)        kx U(-shear,shear)  ky likewise   (`affine_batch` below)
    0x400          1        tx U(.5-tr,.5+tr)*S ty likewise      gate u (> p: no)

Crop rounds r = 0..255, expand rounds r = 0..63; the lowest passing lane of the first round with one wins.
"""
import collections
import math

import numpy as np

from .aug_records import (AFFINE_DTYPE, PLAN_DTYPE, SAMPLE_DTYPE, TILE_DTYPE, AffineParamsRecord,     # noqa: F401
                          plan_dict, plan_records)

PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)

SLOT_MISC, SLOT_CROP, SLOT_EXPAND = 0, 0x100, 0x200
LANE_COINS, LANE_PARAMS, LANE_MISC, LANE_MODE = 0, 1, 2, 63
CROP_TRIALS, CROP_ROUNDS, EXPAND_TRIALS, EXPAND_ROUNDS = 50, 256, 64, 64
CROP_MIN_IOU = (None, 0.1, 0.3, 0.5, 0.7, 0.9, -np.inf)     # data_augment.py CROP_MODES; every upper bound is None
STATUS_BAD_SAMPLE, STATUS_ROWS_DROPPED = 1, 2

AugPlanResult = collections.namedtuple(
    'AugPlanResult', 'plans truths gt_off status crop_rounds expand_rounds sample_rows info')


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10.  Counter words: scalars or arrays (broadcast); key words: scalars.  -> uint32 [..., 4]."""
    c = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & _MASK for v in (c0, c1, c2, c3)])
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    m0, m1 = np.uint64(PHILOX_M[0]), np.uint64(PHILOX_M[1])
    for _ in range(10):
        p0, p1 = c[0] * m0, c[2] * m1
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & _MASK]
        k0, k1 = (k0 + PHILOX_W[0]) & 0xFFFFFFFF, (k1 + PHILOX_W[1]) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def draws(seed, sample_id, slot, lanes):
    """The four words of every lane in `lanes` at (seed, sample_id, slot)."""
    seed, sample_id = int(seed) & (2 ** 64 - 1), int(sample_id) & (2 ** 64 - 1)
    return philox4x32(sample_id & 0xFFFFFFFF, sample_id >> 32, slot, lanes, seed & 0xFFFFFFFF, seed >> 32)


def unit(w):
    return np.asarray(w, dtype=np.float64) * 2.0 ** -32


def uniform(a, b, w):
    return a + (b - a) * unit(w)


def randrange(n, w):
    return ((np.asarray(w, dtype=np.uint64) * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def _crop_trials(d, H, W, b, labels, min_iou, cls):
    """The 50 trials of one crop round: d uint32 [50,4], b float64 [n,4]  ->  ok [50], (l, t, w, h) int64 [50]."""
    scale = uniform(0.3, 1.0, d[:, 0])
    lo, hi = np.maximum(0.5, scale * scale), np.minimum(2.0, 1.0 / scale / scale)
    ratio = np.sqrt(lo + (hi - lo) * unit(d[:, 1]))
    w, h = (scale * ratio * W).astype(np.int64), (scale / ratio * H).astype(np.int64)
    ok = (w >= 1) & (h >= 1) & (w < W) & (h < H)
    l = randrange(np.where(ok, W - w, 1), d[:, 2])
    t = randrange(np.where(ok, H - h, 1), d[:, 3])
    rl, rt, rr, rb = [v.astype(np.float64)[None, :] for v in (l, t, l + w, t + h)]
    x1, y1, x2, y2 = [b[:, k, None] for k in range(4)]
    ltx, lty, rbx, rby = np.maximum(x1, rl), np.maximum(y1, rt), np.minimum(x2, rr), np.minimum(y2, rb)
    area_i = (rbx - ltx) * (rby - lty) * ((ltx < rbx) & (lty < rby))
    area_a, area_b = (x2 - x1) * (y2 - y1), (rr - rl) * (rb - rt)
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = area_i / (area_a + area_b - area_i)
    ok &= (min_iou <= iou.min(0)) & (iou.max(0) <= np.inf)
    cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
    inside = (rl < cx) & (cx < rr) & (rt < cy) & (cy < rb)
    ok &= inside.any(0)
    if cls >= 0:
        ok &= (inside & (labels[:, None] == float(cls + 1))).any(0)
    return ok, l, t, w, h


def _expand_trials(d, cw, ch):
    scale = uniform(1.0, 4.0, d[:, 0])
    lo, hi = np.maximum(0.5, 1.0 / scale / scale), np.minimum(2.0, scale * scale)
    ratio = np.sqrt(lo + (hi - lo) * unit(d[:, 1]))
    ws, hs = scale * ratio, scale / ratio
    ok = ~((ws < 1) | (hs < 1))
    w, h = (ws * cw).astype(np.int64), (hs * ch).astype(np.int64)
    left = randrange(np.where(ok, w - cw + 1, 1), d[:, 2])
    top = randrange(np.where(ok, h - ch + 1, 1), d[:, 3])
    return ok, w, h, left, top


def plan_sample(seed, sample_id, H, W, boxes, cls, p, interp_of_draw):
    """One sample's decisions.  boxes float32 [n,5] pixel (x1,y1,x2,y2,label), cls -1 or the class constraint, p the
    expand probability (a float32 value, like the C ABI's)  ->  dict(plan fields, rows float64 [k,5], rounds, ...)."""
    H, W, cls = int(H), int(W), int(cls)
    bl = np.asarray(boxes, dtype=np.float32).reshape(-1, 5).astype(np.float64)
    b, labels, n = bl[:, :4], bl[:, 4], len(bl)
    misc = draws(seed, sample_id, SLOT_MISC, np.arange(3))
    out = dict(H=H, W=W, crop=(0, 0, W, H), exp=(W, H, 0, 0), mirror=0, interp=0, flags=0, hue=0, beta=0.0, alpha=1.0,
               sat=1.0, crop_rounds=0, expand_rounds=0, crop_mode=0, crop_lane=-1, expand_lane=-1, cropped=False,
               expanded=False, fallback=False)
    # crop
    l, t, w, h, cropped = 0, 0, W, H, False
    if n > 0:
        for r in range(CROP_ROUNDS):
            d = draws(seed, sample_id, SLOT_CROP + r, np.arange(64))
            out['crop_rounds'] = r + 1
            mode = int(randrange(7, d[LANE_MODE, 0]))
            out['crop_mode'] = mode
            if mode == 0:
                break
            ok, tl, tt, tw, th = _crop_trials(d[:CROP_TRIALS], H, W, b, labels, CROP_MIN_IOU[mode], cls)
            idx = np.flatnonzero(ok)
            if len(idx):
                k = int(idx[0])
                l, t, w, h, cropped = int(tl[k]), int(tt[k]), int(tw[k]), int(th[k]), True
                out['crop_lane'] = k
                break
    out['cropped'] = cropped
    # distort
    coins, prm = misc[LANE_COINS] >> 31, misc[LANE_PARAMS]
    flags, beta, alpha, hue, sat = 0, 0.0, 1.0, 0, 1.0
    if coins[0]:
        flags, beta = flags | 1, float(uniform(-32.0, 32.0, prm[0]))
    if coins[1]:
        flags, alpha = flags | 2, float(uniform(0.5, 1.5, prm[1]))
    if coins[2]:
        flags, hue = flags | 4, -18 + int(randrange(37, prm[2]))
    if coins[3]:
        flags, sat = flags | 8, float(uniform(0.5, 1.5, prm[3]))
    # expand
    ew, eh, left, top, expanded = w, h, 0, 0, False
    if not (float(unit(misc[LANE_MISC, 0])) > p):
        for r in range(EXPAND_ROUNDS):
            d = draws(seed, sample_id, SLOT_EXPAND + r, np.arange(EXPAND_TRIALS))
            out['expand_rounds'] = r + 1
            ok, xw, xh, xl, xt = _expand_trials(d, w, h)
            idx = np.flatnonzero(ok)
            if len(idx):
                k = int(idx[0])
                ew, eh, left, top, expanded = int(xw[k]), int(xh[k]), int(xl[k]), int(xt[k]), True
                out['expand_lane'] = k
                break
    out['expanded'] = expanded
    mirror = int(misc[LANE_MISC, 1] >> 31)
    # targets
    x1, y1, x2, y2 = [b[:, k].copy() for k in range(4)]
    keep = np.ones(n, dtype=bool)
    if cropped:
        cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
        keep = (l < cx) & (cx < l + w) & (t < cy) & (cy < t + h)
        x1, y1 = np.maximum(x1, float(l)) - l, np.maximum(y1, float(t)) - t
        x2, y2 = np.minimum(x2, float(l + w)) - l, np.minimum(y2, float(t + h)) - t
    if expanded:
        x1, y1, x2, y2 = x1 + left, y1 + top, x2 + left, y2 + top
    if mirror:
        x1, x2 = ew - x2, ew - x1
    x1, y1, x2, y2 = x1 / ew, y1 / eh, x2 / ew, y2 / eh
    keep = keep & (np.minimum(x2 - x1, y2 - y1) > 0.01)
    if not keep.any() or (cls >= 0 and not (labels[keep] == float(cls + 1)).any()):
        out.update(fallback=True, interp=int(interp_of_draw[int(randrange(5, misc[LANE_MISC, 3]))]),
                   rows=np.stack([b[:, 0] / W, b[:, 1] / H, b[:, 2] / W, b[:, 3] / H, labels], 1))
        return out
    out.update(crop=(l, t, w, h), exp=(ew, eh, left, top), mirror=mirror, flags=flags, beta=beta, alpha=alpha, hue=hue,
               sat=sat, interp=int(interp_of_draw[int(randrange(5, misc[LANE_MISC, 2]))]),
               rows=np.stack([x1, y1, x2, y2, labels], 1)[keep])
    return out


def _identity(plan, H, W):
    plan['H'], plan['W'], plan['crop'], plan['exp'] = H, W, (0, 0, W, H), (W, H, 0, 0)
    plan['mirror'] = plan['interp'] = plan['flags'] = plan['hue'] = 0
    plan['beta'], plan['alpha'], plan['sat'] = 0.0, 1.0, 1.0


def plan_batch(samples, boxes, num_images, max_gt, seed, p_expand, interp_of_draw, fill, truths_cap=None):
    """What `ct_aug_plan` computes, safety rule included.  samples: SAMPLE_DTYPE array; boxes float32 [total,5].
    -> AugPlanResult: plans (PLAN_DTYPE), truths float32 [min(rows, truths_cap), 6], gt_off int32 [num_images+1],
    status int32 [4] = (bits, bad samples, dropped rows, rows before the cap), the crop / expand rounds each sample
    used, each sample's rows, and plan_sample's dicts (None for a refused sample)."""
    samples = np.asarray(samples, dtype=SAMPLE_DTYPE)
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 5)
    total, n = len(boxes), len(samples)
    p = float(np.float32(p_expand))
    plans = np.zeros(n, dtype=PLAN_DTYPE)
    plans['fill'] = np.asarray(fill, dtype=np.float32)
    crop_rounds, expand_rounds = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    rows_of, image_of, info = [], [], []
    prevmax, bad = -1, 0
    for i, s in enumerate(samples):
        H, W, img = int(s['H']), int(s['W']), int(s['image'])
        plans[i]['src_off'] = s['src_off']
        inrange = 0 <= img < num_images
        refused = not inrange or H < 1 or W < 1 or img < prevmax
        if inrange:
            prevmax = max(prevmax, img)
        if refused:
            _identity(plans[i], max(H, 1), max(W, 1))
            bad += 1
            rows_of.append(np.zeros((0, 6), dtype=np.float32))
            image_of.append(-1)
            info.append(None)
            continue
        b0, b1 = min(max(int(s['box_begin']), 0), total), min(max(int(s['box_end']), 0), total)
        cnt = min(max(b1 - b0, 0), int(max_gt))
        r = plan_sample(seed, s['sample_id'], H, W, boxes[b0:b0 + cnt], s['cls'], p, interp_of_draw)
        plan_records(plans[i:i + 1], [r])
        crop_rounds[i], expand_rounds[i] = r['crop_rounds'], r['expand_rounds']
        rows = np.zeros((len(r['rows']), 6), dtype=np.float64)
        rows[:, :5] = r['rows']
        flags = int(s['flags'])
        if flags & 2:
            rows[1:, 4] = -1
        rows[:, 5] = float(s['weight'])
        if flags & 1:
            rows[rows[:, 4] == -1, 5] = 0
        rows_of.append(rows.astype(np.float32))
        image_of.append(img)
        info.append(r)
    counts = np.zeros(num_images, dtype=np.int64)
    for img, rows in zip(image_of, rows_of):
        if img >= 0:
            counts[img] += len(rows)
    all_rows = np.concatenate(rows_of, 0) if rows_of else np.zeros((0, 6), dtype=np.float32)
    n_rows = len(all_rows)
    cap = n_rows if truths_cap is None else int(truths_cap)
    gt_off = np.minimum(np.concatenate([[0], np.cumsum(counts)]), cap).astype(np.int32)
    dropped = max(n_rows - cap, 0)
    status = np.array([(STATUS_BAD_SAMPLE if bad else 0) | (STATUS_ROWS_DROPPED if dropped else 0), bad, dropped, n_rows],
                      dtype=np.int32)
    return AugPlanResult(plans, all_rows[:cap], gt_off, status, crop_rounds, expand_rounds, rows_of, info)


def make_samples(shapes, targets, images=None, sample_ids=None, cls=-1, weights=None, flags=0):
    """Pack per-sample (H, W) shapes and [G,5] target arrays into (SAMPLE_DTYPE array, float32 [total,5] boxes)."""
    n = len(shapes)
    s = np.zeros(n, dtype=SAMPLE_DTYPE)
    pos, parts = 0, []
    for i, (shape, tg) in enumerate(zip(shapes, targets)):
        tg = np.asarray(tg, dtype=np.float32).reshape(-1, 5)
        s[i]['H'], s[i]['W'], s[i]['box_begin'], s[i]['box_end'] = shape[0], shape[1], pos, pos + len(tg)
        pos += len(tg)
        parts.append(tg)
    s['image'] = np.arange(n) if images is None else images
    s['sample_id'] = np.arange(n, dtype=np.uint64) if sample_ids is None else np.asarray(sample_ids, dtype=np.uint64)
    s['cls'], s['flags'] = cls, flags
    s['weight'] = 1.0 if weights is None else weights
    boxes = np.concatenate(parts, 0) if parts else np.zeros((0, 5), dtype=np.float32)
    return s, np.ascontiguousarray(boxes, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------- mosaic
SLOT_MOSAIC = 0x300

MosaicResult = collections.namedtuple('MosaicResult', 'plans tiles truths gt_off status sample_rows fallback info')


def mosaic_tiles(seed, sample_id, size, margin):
    """The four tiles of the image whose first sample draws with `sample_id` -> TILE_DTYPE [4] (include/ctdet.h MOSAIC)."""
    w = draws(seed, sample_id, SLOT_MOSAIC, 0)
    span = size - 2 * margin + 1
    cx, cy = margin + int(randrange(span, w[0])), margin + int(randrange(span, w[1]))
    t = np.zeros(4, dtype=TILE_DTYPE)
    t['x0'], t['y0'] = (0, cx, 0, cx), (0, 0, cy, cy)
    t['w'], t['h'] = (cx, size - cx, cx, size - cx), (cy, cy, size - cy, size - cy)
    return t


def mosaic_rows(rows, tile, size):
    """float32 rows [k,6] of one sample, normalised to its canvas -> (float32 rows in the output image, keep [k])."""
    r = np.asarray(rows, dtype=np.float32).reshape(-1, 6)
    x0, y0, w, h = [float(tile[k]) for k in ('x0', 'y0', 'w', 'h')]
    S = float(size)
    X1, Y1 = (x0 + r[:, 0].astype(np.float64) * w) / S, (y0 + r[:, 1].astype(np.float64) * h) / S
    X2, Y2 = (x0 + r[:, 2].astype(np.float64) * w) / S, (y0 + r[:, 3].astype(np.float64) * h) / S
    out = r.copy()
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = X1, Y1, X2, Y2
    return out, np.minimum(X2 - X1, Y2 - Y1) > 0.01


def mosaic_batch(samples, boxes, num_images, max_gt, seed, p_expand, interp_of_draw, fill, size, margin, truths_cap=None):
    """What `ct_aug_plan_mosaic` computes, safety rule included.  samples: SAMPLE_DTYPE array [4*num_images],
    group-major.  -> MosaicResult: plans (PLAN_DTYPE [4n]), tiles (TILE_DTYPE [4n]), truths float32 [rows, 6] in the
    output image's units, gt_off int32 [n+1], status int32 [4], each sample's kept rows, whether an image's fallback
    fired [n], and plan_sample's dicts (None for a refused sample)."""
    samples = np.asarray(samples, dtype=SAMPLE_DTYPE)
    num_images, size, margin = int(num_images), int(size), int(margin)
    if len(samples) != 4 * num_images or num_images < 1:
        raise ValueError('mosaic_batch: %d samples for %d images' % (len(samples), num_images))
    if size < 2 or not 1 <= margin <= size // 2:
        raise ValueError('mosaic_batch: size %d, margin %d' % (size, margin))
    group = np.arange(len(samples)) // 4
    fixed = samples.copy()
    fixed['image'] = group
    res = plan_batch(fixed, boxes, num_images, max_gt, seed, p_expand, interp_of_draw, fill)
    plans, rows_of, info = res.plans.copy(), list(res.sample_rows), list(res.info)
    bad = int(res.status[1])
    for s in np.flatnonzero(samples['image'] != group):
        if info[s] is not None:                     # planned, but its image field is foreign: refused here
            _identity(plans[s], int(samples[s]['H']), int(samples[s]['W']))
            rows_of[s], info[s] = np.zeros((0, 6), dtype=np.float32), None
            bad += 1
    tiles = np.zeros(len(samples), dtype=TILE_DTYPE)
    fallback = np.zeros(num_images, dtype=bool)
    counts = np.zeros(num_images, dtype=np.int64)
    for i in range(num_images):
        tiles[4 * i:4 * i + 4] = mosaic_tiles(seed, samples[4 * i]['sample_id'], size, margin)
        mapped = [mosaic_rows(rows_of[4 * i + k], tiles[4 * i + k], size) for k in range(4)]
        n_rows, n_kept = sum(len(m[0]) for m in mapped), sum(int(m[1].sum()) for m in mapped)
        fallback[i] = n_rows > 0 and n_kept == 0
        for k, (r, keep) in enumerate(mapped):
            rows_of[4 * i + k] = r if fallback[i] else r[keep]
            counts[i] += len(rows_of[4 * i + k])
    all_rows = np.concatenate(rows_of, 0)
    n_rows = len(all_rows)
    cap = n_rows if truths_cap is None else int(truths_cap)
    gt_off = np.minimum(np.concatenate([[0], np.cumsum(counts)]), cap).astype(np.int32)
    dropped = max(n_rows - cap, 0)
    status = np.array([(STATUS_BAD_SAMPLE if bad else 0) | (STATUS_ROWS_DROPPED if dropped else 0), bad, dropped, n_rows],
                      dtype=np.int32)
    return MosaicResult(plans, tiles, all_rows[:cap], gt_off, status, rows_of, fallback, info)


# ---------------------------------------------------------------------------------------------------- random affine
SLOT_AFFINE = 0x400
AFFINE_APPLIED, AFFINE_FALLBACK, AFFINE_IDENTITY = 1, 2, 4
STATUS_BAD_IMAGE = 1

AffineResult = collections.namedtuple('AffineResult', 'records truths gt_off status image_rows fallback')


class AffineParams(object):
    """The validated parameters of the random affine stage (include/ctdet.h ct_affine_params), built from degrees:
    a rotation of at most `degrees`, an isotropic scale in `scale` = (lo, hi), a shear of at most `shear` degrees per
    axis, a shift of at most `translate` * S, applied with probability `p`; rows are kept when min(w, h) > min_side
    and at least `min_visible` of their area stays inside.  The two tangents are computed here, once, on the host:
    the draw is uniform in tan(angle / 2), neither side evaluates a sine or a cosine."""
    FIELDS = ('rot_half_tan', 'scale_lo', 'scale_hi', 'shear_tan', 'translate', 'p', 'min_side', 'min_visible')

    def __init__(self, degrees=10.0, scale=(0.5, 1.5), shear=2.0, translate=0.1, p=1.0, min_side=0.01, min_visible=0.3):
        vals = dict(degrees=degrees, scale_lo=scale[0], scale_hi=scale[1], shear=shear, translate=translate, p=p,
                    min_side=min_side, min_visible=min_visible)
        for k, v in vals.items():
            if not math.isfinite(float(v)):
                raise ValueError('AffineParams: %s=%r is not finite' % (k, v))
        if not 0 <= degrees <= 90:
            raise ValueError('AffineParams: degrees=%r outside 0..90' % (degrees,))
        if not 0 < scale[0] <= scale[1] <= 4:
            raise ValueError('AffineParams: scale=%r, not 0 < lo <= hi <= 4' % (tuple(scale),))
        if not 0 <= shear <= math.degrees(math.atan(0.5)):
            raise ValueError('AffineParams: shear=%r outside 0..atan(0.5) = 26.56 degrees' % (shear,))
        if not 0 <= translate <= 0.5:
            raise ValueError('AffineParams: translate=%r outside 0..0.5' % (translate,))
        for k in ('p', 'min_side', 'min_visible'):
            if not 0 <= vals[k] <= 1:
                raise ValueError('AffineParams: %s=%r outside 0..1' % (k, vals[k]))
        self.degrees, self.shear = float(degrees), float(shear)
        self.rot_half_tan = min(math.tan(math.radians(float(degrees)) / 2), 1.0)
        self.scale_lo, self.scale_hi = float(scale[0]), float(scale[1])
        self.shear_tan = min(math.tan(math.radians(float(shear))), 0.5)
        self.translate = float(translate)
        # the C struct holds these three as float: both sides compare against the float's value
        self.p, self.min_side, self.min_visible = (float(np.float32(v)) for v in (p, min_side, min_visible))

    def struct(self):
        """-> aug_records.AffineParamsRecord, the host struct ct_aug_affine_plan reads."""
        return AffineParamsRecord(*[getattr(self, k) for k in self.FIELDS])

    def __repr__(self):
        return 'AffineParams(%s)' % ', '.join('%s=%r' % (k, getattr(self, k)) for k in self.FIELDS)


def affine_identity(flags=AFFINE_IDENTITY):
    r = np.zeros((), dtype=AFFINE_DTYPE)
    r['fwd'] = r['inv'] = (1, 0, 0, 0, 1, 0)
    r['flags'] = flags
    return r


def affine_draws(seed, image_id, size, params):
    """-> dict(t, s, kx, ky, tx, ty, applied): the seven draws of one image (include/ctdet.h RANDOM AFFINE)."""
    d = draws(seed, image_id, SLOT_AFFINE, np.arange(2))
    P, S = params, np.float64(size)
    return dict(t=uniform(-P.rot_half_tan, P.rot_half_tan, d[0, 0]), s=uniform(P.scale_lo, P.scale_hi, d[0, 1]),
                kx=uniform(-P.shear_tan, P.shear_tan, d[0, 2]), ky=uniform(-P.shear_tan, P.shear_tan, d[0, 3]),
                tx=uniform(0.5 - P.translate, 0.5 + P.translate, d[1, 0]) * S,
                ty=uniform(0.5 - P.translate, 0.5 + P.translate, d[1, 1]) * S,
                applied=not (float(unit(d[1, 2])) > P.p))


def affine_matrix(seed, image_id, size, params):
    """The record one image draws, gate applied (flags 1, or the identity with flags 4), before its rows are looked
    at -> AFFINE_DTYPE scalar.  fp64, one rounding per operation, in the header's order."""
    w = affine_draws(seed, image_id, size, params)
    if not w['applied']:
        return affine_identity()
    t, s, kx, ky, tx, ty = (np.float64(w[k]) for k in ('t', 's', 'kx', 'ky', 'tx', 'ty'))
    one = np.float64(1.0)
    tt = t * t
    q = one + tt
    c, n = (one - tt) / q, (t + t) / q
    a, b = s * c, s * n
    l00, l01, l10, l11 = a - kx * b, b + kx * a, ky * a - b, ky * b + a
    h = np.float64(size) * np.float64(0.5)
    f2, f5 = tx - (l00 * h + l01 * h), ty - (l10 * h + l11 * h)
    det = l00 * l11 - l01 * l10
    i00, i01, i10, i11 = l11 / det, -l01 / det, -l10 / det, l00 / det
    r = np.zeros((), dtype=AFFINE_DTYPE)
    r['fwd'] = (l00, l01, f2, l10, l11, f5)
    r['inv'] = (i00, i01, -(i00 * f2 + i01 * f5), i10, i11, -(i10 * f2 + i11 * f5))
    r['flags'] = AFFINE_APPLIED
    return r


def affine_rows(rows, fwd, size, min_side, min_visible):
    """float32 rows [k,6] normalised to the image -> (float32 rows after the map, keep [k])."""
    r = np.asarray(rows, dtype=np.float32).reshape(-1, 6)
    S = np.float64(size)
    f = np.asarray(fwd, dtype=np.float64)
    u1, v1, u2, v2 = (r[:, k].astype(np.float64) * S for k in range(4))
    xs, ys = [], []
    for u, v in ((u1, v1), (u2, v1), (u1, v2), (u2, v2)):
        xs.append((f[0] * u + f[1] * v) + f[2])
        ys.append((f[3] * u + f[4] * v) + f[5])
    X1, X2 = np.fmin(np.fmin(np.fmin(xs[0], xs[1]), xs[2]), xs[3]), np.fmax(np.fmax(np.fmax(xs[0], xs[1]), xs[2]), xs[3])
    Y1, Y2 = np.fmin(np.fmin(np.fmin(ys[0], ys[1]), ys[2]), ys[3]), np.fmax(np.fmax(np.fmax(ys[0], ys[1]), ys[2]), ys[3])
    A0 = (X2 - X1) * (Y2 - Y1)
    X1, Y1, X2, Y2 = (np.fmin(np.fmax(v, 0.0), S) for v in (X1, Y1, X2, Y2))
    w, h = X2 - X1, Y2 - Y1
    A1 = w * h
    keep = (np.fmin(w, h) / S > np.float64(min_side)) & (A1 >= np.float64(min_visible) * A0)
    out = r.copy()
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = X1 / S, Y1 / S, X2 / S, Y2 / S
    return out, keep


def affine_batch(truths, gt_off, image_ids, size, seed, params, truths_rows=None):
    """What `ct_aug_affine_plan` computes, safety rule included.  truths float32 [rows,6] and gt_off int32 [B+1] as the
    planners pack them, image_ids [B] 64-bit, truths_rows the capacity the offsets are clamped to (default: the rows
    of `truths`).  -> AffineResult: records (AFFINE_DTYPE [B]), truths float32 [rows out, 6], gt_off int32 [B+1],
    status int32 [4] = (bits, refused images, fallback images, rows out), each image's rows, fallback [B]."""
    truths = np.ascontiguousarray(truths, dtype=np.float32).reshape(-1, 6)
    gt_off = np.asarray(gt_off, dtype=np.int64).reshape(-1)
    B, size = len(gt_off) - 1, int(size)
    cap = len(truths) if truths_rows is None else int(truths_rows)
    if B < 1 or len(image_ids) != B or size < 2 or cap < 0 or cap > len(truths):
        raise ValueError('affine_batch: %d offsets, %d ids, size %d, truths_rows %d of %d'
                         % (len(gt_off), len(image_ids), size, cap, len(truths)))
    off = np.clip(gt_off, 0, cap)
    records = np.zeros(B, dtype=AFFINE_DTYPE)
    fallback = np.zeros(B, dtype=bool)
    image_rows, bad, prev = [], 0, 0
    for i in range(B):
        b, e = int(off[i]), int(off[i + 1])
        refused = b > e or b < prev             # prev: the largest clamped end of the images before this one
        if i >= 1:
            prev = max(prev, b)                 # this image's begin is the end of the one before it
        if refused:
            records[i] = affine_identity()
            image_rows.append(np.zeros((0, 6), dtype=np.float32))
            bad += 1
            continue
        rows = truths[b:e]
        rec = affine_matrix(seed, image_ids[i], size, params)
        if rec['flags'] & AFFINE_APPLIED:
            mapped, keep = affine_rows(rows, rec['fwd'], size, params.min_side, params.min_visible)
            if len(rows) and not keep.any():
                fallback[i] = True
                rec = affine_identity(AFFINE_FALLBACK | AFFINE_IDENTITY)
            else:
                rows = mapped[keep]
        records[i] = rec
        image_rows.append(rows.copy())
    all_rows = np.concatenate(image_rows, 0)
    out_off = np.concatenate([[0], np.cumsum([len(r) for r in image_rows])]).astype(np.int32)
    status = np.array([STATUS_BAD_IMAGE if bad else 0, bad, int(fallback.sum()), len(all_rows)], dtype=np.int32)
    return AffineResult(records, all_rows, out_off, status, image_rows, fallback)


def warp_affine(x, records, border3):
    """What `ct_preproc_warp_affine` computes: x float32 [B,3,S,S], records AFFINE_DTYPE [B], border3 three floats ->
    float32 [B,3,S,S].  Coordinates in float64, the blend in float32, one rounding per operation: bit-comparable to
    the device.  A record with flag 4 copies; any other table, NaN and infinities included, is evaluated by the rule."""
    x = np.asarray(x, dtype=np.float32)
    B, _, S, _ = x.shape
    bd = np.asarray(border3, dtype=np.float32).reshape(3)
    out = np.empty_like(x)
    yy, xx = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing='ij')
    Sd = np.float64(S)
    for n in range(B):
        if int(records[n]['flags']) & AFFINE_IDENTITY:
            out[n] = x[n]
            continue
        v = np.asarray(records[n]['inv'], dtype=np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            X, Y = (v[0] * xx + v[1] * yy) + v[2], (v[3] * xx + v[4] * yy) + v[5]
            inside = (-1.0 < X) & (X < Sd) & (-1.0 < Y) & (Y < Sd)
        X, Y = np.where(inside, X, 0.0), np.where(inside, Y, 0.0)
        flx, fly = np.floor(X), np.floor(Y)
        fx, fy = (X - flx).astype(np.float32), (Y - fly).astype(np.float32)
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        x0, x1, y0, y1 = ix >= 0, ix + 1 < S, iy >= 0, iy + 1 < S
        cx0, cx1, cy0, cy1 = np.maximum(ix, 0), np.minimum(ix + 1, S - 1), np.maximum(iy, 0), np.minimum(iy + 1, S - 1)
        for c in range(3):
            p, bc = x[n, c], bd[c]
            a, b = np.where(x0 & y0, p[cy0, cx0], bc), np.where(x1 & y0, p[cy0, cx1], bc)
            cc, d = np.where(x0 & y1, p[cy1, cx0], bc), np.where(x1 & y1, p[cy1, cx1], bc)
            top, bot = a + fx * (b - a), cc + fx * (d - cc)
            out[n, c] = np.where(inside, top + fy * (bot - top), bc)
    return out
