"""Input transforms with the reference's names and call protocol (data/data_augment.py).

`BaseTransform(resize, rgb_means, swap)(img)` (:224-266, test time): float32 CHW tensor of the resized,
mean-subtracted image; the resize runs on the device (`ct_preproc_resize`, one launch per batch).

`preproc(resize, rgb_means, p)(image, targets[, cls])` (:164-221, training time): random crop -> photometric
distortion -> expand -> mirror -> resize -> minus means, returning (CHW tensor, normalised targets).  Split the
MI355X way: the random DECISIONS are the reference's scalar host logic -- drawn here with the same `random` calls in
the same order, so a seeded run makes the same choices -- and produce one plan record per image; the PIXELS of a whole
batch are then produced by one gather kernel (`ct_preproc_augment`) that never materialises the cropped / distorted /
expanded intermediates.  `filters='cv2'` (or CTDET_AUG_FILTERS=cv2) adds the bicubic and Lanczos4 resize filters the
reference also draws (`ct_preproc_augment_taps`); the default maps those two draws onto linear.
`preproc.batch(images, targets)` is the batched entry that keeps 8 GPUs fed; `mixup_targets` / `mixup_images` are the mixup of data/voc0712.py:240-275.
With `decisions='device'`, `preproc.batch_device` draws the decisions on the device too and `preproc.mosaic_device`
composes four samples into each output image (`ct_aug_plan_mosaic`, `ct_preproc_augment_mosaic`); `affine=` appends
the random affine stage to both (`ct_aug_affine_plan`, `ct_preproc_warp_affine`).
"""
import math
import os
import random

import numpy as np
import torch

from ctdet import ops
from utils.box_utils import matrix_iou

CROP_MODES = (None, (0.1, None), (0.3, None), (0.5, None), (0.7, None), (0.9, None), (None, None))
# preproc_for_test draws one of cv2's [LINEAR, CUBIC, AREA, NEAREST, LANCZOS4].  The device has all five: linear (0),
# nearest (1), area (2), bicubic (3) and Lanczos4 (4).  'fast', the default, runs the two higher-order draws as linear
# (one float gather launch, no tap tables); 'cv2' gives each draw the filter the reference uses.
INTERP_OF_DRAW = (0, 0, 2, 1, 0)
INTERP_FILTERS = {'fast': INTERP_OF_DRAW, 'cv2': (0, 3, 2, 1, 4)}


class BaseTransform(object):
    def __init__(self, resize, rgb_means, swap=(2, 0, 1), device='cuda', max_batch=32):
        if tuple(swap) != (2, 0, 1):
            raise ValueError('BaseTransform: only the HWC->CHW swap (2, 0, 1) is supported')
        self.means, self.resize, self.swap = rgb_means, resize, swap
        self.device, self.max_batch = torch.device(device), max_batch
        self._pre = None

    def _preprocessor(self):
        if self._pre is None:
            self._pre = ops.Preprocessor(self.resize, self.means, self.device, self.max_batch)
        return self._pre

    def batch(self, images, out=None):
        """list of uint8 HxWx3 arrays -> float32 [len,3,resize,resize] on the device."""
        return self._preprocessor()(images, out)

    def __call__(self, img, target=None):
        """data_augment.py:247-266.  With a target the reference returns (tensor, target) untouched."""
        t = self.batch([img])[0]
        return t if target is None else (t, target)


def _plan(h, w):
    """Identity plan for an h x w image: no crop, no distortion, no canvas, no mirror, linear resize."""
    return dict(H=h, W=w, crop=(0, 0, w, h), exp=(w, h, 0, 0), mirror=0, interp=0, flags=0, hue=0,
                beta=0.0, alpha=1.0, sat=1.0)


def _pack_samples(images, targets, offs, sample_ids, image_of, weights, cls):
    """The ct_aug_sample rows of a device batch and its concatenated pixel boxes: per sample its image, [G,5] targets,
    source offset, 64-bit id, batch image and row weight -> (samples, boxes float32 [total,5], max_gt)."""
    samples = np.zeros(len(images), dtype=ops.AUG_SAMPLE_DTYPE)
    parts, pos = [], 0
    for k, (img, tg) in enumerate(zip(images, targets)):
        tg = np.asarray(tg, dtype=np.float32).reshape(-1, 5)
        samples[k] = (offs[k], sample_ids[k], img.shape[0], img.shape[1], pos, pos + len(tg), image_of[k],
                      -1 if cls is None else cls, weights[k], 0)
        pos += len(tg)
        parts.append(tg)
    boxes = np.concatenate(parts, 0) if pos else np.zeros((0, 5), dtype=np.float32)
    return samples, boxes, max(max(len(p) for p in parts), 1)


class preproc(object):
    def __init__(self, resize, rgb_means, p, device='cuda', max_batch=32, rng=None, filters=None, decisions='host',
                 seed=None, affine=None):
        """filters: 'fast' or 'cv2' (INTERP_FILTERS); None reads CTDET_AUG_FILTERS, default 'fast'.  Either way the
        random draws are the same in number and order.
        decisions: 'host' (the default) draws from `random` in the reference's order; 'device' adds `batch_device`,
        which draws them on the device from the counter-based generator keyed by `seed` (ctdet/aug_plan_ref.py).
        affine: None, or an ops.AffineParams (or the dict of its arguments): `batch_device` and `mosaic_device` then
        end with the random affine stage -- rotation, scale, shear, shift, rows carried along (ops.AffineWarp).  It
        needs decisions='device'."""
        if filters is None:
            filters = os.environ.get('CTDET_AUG_FILTERS', 'fast')
        if filters not in INTERP_FILTERS:
            raise ValueError('preproc: filters=%r (known: %s)' % (filters, ', '.join(sorted(INTERP_FILTERS))))
        self.filters, self.interp_of_draw = filters, INTERP_FILTERS[filters]
        self.means, self.resize, self.p = rgb_means, resize, p
        self.device, self.max_batch = torch.device(device), max_batch
        self.rng = rng or random          # the reference uses the module-level generator
        self._aug = None
        if decisions not in ('host', 'device'):
            raise ValueError("preproc: decisions=%r (known: 'host', 'device')" % (decisions,))
        if decisions == 'device' and filters == 'cv2':
            raise ValueError("preproc: filters='cv2' needs host decisions: the bicubic / Lanczos4 tap tables depend on "
                             "the canvas size, which decisions='device' never brings to the host")
        self.decisions, self.seed = decisions, 0 if seed is None else int(seed)
        self._planner = self._aug_dev = None
        if affine is not None and decisions != 'device':
            raise ValueError("preproc: affine= needs decisions='device': the stage runs behind batch_device / mosaic_device")
        self.affine = None if affine is None else ops.affine_params(affine)
        self._affine = None

    # ------------------------------------------------------------------ decisions (host scalars, no pixels)
    def _crop(self, width, height, boxes, labels, cls):
        """data_augment.py:19-79: -> (l, t, w, h), boxes, labels."""
        rng = self.rng
        if len(boxes) == 0:
            return (0, 0, width, height), boxes, labels
        while True:
            mode = rng.choice(CROP_MODES)
            if mode is None:
                return (0, 0, width, height), boxes, labels
            min_iou = float('-inf') if mode[0] is None else mode[0]
            max_iou = float('inf') if mode[1] is None else mode[1]
            for _ in range(50):
                scale = rng.uniform(0.3, 1.)
                lo, hi = max(0.5, scale * scale), min(2, 1. / scale / scale)
                ratio = math.sqrt(rng.uniform(lo, hi))
                w, h = int(scale * ratio * width), int((scale / ratio) * height)
                l, t = rng.randrange(width - w), rng.randrange(height - h)
                roi = np.array((l, t, l + w, t + h))
                iou = matrix_iou(boxes, roi[np.newaxis])
                if not (min_iou <= iou.min() and iou.max() <= max_iou):
                    continue
                centers = (boxes[:, :2] + boxes[:, 2:]) / 2
                inside = np.logical_and(roi[:2] < centers, centers < roi[2:]).all(axis=1)
                bt, lt = boxes[inside].copy(), labels[inside].copy()
                if len(bt) == 0 or (cls is not None and (lt != (cls + 1)).all()):
                    continue
                bt[:, :2] = np.maximum(bt[:, :2], roi[:2]) - roi[:2]
                bt[:, 2:] = np.minimum(bt[:, 2:], roi[2:]) - roi[:2]
                return (l, t, w, h), bt, lt

    def _distort(self, plan):
        """data_augment.py:82-110: which of brightness / contrast / hue / saturation, and by how much."""
        rng = self.rng
        if rng.randrange(2):
            plan['flags'] |= 1
            plan['beta'] = rng.uniform(-32, 32)
        if rng.randrange(2):
            plan['flags'] |= 2
            plan['alpha'] = rng.uniform(0.5, 1.5)
        if rng.randrange(2):
            plan['flags'] |= 4
            plan['hue'] = rng.randint(-18, 18)
        if rng.randrange(2):
            plan['flags'] |= 8
            plan['sat'] = rng.uniform(0.5, 1.5)

    def _expand(self, width, height, boxes):
        """data_augment.py:113-146: -> (canvas w, canvas h, left, top), boxes."""
        rng = self.rng
        if rng.random() > self.p:
            return (width, height, 0, 0), boxes
        while True:
            scale = rng.uniform(1, 4)
            lo, hi = max(0.5, 1. / scale / scale), min(2, scale * scale)
            ratio = math.sqrt(rng.uniform(lo, hi))
            ws, hs = scale * ratio, scale / ratio
            if ws < 1 or hs < 1:
                continue
            w, h = int(ws * width), int(hs * height)
            left, top = rng.randint(0, w - width), rng.randint(0, h - height)
            bt = boxes.copy()
            bt[:, :2] += (left, top)
            bt[:, 2:] += (left, top)
            return (w, h, left, top), bt

    def decide(self, shape, targets, cls=None):
        """All random choices of one `preproc.__call__` for an image of `shape` (h, w, 3) and pixel targets
        [G,5] = (x1, y1, x2, y2, label)  ->  (plan, targets_out [G',5] normalised).  Pure host logic."""
        rng = self.rng
        height_o, width_o = int(shape[0]), int(shape[1])
        targets = np.asarray(targets)
        boxes, labels = targets[:, :-1].copy(), targets[:, -1].copy()
        targets_o = targets.copy()                       # fallback: the untouched image with normalised boxes
        targets_o[:, 0:4:2] /= width_o
        targets_o[:, 1:4:2] /= height_o
        plan = _plan(height_o, width_o)
        plan['crop'], boxes, labels = self._crop(width_o, height_o, boxes, labels, cls)
        self._distort(plan)
        cw, ch = plan['crop'][2], plan['crop'][3]
        plan['exp'], boxes = self._expand(cw, ch, boxes)
        width, height = plan['exp'][0], plan['exp'][1]
        if rng.randrange(2):                             # _mirror (:149-155)
            plan['mirror'] = 1
            boxes = boxes.copy()
            boxes[:, 0::2] = width - boxes[:, 2::-2]
        plan['interp'] = self.interp_of_draw[rng.randrange(5)]            # preproc_for_test (:158-161)
        boxes = boxes.copy()
        boxes[:, 0::2] /= width
        boxes[:, 1::2] /= height
        keep = np.minimum(boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]) > 0.01
        bt, lt = boxes[keep], labels[keep].copy()
        if len(bt) == 0 or (cls is not None and (lt != (cls + 1)).all()):
            plan = _plan(height_o, width_o)              # the original image, resized (:205-212)
            plan['interp'] = self.interp_of_draw[rng.randrange(5)]
            return plan, targets_o
        return plan, np.hstack((bt, np.expand_dims(lt, 1)))

    # ------------------------------------------------------------------ pixels (device)
    def _augmenter(self):
        if self._aug is None:
            self._aug = ops.Augmenter(self.resize, self.means, self.device, self.max_batch)
        return self._aug

    def batch(self, images, targets, cls=None, out=None):
        """lists of uint8 HxWx3 images and [G,5] pixel targets -> (float32 [n,3,S,S] on the device, [targets_out])."""
        plans, touts = [], []
        for img, tg in zip(images, targets):
            plan, tout = self.decide(img.shape, tg, cls)
            plans.append(plan)
            touts.append(tout)
        return self._augmenter()(images, plans, out), touts

    def __call__(self, image, targets, cls=None):
        imgs, touts = self.batch([image], [targets], cls)
        return imgs[0], touts[0]

    # ------------------------------------------------------------------ decisions on the device
    def _device_staging(self, per_image):
        """The staging Augmenter and AugPlanner of the device path, sized for `per_image` samples per batch image
        (2 for mixup, 4 for mosaic); created by the first call that needs them, replaced by larger ones on demand."""
        if self._planner is None or self._aug_dev.max_batch < per_image * self.max_batch:
            self._aug_dev = ops.Augmenter(self.resize, self.means, self.device, per_image * self.max_batch)
            self._planner = ops.AugPlanner(self.device, self.seed, self.p, self.interp_of_draw, self.means,
                                           per_image * self.max_batch)

    def _affine_stage(self, x, packed, image_ids):
        """The random affine post-stage on a rendered batch and its packed rows, when `affine` was given; image i draws
        with image_ids[i].  Outside the image lies the renderers' canvas fill, (float)(int)mean - mean."""
        if self.affine is None:
            return x, packed
        if self._affine is None:
            self._affine = ops.AffineWarp(self.device, self.seed, self.affine)
        border = [float(np.float32(int(m)) - np.float32(m)) for m in self.means]
        return self._affine(x, packed, image_ids, border)

    def batch_device(self, images, targets, sample_ids, cls=None, mix=None):
        """decisions='device': lists of uint8 HxWx3 images and [G,5] pixel targets, one 64-bit sample id per image ->
        (float32 [n,3,S,S], ops.PackedTargets(truths, gt_off, max_gt)), all on the device; no per-sample host work
        beyond packing the inputs.  mix = (second images, second targets, lambdas): image i is blended with its
        second image by lambdas[i] (data/voc0712.py:240-275); a lambda >= 1 means the first sample alone with weight
        1.  A second sample draws with id sample_ids[i] + 2**63.  With `affine`, the (blended) image and its merged
        rows are then warped; the warp draws with sample_ids[i]."""
        if self.decisions != 'device':
            raise ValueError("preproc.batch_device needs preproc(..., decisions='device')")
        n = len(images)
        if n == 0 or n > self.max_batch or len(targets) != n or len(sample_ids) != n:
            raise ValueError('preproc.batch_device: %d images, %d targets, %d sample ids (max %d)'
                             % (n, len(targets), len(sample_ids), self.max_batch))
        self._device_staging(2)
        lam = [1.0] * n if mix is None else [float(v) for v in mix[2]]
        imgs, tgs, rec = [], [], []           # samples in image order: first, then second where there is one
        first, second = [], []
        for i in range(n):
            two = mix is not None and lam[i] < 1
            first.append(len(imgs))
            imgs.append(images[i]); tgs.append(targets[i])
            rec.append((i, int(sample_ids[i]), np.float32(lam[i]) if two else np.float32(1)))
            second.append(len(imgs) if two else first[-1])
            if two:
                imgs.append(mix[0][i]); tgs.append(mix[1][i])
                rec.append((i, int(sample_ids[i]) + 2 ** 63, np.float32(1. - lam[i])))
        m = len(imgs)
        samples, boxes, max_gt = _pack_samples(imgs, tgs, self._aug_dev.upload(imgs), [r[1] % 2 ** 64 for r in rec],
                                               [r[0] for r in rec], [r[2] for r in rec], cls)
        plans, packed = self._planner(samples, boxes, n, max_gt)
        if mix is None:
            return self._affine_stage(self._aug_dev.render(plans, n), packed, sample_ids)
        # the plans of the first samples, then of the second ones (a lambda >= 1 blends an image with itself)
        order = torch.tensor(first + second, dtype=torch.int64).to(self.device, non_blocking=True)
        x = self._aug_dev.render(plans.view(m, ops.PLAN_BYTES).index_select(0, order).reshape(-1), 2 * n)
        x = ops.mixup_blend(x[:n], x[n:], torch.tensor(lam, dtype=torch.float32).clamp(max=1.0).to(self.device))
        return self._affine_stage(x, packed, sample_ids)

    def mosaic_device(self, images, targets, sample_ids, cls=None, margin=None):
        """decisions='device': four-image mosaic.  4n uint8 HxWx3 images and [G,5] pixel targets, group-major (sample
        4i+k is slot k of image i: top-left, top-right, bottom-left, bottom-right), and n 64-bit sample ids ->
        (float32 [n,3,S,S], ops.PackedTargets), all on the device.  Sample k of image i draws with id
        (sample_ids[i] + k * 2**61) mod 2**64 (distinct from mixup's + 2**63); the tiles meet at a point drawn per
        image at least `margin` (default S // 4) pixels from every edge (include/ctdet.h MOSAIC).  Every sample is
        cropped / distorted / expanded / mirrored as in `batch_device`, then resized into its tile; the rows are in
        units of the composed image.  With `affine`, the composed image and its rows are then warped; the warp draws
        with sample_ids[i], the id of the group's first sample."""
        if self.decisions != 'device':
            raise ValueError("preproc.mosaic_device needs preproc(..., decisions='device')")
        n = len(sample_ids)
        if n == 0 or n > self.max_batch or len(images) != 4 * n or len(targets) != 4 * n:
            raise ValueError('preproc.mosaic_device: %d images, %d targets, %d sample ids (4 images per id, max %d ids)'
                             % (len(images), len(targets), n, self.max_batch))
        S = int(self.resize)
        margin = S // 4 if margin is None else int(margin)
        if not 1 <= margin <= S // 2:
            raise ValueError('preproc.mosaic_device: margin %d outside 1..%d' % (margin, S // 2))
        self._device_staging(4)
        ids = [(int(sample_ids[s // 4]) + (s % 4) * 2 ** 61) % 2 ** 64 for s in range(4 * n)]
        samples, boxes, max_gt = _pack_samples(images, targets, self._aug_dev.upload(images), ids,
                                               [s // 4 for s in range(4 * n)], [1.0] * (4 * n), cls)
        plans, tiles, packed = self._planner.mosaic(samples, boxes, n, max_gt, S, margin)
        return self._affine_stage(self._aug_dev.render_mosaic(plans, tiles, n), packed, sample_ids)


def mixup_targets(target1, target2, lambd, ignore_minus1=False):
    """data/voc0712.py:263-273: [G1,5] + [G2,5] -> [G1+G2,6] with the mixup weight as the last column; in phase 2 of
    the incremental setting boxes labelled -1 get weight 0.  lambd >= 1: target1 with weight 1 (:247-250)."""
    if target2 is None or lambd >= 1:
        return np.hstack((target1, np.ones((target1.shape[0], 1))))
    y1 = np.hstack((target1, np.full((target1.shape[0], 1), float(lambd))))
    y2 = np.hstack((target2, np.full((target2.shape[0], 1), 1. - float(lambd))))
    mix = np.vstack((y1, y2))
    if ignore_minus1:
        mix[mix[:, -2] == -1, -1] = 0
    return mix


def mixup_images(img1, img2, lambd):
    """data/voc0712.py:262 on device batches: img1 * lambd + img2 * (1 - lambd), lambd a float or one per image."""
    return ops.mixup_blend(img1, img2, lambd)
