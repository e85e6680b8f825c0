"""Detection results format + PASCAL VOC and COCO bbox evaluation for the batched pipeline.

Restates, on in-memory arrays, what the reference does through files:
  test.py:107-109,171-172           all_boxes[class][image] = float32 [k,5]; `detections.pkl`
  data/voc0712.py:351-376           comp4_det_test_<cls>.txt lines `id score x1+1 y1+1 x2+1 y2+1`
                                     formatted {:.3f} / {:.1f}  (the rounding is part of the metric)
  data/voc_eval.py:33-66            voc_ap  (VOC07 11-point and area-under-curve)
  data/voc_eval.py:67-203           voc_eval (greedy matching at IoU > 0.5 with the +1 pixel
                                     convention, `difficult` boxes ignored, duplicates = FP)
  data/coco.py:232-345              results dicts, COCOeval(..., 'bbox'), _derive_coco_results
  utils/pycocotools/cocoeval.py     evaluate / evaluateImg / accumulate / summarize, maskApi.c bbIou
Host-side numpy like the reference; the Device*Evaluator classes run the same rules in HIP kernels (csrc/ct_eval.hip,
csrc/ct_coco_eval.hip) on the rows the post-processing leaves on the device.
"""
import collections
import os
import pickle

import numpy as np

from ._lib import CtdetError

KEY_UNUSED = np.iinfo(np.int64).max                 # CT_VOC_KEY_UNUSED: sorts behind every record's key


def to_reference_all_boxes(per_image):
    """[img][cls] (DetectionPipeline.results()) -> the reference's all_boxes[cls][img]."""
    ncls = len(per_image[0]) if per_image else 0
    return [[per_image[i][j] for i in range(len(per_image))] for j in range(ncls)]


def save_detections(all_boxes, path):
    """test.py:171-172: pickle of all_boxes with HIGHEST_PROTOCOL."""
    with open(path, 'wb') as f:
        pickle.dump(all_boxes, f, pickle.HIGHEST_PROTOCOL)


def results_lines(all_boxes_cls, image_ids):
    """Text lines of one class's results file (data/voc0712.py:360-376)."""
    lines = []
    for im_ind, index in enumerate(image_ids):
        dets = all_boxes_cls[im_ind]
        if len(dets) == 0:
            continue
        for k in range(dets.shape[0]):
            lines.append('{:s} {:.3f} {:.1f} {:.1f} {:.1f} {:.1f}'.format(
                index, dets[k, -1], dets[k, 0] + 1, dets[k, 1] + 1, dets[k, 2] + 1, dets[k, 3] + 1))
    return lines


def write_voc_results(all_boxes, image_ids, classes, out_dir, template='comp4_det_test_{:s}.txt'):
    os.makedirs(out_dir, exist_ok=True)
    paths = {}
    for cls_ind, cls in enumerate(classes):
        if cls == '__background__':
            continue
        paths[cls] = os.path.join(out_dir, template.format(cls))
        with open(paths[cls], 'wt') as f:
            for line in results_lines(all_boxes[cls_ind], image_ids):
                f.write(line + '\n')
    return paths


def voc_ap(rec, prec, use_07_metric=False):
    """data/voc_eval.py:33-66."""
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def voc_eval_lines(lines, gt, ovthresh=0.5, use_07_metric=False, stable=False):
    """data/voc_eval.py:134-203 on the parsed lines of one class.

    gt: {image_id: {'bbox': int array [k,4], 'difficult': bool array [k]}} for THIS class
    (images without objects of the class may be missing).  Returns (rec, prec, ap).
    stable=True orders equal (three-decimal) scores by line number -- np.argsort(-scores, kind='stable') -- instead of
    the arbitrary order the reference's default sort leaves them in: the pinned order DeviceVOCEvaluator reproduces."""
    per_image, num_pos = {}, 0
    for img, r in gt.items():
        bbox = np.asarray(r['bbox']).reshape(-1, 4) if len(r['bbox']) else np.zeros((0, 4))
        difficult = np.asarray(r['difficult'], dtype=bool).reshape(-1)
        per_image[img] = {'bbox': bbox, 'difficult': difficult, 'det': [False] * len(difficult)}
        num_pos += int(np.sum(~difficult))
    split = [x.strip().split(' ') for x in lines]
    image_ids = [x[0] for x in split]
    scores = np.array([float(x[1]) for x in split])
    BB = np.array([[float(z) for z in x[2:]] for x in split])
    order = np.argsort(-scores, kind='stable') if stable else np.argsort(-scores)
    BB = BB[order, :] if BB.size != 0 else BB
    image_ids = [image_ids[x] for x in order]
    nd = len(image_ids)
    tp, fp = np.zeros(nd), np.zeros(nd)
    empty = {'bbox': np.zeros((0, 4)), 'difficult': np.zeros(0, bool), 'det': []}
    for d in range(nd):
        rec_i = per_image.get(image_ids[d], empty)
        bb = BB[d, :].astype(float)
        best_iou = -np.inf
        gt_boxes = rec_i['bbox'].astype(float)
        if gt_boxes.size > 0:
            iw = np.maximum(np.minimum(gt_boxes[:, 2], bb[2]) - np.maximum(gt_boxes[:, 0], bb[0]) + 1., 0.)
            ih = np.maximum(np.minimum(gt_boxes[:, 3], bb[3]) - np.maximum(gt_boxes[:, 1], bb[1]) + 1., 0.)
            inter_area = iw * ih
            union_area = ((bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) +
                   (gt_boxes[:, 2] - gt_boxes[:, 0] + 1.) * (gt_boxes[:, 3] - gt_boxes[:, 1] + 1.) - inter_area)
            ious = inter_area / union_area
            best_iou = np.max(ious)
            best_j = np.argmax(ious)
        if best_iou > ovthresh:
            if not rec_i['difficult'][best_j]:
                if not rec_i['det'][best_j]:
                    tp[d] = 1.
                    rec_i['det'][best_j] = 1
                else:
                    fp[d] = 1.
        else:
            fp[d] = 1.
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    rec = tp / float(num_pos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec, use_07_metric)


def evaluate_detections(all_boxes, image_ids, gt_by_class, classes, use_07_metric=True, ovthresh=0.5, stable=False):
    """data/voc0712.py:339-426 without the files: all_boxes[cls][img] -> {cls: ap}, mean AP.
    gt_by_class[cls] is the `gt` mapping of voc_eval_lines.  Detections pass through the same text
    formatting as the results files, so scores are compared at 3 and boxes at 1 decimal.
    stable: see voc_eval_lines (True = the host twin of DeviceVOCEvaluator)."""
    aps = {}
    for cls_ind, cls in enumerate(classes):
        if cls == '__background__':
            continue
        lines = results_lines(all_boxes[cls_ind], image_ids)
        aps[cls] = float(voc_eval_lines(lines, gt_by_class.get(cls, {}), ovthresh, use_07_metric, stable)[2])
    return aps, float(np.mean(list(aps.values()))) if aps else float('nan')


def quantise_like_results_file(dets):
    """float32 [k,5] rows -> (boxes float64 [k,4], n int64 [k]): what float() reads back from a results line
    ('{:.1f}' of coordinate + 1, the + 1 in float32) and the integer its '{:.3f}' score prints, without the text.
    Exact: the products by 10 and 1000 are exact in double (24 x 4 and 24 x 10 bits), np.rint rounds half-even like
    format does on an exactly representable tie, and the division by 10.0 is correctly rounded.  ct_voc_match
    (csrc/ct_eval.hip) does the same arithmetic."""
    d = np.asarray(dets, dtype=np.float32).reshape(-1, 5)
    boxes = np.rint((d[:, :4] + np.float32(1)).astype(np.float64) * 10) / 10.0
    return boxes, np.rint(d[:, 4].astype(np.float64) * 1000).astype(np.int64)


def pack_ground_truth(gt_by_class, classes, image_ids):
    """The ground truth of a data set as ct_voc_match reads it: (boxes float32 [G,4], label int32 [G] in 1..T,
    difficult uint8 [G], off int32 [N+1] by position in image_ids, num_pos int32 [T]).  Within an image the boxes of a
    class keep their annotation order.  num_pos counts every non-difficult box of the class's mapping, whether or not
    its image is in image_ids, as voc_eval_lines does."""
    if not classes or classes[0] != '__background__' or '__background__' in classes[1:]:
        raise ValueError("classes must be ['__background__', <foreground classes>]")
    fg = classes[1:]
    num_pos = np.zeros(len(fg), dtype=np.int32)
    for j, cls in enumerate(fg):
        for r in gt_by_class.get(cls, {}).values():
            num_pos[j] += int(np.sum(~np.asarray(r['difficult'], dtype=bool).reshape(-1)))
    boxes, label, difficult, off = [], [], [], [0]
    for iid in image_ids:
        k = 0
        for j, cls in enumerate(fg):
            r = gt_by_class.get(cls, {}).get(iid)
            if r is None or len(r['bbox']) == 0:
                continue
            bb = np.asarray(r['bbox'], dtype=np.float64).reshape(-1, 4)
            if not np.array_equal(bb.astype(np.float32).astype(np.float64), bb):
                raise ValueError('ground truth of %r in image %r is not exact in float32' % (cls, iid))
            boxes.append(bb.astype(np.float32))
            label.append(np.full(len(bb), j + 1, dtype=np.int32))
            difficult.append(np.asarray(r['difficult'], dtype=bool).reshape(-1).astype(np.uint8))
            k += len(bb)
        off.append(off[-1] + k)
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)      # noqa: E731
    return (cat(boxes, (0, 4), np.float32), cat(label, 0, np.int32), cat(difficult, 0, np.uint8),
            np.asarray(off, dtype=np.int32), num_pos)


class DeviceVOCEvaluator:
    """evaluate_detections on the device, fed batch by batch from the pipeline's own output buffers
    (ops.PostProcessor.out_dets / out_count): nothing is copied to the host or formatted as text.

        ev = DeviceVOCEvaluator(gt_by_class, classes, image_ids, device)
        for each batch:  ev.add(out_dets, out_count, image_index)      # one launch, no synchronisation
        aps, mean = ev.finish()                                        # == evaluate_detections(..., stable=True)

    The ground truth is packed and uploaded once, the record buffer (len(image_ids) x per_image_cap keys and flag
    bytes) allocated once.  per_image_cap bounds the rows one image may contribute over all classes; the default 256
    leaves room for the ties the `200 best` rule of test.py:155-161 keeps.  finish() raises, never drops rows, when an
    image had more.  rec, prec and the 11-point AP equal the host's bit for bit; the area AP to the order of its sum.
    Feeding an image twice is refused when image_index is host data; with a device tensor it is not detected and the
    later rows replace the earlier ones."""

    def __init__(self, gt_by_class, classes, image_ids, device, ovthresh=0.5, use_07_metric=True, per_image_cap=None):
        import torch
        from . import ops
        self._torch, self._ops = torch, ops
        self.classes, self.image_ids = list(classes), list(image_ids)
        self.device = torch.device(device)
        self.ovthresh, self.use_07_metric = float(ovthresh), bool(use_07_metric)
        boxes, label, difficult, off, num_pos = pack_ground_truth(gt_by_class, self.classes, self.image_ids)
        self.T, self.N, self.G = len(self.classes) - 1, len(self.image_ids), len(label)
        if self.T < 1 or self.N < 1:
            raise ValueError('DeviceVOCEvaluator needs at least one foreground class and one image')
        self.max_gt = int(np.diff(off).max())
        self.per_image_cap = int(per_image_cap or 256)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)                  # noqa: E731
        pad = lambda a, shape: a if len(a) else np.zeros(shape, a.dtype)                          # noqa: E731
        self.gt_boxes, self.gt_label = up(pad(boxes, (1, 4))), up(pad(label, 1))
        self.gt_difficult, self.gt_off, self.num_pos = up(pad(difficult, 1)), up(off), up(num_pos)
        self.num_pos_host = num_pos
        slots = self.N * self.per_image_cap
        self.keys = torch.empty(slots, dtype=torch.int64, device=self.device)
        self.flags = torch.empty(slots, dtype=torch.uint8, device=self.device)
        self.status = torch.empty(2, dtype=torch.int32, device=self.device)
        self.pr_status = torch.empty(1, dtype=torch.int32, device=self.device)
        self.bounds = (torch.arange(self.T + 1, dtype=torch.int64) << 53).to(self.device)        # first key of each class
        self.rec = torch.empty(slots, dtype=torch.float64, device=self.device)
        self.prec = torch.empty(slots, dtype=torch.float64, device=self.device)
        self.ap = torch.empty(self.T, dtype=torch.float64, device=self.device)
        self.thresholds = np.arange(0., 1.1, 0.1)               # data/voc_eval.py:42; three times 0.1 is not 0.3
        self._ring, self._ring_events, self._ring_pos = None, [None] * 4, 0
        self.reset()

    def reset(self):
        """Forget every image fed so far."""
        self.keys.fill_(KEY_UNUSED)
        self.flags.zero_()
        self.status.zero_()
        self.seen = np.zeros(self.N, dtype=bool)
        self._off_host = None

    def _upload_index(self, idx):
        """Host image indices -> a device int32 tensor through a small ring of pinned buffers: no pageable copy (which
        would wait for the stream), no wait unless four adds are still in flight."""
        torch = self._torch
        n = len(idx)
        if self._ring is None or self._ring.shape[1] < n:
            self._ring = torch.empty(len(self._ring_events), max(n, 32), dtype=torch.int32).pin_memory()
            self._ring_events = [None] * len(self._ring_events)
        k = self._ring_pos
        self._ring_pos = (k + 1) % len(self._ring_events)
        if self._ring_events[k] is not None:
            self._ring_events[k].synchronize()
        self._ring[k, :n] = torch.from_numpy(idx)
        dev = self._ring[k, :n].to(self.device, non_blocking=True)
        self._ring_events[k] = torch.cuda.Event()
        self._ring_events[k].record()
        return dev

    def add(self, out_dets, out_count, image_index):
        """One pipeline batch: out_dets [B,T,cap,5], out_count [B,T] (device, as ct_postprocess_batched leaves them),
        image_index [B] = position of each image in image_ids, -1 for a padding image.  Issues ct_voc_match on the
        current stream and returns without synchronising."""
        torch = self._torch
        self._ops._dev(out_dets, 'out_dets')
        self._ops._dev(out_count, 'out_count', torch.int32)
        if out_dets.dim() != 4 or out_dets.shape[1] != self.T or out_dets.shape[3] != 5:
            raise ValueError('out_dets must be [B,%d,cap,5], got %s' % (self.T, tuple(out_dets.shape)))
        B, cap = out_dets.shape[0], out_dets.shape[2]
        if tuple(out_count.shape) != (B, self.T):
            raise ValueError('out_count must be [%d,%d], got %s' % (B, self.T, tuple(out_count.shape)))
        if isinstance(image_index, torch.Tensor) and image_index.is_cuda:
            index = image_index
        else:
            idx = np.ascontiguousarray(np.asarray(image_index).reshape(-1), dtype=np.int32)
            if len(idx) != B:
                raise ValueError('image_index has %d entries for a batch of %d' % (len(idx), B))
            real = idx[idx >= 0]
            if real.size and real.max() >= self.N:
                raise CtdetError('image_index %d outside the %d images of the data set' % (real.max(), self.N))
            again = np.bincount(real, minlength=self.N) + self.seen > 1
            if again.any():
                raise CtdetError('image fed twice: index %s' % np.flatnonzero(again).tolist())
            self.seen[real] = True
            index = self._upload_index(idx)
        if index.numel() != B:
            raise ValueError('image_index has %d entries for a batch of %d' % (index.numel(), B))
        self._ops.voc_match(out_dets, out_count, index, self, cap)
        self._off_host = None

    def finish(self, use_07_metric=None):
        """-> ({class: ap}, mean AP) in evaluate_detections' shape.  One look at the status words, the key sort
        (torch.sort: plumbing, the keys are unique), ct_voc_pr."""
        torch = self._torch
        use07 = self.use_07_metric if use_07_metric is None else bool(use_07_metric)
        flags, most = self.status.tolist()
        if flags & 1:
            raise CtdetError('an image has %d detection rows, per_image_cap is %d: construct the evaluator with '
                             'per_image_cap >= %d' % (most, self.per_image_cap, most))
        if flags & 2:
            raise CtdetError('ct_voc_match met an image index or a ground-truth offset out of range')
        if flags & 4:
            raise CtdetError('ct_voc_match met a score outside 0 .. 1048.575 (or NaN)')
        sorted_keys, order = torch.sort(self.keys)
        off = torch.searchsorted(sorted_keys, self.bounds)
        self._ops.voc_pr(self, order, off, self.thresholds if use07 else None)
        ap = self.ap.cpu().numpy()
        if int(self.pr_status.item()):
            raise CtdetError('ct_voc_pr met an offset or a permutation entry out of range')
        self._off_host = off.cpu().numpy()
        aps = {cls: float(ap[j]) for j, cls in enumerate(self.classes[1:])}
        return aps, float(np.mean(list(aps.values()))) if aps else float('nan')

    def curves(self, cls):
        """(rec, prec) float64 arrays of one class, as voc_eval_lines returns them; after finish()."""
        if self._off_host is None:
            raise CtdetError('curves() needs finish() after the last add()')
        j = self.classes.index(cls) - 1
        a, b = int(self._off_host[j]), int(self._off_host[j + 1])
        return self.rec[a:b].cpu().numpy(), self.prec[a:b].cpu().numpy()


def coco_results(all_boxes, image_ids, category_ids):
    """data/coco.py:242-270: all_boxes[cls][img] -> the list of COCO result dicts
    {image_id, category_id, bbox [x, y, w, h] with the +1 width/height convention, score}.
    category_ids[cls] is the COCO id of class index cls (index 0 = background is skipped)."""
    out = []
    for cls_ind, cat_id in enumerate(category_ids):
        if cls_ind == 0:
            continue
        for im_ind, image_id in enumerate(image_ids):
            dets = all_boxes[cls_ind][im_ind]
            if len(dets) == 0:
                continue
            dets = np.asarray(dets, dtype=np.float64)
            xs, ys = dets[:, 0], dets[:, 1]
            ws, hs = dets[:, 2] - xs + 1, dets[:, 3] - ys + 1
            out.extend({'image_id': image_id, 'category_id': cat_id,
                        'bbox': [float(xs[k]), float(ys[k]), float(ws[k]), float(hs[k])],
                        'score': float(dets[k, -1])} for k in range(dets.shape[0]))
    return out


def write_coco_results(all_boxes, image_ids, category_ids, res_file):
    """data/coco.py:260-274: JSON file for pycocotools' loadRes."""
    import json
    with open(res_file, 'w') as f:
        json.dump(coco_results(all_boxes, image_ids, category_ids), f)
    return res_file


# ---------------------------------------------------------------------------------------------------------------------
# COCO bbox evaluation (utils/pycocotools/cocoeval.py evaluate / accumulate / summarize with iouType 'bbox' and
# useCats = 1, maskApi.c bbIou, data/coco.py:232-345) on in-memory arrays: the host twin of DeviceCOCOEvaluator.
COCO_MAX_GT_PER_SEGMENT = 256           # CT_COCO_MAX_GT_PER_SEGMENT: boxes of one category in one image
COCO_MAX_CATEGORIES = 127               # 7 key bits, and 127 is left to the `unused` key
COCO_MAX_IMAGES = 1 << 17               # 17 key bits
COCO_AREA_LABELS = ('all', 'small', 'medium', 'large')

COCOGroundTruth = collections.namedtuple('COCOGroundTruth', [
    'boxes',        # float64 [G,4]  [x, y, w, h]
    'area',         # float64 [G]    the annotation's own area
    'iscrowd',      # uint8   [G]
    'label',        # int32   [G]    class index 1 .. T (the position in category_ids)
    'off',          # int32   [N+1]  by image RANK (ascending image id); within an image by class, then annotation order
    'npig',         # int32   [K,A]  non-crowd boxes with lo <= area <= hi, K by ascending category id
    'image_ids',    # list    [N]    the evaluated images in data set order (position = the image_index of add())
    'image_rank',   # int32   [N]    data set position -> rank by ascending image id
    'cat_ids',      # list    [K]    ascending category ids
    'cat_rank',     # int32   [T+1]  class index -> K position ([0], the background, is -1)
    'names',        # list    [K]    category names in K order
    'area_rng',     # float64 [A,2]
])


def coco_default_params():
    """Params.setDetParams (cocoeval.py:502-511), its own expressions: (iou_thrs, rec_thrs, area_rng, max_dets)."""
    iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    area_rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
    return iou_thrs, rec_thrs, np.asarray(area_rng, dtype=np.float64), (1, 10, 100)


def pack_coco_ground_truth(gt, category_ids, image_ids=None, area_rng=None):
    """A COCO-format dict (`images`, `annotations`, `categories`) as ct_coco_match reads it -> COCOGroundTruth.

    category_ids[j] is the COCO id of class index j (index 0 = background), as in coco_results.  image_ids: the
    evaluated images in data set order (default: gt['images'] in their order); annotations of other images are left
    out, as COCOeval leaves out what is not in params.imgIds.  Images are RANKED by ascending id and the K axis runs
    over every category of gt['categories'] by ascending id -- the order COCOeval gets from np.unique, on which the bits
    of every mean depend.  A category of the data set that is not in category_ids keeps its K position and its npig and
    can have no detections.  Boxes are float64: 258.15 is not a float32.  Refused: an annotation id of 0 (the reference
    reads a match to id 0 as `unmatched`), more than COCO_MAX_GT_PER_SEGMENT boxes in one (image, category), ids that
    repeat."""
    area_rng = coco_default_params()[2] if area_rng is None else np.asarray(area_rng, dtype=np.float64).reshape(-1, 2)
    cats = sorted(gt['categories'], key=lambda c: c['id'])
    cat_ids = [c['id'] for c in cats]
    if len(set(cat_ids)) != len(cat_ids) or len(cat_ids) > COCO_MAX_CATEGORIES:
        raise ValueError('categories must have distinct ids, at most %d of them' % COCO_MAX_CATEGORIES)
    k_of = {c: k for k, c in enumerate(cat_ids)}
    fg = list(category_ids)[1:]
    if len(set(fg)) != len(fg) or any(c not in k_of for c in fg):
        raise ValueError('category_ids[1:] must be distinct categories of the data set')
    cls_of = {c: j + 1 for j, c in enumerate(fg)}
    all_ids = [im['id'] for im in gt['images']]
    image_ids = list(all_ids if image_ids is None else image_ids)
    if len(set(image_ids)) != len(image_ids) or not set(image_ids) <= set(all_ids):
        raise ValueError('image_ids must be distinct images of the data set')
    if len(image_ids) > COCO_MAX_IMAGES:
        raise ValueError('%d images, at most %d' % (len(image_ids), COCO_MAX_IMAGES))
    order = sorted(range(len(image_ids)), key=lambda i: image_ids[i])
    image_rank = np.zeros(len(image_ids), dtype=np.int32)
    image_rank[order] = np.arange(len(order), dtype=np.int32)
    rank_of = {image_ids[i]: int(image_rank[i]) for i in range(len(image_ids))}
    npig = np.zeros((len(cat_ids), len(area_rng)), dtype=np.int32)
    per = [dict() for _ in image_ids]                   # rank -> class -> rows, in annotation order
    for ann in gt['annotations']:
        if ann['id'] == 0:
            raise ValueError('annotation id 0: COCOeval reads a match to it as `unmatched`')
        r = rank_of.get(ann['image_id'])
        if r is None:
            continue
        k, crowd = k_of[ann['category_id']], int(bool(ann.get('iscrowd', 0)))
        area = float(ann['area'])
        if not crowd:
            npig[k] += (area_rng[:, 0] <= area) & (area <= area_rng[:, 1])
        j = cls_of.get(ann['category_id'])
        if j is not None:
            per[r].setdefault(j, []).append([float(v) for v in ann['bbox']] + [area, crowd])
    rows, label, off = [], [], [0]
    for r in range(len(image_ids)):
        for j in sorted(per[r]):
            if len(per[r][j]) > COCO_MAX_GT_PER_SEGMENT:
                raise ValueError('%d boxes of category %r in image %r, at most %d'
                                 % (len(per[r][j]), category_ids[j], image_ids[order[r]], COCO_MAX_GT_PER_SEGMENT))
            rows.extend(per[r][j])
            label.extend([j] * len(per[r][j]))
        off.append(len(rows))
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    cat_rank = np.asarray([-1] + [k_of[c] for c in fg], dtype=np.int32)
    return COCOGroundTruth(np.ascontiguousarray(rows[:, :4]), np.ascontiguousarray(rows[:, 4]),
                           rows[:, 5].astype(np.uint8), np.asarray(label, dtype=np.int32),
                           np.asarray(off, dtype=np.int32), npig, image_ids, image_rank, cat_ids, cat_rank,
                           [c.get('name', str(c['id'])) for c in cats], area_rng)


def _coco_segment_rows(dets, packed):
    """all_boxes[cls][img] or (out_dets [N,T,cap,5], out_count [N,T]) by data set position -> a function
    (position, class index) -> float32 [k,5]."""
    if isinstance(dets, tuple):
        rows, count = np.asarray(dets[0], dtype=np.float32), np.asarray(dets[1])
        return lambda i, j: rows[i, j - 1, :max(int(count[i, j - 1]), 0)]
    return lambda i, j: np.asarray(dets[j][i], dtype=np.float32).reshape(-1, 5)


def coco_bbox_iou(d, g, crowd):
    """maskApi.c bbIou:109-120 on [x, y, w, h] boxes: float64 [D,G]."""
    d, g = d[:, None, :], g[None, :, :]
    w = np.minimum(d[..., 2] + d[..., 0], g[..., 2] + g[..., 0]) - np.maximum(d[..., 0], g[..., 0])
    h = np.minimum(d[..., 3] + d[..., 1], g[..., 3] + g[..., 1]) - np.maximum(d[..., 1], g[..., 1])
    da, ga = d[..., 2] * d[..., 3], g[..., 2] * g[..., 3]
    i = w * h
    u = np.where(np.asarray(crowd, dtype=bool)[None, :], da, (da + ga) - i)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where((w <= 0) | (h <= 0), 0., i / u)


def _coco_match_segment(ious, crowd, gt_ignore, det_out, thr):
    """cocoeval.py:256-299 (evaluateImg) for every (threshold, area range) pair at once; the walks over detections and
    over ground-truth positions stay serial.  ious [D,G]; crowd bool [G]; gt_ignore bool [A,G]; det_out bool [A,D]
    (detection area outside the range); thr [T] already clamped -> (matched, ignored) bool [T,A,D]."""
    D, G = ious.shape
    T, A = len(thr), len(gt_ignore)
    order = np.argsort(gt_ignore, axis=1, kind='stable')                # ignored boxes last, per area range
    ig = np.take_along_axis(gt_ignore, order, axis=1)                   # [A,G] by walk position
    cr = crowd[order]
    taken = np.zeros((T, A, G), dtype=bool)
    matched = np.zeros((T, A, D), dtype=bool)
    ignored = np.zeros((T, A, D), dtype=bool)
    rows = np.arange(A)
    for d in range(D):
        iou = np.repeat(thr[:, None], A, axis=1)
        m = np.full((T, A), -1)
        regular = np.zeros((T, A), dtype=bool)          # holds a match to a box that is not ignored
        stopped = np.zeros((T, A), dtype=bool)
        for p in range(G):
            v = ious[d, order[:, p]][None, :]
            skip = taken[:, :, p] & ~cr[None, :, p]
            stopped |= ~skip & regular & ig[None, :, p]
            act = ~stopped & ~skip & ~(v < iou)
            iou = np.where(act, v, iou)
            m = np.where(act, p, m)
            regular = np.where(act, ~ig[None, :, p], regular)
        hit = m >= 0
        matched[:, :, d] = hit
        ignored[:, :, d] = np.where(hit, ig[rows[None, :], np.maximum(m, 0)], det_out[None, :, d])
        tt, aa = np.nonzero(hit)
        taken[tt, aa, m[tt, aa]] = True
    return matched, ignored


def coco_eval_arrays(dets, packed, iou_thrs=None, rec_thrs=None, area_rng=None, max_dets=(1, 10, 100)):
    """COCOeval(...,'bbox').evaluate() + accumulate() -> (precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M]),
    float64, -1 for absent entries, every step restated operation for operation.

    dets: all_boxes[cls][img] (float32 [k,5] rows [x1,y1,x2,y2,s], img = position in packed.image_ids) or the pair
    (out_dets [N,T,cap,5], out_count [N,T]).  A row becomes [x1, y1, x2-x1+1, y2-y1+1] and a score in float64
    (data/coco.py:242-258), its area w*h (loadRes).  Per (image, category): stable sort of -score, cut at max_dets[-1];
    IoU = bbIou; per area range the ground truth is stably reordered with ignored boxes (crowd, or annotation area
    outside the range) last and the greedy walk of evaluateImg run: threshold min(t, 1-1e-10), a matched non-crowd box
    is skipped, the walk breaks on an ignored box once it holds a regular match, an IoU equal to the threshold matches,
    the last best box wins; an unmatched detection whose area is outside the range is ignored.  Per (k, a, m): the first
    m rows of each image in ascending image id, stable sort of -score, integer tp / fp sums, rc = tp/npig,
    pr = tp/(fp+tp+np.spacing(1)), the right-to-left envelope, searchsorted(rc, rec_thrs, 'left') filled until the
    first index equal to the number of rows."""
    d_iou, d_rec, d_area, _ = coco_default_params()
    iou_thrs = d_iou if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64)
    rec_thrs = d_rec if rec_thrs is None else np.asarray(rec_thrs, dtype=np.float64)
    area_rng = packed.area_rng if area_rng is None else np.asarray(area_rng, dtype=np.float64).reshape(-1, 2)
    if not np.array_equal(area_rng, packed.area_rng):
        raise ValueError('area_rng differs from the one the ground truth was packed with (its npig depends on it)')
    if np.any(np.diff(rec_thrs) < 0):
        raise ValueError('rec_thrs must be ascending (the fill of accumulate() stops at the first miss)')
    max_dets = sorted(int(m) for m in max_dets)
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(packed.cat_ids), len(area_rng), len(max_dets)
    thr = np.minimum(iou_thrs, 1 - 1e-10)
    rows_of = _coco_segment_rows(dets, packed)
    N, ncls = len(packed.image_ids), len(packed.cat_rank)
    position = np.argsort(packed.image_rank)            # rank -> data set position
    # evaluate(): per category, the per-image results in ascending image id
    per_k = [[] for _ in range(K)]                      # (score [D], matched [T,A,D], ignored [T,A,D])
    for r in range(N):
        a0, a1 = int(packed.off[r]), int(packed.off[r + 1])
        for j in range(1, ncls):
            row = rows_of(int(position[r]), j)
            if len(row) == 0:
                continue
            row = row.astype(np.float64)
            keep = np.argsort(-row[:, 4], kind='stable')[:max_dets[-1]]
            row = row[keep]
            box = np.stack([row[:, 0], row[:, 1], row[:, 2] - row[:, 0] + 1, row[:, 3] - row[:, 1] + 1], axis=1)
            d_area_ = box[:, 2] * box[:, 3]
            det_out = (d_area_[None, :] < area_rng[:, :1]) | (d_area_[None, :] > area_rng[:, 1:])
            sel = np.flatnonzero(packed.label[a0:a1] == j) + a0
            if len(sel):
                crowd = packed.iscrowd[sel].astype(bool)
                g_area = packed.area[sel]
                gt_ignore = crowd[None, :] | (g_area[None, :] < area_rng[:, :1]) | (g_area[None, :] > area_rng[:, 1:])
                matched, ignored = _coco_match_segment(coco_bbox_iou(box, packed.boxes[sel], crowd), crowd, gt_ignore,
                                                       det_out, thr)
            else:
                matched = np.zeros((T, A, len(row)), dtype=bool)
                ignored = np.repeat(det_out[None], T, axis=0)
            per_k[int(packed.cat_rank[j])].append((row[:, 4], matched, ignored))
    # accumulate()
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        for a in range(A):
            npig = int(packed.npig[k, a])
            if npig == 0:
                continue
            for m, max_det in enumerate(max_dets):
                E = per_k[k]
                dt_scores = np.concatenate([e[0][:max_det] for e in E]) if E else np.zeros(0)
                inds = np.argsort(-dt_scores, kind='mergesort')
                sorted_scores = dt_scores[inds]
                dtm = np.concatenate([e[1][:, a, :max_det] for e in E], axis=1)[:, inds] if E else np.zeros((T, 0), bool)
                dt_ig = np.concatenate([e[2][:, a, :max_det] for e in E], axis=1)[:, inds] if E else np.zeros((T, 0), bool)
                tp_sum = np.cumsum(dtm & ~dt_ig, axis=1).astype(np.float64)
                fp_sum = np.cumsum(~dtm & ~dt_ig, axis=1).astype(np.float64)
                nd = len(inds)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]          # pr[i-1] = max(pr[i-1], pr[i]) from the right
                    at = np.searchsorted(rc, rec_thrs, side='left')
                    ok = at < nd
                    q, ss = np.zeros(R), np.zeros(R)
                    q[ok], ss[ok] = pr[at[ok]], sorted_scores[at[ok]]
                    precision[t, :, k, a, m], scores[t, :, k, a, m] = q, ss
    return precision, recall, scores


def coco_summarize(precision, recall, packed=None, iou_thrs=None, max_dets=(1, 10, 100),
                   area_labels=COCO_AREA_LABELS):
    """summarize() (cocoeval.py:422-472) + _derive_coco_results (data/coco.py:284-345) -> (results dict, stats [12]).

    stats: _summarize's own np.mean(s[s > -1]), -1 when nothing is above -1.  results: AP, AP50, AP75, APs, APm, APl
    (stats x 100) and, with `packed`, 'AP-<name>' per class of the packed category_ids from
    precision[:, :, k, 0, -1] at the class's own K position (NaN when nothing is above -1).  The reference indexes K
    by its id_map -- positions among all 80 COCO categories -- which runs past the axis whenever the annotation file
    holds fewer categories, and its own assertion about that is commented out: that indexing is not reproduced."""
    iou_thrs = coco_default_params()[0] if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64)
    max_dets = sorted(int(m) for m in max_dets)
    labels = list(area_labels)

    def _summarize(ap=1, iou_thr=None, area='all', max_det=100):
        aind = [i for i, lbl in enumerate(labels) if lbl == area]
        mind = [i for i, md in enumerate(max_dets) if md == max_det]
        s = precision if ap == 1 else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    stats = np.zeros((12,))
    stats[0] = _summarize(1)
    stats[1] = _summarize(1, iou_thr=.5, max_det=max_dets[2])
    stats[2] = _summarize(1, iou_thr=.75, max_det=max_dets[2])
    stats[3] = _summarize(1, area='small', max_det=max_dets[2])
    stats[4] = _summarize(1, area='medium', max_det=max_dets[2])
    stats[5] = _summarize(1, area='large', max_det=max_dets[2])
    stats[6] = _summarize(0, max_det=max_dets[0])
    stats[7] = _summarize(0, max_det=max_dets[1])
    stats[8] = _summarize(0, max_det=max_dets[2])
    stats[9] = _summarize(0, area='small', max_det=max_dets[2])
    stats[10] = _summarize(0, area='medium', max_det=max_dets[2])
    stats[11] = _summarize(0, area='large', max_det=max_dets[2])
    results = {metric: float(stats[idx] * 100) for idx, metric in enumerate(['AP', 'AP50', 'AP75', 'APs', 'APm', 'APl'])}
    if packed is not None:
        for j in range(1, len(packed.cat_rank)):
            k = int(packed.cat_rank[j])
            p = precision[:, :, k, 0, -1]
            p = p[p > -1]
            results['AP-' + packed.names[k]] = float(np.mean(p) * 100) if p.size else float('nan')
    return results, stats


class DeviceCOCOEvaluator:
    """coco_eval_arrays + coco_summarize on the device, fed batch by batch from the pipeline's own output buffers
    (ops.PostProcessor.out_dets / out_count): no results JSON, no host copy of a detection.

        ev = DeviceCOCOEvaluator(gt, category_ids, device, image_ids)
        for each batch:  ev.add(out_dets, out_count, image_index)      # one launch, no synchronisation
        results, stats = ev.finish()                                   # == coco_summarize(*coco_eval_arrays(...))

    gt / category_ids / image_ids as pack_coco_ground_truth takes them; image_index is the position in image_ids
    (default: the order of gt['images']).  The ground truth is uploaded once and the record buffer (len(image_ids) x
    per_image_cap keys and two 64-bit masks) allocated once.  per_image_cap bounds the rows one image keeps over all
    classes after the cut at 100 per class; finish() raises, never drops rows, when an image had more.  precision,
    recall and scores equal the host twin's bit for bit; the means of summarize are taken on the host from the
    downloaded arrays, so stats do too.  Feeding an image twice is refused when image_index is host data; with a device
    tensor it is not detected and the later rows replace the earlier ones."""

    def __init__(self, gt, category_ids, device, image_ids=None, per_image_cap=256, iou_thrs=None, rec_thrs=None,
                 area_rng=None, max_dets=(1, 10, 100)):
        import torch
        from . import ops
        self._torch, self._ops = torch, ops
        self.device = torch.device(device)
        d_iou, d_rec, _, _ = coco_default_params()
        self.iou_thrs = d_iou if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
        self.rec_thrs = d_rec if rec_thrs is None else np.asarray(rec_thrs, dtype=np.float64).reshape(-1)
        self.max_dets = sorted(int(m) for m in max_dets)
        self.packed = p = pack_coco_ground_truth(gt, category_ids, image_ids, area_rng)
        self.T, self.N, self.G = len(p.cat_rank) - 1, len(p.image_ids), len(p.label)
        self.K, self.A, self.n_iou = len(p.cat_ids), len(p.area_rng), len(self.iou_thrs)
        if self.T < 1 or self.N < 1:
            raise ValueError('DeviceCOCOEvaluator needs at least one foreground class and one image')
        if not (1 <= self.n_iou <= 16 and 1 <= self.A <= 4 and self.n_iou * self.A <= 64):
            raise ValueError('at most 16 IoU thresholds x 4 area ranges, 64 pairs in all')
        if not (1 <= len(self.rec_thrs) <= 128) or np.any(np.diff(self.rec_thrs) < 0):
            raise ValueError('rec_thrs must be ascending, at most 128 of them')
        if len(self.max_dets) != 3 or self.max_dets[-1] > 100 or self.max_dets[0] < 1:
            raise ValueError('max_dets must be three limits within 1 .. 100')
        self.per_image_cap = int(per_image_cap)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)                  # noqa: E731
        pad = lambda a, shape: a if len(a) else np.zeros(shape, a.dtype)                          # noqa: E731
        self.gt_boxes, self.gt_area = up(pad(p.boxes, (1, 4))), up(pad(p.area, 1))
        self.gt_iscrowd, self.gt_label, self.gt_off = up(pad(p.iscrowd, 1)), up(pad(p.label, 1)), up(p.off)
        self.image_rank, self.cat_rank, self.npig = up(p.image_rank), up(p.cat_rank[1:]), up(p.npig)
        self.iou_thrs_dev = up(np.minimum(self.iou_thrs, 1 - 1e-10))        # cocoeval.py:276
        self.area_rng_dev, self.rec_thrs_dev = up(p.area_rng), up(self.rec_thrs)
        self.max_dets_dev = up(np.asarray(self.max_dets, dtype=np.int32))
        slots = self.N * self.per_image_cap
        self.keys = torch.empty(slots, dtype=torch.int64, device=self.device)
        self.matched = torch.empty(slots, dtype=torch.int64, device=self.device)
        self.ignored = torch.empty(slots, dtype=torch.int64, device=self.device)
        self.status = torch.empty(2, dtype=torch.int32, device=self.device)
        self.acc_status = torch.empty(1, dtype=torch.int32, device=self.device)
        self.bounds = (torch.arange(self.K + 1, dtype=torch.int64) << 56).to(self.device)        # first key per category
        R, M = len(self.rec_thrs), len(self.max_dets)
        self.precision = torch.empty(self.n_iou, R, self.K, self.A, M, dtype=torch.float64, device=self.device)
        self.scores = torch.empty_like(self.precision)
        self.recall = torch.empty(self.n_iou, self.K, self.A, M, dtype=torch.float64, device=self.device)
        self._ring, self._ring_events, self._ring_pos = None, [None] * 4, 0
        self._arrays = None
        self.reset()

    def reset(self):
        """Forget every image fed so far."""
        self.keys.fill_(KEY_UNUSED)
        self.matched.zero_()
        self.ignored.zero_()
        self.status.zero_()
        self.seen = np.zeros(self.N, dtype=bool)
        self._arrays = None

    _upload_index = DeviceVOCEvaluator._upload_index

    def add(self, out_dets, out_count, image_index):
        """One pipeline batch: out_dets [B,T,cap,5], out_count [B,T] (device, as ct_postprocess_batched leaves them),
        image_index [B] = position of each image in image_ids, -1 for a padding image (its rows are never read).
        Issues ct_coco_match on the current stream and returns without synchronising."""
        torch = self._torch
        self._ops._dev(out_dets, 'out_dets')
        self._ops._dev(out_count, 'out_count', torch.int32)
        if out_dets.dim() != 4 or out_dets.shape[1] != self.T or out_dets.shape[3] != 5:
            raise ValueError('out_dets must be [B,%d,cap,5], got %s' % (self.T, tuple(out_dets.shape)))
        B, cap = out_dets.shape[0], out_dets.shape[2]
        if tuple(out_count.shape) != (B, self.T):
            raise ValueError('out_count must be [%d,%d], got %s' % (B, self.T, tuple(out_count.shape)))
        if isinstance(image_index, torch.Tensor) and image_index.is_cuda:
            index = image_index
        else:
            idx = np.ascontiguousarray(np.asarray(image_index).reshape(-1), dtype=np.int32)
            if len(idx) != B:
                raise ValueError('image_index has %d entries for a batch of %d' % (len(idx), B))
            real = idx[idx >= 0]
            if real.size and real.max() >= self.N:
                raise CtdetError('image_index %d outside the %d images of the data set' % (real.max(), self.N))
            again = np.bincount(real, minlength=self.N) + self.seen > 1
            if again.any():
                raise CtdetError('image fed twice: index %s' % np.flatnonzero(again).tolist())
            self.seen[real] = True
            index = self._upload_index(idx)
        if index.numel() != B:
            raise ValueError('image_index has %d entries for a batch of %d' % (index.numel(), B))
        self._ops.coco_match(out_dets, out_count, index, self, cap)
        self._arrays = None

    def finish(self):
        """-> (results dict, stats [12]) as coco_summarize returns them.  One look at the status words, the key sort
        (torch.sort: plumbing, the keys are unique), ct_coco_accumulate, one download of the three arrays."""
        torch = self._torch
        flags, most = self.status.tolist()
        if flags & 1:
            raise CtdetError('an image keeps %d detection rows, per_image_cap is %d: construct the evaluator with '
                             'per_image_cap >= %d' % (most, self.per_image_cap, most))
        if flags & 2:
            raise CtdetError('ct_coco_match met an image index, a ground-truth offset or a category out of range, or '
                             'more than %d boxes in one (image, category)' % COCO_MAX_GT_PER_SEGMENT)
        if flags & 4:
            raise CtdetError('ct_coco_match met a NaN score')
        sorted_keys, order = torch.sort(self.keys)
        off = torch.searchsorted(sorted_keys, self.bounds)
        self.acc_status.zero_()
        self._ops.coco_accumulate(self.keys, self.matched, self.ignored, order, off, self.npig, self.max_dets_dev,
                                  self.n_iou, self.rec_thrs_dev, self.precision, self.recall, self.scores,
                                  self.acc_status)
        arrays = tuple(a.cpu().numpy() for a in (self.precision, self.recall, self.scores))
        if int(self.acc_status.item()):
            raise CtdetError('ct_coco_accumulate met an offset or a permutation entry out of range')
        self._arrays = arrays
        return coco_summarize(arrays[0], arrays[1], self.packed, self.iou_thrs, self.max_dets)

    def arrays(self):
        """(precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M]) as coco_eval_arrays returns them; after
        finish()."""
        if self._arrays is None:
            raise CtdetError('arrays() needs finish() after the last add()')
        return self._arrays


def detection_collate(batch):
    """data/voc0712.py:429-451: (image tensor, [G,6] annotation array) samples -> (stacked images, list of
    float target tensors [x1,y1,x2,y2,label,weight]) -- the layout MultiBoxLoss_combined and init_reweight take."""
    import torch
    imgs, targets = [], []
    for sample in batch:
        for item in sample:
            if torch.is_tensor(item):
                imgs.append(item)
            elif isinstance(item, np.ndarray):
                targets.append(torch.from_numpy(item).float())
    return torch.stack(imgs, 0), targets
