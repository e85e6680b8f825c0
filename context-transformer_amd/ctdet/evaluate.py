"""Detection results format + PASCAL VOC evaluation for the batched pipeline.

Restates, on in-memory arrays, what the reference does through files:
  test.py:107-109,171-172           all_boxes[class][image] = float32 [k,5]; `detections.pkl`
  data/voc0712.py:351-376           comp4_det_test_<cls>.txt lines `id score x1+1 y1+1 x2+1 y2+1`
                                     formatted {:.3f} / {:.1f}  (the rounding is part of the metric)
  data/voc_eval.py:33-66            voc_ap  (VOC07 11-point and area-under-curve)
  data/voc_eval.py:67-203           voc_eval (greedy matching at IoU > 0.5 with the +1 pixel
                                     convention, `difficult` boxes ignored, duplicates = FP)
Host-side numpy like the reference; nothing here is on the device hot path.
"""
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
