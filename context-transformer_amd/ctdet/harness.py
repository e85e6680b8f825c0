"""Batched evaluation harness: test.py:do_test (test.py:96-175) with the per-image loop replaced
by whole batches through DetectionPipeline.

Keeps the reference's dataset protocol (`len(dataset)`, `dataset.pull_image(i)` -> HxWx3 uint8,
`dataset.evaluate_detections(all_boxes, save_folder)`) and its outputs (all_boxes[cls][img],
`detections.pkl`).  The ragged last batch is padded with zero images whose results are dropped.
"""
import os

import torch

from . import evaluate
from .pipeline import DetectionPipeline


def detect_dataset(net, priors, dataset, transform, num_fg, batch=32, max_per_image=200, thresh=0.01,
                   force_cpu_rule=False, progress=None, evaluator=None, keep_boxes=True, nms_method='hard',
                   soft_sigma=0.5, soft_score_threshold=0.001, tta=None, box_vote=None, matrix_pre_top=1024):
    """-> all_boxes[cls][img] (cls 0 = background, empty lists as in test.py:107-108).

    evaluator: an evaluate.DeviceVOCEvaluator or evaluate.DeviceCOCOEvaluator over this data set (image i of the data
    set = its image_ids[i]) -- anything with add(out_dets, out_count, image_index) and finish(); every batch's device output is handed to evaluator.add, the padding images of the ragged last batch as -1.
    keep_boxes=False: no host copy of the detections at all -- no per-batch synchronisation -- and None is returned;
    the post-processing's overflow flag is collected on the device and looked at once, after the last batch.
    nms_method / soft_sigma / soft_score_threshold / matrix_pre_top: DetectionPipeline's ('linear' / 'gaussian' = soft-NMS
    on the device, 'matrix_linear' / 'matrix_gaussian' = Matrix NMS on the best matrix_pre_top candidates of a class).
    tta / box_vote: DetectionPipeline's ('hflip' = a second pass on the mirrored batch; box voting at that IoU threshold)."""
    n = len(dataset)
    all_boxes = [[[] for _ in range(n)] for _ in range(num_fg + 1)] if keep_boxes else None
    if n == 0:
        return all_boxes
    pipe = DetectionPipeline(net, priors, batch, num_fg, conf_thresh=thresh, max_per_image=max_per_image,
                             force_cpu_rule=force_cpu_rule, nms_method=nms_method, soft_sigma=soft_sigma,
                             soft_score_threshold=soft_score_threshold, tta=tta, box_vote=box_vote,
                             matrix_pre_top=matrix_pre_top)
    dev = pipe.device
    overflowed = None if keep_boxes else torch.zeros_like(pipe.post.overflow)
    x = torch.zeros(batch, 3, net.size, net.size, device=dev)
    for start in range(0, n, batch):
        m = min(batch, n - start)
        wh = torch.ones(batch, 2)
        imgs = [dataset.pull_image(start + k) for k in range(m)]
        for k, img in enumerate(imgs):
            wh[k, 0], wh[k, 1] = img.shape[1], img.shape[0]
        if hasattr(transform, 'batch'):                 # device transform: one launch per batch
            transform.batch(imgs, out=x[:m])
        else:
            for k, img in enumerate(imgs):
                x[k].copy_(transform(img), non_blocking=True)
        if m < batch:
            x[m:].zero_()
        out_dets, out_count = pipe.run(x, image_wh=wh)
        if evaluator is not None:
            evaluator.add(out_dets, out_count, [start + k if k < m else -1 for k in range(batch)])
        if keep_boxes:
            per_image = pipe.results()
            for k in range(m):
                for j in range(1, num_fg + 1):
                    all_boxes[j][start + k] = per_image[k][j]
        else:
            overflowed |= pipe.post.overflow
        if progress is not None:
            progress(start + m, n)
    if overflowed is not None and int(overflowed.item()):
        raise evaluate.CtdetError('postprocess output capacity %d exceeded; raise out_cap' % pipe.post.cap)
    return all_boxes


def do_test(net, priors, dataset, transform, num_fg, save_folder, batch=32, max_per_image=200, thresh=0.01,
            force_cpu_rule=False, retest=False, evaluator=None, keep_boxes=True, nms_method='hard', soft_sigma=0.5,
            soft_score_threshold=0.001, tta=None, box_vote=None, matrix_pre_top=1024):
    """test.py:96-175: detect, write `detections.pkl`, hand over to the dataset's evaluator.

    With `evaluator` the second result is its finish() -- (aps, mean) of evaluate.DeviceVOCEvaluator, (results, stats)
    of evaluate.DeviceCOCOEvaluator -- instead of the data set's own evaluation; keep_boxes=False then also skips the host copies and `detections.pkl`, and the first result is None."""
    import pickle
    if retest and (evaluator is not None or not keep_boxes):
        raise ValueError('retest reads detections.pkl: it has nothing to feed a device evaluator and needs the boxes')
    if evaluator is None and not keep_boxes:
        raise ValueError('keep_boxes=False needs an evaluator: nothing would be left of the detections')
    soft = dict(nms_method=nms_method, soft_sigma=soft_sigma, soft_score_threshold=soft_score_threshold, tta=tta,
                box_vote=box_vote, matrix_pre_top=matrix_pre_top)
    os.makedirs(save_folder, exist_ok=True)
    det_file = os.path.join(save_folder, 'detections.pkl')
    if evaluator is not None:
        all_boxes = detect_dataset(net, priors, dataset, transform, num_fg, batch, max_per_image, thresh,
                                   force_cpu_rule, evaluator=evaluator, keep_boxes=keep_boxes, **soft)
        if keep_boxes:
            evaluate.save_detections(all_boxes, det_file)
        return all_boxes, evaluator.finish()
    if retest:
        with open(det_file, 'rb') as f:
            all_boxes = pickle.load(f)
    else:
        all_boxes = detect_dataset(net, priors, dataset, transform, num_fg, batch, max_per_image, thresh,
                                   force_cpu_rule, **soft)
        evaluate.save_detections(all_boxes, det_file)
    if hasattr(dataset, 'evaluate_detections'):
        return all_boxes, dataset.evaluate_detections(all_boxes, save_folder)
    return all_boxes, None
