"""Shared inputs of tests/test_tal_cpu.py and tests/test_gpu_tal.py: every case of the TAL matcher is built once, the numpy twin
(tests/tal_ref.py) evaluated on it once and handed out unchanged.  A case is a namespace: targets (list of [G,6] float32
tensors), priors [P,4], pred (the raw loc / conf / obj of iou_loss_cases.preds), boxes [B,P,4] and scores [B,P,C] (what the
matcher reads), topk / alpha / beta, max_gt, and ref = the twin's result.

The boxes and scores come from `detect`: 'host' is the detection expressions in torch on the CPU (for the tests that run
without a GPU), 'device' is ops.detect_fused(apply_softmax=True) downloaded -- the GPU tests hold the matcher to the twin on
the very numbers the device fed it, so softmax and exp are not part of the comparison."""
import functools
import types

import numpy as np
import torch

import atss_cases
import iou_loss_cases as cases
import tal_ref

VAR = atss_cases.VAR
PARAMS = ((13, 1.0, 6), (10, 0.5, 6), (1, 0.0, 1), (16, 2.0, 8))      # (topk, alpha, beta)
SEEDS = {'A': 5, 'A_mixup_ignored': 5, 'B': 3, 'small': 11, 'edge': 7}


def host_detect(pred, priors):
    """layers/functions/detection.py with the eval softmaxes, float32 torch ops on the CPU -> boxes [B,P,4], scores [B,P,C]."""
    loc, conf, obj = pred
    cxcy = priors[:, :2] + loc[..., :2] * VAR[0] * priors[:, 2:]
    wh = priors[:, 2:] * torch.exp(loc[..., 2:] * VAR[1])
    x1y1 = cxcy - wh / 2
    boxes = torch.cat((x1y1, x1y1 + wh), -1)
    o, q = torch.softmax(obj, -1), torch.softmax(conf, -1)
    return boxes, torch.cat((o[..., :1], o[..., 1:2] * q), -1)


def device_detect(pred, priors):
    from ctdet import ops
    dev = 'cuda:0'
    boxes, scores = ops.detect_fused(*(p.to(dev).contiguous() for p in pred), priors.to(dev).contiguous(), VAR,
                                     apply_softmax=True)
    return boxes.cpu(), scores.cpu()


@functools.lru_cache(None)
def inputs(name, detect='host'):
    """-> targets, priors, pred, boxes, scores of a named case ('A', 'A_mixup_ignored', 'B' or 'small')."""
    if name == 'small':
        pri, targets, ncls = atss_cases.small_pyramid()[0], [atss_cases.SMALL_BOXES], 5
    else:
        size, ncls, targets, _ = cases._targets(name)
        pri = atss_cases.pyramid(size)[0]
    pred = cases.preds(len(targets), pri.shape[0], ncls, SEEDS[name])
    boxes, scores = (host_detect if detect == 'host' else device_detect)(pred, pri)
    return targets, pri, pred, boxes, scores


def build(targets, pri, boxes, scores, topk, alpha, beta, max_gt=None, pred=None, name=''):
    if max_gt is None:
        max_gt = max([int(t.shape[0]) for t in targets] + [1])
    ref = tal_ref.match([t.numpy() for t in targets], pri.numpy(), boxes.numpy(), scores.numpy(), topk, alpha, beta, VAR, max_gt)
    return types.SimpleNamespace(name=name, targets=targets, priors=pri, pred=pred, boxes=boxes, scores=scores, topk=topk,
                                 alpha=alpha, beta=beta, max_gt=max_gt, ref=ref)


@functools.lru_cache(None)
def case(name, topk=13, alpha=1.0, beta=6, detect='host', max_gt=None):
    targets, pri, pred, boxes, scores = inputs(name, detect)
    return build(targets, pri, boxes, scores, topk, alpha, beta, max_gt, pred, name)


def _rows(*rows):
    return torch.tensor(rows, dtype=torch.float32).view(-1, 6)


# edge cases, one image each on VOC_512, predictions of 21 classes: name -> (targets of the image, what to do to boxes / scores)
EDGE_BOX = (0.21, 0.33, 0.55, 0.72)
EDGE_NAMES = ('empty', 'degenerate', 'tiny', 'identical', 'moved_off', 'nan_inf', 'ignored')


@functools.lru_cache(None)
def edge(name, detect='host'):
    pri = atss_cases.pyramid(512)[0]
    pred = cases.preds(1, pri.shape[0], 21, SEEDS['edge'])
    boxes, scores = (host_detect if detect == 'host' else device_detect)(pred, pri)
    boxes, scores = boxes.clone(), scores.clone()
    if name == 'empty':
        targets = torch.zeros(0, 6)
    elif name == 'degenerate':
        targets = _rows((0.3, 0.2, 0.3, 0.6, 2, 1.0), (0.5, 0.5, 0.8, 0.9, 4, 1.0))
    elif name == 'tiny':                              # contains no prior centre of any level
        targets = _rows(atss_cases.TINY)
    elif name == 'identical':                         # the same box and class twice: the same metrics, every prior contested
        targets = _rows(EDGE_BOX + (2, 1.0), EDGE_BOX + (2, 0.5))
    elif name == 'moved_off':                         # no predicted box touches the box: u = 0 everywhere
        targets = _rows(EDGE_BOX + (3, 1.0))
        boxes += 10.0
    elif name == 'nan_inf':
        targets = _rows(EDGE_BOX + (3, 1.0), (0.5, 0.1, 0.9, 0.4, 6, 1.0))
        boxes[0, 0::7] = float('nan')
        boxes[0, 1::7] = torch.tensor([-float('inf'), -float('inf'), float('inf'), float('inf')])
        boxes[0, 2::7, 2] = float('inf')
        scores[0, 3::7] = float('nan')
        scores[0, 4::7] = float('inf')
    elif name == 'ignored':                           # label -1: ranked by 1 - background, weight carried through
        targets = _rows(EDGE_BOX + (-1, 0.37))
    else:
        raise KeyError(name)
    return build([targets], pri, boxes, scores, 13, 1.0, 6, name=name)
