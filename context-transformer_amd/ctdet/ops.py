"""Tensor-level wrappers over the libctdet C ABI.

torch is plumbing here (device memory + the current HIP stream); every function launches
hand-written HIP kernels through ctypes and raises if the tensors are not on a HIP device --
there is deliberately NO CPU / PyTorch fallback for these ops.
"""
import collections
import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .aug_records import (PLAN_BYTES, PLAN_DTYPE, SAMPLE_BYTES, SAMPLE_DTYPE as AUG_SAMPLE_DTYPE, TAP_BYTES, TAP_DTYPE,
                          TILE_BYTES, AugPlan, plan_records)   # noqa: F401  (AugPlan: callers of the C ABI fill it by name)
from .aug_records import AFFINE_BYTES, AFFINE_DTYPE, AffineRecord     # noqa: F401
from .aug_plan_ref import AffineParams


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.CtdetError('%s must be a tensor on the HIP device (got %s); the ctdet ops have no '
                              'CPU fallback' % (name, getattr(t, 'device', type(t))))
    if t.dtype != dtype:
        raise _lib.CtdetError('%s must be %s, got %s' % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise _lib.CtdetError('%s must be contiguous' % name)
    return C.c_void_p(t.data_ptr())


def _opt(t, name, dtype=torch.float32):
    return C.c_void_p(0) if t is None else _dev(t, name, dtype)


# ------------------------------------------------------------------ boxes
def decode(loc, priors, variances, scale=None):
    """utils/box_utils.py:184-202 on [P,4] or [B,P,4]; optional `boxes *= scale` ([4] or [B,4])."""
    batched = loc.dim() == 3
    B = loc.shape[0] if batched else 1
    P = priors.shape[0]
    out = torch.empty_like(loc)
    per_image = int(scale is not None and scale.dim() == 2)
    check(lib().ct_decode(_dev(loc, 'loc'), _dev(priors, 'priors'), B, P, float(variances[0]),
                          float(variances[1]), _opt(scale, 'scale'), per_image, _dev(out, 'out'), _stream()),
          'ct_decode')
    return out


def encode(matched, priors, variances):
    out = torch.empty_like(matched)
    check(lib().ct_encode(_dev(matched, 'matched'), _dev(priors, 'priors'), priors.shape[0],
                          float(variances[0]), float(variances[1]), _dev(out, 'out'), _stream()), 'ct_encode')
    return out


def detect_fused(loc, conf, obj, priors, variances, apply_softmax=False, scale=None, out=None):
    """layers/functions/detection.py:18-55 (+ eval softmaxes when apply_softmax, + the
    `boxes *= scale` of test.py:136 when scale ([4] or [B,4]) is given)."""
    B, P = loc.shape[0], priors.shape[0]
    Cn = conf.shape[-1]
    if out is None:
        boxes = torch.empty(B, P, 4, device=loc.device, dtype=torch.float32)
        scores = torch.empty(B, P, Cn + 1, device=loc.device, dtype=torch.float32)
    else:
        boxes, scores = out
    per_image = int(scale is not None and scale.dim() == 2)
    check(lib().ct_detect_fused(_dev(loc, 'loc'), _dev(conf, 'conf'), _dev(obj, 'obj'), _dev(priors, 'priors'),
                                B, P, Cn, float(variances[0]), float(variances[1]), int(apply_softmax),
                                _opt(scale, 'scale'), per_image,
                                _dev(boxes, 'boxes'), _dev(scores, 'scores'), _stream()), 'ct_detect_fused')
    return boxes, scores


def softmax_lastdim(x):
    out = torch.empty_like(x)
    cols = x.shape[-1]
    check(lib().ct_softmax_lastdim(_dev(x, 'x'), _dev(out, 'out'), x.numel() // cols, cols, _stream()),
          'ct_softmax_lastdim')
    return out


def jaccard(box_a, box_b, b_center_form=False):
    out = torch.empty(box_a.shape[0], box_b.shape[0], device=box_a.device, dtype=torch.float32)
    if out.numel() == 0:
        return out
    check(lib().ct_jaccard(_dev(box_a, 'box_a'), box_a.shape[0], _dev(box_b, 'box_b'), box_b.shape[0],
                           int(b_center_form), _dev(out, 'out'), _stream()), 'ct_jaccard')
    return out


def match_batched(targets, priors, threshold, variances, want_overlap=False):
    """targets: list of [G,6] tensors (x1,y1,x2,y2,label,weight) -> loc_t, conf_t, obj_t[, overlap]."""
    dev = priors.device
    B, P = len(targets), priors.shape[0]
    counts = [int(t.shape[0]) for t in targets]
    max_gt = max(max(counts), 1)
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).to(dev)
    if sum(counts) > 0:
        truths = torch.cat([t.reshape(-1, 6) for t in targets], 0).to(dev, torch.float32).contiguous()
    else:
        truths = torch.zeros(1, 6, device=dev)
    loc_t = torch.empty(B, P, 4, device=dev)
    conf_t = torch.empty(B, P, 2, device=dev)
    obj_t = torch.empty(B, P, device=dev, dtype=torch.uint8)
    overlap = torch.empty(B, P, device=dev) if want_overlap else None
    ws_bytes = lib().ct_match_workspace_bytes(B, P, max_gt)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    check(lib().ct_match_batched(_dev(truths, 'truths'), _dev(off, 'gt_off', torch.int32), B, max_gt,
                                 _dev(priors, 'priors'), P, float(threshold), float(variances[0]),
                                 float(variances[1]), _dev(loc_t, 'loc_t'), _dev(conf_t, 'conf_t'),
                                 _dev(obj_t, 'obj_t', torch.uint8), _opt(overlap, 'overlap'),
                                 _dev(ws, 'ws', torch.uint8), ws_bytes, _stream()), 'ct_match_batched')
    return (loc_t, conf_t, obj_t.bool(), overlap) if want_overlap else (loc_t, conf_t, obj_t.bool())


# the device-resident form of a batch's target list: truths float32 [cap,6] and gt_off int32 [B+1] as ct_match_batched
# reads them (what AugPlanner writes), max_gt the host-known upper bound of an image's row count
PackedTargets = collections.namedtuple('PackedTargets', 'truths gt_off max_gt')


def match_packed(truths, gt_off, batch, max_gt, priors, threshold, variances, want_overlap=False):
    """match_batched on device-resident inputs: the same ct_match_batched call, no host-built offset table and no
    copy.  max_gt: an upper bound of the rows of one image, e.g. the input box count of its samples."""
    dev = priors.device
    B, P, max_gt = int(batch), priors.shape[0], max(int(max_gt), 1)
    if gt_off.numel() < B + 1:
        raise ValueError('match_packed: gt_off has %d entries, batch %d needs %d' % (gt_off.numel(), B, B + 1))
    loc_t = torch.empty(B, P, 4, device=dev)
    conf_t = torch.empty(B, P, 2, device=dev)
    obj_t = torch.empty(B, P, device=dev, dtype=torch.uint8)
    overlap = torch.empty(B, P, device=dev) if want_overlap else None
    ws_bytes = lib().ct_match_workspace_bytes(B, P, max_gt)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    check(lib().ct_match_batched(_dev(truths, 'truths'), _dev(gt_off, 'gt_off', torch.int32), B, max_gt,
                                 _dev(priors, 'priors'), P, float(threshold), float(variances[0]),
                                 float(variances[1]), _dev(loc_t, 'loc_t'), _dev(conf_t, 'conf_t'),
                                 _dev(obj_t, 'obj_t', torch.uint8), _opt(overlap, 'overlap'),
                                 _dev(ws, 'ws', torch.uint8), ws_bytes, _stream()), 'ct_match_batched')
    return (loc_t, conf_t, obj_t.bool(), overlap) if want_overlap else (loc_t, conf_t, obj_t.bool())


def check_atss(level_offsets, topk, num_priors):
    """The rules of include/ctdet.h (ct_atss_match_batched) on the host -> (offsets as a list of ints, topk); ValueError."""
    if level_offsets is None:
        raise ValueError("matcher='atss' needs level_offsets (PriorBox.level_offsets())")
    off = [int(o) for o in level_offsets]
    if len(off) < 2 or off[-1] != int(num_priors):
        raise ValueError('level_offsets must end at the number of priors %d, got %r' % (num_priors, off))
    if int(topk) != topk or not 1 <= int(topk) <= 16:
        raise ValueError('atss_topk must be an integer in 1..16, got %r' % (topk,))
    return off, int(topk)


def _atss_call(truths, gt_off, B, max_gt, priors, level_offsets, topk, variances, want_overlap, want_stats):
    dev = priors.device
    P = priors.shape[0]
    off, topk = check_atss(level_offsets, topk, P)
    levels = (C.c_int * len(off))(*off)             # a host array: it travels in the kernel arguments
    loc_t = torch.empty(B, P, 4, device=dev)
    conf_t = torch.empty(B, P, 2, device=dev)
    obj_t = torch.empty(B, P, device=dev, dtype=torch.uint8)
    overlap = torch.empty(B, P, device=dev) if want_overlap else None
    stats = torch.empty(B, max_gt, 4, device=dev) if want_stats else None
    ws_bytes = lib().ct_atss_workspace_bytes(B, P, max_gt)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    check(lib().ct_atss_match_batched(_dev(truths, 'truths'), _dev(gt_off, 'gt_off', torch.int32), B, max_gt,
                                      _dev(priors, 'priors'), P, levels, len(off) - 1, topk, float(variances[0]),
                                      float(variances[1]), _dev(loc_t, 'loc_t'), _dev(conf_t, 'conf_t'),
                                      _dev(obj_t, 'obj_t', torch.uint8), _opt(overlap, 'overlap'), _opt(stats, 'gt_stats'),
                                      _dev(ws, 'ws', torch.uint8), ws_bytes, _stream()), 'ct_atss_match_batched')
    out = (loc_t, conf_t, obj_t.bool())
    if want_overlap:
        out += (overlap,)
    if want_stats:
        out += (stats,)
    return out


def atss_match_batched(targets, priors, level_offsets, topk, variances, want_overlap=False, want_stats=False):
    """match_batched with the ATSS rule (include/ctdet.h, ct_atss_match_batched) in place of the IoU threshold.  targets:
    list of [G,6] tensors; level_offsets: the L+1 prior offsets of the pyramid levels (PriorBox.level_offsets()); topk:
    candidates per level -> loc_t, conf_t, obj_t[, overlap][, gt_stats [B,max_gt,4]]."""
    dev = priors.device
    B = len(targets)
    counts = [int(t.shape[0]) for t in targets]
    max_gt = max(max(counts), 1)
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).to(dev)
    if sum(counts) > 0:
        truths = torch.cat([t.reshape(-1, 6) for t in targets], 0).to(dev, torch.float32).contiguous()
    else:
        truths = torch.zeros(1, 6, device=dev)
    return _atss_call(truths, off, B, max_gt, priors, level_offsets, topk, variances, want_overlap, want_stats)


def atss_match_packed(truths, gt_off, batch, max_gt, priors, level_offsets, topk, variances, want_overlap=False,
                      want_stats=False):
    """atss_match_batched on device-resident inputs, as match_packed is to match_batched: no host-built offset table and
    no copy.  An image with more than max_gt rows is matched against its first max_gt rows."""
    B, max_gt = int(batch), max(int(max_gt), 1)
    if gt_off.numel() < B + 1:
        raise ValueError('atss_match_packed: gt_off has %d entries, batch %d needs %d' % (gt_off.numel(), B, B + 1))
    return _atss_call(truths, gt_off, B, max_gt, priors, level_offsets, topk, variances, want_overlap, want_stats)


def check_tal(topk, alpha, beta):
    """The rules of include/ctdet.h (ct_tal_match_batched) on the host -> (topk, alpha2 = 2 * alpha, beta) as ints; ValueError."""
    def whole(v):
        return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and int(v) == v
    if not whole(topk) or not 1 <= int(topk) <= 16:
        raise ValueError('tal_topk must be an integer in 1..16, got %r' % (topk,))
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or alpha not in (0, 0.5, 1, 1.5, 2):
        raise ValueError('tal_alpha must be one of 0, 0.5, 1, 1.5, 2, got %r' % (alpha,))
    if not whole(beta) or not 0 <= int(beta) <= 8:
        raise ValueError('tal_beta must be an integer in 0..8, got %r' % (beta,))
    return int(topk), int(2 * alpha), int(beta)


def _tal_call(truths, gt_off, B, max_gt, priors, pred_boxes, pred_scores, topk, alpha, beta, variances, want_overlap,
              want_stats):
    dev = priors.device
    P = priors.shape[0]
    topk, alpha2, beta = check_tal(topk, alpha, beta)
    if tuple(pred_boxes.shape) != (B, P, 4):
        raise _lib.CtdetError('pred_boxes must be [%d,%d,4], got %s' % (B, P, tuple(pred_boxes.shape)))
    if pred_scores.dim() != 3 or tuple(pred_scores.shape[:2]) != (B, P):
        raise _lib.CtdetError('pred_scores must be [%d,%d,score_cols], got %s' % (B, P, tuple(pred_scores.shape)))
    loc_t = torch.empty(B, P, 4, device=dev)
    conf_t = torch.empty(B, P, 2, device=dev)
    obj_t = torch.empty(B, P, device=dev, dtype=torch.uint8)
    overlap = torch.empty(B, P, device=dev) if want_overlap else None
    stats = torch.empty(B, max_gt, 4, device=dev) if want_stats else None
    ws_bytes = lib().ct_tal_workspace_bytes(B, P, max_gt)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    check(lib().ct_tal_match_batched(_dev(truths, 'truths'), _dev(gt_off, 'gt_off', torch.int32), B, max_gt,
                                     _dev(priors, 'priors'), P, _dev(pred_boxes, 'pred_boxes'),
                                     _dev(pred_scores, 'pred_scores'), int(pred_scores.shape[2]), topk, alpha2, beta,
                                     float(variances[0]), float(variances[1]), _dev(loc_t, 'loc_t'), _dev(conf_t, 'conf_t'),
                                     _dev(obj_t, 'obj_t', torch.uint8), _opt(overlap, 'overlap'), _opt(stats, 'gt_stats'),
                                     _dev(ws, 'ws', torch.uint8), ws_bytes, _stream()), 'ct_tal_match_batched')
    out = (loc_t, conf_t, obj_t.bool())
    if want_overlap:
        out += (overlap,)
    if want_stats:
        out += (stats,)
    return out


def tal_match_batched(targets, priors, pred_boxes, pred_scores, topk, alpha, beta, variances, want_overlap=False,
                      want_stats=False):
    """match_batched with the task-aligned rule (include/ctdet.h, ct_tal_match_batched): the priors inside a box are ranked by
    score^alpha * IoU(predicted box, box)^beta and the best topk are its positives.  targets: list of [G,6] tensors;
    pred_boxes [B,P,4] and pred_scores [B,P,1+num_fg]: what detect_fused(apply_softmax=True) returns for the current
    predictions -> loc_t, conf_t, obj_t[, overlap][, gt_stats [B,max_gt,4]]."""
    dev = priors.device
    B = len(targets)
    counts = [int(t.shape[0]) for t in targets]
    max_gt = max(max(counts), 1)
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).to(dev)
    if sum(counts) > 0:
        truths = torch.cat([t.reshape(-1, 6) for t in targets], 0).to(dev, torch.float32).contiguous()
    else:
        truths = torch.zeros(1, 6, device=dev)
    return _tal_call(truths, off, B, max_gt, priors, pred_boxes, pred_scores, topk, alpha, beta, variances, want_overlap,
                     want_stats)


def tal_match_packed(truths, gt_off, batch, max_gt, priors, pred_boxes, pred_scores, topk, alpha, beta, variances,
                     want_overlap=False, want_stats=False):
    """tal_match_batched on device-resident inputs, as match_packed is to match_batched: no host-built offset table and no
    copy.  An image with more than max_gt rows is matched against its first max_gt rows."""
    B, max_gt = int(batch), max(int(max_gt), 1)
    if gt_off.numel() < B + 1:
        raise ValueError('tal_match_packed: gt_off has %d entries, batch %d needs %d' % (gt_off.numel(), B, B + 1))
    return _tal_call(truths, gt_off, B, max_gt, priors, pred_boxes, pred_scores, topk, alpha, beta, variances, want_overlap,
                     want_stats)


# ------------------------------------------------------------------ loss
def _u8(t, name):
    """The matcher's ignore mask: uint8 as ct_match_batched writes it, or the bool view match_batched returns."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return _dev(t, name, torch.uint8)


def _loc_args(priors, loc_loss, variances, num_priors):
    """The trailing (priors, loc_loss, var0, var1) of the _loc entries, or None for the entries without them: the default
    term with no priors given."""
    if loc_loss not in _lib.LOC_LOSSES:
        raise ValueError('loc_loss must be one of %s, got %r' % (', '.join(_lib.LOC_LOSSES), loc_loss))
    if priors is None:
        if loc_loss != 'smooth_l1':
            raise _lib.CtdetError('loc_loss=%r needs the priors the targets were matched against' % (loc_loss,))
        return None
    if tuple(priors.shape) != (num_priors, 4):
        raise _lib.CtdetError('priors must be [%d,4], got %s' % (num_priors, tuple(priors.shape)))
    return (_dev(priors, 'priors'), _lib.LOC_LOSSES.index(loc_loss), float(variances[0]), float(variances[1]))


def check_focal(conf_loss, focal_gamma, focal_alpha):
    """The rules of include/ctdet.h (ct_multibox_loss_fwd_terms) on the host -> (conf_loss, gamma, alpha); ValueError."""
    if conf_loss not in _lib.CONF_LOSSES:
        raise ValueError('conf_loss must be one of %s, got %r' % (', '.join(_lib.CONF_LOSSES), conf_loss))
    gamma, alpha = float(focal_gamma), float(focal_alpha)
    if not (math.isfinite(gamma) and gamma >= 0):
        raise ValueError('focal_gamma must be finite and >= 0, got %r' % (focal_gamma,))
    if not alpha <= 1:
        raise ValueError('focal_alpha must be in [0, 1], or negative for no class balancing, got %r' % (focal_alpha,))
    return conf_loss, gamma, alpha


def _loss_terms(priors, loc_loss, variances, num_priors, conf_loss, focal_gamma, focal_alpha):
    """-> (ct_loss_terms or None, the trailing arguments of the _loc entries or None).  The struct is built for
    conf_loss='focal' alone: with 'ce' the calls are the ones made before the focal form existed."""
    conf_loss, gamma, alpha = check_focal(conf_loss, focal_gamma, focal_alpha)
    extra = _loc_args(priors, loc_loss, variances, num_priors)
    if conf_loss == 'ce':
        return None, extra
    ptr, kind, var0, var1 = extra if extra is not None else (None, 0, float(variances[0]), float(variances[1]))
    return _lib.LossTerms(ptr, kind, var0, var1, _lib.CONF_LOSSES.index(conf_loss), gamma, alpha), None


def multibox_loss(loc, conf, obj, loc_t, conf_t, obj_t, num_classes, negpos_ratio, priors=None, loc_loss='smooth_l1',
                  variances=(0.1, 0.2), conf_loss='ce', focal_gamma=2.0, focal_alpha=0.25):
    """layers/modules/multibox_loss_combined.py:76-122 fused (ct_multibox_loss_fwd) -> sums [3] = un-normalised
    (loc, cls, obj) losses, n int64 [1], num_pos int64 [B], w [B,P] = weight * (pos | hard negative).
    loc_loss: 'smooth_l1' or one of 'iou', 'giou', 'diou', 'ciou' on the boxes decoded with `priors` [P,4] (centre form)
    and `variances` (include/ctdet.h, ct_multibox_loss_fwd_loc, which is called whenever priors are given).
    conf_loss: 'ce', or 'focal' for the mining-free focal terms with `focal_gamma` and `focal_alpha` (a negative alpha: no
    class balancing) through ct_multibox_loss_fwd_terms; w is then weight * (label >= 0) and negpos_ratio is not read."""
    _dev(loc, 'loc')
    dev = loc.device
    B, P = loc.shape[0], loc.shape[1]
    for t, name, last in ((loc, 'loc', 4), (conf, 'conf', num_classes - 1), (obj, 'obj', 2), (loc_t, 'loc_t', 4),
                          (conf_t, 'conf_t', 2)):
        if tuple(t.shape) != (B, P, last):
            raise _lib.CtdetError('%s must be [%d,%d,%d], got %s' % (name, B, P, last, tuple(t.shape)))
    if tuple(obj_t.shape) != (B, P):
        raise _lib.CtdetError('obj_t must be [%d,%d], got %s' % (B, P, tuple(obj_t.shape)))
    terms, extra = _loss_terms(priors, loc_loss, variances, P, conf_loss, focal_gamma, focal_alpha)
    sums = torch.empty(3, device=dev)
    n = torch.empty(1, device=dev, dtype=torch.int64)
    num_pos = torch.empty(B, device=dev, dtype=torch.int64)
    w = torch.empty(B, P, device=dev)
    ws_bytes = lib().ct_multibox_loss_workspace_bytes(B, P, int(num_classes))
    ws = torch.empty(max(ws_bytes, 1), device=dev, dtype=torch.uint8)
    args = (_dev(loc, 'loc'), _dev(conf, 'conf'), _dev(obj, 'obj'), _dev(loc_t, 'loc_t'), _dev(conf_t, 'conf_t'),
            _u8(obj_t, 'obj_t'), B, P, int(num_classes), int(negpos_ratio), _dev(sums, 'sums'),
            _dev(num_pos, 'num_pos', torch.int64), _dev(n, 'n', torch.int64), _dev(w, 'w'), _dev(ws, 'ws', torch.uint8),
            ws_bytes, _stream())
    if terms is not None:
        check(lib().ct_multibox_loss_fwd_terms(*args, C.byref(terms)), 'ct_multibox_loss_fwd_terms')
    elif extra is None:
        check(lib().ct_multibox_loss_fwd(*args), 'ct_multibox_loss_fwd')
    else:
        check(lib().ct_multibox_loss_fwd_loc(*args, *extra), 'ct_multibox_loss_fwd_loc')
    return sums, n, num_pos, w


def multibox_loss_backward(loc, conf, obj, loc_t, conf_t, obj_t, w, g, num_classes, priors=None, loc_loss='smooth_l1',
                           variances=(0.1, 0.2), conf_loss='ce', focal_gamma=2.0, focal_alpha=0.25):
    """Gradients of (g * sums).sum() w.r.t. (loc, conf, obj); g is a DEVICE [3] tensor (ct_multibox_loss_bwd, or
    ct_multibox_loss_bwd_loc when priors are given -- the same priors, loc_loss and variances as in the forward; or
    ct_multibox_loss_bwd_terms with conf_loss='focal' and the forward's focal_gamma / focal_alpha)."""
    B, P = loc.shape[0], loc.shape[1]
    terms, extra = _loss_terms(priors, loc_loss, variances, P, conf_loss, focal_gamma, focal_alpha)
    dloc, dconf, dobj = torch.empty_like(loc), torch.empty_like(conf), torch.empty_like(obj)
    args = (_dev(loc, 'loc'), _dev(conf, 'conf'), _dev(obj, 'obj'), _dev(loc_t, 'loc_t'), _dev(conf_t, 'conf_t'),
            _u8(obj_t, 'obj_t'), _dev(w, 'w'), _dev(g, 'g'), B, P, int(num_classes), _dev(dloc, 'dloc'),
            _dev(dconf, 'dconf'), _dev(dobj, 'dobj'), _stream())
    if terms is not None:
        check(lib().ct_multibox_loss_bwd_terms(*args, C.byref(terms)), 'ct_multibox_loss_bwd_terms')
    elif extra is None:
        check(lib().ct_multibox_loss_bwd(*args), 'ct_multibox_loss_bwd')
    else:
        check(lib().ct_multibox_loss_bwd_loc(*args, *extra), 'ct_multibox_loss_bwd_loc')
    return dloc, dconf, dobj


# ------------------------------------------------------------------ optimizer
def sgd_table(items, ema=False):
    """ctypes table of ct_sgd_tensor for `items` = [(param, grad, momentum_buf or None, lr, weight_decay, first_step)],
    or of ct_sgd_ema_tensor when `ema`: the same with the tensor's average as a seventh column.  Every tensor
    contiguous fp32 on the HIP device (views at any element offset are fine)."""
    struct, who = (_lib.SgdEmaTensor, 'sgd_step_ema') if ema else (_lib.SgdTensor, 'sgd_step')
    table = (struct * max(len(items), 1))()
    for i, (p, g, buf, lr, wd, first, *avg) in enumerate(items):
        n = p.numel()
        if g.numel() != n or (buf is not None and buf.numel() != n) or any(e.numel() != n for e in avg):
            raise _lib.CtdetError('%s: tensor %d has %d elements, its grad %d, its momentum buffer %s%s'
                                  % (who, i, n, g.numel(), None if buf is None else buf.numel(),
                                     ''.join(', its average %d' % e.numel() for e in avg)))
        table[i] = struct(_dev(p, 'param').value, _dev(g, 'grad').value, _opt(buf, 'momentum_buf').value, n, lr, wd,
                          int(bool(first)), *[_dev(e, 'ema').value for e in avg])
    return table


def sgd_step(items, momentum, dampening, nesterov, grad_scale=1.0, clip_state=None):
    """torch.optim.SGD's update of every tensor of `items` (see sgd_table) in ceil(len / ct_sgd_tensors_per_launch)
    launches (ct_sgd_step); params and momentum buffers are updated in place, `first_step` makes buf := d.
    With `clip_state` (what grad_norm_clip returned) the call is ct_sgd_step_clipped: the state's coef is multiplied
    into grad_scale on the device, and a non-finite norm skips the update."""
    if not items:
        return
    table = sgd_table(items)
    if clip_state is None:
        check(lib().ct_sgd_step(table, len(items), float(momentum), float(dampening), int(bool(nesterov)),
                                float(grad_scale), _stream()), 'ct_sgd_step')
    else:
        check(lib().ct_sgd_step_clipped(table, len(items), float(momentum), float(dampening), int(bool(nesterov)),
                                        float(grad_scale), _clip_state(clip_state), _stream()), 'ct_sgd_step_clipped')


CLIP_STATE_BYTES = C.sizeof(_lib.ClipState)


def _clip_state(t):
    if t.numel() != CLIP_STATE_BYTES:
        raise _lib.CtdetError('clip state must hold %d bytes, got %d' % (CLIP_STATE_BYTES, t.numel()))
    return _dev(t, 'clip_state', torch.uint8)


def grad_table(grads):
    """ctypes table of ct_grad_tensor for contiguous fp32 device tensors (an empty tensor passes a NULL pointer)."""
    table = (_lib.GradTensor * max(len(grads), 1))()
    for i, g in enumerate(grads):
        table[i] = _lib.GradTensor(_dev(g, 'grad').value if g.numel() else None, g.numel())
    return table


def grad_norm_workspace_bytes(grads, table=None):
    """Bytes of workspace grad_norm_clip needs for `grads` (`table`: their grad_table, when the caller has it)."""
    return int(lib().ct_grad_norm_workspace_bytes(grad_table(grads) if table is None else table, len(grads)))


def grad_norm_clip(grads, max_norm, grad_scale=1.0, state=None, workspace=None, table=None):
    """ct_grad_norm_clip over `grads`: |grad_scale| * the 2-norm of all of them, and the clipping coefficient
    min(1, max_norm / (norm + 1e-6)) -- 0 when the norm is not finite -- written to the 16-byte device tensor this
    returns (uint8; `state` when given, else allocated zeroed).  No host synchronisation; read it with clip_info().
    `workspace`: a uint8 device tensor of at least grad_norm_workspace_bytes(grads), allocated when None; `table`: the
    grad_table of `grads` when the caller has built it already."""
    if table is None:
        table = grad_table(grads)
    need = 0 if workspace is not None else int(lib().ct_grad_norm_workspace_bytes(table, len(grads)))
    dev = state.device if state is not None else (grads[0].device if grads else torch.device('cuda'))
    if state is None:
        state = torch.zeros(CLIP_STATE_BYTES, device=dev, dtype=torch.uint8)
    if workspace is None:
        workspace = torch.empty(max(need, 8), device=dev, dtype=torch.uint8)
    check(lib().ct_grad_norm_clip(table, len(grads), float(grad_scale), float(max_norm),
                                  _dev(workspace, 'workspace', torch.uint8), workspace.numel(), _clip_state(state),
                                  _stream()), 'ct_grad_norm_clip')
    return state


def clip_info(state):
    """Synchronising read of a clip state -> {'norm', 'coef', 'finite', 'nonfinite'}."""
    s = _lib.ClipState.from_buffer_copy(state.cpu().numpy().tobytes())
    return {'norm': float(s.norm), 'coef': float(s.coef), 'finite': bool(s.finite), 'nonfinite': int(s.nonfinite)}


# ------------------------------------------------------------------ weight averaging
EMA_STATE_BYTES = C.sizeof(_lib.EmaState)


def _ema_state(t):
    if not isinstance(t, torch.Tensor) or t.numel() != EMA_STATE_BYTES:
        raise _lib.CtdetError('ema state must be a uint8 tensor of %d bytes, got %s'
                              % (EMA_STATE_BYTES, t.numel() if isinstance(t, torch.Tensor) else type(t)))
    return _dev(t, 'ema_state', torch.uint8)


def ema_begin(state, decay, warmup=0.0, clip_state=None):
    """ct_ema_begin on the 16-byte device tensor `state` (uint8, zeroed once by the caller): opens one update with the
    decay min(decay, (1 + n) / (warmup + n)) (warmup 0: `decay`), or -- when `clip_state` (what grad_norm_clip
    returned) says the step is skipped -- marks it as not applied and leaves the count alone.  No synchronisation."""
    check(lib().ct_ema_begin(_ema_state(state), float(decay), float(warmup),
                             None if clip_state is None else _clip_state(clip_state), _stream()), 'ct_ema_begin')
    return state


def sgd_step_ema(items, momentum, dampening, nesterov, grad_scale, ema_state, clip_state=None):
    """sgd_step over `items` (see sgd_table, with the average as the seventh column) that also moves each tensor's average towards the new parameter value
    in the same pass (ct_sgd_step_ema), with the decay ema_begin left in `ema_state`.  A step `clip_state` skips, or
    one ema_begin did not open, leaves the averages alone."""
    if not items:
        return
    check(lib().ct_sgd_step_ema(sgd_table(items, ema=True), len(items), float(momentum), float(dampening),
                                int(bool(nesterov)), float(grad_scale),
                                None if clip_state is None else _clip_state(clip_state), _ema_state(ema_state),
                                _stream()), 'ct_sgd_step_ema')


def _pair_table(struct, pairs, what):
    table = (struct * max(len(pairs), 1))()
    for i, (a, b) in enumerate(pairs):
        if a.numel() != b.numel():
            raise _lib.CtdetError('%s: pair %d has %d and %d elements' % (what, i, a.numel(), b.numel()))
        if a.numel():                           # an empty tensor passes NULL pointers, as in grad_table
            table[i] = struct(_dev(a, what + ' tensor').value, _dev(b, what + ' tensor').value, a.numel())
    return table


def ema_update(pairs, ema_state):
    """ema := d * ema + (1 - d) * src for every (ema, src) of `pairs` (ct_ema_update), contiguous fp32 device tensors,
    with the decay ema_begin left in `ema_state`; nothing is written when that update was not opened."""
    if not pairs:
        return
    check(lib().ct_ema_update(_pair_table(_lib.EmaTensor, pairs, 'ema_update'), len(pairs), _ema_state(ema_state),
                              _stream()), 'ct_ema_update')


def tensor_swap(pairs):
    """Exchanges the contents of a and b for every (a, b) of `pairs` in place (ct_tensor_swap).  The tensors' version
    counters are the caller's business (torch.autograd.graph.increment_version)."""
    if not pairs:
        return
    check(lib().ct_tensor_swap(_pair_table(_lib.SwapTensor, pairs, 'tensor_swap'), len(pairs), _stream()),
          'ct_tensor_swap')


def ema_info(state):
    """Synchronising read of an ema state -> {'updates', 'decay', 'applied'}."""
    s = _lib.EmaState.from_buffer_copy(state.cpu().numpy().tobytes())
    return {'updates': int(s.updates), 'decay': float(s.decay), 'applied': bool(s.applied)}


# ------------------------------------------------------------------ AdamW
ADAM_STATE_BYTES = C.sizeof(_lib.AdamState)
ADAM_STATE_DTYPE = np.dtype([('beta1_pow', '<f8'), ('beta2_pow', '<f8'), ('step', '<i4'), ('applied', '<i4'),
                             ('bc1', '<f4'), ('rs2', '<f4')])        # ct_adam_state


def _adam_states(t):
    if not isinstance(t, torch.Tensor) or t.numel() % ADAM_STATE_BYTES:
        raise _lib.CtdetError('adam states must be a uint8 tensor of a multiple of %d bytes, got %s'
                              % (ADAM_STATE_BYTES, t.numel() if isinstance(t, torch.Tensor) else type(t)))
    return _dev(t, 'adam_states', torch.uint8)


def adamw_begin(states, indices, beta1, beta2, clip_state=None):
    """ct_adamw_begin on the records `indices` (distinct ints) of `states`, a uint8 device tensor of ADAM_STATE_BYTES
    per record that the caller zeroed once: each record's beta powers, step count and bias corrections advance by one
    step, or -- when `clip_state` (what grad_norm_clip returned) says the step is skipped -- the record is marked as
    not applied and keeps everything else.  No synchronisation."""
    n = len(indices)
    ptr = _adam_states(states)
    slots = states.numel() // ADAM_STATE_BYTES
    if any(i >= slots for i in indices):        # the library cannot know how many records the tensor holds
        raise _lib.CtdetError('adamw_begin: record %d of %d' % (max(indices), slots))
    table = (C.c_int * max(n, 1))(*indices)
    check(lib().ct_adamw_begin(ptr, table, n, float(beta1), float(beta2),
                               None if clip_state is None else _clip_state(clip_state), _stream()), 'ct_adamw_begin')
    return states


def adamw_table(items, states, ema=False):
    """ctypes table of ct_adamw_tensor for `items` = [(param, grad, exp_avg, exp_avg_sq, record, lr, weight_decay)]
    -- `record` is the tensor's position in `states` -- with the tensor's average as an eighth column when `ema`.
    Every tensor contiguous fp32 on the HIP device (views at any element offset are fine)."""
    base = _adam_states(states).value
    slots = states.numel() // ADAM_STATE_BYTES
    table = (_lib.AdamwTensor * max(len(items), 1))()
    for i, (p, g, m, v, slot, lr, wd, *avg) in enumerate(items):
        n = p.numel()
        if len(avg) != int(bool(ema)):
            raise _lib.CtdetError('adamw_step: tensor %d comes %s an average' % (i, 'with' if avg else 'without'))
        if any(t.numel() != n for t in (g, m, v, *avg)):
            raise _lib.CtdetError('adamw_step: tensor %d has %d elements, its grad %d, its moments %d and %d%s'
                                  % (i, n, g.numel(), m.numel(), v.numel(),
                                     ''.join(', its average %d' % e.numel() for e in avg)))
        if not 0 <= slot < slots:
            raise _lib.CtdetError('adamw_step: tensor %d names record %d of %d' % (i, slot, slots))
        table[i] = _lib.AdamwTensor(_dev(p, 'param').value, _dev(g, 'grad').value, _dev(m, 'exp_avg').value,
                                    _dev(v, 'exp_avg_sq').value, _dev(avg[0], 'ema').value if avg else None,
                                    base + slot * ADAM_STATE_BYTES, n, lr, wd)
    return table


def adamw_step(items, beta1, beta2, eps, grad_scale, states, ema_state=None, clip_state=None):
    """torch.optim.AdamW's update (amsgrad=False, maximize=False) of every tensor of `items` (see adamw_table) in
    ceil(len / ct_adamw_tensors_per_launch) launches (ct_adamw_step), with the bias corrections adamw_begin has just
    left in the tensors' records of `states`; params and both moments are updated in place.  With `ema_state` every
    item carries its average, moved towards the new parameter value in the same pass; with `clip_state` the state's
    coef is multiplied into grad_scale on the device and a non-finite norm skips the update."""
    if not items:
        return
    check(lib().ct_adamw_step(adamw_table(items, states, ema=ema_state is not None), len(items), float(beta1),
                              float(beta2), float(eps), float(grad_scale),
                              None if clip_state is None else _clip_state(clip_state),
                              None if ema_state is None else _ema_state(ema_state), _stream()), 'ct_adamw_step')


def adam_states_read(states):
    """Synchronising read of all records -> a NumPy structured array (ADAM_STATE_DTYPE), one device-to-host copy."""
    _adam_states(states)
    return np.frombuffer(states.cpu().numpy().tobytes(), dtype=ADAM_STATE_DTYPE).copy()


def adam_states_write(states, records):
    """Writes a structured array of one entry per record (ADAM_STATE_DTYPE) over `states`, one host-to-device copy."""
    _adam_states(states)
    records = np.ascontiguousarray(records, dtype=ADAM_STATE_DTYPE)
    if records.size * ADAM_STATE_BYTES != states.numel():
        raise _lib.CtdetError('adam_states_write: %d records for %d' % (records.size, states.numel() // ADAM_STATE_BYTES))
    states.copy_(torch.frombuffer(bytearray(records.tobytes()), dtype=torch.uint8))
    return states


# ------------------------------------------------------------------ NMS
def nms_sorted_host(dets_sorted, thresh, ge=False, device_id=0, plain_iou=False):
    """The `_nms` contract (utils/nms/nms_kernel.cu:91-144): host numpy [n,dim>=4] sorted by
    descending score -> ascending kept indices (int32)."""
    d = np.ascontiguousarray(dets_sorted, dtype=np.float32)
    n = d.shape[0]
    keep = np.empty(max(n, 1), dtype=np.int32)
    num = C.c_int(0)
    check(lib().ct_nms_sorted_host_mode(keep.ctypes.data_as(C.c_void_p), C.cast(C.byref(num), C.c_void_p),
                                        d.ctypes.data_as(C.c_void_p), n, d.shape[1] if n else 5,
                                        float(thresh), int(bool(ge)) | (2 if plain_iou else 0),
                                        int(device_id)), 'ct_nms_sorted_host')
    return keep[:num.value]


def nms_batched(dets, seg_off, thresh, ge=False, max_seg_len=None):
    """dets dev [total,5] (segments sorted by score), seg_off dev int32 [S+1] -> keep [total], count [S]."""
    S = seg_off.numel() - 1
    keep = torch.empty(max(dets.shape[0], 1), device=dets.device, dtype=torch.int32)
    cnt = torch.empty(S, device=dets.device, dtype=torch.int32)
    check(lib().ct_nms_batched_dev(_dev(dets, 'dets'), _dev(seg_off, 'seg_off', torch.int32), S,
                                   int(max_seg_len or dets.shape[0]), float(thresh), int(bool(ge)),
                                   _dev(keep, 'keep', torch.int32), _dev(cnt, 'cnt', torch.int32),
                                   C.c_void_p(0), 0, _stream()), 'ct_nms_batched_dev')
    return keep, cnt


SOFT_METHODS = {'hard': 0, 'linear': 1, 'gaussian': 2}


def soft_method(method):
    """'hard' / 'linear' / 'gaussian' (or the reference's 0 / 1 / 2) -> the library's method number."""
    if isinstance(method, str):
        if method not in SOFT_METHODS:
            raise ValueError('nms_method %r is not one of %s' % (method, sorted(SOFT_METHODS)))
        return SOFT_METHODS[method]
    m = int(method)
    if m not in (0, 1, 2):
        raise ValueError('soft-NMS method %r is not 0, 1 or 2' % (method,))
    return m


def soft_nms_batched(dets, seg_off, method=1, sigma=0.5, Nt=0.3, score_threshold=0.001, max_emit=0, max_seg_len=None,
                     out=None, workspace=None):
    """Soft-NMS of every segment (the device form of cpu_soft_nms): dets dev [total,5] (segments in descending score
    order), seg_off dev int32 [S+1] -> (out_rows [total,5], out_pos [total], out_count [S]); segment s emitted
    out_rows[seg_off[s] : seg_off[s] + out_count[s]] in that order, out_pos are their positions inside the segment.
    out: the three tensors to write into; workspace: uint8 tensor of ct_soft_nms_batched_workspace_bytes."""
    S = seg_off.numel() - 1
    total = dets.shape[0]
    if out is None:
        out = (torch.empty(max(total, 1), 5, device=dets.device), torch.empty(max(total, 1), device=dets.device,
                                                                              dtype=torch.int32),
               torch.empty(S, device=dets.device, dtype=torch.int32))
    rows, pos, cnt = out
    need = lib().ct_soft_nms_batched_workspace_bytes(total, S)
    if workspace is None:
        workspace = torch.empty(need, device=dets.device, dtype=torch.uint8)
    check(lib().ct_soft_nms_batched_dev(_dev(dets, 'dets'), _dev(seg_off, 'seg_off', torch.int32), S,
                                        int(total if max_seg_len is None else max_seg_len), soft_method(method),
                                        float(sigma), float(Nt), float(score_threshold), int(max_emit),
                                        _dev(rows, 'out_rows'), _dev(pos, 'out_pos', torch.int32),
                                        _dev(cnt, 'out_count', torch.int32), _dev(workspace, 'workspace', torch.uint8),
                                        workspace.numel(), _stream()), 'ct_soft_nms_batched_dev')
    return rows, pos, cnt


MATRIX_METHODS = {'matrix_linear': 1, 'matrix_gaussian': 2}


def matrix_method(method):
    """'matrix_linear' / 'matrix_gaussian' (or the library's 1 / 2) -> the Matrix NMS method number."""
    if isinstance(method, str):
        if method not in MATRIX_METHODS:
            raise ValueError('Matrix NMS method %r is not one of %s' % (method, sorted(MATRIX_METHODS)))
        return MATRIX_METHODS[method]
    m = int(method)
    if m not in (1, 2):
        raise ValueError('Matrix NMS method %r is not 1 or 2' % (method,))
    return m


def nms_method_number(nms_method):
    """A post-processing method name -> (is it a Matrix NMS method, the library's method number); ValueError otherwise."""
    if isinstance(nms_method, str) and nms_method in MATRIX_METHODS:
        return True, MATRIX_METHODS[nms_method]
    try:
        return False, soft_method(nms_method)
    except ValueError:
        if isinstance(nms_method, str):
            raise ValueError('nms_method %r is not one of %s' % (nms_method, sorted(SOFT_METHODS) + sorted(MATRIX_METHODS)))
        raise


def matrix_pre_top(pre_top):
    """The number of rows per segment Matrix NMS works on: an int in 1 .. ct_matrix_nms_max_rows()."""
    top = lib().ct_matrix_nms_max_rows()
    if isinstance(pre_top, bool) or int(pre_top) != pre_top or not 0 < int(pre_top) <= top:
        raise ValueError('matrix_pre_top %r is not an integer in 1 .. %d' % (pre_top, top))
    return int(pre_top)


def matrix_nms_batched(dets, seg_off, method=1, sigma=0.5, score_threshold=0.001, pre_top=1024, max_emit=0,
                       max_seg_len=None, out=None, workspace=None):
    """Matrix NMS of every segment (include/ctdet.h; the device form of cpu_matrix_nms): dets dev [total,5] (segments in
    descending score order), seg_off dev int32 [S+1] -> (out_rows [total,5], out_pos [total], out_count [S]); segment s
    emitted out_rows[seg_off[s] : seg_off[s] + out_count[s]] in that order, out_pos are their positions inside the
    segment.  out: the three tensors to write into; workspace: uint8 tensor of ct_matrix_nms_batched_workspace_bytes
    (0 bytes today: None is fine)."""
    S = seg_off.numel() - 1
    total = dets.shape[0]
    if out is None:
        out = (torch.empty(max(total, 1), 5, device=dets.device), torch.empty(max(total, 1), device=dets.device,
                                                                              dtype=torch.int32),
               torch.empty(S, device=dets.device, dtype=torch.int32))
    rows, pos, cnt = out
    need = lib().ct_matrix_nms_batched_workspace_bytes(total, S)
    if workspace is None and need:
        workspace = torch.empty(need, device=dets.device, dtype=torch.uint8)
    check(lib().ct_matrix_nms_batched_dev(_dev(dets, 'dets'), _dev(seg_off, 'seg_off', torch.int32), S,
                                          int(total if max_seg_len is None else max_seg_len), matrix_method(method),
                                          float(sigma), float(score_threshold), int(pre_top), int(max_emit),
                                          _dev(rows, 'out_rows'), _dev(pos, 'out_pos', torch.int32),
                                          _dev(cnt, 'out_count', torch.int32), _opt(workspace, 'workspace', torch.uint8),
                                          0 if workspace is None else workspace.numel(), _stream()),
          'ct_matrix_nms_batched_dev')
    return rows, pos, cnt


def cpu_matrix_nms(rows_sorted, method=1, sigma=0.5, score_threshold=0.001, pre_top=1024, max_emit=0):
    """The host twin on one segment: float32 [n,5] rows in the pipeline's order -> (rows [k,5] with decayed scores in
    emission order, their sorted positions [k])."""
    d = np.ascontiguousarray(rows_sorted, dtype=np.float32).reshape(-1, 5)
    n = d.shape[0]
    rows = np.empty((max(n, 1), 5), dtype=np.float32)
    pos = np.empty(max(n, 1), dtype=np.int32)
    n_out = C.c_int(0)
    check(lib().ct_cpu_matrix_nms(d.ctypes.data_as(C.c_void_p), n, matrix_method(method), float(sigma),
                                  float(score_threshold), int(pre_top), int(max_emit), rows.ctypes.data_as(C.c_void_p),
                                  pos.ctypes.data_as(C.c_void_p), C.cast(C.byref(n_out), C.c_void_p)), 'ct_cpu_matrix_nms')
    return rows[:n_out.value].copy(), pos[:n_out.value].copy()


def cpu_nms(dets, thresh, ge=True):
    """utils/nms/cpu_nms.pyx:17-68 on a host numpy array (the reference's --cpu path)."""
    d = np.ascontiguousarray(dets, dtype=np.float32)
    n = d.shape[0]
    keep = np.empty(max(n, 1), dtype=np.int32)
    num = C.c_int(0)
    check(lib().ct_cpu_nms(d.ctypes.data_as(C.c_void_p), n, float(thresh), int(bool(ge)),
                           keep.ctypes.data_as(C.c_void_p), C.cast(C.byref(num), C.c_void_p)), 'ct_cpu_nms')
    return keep[:num.value]


def cpu_soft_nms(boxes, sigma=0.5, Nt=0.3, threshold=0.001, method=0):
    """utils/nms/cpu_nms.pyx:70-163: mutates `boxes` (float32 [n,5], C-contiguous) in place."""
    if not (isinstance(boxes, np.ndarray) and boxes.dtype == np.float32 and boxes.flags['C_CONTIGUOUS']):
        raise ValueError('cpu_soft_nms needs a C-contiguous float32 array (it is updated in place)')
    n_out = C.c_int(0)
    check(lib().ct_cpu_soft_nms(boxes.ctypes.data_as(C.c_void_p), boxes.shape[0], float(sigma), float(Nt),
                                float(threshold), int(method), C.cast(C.byref(n_out), C.c_void_p)),
          'ct_cpu_soft_nms')
    return n_out.value


TTA_MODES = (None, 'hflip')


def tta_mode(name):
    """None / 'hflip' -> the number of passes of that test-time augmentation (1 / 2)."""
    if name is not None and not isinstance(name, str) or name not in TTA_MODES:
        raise ValueError('tta %r is not one of %s' % (name, list(TTA_MODES)))
    return 1 if name is None else 2


def vote_threshold(box_vote):
    """None (no voting) or the IoU threshold of box voting, a number in (0, 1]."""
    if box_vote is None:
        return None
    if isinstance(box_vote, bool) or not isinstance(box_vote, (int, float, np.floating)) or not 0.0 < float(box_vote) <= 1.0:
        raise ValueError('box_vote %r is not None or a number in (0, 1]' % (box_vote,))
    return float(box_vote)


def hflip(x, out=None):
    """x [..., H, W] mirrored along W into `out` (a different tensor; allocated when None)."""
    if out is None:
        out = torch.empty_like(x)
    if out.shape != x.shape or out.data_ptr() == x.data_ptr():
        raise ValueError('hflip is out of place: `out` must be another tensor of the same shape')
    h, w = x.shape[-2], x.shape[-1]
    check(lib().ct_hflip_f32(_dev(x, 'x'), _dev(out, 'out'), x.numel() // (h * w), h, w, _stream()), 'ct_hflip_f32')
    return out


def tta_merge(boxes_k, scores_k, k, num_passes, mirror, scale, out):
    """Pass k's boxes [B,P,4] / scores [B,P,C] into rows [k*P, (k+1)*P) of out = (boxes [B,K*P,4], scores [B,K*P,C]);
    mirror: the pass saw the mirrored image, x1' = W_b - x2 and x2' = W_b - x1 with W_b from scale ([4] or [B,4])."""
    B, P, Cn = scores_k.shape
    boxes_m, scores_m = out
    if tuple(boxes_m.shape) != (B, num_passes * P, 4) or tuple(scores_m.shape) != (B, num_passes * P, Cn):
        raise ValueError('tta_merge: merged buffers %s / %s do not hold %d passes of %s'
                         % (tuple(boxes_m.shape), tuple(scores_m.shape), num_passes, tuple(scores_k.shape)))
    per_image = int(scale is not None and scale.dim() == 2)
    check(lib().ct_tta_merge(_dev(boxes_k, 'boxes_k'), _dev(scores_k, 'scores_k'), B, P, Cn, int(num_passes), int(k),
                             int(bool(mirror)), _opt(scale, 'scale'), per_image, _dev(boxes_m, 'boxes_merged'),
                             _dev(scores_m, 'scores_merged'), _stream()), 'ct_tta_merge')
    return out


def box_vote_workspace_bytes(batch, num_rows, num_fg, out_cap):
    return lib().ct_box_vote_workspace_bytes(batch, num_rows, num_fg, out_cap)


def box_vote(boxes, scores, out_dets, out_count, conf_thresh, vote_thresh, workspace=None):
    """Box voting on a post-processing result, in place: every row r < out_count[b,c] of out_dets [B,T,cap,5] gets the
    score-weighted mean box of the rows q of boxes [B,N,4] with scores[b,q,1+c] > conf_thresh that overlap it by at least
    vote_thresh (include/ctdet.h).  Scores, counts and order are untouched.  workspace: uint8 tensor of
    box_vote_workspace_bytes (allocated when None)."""
    B, N = boxes.shape[0], boxes.shape[1]
    T, cap = out_dets.shape[1], out_dets.shape[2]
    if tuple(scores.shape) != (B, N, T + 1) or tuple(out_count.shape) != (B, T):
        raise ValueError('box_vote: scores %s / out_count %s do not match boxes %s and out_dets %s'
                         % (tuple(scores.shape), tuple(out_count.shape), tuple(boxes.shape), tuple(out_dets.shape)))
    thr = vote_threshold(vote_thresh)
    if thr is None:
        raise ValueError('box_vote needs a threshold in (0, 1]')
    if workspace is None:
        workspace = torch.empty(box_vote_workspace_bytes(B, N, T, cap), device=boxes.device, dtype=torch.uint8)
    check(lib().ct_box_vote_batched(_dev(boxes, 'boxes'), _dev(scores, 'scores'), B, N, T, float(conf_thresh), thr, cap,
                                    _dev(out_dets, 'out_dets'), _dev(out_count, 'out_count', torch.int32),
                                    _dev(workspace, 'workspace', torch.uint8), workspace.numel(), _stream()),
          'ct_box_vote_batched')
    return out_dets


def cpu_box_vote(cand_boxes, weights, rows, vote_thresh):
    """The host twin on one segment: cand_boxes float32 [n,4] and weights float32 [n] in merged-index order; `rows`
    (float32 [m,5], C-contiguous) is updated in place, its score column untouched."""
    thr = vote_threshold(vote_thresh)
    if thr is None:
        raise ValueError('cpu_box_vote needs a threshold in (0, 1]')
    if not (isinstance(rows, np.ndarray) and rows.dtype == np.float32 and rows.flags['C_CONTIGUOUS'] and rows.ndim == 2
            and rows.shape[1] == 5):
        raise ValueError('cpu_box_vote needs C-contiguous float32 rows [m,5] (they are updated in place)')
    cb = np.ascontiguousarray(cand_boxes, dtype=np.float32).reshape(-1, 4)
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    if len(w) != len(cb):
        raise ValueError('cpu_box_vote: %d boxes, %d weights' % (len(cb), len(w)))
    check(lib().ct_cpu_box_vote(cb.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), len(cb), thr,
                                rows.ctypes.data_as(C.c_void_p), rows.shape[0]), 'ct_cpu_box_vote')
    return rows


class PostProcessor:
    """Batched test.py:136-161 on the device with persistent buffers."""

    def __init__(self, batch, num_priors, num_fg, device, out_cap=None):
        self.B, self.P, self.T = batch, num_priors, num_fg
        self.cap = int(out_cap or min(num_priors, 2048))
        self.ws_bytes = lib().ct_postprocess_workspace_bytes(batch, num_priors, num_fg)
        self.ws = torch.empty(self.ws_bytes, device=device, dtype=torch.uint8)
        self.out_dets = torch.zeros(batch, num_fg, self.cap, 5, device=device)
        self.out_count = torch.zeros(batch, num_fg, device=device, dtype=torch.int32)
        self.out_index = torch.zeros(batch, num_fg, self.cap, device=device, dtype=torch.int32)
        self.overflow = torch.zeros(1, device=device, dtype=torch.int32)
        self.soft_ws = None             # the soft-NMS entry's workspace, allocated by the first run that needs it
        self.vote_ws = None             # box voting's workspace, likewise
        self.matrix_ws = None           # the Matrix NMS entry's workspace, likewise

    def run(self, boxes, scores, conf_thresh=0.01, nms_thresh=0.45, ge=False, max_per_image=200, nms_method='hard',
            soft_sigma=0.5, soft_score_threshold=0.001, box_vote=None, matrix_pre_top=1024):
        """nms_method 'hard': greedy NMS (suppress IoU > nms_thresh, or >= with ge).  'linear' / 'gaussian': soft-NMS
        (cpu_soft_nms methods 1 / 2) with Nt = nms_thresh, sigma = soft_sigma, rows below soft_score_threshold dropped;
        `ge` does not apply to them.  'matrix_linear' / 'matrix_gaussian': Matrix NMS (cpu_matrix_nms methods 1 / 2) on
        the best matrix_pre_top candidates of every class with sigma = soft_sigma, rows below soft_score_threshold dropped;
        neither nms_thresh nor `ge` applies.  box_vote (a float in (0, 1]): after the top-k cut every row's box is replaced
        by the score-weighted mean of the candidates of its class that overlap it by at least that IoU (ops.box_vote)."""
        matrix, method = nms_method_number(nms_method)
        vote = vote_threshold(box_vote)
        if matrix:
            if self.matrix_ws is None:
                nbytes = lib().ct_postprocess_matrix_workspace_bytes(self.B, self.P, self.T)
                self.matrix_ws = torch.empty(nbytes, device=self.out_dets.device, dtype=torch.uint8)
            check(lib().ct_postprocess_batched_matrix(
                _dev(boxes, 'boxes'), _dev(scores, 'scores'), self.B, self.P, self.T, float(conf_thresh), method,
                float(soft_sigma), float(soft_score_threshold), int(matrix_pre_top), int(max_per_image), self.cap,
                _dev(self.out_dets, 'out_dets'), _dev(self.out_count, 'out_count', torch.int32),
                _dev(self.out_index, 'out_index', torch.int32), _dev(self.overflow, 'overflow', torch.int32),
                _dev(self.matrix_ws, 'matrix_ws', torch.uint8), self.matrix_ws.numel(), _stream()),
                'ct_postprocess_batched_matrix')
            return self._vote(boxes, scores, conf_thresh, vote)
        if method != 0:
            if self.soft_ws is None:
                nbytes = lib().ct_postprocess_soft_workspace_bytes(self.B, self.P, self.T)
                self.soft_ws = torch.empty(nbytes, device=self.out_dets.device, dtype=torch.uint8)
            check(lib().ct_postprocess_batched_soft(
                _dev(boxes, 'boxes'), _dev(scores, 'scores'), self.B, self.P, self.T, float(conf_thresh), method,
                float(soft_sigma), float(nms_thresh), float(soft_score_threshold), int(max_per_image), self.cap,
                _dev(self.out_dets, 'out_dets'), _dev(self.out_count, 'out_count', torch.int32),
                _dev(self.out_index, 'out_index', torch.int32), _dev(self.overflow, 'overflow', torch.int32),
                _dev(self.soft_ws, 'soft_ws', torch.uint8), self.soft_ws.numel(), _stream()),
                'ct_postprocess_batched_soft')
            return self._vote(boxes, scores, conf_thresh, vote)
        check(lib().ct_postprocess_batched(
            _dev(boxes, 'boxes'), _dev(scores, 'scores'), self.B, self.P, self.T, float(conf_thresh),
            float(nms_thresh), int(bool(ge)), int(max_per_image), self.cap, _dev(self.out_dets, 'out_dets'),
            _dev(self.out_count, 'out_count', torch.int32), _dev(self.out_index, 'out_index', torch.int32),
            _dev(self.overflow, 'overflow', torch.int32), _dev(self.ws, 'ws', torch.uint8), self.ws_bytes,
            _stream()), 'ct_postprocess_batched')
        return self._vote(boxes, scores, conf_thresh, vote)

    def _vote(self, boxes, scores, conf_thresh, vote):
        if vote is not None:
            if self.vote_ws is None:
                nbytes = box_vote_workspace_bytes(self.B, self.P, self.T, self.cap)
                self.vote_ws = torch.empty(nbytes, device=self.out_dets.device, dtype=torch.uint8)
            box_vote(boxes, scores, self.out_dets, self.out_count, conf_thresh, vote, self.vote_ws)
        return self.out_dets, self.out_count

    def to_all_boxes(self):
        """Host view in the reference's layout: all_boxes[img][cls] = float32 [k,5] (cls 0 empty)."""
        if int(self.overflow.item()):
            raise _lib.CtdetError('postprocess output capacity %d exceeded; raise out_cap' % self.cap)
        cnt = self.out_count.cpu().numpy()
        dets = self.out_dets.cpu().numpy()
        res = []
        for b in range(self.B):
            per = [np.empty((0, 5), dtype=np.float32)]
            for c in range(self.T):
                per.append(dets[b, c, :cnt[b, c]].copy())
            res.append(per)
        return res


# ------------------------------------------------------------------ VOC evaluation
def voc_match(out_dets, out_count, image_index, ev, cap):
    """ct_voc_match of one pipeline batch into the buffers of `ev` (evaluate.DeviceVOCEvaluator): the packed ground
    truth gt_boxes / gt_label / gt_difficult / gt_off, the records keys / flags and the status words."""
    check(lib().ct_voc_match(_dev(out_dets, 'out_dets'), _dev(out_count, 'out_count', torch.int32), out_dets.shape[0],
                             ev.T, int(cap), _dev(image_index, 'image_index', torch.int32), ev.N,
                             _dev(ev.gt_boxes, 'gt_boxes'), _dev(ev.gt_label, 'gt_label', torch.int32),
                             _dev(ev.gt_difficult, 'gt_difficult', torch.uint8), _dev(ev.gt_off, 'gt_off', torch.int32),
                             ev.G, ev.max_gt, float(ev.ovthresh), _dev(ev.keys, 'keys', torch.int64),
                             _dev(ev.flags, 'flags', torch.uint8), ev.per_image_cap,
                             _dev(ev.status, 'status', torch.int32), _stream()), 'ct_voc_match')


def voc_pr(ev, order, cls_off, thresholds=None):
    """ct_voc_pr over the records of `ev` in the order of the key sort: fills ev.rec / ev.prec (sorted positions) and
    ev.ap.  thresholds: host float64 array for the VOC07 rule (np.arange(0., 1.1, 0.1)), None for the area metric."""
    thr = np.ascontiguousarray(thresholds if thresholds is not None else [], dtype=np.float64)
    ev.pr_status.zero_()
    check(lib().ct_voc_pr(_dev(ev.flags, 'flags', torch.uint8), _dev(order, 'order', torch.int64), ev.flags.numel(),
                          _dev(cls_off, 'cls_off', torch.int64), _dev(ev.num_pos, 'num_pos', torch.int32), ev.T,
                          thr.ctypes.data_as(C.c_void_p), len(thr), _dev(ev.rec, 'rec', torch.float64),
                          _dev(ev.prec, 'prec', torch.float64), _dev(ev.ap, 'ap', torch.float64),
                          _dev(ev.pr_status, 'pr_status', torch.int32), _stream()), 'ct_voc_pr')


# ------------------------------------------------------------------ COCO evaluation
def coco_match(out_dets, out_count, image_index, ev, cap):
    """ct_coco_match of one pipeline batch into the buffers of `ev` (evaluate.DeviceCOCOEvaluator): the packed ground
    truth, the thresholds, the records keys / matched / ignored and the status words."""
    i32, f64 = torch.int32, torch.float64
    check(lib().ct_coco_match(_dev(out_dets, 'out_dets'), _dev(out_count, 'out_count', i32), out_dets.shape[0], ev.T,
                              int(cap), _dev(image_index, 'image_index', i32), _dev(ev.image_rank, 'image_rank', i32),
                              ev.N, _dev(ev.gt_boxes, 'gt_boxes', f64), _dev(ev.gt_area, 'gt_area', f64),
                              _dev(ev.gt_iscrowd, 'gt_iscrowd', torch.uint8), _dev(ev.gt_label, 'gt_label', i32),
                              _dev(ev.gt_off, 'gt_off', i32), ev.G, _dev(ev.cat_rank, 'cat_rank', i32),
                              _dev(ev.iou_thrs_dev, 'iou_thrs', f64), ev.n_iou, _dev(ev.area_rng_dev, 'area_rng', f64),
                              ev.A, _dev(ev.keys, 'keys', torch.int64), _dev(ev.matched, 'matched', torch.int64),
                              _dev(ev.ignored, 'ignored', torch.int64), ev.per_image_cap,
                              _dev(ev.status, 'status', i32), _stream()), 'ct_coco_match')


def coco_accumulate(keys, matched, ignored, order, cat_off, npig, max_dets, n_iou, rec_thrs, precision, recall, scores,
                    status):
    """ct_coco_accumulate over records in the order of the key sort (order None: the records are already sorted) into
    precision / scores [T,R,K,A,M] and recall [T,K,A,M] (device float64).  matched / ignored hold the 64 mask bits in
    int64 tensors (torch has no uint64 arithmetic); npig is [K,A] int32, max_dets int32, rec_thrs float64, ascending."""
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    K, A = npig.shape
    check(lib().ct_coco_accumulate(_dev(keys, 'keys', i64), _dev(matched, 'matched', i64),
                                   _dev(ignored, 'ignored', i64), _opt(order, 'order', i64), keys.numel(),
                                   _dev(cat_off, 'cat_off', i64), _dev(npig, 'npig', i32), K, A,
                                   _dev(max_dets, 'max_dets', i32), max_dets.numel(), int(n_iou),
                                   _dev(rec_thrs, 'rec_thrs', f64), rec_thrs.numel(), _dev(precision, 'precision', f64),
                                   _dev(recall, 'recall', f64), _dev(scores, 'scores', f64),
                                   _dev(status, 'acc_status', i32), _stream()), 'ct_coco_accumulate')


# ------------------------------------------------------------------ input transform
class _Staging:
    """A pinned host buffer, its device twin `dev` and the event of the last copy between them; `put` is its one
    operation.  grow: None refuses items that do not fit, a factor replaces both buffers by ones of that many times
    the need.  pad_end: the copy also moves the padding after the last item, as the image copies always have."""

    def __init__(self, device, nbytes, who, grow=None, pad_end=False):
        self.device, self.who, self.grow, self.pad_end = device, who, grow, pad_end
        self.copied = torch.cuda.Event()        # recorded after every copy: the pinned buffer is free for reuse
        self.nbytes = 0                         # of the last copy
        self._alloc(nbytes)

    def _alloc(self, nbytes):
        self.cap = nbytes
        self.host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def put(self, items):
        """Contiguous numpy arrays -> the list of their byte offsets in `dev` (multiples of 16): wait for the previous
        copy, fill the pinned buffer, enqueue ONE non-blocking H2D copy of the bytes in use, record the event."""
        self.copied.synchronize()
        offs, end = [], 0
        for a in items:
            offs.append((end + 15) // 16 * 16)
            end = offs[-1] + a.nbytes
        nb = (end + 15) // 16 * 16 if self.pad_end else end
        if self.grow is None:
            if end > self.cap:
                raise _lib.CtdetError('%s: staging capacity %d bytes exceeded' % (self.who, self.cap))
        elif nb > self.cap:
            self._alloc(int(nb * self.grow))
        for a, o in zip(items, offs):
            self.host[o:o + a.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8))
        self.nbytes = min(nb, self.cap)
        self.dev[:self.nbytes].copy_(self.host[:self.nbytes], non_blocking=True)
        self.copied.record()
        return offs


def _images(images, who):
    """The uint8 HxWx3 images of a batch as contiguous arrays."""
    arrays = [np.ascontiguousarray(img) for img in images]
    for i, a in enumerate(arrays):
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError('%s: image %d is %s %s, expected uint8 HxWx3' % (who, i, a.dtype, a.shape))
    return arrays


class Preprocessor:
    """Batched BaseTransform (data/data_augment.py:224-266) on the device: uint8 HxWx3 images of
    any size -> float32 [B,3,S,S] (bilinear resize, minus means, CHW) in one launch.
    The packed bytes go through one pinned staging buffer and one H2D copy per batch."""

    def __init__(self, size, means, device, max_batch=32, max_pixels=512 * 512):
        self.size, self.device, self.max_batch = size, torch.device(device), max_batch
        self.means = (C.c_float * 3)(*[float(m) for m in means])
        self.src = _Staging(self.device, max_batch * max_pixels * 3, 'Preprocessor', pad_end=True)
        self.meta = _Staging(self.device, max_batch * (8 + 2 * 4), 'Preprocessor')     # offsets (i64) | hw (2 x i32)

    def __call__(self, images, out=None):
        n, mb = len(images), self.max_batch
        if n == 0 or n > mb:
            raise ValueError('Preprocessor: batch of %d images (max %d)' % (n, mb))
        arrays = _images(images, 'Preprocessor')
        meta = np.zeros(4 * mb, dtype=np.int32)
        meta[:2 * mb].view(np.int64)[:n] = self.src.put(arrays)
        meta[2 * mb:2 * mb + 2 * n] = [v for a in arrays for v in a.shape[:2]]
        self.meta.put([meta])
        if out is None:
            out = torch.empty(n, 3, self.size, self.size, device=self.device, dtype=torch.float32)
        offs_d, hw_d = self.meta.dev[:8 * mb], self.meta.dev[8 * mb:]
        check(lib().ct_preproc_resize(_dev(self.src.dev, 'src', torch.uint8), _dev(offs_d, 'offsets', torch.uint8),
                                      _dev(hw_d, 'hw', torch.uint8), n,
                                      self.size, C.cast(self.means, C.c_void_p), _dev(out, 'out'), _stream()),
              'ct_preproc_resize')
        return out


# ------------------------------------------------------------------ resize taps (host decisions of the augmentation)
RESIZE_TAPS = {'cubic': 4, 'lanczos4': 8}           # kind -> taps per axis; AugPlan.interp 3 and 4
INTERP_KIND = {3: 'cubic', 4: 'lanczos4'}


def resize_coeffs(x, kind):
    """float32 fractions [S] -> int16 [S, k]: OpenCV's bicubic (A = -0.75) / Lanczos4 weights in float32, as 11-bit
    fixed point (round half to even, saturated).  The Lanczos4 kernel is OpenCV's sin/cos form, trigonometry in
    double; that double sin/cos is why this is host work (include/ctdet.h)."""
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    if kind == 'cubic':
        A, xp, xm = f32(-0.75), x + f32(1), f32(1) - x
        c0 = ((A * xp - f32(5) * A) * xp + f32(8) * A) * xp - f32(4) * A
        c1 = ((A + f32(2)) * x - (A + f32(3))) * x * x + f32(1)
        c2 = ((A + f32(2)) * xm - (A + f32(3))) * xm * xm + f32(1)
        w = np.stack([c0, c1, c2, f32(1) - c0 - c1 - c2], 1)
    elif kind == 'lanczos4':
        s = 0.70710678118654752440084436210485
        cs = np.array([[1, 0], [-s, -s], [0, 1], [s, -s], [-1, 0], [s, s], [0, -1], [-s, s]])
        y0 = -(x.astype(np.float64) + 3.0) * np.pi * 0.25
        s0, c0 = np.sin(y0), np.cos(y0)
        t = (x + f32(3))[:, None] - np.arange(8, dtype=f32)[None, :]           # float32, like OpenCV's `x+3-i`
        y = -t.astype(np.float64) * np.pi * 0.25
        near = np.abs(t) < f32(1e-6)
        with np.errstate(divide='ignore', invalid='ignore'):
            w = ((cs[None, :, 0] * s0[:, None] + cs[None, :, 1] * c0[:, None]) / (y * y)).astype(f32)
        w[near] = f32(1e30)
        total = np.zeros(len(x), dtype=f32)
        for i in range(8):                          # float32 sum in tap order
            total = total + w[:, i]
        w = w * (f32(1) / total)[:, None]
    else:
        raise ValueError('resize_coeffs: kind %r (known: %s)' % (kind, sorted(RESIZE_TAPS)))
    assert w.dtype == f32
    return np.clip(np.rint(w * f32(2048)), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=4096)
def resize_taps(n_src, S, kind):
    """Taps of one axis of cv2.resize's 8-bit bicubic / Lanczos4 path, n_src source pixels -> S output pixels:
    (first int32 [S] = floor(f), ic int16 [S, k]); tap j of output d reads source index
    clamp(first[d] - (k/2 - 1) + j, 0, n_src - 1).  No edge reset of the fraction, unlike the linear filter.
    Cached per (n_src, S, kind); the arrays are read-only."""
    if kind not in RESIZE_TAPS:
        raise ValueError('resize_taps: kind %r (known: %s)' % (kind, sorted(RESIZE_TAPS)))
    scale = 1.0 / (S / float(n_src))
    f = ((np.arange(S) + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(f)
    first, ic = fl.astype(np.int32), resize_coeffs(f - fl, kind)
    first.setflags(write=False)
    ic.setflags(write=False)
    return first, ic


def tap_records(n_src, S, kind):
    """The S ct_resize_tap records of one axis: `first` unclamped at the first tap (the kernel clamps)."""
    first, ic = resize_taps(int(n_src), int(S), kind)
    rec = np.zeros(S, dtype=TAP_DTYPE)
    rec['first'] = first - (RESIZE_TAPS[kind] // 2 - 1)
    rec['c'][:, :ic.shape[1]] = ic
    return rec


class Augmenter:
    """Batched training-time augmentation (data/data_augment.py:164-221) on the device: the host hands over the
    uint8 images and one plan per image (the random decisions); ONE launch writes float32 [B,3,S,S].  A batch
    with a bicubic or Lanczos4 image (interp 3 / 4) also carries their taps and goes to ct_preproc_augment_taps."""

    def __init__(self, size, means, device, max_batch=32, max_pixels=512 * 512):
        self.size, self.device, self.max_batch = size, torch.device(device), max_batch
        self.means_f = [float(m) for m in means]
        self.means = (C.c_float * 3)(*self.means_f)
        # any image size, like the reference (COCO is 640x480): the source staging grows, never refuses
        self.src = _Staging(self.device, max_batch * max_pixels * 3, 'Augmenter', grow=1.25, pad_end=True)
        self.plans = _Staging(self.device, max_batch * PLAN_BYTES, 'Augmenter')
        self.taps = None                    # ct_resize_tap staging, allocated by the first batch that needs it

    @property
    def dev(self):
        """The device source buffer `upload` filled last (src_off counts from its start)."""
        return self.src.dev

    def __call__(self, images, plans, out=None):
        n = len(images)
        if n == 0 or n > self.max_batch or len(plans) != n:
            raise ValueError('Augmenter: batch of %d images / %d plans (max %d)' % (n, len(plans), self.max_batch))
        for i, (img, p) in enumerate(zip(images, plans)):
            if tuple(np.shape(img)[:2]) != (p['H'], p['W']):
                raise ValueError('Augmenter: image %d is %s, plan says %dx%d' % (i, np.shape(img), p['H'], p['W']))
        recs = np.zeros(n, dtype=PLAN_DTYPE)
        recs['src_off'], recs['fill'] = self.upload(images), self.means_f
        plan_records(recs, plans)
        self.plans.put([recs])
        if not any(p['interp'] in INTERP_KIND for p in plans):
            return self._render('ct_preproc_augment', self.plans.dev, n, out)
        # bicubic / Lanczos4 images: their taps are host decisions too (resize_taps), uploaded like the plans
        S = self.size
        if self.taps is None:
            self.taps = _Staging(self.device, self.max_batch * 2 * S * TAP_BYTES, 'Augmenter')
        recs_t = np.zeros((n, 2, S), dtype=TAP_DTYPE)               # images with interp 0..2 ignore theirs
        for i, p in enumerate(plans):
            kind = INTERP_KIND.get(p['interp'])
            if kind:
                recs_t[i, 0], recs_t[i, 1] = tap_records(p['exp'][0], S, kind), tap_records(p['exp'][1], S, kind)
        self.taps.put([recs_t])
        return self._render('ct_preproc_augment_taps', self.plans.dev, n, out, ('taps', self.taps.dev))

    def upload(self, images):
        """Stage and upload the images: -> int64 [n] byte offsets of the images in the source buffer (the plan's and
        ct_aug_sample's src_off).  On its own for plans the device draws itself (AugPlanner, then `render`)."""
        n = len(images)
        if n == 0 or n > self.max_batch:
            raise ValueError('Augmenter: batch of %d images (max %d)' % (n, self.max_batch))
        return np.array(self.src.put(_images(images, 'Augmenter')), dtype=np.int64)

    def _render(self, entry, plans_d, n, out, *extra):
        """The one body of the ct_preproc_augment* calls over the buffer `upload` filled: n output images from the
        plan records plans_d and the (name, uint8 tensor) tables `extra` the entry takes after them."""
        if out is None:
            out = torch.empty(n, 3, self.size, self.size, device=self.device, dtype=torch.float32)
        u8 = torch.uint8
        check(getattr(lib(), entry)(_dev(self.dev, 'src', u8), _dev(plans_d, 'plans', u8),
                                    *[_dev(t, name, u8) for name, t in extra], n, self.size,
                                    C.cast(self.means, C.c_void_p), _dev(out, 'out'), _stream()), entry)
        return out

    def render(self, plans_d, n, out=None):
        """ct_preproc_augment over n device-resident plan records (uint8 [>= n*PLAN_BYTES]) whose src_off point into
        the buffer `upload` filled.  The float filters only: tap tables are host decisions."""
        if n == 0 or plans_d.numel() < n * PLAN_BYTES:
            raise ValueError('Augmenter.render: %d plans in a buffer of %d bytes' % (n, plans_d.numel()))
        return self._render('ct_preproc_augment', plans_d, n, out)

    def render_mosaic(self, plans_d, tiles_d, n, out=None):
        """ct_preproc_augment_mosaic: n images, each composed of four device-resident plan records (uint8
        [>= 4n*PLAN_BYTES]) resized into their tiles (uint8 [>= 4n*TILE_BYTES], ct_mosaic_tile); what
        AugPlanner.mosaic returns."""
        if n == 0 or plans_d.numel() < 4 * n * PLAN_BYTES or tiles_d.numel() < 4 * n * TILE_BYTES:
            raise ValueError('Augmenter.render_mosaic: %d images, %d plan bytes, %d tile bytes'
                             % (n, plans_d.numel(), tiles_d.numel()))
        return self._render('ct_preproc_augment_mosaic', plans_d, n, out, ('tiles', tiles_d))


AUG_STATUS_BAD_SAMPLE, AUG_STATUS_ROWS_DROPPED = 1, 2


class AugPlanner:
    """The augmentation decisions and box targets of a batch on the device (ct_aug_plan, two launches): the host
    hands over one ct_aug_sample per sample and the pixel boxes -- through one pinned staging buffer and one H2D copy,
    as Augmenter stages its images -- and gets the plan records ct_preproc_augment reads and a PackedTargets that
    ct_match_batched reads.  No host synchronisation unless `check()` is called."""

    def __init__(self, device, seed, p_expand, interp_of_draw, fill, max_samples=64, max_boxes=4096):
        self.device, self.seed, self.p_expand = torch.device(device), int(seed) & (2 ** 64 - 1), float(p_expand)
        if len(interp_of_draw) != 5 or len(fill) != 3:
            raise ValueError('AugPlanner: interp_of_draw has 5 entries and fill 3')
        self.interp = (C.c_int * 5)(*[int(v) for v in interp_of_draw])
        self.fill = (C.c_float * 3)(*[float(v) for v in fill])
        # the sample records, then the float32 [x1,y1,x2,y2,label] boxes; grows to exactly what a batch needs
        self.stage = _Staging(self.device, max_samples * SAMPLE_BYTES + max_boxes * 5 * 4, 'AugPlanner', grow=1.0)
        self.status = None                  # int32 [4] on the device, of the last call
        self.upload_bytes = 0               # of the last call

    def _plan(self, entry, samples, boxes, num_images, max_gt, truths_cap, tiles=None, *geometry):
        """The one body of `__call__` and `mosaic` (which adds its `tiles` output and the (size, margin) geometry):
        normalise the inputs, upload them, allocate the outputs, call `entry` -> (plans, PackedTargets)."""
        mosaic = tiles is not None
        samples = np.ascontiguousarray(samples, dtype=AUG_SAMPLE_DTYPE)
        boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 5)
        n, total, num_images, max_gt = len(samples), len(boxes), int(num_images), int(max_gt)
        if num_images < 1 or max_gt < 1 or (n != 4 * num_images if mosaic else n == 0):
            raise ValueError('%s: %d samples, %d images, max_gt %d'
                             % ('AugPlanner.mosaic' if mosaic else 'AugPlanner', n, num_images, max_gt))
        box_off = self.stage.put([samples, boxes])[1]
        self.upload_bytes = self.stage.nbytes
        cap = max(total, 1) if truths_cap is None else int(truths_cap)
        dev, u8, i32 = self.device, torch.uint8, torch.int32
        plans = torch.empty(n * PLAN_BYTES, dtype=u8, device=dev)
        truths = torch.empty(max(cap, 1), 6, dtype=torch.float32, device=dev)
        gt_off = torch.empty(num_images + 1, dtype=i32, device=dev)
        self.status = torch.empty(4, dtype=i32, device=dev)
        ws_bytes = getattr(lib(), entry + '_workspace_bytes')(num_images if mosaic else n, max_gt)
        ws = torch.empty(ws_bytes, dtype=u8, device=dev)
        smp, bxp = _dev(self.stage.dev, 'samples', u8), C.c_void_p(self.stage.dev.data_ptr() + box_off)
        draw = (max_gt, self.seed, self.p_expand, self.interp, self.fill)
        if mosaic:
            args = (smp, num_images, bxp, total) + draw + geometry + (_dev(plans, 'plans', u8), _dev(tiles, 'tiles', u8))
        else:
            args = (smp, n, bxp, total, num_images) + draw + (_dev(plans, 'plans', u8),)
        check(getattr(lib(), entry)(*args, _dev(truths, 'truths'), cap, _dev(gt_off, 'gt_off', i32),
                                    _dev(self.status, 'status', i32), _dev(ws, 'workspace', u8), ws_bytes, _stream()), entry)
        # host-known bound of an image's rows: the boxes its samples hand in (each capped at max_gt)
        cnt = np.minimum(np.clip(samples['box_end'], 0, total) - np.clip(samples['box_begin'], 0, total), max_gt)
        img = np.arange(n) // 4 if mosaic else samples['image']
        ok = (img >= 0) & (img < num_images)
        per_image = np.bincount(img[ok], weights=np.maximum(cnt[ok], 0), minlength=1) if ok.any() else np.zeros(1)
        return plans, PackedTargets(truths, gt_off, max(int(per_image.max()), 1))

    def __call__(self, samples, boxes, num_images, max_gt, truths_cap=None):
        """samples: AUG_SAMPLE_DTYPE array [n]; boxes float32 [total,5]; max_gt: boxes per sample the kernel looks at.
        -> (plans uint8 [n*PLAN_BYTES] on the device, PackedTargets).  truths_cap defaults to the input box count,
        which the rows cannot exceed."""
        return self._plan('ct_aug_plan', samples, boxes, num_images, max_gt, truths_cap)

    def mosaic(self, samples, boxes, num_images, max_gt, size, margin, truths_cap=None):
        """ct_aug_plan_mosaic (three launches): samples AUG_SAMPLE_DTYPE [4*num_images], group-major (sample s is slot
        s % 4 of image s // 4); boxes float32 [total,5].  -> (plans uint8 [4n*PLAN_BYTES], tiles uint8 [4n*TILE_BYTES],
        PackedTargets in the output image's units), all on the device.  Staged and uploaded like `__call__`."""
        tiles = torch.empty(len(samples) * TILE_BYTES, dtype=torch.uint8, device=self.device)
        plans, packed = self._plan('ct_aug_plan_mosaic', samples, boxes, num_images, max_gt, truths_cap, tiles,
                                   int(size), int(margin))
        return plans, tiles, packed

    def check(self):
        """Read the status words of the last call (a host synchronisation) and raise when a sample was refused or a
        row dropped."""
        st = self.status.cpu().numpy()
        if st[0]:
            raise _lib.CtdetError('ct_aug_plan: status %d (%d samples refused, %d rows dropped of %d)'
                                  % (st[0], st[1], st[2], st[3]))
        return st


def affine_params(params):
    """An AffineParams, or the dict of its keyword arguments (degrees, scale, shear, translate, p, min_side,
    min_visible) -> AffineParams."""
    if isinstance(params, AffineParams):
        return params
    if isinstance(params, dict):
        return AffineParams(**params)
    raise ValueError('affine parameters: an AffineParams or a dict of its arguments, not %r' % (params,))


class AffineWarp:
    """The random affine post-stage on a rendered batch (include/ctdet.h RANDOM AFFINE): `plan` draws one record per
    image and carries the packed rows along (ct_aug_affine_plan, two launches), `warp` resamples the pixels
    (ct_preproc_warp_affine, one launch).  Everything stays on the device; no host synchronisation unless `check()`
    is called."""

    def __init__(self, device, seed, params):
        self.device, self.seed = torch.device(device), int(seed) & (2 ** 64 - 1)
        self.params = affine_params(params)
        self._struct = self.params.struct()
        self.status = None                  # int32 [4] on the device, of the last plan

    def plan(self, packed, image_ids, n, size):
        """packed: PackedTargets normalised to the size x size image; image_ids: n 64-bit ids ->
        (records uint8 [n*AFFINE_BYTES] on the device, PackedTargets).  The ids go up as one small non-blocking copy."""
        n, size = int(n), int(size)
        truths, gt_off = packed.truths, packed.gt_off
        if n < 1 or len(image_ids) != n or gt_off.numel() < n + 1 or truths.dim() != 2 or truths.shape[1] != 6:
            raise ValueError('AffineWarp.plan: %d images, %d ids, %d offsets, truths %s'
                             % (n, len(image_ids), gt_off.numel(), tuple(truths.shape)))
        ids = np.array([int(v) % 2 ** 64 for v in image_ids], dtype=np.uint64).view(np.int64)
        ids_d = torch.from_numpy(ids).to(self.device, non_blocking=True)
        rows = truths.shape[0]
        dev, u8, i32 = self.device, torch.uint8, torch.int32
        records = torch.empty(n * AFFINE_BYTES, dtype=u8, device=dev)
        truths_out = torch.empty(max(rows, 1), 6, dtype=torch.float32, device=dev)
        gt_off_out = torch.empty(n + 1, dtype=i32, device=dev)
        self.status = torch.empty(4, dtype=i32, device=dev)
        ws_bytes = lib().ct_aug_affine_plan_workspace_bytes(n, rows)
        ws = torch.empty(ws_bytes, dtype=u8, device=dev)
        check(lib().ct_aug_affine_plan(_dev(truths, 'truths'), _dev(gt_off, 'gt_off', i32), _dev(ids_d, 'image_ids', torch.int64),
                                       n, rows, size, self.seed, C.byref(self._struct), _dev(records, 'records', u8),
                                       _dev(truths_out, 'truths_out'), _dev(gt_off_out, 'gt_off_out', i32),
                                       _dev(self.status, 'status', i32), _dev(ws, 'workspace', u8), ws_bytes, _stream()),
              'ct_aug_affine_plan')
        return records, PackedTargets(truths_out, gt_off_out, packed.max_gt)

    def warp(self, x, records_d, border3, out=None):
        """x float32 [n,3,S,S] on the device, records_d what `plan` returned, border3 what lies outside the image (three
        floats) -> float32 [n,3,S,S]; `out` must not be x."""
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or records_d.numel() < x.shape[0] * AFFINE_BYTES:
            raise ValueError('AffineWarp.warp: x %s, %d record bytes' % (tuple(x.shape), records_d.numel()))
        if out is None:
            out = torch.empty_like(x)
        border = (C.c_float * 3)(*[float(v) for v in border3])
        check(lib().ct_preproc_warp_affine(_dev(x, 'x'), _dev(records_d, 'records', torch.uint8), x.shape[0], x.shape[2],
                                           border, _dev(out, 'out'), _stream()), 'ct_preproc_warp_affine')
        return out

    def __call__(self, x, packed, image_ids, border3, out=None):
        records, packed = self.plan(packed, image_ids, x.shape[0], x.shape[2])
        return self.warp(x, records, border3, out), packed

    def check(self):
        """Read the status words of the last plan (a host synchronisation) and raise when an image was refused."""
        st = self.status.cpu().numpy()
        if st[0]:
            raise _lib.CtdetError('ct_aug_affine_plan: status %d (%d images refused)' % (st[0], st[1]))
        return st


def mixup_blend(img1, img2, lambd):
    """img1 * lambd + img2 * (1 - lambd) per image (data/voc0712.py:262); lambd: float or [B] tensor."""
    B = img1.shape[0]
    lam = torch.as_tensor(lambd, dtype=torch.float32, device=img1.device).expand(B).contiguous()
    out = torch.empty_like(img1)
    check(lib().ct_mixup_blend(_dev(img1, 'img1'), _dev(img2, 'img2'), _dev(lam, 'lambd'), B, img1.numel() // B,
                               _dev(out, 'out'), _stream()), 'ct_mixup_blend')
    return out


# ------------------------------------------------------------------ pooling / attention
def maxpool2d(x, k, stride, pad=0, ceil_mode=False):
    B, Cn, H, W = x.shape

    def osz(n):
        num = n + 2 * pad - k
        o = (-(-num // stride) if ceil_mode else num // stride) + 1
        if ceil_mode and (o - 1) * stride >= n + pad:
            o -= 1
        return o
    OH, OW = osz(H), osz(W)
    out = torch.empty(B, Cn, OH, OW, device=x.device, dtype=torch.float32)
    check(lib().ct_maxpool2d_fwd(_dev(x, 'x'), _dev(out, 'out'), B * Cn, H, W, OH, OW, k, stride, pad,
                                 _stream()), 'ct_maxpool2d_fwd')
    return out


def _ctx_prm(params, d, T, incre):
    prm = _lib.CtxParams()
    for k in ('theta_w', 'theta_b', 'phi_w', 'phi_b', 'g_w', 'g_b', 'wz', 'obj_w'):
        setattr(prm, k, _dev(params[k], k).value)
    if incre:
        prm.fc_w = _dev(params['fc_w'], 'fc_w').value
        prm.fc_b = _dev(params['fc_b'], 'fc_b').value
    prm.scale = float(params['scale'])
    prm.d, prm.t = d, T
    return prm


def ctx_attention(conf, pool, params, setting_incre=False, out=None, ws=None):
    """models/RFB_Net_vgg.py:253-271.  params: dict of device tensors theta_w, theta_b, phi_w, phi_b,
    g_w, g_b, wz, obj_w[, fc_w, fc_b] and float `scale`.  `out` / `ws`: caller-owned output and workspace
    (ctx_attention_buffers) so a captured / allocation-free forward can reuse them."""
    B, P, d = conf.shape
    M = pool.shape[1]
    T = params['obj_w'].shape[0]
    prm = _ctx_prm(params, d, T, setting_incre)
    if out is None:
        out = torch.empty(B, P, (d if setting_incre else 0) + T, device=conf.device, dtype=torch.float32)
    ws_bytes = lib().ct_ctx_attention_workspace_bytes(B, P, M, d)
    if ws is None:
        ws = torch.empty(ws_bytes, device=conf.device, dtype=torch.uint8)
    check(lib().ct_ctx_attention_fwd(_dev(conf, 'conf'), _dev(pool, 'pool'), B, P, M, C.byref(prm),
                                     _dev(out, 'out'), _dev(ws, 'ws', torch.uint8), ws_bytes, _stream()),
          'ct_ctx_attention_fwd')
    return out


def ctx_attention_buffers(B, P, M, d, T, setting_incre, device):
    """(out, ws) for ctx_attention with these sizes."""
    out = torch.empty(B, P, (d if setting_incre else 0) + T, device=device, dtype=torch.float32)
    ws = torch.empty(lib().ct_ctx_attention_workspace_bytes(B, P, M, d), device=device, dtype=torch.uint8)
    return out, ws


class CtxTrainer:
    """Forward-with-saved-rows + backward of the Context-Transformer block for one (B, P, M, d, T)
    (train.py:222-229 differentiates models/RFB_Net_vgg.py:253-271 through autograd).  Owns the
    workspaces; gradients come back in fresh tensors keyed like `params`.  deterministic=True: the backward is
    ct_ctx_attention_bwd_det (slabs added in a fixed order in place of floating-point atomics; the workspace holds them too)."""
    KEYS = ('theta_w', 'theta_b', 'phi_w', 'phi_b', 'g_w', 'g_b', 'wz', 'obj_w')

    def __init__(self, B, P, M, d, T, incre, device, deterministic=False):
        self.B, self.P, self.M, self.d, self.T, self.incre = B, P, M, d, T, bool(incre)
        self.device = torch.device(device)
        self.deterministic = bool(deterministic)
        L = lib()
        self.bwd_entry = 'ct_ctx_attention_bwd_det' if self.deterministic else 'ct_ctx_attention_bwd'
        if self.deterministic:
            bwd_bytes = L.ct_ctx_attention_bwd_det_workspace_bytes(B, P, M, d, T, int(self.incre), None)
            self.slab_bytes = bwd_bytes - L.ct_ctx_attention_bwd_workspace_bytes(B, P, M)
        else:
            bwd_bytes, self.slab_bytes = L.ct_ctx_attention_bwd_workspace_bytes(B, P, M), 0
        self.ws_bytes = max(L.ct_ctx_attention_workspace_bytes(B, P, M, d), bwd_bytes)
        self.ws = torch.empty(self.ws_bytes, device=self.device, dtype=torch.uint8)
        self.saved_bytes = L.ct_ctx_attention_saved_bytes(B, P)
        self.saved = torch.empty(self.saved_bytes, device=self.device, dtype=torch.uint8)
        self.keys = self.KEYS + (('fc_w', 'fc_b') if self.incre else ())
        self.dconf = torch.empty(B, P, d, device=self.device)
        self.dpool = torch.empty(B, M, d, device=self.device)

    def forward(self, conf, pool, params):
        prm = _ctx_prm(params, self.d, self.T, self.incre)
        out = torch.empty(self.B, self.P, (self.d if self.incre else 0) + self.T, device=self.device)
        check(lib().ct_ctx_attention_fwd_train(_dev(conf, 'conf'), _dev(pool, 'pool'), self.B, self.P, self.M,
                                               C.byref(prm), _dev(out, 'out'), _dev(self.saved, 'saved', torch.uint8),
                                               self.saved_bytes, _dev(self.ws, 'ws', torch.uint8), self.ws_bytes,
                                               _stream()), 'ct_ctx_attention_fwd_train')
        return out

    def backward(self, conf, pool, params, dout):
        """-> (dconf [B,P,d] without the pooled path, dpool [B,M,d], {key: grad})."""
        prm = _ctx_prm(params, self.d, self.T, self.incre)
        grads = {k: torch.empty_like(params[k]) for k in self.keys}
        g = _lib.CtxGrads()
        for k in self.keys:
            setattr(g, k, _dev(grads[k], 'd' + k).value)
        check(getattr(lib(), self.bwd_entry)(_dev(conf, 'conf'), _dev(pool, 'pool'), self.B, self.P, self.M, C.byref(prm),
                                             _dev(self.saved, 'saved', torch.uint8), _dev(dout, 'dout'),
                                             _dev(self.dconf, 'dconf'), _dev(self.dpool, 'dpool'), C.byref(g),
                                             _dev(self.ws, 'ws', torch.uint8), self.ws_bytes, _stream()),
              self.bwd_entry)
        return self.dconf, self.dpool, grads


def ctx_pool_bwd(conf_flat, src_base, dpool_flat, dst_base, dconf_flat, B, h, w, ch, k):
    """Adds the pooled-path gradient of one source into the flat conf gradient (element offsets)."""
    check(lib().ct_ctx_pool_bwd(C.c_void_p(_dev(conf_flat, 'conf').value + 4 * src_base), conf_flat.shape[1],
                                C.c_void_p(_dev(dpool_flat, 'dpool').value + 4 * dst_base), dpool_flat.shape[1],
                                C.c_void_p(_dev(dconf_flat, 'dconf').value + 4 * src_base), dconf_flat.shape[1],
                                B, h, w, ch, k, _stream()), 'ct_ctx_pool_bwd')


def device_info(device=0):
    cu, lds = C.c_int(0), C.c_int(0)
    arch = C.create_string_buffer(64)
    check(lib().ct_device_info(device, C.byref(cu), C.byref(lds), arch, 64), 'ct_device_info')
    return dict(cu_count=cu.value, lds_bytes_per_cu=lds.value, arch=arch.value.decode())
