"""MultiBoxLoss_combined -- drop-in for layers/modules/multibox_loss_combined.py:42-124.

Target assignment (jaccard / match / encode for the whole batch) is ONE call into the HIP
library (`ct_match_batched`) instead of a Python loop over images and ground truths; the loss
arithmetic itself (smooth-L1, two cross-entropies, 3:1 hard-negative ranking) has two forms: torch ops on
the device tensors with autograd (the default), or -- `fused=True` / CTDET_LOSS_FUSED=1 -- the library's
ct_multibox_loss_fwd / _bwd (three launches forward, one backward, no sort) behind one autograd Function.
The localisation term is the reference's smooth-L1 on the encoded offsets (the default) or -- `loc_loss=` /
CTDET_LOC_LOSS -- 1 - IoU, GIoU, DIoU or CIoU between the decoded prediction and the decoded target of every positive
prior (defined in include/ctdet.h at ct_multibox_loss_fwd_loc), in both forms; `loc_weight` multiplies loss_box_reg.
The classification terms are the reference's two cross-entropies over the 3:1 mined sample (the default) or -- `conf_loss=
'focal'` / CTDET_CONF_LOSS -- focal terms over every prior that is not ignored, with no mining (defined in include/ctdet.h
at ct_multibox_loss_fwd_terms), in both forms; focal_prior_init() below sets the objectness biases such a run starts from.
The assignment itself is the reference's fixed IoU rule (the default) or -- `matcher='atss'` / CTDET_MATCHER -- adaptive
training sample selection (defined in include/ctdet.h at ct_atss_match_batched), one library call either way; or --
`matcher='tal'` -- task-aligned assignment from the network's current predictions (ct_tal_match_batched), which costs one
ct_detect_fused pass over the detached predictions before the matching call.
targets: list of [G,6] tensors = [x1,y1,x2,y2,label,mixup_weight], or an ops.PackedTargets holding the same rows on
the device (what preproc(decisions='device').batch_device returns).
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from collections import namedtuple

from ctdet import _lib, ops

# what match() assigns to every prior: encoded box [B,P,4], (label, mixup weight) [B,P,2], ignore mask [B,P] bool
MatchedTargets = namedtuple('MatchedTargets', 'loc_t conf_t obj_t')


class FusedMultiBoxLoss(torch.autograd.Function):
    """(loc, conf, obj, matched targets) -> sums [3] = un-normalised (loc, cls, obj) losses, differentiable w.r.t. the
    three predictions, plus n [1], num_pos [B], w [B,P] (not differentiable).  The incoming [3] gradient goes to the
    backward kernel as a device pointer, so a normaliser applied outside (`sums / n`) scales it for free."""

    @staticmethod
    def forward(ctx, loc, conf, obj, loc_t, conf_t, obj_t, num_classes, negpos_ratio, priors=None, loc_loss='smooth_l1',
                variances=(0.1, 0.2), conf_loss='ce', focal_gamma=2.0, focal_alpha=0.25):
        ctx.terms = dict(priors=priors, loc_loss=loc_loss, variances=tuple(variances), conf_loss=conf_loss,
                         focal_gamma=focal_gamma, focal_alpha=focal_alpha)
        sums, n, num_pos, w = ops.multibox_loss(loc, conf, obj, loc_t, conf_t, obj_t, num_classes, negpos_ratio, **ctx.terms)
        ctx.save_for_backward(loc, conf, obj, loc_t, conf_t, obj_t, w)
        ctx.num_classes = num_classes
        ctx.mark_non_differentiable(n, num_pos, w)
        return sums, n, num_pos, w

    @staticmethod
    def backward(ctx, g, *unused):
        loc, conf, obj, loc_t, conf_t, obj_t, w = ctx.saved_tensors
        dloc, dconf, dobj = ops.multibox_loss_backward(loc, conf, obj, loc_t, conf_t, obj_t, w,
                                                       g.to(torch.float32).contiguous(), ctx.num_classes, **ctx.terms)
        return (dloc, dconf, dobj) + (None,) * 11


LOC_LOSSES = _lib.LOC_LOSSES        # 'smooth_l1' and the four IoU kinds
CONF_LOSSES = _lib.CONF_LOSSES      # 'ce' and 'focal'
MATCHERS = _lib.MATCHERS            # 'ssd' and 'atss': they read the ground truth and the priors only
PRED_MATCHERS = _lib.PRED_MATCHERS  # 'tal': it reads the current predictions too


class _ScaleGrad(torch.autograd.Function):
    """x in the forward, grad * weight in the backward."""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.weight = weight
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.weight, None


class _ScaleValue(torch.autograd.Function):
    """x * weight in the forward, the gradient passed through unchanged: the other half of _ScaleGrad."""

    @staticmethod
    def forward(ctx, x, weight):
        return x * weight

    @staticmethod
    def backward(ctx, g):
        return g, None


def _decode_rows(l, priors, variance):
    """utils/box_utils.py:184 on [B,P,4] offsets: -> x1, y1, x2, y2, cx, cy, w, h, each [B,P]."""
    cx = priors[:, 0] + l[..., 0] * variance[0] * priors[:, 2]
    cy = priors[:, 1] + l[..., 1] * variance[0] * priors[:, 3]
    w = priors[:, 2] * torch.exp(l[..., 2] * variance[1])
    h = priors[:, 3] * torch.exp(l[..., 3] * variance[1])
    return cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cx, cy, w, h


def iou_loss_rows(kind, loc, loc_t, priors, variance):
    """The IoU-family term of every row, [B,P] (torch ops with autograd; include/ctdet.h has the definition)."""
    ax1, ay1, ax2, ay2, acx, acy, aw, ah = _decode_rows(loc, priors, variance)
    tx1, ty1, tx2, ty2, tcx, tcy, tw, th = _decode_rows(loc_t, priors, variance)
    iw = (torch.minimum(ax2, tx2) - torch.maximum(ax1, tx1)).clamp_min(0)
    ih = (torch.minimum(ay2, ty2) - torch.maximum(ay1, ty1)).clamp_min(0)
    inter = iw * ih
    union = aw * ah + tw * th - inter
    iou = inter / union
    loss = 1 - iou
    if kind == 'iou':
        return loss
    cw = torch.maximum(ax2, tx2) - torch.minimum(ax1, tx1)
    ch = torch.maximum(ay2, ty2) - torch.minimum(ay1, ty1)
    if kind == 'giou':
        return loss + (cw * ch - union) / (cw * ch)
    loss = loss + ((acx - tcx) ** 2 + (acy - tcy) ** 2) / (cw ** 2 + ch ** 2)
    if kind == 'diou':
        return loss
    v = (4 / math.pi ** 2) * (torch.atan(tw / th) - torch.atan(aw / ah)) ** 2
    with torch.no_grad():               # alpha is a constant in the backward pass; 0 where v = 0 (never 0 / 0)
        alpha = torch.where(v > 0, v / ((1 - iou) + v).masked_fill(v <= 0, 1.0), torch.zeros_like(v))
    return loss + alpha * v


def focal_rows(ce, p, m, a, gamma):
    """FL = a m^gamma ce per row, with the gradient of include/ctdet.h attached: c * d ce, c = a m^gamma (1 - gamma p r),
    r = log p / m (-1 where m = 0) -- finite for every gamma >= 0, where autograd through m^gamma is not (gamma < 1, m = 0).
    ce = -log p carries the graph; p and m (the sum of the other probabilities) are constants here."""
    with torch.no_grad():
        pw = torch.ones_like(m) if gamma == 0 else m.pow(gamma)             # 0^0 = 1
        r = torch.where(m > 0, -ce / torch.where(m > 0, m, torch.ones_like(m)), -torch.ones_like(m))
        c = a * pw * (1 - gamma * p * r)
        value = a * pw * ce
    return value + c * (ce - ce.detach())


def focal_prior_init(net, pi=0.01):
    """The prior-probability initialisation focal training starts from: every objectness conv of `net.obj` (channel order
    (anchor, 2)) gets bias 0 in column 0 and -log((1 - pi) / pi) in column 1, so that every prior starts at
    softmax(obj)[1] = pi instead of 0.5; the weights are left alone."""
    if not 0.0 < pi < 1.0:
        raise ValueError('pi must be in (0, 1), got %r' % (pi,))
    with torch.no_grad():
        for conv in net.obj:
            bias = conv.bias.view(-1, 2)
            bias[:, 0] = 0.0
            bias[:, 1] = -math.log((1.0 - pi) / pi)
    return net


def _env_int(name, default):
    text = os.environ.get(name, '')
    try:
        return int(text) if text else default
    except ValueError:
        raise ValueError('%s must be an integer, got %r' % (name, text))


def _env_float(name, default):
    text = os.environ.get(name, '')
    try:
        return float(text) if text else default
    except ValueError:
        raise ValueError('%s must be a number, got %r' % (name, text))


class MultiBoxLoss_combined(nn.Module):
    def __init__(self, num_classes, overlap_thresh, prior_for_matching, bkg_label, neg_mining, neg_pos,
                 neg_overlap, encode_target, fused=None, loc_loss=None, loc_weight=1.0, conf_loss=None, focal_gamma=None,
                 focal_alpha=None, matcher=None, atss_topk=None, level_offsets=None, tal_topk=None, tal_alpha=None,
                 tal_beta=None):
        super().__init__()
        # fused: the HIP loss kernels instead of the torch ops below; None reads CTDET_LOSS_FUSED (default off)
        self.fused = os.environ.get('CTDET_LOSS_FUSED', '0') == '1' if fused is None else bool(fused)
        self.num_classes = num_classes
        self.threshold = overlap_thresh
        self.background_label = bkg_label
        self.encode_target = encode_target
        self.use_prior_for_matching = prior_for_matching
        self.do_neg_mining = neg_mining
        self.negpos_ratio = neg_pos
        self.neg_overlap = neg_overlap
        self.variance = [0.1, 0.2]
        # loc_loss: the localisation term, one of LOC_LOSSES; None reads CTDET_LOC_LOSS (unset or empty: smooth_l1)
        if loc_loss is None:
            loc_loss = os.environ.get('CTDET_LOC_LOSS', '') or 'smooth_l1'
        if loc_loss not in LOC_LOSSES:
            raise ValueError('loc_loss must be one of %s, got %r' % (', '.join(LOC_LOSSES), loc_loss))
        self.loc_loss = loc_loss
        self.loc_weight = float(loc_weight)   # multiplies loss_box_reg (published GIoU-style recipes use 2-5)
        # conf_loss: the classification terms, one of CONF_LOSSES; None reads CTDET_CONF_LOSS (unset or empty: ce).  The focal
        # constants: None reads CTDET_FOCAL_GAMMA / CTDET_FOCAL_ALPHA (unset or empty: 2.0 / 0.25; a negative alpha: no balancing)
        if conf_loss is None:
            conf_loss = os.environ.get('CTDET_CONF_LOSS', '') or 'ce'
        self.conf_loss, self.focal_gamma, self.focal_alpha = ops.check_focal(
            conf_loss, _env_float('CTDET_FOCAL_GAMMA', 2.0) if focal_gamma is None else focal_gamma,
            _env_float('CTDET_FOCAL_ALPHA', 0.25) if focal_alpha is None else focal_alpha)
        # matcher: the target assignment, one of MATCHERS; None reads CTDET_MATCHER (unset or empty: ssd, the reference's IoU >=
        # overlap_thresh rule).  'atss' (include/ctdet.h, ct_atss_match_batched) does not read overlap_thresh; it takes atss_topk
        # candidates per pyramid level (None reads CTDET_ATSS_TOPK; unset or empty: 9) and needs level_offsets, the L+1 prior
        # offsets of the levels (PriorBox.level_offsets()), which match() checks against the priors it is given
        if matcher is None:
            matcher = os.environ.get('CTDET_MATCHER', '') or 'ssd'
        if matcher not in MATCHERS + PRED_MATCHERS:
            raise ValueError('matcher must be one of %s, got %r' % (', '.join(MATCHERS + PRED_MATCHERS), matcher))
        self.matcher = matcher
        if atss_topk is None:
            text = os.environ.get('CTDET_ATSS_TOPK', '')
            try:
                atss_topk = int(text) if text else 9
            except ValueError:
                raise ValueError('CTDET_ATSS_TOPK must be an integer, got %r' % text)
        if isinstance(atss_topk, bool) or int(atss_topk) != atss_topk or not 1 <= int(atss_topk) <= 16:
            raise ValueError('atss_topk must be an integer in 1..16, got %r' % (atss_topk,))
        self.atss_topk = int(atss_topk)
        self.level_offsets = None if level_offsets is None else [int(o) for o in level_offsets]
        # 'tal' (include/ctdet.h, ct_tal_match_batched) reads neither overlap_thresh nor level_offsets but the predictions:
        # the tal_topk priors inside a box with the largest score^tal_alpha * IoU(predicted box, box)^tal_beta are its
        # positives.  None reads CTDET_TAL_TOPK / CTDET_TAL_ALPHA / CTDET_TAL_BETA (unset or empty: 13 / 1.0 / 6, TOOD's)
        topk, alpha2, beta = ops.check_tal(_env_int('CTDET_TAL_TOPK', 13) if tal_topk is None else tal_topk,
                                           _env_float('CTDET_TAL_ALPHA', 1.0) if tal_alpha is None else tal_alpha,
                                           _env_int('CTDET_TAL_BETA', 6) if tal_beta is None else tal_beta)
        self.tal_topk, self.tal_alpha, self.tal_beta = topk, alpha2 / 2.0, beta
        self.sync_normalizer = False      # set True under multi-process data parallelism

    @torch.no_grad()
    def match(self, priors, targets, device=None, out=None, predictions=None):
        """The target assignment of :60-76 alone (under 'ssd' and 'atss' it depends on the ground truth and the priors
        only): -> MatchedTargets, which forward() accepts in place of the raw target list.  `out`: a MatchedTargets of the
        same batch to overwrite in place -- a training step captured as a hipGraph (bench.py --train) reads the same three
        tensors at every replay, the matching itself (a host-built offset table, an H2D copy) stays outside the graph.
        `predictions`: the (loc, conf, obj) the network just produced, read by matcher='tal' alone, which cannot match
        without them; they are detached, no gradient flows through the assignment."""
        dev = torch.device(device) if device is not None else priors.device
        if self.matcher == 'tal':
            loc_t, conf_t, obj_t = self._match_tal(priors, targets, dev, predictions)
        elif self.matcher == 'atss':
            loc_t, conf_t, obj_t = self._match_atss(priors, targets, dev)
        elif isinstance(targets, ops.PackedTargets):      # device-resident truths / gt_off (ops.AugPlanner): no host table
            loc_t, conf_t, obj_t = ops.match_packed(targets.truths, targets.gt_off, targets.gt_off.numel() - 1,
                                                    targets.max_gt, priors.to(dev).float().contiguous(),
                                                    self.threshold, self.variance)
        else:
            loc_t, conf_t, obj_t = ops.match_batched([t.to(dev) for t in targets], priors.to(dev).float().contiguous(),
                                                     self.threshold, self.variance)
        if out is None:
            return MatchedTargets(loc_t, conf_t, obj_t)
        out.loc_t.copy_(loc_t); out.conf_t.copy_(conf_t); out.obj_t.copy_(obj_t)
        return out

    def _match_atss(self, priors, targets, dev):
        off, topk = ops.check_atss(self.level_offsets, self.atss_topk, priors.shape[0])
        pri = priors.to(dev).float().contiguous()
        if isinstance(targets, ops.PackedTargets):
            return ops.atss_match_packed(targets.truths, targets.gt_off, targets.gt_off.numel() - 1, targets.max_gt, pri, off,
                                         topk, self.variance)
        return ops.atss_match_batched([t.to(dev) for t in targets], pri, off, topk, self.variance)

    def _match_tal(self, priors, targets, dev, predictions):
        if predictions is None:
            raise ValueError("matcher='tal' assigns targets from the current predictions: match() needs predictions=(loc, "
                             "conf, obj); matching ahead of the forward pass is for matcher='ssd' and 'atss'")
        pri = priors.to(dev).float().contiguous()
        loc, conf, obj = (p.detach().to(dev).float().contiguous() for p in predictions)
        boxes, scores = ops.detect_fused(loc, conf, obj, pri, self.variance, apply_softmax=True)
        tal = (pri, boxes, scores, self.tal_topk, self.tal_alpha, self.tal_beta, self.variance)
        if isinstance(targets, ops.PackedTargets):
            return ops.tal_match_packed(targets.truths, targets.gt_off, targets.gt_off.numel() - 1, targets.max_gt, *tal)
        return ops.tal_match_batched([t.to(dev) for t in targets], *tal)

    def forward(self, predictions, priors, targets):
        loc_data, conf_data, obj_data = predictions
        dev = loc_data.device
        num, num_priors = loc_data.size(0), priors.size(0)
        if isinstance(targets, MatchedTargets):
            loc_t, conf_t, obj_t = targets
        elif self.matcher in PRED_MATCHERS:
            loc_t, conf_t, obj_t = self.match(priors, targets, dev, predictions=predictions)
        else:
            loc_t, conf_t, obj_t = self.match(priors, targets, dev)
        if self.fused:
            return self._forward_fused(loc_data, conf_data, obj_data, loc_t, conf_t, obj_t, priors)
        labels, weights = conf_t[:, :, 0], conf_t[:, :, 1]
        pos = labels > 0
        num_pos = (weights * pos.float()).sum(1, keepdim=True).long()
        # Every term below is a MASKED SUM over all priors instead of the reference's boolean gather (`x[pos]`,
        # `x[pos | neg]`): the same numbers (a masked-out row contributes exactly 0 to the value and to the gradient),
        # but no `nonzero` behind the indexing, i.e. no host synchronisation in the middle of the training step -- the
        # host keeps issuing the backward pass while the forward still runs (tools/train_bench.py at small batches).

        # localisation: smooth-L1 on positives, weighted by the mixup weight (:81-85)
        if self.loc_weight != 1.0:
            # loc_weight in the torch form: the value is multiplied once at the end (_ScaleValue) and the gradient once where
            # it reaches loc_data, so both are the unweighted run's times loc_weight to one rounding, element for element
            loc_data = _ScaleGrad.apply(loc_data, self.loc_weight)
        if self.loc_loss == 'smooth_l1':
            l1 = F.smooth_l1_loss(loc_data, loc_t, reduction='none').sum(2)
            loss_l = (l1 * (weights * pos.float())).sum()
        else:
            # an IoU-family term between the decoded boxes.  A row that is not positive or carries weight 0 is evaluated
            # on zero offsets (prediction = target = its prior: finite, L = 0) so that whatever it holds reaches neither
            # the value nor the gradient
            live = (pos & (weights != 0)).unsqueeze(2)
            zero = torch.zeros((), dtype=loc_data.dtype, device=dev)
            rows = iou_loss_rows(self.loc_loss, torch.where(live, loc_data, zero), torch.where(live, loc_t, zero),
                                 priors.to(dev), self.variance)
            loss_l = (rows * (weights * pos.float())).sum()

        obj_flat = obj_data.reshape(-1, 2)
        obj_lab = obj_t.long().view(-1)
        if self.conf_loss == 'focal':
            loss_c, loss_obj = self._focal_sums(obj_flat, conf_data.reshape(-1, self.num_classes - 1), obj_lab,
                                                labels.reshape(-1), weights.reshape(-1))
            return self._normalized(loss_l, loss_c, loss_obj, num_pos, dev)

        # hard negatives ranked by objectness loss, 3:1 (:88-96)
        with torch.no_grad():
            ce = F.cross_entropy(obj_flat, obj_lab, reduction='none')
            ce = ce.masked_fill(obj_t.view(-1), 0.0)
            rank = ce.view(num, -1).sort(1, descending=True)[1].sort(1)[1]
            num_neg = torch.clamp(self.negpos_ratio * num_pos, max=num_priors - 1)
            neg = rank < num_neg.expand_as(rank)
            w = (weights * (pos | neg).float()).view(-1)
        loss_obj = (F.cross_entropy(obj_flat, obj_lab, reduction='none') * w).sum()

        # class loss on objectness-fused logits (:106-117)
        flat_conf = conf_data.reshape(-1, self.num_classes - 1)
        # log(sum(exp(conf))) of :108 as logsumexp: same value, and an unselected row with a huge logit cannot put
        # inf * 0 = NaN into the masked sum
        bg = obj_flat[:, :1] + torch.logsumexp(flat_conf, dim=1, keepdim=True)
        fg = obj_flat[:, 1:2].expand_as(flat_conf) + flat_conf
        logit = torch.cat((bg, fg), 1)
        # ignored boxes carry label -1 (data/voc0712.py:237-238, 263-264: 'incre' phase 2 / instance_shot); the reference
        # never evaluates them (pos is False, their mining loss is zeroed so they are not drawn as negatives, :93) --
        # here their row is evaluated against class 0 and multiplied by w = 0: a valid target index, the same sum
        cls_t = labels.long().clamp_min(0).view(-1)
        loss_c = (F.cross_entropy(logit, cls_t, reduction='none') * w).sum()
        return self._normalized(loss_l, loss_c, loss_obj, num_pos, dev)

    def _focal_sums(self, obj_flat, flat_conf, obj_lab, labels, weights):
        """The two focal sums over all priors (include/ctdet.h, ct_multibox_loss_fwd_terms): nothing is mined, w = weight of
        every row that is not ignored.  A row of w = 0 is evaluated on zero logits and a background row on a zero conf row
        (finite values, times w = 0 or not used), so that whatever they hold reaches neither a value nor a gradient."""
        gamma, alpha = self.focal_gamma, self.focal_alpha
        w = weights * (labels >= 0).float()
        live = (w != 0).unsqueeze(1)
        cls_t = labels.long().clamp(0, self.num_classes - 1)
        fg = cls_t > 0
        zero = torch.zeros((), dtype=obj_flat.dtype, device=obj_flat.device)
        lo = F.log_softmax(torch.where(live, obj_flat, zero), 1)
        lq = F.log_softmax(torch.where(live & fg.unsqueeze(1), flat_conf, zero), 1)
        col = (cls_t - 1).clamp_min(0).unsqueeze(1)
        with torch.no_grad():
            s, q = lo.exp(), lq.exp()
            q_t = q.gather(1, col).squeeze(1)
            q_others = q.scatter(1, col, 0.0).sum(1)

        def balance(is_fg):             # a = alpha for a foreground target, 1 - alpha for background, 1 when alpha < 0
            return torch.where(is_fg, alpha, 1.0 - alpha).to(w.dtype) if alpha >= 0 else torch.ones_like(w)

        # objectness: target obj_t, p = s_t, m = the other column
        is_obj = obj_lab == 1
        ce_obj = -lo.gather(1, obj_lab.unsqueeze(1)).squeeze(1)
        fl_obj = focal_rows(ce_obj, torch.where(is_obj, s[:, 1], s[:, 0]), torch.where(is_obj, s[:, 0], s[:, 1]),
                            balance(is_obj), gamma)
        # class, on p_0 = s_0, p_k = s_1 q_k: log p_t from the logits, m = the sum of the other probabilities
        ce_cls = torch.where(fg, -(lo[:, 1] + lq.gather(1, col).squeeze(1)), -lo[:, 0])
        fl_cls = focal_rows(ce_cls, torch.where(fg, s[:, 1] * q_t, s[:, 0]),
                            torch.where(fg, s[:, 0] + s[:, 1] * q_others, s[:, 1]), balance(fg), gamma)
        return (fl_cls * w).sum(), (fl_obj * w).sum()

    def _normalized(self, loss_l, loss_c, loss_obj, num_pos, dev):
        n = num_pos.sum()
        if self.sync_normalizer:          # data-parallel: N over the global batch (see ctdet.dist)
            from ctdet.dist import global_normalizer
            n = global_normalizer(n, dev)
        loss_l = loss_l / n
        if self.loc_weight != 1.0:
            loss_l = _ScaleValue.apply(loss_l, self.loc_weight)
        return {'loss_box_reg': loss_l, 'loss_cls': loss_c / n, 'loss_obj': loss_obj / n}

    def _forward_fused(self, loc_data, conf_data, obj_data, loc_t, conf_t, obj_t, priors):
        for t in (loc_data, conf_data, obj_data, loc_t, conf_t, obj_t):
            if not t.is_cuda:
                raise _lib.CtdetError('MultiBoxLoss_combined(fused=True) needs tensors on the HIP device (got %s); '
                                      'there is no CPU form of the fused loss -- use fused=False' % t.device)
        args = (loc_data.contiguous(), conf_data.contiguous(), obj_data.contiguous(), loc_t.contiguous(),
                conf_t.contiguous(), obj_t.contiguous(), self.num_classes, int(self.negpos_ratio))
        # the trailing arguments are given only where they differ from the defaults: the default criterion calls what it always did
        loc_args = (None, 'smooth_l1', tuple(self.variance))
        if self.loc_loss != 'smooth_l1':
            loc_args = (priors.to(loc_data.device, torch.float32).contiguous(), self.loc_loss, tuple(self.variance))
        if self.conf_loss != 'ce':
            args += loc_args + (self.conf_loss, self.focal_gamma, self.focal_alpha)
        elif self.loc_loss != 'smooth_l1':
            args += loc_args
        sums, n, _, _ = FusedMultiBoxLoss.apply(*args)
        n = n[0]
        if self.sync_normalizer:
            from ctdet.dist import global_normalizer
            n = global_normalizer(n, loc_data.device)
        losses = sums / n                 # the one torch op: autograd hands g / n to the backward kernel
        loss_l = losses[0]
        if self.loc_weight != 1.0:        # reaches the backward kernel through g[0]: no launch of its own in the backward
            loss_l = loss_l * self.loc_weight
        return {'loss_box_reg': loss_l, 'loss_cls': losses[1], 'loss_obj': losses[2]}
