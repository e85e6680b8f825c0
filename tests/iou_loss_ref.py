"""Float64 restatement of the IoU-family localisation terms (include/ctdet.h, ct_multibox_loss_fwd_loc), written from
the definition and from nothing else: the yardstick of tests/test_iou_loss_cpu.py and tests/test_gpu_iou_loss.py.
Gradients come from float64 autograd; alpha of `ciou` is detached (a constant in the backward pass)."""
import math

import torch

KINDS = ('iou', 'giou', 'diou', 'ciou')


def decode(l, p, var0=0.1, var1=0.2):
    """utils/box_utils.py:184 on [...,4] offsets and centre-form priors -> (x1, y1, x2, y2, cx, cy, w, h)."""
    cx = p[..., 0] + l[..., 0] * var0 * p[..., 2]
    cy = p[..., 1] + l[..., 1] * var0 * p[..., 3]
    w = p[..., 2] * torch.exp(l[..., 2] * var1)
    h = p[..., 3] * torch.exp(l[..., 3] * var1)
    return cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cx, cy, w, h


def terms(loc, loc_t, priors, var0=0.1, var1=0.2):
    """The pieces of the definition, per row: dict of tensors shaped like loc[..., 0]."""
    ax1, ay1, ax2, ay2, acx, acy, aw, ah = decode(loc, priors, var0, var1)
    tx1, ty1, tx2, ty2, tcx, tcy, tw, th = decode(loc_t, priors, var0, var1)
    zero = torch.zeros_like(ax1)
    iw_raw = torch.minimum(ax2, tx2) - torch.maximum(ax1, tx1)
    ih_raw = torch.minimum(ay2, ty2) - torch.maximum(ay1, ty1)
    iw, ih = torch.maximum(zero, iw_raw), torch.maximum(zero, ih_raw)
    inter = iw * ih
    union = aw * ah + tw * th - inter
    cw = torch.maximum(ax2, tx2) - torch.minimum(ax1, tx1)
    ch = torch.maximum(ay2, ty2) - torch.minimum(ay1, ty1)
    rho2 = (acx - tcx) ** 2 + (acy - tcy) ** 2
    v = (4.0 / math.pi ** 2) * (torch.atan(tw / th) - torch.atan(aw / ah)) ** 2
    return dict(inter=inter, union=union, iou=inter / union, cw=cw, ch=ch, rho2=rho2, c2=cw ** 2 + ch ** 2, v=v,
                iw_raw=iw_raw, ih_raw=ih_raw,
                pairs=((ax2, tx2), (ax1, tx1), (ay2, ty2), (ay1, ty1)))


def alpha_of(t):
    """alpha = v / ((1 - IoU) + v), 0 where v = 0; always detached."""
    v, iou = t['v'].detach(), t['iou'].detach()
    return torch.where(v > 0, v / torch.where(v > 0, (1 - iou) + v, torch.ones_like(v)), torch.zeros_like(v))


def loss_rows(kind, loc, loc_t, priors, var0=0.1, var1=0.2, alpha=None):
    """Per-row L of `kind`; inputs of any float dtype are taken to float64.  alpha: a constant to use for `ciou` in place
    of the detached one (gradcheck supplies it as an input)."""
    if kind not in KINDS:
        raise KeyError(kind)
    loc, loc_t, priors = loc.double(), loc_t.double(), priors.double()
    t = terms(loc, loc_t, priors, var0, var1)
    L = 1 - t['iou']
    if kind == 'giou':
        c = t['cw'] * t['ch']
        L = L + (c - t['union']) / c
    elif kind in ('diou', 'ciou'):
        L = L + t['rho2'] / t['c2']
        if kind == 'ciou':
            L = L + (alpha_of(t) if alpha is None else alpha) * t['v']
    return L


def loc_sum(kind, loc, loc_t, conf_t, priors, var0=0.1, var1=0.2):
    """sum over positives (label > 0) of L * weight, float64: loc [B,P,4] may require grad, conf_t [B,P,2]."""
    pos = conf_t[..., 0] > 0
    L = loss_rows(kind, loc[pos], loc_t[pos], priors.expand(loc.shape[0], -1, -1)[pos], var0, var1)
    return (L * conf_t[..., 1][pos].double()).sum()


def kink_distance(loc, loc_t, priors, var0=0.1, var1=0.2):
    """Per row: the smallest absolute distance of a min / max argument pair, or of the raw iw / ih, from its kink."""
    t = terms(loc.double(), loc_t.double(), priors.double(), var0, var1)
    d = torch.stack([(a - b).abs() for a, b in t['pairs']] + [t['iw_raw'].abs(), t['ih_raw'].abs()], 0)
    return d.min(0)[0]
