"""Float64 restatement of the focal classification terms (include/ctdet.h, ct_multibox_loss_fwd_terms), written from the
definition and from nothing else: the yardstick of tests/test_focal_loss_cpu.py and tests/test_gpu_focal_loss.py.
Gradients come from float64 autograd through the definition itself (m^gamma included), never from the closed form the
kernels and the criterion use.  Rows of weight 0 are dropped before anything is evaluated."""
import functools

import torch

GAMMA_ALPHA = ((0.0, -1.0), (0.5, 0.25), (2.0, 0.25), (2.0, -1.0))      # the (gamma, alpha) pairs of both test files


def probabilities(conf, obj):
    """The fused class probabilities p [N,C] (p_0 = s_0, p_k = s_1 q_k) and log p taken from the logits."""
    ls, lq = torch.log_softmax(obj, -1), torch.log_softmax(conf, -1)
    s, q = torch.softmax(obj, -1), torch.softmax(conf, -1)
    return torch.cat((s[..., :1], s[..., 1:2] * q), -1), torch.cat((ls[..., :1], ls[..., 1:2] + lq), -1)


def focal_rows(p, logp, t, a, gamma):
    """FL = -a m^gamma log p_t per row; m = the SUM OF THE OTHER probabilities, 0^0 = 1."""
    hot = torch.zeros_like(p, dtype=torch.bool).scatter(-1, t.unsqueeze(-1), True)
    m = p.masked_fill(hot, 0.0).sum(-1)
    weight = torch.ones_like(m) if gamma == 0 else m.pow(gamma)
    return -a * weight * logp.gather(-1, t.unsqueeze(-1)).squeeze(-1)


def balance(is_fg, alpha):
    """a = alpha for a foreground target, 1 - alpha for background; 1 when alpha < 0."""
    one = torch.ones(is_fg.shape, dtype=torch.float64)
    return one if alpha < 0 else torch.where(is_fg, alpha * one, (1.0 - alpha) * one)


def row_weights(conf_t):
    """w = weight when label >= 0, 0 for an ignored row."""
    return torch.where(conf_t[..., 0] >= 0, conf_t[..., 1], torch.zeros_like(conf_t[..., 1])).double()


def focal_sums(conf, obj, conf_t, obj_t, gamma, alpha):
    """-> (sum of w FL_cls, sum of w FL_obj), float64; conf [..,C-1] and obj [..,2] may require grad."""
    ncls = conf.shape[-1] + 1
    w = row_weights(conf_t)
    keep = w != 0
    conf, obj, w = conf.double()[keep], obj.double()[keep], w[keep]
    t = conf_t[..., 0][keep].long().clamp(0, ncls - 1)
    ot = obj_t[keep].long()
    p, logp = probabilities(conf, obj)
    cls = focal_rows(p, logp, t, balance(t > 0, alpha), gamma)
    ob = focal_rows(torch.softmax(obj, -1), torch.log_softmax(obj, -1), ot, balance(ot == 1, alpha), gamma)
    return (cls * w).sum(), (ob * w).sum()


def smooth_l1_sum(loc, loc_t, conf_t):
    """The default localisation term: sum over positives of smooth-L1(loc - loc_t) * weight, float64."""
    pos = conf_t[..., 0] > 0
    d = (loc.double()[pos] - loc_t.double()[pos]).abs()
    return (torch.where(d < 1, 0.5 * d * d, d - 0.5).sum(-1) * conf_t[..., 1][pos].double()).sum()


def num_pos(conf_t):
    """long(sum of weight over label > 0) per image, summed: the normaliser n."""
    pos = conf_t[..., 0] > 0
    return int((conf_t[..., 1] * pos.float()).sum(-1).long().sum())


def sums_and_grads(pred, loc_t, conf_t, obj_t, gamma, alpha, g=(1.0, 1.0, 1.0)):
    """The un-normalised (loc [smooth-L1], cls, obj) sums and the gradients of g . sums w.r.t. (loc, conf, obj)."""
    x = [p.double().requires_grad_(True) for p in pred]
    sl = smooth_l1_sum(x[0], loc_t, conf_t)
    sc, so = focal_sums(x[1], x[2], conf_t, obj_t, gamma, alpha)
    grads = torch.autograd.grad(g[0] * sl + g[1] * sc + g[2] * so, x, allow_unused=True)
    grads = [torch.zeros_like(a) if b is None else b for a, b in zip(x, grads)]
    return [float(v.detach()) for v in (sl, sc, so)], grads


@functools.lru_cache(None)
def criterion_reference(name, gamma, alpha):
    """Case `name` of tests/iou_loss_cases.py as the criterion reports it: the three losses divided by n, and the gradients of
    their sum; computed once and handed out unchanged (the loc term here is smooth-L1; the IoU kinds have their own twin)."""
    import iou_loss_cases as cases
    c = cases.case(name)
    g = (1.0 / c.n,) * 3
    sums, grads = sums_and_grads(c.pred, c.loc_t, c.conf_t, c.obj_t, gamma, alpha, g)
    return dict(zip(cases.KEYS, (v / c.n for v in sums))), grads
