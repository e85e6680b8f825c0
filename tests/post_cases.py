"""Case builders for the post-processing chain (csrc/ct_post.hip) and NMS (csrc/ct_nms.hip) at their internal
boundaries.  Pure numpy: nothing here touches a device.

Every chain case is `(boxes [B,P,4] f32, scores [B,P,T+1] f32, kwargs)`; kwargs hold conf_thresh, nms_thresh, ge,
max_per_image and out_cap (None = room for every prior).  Boxes are pixel coordinates, already decoded and scaled
(scale_wh = (1, 1) in the oracle).  `reference` is the oracle loop (oracle/nms_ref.postprocess_image, test.py:136-161)
restated with prior indices; `cut_model` / `bounding_kept` restate, in numpy, which branch of select_sort_kernel /
prefix_cut_kernel an input reaches, so that tests/test_post_cases_cpu.py can prove each case sits where its name says.
"""
import functools
from fractions import Fraction

import numpy as np

from oracle import nms_ref

# The sizes at which the chain switches between special cases.  tests/test_post_cases_cpu.py reads the two sources and
# fails when one of them is retuned, naming the cases that have to move with it.
CONSTANTS = {
    'kSortThreads': 512,     # ct_post.hip:39   constexpr int kSortThreads
    'kSelectBatch': 8,       # ct_post.hip:40   constexpr int kSelectBatch; one trip of the select loop = 512 * 8 priors
    'kPartialMin': 1024,     # ct_post.hip:79   n <= 1024: sort everything, above it cut by histogram
    'kHistBins': 2048,       # ct_post.hip:80   11-bit bins: bits >> 20, then (bits >> 9) & 2047
    'kStageCap': 8192,       # ct_post.hip:308  kth_largest_kept stages at most this many kept scores of an image in LDS
    'kStageMaxT': 128,       # ct_post.hip:309  ... and only with at most this many classes
    'kImageGroup': 8,        # ct_post.hip:143  blockIdx -> (image, class): b = (blk >> 3) / T * 8 + (blk & 7)
    'kPrefix': 256,          # ct_post.hip:596  num_priors > 256 turns the bounding pass + partial sort on
    'kLdsKeys': 4096,        # ct_post.hip:604-606  select_sort_kernel<4096, ..>: keys sorted in LDS
    'kLdsKeysLarge': 8192,   # ct_post.hip:611  select_sort_kernel<8192, false> above kLargePriors priors
    'kLargePriors': 16384,   # ct_post.hip:610  num_priors > 16384
    'kKeptLds': 2048,        # ct_nms.hip:33    kept boxes beyond it are re-read from memory
    'kNmsChunk': 256,        # ct_nms.hip:34    kThreads: candidates per chunk (phase A)
    'kNmsSubChunk': 64,      # ct_nms.hip:199   kThreads / 64 sub-chunks, one wave each (phase B)
    'kThrBand': 1e-5,        # ct_nms.hip:45-46 make_thr: t * (1 -+ 1e-5f); IEEE division only inside the band
}
# constant -> the case families that sit on it
CONSTANT_CASES = {
    'kPrefix': 'A n=255/256/257, B P=255/256/257, D P=200/300, E P=256/257',
    'kSortThreads': 'B P=511/512/513 and 4095/4096/4097 (kSortThreads * kSelectBatch)',
    'kSelectBatch': 'B P=4095/4096/4097',
    'kPartialMin': 'A n=1023/1024/1025, C1, C2',
    'kLdsKeys': 'A n=4095/4096/4097, B P=4096/4097/8192/8193, C3-C6',
    'kLdsKeysLarge': 'none: needs more than 16 384 priors (the 512 pipeline test of test_gpu_kernels.py)',
    'kLargePriors': 'none: as above',
    'kHistBins': 'C1-C6 (bin edges), E powers of two (high bins), F conf_thresh = 0 (bin 0)',
    'kStageCap': 'E P=256/257 with T=32/33',
    'kStageMaxT': 'E P=64 with T=128/129',
    'kImageGroup': 'D B=1/7/8/9/16/17',
    'kKeptLds': 'borderline segment `beyond`, B P=4095.. (all kept)',
    'kNmsChunk': 'borderline segments `phase_a`, `waves`',
    'kNmsSubChunk': 'borderline segment `waves`, `waves3`',
    'kThrBand': 'borderline_pairs kinds equal/below/above (inside) and out_below/out_above (outside)',
}
K_PARTIAL, K_LDS, K_PREFIX = CONSTANTS['kPartialMin'], CONSTANTS['kLdsKeys'], CONSTANTS['kPrefix']
CONF = 0.01


def f2b(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def b2f(x):
    return np.asarray(x, dtype=np.uint32).view(np.float32)


def kw(conf_thresh=CONF, nms_thresh=0.45, ge=False, max_per_image=200, out_cap=None):
    return dict(conf_thresh=conf_thresh, nms_thresh=nms_thresh, ge=ge, max_per_image=max_per_image, out_cap=out_cap)


# ------------------------------------------------------------------ the oracle loop with indices
def reference(boxes, scores, conf_thresh=CONF, nms_thresh=0.45, ge=False, max_per_image=200, out_cap=None, variant=None):
    """-> res[b][c] = (rows [k,5] f32, prior_index [k] int64) for class c + 1 of image b, the rows in the order the chain
    writes them.  out_cap does not enter: the clamp is the caller's to apply.  `variant` names a plausibly WRONG rule (the
    teeth checks): 'conf_ge', 'cut_gt', 'k_plus', 'k_minus', 'tie_desc', 'ge_flip'."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    B, P, T1 = scores.shape
    t = np.float32(conf_thresh)
    nms_ge = (not ge) if variant == 'ge_flip' else bool(ge)
    k = int(max_per_image) + {'k_plus': 1, 'k_minus': -1}.get(variant, 0) if max_per_image > 0 else 0
    res = []
    for b in range(B):
        per = []
        for j in range(1, T1):
            s = scores[b, :, j]
            with np.errstate(invalid='ignore'):
                inds = np.where(s >= t if variant == 'conf_ge' else s > t)[0]
            if variant == 'conf_ge':
                inds = inds[~np.isnan(s[inds])]
            c_dets = np.hstack((boxes[b, inds], s[inds, None])).astype(np.float32, copy=False).reshape(-1, 5)
            order = None
            if variant == 'tie_desc' and len(inds):
                order = np.lexsort((-np.arange(len(inds)), -c_dets[:, 4].astype(np.float64)))
            keep = nms_ref.nms_c(c_dets, nms_thresh, ge=nms_ge, order=order)
            per.append((c_dets[keep], inds[keep]))
        if k > 0:
            alls = np.hstack([r[:, 4] for r, _ in per])
            if len(alls) > k:
                thr = np.sort(alls)[-k]
                per = [((r[r[:, 4] > thr], i[r[:, 4] > thr]) if variant == 'cut_gt' else
                        (r[r[:, 4] >= thr], i[r[:, 4] >= thr])) for r, i in per]
        if variant is None:
            want = nms_ref.postprocess_image(boxes[b], scores[b], (1, 1), conf_thresh=conf_thresh, nms_thresh=nms_thresh,
                                             max_per_image=max_per_image,
                                             nms_fn=lambda d, th: nms_ref.nms_c(d, th, ge=ge))
            for j in range(1, T1):
                assert np.array_equal(per[j - 1][0].view(np.uint32), want[j].view(np.uint32)), (b, j)
                assert np.array_equal(boxes[b, per[j - 1][1]], per[j - 1][0][:, :4])
        res.append(per)
    return res


def same_result(a, b):
    """two results of `reference`: the same rows (bit for bit) and prior indices in every (image, class)"""
    return all(np.array_equal(x[1], y[1]) and np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32))
               for pa, pb in zip(a, b) for x, y in zip(pa, pb))


# ------------------------------------------------------------------ numpy model of the branches
def candidate_bits(scores, b, c, conf_thresh=CONF):
    """score bits of the candidates of image b, class c + 1, in prior order"""
    s = np.asarray(scores, np.float32)[b, :, c + 1]
    with np.errstate(invalid='ignore'):
        return f2b(s[s > np.float32(conf_thresh)])


def cut_model(bits):
    """select_sort_kernel<4096, true> on one segment's candidate bits: n, the first histogram's m and `above`, the
    refined m, and the path taken ('all' / 'lds' / 'refined' / 'full')."""
    bits = np.asarray(bits, np.uint32)
    n = len(bits)
    out = dict(n=n, m=n, above=None, refined=None, path='all')
    if n <= K_PARTIAL:
        return out
    nb = CONSTANTS['kHistBins']
    h = np.bincount(bits >> 20, minlength=nb)[::-1]
    cum = np.cumsum(h)
    d = int(np.argmax(cum >= K_PARTIAL))
    out.update(m=int(cum[d]), above=int(cum[d] - h[d]), path='lds')
    if out['m'] > K_LDS:
        inside = bits[(bits >> 20) == nb - 1 - d]
        h2 = np.bincount((inside >> 9) & (nb - 1), minlength=nb)[::-1]
        cum2 = np.cumsum(h2)
        d2 = int(np.argmax(cum2 >= K_PARTIAL - out['above']))
        out['refined'] = out['above'] + int(cum2[d2])
        out['path'] = 'refined' if out['refined'] <= K_LDS else 'full'
    return out


def bounding_kept(boxes, scores, b, conf_thresh=CONF, nms_thresh=0.45, ge=False):
    """kept boxes of image b after the bounding pass: NMS of every class's best kPrefix candidates"""
    total = 0
    for j in range(1, scores.shape[2]):
        s = scores[b, :, j]
        with np.errstate(invalid='ignore'):
            inds = np.where(s > np.float32(conf_thresh))[0]
        order = nms_ref.stable_desc_order(s[inds])[:K_PREFIX]
        d = np.hstack((boxes[b, inds[order]], s[inds[order], None])).astype(np.float32).reshape(-1, 5)
        total += len(nms_ref.nms_sorted_c(d, nms_thresh, ge=ge))
    return total


# ------------------------------------------------------------------ boxes
def disjoint(P, rng=None, origin=(0.0, 0.0)):
    """a grid of 10 x 10 boxes (+1 convention) 20 apart: nothing suppresses anything.  rng: shuffled over the priors"""
    i = np.arange(P)
    if rng is not None:
        i = rng.permutation(P)
    xy = np.stack([(i % 100) * 20.0 + origin[0], (i // 100) * 20.0 + origin[1]], 1)
    return np.concatenate([xy, xy + 9.0], 1).astype(np.float32)


def mostly_disjoint(P, rng=None):
    """`disjoint`, but every fifth prior sits one pixel beside its predecessor (IoU 0.82): the lower of the two goes"""
    bx = disjoint(P, rng)
    p = np.arange(4, P, 5)
    bx[p] = bx[p - 1] + np.array([1, 0, 1, 0], np.float32)
    return bx


def identical(P):
    return np.tile(np.array([[100, 150, 300, 350]], np.float32), (P, 1))


def clustered(P, seed):
    from ctdet import synth
    return synth.clustered_dets(P, rng=np.random.RandomState(seed))[:, :4].copy()


# ------------------------------------------------------------------ scores from bit patterns
LO_BITS, HI_BITS = int(f2b(0.0117)), int(f2b(0.99))


def ladder_bits(n, lo=LO_BITS, hi=HI_BITS):
    """n distinct score bit patterns, evenly spaced in bit space over some 50 of the 11-bit bins"""
    return np.linspace(lo, hi, n).astype(np.uint32) if n > 1 else np.full(n, hi, np.uint32)


def bits_in_bins(spec):
    """spec: [(bin, count)] or [(bin, sub, count)] -> bit patterns with exactly `count` of them in 11-bit bin `bin`
    (bits >> 20) and, where given, in sub-bin `sub` ((bits >> 9) & 2047).  Distinct inside a bin (2^20 patterns) or as
    far as a sub-bin's 512 patterns go; beyond that they repeat (ties, ordered by prior index)."""
    out = []
    for item in spec:
        if len(item) == 2:
            b, cnt = item
            low = (np.arange(cnt, dtype=np.uint64) * 1048573 // max(cnt, 1)) % (1 << 20) if cnt else np.zeros(0, np.uint64)
            out.append((np.uint32(b) << 20) | low.astype(np.uint32))
        else:
            b, sub, cnt = item
            out.append((np.uint32(b) << 20) | (np.uint32(sub) << 9) | (np.arange(cnt, dtype=np.uint32) % 512))
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)


def place(P, T, per_class_bits, rng, below=0.001):
    """scores [P, T+1]: class c + 1 gets per_class_bits[c] at shuffled priors, everything else `below`"""
    s = np.full((P, T + 1), below, np.float32)
    for c, bits in enumerate(per_class_bits):
        pos = rng.permutation(P)[:len(bits)]
        s[pos, c + 1] = b2f(rng.permutation(np.asarray(bits, np.uint32)))
    return s


# ------------------------------------------------------------------ NMS pairs at the threshold
KINDS = ('equal', 'below', 'above', 'out_below', 'out_above')
NMS_THRESHOLDS = (0.3, 0.45, 0.5)


def pair_kind(a, A, thresh):
    """a / A against the fp32 threshold: the kind of KINDS it is (or None) and its exact relative distance"""
    t32 = np.float32(thresh)
    q = np.float32(a) / np.float32(A)
    rel = (Fraction(a, A) - Fraction(float(t32))) / Fraction(float(t32))
    r = abs(float(rel))
    if q == t32:
        return 'equal', rel
    if r < 5e-6:
        return ('below' if q < t32 else 'above'), rel
    if 2e-5 <= r <= 5e-5:
        return ('out_below' if q < t32 else 'out_above'), rel
    return None, rel


@functools.lru_cache(maxsize=None)
def borderline_pairs(thresh, want=12):
    """{kind: [(W, H, w, h)]}: box [0, 0, w-1, h-1] inside [0, 0, W-1, H-1] has, with the +1 convention, the IoU
    w*h / (W*H) exactly (all areas < 2^24), whose fp32 quotient is equal to / just below / just above the fp32 threshold
    (relative distance < 5e-6, inside make_thr's band) or 2e-5 .. 5e-5 away from it (outside, the reciprocal fast path)."""
    found = {k: [] for k in KINDS}
    t = float(np.float32(thresh))
    for W in range(1200, 599, -1):
        for H in (W, W - 1, W - 13):
            A = W * H
            centre = int(round(t * A))
            far = [int(round(t * A * (1 + s * r))) for s in (-1, 1) for r in (2.5e-5, 3.5e-5, 4.5e-5)]
            for a in list(range(centre - 2, centre + 3)) + far:
                kind, _ = pair_kind(a, A, thresh)
                if kind is None or len(found[kind]) >= want or any(p[0] == W and p[1] == H for p in found[kind]):
                    continue
                ws = np.arange(max(1, -(-a // H)), W + 1)
                ws = ws[a % ws == 0]
                if len(ws):
                    w = int(ws[len(ws) // 2])
                    found[kind].append((W, H, w, a // w))
        if all(len(v) >= want for v in found.values()):
            break
    return found


def pair_boxes(pair, ox, oy, plain=False):
    """(K, C) = the outer and the inner box of `pair`, translated by integers; plain: the same IoU without the +1"""
    W, H, w, h = pair
    e = 0.0 if plain else 1.0
    return (np.array([ox, oy, ox + W - e, oy + H - e], np.float32), np.array([ox, oy, ox + w - e, oy + h - e], np.float32))


def plain_nms_sorted(d, thresh, ge=False):
    """float32 restatement of utils/box_utils.py:288-299 on rows sorted by descending score: no +1,
    union = (Sb - inter) + Sa in that order, suppress IoU > thresh (>= with ge).  -> kept positions"""
    d = np.ascontiguousarray(d, np.float32)
    x1, y1, x2, y2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    area = (x2 - x1) * (y2 - y1)
    t = np.float32(thresh)
    alive = np.ones(len(d), bool)
    keep = []
    for i in range(len(d)):
        if not alive[i]:
            continue
        keep.append(i)
        r = slice(i + 1, None)
        w = np.maximum(np.minimum(x2[i], x2[r]) - np.maximum(x1[i], x1[r]), np.float32(0))
        h = np.maximum(np.minimum(y2[i], y2[r]) - np.maximum(y1[i], y1[r]), np.float32(0))
        inter = w * h
        with np.errstate(divide='ignore', invalid='ignore'):
            iou = inter / ((area[r] - inter) + area[i])
        alive[r] &= ~((iou >= t) if ge else (iou > t))
    return np.asarray(keep, np.int64)


def nms_reference(d, thresh, ge, plain):
    return plain_nms_sorted(d, thresh, ge) if plain else nms_ref.nms_sorted_c(d, thresh, ge=ge)


# segment layouts: n rows; `dups` rows repeat row DUP_OF's box (always suppressed, they set the kept count of what follows);
# `slots` = (K row, C row, what the placement is meant to reach).  See `reach` for the categories.
SEGMENTS = {
    # chunk 0 keeps 255 (one dup): the 4-wide body covers kept 0..251, the tail 252..254; all C in chunk 1 (phase A)
    'phase_a': dict(n=300, dups=(255,), slots=((100, 260, 'a_body0'), (101, 261, 'a_body1'), (102, 262, 'a_body2'),
                                               (103, 263, 'a_body3'), (252, 264, 'a_tail'), (253, 265, 'a_tail'),
                                               (254, 266, 'a_tail'), (0, 267, 'a_body0'), (7, 268, 'a_body3'))),
    # sub-chunk 0 keeps 63: test_range(63, 127) of the later waves starts in the head loop
    'waves': dict(n=256, dups=(40,), slots=((64, 130, 'w_head'), (65, 131, 'w_body0'), (66, 132, 'w_body1'),
                                            (67, 133, 'w_body2'), (68, 195, 'w_body3'), (125, 134, 'w_tail'),
                                            (126, 196, 'w_tail'), (127, 135, 'w_tail'),
                                            (200, 210, 'ballot'), (201, 211, 'ballot'), (202, 212, 'ballot'),
                                            (203, 213, 'ballot'), (204, 255, 'ballot'))),
    # sub-chunk 0 keeps 61: three head iterations
    'waves3': dict(n=200, dups=(10, 20, 30), slots=((64, 130, 'w_head'), (65, 131, 'w_head'), (66, 132, 'w_head'),
                                                    (67, 133, 'w_body0'), (192, 199, 'ballot'), (193, 198, 'ballot'))),
    # more than kKeptLds kept boxes: phase A's part behind the LDS window, the same across waves and inside one wave
    'beyond': dict(n=2330, dups=(), slots=((2047, 2304, 'a_body3'), (2048, 2305, 'a_beyond'), (2100, 2306, 'a_beyond'),
                                           (2303, 2307, 'a_beyond'), (2050, 2120, 'w_beyond'), (2049, 2200, 'w_beyond'),
                                           (2310, 2315, 'ballot'), (2311, 2329, 'ballot'), (3, 2308, 'a_body3'))),
}
DUP_OF = 5          # a filler row no slot uses
REACHES = ('ballot', 'w_head', 'w_body0', 'w_body1', 'w_body2', 'w_body3', 'w_tail', 'w_beyond',
           'a_body0', 'a_body1', 'a_body2', 'a_body3', 'a_tail', 'a_beyond')


def borderline_segment(name, thresh, rot=0, plain=False):
    """-> (rows [n,5] sorted by descending score, slots [(K row, C row, reach, kind, pair)]).  Slot i takes a pair of kind
    KINDS[(i + rot) % 5]; everything else is `disjoint` filler, which outscores nothing it overlaps."""
    lay = SEGMENTS[name]
    n = lay['n']
    rows = np.zeros((n, 5), np.float32)
    rows[:, :4] = disjoint(n)
    rows[:, 4] = np.linspace(0.99, 0.02, n, dtype=np.float32)
    for r in lay['dups']:
        rows[r, :4] = rows[DUP_OF, :4]
    pairs = borderline_pairs(thresh)
    slots = []
    for i, (kr, cr, what) in enumerate(lay['slots']):
        kind = KINDS[(i + rot) % len(KINDS)]
        pair = pairs[kind][(i // len(KINDS) + rot) % len(pairs[kind])]
        rows[kr, :4], rows[cr, :4] = pair_boxes(pair, 3000.0 + 1300.0 * i, 50000.0, plain)
        slots.append((kr, cr, what, kind, pair))
    return rows, slots


def reach(rows_n, keep, k_row, c_row):
    """which loop of nms_segments_kernel compares the candidate at c_row with the kept box at k_row, given the reference
    keep list (restates the chunk / sub-chunk walk and test_range's head, 4-wide body, tail and beyond-LDS parts)"""
    keep = np.asarray(keep)
    chunk, sub, lds = CONSTANTS['kNmsChunk'], CONSTANTS['kNmsSubChunk'], CONSTANTS['kKeptLds']
    kept_before = lambda r: int(np.searchsorted(keep, r))           # noqa: E731
    ki = kept_before(k_row)
    assert ki < len(keep) and keep[ki] == k_row, 'K is not kept'
    c0 = c_row // chunk * chunk

    def in_range(i0, i1, tag):
        assert i0 <= ki < i1
        lds_end = min(i1, lds)
        if ki >= lds_end:
            return tag + '_beyond'
        head_end = min(lds_end, (i0 + 3) // 4 * 4)
        if ki < head_end:
            return tag + '_head'
        body_end = head_end + (lds_end - head_end) // 4 * 4
        return tag + '_body%d' % (ki & 3) if ki < body_end else tag + '_tail'
    if k_row < c0:
        return in_range(0, kept_before(c0), 'a')
    wk, wc = (k_row - c0) // sub, (c_row - c0) // sub
    if wk == wc:
        return 'ballot'
    return in_range(kept_before(c0 + sub * wk), kept_before(c0 + sub * (wk + 1)), 'w')


# ------------------------------------------------------------------ chain cases
A_N = (0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 4999)
B_P = (1, 2, 3, 64, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193)
D_B, D_T, D_P = (1, 7, 8, 9, 16, 17), (1, 3), (300, 200)
E_K = (1, 199, 200, 201, 255, 256, 261)          # total = 256: total - 1, total (kept total == k), total + 5
BASE_BIN = int(f2b(0.25)) >> 20                   # 0x3E8: [0.25, 0.28125)


def with_ties(bits):
    """the best two and the 4th/5th best of a ladder share their score (two ties, decided by prior order)"""
    bits = np.sort(np.asarray(bits, np.uint32))[::-1].copy()
    if len(bits) >= 2:
        bits[1] = bits[0]
    if len(bits) >= 5:
        bits[4] = bits[3]
    return bits


def case_A(n, topk):
    P, T = 5000, 2
    rng = np.random.RandomState(1000 + n)
    s = place(P, T, [with_ties(ladder_bits(n)), with_ties(ladder_bits(n + 1, LO_BITS + 77, HI_BITS - 33))], rng)
    return mostly_disjoint(P)[None], s[None], kw(max_per_image=topk)


def case_B(P, topk):
    B, T = 2, 2
    rng = np.random.RandomState(2000 + P)
    bx = np.stack([mostly_disjoint(P, rng) for _ in range(B)])
    s = np.stack([place(P, T, [ladder_bits(P, LO_BITS + 11 * b, HI_BITS), ladder_bits(P, LO_BITS, HI_BITS - 17 * b - 5)], rng)
                  for b in range(B)])
    return bx, s, kw(max_per_image=topk)


# family C: (bin, [sub,] count) lists with bins in descending order; 6000 candidates each.  expected: m of the first
# histogram, `above`, refined m, path
C_SPECS = {
    'C1': ([(BASE_BIN + 9, 400), (BASE_BIN + 8, 624), (BASE_BIN + 3, 2500), (BASE_BIN, 2476)],
           dict(m=1024, above=400, refined=None, path='lds')),
    'C2': ([(BASE_BIN + 9, 1023), (BASE_BIN + 8, 1), (BASE_BIN + 3, 2500), (BASE_BIN, 2476)],
           dict(m=1024, above=1023, refined=None, path='lds')),
    'C3': ([(BASE_BIN + 9, 500), (BASE_BIN + 8, 3596), (BASE_BIN + 3, 1904)],
           dict(m=4096, above=500, refined=None, path='lds')),
    'C4': ([(BASE_BIN + 9, 500), (BASE_BIN + 8, 2000, 300), (BASE_BIN + 8, 1999, 230)] +
           [(BASE_BIN + 8, 1000 - i, 511 if i < 6 else 1) for i in range(7)] + [(BASE_BIN + 3, 1903)],
           dict(m=4097, above=500, refined=1030, path='refined')),
    'C5': ([(BASE_BIN + 9, 500), (BASE_BIN + 8, 2000, 100), (BASE_BIN + 8, 1999, 3496), (BASE_BIN + 8, 5, 400),
            (BASE_BIN + 3, 1504)], dict(m=4496, above=500, refined=4096, path='refined')),
    'C6': ([(BASE_BIN + 9, 500), (BASE_BIN + 8, 2000, 100), (BASE_BIN + 8, 1999, 3497), (BASE_BIN + 8, 5, 400),
            (BASE_BIN + 3, 1503)], dict(m=4497, above=500, refined=4097, path='full')),
}


def case_C(name, boxes):
    P, T = 6000, 2
    rng = np.random.RandomState(3000 + int(name[1]))
    bits = bits_in_bins(C_SPECS[name][0])
    assert len(bits) == P
    s = place(P, T, [bits, bits], rng)
    bx = disjoint(P) if boxes == 'disjoint' else identical(P)
    return bx[None], s[None], kw()


def d_counts(B, T, P):
    return [[(37 * (b * T + c) + 11 * b) % (P + 1) if b or c else 0 for c in range(T)] for b in range(B)]


def case_D(B, T, P):
    rng = np.random.RandomState(4000 + 100 * B + 10 * T + P)
    # every third image has trained-like overlapping boxes, the others the shuffled grid
    bx = np.stack([clustered(P, 4100 + b) if b % 3 == 2 else mostly_disjoint(P, rng) for b in range(B)])
    cnt = d_counts(B, T, P)
    s = np.stack([place(P, T, [ladder_bits(cnt[b][c], LO_BITS + 1000 * b + 13 * c, HI_BITS - 7 * b) for c in range(T)], rng)
                  for b in range(B)])
    return bx, s, kw(max_per_image=100)


def case_E_all(P, T):
    """every prior a candidate of every class, nothing suppressed: P * T kept"""
    rng = np.random.RandomState(5000 + 10 * P + T)
    s = place(P, T, [ladder_bits(P, LO_BITS + 5 * c, HI_BITS - 3 * c) for c in range(T)], rng)
    return disjoint(P)[None], s[None], kw()


def case_E_k(k):
    bx, s, k_ = case_E_all(64, 4)
    return bx, s, dict(k_, max_per_image=k)


def case_E_ties(r):
    """P = 64, T = 8, all kept, k = 200: 199 distinct scores above v, r rows at v spread over the classes, the rest below"""
    P, T, k = 64, 8, 200
    rng = np.random.RandomState(5500 + r)
    v = int(f2b(0.4))
    bits = np.concatenate([v + 1 + 16 * np.arange(k - 1), np.full(r, v), v - 1 - 16 * np.arange(P * T - (k - 1) - r)])
    bits = rng.permutation(bits.astype(np.uint32)).reshape(T, P)
    s = place(P, T, list(bits), rng)
    return disjoint(P)[None], s[None], kw(max_per_image=k)


def case_E_bytes(which):
    """P = 64, T = 4, all kept, k = 200.  'low': the 256 kept scores share their top three bytes; 'top': powers of two
    2^-6 .. 2^60, which differ in the top byte (and bit 23) alone and reach the high histogram bins"""
    P, T = 64, 4
    rng = np.random.RandomState(5600)
    if which == 'low':
        bits = (int(f2b(0.3)) & ~0xFF) + np.arange(256)
    else:
        bits = f2b(np.ldexp(np.float32(1), -6 + np.arange(256) % 67).astype(np.float32))
    bits = rng.permutation(bits.astype(np.uint32)).reshape(T, P)
    s = place(P, T, list(bits), rng)
    return disjoint(P)[None], s[None], kw()


def case_F_equal():
    """conf_thresh = 0.01: scores bit-equal to it are out, the next float up is in"""
    P, T = 300, 2
    rng = np.random.RandomState(6001)
    t = int(f2b(CONF))
    per = [np.concatenate([ladder_bits(40 + c), np.full(30, t), np.full(30, t + 1), np.full(20, t - 1)]) for c in range(T)]
    return mostly_disjoint(P)[None], place(P, T, per, rng)[None], kw()


def case_F_zero():
    """conf_thresh = 0: +0, -0 and negatives are out; denormals are in and land in bin 0"""
    P, T = 300, 2
    rng = np.random.RandomState(6002)
    per = []
    for c in range(T):
        special = np.array([0, 0, 0x80000000, 0x80000000, 0x80000001, int(f2b(-0.5)), int(f2b(-1e-30)), 1, 2, 3, 0x1234,
                            0x7FFFFF, 0x800000, 0x800001], np.uint32)
        per.append(np.concatenate([ladder_bits(60 + c), special, np.arange(5 + c, 40, dtype=np.uint32) * 3]))
    s = place(P, T, per, rng, below=-0.25)
    return mostly_disjoint(P)[None], s[None], kw(conf_thresh=0.0)


def case_F_nan():
    P, T = 300, 2
    rng = np.random.RandomState(6003)
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], np.uint32)
    per = [np.concatenate([ladder_bits(150 + c), np.tile(nan, 10)]) for c in range(T)]
    return mostly_disjoint(P)[None], place(P, T, per, rng)[None], kw()


def case_F_ge(ge, thresh):
    """P = 300, T = 2: ten pairs at the NMS threshold (two of every kind) among filler; class 2 scores the inner box of
    every pair above the outer one"""
    P, T = 300, 2
    rng = np.random.RandomState(6004)
    bx = disjoint(P)
    s = place(P, T, [ladder_bits(P), ladder_bits(P, LO_BITS + 9, HI_BITS - 9)], rng)
    pairs = borderline_pairs(thresh)
    for i in range(10):
        k_box, c_box = pair_boxes(pairs[KINDS[i % 5]][i // 5], 3000.0 + 1300.0 * i, 50000.0)
        pk, pc = 20 * i + 3, 20 * i + 11
        bx[pk], bx[pc] = k_box, c_box
        hi, lo = max(s[pk, 1], s[pc, 1]), min(s[pk, 1], s[pc, 1])
        s[pk, 1], s[pc, 1] = hi, lo
        hi, lo = max(s[pk, 2], s[pc, 2]), min(s[pk, 2], s[pc, 2])
        s[pk, 2], s[pc, 2] = lo, hi
    return bx[None], s[None], kw(ge=ge, nms_thresh=thresh)


def case_G():
    """B = 2, P = 300, T = 3 with different counts everywhere; the output tests derive their caps from the oracle"""
    return case_D(2, 3, 300)


def case_H_steps():
    """the runs of one PostProcessor(B = 2, P = 6000, T = 2), in order"""
    P, T = 6000, 2
    rng = np.random.RandomState(8000)

    def two(bx_fn, bits_fn, **k):
        return (np.stack([bx_fn(), bx_fn()]), np.stack([place(P, T, [bits_fn(0), bits_fn(1)], rng) for _ in range(2)]), kw(**k))
    c5 = bits_in_bins(C_SPECS['C5'][0])
    steps = [
        ('all_pass_disjoint', two(lambda: disjoint(P), lambda c: ladder_bits(P, LO_BITS + c, HI_BITS))),
        ('ten_candidates', two(lambda: disjoint(P), lambda c: ladder_bits(10 + c))),
        ('redo', two(lambda: identical(P), lambda c: c5)),
        ('topk_off', two(lambda: mostly_disjoint(P), lambda c: ladder_bits(3000 + c), max_per_image=0)),
    ]
    bx, s, k = two(lambda: disjoint(P), lambda c: ladder_bits(700 + c))
    s[1, :, 1:] = 0.001                      # image 1 is empty
    steps.append(('empty_image', (bx, s, k)))
    return steps


def _cases():
    c = {}
    for n in A_N:
        for topk in (200, 0):
            c['A-n%d-k%d' % (n, topk)] = functools.partial(case_A, n, topk)
    for P in B_P:
        for topk in (0, 50):
            c['B-P%d-k%d' % (P, topk)] = functools.partial(case_B, P, topk)
    for name in sorted(C_SPECS):
        for bx in ('disjoint', 'identical'):
            c['%s-%s' % (name, bx)] = functools.partial(case_C, name, bx)
    for B in D_B:
        for T in D_T:
            for P in D_P:
                c['D-B%d-T%d-P%d' % (B, T, P)] = functools.partial(case_D, B, T, P)
    for P, T in ((256, 32), (256, 33), (257, 32), (257, 33), (64, 128), (64, 129)):
        c['E-all-P%d-T%d' % (P, T)] = functools.partial(case_E_all, P, T)
    for r in (1, 2, 57):
        c['E-ties-r%d' % r] = functools.partial(case_E_ties, r)
    for k in E_K:
        c['E-k%d' % k] = functools.partial(case_E_k, k)
    for which in ('low', 'top'):
        c['E-bytes-%s' % which] = functools.partial(case_E_bytes, which)
    c['F-equal'] = case_F_equal
    c['F-zero'] = case_F_zero
    c['F-nan'] = case_F_nan
    for ge in (False, True):
        for t in (0.45, 0.5):
            c['F-ge%d-t%d' % (ge, round(t * 100))] = functools.partial(case_F_ge, ge, t)
    return c


CASES = _cases()
# E-all totals: name -> kept boxes per image (P * T), which side of kStageCap / kStageMaxT they are on
E_TOTALS = {'E-all-P256-T32': 8192, 'E-all-P256-T33': 8448, 'E-all-P257-T32': 8224, 'E-all-P257-T33': 8481,
            'E-all-P64-T128': 8192, 'E-all-P64-T129': 8256}


@functools.lru_cache(maxsize=None)
def case(name):
    boxes, scores, k = CASES[name]()
    boxes = np.ascontiguousarray(boxes, np.float32)
    scores = np.ascontiguousarray(scores, np.float32)
    boxes.setflags(write=False)
    scores.setflags(write=False)
    return boxes, scores, k


@functools.lru_cache(maxsize=None)
def case_reference(name):
    boxes, scores, k = case(name)
    return reference(boxes, scores, **k)
