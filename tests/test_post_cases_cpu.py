"""The inputs of tests/test_gpu_post_edges.py and tests/test_gpu_nms_borderline.py reach what they claim -- proved here,
without a device, from the builders and the oracle alone.  The device exposes none of n, m, redo or `staged`, so a GPU
test whose input missed its branch would pass for nothing.

  constants guard   every size of post_cases.CONSTANTS is read back from csrc/ct_post.hip / csrc/ct_nms.hip; a retuned
                    constant fails here and post_cases.CONSTANT_CASES names the cases that have to move with it
  preconditions     a numpy model of select_sort_kernel's two histogram crossings and of the bounding pass gives each
                    case's n, m, `above`, refined m, redo and kept totals
  teeth             each family's inputs tell the oracle from a named, plausibly wrong variant of it
  NMS pairs         kind and distance of every pair in exact rational arithmetic, the placements, the plain-IoU reference
"""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import post_cases as pc
from oracle import box_ref, nms_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'context-transformer_amd', 'csrc')
C = pc.CONSTANTS


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------ constants guard
def _moved(name):
    return '%s moved: retune post_cases.CONSTANTS and the cases on it (%s)' % (name, pc.CONSTANT_CASES[name])


def test_constants_match_the_sources():
    post, nms = _src('ct_post.hip'), _src('ct_nms.hip')

    def const(text, ident):
        m = re.findall(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % ident, text)
        assert len(m) == 1, ident
        return int(m[0])
    for name in ('kSortThreads', 'kSelectBatch', 'kPartialMin', 'kHistBins', 'kStageCap', 'kStageMaxT', 'kPrefix'):
        assert const(post, name) == C[name], _moved(name)
    assert const(nms, 'kKeptLds') == C['kKeptLds'], _moved('kKeptLds')
    assert const(nms, 'kThreads') == C['kNmsChunk'], _moved('kNmsChunk')
    # one wave (64 candidates) per sub-chunk
    assert re.search(r'w < kThreads / (\d+)', nms).group(1) == str(C['kNmsSubChunk']), _moved('kNmsSubChunk')
    assert re.search(r'c0 \+ w \* (\d+) >= n', nms).group(1) == str(C['kNmsSubChunk']), _moved('kNmsSubChunk')
    # the template arguments of select_sort_kernel and the prior count that switches to the large one
    inst = set(re.findall(r'select_sort_kernel<(\d+), (true|false)>', post))
    assert inst == {(str(C['kLdsKeys']), 'true'), (str(C['kLdsKeys']), 'false'), (str(C['kLdsKeysLarge']), 'false')}, \
        _moved('kLdsKeys')
    assert set(re.findall(r'num_priors > (\d+)\)', post)) == {str(C['kLargePriors'])}, _moved('kLargePriors')
    # the histogram's two 11-bit fields
    assert re.search(r's_hist\[__float_as_uint\(v\[u\]\) >> (\d+)\]', post).group(1) == '20', _moved('kHistBins')
    assert re.search(r's_hist\[\(sb >> (\d+)\) & \(kHistBins - 1\)\]', post).group(1) == '9', _moved('kHistBins')
    assert 1 << (32 - 20 - 1) == C['kHistBins'] and 20 - 9 == 11
    # the radix select's four byte passes
    assert re.search(r'for \(int shift = 24; shift >= 0; shift -= 8\)', post)
    # blockIdx -> (image, class) in groups of 8 images, grid padded to a multiple of 8 images
    g = C['kImageGroup']
    assert re.search(r'\(\(int\)\(blockIdx\.x >> 3\) / T\) \* %d \+ \(int\)\(blockIdx\.x & %d\)' % (g, g - 1), post), \
        _moved('kImageGroup')
    assert len(re.findall(r'sort_grid\(%d \* \(\(batch \+ %d\) / %d\) \* num_fg\)' % (g, g - 1, g), post)) == 3, \
        _moved('kImageGroup')
    # make_thr's band
    band = re.search(r'r\.lo = t \* \(1\.f - (\S+)f\);\s*r\.hi = t \* \(1\.f \+ (\S+)f\);', nms)
    assert band and float(band.group(1)) == float(band.group(2)) == C['kThrBand'], _moved('kThrBand')
    assert set(pc.CONSTANT_CASES) == set(C)


# ------------------------------------------------------------------ preconditions
def _segments(scores):
    B, _, T1 = scores.shape
    return [(b, c) for b in range(B) for c in range(T1 - 1)]


def _kept_totals(name, **over):
    boxes, scores, k = pc.case(name)
    res = pc.reference(boxes, scores, **dict(k, max_per_image=0, **over))
    return [sum(len(i) for _, i in per) for per in res]


def _prefix_cut_model(boxes, scores, k):
    """per image: (bounding pass kept total, [redo per class]) of the top-k route, from the oracle and cut_model"""
    out = []
    for b in range(scores.shape[0]):
        kept_scores, models = [], []
        for c in range(scores.shape[2] - 1):
            s = scores[b, :, c + 1]
            inds = np.where(s > np.float32(k['conf_thresh']))[0]
            order = inds[nms_ref.stable_desc_order(s[inds])]
            models.append((pc.cut_model(pc.f2b(s[inds])), s[order]))
            head = order[:pc.K_PREFIX]
            d = np.hstack((boxes[b, head], s[head, None])).astype(np.float32).reshape(-1, 5)
            kept_scores.append(d[nms_ref.nms_sorted_c(d, k['nms_thresh'], ge=k['ge']), 4])
        alls = np.sort(np.hstack(kept_scores))
        total, kk = len(alls), k['max_per_image']
        thr = alls[-kk] if total > kk else np.float32(0)
        redo = []
        for model, sorted_scores in models:
            m = {'all': model['n'], 'lds': model['m'], 'refined': model['refined'], 'full': model['n']}[model['path']]
            length = int((sorted_scores[:m] >= thr).sum())
            redo.append(length == m and m < model['n'])
        out.append((total, redo))
    return out


@pytest.mark.parametrize('topk', [200, 0])
@pytest.mark.parametrize('n', pc.A_N)
def test_family_a_candidate_counts(n, topk):
    name = 'A-n%d-k%d' % (n, topk)
    boxes, scores, k = pc.case(name)
    assert scores.shape == (1, 5000, 3) and k['max_per_image'] == topk
    models = [pc.cut_model(pc.candidate_bits(scores, 0, c)) for c in range(2)]
    assert [m['n'] for m in models] == [n, n + 1]
    for m in models:
        assert m['path'] == ('all' if m['n'] <= C['kPartialMin'] else 'lds')         # scores span many bins
        assert m['m'] <= C['kLdsKeys'] and m['m'] >= min(m['n'], C['kPartialMin'])
    if n >= 1023:
        assert _kept_totals(name)[0] > 200
        if topk:
            assert sum(len(i) for _, i in pc.case_reference(name)[0]) in range(200, 204)
    for c in range(2):                                                                # candidates at shuffled priors
        pos = np.where(scores[0, :, c + 1] > np.float32(pc.CONF))[0]
        step = np.diff(scores[0, pos, c + 1])
        assert n < 3 or ((step > 0).any() and (step < 0).any())


@pytest.mark.parametrize('P', pc.B_P)
def test_family_b_every_prior_is_a_candidate(P):
    for topk in (0, 50):
        boxes, scores, k = pc.case('B-P%d-k%d' % (P, topk))
        assert scores.shape == (2, P, 3) and k['max_per_image'] == topk
        for b, c in _segments(scores):
            bits = pc.candidate_bits(scores, b, c)
            assert len(bits) == P and len(np.unique(bits)) == P
        if P >= 64:
            assert all(t > 50 for t in _kept_totals('B-P%d-k50' % P))


@pytest.mark.parametrize('name', sorted(pc.C_SPECS))
def test_family_c_prefix_sizes(name):
    want = pc.C_SPECS[name][1]
    for bx in ('disjoint', 'identical'):
        boxes, scores, k = pc.case('%s-%s' % (name, bx))
        assert scores.shape == (1, 6000, 3) and k['max_per_image'] == 200
        for c in range(2):
            got = pc.cut_model(pc.candidate_bits(scores, 0, c))
            assert got == dict(want, n=6000), (name, got)
        (total, redo), = _prefix_cut_model(boxes, scores, k)
        assert total == pc.bounding_kept(boxes, scores, 0)
        if bx == 'identical':
            # every segment flagged and sorted again in full -- but for C6, whose first launch already sorted everything
            assert total == 2 < 200 and redo == [want['path'] != 'full'] * 2
        else:
            assert total == 2 * C['kPrefix'] >= 200 and redo == [False, False]
    assert {'C1': 1024, 'C2': 1024, 'C3': 4096, 'C4': 4097}.get(name, want['m']) == want['m']
    assert {'C4': 1030, 'C5': 4096, 'C6': 4097}.get(name) == want['refined']
    assert name != 'C2' or want['above'] == 1023


@pytest.mark.parametrize('P', pc.D_P)
@pytest.mark.parametrize('T', pc.D_T)
@pytest.mark.parametrize('B', pc.D_B)
def test_family_d_every_segment_is_its_own(B, T, P):
    name = 'D-B%d-T%d-P%d' % (B, T, P)
    boxes, scores, k = pc.case(name)
    assert scores.shape == (B, P, T + 1)
    counts = [len(pc.candidate_bits(scores, b, c)) for b, c in _segments(scores)]
    assert counts == [x for row in pc.d_counts(B, T, P) for x in row]
    assert len(set(counts)) == len(counts) and 0 in counts
    want = pc.case_reference(name)
    seen = set()
    for per in want:
        for rows, idx in per:
            key = rows.tobytes()
            assert key not in seen
            seen.add(key)
    assert all(not np.array_equal(boxes[0], boxes[b]) for b in range(1, B))
    # teeth: class columns shifted by one, images swapped
    if T > 1:
        shifted = np.concatenate([scores[:, :, :1], np.roll(scores[:, :, 1:], 1, axis=2)], 2)
        assert not pc.same_result(want, pc.reference(boxes, shifted, **k))
    if B > 1:
        assert not pc.same_result(want, pc.reference(boxes[::-1], scores[::-1], **k))
        for b in range(B - 1):                 # any two neighbouring images, the 8-image groups' edges among them
            order = list(range(B))
            order[b], order[b + 1] = order[b + 1], order[b]
            sw = [want[i] for i in order]
            assert not pc.same_result(want, sw)
    if P > C['kPrefix']:
        assert any(sum(len(i) for _, i in per) >= k['max_per_image'] for per in want) or B * T < 3


def test_family_e_kept_totals_sit_on_the_staging_limits():
    for name, total in pc.E_TOTALS.items():
        boxes, scores, k = pc.case(name)
        _, P, T1 = scores.shape
        T = T1 - 1
        assert _kept_totals(name) == [total] == [P * T]
        staged_topk = total <= C['kStageCap'] and T <= C['kStageMaxT']
        if P > C['kPrefix']:                    # the bounding pass keeps kPrefix per class: prefix_cut_kernel's select
            bound = pc.bounding_kept(boxes, scores, 0)
            assert bound == C['kPrefix'] * T
            assert (bound <= C['kStageCap']) == (T == 32) and not staged_topk
        elif P == 256:
            assert staged_topk == (T == 32)     # 8192 staged, 8448 not
        else:
            assert staged_topk == (T == 128) and total <= C['kStageCap'] + 64     # T = 129: un-staged by the class count
        assert sum(len(i) for _, i in pc.case_reference(name)[0]) == 200


@pytest.mark.parametrize('r', [1, 2, 57])
def test_family_e_ties_at_the_cut(r):
    name = 'E-ties-r%d' % r
    boxes, scores, k = pc.case(name)
    want = pc.case_reference(name)[0]
    kk = k['max_per_image']
    alls = np.sort(np.hstack([rows[:, 4] for rows, _ in want]))[::-1]
    assert len(alls) == kk - 1 + r
    v = alls[kk - 1]
    with_v = [int((rows[:, 4] == v).sum()) for rows, _ in want]
    assert sum(with_v) == r and (alls > v).sum() == kk - 1
    assert r == 1 or sum(1 for x in with_v if x) >= 2
    assert not pc.same_result(pc.case_reference(name), pc.reference(boxes, scores, **k, variant='cut_gt'))
    assert not pc.same_result(pc.case_reference(name), pc.reference(boxes, scores, **k, variant='k_minus'))
    # k + 1 lands on the same value when the k-th is shared
    assert pc.same_result(pc.case_reference(name), pc.reference(boxes, scores, **k, variant='k_plus')) == (r > 1)


@pytest.mark.parametrize('k', pc.E_K)
def test_family_e_k_values(k):
    name = 'E-k%d' % k
    boxes, scores, kwargs = pc.case(name)
    total, = _kept_totals(name)
    assert total == 256 and kwargs['max_per_image'] == k
    assert set(pc.E_K) == {1, 199, 200, 201, total - 1, total, total + 5}
    out = sum(len(i) for _, i in pc.case_reference(name)[0])
    assert out == min(k, total)                                   # distinct scores: exactly k rows
    differs = {v: not pc.same_result(pc.case_reference(name), pc.reference(boxes, scores, **kwargs, variant=v))
               for v in ('k_plus', 'k_minus', 'cut_gt')}
    # k >= total has nothing to cut: k + 1 cannot show there, k - 1 shows only at k == total
    assert differs == {'k_plus': k < total, 'k_minus': k <= total, 'cut_gt': k < total}


def test_family_e_byte_structure():
    for which in ('low', 'top'):
        name = 'E-bytes-%s' % which
        boxes, scores, k = pc.case(name)
        assert _kept_totals(name) == [256]
        bits = np.hstack([pc.candidate_bits(scores, 0, c) for c in range(4)])
        assert len(bits) == 256
        if which == 'low':
            assert len(np.unique(bits >> 8)) == 1 and len(np.unique(bits & 0xFF)) == 256
        else:
            assert not (bits & 0x007FFFFF).any() and len(np.unique(bits)) == 67
            v = pc.b2f(bits)
            assert v.min() == 2.0 ** -6 and v.max() == 2.0 ** 60
            assert (bits >> 20).max() == (127 + 60) * 8 and (bits >> 20).min() == (127 - 6) * 8     # bins 968 .. 1496
        # 'top' has about four rows per value: the cut falls inside a tie, where only `>` is sure to show
        for v in ('k_minus', 'k_plus', 'cut_gt') if which == 'low' else ('cut_gt',):
            assert not pc.same_result(pc.case_reference(name), pc.reference(boxes, scores, **k, variant=v)), (which, v)


def test_family_f_threshold_semantics():
    t = int(pc.f2b(pc.CONF))
    boxes, scores, k = pc.case('F-equal')
    bits = pc.f2b(scores[0, :, 1:])
    assert (bits == t).sum() == 60 and (bits == t + 1).sum() == 60
    assert pc.b2f(np.uint32(t + 1)) == np.nextafter(np.float32(pc.CONF), np.float32(1))
    want = pc.case_reference('F-equal')
    out_bits = np.hstack([pc.f2b(rows[:, 4]) for rows, _ in want[0]])
    assert (out_bits == t + 1).sum() > 20 and not (out_bits <= t).any()
    assert not pc.same_result(want, pc.reference(boxes, scores, **k, variant='conf_ge'))

    boxes, scores, k = pc.case('F-zero')
    assert k['conf_thresh'] == 0.0
    bits = pc.f2b(scores[0, :, 1:])
    assert (bits == 0).any() and (bits == 0x80000000).any() and (bits == 1).any() and (bits > 0x80000000).any()
    cand = np.hstack([pc.candidate_bits(scores, 0, c, 0.0) for c in range(2)])
    assert ((cand > 0) & (cand < 0x80000000)).all() and (cand == 1).sum() == 2
    assert ((cand >> 20) == 0).sum() >= 40 and (cand < 0x00800000).sum() >= 40         # denormals: bin 0
    want = pc.case_reference('F-zero')
    out_bits = np.hstack([pc.f2b(rows[:, 4]) for rows, _ in want[0]])
    assert (out_bits == 1).any()
    assert not pc.same_result(want, pc.reference(boxes, scores, **k, variant='conf_ge'))    # would let +0 and -0 in

    boxes, scores, k = pc.case('F-nan')
    s = scores[0, :, 1:]
    assert np.isnan(s).sum() == 80 and (pc.f2b(s) == 0xFFC00000).any() and (pc.f2b(s) == 0x7F800001).any()
    want = pc.case_reference('F-nan')
    assert not any(np.isnan(rows).any() for rows, _ in want[0])
    assert [len(pc.candidate_bits(scores, 0, c)) for c in range(2)] == [150, 151]


@pytest.mark.parametrize('thresh', [0.45, 0.5])
@pytest.mark.parametrize('ge', [False, True])
def test_family_f_ge_through_the_chain(ge, thresh):
    name = 'F-ge%d-t%d' % (ge, round(thresh * 100))
    boxes, scores, k = pc.case(name)
    assert k['ge'] == ge and k['nms_thresh'] == thresh
    want = pc.case_reference(name)
    assert not pc.same_result(want, pc.reference(boxes, scores, **k, variant='ge_flip'))
    for c in range(2):
        kept = set(want[0][c][1].tolist())
        for i in range(10):
            pk, pc_ = 20 * i + 3, 20 * i + 11
            first, second = (pk, pc_) if c == 0 else (pc_, pk)
            kind = pc.KINDS[i % 5]
            gone = {'equal': ge, 'below': False, 'above': True, 'out_below': False, 'out_above': True}[kind]
            assert scores[0, first, c + 1] > scores[0, second, c + 1]
            # the cut at 200 of 600 may drop rows, never add them
            assert not (gone and second in kept), (c, i, kind)
    nocut = pc.reference(boxes, scores, **dict(k, max_per_image=0))
    for c in range(2):
        kept = set(nocut[0][c][1].tolist())
        for i in range(10):
            second = 20 * i + (11 if c == 0 else 3)
            gone = {'equal': ge, 'below': False, 'above': True, 'out_below': False, 'out_above': True}[pc.KINDS[i % 5]]
            assert (second not in kept) == gone


def test_family_a_tie_order_has_teeth():
    for n in pc.A_N:
        for topk in (200, 0):
            name = 'A-n%d-k%d' % (n, topk)
            boxes, scores, k = pc.case(name)
            differs = not pc.same_result(pc.case_reference(name), pc.reference(boxes, scores, **k, variant='tie_desc'))
            assert differs == (n >= 1), name            # n = 0: class 2 has a single candidate, nothing can tie


def test_family_g_caps_bite():
    boxes, scores, k = pc.case_G()
    want = pc.reference(boxes, scores, **k)
    counts = sorted(len(i) for per in want for _, i in per)
    assert counts[-1] > counts[-2] > 4 and counts[0] == 0      # one segment alone exceeds cap = largest - 1
    assert len(set(counts)) == len(counts)


def test_family_h_sequence_changes_regime():
    steps = dict(pc.case_H_steps())
    assert list(steps) == ['all_pass_disjoint', 'ten_candidates', 'redo', 'topk_off', 'empty_image']
    for tag, (boxes, scores, k) in steps.items():
        assert scores.shape == (2, 6000, 3)
    boxes, scores, k = steps['all_pass_disjoint']
    assert all(len(pc.candidate_bits(scores, b, c)) == 6000 for b, c in _segments(scores))
    assert [r for _, r in _prefix_cut_model(boxes, scores, k)] == [[False, False]] * 2
    boxes, scores, k = steps['ten_candidates']
    assert [len(pc.candidate_bits(scores, b, c)) for b, c in _segments(scores)] == [10, 11, 10, 11]
    boxes, scores, k = steps['redo']
    assert [r for _, r in _prefix_cut_model(boxes, scores, k)] == [[True, True]] * 2
    assert pc.cut_model(pc.candidate_bits(scores, 1, 1))['path'] == 'refined'
    assert steps['topk_off'][2]['max_per_image'] == 0
    boxes, scores, k = steps['empty_image']
    assert [len(pc.candidate_bits(scores, b, c)) for b, c in _segments(scores)] == [700, 701, 0, 0]


def test_every_case_has_a_precondition_test():
    fams = {n.split('-')[0][0] for n in pc.CASES}
    assert fams == set('ABCDEF') and len(pc.CASES) == 26 + 32 + 12 + 24 + 18 + 7


# ------------------------------------------------------------------ NMS pairs at the threshold
@pytest.mark.parametrize('thresh', pc.NMS_THRESHOLDS)
def test_borderline_pairs_are_what_they_say(thresh):
    pairs = pc.borderline_pairs(thresh)
    t32 = np.float32(thresh)
    T = Fraction(float(t32))
    for kind in pc.KINDS:
        assert len(pairs[kind]) >= 12
        for W, H, w, h in pairs[kind]:
            assert 0 < w <= W <= 1200 and 0 < h <= H <= 1200 and W * H + w * h < 1 << 24
            exact = Fraction(w * h, W * H)
            q = np.float32(w * h) / np.float32(W * H)
            rel = abs(float((exact - T) / T))
            if kind == 'equal':
                assert q == t32 and rel < 6e-8
            elif kind in ('below', 'above'):
                assert rel < 5e-6 and (q < t32) == (kind == 'below') and q != t32 and (exact < T) == (kind == 'below')
            else:
                assert 2e-5 <= rel <= 5e-5 and (exact < T) == (kind == 'out_below')
            assert (rel < C['kThrBand'] * 0.5) == (kind in ('equal', 'below', 'above'))
            for plain in (False, True):
                d = np.zeros((2, 5), np.float32)
                d[0, :4], d[1, :4] = pc.pair_boxes((W, H, w, h), 3000.0, 50000.0, plain)
                d[:, 4] = (0.9, 0.8)
                for ge in (False, True):
                    gone = {'equal': ge, 'below': False, 'above': True, 'out_below': False, 'out_above': True}[kind]
                    assert list(pc.nms_reference(d, thresh, ge, plain)) == ([0] if gone else [0, 1]), (kind, plain, ge)
                    if not plain:
                        assert list(nms_ref.nms_sorted(d, thresh, ge=ge)) == ([0] if gone else [0, 1])
    assert pc.pair_kind(25 * 45, 50 * 50, 0.45)[0] == 'equal'          # 25 x 45 inside 50 x 50


@pytest.mark.parametrize('plain', [False, True])
@pytest.mark.parametrize('thresh', pc.NMS_THRESHOLDS)
def test_borderline_placements_reach_every_loop(thresh, plain):
    for ge in (False, True):
        reached = set()
        for name, lay in pc.SEGMENTS.items():
            kinds_at = {}
            for rot in range(len(pc.KINDS)):
                rows, slots = pc.borderline_segment(name, thresh, rot, plain)
                assert len(rows) == lay['n'] and (np.diff(rows[:, 4]) < 0).all()
                keep = pc.nms_reference(rows, thresh, ge, plain)
                kept = set(keep.tolist())
                assert not kept & set(lay['dups'])
                for kr, cr, what, kind, pair in slots:
                    assert pc.reach(len(rows), keep, kr, cr) == what, (name, rot, kr, cr)
                    gone = {'equal': ge, 'below': False, 'above': True, 'out_below': False, 'out_above': True}[kind]
                    assert (cr not in kept) == gone
                    reached.add((what, kind))
                    kinds_at.setdefault((kr, cr), set()).add(kind)
                # nothing but the dups and the pairs' inner boxes is ever suppressed
                assert set(range(len(rows))) - kept <= set(lay['dups']) | {cr for _, cr, _, _, _ in slots}
                if name in ('phase_a', 'waves'):       # the four lanes of one 4-wide group carry four different kinds
                    group = [s for s in slots if s[2].endswith(('body0', 'body1', 'body2', 'body3'))][:4]
                    assert len({s[3] for s in group}) == 4 and len({s[0] // 4 for s in group if name == 'phase_a'}) <= 1
            assert all(v == set(pc.KINDS) for v in kinds_at.values())
        assert reached == {(w, k) for w in pc.REACHES for k in pc.KINDS}
    assert pc.SEGMENTS['beyond']['n'] > C['kKeptLds'] + C['kNmsChunk']


def test_plain_reference_against_the_box_utils_goldens(golden):
    """post_cases.plain_nms_sorted on the inputs of tests/golden/box_ops.npz's bunms_* keep lists"""
    g = golden('box_ops.npz')
    priors = box_ref.prior_box(box_ref.ANCHOR_CFGS['VOC_300'])
    P = priors.shape[0]
    gen = torch.Generator().manual_seed(11)
    loc = torch.randn(2, P, 4, generator=gen)
    conf = torch.softmax(torch.randn(2, P, 20, generator=gen) * 2, -1)
    obj = torch.softmax(torch.randn(2, P, 2, generator=gen), -1)
    boxes, _ = box_ref.detect(loc, conf, obj, priors)
    sc = torch.rand(P, generator=gen)
    for ovt, topk in ((0.5, 200), (0.3, 400)):
        idx = sc.sort(0)[1][-topk:].flip(0).numpy()
        rows = np.hstack((boxes[0].numpy()[idx], sc.numpy()[idx, None])).astype(np.float32)
        keep = pc.plain_nms_sorted(rows, ovt)
        assert np.array_equal(idx[keep], g['bunms_%02d_%d_keep' % (int(ovt * 100), topk)])
