"""Matrix NMS on the MI355X (csrc/ct_matrix_nms.hip; ct_matrix_nms_batched_dev, ct_postprocess_batched_matrix and what is
built on them) against the host twin ct_cpu_matrix_nms.

Linear method: rows, positions and counts bit for bit.  Gaussian method: the two sides differ only by their libms' double exp
rounded to fp32 -- at most one fp32 ulp of decay -- and the product's rounding, so every score is within 2^-22 of the host's,
relatively; positions and order are the same where the host's own margins exceed that, so every Gaussian case first asserts,
from the twin's result, that consecutive emitted scores and the threshold are separated by at least 4 x 2^-22 relative."""
import functools

import numpy as np
import pytest
import torch

from ctdet import _lib, evaluate, ops, synth
from oracle import nms_ref
from test_gpu_soft_nms import (B, CONF, P, T, _bits, _cuda, _net300, _outputs, _pipeline_case, _prior_index, _topk_rule,
                               _valid_equal)
from test_matrix_nms_cpu import CHAIN, COPIES, DISJOINT, TIES, check_chain, check_copies, seg_rows

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
REL = 2.0 ** -22
SIZES = (1, 2, 37, 63, 64, 65, 255, 256, 257, 600, 1100)
GAUSS_CASES = ((1, 4321), (2, 7), (37, 7), (63, 4321), (64, 7), (65, 4321), (255, 4321), (256, 4321), (257, 7), (600, 4321),
               (1100, 7))


def _top():
    return _lib.lib().ct_matrix_nms_max_rows()


def _segments(segs, method, sigma=0.5, thr=0.001, pre_top=None, max_emit=0, tail=0, sentinel=-7.0):
    """One call over `segs` (host [n,5] arrays in pipeline order) followed by `tail` NaN rows -> per segment (rows, pos),
    after checking that the input is unchanged and that nothing outside the emitted rows, the counts of the segments or
    the workspace was written (the outputs are sentinel-filled; the workspace pointer sits inside a guard buffer)."""
    lens = [len(s) for s in segs]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    total = int(off[-1])
    host = np.full((total + tail, 5), np.nan, dtype=F)
    if total:
        host[:total] = np.concatenate([np.asarray(s, dtype=F).reshape(-1, 5) for s in segs])
    dets = _cuda(host)
    out = (torch.full((total + tail, 5), sentinel, device=DEV), torch.full((total + tail,), -7, device=DEV, dtype=torch.int32),
           torch.full((len(segs) + 3,), -7, device=DEV, dtype=torch.int32))
    need = _lib.lib().ct_matrix_nms_batched_workspace_bytes(total, len(segs))
    guard = 1024
    ws = torch.empty(need + 2 * guard, device=DEV, dtype=torch.uint8)
    ws.fill_(0xA5)
    ops.matrix_nms_batched(dets, _cuda(off), method, sigma, thr, _top() if pre_top is None else pre_top, max_emit,
                           max_seg_len=max(lens + [0]), out=(out[0], out[1], out[2][:len(segs)]),
                           workspace=ws[guard:guard + need])
    torch.cuda.synchronize()
    rows, pos, cnt = (t.cpu().numpy() for t in out)
    assert np.array_equal(_bits(dets.cpu().numpy()), _bits(host))                       # the input is not modified
    assert (cnt[len(segs):] == -7).all()
    wsh = ws.cpu().numpy()
    assert (wsh[:guard] == 0xA5).all() and (wsh[guard + need:] == 0xA5).all()          # nothing outside the workspace
    res = []
    for s, n in enumerate(lens):
        k = int(cnt[s])
        assert 0 <= k <= n, (s, n, k)
        a, b = int(off[s]), int(off[s + 1])
        assert (rows[a + k:b] == sentinel).all() and (pos[a + k:b] == -7).all(), s     # nothing past out_count rows
        res.append((rows[a:a + k].copy(), pos[a:a + k].copy()))
    assert (rows[total:] == sentinel).all() and (pos[total:] == -7).all()
    return res


def _host(rows, method, sigma=0.5, thr=0.001, pre_top=None, max_emit=0):
    return ops.cpu_matrix_nms(rows, method, sigma, thr, _top() if pre_top is None else pre_top, max_emit)


def _check_exact(rows, got, pos, want, wpos):
    assert len(got) == len(want), (len(got), len(want))
    assert np.array_equal(pos, wpos)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(rows[pos, :4]), _bits(got[:, :4])) and len(set(pos.tolist())) == len(pos)
    assert np.all(np.diff(got[:, 4]) <= 0)


def _margins(all_scores, thr):
    """From the twin's decayed scores of EVERY row (its result at threshold 0): the smallest relative gap between
    consecutive scores among the rows at or above thr, and the smallest relative distance of any row to thr."""
    s = np.sort(all_scores.astype(np.float64))[::-1]
    kept = s[s >= F(thr)]
    gap = float(np.min((kept[:-1] - kept[1:]) / kept[:-1])) if len(kept) > 1 else np.inf
    dist = float(np.min(np.abs(s - F(thr)) / F(thr))) if len(s) else np.inf
    return gap, dist


def _check_margins(rows, thr, sigma=0.5, pre_top=None):
    every, _ = _host(rows, 2, sigma, 0.0, pre_top)
    gap, dist = _margins(every[:, 4], thr)
    print('margins: consecutive %.3g threshold %.3g, needed %.3g' % (gap, dist, 4 * REL))
    assert gap >= 4 * REL and dist >= 4 * REL, (gap, dist)


def _check_gauss(rows, got, pos, want, wpos):
    assert len(got) == len(want), (len(got), len(want))
    assert np.array_equal(pos, wpos)
    assert np.array_equal(_bits(got[:, :4]), _bits(want[:, :4]))
    assert np.array_equal(_bits(rows[pos, :4]), _bits(got[:, :4]))
    d = np.abs(got[:, 4].astype(np.float64) - want[:, 4])
    print('scores not bit-equal: %d of %d, worst |dev - host| / host %.3g (bound %.3g)'
          % (int((_bits(got[:, 4]) != _bits(want[:, 4])).sum()), len(got),
             float((d / want[:, 4]).max()) if len(got) else 0.0, REL))
    assert np.all(d <= REL * want[:, 4])
    assert np.all(np.diff(got[:, 4]) <= 0)


# ------------------------------------------------------------------ single segments
@pytest.mark.parametrize('thr', [0.05, 0.001])
@pytest.mark.parametrize('seed', [4321, 7])
@pytest.mark.parametrize('n', SIZES)
def test_linear_equals_the_host_twin_bit_for_bit(n, seed, thr):
    rows = seg_rows(n, seed)
    ((got, pos),) = _segments([rows], 1, thr=thr)
    _check_exact(rows, got, pos, *_host(rows, 1, thr=thr))


@pytest.mark.parametrize('n,seed', GAUSS_CASES)
def test_gaussian_same_positions_scores_inside_the_bound(n, seed):
    rows = seg_rows(n, seed)
    _check_margins(rows, 0.05)
    ((got, pos),) = _segments([rows], 2, thr=0.05)
    _check_gauss(rows, got, pos, *_host(rows, 2, thr=0.05))


# ------------------------------------------------------------------ hand cases
def test_hand_cases_on_the_device():
    ((got, pos),) = _segments([CHAIN], 1)
    check_chain(got, pos)
    ((got0, pos0),) = _segments([COPIES], 1, thr=0.0)
    ((got, pos),) = _segments([COPIES], 1)
    check_copies(got0, pos0, got, pos)
    for method in (1, 2):
        ((got, pos),) = _segments([DISJOINT], method)
        assert pos.tolist() == [0, 1, 2, 3] and np.array_equal(_bits(got), _bits(DISJOINT))
    ((got, pos),) = _segments([COPIES], 2, thr=0.0)         # duplicates, Gaussian: finite too (the scores are far apart)
    want, wpos = _host(COPIES, 2, thr=0.0)
    assert np.isfinite(got).all() and pos.tolist() == wpos.tolist() == [0, 3, 1, 2]
    assert np.all(np.abs(got[:, 4].astype(np.float64) - want[:, 4]) <= REL * want[:, 4])


# ------------------------------------------------------------------ pre_top
@pytest.mark.parametrize('n', [63, 64, 65])
def test_pre_top_is_the_rule_on_the_first_rows(n):
    rows = seg_rows(n, 4321)
    ((got, pos),) = _segments([rows], 1, pre_top=64)
    _check_exact(rows, got, pos, *_host(rows[:64], 1))
    assert (pos < 64).all()


@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_pre_top_at_the_largest_value_the_kernel_holds(delta):
    top = _top()
    rows = seg_rows(top + delta, 4321)
    ((got, pos),) = _segments([rows], 1, pre_top=top)
    _check_exact(rows, got, pos, *_host(rows[:top], 1, pre_top=top + 8))
    assert (pos < top).all()


# ------------------------------------------------------------------ the emission limit
@pytest.mark.parametrize('method', [1, 2])
def test_emission_limit_gives_a_prefix(method):
    for n, seed in ((600, 4321), (1100, 7)):
        rows = seg_rows(n, seed)
        (full,) = _segments([rows], method)
        assert len(full[0]) > 20
        for k in (1, 5, 20):
            ((got, pos),) = _segments([rows], method, max_emit=k)
            assert len(got) == k, (n, k, len(got))
            assert np.array_equal(_bits(got), _bits(full[0][:k])) and np.array_equal(pos, full[1][:k]), (n, k)


def test_emission_limit_keeps_ties_lower_position_first():
    for method in (1, 2):
        ((got, pos),) = _segments([TIES], method, max_emit=2)
        assert pos.tolist() == [0, 1, 2, 3], (method, pos)
        assert np.array_equal(_bits(got), _bits(TIES[:4]))
        ((got, pos),) = _segments([TIES], method, max_emit=1)
        assert pos.tolist() == [0]
        ((got, pos),) = _segments([TIES], method)
        assert pos.tolist() == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------ batching
@pytest.mark.parametrize('method', [1, 2])
def test_batched_segments_equal_single_segments(method):
    lens = [257, 1, 0, 600, 65]
    segs = [seg_rows(n, 100 + i) if n else np.zeros((0, 5), dtype=F) for i, n in enumerate(lens)]
    batched = _segments(segs, method, tail=50)
    for i, (s, (got, pos)) in enumerate(zip(segs, batched)):
        if not len(s):
            assert len(got) == 0
            continue
        ((one, one_pos),) = _segments([s], method)
        assert np.array_equal(_bits(got), _bits(one)) and np.array_equal(pos, one_pos), i
        if method == 1:
            _check_exact(s, got, pos, *_host(s, 1))
    assert sum(len(g) for g, _ in batched) > 200


# ------------------------------------------------------------------ the post-processing entry
THR = 0.001


@functools.lru_cache(maxsize=None)
def _pipeline_reference(method, mpi, pre_top, thr=THR):
    """Per (image, class): candidates in the pipeline's order and the twin on them (each segment stops after mpi rows, as
    the entry has it) -> (prior indices of the candidates, rows the twin emits, the candidates themselves)."""
    boxes, scores = _pipeline_case()
    out = {}
    for b in range(B):
        for c in range(T):
            inds = np.where(scores[b, :, 1 + c] > F(CONF))[0]
            inds = inds[nms_ref.stable_desc_order(scores[b, inds, 1 + c])]
            cand = np.hstack([boxes[b, inds], scores[b, inds, 1 + c][:, None]]).astype(F)
            rows, _ = ops.cpu_matrix_nms(cand, method, 0.5, thr, pre_top, mpi)
            out[b, c] = (inds, rows, cand)
    return out


def _run_post(name, mpi, cap=None, pre_top=1024, thr=THR, vote=None):
    boxes, scores = _pipeline_case()
    pp = ops.PostProcessor(B, P, T, DEV, out_cap=cap or P)
    pp.out_dets.fill_(-7.0)
    pp.out_index.fill_(-7)
    pp.run(_cuda(boxes), _cuda(scores), CONF, 0.45, False, mpi, nms_method=name, soft_score_threshold=thr, box_vote=vote,
           matrix_pre_top=pre_top)
    torch.cuda.synchronize()
    return pp


@pytest.mark.parametrize('mpi,pre_top', [(0, 1024), (20, 1024), (20, 100)])
def test_postprocess_linear_equals_the_host_restatement(mpi, pre_top):
    ref = _pipeline_reference(1, mpi, pre_top)
    want = _topk_rule(ref, mpi)
    assert min(len(ref[k][2]) for k in ref) > 100                           # pre_top = 100 cuts every segment
    pp = _run_post('matrix_linear', mpi, pre_top=pre_top)
    assert int(pp.overflow.item()) == 0
    dets, cnt, idx = pp.out_dets.cpu().numpy(), pp.out_count.cpu().numpy(), pp.out_index.cpu().numpy()
    for (b, c), rows in want.items():
        assert cnt[b, c] == len(rows), (b, c, cnt[b, c], len(rows))
        assert np.array_equal(_bits(dets[b, c, :len(rows)]), _bits(rows)), (b, c)
        assert np.array_equal(idx[b, c, :len(rows)], _prior_index(ref[b, c], rows)), (b, c)
        assert (dets[b, c, len(rows):] == -7.0).all() and (idx[b, c, len(rows):] == -7).all()
        assert np.all(np.diff(dets[b, c, :len(rows), 4]) <= 0)
    if mpi:
        full = _pipeline_reference(1, 0, pre_top)
        assert any(len(want[k]) < len(full[k][1]) for k in want)            # the rule cut something


@pytest.mark.parametrize('mpi', [0, 20])
def test_postprocess_gaussian_inside_the_bound(mpi):
    ref = _pipeline_reference(2, mpi, 1024)
    want = _topk_rule(ref, mpi)
    every = _pipeline_reference(2, 0, 1024, 0.0)                             # the twin's decayed score of every candidate
    for key in every:
        gap, dist = _margins(every[key][1][:, 4], THR)
        assert gap >= 4 * REL and dist >= 4 * REL, (key, gap, dist)
    if mpi:                                                                  # the image's cut is a decision too
        for b in range(B):
            allsc = np.sort(np.concatenate([ref[b, c][1][:, 4] for c in range(T)]).astype(np.float64))
            assert (allsc[-mpi] - allsc[-mpi - 1]) / allsc[-mpi] >= 4 * REL
    pp = _run_post('matrix_gaussian', mpi)
    assert int(pp.overflow.item()) == 0
    dets, cnt, idx = pp.out_dets.cpu().numpy(), pp.out_count.cpu().numpy(), pp.out_index.cpu().numpy()
    for (b, c), rows in want.items():
        assert cnt[b, c] == len(rows), (b, c, cnt[b, c], len(rows))
        got = dets[b, c, :len(rows)]
        assert np.array_equal(_bits(got[:, :4]), _bits(rows[:, :4])), (b, c)
        assert np.all(np.abs(got[:, 4].astype(np.float64) - rows[:, 4]) <= REL * rows[:, 4]), (b, c)
        assert np.array_equal(idx[b, c, :len(rows)], _prior_index(ref[b, c], rows)), (b, c)
        assert np.all(np.diff(got[:, 4]) <= 0)


@pytest.mark.parametrize('name', ['matrix_linear', 'matrix_gaussian'])
def test_postprocess_overflow_and_guards(name):
    boxes, scores = _pipeline_case()
    cap, pad = 4, 256
    pp = ops.PostProcessor(B, P, T, DEV, out_cap=cap)
    big_d = torch.full((B * T * cap * 5 + 2 * pad,), -7.0, device=DEV)
    big_i = torch.full((B * T * cap + 2 * pad,), -7, device=DEV, dtype=torch.int32)
    pp.out_dets = big_d[pad:-pad].view(B, T, cap, 5)
    pp.out_index = big_i[pad:-pad].view(B, T, cap)
    pp.run(_cuda(boxes), _cuda(scores), CONF, 0.45, False, 20, nms_method=name)
    torch.cuda.synchronize()
    assert int(pp.overflow.item()) == 1
    with pytest.raises(_lib.CtdetError):
        pp.to_all_boxes()
    assert (pp.out_count.cpu().numpy() <= cap).all()
    for big in (big_d, big_i):
        h = big.cpu().numpy()
        assert (h[:pad] == -7).all() and (h[-pad:] == -7).all()
    roomy = _run_post(name, 20)
    want = roomy.out_dets.cpu().numpy()[:, :, :cap]
    cnt = pp.out_count.cpu().numpy()
    got = pp.out_dets.cpu().numpy()
    for b in range(B):
        for c in range(T):
            assert np.array_equal(_bits(got[b, c, :cnt[b, c]]), _bits(want[b, c, :cnt[b, c]]))


@pytest.mark.parametrize('name', ['matrix_linear', 'matrix_gaussian'])
def test_two_runs_and_a_side_stream_give_the_same_bits(name):
    first = _run_post(name, 20)
    a = (first.out_dets.cpu().numpy(), first.out_count.cpu().numpy(), first.out_index.cpu().numpy())
    second = _run_post(name, 20)
    boxes, scores = _pipeline_case()
    side = torch.cuda.Stream(device=DEV)
    third = ops.PostProcessor(B, P, T, DEV, out_cap=P)
    third.out_dets.fill_(-7.0)
    third.out_index.fill_(-7)
    db, ds = _cuda(boxes), _cuda(scores)
    busy = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    for _ in range(8):
        busy = busy @ busy * 1e-3                       # the main stream is busy meanwhile
    with torch.cuda.stream(side):
        third.run(db, ds, CONF, 0.45, False, 20, nms_method=name)
    torch.cuda.synchronize()
    for other in (second, third):
        b = (other.out_dets.cpu().numpy(), other.out_count.cpu().numpy(), other.out_index.cpu().numpy())
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------ composition
def test_box_voting_runs_after_it_and_leaves_scores_untouched():
    plain = _run_post('matrix_linear', 20)
    voted = _run_post('matrix_linear', 20, vote=0.5)
    a, b = plain.out_dets.cpu().numpy(), voted.out_dets.cpu().numpy()
    cnt = plain.out_count.cpu().numpy()
    assert np.array_equal(cnt, voted.out_count.cpu().numpy()) and cnt.sum() > 0
    assert np.array_equal(plain.out_index.cpu().numpy(), voted.out_index.cpu().numpy())
    mask = np.arange(a.shape[2])[None, None, :] < cnt[:, :, None]
    assert np.array_equal(_bits(a[..., 4])[mask], _bits(b[..., 4])[mask])
    assert not np.array_equal(_bits(a[..., :4])[mask], _bits(b[..., :4])[mask])          # the clustered boxes do move
    assert np.isfinite(b[mask]).all()


def test_voc_evaluator_takes_the_matrix_result():
    pp = _run_post('matrix_linear', 20)
    classes = ['__background__'] + ['c%d' % j for j in range(1, T + 1)]
    ids = ['img%d' % b for b in range(B)]
    all_boxes = pp.to_all_boxes()
    gt = {c: {} for c in classes[1:]}
    for j in range(1, T + 1):
        for b in range(B):
            d = all_boxes[b][j]
            assert len(d)
            gt[classes[j]][ids[b]] = {'bbox': np.round(d[::3][:3, :4]).astype(int), 'difficult': np.zeros(len(d[::3][:3]), bool)}
    ev = evaluate.DeviceVOCEvaluator(gt, classes, ids, DEV)
    ev.add(pp.out_dets, pp.out_count, list(range(B)))
    aps, mean = ev.finish()
    host = [[all_boxes[b][j] for b in range(B)] for j in range(T + 1)]
    want_aps, want_mean = evaluate.evaluate_detections(host, ids, gt, classes, stable=True)
    assert aps == want_aps and mean == want_mean and 0 < mean <= 1


# ------------------------------------------------------------------ the pipeline
def test_pipeline_matrix_linear_eager_graph_and_default_unchanged():
    from ctdet.pipeline import DetectionPipeline
    from data import VOC_300
    from layers.functions import PriorBox
    net = _net300()
    priors = PriorBox(VOC_300).forward()
    x = synth.images(2, 300, 'randn', 1234).cuda()
    mat = DetectionPipeline(net, priors, 2, 20, image_wh=(500, 375), max_per_image=1000, nms_method='matrix_linear', graph=True)
    mat.run(x)
    eager = _outputs(mat)
    mat.run(x)
    assert mat._graph is None
    mat.run(x)                                          # third run: captured and replayed
    assert mat._graph is not None
    assert _valid_equal(eager, _outputs(mat))
    mat.run(x)
    assert _valid_equal(eager, _outputs(mat))
    pp = ops.PostProcessor(2, mat.P, 20, DEV, mat.post.cap)
    pp.run(mat.boxes, mat.scores, mat.conf_thresh, mat.nms_thresh, False, mat.max_per_image, nms_method='matrix_linear')
    torch.cuda.synchronize()
    assert _valid_equal(eager, (pp.out_dets.cpu().numpy(), pp.out_count.cpu().numpy(), pp.out_index.cpu().numpy()))
    assert int(mat.post.overflow.item()) == 0 and eager[1].sum() > 0
    pp.run(mat.boxes, mat.scores, mat.conf_thresh, mat.nms_thresh, False, mat.max_per_image)
    torch.cuda.synchronize()
    hard = (pp.out_dets.cpu().numpy(), pp.out_count.cpu().numpy(), pp.out_index.cpu().numpy())
    assert not _valid_equal(eager, hard)                # score decay changes the result

    plain = DetectionPipeline(net, priors, 2, 20, image_wh=(500, 375), graph=False)
    plain.run(x)
    base = _outputs(plain)
    named = DetectionPipeline(net, priors, 2, 20, image_wh=(500, 375), graph=False, nms_method='hard', soft_sigma=0.9,
                              soft_score_threshold=0.2, matrix_pre_top=512)
    named.run(x)
    assert _valid_equal(base, _outputs(named))          # the default pipeline next to it: the matrix arguments do not reach it
    assert plain.post.matrix_ws is None and named.post.matrix_ws is None and named.post.soft_ws is None
