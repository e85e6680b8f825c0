"""Soft-NMS on the MI355X (csrc/ct_soft_nms.hip; ct_soft_nms_batched_dev, ct_postprocess_batched_soft and what is built on
them) against the host twin ct_cpu_soft_nms, the reference's recording and the oracle.

Hard and linear methods: bit for bit.  Gaussian method: the same decisions and, for output row i (decayed at most i times,
each decay one ulp of the weight plus one rounding), |dev - host| <= 2 (i + 1) 2^-23 host -- a derived bound that holds only
where no decision is closer than that, so every Gaussian case first checks its decision margins on the host (the smallest
(top - second) / top over all selections, the smallest |score - threshold| / threshold over all threshold comparisons)
against 4 x its largest bound."""
import functools
import types

import numpy as np
import pytest
import torch

from ctdet import _lib, evaluate, ops, synth
from oracle import nms_ref
from test_soft_nms_cpu import alive_set_soft_nms, sorted_rows

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
ULP = 2.0 ** -23
SIZES = (1, 2, 37, 63, 64, 65, 255, 256, 257, 600, 1100)
GAUSS_CASES = ((1, 4321), (2, 4321), (37, 7), (63, 4321), (64, 7), (65, 4321), (255, 7), (256, 4321), (257, 4321),
               (600, 4321), (1100, 7))


def _cuda(a, dtype=None):
    return torch.as_tensor(np.array(a, order='C', copy=True), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _rows(n, seed):
    r = sorted_rows(synth.clustered_dets(n, seed=seed))
    r.setflags(write=False)
    return r


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _segments(segs, method, sigma=0.5, Nt=0.3, thr=0.001, max_emit=0, tail=0, ws_fill=None, sentinel=-7.0):
    """One call over `segs` (host [n,5] arrays in pipeline order) followed by `tail` NaN rows -> per segment (rows, pos),
    after checking that nothing outside the emitted rows was written.  (seg_off is CSR: segments have no gaps between
    them, so rows no segment owns can only follow the last one; the outputs are sentinel-filled everywhere.)"""
    lens = [len(s) for s in segs]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    total = int(off[-1])
    host = np.full((total + tail, 5), np.nan, dtype=F)
    if total:
        host[:total] = np.concatenate([np.asarray(s, dtype=F).reshape(-1, 5) for s in segs])
    dets = _cuda(host)
    out = (torch.full((total + tail, 5), sentinel, device=DEV), torch.full((total + tail,), -7, device=DEV, dtype=torch.int32),
           torch.full((len(segs) + 3,), -7, device=DEV, dtype=torch.int32))
    need = _lib.lib().ct_soft_nms_batched_workspace_bytes(total, len(segs))
    guard = 1024
    ws = torch.empty(need + 2 * guard, device=DEV, dtype=torch.uint8)
    ws.fill_(0xA5)
    if ws_fill is not None:
        ws[guard:guard + need // 4 * 4].view(torch.float32).fill_(ws_fill)
    ops.soft_nms_batched(dets, _cuda(off), method, sigma, Nt, thr, max_emit, max_seg_len=max(lens + [0]),
                         out=(out[0], out[1], out[2][:len(segs)]), workspace=ws[guard:guard + need])
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


def _host(rows, method, sigma=0.5, Nt=0.3, thr=0.001):
    b = np.array(rows, dtype=F, copy=True)
    k = ops.cpu_soft_nms(b, sigma, Nt, thr, method)
    return b[:k]


def _check_exact(rows, method, got, pos):
    want = _host(rows, method)
    assert len(got) == len(want), (len(got), len(want))
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(rows[pos, :4]), _bits(got[:, :4])) and len(set(pos.tolist())) == len(pos)
    assert np.all(np.diff(got[:, 4]) <= 0)


def _gauss_bound(k):
    return 2.0 * (np.arange(k) + 1) * ULP


def _check_margins(rows, k, sigma=0.5, thr=0.001, max_emit=0):
    """The precondition of the Gaussian bound: no decision of the case is within 4 x its largest bound."""
    trace = {}
    alive_set_soft_nms(rows, sigma, 0.3, thr, 2, max_emit, trace)
    worst = float(_gauss_bound(max(k, 1))[-1])
    print('margins: select %.3g threshold %.3g, largest bound %.3g' % (trace['select'], trace['threshold'], worst))
    assert trace['select'] >= 4 * worst and trace['threshold'] >= 4 * worst, (trace, worst)


def _check_gauss(rows, got, pos, want):
    assert len(got) == len(want), (len(got), len(want))
    assert np.array_equal(_bits(got[:, :4]), _bits(want[:, :4]))
    assert np.array_equal(_bits(rows[pos, :4]), _bits(got[:, :4]))
    d = np.abs(got[:, 4].astype(np.float64) - want[:, 4])
    print('scores not bit-equal: %d of %d, worst |dev - host| / bound %.3f'
          % (int((_bits(got[:, 4]) != _bits(want[:, 4])).sum()), len(got),
             float((d / (_gauss_bound(len(got)) * want[:, 4])).max()) if len(got) else 0.0))
    assert np.all(d <= _gauss_bound(len(got)) * want[:, 4])
    assert np.all(np.diff(got[:, 4]) <= 0)


# ------------------------------------------------------------------ single segments
@pytest.mark.parametrize('method', [0, 1])
@pytest.mark.parametrize('seed', [4321, 7])
@pytest.mark.parametrize('n', SIZES)
def test_hard_and_linear_equal_the_host_twin_bit_for_bit(n, seed, method):
    rows = _rows(n, seed)
    ((got, pos),) = _segments([rows], method)
    _check_exact(rows, method, got, pos)


@pytest.mark.parametrize('method', [0, 1])
@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_lds_capacity_boundary(delta, method):
    n = _lib.lib().ct_soft_nms_lds_rows() + delta
    rows = _rows(n, 4321)
    ((got, pos),) = _segments([rows], method)
    _check_exact(rows, method, got, pos)


@pytest.mark.parametrize('method', [0, 1])
def test_overlap_equal_to_Nt_is_left_alone(method):
    """IoU exactly 0.5 (10 x 10 inside 10 x 20, +1 convention) at Nt = 0.5: the rule is `ov > Nt`, the row keeps its
    score; just below that Nt it is removed (hard) or halved (linear)."""
    rows = np.array([[0, 0, 9, 19, 0.9], [0, 0, 9, 9, 0.8], [50, 50, 59, 59, 0.7]], dtype=F)
    ((got, pos),) = _segments([rows], method, Nt=0.5)
    assert pos.tolist() == [0, 1, 2] and np.array_equal(_bits(got), _bits(rows))
    assert np.array_equal(_bits(got), _bits(_host(rows, method, Nt=0.5)))
    ((got, pos),) = _segments([rows], method, Nt=0.4999)
    assert np.array_equal(_bits(got), _bits(_host(rows, method, Nt=0.4999)))
    assert pos.tolist() == ([0, 2] if method == 0 else [0, 2, 1])
    if method == 1:
        assert got[2, 4] == F(0.5) * F(0.8)


@pytest.mark.parametrize('n,seed', GAUSS_CASES)
def test_gaussian_same_decisions_scores_inside_the_bound(n, seed):
    rows = _rows(n, seed)
    want = _host(rows, 2)
    _check_margins(rows, len(want))
    ((got, pos),) = _segments([rows], 2)
    _check_gauss(rows, got, pos, want)


def test_gaussian_above_the_lds_capacity():
    """Both sides of the LDS capacity with the Gaussian method (margins of these cases on the host: >= 1.1e-4 against bounds
    <= 2e-5)."""
    for delta in (0, 1):
        rows = _rows(_lib.lib().ct_soft_nms_lds_rows() + delta, 7)
        want = _host(rows, 2)
        _check_margins(rows, len(want))
        ((got, pos),) = _segments([rows], 2)
        _check_gauss(rows, got, pos, want)


@pytest.mark.parametrize('method', [0, 1, 2])
def test_reference_recording(golden, method):
    """Case c6 of the reference's own recording through the reference-compatible wrapper: count and boxes equal, scores
    rtol 2e-6 (the rule of tests/test_oracle_golden.py::test_soft_nms_oracle)."""
    from utils.nms.gpu_nms import gpu_soft_nms
    g = golden('nms.npz')
    b = np.array(g['c6_dets'], dtype=F, copy=True)
    keep = gpu_soft_nms(b, 0.5, 0.3, 0.001, method)
    n = int(g['soft_m%d_n' % method])
    ref = g['soft_m%d_boxes' % method]
    assert keep == list(range(n))
    assert np.array_equal(b[:n, :4], ref[:n, :4])
    np.testing.assert_allclose(b[:n, 4], ref[:n, 4], rtol=2e-6, atol=0)
    assert np.array_equal(_bits(b[n:]), _bits(np.asarray(g['c6_dets'], dtype=F)[n:]))    # rows behind N' stay


# ------------------------------------------------------------------ batching
@pytest.mark.parametrize('method', [1, 2])
def test_batched_segments_equal_single_segments(method):
    cap = _lib.lib().ct_soft_nms_lds_rows()
    lens = [0, 1, 37, 0, 63, 64, 65, 2, 255, 256, 257, 0, 0, 130, 300, 511, 512, 513, 1, 1, cap + 1, 0, 5, 600, 17, 64, 256,
            0, 3, 129, 191, 192, 193, 7, 41, 1, 2, 0, 320, 100]
    segs = [_rows(n, 100 + i) if n else np.zeros((0, 5), dtype=F) for i, n in enumerate(lens)]
    batched = _segments(segs, method, tail=50)
    poisoned = _segments(segs, method, tail=50, ws_fill=float('nan'), sentinel=-3.0)
    singles = {}
    for i, (s, (got, pos)) in enumerate(zip(segs, batched)):
        if len(s) not in singles or i < 25:
            ((one, one_pos),) = _segments([s], method) if len(s) else ((np.zeros((0, 5), dtype=F), np.zeros(0, np.int32)),)
            assert np.array_equal(_bits(got), _bits(one)) and np.array_equal(pos, one_pos), i
            singles[len(s)] = True
        assert np.array_equal(_bits(got), _bits(poisoned[i][0])) and np.array_equal(pos, poisoned[i][1]), i
        if method == 1:
            _check_exact(s, 1, got, pos) if len(s) else None
    assert sum(len(g) for g, _ in batched) > 200


def test_method_0_equals_hard_nms():
    for n in SIZES:
        for seed in (4321, 7):
            rows = _rows(n, seed)
            ((got, pos),) = _segments([rows], 0, Nt=0.45)
            keep, cnt = ops.nms_batched(_cuda(rows), _cuda(np.array([0, n], dtype=np.int32)), 0.45, ge=False)
            kept = keep.cpu().numpy()[:int(cnt.item())]
            assert np.array_equal(pos, kept), (n, seed)
            assert np.array_equal(_bits(got), _bits(rows[kept]))


# ------------------------------------------------------------------ the emission limit
@pytest.mark.parametrize('method', [0, 1, 2])
def test_emission_limit_gives_a_prefix(method):
    for n, seed in ((600, 4321), (1100, 7)):
        rows = _rows(n, seed)
        (full,) = _segments([rows], method)
        (cut5,) = _segments([rows], method, max_emit=5)
        (cut20,) = _segments([rows], method, max_emit=20)
        assert len(full[0]) > (20 if method else 5)     # (the hard method keeps about ten of these clustered rows)
        for k, (got, pos) in ((5, cut5), (20, cut20)):
            assert len(got) == min(k, len(full[0])), (n, k, len(got))
            assert np.array_equal(_bits(got), _bits(full[0][:k])) and np.array_equal(pos, full[1][:k]), (n, k)


def test_emission_limit_keeps_ties_lower_position_first():
    rows = np.array([[0, 0, 10, 10, 0.9], [100, 0, 110, 10, 0.5], [200, 0, 210, 10, 0.5], [300, 0, 310, 10, 0.5],
                     [400, 0, 410, 10, 0.4]], dtype=F)
    for method in (0, 1, 2):
        ((got, pos),) = _segments([rows], method, max_emit=2)
        assert pos.tolist() == [0, 1, 2, 3], (method, pos)
        assert np.array_equal(_bits(got), _bits(rows[:4]))
        ((got, pos),) = _segments([rows], method, max_emit=1)
        assert pos.tolist() == [0]


# ------------------------------------------------------------------ the post-processing entry
B, T, P = 2, 3, 600
CONF = 0.01
NMS_T = 0.45


@functools.lru_cache(maxsize=None)
def _pipeline_case():
    """Clustered boxes shared by the classes; per class about 170 priors pass conf_thresh with tie-free scores."""
    rng = np.random.RandomState(11)
    boxes = np.stack([synth.clustered_dets(P, seed=50 + b)[:, :4] for b in range(B)]).astype(F)
    scores = np.zeros((B, P, T + 1), dtype=F)
    for b in range(B):
        for c in range(T):
            n_pass = 150 + 20 * c + 10 * b
            col = np.concatenate([np.linspace(0.011, 0.99, n_pass) + 1e-4 * c, np.linspace(0.001, 0.0099, P - n_pass)])
            scores[b, :, 1 + c] = rng.permutation(col)
    scores[..., 0] = 1 - scores[..., 1:].max(-1)
    return boxes, scores


@functools.lru_cache(maxsize=None)
def _pipeline_reference(method):
    """Per (image, class): candidates in the pipeline's order and nms_ref.soft_nms on them -> (prior indices of the
    candidates, rows the reference keeps, the candidates themselves)."""
    boxes, scores = _pipeline_case()
    out = {}
    for b in range(B):
        for c in range(T):
            inds = np.where(scores[b, :, 1 + c] > F(CONF))[0]
            inds = inds[nms_ref.stable_desc_order(scores[b, inds, 1 + c])]
            cand = np.hstack([boxes[b, inds], scores[b, inds, 1 + c][:, None]]).astype(F)
            work = cand.copy()
            k = nms_ref.soft_nms(work, 0.5, NMS_T, 0.001, method)
            out[b, c] = (inds, work[:k].copy(), cand)
    return out


def _topk_rule(ref, mpi):
    """The `>= k-th largest` rule of oracle/nms_ref.postprocess_image on the per-class rows."""
    res = {}
    for b in range(B):
        allsc = np.concatenate([ref[b, c][1][:, 4] for c in range(T)])
        thr = np.sort(allsc)[-mpi] if mpi > 0 and len(allsc) > mpi else -np.inf
        for c in range(T):
            rows = ref[b, c][1]
            res[b, c] = rows[rows[:, 4] >= thr]
    return res


def _prior_index(ref_entry, rows):
    """Prior index of every kept row: boxes are unique per prior."""
    inds, _, cand = ref_entry
    lut = {cand[i, :4].tobytes(): int(inds[i]) for i in range(len(inds))}
    return np.array([lut[r[:4].tobytes()] for r in rows], dtype=np.int64)


def _run_post(method_name, mpi, cap=None):
    boxes, scores = _pipeline_case()
    pp = ops.PostProcessor(B, P, T, DEV, out_cap=cap or P)
    pp.out_dets.fill_(-7.0)
    pp.out_index.fill_(-7)
    pp.run(_cuda(boxes), _cuda(scores), CONF, NMS_T, False, mpi, nms_method=method_name)
    torch.cuda.synchronize()
    return pp


@pytest.mark.parametrize('mpi', [0, 20])
@pytest.mark.parametrize('name,method', [('hard', 0), ('linear', 1)])
def test_postprocess_equals_the_host_restatement(name, method, mpi):
    ref = _pipeline_reference(method)
    want = _topk_rule(ref, mpi)
    if method:
        assert max(len(ref[k][1]) for k in ref) > 20                    # a segment runs into the emission limit
    pp = _run_post(name, mpi)
    assert int(pp.overflow.item()) == 0
    dets, cnt, idx = pp.out_dets.cpu().numpy(), pp.out_count.cpu().numpy(), pp.out_index.cpu().numpy()
    for (b, c), rows in want.items():
        assert cnt[b, c] == len(rows), (b, c, cnt[b, c], len(rows))
        assert np.array_equal(_bits(dets[b, c, :len(rows)]), _bits(rows)), (b, c)
        assert np.array_equal(idx[b, c, :len(rows)], _prior_index(ref[b, c], rows)), (b, c)
        assert (dets[b, c, len(rows):] == -7.0).all() and (idx[b, c, len(rows):] == -7).all()
        assert np.all(np.diff(dets[b, c, :len(rows), 4]) <= 0)
    if mpi:
        assert any(len(want[k]) < len(ref[k][1]) for k in want)         # the rule cut something


@pytest.mark.parametrize('mpi', [0, 5])
def test_soft_entry_with_method_0_equals_the_hard_path(mpi):
    """ct_postprocess_batched_soft accepts method 0 (PostProcessor never sends it): full sort + the soft kernel with the
    emission limit give what the hard path's partial sort and prefix cut give."""
    import ctypes as C
    boxes, scores = _pipeline_case()
    hard = _run_post('hard', mpi)
    pp = ops.PostProcessor(B, P, T, DEV, out_cap=P)
    pp.out_dets.fill_(-7.0)
    pp.out_index.fill_(-7)
    db, ds = _cuda(boxes), _cuda(scores)
    need = _lib.lib().ct_postprocess_soft_workspace_bytes(B, P, T)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    _lib.check(_lib.lib().ct_postprocess_batched_soft(
        db.data_ptr(), ds.data_ptr(), B, P, T, CONF, 0, 0.5, NMS_T, 0.001, mpi, P, pp.out_dets.data_ptr(),
        pp.out_count.data_ptr(), pp.out_index.data_ptr(), pp.overflow.data_ptr(), ws.data_ptr(), need,
        C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'ct_postprocess_batched_soft')
    torch.cuda.synchronize()
    for name in ('out_dets', 'out_count', 'out_index', 'overflow'):
        assert np.array_equal(getattr(pp, name).cpu().numpy(), getattr(hard, name).cpu().numpy()), name


@pytest.mark.parametrize('mpi', [0, 20])
def test_postprocess_gaussian_inside_the_bound(mpi):
    ref = _pipeline_reference(2)
    want = _topk_rule(ref, mpi)
    worst = 0.0
    for key, (inds, kept, cand) in ref.items():
        trace = {}
        alive_set_soft_nms(cand, 0.5, NMS_T, 0.001, 2, 0, trace)
        bound = float(_gauss_bound(max(len(kept), 1))[-1])
        assert trace['select'] >= 4 * bound and trace['threshold'] >= 4 * bound, (key, trace, bound)
        worst = max(worst, bound)
    if mpi:                                                              # the image's cut is a decision too
        for b in range(B):
            allsc = np.sort(np.concatenate([ref[b, c][1][:, 4] for c in range(T)]).astype(np.float64))
            assert (allsc[-mpi] - allsc[-mpi - 1]) / allsc[-mpi] >= 4 * worst
    pp = _run_post('gaussian', mpi)
    assert int(pp.overflow.item()) == 0
    dets, cnt, idx = pp.out_dets.cpu().numpy(), pp.out_count.cpu().numpy(), pp.out_index.cpu().numpy()
    for (b, c), rows in want.items():
        assert cnt[b, c] == len(rows), (b, c, cnt[b, c], len(rows))
        got = dets[b, c, :len(rows)]
        assert np.array_equal(_bits(got[:, :4]), _bits(rows[:, :4])), (b, c)
        assert np.all(np.abs(got[:, 4].astype(np.float64) - rows[:, 4]) <= _gauss_bound(len(rows)) * rows[:, 4]), (b, c)
        assert np.array_equal(idx[b, c, :len(rows)], _prior_index(ref[b, c], rows)), (b, c)
        assert np.all(np.diff(got[:, 4]) <= 0)


@pytest.mark.parametrize('name', ['linear', 'gaussian'])
def test_postprocess_overflow_and_guards(name):
    boxes, scores = _pipeline_case()
    cap, pad = 4, 256
    pp = ops.PostProcessor(B, P, T, DEV, out_cap=cap)
    big_d = torch.full((B * T * cap * 5 + 2 * pad,), -7.0, device=DEV)
    big_i = torch.full((B * T * cap + 2 * pad,), -7, device=DEV, dtype=torch.int32)
    pp.out_dets = big_d[pad:-pad].view(B, T, cap, 5)
    pp.out_index = big_i[pad:-pad].view(B, T, cap)
    pp.run(_cuda(boxes), _cuda(scores), CONF, NMS_T, False, 20, nms_method=name)
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


def test_voc_evaluator_takes_the_soft_result():
    pp = _run_post('linear', 20)
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


# ------------------------------------------------------------------ repeatability
@pytest.mark.parametrize('name', ['linear', 'gaussian'])
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
        third.run(db, ds, CONF, NMS_T, False, 20, nms_method=name)
    torch.cuda.synchronize()
    for other in (second, third):
        b = (other.out_dets.cpu().numpy(), other.out_count.cpu().numpy(), other.out_index.cpu().numpy())
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _net300():
    from models.RFB_Net_vgg import build_net
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), 300, 20)
    net.load_state_dict(synth.fill_state_dict(net.state_dict()), strict=True)
    net = net.eval().cuda()
    net.device = 'cuda'
    return net


def _outputs(pipe):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in (pipe.post.out_dets, pipe.post.out_count, pipe.post.out_index))


def _valid_equal(a, b):
    """out_count equal and the rows / indices it counts bit-equal (rows behind the counts are stale by design)."""
    if not np.array_equal(a[1], b[1]):
        return False
    mask = np.arange(a[0].shape[2])[None, None, :] < a[1][:, :, None]
    return np.array_equal(_bits(a[0])[mask], _bits(b[0])[mask]) and np.array_equal(a[2][mask], b[2][mask])


def test_pipeline_linear_eager_graph_and_default_unchanged():
    from ctdet.pipeline import DetectionPipeline
    from data import VOC_300
    from layers.functions import PriorBox
    net = _net300()
    priors = PriorBox(VOC_300).forward()
    x = synth.images(2, 300, 'randn', 1234).cuda()
    # (1000 rows per image: with synthetic weights the 200 best rows of an image are all undecayed ones, the same rows hard
    # NMS keeps, and the last assertion below could not tell the two paths apart)
    soft = DetectionPipeline(net, priors, 2, 20, image_wh=(500, 375), max_per_image=1000, nms_method='linear', graph=True)
    soft.run(x)
    eager = _outputs(soft)
    soft.run(x)
    assert soft._graph is None
    soft.run(x)                                         # third run: captured and replayed
    assert soft._graph is not None
    assert _valid_equal(eager, _outputs(soft))
    soft.run(x)
    assert _valid_equal(eager, _outputs(soft))
    pp = ops.PostProcessor(2, soft.P, 20, DEV, soft.post.cap)
    pp.run(soft.boxes, soft.scores, soft.conf_thresh, soft.nms_thresh, False, soft.max_per_image, nms_method='linear')
    torch.cuda.synchronize()
    assert _valid_equal(eager, (pp.out_dets.cpu().numpy(), pp.out_count.cpu().numpy(), pp.out_index.cpu().numpy()))
    assert int(soft.post.overflow.item()) == 0 and eager[1].sum() > 0
    pp.run(soft.boxes, soft.scores, soft.conf_thresh, soft.nms_thresh, False, soft.max_per_image)
    torch.cuda.synchronize()
    hard = (pp.out_dets.cpu().numpy(), pp.out_count.cpu().numpy(), pp.out_index.cpu().numpy())
    assert not _valid_equal(eager, hard)                # score decay changes the result

    plain = DetectionPipeline(net, priors, 2, 20, image_wh=(500, 375), graph=False)
    plain.run(x)
    base = _outputs(plain)
    named = DetectionPipeline(net, priors, 2, 20, image_wh=(500, 375), graph=False, nms_method='hard', soft_sigma=0.9,
                              soft_score_threshold=0.2)
    named.run(x)
    assert _valid_equal(base, _outputs(named))
    assert plain.post.soft_ws is None and named.post.soft_ws is None
