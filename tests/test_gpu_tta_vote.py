"""Flip test-time augmentation and box voting on the MI355X (csrc/ct_tta.hip and what is built on it).

ops.box_vote against the host twin ct_cpu_box_vote, per segment: the same members (seen through the result) and
    |dev - twin| <= 2^-23 |twin| + 2^-30 max|coordinate of the segment|
-- the first term is two fp32 roundings (both sides round one float64 quotient), the second bounds two float64 summations of
up to 2^20 exact products taken in different orders.  ops.hflip and ops.tta_merge are pure data movement plus one fp32
subtraction and are held to numpy bit for bit."""
import functools

import numpy as np
import pytest
import torch

from ctdet import _lib, evaluate, ops, synth
from test_box_vote_cpu import iou_plus_one
from test_gpu_soft_nms import B, CONF, NMS_T, P, T, _net300, _outputs, _pipeline_case, _valid_equal

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
SENT = -7.0


def _cuda(a, dtype=None):
    return torch.as_tensor(np.array(a, order='C', copy=True), dtype=dtype).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _lds_rows():
    return int(_lib.lib().ct_box_vote_lds_rows())


def _twin_segment(boxes, scores, b, c, rows, thr, conf=CONF):
    """The host twin on segment (b, c): its candidates in merged-index order -> (voted rows, max|coordinate|)."""
    q = np.flatnonzero(scores[b, :, 1 + c] > F(conf))
    out = np.array(rows, dtype=F, copy=True).reshape(-1, 5)
    ops.cpu_box_vote(boxes[b, q], scores[b, q, 1 + c], out, thr)
    return out, (float(np.abs(boxes[b, q]).max()) if len(q) else 0.0)


def _inside_bound(got, want, cmax):
    g, w = got[:, :4].astype(np.float64), want[:, :4].astype(np.float64)
    err, bound = np.abs(g - w), 2.0 ** -23 * np.abs(w) + 2.0 ** -30 * cmax
    if len(g):
        print('voting: largest |dev - twin| %.3g, its bound %.3g' % (err.max(), bound.flat[err.argmax()]))
    return bool(np.all(err <= bound))


@functools.lru_cache(maxsize=None)
def _vote_case(counts, N, cap, rows_per_seg=None):
    """B x T segments with counts[b*T+c] candidates among N rows: clustered boxes per image, tie-free scores, and as output
    rows what hard NMS keeps of every segment's candidates (the first rows_per_seg[s] of them where given, at most cap) ->
    (boxes [B,N,4], scores [B,N,T+1], out_dets [B,T,cap,5] sentinel-filled, out_count [B,T])."""
    rng = np.random.RandomState(17 + N)
    boxes = np.stack([synth.clustered_dets(N, seed=60 + b)[:, :4] for b in range(B)]).astype(F)
    scores = np.zeros((B, N, T + 1), dtype=F)
    dets = np.full((B, T, cap, 5), SENT, dtype=F)
    cnt = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        for c in range(T):
            s = b * T + c
            n = counts[s]
            col = np.concatenate([np.linspace(0.011, 0.99, n) + 1e-4 * c, np.linspace(0.001, 0.0099, N - n)])
            scores[b, :, 1 + c] = rng.permutation(col)
            q = np.flatnonzero(scores[b, :, 1 + c] > F(CONF))
            assert len(q) == n
            cand = np.hstack([boxes[b, q], scores[b, q, 1 + c][:, None]]).astype(F)
            keep = ops.cpu_nms(cand, NMS_T, ge=False) if n else np.zeros(0, np.int32)
            m = min(len(keep), cap if rows_per_seg is None else rows_per_seg[s])
            dets[b, c, :m] = cand[keep[:m]]
            cnt[b, c] = m
    for a in (boxes, scores, dets, cnt):
        a.setflags(write=False)
    return boxes, scores, dets, cnt


def _run_vote(case, thr, stream=None, conf=CONF):
    """ops.box_vote on a case with guard bands around out_dets and the workspace -> voted out_dets (host)."""
    boxes, scores, dets, cnt = case
    cap, N, pad = dets.shape[2], boxes.shape[1], 256
    big = torch.full((dets.size + 2 * pad,), SENT, device=DEV)
    od = big[pad:-pad].view(B, T, cap, 5)
    od.copy_(_cuda(dets))
    oc = _cuda(cnt)
    need = ops.box_vote_workspace_bytes(B, N, T, cap)
    ws = torch.full((need + 2 * pad,), 0xA5, device=DEV, dtype=torch.uint8)
    db, ds = _cuda(boxes), _cuda(scores)
    torch.cuda.synchronize()
    if stream is None:
        ops.box_vote(db, ds, od, oc, conf, thr, workspace=ws[pad:pad + need])
    else:
        with torch.cuda.stream(stream):
            ops.box_vote(db, ds, od, oc, conf, thr, workspace=ws[pad:pad + need])
    torch.cuda.synchronize()
    h = big.cpu().numpy()
    assert (h[:pad] == SENT).all() and (h[-pad:] == SENT).all()                 # nothing around out_dets
    wsh = ws.cpu().numpy()
    assert (wsh[:pad] == 0xA5).all() and (wsh[pad + need:] == 0xA5).all()       # nothing around the workspace
    assert np.array_equal(oc.cpu().numpy(), cnt)
    assert np.array_equal(_bits(db.cpu().numpy()), _bits(boxes)) and np.array_equal(_bits(ds.cpu().numpy()), _bits(scores))
    return od.cpu().numpy().copy()


def _check_case(case, thr, got):
    boxes, scores, dets, cnt = case
    moved = 0
    for b in range(B):
        for c in range(T):
            m = int(cnt[b, c])
            assert np.array_equal(_bits(got[b, c, m:]), _bits(dets[b, c, m:])), (b, c)      # rows behind out_count: sentinel
            assert np.array_equal(_bits(got[b, c, :m, 4]), _bits(dets[b, c, :m, 4])), (b, c)   # scores untouched
            want, cmax = _twin_segment(boxes, scores, b, c, dets[b, c, :m], thr)
            assert _inside_bound(got[b, c, :m], want, cmax), (b, c)
            moved += int((_bits(want[:, :4]) != _bits(dets[b, c, :m, :4])).any())
    return moved


# ------------------------------------------------------------------ ops.box_vote against the host twin
COUNT_GROUPS = ((0, 1, 2, 63, 64, 65), (255, 256, 257, 2, 0, 65))


@pytest.mark.parametrize('thr', [0.5, 0.9])
@pytest.mark.parametrize('counts', COUNT_GROUPS)
def test_vote_equals_the_twin_inside_the_bound(counts, thr):
    case = _vote_case(counts, 600, 600)
    assert (case[3].reshape(-1) > 0).tolist() == [n > 0 for n in counts]
    got = _run_vote(case, thr)
    moved = _check_case(case, thr, got)
    if thr == 0.5:
        assert moved >= 3                                                   # voting moved boxes: the test sees members


@pytest.mark.parametrize('thr', [0.5])
def test_vote_around_the_lds_chunk_capacity(thr):
    """One candidate fewer than a chunk, a full chunk, one more (a second chunk of one row), two and three chunks: the running
    sums then go through the workspace."""
    L = _lds_rows()
    assert L >= 1024
    N = 2 * L + 200
    case = _vote_case((L - 1, L, L + 1, 2 * L + 1, 2 * L, 1100), N, 256)
    assert ops.box_vote_workspace_bytes(B, N, T, 256) >= B * T * 256 * 40
    assert _check_case(case, thr, _run_vote(case, thr)) == B * T


def test_vote_with_no_one_and_out_cap_output_rows():
    cap = 8
    case = _vote_case((300, 300, 300, 300, 0, 300), 600, cap, rows_per_seg=(0, 1, cap, cap, cap, 1))
    assert case[3].reshape(-1).tolist() == [0, 1, cap, cap, 0, 1]
    got = _run_vote(case, 0.5)
    assert _check_case(case, 0.5, got) >= 3
    assert (got[0, 0] == SENT).all() and (got[1, 1] == SENT).all()


def test_vote_exact_tie_on_the_device():
    """[0,0,9,9] / [0,0,9,4]: IoU exactly 0.5 is a member at vote_thresh 0.5; one pixel off it is not."""
    for other, member in (([0, 0, 9, 4], True), ([0, 0, 9, 3], False), ([0, 0, 10, 4], False)):
        boxes = np.zeros((B, 64, 4), dtype=F)
        boxes[:, :, :] = [500, 300, 520, 330]
        boxes[:, 5] = [0, 0, 9, 9]
        boxes[:, 40] = other
        assert (iou_plus_one(boxes[0, 5], boxes[0, 40:41])[0] == F(0.5)) == member
        scores = np.zeros((B, 64, T + 1), dtype=F)
        scores[:, 5, 1:] = 0.8
        scores[:, 40, 1:] = 0.4
        dets = np.full((B, T, 4, 5), SENT, dtype=F)
        dets[:, :, 0] = [0, 0, 9, 9, 0.8]
        cnt = np.ones((B, T), dtype=np.int32)
        case = (boxes, scores, dets, cnt)
        got = _run_vote(case, 0.5)
        _check_case(case, 0.5, got)
        w8, w4 = np.float64(F(0.8)), np.float64(F(0.4))
        want = F((w8 * 9 + w4 * other[3]) / (w8 + w4)) if member else F(9)
        assert (got[:, :, 0, 3] == want).all() and (got[:, :, 0, 1] == 0).all(), (other, got[0, 0, 0])


def test_vote_two_runs_and_a_side_stream_give_the_same_bits():
    L = _lds_rows()
    case = _vote_case((L + 1, 257, 2 * L + 1, 64, 1100, L), 2 * L + 200, 256)
    first = _run_vote(case, 0.5)
    second = _run_vote(case, 0.5)
    busy = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    for _ in range(8):
        busy = busy @ busy * 1e-3                                           # the main stream is busy meanwhile
    third = _run_vote(case, 0.5, stream=torch.cuda.Stream(device=DEV))
    assert np.array_equal(_bits(first), _bits(second)) and np.array_equal(_bits(first), _bits(third))


# ------------------------------------------------------------------ the post-processor
def _post(method_name, mpi, box_vote='absent'):
    boxes, scores = _pipeline_case()
    pp = ops.PostProcessor(B, P, T, DEV, out_cap=P)
    pp.out_dets.fill_(SENT)
    pp.out_index.fill_(-7)
    kw = {} if box_vote == 'absent' else {'box_vote': box_vote}
    pp.run(_cuda(boxes), _cuda(scores), CONF, NMS_T, False, mpi, nms_method=method_name, **kw)
    torch.cuda.synchronize()
    return pp


def _host(pp):
    return pp.out_dets.cpu().numpy().copy(), pp.out_count.cpu().numpy().copy(), pp.out_index.cpu().numpy().copy()


def _check_voted(plain, voted, boxes, scores, thr, conf=CONF):
    """`voted` = `plain` with every counted row voted by the host twin, inside the bound; everything else bit-equal."""
    assert np.array_equal(plain[1], voted[1]) and np.array_equal(plain[2], voted[2])
    assert np.array_equal(_bits(plain[0][..., 4]), _bits(voted[0][..., 4]))
    moved = 0
    for b in range(plain[1].shape[0]):
        for c in range(plain[1].shape[1]):
            m = int(plain[1][b, c])
            want, cmax = _twin_segment(boxes, scores, b, c, plain[0][b, c, :m], thr, conf)
            assert _inside_bound(voted[0][b, c, :m], want, cmax), (b, c)
            assert np.array_equal(_bits(voted[0][b, c, m:]), _bits(plain[0][b, c, m:])), (b, c)
            moved += int((_bits(want[:, :4]) != _bits(plain[0][b, c, :m, :4])).sum())
    return moved


@pytest.mark.parametrize('mpi', [0, 20])
@pytest.mark.parametrize('name', ['hard', 'linear'])
def test_postprocessor_vote_equals_postprocessing_then_the_twin(name, mpi):
    boxes, scores = _pipeline_case()
    today = _post(name, mpi)
    off = _post(name, mpi, box_vote=None)
    assert off.vote_ws is None
    for a, b in zip(_host(today), _host(off)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))         # box_vote=None: today's bits
    voted = _post(name, mpi, box_vote=0.5)
    assert voted.vote_ws is not None and int(voted.overflow.item()) == 0
    assert _check_voted(_host(today), _host(voted), boxes, scores, 0.5) > 0
    d, cnt = voted.out_dets.cpu().numpy(), voted.out_count.cpu().numpy()
    for b in range(B):
        for c in range(T):
            assert np.all(np.diff(d[b, c, :cnt[b, c], 4]) <= 0)


def test_voc_evaluator_takes_a_voted_result():
    pp = _post('hard', 20, box_vote=0.5)
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


# ------------------------------------------------------------------ mirror and merge
@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (2, 3, 6, 8), (1, 1, 1, 1), (3, 2, 4, 301), (1, 3, 9, 300)])
def test_hflip_equals_numpy(shape):
    x = np.random.RandomState(3).standard_normal(shape).astype(F)
    want = x[..., ::-1]
    dx = _cuda(x)
    assert np.array_equal(_bits(ops.hflip(dx).cpu().numpy()), _bits(want))
    big = torch.full((x.size + 512,), SENT, device=DEV)
    for shift in (256, 257):                                                # 257: not 16-byte aligned
        big.fill_(SENT)
        out = big[shift:shift + x.size].view(shape)
        ops.hflip(dx, out=out)
        h = big.cpu().numpy()
        assert np.array_equal(_bits(h[shift:shift + x.size].reshape(shape)), _bits(want))
        assert (h[:shift] == SENT).all() and (h[shift + x.size:] == SENT).all()
    with pytest.raises(ValueError):
        ops.hflip(dx, out=dx)


@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('p,cols', [(601, 3), (600, 4), (37, 21)])
def test_tta_merge_equals_numpy(p, cols, per_image):
    rng = np.random.RandomState(p)
    bk = [(rng.uniform(-20, 520, (B, p, 4))).astype(F) for _ in range(2)]
    sk = [rng.uniform(0, 1, (B, p, cols)).astype(F) for _ in range(2)]
    wh = np.array([[501.0, 375.0], [333.0, 499.0]], dtype=F)               # odd widths
    scale = np.stack([wh[:, 0], wh[:, 1], wh[:, 0], wh[:, 1]], 1) if per_image else np.array([501, 375, 501, 375], dtype=F)
    pad = 64
    bigb = torch.full((B * 2 * p * 4 + 2 * pad,), SENT, device=DEV)
    bigs = torch.full((B * 2 * p * cols + 2 * pad,), SENT, device=DEV)
    mb, ms = bigb[pad:-pad].view(B, 2 * p, 4), bigs[pad:-pad].view(B, 2 * p, cols)
    ds = _cuda(scale)
    ops.tta_merge(_cuda(bk[1]), _cuda(sk[1]), 1, 2, True, ds, (mb, ms))
    torch.cuda.synchronize()
    assert (mb[:, :p].cpu().numpy() == SENT).all() and (ms[:, :p].cpu().numpy() == SENT).all()     # slot 0 untouched
    ops.tta_merge(_cuda(bk[0]), _cuda(sk[0]), 0, 2, False, ds, (mb, ms))
    torch.cuda.synchronize()
    W = (scale[:, 0] if per_image else np.full(B, scale[0], dtype=F)).astype(F)[:, None]
    mirrored = np.stack([W - bk[1][..., 2], bk[1][..., 1], W - bk[1][..., 0], bk[1][..., 3]], -1)
    assert mirrored.dtype == F
    assert np.array_equal(_bits(mb.cpu().numpy()), _bits(np.concatenate([bk[0], mirrored], 1)))
    assert np.array_equal(_bits(ms.cpu().numpy()), _bits(np.concatenate([sk[0], sk[1]], 1)))
    for big in (bigb, bigs):
        h = big.cpu().numpy()
        assert (h[:pad] == SENT).all() and (h[-pad:] == SENT).all()
    with pytest.raises(ValueError):
        ops.tta_merge(_cuda(bk[0]), _cuda(sk[0]), 0, 3, False, ds, (mb, ms))
    with pytest.raises(_lib.CtdetError):
        ops.tta_merge(_cuda(bk[0]), _cuda(sk[0]), 1, 2, True, None, (mb, ms))


# ------------------------------------------------------------------ the pipeline
def _buffers(pipe):
    torch.cuda.synchronize()
    return pipe.boxes.cpu().numpy().copy(), pipe.scores.cpu().numpy().copy()


def test_pipeline_hflip_and_vote_eager_graph_and_default_unchanged():
    from ctdet.pipeline import DetectionPipeline
    from data import VOC_300
    from layers.functions import PriorBox
    net = _net300()
    priors = PriorBox(VOC_300).forward()
    x = synth.images(2, 300, 'randn', 1234).cuda()
    Wimg = 501.0                                                            # odd width
    plain = DetectionPipeline(net, priors, 2, 20, image_wh=(Wimg, 375), graph=False)
    plain.run(x)
    base, base_buf = _outputs(plain), _buffers(plain)
    plain.run(x)
    again, again_buf = _outputs(plain), _buffers(plain)
    # two eager runs of the plain pipeline give equal bits: everything below depends on that
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(base_buf, again_buf))
    assert _valid_equal(base, again)
    plain.run(x.flip(-1).contiguous())
    flip_buf = _buffers(plain)
    named = DetectionPipeline(net, priors, 2, 20, image_wh=(Wimg, 375), graph=False, tta=None, box_vote=None)
    named.run(x)
    assert _valid_equal(base, _outputs(named)) and named.stage is None and named.x_flip is None
    assert named.post.vote_ws is None and tuple(named.boxes.shape) == (2, plain.P, 4)
    with pytest.raises(ValueError):
        DetectionPipeline(net, priors, 2, 20, tta='vflip')
    with pytest.raises(ValueError):
        DetectionPipeline(net, priors, 2, 20, box_vote=1.5)

    Pn = plain.P
    tta = DetectionPipeline(net, priors, 2, 20, image_wh=(Wimg, 375), graph=True, tta='hflip')
    assert tuple(tta.boxes.shape) == (2, 2 * Pn, 4) and tta.post.P == 2 * Pn
    tta.run(x)
    eager, (mb, ms) = _outputs(tta), _buffers(tta)
    assert np.array_equal(_bits(mb[:, :Pn]), _bits(base_buf[0])) and np.array_equal(_bits(ms[:, :Pn]), _bits(base_buf[1]))
    fb = flip_buf[0]
    mirrored = np.stack([F(Wimg) - fb[..., 2], fb[..., 1], F(Wimg) - fb[..., 0], fb[..., 3]], -1)
    assert np.array_equal(_bits(mb[:, Pn:]), _bits(mirrored)) and np.array_equal(_bits(ms[:, Pn:]), _bits(flip_buf[1]))
    pp = ops.PostProcessor(2, 2 * Pn, 20, DEV, tta.post.cap)
    pp.run(tta.boxes, tta.scores, tta.conf_thresh, tta.nms_thresh, False, tta.max_per_image)
    torch.cuda.synchronize()
    ref = _host(pp)
    assert _valid_equal(eager, ref) and int(tta.post.overflow.item()) == 0 and eager[1].sum() > 0
    valid = np.arange(eager[2].shape[2])[None, None, :] < eager[1][:, :, None]
    assert (eager[2][valid] >= Pn).any() and (eager[2][valid] < Pn).any()      # merged indices k*P + p of both passes
    assert not _valid_equal(eager, base)                                    # the second pass changes the result
    tta.run(x)
    assert tta._graph is None and _valid_equal(eager, _outputs(tta))
    tta.run(x)                                                              # third run: captured and replayed
    g1 = tta._graph
    assert g1 is not None and _valid_equal(eager, _outputs(tta))
    tta.run(x)
    assert tta._graph is g1 and _valid_equal(eager, _outputs(tta))

    tta.box_vote = 0.5                                                      # part of the graph key: captured again
    tta.run(x)
    assert tta._graph is not None and tta._graph is not g1
    voted = _outputs(tta)
    tta.run(x)
    assert _valid_equal(voted, _outputs(tta))
    mask = lambda o: (np.where(valid[..., None], o[0], 0), o[1], np.where(valid, o[2], 0))     # noqa: E731
    moved = _check_voted(mask(eager), mask(voted), mb, ms, 0.5, tta.conf_thresh)
    assert moved > 0 and not _valid_equal(voted, eager)
    with pytest.raises(ValueError):
        tta.box_vote = 0.0
        tta.run(x)

    vote_only = DetectionPipeline(net, priors, 2, 20, image_wh=(Wimg, 375), graph=False, box_vote=0.5)
    vote_only.run(x)
    vo = _outputs(vote_only)
    pvalid = np.arange(base[2].shape[2])[None, None, :] < base[1][:, :, None]
    pmask = lambda o: (np.where(pvalid[..., None], o[0], 0), o[1], np.where(pvalid, o[2], 0))   # noqa: E731
    assert _check_voted(pmask(base), pmask(vo), base_buf[0], base_buf[1], 0.5, plain.conf_thresh) > 0
