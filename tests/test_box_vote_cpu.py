"""Box voting and flip test-time augmentation without a device: the host twin ct_cpu_box_vote against a float64 numpy
restatement of the contract (include/ctdet.h), the exports, the argument checks that return before any device work and the
validation of the new keywords.

The contract: output row t of a segment gets, per coordinate, sum(w_q x_q) / sum(w_q) over the candidates q with
IoU(t, box_q) >= vote_thresh, the IoU being the fp32 +1 pixel expression of the NMS, products and sums in float64 taken in
candidate order, one float64 division, one rounding to fp32.  Twin and restatement sum in the same order (np.cumsum is
sequential), so their coordinates are equal bit for bit, and with them the membership sets."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from ctdet import _lib, ops, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ct_hflip_f32', 'ct_tta_merge', 'ct_box_vote_lds_rows', 'ct_box_vote_workspace_bytes', 'ct_box_vote_batched',
         'ct_cpu_box_vote')
F = np.float32
SIZES = (1, 2, 37, 64, 257, 1100)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ------------------------------------------------------------------ the contract, restated
def iou_plus_one(t, cb):
    """fp32 IoU of box t [4] with every box of cb [n,4]: w = max(min(x2) - max(x1) + 1, 0), ovr = inter / (Sa + Sb - inter)."""
    t = np.asarray(t, dtype=F)
    cb = np.asarray(cb, dtype=F).reshape(-1, 4)
    one, zero = F(1), F(0)
    tarea = (t[2] - t[0] + one) * (t[3] - t[1] + one)
    area = (cb[:, 2] - cb[:, 0] + one) * (cb[:, 3] - cb[:, 1] + one)
    w = np.maximum(np.minimum(t[2], cb[:, 2]) - np.maximum(t[0], cb[:, 0]) + one, zero)
    h = np.maximum(np.minimum(t[3], cb[:, 3]) - np.maximum(t[1], cb[:, 1]) + one, zero)
    inter = w * h
    with np.errstate(invalid='ignore', divide='ignore'):
        ovr = inter / (tarea + area - inter)
    assert ovr.dtype == F
    return ovr


def vote_restated(cand_boxes, weights, rows, vote_thresh):
    """-> (voted rows [m,5], the member indices of every row)."""
    cb = np.asarray(cand_boxes, dtype=F).reshape(-1, 4)
    w = np.asarray(weights, dtype=F).reshape(-1)
    out = np.array(rows, dtype=F, copy=True).reshape(-1, 5)
    members = []
    for r in range(len(out)):
        mem = np.flatnonzero(iou_plus_one(out[r, :4], cb) >= F(vote_thresh))
        members.append(mem)
        if not len(mem):
            continue
        wd = w[mem].astype(np.float64)
        sw = np.cumsum(wd)[-1]
        if sw > 0:
            out[r, :4] = [F(np.cumsum(wd * cb[mem, c].astype(np.float64))[-1] / sw) for c in range(4)]
    return out, members


@functools.lru_cache(maxsize=None)
def clustered_segment(n, seed=4321, shift=0.0):
    """One (image, class) segment: n clustered candidates in merged-index (= unsorted) order and the rows hard NMS keeps of
    them, in descending score order -> (cand_boxes [n,4], weights [n], rows [m,5])."""
    d = synth.clustered_dets(n, seed=seed)
    d[:, :4] -= F(shift)
    keep = ops.cpu_nms(d, 0.45, ge=False)
    out = (np.ascontiguousarray(d[:, :4]), np.ascontiguousarray(d[:, 4]), np.ascontiguousarray(d[keep]))
    for a in out:
        a.setflags(write=False)
    return out


def _twin(cb, w, rows, thr):
    return ops.cpu_box_vote(cb, w, np.array(rows, dtype=F, copy=True).reshape(-1, 5), thr)


# ------------------------------------------------------------------ twin against restatement
@pytest.mark.parametrize('thr', [0.5, 0.9])
@pytest.mark.parametrize('n', SIZES)
def test_twin_equals_the_restatement_bit_for_bit(n, thr):
    cb, w, rows = clustered_segment(n)
    want, members = vote_restated(cb, w, rows, thr)
    got = _twin(cb, w, rows, thr)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got[:, 4]), _bits(rows[:, 4]))              # scores untouched
    assert all(len(m) >= 1 for m in members)                                # a row's own source is always a member
    # equal bits mean equal membership: dropping any one member of a row with several moves that row
    r = int(np.argmax([len(m) for m in members]))
    if len(members[r]) > 1:
        less = np.delete(np.arange(len(w)), members[r][-1])
        moved = _twin(cb[less], w[less], rows[r:r + 1], thr)
        assert not np.array_equal(_bits(moved[0, :4]), _bits(got[r, :4]))
    if n >= 257 and thr == 0.5:
        assert max(len(m) for m in members) > 8 and any(not np.array_equal(_bits(a[:4]), _bits(b[:4]))
                                                         for a, b in zip(got, rows))


@pytest.mark.parametrize('n', [37, 257])
def test_negative_and_mixed_sign_coordinates(n):
    """Boxes that reach outside the image: the segment shifted so that coordinates are negative or straddle zero."""
    for shift in (250.0, 1000.0):
        cb, w, rows = clustered_segment(n, 7, shift)
        assert (cb < 0).any() and ((cb[:, 0] < 0) & (cb[:, 2] > 0)).any() == (shift == 250.0)
        want, members = vote_restated(cb, w, rows, 0.5)
        got = _twin(cb, w, rows, 0.5)
        assert np.array_equal(_bits(got), _bits(want))
        assert max(len(m) for m in members) > 1


def test_an_overlap_equal_to_the_threshold_is_a_member():
    """[0,0,9,9] and [0,0,9,4] with the +1 rule: inter 50, union 100, IoU exactly 0.5."""
    rows = np.array([[0, 0, 9, 9, 0.8]], dtype=F)
    cb = np.array([[0, 0, 9, 9], [0, 0, 9, 4]], dtype=F)
    w = np.array([0.8, 0.4], dtype=F)
    assert iou_plus_one(rows[0, :4], cb)[1] == F(0.5)
    got = _twin(cb, w, rows, 0.5)
    want = (0.8 * 9 + 0.4 * 4) / 1.2
    assert got[0, 3] == F((np.float64(F(0.8)) * 9 + np.float64(F(0.4)) * 4) / (np.float64(F(0.8)) + np.float64(F(0.4))))
    assert abs(got[0, 3] - want) < 1e-5 and got[0, 0] == 0 and got[0, 1] == 0 and got[0, 2] == 9 and got[0, 4] == F(0.8)
    assert np.array_equal(_bits(got), _bits(vote_restated(cb, w, rows, 0.5)[0]))
    for other in ([0, 0, 9, 3], [0, 0, 10, 4], [1, 0, 9, 4]):              # one pixel off: below the threshold
        cb2 = np.array([[0, 0, 9, 9], other], dtype=F)
        assert iou_plus_one(rows[0, :4], cb2)[1] < F(0.5)
        assert np.array_equal(_bits(_twin(cb2, w, rows, 0.5)), _bits(rows))
    # just above the threshold value itself: the same pair is no member at the next float above 0.5
    assert np.array_equal(_bits(_twin(cb, w, rows, float(np.nextafter(F(0.5), F(1))))), _bits(rows))


def test_rows_without_company_and_empty_inputs_keep_their_bits():
    cb, w, rows = clustered_segment(257)
    got = _twin(cb, w, rows, 1.0)                                           # IoU 1 only with itself: w x / w = x exactly
    assert np.array_equal(_bits(got), _bits(rows))
    lone = np.array([[-3.25, 7.1, 40.7, 99.9, 0.3], [300.5, 200.25, 310.125, 260.0, 0.2]], dtype=F)
    assert np.array_equal(_bits(_twin(lone[:, :4], lone[:, 4], lone, 0.5)), _bits(lone))
    assert np.array_equal(_bits(_twin(np.zeros((0, 4), F), np.zeros(0, F), lone, 0.5)), _bits(lone))   # empty segment
    none = np.zeros((0, 5), dtype=F)
    assert _twin(cb, w, none, 0.5).shape == (0, 5)                          # m = 0
    far = np.array([[1000, 1000, 1010, 1010]], dtype=F)                     # candidates, but no member
    assert np.array_equal(_bits(_twin(far, np.array([0.9], F), lone, 0.5)), _bits(lone))


def test_the_weight_is_the_raw_score_not_the_row_score():
    """Soft-NMS decays a kept row's score; voting still weighs its source candidate by the raw score."""
    cb, w, rows = clustered_segment(64)
    decayed = np.array(rows, copy=True)
    decayed[:, 4] *= F(0.25)
    got = _twin(cb, w, decayed, 0.5)
    assert np.array_equal(_bits(got[:, :4]), _bits(_twin(cb, w, rows, 0.5)[:, :4]))
    assert np.array_equal(_bits(got[:, 4]), _bits(decayed[:, 4]))


# ------------------------------------------------------------------ validation
def test_keyword_validation():
    assert ops.tta_mode(None) == 1 and ops.tta_mode('hflip') == 2
    for bad in ('vflip', 'HFLIP', '', 2, ['hflip']):
        with pytest.raises(ValueError):
            ops.tta_mode(bad)
    assert ops.vote_threshold(None) is None and ops.vote_threshold(0.5) == 0.5 and ops.vote_threshold(1) == 1.0
    for bad in (0, 0.0, -0.5, 1.0001, 2, float('nan'), True, '0.5'):
        with pytest.raises(ValueError):
            ops.vote_threshold(bad)
    rows = np.zeros((1, 5), dtype=F)
    for bad in (0.0, 1.5, None):
        with pytest.raises(ValueError):
            ops.cpu_box_vote(rows[:, :4], rows[:, 4], rows, bad)
    with pytest.raises(ValueError):
        ops.cpu_box_vote(rows[:, :4], rows[:, 4], rows.astype(np.float64), 0.5)
    b, s = torch.zeros(1, 8, 4), torch.zeros(1, 8, 3)
    od, oc = torch.zeros(1, 2, 4, 5), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.box_vote(b, s, od, oc, 0.01, 1.5)                               # before any device work
    with pytest.raises(_lib.CtdetError):
        ops.box_vote(b, s, od, oc, 0.01, 0.5)                               # host tensors: no CPU fallback
    with pytest.raises(_lib.CtdetError):
        ops.hflip(torch.zeros(1, 3, 4, 4))
    import inspect
    from ctdet import harness, pipeline
    for fn in (pipeline.DetectionPipeline.__init__, harness.detect_dataset, harness.do_test):
        prm = inspect.signature(fn).parameters
        assert prm['tta'].default is None and prm['box_vote'].default is None
    assert inspect.signature(ops.PostProcessor.run).parameters['box_vote'].default is None


# ------------------------------------------------------------------ the library without a device
def test_exports_header_and_argument_checks():
    lib = _lib.lib()
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + '(' in header, name
    assert lib.ct_abi_version() == 1
    rows = lib.ct_box_vote_lds_rows()
    assert rows >= 1024 and rows % 64 == 0
    assert lib.ct_box_vote_workspace_bytes(2, rows, 3, 100) == 256         # one chunk holds every segment: no sums to keep
    assert lib.ct_box_vote_workspace_bytes(2, rows + 1, 3, 100) >= 2 * 3 * 100 * 5 * 8
    one = C.c_void_p(256)                                                   # never dereferenced: the checks return first
    st = C.c_void_p(0)
    assert lib.ct_box_vote_batched(one, one, 1, 8, 2, 0.01, 0.0, 4, one, one, one, 256, st) != 0
    assert b'vote_thresh' in lib.ct_last_error_string()
    assert lib.ct_box_vote_batched(one, one, 1, 8, 2, 0.01, 1.5, 4, one, one, one, 256, st) != 0
    assert lib.ct_box_vote_batched(one, one, 1, 8, 2, -1.0, 0.5, 4, one, one, one, 256, st) != 0
    assert lib.ct_box_vote_batched(None, one, 1, 8, 2, 0.01, 0.5, 4, one, one, one, 256, st) != 0
    assert lib.ct_box_vote_batched(one, one, 1, rows + 1, 2, 0.01, 0.5, 4, one, one, one, 256, st) != 0
    assert b'workspace' in lib.ct_last_error_string()
    assert lib.ct_hflip_f32(one, one, 3, 4, 4, st) != 0                     # in == out
    assert lib.ct_hflip_f32(one, C.c_void_p(512), 3, 4, 0, st) != 0
    assert lib.ct_tta_merge(one, one, 1, 8, 3, 2, 2, 0, None, 0, one, one, st) != 0      # pass 2 of 2
    assert lib.ct_tta_merge(one, one, 1, 8, 3, 2, 1, 1, None, 0, one, one, st) != 0      # mirrored without widths
    assert lib.ct_cpu_box_vote(None, None, 0, 0.5, None, 0) == 0
    assert lib.ct_cpu_box_vote(None, None, 1, 0.5, None, 0) != 0
