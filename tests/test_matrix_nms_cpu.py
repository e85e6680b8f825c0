"""Matrix NMS (csrc/ct_matrix_nms.hip, ct_cpu_matrix_nms, ct_postprocess_batched_matrix) without a device: the rule of
include/ctdet.h restated densely in numpy fp32 (a full IoU matrix, triu, a column maximum, a term matrix, a column minimum)
against the host twin's loops, hand cases, pre_top and max_emit, exports, the argument checks that return before any device
work, the workspace queries, and what PostProcessor / DetectionPipeline hand to the library (recording proxy of
tests/test_soft_nms_cpu.py).

Linear method: twin == restatement bit for bit (minima and maxima do not depend on the order they are taken in).  Gaussian:
the two differ by numpy's and libm's double exp rounded to fp32, at most one fp32 ulp of decay, plus the product's rounding:
2^-22 relative."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from ctdet import _lib, ops, pipeline, synth
from test_soft_nms_cpu import _pipe, recorded, sorted_rows  # noqa: F401  (recorded: a fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ct_matrix_nms_max_rows', 'ct_matrix_nms_batched_workspace_bytes', 'ct_matrix_nms_batched_dev', 'ct_cpu_matrix_nms',
         'ct_postprocess_matrix_workspace_bytes', 'ct_postprocess_batched_matrix')
F = np.float32
SIZES = (1, 2, 37, 63, 64, 65, 255, 256, 257, 600, 1100)
SEEDS = (4321, 7)
REL = 2.0 ** -22


# ------------------------------------------------------------------ the contract, restated densely
def dense_iou(d):
    """The full fp32 +1-pixel IoU matrix of rows d [n,5] (0 where iw <= 0 or ih <= 0)."""
    one = F(1)
    x1, y1, x2, y2 = (d[:, k] for k in range(4))
    area = (x2 - x1 + one) * (y2 - y1 + one)
    iw = np.minimum(x2[:, None], x2[None, :]) - np.maximum(x1[:, None], x1[None, :]) + one
    ih = np.minimum(y2[:, None], y2[None, :]) - np.maximum(y1[:, None], y1[None, :]) + one
    hit = (iw > 0) & (ih > 0)
    inter = (iw * ih).astype(F)
    ua = ((area[:, None] + area[None, :]).astype(F) - inter).astype(F)
    with np.errstate(divide='ignore', invalid='ignore'):
        ov = (inter / ua).astype(F)
    return np.where(hit, ov, F(0)).astype(F)


def dense_matrix_nms(rows_sorted, method, sigma=0.5, thr=0.001, pre_top=1024, max_emit=0):
    """The rule on rows in the pipeline's order -> (rows [k,5] with decayed scores in emission order, positions [k])."""
    d = np.ascontiguousarray(rows_sorted, dtype=F).reshape(-1, 5)[:pre_top]
    n = len(d)
    if n == 0:
        return np.zeros((0, 5), F), np.zeros(0, np.int64)
    ov = np.triu(dense_iou(d), 1)                               # ov[i, j], i < j
    cmax = ov.max(axis=0)                                       # column maximum; column 0 holds only zeros
    upper = np.triu(np.ones((n, n), bool), 1)
    if method == 1:
        den = (F(1) - cmax).astype(F)
        with np.errstate(divide='ignore', invalid='ignore'):
            t = ((F(1) - ov) / den[:, None]).astype(F)
        valid = upper & (den != 0)[:, None]
    else:
        c64, o64 = cmax.astype(np.float64), ov.astype(np.float64)
        t = np.exp(((c64 * c64)[:, None] - o64 * o64) / np.float64(F(sigma))).astype(F)
        valid = upper
    decay = np.minimum(F(1), np.where(valid, t, F(np.inf)).min(axis=0)).astype(F)
    score = (d[:, 4] * decay).astype(F)
    alive = np.flatnonzero(~(score < F(thr)))
    order = alive[np.argsort(-score[alive].astype(np.float64), kind='stable')]
    if max_emit > 0 and len(order) > max_emit:
        k = max_emit
        while k < len(order) and score[order[k]] == score[order[max_emit - 1]]:
            k += 1
        order = order[:k]
    out = d[order].copy()
    out[:, 4] = score[order]
    return out, order


@functools.lru_cache(maxsize=None)
def seg_rows(n, seed):
    r = sorted_rows(synth.clustered_dets(n, seed=seed))
    r.setflags(write=False)
    return r


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ------------------------------------------------------------------ the twin against the restatement
@pytest.mark.parametrize('thr', [0.05, 0.001])
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n', SIZES)
def test_linear_twin_equals_the_dense_restatement_bit_for_bit(n, seed, thr):
    rows = seg_rows(n, seed)
    want, wpos = dense_matrix_nms(rows, 1, thr=thr, pre_top=2048)
    got, pos = ops.cpu_matrix_nms(rows, 1, 0.5, thr, pre_top=2048)
    assert np.array_equal(pos, wpos)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got[:, :4]), bits(rows[pos, :4])) and len(set(pos.tolist())) == len(pos)
    assert np.all(np.diff(got[:, 4]) <= 0)
    if n >= 37:
        dropped = 1 - len(got) / n
        assert (0.10 <= dropped <= 0.30) if thr == 0.05 else dropped == 0, (n, seed, thr, dropped)


@pytest.mark.parametrize('thr', [0.05, 0.001])
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n', SIZES)
def test_gaussian_twin_same_order_scores_inside_the_bound(n, seed, thr):
    rows = seg_rows(n, seed)
    want, wpos = dense_matrix_nms(rows, 2, thr=thr, pre_top=2048)
    got, pos = ops.cpu_matrix_nms(rows, 2, 0.5, thr, pre_top=2048)
    assert np.array_equal(pos, wpos)
    assert np.array_equal(bits(got[:, :4]), bits(want[:, :4]))
    assert np.all(np.abs(got[:, 4].astype(np.float64) - want[:, 4]) <= REL * want[:, 4])
    assert np.all(np.diff(got[:, 4]) <= 0)
    if n >= 37:
        dropped = 1 - len(got) / n
        assert (0.10 <= dropped <= 0.30) if thr == 0.05 else dropped == 0, (n, seed, thr, dropped)


# ------------------------------------------------------------------ hand cases
CHAIN = np.array([[0, 0, 99, 99, .9], [50, 0, 149, 99, .8], [100, 0, 199, 99, .7]], dtype=F)
COPIES = np.array([[0, 0, 99, 99, .9], [0, 0, 99, 99, .8], [0, 0, 99, 99, .7], [50, 0, 149, 99, .6]], dtype=F)
DISJOINT = np.array([[0, 0, 10, 10, .9], [100, 0, 110, 10, .5], [200, 0, 210, 10, .4], [300, 0, 310, 10, .3]], dtype=F)


def check_chain(got, pos):
    """A-B and B-C overlap by a third, A-C not at all: B decays to 2/3, and C's only term (1 - 1/3) / (1 - cmax[B]) is
    exactly 1 -- B's own suppression cancels it, which a plain one-shot decay (0.7 * 2/3) would not do."""
    third = F(5000) / F(15000)
    two_thirds = (F(1) - third) / F(1)
    assert (F(1) - third) / (F(1) - third) == F(1)
    want = np.array([F(.9), F(.8) * two_thirds, F(.7)], dtype=F)
    order = np.argsort(-want.astype(np.float64), kind='stable')
    assert pos.tolist() == order.tolist() == [0, 2, 1]
    assert np.array_equal(bits(got[:, 4]), bits(want[order]))
    assert np.array_equal(bits(got[:, :4]), bits(CHAIN[order, :4]))


def check_copies(got0, pos0, got, pos):
    """Three identical boxes, then D shifted by half: at threshold 0 the copies come out with score exactly 0 (their terms
    against A are 0 / 1; the terms whose denominator 1 - cmax is 0 are skipped) and D keeps 1 - ov(A, D); at 0.001 the copies
    are gone.  No NaN, no infinity."""
    ov_ad = F(5000) / F(15000)
    d_score = F(.6) * ((F(1) - ov_ad) / F(1))
    assert np.isfinite(got0).all() and np.isfinite(got).all()
    assert pos0.tolist() == [0, 3, 1, 2]
    assert np.array_equal(bits(got0[:, 4]), bits(np.array([.9, d_score, 0, 0], dtype=F)))
    assert pos.tolist() == [0, 3]
    assert np.array_equal(bits(got), bits(got0[:2]))


def test_hand_case_chain_linear():
    check_chain(*ops.cpu_matrix_nms(CHAIN, 1))
    check_chain(*dense_matrix_nms(CHAIN, 1))


def test_hand_case_duplicates_linear():
    check_copies(*ops.cpu_matrix_nms(COPIES, 1, score_threshold=0.0), *ops.cpu_matrix_nms(COPIES, 1))
    check_copies(*dense_matrix_nms(COPIES, 1, thr=0.0), *dense_matrix_nms(COPIES, 1))


@pytest.mark.parametrize('method', [1, 2])
def test_hand_case_disjoint_boxes_are_left_alone(method):
    got, pos = ops.cpu_matrix_nms(DISJOINT, method)
    assert pos.tolist() == [0, 1, 2, 3] and np.array_equal(bits(got), bits(DISJOINT))


def test_gaussian_duplicates_are_finite():
    got, pos = ops.cpu_matrix_nms(COPIES, 2, score_threshold=0.0)
    assert np.isfinite(got).all() and len(got) == 4 and pos[0] == 0 and np.all(np.diff(got[:, 4]) <= 0)


# ------------------------------------------------------------------ pre_top and max_emit
@pytest.mark.parametrize('method', [1, 2])
@pytest.mark.parametrize('n', [63, 64, 65])
def test_pre_top_is_the_rule_on_the_first_rows(n, method):
    rows = seg_rows(n, 4321)
    got, pos = ops.cpu_matrix_nms(rows, method, pre_top=64)
    want, wpos = ops.cpu_matrix_nms(rows[:64], method, pre_top=1024)
    assert np.array_equal(pos, wpos) and np.array_equal(bits(got), bits(want))
    assert (pos < 64).all()
    if method == 1:
        dense, dpos = dense_matrix_nms(rows, 1, pre_top=64)
        assert np.array_equal(pos, dpos) and np.array_equal(bits(got), bits(dense))


@pytest.mark.parametrize('method', [1, 2])
def test_max_emit_gives_a_prefix(method):
    for n, seed in ((600, 4321), (1100, 7)):
        rows = seg_rows(n, seed)
        full, fpos = ops.cpu_matrix_nms(rows, method, pre_top=2048)
        assert len(full) > 20
        for k in (1, 5, 20):
            got, pos = ops.cpu_matrix_nms(rows, method, pre_top=2048, max_emit=k)
            assert len(got) == k and np.array_equal(bits(got), bits(full[:k])) and np.array_equal(pos, fpos[:k])
        got, pos = ops.cpu_matrix_nms(rows, method, pre_top=2048, max_emit=len(full) + 5)
        assert np.array_equal(bits(got), bits(full)) and np.array_equal(pos, fpos)


TIES = np.array([[0, 0, 10, 10, 0.9], [100, 0, 110, 10, 0.5], [200, 0, 210, 10, 0.5], [300, 0, 310, 10, 0.5],
                 [400, 0, 410, 10, 0.4]], dtype=F)


@pytest.mark.parametrize('method', [1, 2])
def test_max_emit_keeps_ties_with_the_last_row(method):
    for fn in (lambda **k: ops.cpu_matrix_nms(TIES, method, **k), lambda **k: dense_matrix_nms(TIES, method, **k)):
        got, pos = fn(max_emit=2)
        assert pos.tolist() == [0, 1, 2, 3] and np.array_equal(bits(got), bits(TIES[:4]))
        assert fn(max_emit=1)[1].tolist() == [0]
        assert fn(max_emit=4)[1].tolist() == [0, 1, 2, 3]
        assert fn(max_emit=0)[1].tolist() == [0, 1, 2, 3, 4]


def test_twin_argument_errors():
    lib = _lib.lib()
    rows = np.array(TIES)
    out, pos, n_out = np.zeros((5, 5), F), np.zeros(5, np.int32), C.c_int(0)

    def call(method=1, sigma=0.5, pre_top=64, max_emit=0):
        return lib.ct_cpu_matrix_nms(rows.ctypes.data_as(C.c_void_p), 5, method, sigma, 0.001, pre_top, max_emit,
                                     out.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p),
                                     C.cast(C.byref(n_out), C.c_void_p))
    assert call() == 0 and n_out.value == 5
    for kw in (dict(method=0), dict(method=3), dict(method=2, sigma=0.0), dict(pre_top=0), dict(max_emit=-1)):
        assert call(**kw) == 1, kw
        assert lib.ct_last_error_string().decode().startswith('ct_cpu_matrix_nms')
    with pytest.raises(ValueError):
        ops.cpu_matrix_nms(rows, 0)
    with pytest.raises(ValueError):
        ops.cpu_matrix_nms(rows, 'linear')                      # the soft-NMS name is not a Matrix NMS method
    assert [ops.matrix_method(m) for m in ('matrix_linear', 'matrix_gaussian', 1, 2)] == [1, 2, 1, 2]


# ------------------------------------------------------------------ exports
def test_exports():
    out = subprocess.run(['nm', '-D', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == 'T'}
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    for n in NAMES:
        assert n in exported, n
        assert n in _lib.SIGNATURES, n
        assert re.search(r'\b(int|size_t)\s+%s\s*\(' % n, header), n
    # ct_soft_nms_batched_dev's arguments with Nt replaced by pre_top; the soft post-processing entry's likewise
    assert len(_lib.SIGNATURES['ct_matrix_nms_batched_dev'][1]) == len(_lib.SIGNATURES['ct_soft_nms_batched_dev'][1]) == 15
    assert len(_lib.SIGNATURES['ct_postprocess_batched_matrix'][1]) == len(_lib.SIGNATURES['ct_postprocess_batched_soft'][1])
    assert _lib.lib().ct_abi_version() == 1
    import importlib.util
    spec = importlib.util.spec_from_file_location('ctdet_build', os.path.join(REPO, 'context-transformer_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SOURCES['ct_matrix_nms.hip'] == ['-ffp-contract=off']


def test_max_rows_query():
    rows = _lib.lib().ct_matrix_nms_max_rows()
    assert rows >= 1024
    # boxes, areas, scores and cmax of that many rows leave room for several segments in a CU's 160 KiB of LDS
    assert rows * 28 * 2 <= 160 * 1024


def test_workspace_queries():
    lib = _lib.lib()
    for total, S in ((0, 1), (1, 1), (1100, 3), (32 * 20 * 11620, 640)):
        assert lib.ct_matrix_nms_batched_workspace_bytes(total, S) >= 0
    got = [lib.ct_matrix_nms_batched_workspace_bytes(r, 40) for r in (0, 1, 1024, 1025, 11620)]
    assert all(a <= b for a, b in zip(got, got[1:])), got
    base = lib.ct_postprocess_matrix_workspace_bytes(1, 16, 1)
    assert base > 0
    for b, p, t in ((2, 16, 1), (1, 600, 1), (1, 16, 3), (2, 600, 3), (32, 11620, 20), (32, 32756, 20)):
        got = lib.ct_postprocess_matrix_workspace_bytes(b, p, t)
        assert got > base, (b, p, t, got)
        assert got >= b * t * p * (5 + 1 + 1) * 4               # sorted rows, their prior indices, the emitted positions


# ------------------------------------------------------------------ argument errors
def test_matrix_nms_argument_errors_before_any_device_work():
    lib = _lib.lib()
    top = lib.ct_matrix_nms_max_rows()

    def call(dets=0x10000, seg_off=0x20000, S=3, maxlen=2000, method=1, sigma=0.5, thr=0.001, pre_top=1024, max_emit=0,
             rows=0x30000, pos=0x40000, cnt=0x50000, ws=None, nbytes=0):
        return lib.ct_matrix_nms_batched_dev(dets, seg_off, S, maxlen, method, sigma, thr, pre_top, max_emit, rows, pos, cnt,
                                             ws, nbytes, None)

    bad = [
        (dict(dets=None), 'null pointer'),
        (dict(seg_off=None), 'null pointer'),
        (dict(rows=None), 'null pointer'),
        (dict(pos=None), 'null pointer'),
        (dict(cnt=None), 'null pointer'),
        (dict(S=0), 'bad sizes'),
        (dict(S=-1), 'bad sizes'),
        (dict(maxlen=-1), 'bad sizes'),
        (dict(max_emit=-1), 'bad sizes'),
        (dict(method=0), 'method'),
        (dict(method=3), 'method'),
        (dict(method=-1), 'method'),
        (dict(method=2, sigma=0.0), 'sigma'),
        (dict(method=2, sigma=-1.0), 'sigma'),
        (dict(method=2, sigma=float('nan')), 'sigma'),
        (dict(thr=-0.5), 'score_threshold'),
        (dict(pre_top=0), 'pre_top'),
        (dict(pre_top=-3), 'pre_top'),
        (dict(pre_top=top + 1), 'pre_top'),
    ]
    for kw, word in bad:
        assert call(**kw) == 1, kw
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith('ct_matrix_nms_batched_dev') and word in msg, (kw, msg)


def test_postprocess_matrix_argument_errors_before_any_device_work():
    lib = _lib.lib()
    need = lib.ct_postprocess_matrix_workspace_bytes(2, 600, 3)
    top = lib.ct_matrix_nms_max_rows()

    def call(boxes=0x10000, scores=0x20000, B=2, P=600, T=3, conf=0.01, method=1, sigma=0.5, thr=0.001, pre_top=1024,
             mpi=200, cap=64, dets=0x30000, cnt=0x40000, idx=0x50000, ovf=0x60000, ws=0x70000, nbytes=need):
        return lib.ct_postprocess_batched_matrix(boxes, scores, B, P, T, conf, method, sigma, thr, pre_top, mpi, cap, dets,
                                                 cnt, idx, ovf, ws, nbytes, None)

    bad = [
        (dict(boxes=None), 'null pointer', 1),
        (dict(scores=None), 'null pointer', 1),
        (dict(dets=None), 'null pointer', 1),
        (dict(cnt=None), 'null pointer', 1),
        (dict(ovf=None), 'null pointer', 1),
        (dict(B=0), 'bad sizes', 1),
        (dict(P=-5), 'bad sizes', 1),
        (dict(T=0), 'bad sizes', 1),
        (dict(cap=0), 'bad sizes', 1),
        (dict(mpi=-1), 'bad sizes', 1),
        (dict(conf=-0.5), 'conf_thresh', 1),
        (dict(thr=-0.5), 'score_threshold', 1),
        (dict(method=0), 'method', 1),
        (dict(method=3), 'method', 1),
        (dict(method=2, sigma=0.0), 'sigma', 1),
        (dict(pre_top=0), 'pre_top', 1),
        (dict(pre_top=top + 1), 'pre_top', 1),
        (dict(ws=None), 'workspace', 3),
        (dict(nbytes=need - 1), 'workspace', 3),
    ]
    for kw, word, code in bad:
        assert call(**kw) == code, kw
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith('ct_postprocess_batched_matrix') and word in msg, (kw, msg)


# ------------------------------------------------------------------ what the Python surface hands to the library
@pytest.mark.parametrize('name,number', [('matrix_linear', 1), ('matrix_gaussian', 2)])
def test_postprocessor_matrix_methods_call_the_matrix_entry(recorded, name, number):
    pp = ops.PostProcessor(2, 600, 3, 'cpu', out_cap=64)
    boxes, scores = torch.zeros(2, 600, 4), torch.zeros(2, 600, 4)
    pp.run(boxes, scores, 0.02, 0.4, False, 100, nms_method=name, soft_sigma=0.6, soft_score_threshold=0.002,
           matrix_pre_top=512)
    need = _lib.lib().ct_postprocess_matrix_workspace_bytes(2, 600, 3)
    assert pp.matrix_ws is not None and pp.matrix_ws.numel() == need and pp.soft_ws is None
    (entry,) = recorded
    assert entry == ('ct_postprocess_batched_matrix', 'boxes', 'scores', 2, 600, 3, 0.02, number, 0.6, 0.002, 512, 100, 64,
                     'out_dets', 'out_count', 'out_index', 'overflow', 'matrix_ws', need, 'stream')
    ws = pp.matrix_ws
    pp.run(boxes, scores, nms_method=name)
    assert pp.matrix_ws is ws                           # allocated once
    assert recorded[-1][10] == 1024                     # the default pre_top


def test_other_methods_leave_the_matrix_workspace_alone(recorded):
    pp = ops.PostProcessor(2, 600, 3, 'cpu', out_cap=64)
    boxes, scores = torch.zeros(2, 600, 4), torch.zeros(2, 600, 4)
    pp.run(boxes, scores)
    pp.run(boxes, scores, nms_method='linear', matrix_pre_top=7)
    assert [e[0] for e in recorded] == ['ct_postprocess_batched', 'ct_postprocess_batched_soft']
    assert pp.matrix_ws is None
    with pytest.raises(ValueError):
        pp.run(boxes, scores, nms_method='matrix')
    with pytest.raises(ValueError):
        ops.soft_method('matrix_linear')                # soft_method keeps its domain
    with pytest.raises(ValueError):
        ops.soft_method(3)
    assert ops.nms_method_number('hard') == (False, 0) and ops.nms_method_number('gaussian') == (False, 2)
    assert ops.nms_method_number('matrix_linear') == (True, 1) and ops.nms_method_number('matrix_gaussian') == (True, 2)


def test_pipeline_graph_key_separates_the_five_methods_and_pre_top():
    names = ('hard', 'linear', 'gaussian', 'matrix_linear', 'matrix_gaussian')
    keys = {m: _pipe(nms_method=m)._post_key() for m in names}
    assert len(set(keys.values())) == 5
    assert keys['hard'] == (0.01, 0.45, False, 200)     # the default pipeline's key is the one it had
    assert keys['linear'] == (0.01, 0.45, False, 200, 1, 0.5, 0.001)
    ml = keys['matrix_linear']
    assert _pipe(nms_method='matrix_linear', matrix_pre_top=1024)._post_key() == ml      # read defensively: 1024 when absent
    assert _pipe(nms_method='matrix_linear', matrix_pre_top=512)._post_key() != ml
    assert _pipe(nms_method='matrix_linear', soft_sigma=0.7)._post_key() != ml
    assert _pipe(nms_method='matrix_linear', soft_score_threshold=0.01)._post_key() != ml
    for m in ('hard', 'linear', 'gaussian'):            # pre_top is part of the key for the matrix methods only
        assert _pipe(nms_method=m, matrix_pre_top=512)._post_key() == keys[m]


def test_pipeline_step_hands_pre_top_to_the_postprocessor_for_matrix_methods_only():
    import inspect
    import unittest.mock as mock
    sig = inspect.signature(pipeline.DetectionPipeline.__init__).parameters
    assert sig['matrix_pre_top'].default == 1024 and sig['nms_method'].default == 'hard'
    sig = inspect.signature(ops.PostProcessor.run).parameters
    assert sig['matrix_pre_top'].default == 1024 and list(sig)[-2:] == ['box_vote', 'matrix_pre_top']
    calls = []

    class Post:
        def run(self, *a):
            calls.append(a[2:])

    class Net:
        def forward_raw(self, *a, **k):
            return torch.zeros(1), torch.zeros(1), torch.zeros(1)

    with mock.patch.object(ops, 'detect_fused', lambda *a, **k: None):
        for kw in (dict(nms_method='hard', matrix_pre_top=512), dict(nms_method='matrix_linear'),
                   dict(nms_method='matrix_gaussian', matrix_pre_top=512, box_vote=0.5)):
            p = _pipe(net=Net(), post=Post(), priors=None, variance=None, scale=None, boxes=None, scores=None, batch=1, **kw)
            p._step()
    assert calls == [(0.01, 0.45, False, 200, 'hard', 0.5, 0.001),
                     (0.01, 0.45, False, 200, 'matrix_linear', 0.5, 0.001, None, 1024),
                     (0.01, 0.45, False, 200, 'matrix_gaussian', 0.5, 0.001, 0.5, 512)]


def test_harness_passes_pre_top_through():
    import inspect
    from ctdet import harness
    for fn in (harness.do_test, harness.detect_dataset):
        assert inspect.signature(fn).parameters['matrix_pre_top'].default == 1024
