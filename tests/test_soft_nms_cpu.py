"""Soft-NMS on the device (csrc/ct_soft_nms.hip, ct_postprocess_batched_soft) without a device: exports, the argument checks
that return before any device work, the workspace queries, the alive-set formulation the kernel implements (restated here in
numpy fp32) against the swapping reference, and what PostProcessor / DetectionPipeline hand to the library (recording proxy
as in tests/test_wgrad_h2_cpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from ctdet import _lib, ops, pipeline, synth
from oracle import nms_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ct_soft_nms_lds_rows', 'ct_soft_nms_batched_workspace_bytes', 'ct_soft_nms_batched_dev',
         'ct_postprocess_soft_workspace_bytes', 'ct_postprocess_batched_soft')
F = np.float32


# ------------------------------------------------------------------ the contract, restated
def alive_set_soft_nms(dets_sorted, sigma=0.5, Nt=0.3, threshold=0.001, method=0, max_emit=0, trace=None):
    """The formulation of csrc/ct_soft_nms.hip on rows in the pipeline's order -> (rows [k,5], positions [k]).
    trace: a dict that receives the smallest relative margins of the run, 'select' = (top - second) / top over all
    selections and 'threshold' = |score - threshold| / threshold over all threshold comparisons."""
    d = np.ascontiguousarray(dets_sorted, dtype=F)
    n = d.shape[0]
    x1, y1, x2, y2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    score = d[:, 4].copy()
    alive = np.ones(n, dtype=bool)
    one = F(1)
    area = (x2 - x1 + one) * (y2 - y1 + one)
    rows, pos = [], []
    sel_margin = thr_margin = np.inf
    while alive.any():
        idx = np.flatnonzero(alive)
        m = idx[np.argmax(score[idx])]                  # first maximum = lowest position
        if max_emit > 0 and len(rows) >= max_emit and score[m] != rows[-1][4]:
            break
        if len(idx) > 1:
            second = np.partition(score[idx], -2)[-2]
            sel_margin = min(sel_margin, float((np.float64(score[m]) - second) / score[m]))
        rows.append(np.array([x1[m], y1[m], x2[m], y2[m], score[m]], dtype=F))
        pos.append(m)
        alive[m] = False
        j = np.flatnonzero(alive)
        if not len(j):
            break
        iw = np.minimum(x2[m], x2[j]) - np.maximum(x1[m], x1[j]) + one
        ih = np.minimum(y2[m], y2[j]) - np.maximum(y1[m], y1[j]) + one
        hit = (iw > 0) & (ih > 0)
        j, iw, ih = j[hit], iw[hit], ih[hit]
        inter = iw * ih
        ua = (x2[m] - x1[m] + one) * (y2[m] - y1[m] + one) + area[j] - inter
        ov = inter / ua
        if method == 1:
            w = np.where(ov > F(Nt), one - ov, one).astype(F)
        elif method == 2:
            w = np.exp(-(ov.astype(np.float64) * ov.astype(np.float64)) / np.float64(F(sigma))).astype(F)
        else:
            w = np.where(ov > F(Nt), F(0), one).astype(F)
        s = (w * score[j]).astype(F)
        score[j] = s
        if len(j):
            thr_margin = min(thr_margin, float(np.min(np.abs(s.astype(np.float64) - F(threshold))) / F(threshold)))
        alive[j[s < F(threshold)]] = False
    if trace is not None:
        trace['select'], trace['threshold'] = sel_margin, thr_margin
    out = np.stack(rows) if rows else np.zeros((0, 5), dtype=F)
    return out, np.asarray(pos, dtype=np.int64)


def sorted_rows(dets):
    return np.ascontiguousarray(dets[nms_ref.stable_desc_order(dets[:, 4])], dtype=F)


# ------------------------------------------------------------------ exports
def test_exports():
    out = subprocess.run(['nm', '-D', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == 'T'}
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    for n in NAMES:
        assert n in exported, n
        assert n in _lib.SIGNATURES, n
        assert re.search(r'\b(int|size_t)\s+%s\s*\(' % n, header), n
    assert len(_lib.SIGNATURES['ct_soft_nms_batched_dev'][1]) == 15
    # ct_postprocess_batched's arguments with (nms_thresh, ge) replaced by (method, sigma, Nt, score_threshold)
    assert len(_lib.SIGNATURES['ct_postprocess_batched_soft'][1]) == len(_lib.SIGNATURES['ct_postprocess_batched'][1]) + 2
    assert _lib.lib().ct_abi_version() == 1
    assert re.search(r'#define\s+CTDET_ABI_VERSION\s+1\b', header)


def test_lds_rows_query():
    rows = _lib.lib().ct_soft_nms_lds_rows()
    assert rows >= 256 and rows % 256 == 0, rows
    # boxes and scores of that many rows leave room for several segments in a CU's 160 KiB of LDS
    assert rows * 20 * 4 <= 160 * 1024


# ------------------------------------------------------------------ workspace queries
def test_workspace_queries_positive_and_monotone():
    lib = _lib.lib()
    rows = [0, 1, 255, 1024, 1025, 11620, 32756 * 20, 32 * 20 * 11620]
    for S in (1, 40, 640):
        got = [lib.ct_soft_nms_batched_workspace_bytes(r, S) for r in rows]
        assert all(g > 0 for g in got), got
        assert all(a <= b for a, b in zip(got, got[1:])), got
        assert got[-1] >= rows[-1] * 4 and got[-1] > got[0]
    for r in (1, 1025, 11620):
        got = [lib.ct_soft_nms_batched_workspace_bytes(r, S) for S in (1, 2, 64, 640, 6400)]
        assert all(a <= b for a, b in zip(got, got[1:])), got
    base = lib.ct_postprocess_soft_workspace_bytes(1, 16, 1)
    assert base > 0
    for b, p, t in ((2, 16, 1), (1, 600, 1), (1, 16, 3), (2, 600, 3), (32, 11620, 20), (32, 32756, 20)):
        got = lib.ct_postprocess_soft_workspace_bytes(b, p, t)
        assert got > base, (b, p, t, got)
        assert got >= b * t * p * (5 + 1 + 1) * 4               # sorted rows, their prior indices, the emitted positions
    assert lib.ct_postprocess_soft_workspace_bytes(32, 11620, 20) < lib.ct_postprocess_soft_workspace_bytes(32, 32756, 20)


# ------------------------------------------------------------------ argument errors
def test_soft_nms_argument_errors_before_any_device_work():
    lib = _lib.lib()
    need = lib.ct_soft_nms_batched_workspace_bytes(2000, 3)

    def call(dets=0x10000, seg_off=0x20000, S=3, maxlen=2000, method=1, sigma=0.5, Nt=0.3, thr=0.001, max_emit=0,
             rows=0x30000, pos=0x40000, cnt=0x50000, ws=0x60000, nbytes=need):
        return lib.ct_soft_nms_batched_dev(dets, seg_off, S, maxlen, method, sigma, Nt, thr, max_emit, rows, pos, cnt, ws,
                                           nbytes, None)

    bad = [
        (dict(dets=None), 'null pointer', 1),
        (dict(seg_off=None), 'null pointer', 1),
        (dict(rows=None), 'null pointer', 1),
        (dict(pos=None), 'null pointer', 1),
        (dict(cnt=None), 'null pointer', 1),
        (dict(S=0), 'bad sizes', 1),
        (dict(S=-1), 'bad sizes', 1),
        (dict(maxlen=-1), 'bad sizes', 1),
        (dict(max_emit=-1), 'bad sizes', 1),
        (dict(method=3), 'method', 1),
        (dict(method=-1), 'method', 1),
        (dict(method=2, sigma=0.0), 'sigma', 1),
        (dict(method=2, sigma=-1.0), 'sigma', 1),
        (dict(method=2, sigma=float('nan')), 'sigma', 1),
        (dict(ws=None), 'workspace', 3),
        (dict(nbytes=need - 1), 'workspace', 3),
        (dict(nbytes=0), 'workspace', 3),
    ]
    for kw, word, code in bad:
        assert call(**kw) == code, kw
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith('ct_soft_nms_batched_dev') and word in msg, (kw, msg)


def test_postprocess_soft_argument_errors_before_any_device_work():
    lib = _lib.lib()
    need = lib.ct_postprocess_soft_workspace_bytes(2, 600, 3)

    def call(boxes=0x10000, scores=0x20000, B=2, P=600, T=3, conf=0.01, method=1, sigma=0.5, Nt=0.45, thr=0.001, mpi=200,
             cap=64, dets=0x30000, cnt=0x40000, idx=0x50000, ovf=0x60000, ws=0x70000, nbytes=need):
        return lib.ct_postprocess_batched_soft(boxes, scores, B, P, T, conf, method, sigma, Nt, thr, mpi, cap, dets, cnt,
                                               idx, ovf, ws, nbytes, None)

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
        (dict(method=3), 'method', 1),
        (dict(method=-2), 'method', 1),
        (dict(method=2, sigma=0.0), 'sigma', 1),
        (dict(ws=None), 'workspace', 3),
        (dict(nbytes=need - 1), 'workspace', 3),
    ]
    for kw, word, code in bad:
        assert call(**kw) == code, kw
        msg = lib.ct_last_error_string().decode()
        assert msg.startswith('ct_postprocess_batched_soft') and word in msg, (kw, msg)


# ------------------------------------------------------------------ the formulation equals the swapping reference
@pytest.mark.parametrize('method', [0, 1, 2])
@pytest.mark.parametrize('n,seed', [(1, 4321), (2, 7), (37, 4321), (64, 7), (65, 4321), (130, 7), (300, 4321)])
def test_alive_set_formulation_equals_the_swapping_reference(n, seed, method):
    rows = sorted_rows(synth.clustered_dets(n, seed=seed))
    ref = rows.copy()
    k = nms_ref.soft_nms(ref, 0.5, 0.3, 0.001, method)
    got, pos = alive_set_soft_nms(rows, 0.5, 0.3, 0.001, method)
    assert len(got) == k
    assert np.array_equal(got.view(np.uint32), ref[:k].view(np.uint32))
    assert np.array_equal(rows[pos, :4], got[:, :4]) and len(set(pos.tolist())) == k
    assert np.all(np.diff(got[:, 4]) <= 0)
    for cap in (1, 5):
        lim, _ = alive_set_soft_nms(rows, 0.5, 0.3, 0.001, method, max_emit=cap)
        assert np.array_equal(lim, got[:cap])


@pytest.mark.parametrize('method', [0, 1, 2])
def test_alive_set_formulation_equals_the_recorded_reference(golden, method):
    g = golden('nms.npz')
    if not bool(g['have_ge']):
        pytest.skip('no patched reference build was available when goldens were made')
    got, _ = alive_set_soft_nms(sorted_rows(g['c6_dets']), 0.5, 0.3, 0.001, method)
    n = int(g['soft_m%d_n' % method])
    ref = g['soft_m%d_boxes' % method]
    assert len(got) == n
    assert np.array_equal(got[:, :4], ref[:n, :4])
    np.testing.assert_allclose(got[:, 4], ref[:n, 4], rtol=2e-6, atol=0)


def test_emission_limit_keeps_ties_with_the_last_row():
    rows = np.array([[0, 0, 10, 10, 0.9], [100, 0, 110, 10, 0.5], [200, 0, 210, 10, 0.5], [300, 0, 310, 10, 0.4]], dtype=F)
    got, pos = alive_set_soft_nms(rows, method=1, max_emit=2)
    assert pos.tolist() == [0, 1, 2]
    got, pos = alive_set_soft_nms(rows, method=1, max_emit=3)
    assert pos.tolist() == [0, 1, 2]


# ------------------------------------------------------------------ what the Python surface hands to the library
class _Lib:
    """Host queries go to the real library, every other call is recorded instead of run."""

    def __init__(self, log):
        self._real, self._log = _lib.lib(), log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.endswith('_bytes'):
            return fn

        def call(*args):
            self._log.append((name,) + tuple(getattr(a, 'value', a) for a in args))
            return 0
        return call


@pytest.fixture
def recorded(monkeypatch):
    log = []
    monkeypatch.setattr(ops, 'lib', lambda: _Lib(log))
    monkeypatch.setattr(ops, '_dev', lambda t, name, dtype=torch.float32: name)
    monkeypatch.setattr(ops, '_stream', lambda: 'stream')
    return log


def test_postprocessor_default_makes_the_call_it_made_before(recorded):
    pp = ops.PostProcessor(2, 600, 3, 'cpu', out_cap=64)
    boxes, scores = torch.zeros(2, 600, 4), torch.zeros(2, 600, 4)
    before = ('ct_postprocess_batched', 'boxes', 'scores', 2, 600, 3, 0.01, 0.45, 0, 200, 64, 'out_dets', 'out_count',
              'out_index', 'overflow', 'ws', pp.ws_bytes, 'stream')
    pp.run(boxes, scores)
    pp.run(boxes, scores, 0.01, 0.45, False, 200, nms_method='hard')
    pp.run(boxes, scores, nms_method='hard', soft_sigma=0.7, soft_score_threshold=0.1)
    assert recorded == [before] * 3
    assert pp.soft_ws is None                           # the soft workspace is not even allocated
    del recorded[:]
    pp.run(boxes, scores, 0.05, 0.5, True, 0)
    assert recorded == [('ct_postprocess_batched', 'boxes', 'scores', 2, 600, 3, 0.05, 0.5, 1, 0, 64, 'out_dets', 'out_count',
                         'out_index', 'overflow', 'ws', pp.ws_bytes, 'stream')]


@pytest.mark.parametrize('name,number', [('linear', 1), ('gaussian', 2)])
def test_postprocessor_soft_methods_call_the_soft_entry(recorded, name, number):
    pp = ops.PostProcessor(2, 600, 3, 'cpu', out_cap=64)
    boxes, scores = torch.zeros(2, 600, 4), torch.zeros(2, 600, 4)
    pp.run(boxes, scores, 0.02, 0.4, False, 100, nms_method=name, soft_sigma=0.6, soft_score_threshold=0.002)
    need = _lib.lib().ct_postprocess_soft_workspace_bytes(2, 600, 3)
    assert pp.soft_ws is not None and pp.soft_ws.numel() == need
    (entry,) = recorded
    assert entry == ('ct_postprocess_batched_soft', 'boxes', 'scores', 2, 600, 3, 0.02, number, 0.6, 0.4, 0.002, 100, 64,
                     'out_dets', 'out_count', 'out_index', 'overflow', 'soft_ws', need, 'stream')
    assert entry[9] == 0.4                              # Nt == nms_thresh
    ws = pp.soft_ws
    pp.run(boxes, scores, nms_method=name)
    assert pp.soft_ws is ws                             # allocated once


def test_unknown_method_names_are_errors(recorded):
    pp = ops.PostProcessor(1, 16, 1, 'cpu', out_cap=4)
    with pytest.raises(ValueError):
        pp.run(torch.zeros(1, 16, 4), torch.zeros(1, 16, 2), nms_method='soft')
    with pytest.raises(ValueError):
        ops.soft_method(3)
    assert recorded == []
    assert [ops.soft_method(m) for m in ('hard', 'linear', 'gaussian', 0, 1, 2)] == [0, 1, 2, 0, 1, 2]


def _pipe(**kw):
    p = pipeline.DetectionPipeline.__new__(pipeline.DetectionPipeline)
    p.conf_thresh, p.nms_thresh, p.ge, p.max_per_image = 0.01, 0.45, False, 200
    p.nms_method, p.soft_sigma, p.soft_score_threshold = 'hard', 0.5, 0.001
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_pipeline_graph_key_separates_the_methods():
    keys = {m: _pipe(nms_method=m)._post_key() for m in ('hard', 'linear', 'gaussian')}
    assert len(set(keys.values())) == 3
    assert keys['hard'] == (0.01, 0.45, False, 200)     # the default pipeline's key is the one it had
    assert _pipe(nms_method='linear', soft_sigma=0.7)._post_key() != keys['linear']
    assert _pipe(nms_method='linear', soft_score_threshold=0.01)._post_key() != keys['linear']
    assert _pipe(nms_method='linear', nms_thresh=0.3)._post_key() != keys['linear']


def test_pipeline_step_hands_the_method_to_the_postprocessor():
    import inspect
    sig = inspect.signature(pipeline.DetectionPipeline.__init__).parameters
    assert [sig[k].default for k in ('nms_method', 'soft_sigma', 'soft_score_threshold')] == ['hard', 0.5, 0.001]
    calls = []

    class Post:
        def run(self, *a):
            calls.append(a[2:])

    class Net:
        def forward_raw(self, *a, **k):
            return torch.zeros(1), torch.zeros(1), torch.zeros(1)

    import unittest.mock as mock
    with mock.patch.object(ops, 'detect_fused', lambda *a, **k: None):
        for m in ('hard', 'gaussian'):
            p = _pipe(nms_method=m, net=Net(), post=Post(), priors=None, variance=None, scale=None, boxes=None, scores=None,
                      batch=1)
            p._step()
    assert calls == [(0.01, 0.45, False, 200, 'hard', 0.5, 0.001), (0.01, 0.45, False, 200, 'gaussian', 0.5, 0.001)]
