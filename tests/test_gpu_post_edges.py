"""The hard-NMS post-processing chain (csrc/ct_post.hip: threshold -> per-class sort -> NMS -> per-image top-k -> gather)
at the sizes where it switches between special cases, bit for bit against the oracle loop (tests/post_cases.reference,
which asserts itself against oracle/nms_ref.postprocess_image).  The inputs are small and built on bit patterns;
tests/test_post_cases_cpu.py proves, without a device, that each one reaches the branch its name says.  No tolerance
anywhere: counts, rows, prior indices and the untouched rest of the output buffers are compared exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import post_cases as pc
from ctdet import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _cuda(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)      # the cached cases are read-only


def _run(pp, boxes, scores, k):
    pp.out_dets.fill_(float('nan'))
    pp.out_index.fill_(-7)
    pp.out_count.fill_(-7)
    pp.run(_cuda(boxes), _cuda(scores), k['conf_thresh'], k['nms_thresh'], k['ge'], k['max_per_image'])
    torch.cuda.synchronize()
    return (pp.out_dets.cpu().numpy(), pp.out_index.cpu().numpy(), pp.out_count.cpu().numpy(), int(pp.overflow.item()))


def _check(got, want, cap, tag):
    """every (image, class): count, rows, prior indices, and nothing written behind the count"""
    dets, index, count, overflow = got
    over = 0
    for b, per in enumerate(want):
        for c, (rows, idx) in enumerate(per):
            n = min(len(idx), cap)
            over |= len(idx) > cap
            assert count[b, c] == n, (tag, b, c, int(count[b, c]), len(idx))
            assert np.array_equal(dets[b, c, :n].view(np.uint32), rows[:n].view(np.uint32)), (tag, b, c)
            assert np.array_equal(index[b, c, :n], idx[:n]), (tag, b, c)
            assert np.isnan(dets[b, c, n:]).all() and (index[b, c, n:] == -7).all(), (tag, b, c)
    assert overflow == int(over), (tag, overflow)


def _fresh(boxes, scores, k, cap=None):
    B, P, T1 = scores.shape
    pp = ops.PostProcessor(B, P, T1 - 1, DEV, out_cap=cap or k['out_cap'] or P)
    return pp, _run(pp, boxes, scores, k)


@pytest.mark.parametrize('name', list(pc.CASES))
def test_chain_case_vs_oracle(name):
    boxes, scores, k = pc.case(name)
    pp, got = _fresh(boxes, scores, k)
    _check(got, pc.case_reference(name), pp.cap, name)


# ------------------------------------------------------------------ G: outputs
def _g():
    boxes, scores, k = pc.case_G()
    want = pc.reference(boxes, scores, **k)
    return boxes, scores, k, want, max(len(i) for per in want for _, i in per)


@pytest.mark.parametrize('short', [1, 0])
def test_out_cap_clamp_and_overflow(short):
    """out_cap one below the largest oracle count: overflow == 1, every count min(oracle, cap), the first cap oracle rows;
    out_cap equal to it: overflow == 0"""
    boxes, scores, k, want, largest = _g()
    cap = largest - short
    pp, got = _fresh(boxes, scores, k, cap=cap)
    assert got[3] == short
    _check(got, want, cap, 'cap%d' % cap)


def test_outputs_inside_guard_buffers():
    boxes, scores, k, want, largest = _g()
    B, P, T1 = scores.shape
    T, cap, pad = T1 - 1, largest - 1, 256
    pp = ops.PostProcessor(B, P, T, DEV, out_cap=cap)
    big_d = torch.full((B * T * cap * 5 + 2 * pad,), -7.0, device=DEV)
    big_i = torch.full((B * T * cap + 2 * pad,), -9, device=DEV, dtype=torch.int32)
    pp.out_dets = big_d[pad:-pad].view(B, T, cap, 5)
    pp.out_index = big_i[pad:-pad].view(B, T, cap)
    got = _run(pp, boxes, scores, k)
    _check(got, want, cap, 'guards')
    assert got[3] == 1
    hd, hi = big_d.cpu().numpy(), big_i.cpu().numpy()
    assert (hd[:pad] == -7).all() and (hd[-pad:] == -7).all()
    assert (hi[:pad] == -9).all() and (hi[-pad:] == -9).all()


def test_null_out_index_through_the_c_abi():
    boxes, scores, k, want, largest = _g()
    B, P, T1 = scores.shape
    T, cap = T1 - 1, largest
    pp = ops.PostProcessor(B, P, T, DEV, out_cap=cap)
    pp.out_dets.fill_(float('nan'))
    pp.out_index.fill_(-7)
    db, ds = _cuda(boxes), _cuda(scores)
    ops.check(ops.lib().ct_postprocess_batched(
        ops._dev(db, 'boxes'), ops._dev(ds, 'scores'), B, P, T, float(k['conf_thresh']), float(k['nms_thresh']),
        int(k['ge']), int(k['max_per_image']), cap, ops._dev(pp.out_dets, 'out_dets'),
        ops._dev(pp.out_count, 'out_count', torch.int32), C.c_void_p(0), ops._dev(pp.overflow, 'overflow', torch.int32),
        ops._dev(pp.ws, 'ws', torch.uint8), pp.ws_bytes, ops._stream()), 'ct_postprocess_batched')
    torch.cuda.synchronize()
    dets, count = pp.out_dets.cpu().numpy(), pp.out_count.cpu().numpy()
    assert int(pp.overflow.item()) == 0 and (pp.out_index.cpu().numpy() == -7).all()
    for b, per in enumerate(want):
        for c, (rows, idx) in enumerate(per):
            assert count[b, c] == len(idx), (b, c)
            assert np.array_equal(dets[b, c, :len(idx)].view(np.uint32), rows.view(np.uint32)), (b, c)
            assert np.isnan(dets[b, c, len(idx):]).all(), (b, c)


# ------------------------------------------------------------------ H: one workspace, runs of different regimes
def test_workspace_reuse_across_regimes():
    """seg_len, redo and thr_img persist in the workspace: after each run of the sequence the result is the oracle's and
    bit-equal to a fresh PostProcessor's on the same input.  The workspace starts as 0xFF."""
    steps = pc.case_H_steps()
    B, P, T1 = steps[0][1][1].shape
    pp = ops.PostProcessor(B, P, T1 - 1, DEV, out_cap=P)
    pp.ws.fill_(0xFF)
    for tag, (boxes, scores, k) in steps:
        got = _run(pp, boxes, scores, k)
        _check(got, pc.reference(boxes, scores, **k), P, tag)
        _, fresh = _fresh(boxes, scores, k)
        assert got[3] == fresh[3] and np.array_equal(got[2], fresh[2]), tag
        assert np.array_equal(got[0].view(np.uint32), fresh[0].view(np.uint32)), tag
        assert np.array_equal(got[1], fresh[1]), tag
