"""nms_segments_kernel (csrc/ct_nms.hip) on pairs whose IoU is equal to the threshold, within 5e-6 of it on either side
(inside make_thr's 1e-5 band: IEEE division decides) or 2e-5 .. 5e-5 away (outside: the reciprocal estimate decides),
with the kept box of every pair placed so that the comparison happens in a chosen loop: the ballot loop of one wave, the
head / 4-wide body (each of its lanes) / tail of test_range across waves and across chunks, and the part behind the
2048-entry LDS window.  tests/test_post_cases_cpu.py proves the placements and the kinds without a device.  Kept indices
must equal the reference's: oracle/nms_ref.nms_sorted_c for the +1 rule, post_cases.plain_nms_sorted for box_utils' rule."""
import numpy as np
import pytest
import torch

import post_cases as pc
from ctdet import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROTS = range(len(pc.KINDS))


@pytest.mark.parametrize('plain', [False, True], ids=['plus1', 'plain'])
@pytest.mark.parametrize('thresh', pc.NMS_THRESHOLDS)
def test_borderline_segments_through_nms_sorted_host(thresh, plain):
    for name in pc.SEGMENTS:
        for rot in ROTS:
            rows, _ = pc.borderline_segment(name, thresh, rot, plain)
            for ge in (False, True):
                got = ops.nms_sorted_host(rows, thresh, ge=ge, plain_iou=plain)
                want = pc.nms_reference(rows, thresh, ge, plain)
                assert np.array_equal(got, want), (name, rot, ge, sorted(set(want.tolist()) ^ set(got.tolist())))


@pytest.mark.parametrize('ge', [False, True])
@pytest.mark.parametrize('thresh', pc.NMS_THRESHOLDS)
def test_borderline_segments_in_one_csr_launch(thresh, ge):
    """segments of different lengths, an empty one among them, in one ct_nms_batched_dev launch"""
    for rot in ROTS:
        segs = [pc.borderline_segment('waves', thresh, rot)[0], np.zeros((0, 5), np.float32),
                pc.borderline_segment('beyond', thresh, rot)[0], pc.borderline_segment('waves3', thresh, (rot + 1) % 5)[0],
                pc.borderline_segment('phase_a', thresh, (rot + 2) % 5)[0]]
        off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int32)
        dets = torch.from_numpy(np.concatenate(segs, 0)).to(DEV)
        keep, cnt = ops.nms_batched(dets, torch.from_numpy(off).to(DEV), thresh, ge=ge)
        keep, cnt = keep.cpu().numpy(), cnt.cpu().numpy()
        for s, rows in enumerate(segs):
            want = pc.nms_reference(rows, thresh, ge, False)
            assert cnt[s] == len(want), (rot, s)
            assert np.array_equal(keep[off[s]:off[s] + cnt[s]], want), (rot, s)
