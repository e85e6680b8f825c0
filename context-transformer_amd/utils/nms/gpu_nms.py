"""gpu_nms -- replaces the reference's Cython shim utils/nms/gpu_nms.pyx:16-31.

argsort by descending score on the host (ties: lower index first -- the reference's tie order
is numpy-implementation-defined), then the `_nms`-contract entry point of libctdet
(`ct_nms_sorted_host`, the HIP twin of utils/nms/nms_kernel.cu:91-144), then map back.
"""
import numpy as np

from ctdet import ops


def gpu_nms(dets, thresh, device_id=0):
    dets = np.ascontiguousarray(dets, dtype=np.float32)
    if dets.shape[0] == 0:
        return []
    order = np.argsort(-dets[:, 4], kind='stable')
    keep = ops.nms_sorted_host(dets[order, :], thresh, ge=False, device_id=device_id)
    return list(order[keep])


def gpu_soft_nms(boxes, sigma=0.5, Nt=0.3, threshold=0.001, method=0, device_id=0):
    """Drop-in for cpu_soft_nms (utils/nms/cpu_nms.pyx:70-163) on the device: the rows are put in descending score order
    (ties: lower index first), one segment runs through `ct_soft_nms_batched_dev`, the emitted rows (boxes and decayed
    scores) are written back into `boxes[:N']` and list(range(N')) is returned.  Methods 0 and 1 give cpu_soft_nms's
    rows bit for bit on tie-free input, method 2 the same rows with scores within an ulp of the weight per decay."""
    import torch
    if not (isinstance(boxes, np.ndarray) and boxes.dtype == np.float32 and boxes.flags['C_CONTIGUOUS']
            and boxes.ndim == 2 and boxes.shape[1] == 5):
        raise ValueError('gpu_soft_nms needs a C-contiguous float32 [n,5] array (it is updated in place)')
    n = boxes.shape[0]
    if n == 0:
        return []
    order = np.argsort(-boxes[:, 4], kind='stable')
    dev = torch.device('cuda', device_id)
    with torch.cuda.device(dev):
        dets = torch.from_numpy(boxes[order]).to(dev)
        seg_off = torch.tensor([0, n], dtype=torch.int32, device=dev)
        rows, _, cnt = ops.soft_nms_batched(dets, seg_off, method, sigma, Nt, threshold)
        k = int(cnt.item())
        if k < 0:
            raise RuntimeError('ct_soft_nms_batched_dev: workspace too small for %d rows' % n)
        boxes[:k] = rows[:k].cpu().numpy()
    return list(range(k))
