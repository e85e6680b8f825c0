"""Shared inputs of tests/test_atss_cpu.py and tests/test_gpu_atss.py: every case of the ATSS matcher is built once, the
numpy twin (tests/atss_ref.py) evaluated on it once and handed out unchanged.  A case is a namespace: targets (list of [G,6]
float32 tensors), priors [P,4] float32 tensor, off (level offsets), topk, max_gt, and ref = the twin's result."""
import functools
import types

import numpy as np
import torch

import atss_ref
import iou_loss_cases as cases

VAR = (0.1, 0.2)


@functools.lru_cache(None)
def pyramid(size):
    """-> priors [P,4], level offsets of VOC_300 / VOC_512."""
    from layers.functions import PriorBox
    import data as cfgs
    pb = PriorBox(cfgs.VOC_300 if size == 300 else cfgs.VOC_512)
    return pb.forward(), pb.level_offsets()


@functools.lru_cache(None)
def small_pyramid():
    """Levels of 4x4 cells x 2 priors, 2x2 x 2 and 1x1 x 1: P = 41, every number dyadic, small enough to enumerate by hand."""
    rows = []
    for cells, shapes in ((4, ((0.25, 0.25), (0.375, 0.125))), (2, ((0.5, 0.5), (0.75, 0.25))), (1, ((0.875, 0.875),))):
        for i in range(cells):
            for j in range(cells):
                rows.extend(((j + 0.5) / cells, (i + 0.5) / cells, w, h) for w, h in shapes)
    return torch.tensor(rows, dtype=torch.float32), [0, 32, 40, 41]


def _rows(*rows):
    return torch.tensor(rows, dtype=torch.float32).view(-1, 6)


# the four boxes of the small pyramid.  Box 0 is centred on a cell corner of level 0 and on a cell centre of level 1; box 3 IS
# prior 32 (level 1, cell 0, the square one), which box 0 claims too
SMALL_BOXES = _rows((0.0625, 0.0625, 0.4375, 0.4375, 1, 1.0), (0.5, 0.125, 1.0, 0.375, 2, 1.0),
                    (0.5625, 0.5625, 0.9375, 0.9375, 3, 0.5), (0.0, 0.0, 0.5, 0.5, 4, 1.0))

# edge cases, one image each, all on VOC_512 (its prior centres are dyadic: (i + 0.5) / 64 on level 0)
TINY = (0.0260, 0.0260, 0.0300, 0.0300, 5, 1.0)          # contains no prior centre of any level


def _edge_images():
    pri, off = pyramid(512)
    tiny = atss_ref.box_candidates(np.asarray(TINY, np.float32), pri.numpy(), off, 9)
    # the prior the tiny box is forced onto, as a box of its own: it claims that prior too, as an ordinary positive
    p = pri[int(tiny.idx[tiny.forced])]
    twin_of_prior = (max(float(p[0] - p[2] / 2), 0.0), max(float(p[1] - p[3] / 2), 0.0), float(p[0] + p[2] / 2),
                     float(p[1] + p[3] / 2), 7, 1.0)
    return {
        'empty': torch.zeros(0, 6),
        'whole_image': _rows((0.0, 0.0, 1.0, 1.0, 3, 1.0)),
        'tiny': _rows(TINY),
        'degenerate': _rows((0.3, 0.2, 0.3, 0.6, 2, 1.0), (0.5, 0.5, 0.8, 0.9, 4, 1.0)),
        'identical': _rows((0.21, 0.33, 0.55, 0.72, 2, 1.0), (0.21, 0.33, 0.55, 0.72, 9, 0.5)),
        'corner_tie': _rows((0.125, 0.125, 0.375, 0.375, 6, 1.0)),     # centre (0.25, 0.25) = a corner of four level-0 cells
        'forced_vs_ordinary': _rows(twin_of_prior, TINY),
    }


EDGE_NAMES = ('empty', 'whole_image', 'tiny', 'degenerate', 'identical', 'corner_tie', 'forced_vs_ordinary')
NAMES = ('A', 'A_mixup_ignored', 'B', 'small_k1', 'small_k3', 'small_k16') + EDGE_NAMES + ('edge_batch', 'A_max_gt_2')


@functools.lru_cache(None)
def case(name):
    topk, max_gt = 9, None
    if name in ('A', 'A_mixup_ignored', 'B'):
        size, ncls, targets, seed = cases._targets(name)
        pri, off = pyramid(size)
    elif name.startswith('small_k'):
        pri, off = small_pyramid()
        targets, topk = [SMALL_BOXES], int(name[len('small_k'):])
    elif name == 'A_max_gt_2':                      # more boxes than max_gt: only the first two of every image count
        pri, off = pyramid(300)
        targets, max_gt = cases._targets('A')[2], 2
    else:
        pri, off = pyramid(512)
        images = _edge_images()
        targets = [images[k] for k in EDGE_NAMES] if name == 'edge_batch' else [images[name]]
    if max_gt is None:
        max_gt = max([int(t.shape[0]) for t in targets] + [1])
    ref = atss_ref.match([t.numpy() for t in targets], pri.numpy(), off, topk, VAR, max_gt)
    return types.SimpleNamespace(name=name, targets=targets, priors=pri, off=off, topk=topk, max_gt=max_gt, ref=ref)


def packed(c, device):
    """The case's targets as ops.atss_match_packed reads them: truths [sum G,6], gt_off int32 [B+1] on `device`."""
    counts = [int(t.shape[0]) for t in c.targets]
    rows = [t for t in c.targets if t.shape[0]]
    truths = torch.cat(rows, 0) if rows else torch.zeros(1, 6)
    gt_off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    return truths.to(device).contiguous(), gt_off.to(device)
