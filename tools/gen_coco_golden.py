#!/usr/bin/env python3
"""Generate tests/golden/coco_eval.npz by running the REFERENCE's own COCO / loadRes / COCOeval(..., 'bbox').

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_coco_golden.py --reference <checkout of Ze-Yang/Context-Transformer>
    ... --check      writes nothing and compares what it computed with the arrays of the committed file

The reference's utils/pycocotools is copied into a temporary package (maskApi.c / maskApi.h to ../common beside it,
where the `distutils: sources` line of _mask.pyx points), cythonized there and imported from there; none of its text
is edited and nothing of it is kept: only the inputs and the arrays it computed are stored.  np.float is aliased for the
duration of the call (cocoeval.py:378) and empty modules stand in for matplotlib where it is absent (coco.py:49-51
imports it for drawing only).

The case: 14 images (ids neither contiguous nor ascending in data set order) x 5 categories (ids 3 7 18 44 90, class
order different from id order), ground-truth ids from 1, holding every place the kernels can go wrong -- see build_case.
"""
import argparse
import contextlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'coco_eval.npz')
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, 'context-transformer_amd'))

IMAGE_IDS = [139, 42, 785, 8021, 57, 1000, 724, 3501, 13, 632, 9999, 2153, 400, 87]     # data set order
CATEGORIES = [(3, 'car'), (7, 'train'), (18, 'dog'), (44, 'bottle'), (90, 'toothbrush')]
CATEGORY_IDS = [0, 18, 3, 90, 7, 44]            # class index -> COCO id; 0 = background
NEVER_FED, NO_BOXES, MANY_ROWS = 8021, 724, 57  # image ids
CAP = 136


def r2(v):
    return float(np.round(v, 2))


def build_case(seed):
    """-> (gt dict, rows {(position, class index): float32 [k,5]}).

    class 1 (id 18) and 2 (id 3)  random boxes of all sizes with annotation area = 0.55 .. 1 of w*h, some crowds,
                                  detections = jittered boxes (several per crowd) + false positives, scores at two
                                  decimals (ties inside segments and across images); the hand-made situations below
    class 3 (id 90)               crowd boxes only (npig == 0 -> -1), with detections
    class 4 (id 7)                detections and no boxes anywhere
    class 5 (id 44)               boxes and no detections (recall 0, precision 0)
    image 724 has no boxes, image 8021 is never fed (boxes, no detections), image 57 has a segment of more
    than 130 rows, 130 of them stored worst first."""
    rng = np.random.RandomState(seed)
    anns, rows = [], {}

    def add_gt(img, cat, box, area=None, crowd=0):
        box = [r2(v) for v in box]
        anns.append({'id': len(anns) + 1, 'image_id': img, 'category_id': cat, 'bbox': box,
                     'area': r2(box[2] * box[3]) if area is None else float(area), 'iscrowd': int(crowd)})

    def add_det(pos, cls, x, y, w, h, s):
        rows.setdefault((pos, cls), []).append([r2(x), r2(y), r2(x + w - 1), r2(y + h - 1), r2(s)])

    sizes = [(6, 30), (30, 34), (33, 95), (90, 100), (97, 300)]         # straddling 32 and 96 on both sides
    for pos, img in enumerate(IMAGE_IDS):
        if img == NO_BOXES:
            for cls in (1, 2, 3, 4):
                for _ in range(4):
                    add_det(pos, cls, rng.uniform(0, 300), rng.uniform(0, 300), rng.uniform(5, 150),
                            rng.uniform(5, 150), rng.randint(1, 100) / 100.)
            continue
        for cls in (1, 2):
            cat = CATEGORY_IDS[cls]
            for _ in range(rng.randint(2, 7)):
                lo, hi = sizes[rng.randint(len(sizes))]
                w, h = rng.uniform(lo, hi), rng.uniform(lo, hi)
                x, y = rng.uniform(0, 400), rng.uniform(0, 400)
                crowd = rng.rand() < 0.15
                add_gt(img, cat, [x, y, w, h], area=r2(w * h * rng.uniform(0.55, 1.0)), crowd=crowd)
                if img == NEVER_FED:
                    continue
                for _ in range(rng.randint(2, 5) if crowd else rng.randint(0, 3)):
                    j = rng.uniform(-0.12, 0.12, 4) * [w, h, w, h]
                    add_det(pos, cls, x + j[0], y + j[1], w + j[2], h + j[3], rng.randint(20, 100) / 100.)
            if img != NEVER_FED:
                for _ in range(rng.randint(0, 4)):
                    lo, hi = sizes[rng.randint(len(sizes))]
                    add_det(pos, cls, rng.uniform(0, 400), rng.uniform(0, 400), rng.uniform(lo, hi),
                            rng.uniform(lo, hi), rng.randint(1, 70) / 100.)
        # class 3: crowds only; class 4: detections only; class 5: boxes only
        if pos % 3 == 0:
            x, y, w, h = rng.uniform(0, 300), rng.uniform(0, 300), rng.uniform(40, 200), rng.uniform(40, 200)
            add_gt(img, CATEGORY_IDS[3], [x, y, w, h], crowd=1)
            if img != NEVER_FED:
                for _ in range(3):
                    add_det(pos, 3, x + rng.uniform(0, 20), y + rng.uniform(0, 20), w * 0.5, h * 0.5,
                            rng.randint(1, 100) / 100.)
        if pos % 4 == 1 and img != NEVER_FED:
            for _ in range(3):
                add_det(pos, 4, rng.uniform(0, 300), rng.uniform(0, 300), rng.uniform(5, 150), rng.uniform(5, 150),
                        rng.randint(1, 100) / 100.)
        if pos % 2 == 0:
            lo, hi = sizes[pos % len(sizes)]
            add_gt(img, CATEGORY_IDS[5], [rng.uniform(0, 300), rng.uniform(0, 300), rng.uniform(lo, hi),
                                          rng.uniform(lo, hi)])

    # ---- hand-made situations, far from the random boxes (x >= 1000) ----
    p0, i0 = 0, IMAGE_IDS[0]
    # IoU exactly 0.5: [0,0,10,10] against [0,0,10,20]; matches at t = 0.5 (`ious < iou` continues), not at 0.55
    add_gt(i0, 18, [1000, 0, 10, 20])
    add_det(p0, 1, 1000, 0, 10, 10, 0.93)
    # annotation areas exactly 32^2 and 96^2 (both ends inclusive: the box counts in two ranges), boxes of another size
    add_gt(i0, 18, [1100, 0, 40, 40], area=32 ** 2)
    add_det(p0, 1, 1101, 1, 40, 40, 0.88)
    add_gt(i0, 18, [1200, 0, 120, 120], area=96 ** 2)
    add_det(p0, 1, 1202, 2, 120, 120, 0.88)
    # detection areas exactly on the bounds, unmatched: ignored in no range that includes the bound
    add_det(p0, 1, 1400, 300, 32, 32, 0.5)
    add_det(p0, 1, 1500, 300, 96, 96, 0.5)
    # a detection that prefers an ignored box only because the regular one is taken: R regular, C crowd over it
    p1, i1 = 1, IMAGE_IDS[1]
    add_gt(i1, 3, [1000, 500, 100, 100])
    add_gt(i1, 3, [1000, 500, 110, 110], crowd=1)
    add_det(p1, 2, 1000, 500, 100, 100, 0.99)           # takes R
    add_det(p1, 2, 1002, 502, 100, 100, 0.98)           # R is taken -> the crowd
    add_det(p1, 2, 1004, 504, 100, 100, 0.98)           # and again (a crowd matches any number), equal score
    # the same for a box ignored by its area only: it can be taken once
    add_gt(i1, 3, [1300, 500, 50, 50])
    add_gt(i1, 3, [1300, 500, 52, 52], area=20000.)
    add_det(p1, 2, 1300, 500, 50, 50, 0.97)
    add_det(p1, 2, 1301, 501, 50, 50, 0.96)
    add_det(p1, 2, 1301, 500, 50, 50, 0.95)
    # one segment with more than 100 rows, in ascending score order with ties: only the best 100 count
    pm = IMAGE_IDS.index(MANY_ROWS)
    for k in range(130):
        add_det(pm, 2, 2000 + 7 * (k % 13), 20 * (k // 13), 30 + k % 5, 30 + k % 7, 0.02 + 0.01 * (k // 2))
    add_gt(MANY_ROWS, 3, [2000, 0, 32, 34])
    add_gt(MANY_ROWS, 3, [2035, 160, 31, 33])

    gt = {'images': [{'id': i, 'width': 4000, 'height': 600, 'file_name': '%012d.jpg' % i} for i in IMAGE_IDS],
          'annotations': anns,
          'categories': [{'id': c, 'name': n, 'supercategory': 'thing'} for c, n in CATEGORIES]}
    rows = {k: np.asarray(v, dtype=np.float32) for k, v in rows.items()}
    assert max(len(v) for v in rows.values()) <= CAP
    return gt, rows


def import_reference_pycocotools(ref):
    """The reference's pycocotools, built in and imported from a temporary directory -> (COCO, COCOeval, tmp dir)."""
    src = os.path.join(ref, 'utils', 'pycocotools')
    tmp = tempfile.mkdtemp(prefix='ctref_coco_')
    pkg = os.path.join(tmp, 'refcoco', 'pycocotools')
    os.makedirs(pkg)
    os.makedirs(os.path.join(tmp, 'refcoco', 'common'))
    for f in ('__init__.py', 'coco.py', 'cocoeval.py', 'mask.py', '_mask.pyx'):
        shutil.copy(os.path.join(src, f), os.path.join(pkg, f))
    for f in ('maskApi.c', 'maskApi.h'):
        shutil.copy(os.path.join(src, f), os.path.join(tmp, 'refcoco', 'common', f))
    with open(os.path.join(pkg, 'setup.py'), 'w') as f:
        f.write("from setuptools import setup, Extension\nfrom Cython.Build import cythonize\nimport numpy\n"
                "setup(ext_modules=cythonize([Extension('_mask', ['_mask.pyx'], include_dirs=[numpy.get_include(), "
                "'../common'], extra_compile_args=['-std=c99', '-w'])], language_level=2))\n")
    subprocess.check_call([sys.executable, 'setup.py', 'build_ext', '--inplace'], cwd=pkg,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    try:
        import matplotlib.pyplot    # noqa: F401
    except Exception:
        for name in ('matplotlib', 'matplotlib.pyplot', 'matplotlib.collections', 'matplotlib.patches'):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules['matplotlib.collections'].PatchCollection = None
        sys.modules['matplotlib.patches'].Polygon = None
    sys.path.insert(0, os.path.join(tmp, 'refcoco'))
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    return COCO, COCOeval, tmp


def run_reference(COCO, COCOeval, gt, results, tmp):
    ann_file = os.path.join(tmp, 'instances.json')
    with open(ann_file, 'w') as f:
        json.dump(gt, f)
    had = hasattr(np, 'float')
    if not had:
        np.float = float
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            coco_gt = COCO(ann_file)
            coco_dt = coco_gt.loadRes(results)
            ev = COCOeval(coco_gt, coco_dt, 'bbox')
            ev.evaluate()
            ev.accumulate()
            ev.summarize()
    finally:
        if not had:
            del np.float
    return ev.eval['precision'], ev.eval['recall'], ev.eval['scores'], np.asarray(ev.stats, dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference repository')
    ap.add_argument('--seed', type=int, default=2017)
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--check', action='store_true', help='write nothing: compare with the arrays already in --out')
    a = ap.parse_args()
    from ctdet import evaluate

    gt, rows = build_case(a.seed)
    n, t = len(IMAGE_IDS), len(CATEGORY_IDS) - 1
    all_boxes = [[rows.get((i, j), np.zeros((0, 5), np.float32)) for i in range(n)] for j in range(t + 1)]
    results = evaluate.coco_results(all_boxes, IMAGE_IDS, CATEGORY_IDS)
    COCO, COCOeval, tmp = import_reference_pycocotools(a.reference)
    try:
        precision, recall, scores, stats = run_reference(COCO, COCOeval, json.loads(json.dumps(gt)), results, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    # the case must exercise -1, 0 and values strictly inside (0, 1) in every area range
    for name, arr, axis in (('precision', precision, 3), ('recall', recall, 2)):
        for ai in range(arr.shape[axis]):
            s = np.take(arr, ai, axis=axis)
            assert (s == -1).any() and (s == 0).any() and ((s > 0) & (s < 1)).any(), (name, ai)
    count = np.zeros((n, t), dtype=np.int32)
    for (i, j), v in rows.items():
        count[i, j - 1] = len(v)
    flat = [rows[(i, j)] for i in range(n) for j in range(1, t + 1) if (i, j) in rows]
    store = dict(gt_json=np.array(json.dumps(gt, sort_keys=True)), image_ids=np.asarray(IMAGE_IDS, dtype=np.int64),
                 category_ids=np.asarray(CATEGORY_IDS, dtype=np.int64), det_rows=np.concatenate(flat),
                 det_count=count, never_fed=np.int64(IMAGE_IDS.index(NEVER_FED)), cap=np.int64(CAP),
                 precision=precision, recall=recall, scores=scores, stats=stats)
    if a.check:
        old = np.load(a.out)
        differ = [k for k in store if k not in old.files or not np.array_equal(old[k], store[k])]
        differ += [k for k in old.files if k not in store]
        print('%s: %s' % (os.path.basename(a.out), 'every array regenerates identically' if not differ
                          else 'DIFFERS in %s' % differ))
        sys.exit(1 if differ else 0)
    np.savez_compressed(a.out, **store)
    print('%s  %.1f KB  stats %s' % (os.path.basename(a.out), os.path.getsize(a.out) / 1024, np.round(stats, 4)))
    packed = evaluate.pack_coco_ground_truth(gt, CATEGORY_IDS, IMAGE_IDS)
    mine = evaluate.coco_eval_arrays(all_boxes, packed)
    print('host twin equal: precision %s recall %s scores %s' % tuple(
        np.array_equal(x, y) for x, y in zip(mine, (precision, recall, scores))))


if __name__ == '__main__':
    main()
