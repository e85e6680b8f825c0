"""Cases shared by test_coco_eval_cpu.py and test_gpu_coco_eval.py: the golden of the reference's own COCOeval
(tests/golden/coco_eval.npz, tools/gen_coco_golden.py) and a seeded random data set, both in the layout the
post-processing leaves (out_dets [N,T,cap,5], out_count [N,T]) next to the COCO-format ground truth."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coco_eval.npz')


def pack_rows(rows, n, t, cap):
    """{(position, class index): float32 [k,5]} -> (out_dets [n,t,cap,5], out_count [n,t])."""
    dets, count = np.zeros((n, t, cap, 5), np.float32), np.zeros((n, t), np.int32)
    for (i, j), v in rows.items():
        dets[i, j - 1, :len(v)], count[i, j - 1] = v, len(v)
    return dets, count


def all_boxes_of(dets, count):
    """(out_dets, out_count) -> the reference's all_boxes[cls][img] (class 0 = background: empty lists)."""
    n, t = count.shape
    return [[[] for _ in range(n)]] + [[dets[i, j, :count[i, j]].copy() for i in range(n)] for j in range(t)]


def golden_case():
    z = np.load(GOLDEN)
    count = z['det_count']
    n, t = count.shape
    cap = int(z['cap'])
    dets = np.zeros((n, t, cap, 5), np.float32)
    at = 0
    for i in range(n):
        for j in range(t):
            dets[i, j, :count[i, j]] = z['det_rows'][at:at + count[i, j]]
            at += count[i, j]
    assert at == len(z['det_rows'])
    return dict(gt=json.loads(str(z['gt_json'])), image_ids=z['image_ids'].tolist(),
                category_ids=z['category_ids'].tolist(), dets=dets, count=count, never_fed=int(z['never_fed']),
                precision=z['precision'], recall=z['recall'], scores=z['scores'], stats=z['stats'])


def random_case(seed=11, n=150, ncat=12, cap=40):
    """About 150 images x 12 categories, up to `cap` rows per segment: boxes on a half-pixel grid and scores at two
    decimals (exact IoU ties with the thresholds and equal scores do occur), crowds, annotation areas below w*h, images
    without boxes, images that are never fed, segments stored unsorted."""
    rng = np.random.RandomState(seed)
    cat_ids = sorted(rng.choice(np.arange(1, 91), ncat, replace=False).tolist())
    category_ids = [0] + [cat_ids[i] for i in rng.permutation(ncat)]
    image_ids = rng.choice(np.arange(1, 100000), n, replace=False).tolist()
    anns, rows = [], {}
    fed = rng.rand(n) > 0.05
    for pos, img in enumerate(image_ids):
        for cls in range(1, ncat + 1):
            if rng.rand() < 0.6:
                continue
            boxes = []
            for _ in range(rng.randint(0, 5) if rng.rand() < 0.9 else 0):
                side = [rng.uniform(4, 40), rng.uniform(25, 110), rng.uniform(80, 300)][rng.randint(3)]
                w, h = np.round(side * rng.uniform(0.6, 1.4, 2) * 2) / 2
                x, y = np.round(rng.uniform(0, 500, 2) * 2) / 2
                crowd = int(rng.rand() < 0.12)
                area = float(w * h) if rng.rand() < 0.3 else float(np.round(w * h * rng.uniform(0.5, 1), 1))
                anns.append({'id': len(anns) + 1, 'image_id': img, 'category_id': category_ids[cls],
                             'bbox': [float(x), float(y), float(w), float(h)], 'area': area, 'iscrowd': crowd})
                boxes.append((x, y, w, h))
            if not fed[pos]:
                continue
            seg = []
            for (x, y, w, h) in boxes:
                for _ in range(rng.randint(0, 4)):
                    j = np.round(rng.uniform(-0.15, 0.15, 4) * [w, h, w, h] * 2) / 2
                    seg.append([x + j[0], y + j[1], x + j[0] + w + j[2] - 1, y + j[1] + h + j[3] - 1,
                                rng.randint(1, 100) / 100.])
            for _ in range(rng.randint(0, 6)):
                x, y = np.round(rng.uniform(0, 500, 2) * 2) / 2
                w, h = np.round(rng.uniform(4, 200, 2) * 2) / 2
                seg.append([x, y, x + w - 1, y + h - 1, rng.randint(1, 60) / 100.])
            if seg:
                seg = np.asarray(seg, dtype=np.float32)[:cap]
                rows[(pos, cls)] = seg[rng.permutation(len(seg))]
    dets, count = pack_rows(rows, n, ncat, cap)
    gt = {'images': [{'id': i} for i in image_ids], 'annotations': anns,
          'categories': [{'id': c, 'name': 'cat%d' % c} for c in cat_ids]}
    return dict(gt=gt, image_ids=image_ids, category_ids=category_ids, dets=dets, count=count,
                fed=np.flatnonzero(fed).tolist())
