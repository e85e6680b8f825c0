"""The device COCO evaluator without a device: the C ABI surface of ct_coco_match / ct_coco_accumulate (export, header,
binding, host-side argument errors before any launch) and the limits the header states against the host twin's."""
import ctypes as C
import os
import re
import subprocess

import pytest

from ctdet import _lib, evaluate

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, 'context-transformer_amd', 'lib', 'libctdet.so')
CT_ERR_INVALID = 1


def _define(header, name):
    return int(re.search(r'#define %s (\d+)' % name, header).group(1))


def test_library_exports_declares_and_binds_the_entry_points():
    assert os.path.exists(LIB), 'build the library first (context-transformer_amd/build.py)'
    r = subprocess.run(['nm', '-D', '--defined-only', LIB], capture_output=True, text=True)
    assert r.returncode == 0 and ' T ct_coco_match' in r.stdout and ' T ct_coco_accumulate' in r.stdout
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    assert 'int ct_coco_match(const float* out_dets, const int* out_count, int batch, int num_fg, int cap,' in header
    assert 'int ct_coco_accumulate(const long long* rec_key, const unsigned long long* rec_matched,' in header
    assert _define(header, 'CT_COCO_MAX_GT_PER_SEGMENT') == evaluate.COCO_MAX_GT_PER_SEGMENT >= 128
    assert _define(header, 'CT_COCO_MAX_CATEGORIES') == evaluate.COCO_MAX_CATEGORIES >= 80
    assert _define(header, 'CT_COCO_MAX_IMAGES') == evaluate.COCO_MAX_IMAGES >= 40504
    assert _define(header, 'CT_COCO_MAX_DETS') == 100 and _define(header, 'CT_COCO_ACC_CHUNK') == 512
    assert len(_lib.SIGNATURES['ct_coco_match'][1]) == 25 and len(_lib.SIGNATURES['ct_coco_accumulate'][1]) == 19
    assert _lib.SIGNATURES['ct_coco_accumulate'][1][4] is C.c_longlong
    assert _lib.lib().ct_coco_match.restype is C.c_int and _lib.lib().ct_coco_accumulate.restype is C.c_int
    src = open(os.path.join(REPO, 'context-transformer_amd', 'build.py')).read()
    assert "'ct_coco_eval.hip': ['-ffp-contract=off']" in src


def _match_args(**over):
    """A valid argument list of ct_coco_match on host memory (never launched: every case below breaks one rule)."""
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    a = dict(out_dets=p, out_count=p, batch=2, num_fg=3, cap=8, image_index=p, image_rank=p, num_images=14, gt_boxes=p,
             gt_area=p, gt_iscrowd=p, gt_label=p, gt_off=p, num_gt=4, cat_rank=p, iou_thrs=p, num_iou_thrs=10,
             area_rng=p, num_area_rng=4, rec_key=p, rec_matched=p, rec_ignored=p, per_image_cap=16, status=p,
             stream=None)
    a.update(over)
    return list(a.values()), buf


def _acc_args(**over):
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    a = dict(rec_key=p, rec_matched=p, rec_ignored=p, order=None, num_records=16, cat_off=p, npig=p, num_categories=5,
             num_area_rng=4, max_dets=p, num_max_dets=3, num_iou_thrs=10, rec_thrs=p, num_rec_thrs=101, precision=p,
             recall=p, scores=p, status=p, stream=None)
    a.update(over)
    return list(a.values()), buf


@pytest.mark.parametrize('over', [
    dict(batch=0), dict(batch=-1), dict(num_fg=0), dict(cap=-8), dict(num_images=0), dict(num_gt=-1),
    dict(per_image_cap=0), dict(out_dets=None), dict(out_count=None), dict(image_index=None), dict(gt_boxes=None),
    dict(gt_area=None), dict(gt_iscrowd=None), dict(gt_label=None), dict(gt_off=None), dict(cat_rank=None),
    dict(iou_thrs=None), dict(area_rng=None), dict(rec_key=None), dict(rec_matched=None), dict(rec_ignored=None),
    dict(status=None),
    dict(num_fg=128), dict(cap=4097), dict(num_images=(1 << 17) + 1),   # beyond the key's bit fields
    dict(num_iou_thrs=0), dict(num_iou_thrs=17), dict(num_area_rng=0), dict(num_area_rng=5)])
def test_coco_match_refuses_bad_arguments_before_any_launch(over):
    args, keep = _match_args(**over)
    assert _lib.lib().ct_coco_match(*args) == CT_ERR_INVALID, over
    assert b'ct_coco_match' in _lib.lib().ct_last_error_string()


@pytest.mark.parametrize('over', [
    dict(num_records=-1), dict(num_categories=0), dict(num_categories=128), dict(num_area_rng=0), dict(num_area_rng=5),
    dict(num_max_dets=0), dict(num_max_dets=5), dict(num_iou_thrs=0), dict(num_iou_thrs=17), dict(num_rec_thrs=0),
    dict(num_rec_thrs=129), dict(rec_key=None), dict(rec_matched=None), dict(rec_ignored=None), dict(cat_off=None),
    dict(npig=None), dict(max_dets=None), dict(rec_thrs=None), dict(precision=None), dict(recall=None),
    dict(scores=None), dict(status=None)])
def test_coco_accumulate_refuses_bad_arguments_before_any_launch(over):
    args, keep = _acc_args(**over)
    assert _lib.lib().ct_coco_accumulate(*args) == CT_ERR_INVALID, over
    assert b'ct_coco_accumulate' in _lib.lib().ct_last_error_string()
