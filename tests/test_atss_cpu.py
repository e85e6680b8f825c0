"""The ATSS matcher (matcher='atss', ct_atss_match_batched) as far as it can be checked without a GPU: the numpy twin against
a second, float64 brute-force formulation and against numbers worked out by hand, PriorBox.level_offsets(), the criterion's
arguments and environment, the refusals of the C entry (all before any HIP call) and the header."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from ctdet import _lib, ops
from layers.functions import PriorBox
from layers.modules.multibox_loss_combined import MultiBoxLoss_combined
import data as cfgs

import atss_cases
import atss_ref


def _crit(**kw):
    return MultiBoxLoss_combined(21, 0.5, True, 0, True, 3, 0.5, False, **kw)


# ------------------------------------------------------------------------------------ 1: the twin
def brute_force(targets, priors, off, topk, max_gt):
    """The rule once more, in float64 and in another shape: all claims of an image are listed first (one lexsort per level
    for the candidates, numpy's mean / std for the threshold) and the conflicts are settled by one sort over the list.
    -> per image: owner [P] (box index or -1), forced flags, stats rows (n, positives, forced), thresholds."""
    pri = priors.astype(np.float64)
    px1, py1 = pri[:, 0] - pri[:, 2] / 2, pri[:, 1] - pri[:, 3] / 2
    px2, py2 = pri[:, 0] + pri[:, 2] / 2, pri[:, 1] + pri[:, 3] / 2
    index = np.arange(len(pri))
    out = []
    for t in targets:
        t = np.asarray(t, np.float64).reshape(-1, 6)
        claims, stats = [], np.zeros((max_gt, 4))
        for g, (x1, y1, x2, y2) in enumerate(t[:max_gt, :4]):
            if not (x2 > x1 and y2 > y1):
                continue
            d = (pri[:, 0] - (x1 + x2) / 2) ** 2 + (pri[:, 1] - (y1 + y2) / 2) ** 2
            cand = np.concatenate([lo + np.lexsort((index[lo:hi], d[lo:hi]))[:topk] for lo, hi in zip(off[:-1], off[1:])])
            iw = np.clip(np.minimum(x2, px2[cand]) - np.maximum(x1, px1[cand]), 0, None)
            ih = np.clip(np.minimum(y2, py2[cand]) - np.maximum(y1, py1[cand]), 0, None)
            iou = iw * ih / ((x2 - x1) * (y2 - y1) + pri[cand, 2] * pri[cand, 3] - iw * ih)
            thr = iou.mean() + (iou.std(ddof=1) if len(cand) > 1 else 0.0)
            inside = (x1 < pri[cand, 0]) & (pri[cand, 0] < x2) & (y1 < pri[cand, 1]) & (pri[cand, 1] < y2)
            pos = np.nonzero((iou >= thr) & inside)[0]
            forced = len(pos) == 0
            if forced:
                pos = np.array([int(np.argmax(iou))])
            stats[g] = (thr, len(cand), len(pos), forced)
            claims += [(not forced, -iou[k], g, int(cand[k])) for k in pos]
        owner = np.full(len(pri), -1)
        for _, _, g, p in sorted(claims, reverse=True):      # the worst claim first, the winning one written last
            owner[p] = g
        out.append((owner, stats))
    return out


@pytest.mark.parametrize('name', atss_cases.NAMES)
def test_twin_against_the_float64_brute_force(name):
    c = atss_cases.case(name)
    ref = c.ref
    margins = [m for image in ref.margins for m in image]
    print(name, 'boxes', len(margins), 'smallest margin %.3g' % min(margins + [math.inf]),
          'positives', [int((ref.conf_t[b, :, 0] != 0).sum()) for b in range(len(c.targets))])
    assert all(m > 1e-5 for m in margins), margins         # no decision of the case hangs on the last bits of an IoU
    brute = brute_force([t.numpy() for t in c.targets], c.priors.numpy(), c.off, c.topk, c.max_gt)
    for b, (owner, stats) in enumerate(brute):
        t = c.targets[b].numpy()
        assert np.array_equal(ref.gt_stats[b][:, 1:], stats[:, 1:].astype(np.float32))
        assert np.abs(ref.gt_stats[b][:, 0] - stats[:, 0]).max() < 1e-6
        got = owner >= 0
        assert np.array_equal(got, (ref.conf_t[b, :, 0] != 0) | (ref.overlap[b] > 0))
        assert np.array_equal(ref.conf_t[b][got], t[owner[got]][:, 4:6])
        labels = np.zeros(len(owner), np.float32)
        labels[got] = t[owner[got], 4]
        assert np.array_equal(ref.obj_t[b], labels != 0)
        # every other prior: zeros and (0, 1), exactly
        assert not ref.loc_t[b][~got].any() and not ref.overlap[b][~got].any() and not ref.obj_t[b][~got].any()
        assert (ref.conf_t[b][~got] == (0, 1)).all()
        # loc_t of the assigned priors against utils/box_utils.py::encode in float64
        if got.any():
            m, p = t[owner[got]].astype(np.float64), c.priors.numpy()[got].astype(np.float64)
            want = np.stack([((m[:, 0] + m[:, 2]) / 2 - p[:, 0]) / (0.1 * p[:, 2]), ((m[:, 1] + m[:, 3]) / 2 - p[:, 1]) / (0.1 * p[:, 3]),
                             np.log((m[:, 2] - m[:, 0]) / p[:, 2]) / 0.2, np.log((m[:, 3] - m[:, 1]) / p[:, 3]) / 0.2], 1)
            assert np.allclose(ref.loc_t[b][got], want, rtol=1e-5, atol=2e-5)
        assert np.isfinite(ref.loc_t[b]).all()


def test_positives_of_the_loss_cases():
    """The counts the matcher was designed around: every box of the synthetic targets gets 7-12 positives before conflicts."""
    for name, want in (('A', [19, 38, 37]), ('A_mixup_ignored', [19, 38, 37]), ('B', [60, 73])):
        ref = atss_cases.case(name).ref
        assert [int((ref.conf_t[b, :, 0] != 0).sum()) for b in range(len(want))] == want, name
        live = ref.gt_stats[..., 1] > 0
        assert set(ref.gt_stats[..., 1][live]) == ({49.0} if name != 'B' else {58.0})
        assert 7 <= ref.gt_stats[..., 2][live].min() and ref.gt_stats[..., 2][live].max() <= 12
        assert not ref.gt_stats[..., 3].any()
    ref = atss_cases.case('A_mixup_ignored').ref
    assert (ref.conf_t[..., 0] == -1).any() and set(np.unique(ref.conf_t[..., 1])) == {np.float32(0.37), np.float32(0.63), 1.0}
    assert np.array_equal(ref.obj_t, ref.conf_t[..., 0] != 0)


def test_small_pyramid_by_hand():
    """Box 0 = (1/16, 1/16, 7/16, 7/16), centre (1/4, 1/4).  Level 0: the four cells around that corner tie at d = 1/32, the
    lowest index is prior 0 = (0, 0, 1/4, 1/4): IoU = (3/16)^2 / (9/64 + 1/16 - 9/256) = 9/43.  Level 1: prior 32 = (0, 0, 1/2,
    1/2), d = 0, IoU = (9/64) / (1/4) = 9/16.  Level 2: prior 40 = (1/16 .. 15/16)^2, IoU = (9/64) / (49/64) = 9/49.
    mean = 0.31849, s = 0.21171, t = 0.53020: prior 32 alone is positive -- and box 3, which IS prior 32 (IoU 1), takes it."""
    c = atss_cases.case('small_k1')
    t = c.targets[0].numpy()
    b0 = atss_ref.box_candidates(t[0], c.priors.numpy(), c.off, 1)
    assert list(b0.idx) == [0, 32, 40]
    assert np.allclose(b0.iou, [9 / 43, 9 / 16, 9 / 49], rtol=1e-6)
    ious = np.array([9 / 43, 9 / 16, 9 / 49])
    assert abs(float(b0.t) - (ious.mean() + ious.std(ddof=1))) < 1e-6 and abs(float(b0.t) - 0.53020) < 1e-5
    assert list(b0.positive) == [False, True, False] and b0.forced == -1
    b3 = atss_ref.box_candidates(t[3], c.priors.numpy(), c.off, 1)
    assert 32 in list(b3.idx) and float(b3.iou[list(b3.idx).index(32)]) == 1.0
    ref = c.ref
    assert tuple(ref.conf_t[0, 32]) == (4.0, 1.0) and ref.overlap[0, 32] == 1.0
    assert not (ref.conf_t[0, :, 0] == 1).any()            # box 0 lost its one positive under rule 7: it ends with no prior
    assert (ref.conf_t[0, :, 0] == 3).any() and set(ref.conf_t[0][ref.conf_t[0, :, 0] == 3][:, 1]) == {0.5}
    # the candidate counts: min(topk, n_l) per level
    for k, n in ((1, 3), (3, 7), (16, 16 + 8 + 1)):
        assert set(atss_cases.case('small_k%d' % k).ref.gt_stats[0][:, 1]) == {float(n)}
    # ties go to the lower index and the order is level-major, then (d, index): box 0 at topk = 3
    assert list(atss_ref.box_candidates(t[0], c.priors.numpy(), c.off, 3).idx) == [0, 1, 2, 32, 33, 34, 40]


def test_edge_cases_on_the_twin():
    pri, off = atss_cases.pyramid(512)
    ref = atss_cases.case('empty').ref
    assert not ref.loc_t.any() and not ref.obj_t.any() and (ref.conf_t == (0, 1)).all() and not ref.gt_stats.any()
    ref = atss_cases.case('tiny').ref
    assert tuple(ref.gt_stats[0, 0, 1:]) == (58.0, 1.0, 1.0) and int((ref.conf_t[0, :, 0] == 5).sum()) == 1
    x1, y1, x2, y2 = atss_cases.TINY[:4]
    p = pri.numpy()
    assert not ((x1 < p[:, 0]) & (p[:, 0] < x2) & (y1 < p[:, 1]) & (p[:, 1] < y2)).any()
    ref = atss_cases.case('degenerate').ref
    assert not ref.gt_stats[0, 0].any() and ref.gt_stats[0, 1, 1] == 58 and set(np.unique(ref.conf_t[0, :, 0])) == {0.0, 4.0}
    ref = atss_cases.case('identical').ref
    assert np.array_equal(ref.gt_stats[0, 0], ref.gt_stats[0, 1]) and ref.gt_stats[0, 0, 2] >= 2
    assert set(np.unique(ref.conf_t[0, :, 0])) == {0.0, 2.0}               # the lower index wins every prior
    c = atss_cases.case('corner_tie')
    box = atss_ref.box_candidates(c.targets[0].numpy()[0], p, off, 9)
    # cells (15,15), (15,16), (16,15), (16,16) tie exactly; 6 priors per cell: the first cell's six and three of the second
    first = (15 * 64 + 15) * 6
    assert list(box.idx[:9]) == list(range(first, first + 9))
    d = (p[box.idx[:9], 0] - np.float32(0.25)) ** 2 + (p[box.idx[:9], 1] - np.float32(0.25)) ** 2
    assert len(set(d)) == 1
    corners = np.array([(i * 64 + j) * 6 for i in (15, 16) for j in (15, 16)])
    assert len(set((p[corners, 0] - np.float32(0.25)) ** 2 + (p[corners, 1] - np.float32(0.25)) ** 2)) == 1
    c = atss_cases.case('forced_vs_ordinary')
    t = c.targets[0].numpy()
    big, tiny = (atss_ref.box_candidates(t[g], p, off, 9) for g in (0, 1))
    shared = int(tiny.idx[tiny.forced])
    k = list(big.idx).index(shared)
    assert tiny.forced >= 0 and big.forced < 0 and big.positive[k] and big.iou[k] > tiny.iou[tiny.forced]
    assert tuple(c.ref.conf_t[0, shared]) == (5.0, 1.0)                     # the forced claim wins although its IoU is smaller
    assert c.ref.overlap[0, shared] == tiny.iou[tiny.forced] and (c.ref.conf_t[0, :, 0] == 7).any()
    ref, full = atss_cases.case('A_max_gt_2').ref, atss_cases.case('A').ref
    assert ref.gt_stats.shape == (3, 2, 4) and np.array_equal(ref.gt_stats, full.gt_stats[:, :2])
    for b, t in enumerate(atss_cases.case('A').targets):
        assert set(np.unique(ref.conf_t[b, :, 0])) <= {0.0} | set(t[:2, 4].tolist())
    assert not np.array_equal(ref.conf_t, full.conf_t)
    # the whole batch is its images side by side
    ref = atss_cases.case('edge_batch').ref
    for b, name in enumerate(atss_cases.EDGE_NAMES):
        one = atss_cases.case(name).ref
        for key in ('loc_t', 'conf_t', 'obj_t', 'overlap'):
            assert np.array_equal(getattr(ref, key)[b], getattr(one, key)[0]), (name, key)
        assert np.array_equal(ref.gt_stats[b, :one.gt_stats.shape[1]], one.gt_stats[0])


# ------------------------------------------------------------------------------------ 2: level offsets
def test_level_offsets_of_every_config():
    configs = [v for k, v in sorted(vars(cfgs).items()) if isinstance(v, dict) and 'feature_maps' in v]
    assert len(configs) == 7
    for cfg in configs:
        pb = PriorBox(cfg)
        off = pb.level_offsets()
        assert off[0] == 0 and off[-1] == pb.forward().shape[0] and len(off) == len(cfg['feature_maps']) + 1
        assert all(a < b for a, b in zip(off, off[1:]))
    assert PriorBox(cfgs.VOC_300).level_offsets() == [0, 8664, 10830, 11430, 11580, 11616, 11620]
    assert PriorBox(cfgs.VOC_512).level_offsets()[-2:] == [32752, 32756]


# ------------------------------------------------------------------------------------ 3: the criterion's switches
ENV = ('CTDET_MATCHER', 'CTDET_ATSS_TOPK')


def test_default_is_ssd_and_the_environment_is_honoured(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    crit = _crit()
    assert (crit.matcher, crit.atss_topk, crit.level_offsets) == ('ssd', 9, None)
    monkeypatch.setenv('CTDET_MATCHER', '')
    monkeypatch.setenv('CTDET_ATSS_TOPK', '')
    crit = _crit()
    assert (crit.matcher, crit.atss_topk) == ('ssd', 9)
    monkeypatch.setenv('CTDET_MATCHER', 'atss')
    monkeypatch.setenv('CTDET_ATSS_TOPK', '5')
    crit = _crit(level_offsets=(0, 4, 6))
    assert (crit.matcher, crit.atss_topk, crit.level_offsets) == ('atss', 5, [0, 4, 6])
    crit = _crit(matcher='ssd', atss_topk=16)               # arguments win over the environment
    assert (crit.matcher, crit.atss_topk) == ('ssd', 16)
    assert _lib.MATCHERS == ('ssd', 'atss')
    # overlap_thresh is accepted and not read under atss
    assert MultiBoxLoss_combined(21, None, True, 0, True, 3, 0.5, False, matcher='atss').matcher == 'atss'


def test_bad_matchers_and_topk_raise_value_error(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for kw in (dict(matcher='ATSS'), dict(matcher='max_iou'), dict(atss_topk=0), dict(atss_topk=17), dict(atss_topk=-1),
               dict(atss_topk=2.5), dict(matcher='atss', atss_topk=0)):
        with pytest.raises(ValueError):
            _crit(**kw)
    for name, text in (('CTDET_MATCHER', 'Atss'), ('CTDET_ATSS_TOPK', '0'), ('CTDET_ATSS_TOPK', '17'),
                       ('CTDET_ATSS_TOPK', 'nine')):
        monkeypatch.setenv(name, text)
        with pytest.raises(ValueError):
            _crit()
        monkeypatch.delenv(name)
    for k in (1, 9, 16):
        assert _crit(matcher='atss', atss_topk=k).atss_topk == k


def test_match_refuses_missing_or_wrong_level_offsets():
    pri, off = atss_cases.small_pyramid()
    targets = [atss_cases.SMALL_BOXES]
    with pytest.raises(ValueError, match='level_offsets'):
        _crit(matcher='atss').match(pri, targets)
    with pytest.raises(ValueError, match='41'):
        _crit(matcher='atss', level_offsets=[0, 32, 40]).match(pri, targets)
    with pytest.raises(ValueError, match='41'):
        _crit(matcher='atss', level_offsets=off).match(pri[:40], targets)
    packed = ops.PackedTargets(torch.zeros(4, 6), torch.zeros(2, dtype=torch.int32), 4)
    with pytest.raises(ValueError, match='level_offsets'):
        _crit(matcher='atss').match(pri, packed)
    # with good offsets the call reaches the library's wrappers, which have no CPU form
    with pytest.raises(_lib.CtdetError, match='HIP device'):
        _crit(matcher='atss', level_offsets=off).match(pri, targets)
    with pytest.raises(ValueError):
        ops.check_atss(off, 17, 41)
    assert ops.check_atss(tuple(off), 9, 41) == (off, 9)


def test_ssd_constructs_and_matches_through_the_old_entry(monkeypatch):
    """matcher='ssd' makes the calls the criterion made before: ops.match_batched / ops.match_packed with the same arguments,
    and never the ATSS wrappers."""
    calls = []
    monkeypatch.setattr(ops, 'match_batched', lambda *a, **k: calls.append(('batched', a, k)) or (1, 2, 3))
    monkeypatch.setattr(ops, 'match_packed', lambda *a, **k: calls.append(('packed', a, k)) or (1, 2, 3))
    monkeypatch.setattr(ops, 'atss_match_batched', lambda *a, **k: pytest.fail('the ATSS matcher was called'))
    monkeypatch.setattr(ops, 'atss_match_packed', lambda *a, **k: pytest.fail('the ATSS matcher was called'))
    pri, off = atss_cases.small_pyramid()
    for crit in (_crit(), _crit(matcher='ssd', level_offsets=off, atss_topk=3)):
        assert tuple(crit.match(pri, [atss_cases.SMALL_BOXES])) == (1, 2, 3)
        kind, a, k = calls.pop()
        assert kind == 'batched' and len(a) == 4 and a[2:] == (0.5, [0.1, 0.2]) and not k and torch.equal(a[1], pri)
        truths, gt_off = torch.zeros(4, 6), torch.zeros(2, dtype=torch.int32)
        crit.match(pri, ops.PackedTargets(truths, gt_off, 4))
        kind, a, k = calls.pop()
        assert kind == 'packed' and a[0] is truths and a[1] is gt_off and a[2:4] == (1, 4) and a[5:] == (0.5, [0.1, 0.2]) and not k


# ------------------------------------------------------------------------------------ 4: the C entry and the header
def test_c_abi_refuses_bad_arguments_without_a_device():
    """Every check of ct_atss_match_batched comes before any HIP call: host pointers stand in for the tensors."""
    lib = _lib.lib()
    buf = (C.c_float * 64)()
    host = C.cast(buf, C.c_void_p)
    good_off = (C.c_int * 4)(0, 32, 40, 41)

    def call(truths=host, gt_off=host, batch=2, max_gt=4, priors=host, P=41, off=good_off, levels=3, topk=9, v0=0.1, v1=0.2,
             loc_t=host, conf_t=host, obj_t=host, ws=host, ws_bytes=1 << 20):
        return lib.ct_atss_match_batched(truths, gt_off, batch, max_gt, priors, P, off, levels, topk, v0, v1, loc_t, conf_t,
                                         obj_t, None, None, ws, ws_bytes, None)

    def offsets(*v):
        return (C.c_int * len(v))(*v)

    need = lib.ct_atss_workspace_bytes(2, 41, 4)
    assert need >= 2 * 41 * 8 and lib.ct_atss_workspace_bytes(1, 41, 4) < need
    bad = [(dict(truths=None), b'null'), (dict(gt_off=None), b'null'), (dict(priors=None), b'null'), (dict(off=None), b'null'),
           (dict(loc_t=None), b'null'), (dict(conf_t=None), b'null'), (dict(obj_t=None), b'null'), (dict(ws=None), b'null'),
           (dict(batch=0), b'batch=0'), (dict(P=0), b'num_priors=0'), (dict(max_gt=0), b'max_gt=0'),
           (dict(P=(1 << 30) + 1), b'num_priors='), (dict(batch=65536), b'batch=65536'),
           (dict(levels=0), b'num_levels=0'), (dict(levels=9, off=offsets(*range(10))), b'num_levels=9'),
           (dict(topk=0), b'topk=0'), (dict(topk=17), b'topk=17'),
           (dict(off=offsets(1, 32, 40, 41)), b'level_off'), (dict(off=offsets(0, 32, 32, 41)), b'level_off'),
           (dict(off=offsets(0, 40, 32, 41)), b'level_off'), (dict(off=offsets(0, 32, 40, 42)), b'level_off'),
           (dict(P=40), b'level_off'),
           (dict(v0=0.0), b'variances'), (dict(v1=-0.2), b'variances'), (dict(v0=math.nan), b'variances'),
           (dict(v1=math.inf), b'variances'), (dict(ws_bytes=need - 1), b'workspace')]
    for kw, word in bad:
        assert call(**kw) == 1, kw                          # CT_ERR_INVALID
        msg = lib.ct_last_error_string()
        assert b'ct_atss_match_batched' in msg and word in msg, (kw, msg)


def test_header_documents_the_rule_and_the_binding_matches():
    hdr = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    declared = set(re.findall(r'\b(ct_[a-z0-9_]+)\s*\(', hdr))
    for s in ('ct_atss_match_batched', 'ct_atss_workspace_bytes'):
        assert s in declared and s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES['ct_atss_match_batched'][1]) == 19
    assert 'CTDET_ABI_VERSION 1' in hdr and _lib.lib().ct_abi_version() == 1
    text = re.sub(r'\s*\n \*\s*', ' ', hdr)
    for words in ('ADAPTIVE TRAINING SAMPLE SELECTION', 'DEGENERATE BOXES', 'Ties go to the lower prior index',
                  'Candidate order is level-major, then ascending (d, index)', 'accumulated in float64 in candidate order',
                  't = (float)(mean + sqrt(var))', 'The inequalities are strict', 'FORCED POSITIVE',
                  'The first in candidate order wins a tie', 'A BOX CAN STILL END WITH NO PRIOR',
                  'a forced claim over an ordinary one, then the larger IoU, then the lower box index',
                  'conf_t = (0, 1)', 'level_off travels in the kernel arguments'):
        assert words in text, words
    for name in ('ct_box.hip', 'ct_atss.hip'):
        src = open(os.path.join(REPO, 'context-transformer_amd', 'csrc', name)).read()
        assert '#include "ct_box_math.h"' in src and 'float iou_plain(' not in src, name   # shared, not copied
    import importlib.util
    spec = importlib.util.spec_from_file_location('ctdet_build', os.path.join(REPO, 'context-transformer_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SOURCES['ct_atss.hip'] == ['-ffp-contract=off']
