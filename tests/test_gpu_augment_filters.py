"""Device pixels of the bicubic / Lanczos4 augmentation filters (ct_preproc_augment_taps) against the NumPy definition
(tests/resize_taps_ref.py).  The arithmetic is integer, so every comparison is array_equal: no tolerance anywhere.
Outputs are S = 24 (less than one 32-wide tile) and S = 40 (two tiles across, the second partial; five down).

Run as a script (`python tests/test_gpu_augment_filters.py OUT.npz`) it writes the mixed batch's device output; the
tiled-equals-gather test starts it in a fresh process with CTDET_AUG_TILED=0."""
import ctypes as C
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path when this file runs as a script)
import resize_taps_ref as ref
from ctdet import ops
from ctdet._lib import check, lib
from data.data_augment import preproc, _plan

pytestmark = pytest.mark.gpu
MEANS = (104, 117, 123)
KIND = {3: 'cubic', 4: 'lanczos4'}
SIZES = (24, 40)


def _image(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def pre_resize(img, plan):
    """The image that enters the resize, on the host: crop -> mean-filled canvas -> mirror (no distortion)."""
    assert plan['flags'] == 0
    l, t, w, h = plan['crop']
    ew, eh, left, top = plan['exp']
    canvas = np.empty((eh, ew, 3), dtype=np.uint8)
    canvas[:] = np.array(MEANS, dtype=np.uint8)
    canvas[top:top + h, left:left + w] = img[t:t + h, l:l + w]
    return canvas[:, ::-1] if plan['mirror'] else canvas


def minus_means(u8_hwc):
    return u8_hwc.transpose(2, 0, 1).astype(np.float32) - np.array(MEANS, dtype=np.float32)[:, None, None]


def launch(images, plans, S, taps=None, entry='taps'):
    """The C ABI, directly: pack images, plans and tap tables the way include/ctdet.h states them -> [n,3,S,S] cpu.
    taps: [n, 2, S] records (ops.TAP_DTYPE); None builds the two filters' own tables."""
    n = len(images)
    recs = (ops.AugPlan * n)()
    chunks, pos = [], 0
    for r, img, p in zip(recs, images, plans):
        r.src_off, r.H, r.W = pos, p['H'], p['W']
        r.crop_l, r.crop_t, r.crop_w, r.crop_h = p['crop']
        r.exp_w, r.exp_h, r.exp_left, r.exp_top = p['exp']
        r.mirror, r.interp, r.flags, r.hue_delta = p['mirror'], p['interp'], p['flags'], p['hue']
        r.beta, r.alpha, r.sat_alpha = p['beta'], p['alpha'], p['sat']
        for c in range(3):
            r.fill[c] = MEANS[c]
        a = np.ascontiguousarray(img).reshape(-1)
        pad = -a.size % 16
        chunks.append(np.concatenate([a, np.zeros(pad, np.uint8)]))
        pos += a.size + pad
    src = torch.from_numpy(np.concatenate(chunks)).cuda()
    plans_d = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).cuda()
    out = torch.full((n, 3, S, S), float('nan'), device='cuda')
    means = (C.c_float * 3)(*MEANS)
    ptr = lambda t: C.c_void_p(t.data_ptr())        # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if entry == 'plain':
        check(lib().ct_preproc_augment(ptr(src), ptr(plans_d), n, S, C.cast(means, C.c_void_p), ptr(out), stream))
    else:
        if taps is None:
            taps = np.zeros((n, 2, S), dtype=ops.TAP_DTYPE)
            for i, p in enumerate(plans):
                if p['interp'] in KIND:
                    taps[i, 0] = ops.tap_records(p['exp'][0], S, KIND[p['interp']])
                    taps[i, 1] = ops.tap_records(p['exp'][1], S, KIND[p['interp']])
        assert taps.shape == (n, 2, S) and taps.dtype == ops.TAP_DTYPE
        taps_d = torch.from_numpy(np.ascontiguousarray(taps).reshape(-1).view(np.uint8)).cuda()
        check(lib().ct_preproc_augment_taps(ptr(src), ptr(plans_d), ptr(taps_d), n, S, C.cast(means, C.c_void_p),
                                            ptr(out), stream))
    torch.cuda.synchronize()
    return out.cpu()


def plan_of(img, crop=None, exp=None, mirror=0, interp=0):
    p = _plan(img.shape[0], img.shape[1])
    if crop:
        p['crop'] = crop
    p['exp'] = exp or (p['crop'][2], p['crop'][3], 0, 0)
    p['mirror'], p['interp'] = mirror, interp
    return p


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """(images, plans): every source of the issue, both filters, some mirrored, plus the three float filters."""
    square, narrow, odd, wide, big = _image(1, 24, 24), _image(2, 9, 5), _image(3, 37, 53), _image(4, 61, 200), _image(5, 64, 48)
    on_canvas = dict(crop=(7, 11, 30, 30), exp=(1000, 1000, 333, 480))         # window of any tile >> the LDS budget
    items = [(square, plan_of(square, interp=3)), (square, plan_of(square, interp=4, mirror=1)),
             (narrow, plan_of(narrow, interp=3, mirror=1)), (narrow, plan_of(narrow, interp=4)),
             (odd, plan_of(odd, interp=3)), (odd, plan_of(odd, interp=4, mirror=1)),
             (wide, plan_of(wide, interp=3, mirror=1)), (wide, plan_of(wide, interp=4)),
             (big, plan_of(big, interp=3, **on_canvas)), (big, plan_of(big, interp=4, mirror=1, **on_canvas)),
             (odd, plan_of(odd, crop=(5, 3, 40, 30), exp=(71, 52, 20, 9), mirror=1, interp=4)),
             (odd, plan_of(odd, crop=(5, 3, 40, 30), exp=(71, 52, 20, 9), mirror=1, interp=0)),
             (wide, plan_of(wide, interp=1, mirror=1)), (wide, plan_of(wide, interp=2)),
             (odd, plan_of(odd, interp=2, mirror=1))]
    return [im for im, _ in items], [p for _, p in items]


@functools.lru_cache(maxsize=None)
def mixed_out(S):
    images, plans = mixed_batch()
    return launch(images, plans, S)


@pytest.mark.parametrize('S', SIZES)
def test_both_filters_against_the_definition(S):
    images, plans = mixed_batch()
    got = mixed_out(S)
    assert not torch.isnan(got).any()
    plain = launch(images, plans, S, entry='plain')
    for i, (img, p) in enumerate(zip(images, plans)):
        if p['interp'] in KIND:
            want = minus_means(ref.resize(pre_resize(img, p), S, KIND[p['interp']]))
            assert np.array_equal(got[i].numpy(), want), (i, p, float(np.abs(got[i].numpy() - want).max()))
        else:                                       # the float filters: today's entry, bit for bit
            assert torch.equal(got[i], plain[i]), (i, p)
    if S == 24:                                     # identity at n == S
        assert np.array_equal(got[0].numpy(), minus_means(images[0]))


@pytest.mark.parametrize('interp', [3, 4])
@pytest.mark.parametrize('S', SIZES)
def test_known_geometry_with_hand_made_tables(S, interp):
    """Rows [2048, 0, ...] on both axes return the addressed source pixels: index plumbing, the kernel's clamp (firsts
    run past both ends of the canvas, in no order), mirror and canvas -- apart from the coefficients."""
    img = _image(6, 37, 53)
    images = [img, img, _image(5, 64, 48)]
    plans = [plan_of(img, interp=interp), plan_of(img, crop=(5, 3, 40, 30), exp=(71, 52, 20, 9), mirror=1, interp=interp),
             plan_of(images[2], crop=(7, 11, 30, 30), exp=(1000, 1000, 333, 480), interp=interp)]
    rng = np.random.RandomState(S + interp)
    taps = np.zeros((3, 2, S), dtype=ops.TAP_DTYPE)
    taps['c'][..., 0] = 2048
    for i, p in enumerate(plans):
        lo, hi = (320, 520) if i == 2 else (-6, 6 + max(p['exp'][:2]))      # image 2: around the crop on the canvas
        taps['first'][i] = rng.randint(lo, hi, (2, S))
    got = launch(images, plans, S, taps)
    for i, (im, p) in enumerate(zip(images, plans)):
        P = pre_resize(im, p)
        ix = np.clip(taps['first'][i, 0], 0, p['exp'][0] - 1)
        iy = np.clip(taps['first'][i, 1], 0, p['exp'][1] - 1)
        assert np.array_equal(got[i].numpy(), minus_means(P[iy][:, ix])), (i, p)


def test_distortion_without_a_tolerance():
    """The HSV arithmetic has a tolerance of its own, so the device's own distorted image is the reference input: an
    exact gather (nearest at scale 1) yields it, and the same plan through both filters must be its resize."""
    img = _image(8, 50, 60)
    p = plan_of(img, crop=(3, 5, 40, 40), interp=1)
    p.update(flags=15, beta=17.5, alpha=1.23, hue=-11, sat=0.8)
    base = launch([img], [p], 40, entry='plain')[0].numpy() + np.array(MEANS, dtype=np.float32)[:, None, None]
    distorted = base.transpose(1, 2, 0)
    assert np.array_equal(distorted, np.rint(distorted)) and distorted.min() >= 0 and distorted.max() <= 255
    distorted = distorted.astype(np.uint8)
    assert (distorted != img[5:45, 3:43]).mean() > 0.5          # the distortion did something
    plans = [dict(p, interp=3), dict(p, interp=4)]
    got = launch([img, img], plans, 24)
    for i, q in enumerate(plans):
        assert np.array_equal(got[i].numpy(), minus_means(ref.resize(distorted, 24, KIND[q['interp']]))), q['interp']


def test_tiled_equals_gather(tmp_path):
    """The same batch in a fresh process that forces the gather form everywhere (the switch is read once)."""
    path = str(tmp_path / 'gather.npz')
    env = dict(os.environ, CTDET_AUG_TILED='0')
    subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, timeout=300)
    with np.load(path) as z:
        for S in SIZES:
            assert torch.equal(torch.from_numpy(z['s%d' % S]), mixed_out(S)), S


def test_augmenter_routing(monkeypatch):
    images, plans = mixed_batch()
    aug = ops.Augmenter(24, MEANS, 'cuda')
    # no interp >= 3: today's entry, the same bytes, and the new entry is not called
    low = [(im, p) for im, p in zip(images, plans) if p['interp'] < 3]

    def boom(*a):
        raise AssertionError('ct_preproc_augment_taps called for a batch without interp >= 3')
    with monkeypatch.context() as m:
        m.setattr(lib(), 'ct_preproc_augment_taps', boom)
        got = aug([im for im, _ in low], [p for _, p in low]).cpu()
    assert torch.equal(got, launch([im for im, _ in low], [p for _, p in low], 24, entry='plain'))
    # a mixed batch goes through the tables
    assert torch.equal(aug(images, plans).cpu(), mixed_out(24))
    # preproc(filters='cv2'), seeded: its bicubic / Lanczos4 images without distortion are the definition's resize
    random.seed(ROUTING_SEED)
    rng = np.random.RandomState(ROUTING_SEED)
    pre = preproc(24, MEANS, 0.6, filters='cv2')
    imgs = [_image(100 + i, int(rng.randint(30, 70)), int(rng.randint(30, 80))) for i in range(32)]
    tgs = []
    for im in imgs:
        h, w = im.shape[:2]
        xy = rng.uniform(0, 0.6, (2, 2)) * (w, h)
        tgs.append(np.hstack([xy, np.minimum(xy + rng.uniform(0.1, 0.4, (2, 2)) * (w, h), (w - 1, h - 1)),
                              rng.randint(0, 20, (2, 1)).astype(np.float64)]))
    spied, orig = [], pre.decide

    def spy(shape, tg, cls=None):
        plan, out = orig(shape, tg, cls)
        spied.append(plan)
        return plan, out
    pre.decide = spy
    out = pre.batch(imgs, tgs)[0].cpu().numpy()
    checked = set()
    for i, (im, p) in enumerate(zip(imgs, spied)):
        if p['interp'] in KIND and p['flags'] == 0:
            assert np.array_equal(out[i], minus_means(ref.resize(pre_resize(im, p), 24, KIND[p['interp']]))), (i, p)
            checked.add(p['interp'])
    assert checked == {3, 4}


ROUTING_SEED = 83         # a seed whose 32 plans hold an undistorted image of either filter (asserted above)


if __name__ == '__main__':
    np.savez(sys.argv[1], **{'s%d' % S: mixed_out(S).numpy() for S in SIZES})
