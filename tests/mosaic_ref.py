"""Test infrastructure: the pixels of the four-image mosaic for GIVEN plans and tiles (include/ctdet.h MOSAIC), in
float64.  Every sample goes through the steps of oracle.augment_ref.augment up to the resize (crop, `distort`, canvas,
mirror, materialised like the reference does), is resized to its tile's w x h by `resize_wh` -- resize_u8's three rules
restated with two target sizes -- and pasted at (x0, y0); the lowest slot wins a pixel, empty tiles are skipped and a
pixel no tile holds gets slot 0's canvas fill.  dtype=np.float32 evaluates the resize arithmetic (weights, products,
sums) in float32 instead, which is how far a float32 evaluation may stray from this one."""
import numpy as np

from oracle import augment_ref


def resize_wh(img, w, h, interp, dtype=np.float64):
    """cv2.resize(img, (w, h)) for INTER_LINEAR (0), INTER_NEAREST (1), INTER_AREA (2; enlarging: linear); unknown
    values run as linear.  uint8 [H,W,3] -> uint8 [h,w,3]."""
    H, W = img.shape[:2]
    src = img.astype(dtype)
    sx, sy = np.float32(W) / np.float32(w), np.float32(H) / np.float32(h)
    if interp == 1:
        xs = np.minimum(np.floor(np.arange(w, dtype=np.float32) * sx).astype(int), W - 1)
        ys = np.minimum(np.floor(np.arange(h, dtype=np.float32) * sy).astype(int), H - 1)
        return img[ys][:, xs]
    if interp == 2 and (sx > 1 or sy > 1):
        out = np.zeros((h, w, 3), dtype=dtype)

        def weights(n_dst, n_src, sc):
            wt = np.zeros((n_dst, n_src), dtype=dtype)
            for d in range(n_dst):
                a, b = np.float32(d) * sc, min(np.float32(d + 1) * sc, np.float32(n_src))
                for i in range(int(np.floor(a)), int(np.ceil(b))):
                    wt[d, i] = min(b, i + 1.0) - max(a, float(i))
            return wt
        wy, wx = weights(h, H, sy), weights(w, W, sx)
        for c in range(3):
            out[..., c] = (wy @ src[..., c] @ wx.T) / (wy.sum(1)[:, None] * wx.sum(1)[None, :])
        return np.clip(np.rint(out), 0, 255).astype(np.uint8)
    fx = (np.arange(w, dtype=np.float32) + np.float32(0.5)) * sx - np.float32(0.5)
    fy = (np.arange(h, dtype=np.float32) + np.float32(0.5)) * sy - np.float32(0.5)
    ix, iy = np.floor(fx).astype(int), np.floor(fy).astype(int)
    ax, ay = (fx - ix).astype(dtype), (fy - iy).astype(dtype)
    lo, hi = ix < 0, ix >= W - 1
    ax[lo], ix[lo] = 0, 0
    ax[hi], ix[hi] = 0, W - 1
    ix1 = np.minimum(ix + 1, W - 1)
    iy0, iy1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    top = src[iy0][:, ix] * (1 - ax)[None, :, None] + src[iy0][:, ix1] * ax[None, :, None]
    bot = src[iy1][:, ix] * (1 - ax)[None, :, None] + src[iy1][:, ix1] * ax[None, :, None]
    out = top * (1 - ay)[:, None, None] + bot * ay[:, None, None]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def before_resize(img, plan, fill):
    """The uint8 image that enters the resize: crop, distortion, canvas, mirror (augment_ref.augment's steps)."""
    l, t, w, h = plan['crop']
    x = img[t:t + h, l:l + w]
    x = augment_ref.distort(x, plan) if plan['flags'] else x.copy()
    ew, eh, left, top = plan['exp']
    if (ew, eh) != (w, h):
        canvas = np.empty((eh, ew, 3), dtype=np.uint8)
        canvas[:, :] = np.asarray(fill)                  # float means cast into the uint8 canvas
        canvas[top:top + h, left:left + w] = x
        x = canvas
    if plan['mirror']:
        x = x[:, ::-1]
    return x


def mosaic(images, plans, tiles, size, means, fill=None, dtype=np.float64):
    """One mosaic image: four uint8 [H,W,3] sources, four plan dicts (aug_plan_ref.plan_dict), four tiles
    (x0, y0, w, h) -> float32 [3,size,size]."""
    S = int(size)
    fill = means if fill is None else fill
    out = np.empty((S, S, 3), dtype=np.uint8)
    out[:, :] = np.asarray(fill)
    for k in (3, 2, 1, 0):                               # painted in reverse: the lowest slot wins a pixel
        x0, y0, w, h = (int(v) for v in tiles[k])
        if w < 1 or h < 1:
            continue
        xa, xb, ya, yb = max(x0, 0), min(x0 + w, S), max(y0, 0), min(y0 + h, S)
        if xa >= xb or ya >= yb:
            continue
        tile = resize_wh(before_resize(images[k], plans[k], fill), w, h, plans[k]['interp'], dtype)
        out[ya:yb, xa:xb] = tile[ya - y0:yb - y0, xa - x0:xb - x0]
    res = out.astype(np.float32)
    res -= np.asarray(means, dtype=np.float32)
    return res.transpose(2, 0, 1).copy()
