// libctdet: test-time input transform (data/data_augment.py:224-266 BaseTransform):
//   cv2.resize(img, (S,S), INTER_LINEAR) on uint8 HxWx3  ->  float32  ->  -= means  ->  CHW.
// One launch per batch of variable-size images packed back to back in one byte buffer.
// HBM-bound byte work: a thread produces one output pixel (4 source pixels x 3 bytes in,
// three coalesced fp32 plane stores out).  Arithmetic is OpenCV's published 8-bit bilinear
// path (imgproc/resize.cpp: 11-bit fixed-point coefficients, HResizeLinear then
// VResizeLinear with the (b*(s>>4))>>16, +2, >>2 rounding), so results are whole numbers
// exactly as the uint8 image cv2 returns.
#include "ct_common.h"
#include <algorithm>
#include <cstdlib>

namespace {

struct Tap {
    int s0, s1;
    int c0, c1;
};

// coefficient pair of one output coordinate.  zero_frac_at_edges: OpenCV clears the fraction
// at the horizontal borders; vertically it only clamps the row indices.
__device__ inline Tap make_tap(int d, double scale, int n, bool zero_frac_at_edges)
{
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    Tap t;
    if (zero_frac_at_edges) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= n - 1) { f = 0.f; s = n - 1; }
        t.s0 = s;
        t.s1 = min(s + 1, n - 1);
    } else {
        t.s0 = min(max(s, 0), n - 1);
        t.s1 = min(max(s + 1, 0), n - 1);
    }
    t.c0 = __float2int_rn((1.f - f) * 2048.f);
    t.c1 = __float2int_rn(f * 2048.f);
    return t;
}

__global__ __launch_bounds__(256) void resize_sub_chw(const unsigned char* __restrict__ src,
                                                      const long long* __restrict__ offs,
                                                      const int* __restrict__ hw, float* __restrict__ out,
                                                      int S, float m0, float m1, float m2)
{
    const int n = blockIdx.y;
    const int H = hw[2 * n], W = hw[2 * n + 1];
    const unsigned char* img = src + offs[n];
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= S * S) return;
    const int dy = pix / S, dx = pix - dy * S;
    const Tap tx = make_tap(dx, (double)W / S, W, true);
    const Tap ty = make_tap(dy, (double)H / S, H, false);
    const unsigned char* r0 = img + (long)ty.s0 * W * 3;
    const unsigned char* r1 = img + (long)ty.s1 * W * 3;
    const float mean[3] = {m0, m1, m2};
    float* o = out + (long)n * 3 * S * S + pix;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int h0 = r0[tx.s0 * 3 + c] * tx.c0 + r0[tx.s1 * 3 + c] * tx.c1;
        const int h1 = r1[tx.s0 * 3 + c] * tx.c0 + r1[tx.s1 * 3 + c] * tx.c1;
        int v = (((ty.c0 * (h0 >> 4)) >> 16) + ((ty.c1 * (h1 >> 4)) >> 16) + 2) >> 2;
        v = min(max(v, 0), 255);
        o[(long)c * S * S] = (float)v - mean[c];
    }
}

}  // namespace

extern "C" int ct_preproc_resize(const unsigned char* src, const long long* offsets, const int* hw,
                                 int batch, int size, const float* means3, float* out, ct_stream_t stream)
{
    CT_REQUIRE(src && offsets && hw && out && means3, "ct_preproc_resize: null pointer");
    CT_REQUIRE(batch > 0 && batch <= 65535 && size > 0 && size <= 4096, "ct_preproc_resize: batch=%d size=%d",
               batch, size);
    dim3 grid((size * size + 255) / 256, batch);
    hipLaunchKernelGGL(resize_sub_chw, grid, dim3(256), 0, ctdet::as_stream(stream), src, offsets, hw, out, size,
                       means3[0], means3[1], means3[2]);
    CT_LAUNCH_CHECK("resize_sub_chw");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// Training-time augmentation (data/data_augment.py:164-221 `preproc.__call__`): crop -> photometric distortion
// (brightness, contrast, hue, saturation in the 8-bit HSV space of cv2.cvtColor) -> expand on a mean-filled
// canvas -> mirror -> resize -> minus means -> CHW, as ONE gather kernel per batch.  The random DECISIONS (which
// crop, which distortions, where on the canvas, which interpolation) are the reference's host-side scalar logic
// (context-transformer_amd/data/data_augment.py draws them with the same `random` calls in the same order);
// only the pixel work runs here.  A thread produces one output pixel: it maps it back through resize, mirror,
// canvas and crop to the source pixels it depends on and applies the distortion to each of them, so no
// intermediate image exists.  cv2 itself is not in this image: the 8-bit HSV arithmetic restates OpenCV's
// published formulas (imgproc/color_hsv: V = max, S = 255*(V-min)/V, H = 30*sector position, all rounded to
// nearest) -- tolerance-based parity, pinned by oracle/augment_ref.py.
namespace {

using AugPlan = ct_aug_plan_record;         // one image's decisions (include/ctdet.h)

__device__ __forceinline__ int clip255_trunc(double v)      // numpy: float64 tmp clipped to [0,255], stored into uint8 (truncation)
{
    return (int)fmin(fmax(v, 0.0), 255.0);
}

// distortion of one BGR pixel, 8-bit at every stage like the reference's uint8 arrays
__device__ inline void distort_px(int& b, int& g, int& r, const AugPlan& p)
{
    if (p.flags & 1) { const double be = p.beta; b = clip255_trunc(b + be); g = clip255_trunc(g + be); r = clip255_trunc(r + be); }
    if (p.flags & 2) { const double al = p.alpha; b = clip255_trunc(b * al); g = clip255_trunc(g * al); r = clip255_trunc(r * al); }
    // BGR -> HSV, 8 bit: H in [0,180), S, V in [0,255]; exact integer round-half-up of 255*diff/V and 30*pos/diff
    // (OpenCV's fixed-point tables approximate exactly that)
    const int v = max(b, max(g, r)), mn = min(b, min(g, r)), diff = v - mn;
    int s = v == 0 ? 0 : (2 * 255 * diff + v) / (2 * v);
    int h = 0;
    if (diff != 0) {
        int num;                         // hue position in units of 1/diff sectors
        if (v == r) num = g - b;
        else if (v == g) num = 2 * diff + (b - r);
        else num = 4 * diff + (r - g);
        if (num < 0) num += 6 * diff;
        h = (2 * 30 * num + diff) / (2 * diff);
        if (h >= 180) h -= 180;
    }
    if (p.flags & 4) { h = (h + p.hue_delta) % 180; if (h < 0) h += 180; }
    if (p.flags & 8) s = clip255_trunc(s * (double)p.sat_alpha);
    // HSV -> BGR (float sector formula, rounded to nearest)
    const float S = s * (1.f / 255.f), V = (float)v;
    const float hh = h * (1.f / 30.f);
    const int sec = min((int)hh, 5);
    const float f = hh - sec;
    const float pq = V * (1.f - S), qq = V * (1.f - S * f), tq = V * (1.f - S * (1.f - f));
    float R, G, B;
    switch (sec) {
        case 0: R = V; G = tq; B = pq; break;
        case 1: R = qq; G = V; B = pq; break;
        case 2: R = pq; G = V; B = tq; break;
        case 3: R = pq; G = qq; B = V; break;
        case 4: R = tq; G = pq; B = V; break;
        default: R = V; G = pq; B = qq; break;
    }
    b = min(max(__float2int_rn(B), 0), 255);
    g = min(max(__float2int_rn(G), 0), 255);
    r = min(max(__float2int_rn(R), 0), 255);
}

// pixel (x, y) of the image that enters the resize: mirror -> canvas -> crop -> source (+ distortion), 8 bit
__device__ inline void final_px_u8(const unsigned char* __restrict__ img, const AugPlan& p, int x, int y, int (&o)[3])
{
    if (p.mirror) x = p.exp_w - 1 - x;
    const int cx = x - p.exp_left, cy = y - p.exp_top;
    if ((unsigned)cx >= (unsigned)p.crop_w || (unsigned)cy >= (unsigned)p.crop_h) {
        o[0] = (int)p.fill[0]; o[1] = (int)p.fill[1]; o[2] = (int)p.fill[2];   // means cast to uint8
        return;
    }
    const unsigned char* s = img + ((long)(p.crop_t + cy) * p.W + (p.crop_l + cx)) * 3;
    int b = s[0], g = s[1], r = s[2];
    if (p.flags) distort_px(b, g, r, p);
    o[0] = b; o[1] = g; o[2] = r;
}

__device__ inline void final_px(const unsigned char* __restrict__ img, const AugPlan& p, int x, int y, float (&o)[3])
{
    int v[3];
    final_px_u8(img, p, x, y, v);
    o[0] = (float)v[0]; o[1] = (float)v[1]; o[2] = (float)v[2];
}

// output pixel (dx, dy) of the float filters (interp 0 linear, 1 nearest, 2 area; anything else runs as linear), before
// rounding, of a resize to tw x th (the whole square, or a mosaic tile).  The one definition every augmentation kernel
// calls.
__device__ inline void float_filter_px(const unsigned char* __restrict__ img, const AugPlan& p, int tw, int th, int dx,
                                       int dy, float (&acc)[3])
{
    const float sx = (float)p.exp_w / tw, sy = (float)p.exp_h / th;
    acc[0] = acc[1] = acc[2] = 0.f;
    if (p.interp == 1) {                        // INTER_NEAREST: floor(d * scale)
        final_px(img, p, min((int)floorf(dx * sx), p.exp_w - 1), min((int)floorf(dy * sy), p.exp_h - 1), acc);
    } else if (p.interp == 2 && (sx > 1.f || sy > 1.f)) {      // INTER_AREA when shrinking: fractional box average
        const float x0 = dx * sx, x1 = fminf((dx + 1) * sx, (float)p.exp_w), y0 = dy * sy, y1 = fminf((dy + 1) * sy, (float)p.exp_h);
        float wsum = 0.f;
        for (int yy = (int)floorf(y0); yy < (int)ceilf(y1); ++yy) {
            const float wy = fminf(y1, yy + 1.f) - fmaxf(y0, (float)yy);
            for (int xx = (int)floorf(x0); xx < (int)ceilf(x1); ++xx) {
                const float w = wy * (fminf(x1, xx + 1.f) - fmaxf(x0, (float)xx));
                float v[3];
                final_px(img, p, xx, yy, v);
                acc[0] += w * v[0]; acc[1] += w * v[1]; acc[2] += w * v[2];
                wsum += w;
            }
        }
        acc[0] /= wsum; acc[1] /= wsum; acc[2] /= wsum;
    } else {                                     // INTER_LINEAR (and INTER_AREA when enlarging): half-pixel centres
        float fx = (dx + 0.5f) * sx - 0.5f, fy = (dy + 0.5f) * sy - 0.5f;
        int ix = (int)floorf(fx), iy = (int)floorf(fy);
        fx -= ix; fy -= iy;
        if (ix < 0) { ix = 0; fx = 0.f; }
        if (ix >= p.exp_w - 1) { ix = p.exp_w - 1; fx = 0.f; }
        const int ix1 = min(ix + 1, p.exp_w - 1);
        const int iy0 = min(max(iy, 0), p.exp_h - 1), iy1 = min(max(iy + 1, 0), p.exp_h - 1);
        float v00[3], v01[3], v10[3], v11[3];
        final_px(img, p, ix, iy0, v00); final_px(img, p, ix1, iy0, v01);
        final_px(img, p, ix, iy1, v10); final_px(img, p, ix1, iy1, v11);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            acc[c] = (1.f - fy) * ((1.f - fx) * v00[c] + fx * v01[c]) + fy * ((1.f - fx) * v10[c] + fx * v11[c]);
    }
}

// cv2.resize returns uint8: round to nearest, then float32 minus mean
__device__ inline void store_float_px(const float (&acc)[3], float* __restrict__ o, int S, float m0, float m1, float m2)
{
    const float mean[3] = {m0, m1, m2};
#pragma unroll
    for (int c = 0; c < 3; ++c)
        o[(long)c * S * S] = fminf(fmaxf(rintf(acc[c]), 0.f), 255.f) - mean[c];
}

__global__ __launch_bounds__(256) void augment_kernel(const unsigned char* __restrict__ src, const AugPlan* __restrict__ plans,
                                                      float* __restrict__ out, int S, float m0, float m1, float m2)
{
    const int n = blockIdx.y;
    const AugPlan p = plans[n];
    const unsigned char* img = src + p.src_off;
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= S * S) return;
    const int dy = pix / S, dx = pix - dy * S;
    float acc[3];
    float_filter_px(img, p, S, S, dx, dy, acc);
    store_float_px(acc, out + (long)n * 3 * S * S + pix, S, m0, m1, m2);
}

// Mosaic (include/ctdet.h MOSAIC): image n is composed of the plans 4n..4n+3, each resized into its tile instead of
// the whole square.  A thread finds its pixel's tile with four comparisons (the lowest slot that holds it; the
// differences are formed unsigned, so no tile content overflows) and runs the filter of augment_kernel with the tile's
// size as the resize target.  Lanes diverge only where a wave crosses a seam.  A pixel no tile holds gets slot 0's
// canvas fill: that, and skipping empty tiles, is what makes foreign tile tables memory-safe.
__global__ __launch_bounds__(256) void augment_mosaic_kernel(const unsigned char* __restrict__ src, const AugPlan* __restrict__ plans,
                                                             const ct_mosaic_tile* __restrict__ tiles, float* __restrict__ out,
                                                             int S, float m0, float m1, float m2)
{
    const int n = blockIdx.y;
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= S * S) return;
    const int dy = pix / S, dx = pix - dy * S;
    int k = -1, tx = 0, ty = 0, tw = 0, th = 0;
#pragma unroll
    for (int kk = 3; kk >= 0; --kk) {
        const ct_mosaic_tile t = tiles[4 * n + kk];
        const unsigned ux = (unsigned)dx - (unsigned)t.x0, uy = (unsigned)dy - (unsigned)t.y0;
        if (t.w >= 1 && t.h >= 1 && ux < (unsigned)t.w && uy < (unsigned)t.h) { k = kk; tx = (int)ux; ty = (int)uy; tw = t.w; th = t.h; }
    }
    float* o = out + (long)n * 3 * S * S + pix;
    float acc[3];
    if (k < 0) {
        const AugPlan& p0 = plans[4 * n];
        acc[0] = (float)(int)p0.fill[0]; acc[1] = (float)(int)p0.fill[1]; acc[2] = (float)(int)p0.fill[2];
        o[0] = acc[0] - m0; o[(long)S * S] = acc[1] - m1; o[2L * S * S] = acc[2] - m2;
        return;
    }
    const AugPlan p = plans[4 * n + k];
    float_filter_px(src + p.src_off, p, tw, th, tx, ty, acc);
    store_float_px(acc, o, S, m0, m1, m2);
}

// ---------------------------------------------------------------------------------------------------------
// The two higher-order filters (interp 3 bicubic, 4 Lanczos4): OpenCV's 8-bit separable fixed-point resize.  The
// taps (`first` index and 11-bit coefficients per output coordinate) are HOST decisions like the rest of the plan
// (ctdet/ops.py resize_taps: the Lanczos4 coefficients need a double sin/cos, which a device evaluates differently
// in the last bit); the device does integer work only, so its pixels are bit-reproducible:
//   h[r][d] = sum_j cx[d][j] * P(clamp(first_x[d] + j), r),   v = sum_j cy[d][j] * h[clamp(first_y[d] + j)][.],
//   pixel = clamp((v + 2^21) >> 22, 0, 255).
// The kernel clamps every index it forms from a table to the canvas, so no table content can make it read outside
// the image.  Sums wrap modulo 2^32 (unsigned accumulation): defined for every table, meaningful for those whose
// rows keep |v| inside int32 (include/ctdet.h).
constexpr int TAP_TW = 32, TAP_TH = 8;          // output tile of one workgroup (256 threads, one pixel each)
constexpr int TAP_LDS_WORDS = 9728;             // 38 KiB: packed source window + horizontal pass; 4 workgroups per CU

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ float tap_result(unsigned v, float mean)
{
    return (float)clampi((int)(v + (1u << 21)) >> 22, 0, 255) - mean;
}

// One workgroup = one 32x8 output tile of one image, so every branch on the plan or on the tile's window is
// block-uniform.  interp 0..2 (and unknown values): float_filter_px, the code of augment_kernel.  interp 3 / 4:
//   tiled form   the tile's source window goes through final_px_u8 (crop, canvas, mirror, distortion) ONCE per source
//                pixel into LDS as packed BGR, then a horizontal pass into an int32 LDS image, then the vertical pass;
//   gather form  a thread evaluates final_px_u8 k x k times for its own pixel -- any canvas size; taken when the
//                window does not fit TAP_LDS_WORDS, when the canvas fill is no 8-bit value, or when tiled == 0.
// Both forms add the same integers modulo 2^32, so they agree bit for bit.
__global__ __launch_bounds__(256) void augment_taps_kernel(const unsigned char* __restrict__ src, const AugPlan* __restrict__ plans,
                                                           const ct_resize_tap* __restrict__ taps, float* __restrict__ out,
                                                           int S, int tiles_x, int tiled, float m0, float m1, float m2)
{
    __shared__ ct_resize_tap tap_x[TAP_TW], tap_y[TAP_TH];
    __shared__ unsigned lds[TAP_LDS_WORDS];
    const int n = blockIdx.y, tid = threadIdx.x;
    const AugPlan p = plans[n];
    const unsigned char* img = src + p.src_off;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int lx = tid % TAP_TW, ly = tid / TAP_TW;
    const int dx = tile_x * TAP_TW + lx, dy = tile_y * TAP_TH + ly;
    const bool live = dx < S && dy < S;
    float* o = out + (long)n * 3 * S * S + (long)dy * S + dx;
    if (p.interp != 3 && p.interp != 4) {
        if (!live) return;
        float acc[3];
        float_filter_px(img, p, S, S, dx, dy, acc);
        store_float_px(acc, o, S, m0, m1, m2);
        return;
    }
    const int k = p.interp == 3 ? 4 : 8;
    const int nx = p.exp_w, ny = p.exp_h;
    // the tile's tap records; coordinates past the image edge reuse the last one (computed, never stored)
    const ct_resize_tap* tab = taps + (long)n * 2 * S;
    if (tid < TAP_TW) tap_x[tid] = tab[min(tile_x * TAP_TW + tid, S - 1)];
    else if (tid < TAP_TW + TAP_TH) tap_y[tid - TAP_TW] = tab[S + min(tile_y * TAP_TH + (tid - TAP_TW), S - 1)];
    __syncthreads();
    // source window of the tile: min / max over the clamped indices the passes below will form (no order assumed)
    int x0 = nx - 1, x1 = 0, y0 = ny - 1, y1 = 0;
    for (int i = 0; i < TAP_TW; ++i) {
        x0 = min(x0, clampi(tap_x[i].first, 0, nx - 1));
        x1 = max(x1, clampi(tap_x[i].first + k - 1, 0, nx - 1));
    }
    for (int i = 0; i < TAP_TH; ++i) {
        y0 = min(y0, clampi(tap_y[i].first, 0, ny - 1));
        y1 = max(y1, clampi(tap_y[i].first + k - 1, 0, ny - 1));
    }
    const long ww = (long)x1 - x0 + 1, wh = (long)y1 - y0 + 1;
    const bool fill_u8 = (unsigned)(int)p.fill[0] < 256u && (unsigned)(int)p.fill[1] < 256u && (unsigned)(int)p.fill[2] < 256u;
    unsigned v[3] = {0u, 0u, 0u};
    if (tiled && fill_u8 && ww > 0 && wh > 0 && ww * wh + 3 * wh * TAP_TW <= TAP_LDS_WORDS) {
        const int w = (int)ww, h = (int)wh;
        unsigned* hbuf = lds + w * h;                         // [3][h][TAP_TW]
        for (int i = tid; i < w * h; i += 256) {
            const int y = i / w, x = i - y * w;
            int c[3];
            final_px_u8(img, p, x0 + x, y0 + y, c);
            lds[i] = (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16;
        }
        __syncthreads();
        for (int i = tid; i < h * TAP_TW; i += 256) {         // horizontal pass: row r of the window, output column d
            const int r = i / TAP_TW, d = i - r * TAP_TW;
            unsigned a[3] = {0u, 0u, 0u};
            for (int j = 0; j < k; ++j) {
                const unsigned px = lds[r * w + clampi(tap_x[d].first + j, 0, nx - 1) - x0];
                const unsigned cf = (unsigned)(int)tap_x[d].c[j];
                a[0] += cf * (px & 255u); a[1] += cf * (px >> 8 & 255u); a[2] += cf * (px >> 16);
            }
            hbuf[i] = a[0]; hbuf[h * TAP_TW + i] = a[1]; hbuf[2 * h * TAP_TW + i] = a[2];
        }
        __syncthreads();
        for (int j = 0; j < k; ++j) {                         // vertical pass
            const int r = clampi(tap_y[ly].first + j, 0, ny - 1) - y0;
            const unsigned cf = (unsigned)(int)tap_y[ly].c[j];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] += cf * hbuf[(c * h + r) * TAP_TW + lx];
        }
    } else {
        for (int jy = 0; jy < k; ++jy) {
            const int y = clampi(tap_y[ly].first + jy, 0, ny - 1);
            unsigned a[3] = {0u, 0u, 0u};
            for (int jx = 0; jx < k; ++jx) {
                int c[3];
                final_px_u8(img, p, clampi(tap_x[lx].first + jx, 0, nx - 1), y, c);
                const unsigned cf = (unsigned)(int)tap_x[lx].c[jx];
                a[0] += cf * (unsigned)c[0]; a[1] += cf * (unsigned)c[1]; a[2] += cf * (unsigned)c[2];
            }
            const unsigned cf = (unsigned)(int)tap_y[ly].c[jy];
            v[0] += cf * a[0]; v[1] += cf * a[1]; v[2] += cf * a[2];
        }
    }
    if (!live) return;
    o[0] = tap_result(v[0], m0);
    o[(long)S * S] = tap_result(v[1], m1);
    o[2L * S * S] = tap_result(v[2], m2);
}

__global__ __launch_bounds__(256) void mixup_blend_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const float* __restrict__ lambd, float* __restrict__ out,
                                                          long per_image, int batch)
{
    const long total = per_image * batch;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const float l = lambd[i / per_image];
        out[i] = a[i] * l + b[i] * (1.f - l);       // voc0712.py:262: img1 * lambd + img2 * (1 - lambd)
    }
}

}  // namespace

extern "C" int ct_preproc_augment(const unsigned char* src, const void* plans, int batch, int size,
                                  const float* means3, float* out, ct_stream_t stream)
{
    CT_REQUIRE(src && plans && out && means3, "ct_preproc_augment: null pointer");
    CT_REQUIRE(batch > 0 && batch <= 65535 && size > 0 && size <= 4096, "ct_preproc_augment: batch=%d size=%d", batch, size);
    dim3 grid((size * size + 255) / 256, batch);
    hipLaunchKernelGGL(augment_kernel, grid, dim3(256), 0, ctdet::as_stream(stream), src, (const AugPlan*)plans, out, size,
                       means3[0], means3[1], means3[2]);
    CT_LAUNCH_CHECK("augment_kernel");
    return CT_OK;
}

extern "C" int ct_preproc_augment_mosaic(const unsigned char* src, const void* plans, const ct_mosaic_tile* tiles,
                                         int num_images, int size, const float* means3, float* out, ct_stream_t stream)
{
    CT_REQUIRE(src && plans && tiles && out && means3, "ct_preproc_augment_mosaic: null pointer");
    CT_REQUIRE(num_images > 0 && num_images <= 65535 && size >= 2 && size <= 4096,
               "ct_preproc_augment_mosaic: num_images=%d size=%d", num_images, size);
    dim3 grid((size * size + 255) / 256, num_images);
    hipLaunchKernelGGL(augment_mosaic_kernel, grid, dim3(256), 0, ctdet::as_stream(stream), src, (const AugPlan*)plans,
                       tiles, out, size, means3[0], means3[1], means3[2]);
    CT_LAUNCH_CHECK("augment_mosaic_kernel");
    return CT_OK;
}

extern "C" int ct_preproc_augment_taps(const unsigned char* src, const void* plans, const ct_resize_tap* taps, int batch,
                                       int size, const float* means3, float* out, ct_stream_t stream)
{
    CT_REQUIRE(src && plans && taps && out && means3, "ct_preproc_augment_taps: null pointer");
    CT_REQUIRE(batch > 0 && batch <= 65535 && size > 0 && size <= 4096, "ct_preproc_augment_taps: batch=%d size=%d", batch, size);
    static const int tiled = [] {                   // CTDET_AUG_TILED=0: gather form everywhere (read once)
        const char* e = getenv("CTDET_AUG_TILED");
        return !(e && e[0] == '0' && e[1] == 0);
    }();
    const int tiles_x = (size + TAP_TW - 1) / TAP_TW, tiles_y = (size + TAP_TH - 1) / TAP_TH;
    hipLaunchKernelGGL(augment_taps_kernel, dim3(tiles_x * tiles_y, batch), dim3(256), 0, ctdet::as_stream(stream), src,
                       (const AugPlan*)plans, taps, out, size, tiles_x, tiled, means3[0], means3[1], means3[2]);
    CT_LAUNCH_CHECK("augment_taps_kernel");
    return CT_OK;
}

extern "C" int ct_mixup_blend(const float* img1, const float* img2, const float* lambd, int batch, long per_image,
                              float* out, ct_stream_t stream)
{
    CT_REQUIRE(img1 && img2 && lambd && out && batch > 0 && per_image > 0, "ct_mixup_blend: bad arguments");
    const long total = per_image * batch;
    hipLaunchKernelGGL(mixup_blend_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0,
                       ctdet::as_stream(stream), img1, img2, lambd, out, per_image, batch);
    CT_LAUNCH_CHECK("mixup_blend_kernel");
    return CT_OK;
}
