// libctdet: the random affine post-stage of the device input pipeline (include/ctdet.h RANDOM AFFINE).
//   ct_aug_affine_plan      launch 1  affine_plan_kernel: one wave per image draws the matrix, maps the image's rows
//                                     (lanes stride over them), applies the gate and the fallback and compacts the kept
//                                     rows by ballot prefix counts into the workspace, at the image's own input range.
//                           launch 2  affine_pack_kernel: one workgroup scans the per-image counts into gt_off_out,
//                                     copies the rows and writes the status words.
//   ct_preproc_warp_affine  one launch, a 32x8 output tile per workgroup, one thread per output pixel for the three
//                           channels: fp64 source coordinates, a bilinear gather with a constant border.
// All arithmetic is + - * / floor, comparisons and fmin / fmax, compiled with contraction off: the sequence
// ctdet/aug_plan_ref.py evaluates in numpy.  Both give the same bytes.
#include "ct_common.h"
#include "ct_aug_draw.h"
#include <cmath>

namespace {

using namespace ctdet::aug;                 // philox, the draw rules, block_scan

using Rec = ct_affine_record;

constexpr unsigned SLOT_AFFINE = 0x400;
constexpr int WARP_TW = 32, WARP_TH = 8;        // ct_preproc.hip's TAP_TW x TAP_TH: 256 threads, one pixel each

__device__ __forceinline__ void identity_record(Rec& r, int flags)
{
#pragma unroll
    for (int k = 0; k < 6; ++k) r.fwd[k] = r.inv[k] = (k == 0 || k == 4) ? 1.0 : 0.0;
    r.flags = flags;
    r.pad = 0;
}

// include/ctdet.h MATRIX, operation by operation
__device__ inline void draw_matrix(unsigned long long seed, unsigned long long id, int size, const ct_affine_params& P,
                                   Rec& r, bool& applied)
{
    const Words d0 = philox(seed, id, SLOT_AFFINE, 0), d1 = philox(seed, id, SLOT_AFFINE, 1);
    const double S = size;
    const double t = uniform(-P.rot_half_tan, P.rot_half_tan, d0.w[0]);
    const double s = uniform(P.scale_lo, P.scale_hi, d0.w[1]);
    const double kx = uniform(-P.shear_tan, P.shear_tan, d0.w[2]), ky = uniform(-P.shear_tan, P.shear_tan, d0.w[3]);
    const double tx = uniform(0.5 - P.translate, 0.5 + P.translate, d1.w[0]) * S;
    const double ty = uniform(0.5 - P.translate, 0.5 + P.translate, d1.w[1]) * S;
    applied = !(unit(d1.w[2]) > (double)P.p);
    const double tt = t * t;
    const double q = 1.0 + tt, c = (1.0 - tt) / q, n = (t + t) / q, a = s * c, b = s * n;
    const double l00 = a - kx * b, l01 = b + kx * a, l10 = ky * a - b, l11 = ky * b + a;
    const double h = S * 0.5;
    r.fwd[0] = l00; r.fwd[1] = l01; r.fwd[2] = tx - (l00 * h + l01 * h);
    r.fwd[3] = l10; r.fwd[4] = l11; r.fwd[5] = ty - (l10 * h + l11 * h);
    const double det = l00 * l11 - l01 * l10;
    const double i00 = l11 / det, i01 = -l01 / det, i10 = -l10 / det, i11 = l00 / det;
    r.inv[0] = i00; r.inv[1] = i01; r.inv[2] = -(i00 * r.fwd[2] + i01 * r.fwd[5]);
    r.inv[3] = i10; r.inv[4] = i11; r.inv[5] = -(i10 * r.fwd[2] + i11 * r.fwd[5]);
    r.flags = 1;
    r.pad = 0;
}

// include/ctdet.h ROWS: the bounding box of the mapped corners, clipped and normalised; false when the row is not kept
__device__ inline bool map_row(const float* __restrict__ q, const double (&f)[6], double S, double min_side,
                               double min_visible, float (&o)[4])
{
    const double u1 = (double)q[0] * S, v1 = (double)q[1] * S, u2 = (double)q[2] * S, v2 = (double)q[3] * S;
    const double xa = (f[0] * u1 + f[1] * v1) + f[2], ya = (f[3] * u1 + f[4] * v1) + f[5];
    const double xb = (f[0] * u2 + f[1] * v1) + f[2], yb = (f[3] * u2 + f[4] * v1) + f[5];
    const double xc = (f[0] * u1 + f[1] * v2) + f[2], yc = (f[3] * u1 + f[4] * v2) + f[5];
    const double xd = (f[0] * u2 + f[1] * v2) + f[2], yd = (f[3] * u2 + f[4] * v2) + f[5];
    double X1 = fmin(fmin(fmin(xa, xb), xc), xd), X2 = fmax(fmax(fmax(xa, xb), xc), xd);
    double Y1 = fmin(fmin(fmin(ya, yb), yc), yd), Y2 = fmax(fmax(fmax(ya, yb), yc), yd);
    const double A0 = (X2 - X1) * (Y2 - Y1);
    X1 = fmin(fmax(X1, 0.0), S); Y1 = fmin(fmax(Y1, 0.0), S);
    X2 = fmin(fmax(X2, 0.0), S); Y2 = fmin(fmax(Y2, 0.0), S);
    const double w = X2 - X1, h = Y2 - Y1;
    const double A1 = w * h;
    o[0] = (float)(X1 / S); o[1] = (float)(Y1 / S); o[2] = (float)(X2 / S); o[3] = (float)(Y2 / S);
    return fmin(w, h) / S > min_side && A1 >= min_visible * A0;
}

__device__ __forceinline__ int clamp_off(int v, int rows) { return min(max(v, 0), rows); }

// One wave per image.  counts[i] = rows kept (-1: refused), counts[batch + i] = 1 when the fallback fired.  The kept
// rows go to `rows` (the workspace, [truths_rows,6]) from the image's own begin on: accepted images read disjoint
// ranges of truths_in, so their slots are disjoint too.
__global__ __launch_bounds__(64) void affine_plan_kernel(const float* __restrict__ truths, const int* __restrict__ gt_off,
                                                         const unsigned long long* __restrict__ ids, int batch,
                                                         int truths_rows, int size, unsigned long long seed,
                                                         ct_affine_params P, Rec* __restrict__ records,
                                                         int* __restrict__ counts, float* __restrict__ rows)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= batch) return;
    const int b = clamp_off(gt_off[i], truths_rows), e = clamp_off(gt_off[i + 1], truths_rows);
    // the largest clamped end of the images before this one (gt_off[1..i-1]; gt_off[i] is this image's begin)
    int prev = 0;
    for (int j = 1 + lane; j < i; j += 64) prev = max(prev, clamp_off(gt_off[j], truths_rows));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) prev = max(prev, __shfl_xor(prev, d));
    Rec rec;
    if (b > e || b < prev) {                                    // refused: identity, no rows
        identity_record(rec, 4);
        if (lane == 0) { records[i] = rec; counts[i] = -1; counts[batch + i] = 0; }
        return;
    }
    const int n = e - b;
    bool applied;
    draw_matrix(seed, ids[i], size, P, rec, applied);
    const double S = size, min_side = P.min_side, min_visible = P.min_visible;
    const float* __restrict__ src = truths + (size_t)b * 6;
    float* __restrict__ dst = rows + (size_t)b * 6;
    // pass 1: does any mapped row pass
    bool any_kept = false;
    if (applied) {
        for (int base = 0; base < n; base += 64) {
            const int j = base + lane;
            float o[4];
            any_kept |= __ballot(j < n && map_row(src + (size_t)j * 6, rec.fwd, S, min_side, min_visible, o)) != 0;
        }
    }
    const bool fallback = applied && n > 0 && !any_kept;
    const bool warped = applied && !fallback;
    // pass 2: the rows, compacted in input order; an image that is not warped keeps its rows bit for bit
    int at = 0;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        float o[4];
        bool keep = false;
        if (j < n) keep = warped ? map_row(src + (size_t)j * 6, rec.fwd, S, min_side, min_visible, o) : true;
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const unsigned* q = (const unsigned*)(src + (size_t)j * 6);
            unsigned* w = (unsigned*)(dst + (size_t)(at + __popcll(mask & ((1ull << lane) - 1ull))) * 6);
            if (warped) {
                w[0] = __float_as_uint(o[0]); w[1] = __float_as_uint(o[1]);
                w[2] = __float_as_uint(o[2]); w[3] = __float_as_uint(o[3]);
            } else {
                w[0] = q[0]; w[1] = q[1]; w[2] = q[2]; w[3] = q[3];
            }
            w[4] = q[4]; w[5] = q[5];
        }
        at += __popcll(mask);
    }
    if (lane == 0) {
        if (!warped) identity_record(rec, fallback ? (2 | 4) : 4);
        records[i] = rec;
        counts[i] = at;
        counts[batch + i] = fallback ? 1 : 0;
    }
}

// One workgroup: a thread owns one image of the current chunk of PACK_THREADS.  gt_off_out[i] = rows of the images
// before i.  The total never exceeds truths_rows: the accepted images' input ranges are disjoint and none gains rows.
__global__ __launch_bounds__(PACK_THREADS) void affine_pack_kernel(const int* __restrict__ gt_off_in, int batch,
                                                                   int truths_rows, const int* __restrict__ counts,
                                                                   const float* __restrict__ rows,
                                                                   float* __restrict__ truths, int* __restrict__ gt_off,
                                                                   int* __restrict__ status)
{
    __shared__ int sh[PACK_THREADS];
    __shared__ int carry_sum, n_bad, n_fallback;
    const int tid = threadIdx.x;
    if (tid == 0) { carry_sum = 0; n_bad = 0; n_fallback = 0; }
    __syncthreads();
    for (int base = 0; base < batch; base += PACK_THREADS) {
        const int i = base + tid;
        const bool live = i < batch;
        int cnt = 0, begin = 0;
        if (live) {
            const int c = counts[i];
            begin = clamp_off(gt_off_in[i], truths_rows);
            if (c < 0) atomicAdd(&n_bad, 1);
            if (counts[batch + i]) atomicAdd(&n_fallback, 1);
            cnt = min(max(c, 0), truths_rows - begin);
        }
        const int csum = carry_sum;
        const int incl = block_scan<false>(cnt, sh);
        const int off = csum + incl - cnt;
        if (live) gt_off[i] = min(off, truths_rows);
        const unsigned* __restrict__ src = (const unsigned*)(rows + (size_t)begin * 6);
        for (int j = 0; j < cnt; ++j) {
            const int dst = off + j;
            if (dst < truths_rows)
                for (int c = 0; c < 6; ++c) ((unsigned*)truths)[(size_t)dst * 6 + c] = src[j * 6 + c];
        }
        __syncthreads();
        if (tid == PACK_THREADS - 1) carry_sum = csum + incl;
        __syncthreads();
    }
    if (tid == 0) {
        const int total = min(carry_sum, truths_rows);
        gt_off[batch] = total;
        status[0] = n_bad ? 1 : 0;
        status[1] = n_bad;
        status[2] = n_fallback;
        status[3] = total;
    }
}

struct Border3 { float v[3]; };

// 16-byte copies of image n where the buffers allow: the floats [g0, g1) of the batch, a scalar head up to the first
// multiple of 4, float4 in between, a scalar tail.  `vec` is false when a base pointer is not 16-byte aligned.
__device__ inline void copy_image(const float* __restrict__ in, float* __restrict__ out, long g0, long g1, bool vec,
                                  int block, int blocks)
{
    const int tid = threadIdx.x;
    long a0 = g1, a1 = g1;
    if (vec) {
        a0 = min((g0 + 3) / 4 * 4, g1);
        a1 = max(g1 / 4 * 4, a0);
    }
    const float4* __restrict__ s4 = (const float4*)(in + a0);
    float4* __restrict__ d4 = (float4*)(out + a0);
    const long nv = (a1 - a0) / 4;
    for (long k = (long)block * 256 + tid; k < nv; k += (long)blocks * 256) d4[k] = s4[k];
    // what the float4 loop leaves: at most 3 + 3 floats, or the whole image when vec is false
    const long head = a0 - g0, rest = head + (g1 - a1);
    for (long k = (long)block * 256 + tid; k < rest; k += (long)blocks * 256) {
        const long g = k < head ? g0 + k : a1 + (k - head);
        out[g] = in[g];
    }
}

__global__ __launch_bounds__(256) void warp_affine_kernel(const float* __restrict__ in, const Rec* __restrict__ records,
                                                          float* __restrict__ out, int S, int tiles_x, bool vec, Border3 bd)
{
    const int n = blockIdx.y, tid = threadIdx.x;
    const Rec* __restrict__ r = records + n;            // wave-uniform: scalar loads
    const long plane = (long)S * S;
    if (r->flags & 4) {
        copy_image(in, out, (long)n * 3 * plane, (long)(n + 1) * 3 * plane, vec, blockIdx.x, gridDim.x);
        return;
    }
    const double i0 = r->inv[0], i1 = r->inv[1], i2 = r->inv[2], i3 = r->inv[3], i4 = r->inv[4], i5 = r->inv[5];
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x = tile_x * WARP_TW + tid % WARP_TW, y = tile_y * WARP_TH + tid / WARP_TW;
    if (x >= S || y >= S) return;
    const float* __restrict__ src = in + (long)n * 3 * plane;
    float* __restrict__ o = out + (long)n * 3 * plane + (long)y * S + x;
    const double X = (i0 * (double)x + i1 * (double)y) + i2, Y = (i3 * (double)x + i4 * (double)y) + i5;
    const double Sd = S;
    if (!(-1.0 < X && X < Sd && -1.0 < Y && Y < Sd)) {
        o[0] = bd.v[0]; o[plane] = bd.v[1]; o[2 * plane] = bd.v[2];
        return;
    }
    const double flx = floor(X), fly = floor(Y);
    const float fx = (float)(X - flx), fy = (float)(Y - fly);
    const int ix = (int)flx, iy = (int)fly;                     // -1 .. S-1
    const bool x0 = ix >= 0, x1 = ix + 1 < S, y0 = iy >= 0, y1 = iy + 1 < S;
    const long at = (long)iy * S + ix;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* __restrict__ p = src + c * plane;
        const float bc = bd.v[c];
        const float a = (x0 && y0) ? p[at] : bc, b = (x1 && y0) ? p[at + 1] : bc;
        const float cc = (x0 && y1) ? p[at + S] : bc, d = (x1 && y1) ? p[at + S + 1] : bc;
        const float top = a + fx * (b - a), bot = cc + fx * (d - cc);
        o[c * plane] = top + fy * (bot - top);
    }
}

size_t counts_bytes(int batch) { return ctdet::align_up((size_t)batch * 2 * sizeof(int), 256); }

bool in_range(double v, double lo, double hi) { return std::isfinite(v) && lo <= v && v <= hi; }

bool overlap(const void* a, const void* b, size_t bytes)
{
    const size_t x = (size_t)a, y = (size_t)b;
    return x < y + bytes && y < x + bytes;
}

}  // namespace

extern "C" size_t ct_aug_affine_plan_workspace_bytes(int batch, int truths_rows)
{
    if (batch < 1 || truths_rows < 0) return 0;
    return counts_bytes(batch) + (size_t)truths_rows * 6 * sizeof(float);
}

extern "C" int ct_aug_affine_plan(const float* truths_in, const int* gt_off_in, const unsigned long long* image_ids,
                                  int batch, int truths_rows, int size, unsigned long long seed,
                                  const ct_affine_params* params, ct_affine_record* records_out, float* truths_out,
                                  int* gt_off_out, int* status, void* workspace, size_t workspace_bytes,
                                  ct_stream_t stream)
{
    CT_REQUIRE(truths_in && gt_off_in && image_ids && params && records_out && truths_out && gt_off_out && status && workspace,
               "ct_aug_affine_plan: null pointer");
    CT_REQUIRE(batch >= 1 && batch <= 65535 && size >= 2 && size <= 16384 && truths_rows >= 0,
               "ct_aug_affine_plan: batch=%d size=%d truths_rows=%d", batch, size, truths_rows);
    const ct_affine_params P = *params;
    CT_REQUIRE(in_range(P.rot_half_tan, 0.0, 1.0), "ct_aug_affine_plan: rot_half_tan=%g outside 0..1", P.rot_half_tan);
    CT_REQUIRE(in_range(P.scale_lo, 0.0, 4.0) && P.scale_lo > 0.0 && in_range(P.scale_hi, P.scale_lo, 4.0),
               "ct_aug_affine_plan: scale %g..%g, not 0 < lo <= hi <= 4", P.scale_lo, P.scale_hi);
    CT_REQUIRE(in_range(P.shear_tan, 0.0, 0.5), "ct_aug_affine_plan: shear_tan=%g outside 0..0.5", P.shear_tan);
    CT_REQUIRE(in_range(P.translate, 0.0, 0.5), "ct_aug_affine_plan: translate=%g outside 0..0.5", P.translate);
    CT_REQUIRE(in_range(P.p, 0.0, 1.0) && in_range(P.min_side, 0.0, 1.0) && in_range(P.min_visible, 0.0, 1.0),
               "ct_aug_affine_plan: p=%g min_side=%g min_visible=%g, each 0..1", (double)P.p, (double)P.min_side,
               (double)P.min_visible);
    const size_t row_bytes = (size_t)truths_rows * 6 * sizeof(float);
    CT_REQUIRE(!overlap(truths_in, truths_out, row_bytes), "ct_aug_affine_plan: truths_in and truths_out overlap");
    CT_REQUIRE(workspace_bytes >= ct_aug_affine_plan_workspace_bytes(batch, truths_rows),
               "ct_aug_affine_plan: workspace of %zu bytes, %zu needed", workspace_bytes,
               ct_aug_affine_plan_workspace_bytes(batch, truths_rows));
    CT_REQUIRE(((size_t)workspace & 15) == 0, "ct_aug_affine_plan: workspace is not 16-byte aligned");
    hipStream_t st = ctdet::as_stream(stream);
    int* counts = (int*)workspace;
    float* rows = (float*)((char*)workspace + counts_bytes(batch));
    {
        CT_PROF("affine_plan_kernel", st);
        hipLaunchKernelGGL(affine_plan_kernel, dim3(batch), dim3(64), 0, st, truths_in, gt_off_in, image_ids, batch,
                           truths_rows, size, seed, P, records_out, counts, rows);
        CT_LAUNCH_CHECK("affine_plan_kernel");
    }
    CT_PROF("affine_pack_kernel", st);
    hipLaunchKernelGGL(affine_pack_kernel, dim3(1), dim3(PACK_THREADS), 0, st, gt_off_in, batch, truths_rows,
                       (const int*)counts, (const float*)rows, truths_out, gt_off_out, status);
    CT_LAUNCH_CHECK("affine_pack_kernel");
    return CT_OK;
}

extern "C" int ct_preproc_warp_affine(const float* in, const ct_affine_record* records, int batch, int size,
                                      const float* border3, float* out, ct_stream_t stream)
{
    CT_REQUIRE(in && records && border3 && out, "ct_preproc_warp_affine: null pointer");
    CT_REQUIRE(batch >= 1 && batch <= 65535 && size >= 2 && size <= 16384, "ct_preproc_warp_affine: batch=%d size=%d", batch,
               size);
    const size_t bytes = (size_t)batch * 3 * size * size * sizeof(float);
    CT_REQUIRE(!overlap(in, out, bytes), "ct_preproc_warp_affine: in and out overlap");
    Border3 bd;
    for (int c = 0; c < 3; ++c) bd.v[c] = border3[c];
    const bool vec = (((size_t)in | (size_t)out) & 15) == 0;
    const int tiles_x = (size + WARP_TW - 1) / WARP_TW, tiles_y = (size + WARP_TH - 1) / WARP_TH;
    hipStream_t st = ctdet::as_stream(stream);
    CT_PROF("warp_affine_kernel", st);
    hipLaunchKernelGGL(warp_affine_kernel, dim3(tiles_x * tiles_y, batch), dim3(256), 0, st, in, records, out, size, tiles_x,
                       vec, bd);
    CT_LAUNCH_CHECK("warp_affine_kernel");
    return CT_OK;
}
