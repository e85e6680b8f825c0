// libctdet: the non-convolution training kernels of the RFBNet stack (part of what autograd + cuDNN do for the reference
// in train.py:222-229): batch-statistics BatchNorm forward / backward, bias+ReLU backward, max-pool backward and the
// head-gradient gather.  The weight gradients of a convolution are in ct_wgrad.hip (direct), ct_wino_wgrad.hip,
// ct_wino4_wgrad.hip and ct_wgrad_h2.hip; its data gradient is the `transposed` mode of ct_conv2d_fwd (ct_conv.hip).
#include "ct_common.h"
#include "ct_device.h"
#include "ct_f16x2.h"
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

// ------------------------------------------------------------------------------------------
// Per-channel reductions of the BatchNorm passes over (batch, h, w) of a channel slice of an NCHW buffer
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* red)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    return t;
}

// Both passes sum two double terms per element of a channel (StatsOp: z, z^2; BwdOp: dy, dy * xhat) with 256 threads.  An Op adds
// the terms of element (n, c, i) and finishes a channel from its two sums; the walk over the elements is one of two:
//   WHOLE (grid = channels): images outer, i = tid, tid + 256, ... inside each image; the block finishes its channel in place.
//   SLICE (grid = channels x slices, most of the chip would idle otherwise): e = e0 + tid, e0 + tid + 256, ... over slice blockIdx.y
//     of the flat batch*HW range.  The block sums meet in `scratch` ([2][C] doubles, zeroed by the host entry) through f64 atomics;
//     det: slice y STORES them at scratch[y][2][C] instead (nothing zeroed).  The *_final_kernel adds the records in slice order.
// A thread's partial sums differ between the walks whenever HW % 256 != 0: one walk for both would move result bits.
enum class Walk { WHOLE, SLICE };

template <Walk WALK, class Op>
__device__ __forceinline__ void bn_reduce(Op op, int batch, int C, int HW, int per_slice, double* __restrict__ scratch, int det)
{
    __shared__ double red[4];
    const int c = blockIdx.x;
    op.channel(c);
    double s0 = 0.0, s1 = 0.0;
    if (WALK == Walk::WHOLE) {
        for (int n = 0; n < batch; ++n)
            for (int i = threadIdx.x; i < HW; i += 256) op.add(n, c, i, s0, s1);
    } else {
        const long e0 = (long)blockIdx.y * per_slice, e1 = min(e0 + per_slice, (long)batch * HW);
        for (long e = e0 + threadIdx.x; e < e1; e += 256) {
            const int n = (int)(e / HW);
            op.add(n, c, (int)(e - (long)n * HW), s0, s1);
        }
    }
    s0 = block_sum(s0, red);
    s1 = block_sum(s1, red);
    if (threadIdx.x != 0) return;
    if (WALK == Walk::WHOLE) {
        op.finish(c, s0, s1);
    } else if (det) {
        scratch[(size_t)blockIdx.y * 2 * C + c] = s0;
        scratch[(size_t)blockIdx.y * 2 * C + C + c] = s1;
    } else {
        unsafeAtomicAdd(&scratch[c], s0);
        unsafeAtomicAdd(&scratch[C + c], s1);
    }
}

// the two sums of channel c over `slices` records [2][C] (one for the atomic path), in slice order
__device__ __forceinline__ void slice_sums(const double* __restrict__ scratch, int C, int slices, int c, double& s0, double& s1)
{
    s0 = scratch[c];
    s1 = scratch[C + c];
#pragma unroll 4
    for (int y = 1; y < slices; ++y) {
        s0 += scratch[(size_t)y * 2 * C + c];
        s1 += scratch[(size_t)y * 2 * C + C + c];
    }
}

template <class Op>
__device__ __forceinline__ void bn_reduce_final(const Op& op, const double* __restrict__ scratch, int slices, int C)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s0, s1;
    slice_sums(scratch, C, slices, c, s0, s1);
    op.finish(c, s0, s1);
}

// BatchNorm2d training statistics of channels [coff, coff + C) of z
struct StatsOp {
    const float* z;
    float *mean, *var;
    float *rmean, *rvar;     // running statistics of nn.BatchNorm2d (momentum, unbiased variance), same launch; or null
    double cnt;              // batch * HW
    int batch, ctot, coff, C, HW;
    float momentum, unbias;

    __device__ void channel(int) {}
    __device__ void add(int n, int c, int i, double& s, double& ss) const
    {
        const double v = z[((size_t)n * ctot + coff + c) * HW + i];
        s += v;
        ss += v * v;
    }
    __device__ void finish(int c, double s, double ss) const
    {
        const double m = s / cnt;
        const float mf = (float)m, vf = (float)fmax(ss / cnt - m * m, 0.0);   // biased variance (normalisation)
        mean[c] = mf;
        var[c] = vf;
        if (rmean) {
            rmean[c] = (1.f - momentum) * rmean[c] + momentum * mf;
            rvar[c] = (1.f - momentum) * rvar[c] + momentum * (vf * unbias);
        }
    }
};

__global__ __launch_bounds__(256) void bn_stats_kernel(const StatsOp op) { bn_reduce<Walk::WHOLE>(op, op.batch, op.C, op.HW, 0, nullptr, 0); }
__global__ __launch_bounds__(256) void bn_stats_part_kernel(const StatsOp op, int per_slice, double* __restrict__ scratch, int det)
{
    bn_reduce<Walk::SLICE>(op, op.batch, op.C, op.HW, per_slice, scratch, det);
}
__global__ void bn_stats_final_kernel(const StatsOp op, const double* __restrict__ scratch, int slices) { bn_reduce_final(op, scratch, slices, op.C); }

// The synchronized (cross-rank) forms split a pass into local sums, a collective the caller runs on them, and a finish.  SumsOp
// gives a reduction the terms of Inner, but a channel ends as its two double sums at sums[2][C]; KEEP also runs Inner's finish
// on those local sums (the backward's parameter gradients, which the gradient all-reduce averages).
template <class Inner, bool KEEP>
struct SumsOp {
    Inner in;
    double* sums;
    int C;

    __device__ void channel(int c) { in.channel(c); }
    __device__ void add(int n, int c, int i, double& s0, double& s1) const { in.add(n, c, i, s0, s1); }
    __device__ void finish(int c, double s0, double s1) const
    {
        sums[c] = s0;
        sums[C + c] = s1;
        if (KEEP) in.finish(c, s0, s1);
    }
};

struct BnSyncStatsArgs {
    StatsOp op;              // z and its slicing; nothing of `finish` is used
    double* sums;
};
using SyncStatsOp = SumsOp<StatsOp, false>;

__global__ __launch_bounds__(256) void bn_sync_stats_kernel(const BnSyncStatsArgs s)
{
    bn_reduce<Walk::WHOLE>(SyncStatsOp{s.op, s.sums, s.op.C}, s.op.batch, s.op.C, s.op.HW, 0, nullptr, 0);
}
__global__ __launch_bounds__(256) void bn_sync_stats_part_kernel(const BnSyncStatsArgs s, int per_slice, double* __restrict__ scratch, int det)
{
    bn_reduce<Walk::SLICE>(SyncStatsOp{s.op, s.sums, s.op.C}, s.op.batch, s.op.C, s.op.HW, per_slice, scratch, det);
}
__global__ void bn_sync_stats_final_kernel(const BnSyncStatsArgs s, const double* __restrict__ scratch, int slices)
{
    bn_reduce_final(SyncStatsOp{s.op, s.sums, s.op.C}, scratch, slices, s.op.C);
}
// mean, variance and running statistics from the reduced sums: StatsOp::finish with the global count, on ONE record
__global__ void bn_sync_finish_kernel(const StatsOp op, const double* __restrict__ sums) { bn_reduce_final(op, sums, 1, op.C); }

struct BnApplyArgs {
    const float* z;          // conv output, channel slice [z_coff, z_coff+C) of z_ctot
    const float* mean;
    const float* var;
    const float* gamma;
    const float* beta;
    const float* lo;         // per-channel clamp (0 / -inf) or null
    const float* res;        // residual slice or null
    float* y;
    int batch, C, HW, y_ctot, y_coff, res_ctot, res_coff, z_ctot, z_coff;
    float eps, rscale;
    int relu;
};

__global__ __launch_bounds__(256) void bn_apply_kernel(const BnApplyArgs a)
{
    const long total = (long)a.batch * a.C * a.HW;
    for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < (unsigned)total; idx += gridDim.x * blockDim.x) {
        const int i = (int)(idx % a.HW);
        const unsigned t = idx / a.HW;
        const int c = (int)(t % a.C);
        const int n = (int)(t / a.C);
        const float inv = 1.f / sqrtf(a.var[c] + a.eps);
        float v = (a.z[((size_t)n * a.z_ctot + a.z_coff + c) * a.HW + i] - a.mean[c]) * inv * a.gamma[c] + a.beta[c];
        if (a.res) v = v * a.rscale + a.res[((size_t)n * a.res_ctot + a.res_coff + c) * a.HW + i];
        if (a.lo) v = fmaxf(v, a.lo[c]);
        else if (a.relu) v = fmaxf(v, 0.f);
        a.y[((size_t)n * a.y_ctot + a.y_coff + c) * a.HW + i] = v;
    }
}

struct BnBwdArgs {
    const float* dy;         // slice of the consumer-side gradient buffer
    const float* y;          // slice of the forward output (ReLU mask) or null
    const float* z;          // conv output slice (z_ctot / z_coff); dz uses the same slicing
    const float* mean;
    const float* var;
    const float* gamma;
    const float* lo;
    float* dz;               // dense
    float* dgamma;
    float* dbeta;
    float* dres;             // where the residual branch's gradient goes (slice) or null
    int batch, C, HW, dy_ctot, dy_coff, y_ctot, y_coff, dres_ctot, dres_coff, dres_accumulate, z_ctot, z_coff;
    float eps, rscale;
    int relu;
    int frozen;              // 1: mean/var are constants (nn.BatchNorm2d in eval mode): no statistics terms in dz
};

__device__ __forceinline__ float masked_dy(const BnBwdArgs& a, int n, int c, int i)
{
    float g = a.dy[((size_t)n * a.dy_ctot + a.dy_coff + c) * a.HW + i];
    const bool act = a.lo ? (a.lo[c] == 0.f) : (a.relu != 0);
    if (act && a.y[((size_t)n * a.y_ctot + a.y_coff + c) * a.HW + i] <= 0.f) g = 0.f;
    return g;
}

// dbeta = sum of the masked, scaled dy; dgamma = sum of that times the normalised z
struct BwdOp {
    const BnBwdArgs& a;
    float inv, mu;

    __device__ void channel(int c) { inv = 1.f / sqrtf(a.var[c] + a.eps); mu = a.mean[c]; }
    __device__ void add(int n, int c, int i, double& sb, double& sg) const
    {
        const float g = masked_dy(a, n, c, i) * a.rscale;
        sb += g;
        sg += (double)g * ((a.z[((size_t)n * a.z_ctot + a.z_coff + c) * a.HW + i] - mu) * inv);
    }
    __device__ void finish(int c, double sb, double sg) const { a.dbeta[c] = (float)sb; a.dgamma[c] = (float)sg; }
};

__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const BnBwdArgs a) { bn_reduce<Walk::WHOLE>(BwdOp{a}, a.batch, a.C, a.HW, 0, nullptr, 0); }
__global__ __launch_bounds__(256) void bn_bwd_reduce_part_kernel(const BnBwdArgs a, int per_slice, double* __restrict__ scratch, int det)
{
    bn_reduce<Walk::SLICE>(BwdOp{a}, a.batch, a.C, a.HW, per_slice, scratch, det);
}
__global__ void bn_bwd_reduce_final_kernel(const BnBwdArgs a, const double* __restrict__ scratch, int slices) { bn_reduce_final(BwdOp{a}, scratch, slices, a.C); }

// dz (and the residual branch's gradient) of every element.  G gives the two sums of the statistics terms and their divisor: the
// layer's own dbeta / dgamma and element count, or the cross-rank sums and the global count of the synchronized form.  The kernel
// passes its grid-stride loop's first index and stride.
template <class G>
__device__ __forceinline__ void bn_bwd_apply(const BnBwdArgs& a, const G grads, unsigned first, unsigned stride)
{
    const long total = (long)a.batch * a.C * a.HW;
    const float cnt = grads.count();
    for (unsigned idx = first; idx < (unsigned)total; idx += stride) {
        const int i = (int)(idx % a.HW);
        const unsigned t = idx / a.HW;
        const int c = (int)(t % a.C);
        const int n = (int)(t / a.C);
        const float inv = 1.f / sqrtf(a.var[c] + a.eps);
        const float gm = masked_dy(a, n, c, i);
        if (a.dres) {
            float* d = a.dres + ((size_t)n * a.dres_ctot + a.dres_coff + c) * a.HW + i;
            *d = a.dres_accumulate ? *d + gm : gm;
        }
        const float g = gm * a.rscale;
        const size_t zi = ((size_t)n * a.z_ctot + a.z_coff + c) * a.HW + i;
        const float xh = (a.z[zi] - a.mean[c]) * inv;
        a.dz[zi] = a.frozen ? a.gamma[c] * inv * g
                            : a.gamma[c] * inv * (g - grads.dbeta(c) / cnt - xh * grads.dgamma(c) / cnt);
    }
}

struct OwnGrads {
    const BnBwdArgs& a;
    __device__ float count() const { return (float)a.batch * a.HW; }
    __device__ float dbeta(int c) const { return a.dbeta[c]; }
    __device__ float dgamma(int c) const { return a.dgamma[c]; }
};
struct ReducedGrads {
    const double* sums;      // [2][C]: sum g, sum g * xhat over every rank's shard
    double cnt;
    int C;
    __device__ float count() const { return (float)cnt; }
    __device__ float dbeta(int c) const { return (float)sums[c]; }
    __device__ float dgamma(int c) const { return (float)sums[C + c]; }
};

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const BnBwdArgs a)
{
    bn_bwd_apply(a, OwnGrads{a}, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

struct BnSyncBwdArgs {
    BnBwdArgs a;
    double* sums;
};
using SyncBwdOp = SumsOp<BwdOp, true>;

__global__ __launch_bounds__(256) void bn_sync_bwd_kernel(const BnSyncBwdArgs s)
{
    bn_reduce<Walk::WHOLE>(SyncBwdOp{BwdOp{s.a}, s.sums, s.a.C}, s.a.batch, s.a.C, s.a.HW, 0, nullptr, 0);
}
__global__ __launch_bounds__(256) void bn_sync_bwd_part_kernel(const BnSyncBwdArgs s, int per_slice, double* __restrict__ scratch, int det)
{
    bn_reduce<Walk::SLICE>(SyncBwdOp{BwdOp{s.a}, s.sums, s.a.C}, s.a.batch, s.a.C, s.a.HW, per_slice, scratch, det);
}
__global__ void bn_sync_bwd_final_kernel(const BnSyncBwdArgs s, const double* __restrict__ scratch, int slices)
{
    bn_reduce_final(SyncBwdOp{BwdOp{s.a}, s.sums, s.a.C}, scratch, slices, s.a.C);
}
__global__ __launch_bounds__(256) void bn_sync_bwd_apply_kernel(const BnBwdArgs a, const double* __restrict__ sums, double count)
{
    bn_bwd_apply(a, ReducedGrads{sums, count, a.C}, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// The tail of the two bias backward kernels: the block's share of dbias[c] is stored at slab[slot][C] (deterministic mode:
// dbias_slab_sum_kernel adds the slots in order), else it joins dbias[c] through one float atomic.
__device__ __forceinline__ void dbias_sink(double sb, double* red, int c, int C, int slot, float* __restrict__ dbias,
                                           double* __restrict__ slab)
{
    sb = block_sum(sb, red);
    if (threadIdx.x == 0 && dbias) {
        if (slab) slab[(size_t)slot * C + c] = sb;
        else unsafeAtomicAdd(&dbias[c], (float)sb);
    }
}

// y = act(conv + bias):  dz = dy * (y > 0 if relu),  dbias = sum dz   (VGG convs, heads)
// grid (channel, slice): a slice is a contiguous range of the channel's batch*HW elements, so a 64-channel
// 300x300 layer still fills the chip; per-slice sums meet in dbias through one float atomic per block -- or, with `slab`, are
// stored as doubles at slab[slice][C] for dbias_slab_sum_kernel to add in order.
__global__ __launch_bounds__(256) void bias_act_bwd_kernel(const float* __restrict__ dy, int dy_ctot,
                                                           int dy_coff, const float* __restrict__ y,
                                                           int y_ctot, int y_coff, int relu, int batch,
                                                           int C, int HW, float* __restrict__ dz,
                                                           int dz_ctot, int dz_coff,
                                                           float* __restrict__ dbias, int per_slice,
                                                           unsigned* __restrict__ amax, double* __restrict__ slab)
{
    __shared__ double red[4];
    const int c = blockIdx.x;
    const long e0 = (long)blockIdx.y * per_slice, e1 = min(e0 + per_slice, (long)batch * HW);
    double sb = 0.0;
    const bool vec = (HW & 3) == 0 && (per_slice & 3) == 0;
    int n = (int)(e0 / HW);
    int i0 = (int)(e0 - (long)n * HW);
    for (long e = e0; e < e1;) {
        const int len = (int)min((long)(HW - i0), e1 - e);
        const float* g = dy + ((size_t)n * dy_ctot + dy_coff + c) * HW + i0;
        const float* yy = y ? y + ((size_t)n * y_ctot + y_coff + c) * HW + i0 : nullptr;
        float* o = dz + ((size_t)n * dz_ctot + dz_coff + c) * HW + i0;
        float run = 0.f;                 // max |dz| of what this thread stores for image n (ct_f16x2.h: the f16x2 data gradients)
        if (vec) {
            for (int i = threadIdx.x * 4; i < len; i += 1024) {
                float4 v = *reinterpret_cast<const float4*>(g + i);
                if (relu) {
                    const float4 t = *reinterpret_cast<const float4*>(yy + i);
                    v.x = t.x <= 0.f ? 0.f : v.x;
                    v.y = t.y <= 0.f ? 0.f : v.y;
                    v.z = t.z <= 0.f ? 0.f : v.z;
                    v.w = t.w <= 0.f ? 0.f : v.w;
                }
                *reinterpret_cast<float4*>(o + i) = v;
                sb += (double)((v.x + v.y) + (v.z + v.w));
                ctdet::h2::track_absmax(run, v.x);
                ctdet::h2::track_absmax(run, v.y);
                ctdet::h2::track_absmax(run, v.z);
                ctdet::h2::track_absmax(run, v.w);
            }
        } else {
            for (int i = threadIdx.x; i < len; i += 256) {
                float v = g[i];
                if (relu && yy[i] <= 0.f) v = 0.f;
                o[i] = v;
                sb += v;
                ctdet::h2::track_absmax(run, v);
            }
        }
        if (amax) ctdet::h2::flush_absmax(amax, n, run);         // uniform over the block: every lane is in the same image
        e += len;
        i0 = 0;
        ++n;
    }
    dbias_sink(sb, red, c, C, blockIdx.y, dbias, slab);
}

// dbias[c] = the `nslabs` partial sums slab[.][C] of channel c added in slab order (bias + activation backward: one per
// slice; fused pool backward: one per image)
__global__ void dbias_slab_sum_kernel(const double* __restrict__ slab, int nslabs, int C, float* __restrict__ dbias)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = slab[c];
#pragma unroll 8
    for (int y = 1; y < nslabs; ++y) s += slab[(size_t)y * C + c];       // loads issued in groups, additions in slab order
    dbias[c] = (float)s;
}

// max-pool backward (gather form): every input element collects dy of the windows whose FIRST
// maximum (row-major scan, torch's tie rule) it is.
__global__ __launch_bounds__(256) void maxpool2d_bwd_kernel(const float* __restrict__ x,
                                                            const float* __restrict__ dy,
                                                            float* __restrict__ dx, long planes, int H,
                                                            int W, int OH, int OW, int k, int stride,
                                                            int pad, int accumulate)
{
    const long total = planes * H * W;
    for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < (unsigned)total; idx += gridDim.x * blockDim.x) {
        const int w = (int)(idx % W);
        const unsigned t = idx / W;
        const int h = (int)(t % H);
        const long pl = t / H;
        const float* xp = x + pl * (long)H * W;
        const float* gp = dy + pl * (long)OH * OW;
        float g = 0.f;
        const int oh_lo = max(0, (h + pad - k + stride) / stride), oh_hi = min(OH - 1, (h + pad) / stride);
        const int ow_lo = max(0, (w + pad - k + stride) / stride), ow_hi = min(OW - 1, (w + pad) / stride);
        for (int oh = oh_lo; oh <= oh_hi; ++oh)
            for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                const int h0 = oh * stride - pad, w0 = ow * stride - pad;
                float m = -INFINITY;
                int mh = -1, mw = -1;
                for (int hh = max(h0, 0); hh < min(h0 + k, H); ++hh)
                    for (int ww = max(w0, 0); ww < min(w0 + k, W); ++ww) {
                        const float v = xp[(long)hh * W + ww];
                        if (v > m) { m = v; mh = hh; mw = ww; }
                    }
                if (mh == h && mw == w) g += gp[(long)oh * OW + ow];
            }
        dx[idx] = accumulate ? dx[idx] + g : g;
    }
}

// The same for planes that fit in LDS (pool5: 3x3 / stride 1 on 19x19 or 32x32 -- 81 global reads per element in the kernel
// above, 492 us of the bs-32 training step): workgroup = one plane; the plane goes to LDS once, every window's first maximum
// is found once (its flat index), every element then sums dy over the <= k*k windows that name it.  Same tie rule, same sum
// order (windows in row-major order) as the kernel above.
constexpr int kPoolPlaneMax = 4096;
__global__ __launch_bounds__(256) void maxpool2d_bwd_plane_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                  float* __restrict__ dx, int H, int W, int OH, int OW,
                                                                  int k, int stride, int pad, int accumulate)
{
    __shared__ float xs[kPoolPlaneMax];
    __shared__ int am[kPoolPlaneMax];
    const long pl = blockIdx.x;
    const float* xp = x + pl * (long)H * W;
    const float* gp = dy + pl * (long)OH * OW;
    float* dp = dx + pl * (long)H * W;
    for (int i = threadIdx.x; i < H * W; i += 256) xs[i] = xp[i];
    __syncthreads();
    for (int o = threadIdx.x; o < OH * OW; o += 256) {
        const int oh = o / OW, ow = o - oh * OW;
        const int h0 = oh * stride - pad, w0 = ow * stride - pad;
        float m = -INFINITY;
        int mi = -1;
        for (int hh = max(h0, 0); hh < min(h0 + k, H); ++hh)
            for (int ww = max(w0, 0); ww < min(w0 + k, W); ++ww) {
                const float v = xs[hh * W + ww];
                if (v > m) { m = v; mi = hh * W + ww; }
            }
        am[o] = mi;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < H * W; i += 256) {
        const int h = i / W, w = i - h * W;
        float g = 0.f;
        const int oh_lo = max(0, (h + pad - k + stride) / stride), oh_hi = min(OH - 1, (h + pad) / stride);
        const int ow_lo = max(0, (w + pad - k + stride) / stride), ow_hi = min(OW - 1, (w + pad) / stride);
        for (int oh = oh_lo; oh <= oh_hi; ++oh)
            for (int ow = ow_lo; ow <= ow_hi; ++ow)
                if (am[oh * OW + ow] == i) g += gp[oh * OW + ow];
        dp[i] = accumulate ? dp[i] + g : g;
    }
}

// MaxPool2d(2, 2) (floor or ceil mode): the windows do not overlap, so one thread owns one window -- reads its
// (up to) 2x2 inputs, finds the first maximum in row-major order (strict >, as the gather kernel above) and
// writes all four gradients; input rows/columns no window covers (floor mode, odd extent) get zeros.
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ dy,
                                                             float* __restrict__ dx, int H, int W, int OH, int OW,
                                                             int accumulate)
{
    const int WH = (H + 1) >> 1, WW = (W + 1) >> 1;
    const float* xp = x + (size_t)blockIdx.x * H * W;
    float* dp = dx + (size_t)blockIdx.x * H * W;
    const float* gp = dy + (size_t)blockIdx.x * OH * OW;
    for (unsigned idx = threadIdx.x; idx < (unsigned)(WH * WW); idx += 256) {
        const int wh = idx / (unsigned)WW, ww = idx - wh * WW;
        const int h0 = 2 * wh, w0 = 2 * ww;
        const bool h1 = h0 + 1 < H, w1 = w0 + 1 < W;
        const float g = (wh < OH && ww < OW) ? gp[wh * OW + ww] : 0.f;
        const int o = h0 * W + w0;
        const float v00 = xp[o];
        const float v01 = w1 ? xp[o + 1] : -INFINITY;
        const float v10 = h1 ? xp[o + W] : -INFINITY;
        const float v11 = (h1 && w1) ? xp[o + W + 1] : -INFINITY;
        int sel = -1;
        float m = -INFINITY;
        if (v00 > m) { m = v00; sel = 0; }
        if (v01 > m) { m = v01; sel = 1; }
        if (v10 > m) { m = v10; sel = 2; }
        if (v11 > m) { m = v11; sel = 3; }
        const float g0 = sel == 0 ? g : 0.f, g1 = sel == 1 ? g : 0.f, g2 = sel == 2 ? g : 0.f, g3 = sel == 3 ? g : 0.f;
        if (accumulate) {
            dp[o] += g0;
            if (w1) dp[o + 1] += g1;
            if (h1) dp[o + W] += g2;
            if (h1 && w1) dp[o + W + 1] += g3;
        } else {
            dp[o] = g0;
            if (w1) dp[o + 1] = g1;
            if (h1) dp[o + W] = g2;
            if (h1 && w1) dp[o + W + 1] = g3;
        }
    }
}

// MaxPool2d(2, 2) backward FUSED with the bias + ReLU backward of the convolution that feeds the pool (conv1_2 / conv2_2 /
// conv3_3 of the VGG trunk: the pool is the only reader of their output): dz = (y > 0) * [this element is the first maximum of its
// window] * dy_pool, dbias[c] = sum dz, max |dz| per image -- the pool's input gradient (as large as the activation) is never
// written and read back, and y is read once instead of twice: 2.2 GB less per step on 64 x 300 x 300 x 32.  One block per (n, c) plane.
__global__ __launch_bounds__(256) void maxpool2x2_bias_relu_bwd_kernel(const float* __restrict__ y, int y_ctot, int y_coff,
                                                                       const float* __restrict__ dy, int C, int H, int W,
                                                                       int OH, int OW, float* __restrict__ dz, int dz_ctot,
                                                                       int dz_coff, float* __restrict__ dbias,
                                                                       unsigned* __restrict__ amax, double* __restrict__ slab)
{
    __shared__ double red[4];
    const int n = blockIdx.x / C, c = blockIdx.x - n * C;
    const int WH = (H + 1) >> 1, WW = (W + 1) >> 1;
    const float* xp = y + ((size_t)n * y_ctot + y_coff + c) * H * W;
    float* dp = dz + ((size_t)n * dz_ctot + dz_coff + c) * H * W;
    const float* gp = dy + (size_t)blockIdx.x * OH * OW;
    double sb = 0.0;
    float run = 0.f;
    for (unsigned idx = threadIdx.x; idx < (unsigned)(WH * WW); idx += 256) {
        const int wh = idx / (unsigned)WW, ww = idx - wh * WW;
        const int h0 = 2 * wh, w0 = 2 * ww;
        const bool h1 = h0 + 1 < H, w1 = w0 + 1 < W;
        const float g = (wh < OH && ww < OW) ? gp[wh * OW + ww] : 0.f;
        const int o = h0 * W + w0;
        const float v00 = xp[o];
        const float v01 = w1 ? xp[o + 1] : -INFINITY;
        const float v10 = h1 ? xp[o + W] : -INFINITY;
        const float v11 = (h1 && w1) ? xp[o + W + 1] : -INFINITY;
        int sel = -1;
        float m = -INFINITY;
        if (v00 > m) { m = v00; sel = 0; }
        if (v01 > m) { m = v01; sel = 1; }
        if (v10 > m) { m = v10; sel = 2; }
        if (v11 > m) { m = v11; sel = 3; }
        const float gm = m <= 0.f ? 0.f : g;               // ReLU: the selected element passes its gradient only where y > 0
        dp[o] = sel == 0 ? gm : 0.f;
        if (w1) dp[o + 1] = sel == 1 ? gm : 0.f;
        if (h1) dp[o + W] = sel == 2 ? gm : 0.f;
        if (h1 && w1) dp[o + W + 1] = sel == 3 ? gm : 0.f;
        sb += (double)gm;
        ctdet::h2::track_absmax(run, gm);
    }
    if (amax) ctdet::h2::flush_absmax(amax, n, run);
    dbias_sink(sb, red, c, C, n, dbias, slab);          // one partial sum per image, added in image order
}

// gradient of the channels-last head scatter: dz[n][co][pix] = dflat[n*img_stride + base + pix*ps + (co-co0)]
struct HeadGatherArgs {
    ct_out_segment seg[3];
    int nseg;
    float* dz;
    int batch, C, HW;
};

__global__ __launch_bounds__(256) void head_grad_gather_kernel(const HeadGatherArgs a)
{
    const long total = (long)a.batch * a.C * a.HW;
    for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < (unsigned)total; idx += gridDim.x * blockDim.x) {
        const int i = (int)(idx % a.HW);
        const unsigned t = idx / a.HW;
        const int c = (int)(t % a.C);
        const int n = (int)(t / a.C);
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < 3; ++g)
            if (g < a.nseg && c >= a.seg[g].co_begin && c < a.seg[g].co_end)
                v = a.seg[g].ptr[(size_t)n * a.seg[g].img_stride + a.seg[g].base +
                                 (size_t)i * a.seg[g].pix_stride + (c - a.seg[g].co_begin)];
        a.dz[idx] = v;
    }
}

// The element-wise kernels above walk an `unsigned idx` grid-stride loop.  `idx += gridDim.x * blockDim.x` is 32-bit
// arithmetic: with a total within one grid stride of 2^32 the last step would wrap idx to a small value and the loop
// would never end, so their entry points refuse totals above kMaxLoopElems (2^32 minus the largest stride grid_for gives).
constexpr long kGridMaxBlocks = 256 * 16;
constexpr long kMaxLoopElems = 0x100000000L - kGridMaxBlocks * 256;
inline int grid_for(long total) { return (int)std::min<long>((total + 255) / 256, kGridMaxBlocks); }

}  // namespace

// slices of a channel's batch*hw elements in the BatchNorm reductions (both passes)
static int bn_slices(int batch, int channels, int hw)
{
    const long per_channel = (long)batch * hw;
    return (int)std::max<long>(1, std::min<long>((1024 + channels - 1) / channels, per_channel / 2048));
}

// the scratch of a _det reduction: `slices` records of `per_slice_bytes`, 8-byte aligned
static int det_scratch_check(const char* who, const void* scratch, size_t have, size_t need)
{
    CT_REQUIRE(scratch, "%s: scratch is null", who);
    CT_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "%s: scratch must be 8-byte aligned", who);
    if (have < need) return ctdet::fail(CT_ERR_WORKSPACE, "%s: scratch_bytes %zu, needs %zu", who, have, need);
    return CT_OK;
}

// the three kernels of one BatchNorm reduction (each takes the arguments A first) and the names their launch checks report
template <class A>
struct BnReduction {
    void (*whole)(A);
    void (*part)(A, int per_slice, double* scratch, int det);
    void (*fin)(A, const double* scratch, int slices);
    const char *whole_name, *part_name, *fin_name;
};

// One reduction: sliced (part + final launch) when there is a scratch and more than one slice, else one block per channel.  The
// atomic path zeroes its [2][C] record unless the caller has (ct_scratch_prezeroed); det stores `slices` records, zeroes nothing.
template <class A>
static int bn_reduce_launch(const char* who, const BnReduction<A>& k, const A& a, int batch, int channels, int hw, void* scratch,
                            bool det, size_t scratch_bytes, hipStream_t st)
{
    const long per_channel = (long)batch * hw;
    const int slices = bn_slices(batch, channels, hw);
    if (det && slices > 1)
        if (int rc = det_scratch_check(who, scratch, scratch_bytes, (size_t)slices * 2 * channels * sizeof(double))) return rc;
    if (!scratch || slices == 1) {
        hipLaunchKernelGGL(k.whole, dim3(channels), dim3(256), 0, st, a);
        CT_LAUNCH_CHECK(k.whole_name);
        return CT_OK;
    }
    const int per_slice = (int)((per_channel + slices - 1) / slices);
    if (!det && !ctdet::scratch_prezeroed()) CT_HIP(hipMemsetAsync(scratch, 0, (size_t)2 * channels * sizeof(double), st));
    hipLaunchKernelGGL(k.part, dim3(channels, slices), dim3(256), 0, st, a, per_slice, (double*)scratch, (int)det);
    CT_LAUNCH_CHECK(k.part_name);
    hipLaunchKernelGGL(k.fin, dim3((channels + 255) / 256), dim3(256), 0, st, a, (const double*)scratch, det ? slices : 1);
    CT_LAUNCH_CHECK(k.fin_name);
    return CT_OK;
}

static int bn_stats_impl(const char* who, const float* z, int batch, int ctot, int coff, int channels, int hw,
                         float* mean, float* var, float momentum, float* running_mean,
                         float* running_var, void* scratch, bool det, size_t scratch_bytes, ct_stream_t stream)
{
    CT_REQUIRE(z && mean && var && batch > 0 && channels > 0 && hw > 0, "%s: bad arguments", who);
    const bool run = running_mean && running_var;
    const float cntf = (float)batch * hw;
    StatsOp op{};
    op.z = z; op.mean = mean; op.var = var; op.rmean = run ? running_mean : nullptr; op.rvar = run ? running_var : nullptr;
    op.cnt = (double)((long)batch * hw); op.batch = batch; op.ctot = ctot; op.coff = coff; op.C = channels; op.HW = hw;
    op.momentum = momentum; op.unbias = cntf > 1.f ? cntf / (cntf - 1.f) : 1.f;
    static const BnReduction<StatsOp> kernels{bn_stats_kernel, bn_stats_part_kernel, bn_stats_final_kernel,
                                              "bn_stats_kernel", "bn_stats_part_kernel", "bn_stats_final_kernel"};
    return bn_reduce_launch(who, kernels, op, batch, channels, hw, scratch, det, scratch_bytes, ctdet::as_stream(stream));
}

extern "C" int ct_bn_train_stats(const float* z, int batch, int ctot, int coff, int channels, int hw,
                                 float* mean, float* var, float momentum, float* running_mean,
                                 float* running_var, void* scratch, ct_stream_t stream)
{
    return bn_stats_impl("ct_bn_train_stats", z, batch, ctot, coff, channels, hw, mean, var, momentum, running_mean, running_var,
                         scratch, false, 0, stream);
}

extern "C" size_t ct_bn_det_scratch_bytes(int batch, int channels, int hw, int* partials)
{
    if (partials) *partials = 0;
    if (batch <= 0 || channels <= 0 || hw <= 0) return 0;
    if (partials) *partials = bn_slices(batch, channels, hw);
    // slices * channels records of two doubles, bounded from above by an expression that grows with batch and with channels
    // (slices * channels itself does not: 2 x 513 > 1 x 1024)
    const long per_channel = (long)batch * hw;
    const long records = std::max<long>(channels, std::min<long>(1023L + channels, (long)channels * std::max<long>(1, per_channel / 2048)));
    return (size_t)records * 2 * sizeof(double);
}

extern "C" int ct_bn_train_stats_det(const float* z, int batch, int ctot, int coff, int channels, int hw,
                                     float* mean, float* var, float momentum, float* running_mean,
                                     float* running_var, void* scratch, size_t scratch_bytes, ct_stream_t stream)
{
    return bn_stats_impl("ct_bn_train_stats_det", z, batch, ctot, coff, channels, hw, mean, var, momentum, running_mean, running_var,
                         scratch, true, scratch_bytes, stream);
}

extern "C" int ct_bn_train_apply(const float* z, const float* mean, const float* var, const float* gamma,
                                 const float* beta, float eps, int relu, const float* lo, const float* res,
                                 int res_ctot, int res_coff, float res_scale, float* y, int y_ctot,
                                 int y_coff, int z_ctot, int z_coff, int batch, int channels, int hw,
                                 ct_stream_t stream)
{
    CT_REQUIRE(z && mean && var && gamma && beta && y, "ct_bn_train_apply: null pointer");
    BnApplyArgs a{};
    a.z = z; a.mean = mean; a.var = var; a.gamma = gamma; a.beta = beta; a.lo = lo; a.res = res; a.y = y;
    a.batch = batch; a.C = channels; a.HW = hw; a.y_ctot = y_ctot; a.y_coff = y_coff;
    a.res_ctot = res_ctot; a.res_coff = res_coff; a.eps = eps; a.rscale = res_scale; a.relu = relu;
    a.z_ctot = z_ctot; a.z_coff = z_coff;
    CT_REQUIRE((long)batch * channels * hw <= kMaxLoopElems, "ct_bn_train_apply: too many elements (2^32 less one grid stride at most)");
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for((long)batch * channels * hw)), dim3(256), 0,
                       ctdet::as_stream(stream), a);
    CT_LAUNCH_CHECK("bn_apply_kernel");
    return CT_OK;
}

// the checks and the argument record all BatchNorm backward entries share (dgamma / dbeta: null where the entry writes none)
static int bn_bwd_args(const char* who, BnBwdArgs& a, int frozen, const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot,
                       int y_coff, const float* z, const float* mean, const float* var,
                       const float* gamma, float eps, int relu, const float* lo,
                       float res_scale, float* dres, int dres_ctot, int dres_coff,
                       int dres_accumulate, float* dz, float* dgamma, float* dbeta,
                       int z_ctot, int z_coff, int batch, int channels, int hw)
{
    CT_REQUIRE(!(relu || lo) || y, "%s: ReLU mask needs the forward output", who);
    CT_REQUIRE((long)batch * channels * hw <= kMaxLoopElems, "%s: too many elements (2^32 less one grid stride at most)", who);
    a = BnBwdArgs{};
    a.dy = dy; a.y = y; a.z = z; a.mean = mean; a.var = var; a.gamma = gamma; a.lo = lo;
    a.dz = dz; a.dgamma = dgamma; a.dbeta = dbeta; a.dres = dres;
    a.batch = batch; a.C = channels; a.HW = hw; a.dy_ctot = dy_ctot; a.dy_coff = dy_coff;
    a.y_ctot = y_ctot; a.y_coff = y_coff; a.dres_ctot = dres_ctot; a.dres_coff = dres_coff;
    a.dres_accumulate = dres_accumulate; a.eps = eps; a.rscale = res_scale; a.relu = relu;
    a.z_ctot = z_ctot; a.z_coff = z_coff;
    a.frozen = frozen;
    return CT_OK;
}

static int bn_backward_impl(const char* who, bool det, size_t scratch_bytes, int frozen, const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot,
                            int y_coff, const float* z, const float* mean, const float* var,
                            const float* gamma, float eps, int relu, const float* lo,
                            float res_scale, float* dres, int dres_ctot, int dres_coff,
                            int dres_accumulate, float* dz, float* dgamma, float* dbeta,
                            int z_ctot, int z_coff, int batch, int channels, int hw,
                            void* scratch, ct_stream_t stream)
{
    CT_REQUIRE(dy && z && mean && var && gamma && dz && dgamma && dbeta, "%s: null pointer", who);
    BnBwdArgs a;
    if (int rc = bn_bwd_args(who, a, frozen, dy, dy_ctot, dy_coff, y, y_ctot, y_coff, z, mean, var, gamma, eps, relu, lo, res_scale, dres,
                             dres_ctot, dres_coff, dres_accumulate, dz, dgamma, dbeta, z_ctot, z_coff, batch, channels, hw)) return rc;
    hipStream_t st = ctdet::as_stream(stream);
    static const BnReduction<BnBwdArgs> kernels{bn_bwd_reduce_kernel, bn_bwd_reduce_part_kernel, bn_bwd_reduce_final_kernel,
                                                "bn_bwd_reduce_kernel", "bn_bwd_reduce_part_kernel", "bn_bwd_reduce_final_kernel"};
    if (int rc = bn_reduce_launch(who, kernels, a, batch, channels, hw, scratch, det, scratch_bytes, st)) return rc;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for((long)batch * channels * hw)), dim3(256), 0, st, a);
    CT_LAUNCH_CHECK("bn_bwd_apply_kernel");
    return CT_OK;
}

extern "C" int ct_bn_train_backward(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot,
                                    int y_coff, const float* z, const float* mean, const float* var,
                                    const float* gamma, float eps, int relu, const float* lo,
                                    float res_scale, float* dres, int dres_ctot, int dres_coff,
                                    int dres_accumulate, float* dz, float* dgamma, float* dbeta,
                                    int z_ctot, int z_coff, int batch, int channels, int hw,
                                    void* scratch, ct_stream_t stream)
{
    return bn_backward_impl("ct_bn_train_backward", false, 0, 0, dy, dy_ctot, dy_coff, y, y_ctot, y_coff, z, mean, var, gamma, eps, relu, lo, res_scale,
                            dres, dres_ctot, dres_coff, dres_accumulate, dz, dgamma, dbeta, z_ctot, z_coff, batch,
                            channels, hw, scratch, stream);
}

extern "C" int ct_bn_eval_backward(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot,
                                   int y_coff, const float* z, const float* running_mean, const float* running_var,
                                   const float* gamma, float eps, int relu, const float* lo,
                                   float res_scale, float* dres, int dres_ctot, int dres_coff,
                                   int dres_accumulate, float* dz, float* dgamma, float* dbeta,
                                   int z_ctot, int z_coff, int batch, int channels, int hw,
                                   void* scratch, ct_stream_t stream)
{
    return bn_backward_impl("ct_bn_eval_backward", false, 0, 1, dy, dy_ctot, dy_coff, y, y_ctot, y_coff, z, running_mean, running_var, gamma, eps, relu,
                            lo, res_scale, dres, dres_ctot, dres_coff, dres_accumulate, dz, dgamma, dbeta, z_ctot,
                            z_coff, batch, channels, hw, scratch, stream);
}

extern "C" int ct_bn_train_backward_det(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot,
                                        int y_coff, const float* z, const float* mean, const float* var,
                                        const float* gamma, float eps, int relu, const float* lo,
                                        float res_scale, float* dres, int dres_ctot, int dres_coff,
                                        int dres_accumulate, float* dz, float* dgamma, float* dbeta,
                                        int z_ctot, int z_coff, int batch, int channels, int hw,
                                        void* scratch, size_t scratch_bytes, ct_stream_t stream)
{
    return bn_backward_impl("ct_bn_train_backward_det", true, scratch_bytes, 0, dy, dy_ctot, dy_coff, y, y_ctot, y_coff, z, mean, var, gamma,
                            eps, relu, lo, res_scale, dres, dres_ctot, dres_coff, dres_accumulate, dz, dgamma, dbeta, z_ctot, z_coff,
                            batch, channels, hw, scratch, stream);
}

extern "C" int ct_bn_eval_backward_det(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot,
                                       int y_coff, const float* z, const float* running_mean, const float* running_var,
                                       const float* gamma, float eps, int relu, const float* lo,
                                       float res_scale, float* dres, int dres_ctot, int dres_coff,
                                       int dres_accumulate, float* dz, float* dgamma, float* dbeta,
                                       int z_ctot, int z_coff, int batch, int channels, int hw,
                                       void* scratch, size_t scratch_bytes, ct_stream_t stream)
{
    return bn_backward_impl("ct_bn_eval_backward_det", true, scratch_bytes, 1, dy, dy_ctot, dy_coff, y, y_ctot, y_coff, z, running_mean,
                            running_var, gamma, eps, relu, lo, res_scale, dres, dres_ctot, dres_coff, dres_accumulate, dz, dgamma,
                            dbeta, z_ctot, z_coff, batch, channels, hw, scratch, stream);
}

// ------------------------------------------------------------------------------------------
// Synchronized BatchNorm: a pass is local sums -> the caller's SUM collective over the ranks -> finish / apply
// ------------------------------------------------------------------------------------------
// what the four entries refuse before any HIP call, beyond their null pointers
static int bn_sync_sizes(const char* who, int batch, int channels, int hw)
{
    CT_REQUIRE(batch > 0 && channels > 0 && hw > 0, "%s: batch, channels and hw must be positive", who);
    return CT_OK;
}
static int bn_sync_count(const char* who, double count)
{
    CT_REQUIRE(std::isfinite(count) && count >= 1.0, "%s: count must be finite and at least 1 (the global batch * hw)", who);
    return CT_OK;
}
static int bn_sync_scratch(const char* who, const void* scratch)
{
    CT_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "%s: scratch must be 8-byte aligned", who);
    return CT_OK;
}

extern "C" int ct_bn_sync_stats_local(const float* z, int batch, int ctot, int coff, int channels, int hw, double* sums,
                                      void* scratch, size_t scratch_bytes, ct_stream_t stream)
{
    const char* who = "ct_bn_sync_stats_local";
    CT_REQUIRE(z && sums, "%s: null pointer", who);
    if (int rc = bn_sync_sizes(who, batch, channels, hw)) return rc;
    if (int rc = bn_sync_scratch(who, scratch)) return rc;
    BnSyncStatsArgs s{};
    s.op.z = z; s.op.batch = batch; s.op.ctot = ctot; s.op.coff = coff; s.op.C = channels; s.op.HW = hw;
    s.sums = sums;
    static const BnReduction<BnSyncStatsArgs> kernels{bn_sync_stats_kernel, bn_sync_stats_part_kernel, bn_sync_stats_final_kernel,
                                                      "bn_sync_stats_kernel", "bn_sync_stats_part_kernel", "bn_sync_stats_final_kernel"};
    return bn_reduce_launch(who, kernels, s, batch, channels, hw, scratch, true, scratch_bytes, ctdet::as_stream(stream));
}

extern "C" int ct_bn_sync_stats_finish(const double* sums, double count, int channels, float* mean, float* var, float momentum,
                                       float* running_mean, float* running_var, ct_stream_t stream)
{
    const char* who = "ct_bn_sync_stats_finish";
    CT_REQUIRE(sums && mean && var, "%s: null pointer", who);
    CT_REQUIRE(channels > 0, "%s: channels must be positive", who);
    if (int rc = bn_sync_count(who, count)) return rc;
    const bool run = running_mean && running_var;
    const float cntf = (float)count;
    StatsOp op{};
    op.mean = mean; op.var = var; op.rmean = run ? running_mean : nullptr; op.rvar = run ? running_var : nullptr;
    op.cnt = count; op.C = channels; op.momentum = momentum; op.unbias = cntf > 1.f ? cntf / (cntf - 1.f) : 1.f;
    hipLaunchKernelGGL(bn_sync_finish_kernel, dim3((channels + 255) / 256), dim3(256), 0, ctdet::as_stream(stream), op, sums);
    CT_LAUNCH_CHECK("bn_sync_finish_kernel");
    return CT_OK;
}

extern "C" int ct_bn_sync_backward_local(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot, int y_coff,
                                         const float* z, const float* mean, const float* var, float eps, int relu, const float* lo,
                                         float res_scale, int z_ctot, int z_coff, int batch, int channels, int hw,
                                         double* sums, float* dgamma, float* dbeta, void* scratch, size_t scratch_bytes,
                                         ct_stream_t stream)
{
    const char* who = "ct_bn_sync_backward_local";
    CT_REQUIRE(dy && z && mean && var && sums && dgamma && dbeta, "%s: null pointer", who);
    if (int rc = bn_sync_sizes(who, batch, channels, hw)) return rc;
    if (int rc = bn_sync_scratch(who, scratch)) return rc;
    BnSyncBwdArgs s{};
    if (int rc = bn_bwd_args(who, s.a, 0, dy, dy_ctot, dy_coff, y, y_ctot, y_coff, z, mean, var, nullptr, eps, relu, lo, res_scale, nullptr,
                             0, 0, 0, nullptr, dgamma, dbeta, z_ctot, z_coff, batch, channels, hw)) return rc;
    s.sums = sums;
    static const BnReduction<BnSyncBwdArgs> kernels{bn_sync_bwd_kernel, bn_sync_bwd_part_kernel, bn_sync_bwd_final_kernel,
                                                    "bn_sync_bwd_kernel", "bn_sync_bwd_part_kernel", "bn_sync_bwd_final_kernel"};
    return bn_reduce_launch(who, kernels, s, batch, channels, hw, scratch, true, scratch_bytes, ctdet::as_stream(stream));
}

extern "C" int ct_bn_sync_backward_apply(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot, int y_coff,
                                         const float* z, const float* mean, const float* var, const float* gamma, float eps,
                                         int relu, const float* lo, float res_scale, float* dres, int dres_ctot, int dres_coff,
                                         int dres_accumulate, float* dz, int z_ctot, int z_coff, int batch, int channels, int hw,
                                         const double* sums, double count, ct_stream_t stream)
{
    const char* who = "ct_bn_sync_backward_apply";
    CT_REQUIRE(dy && z && mean && var && gamma && dz && sums, "%s: null pointer", who);
    if (int rc = bn_sync_sizes(who, batch, channels, hw)) return rc;
    if (int rc = bn_sync_count(who, count)) return rc;
    BnBwdArgs a;
    if (int rc = bn_bwd_args(who, a, 0, dy, dy_ctot, dy_coff, y, y_ctot, y_coff, z, mean, var, gamma, eps, relu, lo, res_scale, dres,
                             dres_ctot, dres_coff, dres_accumulate, dz, nullptr, nullptr, z_ctot, z_coff, batch, channels, hw)) return rc;
    hipLaunchKernelGGL(bn_sync_bwd_apply_kernel, dim3(grid_for((long)batch * channels * hw)), dim3(256), 0, ctdet::as_stream(stream),
                       a, sums, count);
    CT_LAUNCH_CHECK("bn_sync_bwd_apply_kernel");
    return CT_OK;
}

// slices of a channel's batch*hw elements in the bias + activation backward, and the elements of one
struct BiasSlices { int slices, per_slice; };
static BiasSlices bias_slices(int batch, int channels, int hw)
{
    const long per_channel = (long)batch * hw;
    int slices = (int)std::max<long>(1, std::min<long>((2048 + channels - 1) / channels, (per_channel + 4095) / 4096));
    slices = std::min(slices, 65535);
    int per_slice = (int)((per_channel + slices - 1) / slices);
    per_slice = (per_slice + 3) / 4 * 4;
    slices = (int)((per_channel + per_slice - 1) / per_slice);
    return {slices, per_slice};
}

// Around the launch of a bias backward kernel: where its per-block dbias sums go.  det: `nslabs` x channels doubles in the checked
// scratch, added in order after the launch; else float atomics into dbias, zeroed here unless the caller has
// (ct_scratch_prezeroed).  launch(slab) returns a status.
template <class Launch>
static int with_dbias_sink(const char* who, bool det, float* dbias, int nslabs, int channels, void* scratch, size_t scratch_bytes,
                           hipStream_t st, Launch launch)
{
    double* slab = nullptr;
    if (det && dbias) {
        if (int rc = det_scratch_check(who, scratch, scratch_bytes, (size_t)nslabs * channels * sizeof(double))) return rc;
        slab = static_cast<double*>(scratch);
    }
    if (dbias && !slab && !ctdet::scratch_prezeroed()) CT_HIP(hipMemsetAsync(dbias, 0, (size_t)channels * 4, st));
    if (int rc = launch(slab)) return rc;
    if (!slab) return CT_OK;
    hipLaunchKernelGGL(dbias_slab_sum_kernel, dim3((channels + 255) / 256), dim3(256), 0, st, slab, nslabs, channels, dbias);
    CT_LAUNCH_CHECK("dbias_slab_sum_kernel");
    return CT_OK;
}

static int bias_act_backward_impl(const char* who, const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot,
                                  int y_coff, int relu, int batch, int channels, int hw, float* dz,
                                  int dz_ctot, int dz_coff, float* dbias, unsigned* dz_absmax, bool det, void* scratch,
                                  size_t scratch_bytes, ct_stream_t stream)
{
    CT_REQUIRE(dy && dz && (!relu || y), "%s: null pointer", who);
    CT_REQUIRE(batch > 0 && channels > 0 && hw > 0, "%s: bad shape", who);
    hipStream_t st = ctdet::as_stream(stream);
    const BiasSlices sl = bias_slices(batch, channels, hw);
    return with_dbias_sink(who, det, dbias, sl.slices, channels, scratch, scratch_bytes, st, [&](double* slab) {
        hipLaunchKernelGGL(bias_act_bwd_kernel, dim3(channels, sl.slices), dim3(256), 0, st, dy, dy_ctot, dy_coff, y,
                           y_ctot, y_coff, relu, batch, channels, hw, dz, dz_ctot, dz_coff, dbias, sl.per_slice, dz_absmax, slab);
        CT_LAUNCH_CHECK("bias_act_bwd_kernel");
        return (int)CT_OK;
    });
}

extern "C" int ct_bias_act_backward_amax(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot,
                                         int y_coff, int relu, int batch, int channels, int hw, float* dz,
                                         int dz_ctot, int dz_coff, float* dbias, unsigned* dz_absmax, ct_stream_t stream)
{
    return bias_act_backward_impl("ct_bias_act_backward", dy, dy_ctot, dy_coff, y, y_ctot, y_coff, relu, batch, channels, hw, dz, dz_ctot,
                                  dz_coff, dbias, dz_absmax, false, nullptr, 0, stream);
}

extern "C" size_t ct_bias_det_scratch_bytes(int batch, int channels, int hw, int* partials)
{
    if (partials) *partials = 0;
    if (batch <= 0 || channels <= 0 || hw <= 0) return 0;
    if (partials) *partials = bias_slices(batch, channels, hw).slices;
    // slices * channels doubles, bounded from above by an expression that grows with batch and with channels
    const long per_channel = (long)batch * hw;
    const long records = std::max<long>(channels, std::min<long>(2047L + channels, (long)channels * ((per_channel + 4095) / 4096)));
    return (size_t)records * sizeof(double);
}

extern "C" int ct_bias_act_backward_det(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot,
                                        int y_coff, int relu, int batch, int channels, int hw, float* dz,
                                        int dz_ctot, int dz_coff, float* dbias, unsigned* dz_absmax, void* scratch,
                                        size_t scratch_bytes, ct_stream_t stream)
{
    return bias_act_backward_impl("ct_bias_act_backward_det", dy, dy_ctot, dy_coff, y, y_ctot, y_coff, relu, batch, channels, hw, dz,
                                  dz_ctot, dz_coff, dbias, dz_absmax, true, scratch, scratch_bytes, stream);
}

extern "C" int ct_bias_act_backward(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot,
                                    int y_coff, int relu, int batch, int channels, int hw, float* dz,
                                    int dz_ctot, int dz_coff, float* dbias, ct_stream_t stream)
{
    return ct_bias_act_backward_amax(dy, dy_ctot, dy_coff, y, y_ctot, y_coff, relu, batch, channels, hw, dz, dz_ctot, dz_coff, dbias,
                                     nullptr, stream);
}

extern "C" int ct_maxpool2d_bwd(const float* x, const float* dy, float* dx, long planes, int h, int w,
                                int oh, int ow, int k, int stride, int pad, int accumulate,
                                ct_stream_t stream)
{
    CT_REQUIRE(x && dy && dx && planes > 0, "ct_maxpool2d_bwd: bad arguments");
    CT_REQUIRE(planes <= kMaxLoopElems && planes * h * w <= kMaxLoopElems, "ct_maxpool2d_bwd: too many elements (2^32 less one grid stride at most)");
    if (k == 2 && stride == 2 && pad == 0 && oh <= (h + 1) / 2 && ow <= (w + 1) / 2 && planes <= 0x7FFFFFFFL) {
        hipLaunchKernelGGL(maxpool2x2_bwd_kernel, dim3((unsigned)planes), dim3(256), 0, ctdet::as_stream(stream), x,
                           dy, dx, h, w, oh, ow, accumulate);
        CT_LAUNCH_CHECK("maxpool2x2_bwd_kernel");
        return CT_OK;
    }
    if (h * w <= kPoolPlaneMax && oh * ow <= kPoolPlaneMax && planes <= 0x7FFFFFFFL) {
        hipLaunchKernelGGL(maxpool2d_bwd_plane_kernel, dim3((unsigned)planes), dim3(256), 0, ctdet::as_stream(stream), x, dy, dx,
                           h, w, oh, ow, k, stride, pad, accumulate);
        CT_LAUNCH_CHECK("maxpool2d_bwd_plane_kernel");
        return CT_OK;
    }
    hipLaunchKernelGGL(maxpool2d_bwd_kernel, dim3(grid_for(planes * h * w)), dim3(256), 0,
                       ctdet::as_stream(stream), x, dy, dx, planes, h, w, oh, ow, k, stride, pad, accumulate);
    CT_LAUNCH_CHECK("maxpool2d_bwd_kernel");
    return CT_OK;
}

static int maxpool2x2_bias_relu_bwd_impl(const char* who, const float* y, int y_ctot, int y_coff, const float* dy, int batch, int channels,
                                        int h, int w, int oh, int ow, float* dz, int dz_ctot, int dz_coff, float* dbias,
                                        unsigned* dz_absmax, bool det, void* scratch, size_t scratch_bytes, ct_stream_t stream)
{
    CT_REQUIRE(y && dy && dz && batch > 0 && channels > 0 && h > 0 && w > 0, "%s: bad arguments", who);
    CT_REQUIRE(oh <= (h + 1) / 2 && ow <= (w + 1) / 2 && oh >= h / 2 && ow >= w / 2, "%s: %dx%d is not a 2x2 / stride 2 "
               "pooling of %dx%d", who, oh, ow, h, w);
    CT_REQUIRE(y_coff >= 0 && y_coff + channels <= y_ctot && dz_coff >= 0 && dz_coff + channels <= dz_ctot, "%s: channel slice", who);
    CT_REQUIRE((long)batch * channels <= 0x7FFFFFFFL, "%s: too many planes", who);
    hipStream_t st = ctdet::as_stream(stream);
    return with_dbias_sink(who, det, dbias, batch, channels, scratch, scratch_bytes, st, [&](double* slab) {
        hipLaunchKernelGGL(maxpool2x2_bias_relu_bwd_kernel, dim3((unsigned)(batch * channels)), dim3(256), 0, st, y, y_ctot, y_coff,
                           dy, channels, h, w, oh, ow, dz, dz_ctot, dz_coff, dbias, dz_absmax, slab);
        CT_LAUNCH_CHECK("maxpool2x2_bias_relu_bwd_kernel");
        return (int)CT_OK;
    });
}

extern "C" int ct_maxpool2x2_bias_relu_bwd(const float* y, int y_ctot, int y_coff, const float* dy, int batch, int channels, int h,
                                           int w, int oh, int ow, float* dz, int dz_ctot, int dz_coff, float* dbias,
                                           unsigned* dz_absmax, ct_stream_t stream)
{
    return maxpool2x2_bias_relu_bwd_impl("ct_maxpool2x2_bias_relu_bwd", y, y_ctot, y_coff, dy, batch, channels, h, w, oh, ow, dz, dz_ctot,
                                         dz_coff, dbias, dz_absmax, false, nullptr, 0, stream);
}

extern "C" size_t ct_maxpool2x2_bias_relu_bwd_det_scratch_bytes(int batch, int channels, int* partials)
{
    if (partials) *partials = 0;
    if (batch <= 0 || channels <= 0) return 0;
    if (partials) *partials = batch;            // one workgroup, one partial sum per (image, channel) plane
    return (size_t)batch * channels * sizeof(double);
}

extern "C" int ct_maxpool2x2_bias_relu_bwd_det(const float* y, int y_ctot, int y_coff, const float* dy, int batch, int channels, int h,
                                               int w, int oh, int ow, float* dz, int dz_ctot, int dz_coff, float* dbias,
                                               unsigned* dz_absmax, void* scratch, size_t scratch_bytes, ct_stream_t stream)
{
    return maxpool2x2_bias_relu_bwd_impl("ct_maxpool2x2_bias_relu_bwd_det", y, y_ctot, y_coff, dy, batch, channels, h, w, oh, ow, dz,
                                         dz_ctot, dz_coff, dbias, dz_absmax, true, scratch, scratch_bytes, stream);
}

extern "C" int ct_head_grad_gather(const ct_out_segment* segs, int nseg, int batch, int channels, int hw,
                                   float* dz, ct_stream_t stream)
{
    CT_REQUIRE(segs && dz && nseg >= 1 && nseg <= 3, "ct_head_grad_gather: bad arguments");
    CT_REQUIRE((long)batch * channels * hw <= kMaxLoopElems, "ct_head_grad_gather: too many elements (2^32 less one grid stride at most)");
    HeadGatherArgs a{};
    for (int g = 0; g < nseg; ++g) a.seg[g] = segs[g];
    a.nseg = nseg; a.dz = dz; a.batch = batch; a.C = channels; a.HW = hw;
    hipLaunchKernelGGL(head_grad_gather_kernel, dim3(grid_for((long)batch * channels * hw)), dim3(256), 0,
                       ctdet::as_stream(stream), a);
    CT_LAUNCH_CHECK("head_grad_gather_kernel");
    return CT_OK;
}
