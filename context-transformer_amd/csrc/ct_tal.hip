// libctdet: task-aligned assignment (TAL), the prediction-aware matcher of MultiBoxLoss.  The rule is in include/ctdet.h at
// ct_tal_match_batched; tests/tal_ref.py restates it in numpy.  Two kernels, like ATSS: a selection kernel, one workgroup per
// (image, box), which ranks the priors inside the box by score^alpha * IoU(predicted box, box)^beta, keeps the best topk and
// publishes claims, and an assign kernel, one thread per (image, prior), shared with ct_atss.hip through ct_claims.h.
//
// Compiled with -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt: the IoU, sqrtf and the metric's products round
// operation by operation.
#include "ct_common.h"
#include "ct_box_math.h"
#include "ct_claims.h"
#include <cfloat>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

using ctdet::iou_plain;
using ctdet::pack_claim;         // ordered by rule 6
using ctdet::point_form;

constexpr int kMaxTopk = 16;
constexpr int kUnroll = 8;                               // priors a thread handles per round, their loads in flight together
constexpr int kRound = 256 * kUnroll;                    // priors of one round
constexpr int kKeysPerThread = 16;                       // of the key buffer, held in registers while it is reduced
constexpr int kCap = 256 * kKeysPerThread;               // keys the LDS buffer holds: 32 KiB, whatever P is
static_assert(kCap >= kMaxTopk + kRound, "the buffer must take the survivors of a reduction plus one full round");

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(v, s);
        v = o > v ? o : v;
    }
    return v;
}

// The maximum over the 256 threads, returned to all of them: a wave reduction, then across the four waves through LDS.  Two
// alternating slots make one barrier per call enough: `step` counts the calls of the workgroup.
__device__ __forceinline__ unsigned long long group_max(unsigned long long v, unsigned long long (*wmax)[4], int& step)
{
    v = wave_max(v);
    const int s = step & 1;
    ++step;
    if ((threadIdx.x & 63) == 0) wmax[s][threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned long long a0 = wmax[s][0], a1 = wmax[s][1], a2 = wmax[s][2], a3 = wmax[s][3];
    const unsigned long long m01 = a0 > a1 ? a0 : a1, m23 = a2 > a3 ? a2 : a3;
    return m01 > m23 ? m01 : m23;
}

// Rule 3 from u and s: 1 * [sqrt(s)] * s^(alpha2/2) * u^beta in this order, below FLT_MIN -> 0.
__device__ __forceinline__ float metric(float s, float u, int alpha2, int beta)
{
    float m = 1.f;
    if (alpha2 & 1) m = m * sqrtf(s);
    for (int i = 0; i < (alpha2 >> 1); ++i) m = m * s;
    for (int i = 0; i < beta; ++i) m = m * u;
    return m >= FLT_MIN ? m : 0.f;
}

__device__ __forceinline__ float clamped_iou(const float4 gt, const float4 box)
{
    const float u = iou_plain(gt, box);
    return u > 0.f ? u : 0.f;                            // NaN included
}

// The n keys of buf reduced to their k = min(topk, n) largest, left in buf[0..k) in descending order; -> k.  Every thread takes
// its share of the buffer into registers, then the keys are picked one at a time: the largest key below the last one chosen
// (keys are distinct and never 0).  Entered by the whole workgroup with pushes complete; ends with a barrier.
__device__ __forceinline__ int reduce_keys(unsigned long long* buf, int n, int topk, unsigned long long (*wmax)[4], int& step,
                                           unsigned long long& kth)
{
    const int tid = threadIdx.x;
    unsigned long long mine[kKeysPerThread];
#pragma unroll
    for (int i = 0; i < kKeysPerThread; ++i) mine[i] = tid + 256 * i < n ? buf[tid + 256 * i] : 0ull;
    __syncthreads();                                     // all of buf is read before its head is rewritten
    const int k = min(topk, n);
    unsigned long long last = ~0ull;
    for (int j = 0; j < k; ++j) {
        unsigned long long best = 0ull;
#pragma unroll
        for (int i = 0; i < kKeysPerThread; ++i)
            if (mine[i] < last && mine[i] > best) best = mine[i];
        last = group_max(best, wmax, step);
        if (tid == 0) buf[j] = last;
    }
    kth = k == topk ? last : 0ull;                       // fewer than topk so far: every eligible key is still wanted
    __syncthreads();
    return k;
}

// One 256-thread workgroup per (image b, box g).  One pass over the priors in rounds of kRound: a prior whose centre lies in the
// box has its predicted box and score loaded and its metric computed once; (metric bits << 32 | ~prior) keys above the running
// threshold go into an LDS buffer through an LDS counter.  When the buffer cannot take another full round it is reduced to its
// topk largest and the topk-th becomes the threshold; it is reduced once more at the end.  Keys are distinct, so the final set
// does not depend on the order of arrival.  The IoU a claim carries is recomputed for the topk chosen: two evaluations per
// (box, prior) at most.  Only a box with no eligible candidate scans the priors' own IoUs for its forced positive.
__global__ __launch_bounds__(256) void tal_select(const float* __restrict__ truths, const int* __restrict__ gt_off,
                                                  const float4* __restrict__ priors, int P,
                                                  const float4* __restrict__ pred_boxes, const float* __restrict__ pred_scores,
                                                  int score_cols, int topk, int alpha2, int beta, int max_gt,
                                                  unsigned long long* __restrict__ claims, float* __restrict__ gt_stats)
{
    __shared__ unsigned long long buf[kCap];
    __shared__ unsigned long long wmax[2][4];
    __shared__ int s_cnt, s_elig;

    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int g0 = gt_off[b], G = min(gt_off[b + 1] - g0, max_gt);
    float* stats = gt_stats ? gt_stats + ((size_t)b * max_gt + g) * 4 : nullptr;
    float4 gt = make_float4(0.f, 0.f, 0.f, 0.f);
    float label = 0.f;
    if (g < G) {
        const float* t = truths + (size_t)(g0 + g) * 6;
        gt = make_float4(t[0], t[1], t[2], t[3]);
        label = t[4];
    }
    if (g >= G || !(gt.z > gt.x && gt.w > gt.y)) {      // absent or degenerate (rule 1): a row of zeros, no claims
        if (stats && tid < 4) stats[tid] = 0.f;
        return;
    }
    // the score column of rule 3: the box's class, or 1 - background for a label that names no foreground column
    const bool fg = label >= 1.f && label <= (float)(score_cols - 1) && label == truncf(label);
    const int col = fg ? (int)label : 0;
    const size_t row0 = (size_t)b * P;

    if (tid == 0) { s_cnt = 0; s_elig = 0; }
    __syncthreads();

    int step = 0, elig = 0;
    unsigned long long thr = 0ull;
    for (int base = 0; base < P; base += kRound) {
        const int n = s_cnt;
        __syncthreads();                                 // everyone has read the count before anyone pushes again
        if (n + kRound > kCap) {                         // workgroup-uniform
            const int k = reduce_keys(buf, n, topk, wmax, step, thr);
            if (tid == 0) s_cnt = k;
            __syncthreads();
        }
        bool in[kUnroll];
        float4 box[kUnroll];
        float sc[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int p = base + tid + 256 * u;
            in[u] = false;
            if (p < P) {
                const float2 c = *reinterpret_cast<const float2*>(priors + p);      // the centre alone
                in[u] = gt.x < c.x && c.x < gt.z && gt.y < c.y && c.y < gt.w;
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (in[u]) {
                const size_t o = row0 + (size_t)(base + tid + 256 * u);
                box[u] = pred_boxes[o];
                sc[u] = pred_scores[o * score_cols + col];
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (in[u]) {
                const int p = base + tid + 256 * u;
                float s = fg ? sc[u] : 1.f - sc[u];
                s = s > 0.f ? s : 0.f;
                const float m = metric(s, clamped_iou(gt, box[u]), alpha2, beta);
                if (m > 0.f) {
                    ++elig;
                    const unsigned long long key = ((unsigned long long)__float_as_uint(m) << 32) | (unsigned)~(unsigned)p;
                    if (key > thr) buf[atomicAdd(&s_cnt, 1)] = key;      // at most kRound pushes a round: below kCap
                }
            }
        }
        __syncthreads();                                 // the round's pushes are complete
    }
    if (elig) atomicAdd(&s_elig, elig);
    __syncthreads();
    const int k = reduce_keys(buf, s_cnt, topk, wmax, step, thr);
    const int eligible = s_elig;

    if (eligible == 0) {                                 // rule 5, workgroup-uniform: the best prior by its own IoU
        unsigned long long best = 0ull;
        for (int p = tid; p < P; p += 256) {
            const float u = iou_plain(gt, point_form(priors[p]));
            const unsigned long long key = ((unsigned long long)(__float_as_uint(u) & 0x7FFFFFFFu) << 32) | (unsigned)~(unsigned)p;
            best = key > best ? key : best;
        }
        best = group_max(best, wmax, step);
        if (tid == 0) {
            const int p = (int)~(unsigned)(best & 0xFFFFFFFFull);
            atomicMax(&claims[row0 + p], pack_claim(true, __uint_as_float((unsigned)(best >> 32)), g));
            if (stats) {
                stats[0] = 0.f;
                stats[1] = 1.f;
                stats[2] = 0.f;
                stats[3] = 1.f;
            }
        }
        return;
    }
    if (tid < k) {                                       // rule 4: the claims carry u, evaluated a second time
        const int p = (int)~(unsigned)(buf[tid] & 0xFFFFFFFFull);
        atomicMax(&claims[row0 + p], pack_claim(false, clamped_iou(gt, pred_boxes[row0 + p]), g));
    }
    if (stats && tid == 0) {
        stats[0] = (float)eligible;
        stats[1] = (float)k;
        stats[2] = __uint_as_float((unsigned)(buf[k - 1] >> 32));
        stats[3] = 0.f;
    }
}

__global__ __launch_bounds__(256) void tal_assign(const float* __restrict__ truths, const int* __restrict__ gt_off,
                                                  const float4* __restrict__ priors, int P,
                                                  const unsigned long long* __restrict__ claims, float v0, float v1,
                                                  float4* __restrict__ loc_t, float2* __restrict__ conf_t,
                                                  uint8_t* __restrict__ obj_t, float* __restrict__ overlap)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) ctdet::assign_claim(truths, gt_off, priors, P, blockIdx.y, p, claims, v0, v1, loc_t, conf_t, obj_t, overlap);
}

}  // namespace

extern "C" int ct_tal_lds_keys(void) { return kCap; }

extern "C" size_t ct_tal_workspace_bytes(int batch, int num_priors, int max_gt)
{
    (void)max_gt;                                        // the claims are per prior; kept in the signature for the caller's symmetry
    if (batch < 1 || num_priors < 1) return 0;
    return ctdet::align_up((size_t)batch * num_priors * 8, 256);
}

extern "C" int ct_tal_match_batched(const float* truths, const int* gt_off, int batch, int max_gt, const float* priors,
                                    int num_priors, const float* pred_boxes, const float* pred_scores, int score_cols, int topk,
                                    int alpha2, int beta, float var0, float var1, float* loc_t, float* conf_t, uint8_t* obj_t,
                                    float* overlap, float* gt_stats, void* workspace, size_t workspace_bytes, ct_stream_t stream)
{
    CT_REQUIRE(truths && gt_off && priors && pred_boxes && pred_scores && loc_t && conf_t && obj_t && workspace,
               "ct_tal_match_batched: null pointer");
    CT_REQUIRE(batch >= 1 && num_priors >= 1, "ct_tal_match_batched: bad shape (batch=%d, num_priors=%d)", batch, num_priors);
    CT_REQUIRE(num_priors <= (1 << 30), "ct_tal_match_batched: num_priors=%d (<= 2^30: prior indices plus a scan round stay in int)",
               num_priors);
    CT_REQUIRE(max_gt >= 1, "ct_tal_match_batched: max_gt=%d", max_gt);
    CT_REQUIRE(batch <= 65535, "ct_tal_match_batched: batch=%d (<= 65535)", batch);
    CT_REQUIRE(score_cols >= 2, "ct_tal_match_batched: score_cols=%d (>= 2: background plus one class)", score_cols);
    CT_REQUIRE(topk >= 1 && topk <= kMaxTopk, "ct_tal_match_batched: topk=%d (1..%d)", topk, kMaxTopk);
    CT_REQUIRE(alpha2 >= 0 && alpha2 <= 4, "ct_tal_match_batched: alpha2=%d (0..4: twice alpha)", alpha2);
    CT_REQUIRE(beta >= 0 && beta <= 8, "ct_tal_match_batched: beta=%d (0..8)", beta);
    CT_REQUIRE(std::isfinite(var0) && std::isfinite(var1) && var0 > 0.f && var1 > 0.f,
               "ct_tal_match_batched: variances (%g, %g) must be positive and finite", (double)var0, (double)var1);
    CT_REQUIRE(workspace_bytes >= ct_tal_workspace_bytes(batch, num_priors, max_gt), "ct_tal_match_batched: workspace %zu < %zu",
               workspace_bytes, ct_tal_workspace_bytes(batch, num_priors, max_gt));
    CT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "ct_tal_match_batched: workspace must be 8-byte aligned");
    unsigned long long* claims = (unsigned long long*)workspace;
    hipStream_t st = ctdet::as_stream(stream);
    CT_HIP(hipMemsetAsync(claims, 0, (size_t)batch * num_priors * 8, st));
    {
        CT_PROF("tal_select", st);
        hipLaunchKernelGGL(tal_select, dim3(max_gt, batch), dim3(256), 0, st, truths, gt_off, (const float4*)priors, num_priors,
                           (const float4*)pred_boxes, pred_scores, score_cols, topk, alpha2, beta, max_gt, claims, gt_stats);
    }
    CT_LAUNCH_CHECK("tal_select");
    {
        CT_PROF("tal_assign", st);
        hipLaunchKernelGGL(tal_assign, dim3((num_priors + 255) / 256, batch), dim3(256), 0, st, truths, gt_off,
                           (const float4*)priors, num_priors, claims, var0, var1, (float4*)loc_t, (float2*)conf_t, obj_t, overlap);
    }
    CT_LAUNCH_CHECK("tal_assign");
    return CT_OK;
}
