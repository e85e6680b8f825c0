// libctdet: adaptive training sample selection (ATSS), the second matcher of MultiBoxLoss.  The rule is in include/ctdet.h at
// ct_atss_match_batched; tests/atss_ref.py restates it in numpy.  Two kernels: a selection kernel, one workgroup per (image,
// box), which picks the candidates, sets the threshold and publishes claims, and an assign kernel, one thread per (image,
// prior), which turns the winning claim into the outputs ct_match_batched would write.
//
// Compiled with -ffp-contract=off like ct_box.hip: distances, IoUs and the float64 statistics round operation by operation.
#include "ct_common.h"
#include "ct_box_math.h"
#include "ct_claims.h"
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

using ctdet::iou_plain;
using ctdet::pack_claim;         // ordered by rule 7
using ctdet::point_form;

constexpr int kMaxLevels = 8;
constexpr int kMaxTopk = 16;
constexpr int kMaxCand = kMaxLevels * kMaxTopk;         // 128 candidates of one box, in LDS
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kUnroll = 8;                              // loads a thread keeps in flight while it scans a level

struct Levels {                                          // level_off travels in the kernel arguments: no H2D copy
    int n;
    int off[kMaxLevels + 1];
};

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(v, s);
        v = o < v ? o : v;
    }
    return v;
}

// One 256-thread workgroup per (image b, box g).  Per level the min(topk, n_l) nearest prior centres are found one at a time:
// the smallest (d bits << 32 | prior) key greater than the last one chosen, by a wave reduction and then across the four
// waves through LDS (two alternating slots: one barrier per pick).  Keys are distinct, so nothing is marked.
// With a few hundred workgroups the kernel waits on its loads, so a thread scans its share of a level in whole rounds of
// kUnroll loads issued together; a plain loop takes the tail, and no prior is loaded twice.
__global__ __launch_bounds__(256) void atss_select(const float* __restrict__ truths, const int* __restrict__ gt_off,
                                                   const float4* __restrict__ priors, int P, Levels lv, int topk, int max_gt,
                                                   unsigned long long* __restrict__ claims, float* __restrict__ gt_stats)
{
    __shared__ unsigned long long wmin[2][4];
    __shared__ int cand[kMaxCand];
    __shared__ float ciou[kMaxCand];
    __shared__ unsigned char cin[kMaxCand];
    __shared__ float s_t;
    __shared__ int s_forced;

    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int g0 = gt_off[b], G = min(gt_off[b + 1] - g0, max_gt);
    float* stats = gt_stats ? gt_stats + ((size_t)b * max_gt + g) * 4 : nullptr;
    float4 gt = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g < G) {
        const float* t = truths + (size_t)(g0 + g) * 6;
        gt = make_float4(t[0], t[1], t[2], t[3]);
    }
    if (g >= G || !(gt.z > gt.x && gt.w > gt.y)) {      // absent or degenerate (rule 1): a row of zeros, no claims
        if (stats && tid < 4) stats[tid] = 0.f;
        return;
    }
    const float gx = (gt.x + gt.z) / 2.f, gy = (gt.y + gt.w) / 2.f;

    int n = 0, step = 0;
    for (int l = 0; l < lv.n; ++l) {
        const int lo = lv.off[l], hi = lv.off[l + 1];
        const int k = min(topk, hi - lo);
        unsigned long long last = 0ull;
        bool first = true;
        for (int j = 0; j < k; ++j, ++step) {
            unsigned long long best = kNoKey;
            const auto take = [&](int p, const float2 c) {
                const float dx = c.x - gx, dy = c.y - gy;
                const float d = dx * dx + dy * dy;
                const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)p;
                if ((first || key > last) && key < best) best = key;
            };
            int p = lo + tid;
            for (; p + 256 * (kUnroll - 1) < hi; p += 256 * kUnroll) {      // whole rounds: kUnroll loads in flight together
                float2 c[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) c[u] = *reinterpret_cast<const float2*>(priors + p + 256 * u);
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) take(p + 256 * u, c[u]);
            }
            for (; p < hi; p += 256) take(p, *reinterpret_cast<const float2*>(priors + p));      // the centre alone
            best = wave_min(best);
            if ((tid & 63) == 0) wmin[step & 1][tid >> 6] = best;
            __syncthreads();
            const unsigned long long a0 = wmin[step & 1][0], a1 = wmin[step & 1][1], a2 = wmin[step & 1][2],
                                     a3 = wmin[step & 1][3];
            const unsigned long long m01 = a0 < a1 ? a0 : a1, m23 = a2 < a3 ? a2 : a3;
            last = m01 < m23 ? m01 : m23;
            first = false;
            if (tid == 0) cand[n + j] = (int)(unsigned)(last & 0xFFFFFFFFull);
        }
        n += k;
    }
    __syncthreads();

    // rule 3 and the centre test of rule 5, one candidate per thread (n <= 128)
    if (tid < n) {
        const float4 pr = priors[cand[tid]];
        ciou[tid] = iou_plain(gt, point_form(pr));
        cin[tid] = (gt.x < pr.x && pr.x < gt.z && gt.y < pr.y && pr.y < gt.w) ? 1 : 0;
    }
    __syncthreads();

    // rules 4 and 6 by one lane, in candidate order (49 values on VOC_300, 58 on VOC_512)
    if (tid == 0) {
        double sum = 0.0;
        for (int c = 0; c < n; ++c) sum += (double)ciou[c];
        const double mean = sum / (double)n;
        double var = 0.0;
        if (n >= 2) {
            for (int c = 0; c < n; ++c) {
                const double e = (double)ciou[c] - mean;
                var += e * e;
            }
            var = var / (double)(n - 1);
        }
        const float t = (float)(mean + sqrt(var));
        int npos = 0, arg = 0;
        float top = ciou[0];
        for (int c = 0; c < n; ++c) {
            if (ciou[c] >= t && cin[c]) ++npos;
            if (ciou[c] > top) { top = ciou[c]; arg = c; }          // the first maximum in candidate order
        }
        const int forced = npos == 0 ? arg : -1;
        s_t = t;
        s_forced = forced;
        if (stats) {
            stats[0] = t;
            stats[1] = (float)n;
            stats[2] = (float)(npos == 0 ? 1 : npos);
            stats[3] = npos == 0 ? 1.f : 0.f;
        }
    }
    __syncthreads();

    if (tid < n) {
        const float t = s_t;
        const int forced = s_forced;
        const bool is_forced = tid == forced;
        if (is_forced || (forced < 0 && ciou[tid] >= t && cin[tid]))
            atomicMax(&claims[(size_t)b * P + cand[tid]], pack_claim(is_forced, ciou[tid], g));
    }
}

// One thread per (image, prior): the winning claim, if any, becomes rule 8's outputs.
__global__ __launch_bounds__(256) void atss_assign(const float* __restrict__ truths, const int* __restrict__ gt_off,
                                                   const float4* __restrict__ priors, int P,
                                                   const unsigned long long* __restrict__ claims, float v0, float v1,
                                                   float4* __restrict__ loc_t, float2* __restrict__ conf_t,
                                                   uint8_t* __restrict__ obj_t, float* __restrict__ overlap)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) ctdet::assign_claim(truths, gt_off, priors, P, blockIdx.y, p, claims, v0, v1, loc_t, conf_t, obj_t, overlap);
}

}  // namespace

extern "C" size_t ct_atss_workspace_bytes(int batch, int num_priors, int max_gt)
{
    (void)max_gt;                                        // the claims are per prior; kept in the signature for the caller's symmetry
    if (batch < 1 || num_priors < 1) return 0;
    return ctdet::align_up((size_t)batch * num_priors * 8, 256);
}

extern "C" int ct_atss_match_batched(const float* truths, const int* gt_off, int batch, int max_gt, const float* priors,
                                     int num_priors, const int* level_off_host, int num_levels, int topk, float var0,
                                     float var1, float* loc_t, float* conf_t, uint8_t* obj_t, float* overlap, float* gt_stats,
                                     void* workspace, size_t workspace_bytes, ct_stream_t stream)
{
    CT_REQUIRE(truths && gt_off && priors && level_off_host && loc_t && conf_t && obj_t && workspace,
               "ct_atss_match_batched: null pointer");
    CT_REQUIRE(batch >= 1 && num_priors >= 1, "ct_atss_match_batched: bad shape (batch=%d, num_priors=%d)", batch, num_priors);
    CT_REQUIRE(num_priors <= (1 << 30), "ct_atss_match_batched: num_priors=%d (<= 2^30: prior indices plus a scan round stay in int)",
               num_priors);
    CT_REQUIRE(max_gt >= 1, "ct_atss_match_batched: max_gt=%d", max_gt);
    CT_REQUIRE(batch <= 65535, "ct_atss_match_batched: batch=%d (<= 65535)", batch);
    CT_REQUIRE(num_levels >= 1 && num_levels <= kMaxLevels, "ct_atss_match_batched: num_levels=%d (1..%d)", num_levels,
               kMaxLevels);
    CT_REQUIRE(topk >= 1 && topk <= kMaxTopk, "ct_atss_match_batched: topk=%d (1..%d)", topk, kMaxTopk);
    Levels lv;
    lv.n = num_levels;
    for (int l = 0; l <= kMaxLevels; ++l) lv.off[l] = l <= num_levels ? level_off_host[l] : num_priors;
    bool ascending = lv.off[0] == 0 && lv.off[num_levels] == num_priors;
    for (int l = 0; l < num_levels; ++l) ascending = ascending && lv.off[l] < lv.off[l + 1];
    CT_REQUIRE(ascending, "ct_atss_match_batched: level_off must be 0 = off[0] < ... < off[%d] = num_priors = %d", num_levels,
               num_priors);
    CT_REQUIRE(std::isfinite(var0) && std::isfinite(var1) && var0 > 0.f && var1 > 0.f,
               "ct_atss_match_batched: variances (%g, %g) must be positive and finite", (double)var0, (double)var1);
    CT_REQUIRE(workspace_bytes >= ct_atss_workspace_bytes(batch, num_priors, max_gt),
               "ct_atss_match_batched: workspace %zu < %zu", workspace_bytes,
               ct_atss_workspace_bytes(batch, num_priors, max_gt));
    CT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "ct_atss_match_batched: workspace must be 8-byte aligned");
    unsigned long long* claims = (unsigned long long*)workspace;
    hipStream_t st = ctdet::as_stream(stream);
    CT_HIP(hipMemsetAsync(claims, 0, (size_t)batch * num_priors * 8, st));
    {
        CT_PROF("atss_select", st);
        hipLaunchKernelGGL(atss_select, dim3(max_gt, batch), dim3(256), 0, st, truths, gt_off, (const float4*)priors,
                           num_priors, lv, topk, max_gt, claims, gt_stats);
    }
    CT_LAUNCH_CHECK("atss_select");
    {
        CT_PROF("atss_assign", st);
        hipLaunchKernelGGL(atss_assign, dim3((num_priors + 255) / 256, batch), dim3(256), 0, st, truths, gt_off,
                           (const float4*)priors, num_priors, claims, var0, var1, (float4*)loc_t, (float2*)conf_t, obj_t,
                           overlap);
    }
    CT_LAUNCH_CHECK("atss_assign");
    return CT_OK;
}
