// libctdet: soft-NMS (utils/nms/cpu_nms.pyx:70-163 `cpu_soft_nms`) on the device, one workgroup per segment.
//
// The reference swaps rows inside one array; on tie-free input the same rows come out in the same order from
//
//   alive = all rows
//   repeat: m = the alive row with the largest CURRENT score (ties: lowest position in the sorted input)
//           [max_emit > 0, already max_emit rows out and score[m] != the last emitted score: stop]
//           emit (box[m], score[m]); remove m
//           every alive j that overlaps m:  score[j] = w(ov) * score[j];  score[j] < score_threshold: remove j
//
// with the reference's fp32 expression order (area, iw, ih, ua = t_area + area - iw*ih, ov = iw*ih / ua; IEEE division,
// no contraction) and w = (ov > Nt ? 1 - ov : 1) | (float)exp(-((double)ov*ov) / (double)sigma) | (ov > Nt ? 0 : 1).
// Hard and linear results are bit-exact against ct_cpu_soft_nms; the Gaussian weight goes through another libm's double exp
// than the host's, so its scores agree to an ulp of the weight per decay.
//
//   * row j of a segment belongs to thread j % 256 for the whole kernel: its current score (and whether it is alive) is
//     read and written by that thread alone -- in LDS while the segment has at most kLdsRows rows (boxes are staged there
//     too), in the caller's workspace otherwise (boxes then come from L2);
//   * one sweep per emitted row: a thread decays its rows against the winner and, in the same pass, finds the largest
//     64-bit key (ordered score bits << 32 | ~position) among those that stay alive; the wave maximum (DPP inside a row of
//     16 lanes, readlane across the four rows) goes to a double-buffered LDS slot, ONE barrier, every thread reads the
//     four wave maxima: the winner's position and current score are in the key itself;
//   * the trip count is uniform and at most n whatever the data holds: every trip removes the row it emits.
// No workgroup talks to another one.
//
// Compiled with -ffp-contract=off.
#include "ct_common.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsRows = 1024;              // 16 KB of boxes + 4 KB of scores: seven segments resident per CU
constexpr int kRowsInFlight = 4;            // rows a thread loads before it decays the first of them
constexpr unsigned kDead = 0xFFFFFFFFu;    // score bits of a removed row (a NaN no arithmetic here produces)

struct SoftPrm {
    float sigma, Nt, thr;
    int max_emit;
};

// float bits -> unsigned with the order of the floats (negative scores included)
__device__ __forceinline__ unsigned ordered_bits(unsigned b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ unsigned unordered_bits(unsigned o) { return o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

__device__ __forceinline__ u64 make_key(unsigned score_bits, int pos)
{
    return ((u64)ordered_bits(score_bits) << 32) | (unsigned)~pos;
}

template <int CTRL>
__device__ __forceinline__ u64 dpp_max(u64 v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, false);
    const u64 o = ((u64)(unsigned)hi << 32) | (unsigned)lo;
    return o > v ? o : v;
}

// maximum over the wave in every lane; all 64 lanes must be active
__device__ __forceinline__ u64 wave_max(u64 v)
{
    v = dpp_max<0xB1>(v);       // quad_perm [1,0,3,2]
    v = dpp_max<0x4E>(v);       // quad_perm [2,3,0,1]
    v = dpp_max<0x141>(v);      // row_half_mirror
    v = dpp_max<0x140>(v);      // row_mirror: every lane holds the maximum of its row of 16
    u64 r = 0;
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, row * 16);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), row * 16);
        const u64 o = ((u64)hi << 32) | lo;
        r = o > r ? o : r;
    }
    return r;
}

template <int METHOD>
__device__ __forceinline__ float decay_weight(float ov, const SoftPrm& p)
{
    if (METHOD == 1) return ov > p.Nt ? 1.0f - ov : 1.0f;
    if (METHOD == 2) return (float)exp(-((double)ov * (double)ov) / (double)p.sigma);
    return ov > p.Nt ? 0.0f : 1.0f;
}

// One segment: d = its n rows [x1,y1,x2,y2,score]; sc = n current scores (LDS or workspace), bx = LDS boxes (IN_LDS only).
// wb: where the emitted rows' scores are also written back in place (row m, column 4), or null.
template <bool IN_LDS, int METHOD>
__device__ __forceinline__ void soft_segment(const float* d, const int n, const SoftPrm p, float* sc, const float4* bx,
                                             u64 (*s_wmax)[kWaves], float* out_rows, int* out_pos, int* out_count,
                                             float* wb)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto box_of = [&](int j) {
        if (IN_LDS) return bx[j];
        const float* r = d + (size_t)j * 5;
        return make_float4(r[0], r[1], r[2], r[3]);
    };

    u64 local = 0;
    for (int j = tid; j < n; j += kThreads) {
        const unsigned sb = __float_as_uint(IN_LDS ? sc[j] : d[(size_t)j * 5 + 4]);
        if (!IN_LDS) sc[j] = __uint_as_float(sb);
        if (sb != kDead) {
            const u64 k = make_key(sb, j);
            local = k > local ? k : local;
        }
    }

    int emitted = 0;
    float last = 0.f;
    for (int it = 0; it < n; ++it) {
        const u64 wmax = wave_max(local);
        if (lane == 0) s_wmax[it & 1][wave] = wmax;
        __syncthreads();
        u64 key = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const u64 o = s_wmax[it & 1][w];
            key = o > key ? o : key;
        }
        if (key == 0) break;                                     // nothing alive (uniform)
        const int m = __builtin_amdgcn_readfirstlane((int)~(unsigned)key);
        const float ms = __uint_as_float(unordered_bits((unsigned)(key >> 32)));
        if (p.max_emit > 0 && emitted >= p.max_emit && ms != last) break;
        const float4 t = box_of(m);
        if (tid == (m & (kThreads - 1))) {
            sc[m] = __uint_as_float(kDead);
            if (out_rows) {
                float* r = out_rows + (size_t)emitted * 5;
                r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w; r[4] = ms;
            }
            if (wb) wb[(size_t)m * 5 + 4] = ms;
            out_pos[emitted] = m;
        }
        ++emitted;
        last = ms;

        const float tarea = (t.z - t.x + 1.0f) * (t.w - t.y + 1.0f);
        local = 0;
        auto decay_row = [&](int j, float s, const float4 b) {
            if (__float_as_uint(s) == kDead) return;
            const float area = (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f);
            const float iw = (b.z < t.z ? b.z : t.z) - (t.x < b.x ? b.x : t.x) + 1.0f;
            if (iw > 0) {
                const float ih = (b.w < t.w ? b.w : t.w) - (t.y < b.y ? b.y : t.y) + 1.0f;
                if (ih > 0) {
                    const float inter = iw * ih;
                    const float ua = tarea + area - inter;
                    const float ov = inter / ua;
                    s = decay_weight<METHOD>(ov, p) * s;
                    if (s < p.thr) {
                        sc[j] = __uint_as_float(kDead);
                        return;
                    }
                    sc[j] = s;
                }
            }
            if (__float_as_uint(s) != kDead) {                   // (a decay that lands on the marker's bits: removed)
                const u64 k = make_key(__float_as_uint(s), j);
                local = k > local ? k : local;
            }
        };
        // kRowsInFlight rows per thread and trip: their scores and boxes (dead rows' too) are loaded before the first one
        // is decayed -- through L2 one row after the other costs two dependent loads per row
        for (int j0 = tid; j0 < n; j0 += kThreads * kRowsInFlight) {
            float s[kRowsInFlight];
            float4 b[kRowsInFlight];
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) {
                const int j = j0 + u * kThreads;
                s[u] = j < n ? sc[j] : __uint_as_float(kDead);
            }
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) {
                const int j = j0 + u * kThreads;
                b[u] = j < n ? box_of(j) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) decay_row(j0 + u * kThreads, s[u], b[u]);
        }
    }
    if (tid == 0) *out_count = emitted;
}

// Segments are CSR (seg_off) or fixed-stride slots with a length array, as in nms_segments_kernel.
template <int METHOD>
__global__ __launch_bounds__(kThreads) void soft_nms_segments_kernel(const float* dets, const int* __restrict__ seg_off,
                                                                     const int* __restrict__ seg_len, const int seg_stride,
                                                                     const int max_seg_len, const SoftPrm p, float* cur_ws,
                                                                     const long long ws_rows, float* out_rows, int* __restrict__ out_pos,
                                                                     int* __restrict__ out_count, float* wb)
{
    __shared__ float4 s_box[kLdsRows];
    __shared__ float s_score[kLdsRows];
    __shared__ u64 s_wmax[2][kWaves];

    const int seg = blockIdx.x;
    const int base = seg_len ? seg * seg_stride : seg_off[seg];
    int n = seg_len ? seg_len[seg] : seg_off[seg + 1] - base;
    n = min(n, max_seg_len);
    if (n <= 0) {
        if (threadIdx.x == 0) out_count[seg] = 0;
        return;
    }
    const float* d = dets + (size_t)base * 5;
    float* orow = out_rows ? out_rows + (size_t)base * 5 : nullptr;
    float* wbs = wb ? wb + (size_t)base * 5 : nullptr;
    if (n <= kLdsRows) {
        for (int j = threadIdx.x; j < n; j += kThreads) {
            const float* r = d + (size_t)j * 5;
            s_box[j] = make_float4(r[0], r[1], r[2], r[3]);
            s_score[j] = r[4];
        }
        // (no barrier: a thread reads the scores it wrote itself; the first box of another thread's row is read after
        // the first trip's barrier)
        soft_segment<true, METHOD>(d, n, p, s_score, s_box, s_wmax, orow, out_pos + base, out_count + seg, wbs);
    } else {
        if ((long long)base + n > ws_rows) {          // the workspace was queried for fewer rows than seg_off addresses
            if (threadIdx.x == 0) out_count[seg] = -1;
            return;
        }
        soft_segment<false, METHOD>(d, n, p, cur_ws + base, nullptr, s_wmax, orow, out_pos + base, out_count + seg, wbs);
    }
}

int launch_soft(const float* dets, const int* seg_off, const int* seg_len, int seg_stride, int nseg, int max_seg_len,
                int method, float sigma, float Nt, float thr, int max_emit, float* cur_ws, long long ws_rows, float* out_rows,
                int* out_pos, int* out_count, float* wb, hipStream_t st)
{
    const SoftPrm p{sigma, Nt, thr, max_emit};
    const dim3 grid(nseg), block(kThreads);
#define CT_SOFT_LAUNCH(M)                                                                                         \
    hipLaunchKernelGGL((soft_nms_segments_kernel<M>), grid, block, 0, st, dets, seg_off, seg_len, seg_stride, \
                       max_seg_len, p, cur_ws, ws_rows, out_rows, out_pos, out_count, wb)
    CT_PROF("soft_nms_segments_kernel", st);
    switch (method) {
        case 0: CT_SOFT_LAUNCH(0); break;
        case 1: CT_SOFT_LAUNCH(1); break;
        default: CT_SOFT_LAUNCH(2); break;
    }
#undef CT_SOFT_LAUNCH
    CT_LAUNCH_CHECK("soft_nms_segments_kernel");
    return CT_OK;
}

}  // namespace

namespace ctdet {
// Fixed-stride segments (slot s = rows [s*stride, s*stride + seg_len[s])), used by ct_post.hip: keep[] receives the emitted
// positions in emission order and the emitted scores are written back into dets' own score column, so the rows
// `dets[keep[i]]` are what the top-k and gather stages expect.  cur_ws: nseg * stride floats.
int soft_nms_launch_strided(float* dets, const int* seg_len, int seg_stride, int nseg, int method, float sigma, float Nt,
                            float score_threshold, int max_emit, float* cur_ws, int* keep, int* keep_count, hipStream_t st)
{
    return launch_soft(dets, nullptr, seg_len, seg_stride, nseg, seg_stride, method, sigma, Nt, score_threshold, max_emit,
                       cur_ws, (long long)nseg * seg_stride, nullptr, keep, keep_count, dets, st);
}

// the parameter checks the two soft entries share (`who` = the entry's name)
int soft_nms_check_params(const char* who, int method, float sigma)
{
    if (method < 0 || method > 2) return fail(CT_ERR_INVALID, "%s: method %d is not 0 (hard), 1 (linear) or 2 (Gaussian)", who, method);
    if (method == 2 && !(sigma > 0.f)) return fail(CT_ERR_INVALID, "%s: sigma must be > 0 for the Gaussian method", who);
    return CT_OK;
}
}  // namespace ctdet

extern "C" int ct_soft_nms_lds_rows(void) { return kLdsRows; }

extern "C" size_t ct_soft_nms_batched_workspace_bytes(int total_rows, int num_segments)
{
    // current scores of the segments too long for LDS (one float per row) + one line per segment of slack
    return ctdet::align_up((size_t)(total_rows > 0 ? total_rows : 0) * 4, 256) +
           256 * ((size_t)(num_segments > 0 ? num_segments : 0) / 64 + 1);
}

extern "C" int ct_soft_nms_batched_dev(const float* dets, const int* seg_off, int num_segments, int max_seg_len, int method,
                                       float sigma, float Nt, float score_threshold, int max_emit, float* out_rows,
                                       int* out_pos, int* out_count, void* workspace, size_t workspace_bytes,
                                       ct_stream_t stream)
{
    CT_REQUIRE(dets && seg_off && out_rows && out_pos && out_count, "ct_soft_nms_batched_dev: null pointer");
    CT_REQUIRE(num_segments > 0 && max_seg_len >= 0 && max_emit >= 0,
               "ct_soft_nms_batched_dev: bad sizes (num_segments=%d max_seg_len=%d max_emit=%d)", num_segments, max_seg_len,
               max_emit);
    const int rc = ctdet::soft_nms_check_params("ct_soft_nms_batched_dev", method, sigma);
    if (rc != CT_OK) return rc;
    // seg_off lives on the device, so the total row count is the caller's word: the host checks what it can (the longest
    // segment fits), the kernel refuses a long segment the workspace does not cover (out_count[s] = -1) and writes nothing.
    if (!workspace) return ctdet::fail(CT_ERR_WORKSPACE, "ct_soft_nms_batched_dev: workspace is NULL");
    const size_t need = ct_soft_nms_batched_workspace_bytes(max_seg_len, num_segments);
    if (workspace_bytes < need)
        return ctdet::fail(CT_ERR_WORKSPACE, "ct_soft_nms_batched_dev: workspace %zu < %zu", workspace_bytes, need);
    return launch_soft(dets, seg_off, nullptr, 0, num_segments, max_seg_len, method, sigma, Nt, score_threshold, max_emit,
                       (float*)workspace, (long long)(workspace_bytes / 4), out_rows, out_pos, out_count, nullptr, ctdet::as_stream(stream));
}
