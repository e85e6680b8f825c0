// libctdet: Matrix NMS (Wang et al., SOLOv2 section 3.3) on the device, one workgroup per segment.
//
// The rule on one segment's rows in the pipeline's order (descending score, lower prior index first on ties); only the
// first n = min(len, pre_top) rows take part:
//
//   ov(i, j), i < j   the +1-pixel fp32 IoU of ct_soft_nms.hip (0 unless iw > 0 && ih > 0; IEEE division, no contraction)
//   cmax[i]           max over k < i of ov(k, i); cmax[0] = 0            -- how much row i was itself suppressed
//   decay[j]          min(1, min over i < j of t(i, j)); decay[0] = 1
//                       linear    t = (1 - ov(i,j)) / (1 - cmax[i]); a term with 1 - cmax[i] == 0 is skipped
//                       Gaussian  t = (float)exp(((double)cmax[i]^2 - (double)ov(i,j)^2) / (double)sigma)
//   score'[j]         score[j] * decay[j]; rows with score' < score_threshold are removed
//   emission          non-increasing score', ties lower position first; max_emit as in the soft kernel
//
// No row waits on a decision about another one: two triangular passes over the segment and one sort.
//
//   * the n rows are staged in LDS: boxes (float4), areas, scores, cmax;
//   * pass A (cmax) and pass B (decay) both evaluate the IoUs, the n x n matrix is never stored.  A thread owns whole
//     columns j and walks the rows i < j: every lane reads the same row i (an LDS broadcast).  Thread t takes the columns
//     t, t + 256, ... of the first half and their mirror images n - 1 - j, so every lane walks about n rows.  The trip
//     count is the wave's (its highest column), a lane masks the rows at or above its own j;
//   * a pair that does not overlap contributes nothing: ov = 0 gives t = 1 / (1 - cmax[i]) >= 1 (linear) or
//     exp(cmax[i]^2 / sigma) >= 1 (Gaussian), and leaves a maximum that starts at 0 alone;
//   * few rows move a running maximum or minimum, and the IEEE division is a third of a row's instructions: a row is first
//     judged by inter * rcp(ua), good to 2^-22, against the running value with a margin of 2^-16, and only a row that
//     could move it takes the IEEE quotients the contract names.  The result is the one every row would have given;
//   * the minima and maxima do not depend on the order they are taken in, so the linear method equals ct_cpu_matrix_nms bit
//     for bit.  Gaussian: (float)exp(x / sigma) does not decrease with x, so the column keeps the smallest exponent
//     numerator and takes ONE double exp: min over i of t(i, j) up to the two libms' difference, at most one fp32 ulp of
//     decay (include/ctdet.h has the bound);
//   * the 64-bit keys (ordered score' bits << 32 | ~position, 0 for removed rows and padding) are sorted in descending
//     order by a bitonic network in LDS, over the area / cmax arrays, which are dead by then; the emitted rows are a prefix.
// No workgroup talks to another one; nothing is allocated and nothing synchronises with the host.
//
// Compiled with -ffp-contract=off.
#include "ct_common.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;
constexpr int kThreads = 256;
constexpr int kMaxRows = 1024;      // 16 KB of boxes + 4 KB each of scores, areas, cmax = 28 KB: five segments resident per CU

struct MatrixPrm {
    float sigma, thr;
    int pre_top, max_emit;
};

// float bits -> unsigned with the order of the floats (negative scores included); the key layout of ct_soft_nms.hip
__device__ __forceinline__ unsigned ordered_bits(unsigned b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ unsigned unordered_bits(unsigned o) { return o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

__device__ __forceinline__ u64 make_key(unsigned score_bits, int pos)
{
    return ((u64)ordered_bits(score_bits) << 32) | (unsigned)~pos;
}

// What row i and column j share: whether they overlap, iw * ih and ua (ov = inter / ua where `hit`).  No branch: every
// operand is loaded and used whatever the boxes are, so a row costs one LDS round trip.
struct Pair {
    bool hit;
    float inter, ua;
};

__device__ __forceinline__ Pair pair_of(const float4 t, const float tarea, const float4 b, const float area)
{
    const float iw = (b.z < t.z ? b.z : t.z) - (t.x < b.x ? b.x : t.x) + 1.0f;
    const float ih = (b.w < t.w ? b.w : t.w) - (t.y < b.y ? b.y : t.y) + 1.0f;
    const float inter = iw * ih;
    return {(bool)((iw > 0) & (ih > 0)), inter, tarea + area - inter};
}

// v_rcp_f32 is good to one ulp: x * rcp(y) is within 2^-22 of the IEEE quotient, relatively.  The passes keep their running
// maximum / minimum with the IEEE quotient, but take it only for the rows this estimate cannot rule out; the margins below
// are far wider than the estimate's error, so the rows ruled out are rows that would not have changed the result.
__device__ __forceinline__ float rcp_est(float y) { return __builtin_amdgcn_rcpf(y); }
constexpr float kBelow = 1.0f - 0x1p-16f;
constexpr float kSlack = 0x1p-20f;

// The columns of thread `tid`: j = tid, tid + 256, ... below ceil(n / 2), each followed by its mirror n - 1 - j.
// f(j, bound): bound is the same for the whole wave and at least the j of each of its lanes (and at most n - 1).
template <typename F>
__device__ __forceinline__ void for_my_columns(int n, F&& f)
{
    const int half = (n + 1) >> 1;
    for (int j = threadIdx.x; j < half; j += kThreads) {
        const int jb = __builtin_amdgcn_readfirstlane(j);        // the wave's lowest column
        f(j, min(jb + 63, n - 1));
        const int m = n - 1 - j;
        if (m != j) f(m, n - 1 - jb);
    }
}

template <int METHOD>
__global__ __launch_bounds__(kThreads) void matrix_nms_segments_kernel(const float* dets, const int* __restrict__ seg_off,
                                                                       const int* __restrict__ seg_len, const int seg_stride,
                                                                       const int max_seg_len, const MatrixPrm p, float* out_rows,
                                                                       int* __restrict__ out_pos, int* __restrict__ out_count,
                                                                       float* wb)
{
    __shared__ float4 s_box[kMaxRows];
    __shared__ float s_score[kMaxRows];
    __shared__ __attribute__((aligned(16))) float s_ac[2 * kMaxRows];     // areas, cmax; then the sort keys
    float* const s_area = s_ac;
    float* const s_cmax = s_ac + kMaxRows;
    u64* const s_key = reinterpret_cast<u64*>(s_ac);
    static_assert(sizeof(u64) * kMaxRows == sizeof(float) * 2 * kMaxRows, "the keys take the place of areas and cmax");

    const int seg = blockIdx.x, tid = threadIdx.x;
    const int base = seg_len ? seg * seg_stride : seg_off[seg];
    int n = seg_len ? seg_len[seg] : seg_off[seg + 1] - base;
    n = min(min(n, max_seg_len), min(p.pre_top, kMaxRows));
    if (n <= 0) {
        if (tid == 0) out_count[seg] = 0;
        return;
    }
    const float* d = dets + (size_t)base * 5;

    for (int j = tid; j < n; j += kThreads) {
        const float* r = d + (size_t)j * 5;
        const float4 b = make_float4(r[0], r[1], r[2], r[3]);
        s_box[j] = b;
        s_area[j] = (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f);
        s_score[j] = r[4];
    }
    __syncthreads();

    // Both passes walk the rows i < bound with a trip count the wave shares (a lane's own rows are those below its j) and
    // load row i + 1 (at most bound <= n - 1) before they work on row i.

    // ---- pass A: cmax[j] = max over i < j of ov(i, j) ----
    for_my_columns(n, [&](int j, int bound) {
        const float4 b = s_box[j];
        const float area = s_area[j];
        float c = 0.0f;
        float4 t = s_box[0];
        float ta = s_area[0];
        for (int i = 0; i < bound; ++i) {
            const float4 tn = s_box[i + 1];
            const float tan = s_area[i + 1];
            const Pair q = pair_of(t, ta, b, area);
            // ov > c needs inter * rcp(ua) >= ov (1 - 2^-22) > c (1 - 2^-22)
            if (q.hit & (i < j) & (q.inter * rcp_est(q.ua) >= c * kBelow)) {
                const float ov = q.inter / q.ua;
                c = ov > c ? ov : c;
            }
            t = tn;
            ta = tan;
        }
        s_cmax[j] = c;
    });
    __syncthreads();

    // ---- pass B: decay[j], score'[j] (written over score[j], which only this thread reads) ----
    for_my_columns(n, [&](int j, int bound) {
        const float4 b = s_box[j];
        const float area = s_area[j];
        float decay = 1.0f;
        float4 t = s_box[0];
        float ta = s_area[0], cm = s_cmax[0];
        if (METHOD == 1) {
            for (int i = 0; i < bound; ++i) {
                const float4 tn = s_box[i + 1];
                const float tan = s_area[i + 1], cmn = s_cmax[i + 1];
                const Pair q = pair_of(t, ta, b, area);
                const float den = 1.0f - cm;
                const float r = rcp_est(den);
                // the term is within 2^-21 (|r| + |est|) of est; a pair that does not overlap has a term >= 1
                const float est = (1.0f - q.inter * rcp_est(q.ua)) * r;
                if (q.hit & (i < j) & (den != 0.0f) & (est * kBelow - kSlack * fabsf(r) < decay)) {
                    const float term = (1.0f - q.inter / q.ua) / den;
                    decay = term < decay ? term : decay;
                }
                t = tn;
                ta = tan;
                cm = cmn;
            }
        } else {
            double num = 0.0;                 // the smallest cmax[i]^2 - ov(i,j)^2 that is below 0 (others give t >= 1)
            float numf = 0.0f;
            for (int i = 0; i < bound; ++i) {
                const float4 tn = s_box[i + 1];
                const float tan = s_area[i + 1], cmn = s_cmax[i + 1];
                const Pair q = pair_of(t, ta, b, area);
                const float e = q.inter * rcp_est(q.ua);
                // cmax^2 - ov^2 is within 2^-20 of this fp32 estimate (both are at most 1 in size)
                if (q.hit & (i < j) & (cm * cm - e * e - 1e-5f < numf)) {
                    const float ov = q.inter / q.ua;
                    const double x = (double)cm * (double)cm - (double)ov * (double)ov;
                    num = x < num ? x : num;
                    numf = (float)num;
                }
                t = tn;
                ta = tan;
                cm = cmn;
            }
            if (num < 0.0) {
                const float tmin = (float)exp(num / (double)p.sigma);
                decay = tmin < decay ? tmin : decay;
            }
        }
        s_score[j] = s_score[j] * decay;
    });
    __syncthreads();                          // areas and cmax are dead: the keys go there

    int N = 1;
    while (N < n) N <<= 1;
    for (int i = tid; i < N; i += kThreads) {
        u64 k = 0;
        if (i < n) {
            const float s = s_score[i];
            if (!(s < p.thr)) k = make_key(__float_as_uint(s), i);
        }
        s_key[i] = k;
    }
    __syncthreads();
    // bitonic network, descending
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < N / 2; t += kThreads) {
                const int i = 2 * t - (t & (j - 1));
                const bool desc = (i & k) == 0;
                const u64 a = s_key[i], c = s_key[i + j];
                if ((a < c) == desc) {
                    s_key[i] = c;
                    s_key[i + j] = a;
                }
            }
            __syncthreads();
        }
    }

    // ---- emission: the rows that are left, a prefix of the sorted keys; max_emit cuts it except for ties with its last row ----
    const bool limited = p.max_emit > 0 && p.max_emit <= N && s_key[p.max_emit - 1] != 0;
    const float last = limited ? __uint_as_float(unordered_bits((unsigned)(s_key[p.max_emit - 1] >> 32))) : 0.0f;
    float* orow = out_rows ? out_rows + (size_t)base * 5 : nullptr;
    float* wbs = wb ? wb + (size_t)base * 5 : nullptr;
    int* opos = out_pos + base;
    int emitted = 0;
    for (int i0 = 0; i0 < N; i0 += kThreads) {
        const int i = i0 + tid;
        bool emit = false;
        if (i < N) {
            const u64 key = s_key[i];
            if (key != 0) {
                const float s = __uint_as_float(unordered_bits((unsigned)(key >> 32)));
                emit = !limited || i < p.max_emit || s == last;
                if (emit) {
                    const int pos = (int)~(unsigned)key;
                    if (orow) {
                        const float4 b = s_box[pos];
                        float* r = orow + (size_t)i * 5;
                        r[0] = b.x; r[1] = b.y; r[2] = b.z; r[3] = b.w; r[4] = s;
                    }
                    if (wbs) wbs[(size_t)pos * 5 + 4] = s;
                    opos[i] = pos;
                }
            }
        }
        emitted += __syncthreads_count(emit);
    }
    if (tid == 0) out_count[seg] = emitted;
}

int launch_matrix(const float* dets, const int* seg_off, const int* seg_len, int seg_stride, int nseg, int max_seg_len,
                  int method, float sigma, float thr, int pre_top, int max_emit, float* out_rows, int* out_pos,
                  int* out_count, float* wb, hipStream_t st)
{
    const MatrixPrm p{sigma, thr, pre_top, max_emit};
    const dim3 grid(nseg), block(kThreads);
    CT_PROF("matrix_nms_segments_kernel", st);
    if (method == 1)
        hipLaunchKernelGGL((matrix_nms_segments_kernel<1>), grid, block, 0, st, dets, seg_off, seg_len, seg_stride, max_seg_len,
                           p, out_rows, out_pos, out_count, wb);
    else
        hipLaunchKernelGGL((matrix_nms_segments_kernel<2>), grid, block, 0, st, dets, seg_off, seg_len, seg_stride, max_seg_len,
                           p, out_rows, out_pos, out_count, wb);
    CT_LAUNCH_CHECK("matrix_nms_segments_kernel");
    return CT_OK;
}

}  // namespace

namespace ctdet {
// the parameter checks the two matrix entries share (`who` = the entry's name)
int matrix_nms_check_params(const char* who, int method, float sigma, float score_threshold, int pre_top)
{
    if (method != 1 && method != 2) return fail(CT_ERR_INVALID, "%s: method %d is not 1 (linear) or 2 (Gaussian)", who, method);
    if (method == 2 && !(sigma > 0.f)) return fail(CT_ERR_INVALID, "%s: sigma must be > 0 for the Gaussian method", who);
    if (!(score_threshold >= 0.f))
        return fail(CT_ERR_INVALID, "%s: score_threshold must be >= 0 (the top-k rule compares score bits)", who);
    if (pre_top <= 0 || pre_top > kMaxRows)
        return fail(CT_ERR_INVALID, "%s: pre_top %d is outside 1 .. ct_matrix_nms_max_rows() = %d", who, pre_top, kMaxRows);
    return CT_OK;
}

// Fixed-stride segments (slot s = rows [s*stride, s*stride + seg_len[s])), used by ct_post.hip: keep[] receives the emitted
// positions in emission order and the decayed scores are written into dets' own score column, so the rows `dets[keep[i]]`
// are what the top-k and gather stages expect.
int matrix_nms_launch_strided(float* dets, const int* seg_len, int seg_stride, int nseg, int method, float sigma,
                              float score_threshold, int pre_top, int max_emit, int* keep, int* keep_count, hipStream_t st)
{
    return launch_matrix(dets, nullptr, seg_len, seg_stride, nseg, seg_stride, method, sigma, score_threshold, pre_top, max_emit,
                         nullptr, keep, keep_count, dets, st);
}
}  // namespace ctdet

extern "C" int ct_matrix_nms_max_rows(void) { return kMaxRows; }

extern "C" size_t ct_matrix_nms_batched_workspace_bytes(int total_rows, int num_segments)
{
    (void)total_rows;
    (void)num_segments;
    return 0;                                 // a segment's whole state is in LDS
}

extern "C" int ct_matrix_nms_batched_dev(const float* dets, const int* seg_off, int num_segments, int max_seg_len, int method,
                                         float sigma, float score_threshold, int pre_top, int max_emit, float* out_rows,
                                         int* out_pos, int* out_count, void* workspace, size_t workspace_bytes,
                                         ct_stream_t stream)
{
    (void)workspace;
    (void)workspace_bytes;
    CT_REQUIRE(dets && seg_off && out_rows && out_pos && out_count, "ct_matrix_nms_batched_dev: null pointer");
    CT_REQUIRE(num_segments > 0 && max_seg_len >= 0 && max_emit >= 0,
               "ct_matrix_nms_batched_dev: bad sizes (num_segments=%d max_seg_len=%d max_emit=%d)", num_segments, max_seg_len,
               max_emit);
    const int rc = ctdet::matrix_nms_check_params("ct_matrix_nms_batched_dev", method, sigma, score_threshold, pre_top);
    if (rc != CT_OK) return rc;
    return launch_matrix(dets, seg_off, nullptr, 0, num_segments, max_seg_len, method, sigma, score_threshold, pre_top, max_emit,
                         out_rows, out_pos, out_count, nullptr, ctdet::as_stream(stream));
}
