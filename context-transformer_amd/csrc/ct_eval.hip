// libctdet: PASCAL VOC evaluation on the device, fed from the [B,T,cap,5] rows ct_postprocess_batched leaves
// (data/voc0712.py:339-426 + data/voc_eval.py:134-203 without the results files).
//
//   voc_match_kernel  one workgroup per image of a pipeline batch: quantises every kept row the way the results
//                     files do ({:.1f} of box + 1, {:.3f} of the score), finds its best ground-truth box of the
//                     row's class (IoU in double, +1 pixel convention, first maximum wins) and decides true positive /
//                     false positive / neither.  The greedy "first detection takes the box" rule needs no serial
//                     walk: a row's best box does not depend on which boxes are taken, and all rows that can take a
//                     box sit in one (image, class) segment, so the box goes to the row that comes first in
//                     evaluation order -- rounded score descending, then row ascending; the stored order of a
//                     descending segment -- among those that point at it (one LDS atomicMin per row).  One (64-bit
//                     key, flag byte) record per row goes to the image's slot range of the caller's record buffer.
//   voc_pr_kernel     one workgroup per class over that class's flags in sorted key order: integer scans of tp / fp
//                     chunk by chunk with a carry, rec / prec in double, then the VOC07 11-point AP (forward pass) or
//                     the area AP (a second pass from the right: the running maximum of precision comes from there).
//
// Compiled with -ffp-contract=off: every double expression is the host's (ctdet/evaluate.py) operation for operation.
#include "ct_common.h"
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

typedef long long i64;
typedef unsigned long long u64;

constexpr int kMaxGT = CT_VOC_MAX_GT_PER_IMAGE;
constexpr int kMaxT = 1023;            // classes: 10 key bits, and class 1023 is left to the `unused` key
constexpr int kMaxCap = 4096;          // rows per segment: 12 key bits
constexpr int kMaxImages = 1 << 21;    // data set images: 21 key bits
constexpr int kMaxN = (1 << 20) - 1;   // rounded score * 1000: 20 key bits
constexpr int kThreads = 256;

// float('{:.1f}'.format(c + 1)) for an fp32 coordinate: the + 1 in fp32 (numpy on the float32 array), the product by ten
// exact in double (24 x 4 bits), rint = half-even like format on an exactly representable tie, one correctly rounded
// division
__device__ __forceinline__ double quant_coord(float c)
{
    return rint((double)(c + 1.0f) * 10.0) / 10.0;
}

// '{:.3f}'.format(s) as the integer it prints, kMaxN - n so that ascending = descending score; -> false when n is
// outside the key's 20 bits (negative, above 1048.575 or NaN: not a detector's score; clamped)
__device__ __forceinline__ bool score_rank(float s, unsigned* nrev)
{
    const double nd = rint((double)s * 1000.0);
    const bool ok = nd >= 0. && nd <= (double)kMaxN;
    *nrev = (unsigned)kMaxN - (ok ? (unsigned)nd : nd > 0. ? (unsigned)kMaxN : 0u);
    return ok;
}

struct Best {
    int j;
    double iou;
};

// data/voc_eval.py:166-180 for one row against the image's boxes of class `label` (in LDS, stored order)
__device__ __forceinline__ Best best_match(const float* __restrict__ row, int label, int ng,
                                           const float4* s_box, const int* s_label)
{
    const double b0 = quant_coord(row[0]), b1 = quant_coord(row[1]);
    const double b2 = quant_coord(row[2]), b3 = quant_coord(row[3]);
    const double area_b = (b2 - b0 + 1.) * (b3 - b1 + 1.);
    Best best{-1, -INFINITY};
    for (int g = 0; g < ng; ++g) {
        if (s_label[g] != label) continue;
        const float4 q = s_box[g];
        const double g0 = q.x, g1 = q.y, g2 = q.z, g3 = q.w;
        const double iw = fmax(fmin(g2, b2) - fmax(g0, b0) + 1., 0.);
        const double ih = fmax(fmin(g3, b3) - fmax(g1, b1) + 1., 0.);
        const double inter = iw * ih;
        const double uni = (area_b + (g2 - g0 + 1.) * (g3 - g1 + 1.)) - inter;
        const double iou = inter / uni;
        if (iou > best.iou) {              // strict: the first maximum wins, as np.argmax
            best.j = g;
            best.iou = iou;
        }
    }
    return best;
}

__global__ __launch_bounds__(kThreads) void voc_match_kernel(
    const float* __restrict__ dets, const int* __restrict__ count, int T, int cap,
    const int* __restrict__ image_index, int N, const float4* __restrict__ gt_boxes,
    const int* __restrict__ gt_label, const uint8_t* __restrict__ gt_difficult, const int* __restrict__ gt_off, int G,
    double ovthresh, i64* __restrict__ rec_key, uint8_t* __restrict__ rec_flag, int per_image_cap,
    int* __restrict__ status)
{
    __shared__ float4 s_box[kMaxGT];
    __shared__ int s_label[kMaxGT];
    __shared__ unsigned s_first[kMaxGT];   // (kMaxN - n) << 12 | row of the row that takes the box: the `det` flags of
                                           // voc_eval.py:139,183-187
    __shared__ uint8_t s_diff[kMaxGT];
    __shared__ int s_off[kMaxT + 2];       // exclusive prefix of the image's segment lengths
    __shared__ int s_part[kThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    // every exit below is uniform over the workgroup
    const int img = image_index[b];
    if (img < 0) return;                   // padding image of a ragged batch
    if (img >= N) {
        if (tid == 0) atomicOr(status, CT_VOC_BAD_INDEX);
        return;
    }
    const int g_begin = gt_off[img], g_end = gt_off[img + 1];
    const int ng = g_end - g_begin;
    if (g_begin < 0 || g_end < g_begin || g_end > G || ng > kMaxGT) {
        if (tid == 0) atomicOr(status, CT_VOC_BAD_INDEX);
        return;
    }
    for (int g = tid; g < ng; g += kThreads) {
        s_box[g] = gt_boxes[g_begin + g];
        s_label[g] = gt_label[g_begin + g];
        s_diff[g] = gt_difficult[g_begin + g];
        s_first[g] = ~0u;
    }
    // prefix over out_count[b, :] (clamped to the rows that exist): thread t owns `per` consecutive classes
    const int per = (T + kThreads - 1) / kThreads;
    const int c_lo = min(tid * per, T), c_hi = min(c_lo + per, T);
    int mine = 0;
    for (int c = c_lo; c < c_hi; ++c) mine += min(max(count[b * T + c], 0), cap);
    s_part[tid] = mine;
    __syncthreads();
    int run = 0;
    for (int t = 0; t < tid; ++t) run += s_part[t];
    for (int c = c_lo; c < c_hi; ++c) {
        s_off[c] = run;
        run += min(max(count[b * T + c], 0), cap);
    }
    if (tid == kThreads - 1) s_off[T] = run;
    __syncthreads();
    const int total = s_off[T];
    if (tid == 0) atomicMax(status + 1, total);
    if (total > per_image_cap) {           // the image's slot range cannot take its rows: nothing is written
        if (tid == 0) atomicOr(status, CT_VOC_OVERFLOW);
        return;
    }
    auto segment_of = [&](int e) {         // last class c with s_off[c] <= e (empty classes share an offset)
        int lo = 0, hi = T;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= e) lo = mid; else hi = mid;
        }
        return lo;
    };
    // pass 1: who takes which box
    for (int e = tid; e < total; e += kThreads) {
        const int c = segment_of(e);
        const int r = e - s_off[c];
        const float* row = dets + ((size_t)(b * T + c) * cap + r) * 5;
        const Best m = best_match(row, c + 1, ng, s_box, s_label);
        unsigned nrev;
        score_rank(row[4], &nrev);
        if (m.j >= 0 && m.iou > ovthresh && !s_diff[m.j]) atomicMin(&s_first[m.j], (nrev << 12) | (unsigned)r);
    }
    __syncthreads();
    // pass 2: the records (the match is computed again rather than kept: an image may have more rows than LDS holds)
    for (int e = tid; e < total; e += kThreads) {
        const int c = segment_of(e), r = e - s_off[c];
        const float* row = dets + ((size_t)(b * T + c) * cap + r) * 5;
        const Best m = best_match(row, c + 1, ng, s_box, s_label);
        unsigned nrev;
        if (!score_rank(row[4], &nrev)) atomicOr(status, CT_VOC_BAD_SCORE);
        uint8_t flag = CT_VOC_FP;
        if (m.j >= 0 && m.iou > ovthresh) {
            if (s_diff[m.j]) flag = CT_VOC_NEITHER;
            else if (s_first[m.j] == ((nrev << 12) | (unsigned)r)) flag = CT_VOC_TP;
        }
        const size_t slot = (size_t)img * per_image_cap + e;
        rec_key[slot] = ((i64)c << 53) | ((i64)nrev << 33) | ((i64)img << 12) | (i64)r;
        rec_flag[slot] = flag;
    }
}

// ---- precision / recall / AP ------------------------------------------------------------------------------------
constexpr int kItems = 8;
constexpr int kChunk = kThreads * kItems;

struct Thresholds {
    double t[CT_VOC_MAX_THRESHOLDS];
};

// inclusive scans over the workgroup in thread order; s_w: one slot per wave
__device__ __forceinline__ int block_scan_add(int v, int* s_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += s_w[w];
    __syncthreads();
    return x + base;
}

__device__ __forceinline__ double block_scan_max(double v, double* s_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double y = __shfl_up(x, off);
        if (lane >= off) x = fmax(x, y);
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    double base = 0.;                      // precisions are >= 0
    for (int w = 0; w < wave; ++w) base = fmax(base, s_w[w]);
    __syncthreads();
    return fmax(x, base);
}

__global__ __launch_bounds__(kThreads) void voc_pr_kernel(
    const uint8_t* __restrict__ rec_flag, const i64* __restrict__ order, i64 num_records,
    const i64* __restrict__ cls_off, const int* __restrict__ num_pos, Thresholds thr, int nthr,
    double* __restrict__ rec_out, double* __restrict__ prec_out, double* __restrict__ ap_out,
    int* __restrict__ status)
{
    __shared__ int s_wi[kThreads / 64];
    __shared__ double s_wd[kThreads / 64];
    __shared__ int s_tot;
    __shared__ double s_carry_max;
    __shared__ u64 s_pmax[CT_VOC_MAX_THRESHOLDS];
    __shared__ double s_sum[kThreads];
    const int c = blockIdx.x, tid = threadIdx.x;
    const i64 o0 = cls_off[c], o1 = cls_off[c + 1];
    if (o0 < 0 || o1 < o0 || o1 > num_records) {       // uniform
        if (tid == 0) {
            atomicOr(status, CT_VOC_BAD_INDEX);
            ap_out[c] = NAN;
        }
        return;
    }
    const i64 n = o1 - o0;
    const double dpos = (double)num_pos[c];
    auto flag_at = [&](i64 i) -> int {                  // flag of the class's i-th row in sorted order
        i64 at = o0 + i;
        if (order) {
            at = order[at];
            if (at < 0 || at >= num_records) {
                atomicOr(status, CT_VOC_BAD_INDEX);
                return CT_VOC_NEITHER;
            }
        }
        return rec_flag[at];
    };
    if (tid < CT_VOC_MAX_THRESHOLDS) s_pmax[tid] = 0ull;
    __syncthreads();

    // ---- forward: cumulative tp / fp, rec, prec, the 11-point maxima ----
    double pmax[CT_VOC_MAX_THRESHOLDS];
#pragma unroll
    for (int k = 0; k < CT_VOC_MAX_THRESHOLDS; ++k) pmax[k] = 0.;
    int carry_tp = 0, carry_fp = 0;
    for (i64 base = 0; base < n; base += kChunk) {
        int f[kItems], v = 0;                           // v: tp in the low, fp in the high half (a chunk has 2048 rows)
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            const i64 i = base + tid * kItems + u;
            f[u] = i < n ? flag_at(i) : CT_VOC_NEITHER;
            v += (f[u] == CT_VOC_TP ? 1 : 0) + (f[u] == CT_VOC_FP ? 1 << 16 : 0);
        }
        const int incl = block_scan_add(v, s_wi);
        if (tid == kThreads - 1) s_tot = incl;
        int tp = carry_tp + ((incl - v) & 0xFFFF), fp = carry_fp + ((incl - v) >> 16);
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            const i64 i = base + tid * kItems + u;
            tp += f[u] == CT_VOC_TP;
            fp += f[u] == CT_VOC_FP;
            if (i < n) {
                const double rec = (double)tp / dpos;
                const double prec = (double)tp / fmax((double)tp + (double)fp, DBL_EPSILON);
                if (rec_out) rec_out[o0 + i] = rec;
                if (prec_out) prec_out[o0 + i] = prec;
#pragma unroll
                for (int k = 0; k < CT_VOC_MAX_THRESHOLDS; ++k)
                    if (k < nthr && rec >= thr.t[k]) pmax[k] = fmax(pmax[k], prec);
            }
        }
        __syncthreads();
        carry_tp += s_tot & 0xFFFF;
        carry_fp += s_tot >> 16;
        __syncthreads();
    }
    if (nthr > 0) {
        // data/voc_eval.py:41-48.  A maximum does not depend on the order it is taken in, and the bit pattern of a
        // non-negative double orders like the value.
#pragma unroll
        for (int k = 0; k < CT_VOC_MAX_THRESHOLDS; ++k)
            if (k < nthr && pmax[k] > 0.) atomicMax(&s_pmax[k], (u64)__double_as_longlong(pmax[k]));
        __syncthreads();
        if (tid == 0) {
            double ap = 0.;
            for (int k = 0; k < nthr; ++k) ap = ap + __longlong_as_double((i64)s_pmax[k]) / (double)nthr;
            ap_out[c] = ap;
        }
        return;
    }

    // ---- area metric (data/voc_eval.py:50-65): from the right, where the running maximum of precision comes from ----
    if (n == 0) {
        if (tid == 0) ap_out[c] = 0.;                   // mrec = [0, 1], mpre = [0, 0]
        return;
    }
    const int all_tp = carry_tp, all_fp = carry_fp;
    int suf_tp = 0, suf_fp = 0;                         // tp / fp among the rows right of the chunk
    double sum = 0.;
    if (tid == 0) s_carry_max = 0.;
    __syncthreads();
    for (i64 end = n; end > 0; end -= kChunk) {
        // thread order = descending row order: item (tid, u) is row end - 1 - (tid * kItems + u)
        int f[kItems], v = 0;
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            const i64 i = end - 1 - (tid * kItems + u);
            f[u] = i >= 0 ? flag_at(i) : CT_VOC_NEITHER;
            v += (f[u] == CT_VOC_TP ? 1 : 0) + (f[u] == CT_VOC_FP ? 1 << 16 : 0);
        }
        const int incl = block_scan_add(v, s_wi);
        if (tid == kThreads - 1) s_tot = incl;
        int right_tp = suf_tp + ((incl - v) & 0xFFFF), right_fp = suf_fp + ((incl - v) >> 16);
        double prec[kItems], rec[kItems], rec_prev[kItems], local = 0.;
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            const i64 i = end - 1 - (tid * kItems + u);
            const int tp = all_tp - right_tp, fp = all_fp - right_fp;          // cumulative counts at row i
            right_tp += f[u] == CT_VOC_TP;
            right_fp += f[u] == CT_VOC_FP;
            rec[u] = (double)tp / dpos;
            rec_prev[u] = i > 0 ? (double)(tp - (f[u] == CT_VOC_TP)) / dpos : 0.;
            prec[u] = i >= 0 ? (double)tp / fmax((double)tp + (double)fp, DBL_EPSILON) : 0.;
            local = fmax(local, prec[u]);
        }
        const double incl_max = block_scan_max(local, s_wd);
        // maximum over the rows right of this thread's: the threads before it and the chunks before this one
        double run = fmax(s_carry_max, __shfl_up(incl_max, 1));
        if ((tid & 63) == 0) {
            run = s_carry_max;
            for (int w = 0; w < (tid >> 6); ++w) run = fmax(run, s_wd[w]);
        }
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            const i64 i = end - 1 - (tid * kItems + u);
            run = fmax(run, prec[u]);                   // mpre[i + 1]
            if (i >= 0 && rec[u] != rec_prev[u]) sum += (rec[u] - rec_prev[u]) * run;
        }
        __syncthreads();
        suf_tp += s_tot & 0xFFFF;
        suf_fp += s_tot >> 16;
        if (tid == kThreads - 1) s_carry_max = fmax(s_carry_max, incl_max);
        __syncthreads();
    }
    s_sum[tid] = sum;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) s_sum[tid] += s_sum[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        const double last = (double)all_tp / dpos;      // mrec[n]; the closing step to mrec[n + 1] = 1 meets mpre = 0
        double ap = s_sum[0];
        if (1. != last) ap += (1. - last) * 0.;
        ap_out[c] = ap;
    }
}

}  // namespace

extern "C" int ct_voc_match(const float* out_dets, const int* out_count, int batch, int num_fg, int cap,
                            const int* image_index, int num_images, const float* gt_boxes, const int* gt_label,
                            const uint8_t* gt_difficult, const int* gt_off, int num_gt, int max_gt_per_image,
                            double ovthresh, long long* rec_key, uint8_t* rec_flag, int per_image_cap, int* status,
                            ct_stream_t stream)
{
    CT_REQUIRE(batch > 0 && num_fg > 0 && cap > 0 && num_images > 0 && num_gt >= 0 && max_gt_per_image >= 0 &&
                   per_image_cap > 0,
               "ct_voc_match: bad sizes (batch %d, num_fg %d, cap %d, num_images %d, num_gt %d, max_gt_per_image %d, "
               "per_image_cap %d)", batch, num_fg, cap, num_images, num_gt, max_gt_per_image, per_image_cap);
    CT_REQUIRE(out_dets && out_count && image_index && gt_boxes && gt_label && gt_difficult && gt_off && rec_key &&
                   rec_flag && status, "ct_voc_match: null pointer");
    CT_REQUIRE(max_gt_per_image <= kMaxGT, "ct_voc_match: %d ground-truth boxes in one image (at most %d)",
               max_gt_per_image, kMaxGT);
    CT_REQUIRE(num_fg <= kMaxT && cap <= kMaxCap && num_images <= kMaxImages,
               "ct_voc_match: num_fg %d (<= %d), cap %d (<= %d), num_images %d (<= %d): the 64-bit key has 10 + 12 + 21 "
               "bits for them", num_fg, kMaxT, cap, kMaxCap, num_images, kMaxImages);
    CT_REQUIRE(ovthresh == ovthresh, "ct_voc_match: ovthresh is NaN");
    hipLaunchKernelGGL(voc_match_kernel, dim3(batch), dim3(kThreads), 0, ctdet::as_stream(stream), out_dets, out_count,
                       num_fg, cap, image_index, num_images, (const float4*)gt_boxes, gt_label, gt_difficult, gt_off,
                       num_gt, ovthresh, rec_key, rec_flag, per_image_cap, status);
    CT_LAUNCH_CHECK("voc_match_kernel");
    return CT_OK;
}

extern "C" int ct_voc_pr(const uint8_t* rec_flag, const long long* order, long long num_records,
                         const long long* cls_off, const int* num_pos, int num_fg, const double* thresholds_host,
                         int num_thresholds, double* rec_out, double* prec_out, double* ap_out, int* status,
                         ct_stream_t stream)
{
    CT_REQUIRE(num_records >= 0 && num_fg > 0 && num_fg <= kMaxT && num_thresholds >= 0 &&
                   num_thresholds <= CT_VOC_MAX_THRESHOLDS,
               "ct_voc_pr: bad sizes (num_records %lld, num_fg %d, num_thresholds %d)", num_records, num_fg,
               num_thresholds);
    CT_REQUIRE(rec_flag && cls_off && num_pos && ap_out && status && (thresholds_host || num_thresholds == 0),
               "ct_voc_pr: null pointer");
    Thresholds thr{};
    for (int k = 0; k < num_thresholds; ++k) thr.t[k] = thresholds_host[k];
    hipLaunchKernelGGL(voc_pr_kernel, dim3(num_fg), dim3(kThreads), 0, ctdet::as_stream(stream), rec_flag, order,
                       num_records, cls_off, num_pos, thr, num_thresholds, rec_out, prec_out, ap_out, status);
    CT_LAUNCH_CHECK("voc_pr_kernel");
    return CT_OK;
}
