// libctdet: COCO bbox evaluation (AP / AR at IoU .50:.95) on the device, fed from the [B,T,cap,5] rows
// ct_postprocess_batched leaves (utils/pycocotools/cocoeval.py evaluate / accumulate with iouType 'bbox', useCats = 1,
// and maskApi.c bbIou, without the results JSON).  Host twin: ctdet/evaluate.py coco_eval_arrays.
//
//   coco_match_kernel  grid (image of the batch, class slice), ONE 64-lane wave per workgroup.  A workgroup walks the
//                      (image, class) segments of its slice that have rows.  Per segment: the category's boxes of the
//                      image are gathered in annotation order into LDS (double), every area range's walk order (ignored
//                      boxes last, stable) is found by counting, the stable descending-score rank of every row by
//                      counting too (nothing assumes a sorted segment), ranks >= 100 are dropped.  Then the greedy walk
//                      of evaluateImg, which IS serial in the detections: per detection the wave first fills one row of
//                      IoUs (lane = box), then lane = (threshold, area range) pair walks the boxes in its range's
//                      order against its own bit of the boxes' `taken` words.  Two ballots give the record's masks.
//                      Why one wave per workgroup instead of several segments per workgroup: the IoU row and the
//                      `taken` words go from lane to lane through LDS, so every detection needs a barrier, and the
//                      segments of an image have different lengths -- with a workgroup of one wave __syncthreads() is
//                      that barrier and costs nothing, and occupancy is the same: a workgroup holds 14 KiB of the
//                      160 KiB LDS of a CU (boxes 8 KiB, IoU row 2 KiB, taken 2 KiB, orders 1 KiB, ...), i.e. 11 waves
//                      per CU next to each other, where the walk is latency bound and wants no more.
//                      That budget is what sets CT_COCO_MAX_GT_PER_SEGMENT = 256.
//   coco_acc_kernel    one workgroup per (category, area range, detection limit), one wave per IoU threshold.  The
//                      waves of a workgroup read the same records (the second to the tenth hit the cache) and share no
//                      state: each scans its own tp / fp with wave shuffles only, so the chunk loop holds no barrier.
//                      Chosen over one workgroup looping over the thresholds because the work per threshold is a
//                      chain of scans over the same rows -- ten waves run the ten chains at once from one fetch -- and
//                      over one thread block per threshold because all ten share rec_thrs and the category bounds.
//                      A wave goes over the category's rows twice: totals first, then from the right in chunks of
//                      CT_COCO_ACC_CHUNK rows with a carry, because the precision envelope is a running maximum from
//                      the right; at a row that raises tp (or the first row) the recall samples between the previous
//                      and the new recall take the envelope and the score there -- searchsorted(rc, rec_thrs, 'left').
//
// Compiled with -ffp-contract=off: every double expression is the host's, operation for operation; tp / fp are integers.
#include "ct_common.h"
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

typedef long long i64;
typedef unsigned long long u64;

constexpr int kMaxGT = CT_COCO_MAX_GT_PER_SEGMENT;
constexpr int kMaxDets = CT_COCO_MAX_DETS;
constexpr int kMaxThr = CT_COCO_MAX_IOU_THRS;
constexpr int kMaxArea = CT_COCO_MAX_AREA_RNG;
constexpr int kMaxRec = CT_COCO_MAX_REC_THRS;
constexpr int kMaxClasses = CT_COCO_MAX_CATEGORIES;     // 7 key bits; 127 belongs to the `unused` key
constexpr int kMaxImages = CT_COCO_MAX_IMAGES;          // 17 key bits
constexpr int kMaxCap = 4096;                           // rows per segment: 16-bit row numbers in LDS
constexpr int kWave = 64;
constexpr int kMaxSlices = 16;

static_assert(kMaxGT <= 256, "walk orders are stored as bytes");
static_assert(kMaxDets <= 128 && kMaxThr * kMaxArea <= 64, "7 rank bits in the key, one mask bit per pair");

// the order-preserving 32-bit image of a float32 score, inverted: ascending = descending score.  -0 counts as +0 (the
// host compares values); a NaN still gets a place, so that the ranks stay a permutation, and is reported.
__device__ __forceinline__ unsigned score_key(float s)
{
    if (s == 0.0f) s = 0.0f;
    unsigned u = __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

__device__ __forceinline__ float key_score(i64 key)
{
    unsigned u = ~(unsigned)((u64)key >> 24);
    u = (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
    return __uint_as_float(u);
}

__global__ __launch_bounds__(kWave) void coco_match_kernel(
    const float* __restrict__ dets, const int* __restrict__ count, int T, int cap,
    const int* __restrict__ image_index, const int* __restrict__ image_rank, int N,
    const double* __restrict__ gt_boxes, const double* __restrict__ gt_area, const uint8_t* __restrict__ gt_iscrowd,
    const int* __restrict__ gt_label, const int* __restrict__ gt_off, int G, const int* __restrict__ cat_rank,
    const double* __restrict__ iou_thrs, int n_thr, const double* __restrict__ area_rng, int n_area,
    i64* __restrict__ rec_key, u64* __restrict__ rec_matched, u64* __restrict__ rec_ignored, int per_image_cap,
    int* __restrict__ status)
{
    __shared__ double s_box[kMaxGT][4];
    __shared__ double s_iou[kMaxGT];
    __shared__ u64 s_taken[kMaxGT];                     // bit p: pair p has matched this box (gtm of evaluateImg)
    __shared__ uint8_t s_order[kMaxArea][kMaxGT];       // walk position -> box, per area range
    __shared__ uint8_t s_flag[kMaxGT];                  // bit a: ignored in area range a; bit 4: crowd
    __shared__ unsigned short s_row[kMaxDets];          // rank -> row of the segment
    __shared__ int s_off[kMaxClasses + 2];              // exclusive prefix of the image's kept rows per class
    const int b = blockIdx.x, lane = threadIdx.x;
    // the workgroup is one wave: every exit and every `continue` below is uniform over it
    const int pos = image_index[b];
    if (pos < 0) return;                                // padding image of a ragged batch: its rows are never read
    if (pos >= N) {
        if (lane == 0) atomicOr(status, CT_COCO_BAD_INDEX);
        return;
    }
    const int img = image_rank ? image_rank[pos] : pos;
    if (img < 0 || img >= N) {
        if (lane == 0) atomicOr(status, CT_COCO_BAD_INDEX);
        return;
    }
    const int g_begin = gt_off[img], g_end = gt_off[img + 1];
    if (g_begin < 0 || g_end < g_begin || g_end > G) {
        if (lane == 0) atomicOr(status, CT_COCO_BAD_INDEX);
        return;
    }
    for (int c = lane; c < T; c += kWave) s_off[c + 1] = min(min(max(count[b * T + c], 0), cap), kMaxDets);
    __syncthreads();
    if (lane == 0) {
        int run = 0;
        for (int c = 0; c < T; ++c) {
            const int k = s_off[c + 1];
            s_off[c] = run;
            run += k;
        }
        s_off[T] = run;
    }
    __syncthreads();
    const int total = s_off[T];
    if (blockIdx.y == 0 && lane == 0) atomicMax(status + 1, total);
    if (total > per_image_cap) {                        // the image's slot range cannot take its rows: nothing is written
        if (blockIdx.y == 0 && lane == 0) atomicOr(status, CT_COCO_OVERFLOW);
        return;
    }
    const int npairs = n_thr * n_area;
    const bool active = lane < npairs;
    const int my_a = active ? lane % n_area : 0;
    const double my_thr = active ? iou_thrs[lane / n_area] : 2.;
    const double my_lo = area_rng[2 * my_a], my_hi = area_rng[2 * my_a + 1];

    for (int c = blockIdx.y; c < T; c += gridDim.y) {
        const int n = min(max(count[b * T + c], 0), cap);
        if (n == 0) continue;
        const int kc = cat_rank[c];
        if (kc < 0 || kc >= kMaxClasses) {
            if (lane == 0) atomicOr(status, CT_COCO_BAD_INDEX);
            continue;
        }
        const float* seg = dets + (size_t)(b * T + c) * cap * 5;
        __syncthreads();                                // the previous segment's LDS is no longer read
        // the category's boxes of this image, in annotation order
        int ng = 0;
        for (int base = g_begin; base < g_end; base += kWave) {
            const int g = base + lane;
            const bool hit = g < g_end && gt_label[g] == c + 1;
            const u64 mask = __ballot(hit);
            const int p = ng + __popcll(mask & ((1ull << lane) - 1ull));
            if (hit && p < kMaxGT) {
                const double area = gt_area[g];
                const int crowd = gt_iscrowd[g] ? 1 : 0;
                int f = crowd << 4;
                for (int a = 0; a < n_area; ++a)
                    if (crowd || area < area_rng[2 * a] || area > area_rng[2 * a + 1]) f |= 1 << a;
                s_flag[p] = (uint8_t)f;
                s_taken[p] = 0ull;
#pragma unroll
                for (int k = 0; k < 4; ++k) s_box[p][k] = gt_boxes[(size_t)g * 4 + k];
            }
            ng += __popcll(mask);
        }
        if (ng > kMaxGT) {
            if (lane == 0) atomicOr(status, CT_COCO_BAD_INDEX);
            continue;
        }
        __syncthreads();
        // walk order per area range: a stable partition, ignored boxes last (np.argsort of _ignore, mergesort)
        for (int g = lane; g < ng; g += kWave) {
            const int f = s_flag[g];
            for (int a = 0; a < n_area; ++a) {
                int before = 0, regular = 0;
                for (int h = 0; h < ng; ++h) {
                    const int reg = !((s_flag[h] >> a) & 1);
                    regular += reg;
                    before += reg & (h < g);
                }
                s_order[a][((f >> a) & 1) ? regular + (g - before) : before] = (uint8_t)g;
            }
        }
        // rank by counting: rows with a greater score, or an equal score and a smaller row number
        for (int r = lane; r < n; r += kWave) {
            const float s = seg[r * 5 + 4];
            if (s != s) atomicOr(status, CT_COCO_BAD_SCORE);
            const unsigned key = score_key(s);
            int rank = 0;
            for (int q = 0; q < n; ++q) {
                const unsigned kq = score_key(seg[q * 5 + 4]);
                rank += (kq < key) | ((kq == key) & (q < r));
            }
            if (rank < kMaxDets) s_row[rank] = (unsigned short)r;
        }
        __syncthreads();
        const int kept = min(n, kMaxDets), e0 = s_off[c];
        for (int d = 0; d < kept; ++d) {
            const int r = s_row[d];
            const float* row = seg + r * 5;
            // data/coco.py:248-252 in double: [x, y, w, h] = [x1, y1, x2 - x1 + 1, y2 - y1 + 1]; loadRes: area = w * h
            const double D0 = (double)row[0], D1 = (double)row[1];
            const double D2 = (double)row[2] - D0 + 1., D3 = (double)row[3] - D1 + 1.;
            const double da = D2 * D3;
            for (int g = lane; g < ng; g += kWave) {    // maskApi.c bbIou
                const double G0 = s_box[g][0], G1 = s_box[g][1], G2 = s_box[g][2], G3 = s_box[g][3];
                const double ga = G2 * G3;
                double iou = 0.;
                const double w = fmin(D2 + D0, G2 + G0) - fmax(D0, G0);
                if (!(w <= 0.)) {
                    const double h = fmin(D3 + D1, G3 + G1) - fmax(D1, G1);
                    if (!(h <= 0.)) {
                        const double i = w * h;
                        const double u = (s_flag[g] & 16) ? da : (da + ga) - i;
                        iou = i / u;
                    }
                }
                s_iou[g] = iou;
            }
            __syncthreads();
            // cocoeval.py:274-296 for this lane's (threshold, area range)
            int m = -1;
            bool regular = false;                       // holds a match to a box that is not ignored
            if (active) {
                double best = my_thr;
                for (int p = 0; p < ng; ++p) {
                    const int g = s_order[my_a][p];
                    const int f = s_flag[g];
                    const bool ig = (f >> my_a) & 1;
                    if (((s_taken[g] >> lane) & 1ull) && !(f & 16)) continue;
                    if (m >= 0 && regular && ig) break;
                    const double v = s_iou[g];
                    if (v < best) continue;
                    best = v;
                    m = g;
                    regular = !ig;
                }
                if (m >= 0) atomicOr(&s_taken[m], 1ull << lane);        // only this lane reads or sets this bit
            }
            const bool matched = active && m >= 0;
            const bool ignored = active && (matched ? !regular : (da < my_lo || da > my_hi));
            const u64 mm = __ballot(matched), mi = __ballot(ignored);
            if (lane == 0) {
                const size_t slot = (size_t)img * per_image_cap + e0 + d;
                rec_key[slot] = ((i64)kc << 56) | ((i64)score_key(row[4]) << 24) | ((i64)img << 7) | (i64)d;
                rec_matched[slot] = mm;
                rec_ignored[slot] = mi;
            }
            __syncthreads();                            // s_iou is written again, s_taken read again
        }
    }
}

// ---- accumulate ---------------------------------------------------------------------------------------------------
constexpr int kItems = CT_COCO_ACC_CHUNK / kWave;

__device__ __forceinline__ int wave_scan_add(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int y = __shfl_up(v, off);
        if (lane >= off) v += y;
    }
    return v;
}

__device__ __forceinline__ double wave_scan_max(double v, int lane)
{
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const double y = __shfl_up(v, off);
        if (lane >= off) v = fmax(v, y);
    }
    return v;
}

// number of thresholds <= x in the ascending s_thr[0 .. R)
__device__ __forceinline__ int count_le(const double* s_thr, int R, double x)
{
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_thr[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kMaxThr * kWave) void coco_acc_kernel(
    const i64* __restrict__ rec_key, const u64* __restrict__ rec_matched, const u64* __restrict__ rec_ignored,
    const i64* __restrict__ order, i64 num_records, const i64* __restrict__ cat_off, const int* __restrict__ npig,
    int K, int A, int M, const int* __restrict__ max_dets, const double* __restrict__ rec_thrs, int R,
    double* __restrict__ precision, double* __restrict__ recall, double* __restrict__ scores, int* __restrict__ status)
{
    __shared__ double s_thr[kMaxRec];
    __shared__ double s_q[kMaxThr][kMaxRec];
    __shared__ double s_ss[kMaxThr][kMaxRec];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), t = tid >> 6;
    const int m = blockIdx.x % M, a = (blockIdx.x / M) % A, k = blockIdx.x / (M * A);
    const int bit = t * A + a;
    const int np = npig[k * A + a];
    const size_t rc_at = (((size_t)t * K + k) * A + a) * M + m;
    auto pr_at = [&](int r) { return ((((size_t)t * R + r) * K + k) * A + a) * M + m; };
    const i64 o0 = cat_off[k], o1 = cat_off[k + 1];
    const bool bad = o0 < 0 || o1 < o0 || o1 > num_records;
    // uniform over the workgroup
    if (np == 0 || bad) {
        if (bad && tid == 0) atomicOr(status, CT_COCO_BAD_INDEX);
        for (int r = lane; r < R; r += kWave) {
            precision[pr_at(r)] = -1.;
            scores[pr_at(r)] = -1.;
        }
        if (lane == 0) recall[rc_at] = -1.;
        return;
    }
    const i64 n = o1 - o0;
    const int limit = max_dets[m];
    const double dnp = (double)np;
    for (int r = tid; r < R; r += blockDim.x) s_thr[r] = rec_thrs[r];
    for (int r = lane; r < R; r += kWave) {
        s_q[t][r] = 0.;
        s_ss[t][r] = 0.;
    }
    __syncthreads();
    // row i of the category in sorted order -> slot, or -1; bits: 1 = counts (rank < limit), 2 = tp, 4 = fp
    auto slot_of = [&](i64 i) -> i64 {
        i64 at = o0 + i;
        if (order) {
            at = order[at];
            if (at < 0 || at >= num_records) {
                atomicOr(status, CT_COCO_BAD_INDEX);
                return -1;
            }
        }
        return at;
    };
    auto bits_of = [&](i64 at) -> int {
        if (at < 0) return 0;
        if ((int)(rec_key[at] & 127) >= limit) return 0;
        const int mt = (int)((rec_matched[at] >> bit) & 1ull), ig = (int)((rec_ignored[at] >> bit) & 1ull);
        return 1 | ((mt & !ig) << 1) | ((!mt & !ig) << 2);
    };
    // totals
    int all_tp = 0, all_fp = 0, all_n = 0;
    for (i64 i = lane; i < n; i += kWave) {
        const int f = bits_of(slot_of(i));
        all_n += f & 1;
        all_tp += (f >> 1) & 1;
        all_fp += (f >> 2) & 1;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        all_n += __shfl_xor(all_n, off);
        all_tp += __shfl_xor(all_tp, off);
        all_fp += __shfl_xor(all_fp, off);
    }
    // from the right, where the running maximum of precision comes from
    int right_n = 0, right_tp = 0, right_fp = 0;        // among the rows right of the chunk
    double right_max = 0.;                              // precisions are >= 0
    for (i64 end = n; end > 0; end -= CT_COCO_ACC_CHUNK) {
        // lane order = descending row order: item (lane, u) is row end - 1 - (lane * kItems + u)
        i64 at[kItems];
        int f[kItems], loc_n = 0, loc_tp = 0, loc_fp = 0;
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            const i64 i = end - 1 - (lane * kItems + u);
            at[u] = i >= 0 ? slot_of(i) : -1;
            f[u] = bits_of(at[u]);
            loc_n += f[u] & 1;
            loc_tp += (f[u] >> 1) & 1;
            loc_fp += (f[u] >> 2) & 1;
        }
        const int inc_n = wave_scan_add(loc_n, lane), inc_tp = wave_scan_add(loc_tp, lane);
        const int inc_fp = wave_scan_add(loc_fp, lane);
        int rn = right_n + inc_n - loc_n, rtp = right_tp + inc_tp - loc_tp, rfp = right_fp + inc_fp - loc_fp;
        double pr[kItems], loc_max = 0.;
        int tp_at[kItems], n_at[kItems];
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            const int tp = all_tp - rtp, fp = all_fp - rfp;             // cumulative counts at this row
            tp_at[u] = tp;
            n_at[u] = all_n - rn;
            rn += f[u] & 1;
            rtp += (f[u] >> 1) & 1;
            rfp += (f[u] >> 2) & 1;
            pr[u] = (f[u] & 1) ? (double)tp / (((double)fp + (double)tp) + DBL_EPSILON) : 0.;
            loc_max = fmax(loc_max, pr[u]);
        }
        const double inc_max = wave_scan_max(loc_max, lane);
        double run = __shfl_up(inc_max, 1);             // maximum over the rows right of this lane's
        run = lane == 0 ? right_max : fmax(right_max, run);
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            run = fmax(run, pr[u]);                     // the envelope at this row
            const int is_tp = (f[u] >> 1) & 1;
            if ((f[u] & 1) && (is_tp || n_at[u] == 1)) {
                // searchsorted(rc, rec_thrs, 'left') lands here for the thresholds in (previous recall, this recall]
                const int r0 = n_at[u] == 1 ? 0 : count_le(s_thr, R, (double)(tp_at[u] - is_tp) / dnp);
                const int r1 = count_le(s_thr, R, (double)tp_at[u] / dnp);
                const double sc = (double)key_score(rec_key[at[u]]);
                for (int r = r0; r < r1; ++r) {
                    s_q[t][r] = run;
                    s_ss[t][r] = sc;
                }
            }
        }
        right_n += __shfl(inc_n, kWave - 1);
        right_tp += __shfl(inc_tp, kWave - 1);
        right_fp += __shfl(inc_fp, kWave - 1);
        right_max = fmax(right_max, __shfl(inc_max, kWave - 1));
    }
    __syncthreads();
    for (int r = lane; r < R; r += kWave) {
        precision[pr_at(r)] = s_q[t][r];
        scores[pr_at(r)] = s_ss[t][r];
    }
    if (lane == 0) recall[rc_at] = all_n ? (double)all_tp / dnp : 0.;
}

}  // namespace

extern "C" int ct_coco_match(const float* out_dets, const int* out_count, int batch, int num_fg, int cap,
                             const int* image_index, const int* image_rank, int num_images, const double* gt_boxes,
                             const double* gt_area, const uint8_t* gt_iscrowd, const int* gt_label, const int* gt_off,
                             int num_gt, const int* cat_rank, const double* iou_thrs, int num_iou_thrs,
                             const double* area_rng, int num_area_rng, long long* rec_key,
                             unsigned long long* rec_matched, unsigned long long* rec_ignored, int per_image_cap,
                             int* status, ct_stream_t stream)
{
    CT_REQUIRE(batch > 0 && num_fg > 0 && cap > 0 && num_images > 0 && num_gt >= 0 && per_image_cap > 0,
               "ct_coco_match: bad sizes (batch %d, num_fg %d, cap %d, num_images %d, num_gt %d, per_image_cap %d)",
               batch, num_fg, cap, num_images, num_gt, per_image_cap);
    CT_REQUIRE(out_dets && out_count && image_index && gt_boxes && gt_area && gt_iscrowd && gt_label && gt_off &&
                   cat_rank && iou_thrs && area_rng && rec_key && rec_matched && rec_ignored && status,
               "ct_coco_match: null pointer");
    CT_REQUIRE(num_fg <= kMaxClasses && cap <= kMaxCap && num_images <= kMaxImages,
               "ct_coco_match: num_fg %d (<= %d), cap %d (<= %d), num_images %d (<= %d): the 64-bit key has 7 + 17 bits "
               "for category and image", num_fg, kMaxClasses, cap, kMaxCap, num_images, kMaxImages);
    CT_REQUIRE(num_iou_thrs > 0 && num_iou_thrs <= kMaxThr && num_area_rng > 0 && num_area_rng <= kMaxArea &&
                   num_iou_thrs * num_area_rng <= 64,
               "ct_coco_match: %d IoU thresholds (<= %d) x %d area ranges (<= %d): one mask bit per pair, at most 64",
               num_iou_thrs, kMaxThr, num_area_rng, kMaxArea);
    const int slices = num_fg < kMaxSlices ? num_fg : kMaxSlices;
    hipLaunchKernelGGL(coco_match_kernel, dim3(batch, slices), dim3(kWave), 0, ctdet::as_stream(stream), out_dets,
                       out_count, num_fg, cap, image_index, image_rank, num_images, gt_boxes, gt_area, gt_iscrowd,
                       gt_label, gt_off, num_gt, cat_rank, iou_thrs, num_iou_thrs, area_rng, num_area_rng, rec_key,
                       (u64*)rec_matched, (u64*)rec_ignored, per_image_cap, status);
    CT_LAUNCH_CHECK("coco_match_kernel");
    return CT_OK;
}

extern "C" int ct_coco_accumulate(const long long* rec_key, const unsigned long long* rec_matched,
                                  const unsigned long long* rec_ignored, const long long* order, long long num_records,
                                  const long long* cat_off, const int* npig, int num_categories, int num_area_rng,
                                  const int* max_dets, int num_max_dets, int num_iou_thrs, const double* rec_thrs,
                                  int num_rec_thrs, double* precision, double* recall, double* scores, int* status,
                                  ct_stream_t stream)
{
    CT_REQUIRE(num_records >= 0 && num_categories > 0 && num_categories <= kMaxClasses && num_area_rng > 0 &&
                   num_area_rng <= kMaxArea && num_max_dets > 0 && num_max_dets <= 4 && num_iou_thrs > 0 &&
                   num_iou_thrs <= kMaxThr && num_iou_thrs * num_area_rng <= 64 && num_rec_thrs > 0 &&
                   num_rec_thrs <= kMaxRec,
               "ct_coco_accumulate: bad sizes (num_records %lld, categories %d, area ranges %d, limits %d, IoU "
               "thresholds %d, recall thresholds %d)", num_records, num_categories, num_area_rng, num_max_dets,
               num_iou_thrs, num_rec_thrs);
    CT_REQUIRE(rec_key && rec_matched && rec_ignored && cat_off && npig && max_dets && rec_thrs && precision &&
                   recall && scores && status, "ct_coco_accumulate: null pointer");
    hipLaunchKernelGGL(coco_acc_kernel, dim3(num_categories * num_area_rng * num_max_dets),
                       dim3(num_iou_thrs * kWave), 0, ctdet::as_stream(stream), rec_key, (const u64*)rec_matched,
                       (const u64*)rec_ignored, order, num_records, cat_off, npig, num_categories, num_area_rng,
                       num_max_dets, max_dets, rec_thrs, num_rec_thrs, precision, recall, scores, status);
    CT_LAUNCH_CHECK("coco_acc_kernel");
    return CT_OK;
}
