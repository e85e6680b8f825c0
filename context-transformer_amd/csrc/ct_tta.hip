// libctdet: horizontal-flip test-time augmentation and box voting for the detection pipeline.
//
//   hflip_kernel       out[plane][y][j] = in[plane][y][w-1-j] (the second pass's input).
//   tta_merge_kernel   pass k's [B,P,4] boxes / [B,P,C] scores -> rows [k*P, (k+1)*P) of the merged [B,K*P,...] buffers;
//                      a mirrored pass's boxes go back to the image's frame in pixels: x1' = W_b - x2, x2' = W_b - x1 (fp32).
//   box_vote_kernel    Detectron's box_voting with scoring method ID, on the rows of out_dets after the top-k cut: the box of
//                      output row r of (image b, class c) becomes the score-weighted mean of every row q of the image with
//                      scores[b,q,c] > conf_thresh and IoU(row, box_q) >= vote_thresh; scores, counts and order stay.
//
// box_vote_kernel, one workgroup per (image, class):
//   * candidates are re-selected from the raw score column in merged-index order (a ballot per wave, one barrier per 1024
//     rows for the workgroup-wide offsets: no atomics, so a candidate's LDS slot does not depend on timing) and staged in LDS
//     (box + weight, 20 bytes) in chunks of `chunk` rows; a segment with more candidates is voted chunk after chunk;
//   * one wave per output row, lanes over the chunk's candidates: the IoU is ct_nms.hip's +1 expression with the IEEE
//     quotient; members add w, w*x1, w*y1, w*x2, w*y2 to five float64 accumulators (a product of two floats is exact in
//     float64); the lanes are summed by a butterfly, chunks in their order through the workspace (out_cap * 5 doubles per
//     segment, touched only by segments longer than one chunk);
//   * after the last chunk: one float64 division per coordinate, rounded once to fp32, written over the row's box.
// A row is read (its box is the voting target) and written by the same wave, in program order, so voting in place is safe;
// members come from `boxes`, never from out_dets.  Same input, same bits: no atomics, every order is fixed.
//
// Compiled with -ffp-contract=off.
#include "ct_common.h"
#include <algorithm>

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBatch = 4;                            // strided score loads in flight per thread in the select loop
constexpr int kIterRows = kThreads * kBatch;         // rows one select trip looks at: a chunk holds at least that many
constexpr int kChunkRowsMax = 2048;                  // 40 KB of LDS: four segments resident per CU
constexpr int kChunkBytesPerRow = 20;
constexpr int kLdsExtra = 2 * kBatch * kWaves * 4;   // the double-buffered ballot counts

__global__ __launch_bounds__(256) void hflip_kernel(const float* __restrict__ in, float* __restrict__ out, long rows, int w)
{
    const long total = rows * w;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / w;
        const int j = (int)(i - r * w);
        out[i] = in[r * w + (w - 1 - j)];
    }
}

// w % 4 == 0 and both pointers 16-byte aligned: a thread writes four neighbouring columns
__global__ __launch_bounds__(256) void hflip4_kernel(const float4* __restrict__ in, float4* __restrict__ out, long rows, int w4)
{
    const long total = rows * w4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / w4;
        const int j = (int)(i - r * w4);
        const float4 v = in[r * w4 + (w4 - 1 - j)];
        out[i] = make_float4(v.w, v.z, v.y, v.x);
    }
}

// grid (blocks, batch).  VEC: P * C is a multiple of 4 and the score pointers are 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void tta_merge_kernel(const float4* __restrict__ boxes_k, const float* __restrict__ scores_k,
                                                        int P, int C, int K, int k, int mirror, const float* __restrict__ scale,
                                                        int scale_per_image, float4* __restrict__ boxes_m,
                                                        float* __restrict__ scores_m)
{
    const int b = blockIdx.y;
    const long step = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const float4* bs = boxes_k + (size_t)b * P;
    float4* bd = boxes_m + ((size_t)b * K + k) * P;
    const float W = mirror ? scale[scale_per_image ? b * 4 : 0] : 0.f;
    for (long p = t0; p < P; p += step) {
        float4 q = bs[p];
        if (mirror) q = make_float4(W - q.z, q.y, W - q.x, q.w);
        bd[p] = q;
    }
    const long n = (long)P * C;
    const float* ss = scores_k + (size_t)b * n;
    float* sd = scores_m + ((size_t)b * K + k) * n;
    if (VEC) {
        const float4* s4 = reinterpret_cast<const float4*>(ss);
        float4* d4 = reinterpret_cast<float4*>(sd);
        for (long i = t0; i < n / 4; i += step) d4[i] = s4[i];
    } else {
        for (long i = t0; i < n; i += step) sd[i] = ss[i];
    }
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);      // the same tree in every lane, every run
    return v;
}

// Rows [0, m) of one segment against the `count` candidates staged in LDS.  first: no earlier chunk (nothing to read from
// acc); last: divide and write the boxes, else leave the running sums in acc.
__device__ __forceinline__ void vote_chunk(const float4* s_box, const float* s_w, int count, float vote_thresh, float* od,
                                           int m, double* acc, bool first, bool last)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < m; r += kWaves) {
        float* row = od + (size_t)r * 5;
        const float tx1 = row[0], ty1 = row[1], tx2 = row[2], ty2 = row[3];
        const float tarea = (tx2 - tx1 + 1.0f) * (ty2 - ty1 + 1.0f);
        double sw = 0.0, sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
        for (int j = lane; j < count; j += 64) {
            const float4 q = s_box[j];
            const float xx1 = tx1 >= q.x ? tx1 : q.x, yy1 = ty1 >= q.y ? ty1 : q.y;
            const float xx2 = tx2 <= q.z ? tx2 : q.z, yy2 = ty2 <= q.w ? ty2 : q.w;
            const float w0 = xx2 - xx1 + 1.0f, h0 = yy2 - yy1 + 1.0f;
            const float w = 0.0f >= w0 ? 0.0f : w0, h = 0.0f >= h0 ? 0.0f : h0;
            const float inter = w * h;
            // (inter == 0: the quotient is 0, -0 or NaN, never >= vote_thresh > 0 -- the same decision without the division;
            // neighbouring merged indices are neighbouring priors, so whole waves skip it)
            if (!(inter > 0.0f)) continue;
            const float area = (q.z - q.x + 1.0f) * (q.w - q.y + 1.0f);
            const float ovr = inter / (tarea + area - inter);
            if (ovr >= vote_thresh) {
                const double wq = (double)s_w[j];
                sw += wq;
                sx1 += wq * (double)q.x;
                sy1 += wq * (double)q.y;
                sx2 += wq * (double)q.z;
                sy2 += wq * (double)q.w;
            }
        }
        sw = wave_sum(sw);
        sx1 = wave_sum(sx1);
        sy1 = wave_sum(sy1);
        sx2 = wave_sum(sx2);
        sy2 = wave_sum(sy2);
        if (lane == 0) {
            double* a = acc + (size_t)r * 5;
            if (!first) {
                sw = a[0] + sw;
                sx1 = a[1] + sx1;
                sy1 = a[2] + sy1;
                sx2 = a[3] + sx2;
                sy2 = a[4] + sy2;
            }
            if (!last) {
                a[0] = sw; a[1] = sx1; a[2] = sy1; a[3] = sx2; a[4] = sy2;
            } else if (sw > 0.0) {                                      // (no member: the row keeps its bits)
                row[0] = (float)(sx1 / sw);
                row[1] = (float)(sy1 / sw);
                row[2] = (float)(sx2 / sw);
                row[3] = (float)(sy2 / sw);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void box_vote_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                            int batch, int N, int T, float thresh, float vote_thresh,
                                                            int out_cap, int chunk, float* out_dets,
                                                            const int* __restrict__ out_count, double* acc_ws)
{
    extern __shared__ __attribute__((aligned(16))) float4 s_dyn[];     // chunk boxes, chunk weights, 2 x 16 ballot counts
    float4* const s_box = s_dyn;
    float* const s_w = reinterpret_cast<float*>(s_dyn + chunk);
    int* const s_cnt = reinterpret_cast<int*>(s_w + chunk);
    // blockIdx -> (image, class) as in select_sort_kernel (ct_post.hip): the T workgroups of an image read the same lines of
    // its score array (a class column is a strided read) and share them through one XCD's L2
    const int b = ((int)(blockIdx.x >> 3) / T) * 8 + (int)(blockIdx.x & 7);
    const int cls = 1 + (int)(blockIdx.x >> 3) % T;
    if (b >= batch) return;
    const int seg = b * T + (cls - 1);
    const int m = min(out_count[seg], out_cap);
    if (m <= 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* od = out_dets + (size_t)seg * out_cap * 5;
    double* acc = acc_ws + (size_t)seg * out_cap * 5;                  // (not dereferenced by a one-chunk segment)
    const float* sc = scores + (size_t)b * N * (T + 1) + cls;
    const float4* bx = reinterpret_cast<const float4*>(boxes) + (size_t)b * N;

    int base = 0, chunk_start = 0, it = 0;                             // candidates seen; first candidate of the open chunk
    // scores and boxes of a trip's rows are loaded one trip ahead (the boxes of rows that will not pass too: coalesced 16-byte
    // loads of lines the image's other classes read anyway), so that no trip waits for its strided column read
    float v[kBatch], vn[kBatch];
    float4 q[kBatch], qn[kBatch];
    auto load_rows = [&](int p0, float* vv, float4* qq) {
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int p = p0 + u * kThreads + tid;
            vv[u] = p < N ? sc[(size_t)p * (T + 1)] : -INFINITY;
            qq[u] = p < N ? bx[p] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    load_rows(0, v, q);
    for (int p0 = 0; p0 < N; p0 += kIterRows, ++it) {
        if (p0 + kIterRows < N) load_rows(p0 + kIterRows, vn, qn);
        u64 mk[kBatch];
        int* cnt = s_cnt + (it & 1) * (kBatch * kWaves);
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            mk[u] = __ballot(v[u] > thresh);                           // padding lanes: -inf never passes
            if (lane == 0) cnt[u * kWaves + wave] = __popcll(mk[u]);
        }
        __syncthreads();
        // (the counts are double-buffered: the next trip writes the other half, the one after that only behind the next
        // barrier, which every thread reaches after these reads)
        int tot = 0, pre[kBatch] = {};
#pragma unroll
        for (int k = 0; k < kBatch * kWaves; ++k) {
#pragma unroll
            for (int u = 0; u < kBatch; ++u)
                if (k == u * kWaves + wave) pre[u] = tot;
            tot += cnt[k];
        }
        int g[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const bool pass = v[u] > thresh;
            g[u] = pass ? base + pre[u] + __popcll(mk[u] & ((1ull << lane) - 1ull)) : -1;
            const int slot = g[u] - chunk_start;
            if (pass && slot < chunk) {
                s_box[slot] = q[u];
                s_w[slot] = v[u];
            }
        }
        if (base + tot > chunk_start + chunk) {                        // uniform: the open chunk is full and rows are left over
            __syncthreads();
            vote_chunk(s_box, s_w, chunk, vote_thresh, od, m, acc, chunk_start == 0, false);
            __syncthreads();
            chunk_start += chunk;
            // tot <= kIterRows <= chunk: what is left over fits into the new chunk
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int slot = g[u] - chunk_start;
                if (g[u] >= 0 && slot >= 0) {
                    s_box[slot] = q[u];
                    s_w[slot] = v[u];
                }
            }
        }
        base += tot;
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            v[u] = vn[u];
            q[u] = qn[u];
        }
    }
    __syncthreads();
    vote_chunk(s_box, s_w, base - chunk_start, vote_thresh, od, m, acc, chunk_start == 0, true);
}

// rows of one chunk: what the device's LDS per workgroup holds, at most kChunkRowsMax
int chunk_rows()
{
    static const int rows = [] {
        int dev = 0, bytes = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess)
            return kChunkRowsMax;                 // no device to ask (the CPU-side symbol checks)
        const int fit = (std::min(bytes, 64 * 1024) - kLdsExtra) / kChunkBytesPerRow / 64 * 64;
        return std::min(fit, kChunkRowsMax);
    }();
    return rows;
}

}  // namespace

extern "C" int ct_hflip_f32(const float* in, float* out, long planes, int h, int w, ct_stream_t stream)
{
    CT_REQUIRE(in && out && in != out, "ct_hflip_f32: null pointer or in == out (the mirror is out of place)");
    CT_REQUIRE(planes > 0 && h > 0 && w > 0, "ct_hflip_f32: bad shape (planes=%ld h=%d w=%d)", planes, h, w);
    const long rows = planes * h;
    hipStream_t st = ctdet::as_stream(stream);
    const bool vec = w % 4 == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const long items = vec ? rows * (w / 4) : rows * w;
    const dim3 grid((unsigned)std::min<long>((items + 255) / 256, 65536)), block(256);
    CT_PROF("hflip_kernel", st);
    if (vec)
        hipLaunchKernelGGL(hflip4_kernel, grid, block, 0, st, (const float4*)in, (float4*)out, rows, w / 4);
    else
        hipLaunchKernelGGL(hflip_kernel, grid, block, 0, st, in, out, rows, w);
    CT_LAUNCH_CHECK("hflip_kernel");
    return CT_OK;
}

extern "C" int ct_tta_merge(const float* boxes_k, const float* scores_k, int batch, int num_priors, int num_cls_cols,
                            int num_passes, int k, int mirror, const float* scale4, int scale_per_image,
                            float* boxes_merged, float* scores_merged, ct_stream_t stream)
{
    CT_REQUIRE(boxes_k && scores_k && boxes_merged && scores_merged, "ct_tta_merge: null pointer");
    CT_REQUIRE(batch > 0 && batch <= 65535 && num_priors > 0 && num_cls_cols > 0, "ct_tta_merge: bad shape");
    CT_REQUIRE(num_passes > 0 && k >= 0 && k < num_passes, "ct_tta_merge: pass %d of %d", k, num_passes);
    CT_REQUIRE(!mirror || scale4, "ct_tta_merge: a mirrored pass needs the image widths (scale4)");
    CT_REQUIRE(((reinterpret_cast<uintptr_t>(boxes_k) | reinterpret_cast<uintptr_t>(boxes_merged)) & 15) == 0,
               "ct_tta_merge: boxes must be 16-byte aligned");
    CT_REQUIRE((long)num_passes * num_priors < 0x7FFFFFFFL, "ct_tta_merge: too many merged rows");
    hipStream_t st = ctdet::as_stream(stream);
    const long n = (long)num_priors * num_cls_cols;
    const bool vec = n % 4 == 0 && ((reinterpret_cast<uintptr_t>(scores_k) | reinterpret_cast<uintptr_t>(scores_merged)) & 15) == 0;
    const long items = vec ? n / 4 : n;
    const dim3 grid((unsigned)std::min<long>((std::max<long>(items, num_priors) + 255) / 256, 1024), batch), block(256);
    CT_PROF("tta_merge_kernel", st);
    if (vec)
        hipLaunchKernelGGL(tta_merge_kernel<true>, grid, block, 0, st, (const float4*)boxes_k, scores_k, num_priors, num_cls_cols,
                           num_passes, k, mirror, scale4, scale_per_image, (float4*)boxes_merged, scores_merged);
    else
        hipLaunchKernelGGL(tta_merge_kernel<false>, grid, block, 0, st, (const float4*)boxes_k, scores_k, num_priors, num_cls_cols,
                           num_passes, k, mirror, scale4, scale_per_image, (float4*)boxes_merged, scores_merged);
    CT_LAUNCH_CHECK("tta_merge_kernel");
    return CT_OK;
}

extern "C" int ct_box_vote_lds_rows(void) { return chunk_rows(); }

extern "C" size_t ct_box_vote_workspace_bytes(int batch, int num_rows, int num_fg, int out_cap)
{
    // the running sums of the segments that may hold more candidates than one chunk; 256 bytes otherwise
    if (batch <= 0 || num_rows <= chunk_rows() || num_fg <= 0 || out_cap <= 0) return 256;
    return ctdet::align_up((size_t)batch * num_fg * out_cap * 5 * sizeof(double), 256);
}

extern "C" int ct_box_vote_batched(const float* boxes, const float* scores, int batch, int num_rows, int num_fg,
                                   float conf_thresh, float vote_thresh, int out_cap, float* out_dets, const int* out_count,
                                   void* workspace, size_t workspace_bytes, ct_stream_t stream)
{
    CT_REQUIRE(boxes && scores && out_dets && out_count, "ct_box_vote_batched: null pointer");
    CT_REQUIRE(batch > 0 && num_rows > 0 && num_fg > 0 && out_cap > 0, "ct_box_vote_batched: bad sizes");
    CT_REQUIRE(conf_thresh >= 0.f, "ct_box_vote_batched: conf_thresh must be >= 0 (the weights are the scores above it)");
    CT_REQUIRE(vote_thresh > 0.f && vote_thresh <= 1.f, "ct_box_vote_batched: vote_thresh %g is outside (0, 1]", (double)vote_thresh);
    CT_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 15) == 0, "ct_box_vote_batched: boxes must be 16-byte aligned");
    const int chunk = chunk_rows();
    if (chunk < kIterRows)
        return ctdet::fail(CT_ERR_INVALID, "ct_box_vote_batched: the device's LDS holds %d candidates, %d are needed", chunk, kIterRows);
    const size_t need = ct_box_vote_workspace_bytes(batch, num_rows, num_fg, out_cap);
    if (num_rows > chunk) {
        if (!workspace) return ctdet::fail(CT_ERR_WORKSPACE, "ct_box_vote_batched: workspace is NULL");
        if (workspace_bytes < need)
            return ctdet::fail(CT_ERR_WORKSPACE, "ct_box_vote_batched: workspace %zu < %zu", workspace_bytes, need);
        CT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "ct_box_vote_batched: workspace must be 8-byte aligned");
    }
    hipStream_t st = ctdet::as_stream(stream);
    const size_t lds = (size_t)chunk * kChunkBytesPerRow + kLdsExtra;
    const dim3 grid(8 * ((batch + 7) / 8) * num_fg), block(kThreads);
    CT_PROF("box_vote_kernel", st);
    hipLaunchKernelGGL(box_vote_kernel, grid, block, lds, st, boxes, scores, batch, num_rows, num_fg, conf_thresh, vote_thresh,
                       out_cap, chunk, out_dets, out_count, (double*)workspace);
    CT_LAUNCH_CHECK("box_vote_kernel");
    return CT_OK;
}
