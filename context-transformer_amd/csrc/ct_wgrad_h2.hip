// libctdet: weight gradient of the 1x1 convolutions on the f16 matrix pipe, f16x2 operand form (ct_f16x2.h).
//
//   dW[co][ci] = sum_p dZ[co][p] X[ci][p],  p over batch x output pixels:  ONE GEMM, M = cout, N = cin, K = batch * OH * OW,
//   on v_mfma_f32_32x32x16_f16 with the three piece products hi.hi + hi.lo + lo.hi and fp32 accumulation (hi.hi in an
//   accumulator of its own, the two small products in a second one).
//
// Both operands are contiguous along K inside an (image, channel) plane, and a lane's A / B fragment of the 32x32x16 MFMA is 8
// consecutive k of one row: 8 consecutive pixels of one channel through split2 four times ARE a lane's hi and lo fragment, so
// nothing is transposed.  K is cut into GROUPS of 8 pixels that never straddle a plane (ceil(OH OW / 8) groups per image, the
// last one of an image zero-filled).  A workgroup (256 threads, 128 couts x 128 cins, 2 x 2 waves of 64 x 64) takes 8 groups
// (64 k) per stage: thread t loads group t & 7 of rows (t >> 3) + 32 j (j < 4: dZ rows, j >= 4: X rows) -- 8 neighbouring lanes
// read 256 contiguous bytes of one row --, scales by the launch's power of two, splits ONCE per workgroup and writes the
// pieces to LDS in fragment order (1 KB per [k16 step][row block][piece]; the 16-byte slot of a row is XORed with the group
// index so that the 8 lanes of a row write 8 different bank quads); the waves read their fragments back with one 16-byte read
// each.  Stride 2 (the RFB shortcut, BasicRFB(stride=2)) gathers X at (2 oh, 2 ow) with one load per pixel; dZ stays contiguous.
//
// Scaling: the sum runs over the whole batch, so each operand gets ONE exponent per launch, exponent_for(max over the batch's
// lines, kGrowthNone); a missing maximum is taken by a pass of this entry point (ct_absmax_f32) into lines of the workspace,
// which it clears first.  Deterministic: K is split over workgroups in a partition fixed by the descriptor, every split writes
// its own [cout][cin] slab of the workspace, and wgrad_h2_finish adds the slabs in order, multiplies by 2^-(eZ + eX) as two exact
// factors and stores: no atomics, dw is overwritten, two calls give the same bits.
// Buffers above 2 GiB (32-bit buffer offsets) are REFUSED with a message; ct_conv2d_wgrad takes them in batch chunks.
#include "ct_common.h"
#include "ct_device.h"
#include "ct_f16x2.h"
#include "ct_wgrad_launch.h"

namespace {

using ctdet::f16x8;
using ctdet::f32x16;
using ctdet::i32x4;
using ctdet::kInvalidOff;
using ctdet::kMaxBufBytes;
using ctdet::make_rsrc;
using ctdet::h2::exponent_for;
using ctdet::h2::kGrowthNone;
using ctdet::h2::kLineWords;

struct __attribute__((packed, aligned(4))) Pix8 { float v[8]; };      // 8 pixels of a plane: two 16-byte loads
constexpr int BT = 128;                     // workgroup tile: BT couts x BT cins
constexpr int GROUP = 8;                    // pixels per k group (one lane's fragment)
constexpr int STAGE_GROUPS = 8;             // groups per stage: 64 k = 4 MFMA k steps
constexpr int FRAG_BYTES = 1024;            // 64 lanes x 8 binary16
constexpr int LDS_BYTES = 4 * 8 * 2 * FRAG_BYTES;      // [k16 step 4][row block 8][piece 2]
constexpr size_t kSlabBudget = (size_t)32 << 20;       // the split count keeps the slabs of one launch below this

struct WgradH2Args {
    const float* x;
    const float* dz;
    float* slabs;
    const unsigned* x_lines;
    const unsigned* z_lines;
    unsigned x_bytes, dz_bytes;
    int batch, Cin, Cout;
    int HW, W, x_ctot, x_coff;              // input plane
    int OHW, OW, dz_ctot, dz_coff;          // dZ plane
    int stride;
    int G;                                  // groups per image
    int groups;                             // batch * G
    int tiles_m, stages_per_split;
};

// maximum over the batch's lines, by every lane of the calling wave
__device__ __forceinline__ unsigned batch_max(const unsigned* __restrict__ lines, int batch)
{
    unsigned m = 0;
    for (int n = threadIdx.x & 63; n < batch; n += 64) {
        const unsigned v = lines[(size_t)n * kLineWords];
        m = v > m ? v : m;
    }
    return ctdet::h2::wave_max(m);
}

template <bool STRIDED>
__global__ __launch_bounds__(256) void wgrad_h2_gemm(const WgradH2Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char wh_lds[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hsel = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave & 1, wc = wave >> 1;
    const int tile = blockIdx.x;
    const int m0 = (tile % a.tiles_m) * BT, c0 = (tile / a.tiles_m) * BT;
    const int g_begin = blockIdx.y * a.stages_per_split * STAGE_GROUPS;
    const int g_end = min(g_begin + a.stages_per_split * STAGE_GROUPS, a.groups);

    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rz = make_rsrc(a.dz, a.dz_bytes);
    const float sz = __builtin_ldexpf(1.f, exponent_for(batch_max(a.z_lines, a.batch), kGrowthNone));
    const float sx = __builtin_ldexpf(1.f, exponent_for(batch_max(a.x_lines, a.batch), kGrowthNone));

    // loader role: group kg of the stage, rows r31 + 32 j
    const int kg = tid & 7, r31 = tid >> 3;
    int row_off[8];                         // byte offset of the row's plane inside an image; rows past the matrix: invalid
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + 32 * j + r31, c = c0 + 32 * j + r31;
        row_off[j] = m < a.Cout ? (a.dz_coff + m) * a.OHW * 4 : -1;
        row_off[4 + j] = c < a.Cin ? (a.x_coff + c) * a.HW * 4 : -1;
    }
    // LDS slot of this thread's pieces inside a fragment: k half (kg & 1), row r31 ^ kg
    const int wslot = ((kg >> 1) * 16 * FRAG_BYTES) + ((((kg & 1) << 5) | (r31 ^ kg)) << 4);

    float v[8][GROUP];
    auto load_stage = [&](int g0) {
        const int g = g0 + kg;
        const bool gv = g < g_end;
        const int gc = gv ? g : 0;
        const int n = gc / a.G;
        const int p0 = (gc - n * a.G) * GROUP;
        const int cnt = gv ? min(GROUP, a.OHW - p0) : 0;
        const int zimg = n * a.dz_ctot * a.OHW * 4 + p0 * 4;
        const int ximg = n * a.x_ctot * a.HW * 4;
        // dZ rows (and X rows of a stride-1 layer): contiguous pixels; a full group as two 16-byte loads, a group cut by
        // the end of its plane (or a row past the matrix) as bounds-checked single loads that return zeros
#pragma unroll
        for (int j = 0; j < (STRIDED ? 4 : 8); ++j) {
            const int base = (j < 4 ? zimg : ximg + p0 * 4) + row_off[j];
            const __amdgpu_buffer_rsrc_t r = j < 4 ? rz : rx;
            if (row_off[j] >= 0 && cnt == GROUP) {
                // inside the buffer by construction; plane bases are only 4-byte aligned when OH OW is odd
                const Pix8 q = *reinterpret_cast<const Pix8*>(reinterpret_cast<const char*>(j < 4 ? a.dz : a.x) + base);
#pragma unroll
                for (int i = 0; i < GROUP; ++i) v[j][i] = q.v[i];
            } else {
#pragma unroll
                for (int i = 0; i < GROUP; ++i) {
                    const int off = (row_off[j] >= 0 && i < cnt) ? base + 4 * i : kInvalidOff;
                    v[j][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
                }
            }
        }
        if (STRIDED) {
            int oh = p0 / a.OW, ow = p0 - oh * a.OW;
            int poff[GROUP];
#pragma unroll
            for (int i = 0; i < GROUP; ++i) {
                poff[i] = i < cnt ? ximg + (oh * a.stride * a.W + ow * a.stride) * 4 : -1;
                if (++ow == a.OW) { ow = 0; ++oh; }
            }
#pragma unroll
            for (int j = 4; j < 8; ++j)
#pragma unroll
                for (int i = 0; i < GROUP; ++i) {
                    const int off = (row_off[j] >= 0 && poff[i] >= 0) ? poff[i] + row_off[j] : kInvalidOff;
                    v[j][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, off, 0, 0));
                }
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float s = j < 4 ? sz : sx;
            i32x4 hi, lo;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int h, l;
                ctdet::h2::split2(v[j][2 * i] * s, v[j][2 * i + 1] * s, h, l);
                hi[i] = h;
                lo[i] = l;
            }
            unsigned char* dst = wh_lds + wslot + j * 2 * FRAG_BYTES;
            *reinterpret_cast<i32x4*>(dst) = hi;
            *reinterpret_cast<i32x4*>(dst + FRAG_BYTES) = lo;
        }
    };

    f32x16 acc[2][2], acs[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; acs[i][j][r] = 0.f; }

    if (g_begin < g_end) load_stage(g_begin);
    for (int g0 = g_begin; g0 < g_end; g0 += STAGE_GROUPS) {
        store_stage();
        __syncthreads();
        if (g0 + STAGE_GROUPS < g_end) load_stage(g0 + STAGE_GROUPS);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            // fragment (ks, k half hsel) keeps row r at slot r ^ (2 ks + hsel)
            const unsigned char* fb = wh_lds + ks * 16 * FRAG_BYTES + (((hsel << 5) | (l31 ^ (2 * ks + hsel))) << 4);
            f16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = *reinterpret_cast<const f16x8*>(fb + (wr * 2 + i) * 2 * FRAG_BYTES);
                al[i] = *reinterpret_cast<const f16x8*>(fb + (wr * 2 + i) * 2 * FRAG_BYTES + FRAG_BYTES);
                bh[i] = *reinterpret_cast<const f16x8*>(fb + (4 + wc * 2 + i) * 2 * FRAG_BYTES);
                bl[i] = *reinterpret_cast<const f16x8*>(fb + (4 + wc * 2 + i) * 2 * FRAG_BYTES + FRAG_BYTES);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                    acs[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acs[i][j], 0, 0, 0);
                    acs[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acs[i][j], 0, 0, 0);
                }
        }
        __syncthreads();
    }

    // this split's slab [cout][cin]: lanes along cin
    float* slab = a.slabs + (size_t)blockIdx.y * a.Cout * a.Cin;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = c0 + wc * 64 + 32 * j + l31;
        if (c >= a.Cin) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wr * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hsel;
                if (m < a.Cout) slab[(size_t)m * a.Cin + c] = acc[i][j][r] + acs[i][j][r];
            }
    }
}

// dw = (slab 0 + slab 1 + ... in order) 2^-(eZ + eX)
__global__ __launch_bounds__(256) void wgrad_h2_finish(const float* __restrict__ slabs, int splits, int n,
                                                       const unsigned* __restrict__ z_lines,
                                                       const unsigned* __restrict__ x_lines, int batch,
                                                       float* __restrict__ dw)
{
    const int ez = exponent_for(batch_max(z_lines, batch), kGrowthNone);
    const int ex = exponent_for(batch_max(x_lines, batch), kGrowthNone);
    const ctdet::h2::pow2x2 u = ctdet::h2::unscale_for(ez, ex);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = slabs[i];
    for (int k = 1; k < splits; ++k) s += slabs[(size_t)k * n + i];
    dw[i] = (s * u.lo) * u.hi;
}

bool geometry_ok(const ct_conv_desc* d)
{
    return d && d->kh == 1 && d->kw == 1 && d->pad_h == 0 && d->pad_w == 0 && d->dil == 1 &&
           (d->stride == 1 || d->stride == 2) && d->batch > 0 && d->cin > 0 && d->cout > 0 && d->h > 0 && d->w > 0 &&
           d->oh == (d->h - 1) / d->stride + 1 && d->ow == (d->w - 1) / d->stride + 1;
}

struct Layout {
    size_t lines_bytes;         // one operand's maxima lines
    size_t dw_bytes;
    int G, groups, stages, tiles_m, tiles_n, stages_per_split, splits;
};

// everything here follows from the descriptor alone: the K partition is part of the result's bits
Layout layout_of(const ct_conv_desc* d)
{
    Layout l{};
    l.lines_bytes = ctdet::align_up((size_t)d->batch * CT_ABSMAX_LINE_BYTES, 256);
    l.dw_bytes = (size_t)d->cout * d->cin * 4;
    l.G = (d->oh * d->ow + GROUP - 1) / GROUP;
    l.groups = d->batch * l.G;
    l.stages = (l.groups + STAGE_GROUPS - 1) / STAGE_GROUPS;
    l.tiles_m = (d->cout + BT - 1) / BT;
    l.tiles_n = (d->cin + BT - 1) / BT;
    // two workgroups per compute unit of a 256-unit chip, at least two stages per split, slabs within the budget
    const long tiles = (long)l.tiles_m * l.tiles_n;
    long want = std::max<long>(1, (512 + tiles - 1) / tiles);
    want = std::min<long>(want, std::max(1, l.stages / 2));
    want = std::min<long>(want, std::max<size_t>(1, kSlabBudget / l.dw_bytes));
    const ctdet::Split sp = ctdet::even_split(l.stages, (int)want);
    l.stages_per_split = sp.per_split;
    l.splits = sp.splits;
    return l;
}

// an upper bound of splits * dw_bytes that grows with cout * cin on a fixed map
size_t slab_bytes(const Layout& l)
{
    const size_t by_k = (size_t)std::max(1, l.stages / 2) * l.dw_bytes;
    return ctdet::align_up(std::max(l.dw_bytes, std::min(kSlabBudget, by_k)), 256);
}

}  // namespace

extern "C" int ct_conv_wgrad_h2_supported(const ct_conv_desc* d)
{
    return geometry_ok(d) && (long long)d->batch * d->in_ctot * d->h * d->w * 4 < kMaxBufBytes &&
           (long long)d->batch * d->cout * d->oh * d->ow * 4 < kMaxBufBytes;
}

extern "C" size_t ct_conv_wgrad_h2_workspace_bytes(const ct_conv_desc* d)
{
    if (!ct_conv_wgrad_h2_supported(d)) return 0;
    const Layout l = layout_of(d);
    return 2 * l.lines_bytes + slab_bytes(l);
}

extern "C" int ct_conv2d_wgrad_h2(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff,
                                  const unsigned* dz_absmax, float* dw, void* workspace, size_t workspace_bytes,
                                  ct_stream_t stream)
{
    const char* who = "ct_conv2d_wgrad_h2";
    if (int rc = ctdet::wgrad_check_pointers(d, dz, dw, workspace, who)) return rc;
    CT_REQUIRE(d->batch > 0 && d->cin > 0 && d->cout > 0 && d->h > 0 && d->w > 0, "%s: bad shape in d", who);
    if (!(d->kh == 1 && d->kw == 1 && d->pad_h == 0 && d->pad_w == 0 && d->dil == 1 && (d->stride == 1 || d->stride == 2)))
        return ctdet::fail(CT_ERR_UNSUPPORTED, "%s: geometry of d: needs a 1x1 filter, pad 0, dilation 1, stride 1 or 2 (got %dx%d "
                           "pad %d,%d dilation %d stride %d)", who, d->kh, d->kw, d->pad_h, d->pad_w, d->dil, d->stride);
    CT_REQUIRE(d->oh == (d->h - 1) / d->stride + 1 && d->ow == (d->w - 1) / d->stride + 1,
               "%s: oh/ow mismatch in d (%dx%d for a %dx%d input, stride %d)", who, d->oh, d->ow, d->h, d->w, d->stride);
    if (int rc = ctdet::wgrad_check_slices(d, dz_ctot, dz_coff, who)) return rc;
    // one launch covers the batch; an oversized one is a missing kernel here, not a bad argument
    const ctdet::WgradLimits lim = ctdet::wgrad_sizes(d, dz_ctot);
    if (lim.x_bytes >= kMaxBufBytes || lim.z_bytes >= kMaxBufBytes)
        return ctdet::fail(CT_ERR_UNSUPPORTED, "%s: buffers of d->in / dz above 2 GiB are not built (ct_conv2d_wgrad takes them in "
                           "batch chunks)", who);
    const Layout l = layout_of(d);
    const size_t need = 2 * l.lines_bytes + slab_bytes(l);
    if (workspace_bytes < need)
        return ctdet::fail(CT_ERR_WORKSPACE, "ct_conv2d_wgrad_h2: workspace_bytes is %zu, needs %zu", workspace_bytes, need);

    hipStream_t st = ctdet::as_stream(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    const int OHW = d->oh * d->ow, HW = d->h * d->w;
    const unsigned* x_lines = d->in_absmax;
    const unsigned* z_lines = dz_absmax;
    if (!x_lines || !z_lines) {
        // the missing maxima, into lines of our own (the workspace may hold anything)
        CT_HIP(hipMemsetAsync(ws, 0, 2 * l.lines_bytes, st));
        if (!x_lines) {
            unsigned* lines = reinterpret_cast<unsigned*>(ws);
            const int rc = ct_absmax_f32(d->in + (size_t)d->in_coff * HW, d->batch, (long long)d->cin * HW,
                                         (long long)d->in_ctot * HW, lines, stream);
            if (rc != CT_OK) return rc;
            x_lines = lines;
        }
        if (!z_lines) {
            unsigned* lines = reinterpret_cast<unsigned*>(ws + l.lines_bytes);
            const int rc = ct_absmax_f32(dz + (size_t)dz_coff * OHW, d->batch, (long long)d->cout * OHW,
                                         (long long)dz_ctot * OHW, lines, stream);
            if (rc != CT_OK) return rc;
            z_lines = lines;
        }
    }
    WgradH2Args a{};
    ctdet::wgrad_fill(a, d, dz, dz_ctot, dz_coff, lim, 0, d->batch);
    a.slabs = reinterpret_cast<float*>(ws + 2 * l.lines_bytes);
    a.x_lines = x_lines; a.z_lines = z_lines;
    a.batch = d->batch;
    a.HW = HW; a.W = d->w;
    a.OHW = OHW; a.OW = d->ow;
    a.stride = d->stride;
    a.G = l.G; a.groups = l.groups;
    a.tiles_m = l.tiles_m; a.stages_per_split = l.stages_per_split;
    const dim3 grid(l.tiles_m * l.tiles_n, l.splits), block(256);
    {
        CT_PROF("wgrad_h2_gemm", st);
        if (d->stride == 1) hipLaunchKernelGGL(wgrad_h2_gemm<false>, grid, block, LDS_BYTES, st, a);
        else hipLaunchKernelGGL(wgrad_h2_gemm<true>, grid, block, LDS_BYTES, st, a);
        CT_LAUNCH_CHECK("wgrad_h2_gemm");
    }
    {
        CT_PROF("wgrad_h2_finish", st);
        const int n = d->cout * d->cin;
        hipLaunchKernelGGL(wgrad_h2_finish, dim3((n + 255) / 256), dim3(256), 0, st, a.slabs, l.splits, n, z_lines, x_lines,
                           d->batch, dw);
        CT_LAUNCH_CHECK("wgrad_h2_finish");
    }
    return CT_OK;
}
