// libctdet: the direct weight gradient of a convolution (ct_conv2d_wgrad and its deterministic twin), an fp32 MFMA GEMM over
// the output pixels.  The other routes: ct_wino_wgrad.hip, ct_wino4_wgrad.hip, ct_wgrad_h2.hip; the launch checks they share:
// ct_wgrad_launch.h.  The data gradient of a convolution is the `transposed` mode of ct_conv2d_fwd (ct_conv.hip).
#include "ct_common.h"
#include "ct_device.h"
#include "ct_wgrad_launch.h"
#include <algorithm>
#include <cstdint>

namespace {

using ctdet::f32x16;
using ctdet::kInvalidOff;
using ctdet::kMaxBufBytes;
using ctdet::make_rsrc;

// ------------------------------------------------------------------------------------------
// weight gradient:  dW[co][ci][kh][kw] = sum_{n,oh,ow} dZ[n][co][oh][ow] * X[n][ci][ih][iw]
// GEMM  M = cout, N = cin*kh*kw, K = batch*oh*ow (pixels), fp32 MFMA 32x32x2, 128x128 (or 64x64) tile,
// split over pixel ranges across workgroups (fp32 atomicAdd into a zeroed dW; with WgradArgs::slab every split stores its
// tile into its own [Cout][Ncols] slab instead, and ctdet::wgrad_slab_sum adds the slabs in order: ct_conv2d_wgrad_det).
// Lanes run along pixels (coalesced rows of dZ and of the shifted X), tiles are staged to LDS
// transposed ([pixel][row], stride 65) so the MFMA fragments read conflict-free.
// ------------------------------------------------------------------------------------------
struct WgradArgs {
    const float* x;
    const float* dz;
    float* dw;
    float* slab;             // null: atomics into dw.  Else slab blockIdx.y of [splits][Cout][Ncols], every element stored
    unsigned x_bytes, dz_bytes;
    int Cin, H, W, x_ctot, x_coff;
    int Cout, OW, OHW, dz_ctot, dz_coff;
    int stride, pad_h, pad_w, dil;
    int Npix, Ncols;
    int tiles_m, tiles_n, pix_per_split;
};

// TAPMAJOR (needs cin % (64*TB) == 0): the GEMM columns are ordered tap-major (col = tap*cin + ci), so all rows of
// a column tile share ONE filter tap: the shifted-pixel offset and its bounds test are computed once per chunk and
// lane instead of once per gathered row -- the generic path spends ~12 VALU instructions per MFMA on that and starves
// the matrix pipe (measured 78 TFLOP/s, half of peak, independent of tile shape).
template <int KH, int KW, int TB, bool TAPMAJOR>
__global__ __launch_bounds__(256) void conv_wgrad_f32(const WgradArgs a)
{
    // workgroup tile (64*TB couts) x (64*TB columns), each wave TB x TB accumulator blocks of 32x32
    constexpr int KHW = KH * KW;
    constexpr int BM = 64 * TB, BN = 64 * TB, BKP = 64, LD = BM + 1, ROWS = 16 * TB;
    extern __shared__ float wg_lds[];
    float* As = wg_lds;
    float* Bs = wg_lds + BKP * LD;

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hsel = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave & 1) * 32 * TB, wn0 = (wave >> 1) * 32 * TB;
    const int tile = blockIdx.x;
    const int m0 = (tile % a.tiles_m) * BM;
    const int c0 = (tile / a.tiles_m) * BN;
    const int p_begin = blockIdx.y * a.pix_per_split;
    const int p_end = min(p_begin + a.pix_per_split, a.Npix);
    if (p_begin >= p_end) return;

    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rz = make_rsrc(a.dz, a.dz_bytes);
    const int HW = a.H * a.W;

    // wave-uniform row descriptors: A rows = cout m0 + wave + 4j, B rows = column c0 + wave + 4j
    int a_soff[ROWS], b_soff[ROWS], b_dh[ROWS], b_dw[ROWS];
    const int tm_tap = TAPMAJOR ? c0 / a.Cin : 0, tm_ci0 = TAPMAJOR ? c0 - tm_tap * a.Cin : 0;
    const int tm_dh = (tm_tap / KW) * a.dil - a.pad_h, tm_dw = (tm_tap % KW) * a.dil - a.pad_w;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int m = m0 + wave + 4 * j;
        a_soff[j] = min(m, a.Cout - 1) * a.OHW * 4;      // rows past Cout repeat the last one: their results are never stored
        if (TAPMAJOR) {
            b_soff[j] = (tm_ci0 + wave + 4 * j) * HW * 4;
            b_dh[j] = tm_dh;
            b_dw[j] = tm_dw;
        } else {
            const int col = c0 + wave + 4 * j;
            const int ci = col / KHW, tap = col - ci * KHW;
            const int kh = tap / KW, kw = tap - kh * KW;
            b_soff[j] = min(ci, a.Cin - 1) * HW * 4;    // columns past Ncols: clamped, never stored
            b_dh[j] = kh * a.dil - a.pad_h;
            b_dw[j] = kw * a.dil - a.pad_w;
        }
    }

    float areg[ROWS], breg[ROWS];
    auto load_chunk = [&](int p0) {
        const int P = p0 + lane;
        const bool pv = P < p_end;
        const int Pc = pv ? P : 0;
        const int n = Pc / a.OHW;
        const int s = Pc - n * a.OHW;
        const int oh = s / a.OW, ow = s - oh * a.OW;
        const int zoff = pv ? ((n * a.dz_ctot + a.dz_coff) * a.OHW + s) * 4 : kInvalidOff;
        const int xbase = (n * a.x_ctot + a.x_coff) * HW;
        const int ih0 = oh * a.stride, iw0 = ow * a.stride;
        if (TAPMAJOR) {
            const int ih = ih0 + tm_dh, iw = iw0 + tm_dw;
            const bool ok = pv && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
            const int xoff = ok ? (xbase + ih * a.W + iw) * 4 : kInvalidOff;
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                areg[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rz, zoff, a_soff[j], 0));
                breg[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, xoff, b_soff[j], 0));
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            areg[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rz, zoff, a_soff[j], 0));
            const int ih = ih0 + b_dh[j], iw = iw0 + b_dw[j];
            const bool ok = pv && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
            const int xoff = ok ? (xbase + ih * a.W + iw) * 4 : kInvalidOff;
            breg[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, xoff, b_soff[j], 0));
        }
    };

    f32x16 acc[TB][TB], acc2[TB][TB];
#pragma unroll
    for (int i = 0; i < TB; ++i)
#pragma unroll
        for (int j = 0; j < TB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; acc2[i][j][r] = 0.f; }

    if (TAPMAJOR && TB == 1) {
        // Pipelined variant (same structure as the forward implicit-GEMM kernel): two LDS buffers, ONE barrier
        // per chunk; in k-pair slot e the wave stores element e of chunk c+1 (loaded during chunk c-1) into
        // the other buffer and re-issues the load of element e for chunk c+2, then runs the slot's MFMA.
        float* As2 = wg_lds + 2 * BKP * LD;
        float* Bs2 = As2 + BKP * LD;
        int zoff, xoff;
        auto setup = [&](int p0) {
            const int P = p0 + lane;
            const bool pv = P < p_end;
            const int Pc = pv ? P : 0;
            const int n = Pc / a.OHW;
            const int sp = Pc - n * a.OHW;
            const int oh = sp / a.OW, ow = sp - oh * a.OW;
            zoff = pv ? ((n * a.dz_ctot + a.dz_coff) * a.OHW + sp) * 4 : kInvalidOff;
            const int ih = oh * a.stride + tm_dh, iw = ow * a.stride + tm_dw;
            const bool ok = pv && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
            xoff = ok ? ((n * a.x_ctot + a.x_coff) * HW + ih * a.W + iw) * 4 : kInvalidOff;
        };
        auto load_e = [&](int e) {
            if (e < ROWS) areg[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rz, zoff, a_soff[e], 0));
            else breg[e - ROWS] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, xoff, b_soff[e - ROWS], 0));
        };
        auto store_e = [&](int e, float* Ad, float* Bd) {
            if (e < ROWS) Ad[lane * LD + wave + 4 * e] = areg[e];
            else Bd[lane * LD + wave + 4 * (e - ROWS)] = breg[e - ROWS];
        };
        setup(p_begin);
#pragma unroll
        for (int e = 0; e < 2 * ROWS; ++e) load_e(e);
#pragma unroll
        for (int e = 0; e < 2 * ROWS; ++e) store_e(e, As, Bs);
        setup(p_begin + BKP);                    // past the end: every offset invalid -> zeros
#pragma unroll
        for (int e = 0; e < 2 * ROWS; ++e) load_e(e);
        __syncthreads();
        int cidx = 0;
        for (int p0 = p_begin; p0 < p_end; p0 += BKP, ++cidx) {
            const float* Ac = (cidx & 1) ? As2 : As;
            const float* Bc = (cidx & 1) ? Bs2 : Bs;
            float* An = (cidx & 1) ? As : As2;
            float* Bn = (cidx & 1) ? Bs : Bs2;
            const float* Ab = Ac + hsel * LD + wm0 + l31;
            const float* Bb = Bc + hsel * LD + wn0 + l31;
            // registers hold chunk c+1; the loads issued below fetch chunk c+2
            setup(p0 + 2 * BKP);
            float af[2], bf[2];
            af[0] = Ab[0];
            bf[0] = Bb[0];
#pragma unroll
            for (int sidx = 0; sidx < BKP / 2; ++sidx) {
                const int cur = sidx & 1;
                if (sidx + 1 < BKP / 2) {
                    af[cur ^ 1] = Ab[(2 * sidx + 2) * LD];
                    bf[cur ^ 1] = Bb[(2 * sidx + 2) * LD];
                }
                store_e(sidx, An, Bn);
                load_e(sidx);
                if (sidx & 1) acc2[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur], bf[cur], acc2[0][0], 0, 0, 0);
                else acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur], bf[cur], acc[0][0], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
        }
    } else {
    load_chunk(p_begin);
        for (int p0 = p_begin; p0 < p_end; p0 += BKP) {
    #pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                As[lane * LD + wave + 4 * j] = areg[j];
                Bs[lane * LD + wave + 4 * j] = breg[j];
            }
            __syncthreads();
            if (p0 + BKP < p_end) load_chunk(p0 + BKP);
            const float* Ab = As + hsel * LD + wm0 + l31;
            const float* Bb = Bs + hsel * LD + wn0 + l31;
    #pragma unroll 8
            for (int s = 0; s < BKP / 2; ++s) {
                float af[TB], bf[TB];
    #pragma unroll
                for (int i = 0; i < TB; ++i) {
                    af[i] = Ab[(2 * s) * LD + 32 * i];
                    bf[i] = Bb[(2 * s) * LD + 32 * i];
                }
    #pragma unroll
                for (int i = 0; i < TB; ++i)
    #pragma unroll
                    for (int j = 0; j < TB; ++j) {
                        if (s & 1) acc2[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc2[i][j], 0, 0, 0);
                        else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
                    }
            }
            __syncthreads();
        }
    }

#pragma unroll
    for (int j = 0; j < TB; ++j) {
        int col = c0 + wn0 + 32 * j + l31;
        if (col >= a.Ncols) continue;
        if (TAPMAJOR) col = (tm_ci0 + wn0 + 32 * j + l31) * KHW + tm_tap;      // back to dW's [ci][tap] order
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm0 + 32 * i + ctdet::acc_row(r, hsel);
                if (m >= a.Cout) continue;
                const float v = acc[i][j][r] + acc2[i][j][r];
                if (a.slab) a.slab[((size_t)blockIdx.y * a.Cout + m) * a.Ncols + col] = v;
                else unsafeAtomicAdd(a.dw + (size_t)m * a.Ncols + col, v);
            }
    }
}

}  // namespace

static bool wgrad_filter_built(const ct_conv_desc* d)
{
    return (d->kh == 3 && d->kw == 3) || (d->kh == 1 && d->kw == 1) || (d->kh == 1 && d->kw == 3) || (d->kh == 3 && d->kw == 1) ||
           (d->kh == 4 && d->kw == 4);
}

// Tile edge and pixel splits of a launch over nb images: a pure function of the descriptor and the environment (host only).
struct WgradPlan { int tb, tiles_m, tiles_n, splits, pix_per_split; };
static WgradPlan wgrad_plan(const ct_conv_desc* d, int nb)
{
    WgradPlan p{};
    const int Npix = nb * d->oh * d->ow, Ncols = d->cin * d->kh * d->kw;
    // the 128x128 variant (TB = 2) measured slower on the RFBNet shapes (fewer pixel splits in flight, the
    // 64 gathers per thread arrive in one burst); kept for experiments behind CTDET_WGRAD_TB=2
    static const int tb_env = getenv("CTDET_WGRAD_TB") ? atoi(getenv("CTDET_WGRAD_TB")) : 1;
    p.tb = (tb_env == 2 && d->cout >= 96 && Ncols >= 96) ? 2 : 1;
    const int bt = 64 * p.tb;
    p.tiles_m = (d->cout + bt - 1) / bt;
    p.tiles_n = (Ncols + bt - 1) / bt;
    const int tiles = p.tiles_m * p.tiles_n;
    // Pixel splits: the chip holds `slots` workgroups at a time (2 per CU with the double-buffered LDS); take the
    // smallest split count whose last round is at least 92 % full -- one workgroup too many costs a whole round,
    // and every extra split pays the atomic epilogue again.
    static const int slots = getenv("CTDET_WGRAD_WGS") ? atoi(getenv("CTDET_WGRAD_WGS")) : 512;
    const int smax = std::max(1, std::min((Npix + 255) / 256, (4 * slots) / tiles));
    int splits = 1;
    double best = 0.0;
    for (int sp = 1; sp <= smax; ++sp) {
        const int wg = tiles * sp, rounds = (wg + slots - 1) / slots;
        const double eff = (double)wg / ((double)rounds * slots);
        if (eff > best + 1e-9) { best = eff; splits = sp; }
        if (eff >= 0.92) break;
    }
    const ctdet::Split sp = ctdet::even_split((Npix + 63) / 64, splits);       // in blocks of 64 pixels: no split is empty
    p.pix_per_split = sp.per_split * 64;
    p.splits = sp.splits;
    return p;
}

// the images [b0, b0 + nb) of the batch; the first chunk zeroes dw.  slab != null (ct_conv2d_wgrad_det): the chunk's splits
// store into slab[0 .. splits) instead and dw is left to the caller's slab sum.
static int wgrad_chunk(const char* who, const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, float* dw,
                       const ctdet::WgradLimits& lim, int b0, int nb, const WgradPlan& plan, float* slab, ct_stream_t stream)
{
    WgradArgs a{};
    ctdet::wgrad_fill(a, d, dz, dz_ctot, dz_coff, lim, b0, nb);
    a.dw = dw;
    a.slab = slab;
    a.H = d->h; a.W = d->w;
    a.OW = d->ow; a.OHW = d->oh * d->ow;
    a.stride = d->stride; a.pad_h = d->pad_h; a.pad_w = d->pad_w; a.dil = d->dil;
    a.Npix = nb * a.OHW;
    a.Ncols = d->cin * d->kh * d->kw;
    const int tb = plan.tb, bt = 64 * tb;
    a.tiles_m = plan.tiles_m;
    a.tiles_n = plan.tiles_n;
    const int tiles = a.tiles_m * a.tiles_n;
    a.pix_per_split = plan.pix_per_split;
    const int splits = plan.splits;
    hipStream_t st = ctdet::as_stream(stream);
    if (!slab && b0 == 0 && !ctdet::scratch_prezeroed()) CT_HIP(hipMemsetAsync(dw, 0, (size_t)d->cout * a.Ncols * 4, st));
    const bool tapmajor = d->cin % bt == 0 && !(getenv("CTDET_WGRAD_GENERIC"));
    const bool tapmajor_for_smem = tapmajor;
    const dim3 grid(tiles, splits), block(256);
    const bool pipelined = tapmajor_for_smem && tb == 1;
    const size_t smem = (pipelined ? 4 : 2) * 64 * (size_t)(bt + 1) * 4;
    hipError_t le = hipSuccess;
    auto go = [&](auto kernel) {
        le = ctdet::raise_lds_limit((const void*)kernel, smem);
        if (le == hipSuccess) hipLaunchKernelGGL(kernel, grid, block, smem, st, a);
    };
#define CT_WGRAD_GO(KH, KW)                                                    \
    do {                                                                       \
        if (tb == 2 && tapmajor) go(conv_wgrad_f32<KH, KW, 2, true>);          \
        else if (tb == 2) go(conv_wgrad_f32<KH, KW, 2, false>);                \
        else if (tapmajor) go(conv_wgrad_f32<KH, KW, 1, true>);                \
        else go(conv_wgrad_f32<KH, KW, 1, false>);                             \
    } while (0)
    if (d->kh == 3 && d->kw == 3) CT_WGRAD_GO(3, 3);
    else if (d->kh == 1 && d->kw == 1) CT_WGRAD_GO(1, 1);
    else if (d->kh == 1 && d->kw == 3) CT_WGRAD_GO(1, 3);
    else if (d->kh == 3 && d->kw == 1) CT_WGRAD_GO(3, 1);
    else if (d->kh == 4 && d->kw == 4) CT_WGRAD_GO(4, 4);
    else return ctdet::fail(CT_ERR_UNSUPPORTED, "%s: %dx%d filters not built", who, d->kh, d->kw);
#undef CT_WGRAD_GO
    CT_HIP(le);
    CT_LAUNCH_CHECK("conv_wgrad_f32");
    return CT_OK;
}

static bool wgrad_geometry_ok(const ct_conv_desc* d)
{
    if (d->stride < 1 || d->dil < 1 || d->kh < 1 || d->kw < 1) return false;
    const int eoh = (d->h + 2 * d->pad_h - d->dil * (d->kh - 1) - 1) / d->stride + 1;
    const int eow = (d->w + 2 * d->pad_w - d->dil * (d->kw - 1) - 1) / d->stride + 1;
    return eoh == d->oh && eow == d->ow;
}

// slabs of all batch chunks of a launch, in chunk order (the count ct_conv2d_wgrad_det writes and sums)
static int wgrad_total_splits(const ct_conv_desc* d, const ctdet::WgradLimits& lim)
{
    int total = 0;
    for (int b0 = 0; b0 < d->batch; b0 += lim.max_chunk) total += wgrad_plan(d, std::min(lim.max_chunk, d->batch - b0)).splits;
    return total;
}

// ws == null: ct_conv2d_wgrad (atomics); else ct_conv2d_wgrad_det with ws_bytes of slabs
static int wgrad_impl(const char* who, const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, float* dw, bool det, void* ws,
                      size_t ws_bytes, ct_stream_t stream)
{
    if (int rc = ctdet::wgrad_check_pointers(d, dz, dw, det ? ws : ctdet::no_workspace(), who)) return rc;
    if (int rc = ctdet::wgrad_check_slices(d, dz_ctot, dz_coff, who)) return rc;
    CT_REQUIRE(wgrad_geometry_ok(d), "%s: oh/ow mismatch", who);
    // buffers above 2 GiB (32-bit buffer offsets): batch chunks accumulate into the same dw (det: append their slabs)
    ctdet::WgradLimits lim;
    if (int rc = ctdet::wgrad_limits(d, dz_ctot, who, &lim, kMaxBufBytes - 1)) return rc;
    const size_t n = (size_t)d->cout * d->cin * d->kh * d->kw;
    int total = 0;
    if (det) {
        if (!wgrad_filter_built(d)) return ctdet::fail(CT_ERR_UNSUPPORTED, "%s: %dx%d filters not built", who, d->kh, d->kw);
        if (int rc = ctdet::wgrad_check_det_workspace(ws, ws_bytes, (size_t)wgrad_total_splits(d, lim) * n * sizeof(float), who)) return rc;
    }
    for (int b0 = 0; b0 < d->batch; b0 += lim.max_chunk) {
        const int nb = std::min(lim.max_chunk, d->batch - b0);
        float* slab = det ? static_cast<float*>(ws) + (size_t)total * n : nullptr;
        const WgradPlan plan = wgrad_plan(d, nb);
        if (int rc = wgrad_chunk(who, d, dz, dz_ctot, dz_coff, dw, lim, b0, nb, plan, slab, stream)) return rc;
        total += plan.splits;
    }
    if (det) {
        if (int rc = ctdet::wgrad_slab_sum(static_cast<const float*>(ws), total, n, dw, ctdet::as_stream(stream))) return rc;
    }
    return CT_OK;
}

extern "C" int ct_conv2d_wgrad(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff,
                               float* dw, ct_stream_t stream)
{
    return wgrad_impl("ct_conv2d_wgrad", d, dz, dz_ctot, dz_coff, dw, false, nullptr, 0, stream);
}

extern "C" size_t ct_conv_wgrad_det_workspace_bytes(const ct_conv_desc* d, int* partials)
{
    if (partials) *partials = 0;
    if (!d || d->batch <= 0 || d->cin <= 0 || d->cout <= 0 || d->oh <= 0 || d->ow <= 0 || !wgrad_geometry_ok(d) ||
        !wgrad_filter_built(d))
        return 0;
    const ctdet::WgradLimits lim = ctdet::wgrad_sizes(d, d->cout, kMaxBufBytes - 1);      // dZ taken as dense
    if (lim.img_x_bytes >= kMaxBufBytes || lim.img_z_bytes >= kMaxBufBytes) return 0;
    const int total = wgrad_total_splits(d, lim);
    if (partials) *partials = total;
    return (size_t)total * d->cout * d->cin * d->kh * d->kw * sizeof(float);
}

extern "C" int ct_conv2d_wgrad_det(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, float* dw, void* workspace,
                                   size_t workspace_bytes, ct_stream_t stream)
{
    return wgrad_impl("ct_conv2d_wgrad_det", d, dz, dz_ctot, dz_coff, dw, true, workspace, workspace_bytes, stream);
}
