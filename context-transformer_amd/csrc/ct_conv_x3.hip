// libctdet: fp32 convolution on the bf16 matrix pipe -- "bf16x3": every fp32 operand is split EXACTLY into three
// bfloat16 pieces (x = hi + mid + lo, 3 x 8 significant bits, by truncation) and the product a.b is evaluated as the
// six piece products of weight 2^0 .. 2^-16 (hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid) on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation; the three dropped products are below 2^-24 |a.b|.  Same layers,
// descriptor and fused epilogue as ct_conv2d_fwd (models/RFB_Net_vgg.py:7-22 BasicConv, the plain Conv2d layers and the
// multibox heads :238-248): NCHW fp32 in, NCHW fp32 / channels-last head scatter out.
//
// Why: the fp32-input MFMA runs at the vector rate (157 TFLOP/s); the bf16 MFMA at 16x that, so six bf16 MFMAs cost
// 0.375 of one fp32 MFMA (MI355X_MICROARCH.md) -- for the layers that have no Winograd form (1x1, dilated, strided,
// 1x3 / 3x1: ~40 % of the conv time of a step).  Accuracy: bf16 x bf16 products are exact in fp32 and a k-group of 16
// is summed inside the MFMA before ONE rounding into the accumulator, so the accumulator sees 6 K / 16 roundings
// where the fp32 MFMA kernel (v_mfma_f32_32x32x2_f32) sees K / 2; measured per layer against fp64 in
// tests/test_gpu_x3.py (gate: no worse than ct_conv2d_fwd's error).
//
// GEMM view:  C[M = cout][N = batch*oh*ow] = W[M][K] * im2col(X)[K][N],  k ordered (channel group, tap, channel in group):
// a k-step = BK (16 or 32) input channels of ONE filter tap, so filter geometry is a runtime loop (no template per
// filter size) and a thread's gather of a k-step is 8 loads `buffer_load_dword voffset = its pixel at that tap,
// soffset = wave-uniform channel` (adjacent lanes = adjacent pixels: coalesced; out-of-range offset = 0 = padding).
//   workgroup 256 threads = 4 waves, tile BM x BN in {128x128, 64x128, 128x64, 64x64}, wave tile (BM/2) x (BN/2)
//   B side: thread (pixel p = tid % BN, k-octet) loads 8 channels, splits them in registers (4 VALU per element + 3
//     v_perm per pair) and writes three 16-byte rows into LDS [piece][k-octet][pixel][8 bf16]: linear in the lane
//     index, so every ds_write_b128 / ds_read_b128 is conflict-free without padding;
//   A side: the weights are split once per parameter version by ct_conv_pack_weights_x3 into
//     [k-step][piece][k-octet][m_pad][8 bf16]; a tile is three contiguous runs per octet, copied with 16-byte loads;
//   LDS double buffered, one barrier per k-step; the loads of step s+1 are issued before the MFMAs of step s.
// Small maps use the same deterministic slab split-K as ct_conv2d_fwd (desc->ksplit).
#include "ct_common.h"
#include "ct_conv_emit.h"
#include "ct_conv_launch.h"
#include "ct_device.h"
#include "ct_f16x2.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace {

using ctdet::bf16x8;
using ctdet::f16x8;
using ctdet::f32x16;
using ctdet::i32x4;
using ctdet::kInvalidOff;
using ctdet::kMaxBufBytes;
using ctdet::make_rsrc;
using ctdet::split3;
using ctdet::pack_hi;


struct X3Args {
    const float* in;
    const unsigned char* wx3;       // [step][piece 3][octet BK/8][m_pad][8 bf16]
    const float* scale;
    const float* shift;
    const float* res;
    const float* lo;
    float* out;
    unsigned in_bytes, w_bytes;
    int Cin, H, W, in_ctot, in_coff;
    int M, M_pad, cgroups, KH, KW;
    int stride, pad_h, pad_w, dil;
    int OW, OHW, Npix;
    int out_ctot, out_coff, res_ctot, res_coff;
    float res_scale;
    int relu;
    int nseg;
    ct_out_segment seg[3];
    int tiles_m, tiles_n;
    int ksplit, steps_per_split, nsteps;
    int transposed;                 // data gradient: `in` = dY, output pixel = input pixel of the forward convolution
    float* ws;
    // f16x2 form (H2 instantiations, ct_f16x2.h): activations are split as x 2^eX with eX from the producer's maximum of |input|
    // (ct_conv_desc.in_absmax), the weights arrive as w 2^eW (eW in the trailer of the split weights); the epilogue's per-channel
    // scale takes 2^-(eX + eW)
    const unsigned* in_amax;
    const int* eW;
    unsigned* out_amax;             // ct_conv_desc.out_absmax: max |y| of what the launch stores, or null (any form)
};

// ---- epilogue (the arithmetic of ct_conv2d_fwd), shared by conv_x3_f32 and its pointwise form conv_x3_f32_pw: the wave's
// (BM/2) x (BN/2) block of sums `acc` (DUAL already folded in) -> scale / shift, residual, floor, maxima, stores.  `lds`: the
// workgroup's operand tiles, dead after the last barrier of the k-loop.
template <int BM, int BN, bool H2, int TM, int TN>
__device__ __forceinline__ void x3_epilogue(const X3Args& a, const f32x16 (&acc)[TM][TN], unsigned char* lds, int m0, int n0,
                                            int wm0, int wn0, int tid, int l31, int hsel)
{
    float* const ev = reinterpret_cast<float*>(lds);              // [3][BM]: scale, shift, floor (the operand tiles are dead)
    for (int i = tid; i < BM; i += 256) ctdet::stage_epilogue_vector<BM>(ev, a, m0, i);
    __syncthreads();
    const bool track = a.out_amax != nullptr;
    int eW = 0;
    if constexpr (H2) eW = *a.eW;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int P = n0 + wn0 + j * 32 + l31;
        const bool live = P < a.Npix;
        const int n = live ? P / a.OHW : -1;
        float amax_run = 0.f;                       // a.out_amax: the thread's maximum of |v| over what it stores for pixel P's image
        if (live) {
            const int s = P - n * a.OHW;
            // f16x2: the sums carry 2^(eX[image] + eW); undone with an exact power of two in front of the per-channel scale
            ctdet::h2::pow2x2 ymul{1.f, 1.f};
            if constexpr (H2) ymul = ctdet::h2::unscale_for(eW, ctdet::h2::image_exponent(a.in_amax, n, ctdet::h2::kGrowthNone));
            float* const orow = a.nseg == 0 ? a.out + ((size_t)n * a.out_ctot + a.out_coff) * a.OHW + s : nullptr;
            const float* const rrow = a.res ? a.res + ((size_t)n * a.res_ctot + a.res_coff) * a.OHW + s : nullptr;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                // the residual values of the whole 32 x 32 block first, sixteen loads in flight: taken one by one between the
                // stores (which they may alias, so the compiler keeps the order) every load waited a full round trip behind the
                // previous store -- the RFB blocks' ConvLinear layers ran at 0.6 of the rate of the same GEMM without a shortcut
                float rv[16];
                if (rrow) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int co = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
                        rv[r] = co < a.M ? rrow[(size_t)co * a.OHW] : 0.f;
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int cl = wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;      // cout inside the tile
                    const int co = m0 + cl;
                    if (co >= a.M) continue;
                    float v = (H2 ? (acc[i][j][r] * ymul.lo) * ymul.hi : acc[i][j][r]) * ev[cl] + ev[BM + cl];
                    if (rrow) v = v * a.res_scale + rv[r];
                    { const float fl = ev[2 * BM + cl]; v = v < fl ? fl : v; }      // NaN propagates (torch.relu / no clamp)
                    if (track) ctdet::h2::track_absmax(amax_run, v);
                    if (a.nseg == 0) {
                        orow[(size_t)co * a.OHW] = v;
                    } else {
#pragma unroll
                        for (int g = 0; g < 3; ++g)
                            if (g < a.nseg && co >= a.seg[g].co_begin && co < a.seg[g].co_end)
                                a.seg[g].ptr[(size_t)n * a.seg[g].img_stride + a.seg[g].base +
                                             (size_t)s * a.seg[g].pix_stride + (co - a.seg[g].co_begin)] = v;
                    }
                }
            }
        }
        // ct_conv_desc.out_absmax: every lane arrives here; one atomic per image present in the wave
        if (track) ctdet::h2::flush_absmax(a.out_amax, n, amax_run);
    }
}

// DUAL: the hi.hi products accumulate in one register block, the five small products (2^-8 .. 2^-16 of it) in a second
//   one, added at the end -- the large accumulator then sees K / 16 roundings instead of 6 K / 16 (measured: 2.5x less
//   error against fp64 than ct_conv2d_fwd's v_mfma_f32_32x32x2_f32, which sees K / 2).
// One k-step is ONE basic block: in source order a slice of the side work of the step (LDS write of tile s+1 from the
// staging registers, the split of one gathered element, the re-issue of the same registers' loads for tile s+2) follows
// every MFMA, and the compiler's scheduler keeps that interleaving (pinning the slots with sched_barrier measured
// 10-40 % SLOWER here, as cdna_hip_programming.md warns for 32-cycle MFMAs); first / last steps are peeled (STORE /
// LOAD flags) so no branch cuts the block.
// H2: the f16x2 operand form (csrc/ct_f16x2.h): two binary16 pieces per operand, the three products (lo, hi), (hi, lo), (hi, hi) on
//   v_mfma_f32_32x32x16_f16 -- half the MFMAs, two thirds of the LDS traffic and of the weight bytes, 2 instead of 5.5 vector
//   instructions per split activation; DUAL then keeps (hi, hi) apart from the two small products.
template <int BM, int BN, int BK, bool DUAL, bool H2>
__global__ __launch_bounds__(256, 2) void conv_x3_f32(const X3Args a)
{
    constexpr int NP = H2 ? 2 : 3;              // pieces per operand
    constexpr int NPROD = H2 ? 3 : 6;           // piece products per multiply-add
    constexpr int OCT = BK / 8;                 // k-octets per k-step
    constexpr int NH = BK / 16;                 // MFMA k-groups per k-step
    constexpr int WM = BM / 2, WN = BN / 2;     // wave tile (2 x 2 waves)
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int A_PIECE = OCT * BM * 16;      // bytes of one piece of the A tile
    constexpr int B_PIECE = OCT * BN * 16;
    constexpr int A_BYTES = NP * A_PIECE, B_BYTES = NP * B_PIECE;
    constexpr int NA = (NP * OCT * BM + 255) / 256;         // 16-byte rows of A per thread and k-step
    constexpr int OSTR = 256 / BN;                          // octet stride between a thread's gathers
    constexpr int GPT = OCT / OSTR;                         // k-octets gathered per thread and k-step
    static_assert(256 % BN == 0 && OCT % OSTR == 0 && GPT >= 1, "B staging: every thread gathers GPT whole octets");
    static_assert(TM >= 1 && TN >= 1, "wave tile");

    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];    // 2 x (A_BYTES + B_BYTES)

    const int tid = threadIdx.x;
    const int lane = tid & 63, l31 = lane & 31, hsel = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave & 1) * WM, wn0 = (wave >> 1) * WN;

    int wg;
    {   // XCD-aware tile order (cout-tile fastest): workgroups sharing an im2col tile share an L2
        const int nwg = a.tiles_m * a.tiles_n;
        const int bid = blockIdx.x;
        const int xcd = bid & 7, local = bid >> 3;
        const int q = nwg >> 3, r = nwg & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
    }
    const int m0 = (wg % a.tiles_m) * BM;
    const int n0 = (wg / a.tiles_m) * BN;

    const __amdgpu_buffer_rsrc_t rin = make_rsrc(a.in, a.in_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.wx3, a.w_bytes);

    // ---- this thread's output pixel (B gather) ----
    const int bp = tid % BN;
    const int oct0 = __builtin_amdgcn_readfirstlane(tid / BN);       // first k-octet of this thread; next: + OSTR
    const int HW = a.H * a.W;
    int img_base, ih0, iw0, bp_image;
    bool pvalid;
    {
        const int P = n0 + bp;
        pvalid = P < a.Npix;
        const int Pc = pvalid ? P : 0;
        const int n = Pc / a.OHW;
        bp_image = n;
        const int s = Pc - n * a.OHW;
        const int oh = s / a.OW, ow = s - oh * a.OW;
        // forward: (oh, ow) reads ih = oh*stride - pad + kh*dil.  transposed (this "output" pixel is the forward conv's
        // INPUT pixel, `in` is dY): dY row = (oh + pad - kh*dil) / stride when that divides
        ih0 = a.transposed ? oh + a.pad_h : oh * a.stride - a.pad_h;
        iw0 = a.transposed ? ow + a.pad_w : ow * a.stride - a.pad_w;
        img_base = (n * a.in_ctot + a.in_coff) * HW;
    }

    // ---- A staging constants ----
    int a_voff[NA], a_lds[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        int f = tid + 256 * j;
        if (f >= NP * OCT * BM) f %= (NP * OCT * BM);    // surplus lanes duplicate an element (same data, same slot)
        const int row = f % BM, po = f / BM;             // po = piece * OCT + octet
        const int col = m0 + row;
        a_voff[j] = col < a.M_pad ? (po * a.M_pad + col) * 16 : kInvalidOff;
        a_lds[j] = po * (BM * 16) + row * 16;
    }
    const int a_step_bytes = NP * OCT * a.M_pad * 16;
    // f16x2: this thread's gathered activations are split as x 2^eX with eX from the maximum of |input| of ITS pixel's image
    // (ct_f16x2.h: per image, so that an image's results do not depend on its batch mates)
    float vscale = 1.f;
    if constexpr (H2) vscale = __builtin_ldexpf(1.f, ctdet::h2::image_exponent(a.in_amax, bp_image, ctdet::h2::kGrowthNone));
    const int chan_bytes = HW * 4;

    i32x4 areg[NA];
    float breg[GPT][8];
    unsigned sh[GPT][8], sm[GPT][8], sl[GPT][8];      // split pieces of the tile being stored (bf16x3)
    int ph[GPT][4], pl[GPT][4];                       // ... packed pairs of hi / lo pieces (f16x2)

    // ---- loader state: (channel group, tap) of the NEXT tile to load, advanced tap-fastest so the BK channels of a
    // group stay in cache over the filter taps; everything wave-uniform lives in SGPRs
    const int s0 = blockIdx.y * a.steps_per_split;
    const int s1 = min(a.nsteps, s0 + a.steps_per_split);
    int ld_kh, ld_kw, ld_cbase, ld_asoff;
    {
        const int khw = a.KH * a.KW;
        const int cg = s0 / khw, tap = s0 - cg * khw;
        ld_kh = tap / a.KW;
        ld_kw = tap - ld_kh * a.KW;
        ld_cbase = cg * BK;
        ld_asoff = s0 * a_step_bytes;
    }
    int ld_voff = 0;
    const int tap_sgn = a.transposed ? -a.dil : a.dil, tap_sh = a.transposed ? a.stride - 1 : 0;
    auto begin_load = [&]() {                      // per-tile part of the gather address: this lane's pixel at the tap
        // forward: ih = ih0 + kh*dil.  transposed: th = ih0 - kh*dil must be >= 0 and divisible by the stride (1 or 2).
        // One branch-free form for both (the k-step has to stay ONE basic block): tap_sgn = +-dil, tap_sh = 0 or 1; a
        // negative th stays negative under the arithmetic shift and fails the unsigned range check.
        const int th = ih0 + ld_kh * tap_sgn, tw = iw0 + ld_kw * tap_sgn;
        const int ih = th >> tap_sh, iw = tw >> tap_sh;
        const bool ok = pvalid & ((unsigned)ih < (unsigned)a.H) & ((unsigned)iw < (unsigned)a.W) & (((th | tw) & tap_sh) == 0);
        ld_voff = ok ? (img_base + ih * a.W + iw) * 4 : kInvalidOff;
    };
    auto end_load = [&]() {                        // advance (tap, channel group)
        ld_asoff += a_step_bytes;
        ++ld_kw;
        const int wrap_w = ld_kw == a.KW;               // scalar selects, no branches
        ld_kw = wrap_w ? 0 : ld_kw;
        ld_kh += wrap_w;
        const int wrap_h = ld_kh == a.KH;
        ld_kh = wrap_h ? 0 : ld_kh;
        ld_cbase += wrap_h ? BK : 0;
    };
    auto load_a = [&](int j) { areg[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, a_voff[j], ld_asoff, 0); };
    int ld_soff = 0;                               // running channel offset of the gather (bytes, wave-uniform)
    auto load_b = [&](int g, int e) {
        // Cin is a multiple of BK (checked by the launcher): every channel of a group exists
        if (e == 0) ld_soff = (ld_cbase + (oct0 + g * OSTR) * 8) * chan_bytes;
        breg[g][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, ld_voff, ld_soff, 0));
        ld_soff += chan_bytes;
    };
    auto store_a = [&](int j, int buf) {
        *reinterpret_cast<i32x4*>(lds + buf * (A_BYTES + B_BYTES) + a_lds[j]) = areg[j];
    };
    auto store_b = [&](int g, int piece, int buf) {
        i32x4 pk;
        if constexpr (H2) {
#pragma unroll
            for (int q = 0; q < 4; ++q) pk[q] = piece == 0 ? ph[g][q] : pl[g][q];
        } else {
            const unsigned(&v)[8] = piece == 0 ? sh[g] : piece == 1 ? sm[g] : sl[g];
#pragma unroll
            for (int q = 0; q < 4; ++q) pk[q] = pack_hi(v[2 * q], v[2 * q + 1]);
        }
        *reinterpret_cast<i32x4*>(lds + buf * (A_BYTES + B_BYTES) + A_BYTES + piece * B_PIECE +
                                  ((oct0 + g * OSTR) * BN + bp) * 16) = pk;
    };
    // side work of a k-step as a list of items: A rows, then per gathered octet 8 x (split + reload) and NP x (pack + write);
    // f16x2 splits a PAIR (r, r + 1) at the even item, before either register is reloaded
    constexpr int IPG = 8 + NP;
    constexpr int NW = NA + GPT * IPG;
    auto side_item = [&](int w, int buf, auto store_c, auto load_c) {
        constexpr bool STORE = decltype(store_c)::value, LOAD = decltype(load_c)::value;
        if (w < NA) {
            if (STORE) store_a(w, buf);
            if (LOAD) load_a(w);
        } else {
            const int g = (w - NA) / IPG, r = (w - NA) % IPG;
            if (r < 8) {
                if (STORE) {
                    if constexpr (H2) {
                        if ((r & 1) == 0) ctdet::h2::split2(breg[g][r] * vscale, breg[g][r + 1] * vscale, ph[g][r >> 1], pl[g][r >> 1]);
                    } else {
                        split3(breg[g][r], sh[g][r], sm[g][r], sl[g][r]);
                    }
                }
                if (LOAD) load_b(g, r);
            } else if (STORE) {
                store_b(g, r - 8, buf);
            }
        }
    };

    f32x16 acc[TM][TN];
    f32x16 acs[DUAL ? TM : 1][DUAL ? TN : 1];     // DUAL: sum of the five small products
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[i][j][r] = 0.f;
                if (DUAL) acs[i][j][r] = 0.f;
            }

    constexpr int NMF = NH * NPROD * TM * TN;                 // MFMAs per k-step and wave
    constexpr int WPS = (NW + NMF - 2) / (NMF - 1);           // side items per MFMA slot (the last slot stays free)
    using T_ = std::true_type;
    using F_ = std::false_type;

    auto k_step = [&](int buf, auto store_c, auto load_c) {
        constexpr bool LOAD = decltype(load_c)::value;
        const unsigned char* A = lds + buf * (A_BYTES + B_BYTES) + (wm0 + l31) * 16;
        const unsigned char* B = lds + buf * (A_BYTES + B_BYTES) + A_BYTES + (wn0 + l31) * 16;
        i32x4 fa[NH][NP][TM], fb[NH][NP][TN];
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    fa[h][p][i] = *reinterpret_cast<const i32x4*>(A + p * A_PIECE + (2 * h + hsel) * (BM * 16) + i * 512);
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    fb[h][p][j] = *reinterpret_cast<const i32x4*>(B + p * B_PIECE + (2 * h + hsel) * (BN * 16) + j * 512);
            }
        if (LOAD) begin_load();
        // smallest products first: bf16x3 (mid, mid), (lo, hi), (hi, lo), (mid, hi), (hi, mid), then (hi, hi); f16x2 (lo, hi), (hi, lo), (hi, hi)
        constexpr int PA[6] = {1, H2 ? 0 : 2, 0, 1, 0, 0}, PB[6] = {H2 ? 0 : 1, H2 ? 1 : 0, H2 ? 0 : 2, 0, 1, 0};
#pragma unroll
        for (int s = 0; s < NMF; ++s) {
            const int h = s / (NPROD * TM * TN), t = (s / (TM * TN)) % NPROD, i = (s / TN) % TM, j = s % TN;
            f32x16& dst = (DUAL && t < NPROD - 1) ? acs[i][j] : acc[i][j];
            if constexpr (H2)
                dst = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[h][PA[t]][i]),
                                                             __builtin_bit_cast(f16x8, fb[h][PB[t]][j]), dst, 0, 0, 0);
            else
                dst = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[h][PA[t]][i]),
                                                              __builtin_bit_cast(bf16x8, fb[h][PB[t]][j]), dst, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < WPS; ++q) {
                const int w = s * WPS + q;
                if (w < NW) side_item(w, buf ^ 1, store_c, load_c);
            }
        }
        if (LOAD) end_load();
        // A bare barrier behind the LDS counter only: __syncthreads() carries a workgroup fence that the compiler turns into
        // s_waitcnt vmcnt(0), i.e. a wait for the global loads this step has just issued for the tile two steps ahead (the
        // staging registers are private, only the LDS tiles are shared, and the compiler still waits for a register's own
        // load before its split).  Measured in round 5: no difference on any layer (the loads of a step land within it);
        // a second set of staging registers (loads three tiles ahead) was 10-25 % SLOWER on the layers that cannot fill the
        // chip -- their ~0.7 us per 12-MFMA step is not a memory round trip.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    // prologue: tile s0 -> LDS buffer 0, tile s0 + 1 -> staging registers
    begin_load();
#pragma unroll
    for (int w = 0; w < NW; ++w) side_item(w, 0, F_{}, T_{});
    end_load();
#pragma unroll
    for (int w = 0; w < NW; ++w) side_item(w, 0, T_{}, F_{});
    if (s0 + 1 < s1) {
        begin_load();
#pragma unroll
        for (int w = 0; w < NW; ++w) side_item(w, 0, F_{}, T_{});
        end_load();
    }
    __syncthreads();
    int step = s0;
    for (; step + 2 < s1; ++step) k_step((step - s0) & 1, T_{}, T_{});
    if (step + 1 < s1) { k_step((step - s0) & 1, T_{}, F_{}); ++step; }
    k_step((step - s0) & 1, F_{}, F_{});
    if (DUAL) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += acs[i][j][r];
    }

    if (a.ksplit > 1) {
        float* const slab = a.ws + (size_t)blockIdx.y * a.M * a.Npix;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int P = n0 + wn0 + j * 32 + l31;
            if (P >= a.Npix) continue;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
                    if (co < a.M) slab[(size_t)co * a.Npix + P] = acc[i][j][r];
                }
        }
        return;
    }

    x3_epilogue<BM, BN, H2>(a, acc, lds, m0, n0, wm0, wn0, tid, l31, hsel);
}

// The pointwise form of the f16x2 twins: 1x1 / stride 1 / pad 0 forward layers, a plain GEMM C[cout][pixel] = W[cout][cin] X[cin][pixel]
// with X contiguous along the pixels.  Same tiles, wave layout, operand pieces, MFMA order per accumulator and epilogue as
// conv_x3_f32<BM, BN, BK, true, true> -- every accumulator receives the same MFMA results in the same order, so the results are
// bit-identical -- without what the generic gather pays per 16 channels:
//   * ONE barrier per 32 input channels (two MFMA k-groups) for every tile; a k16 configuration consumes two packed steps;
//   * the weights go HBM -> LDS by LDS-DMA (buffer_load ... lds, 16 bytes per lane): for a fixed (step, piece, octet) the BM rows
//     of a tile are one contiguous run of the packed buffer and that run IS the LDS image -- 32 channels are eight runs, and
//     eight runs of M_pad rows are 128 M_pad bytes in the packed buffer whatever the packing k-step; only the ORDER of the eight
//     runs differs: k16 [k-group][piece][octet 2], k32 [piece][octet 4] (run_of below).  No staging registers, no ds_write_b128;
//     rows at or beyond M_pad carry the out-of-range offset, for which the DMA writes zeros;
//   * the activations: a thread's pixel offset is computed once, the channel advances by a wave-uniform scalar add; no tap
//     counters, no bounds selects (pvalid only, for the last pixel tile).
// Pipeline of iteration `it` (tile `it` in LDS buffer it & 1): DMA of the weights of tile it + 1 into the other buffer (free since
// the barrier that ended iteration it - 1), then per k-group the fragment reads and the 3 TM TN MFMAs, and behind the MFMAs the
// split and LDS write of the activations of tile it + 1 (staging registers) with the re-issue of the same registers' loads for
// tile it + 2.  The barrier at the end waits for the LDS counter and for the DMA alone: the gathers issued after the DMA (their
// count is static) stay in flight across it (vmcnt counts loads in issue order).
template <int BM, int BN, int BK, bool DUAL, bool H2>
__global__ __launch_bounds__(256, 2) void conv_x3_f32_pw(const X3Args a)
{
    static_assert(DUAL && H2 && (BK == 16 || BK == 32), "the pointwise form exists for the dual-accumulator f16x2 twins");
    constexpr int WM = BM / 2, WN = BN / 2;     // wave tile (2 x 2 waves)
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int RUN_A = BM * 16, RUN_B = BN * 16;          // bytes of one (k-group, piece, octet) run of a tile
    constexpr int A_BYTES = 8 * RUN_A, B_BYTES = 8 * RUN_B;  // 32 channels: 2 pieces x 4 octets
    constexpr int NAD = BM / 32;                             // DMA instructions (64 rows of 16 bytes) per wave and iteration
    constexpr int OSTR = 256 / BN;                           // octet stride between a thread's gathers
    constexpr int GPT = 4 / OSTR;                            // k-octets gathered per thread and iteration
    static_assert(BM % 64 == 0 && 256 % BN == 0 && 4 % OSTR == 0 && GPT >= 1, "staging");
    // run of (k-group h, piece p, octet o of the group) among the eight runs of an iteration, in the packed buffer's order
    auto run_of = [](int h, int p, int o) { return BK == 16 ? h * 4 + p * 2 + o : p * 4 + 2 * h + o; };

    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];    // 2 x A_BYTES, then 2 x B_BYTES
    constexpr int B_BASE = 2 * A_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63, l31 = lane & 31, hsel = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave & 1) * WM, wn0 = (wave >> 1) * WN;

    int wg;
    {   // XCD-aware tile order (cout-tile fastest), as conv_x3_f32
        const int nwg = a.tiles_m * a.tiles_n;
        const int bid = blockIdx.x;
        const int xcd = bid & 7, local = bid >> 3;
        const int q = nwg >> 3, r = nwg & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
    }
    const int m0 = (wg % a.tiles_m) * BM;
    const int n0 = (wg / a.tiles_m) * BN;

    const __amdgpu_buffer_rsrc_t rin = make_rsrc(a.in, a.in_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.wx3, a.w_bytes);

    // ---- this thread's pixel (B gather): input pixel = output pixel ----
    const int bp = tid % BN;
    const int oct0 = __builtin_amdgcn_readfirstlane(tid / BN);       // first k-octet of this thread; next: + OSTR
    const int HW = a.H * a.W;
    const int chan_bytes = HW * 4;
    int b_voff;
    float vscale;
    {
        const int P = n0 + bp;
        const bool pvalid = P < a.Npix;
        const int Pc = pvalid ? P : 0;
        const int n = Pc / a.OHW;
        const int s = Pc - n * a.OHW;
        b_voff = pvalid ? ((n * a.in_ctot + a.in_coff) * HW + s) * 4 : kInvalidOff;
        // split as x 2^eX with eX from the maximum of |input| of THIS pixel's image: a pixel tile may straddle images
        vscale = __builtin_ldexpf(1.f, ctdet::h2::image_exponent(a.in_amax, n, ctdet::h2::kGrowthNone));
    }

    // ---- A: this wave's DMA instructions of an iteration: item = wave * NAD + j -> (run, 64-row half of the run) ----
    int a_voff[NAD], a_dst[NAD];
#pragma unroll
    for (int j = 0; j < NAD; ++j) {
        const int item = wave * NAD + j;
        const int run = item / (BM / 64), half = item % (BM / 64);
        const int col = m0 + half * 64 + lane;
        a_voff[j] = col < a.M_pad ? (run * a.M_pad + col) * 16 : kInvalidOff;
        a_dst[j] = run * RUN_A + half * 1024;          // wave-uniform; the lane's 16 bytes land at + lane * 16
    }
    const int a_iter_bytes = 128 * a.M_pad;            // 32 channels x 2 pieces x M_pad rows x 2 bytes
    const int niter = a.Cin / 32;                      // the launcher's rule: Cin % 32 == 0
    int a_soff = 0;                                    // next tile of the weights (bytes, wave-uniform)
    int b_tile_soff = oct0 * 8 * chan_bytes;           // next tile of the activations: its first channel of this thread

    auto dma_a = [&](int buf) {
        unsigned char* const dst = lds + buf * A_BYTES;
        (void)dst; (void)rw; (void)a_voff; (void)a_dst; (void)a_soff;         // the host pass does not see the builtin
#if defined(__HIP_DEVICE_COMPILE__)
        typedef __attribute__((address_space(3))) void* lds_ptr;
#pragma unroll
        for (int j = 0; j < NAD; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr)(dst + a_dst[j]), 16, a_voff[j], a_soff, 0, 0);
#endif
        a_soff += a_iter_bytes;
    };

    float breg[GPT][8];
    int ph[GPT][4], pl[GPT][4];                       // packed pairs of hi / lo pieces of the tile being stored
    int ld_soff = 0;
    auto load_b = [&](int g, int e) {
        if (e == 0) ld_soff = b_tile_soff + g * (OSTR * 8) * chan_bytes;
        breg[g][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, b_voff, ld_soff, 0));
        ld_soff += chan_bytes;
    };
    auto end_load_b = [&]() { b_tile_soff += 32 * chan_bytes; };
    auto store_b = [&](int g, int piece, int buf) {
        const int o4 = oct0 + g * OSTR;                // octet of the iteration: k-group o4 >> 1, octet o4 & 1 of the group
        i32x4 pk;
#pragma unroll
        for (int q = 0; q < 4; ++q) pk[q] = piece == 0 ? ph[g][q] : pl[g][q];
        *reinterpret_cast<i32x4*>(lds + B_BASE + buf * B_BYTES + run_of(o4 >> 1, piece, o4 & 1) * RUN_B + bp * 16) = pk;
    };
    // side work of an iteration as a list of items: per gathered octet 4 x (split of a pair + reload of both) and 2 x (write)
    constexpr int IPG = 4 + 2;
    constexpr int NW = GPT * IPG;
    auto side_item = [&](int w, int buf, auto store_c, auto load_c) {
        constexpr bool STORE = decltype(store_c)::value, LOAD = decltype(load_c)::value;
        const int g = w / IPG, r = w % IPG;
        if (r < 4) {
            if (STORE) ctdet::h2::split2(breg[g][2 * r] * vscale, breg[g][2 * r + 1] * vscale, ph[g][r], pl[g][r]);
            if (LOAD) { load_b(g, 2 * r); load_b(g, 2 * r + 1); }
        } else if (STORE) {
            store_b(g, r - 4, buf);
        }
    };

    f32x16 acc[TM][TN], acs[TM][TN];              // (hi, hi) products; sum of the two small products
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; acs[i][j][r] = 0.f; }

    constexpr int NMF = 2 * 3 * TM * TN;          // MFMAs per iteration and wave
    using T_ = std::true_type;
    using F_ = std::false_type;

    // STORE: tile it + 1 exists (its activations sit in the staging registers, its weights are fetched here); LOAD: tile it + 2 exists
    auto iteration = [&](int buf, auto store_c, auto load_c) {
        constexpr bool STORE = decltype(store_c)::value, LOAD = decltype(load_c)::value;
        if (STORE) dma_a(buf ^ 1);
        asm volatile("" ::: "memory");            // the DMA stays ahead of this iteration's gathers (the counted wait below)
        const unsigned char* A = lds + buf * A_BYTES + (wm0 + l31) * 16;
        const unsigned char* B = lds + B_BASE + buf * B_BYTES + (wn0 + l31) * 16;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // fragments per k-group, just ahead of their MFMAs (hoisted for the whole iteration they would cost 32 more registers)
            i32x4 fa[2][TM], fb[2][TN];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[p][i] = *reinterpret_cast<const i32x4*>(A + run_of(h, p, hsel) * RUN_A + i * 512);
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[p][j] = *reinterpret_cast<const i32x4*>(B + run_of(h, p, hsel) * RUN_B + j * 512);
            }
            // (lo, hi), (hi, lo) into the small-products accumulator, then (hi, hi) into the large one: conv_x3_f32's order
            constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
#pragma unroll
            for (int u = 0; u < NMF / 2; ++u) {
                const int t = u / (TM * TN), i = (u / TN) % TM, j = u % TN;
                f32x16& dst = t < 2 ? acs[i][j] : acc[i][j];
                dst = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[PA[t]][i]),
                                                             __builtin_bit_cast(f16x8, fb[PB[t]][j]), dst, 0, 0, 0);
                const int s = h * (NMF / 2) + u;  // side items spread evenly behind the MFMAs of the iteration
#pragma unroll
                for (int w = 0; w < NW; ++w)
                    if (w * NMF / NW == s) side_item(w, buf ^ 1, store_c, load_c);
            }
        }
        if (LOAD) end_load_b();
        // bare barrier (conv_x3_f32 says why) behind the LDS counter and the DMA: the GPT * 8 gathers issued after it stay in flight
        if (STORE) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LOAD ? GPT * 8 : 0) : "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    // prologue: tile 0 -> LDS buffer 0, the activations of tile 1 -> staging registers
    dma_a(0);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int w = 0; w < NW; ++w) side_item(w, 0, F_{}, T_{});
    end_load_b();
#pragma unroll
    for (int w = 0; w < NW; ++w) side_item(w, 0, T_{}, F_{});
    // the DMA of tile 0 was issued ahead of the gathers of tile 0, which the splits above have waited for (loads return in issue
    // order); the counted wait says so again and leaves the gathers of tile 1 in flight across the barrier, which
    // __syncthreads() would drain: one exposed memory round trip per workgroup, 5-10 % of a 16-iteration workgroup (Cin = 512)
    if (niter > 1) {
#pragma unroll
        for (int w = 0; w < NW; ++w) side_item(w, 0, F_{}, T_{});
        end_load_b();
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(GPT * 8) : "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    int it = 0;
    for (; it + 2 < niter; ++it) iteration(it & 1, T_{}, T_{});
    if (it + 1 < niter) { iteration(it & 1, T_{}, F_{}); ++it; }
    iteration(it & 1, F_{}, F_{});
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] += acs[i][j][r];

    x3_epilogue<BM, BN, H2>(a, acc, lds, m0, n0, wm0, wn0, tid, l31, hsel);
}

// ---- weight split: [cout][cin][kh][kw] fp32 -> [step = (cgroup, tap)][piece][octet][m_pad][8 bf16] ----
struct X3PackArgs {
    const float* w[6];
    int mbeg[7];
    int nparts, cin, khw, bk, m_pad, cgroups;
    int dgrad;                // rows m = forward INPUT channels, k-channels = forward OUTPUT channels (concatenated parts)
    unsigned short* out;
    // f16x2 layout: [step][piece 2][octet][m_pad][8 f16] of w 2^eW, eW from max |w| over the layer (trailer[0] = its bit pattern,
    // filled by x3h_wmax_kernel; the packing records trailer[1] = eW)
    unsigned* trailer;        // null: bf16x3
};

__device__ __forceinline__ void x3_pack_body(const X3PackArgs& p, long first, long stride)
{
    const int oct = p.bk / 8;
    const long rows = (long)p.cgroups * p.khw * oct * p.m_pad;            // 8-channel rows (all three pieces each)
    for (long idx = first; idx < rows; idx += stride) {
        const int m = (int)(idx % p.m_pad);
        long t = idx / p.m_pad;
        const int o = (int)(t % oct);
        t /= oct;
        const int tap = (int)(t % p.khw), cg = (int)(t / p.khw);
        const float* src = nullptr;
        int mm = 0;
        if (!p.dgrad) {
#pragma unroll
            for (int i = 0; i < 6; ++i)
                if (i < p.nparts && m >= p.mbeg[i] && m < p.mbeg[i + 1]) { src = p.w[i]; mm = m - p.mbeg[i]; }
        }
        const long step = (long)cg * p.khw + tap;
        const int np = p.trailer ? 2 : 3;
        unsigned short* base = p.out + (((step * np) * oct + o) * (long)p.m_pad + m) * 8;
        const long piece_stride = (long)oct * p.m_pad * 8;
        const int eW = p.trailer ? ctdet::h2::exponent_for(p.trailer[0], ctdet::h2::kGrowthNone) : 0;
        // the eight channels of a row: pieces collected in registers, ONE 16-byte store per piece (24 two-byte stores before)
        unsigned q0[4] = {0u, 0u, 0u, 0u}, q1[4] = {0u, 0u, 0u, 0u}, q2[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ci = cg * p.bk + o * 8 + e;
            float v = 0.f;
            if (!p.dgrad) {
                if (src && ci < p.cin) v = src[((size_t)mm * p.cin + ci) * p.khw + tap];
            } else if (m < p.cin) {             // ci runs over the concatenated forward output channels
#pragma unroll
                for (int i = 0; i < 6; ++i)
                    if (i < p.nparts && ci >= p.mbeg[i] && ci < p.mbeg[i + 1])
                        v = p.w[i][((size_t)(ci - p.mbeg[i]) * p.cin + m) * p.khw + tap];
            }
            const int sh = 16 * (e & 1);
            if (p.trailer) {
                const float vs = __builtin_ldexpf(v, eW);
                const _Float16 hi = (_Float16)vs;
                const _Float16 lo = (_Float16)(vs - (float)hi);
                q0[e >> 1] |= (unsigned)__builtin_bit_cast(unsigned short, hi) << sh;
                q1[e >> 1] |= (unsigned)__builtin_bit_cast(unsigned short, lo) << sh;
                continue;
            }
            unsigned h, mid, l;
            split3(v, h, mid, l);
            q0[e >> 1] |= (h >> 16) << sh;
            q1[e >> 1] |= (mid >> 16) << sh;
            q2[e >> 1] |= (l >> 16) << sh;
        }
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        *reinterpret_cast<u32x4*>(base) = u32x4{q0[0], q0[1], q0[2], q0[3]};
        *reinterpret_cast<u32x4*>(base + piece_stride) = u32x4{q1[0], q1[1], q1[2], q1[3]};
        if (!p.trailer) *reinterpret_cast<u32x4*>(base + 2 * piece_stride) = u32x4{q2[0], q2[1], q2[2], q2[3]};
    }
    if (p.trailer && first == 0) p.trailer[1] = (unsigned)ctdet::h2::exponent_for(p.trailer[0], ctdet::h2::kGrowthNone);
}

// max |w| over the parts of a layer -> trailer[0] (atomic max; the caller zeroes the trailer)
__global__ __launch_bounds__(256) void x3h_wmax_kernel(const X3PackArgs p)
{
    unsigned m = 0;
    for (int part = 0; part < p.nparts; ++part) {
        const long n = (long)(p.mbeg[part + 1] - p.mbeg[part]) * p.cin * p.khw;
        const float* w = p.w[part];
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
            const unsigned a = __builtin_bit_cast(unsigned, w[i]) & 0x7FFFFFFFu;
            m = a > m ? a : m;
        }
    }
    m = ctdet::h2::wave_max(m);
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(p.trailer, m);
}

__global__ void x3_pack_kernel(const X3PackArgs p)
{
    x3_pack_body(p, blockIdx.x * (long)blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}

// every bf16x3 weight split of a training step in ONE launch: blockIdx.y = item of a device-resident list
__global__ void x3_pack_batched_kernel(const X3PackArgs* __restrict__ items)
{
    const X3PackArgs p = items[blockIdx.y];
    x3_pack_body(p, blockIdx.x * (long)blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}

struct X3Cfg {
    int bm, bn, bk, dual;
    const char* name;
    int h2;                   // 1: the f16x2 operand form (weights from ct_conv_pack_weights_x3h, needs ct_conv_desc.in_absmax)
};
// name: x3:<BM>x<BN>k<BK>[d]   d = dual accumulators -- the configurations the engine may select (accuracy gate);
// the single-accumulator forms are kept for the comparison in tests/test_gpu_x3.py and tools/x3_probe.py
const X3Cfg kX3[] = {
    {128, 128, 16, 1, "x3:128x128k16d"}, {64, 128, 16, 1, "x3:64x128k16d"}, {128, 64, 32, 1, "x3:128x64k32d"},
    {64, 64, 32, 1, "x3:64x64k32d"},     {128, 128, 16, 0, "x3:128x128k16"}, {64, 128, 16, 0, "x3:64x128k16"},
    // the same tiles on f16x2 ("h2:..."): the engine maps a table entry x3:<tile> to h2:<tile> where the runtime uses that form
    {128, 128, 16, 1, "h2:128x128k16d", 1}, {64, 128, 16, 1, "h2:64x128k16d", 1}, {128, 64, 32, 1, "h2:128x64k32d", 1},
    {64, 64, 32, 1, "h2:64x64k32d", 1},
};
constexpr int kNumX3 = sizeof(kX3) / sizeof(kX3[0]);

template <typename K>
hipError_t launch_x3(K kernel, size_t smem, const X3Args& a, hipStream_t st)
{
    if (hipError_t e = ctdet::raise_lds_limit(reinterpret_cast<const void*>(kernel), smem)) return e;
    hipLaunchKernelGGL(kernel, dim3(a.tiles_m * a.tiles_n, a.ksplit > 1 ? a.ksplit : 1), dim3(256), smem, st, a);
    return hipGetLastError();
}

hipError_t launch_cfg(int cfg, const X3Args& a, hipStream_t st)
{
    switch (cfg) {
#define X3_CASE(idx, BM, BN, BK, DU, H2) \
    case idx: return launch_x3(conv_x3_f32<BM, BN, BK, DU, H2>, (size_t)2 * (H2 ? 2 : 3) * (BK / 8) * (BM + BN) * 16, a, st);
        X3_CASE(0, 128, 128, 16, true, false)
        X3_CASE(1, 64, 128, 16, true, false)
        X3_CASE(2, 128, 64, 32, true, false)
        X3_CASE(3, 64, 64, 32, true, false)
        X3_CASE(4, 128, 128, 16, false, false)
        X3_CASE(5, 64, 128, 16, false, false)
        X3_CASE(6, 128, 128, 16, true, true)
        X3_CASE(7, 64, 128, 16, true, true)
        X3_CASE(8, 128, 64, 32, true, true)
        X3_CASE(9, 64, 64, 32, true, true)
#undef X3_CASE
        default: return hipErrorInvalidValue;
    }
}

// the pointwise form of the four f16x2 twins (configurations 6 .. 9): 32 channels per LDS buffer whatever the packing k-step
hipError_t launch_cfg_pw(int cfg, const X3Args& a, hipStream_t st)
{
    switch (cfg) {
#define X3_PW_CASE(idx, BM, BN, BK) \
    case idx: return launch_x3(conv_x3_f32_pw<BM, BN, BK, true, true>, (size_t)2 * 8 * (BM + BN) * 16, a, st);
        X3_PW_CASE(6, 128, 128, 16)
        X3_PW_CASE(7, 64, 128, 16)
        X3_PW_CASE(8, 128, 64, 32)
        X3_PW_CASE(9, 64, 64, 32)
#undef X3_PW_CASE
        default: return hipErrorInvalidValue;
    }
}

// ct_conv_x3_pointwise_enable: process-wide, initialised ONCE from CTDET_X3_POINTWISE (default on) -- a captured graph must not
// disagree with what the environment says later
std::atomic<int>& pointwise_flag()
{
    static std::atomic<int> flag{[] {
        const char* e = getenv("CTDET_X3_POINTWISE");
        return (e && *e) ? (atoi(e) != 0 ? 1 : 0) : 1;
    }()};
    return flag;
}

// The pure rule of the pointwise form: an f16x2 twin, a forward 1x1 / stride 1 / dilation 1 / pad 0 layer into an NCHW slice (no
// head scatter), no split-K, whole 32-channel iterations.  Everything else keeps conv_x3_f32.
bool pointwise_rule(const ct_conv_desc* d, bool h2, int ksplit)
{
    return h2 && !d->transposed && d->kh == 1 && d->kw == 1 && d->stride == 1 && d->dil == 1 && d->pad_h == 0 && d->pad_w == 0 &&
           ksplit <= 1 && d->nseg == 0 && d->cin % 32 == 0;
}

}  // namespace

extern "C" int ct_conv_x3_pointwise_enable(int on) { return pointwise_flag().exchange(on != 0 ? 1 : 0); }

extern "C" int ct_conv_x3_num_configs(void) { return kNumX3; }

extern "C" const char* ct_conv_x3_config_name(int i) { return (i >= 0 && i < kNumX3) ? kX3[i].name : "?"; }

extern "C" int ct_conv_x3_config_bk(int i) { return (i >= 0 && i < kNumX3) ? kX3[i].bk : -1; }

extern "C" int ct_conv_x3_config_h2(int i) { return (i >= 0 && i < kNumX3) ? kX3[i].h2 : -1; }

constexpr int kX3hTrailerBytes = 256;

// bytes of the f16x2 split weights for k-steps of bk channels, trailer { max |w| bits, eW } included
extern "C" size_t ct_conv_x3h_packed_bytes(int cin, int cout, int kh, int kw, int bk)
{
    if (bk != 16 && bk != 32) return 0;
    const size_t cgroups = (size_t)(cin + bk - 1) / bk;
    return cgroups * kh * kw * 2 * (size_t)bk * ct_conv_mpad(cout) * 2 + kX3hTrailerBytes;
}

// bytes of the split weights for k-steps of bk (16 or 32) channels
extern "C" size_t ct_conv_x3_packed_bytes(int cin, int cout, int kh, int kw, int bk)
{
    if (bk != 16 && bk != 32) return 0;
    const size_t cgroups = (size_t)(cin + bk - 1) / bk;
    return cgroups * kh * kw * 3 * (size_t)bk * ct_conv_mpad(cout) * 2;
}

static int x3_pack_fill(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw, int bk, void* wx3,
                        int dgrad, X3PackArgs& p);

static int x3_pack_impl(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw, int bk, void* wx3,
                        int dgrad, ct_stream_t stream)
{
    X3PackArgs p{};
    if (int rc = x3_pack_fill(w, cout, nparts, cin, kh, kw, bk, wx3, dgrad, p)) return rc;
    const long rows = (long)p.cgroups * p.khw * (bk / 8) * p.m_pad;
    hipLaunchKernelGGL(x3_pack_kernel, dim3((unsigned)std::min<long>((rows + 255) / 256, 4096)), dim3(256), 0,
                       ctdet::as_stream(stream), p);
    CT_LAUNCH_CHECK("x3_pack_kernel");
    return CT_OK;
}

static int x3_pack_fill(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw, int bk, void* wx3,
                        int dgrad, X3PackArgs& p)
{
    CT_REQUIRE(w && cout && wx3, "ct_conv_pack_weights_x3: null pointer");
    CT_REQUIRE(nparts >= 1 && nparts <= 6, "ct_conv_pack_weights_x3: nparts=%d (1..6)", nparts);
    CT_REQUIRE(bk == 16 || bk == 32, "ct_conv_pack_weights_x3: bk=%d (16 or 32)", bk);
    CT_REQUIRE(cin > 0 && kh > 0 && kw > 0, "ct_conv_pack_weights_x3: bad filter shape");
    p = X3PackArgs{};
    int mtot = 0;
    for (int i = 0; i < nparts; ++i) {
        CT_REQUIRE(w[i] && cout[i] > 0, "ct_conv_pack_weights_x3: part %d", i);
        p.w[i] = w[i];
        p.mbeg[i] = mtot;
        mtot += cout[i];
    }
    for (int i = nparts; i < 7; ++i) p.mbeg[i] = mtot;
    p.nparts = nparts;
    p.cin = cin;
    p.khw = kh * kw;
    p.bk = bk;
    p.dgrad = dgrad;
    // forward: rows = concatenated couts, k-channels = cin; data gradient: rows = cin, k-channels = concatenated couts
    p.m_pad = ct_conv_mpad(dgrad ? cin : mtot);
    p.cgroups = ((dgrad ? mtot : cin) + bk - 1) / bk;
    p.out = static_cast<unsigned short*>(wx3);
    return CT_OK;
}

// A training step re-splits the weights of every bf16x3 launch (forward and data gradient): ~80 small launches.  The
// arguments never change between steps, so the caller builds the list once -- ct_conv_x3_pack_item fills ONE item of
// ct_conv_x3_pack_item_bytes() bytes in HOST memory from the arguments of ct_conv_pack_weights_x3[_dgrad] --, copies
// it to the device and replays it with ct_conv_x3_pack_run: one launch.
extern "C" size_t ct_conv_x3_pack_item_bytes(void) { return sizeof(X3PackArgs); }

extern "C" int ct_conv_x3_pack_item(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw, int bk,
                                    void* wx3, int dgrad, void* host_item)
{
    CT_REQUIRE(host_item, "ct_conv_x3_pack_item: null item");
    X3PackArgs p{};
    if (int rc = x3_pack_fill(w, cout, nparts, cin, kh, kw, bk, wx3, dgrad, p)) return rc;
    memcpy(host_item, &p, sizeof(p));
    return CT_OK;
}

extern "C" int ct_conv_x3_pack_run(const void* items_dev, int n, ct_stream_t stream)
{
    CT_REQUIRE(items_dev || n == 0, "ct_conv_x3_pack_run: null list");
    if (n <= 0) return CT_OK;
    hipLaunchKernelGGL(x3_pack_batched_kernel, dim3(64, n), dim3(256), 0, ctdet::as_stream(stream),
                       static_cast<const X3PackArgs*>(items_dev));
    CT_LAUNCH_CHECK("x3_pack_batched_kernel");
    return CT_OK;
}

extern "C" int ct_conv_pack_weights_x3(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw,
                                       int bk, void* wx3, ct_stream_t stream)
{
    return x3_pack_impl(w, cout, nparts, cin, kh, kw, bk, wx3, 0, stream);
}

// f16x2: max |w| first, then the split of w 2^eW (forward layout only; three launches, not recordable)
extern "C" int ct_conv_pack_weights_x3h(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw,
                                        int bk, void* wx3, ct_stream_t stream)
{
    X3PackArgs p{};
    if (int rc = x3_pack_fill(w, cout, nparts, cin, kh, kw, bk, wx3, 0, p)) return rc;
    hipStream_t st = ctdet::as_stream(stream);
    int mtot = p.mbeg[nparts];
    p.trailer = reinterpret_cast<unsigned*>(static_cast<unsigned char*>(wx3) + ct_conv_x3h_packed_bytes(cin, mtot, kh, kw, bk) -
                                            kX3hTrailerBytes);
    CT_HIP(hipMemsetAsync(p.trailer, 0, kX3hTrailerBytes, st));
    const long nw = (long)mtot * cin * kh * kw;
    hipLaunchKernelGGL(x3h_wmax_kernel, dim3((unsigned)std::min<long>((nw + 255) / 256, 1024)), dim3(256), 0, st, p);
    CT_LAUNCH_CHECK("x3h_wmax_kernel");
    const long rows = (long)p.cgroups * p.khw * (bk / 8) * p.m_pad;
    hipLaunchKernelGGL(x3_pack_kernel, dim3((unsigned)std::min<long>((rows + 255) / 256, 4096)), dim3(256), 0, st, p);
    CT_LAUNCH_CHECK("x3_pack_kernel");
    return CT_OK;
}

extern "C" int ct_conv_pack_weights_x3_dgrad(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw,
                                             int bk, void* wx3, ct_stream_t stream)
{
    return x3_pack_impl(w, cout, nparts, cin, kh, kw, bk, wx3, 1, stream);
}

extern "C" int ct_conv2d_x3_fwd(const ct_conv_desc* d, const void* wx3, int config, ct_stream_t stream)
{
    CT_REQUIRE(d != nullptr && wx3 != nullptr, "ct_conv2d_x3_fwd: null pointer");
    CT_REQUIRE(d->in && d->scale && d->shift, "ct_conv2d_x3_fwd: null tensor");
    CT_REQUIRE(config >= 0 && config < kNumX3, "ct_conv2d_x3_fwd: config %d (0..%d)", config, kNumX3 - 1);
    CT_REQUIRE(d->batch > 0 && d->cin > 0 && d->cout > 0 && d->h > 0 && d->w > 0, "ct_conv2d_x3_fwd: bad shape");
    CT_REQUIRE(d->kh >= 1 && d->kw >= 1 && d->stride >= 1 && d->dil >= 1, "ct_conv2d_x3_fwd: filter geometry");
    if (d->transposed && d->stride > 2)
        return ctdet::fail(CT_ERR_UNSUPPORTED, "ct_conv2d_x3_fwd(transposed): stride %d (1 or 2)", d->stride);
    const char* const who = "ct_conv2d_x3_fwd";
    if (int rc = ctdet::conv_check_sizes(d, who)) return rc;
    if (int rc = ctdet::conv_check_outputs(d, who)) return rc;
    const int bm = kX3[config].bm, bn = kX3[config].bn, bk = kX3[config].bk;
    const bool h2 = kX3[config].h2 != 0;
    CT_REQUIRE(!h2 || d->in_absmax, "ct_conv2d_x3_fwd: the f16x2 configurations need the maximum of |input| (ct_conv_desc.in_absmax: "
               "the producer's out_absmax slot, or ct_absmax_f32)");
    CT_REQUIRE(!h2 || !d->transposed, "ct_conv2d_x3_fwd: the f16x2 configurations are forward-only");
    if (d->cin % bk != 0)
        return ctdet::fail(CT_ERR_UNSUPPORTED, "ct_conv2d_x3_fwd: cin=%d is not a multiple of the k-step (%d channels)",
                           d->cin, bk);
    const int m_pad = ct_conv_mpad(d->cout);
    const size_t wbytes = h2 ? ct_conv_x3h_packed_bytes(d->cin, d->cout, d->kh, d->kw, bk) - kX3hTrailerBytes
                             : ct_conv_x3_packed_bytes(d->cin, d->cout, d->kh, d->kw, bk);
    CT_REQUIRE((long long)wbytes < kMaxBufBytes, "ct_conv2d_x3_fwd: weights too large");
    long long img_in_bytes;
    int max_chunk;
    if (int rc = ctdet::conv_check_image(d, who, &img_in_bytes, &max_chunk)) return rc;
    hipStream_t st = ctdet::as_stream(stream);

    for (int b0 = 0; b0 < d->batch; b0 += max_chunk) {
        const int nb = std::min(max_chunk, d->batch - b0);
        X3Args a{};
        ctdet::conv_fill(a, d, b0, nb, img_in_bytes);
        a.wx3 = static_cast<const unsigned char*>(wx3);
        a.w_bytes = (unsigned)wbytes;
        a.M_pad = m_pad;
        a.cgroups = (d->cin + bk - 1) / bk;
        a.KH = d->kh;
        a.KW = d->kw;
        a.nsteps = a.cgroups * d->kh * d->kw;
        a.in_amax = d->in_absmax ? d->in_absmax + (size_t)b0 * ctdet::h2::kLineWords : nullptr;
        a.eW = h2 ? reinterpret_cast<const int*>(static_cast<const unsigned char*>(wx3) + wbytes) + 1 : nullptr;
        a.tiles_m = (d->cout + bm - 1) / bm;
        a.tiles_n = (a.Npix + bn - 1) / bn;
        const ctdet::SplitK sk = ctdet::plan_splitk(d->ksplit, a.tiles_m * a.tiles_n, a.nsteps, (long long)d->cout * a.Npix,
                                                    d->ksplit_ws, d->ksplit_ws_floats, nb == d->batch, 768);
        a.ksplit = sk.ksplit;
        a.steps_per_split = sk.steps_per_split;
        if (sk.ksplit > 1) a.ws = d->ksplit_ws;
        const bool pw = pointwise_flag().load(std::memory_order_relaxed) != 0 && pointwise_rule(d, h2, a.ksplit);
        hipError_t e = pw ? launch_cfg_pw(config, a, st) : launch_cfg(config, a, st);
        if (e != hipSuccess) return ctdet::fail(CT_ERR_HIP, "conv_x3_f32 launch failed: %s", hipGetErrorString(e));
        if (a.ksplit > 1) {
            const int total = a.M * a.Npix;
            hipLaunchKernelGGL(ctdet::conv_splitk_finish<X3Args>, dim3(std::min((total + 255) / 256, 2048)), dim3(256), 0, st, a);
            CT_LAUNCH_CHECK("conv_splitk_finish");
        }
    }
    return CT_OK;
}
