// libctdet: Winograd F(4x4,3x3) as THREE kernels with the transform-domain GEMMs on the bf16 matrix pipe ("bf16x3") --
// the wide 3x3 / stride 1 / dilation 1 / pad 1 layers of the RFBNet-VGG stack (models/RFB_Net_vgg.py:219-227 conv3_x ..
// conv5_x of the VGG trunk, :238-248 the multibox heads on the 38x38 / 19x19 sources).  Same ct_conv_desc contract and
// fused epilogue as ct_conv2d_wino4_fwd, same transforms (ct_wino4_points.h), same fp32 results up to summation order.
//
//   Y = A^T [ sum_c (G g G^T) .* (B^T d B) ] A        per 4x4 output tile, 6x6 input patch d
//
// Why three kernels.  On a SIMD the vector ALU and the matrix pipe do not overlap ("law 1": SIMD time
// = 32 or 64 cycles per MFMA + 4 cycles per wave64 VALU instruction), and a fused Winograd workgroup repeats the input
// transform for every block of 64 output channels: ct_wino4.hip spends 6.7 VALU instructions per fp32 MFMA and stays at
// 0.52 of the pipe, the fused bf16x3 forms of ct_wino_x3.hip 8-11 per bf16 MFMA.  A fused workgroup also owns ALL 36
// transform points of a 32-tile x 64-cout block, which is a bad GEMM shape: 331 KB of operands per 16 channels, more than
// the 64 B/clk a CU pulls through its L1 ("law 2").  Here
//   1. wino4s_in    transforms and splits every (tile, channel) ONCE: V = B^T d B, V = hi + mid + lo (three bfloat16
//                   pieces, exact), written as ready-made MFMA operand fragments -- memory-bound, 13.5 bytes per (output
//                   pixel, input channel);
//   2. wino4s_gemm  36 independent GEMMs  M[xi][cout][tile] = sum_c U[xi][cout][c] V[xi][c][tile]  in 128 x 128 blocks:
//                   both operands arrive in LDS by DMA (buffer_load ... lds, 1 KB per wave instruction, no VGPR staging),
//                   a wave reads twelve 16-byte fragments and issues 24 v_mfma_f32_32x32x16_bf16 (the six piece products
//                   hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid) per 16-channel step -- NO vector-ALU work in the loop;
//   3. wino4s_out   y = A^T M A per (cout, tile) and the usual epilogue (scale / shift, residual, ReLU / floor, fused 2x2
//                   max-pool, NCHW or head scatter) -- memory-bound, 9 bytes per (output pixel, output channel).
// The price is HBM traffic (V and M live in a workspace: 354 + 236 MB for 512 -> 512 @38x38, bs 32), which is why this
// form is for layers with >= 256 channels on maps up to 75 x 75; the fused kernels keep the rest.
#include "ct_common.h"
#include <type_traits>
#include "ct_wino_launch.h"
#include "ct_wgrad_launch.h"
#include "ct_wino_pack.h"
#include "ct_wino4_points.h"
#include "ct_wino4_emit.h"
#include "ct_f16x2.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace {

using ctdet::bf16x8;
using ctdet::f16x8;
using ctdet::f32x4;
using ctdet::f32x16;
using ctdet::i32x4;
using ctdet::kInvalidOff;
using ctdet::kMaxBufBytes;
using ctdet::make_rsrc;
using ctdet::split3;
using ctdet::pack_hi;
typedef float f32x3 __attribute__((ext_vector_type(3)));
typedef int i32x3 __attribute__((ext_vector_type(3)));
constexpr int CC = 16;                      // input channels per k-step (one bf16 MFMA k-group)
constexpr int TB = 32;                      // tiles per transform workgroup = one operand fragment
constexpr int NXI = 36;                     // transform points
constexpr int BM = ctdet::kWino4sBM;        // output channels per GEMM workgroup
constexpr int BT = 128;                     // tiles per GEMM workgroup
constexpr int FRAG = ctdet::kWino4sFragBytes;          // [k half 2][row 32][8 bf16]
constexpr int OPB = ctdet::kWino4sChunkBytes;          // one operand block of a k-step: [sub 4][piece 3][1 KB] = 12 KB
constexpr int NBUF = 3;                     // LDS ring: two k-steps in flight
constexpr int GEMM_LDS_BYTES = NBUF * 2 * OPB;         // 72 KB: two workgroups per CU
constexpr int PT_STRIDE = CC * TB;          // wino4s_in: floats per point in LDS, V[point][channel 16][tile 32]
constexpr int IN_LDS_BYTES = NXI * PT_STRIDE * 4;      // 72 KB
// The f16x2 operand form (variant 3, round 6): two binary16 pieces per value instead of three bfloat16 ones, three piece
// products instead of six (see the section "f16x2" below)
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int HP = 2;                                  // pieces per value
constexpr int OPBH = 4 * HP * FRAG;                    // one operand block of a 16-channel k-group: [sub 4][piece 2][1 KB] = 8 KB
constexpr int LINE_BYTES = ctdet::h2::kLineWords * 4;  // one image's maximum of |input| (CT_ABSMAX_LINE_BYTES)

struct Wino4sArgs {
    const float* in;
    const unsigned short* U;
    const float* scale;
    const float* shift;
    const float* res;
    const float* lo;
    float* out;
    unsigned in_bytes, out_bytes, res_bytes;
    int Cin, H, W, in_ctot, in_coff;
    int M, chunks, kblocks;
    int TY, TX, NT, tblk32, tblk128, Tpad;
    int out_ctot, out_coff, res_ctot, res_coff;
    float res_scale;
    int relu;
    float* pool_out;         // optional fused 2x2 / stride 2 max-pool of the activation (NCHW), else null
    int pool_ctot, pool_coff, pool_oh, pool_ow, write_full;
    int nseg;
    ct_out_segment seg[3];
    unsigned short* V;       // workspace: [point 36][tile block 128][chunk][sub 4][piece 3][1 KB]
    float* Mw;               // workspace: [point 36][cout (kblocks * 128)][tile (Tpad)]
    size_t v_plane, u_plane; // bytes per point
    size_t m_plane;          // floats per point
    int chunks_per_wg;       // wino4s_in: blockIdx.y owns chunks [y * chunks_per_wg, ...)
    int dil;                 // > 1: dilated layer, tiles live on the dil x dil sub-lattices (wino4s_in_dil)
    // f16x2 form only: V is stored scaled by 2^eV, U by 2^eU (powers of two from the operands' maxima, so that no binary16
    // piece overflows and the small pieces keep their bits); wino4s_out multiplies M by 2^-(eU + eV)
    const unsigned* amax;    // per-image maxima of |input| (ct_f16x2.h): the producer's lines (ct_conv_desc.in_absmax) or, after an
                             // absmax pass of its own, the workspace header
    const int* eU;           // the exponent the weight packing chose (trailer of the packed weights)
    unsigned* out_amax;      // any variant: ct_conv_desc.out_absmax (per-image max |y| of what wino4s_out stores), or null
    int batch;               // images of this launch (lines of amax / out_amax)
};

// 36 GEMMs  M[xi][row][col] = sum_k A[xi][row][k] B[xi][col][k], both operands as 12 KB fragment blocks
// [point][block of 128 rows][k chunk of 16][sub 4][piece 3][1 KB] (forward: A = U rows = cout, B = V rows = tiles, k = cin;
// weight gradient: A = E rows = cout, B = V rows = cin, k = tiles).  blockIdx.y = k split: chunks [y * chunks_per_split, ...)
// into slab y of M (forward: one split).
struct GemmArgs {
    const unsigned char* A;
    const unsigned char* B;
    float* M;
    size_t a_plane, b_plane;     // bytes per point
    size_t m_plane, m_slab;      // floats per point / per k split
    int chunks, chunks_per_split, rowblocks, colblocks, ldm;
    int rows, cols;              // live rows (couts) / columns (tiles): 32 x 32 accumulator blocks wholly outside issue no MFMAs
};

using ctdet::w4::bt6;
using ctdet::w4::at4;

// The operand fragments of eight channels of one (point, 32-tile block): bf16x3 = three 16-byte pieces (hi, mid, lo by
// truncation), f16x2 = two (hi, lo by rounding) of the values scaled by vscale = 2^eV.
template <bool H2>
__device__ __forceinline__ void split_store(const float (&raw)[8], unsigned char* dst, float vscale)
{
    if constexpr (H2) {
        i32x4 fb[2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int hi, lo;
            ctdet::h2::split2(raw[2 * q] * vscale, raw[2 * q + 1] * vscale, hi, lo);
            fb[0][q] = hi;
            fb[1][q] = lo;
        }
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) *reinterpret_cast<i32x4*>(dst + pc * FRAG) = fb[pc];
    } else {
        i32x4 fb[3];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned h0, m0, l0, h1, m1, l1;
            split3(raw[2 * q], h0, m0, l0);
            split3(raw[2 * q + 1], h1, m1, l1);
            fb[0][q] = pack_hi(h0, h1);
            fb[1][q] = pack_hi(m0, m1);
            fb[2][q] = pack_hi(l0, l1);
        }
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<i32x4*>(dst + pc * FRAG) = fb[pc];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 1. input transform + split.  Workgroup = (32 tiles, a run of 16-channel chunks), 256 threads.  Per chunk every thread
// loads two 6x6 patches (tile = lane & 31, channels 4 wave + h and 4 wave + 2 + h; twelve 12-byte buffer loads each,
// out-of-map rows / columns read as zero), applies B^T d B in registers and writes the 36 values lane-linearly to LDS
// V[point][channel][tile]; then wave w splits the points 9w .. 9w+8 -- a lane reads its 8 channels of a point, splits
// them into three pieces and stores 16 bytes of each: one 1 KB fragment per (point, piece) and wave instruction.
template <bool H2>
__global__ __launch_bounds__(256, 2) void wino4s_in(const Wino4sArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tblk = blockIdx.x;
    const int tb0 = tblk * TB;
    const int HW = a.H * a.W;
    const int c_begin = blockIdx.y * a.chunks_per_wg, c_end = min(a.chunks, c_begin + a.chunks_per_wg);
    if (c_begin >= c_end) return;
    constexpr int PF = (H2 ? HP : 3) * FRAG, OPBX = 4 * PF;       // bytes of a sub-block's pieces / of a chunk's operand block
    float vscale = 1.f;          // f16x2: 2^eV of the image this lane's tile belongs to (transform role and split role: tile tb0 + l31)

    int voffr[6];
    bool mc[6], lp;
    int hy_delta;
    {
        const int T = tb0 + l31;
        const bool live = T < a.NT;
        const int n = T / (a.TY * a.TX);
        if constexpr (H2) vscale = __builtin_ldexpf(1.f, ctdet::h2::image_exponent(a.amax, live ? n : 0, ctdet::h2::kGrowthBtB));
        const int rem = T - n * (a.TY * a.TX);
        const int ty = rem / a.TX, tx = rem - ty * a.TX;
        const int y0 = 4 * ty - 1, x0 = 4 * tx - 1;
#pragma unroll
        for (int c = 0; c < 6; ++c) mc[c] = (unsigned)(x0 + c) < (unsigned)a.W;
        // a buffer load whose first byte lies before the row is dropped whole, so the left-edge tiles load from x = 0 and
        // shift (their column 0 is padding anyway)
        lp = tx == 0;
        hy_delta = lp ? 8 : 12;
        const long base = (((long)n * a.in_ctot + a.in_coff + h) * a.H + y0) * (long)a.W + x0 + (lp ? 1 : 0);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const bool ok = live && (unsigned)(y0 + i) < (unsigned)a.H;
            voffr[i] = ok ? (int)((base + (long)i * a.W) * 4) : kInvalidOff;
        }
    }
    const __amdgpu_buffer_rsrc_t rin = make_rsrc(a.in, a.in_bytes);
    const int chunk_bytes = CC * HW * 4;
    const int chan_base = 4 * wave * HW * 4;

    struct Half { i32x3 r[6]; };
    auto load_patch = [&](int c, int q, Half& hx, Half& hy) {
        const int soff = c * chunk_bytes + chan_base + q * (2 * HW * 4);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            hx.r[i] = __builtin_amdgcn_raw_buffer_load_b96(rin, voffr[i], soff, 0);
            hy.r[i] = __builtin_amdgcn_raw_buffer_load_b96(rin, voffr[i] == kInvalidOff ? kInvalidOff : voffr[i] + hy_delta, soff, 0);
        }
    };
    float* const vw_base = lds + wave * 128 + lane;          // channel 4 wave + 2 q + h, tile l31
    // (B^T d B in double, rounded once, was measured: error vs fp64 2.0e-6 -> 1.7e-6 on 512 -> 512 @38x38, +6 us -- the
    // remaining error is the accumulation's and the dropped piece products', so the fp32 chain stays)
    auto transform_store = [&](const Half& hx, const Half& hy, int q) {
        float t[6][6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            float d[6], o[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const f32x3 qv = __builtin_bit_cast(f32x3, (c < 3 ? hx : hy).r[i]);
                const float v = c == 1 ? (lp ? qv.x : qv.y) : c == 2 ? (lp ? qv.y : qv.z) : c % 3 == 0 ? qv.x : c % 3 == 1 ? qv.y : qv.z;
                d[i] = mc[c] ? v : 0.f;
            }
            bt6(d, o);
#pragma unroll
            for (int i = 0; i < 6; ++i) t[i][c] = o[i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            float v[6];
            bt6(t[i], v);
            float* vp = vw_base + q * 64 + (i * 6) * PT_STRIDE;
#pragma unroll
            for (int j = 0; j < 6; ++j) vp[j * PT_STRIDE] = v[j];
        }
    };
    const float* const vr_base = lds + (8 * h) * TB + l31;
    // destination of this workgroup's fragments inside a point's plane: (128-tile block, chunk, sub-block, piece)
    unsigned char* const vdst = reinterpret_cast<unsigned char*>(a.V) + (size_t)(tblk >> 2) * a.chunks * OPBX +
                                (tblk & 3) * PF + lane * 16;

    Half x0h, y0h, x1h, y1h;
    load_patch(c_begin, 0, x0h, y0h);
    load_patch(c_begin, 1, x1h, y1h);
    for (int c = c_begin; c < c_end; ++c) {
        transform_store(x0h, y0h, 0);
        transform_store(x1h, y1h, 1);
        if (c + 1 < c_end) {                       // the next chunk's rows are under way while this one is split and stored
            load_patch(c + 1, 0, x0h, y0h);
            load_patch(c + 1, 1, x1h, y1h);
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 9; ++p) {
            const int xi = 9 * wave + p;
            const float* ptr = vr_base + xi * PT_STRIDE;
            float raw[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) raw[e] = ptr[e * TB];
            split_store<H2>(raw, vdst + (size_t)xi * a.v_plane + (size_t)c * OPBX, vscale);
        }
        __syncthreads();
    }
}

// Dilated 3x3 layers (dilation d, pad d: conv6 of models/RFB_Net_vgg.py:226 with d = 6, the RFB branches :38-63,:82-110 with
// d = 2, 3, 5).  Output pixel (y, x) = (sy + d u, sx + d v) only sees input pixels of its own residue class (sy, sx) mod d, and
// on that sub-lattice the layer is an ordinary pad-1 3x3 convolution of a ceil(H / d) x ceil(W / d) image -- so the d x d
// sub-lattices are tiled with F(4x4,3x3) like d x d small images per input image: tile index
//   T = (((n d + sy) d + sx) TY + ty) TX + tx,   TY = ceil(ceil(H / d) / 4),
// patch element (i, j) of a tile = input pixel (sy + d (4 ty - 1 + i), sx + d (4 tx - 1 + j)).  A 19x19 map with d = 6 is 36
// sub-lattices of 4x4 / 3x4 / 3x3 pixels = one tile each: 2.5x fewer multiplications than the direct kernel in spite of the
// 63 % tile fill.  Only the two transform kernels know about it; V, the GEMMs and M are as for d = 1.  Patches are 36 scalar
// loads (stride d), no software prefetch: these layers are small.
template <bool H2>
__global__ __launch_bounds__(256, 2) void wino4s_in_dil(const Wino4sArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tblk = blockIdx.x;
    const int HW = a.H * a.W, d = a.dil;
    const int c_begin = blockIdx.y * a.chunks_per_wg, c_end = min(a.chunks, c_begin + a.chunks_per_wg);
    if (c_begin >= c_end) return;
    constexpr int PF = (H2 ? HP : 3) * FRAG, OPBX = 4 * PF;
    float vscale = 1.f;
    int rowoff[6], coloff[6];
    {
        const int T = tblk * TB + l31;
        const bool live = T < a.NT;
        const int per = a.TY * a.TX;
        int q = T / per;
        const int rem = T - q * per;
        const int ty = rem / a.TX, tx = rem - ty * a.TX;
        const int sx = q % d; q /= d;
        const int sy = q % d;
        const int n = q / d;
        if constexpr (H2) vscale = __builtin_ldexpf(1.f, ctdet::h2::image_exponent(a.amax, live ? n : 0, ctdet::h2::kGrowthBtB));
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int y = sy + d * (4 * ty - 1 + i), x = sx + d * (4 * tx - 1 + i);
            rowoff[i] = (live && (unsigned)y < (unsigned)a.H) ? (int)(((((long)n * a.in_ctot + a.in_coff + h) * a.H + y) * (long)a.W) * 4) : -1;
            coloff[i] = (unsigned)x < (unsigned)a.W ? x * 4 : -1;
        }
    }
    const __amdgpu_buffer_rsrc_t rin = make_rsrc(a.in, a.in_bytes);
    const int chunk_bytes = CC * HW * 4;
    const int chan_base = 4 * wave * HW * 4;
    float* const vw_base = lds + wave * 128 + lane;
    const float* const vr_base = lds + (8 * h) * TB + l31;
    unsigned char* const vdst = reinterpret_cast<unsigned char*>(a.V) + (size_t)(tblk >> 2) * a.chunks * OPBX +
                                (tblk & 3) * PF + lane * 16;
    for (int c = c_begin; c < c_end; ++c) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int soff = c * chunk_bytes + chan_base + q * (2 * HW * 4);
            float t[6][6];
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) {
                float dd[6], o[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const bool ok = rowoff[i] >= 0 && coloff[cc] >= 0;
                    dd[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, ok ? rowoff[i] + coloff[cc] : kInvalidOff, soff, 0));
                }
                bt6(dd, o);
#pragma unroll
                for (int i = 0; i < 6; ++i) t[i][cc] = o[i];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                float v[6];
                bt6(t[i], v);
                float* vp = vw_base + q * 64 + (i * 6) * PT_STRIDE;
#pragma unroll
                for (int j = 0; j < 6; ++j) vp[j * PT_STRIDE] = v[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 9; ++p) {
            const int xi = 9 * wave + p;
            const float* ptr = vr_base + xi * PT_STRIDE;
            float raw[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) raw[e] = ptr[e * TB];
            split_store<H2>(raw, vdst + (size_t)xi * a.v_plane + (size_t)c * OPBX, vscale);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 2. the GEMMs.  Workgroup = one point xi, 128 couts x 128 tiles, 256 threads = 2 x 2 waves of 64 x 64 (four 32x32
// accumulator blocks; DUAL: the hi.hi products in their own accumulator, as ct_conv_x3.hip).  A = U (rows = couts),
// B = V (columns = tiles), so a lane's accumulator registers are 32 consecutive tiles of one cout: M[xi][cout][tile]
// rows, which is the order wino4s_out reads.  Per 16-channel step the workgroup needs 12 KB of each operand, stored in
// HBM exactly as the LDS image: wave w copies sub-block w of both (six 1 KB DMA instructions), three buffers deep.
// Grid: (point, tile block, cout block) with the cout block fastest -- the workgroups that share a V block (the large
// operand) are neighbours -- and every XCD gets a contiguous run of that sequence, so they also share an L2.
template <bool DUAL>
__global__ __launch_bounds__(256, 2) void wino4s_gemm(const GemmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kg = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave & 1, wc = wave >> 1;
    int wg;
    {
        const int nwg = gridDim.x, bid = blockIdx.x;
        const int xcd = bid & 7, local = bid >> 3;
        const int q = nwg >> 3, r = nwg & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
    }
    const int cb = wg % a.rowblocks;
    const int rest = wg / a.rowblocks;
    const int tb = rest % a.colblocks;
    const int xi = rest / a.colblocks;
    const unsigned strip = (unsigned)a.chunks * OPB;
    const int k_begin = blockIdx.y * a.chunks_per_split;
    const int chunks = min(a.chunks, k_begin + a.chunks_per_split) - k_begin;      // steps of this workgroup
    const __amdgpu_buffer_rsrc_t rU = make_rsrc(a.A + (size_t)xi * a.a_plane + (size_t)cb * strip, strip);
    const __amdgpu_buffer_rsrc_t rV = make_rsrc(a.B + (size_t)xi * a.b_plane + (size_t)tb * strip, strip);

    f32x16 acc[2][2], acs[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; acs[i][j][r] = 0.f; }

    typedef __attribute__((address_space(3))) void* lds_ptr;
    const int voff = lane * 16;
    auto load_step = [&](int c, int buf) {
        unsigned char* Ad = lds_raw + buf * (2 * OPB) + wave * (3 * FRAG);
        unsigned char* Bd = Ad + OPB;
        const int soff = (k_begin + c) * OPB + wave * (3 * FRAG);
        (void)Ad; (void)Bd; (void)soff;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rU, (lds_ptr)(Ad + pc * FRAG), 16, voff, soff + pc * FRAG, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rV, (lds_ptr)(Bd + pc * FRAG), 16, voff, soff + pc * FRAG, 0, 0);
        }
#endif
    };
    constexpr int PIECES = 6;                          // DMA instructions per step and wave
    // the six piece products, small ones first: (mid,mid) (lo,hi) (hi,lo) (mid,hi) (hi,mid) (hi,hi)
    constexpr int PA[6] = {1, 2, 0, 1, 0, 0}, PB[6] = {1, 0, 2, 0, 1, 0};
    const unsigned char* const Abase = lds_raw + (2 * wr) * (3 * FRAG) + voff;
    const unsigned char* const Bbase = lds_raw + OPB + (2 * wc) * (3 * FRAG) + voff;
    // Remainder blocks (round 5, VERDICT r04 task 3b): the 156-cout heads fill 28 rows of their second 128-row block and a
    // 19 x 19 map's 800 tiles 32 columns of its seventh 128-column block -- 39 % of head.0/1/2's MFMAs multiplied padding.
    // A wave issues MFMAs only for its 32 x 32 blocks with a live row and column (the DMA, the barriers and the ring are
    // unchanged; a workgroup is as fast as its busiest wave: half the time for the heads' second row block).  The count of
    // live blocks per direction is a compile-time parameter of the pipeline below (four instantiations): run-time tests
    // inside the unrolled MFMA sequence cost the dual-accumulator form 364 spilled registers.
    const int live_r = a.rows - (cb * BM + 64 * wr), live_c = a.cols - (tb * BT + 64 * wc);
    const bool dead = live_r <= 0 || live_c <= 0;
    const bool on[2][2] = {{!dead, !dead && live_c > 32}, {!dead && live_r > 32, live_r > 32 && live_c > 32}};
    auto pipeline = [&](auto ni_c, auto nj_c) {
        constexpr int NI = decltype(ni_c)::value, NJ = decltype(nj_c)::value;
        auto read_frags = [&](int buf, i32x4 (&fa)[2][3], i32x4 (&fb)[2][3]) {
            const unsigned char* A = Abase + buf * (2 * OPB);
            const unsigned char* B = Bbase + buf * (2 * OPB);
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) {
#pragma unroll
                for (int i = 0; i < NI; ++i) fa[i][pc] = *reinterpret_cast<const i32x4*>(A + (i * 3 + pc) * FRAG);
#pragma unroll
                for (int j = 0; j < NJ; ++j) fb[j][pc] = *reinterpret_cast<const i32x4*>(B + (j * 3 + pc) * FRAG);
            }
        };
        auto mfmas = [&](const i32x4 (&fa)[2][3], const i32x4 (&fb)[2][3]) {
            if (NI * NJ == 1 && dead) return;           // a wave wholly outside: DMA and barriers only
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        f32x16& dst = (DUAL && p < 5) ? acs[i][j] : acc[i][j];
                        dst = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i][PA[p]]),
                                                                      __builtin_bit_cast(bf16x8, fb[j][PB[p]]), dst, 0, 0, 0);
                    }
        };
        // Software pipeline over the barrier: the fragments of step c are in registers before its MFMAs start -- they were
        // read from LDS behind the MFMAs of step c - 1.  Top of iteration c: wait for this wave's DMA pieces of step c + 1,
        // barrier (now step c + 1 is complete in LDS, and every wave has finished READING step c: its buffer is free for
        // step c + 3), issue that DMA, issue the twelve fragment reads of step c + 1, then the 24 MFMAs of step c.
        // Ring of three buffers: step c + 1 (being read), c + 2 (in flight), c + 3 (just issued).  (A ring of two with the
        // one-accumulator register budget -- 48 KB, three workgroups per CU -- measured the same: 526 vs 469-531 us on
        // 512 -> 512 @38x38, 3 516-3 526 vs 3 504-3 525 images/s in the pipeline; the kernel is not latency-bound.)
        // Barriers are bare s_barrier instructions with hand-written waits: __syncthreads() carries a workgroup fence that the
        // compiler implements as s_waitcnt vmcnt(0), which would drain the DMA queue (the steps in flight) at every step.
        load_step(0, 0);
        if (chunks > 1) load_step(1, 1);
        if (chunks > 2) load_step(2, 2);
        if (chunks > 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PIECES) : "memory");
        else if (chunks > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        i32x4 fa0[2][3], fb0[2][3], fa1[2][3], fb1[2][3];
        read_frags(0, fa0, fb0);
        auto top = [&](int c) {                             // before the MFMAs of step c; returns after issuing the DMA of step c + 3
            // outstanding DMA groups of this wave, oldest first: steps c + 1, c + 2 (those that exist); lgkmcnt(0): this wave's
            // fragment reads of step c (issued one MFMA phase ago) are done before its buffer is handed back
            if (c + 2 < chunks) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PIECES) : "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (c + 3 < chunks) load_step(c + 3, c % 3);
        };
        int c = 0;
        for (; c + 1 < chunks; c += 2) {
            top(c);
            read_frags((c + 1) % 3, fa1, fb1);
            mfmas(fa0, fb0);
            top(c + 1);
            if (c + 2 < chunks) read_frags((c + 2) % 3, fa0, fb0);
            mfmas(fa1, fb1);
        }
        if (c < chunks) mfmas(fa0, fb0);
    };
    using std::integral_constant;
    if (live_r > 32 && live_c > 32) pipeline(integral_constant<int, 2>{}, integral_constant<int, 2>{});
    else if (live_r > 32) pipeline(integral_constant<int, 2>{}, integral_constant<int, 1>{});
    else if (live_c > 32) pipeline(integral_constant<int, 1>{}, integral_constant<int, 2>{});
    else pipeline(integral_constant<int, 1>{}, integral_constant<int, 1>{});

    // M[xi][cout][tile]: register r of block (i, j) = cout 32 (2 wr + i) + (r & 3) + 8 (r >> 2) + 4 kg, tile 32 (2 wc + j) + l31
    float* const Mp = a.M + (size_t)blockIdx.y * a.m_slab + (size_t)xi * a.m_plane + (size_t)(cb * BM + 64 * wr + 4 * kg) * a.ldm +
                      tb * BT + 64 * wc + l31;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!on[i][j]) continue;                   // nobody reads M outside the live rows / columns
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = DUAL ? acc[i][j][r] + acs[i][j][r] : acc[i][j][r];
                Mp[(size_t)(32 * i + (r & 3) + 8 * (r >> 2)) * a.ldm + 32 * j] = v;
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// f16x2 (round 6; ct_f16x2.h).  Every matrix kernel of this library sits on the same plateau -- the pipe gives ~1.0 PFLOP/s to
// any loop that also moves its operands ("law 3") -- so the lever left is FEWER matrix instructions per
// multiply-add.  Two binary16 pieces per value and three piece products (hi.hi, hi.lo, lo.hi) carry the same 22-24 bits as
// three bfloat16 pieces and six products: half the MFMAs, two thirds of the V / U bytes, 2 instead of 5.5 VALU instructions
// per split value in wino4s_in, same error against fp64 (tests/test_gpu_wino.py::test_wino_rounding_error_vs_fp64).
//   0. absmax_lines_kernel  max |x| of every image's input slice -> the workspace header (when the producer of the input did not
//                     leave the maxima: ct_conv_desc.in_absmax);
//   1. wino4s_in<true>   V 2^eV as two pieces, eV PER IMAGE from that maximum (no hi piece above 2^15, ct_f16x2.h);
//   2. wino4h_gemm       below: the bf16x3 pipeline with 8 KB operand blocks per 16-channel k-group, KG groups per barrier;
//   3. wino4s_out<true>  M 2^-(eU + eV[image]), then as before.
// Operand blocks: [point][block of 128 rows][k-group of 16][sub 4][piece 2][k half 2][row 32][8 f16].

// max |x| over the [per_image] floats of every image's channel slice, folded into the image's line (atomic max, one per wave and
// item of 4096 floats; the caller zeroes the lines): ct_absmax_f32 and the absmax pass of ct_conv2d_wino4s_fwd variant 3
__global__ __launch_bounds__(256) void absmax_lines_kernel(const float* __restrict__ in, int batch, long per_image, long img_stride,
                                                           int vec_ok, unsigned* __restrict__ lines)
{
    const int ipi = (int)((per_image + 4095) / 4096);
    const long nitems = (long)batch * ipi;
    for (long it = blockIdx.x; it < nitems; it += gridDim.x) {
        const int n = (int)(it / ipi), sgm = (int)(it - (long)n * ipi);
        const float* base = in + (size_t)n * img_stride;
        const long e0 = (long)sgm * 4096;
        unsigned m = 0;
        for (int r = 0; r < (vec_ok ? 4 : 16); ++r) {
            const long e = vec_ok ? e0 + (long)(r * 256 + threadIdx.x) * 4 : e0 + r * 256 + threadIdx.x;
            if (e >= per_image) continue;
            if (vec_ok && e + 3 < per_image) {
                const i32x4 v = *reinterpret_cast<const i32x4*>(base + e);
                const unsigned a0 = (unsigned)v.x & 0x7FFFFFFFu, a1 = (unsigned)v.y & 0x7FFFFFFFu;
                const unsigned a2 = (unsigned)v.z & 0x7FFFFFFFu, a3 = (unsigned)v.w & 0x7FFFFFFFu;
                const unsigned b0 = a0 > a1 ? a0 : a1, b1 = a2 > a3 ? a2 : a3, b = b0 > b1 ? b0 : b1;
                m = b > m ? b : m;
            } else {
                for (int t = 0; t < (vec_ok ? 4 : 1); ++t)
                    if (e + t < per_image) {
                        const unsigned a0 = __builtin_bit_cast(unsigned, base[e + t]) & 0x7FFFFFFFu;
                        m = a0 > m ? a0 : m;
                    }
            }
        }
        m = ctdet::h2::wave_max(m);
        if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(lines + (size_t)n * ctdet::h2::kLineWords, m);
    }
}

// Workgroup = one point xi, 128 couts x 128 tiles, 2 x 2 waves of 64 x 64, as wino4s_gemm.  A step = KG k-groups of 16 channels
// (KG x 16 KB in LDS: [group][A 8 KB][B 8 KB]), ring of NB steps.  The pipeline runs over k-GROUPS: the fragments of group q + 1
// are read behind the MFMAs of group q; where q + 1 opens a new step the wave first waits for its DMA pieces of that step and
// its own reads of the step just finished, then the barrier (the finished step's buffer is free: the DMA of step + NB goes
// there).  DUAL: the hi.hi products in their own accumulator (the two small products, <= 2^-11 of them, in the other).
template <bool DUAL, int KG, int NB>
__global__ __launch_bounds__(256, 2) void wino4h_gemm(const GemmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kg = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave & 1, wc = wave >> 1;
    int wg;
    {
        const int nwg = gridDim.x, bid = blockIdx.x;
        const int xcd = bid & 7, local = bid >> 3;
        const int q = nwg >> 3, r = nwg & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
    }
    const int cb = wg % a.rowblocks;
    const int rest = wg / a.rowblocks;
    const int tb = rest % a.colblocks;
    const int xi = rest / a.colblocks;
    const unsigned strip = (unsigned)a.chunks * OPBH;
    const int groups = a.chunks;                       // forward only: one k split
    const int steps = groups / KG;                     // the host picks KG = 1 when groups is odd
    const __amdgpu_buffer_rsrc_t rU = make_rsrc(a.A + (size_t)xi * a.a_plane + (size_t)cb * strip, strip);
    const __amdgpu_buffer_rsrc_t rV = make_rsrc(a.B + (size_t)xi * a.b_plane + (size_t)tb * strip, strip);

    f32x16 acc[2][2], acs[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; acs[i][j][r] = 0.f; }

    typedef __attribute__((address_space(3))) void* lds_ptr;
    const int voff = lane * 16;
    constexpr int GB = 2 * OPBH;                       // LDS bytes of one k-group: A block, B block
    constexpr int SB = KG * GB;                        // ... of one step
    constexpr int PIECES = KG * 2 * HP;                // DMA instructions per step and wave
    auto load_step = [&](int st, int buf) {
#pragma unroll
        for (int g = 0; g < KG; ++g) {
            unsigned char* Ad = lds_raw + buf * SB + g * GB + wave * (HP * FRAG);
            unsigned char* Bd = Ad + OPBH;
            const int soff = (st * KG + g) * OPBH + wave * (HP * FRAG);
            (void)Ad; (void)Bd; (void)soff;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
            for (int pc = 0; pc < HP; ++pc) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rU, (lds_ptr)(Ad + pc * FRAG), 16, voff, soff + pc * FRAG, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rV, (lds_ptr)(Bd + pc * FRAG), 16, voff, soff + pc * FRAG, 0, 0);
            }
#endif
        }
    };
    const unsigned char* const Abase = lds_raw + (2 * wr) * (HP * FRAG) + voff;
    const unsigned char* const Bbase = lds_raw + OPBH + (2 * wc) * (HP * FRAG) + voff;
    const int live_r = a.rows - (cb * BM + 64 * wr), live_c = a.cols - (tb * BT + 64 * wc);
    const bool dead = live_r <= 0 || live_c <= 0;
    const bool on[2][2] = {{!dead, !dead && live_c > 32}, {!dead && live_r > 32, live_r > 32 && live_c > 32}};
    auto pipeline = [&](auto ni_c, auto nj_c) {
        constexpr int NI = decltype(ni_c)::value, NJ = decltype(nj_c)::value;
        auto read_frags = [&](int q, i32x4 (&fa)[2][HP], i32x4 (&fb)[2][HP]) {
            const int off = ((q / KG) % NB) * SB + (q % KG) * GB;
            const unsigned char* A = Abase + off;
            const unsigned char* B = Bbase + off;
#pragma unroll
            for (int pc = 0; pc < HP; ++pc) {
#pragma unroll
                for (int i = 0; i < NI; ++i) fa[i][pc] = *reinterpret_cast<const i32x4*>(A + (i * HP + pc) * FRAG);
#pragma unroll
                for (int j = 0; j < NJ; ++j) fb[j][pc] = *reinterpret_cast<const i32x4*>(B + (j * HP + pc) * FRAG);
            }
        };
        // the three piece products, small ones first: (lo, hi) (hi, lo) (hi, hi)   [A piece, B piece]
        constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
        auto mfmas = [&](const i32x4 (&fa)[2][HP], const i32x4 (&fb)[2][HP]) {
            if (NI * NJ == 1 && dead) return;
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        f32x16& dst = (DUAL && p < 2) ? acs[i][j] : acc[i][j];
                        dst = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[i][PA[p]]),
                                                                     __builtin_bit_cast(f16x8, fb[j][PB[p]]), dst, 0, 0, 0);
                    }
        };
        const int pre = steps < NB ? steps : NB;
        for (int st = 0; st < pre; ++st) load_step(st, st);
        // wait for step 0: the pre - 1 later steps may stay in flight
        if (pre >= 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * PIECES > 63 ? 63 : 3 * PIECES) : "memory");
        else if (pre == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PIECES) : "memory");
        else if (pre == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        i32x4 fa0[2][HP], fb0[2][HP], fa1[2][HP], fb1[2][HP];
        read_frags(0, fa0, fb0);
        // before the MFMAs of group q: make group q + 1 readable
        auto top = [&](int q) {
            if ((q + 1) % KG != 0) return;                 // same step: its buffer is complete since the step was opened
            const int s1 = (q + 1) / KG;                   // the step being opened; step s1 - 1 has been read by this wave
            if (s1 < steps) {
                // DMA groups of this wave issued after step s1: steps s1 + 1 .. min(steps - 1, s1 - 2 + NB)
                const int later = min(steps - 1 - s1, NB - 2);
                if (later >= 3) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(3 * PIECES > 63 ? 63 : 3 * PIECES) : "memory");
                else if (later == 2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * PIECES) : "memory");
                else if (later == 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PIECES) : "memory");
                else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if (s1 - 1 + NB < steps) load_step(s1 - 1 + NB, (s1 - 1) % NB);
            }
        };
        int q = 0;
        for (; q + 1 < groups; q += 2) {
            top(q);
            read_frags(q + 1, fa1, fb1);
            mfmas(fa0, fb0);
            top(q + 1);
            if (q + 2 < groups) read_frags(q + 2, fa0, fb0);
            mfmas(fa1, fb1);
        }
        if (q < groups) mfmas(fa0, fb0);
    };
    using std::integral_constant;
    if (live_r > 32 && live_c > 32) pipeline(integral_constant<int, 2>{}, integral_constant<int, 2>{});
    else if (live_r > 32) pipeline(integral_constant<int, 2>{}, integral_constant<int, 1>{});
    else if (live_c > 32) pipeline(integral_constant<int, 1>{}, integral_constant<int, 2>{});
    else pipeline(integral_constant<int, 1>{}, integral_constant<int, 1>{});

    float* const Mp = a.M + (size_t)xi * a.m_plane + (size_t)(cb * BM + 64 * wr + 4 * kg) * a.ldm + tb * BT + 64 * wc + l31;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!on[i][j]) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = DUAL ? acc[i][j][r] + acs[i][j][r] : acc[i][j][r];
                Mp[(size_t)(32 * i + (r & 3) + 8 * (r >> 2)) * a.ldm + 32 * j] = v;
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// 3. output transform + epilogue.  Thread = one (cout, tile): 36 coalesced loads (lanes = 64 consecutive tiles of a
// cout row), y = A^T M A, the epilogue of ct_wino4.hip.
template <bool H2>
__device__ __forceinline__ void wino4s_out_one(const Wino4sArgs& a, int T, int co, bool track, float& amax_run, int& img);

template <bool H2>
__global__ __launch_bounds__(256) void wino4s_out(const Wino4sArgs a)
{
    const int T = blockIdx.x * 64 + (threadIdx.x & 63);
    const int co = blockIdx.y * 4 + (threadIdx.x >> 6);
    float amax_run = 0.f;            // max |y| of what this thread stores (a.out_amax)
    int img = -1;                    // ... and the image it belongs to
    if (T < a.NT && co < a.M) wino4s_out_one<H2>(a, T, co, a.out_amax != nullptr, amax_run, img);
    // every lane of the wave arrives here (no early exit above): one atomic per image present in the wave
    if (a.out_amax) ctdet::h2::flush_absmax(a.out_amax, img, amax_run);
}

template <bool H2>
__device__ __forceinline__ void wino4s_out_one(const Wino4sArgs& a, const int T, const int co, const bool track, float& amax_run, int& img)
{
    const float* src = a.Mw + (size_t)co * a.Tpad + T;
    float m[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) m[i][j] = __builtin_nontemporal_load(src + (size_t)(i * 6 + j) * a.m_plane);
    // f16x2: the operands were scaled by 2^eU, 2^eV[image] (exact powers of two); folded into the per-channel scale of the epilogue
    ctdet::h2::pow2x2 ymul{1.f, 1.f};      // f16x2: 2^-(eU + eV[image]) as two exact factors (h2::unscale_for)
    // A^T M A in double, rounded once: this kernel waits for HBM, the fp32 chain of ct_wino4.hip rounds ~10 times per output
    double t[6][4];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double row[6] = {m[i][0], m[i][1], m[i][2], m[i][3], m[i][4], m[i][5]};
        ctdet::w4::at4d(row, t[i]);
    }
    float y[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const double col[6] = {t[0][b], t[1][b], t[2][b], t[3][b], t[4][b], t[5][b]};
        double o[4];
        ctdet::w4::at4d(col, o);
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r][b] = (float)o[r];
    }
    if (a.dil > 1) {
        // dilated layer (see wino4s_in_dil): the 4x4 outputs of a tile are d pixels apart; scale / shift and the floor only
        // (the dilated layers of this network have no residual, pooling or head scatter)
        const int d = a.dil, per = a.TY * a.TX;
        int q = T / per;
        const int rem = T - q * per;
        const int ty = rem / a.TX, tx = rem - ty * a.TX;
        const int sx = q % d; q /= d;
        const int sy = q % d;
        const int n = q / d;
        img = n;
        if constexpr (H2) ymul = ctdet::h2::unscale_for(*a.eU, ctdet::h2::image_exponent(a.amax, n, ctdet::h2::kGrowthBtB));
        const float sc = a.scale[co] * ymul.hi, sh = a.shift[co];
        const float lo = a.lo ? a.lo[co] : (a.relu ? 0.f : -INFINITY);
        float* const plane = a.out + ((size_t)n * a.out_ctot + a.out_coff + co) * a.H * a.W;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int yy = sy + d * (4 * ty + r);
            if (yy >= a.H) continue;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int xx = sx + d * (4 * tx + c);
                if (xx >= a.W) continue;
                float v = (y[r][c] * ymul.lo) * sc + sh;
                v = v < lo ? lo : v;
                plane[(size_t)yy * a.W + xx] = v;
                if (track) ctdet::h2::track_absmax(amax_run, v);
            }
        }
        return;
    }
    const int n = T / (a.TY * a.TX);
    img = n;
    if constexpr (H2) ymul = ctdet::h2::unscale_for(*a.eU, ctdet::h2::image_exponent(a.amax, n, ctdet::h2::kGrowthBtB));
    const int rem = T - n * (a.TY * a.TX);
    const int ty = rem / a.TX, tx = rem - ty * a.TX;
    const __amdgpu_buffer_rsrc_t rout = make_rsrc(a.out, a.out_bytes);
    const __amdgpu_buffer_rsrc_t rres = make_rsrc(a.res, a.res_bytes);
    ctdet::w4::emit_tile4(a, rout, rres, n, ty, tx, co, y, ymul.lo, ymul.hi, track, amax_run);
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient in the same form:  dw = G^T [ sum_tiles (A e A^T) .* (B^T d B) ] G  with 4x4 tiles e of dZ and 6x6 input
// patches d (F(3x3,4x4), the arithmetic of ct_wino4_wgrad.hip) is, per transform point, the GEMM
//   dU[xi][cout][cin] = sum_t E[xi][cout][t] V[xi][cin][t]
// with the TILE index as k.  wino4s_tk writes either operand -- IS_E: E = A e A^T from dZ, else V = B^T d B from the layer's
// input -- split into three bfloat16 pieces, as fragments [point][block of 128 channels][chunk of 16 tiles][sub 4][piece 3]
// [k half 2][channel 32][8 tiles]; wino4s_gemm (k split over blockIdx.y, one slab of dU per split) is the forward kernel;
// wino4s_wgrad_finish adds the slabs in order and applies G^T . G.
constexpr int TK_CH_STRIDE = TB + 1;                          // LDS: V[point][channel 16][33]: conflict-free writes, 2-way reads
constexpr int TK_PT_STRIDE = CC * TK_CH_STRIDE;
constexpr int TK_LDS_BYTES = NXI * TK_PT_STRIDE * 4;          // 76 KB

struct TkArgs {
    const float* src;        // NCHW, channel slice [coff, coff + C) of a buffer with ctot channels
    unsigned src_bytes;
    int C, H, W, ctot, coff;
    int TY, TX, NT, tblk32, kchunks;       // kchunks = 2 * tblk32 (16 tiles each)
    int chunks;              // channel chunks of 16 (C rounded up)
    int chunks_per_wg;
    unsigned char* dst;
    size_t plane;            // bytes per point
    int dil;                 // > 1: tiles on the dil x dil sub-lattices (see wino4s_in_dil)
};

template <bool IS_E>
__global__ __launch_bounds__(256, 2) void wino4s_tk(const TkArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tblk = blockIdx.x;
    const int HW = a.H * a.W;
    const int c_begin = blockIdx.y * a.chunks_per_wg, c_end = min(a.chunks, c_begin + a.chunks_per_wg);
    if (c_begin >= c_end) return;
    constexpr int NR = IS_E ? 4 : 6;                 // rows / columns of the spatial block a thread loads
    int voffr[NR];
    bool mc[NR], lp = false;
    int coloff[NR];                                  // dilated layers: byte offset of column j inside a row, -1 = outside
    const bool dilated = a.dil > 1;
    {
        const int T = tblk * TB + l31;
        const bool live = T < a.NT;
        const int per = a.TY * a.TX, d = a.dil;
        int q = T / per;
        const int rem = T - q * per;
        const int ty = rem / a.TX, tx = rem - ty * a.TX;
        const int sx = q % d; q /= d;                // d = 1: sx = sy = 0, q = image
        const int sy = q % d;
        const int n = q / d;
        const int u0 = 4 * ty - (IS_E ? 0 : 1), v0 = 4 * tx - (IS_E ? 0 : 1);
#pragma unroll
        for (int c = 0; c < NR; ++c) {
            const int x = sx + d * (v0 + c);
            mc[c] = (unsigned)x < (unsigned)a.W;
            coloff[c] = mc[c] ? x * 4 : -1;
        }
        if (!IS_E && !dilated) lp = tx == 0;         // see wino4s_in: left-edge patches load from x = 0 and shift
        const long plane0 = ((long)n * a.ctot + a.coff + h) * a.H;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int y = sy + d * (u0 + i);
            const bool ok = live && (unsigned)y < (unsigned)a.H;
            // d = 1: offset of the first loaded column (vector loads); dilated: offset of the row start (scalar loads)
            const long first = dilated ? 0 : (long)(v0 + (lp ? 1 : 0));
            voffr[i] = ok ? (int)(((plane0 + y) * (long)a.W + first) * 4) : kInvalidOff;
        }
    }
    const int hy_delta = lp ? 8 : 12;
    const __amdgpu_buffer_rsrc_t rin = make_rsrc(a.src, a.src_bytes);
    const int chunk_bytes = CC * HW * 4;
    const int chan_base = 4 * wave * HW * 4;
    float* const vw_base = lds + (4 * wave + h) * TK_CH_STRIDE + l31;      // channel 4 wave + 2 q + h, tile l31
    // pack stage: lane = (k chunk kc of the two 16-tile chunks, k half kh, channel rr): 8 consecutive tiles of one channel
    const int kc = lane >> 5, kh = (lane >> 4) & 1, rr = lane & 15;
    const float* const vr_base = lds + rr * TK_CH_STRIDE + kc * 16 + kh * 8;

    for (int c = c_begin; c < c_end; ++c) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ch = c * CC + 4 * wave + 2 * q + h;
            const bool chok = ch < a.C;
            const int soff = c * chunk_bytes + chan_base + q * (2 * HW * 4);
            float t[6][NR];
            if constexpr (IS_E) {
                float e[4][4];
                if (dilated) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const bool ok = chok && voffr[i] != kInvalidOff && coloff[j] >= 0;
                            e[i][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, ok ? voffr[i] + coloff[j] : kInvalidOff, soff, 0));
                        }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const i32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rin, chok ? voffr[i] : kInvalidOff, soff, 0);
                        const f32x4 q4 = __builtin_bit_cast(f32x4, r);
                        e[i][0] = q4.x;
                        e[i][1] = mc[1] ? q4.y : 0.f;
                        e[i][2] = mc[2] ? q4.z : 0.f;
                        e[i][3] = mc[3] ? q4.w : 0.f;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float col[4] = {e[0][j], e[1][j], e[2][j], e[3][j]};
                    float o[6];
                    ctdet::w4::a6(col, o);
#pragma unroll
                    for (int i = 0; i < 6; ++i) t[i][j] = o[i];
                }
            } else {
                if (dilated) {
#pragma unroll
                    for (int cc = 0; cc < 6; ++cc) {
                        float d[6], o[6];
#pragma unroll
                        for (int i = 0; i < 6; ++i) {
                            const bool ok = chok && voffr[i] != kInvalidOff && coloff[cc] >= 0;
                            d[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, ok ? voffr[i] + coloff[cc] : kInvalidOff, soff, 0));
                        }
                        bt6(d, o);
#pragma unroll
                        for (int i = 0; i < 6; ++i) t[i][cc] = o[i];
                    }
                } else {
                    i32x3 hx[6], hy[6];
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        const int vo = chok ? voffr[i] : kInvalidOff;
                        hx[i] = __builtin_amdgcn_raw_buffer_load_b96(rin, vo, soff, 0);
                        hy[i] = __builtin_amdgcn_raw_buffer_load_b96(rin, vo == kInvalidOff ? kInvalidOff : vo + hy_delta, soff, 0);
                    }
#pragma unroll
                    for (int cc = 0; cc < 6; ++cc) {
                        float d[6], o[6];
#pragma unroll
                        for (int i = 0; i < 6; ++i) {
                            const f32x3 qv = __builtin_bit_cast(f32x3, cc < 3 ? hx[i] : hy[i]);
                            const float v = cc == 1 ? (lp ? qv.x : qv.y) : cc == 2 ? (lp ? qv.y : qv.z) : cc % 3 == 0 ? qv.x : cc % 3 == 1 ? qv.y : qv.z;
                            d[i] = mc[cc] ? v : 0.f;
                        }
                        bt6(d, o);
#pragma unroll
                        for (int i = 0; i < 6; ++i) t[i][cc] = o[i];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                float v[6];
                if constexpr (IS_E) {
                    const float row[4] = {t[i][0], t[i][1], t[i][2], t[i][3]};
                    ctdet::w4::a6(row, v);
                } else {
                    const float row[6] = {t[i][0], t[i][1], t[i][2], t[i][3], t[i][4], t[i][5]};
                    bt6(row, v);
                }
                float* vp = vw_base + q * (2 * TK_CH_STRIDE) + (i * 6) * TK_PT_STRIDE;
#pragma unroll
                for (int j = 0; j < 6; ++j) vp[j * TK_PT_STRIDE] = v[j];
            }
        }
        __syncthreads();
        // rows c * 16 .. + 15 of the operand: 128-row block c >> 3, 32-row sub-block (c >> 1) & 3, upper / lower half c & 1
        unsigned char* const dst0 = a.dst + ((size_t)(c >> 3) * a.kchunks + 2 * tblk + kc) * OPB + ((c >> 1) & 3) * (3 * FRAG) +
                                    (kh * 32 + (c & 1) * 16 + rr) * 16;
#pragma unroll
        for (int p = 0; p < 9; ++p) {
            const int xi = 9 * wave + p;
            const float* ptr = vr_base + xi * TK_PT_STRIDE;
            float raw[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) raw[e] = ptr[e];
            i32x4 fb[3];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                unsigned h0, m0, l0, h1, m1, l1;
                split3(raw[2 * q], h0, m0, l0);
                split3(raw[2 * q + 1], h1, m1, l1);
                fb[0][q] = pack_hi(h0, h1);
                fb[1][q] = pack_hi(m0, m1);
                fb[2][q] = pack_hi(l0, l1);
            }
            unsigned char* dst = dst0 + (size_t)xi * a.plane;
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<i32x4*>(dst + pc * FRAG) = fb[pc];
        }
        __syncthreads();
    }
}

// dw[k][c][3][3] = G^T (sum over slabs of dU[.][k][c]) G; slabs added in order (no atomics: results do not depend on timing)
__global__ __launch_bounds__(256) void wino4s_wgrad_finish(const float* __restrict__ dU, float* __restrict__ dw, int Cout, int Cin,
                                                           int ld, size_t plane, size_t slab, int slabs)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Cout * Cin) return;
    const int k = i / Cin, c = i - k * Cin;
    const float* src = dU + (size_t)k * ld + c;
    float w[3][6];
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        float u[6], o[3];
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            float sum = src[(size_t)(m * 6 + n) * plane];
            for (int sl = 1; sl < slabs; ++sl) sum += src[(size_t)sl * slab + (size_t)(m * 6 + n) * plane];
            u[m] = sum;
        }
        ctdet::w4::gt3(u, o);
#pragma unroll
        for (int m = 0; m < 3; ++m) w[m][n] = o[m];
    }
    float* out = dw + (size_t)i * 9;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        float o[3];
        ctdet::w4::gt3(w[m], o);
        out[m * 3 + 0] = o[0];
        out[m * 3 + 1] = o[1];
        out[m * 3 + 2] = o[2];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// f16x2 weights: U = G g G^T in double (as the bf16x3 packing), times 2^eU, as two binary16 pieces in the GEMM operand order
// [point 36][cout block of 128][k-group 16 ch][sub 4][piece 2][k half 2][row 32][8 f16]; eU from max |g| over the layer
// (wino4h_wmax, one atomic per wave into the trailer behind the packed weights; the packing kernel records eU there).
__device__ __forceinline__ void wino4h_wmax_body(const ctdet::WinoPackArgs& p, unsigned* trailer, int bx, int gx)
{
    unsigned m = 0;
    for (int part = 0; part < p.nparts; ++part) {
        const long n = (long)(p.mbeg[part + 1] - p.mbeg[part]) * p.cin_fwd * 9;
        const float* w = p.w[part];
        for (long i = bx * 256L + threadIdx.x; i < n; i += gx * 256L) {
            const unsigned a = __builtin_bit_cast(unsigned, w[i]) & 0x7FFFFFFFu;
            m = a > m ? a : m;
        }
    }
    m = ctdet::h2::wave_max(m);
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(trailer, m);
}

__global__ __launch_bounds__(256) void wino4h_wmax(const ctdet::WinoPackArgs p, unsigned* trailer)
{
    wino4h_wmax_body(p, trailer, blockIdx.x, gridDim.x);
}

// one thread = one (cout, 8 consecutive input channels, transform row i): six 16-byte stores per piece
__device__ __forceinline__ void wino4h_pack_body(const ctdet::WinoPackArgs& p, unsigned* trailer, int bx, int gx)
{
    const int eU = ctdet::h2::exponent_for(trailer[0], ctdet::h2::kGrowthGG);
    if (bx == 0 && threadIdx.x == 0) trailer[1] = (unsigned)eU;
    const bool fused = p.tile == 48;                   // ct_wino4f.hip's unit order (64-cout blocks) instead of the GEMM operand's
    const int rows = p.kblocks * (fused ? ctdet::kWinoKB : BM);
    const int groups8 = p.cin / 8;
    const long total = (long)rows * groups8 * 6;
    unsigned char* const out = reinterpret_cast<unsigned char*>(p.U);
    const size_t plane = (size_t)p.kblocks * p.chunks * OPBH;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    for (long idx = bx * 256L + threadIdx.x; idx < total; idx += gx * 256L) {
        const int co = (int)(idx % rows);
        const long rest = idx / rows;
        const int ci8 = (int)(rest % groups8);
        const int i = (int)(rest / groups8);
        u32x4 v[6][2];
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) v[j][pc] = u32x4{0u, 0u, 0u, 0u};
        if (co < p.cout) {
            // the 8 x 9 taps of this thread.  Forward layout: 72 consecutive floats of one filter row (288 bytes: eighteen 16-byte
            // loads where the parameter is 16-byte aligned -- scalar loads of a wave whose lanes are cin * 36 bytes apart made this
            // kernel 0.7 ms of a training step); data gradient: 8 forward couts, cin_fwd * 36 bytes apart, taps rotated by 180 degrees
            float g[8][9];
            if (!p.dgrad) {
                const float* w = ctdet::wino_taps(p, co, ci8 * 8);
                if ((reinterpret_cast<uintptr_t>(w) & 15) == 0) {
#pragma unroll
                    for (int q4 = 0; q4 < 18; ++q4) {
                        const float4 f = reinterpret_cast<const float4*>(w)[q4];
                        (&g[0][0])[4 * q4 + 0] = f.x; (&g[0][0])[4 * q4 + 1] = f.y; (&g[0][0])[4 * q4 + 2] = f.z; (&g[0][0])[4 * q4 + 3] = f.w;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 72; ++k) (&g[0][0])[k] = w[k];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float* w = ctdet::wino_taps(p, co, ci8 * 8 + e);
#pragma unroll
                    for (int k = 0; k < 9; ++k) g[e][k] = w[8 - k];
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                double t[3];                                      // row i of G g
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    // (all six rows and a select, not the one row needed: the packed bits of rounds 1-6 -- and with them the last
                    // digits of every committed parity measurement -- come from THIS expression tree as the compiler contracts it)
                    double o[6];
                    ctdet::w4::gmul6(g[e][0 * 3 + c], g[e][1 * 3 + c], g[e][2 * 3 + c], o);
                    t[c] = ctdet::wino_pick6(o, i);
                }
                double o[6];                                      // (G g) G^T, row i
                ctdet::w4::gmul6(t[0], t[1], t[2], o);
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const double us = __builtin_ldexp(o[j], eU);
                    const _Float16 hi = (_Float16)(float)us;
                    const _Float16 lo = (_Float16)(float)(us - (double)(float)hi);
                    const int sh = 16 * (e & 1);                  // even channel: low half-word
                    v[j][0][e >> 1] |= (unsigned)__builtin_bit_cast(unsigned short, hi) << sh;
                    v[j][1][e >> 1] |= (unsigned)__builtin_bit_cast(unsigned short, lo) << sh;
                }
            }
        }
        const int chunk = ci8 >> 1, kh = ci8 & 1;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int xi = i * 6 + j;
            unsigned char* q;
            if (fused) {
                const int kb = co / ctdet::kWinoKB, half = (co % ctdet::kWinoKB) / 32;
                const int wv = xi < 32 ? xi >> 2 : 2 * (xi - 32) + half;
                const int unit = xi < 32 ? 2 * (xi & 3) + half : 8;
                q = out + ((size_t)kb * p.chunks + chunk) * ctdet::kWino4fhChunkBytes + (size_t)wv * ctdet::kWino4fhWaveBytes +
                    unit * ctdet::kWino4fhUnitBytes + (co % 32 + 32 * kh) * 16;
            } else {
                const int cb = co / BM, sub = (co % BM) / 32;
                q = out + (size_t)xi * plane + ((((size_t)cb * p.chunks + chunk) * 4 + sub) * HP) * FRAG + (kh * 32 + co % 32) * 16;
            }
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) *reinterpret_cast<u32x4*>(q + pc * FRAG) = v[j][pc];
        }
    }
}

__global__ __launch_bounds__(256) void wino4h_pack(const ctdet::WinoPackArgs p, unsigned* trailer)
{
    wino4h_pack_body(p, trailer, blockIdx.x, gridDim.x);
}

// The same three steps for a LIST of layers (the training engine re-packs every f16x2 layer once per optimizer step: one launch per
// step instead of three per layer).  blockIdx.y = item; items read by reference from device memory (a by-value copy would put the
// w[] / mbeg[] arrays, indexed by a run-time part number, into scratch).
struct WinoH2Item {
    ctdet::WinoPackArgs p;
    unsigned* trailer;
};

__global__ __launch_bounds__(64) void wino4h_trailer_zero_list(const WinoH2Item* items, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) { items[i].trailer[0] = 0u; items[i].trailer[1] = 0u; }
}

__global__ __launch_bounds__(256) void wino4h_wmax_list(const WinoH2Item* items)
{
    const WinoH2Item& it = items[blockIdx.y];
    wino4h_wmax_body(it.p, it.trailer, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void wino4h_pack_list(const WinoH2Item* items)
{
    const WinoH2Item& it = items[blockIdx.y];
    wino4h_pack_body(it.p, it.trailer, blockIdx.x, gridDim.x);
}

struct WgSizes { int TY, TX, NT, tblk32, kchunks, rb, cb, splits, cps; size_t e_plane, v_plane, m_plane, m_slab, e_bytes, v_bytes, m_bytes; };

WgSizes wg_sizes_of(int batch, int oh, int ow, int cin, int cout, int dil)
{
    WgSizes s{};
    s.TY = ((oh + dil - 1) / dil + 3) / 4; s.TX = ((ow + dil - 1) / dil + 3) / 4;      // per sub-lattice (dil = 1: the map)
    s.NT = batch * dil * dil * s.TY * s.TX;
    s.tblk32 = (s.NT + TB - 1) / TB;
    s.kchunks = 2 * s.tblk32;
    s.rb = (cout + BM - 1) / BM;
    s.cb = (cin + BT - 1) / BT;
    // k splits: about three rounds of two workgroups per CU, at least 8 k-steps each
    const int wgs = NXI * s.rb * s.cb;
    const ctdet::Split sp = ctdet::even_split(s.kchunks, std::max(1, std::min((1536 + wgs - 1) / wgs, s.kchunks / 8)));
    s.splits = sp.splits;
    s.cps = sp.per_split;
    s.e_plane = (size_t)s.rb * s.kchunks * OPB;
    s.v_plane = (size_t)s.cb * s.kchunks * OPB;
    s.m_plane = (size_t)s.rb * BM * s.cb * BT;
    s.m_slab = s.m_plane * NXI;
    s.e_bytes = ctdet::align_up(s.e_plane * NXI, 256);
    s.v_bytes = ctdet::align_up(s.v_plane * NXI, 256);
    s.m_bytes = s.m_slab * s.splits * 4;
    return s;
}

bool wino4s_wg_ok(const ct_conv_desc* d)
{
    return d->kh == 3 && d->kw == 3 && d->stride == 1 && d->dil >= 1 && d->dil <= 8 && d->pad_h == d->dil && d->pad_w == d->dil &&
           d->oh == d->h && d->ow == d->w && !d->transposed && d->cin >= 16 && d->cin % CC == 0 && d->cout >= 1 &&
           // one launch covers the batch (no chunking): both tensors must stay below 2 GiB as a whole
           (long long)std::max(d->batch, 1) * d->in_ctot * d->h * d->w * 4 < kMaxBufBytes &&
           (long long)std::max(d->batch, 1) * d->cout * d->oh * d->ow * 4 < kMaxBufBytes;
}

bool wino4s_ok(const ct_conv_desc* d)
{
    if (!(d->kh == 3 && d->kw == 3 && d->stride == 1 && d->dil >= 1 && d->pad_h == d->dil && d->pad_w == d->dil &&
          d->cin % CC == 0 && d->nseg >= 0 && d->nseg <= 3 && (d->nseg == 0 || !d->res) && !d->transposed &&
          d->oh == d->h && d->ow == d->w))
        return false;
    // dilated: plain NCHW output with scale / shift / floor (what the dilated layers of the network use)
    return d->dil == 1 || (d->dil <= 8 && d->nseg == 0 && !d->res);
}

struct Sizes { int TY, TX, NT, Tpad, kblocks, chunks; size_t v_plane, m_plane, v_bytes, m_bytes; };

Sizes sizes_of(int batch, int oh, int ow, int cin, int cout, int dil, int opb = OPB)
{
    Sizes s{};
    s.TY = ((oh + dil - 1) / dil + 3) / 4; s.TX = ((ow + dil - 1) / dil + 3) / 4;      // per sub-lattice (dil = 1: the map)
    s.NT = batch * dil * dil * s.TY * s.TX;
    s.Tpad = (s.NT + BT - 1) / BT * BT;
    s.kblocks = (cout + BM - 1) / BM;
    s.chunks = cin / CC;
    s.v_plane = (size_t)(s.Tpad / BT) * s.chunks * opb;
    s.m_plane = (size_t)s.kblocks * BM * s.Tpad;
    s.v_bytes = ctdet::align_up(s.v_plane * NXI, 256);
    s.m_bytes = s.m_plane * NXI * 4;
    return s;
}

}  // namespace

extern "C" int ct_conv_wino4s_supported(const ct_conv_desc* d) { return d && wino4s_ok(d) ? 1 : 0; }

extern "C" size_t ct_conv_wino4s_packed_bytes(int cin, int cout)
{
    if (cin <= 0 || cout <= 0 || cin % CC) return 0;
    return (size_t)NXI * ((cout + BM - 1) / BM) * (cin / CC) * OPB;
}

extern "C" size_t ct_conv_wino4s_workspace_bytes(const ct_conv_desc* d)
{
    if (!d || !wino4s_ok(d) || d->batch <= 0 || d->cout <= 0) return 0;
    const Sizes s = sizes_of(d->batch, d->oh, d->ow, d->cin, d->cout, d->dil);
    // any variant (the f16x2 form: a header of one line per image for the maxima of |input| + a V two thirds the size)
    return ctdet::align_up((size_t)d->batch * LINE_BYTES, 256) + s.v_bytes + s.m_bytes;
}

extern "C" int ct_absmax_f32(const float* in, int batch, long long per_image, long long img_stride, unsigned* lines, ct_stream_t stream)
{
    CT_REQUIRE(in && lines && batch > 0 && per_image > 0 && img_stride >= per_image, "ct_absmax_f32: bad argument");
    const bool vec_ok = per_image % 4 == 0 && img_stride % 4 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0;
    const long items = (long)batch * ((per_image + 4095) / 4096);
    hipLaunchKernelGGL(absmax_lines_kernel, dim3((int)std::min<long>(items, 2048)), dim3(256), 0, ctdet::as_stream(stream), in, batch,
                       (long)per_image, (long)img_stride, vec_ok ? 1 : 0, lines);
    CT_LAUNCH_CHECK("absmax_lines_kernel");
    return CT_OK;
}

extern "C" size_t ct_conv_wino4s_h2_packed_bytes(int cin, int cout)
{
    if (cin <= 0 || cout <= 0 || cin % CC) return 0;
    return ctdet::wino_h2_trailer_offset(cin, cout, 47) + ctdet::kWino4hTrailerBytes;
}

size_t ctdet::wino_h2_trailer_offset(int cin, int cout, int tile)
{
    return tile == 48 ? (size_t)((cout + ctdet::kWinoKB - 1) / ctdet::kWinoKB) * (cin / CC) * ctdet::kWino4fhChunkBytes
                      : (size_t)NXI * ((cout + BM - 1) / BM) * (cin / CC) * OPBH;
}

namespace {
int fill_h2_item(const float* const* w, const int* cout, int nparts, int cin, int dgrad, int tile, void* upacked, WinoH2Item& it, const char* who)
{
    CT_REQUIRE(w && cout && upacked && nparts >= 1 && nparts <= 6, "%s: bad argument", who);
    CT_REQUIRE(tile == 47 || tile == 48, "%s: tile %d (47 = three-kernel form, 48 = fused)", who, tile);
    ctdet::WinoPackArgs& p = it.p;
    p = ctdet::WinoPackArgs{};
    int tot = 0;
    for (int i = 0; i < nparts; ++i) {
        CT_REQUIRE(w[i] && cout[i] > 0, "%s: part %d", who, i);
        p.w[i] = w[i];
        p.mbeg[i] = tot;
        tot += cout[i];
    }
    p.mbeg[nparts] = tot;
    p.nparts = nparts;
    p.dgrad = dgrad;
    p.tile = tile;
    p.cin_fwd = cin;
    p.cin = dgrad ? tot : cin;
    p.cout = dgrad ? cin : tot;
    CT_REQUIRE(p.cin > 0 && p.cin % CC == 0, "%s: %d input channels, must be a multiple of %d", who, p.cin, CC);
    p.chunks = p.cin / CC;
    const int rowblock = tile == 48 ? ctdet::kWinoKB : BM;
    p.kblocks = (p.cout + rowblock - 1) / rowblock;
    p.U = static_cast<float*>(upacked);
    it.trailer = reinterpret_cast<unsigned*>(static_cast<unsigned char*>(upacked) + ctdet::wino_h2_trailer_offset(p.cin, p.cout, tile));
    return CT_OK;
}
}  // namespace

int ctdet::pack_wino_h2(const float* const* w, const int* cout, int nparts, int cin, int dgrad, int tile, void* upacked,
                        ct_stream_t stream, const char* who)
{
    CT_REQUIRE(!ctdet::pack_recording(), "%s: the f16x2 packing takes the layer's maximum first and cannot be recorded (ct_pack_record_begin); "
               "batch it with ct_conv_wino_h2_pack_item / _run", who);
    WinoH2Item it;
    if (int e = fill_h2_item(w, cout, nparts, cin, dgrad, tile, upacked, it, who)) return e;
    const ctdet::WinoPackArgs& p = it.p;
    hipStream_t st = ctdet::as_stream(stream);
    CT_HIP(hipMemsetAsync(it.trailer, 0, ctdet::kWino4hTrailerBytes, st));
    const long nw = (long)p.mbeg[p.nparts] * cin * 9;
    hipLaunchKernelGGL(wino4h_wmax, dim3((int)std::min<long>((nw + 255) / 256, 1024)), dim3(256), 0, st, p, it.trailer);
    CT_LAUNCH_CHECK("wino4h_wmax");
    const int rowblock = tile == 48 ? ctdet::kWinoKB : BM;
    const long total = (long)p.kblocks * rowblock * (p.cin / 8) * 6;
    hipLaunchKernelGGL(wino4h_pack, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, p, it.trailer);
    CT_LAUNCH_CHECK("wino4h_pack");
    return CT_OK;
}

extern "C" size_t ct_conv_wino_h2_pack_item_bytes(void) { return sizeof(WinoH2Item); }

extern "C" int ct_conv_wino_h2_pack_item(const float* const* w, const int* cout, int nparts, int cin, int dgrad, int tile, void* upacked,
                                         void* item_out)
{
    CT_REQUIRE(item_out, "ct_conv_wino_h2_pack_item: null item");
    WinoH2Item it;
    if (int e = fill_h2_item(w, cout, nparts, cin, dgrad ? 1 : 0, tile, upacked, it, "ct_conv_wino_h2_pack_item")) return e;
    std::memcpy(item_out, &it, sizeof(it));
    return CT_OK;
}

extern "C" int ct_conv_wino_h2_pack_run(const void* items_dev, int n, ct_stream_t stream)
{
    CT_REQUIRE(items_dev && n > 0 && n <= 65535, "ct_conv_wino_h2_pack_run: bad argument");
    const WinoH2Item* items = static_cast<const WinoH2Item*>(items_dev);
    hipStream_t st = ctdet::as_stream(stream);
    hipLaunchKernelGGL(wino4h_trailer_zero_list, dim3((n + 63) / 64), dim3(64), 0, st, items, n);
    CT_LAUNCH_CHECK("wino4h_trailer_zero_list");
    hipLaunchKernelGGL(wino4h_wmax_list, dim3(64, n), dim3(256), 0, st, items);
    CT_LAUNCH_CHECK("wino4h_wmax_list");
    hipLaunchKernelGGL(wino4h_pack_list, dim3(256, n), dim3(256), 0, st, items);
    CT_LAUNCH_CHECK("wino4h_pack_list");
    return CT_OK;
}

extern "C" int ct_conv_pack_weights_wino4s_h2(const float* const* w, const int* cout, int nparts, int cin, void* upacked,
                                              ct_stream_t stream)
{
    return ctdet::pack_wino_h2(w, cout, nparts, cin, 0, 47, upacked, stream, "ct_conv_pack_weights_wino4s_h2");
}

extern "C" int ct_conv_pack_weights_wino4s_h2_dgrad(const float* const* w, const int* cout, int nparts, int cin, void* upacked,
                                                    ct_stream_t stream)
{
    return ctdet::pack_wino_h2(w, cout, nparts, cin, 1, 47, upacked, stream, "ct_conv_pack_weights_wino4s_h2_dgrad");
}

extern "C" int ct_conv_pack_weights_wino4s(const float* const* w, const int* cout, int nparts, int cin,
                                           void* upacked, ct_stream_t stream)
{
    return ctdet::pack_wino_any(w, cout, nparts, cin, 0, 44, (float*)upacked, stream, "ct_conv_pack_weights_wino4s");
}

extern "C" int ct_conv_pack_weights_wino4s_dgrad(const float* const* w, const int* cout, int nparts, int cin,
                                                 void* upacked, ct_stream_t stream)
{
    return ctdet::pack_wino_any(w, cout, nparts, cin, 1, 44, (float*)upacked, stream, "ct_conv_pack_weights_wino4s_dgrad");
}

static int launch_wino4s(const ct_conv_desc* d, const void* upacked, void* workspace, size_t workspace_bytes, int variant,
                         const ctdet::PoolOut& pool, ct_stream_t stream, const char* who)
{
    if (int rc = ctdet::wino_check_desc(d, upacked && workspace, d && wino4s_ok(d), who,
                                        "3x3 stride 1 pad = dilation (dilated: plain NCHW output), cin % 16 == 0"))
        return rc;
    CT_REQUIRE(variant == 1 || variant == 3, "%s: variant %d (1 = bf16x3, 3 = f16x2; both with two accumulators -- the one-accumulator "
               "variant 2 of rounds 4-5 was removed)", who, variant);
    const bool h2 = variant == 3;
    CT_REQUIRE(d->dil == 1 || !pool.pool_out, "%s: fused pooling on a dilated layer", who);
    ctdet::WinoLimits lim;
    if (int rc = ctdet::wino_check_launch(d, who, pool, &lim)) return rc;
    const int max_chunk = lim.max_chunk;
    const size_t hdr_bytes = h2 ? ctdet::align_up((size_t)std::min(d->batch, max_chunk) * LINE_BYTES, 256) : 0;
    {
        const Sizes s = sizes_of(std::min(d->batch, max_chunk), d->oh, d->ow, d->cin, d->cout, d->dil, h2 ? OPBH : OPB);
        CT_REQUIRE(workspace_bytes >= hdr_bytes + s.v_bytes + s.m_bytes, "%s: workspace of %zu bytes, needs %zu "
                   "(ct_conv_wino4s_workspace_bytes)", who, workspace_bytes, hdr_bytes + s.v_bytes + s.m_bytes);
        CT_REQUIRE((size_t)s.chunks * OPB < (size_t)kMaxBufBytes, "%s: too many input channels", who);
    }
    hipStream_t st = ctdet::as_stream(stream);
    {
        static std::once_flag once;
        static hipError_t attr_err = hipSuccess;
        std::call_once(once, [] {
            const std::pair<const void*, int> fs[] = {
                {(const void*)wino4s_in<false>, IN_LDS_BYTES}, {(const void*)wino4s_in<true>, IN_LDS_BYTES},
                {(const void*)wino4s_in_dil<false>, IN_LDS_BYTES}, {(const void*)wino4s_in_dil<true>, IN_LDS_BYTES},
                {(const void*)wino4s_gemm<true>, GEMM_LDS_BYTES},
                {(const void*)wino4h_gemm<true, 1, 4>, 4 * 2 * OPBH}, {(const void*)wino4h_gemm<true, 1, 5>, 5 * 2 * OPBH},
                {(const void*)wino4h_gemm<true, 2, 2>, 2 * 2 * 2 * OPBH}};
            for (const auto& f : fs)
                if (attr_err == hipSuccess) attr_err = hipFuncSetAttribute(f.first, hipFuncAttributeMaxDynamicSharedMemorySize, f.second);
        });
        CT_HIP(attr_err);
    }
    // f16x2: k-groups per barrier / ring depth of the GEMM pipeline (measurement switch; default below)
    static const int h2_pipe = [] { const char* e = std::getenv("CTDET_W4H_PIPE"); return e ? std::atoi(e) : 22; }();
    for (int b0 = 0; b0 < d->batch; b0 += max_chunk) {
        const int nb = std::min(max_chunk, d->batch - b0);
        const Sizes s = sizes_of(nb, d->oh, d->ow, d->cin, d->cout, d->dil, h2 ? OPBH : OPB);
        Wino4sArgs a{};
        ctdet::wino_fill(a, d, upacked, lim, pool, b0, nb, 0);
        a.chunks = s.chunks; a.kblocks = s.kblocks;
        a.TY = s.TY; a.TX = s.TX; a.NT = s.NT; a.Tpad = s.Tpad;
        a.tblk32 = s.Tpad / TB; a.tblk128 = s.Tpad / BT;
        a.dil = d->dil;
        a.V = reinterpret_cast<unsigned short*>(static_cast<unsigned char*>(workspace) + hdr_bytes);
        a.Mw = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + hdr_bytes + s.v_bytes);
        a.v_plane = s.v_plane;
        a.u_plane = (size_t)s.kblocks * s.chunks * (h2 ? OPBH : OPB);
        a.m_plane = s.m_plane;
        a.batch = nb;
        if (h2) {
            a.eU = reinterpret_cast<const int*>(static_cast<const unsigned char*>(upacked) + (size_t)NXI * a.u_plane) + 1;
            if (d->in_absmax) {              // the producer of the input left the maxima (upper bounds over the slice, per image)
                a.amax = d->in_absmax + (size_t)b0 * ctdet::h2::kLineWords;
            } else {                         // an absmax pass of its own into the workspace header
                unsigned* hdr = static_cast<unsigned*>(workspace);
                a.amax = hdr;
                const long per_image = (long)d->cin * d->h * d->w;
                const long img_stride = (long)d->in_ctot * d->h * d->w;
                const float* base = a.in + (size_t)d->in_coff * d->h * d->w;
                const bool vec_ok = per_image % 4 == 0 && img_stride % 4 == 0 && reinterpret_cast<uintptr_t>(base) % 16 == 0;
                const long items = (long)nb * ((per_image + 4095) / 4096);
                CT_PROF("wino4h_absmax", st);
                CT_HIP(hipMemsetAsync(hdr, 0, hdr_bytes, st));
                hipLaunchKernelGGL(absmax_lines_kernel, dim3((int)std::min<long>(items, 2048)), dim3(256), 0, st, base, nb, per_image,
                                   img_stride, vec_ok ? 1 : 0, hdr);
                CT_LAUNCH_CHECK("absmax_lines_kernel");
            }
        }
        a.out_amax = d->out_absmax ? d->out_absmax + (size_t)b0 * ctdet::h2::kLineWords : nullptr;
        // transform: ~2048 workgroups (four rounds of two per CU) unless the layer has fewer (tile block, chunk) pairs
        const long pairs = (long)a.tblk32 * a.chunks;
        a.chunks_per_wg = (int)std::max<long>(1, std::min<long>(a.chunks, pairs / 2048));
        const int ygroups = (a.chunks + a.chunks_per_wg - 1) / a.chunks_per_wg;
        {
            CT_PROF("wino4s_in", st);
            if (h2) {
                if (a.dil > 1) hipLaunchKernelGGL(wino4s_in_dil<true>, dim3(a.tblk32, ygroups), dim3(256), IN_LDS_BYTES, st, a);
                else hipLaunchKernelGGL(wino4s_in<true>, dim3(a.tblk32, ygroups), dim3(256), IN_LDS_BYTES, st, a);
            } else {
                if (a.dil > 1) hipLaunchKernelGGL(wino4s_in_dil<false>, dim3(a.tblk32, ygroups), dim3(256), IN_LDS_BYTES, st, a);
                else hipLaunchKernelGGL(wino4s_in<false>, dim3(a.tblk32, ygroups), dim3(256), IN_LDS_BYTES, st, a);
            }
            CT_LAUNCH_CHECK("wino4s_in");
        }
        {
            CT_PROF("wino4s_gemm", st);
            GemmArgs g{};
            g.A = reinterpret_cast<const unsigned char*>(a.U); g.B = reinterpret_cast<const unsigned char*>(a.V); g.M = a.Mw;
            g.a_plane = a.u_plane; g.b_plane = a.v_plane; g.m_plane = a.m_plane; g.m_slab = 0;
            g.chunks = g.chunks_per_split = a.chunks; g.rowblocks = a.kblocks; g.colblocks = a.tblk128; g.ldm = a.Tpad;
            g.rows = a.M; g.cols = a.NT;
            const int nwg = NXI * a.tblk128 * a.kblocks;
            if (h2) {
                const int pipe = (a.chunks & 1) && h2_pipe == 22 ? 14 : h2_pipe;       // two k-groups per barrier need an even count
                if (pipe == 22) hipLaunchKernelGGL((wino4h_gemm<true, 2, 2>), dim3(nwg), dim3(256), 2 * 2 * 2 * OPBH, st, g);
                else if (pipe == 15) hipLaunchKernelGGL((wino4h_gemm<true, 1, 5>), dim3(nwg), dim3(256), 5 * 2 * OPBH, st, g);
                else hipLaunchKernelGGL((wino4h_gemm<true, 1, 4>), dim3(nwg), dim3(256), 4 * 2 * OPBH, st, g);
            } else hipLaunchKernelGGL(wino4s_gemm<true>, dim3(nwg), dim3(256), GEMM_LDS_BYTES, st, g);
            CT_LAUNCH_CHECK("wino4s_gemm");
        }
        {
            CT_PROF("wino4s_out", st);
            if (h2) hipLaunchKernelGGL(wino4s_out<true>, dim3((a.NT + 63) / 64, (a.M + 3) / 4), dim3(256), 0, st, a);
            else hipLaunchKernelGGL(wino4s_out<false>, dim3((a.NT + 63) / 64, (a.M + 3) / 4), dim3(256), 0, st, a);
            CT_LAUNCH_CHECK("wino4s_out");
        }
    }
    return CT_OK;
}

extern "C" int ct_conv2d_wino4s_pool_fwd(const ct_conv_desc* d, const void* upacked, void* workspace,
                                         size_t workspace_bytes, int variant, float* pool_out, int pool_ctot,
                                         int pool_coff, int pool_oh, int pool_ow, int write_full, ct_stream_t stream)
{
    return launch_wino4s(d, upacked, workspace, workspace_bytes, variant, {pool_out, pool_ctot, pool_coff, pool_oh, pool_ow, write_full},
                         stream, "ct_conv2d_wino4s_pool_fwd");
}

extern "C" int ct_conv2d_wino4s_fwd(const ct_conv_desc* d, const void* upacked, void* workspace, size_t workspace_bytes,
                                    int variant, ct_stream_t stream)
{
    return launch_wino4s(d, upacked, workspace, workspace_bytes, variant, {nullptr, 0, 0, 0, 0, 1}, stream, "ct_conv2d_wino4s_fwd");
}

extern "C" int ct_conv_wgrad_wino4s_supported(const ct_conv_desc* d) { return d && wino4s_wg_ok(d) ? 1 : 0; }

extern "C" size_t ct_conv_wgrad_wino4s_workspace_bytes(const ct_conv_desc* d)
{
    if (!d || !wino4s_wg_ok(d) || d->batch <= 0) return 0;
    const WgSizes s = wg_sizes_of(d->batch, d->oh, d->ow, d->cin, d->cout, d->dil);
    return s.e_bytes + s.v_bytes + s.m_bytes;
}

extern "C" int ct_conv2d_wgrad_wino4s(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, float* dw,
                                      void* workspace, size_t workspace_bytes, ct_stream_t stream)
{
    const char* who = "ct_conv2d_wgrad_wino4s";
    if (int rc = ctdet::wgrad_check_pointers(d, dz, dw, workspace, who)) return rc;
    if (!wino4s_wg_ok(d))
        return ctdet::fail(CT_ERR_UNSUPPORTED, "%s: needs 3x3 stride 1 pad = dilation, cin %% 16 == 0 (got %dx%d s%d d%d p%d cin=%d)",
                           who, d->kh, d->kw, d->stride, d->dil, d->pad_h, d->cin);
    if (int rc = ctdet::wgrad_check_slices(d, dz_ctot, dz_coff, who)) return rc;
    ctdet::WgradLimits lim;
    if (int rc = ctdet::wgrad_limits(d, dz_ctot, who, &lim)) return rc;
    const long long x_bytes = lim.x_bytes, z_bytes = lim.z_bytes;       // one launch covers the batch (no chunking)
    CT_REQUIRE(x_bytes < kMaxBufBytes && z_bytes < kMaxBufBytes, "%s: a tensor exceeds 2 GiB (use ct_conv2d_wgrad_wino4)", who);
    const WgSizes s = wg_sizes_of(d->batch, d->oh, d->ow, d->cin, d->cout, d->dil);
    CT_REQUIRE(workspace_bytes >= s.e_bytes + s.v_bytes + s.m_bytes, "%s: workspace of %zu bytes, needs %zu", who, workspace_bytes,
               s.e_bytes + s.v_bytes + s.m_bytes);
    CT_REQUIRE((size_t)s.kchunks * OPB < (size_t)kMaxBufBytes, "%s: too many tiles for one launch", who);
    hipStream_t st = ctdet::as_stream(stream);
    for (const void* fn : {(const void*)wino4s_tk<true>, (const void*)wino4s_tk<false>})
        CT_HIP(ctdet::raise_lds_limit(fn, TK_LDS_BYTES));
    CT_HIP(ctdet::raise_lds_limit((const void*)wino4s_gemm<true>, GEMM_LDS_BYTES));
    unsigned char* E = static_cast<unsigned char*>(workspace);
    unsigned char* V = E + s.e_bytes;
    float* M = reinterpret_cast<float*>(V + s.v_bytes);
    auto launch_tk = [&](bool is_e) -> int {
        TkArgs t{};
        t.src = is_e ? dz : d->in;
        t.src_bytes = (unsigned)(is_e ? z_bytes : x_bytes);
        t.C = is_e ? d->cout : d->cin; t.H = d->h; t.W = d->w;
        t.ctot = is_e ? dz_ctot : d->in_ctot; t.coff = is_e ? dz_coff : d->in_coff;
        t.TY = s.TY; t.TX = s.TX; t.NT = s.NT; t.tblk32 = s.tblk32; t.kchunks = s.kchunks;
        t.chunks = (is_e ? s.rb : s.cb) * (BM / CC);       // every 16-channel chunk of the padded 128-row blocks: rows past C are zeros
        const long pairs = (long)t.tblk32 * t.chunks;
        t.chunks_per_wg = (int)std::max<long>(1, std::min<long>(t.chunks, pairs / 2048));
        t.dst = is_e ? E : V;
        t.plane = is_e ? s.e_plane : s.v_plane;
        t.dil = d->dil;
        const dim3 grid(t.tblk32, (t.chunks + t.chunks_per_wg - 1) / t.chunks_per_wg);
        if (is_e) hipLaunchKernelGGL(wino4s_tk<true>, grid, dim3(256), TK_LDS_BYTES, st, t);
        else hipLaunchKernelGGL(wino4s_tk<false>, grid, dim3(256), TK_LDS_BYTES, st, t);
        CT_LAUNCH_CHECK("wino4s_tk");
        return CT_OK;
    };
    {
        CT_PROF("wino4s_tk_e", st);
        const int rc = launch_tk(true);
        if (rc != CT_OK) return rc;
    }
    {
        CT_PROF("wino4s_tk_v", st);
        const int rc = launch_tk(false);
        if (rc != CT_OK) return rc;
    }
    {
        CT_PROF("wino4s_gemm_wgrad", st);
        GemmArgs g{};
        g.A = E; g.B = V; g.M = M;
        g.a_plane = s.e_plane; g.b_plane = s.v_plane; g.m_plane = s.m_plane; g.m_slab = s.m_slab;
        g.chunks = s.kchunks; g.chunks_per_split = s.cps; g.rowblocks = s.rb; g.colblocks = s.cb; g.ldm = s.cb * BT;
        g.rows = d->cout; g.cols = d->cin;
        hipLaunchKernelGGL(wino4s_gemm<true>, dim3(NXI * s.rb * s.cb, s.splits), dim3(256), GEMM_LDS_BYTES, st, g);
        CT_LAUNCH_CHECK("wino4s_gemm (weight gradient)");
    }
    const int KC = d->cout * d->cin;
    hipLaunchKernelGGL(wino4s_wgrad_finish, dim3((KC + 255) / 256), dim3(256), 0, st, M, dw, d->cout, d->cin, s.cb * BT, s.m_plane,
                       s.m_slab, s.splits);
    CT_LAUNCH_CHECK("wino4s_wgrad_finish");
    return CT_OK;
}
