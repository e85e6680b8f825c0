// libctdet: Winograd F(4x4,3x3) for the bf16 channels-last path, transform-domain operands as SINGLE binary16 pieces on the f16
// matrix pipe (v_mfma_f32_32x32x16_f16).  3x3 / stride 1 / pad 1 / dilation 1 layers, cin % 8 == 0, cin >= 16, plain NHWC
// bf16 output (no head scatter, residual or per-channel floor).
//
// Why binary16 and not bfloat16 in the transform domain: B^T d B and G g G^T spread the values over a few more bits than the
// activations have, and eight significant bits there cost 6-8x the error of the direct bf16 kernel; eleven bits with one
// power-of-two scale per image (V) and per layer (U) stay at the direct kernel's error (ct_f16x2.h: exponent_for, the matrix
// pipe honours subnormal binary16 inputs) at F(4x4)'s 4x fewer multiplications.
//
// Three kernels and a packer, interpolation points 0, +-3/4, +-3/2, inf (ct_wino4_points.h):
//   pack     U = G g G^T in double, eU = exponent_for(max |g| of the layer, kGrowthGG), rne16(U 2^eU) in the GEMM's fragment
//            order [36][cout block of 32][k-step of 16][lane 64][8]; a 256-byte trailer carries eU.
//   wbf_in   one lane = one (tile, 8 channels): 6x6 patch, B^T d B in fp32 (two passes of 4 channels, 8-byte loads: the two
//            halves of one 16-byte fragment slot), times 2^eImg (eImg from line n of the maxima), rounded once, written as
//            MFMA A fragments [36][tile block of 32][k-step][lane][8]; tiles past the batch and channels past cin are zeros.
//   wbf_gemm 36 GEMMs M[xi] = V[xi] U[xi], fp32 accumulators: 128 tiles x 128 couts per workgroup (2 x 2 waves of 64 x 64), four
//            k-steps per stage copied global -> registers -> LDS (fragments are stored ready-made: a straight 16-byte copy,
//            conflict-free reads), the next stage's loads in flight behind the MFMAs; 32 x 32 accumulator blocks wholly past
//            the layer's tiles / couts issue no MFMAs and store nothing.
//   wbf_out  one lane = one (tile, 2 couts): A^T M A in fp32, times 2^-(eU + eImg) as two exact factors, scale / shift / ReLU,
//            rne to bf16, stored into the channel slice; max |y| of what it stores folded per image into out_absmax.
// An image's result does not depend on its batch mates: its exponent is its own, and a tile's sums run over k in one order.
#include "ct_common.h"
#include "ct_device.h"
#include "ct_f16x2.h"
#include "ct_wino4_points.h"
#include <algorithm>

namespace {

using ctdet::f16x8;
using ctdet::f32x16;
using ctdet::i32x4;
using ctdet::kMaxBufBytes;
using ctdet::h2::exponent_for;
using ctdet::h2::kGrowthBtB;
using ctdet::h2::kGrowthGG;
using ctdet::h2::kLineWords;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int kMaxParts = 6;
constexpr int FRAG_BYTES = 1024;            // 64 lanes x 8 binary16: one 32 x 16 operand block
constexpr int TRAILER_BYTES = 256;          // word 0: eU, word 1: bit pattern of max |g|
constexpr int STAGE_KS = 4;                 // k-steps per LDS stage (64 channels)
constexpr int GEMM_LDS = 2 * 4 * STAGE_KS * FRAG_BYTES;       // [operand][block of 32][k-step]

__device__ __forceinline__ float bf16_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xFFFF0000u); }
// round to nearest even; a NaN stays a (quiet) NaN
__device__ __forceinline__ unsigned to_bf16(float f)
{
    const unsigned u = __builtin_bit_cast(unsigned, f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ unsigned pack_f16(float a, float b)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, f16x2));
}

// ------------------------------------------------------------------------------------------------ weights
struct PackArgs {
    const float* w[kMaxParts];
    int cout_end[kMaxParts];        // running ends of the concatenated couts
    int nparts, cin, cout;
    int NB, KS;
    unsigned char* out;
};

__device__ __forceinline__ const float* filter_of(const PackArgs& a, int co, int ci)
{
    int p = 0, begin = 0;
    while (p + 1 < a.nparts && co >= a.cout_end[p]) { begin = a.cout_end[p]; ++p; }
    return a.w[p] + ((size_t)(co - begin) * a.cin + ci) * 9;
}

__global__ __launch_bounds__(256) void wbf_pack_max(const PackArgs a)
{
    const int n = a.cout * a.cin;
    float run = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float* g = filter_of(a, i / a.cin, i % a.cin);
#pragma unroll
        for (int t = 0; t < 9; ++t) ctdet::h2::track_absmax(run, g[t]);
    }
    const unsigned m = ctdet::h2::wave_max(__builtin_bit_cast(unsigned, run) & 0x7FFFFFFFu);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(reinterpret_cast<unsigned*>(a.out + (size_t)36 * a.NB * a.KS * FRAG_BYTES) + 1, m);
}

// one thread = one (cout, cin) of the padded [NB * 32][KS * 16] matrix
__global__ __launch_bounds__(256) void wbf_pack(const PackArgs a)
{
    const int Kp = a.KS * 16;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.NB * 32 * Kp) return;
    const int co = i / Kp, ci = i - co * Kp;
    int* trailer = reinterpret_cast<int*>(a.out + (size_t)36 * a.NB * a.KS * FRAG_BYTES);
    const int eU = exponent_for((unsigned)trailer[1], kGrowthGG);
    if (i == 0) trailer[0] = eU;
    double U[6][6];
    if (co < a.cout && ci < a.cin) {
        const float* g = filter_of(a, co, ci);
        double t[3][6];
#pragma unroll
        for (int r = 0; r < 3; ++r) ctdet::w4::gmul6(g[3 * r], g[3 * r + 1], g[3 * r + 2], t[r]);      // g G^T, row r
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            double col[6];
            ctdet::w4::gmul6(t[0][b], t[1][b], t[2][b], col);
#pragma unroll
            for (int x = 0; x < 6; ++x) U[x][b] = col[x];
        }
    } else {
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
            for (int b = 0; b < 6; ++b) U[x][b] = 0.0;
    }
    // B fragment of the 32x32x16 MFMA: lane = (k half) * 32 + column, 8 consecutive k per lane
    const int nb = co >> 5, ks = ci >> 4, lane = (((ci >> 3) & 1) << 5) | (co & 31);
    const double s = __builtin_ldexp(1.0, eU);
    _Float16* out = reinterpret_cast<_Float16*>(a.out);
#pragma unroll
    for (int x = 0; x < 6; ++x)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const size_t frag = ((size_t)(x * 6 + b) * a.NB + nb) * a.KS + ks;
            out[frag * (FRAG_BYTES / 2) + lane * 8 + (ci & 7)] = (_Float16)(U[x][b] * s);
        }
}

// ------------------------------------------------------------------------------------------------ maxima
// max |x| over the channel slice of every image: grid (blocks, batch)
__global__ __launch_bounds__(256) void absmax_bf16_nhwc(const unsigned short* __restrict__ x, int hw, int ctot, int coff, int c,
                                                        unsigned* __restrict__ lines)
{
    const int n = blockIdx.y;
    const unsigned short* img = x + (size_t)n * hw * ctot + coff;
    float run = 0.f;
    if (((ctot | coff | c) & 7) == 0 && (reinterpret_cast<size_t>(x) & 15) == 0) {
        const int g8 = c >> 3;
        const long long total = (long long)hw * g8;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
            const long long p = i / g8;
            const int g = (int)(i - p * g8);
            const i32x4 q = *reinterpret_cast<const i32x4*>(img + p * ctot + g * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ctdet::h2::track_absmax(run, bf16_lo((unsigned)q[j]));
                ctdet::h2::track_absmax(run, bf16_hi((unsigned)q[j]));
            }
        }
    } else {
        const long long total = (long long)hw * c;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
            const long long p = i / c;
            ctdet::h2::track_absmax(run, bf16_lo(img[p * ctot + (i - p * c)]));
        }
    }
    const unsigned m = ctdet::h2::wave_max(__builtin_bit_cast(unsigned, run) & 0x7FFFFFFFu);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(lines + (size_t)n * kLineWords, m);
}

// ------------------------------------------------------------------------------------------------ forward
struct FwdArgs {
    const unsigned short* in;
    unsigned short* out;
    const unsigned char* U;
    unsigned char* V;
    float* M;
    const unsigned* in_lines;
    unsigned* out_lines;
    const float* scale;
    const float* shift;
    int batch, cin, cout, H, W;
    int in_ctot, in_coff, out_ctot, out_coff;
    int th, tw, T;              // tiles per image column / row, tiles of the batch
    int TB, NB, KS;             // tile blocks of 32, cout blocks of 32, k-steps of 16
    int relu;
};

// grid (TB, ceil(KS / 4)), 4 waves: wave w writes the A fragment (tile block, k-step 4 y + w)
__global__ __launch_bounds__(256) void wbf_in(const FwdArgs a)
{
    const int lane = threadIdx.x & 63;
    const int ks = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (ks >= a.KS) return;
    const int tb = blockIdx.x;
    const int tile = tb * 32 + (lane & 31);
    const int c0 = ks * 16 + (lane >> 5) * 8;
    const bool live = tile < a.T && c0 < a.cin;
    const int tpi = a.th * a.tw;
    const int n = live ? tile / tpi : 0;
    const int tr = live ? tile - n * tpi : 0;
    const int ty = tr / a.tw, tx = tr - ty * a.tw;
    const int y0 = 4 * ty - 1, x0 = 4 * tx - 1;
    const float s = __builtin_ldexpf(1.f, ctdet::h2::image_exponent(a.in_lines, n, kGrowthBtB));
    const unsigned short* img = a.in + (size_t)n * a.H * a.W * a.in_ctot + a.in_coff + c0;
    unsigned char* vbase = a.V + ((size_t)tb * a.KS + ks) * FRAG_BYTES + lane * 16;
    const size_t xi_stride = (size_t)a.TB * a.KS * FRAG_BYTES;

    for (int q = 0; q < 2; ++q) {           // the two 8-byte halves of the lane's fragment slot
        u32x2 raw[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int y = y0 + i, x = x0 + j;
                raw[i][j] = u32x2{0u, 0u};
                if (live && y >= 0 && y < a.H && x >= 0 && x < a.W)
                    raw[i][j] = *reinterpret_cast<const u32x2*>(img + ((size_t)y * a.W + x) * a.in_ctot + 4 * q);
            }
        unsigned outw[36][2];
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {    // channel pair (2 pr, 2 pr + 1) of the four
            float v0[6][6], v1[6][6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {   // B^T along the rows of the patch, column j
                float d0[6], d1[6], o0[6], o1[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    d0[i] = bf16_lo(raw[i][j][pr]) * s;
                    d1[i] = bf16_hi(raw[i][j][pr]) * s;
                }
                ctdet::w4::bt6(d0, o0);
                ctdet::w4::bt6(d1, o1);
#pragma unroll
                for (int i = 0; i < 6; ++i) { v0[i][j] = o0[i]; v1[i][j] = o1[i]; }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {   // ... and along the columns
                float o0[6], o1[6];
                ctdet::w4::bt6(v0[i], o0);
                ctdet::w4::bt6(v1[i], o1);
#pragma unroll
                for (int j = 0; j < 6; ++j) outw[i * 6 + j][pr] = pack_f16(o0[j], o1[j]);
            }
        }
#pragma unroll
        for (int xi = 0; xi < 36; ++xi)
            *reinterpret_cast<u32x2*>(vbase + xi * xi_stride + q * 8) = u32x2{outw[xi][0], outw[xi][1]};
    }
}

// grid (ceil(TB / 4) * ceil(NB / 4), 36)
__global__ __launch_bounds__(256) void wbf_gemm(const FwdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char wb_lds[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hsel = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave & 1, wc = wave >> 1;
    const int xi = blockIdx.y;
    const int gm = (a.TB + 3) >> 2;
    const int tb0 = (blockIdx.x % gm) * 4, nb0 = (blockIdx.x / gm) * 4;
    const unsigned char* Vx = a.V + (size_t)xi * a.TB * a.KS * FRAG_BYTES;
    const unsigned char* Ux = a.U + (size_t)xi * a.NB * a.KS * FRAG_BYTES;

    // copy role: piece j of the stage = block j (j < 4: tiles, else couts), this thread's 16 bytes of its 4 KB
    const int cks = tid >> 6;               // k-step of the stage this thread copies
    i32x4 pre[8];
    auto load_stage = [&](int ks0) {
        const bool kv = ks0 + cks < a.KS;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int blk = j < 4 ? tb0 + j : nb0 + j - 4;
            const bool ok = kv && blk < (j < 4 ? a.TB : a.NB);
            const unsigned char* src = (j < 4 ? Vx : Ux) + ((size_t)(ok ? blk : 0) * a.KS + (ok ? ks0 + cks : 0)) * FRAG_BYTES +
                                       (tid & 63) * 16;
            pre[j] = ok ? *reinterpret_cast<const i32x4*>(src) : i32x4{0, 0, 0, 0};
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int j = 0; j < 8; ++j) *reinterpret_cast<i32x4*>(wb_lds + (j * STAGE_KS) * FRAG_BYTES + tid * 16) = pre[j];
    };

    bool on[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) on[i][j] = tb0 + wr * 2 + i < a.TB && nb0 + wc * 2 + j < a.NB;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load_stage(0);
    for (int ks0 = 0; ks0 < a.KS; ks0 += STAGE_KS) {
        store_stage();
        __syncthreads();
        if (ks0 + STAGE_KS < a.KS) load_stage(ks0 + STAGE_KS);
#pragma unroll
        for (int ks = 0; ks < STAGE_KS; ++ks) {
            if (ks0 + ks >= a.KS) break;
            const unsigned char* fb = wb_lds + ks * FRAG_BYTES + lane * 16;
            f16x8 va[2], ub[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                va[i] = *reinterpret_cast<const f16x8*>(fb + (wr * 2 + i) * STAGE_KS * FRAG_BYTES);
                ub[i] = *reinterpret_cast<const f16x8*>(fb + (4 + wc * 2 + i) * STAGE_KS * FRAG_BYTES);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (on[i][j]) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va[i], ub[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // M[xi][tile][cout]: lanes along couts
    const int Np = a.NB * 32;
    float* Mx = a.M + (size_t)xi * a.TB * 32 * Np;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!on[i][j]) continue;
            const int co = (nb0 + wc * 2 + j) * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = (tb0 + wr * 2 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
                Mx[(size_t)t * Np + co] = acc[i][j][r];
            }
        }
}

// one lane = one (tile, 2 couts); every lane of a wave reaches flush_absmax
__global__ __launch_bounds__(256) void wbf_out(const FwdArgs a)
{
    const int Np = a.NB * 32, pairs = Np >> 1;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int tile = (int)(gid / pairs);
    const int co = 2 * (int)(gid - (long long)tile * pairs);
    const bool live = tile < a.T && co < a.cout;
    const int tpi = a.th * a.tw;
    const int n = live ? tile / tpi : 0;
    const int tr = live ? tile - n * tpi : 0;
    const int ty = tr / a.tw, tx = tr - ty * a.tw;
    float run = 0.f;
    if (live) {
        const int eU = reinterpret_cast<const int*>(a.U + (size_t)36 * a.NB * a.KS * FRAG_BYTES)[0];
        const ctdet::h2::pow2x2 u = ctdet::h2::unscale_for(eU, ctdet::h2::image_exponent(a.in_lines, n, kGrowthBtB));
        const size_t xi_stride = (size_t)a.TB * 32 * Np;
        const float* m = a.M + (size_t)tile * Np + co;
        float t0[4][6], t1[4][6];           // A^T M: column b
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            float c0[6], c1[6], o0[4], o1[4];
#pragma unroll
            for (int x = 0; x < 6; ++x) {
                const f32x2 v = *reinterpret_cast<const f32x2*>(m + (size_t)(x * 6 + b) * xi_stride);
                c0[x] = v[0];
                c1[x] = v[1];
            }
            ctdet::w4::at4(c0, o0);
            ctdet::w4::at4(c1, o1);
#pragma unroll
            for (int i = 0; i < 4; ++i) { t0[i][b] = o0[i]; t1[i][b] = o1[i]; }
        }
        const bool two = co + 1 < a.cout;
        const float sc0 = a.scale[co], sh0 = a.shift[co];
        const float sc1 = two ? a.scale[co + 1] : 0.f, sh1 = two ? a.shift[co + 1] : 0.f;
        const bool wide = two && ((a.out_ctot | (a.out_coff + co)) & 1) == 0;
        unsigned short* img = a.out + (size_t)n * a.H * a.W * a.out_ctot + a.out_coff + co;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float y0[4], y1[4];
            ctdet::w4::at4(t0[i], y0);
            ctdet::w4::at4(t1[i], y1);
            const int oy = 4 * ty + i;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ox = 4 * tx + j;
                if (oy >= a.H || ox >= a.W) continue;
                float r0 = fmaf((y0[j] * u.lo) * u.hi, sc0, sh0);
                float r1 = fmaf((y1[j] * u.lo) * u.hi, sc1, sh1);
                if (a.relu) { r0 = fmaxf(r0, 0.f); r1 = fmaxf(r1, 0.f); }
                const unsigned b0 = to_bf16(r0), b1 = to_bf16(r1);
                unsigned short* p = img + ((size_t)oy * a.W + ox) * a.out_ctot;
                ctdet::h2::track_absmax(run, bf16_lo(b0));
                if (wide) {
                    *reinterpret_cast<unsigned*>(p) = b0 | (b1 << 16);
                } else {
                    p[0] = (unsigned short)b0;
                    if (two) p[1] = (unsigned short)b1;
                }
                if (two) ctdet::h2::track_absmax(run, bf16_lo(b1));
            }
        }
    }
    if (a.out_lines) ctdet::h2::flush_absmax(a.out_lines, live ? n : -1, run);
}

bool geometry_ok(const ct_conv_desc* d)
{
    return d && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad_h == 1 && d->pad_w == 1 && d->dil == 1 &&
           d->cin % 8 == 0 && d->cin >= 16 && d->cout > 0 && d->batch > 0 && d->h > 0 && d->w > 0 && d->oh == d->h &&
           d->ow == d->w && d->nseg == 0 && !d->res && !d->lo;
}

struct Layout {
    int th, tw, T, TB, NB, KS;
    size_t lines_bytes, v_bytes, m_bytes;
};

Layout layout_of(const ct_conv_desc* d)
{
    Layout l{};
    l.th = (d->h + 3) / 4;
    l.tw = (d->w + 3) / 4;
    const long long T = (long long)d->batch * l.th * l.tw;
    l.T = (int)T;
    l.TB = (int)((T + 31) / 32);
    l.NB = (d->cout + 31) / 32;
    l.KS = (d->cin + 15) / 16;
    l.lines_bytes = ctdet::align_up((size_t)d->batch * CT_ABSMAX_LINE_BYTES, 256);
    l.v_bytes = (size_t)36 * l.TB * l.KS * FRAG_BYTES;
    l.m_bytes = (size_t)36 * l.TB * 32 * l.NB * 32 * 4;
    return l;
}

size_t u_bytes(int cin, int cout) { return (size_t)36 * ((cout + 31) / 32) * ((cin + 15) / 16) * FRAG_BYTES; }

}  // namespace

extern "C" int ct_conv_bf16_wino_supported(const ct_conv_desc* d) { return geometry_ok(d) ? 1 : 0; }

extern "C" size_t ct_conv_bf16_wino_packed_bytes(int cin, int cout)
{
    if (cin <= 0 || cout <= 0) return 0;
    return u_bytes(cin, cout) + TRAILER_BYTES;
}

extern "C" int ct_conv_pack_weights_bf16_wino(const float* const* w, const int* cout, int nparts, int cin, void* out,
                                              ct_stream_t stream)
{
    CT_REQUIRE(w && cout && out, "ct_conv_pack_weights_bf16_wino: null argument");
    CT_REQUIRE(nparts >= 1 && nparts <= kMaxParts, "ct_conv_pack_weights_bf16_wino: nparts is %d (1..%d)", nparts, kMaxParts);
    CT_REQUIRE(cin > 0 && cin % 8 == 0, "ct_conv_pack_weights_bf16_wino: cin is %d (a positive multiple of 8)", cin);
    PackArgs a{};
    int total = 0;
    for (int p = 0; p < nparts; ++p) {
        CT_REQUIRE(w[p] && cout[p] > 0, "ct_conv_pack_weights_bf16_wino: part %d is empty", p);
        total += cout[p];
        a.w[p] = w[p];
        a.cout_end[p] = total;
    }
    a.nparts = nparts; a.cin = cin; a.cout = total;
    a.NB = (total + 31) / 32; a.KS = (cin + 15) / 16;
    a.out = static_cast<unsigned char*>(out);
    hipStream_t st = ctdet::as_stream(stream);
    CT_HIP(hipMemsetAsync(a.out + u_bytes(cin, total), 0, TRAILER_BYTES, st));
    const int n = total * cin;
    hipLaunchKernelGGL(wbf_pack_max, dim3(std::min(1024, (n + 255) / 256)), dim3(256), 0, st, a);
    CT_LAUNCH_CHECK("wbf_pack_max");
    hipLaunchKernelGGL(wbf_pack, dim3((a.NB * 32 * a.KS * 16 + 255) / 256), dim3(256), 0, st, a);
    CT_LAUNCH_CHECK("wbf_pack");
    return CT_OK;
}

extern "C" int ct_absmax_bf16_nhwc(const void* x, int batch, int hw, int ctot, int coff, int c, unsigned* lines,
                                   ct_stream_t stream)
{
    CT_REQUIRE(x && lines, "ct_absmax_bf16_nhwc: null argument");
    CT_REQUIRE(batch > 0 && hw > 0 && c > 0 && coff >= 0 && coff + c <= ctot,
               "ct_absmax_bf16_nhwc: bad shape (batch %d, hw %d, slice %d + %d of %d)", batch, hw, coff, c, ctot);
    hipStream_t st = ctdet::as_stream(stream);
    CT_HIP(hipMemsetAsync(lines, 0, (size_t)batch * CT_ABSMAX_LINE_BYTES, st));
    const long long work = (long long)hw * c / 8;
    const int blocks = (int)std::max<long long>(1, std::min<long long>(256, (work + 1023) / 1024));
    CT_PROF("absmax_bf16_nhwc", st);
    hipLaunchKernelGGL(absmax_bf16_nhwc, dim3(blocks, batch), dim3(256), 0, st, static_cast<const unsigned short*>(x), hw, ctot,
                       coff, c, lines);
    CT_LAUNCH_CHECK("absmax_bf16_nhwc");
    return CT_OK;
}

extern "C" size_t ct_conv_bf16_wino_workspace_bytes(const ct_conv_desc* d)
{
    if (!geometry_ok(d)) return 0;
    const Layout l = layout_of(d);
    return l.lines_bytes + l.v_bytes + l.m_bytes;
}

extern "C" int ct_conv2d_bf16_wino_fwd(const ct_conv_desc* d, void* workspace, size_t workspace_bytes, ct_stream_t stream)
{
    CT_REQUIRE(d, "ct_conv2d_bf16_wino_fwd: desc is null");
    if (!geometry_ok(d))
        return ctdet::fail(CT_ERR_UNSUPPORTED, "ct_conv2d_bf16_wino_fwd: needs a 3x3 / stride 1 / pad 1 / dilation 1 layer with "
                           "cin %% 8 == 0, cin >= 16, oh x ow = h x w and no segments, residual or per-channel floor (got %dx%d "
                           "stride %d pad %d,%d dilation %d cin %d nseg %d res %d lo %d)", d->kh, d->kw, d->stride, d->pad_h,
                           d->pad_w, d->dil, d->cin, d->nseg, d->res != nullptr, d->lo != nullptr);
    CT_REQUIRE(d->in && d->out && d->wpacked && d->scale && d->shift, "ct_conv2d_bf16_wino_fwd: null in / out / wpacked / scale / shift");
    CT_REQUIRE(workspace, "ct_conv2d_bf16_wino_fwd: workspace is null");
    CT_REQUIRE(d->in_coff >= 0 && d->in_coff + d->cin <= d->in_ctot && d->in_ctot % 8 == 0 && d->in_coff % 8 == 0,
               "ct_conv2d_bf16_wino_fwd: input slice %d + %d of %d channels (multiples of 8)", d->in_coff, d->cin, d->in_ctot);
    CT_REQUIRE(d->out_coff >= 0 && d->out_coff + d->cout <= d->out_ctot, "ct_conv2d_bf16_wino_fwd: output slice %d + %d of %d channels",
               d->out_coff, d->cout, d->out_ctot);
    CT_REQUIRE((reinterpret_cast<size_t>(d->in) & 15) == 0 && (reinterpret_cast<size_t>(d->out) & 3) == 0 &&
               (reinterpret_cast<size_t>(workspace) & 15) == 0 && (reinterpret_cast<size_t>(d->wpacked) & 15) == 0,
               "ct_conv2d_bf16_wino_fwd: in / wpacked / workspace must be 16-byte aligned, out 4-byte aligned");
    const long long hw = (long long)d->h * d->w;
    // (the third clause keeps tile x channel counts, which the kernels hold in int, far inside 31 bits)
    const long long tiles = (long long)d->batch * ((d->h + 3) / 4) * ((d->w + 3) / 4);
    if (d->batch * hw * d->in_ctot * 2 >= kMaxBufBytes || d->batch * hw * d->out_ctot * 2 >= kMaxBufBytes ||
        tiles * 18 * std::max(d->cin, d->cout) >= kMaxBufBytes)
        return ctdet::fail(CT_ERR_UNSUPPORTED, "ct_conv2d_bf16_wino_fwd: buffers beyond 32-bit offsets are not built (batch %d, "
                           "%dx%d, %d / %d channels): run the batch in chunks", d->batch, d->h, d->w, d->in_ctot, d->out_ctot);
    const Layout l = layout_of(d);
    const size_t need = l.lines_bytes + l.v_bytes + l.m_bytes;
    if (workspace_bytes < need)
        return ctdet::fail(CT_ERR_WORKSPACE, "ct_conv2d_bf16_wino_fwd: workspace_bytes is %zu, needs %zu", workspace_bytes, need);

    hipStream_t st = ctdet::as_stream(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    const unsigned* lines = d->in_absmax;
    if (!lines) {
        const int rc = ct_absmax_bf16_nhwc(d->in, d->batch, (int)hw, d->in_ctot, d->in_coff, d->cin, reinterpret_cast<unsigned*>(ws),
                                           stream);
        if (rc != CT_OK) return rc;
        lines = reinterpret_cast<const unsigned*>(ws);
    }
    FwdArgs a{};
    a.in = reinterpret_cast<const unsigned short*>(d->in);
    a.out = reinterpret_cast<unsigned short*>(d->out);
    a.U = reinterpret_cast<const unsigned char*>(d->wpacked);
    a.V = ws + l.lines_bytes;
    a.M = reinterpret_cast<float*>(ws + l.lines_bytes + l.v_bytes);
    a.in_lines = lines; a.out_lines = d->out_absmax;
    a.scale = d->scale; a.shift = d->shift;
    a.batch = d->batch; a.cin = d->cin; a.cout = d->cout; a.H = d->h; a.W = d->w;
    a.in_ctot = d->in_ctot; a.in_coff = d->in_coff; a.out_ctot = d->out_ctot; a.out_coff = d->out_coff;
    a.th = l.th; a.tw = l.tw; a.T = l.T; a.TB = l.TB; a.NB = l.NB; a.KS = l.KS;
    a.relu = d->relu;
    {
        CT_PROF("wbf_in", st);
        hipLaunchKernelGGL(wbf_in, dim3(l.TB, (l.KS + 3) / 4), dim3(256), 0, st, a);
        CT_LAUNCH_CHECK("wbf_in");
    }
    {
        CT_PROF("wbf_gemm", st);
        hipLaunchKernelGGL(wbf_gemm, dim3(((l.TB + 3) / 4) * ((l.NB + 3) / 4), 36), dim3(256), GEMM_LDS, st, a);
        CT_LAUNCH_CHECK("wbf_gemm");
    }
    {
        CT_PROF("wbf_out", st);
        const long long threads = (long long)l.T * (l.NB * 16);
        hipLaunchKernelGGL(wbf_out, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a);
        CT_LAUNCH_CHECK("wbf_out");
    }
    return CT_OK;
}
