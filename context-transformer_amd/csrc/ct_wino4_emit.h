// libctdet: the fused epilogue of one (cout, 4x4 output tile) of the F(4x4,3x3) kernels -- ct_wino4.hip (fused form)
// and ct_wino4s.hip (three-kernel bf16x3 form) apply the same arithmetic to their output-transformed sums.  Internal header.
#pragma once
#include "ct_common.h"
#include "ct_f16x2.h"

namespace ctdet {
namespace w4 {

typedef int emit_i32x4 __attribute__((ext_vector_type(4)));
constexpr int kEmitInvalidOff = 0x7FFFFFF0;

// y = A^T M A of one tile.  *scale + shift, residual, ReLU / per-channel floor (NaN propagates), the four 2x2 pooling
// windows a 4x4 tile holds, NCHW or head-scatter stores.  Args: any record with the epilogue fields of Wino4Args.
// ymul, ymul2: two factors applied to the sums in front of the per-channel scale (the f16x2 kernels' 2^-(eU + eV) in two exact
// halves, h2::unscale_for; 1, 1 elsewhere).  track / amax_run: the thread's
// running maximum of |v| over everything this call stores (ct_conv_desc.out_absmax; the caller folds it into the slot once, at
// the end of the kernel) -- a reference and a flag, not a nullable pointer, so that the value stays in a register.
template <class Args>
__device__ __forceinline__ void emit_tile4(const Args& a, const __amdgpu_buffer_rsrc_t rout,
                                           const __amdgpu_buffer_rsrc_t rres, const int n, const int ty, const int tx,
                                           const int co, const float (&y)[4][4], const float ymul, const float ymul2, const bool track, float& amax_run)
{
    const int OH = a.H, OW = a.W;                      // pad 1, stride 1: same spatial size
    const int oy = 4 * ty, ox = 4 * tx;
    const bool c1 = ox + 1 < OW, c2 = ox + 2 < OW, c3 = ox + 3 < OW;
    float sc = a.scale[co] * ymul2, sh = a.shift[co];      // (exact: a power of two of at most half the total exponent)
    float lo = a.lo ? a.lo[co] : (a.relu ? 0.f : -INFINITY);
    // The three per-channel values are needed by every row below, and every row sits behind its own `yy >= OH` test: left
    // alone, the compiler waits for these loads at the first use in EACH row block with s_waitcnt vmcnt(0) -- which from the
    // second row on also waits for the previous rows' STORES to drain (loads and stores share the counter).  Making the
    // values opaque here forces the one wait to this point, in front of all stores of the tile.
    asm volatile("" : "+v"(sc), "+v"(sh), "+v"(lo));
    float pl[2][2] = {{-INFINITY, -INFINITY}, {-INFINITY, -INFINITY}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int yy = oy + i;
        if (yy >= OH) continue;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (y[i][j] * ymul) * sc + sh;
        if (a.res) {
            const unsigned ro = (unsigned)(((((size_t)n * a.res_ctot + a.res_coff + co) * OH + yy) * OW + ox) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = j == 0 || (j == 1 ? c1 : j == 2 ? c2 : c3);
                const float r = __builtin_bit_cast(
                    float, __builtin_amdgcn_raw_buffer_load_b32(rres, ok ? ro + 4 * j : (unsigned)kEmitInvalidOff, 0, 0));
                v[j] = v[j] * a.res_scale + r;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] < lo ? lo : v[j];      // NaN propagates
        if (track) {
            ctdet::h2::track_absmax(amax_run, v[0]);
            if (c1) ctdet::h2::track_absmax(amax_run, v[1]);
            if (c2) ctdet::h2::track_absmax(amax_run, v[2]);
            if (c3) ctdet::h2::track_absmax(amax_run, v[3]);
        }
        pl[i >> 1][0] = fmaxf(pl[i >> 1][0], c1 ? fmaxf(v[0], v[1]) : v[0]);
        if (c2) pl[i >> 1][1] = fmaxf(pl[i >> 1][1], c3 ? fmaxf(v[2], v[3]) : v[2]);
        if (!a.write_full) continue;
        if (a.nseg > 0) {          // heads: permute(0,2,3,1) + view + cat of models/RFB_Net_vgg.py:239-248
#pragma unroll
            for (int g = 0; g < 3; ++g)
                if (g < a.nseg && co >= a.seg[g].co_begin && co < a.seg[g].co_end) {
                    float* dst = a.seg[g].ptr + (size_t)n * a.seg[g].img_stride + a.seg[g].base +
                                 (size_t)(yy * OW + ox) * a.seg[g].pix_stride + (co - a.seg[g].co_begin);
                    dst[0] = v[0];
                    if (c1) dst[a.seg[g].pix_stride] = v[1];
                    if (c2) dst[2 * a.seg[g].pix_stride] = v[2];
                    if (c3) dst[3 * a.seg[g].pix_stride] = v[3];
                }
            continue;
        }
        const unsigned oo = (unsigned)(((((size_t)n * a.out_ctot + a.out_coff + co) * OH + yy) * OW + ox) * 4);
        if (c3) {
            emit_i32x4 pk;
            pk.x = __builtin_bit_cast(int, v[0]);
            pk.y = __builtin_bit_cast(int, v[1]);
            pk.z = __builtin_bit_cast(int, v[2]);
            pk.w = __builtin_bit_cast(int, v[3]);
            __builtin_amdgcn_raw_buffer_store_b128(pk, rout, oo, 0, 0);
        } else {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v[0]), rout, oo, 0, 0);
            if (c1) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v[1]), rout, oo + 4, 0, 0);
            if (c2) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v[2]), rout, oo + 8, 0, 0);
        }
    }
    // a 4x4 output tile holds the four windows (2ty + pi, 2tx + pj) of MaxPool2d(2, 2[, ceil_mode])
    // (models/RFB_Net_vgg.py:328-330)
    if (a.pool_out) {
#pragma unroll
        for (int pi = 0; pi < 2; ++pi)
#pragma unroll
            for (int pj = 0; pj < 2; ++pj) {
                const int py = 2 * ty + pi, px = 2 * tx + pj;
                if (py < a.pool_oh && px < a.pool_ow && oy + 2 * pi < OH && ox + 2 * pj < OW)
                    a.pool_out[(((size_t)n * a.pool_ctot + a.pool_coff + co) * a.pool_oh + py) * a.pool_ow + px] = pl[pi][pj];
            }
    }
}

template <class Args>
__device__ __forceinline__ void emit_tile4(const Args& a, const __amdgpu_buffer_rsrc_t rout,
                                           const __amdgpu_buffer_rsrc_t rres, const int n, const int ty, const int tx,
                                           const int co, const float (&y)[4][4])
{
    float unused = 0.f;
    emit_tile4(a, rout, rres, n, ty, tx, co, y, 1.f, 1.f, false, unused);
}

// ---- The PLAIN epilogue (no residual, no per-channel floor, no head scatter) in two parts, for a kernel whose threads keep their
// tile while the output channel moves (ct_wino4f.hip: four quarters of 16 channels per item).  emit_tile4 above re-derives the
// tile's geometry per call and puts every row behind its own divergent test; here the geometry is worked out ONCE per tile
// (plan_tile4) and the per-channel part (emit_tile4_plain) is straight-line: same arithmetic per stored value, bit for bit.
struct Tile4Plan {
    unsigned row_full[4];      // byte offset of output row i within the buffer, for the channel the plan was made for -- where the
                               // row is stored whole (row and all four columns inside the map, full map wanted), else kEmitInvalidOff
    unsigned row0;             // byte offset of row 0, column 0 (inside the map for every live tile), else kEmitInvalidOff
    unsigned pool[2][2];       // byte offsets of the four pooling windows, kEmitInvalidOff for a window that is not written
    unsigned row_bytes, plane_bytes, pool_plane_bytes;
    bool r1, r2, r3, c1, c2, c3;       // rows / columns 1..3 of the tile inside the map (row 0 and column 0 always are)
};

// Args: H, W, relu, out_ctot, out_coff, write_full, pool_out, pool_ctot, pool_coff, pool_oh, pool_ow.  Offsets are 32-bit: the launchers
// keep the input / output / residual buffers below 2 GiB by chunking the batch (wino_check_launch), but NOT the pooled one -- a caller
// has to check its byte count against kMaxBufBytes itself and fall back to emit_tile4 above it (wino4f_launch does).
// A dead tile (live = false) gets no valid offset at all.
template <class Args>
__device__ __forceinline__ void plan_tile4(const Args& a, const bool live, const int n, const int ty, const int tx, const int co,
                                           Tile4Plan& g)
{
    const unsigned OH = (unsigned)a.H, OW = (unsigned)a.W, oy = 4u * (unsigned)ty, ox = 4u * (unsigned)tx;
    g.r1 = oy + 1 < OH; g.r2 = oy + 2 < OH; g.r3 = oy + 3 < OH;
    g.c1 = ox + 1 < OW; g.c2 = ox + 2 < OW; g.c3 = ox + 3 < OW;
    g.row_bytes = OW * 4u;
    g.plane_bytes = OH * OW * 4u;
    g.pool_plane_bytes = (unsigned)a.pool_oh * (unsigned)a.pool_ow * 4u;
    const unsigned row0 = ((((unsigned)n * (unsigned)a.out_ctot + (unsigned)a.out_coff + (unsigned)co) * OH + oy) * OW + ox) * 4u;
    g.row0 = live ? row0 : (unsigned)kEmitInvalidOff;
    const bool whole = live && a.write_full && g.c3;
    g.row_full[0] = whole ? row0 : (unsigned)kEmitInvalidOff;
    g.row_full[1] = whole && g.r1 ? row0 + g.row_bytes : (unsigned)kEmitInvalidOff;
    g.row_full[2] = whole && g.r2 ? row0 + 2u * g.row_bytes : (unsigned)kEmitInvalidOff;
    g.row_full[3] = whole && g.r3 ? row0 + 3u * g.row_bytes : (unsigned)kEmitInvalidOff;
    const unsigned POH = (unsigned)a.pool_oh, POW = (unsigned)a.pool_ow;
    const unsigned pbase = ((unsigned)n * (unsigned)a.pool_ctot + (unsigned)a.pool_coff + (unsigned)co) * POH;
#pragma unroll
    for (int pi = 0; pi < 2; ++pi)
#pragma unroll
        for (int pj = 0; pj < 2; ++pj) {
            const unsigned py = 2u * (unsigned)ty + pi, px = 2u * (unsigned)tx + pj;
            const bool ok = live && a.pool_out && py < POH && px < POW && oy + 2 * pi < OH && ox + 2 * pj < OW;
            g.pool[pi][pj] = ok ? ((pbase + py) * POW + px) * 4u : (unsigned)kEmitInvalidOff;
        }
}

// One (cout, tile): the plan's channel + dco (dco >= 0, the same for the whole wave), whose scale and shift the caller has loaded
// (ahead of the stores of the previous channels: a load issued behind them would wait for them -- loads and stores share the
// counter).  rout / rpool: descriptors of the full and the pooled output (rpool of zero bytes without one).  Per stored value the arithmetic of emit_tile4: (y * ymul) * sc + sh,
// v < lo ? lo : v (NaN propagates), the pooling maxima in the same order.  Elements outside the map are not branched around: the
// maxima take a copy in which such an element repeats an element of its tile that IS inside (its row's column 0 / 2, the row
// above) -- max(x, x) = x, so |v| is tracked and pooled over exactly the elements emit_tile4 visits -- and the stores use offsets
// the descriptor drops.  Only the tiles that cross the right edge store their rows piecewise, behind the one divergent test left.
template <class Args>
__device__ __forceinline__ void emit_tile4_plain(const Args& a, const Tile4Plan& g, const __amdgpu_buffer_rsrc_t rout,
                                                 const __amdgpu_buffer_rsrc_t rpool, const float scale_co, const float shift_co,
                                                 const int dco, const float (&y)[4][4], const float ymul, const float ymul2,
                                                 const bool track, float& amax_run)
{
    const float sc = scale_co * ymul2, sh = shift_co;
    const float lo = a.relu ? 0.f : -INFINITY;
    float v[4][4], w[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            t[j] = (y[i][j] * ymul) * sc + sh;
            t[j] = t[j] < lo ? lo : t[j];           // NaN propagates
        }
        // (values, not array elements, under the selects: a select between two elements becomes an indexed access)
        const float t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
        const float w1 = g.c1 ? t1 : t0, w2 = g.c2 ? t2 : t0, w3 = g.c3 ? t3 : w2;
        v[i][0] = t0; v[i][1] = t1; v[i][2] = t2; v[i][3] = t3;
        w[i][0] = t0; w[i][1] = w1; w[i][2] = w2; w[i][3] = w3;
    }
    if (track) {
        float rm[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rm[i] = __builtin_fabsf(w[i][0]);
#pragma unroll
            for (int j = 1; j < 4; ++j) ctdet::h2::track_absmax(rm[i], w[i][j]);
        }
        ctdet::h2::track_absmax(amax_run, rm[0]);
        ctdet::h2::track_absmax(amax_run, g.r1 ? rm[1] : 0.f);
        ctdet::h2::track_absmax(amax_run, g.r2 ? rm[2] : 0.f);
        ctdet::h2::track_absmax(amax_run, g.r3 ? rm[3] : 0.f);
    }
    if (a.write_full) {
        const unsigned so = (unsigned)dco * g.plane_bytes;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            emit_i32x4 pk;
            pk.x = __builtin_bit_cast(int, v[i][0]);
            pk.y = __builtin_bit_cast(int, v[i][1]);
            pk.z = __builtin_bit_cast(int, v[i][2]);
            pk.w = __builtin_bit_cast(int, v[i][3]);
            __builtin_amdgcn_raw_buffer_store_b128(pk, rout, g.row_full[i], so, 0);
        }
        if (!g.c3) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool ri = i == 0 || (i == 1 ? g.r1 : i == 2 ? g.r2 : g.r3);
                const unsigned o = ri ? g.row0 + i * g.row_bytes : (unsigned)kEmitInvalidOff;      // (invalid + 8 stays out of range)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v[i][0]), rout, o, so, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v[i][1]), rout, g.c1 ? o + 4 : (unsigned)kEmitInvalidOff, so, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v[i][2]), rout, g.c2 ? o + 8 : (unsigned)kEmitInvalidOff, so, 0);
            }
        }
    }
    // the four windows (2ty + pi, 2tx + pj) of MaxPool2d(2, 2[, ceil_mode]).  emit_tile4 skips a row below the map and takes v[0] /
    // v[2] alone where column 1 / 3 is outside; here such an operand repeats one already in the maximum.  (A window whose first
    // row or column is outside is not written.)
    if (a.pool_out) {
        const unsigned sp = (unsigned)dco * g.pool_plane_bytes;
        float L[4], R[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            L[i] = fmaxf(w[i][0], w[i][1]);
            R[i] = fmaxf(w[i][2], w[i][3]);
        }
        const float pl00 = fmaxf(fmaxf(-INFINITY, L[0]), g.r1 ? L[1] : L[0]);
        const float pl01 = fmaxf(fmaxf(-INFINITY, R[0]), g.r1 ? R[1] : R[0]);
        const float pl10 = fmaxf(fmaxf(-INFINITY, L[2]), g.r3 ? L[3] : L[2]);
        const float pl11 = fmaxf(fmaxf(-INFINITY, R[2]), g.r3 ? R[3] : R[2]);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, pl00), rpool, g.pool[0][0], sp, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, pl01), rpool, g.pool[0][1], sp, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, pl10), rpool, g.pool[1][0], sp, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, pl11), rpool, g.pool[1][1], sp, 0);
    }
}

}  // namespace w4
}  // namespace ctdet
