// Fused MultiBoxLoss_combined (layers/modules/multibox_loss_combined.py:76-122 of the reference): three launches
// forward (per-prior terms, per-image hard-negative selection, batch finish) and one backward.  No sort: the mining
// keys are non-negative floats, so their bit patterns order like unsigned integers and a four-pass radix select over
// the image's keys (held in LDS) finds the num_neg-th largest.  Every reduction runs in a fixed order -- no float
// atomics in this file -- so results are bit-identical from run to run and an image's selection does not depend on
// its batch mates.  Compiled with -ffp-contract=off.
// The localisation term is smooth-L1 on the encoded offsets or, in the IOU instantiations of the two per-prior kernels
// (ct_multibox_loss_fwd_loc / _bwd_loc), one of the IoU-family terms of ct_iou_loss.h on the decoded boxes.
// The classification terms are those cross-entropies over the mined sample or, with CT_CONF_FOCAL (ct_multibox_loss_fwd_terms
// / _bwd_terms), focal terms over every prior that is not ignored: focal_prior_kernel, loss_image_sum_kernel (no keys, no radix
// passes) and focal_bwd_kernel, which never read the conf row of a background prior.
#include "ct_common.h"
#include "ct_iou_loss.h"

#include <cmath>

#include <algorithm>
#include <cstdint>
#include <mutex>

namespace {

constexpr int ROW_THREADS = 256;        // per-prior kernels: 256 / G rows per workgroup, G lanes share one row of conf
constexpr int SEL_THREADS = 1024;       // selection: one workgroup per image
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int LDS_MAX_KEYS = 36864;     // 144 KiB of keys + the static arrays below stay inside the 160 KiB of a CU

// One "item" of a conf row: a 16-byte load when the row length is a multiple of 4 (rows are then 16-byte aligned),
// one float otherwise.  Lanes past the end of the row hold -inf, which neither the max nor the exp-sum sees.
template <bool VEC>
__device__ inline float4 load_item(const float* row, int i, int items)
{
    const float ninf = -INFINITY;
    if (i >= items) return make_float4(ninf, ninf, ninf, ninf);
    if (VEC) return reinterpret_cast<const float4*>(row)[i];
    return make_float4(row[i], ninf, ninf, ninf);
}

__device__ inline float max4(float4 v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }
__device__ inline float sumexp4(float4 v, float m)
{
    return (expf(v.x - m) + expf(v.y - m)) + (expf(v.z - m) + expf(v.w - m));
}

// max and sum(exp(x - max)) of one conf row, spread over the G lanes of a group (xor butterflies: every lane ends
// with the same value, the order of the additions is fixed by G alone).  v0 = the lane's first item, kept by the caller.
template <int G, bool VEC>
__device__ inline void row_max_sumexp(const float* row, int sub, int items, float4 v0, float& m, float& s)
{
    m = max4(v0);
    for (int i = sub + G; i < items; i += G) m = fmaxf(m, max4(load_item<VEC>(row, i, items)));
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    s = sumexp4(v0, m);
    for (int i = sub + G; i < items; i += G) s += sumexp4(load_item<VEC>(row, i, items), m);
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
}

__device__ inline int class_target(float label, int nfg)
{
    // labels.long().clamp_min(0); the upper clamp only keeps a malformed label inside the row
    const long long t = (long long)label;
    return (int)(t < 0 ? 0 : (t > nfg ? nfg : t));
}

__device__ inline float smooth_l1(float d)
{
    const float a = fabsf(d);
    return a < 1.f ? 0.5f * d * d : a - 0.5f;
}

// What the IOU instantiations need beyond the smooth-L1 arguments; the others ignore it.
struct LocArgs {
    const float4* priors;   // [P] centre form
    int num_priors;
    int kind;               // CT_LOC_*
    float var0, var1;
};

// The row pieces of loss_prior_kernel / loss_bwd_kernel below as functions, for the focal kernels.  The two cross-entropy
// kernels keep their own text: a call in place of it moved their instruction schedule, and their code is held to the bits
// and the time they had before the focal form came.
// The localisation term of one row: the smooth-L1 sum of every row or, with IOU, the IoU-family term of a positive row of
// non-zero weight and 0 of any other row, whose loc, loc_t and prior are then not read (la.kind is uniform over the launch).
template <bool IOU>
__device__ inline float loc_row_forward(const float4* __restrict__ loc, const float4* __restrict__ loc_t, long long r,
                                        float2 ct, const LocArgs& la)
{
    float l1 = 0.f;
    if (!IOU) {
        const float4 a = loc[r], b = loc_t[r];
        l1 = (smooth_l1(a.x - b.x) + smooth_l1(a.y - b.y)) + (smooth_l1(a.z - b.z) + smooth_l1(a.w - b.w));
    } else if (ct.x > 0.f && ct.y != 0.f) {
        l1 = ctdet::iou_row_forward(loc[r], loc_t[r], la.priors[r % la.num_priors], la.var0, la.var1, la.kind).loss;
    }
    return l1;
}

// ... and its gradient times g0 * weight: zeros for a row that is not positive or has weight 0, which is not read
template <bool IOU>
__device__ inline float4 loc_row_backward(const float4* __restrict__ loc, const float4* __restrict__ loc_t, long long row,
                                          float2 ct, float g0, const LocArgs& la)
{
    float4 dl = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ct.x > 0.f && ct.y != 0.f) {
        const float4 a = loc[row], b = loc_t[row];
        const float gl = g0 * ct.y;
        if (!IOU) {
            dl.x = gl * fminf(fmaxf(a.x - b.x, -1.f), 1.f);
            dl.y = gl * fminf(fmaxf(a.y - b.y, -1.f), 1.f);
            dl.z = gl * fminf(fmaxf(a.z - b.z, -1.f), 1.f);
            dl.w = gl * fminf(fmaxf(a.w - b.w, -1.f), 1.f);
        } else {
            const float4 p = la.priors[row % la.num_priors];
            const ctdet::IouRow ir = ctdet::iou_row_forward(a, b, p, la.var0, la.var1, la.kind);
            ctdet::iou_row_backward(ir, p, la.var0, la.var1, la.kind, gl, dl.x, dl.y, dl.z, dl.w);
        }
    }
    return dl;
}

// drow = gw * (softmax(crow) - onehot(col)) from the row's max m and exp-sum s, each lane its own items; or zeros
template <int G, bool VEC>
__device__ inline void write_dconf_row(const float* crow, float* drow, int sub, int items, float4 v0, float m, float s,
                                       int col, float gw)
{
    for (int i = sub; i < items; i += G) {
        const float4 v = i == sub ? v0 : load_item<VEC>(crow, i, items);
        const int c0 = VEC ? 4 * i : i;
        const float dx = gw * (expf(v.x - m) / s - (c0 == col ? 1.f : 0.f));
        if (VEC) {
            const float dy = gw * (expf(v.y - m) / s - (c0 + 1 == col ? 1.f : 0.f));
            const float dz = gw * (expf(v.z - m) / s - (c0 + 2 == col ? 1.f : 0.f));
            const float dw = gw * (expf(v.w - m) / s - (c0 + 3 == col ? 1.f : 0.f));
            reinterpret_cast<float4*>(drow)[i] = make_float4(dx, dy, dz, dw);
        } else {
            drow[i] = dx;
        }
    }
}

template <int G, bool VEC>
__device__ inline void zero_dconf_row(float* drow, int sub, int items)
{
    for (int i = sub; i < items; i += G) {
        if (VEC) reinterpret_cast<float4*>(drow)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        else drow[i] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------- focal terms
// CT_CONF_FOCAL (include/ctdet.h, ct_multibox_loss_fwd_terms).  For a target of probability p, with m the SUM OF THE OTHER
// probabilities and ce = -log p taken from the logits: FL = a m^gamma ce, dFL/dz_j = c (p_j - [j = t]) with
// c = a m^gamma (1 - gamma p r), r = log p / m (-1 at m = 0).
struct FocalArgs {
    float gamma;
    float a_fg, a_bg;       // alpha and 1 - alpha; both 1 when alpha < 0
};

// m^gamma with 0^0 = 1; gamma is uniform over the launch, and the usual 2 needs no powf
__device__ inline float focal_weight(float m, float gamma)
{
    return gamma == 0.f ? 1.f : gamma == 2.f ? m * m : powf(m, gamma);
}

__device__ inline float focal_grad_factor(float a, float gamma, float p, float m, float ce)
{
    const float r = m == 0.f ? -1.f : -ce / m;
    return a * focal_weight(m, gamma) * (1.f - gamma * p * r);
}

// softmax and both cross-entropies of one objectness row, in the arithmetic of loss_prior_kernel / loss_bwd_kernel
struct ObjRow { float s0, s1, ce0, ce1; };
__device__ inline ObjRow obj_row(float2 o)
{
    const float om = fmaxf(o.x, o.y);
    const float e0 = expf(o.x - om), e1 = expf(o.y - om);
    const float olse = logf(e0 + e1);
    return {e0 / (e0 + e1), e1 / (e0 + e1), olse - (o.x - om), olse - (o.y - om)};
}

__device__ inline float sumexp4_except(float4 v, float m, int c0, int col)
{
    return ((c0 == col ? 0.f : expf(v.x - m)) + (c0 + 1 == col ? 0.f : expf(v.y - m))) +
           ((c0 + 2 == col ? 0.f : expf(v.z - m)) + (c0 + 3 == col ? 0.f : expf(v.w - m)));
}

// sum(exp(x - m)) over one conf row WITHOUT column col, spread over the group like row_max_sumexp
template <int G, bool VEC>
__device__ inline float row_sumexp_except(const float* row, int sub, int items, float4 v0, float m, int col)
{
    float s = 0.f;
    for (int i = sub; i < items; i += G)
        s += sumexp4_except(i == sub ? v0 : load_item<VEC>(row, i, items), m, VEC ? 4 * i : i, col);
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// What a foreground row (target column col of conf) hands to the class term: ce = -log p_t on the fused logits,
// p = s_1 q_t and m = s_0 + s_1 * (sum of the other q), every lane of the group with the same values.
struct FgRow { float mx, s, ce, p, m; };
template <int G, bool VEC>
__device__ inline FgRow fg_row(const float* crow, int sub, int items, float4 v0, int col, const ObjRow& o)
{
    FgRow f;
    row_max_sumexp<G, VEC>(crow, sub, items, v0, f.mx, f.s);
    const float others = row_sumexp_except<G, VEC>(crow, sub, items, v0, f.mx, col);
    const float zt = crow[col];
    f.ce = ((f.mx + logf(f.s)) - zt) + o.ce1;
    f.p = o.s1 * (expf(zt - f.mx) / f.s);
    f.m = o.s0 + o.s1 * (others / f.s);
    return f;
}

// ---------------------------------------------------------------------------------------------------- per prior
// ws[row] = (localisation term, objectness CE, mining key, class CE).  The localisation term is the smooth-L1 sum of
// every row or, with IOU, the IoU-family term of a positive row of non-zero weight and 0 of any other row, whose loc,
// loc_t and prior are then not read (kind is uniform over the launch).  The class CE is taken on the fused logits
// z = [o0 + lse(conf), o1 + conf_1 ..]; since logsumexp(z) = lse(conf) + logsumexp(o0, o1), it is
// CE_obj(0) for target 0 and (lse(conf) - conf_t) + CE_obj(1) for a foreground target.
template <int G, bool VEC, bool IOU>
__global__ __launch_bounds__(ROW_THREADS) void loss_prior_kernel(
    const float4* __restrict__ loc, const float* __restrict__ conf, const float2* __restrict__ obj,
    const float4* __restrict__ loc_t, const float2* __restrict__ conf_t, const uint8_t* __restrict__ obj_t,
    long long rows, int nfg, float4* __restrict__ ws, LocArgs la)
{
    const int sub = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    const bool live = row < rows;
    const long long r = live ? row : rows - 1;          // dead groups recompute the last row and write nothing
    const float* crow = conf + r * nfg;
    const int items = VEC ? nfg / 4 : nfg;
    const float4 v0 = load_item<VEC>(crow, sub, items);
    float m, s;
    row_max_sumexp<G, VEC>(crow, sub, items, v0, m, s);
    if (sub != 0 || !live) return;

    const float2 ct = conf_t[r];
    float l1 = 0.f;
    if (!IOU) {
        const float4 a = loc[r], b = loc_t[r];
        l1 = (smooth_l1(a.x - b.x) + smooth_l1(a.y - b.y)) + (smooth_l1(a.z - b.z) + smooth_l1(a.w - b.w));
    } else if (ct.x > 0.f && ct.y != 0.f) {
        l1 = ctdet::iou_row_forward(loc[r], loc_t[r], la.priors[r % la.num_priors], la.var0, la.var1, la.kind).loss;
    }
    const float2 o = obj[r];
    const float om = fmaxf(o.x, o.y);
    const float olse = logf(expf(o.x - om) + expf(o.y - om));
    const float ce0 = olse - (o.x - om), ce1 = olse - (o.y - om);
    const bool ot = obj_t[r] != 0;
    const float ce_obj = ot ? ce1 : ce0;
    const float key = (!ot && ce_obj > 0.f) ? ce_obj : 0.f;            // never -0 or NaN: the select orders bit patterns
    const int t = class_target(ct.x, nfg);
    float ce_cls = ce0;
    if (t > 0) ce_cls = ((m + logf(s)) - crow[t - 1]) + ce1;
    ws[r] = make_float4(l1, ce_obj, key, ce_cls);
}

// The focal form: ws[row] = (localisation term, objectness FL, 0, class FL).  The row weight is known before any logit
// is loaded (w = weight for label >= 0, 0 for an ignored row; nothing is mined), so a row of weight 0 reads neither obj
// nor conf, and conf is read by the groups of foreground rows alone: a background target has p = s_0, m = s_1.
template <int G, bool VEC, bool IOU>
__global__ __launch_bounds__(ROW_THREADS) void focal_prior_kernel(
    const float4* __restrict__ loc, const float* __restrict__ conf, const float2* __restrict__ obj,
    const float4* __restrict__ loc_t, const float2* __restrict__ conf_t, const uint8_t* __restrict__ obj_t,
    long long rows, int nfg, float4* __restrict__ ws, LocArgs la, FocalArgs fa)
{
    const int sub = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;                            // whole groups leave together; shuffles stay inside a group
    const float2 ct = conf_t[row];
    const float wr = ct.x >= 0.f ? ct.y : 0.f;
    const int t = class_target(ct.x, nfg);
    ObjRow o = {0.f, 0.f, 0.f, 0.f};
    FgRow f = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (wr != 0.f) o = obj_row(obj[row]);
    if (wr != 0.f && t > 0) {
        const float* crow = conf + row * nfg;
        const int items = VEC ? nfg / 4 : nfg;
        f = fg_row<G, VEC>(crow, sub, items, load_item<VEC>(crow, sub, items), t - 1, o);
    }
    if (sub != 0) return;

    const float l1 = loc_row_forward<IOU>(loc, loc_t, row, ct, la);
    float fl_obj = 0.f, fl_cls = 0.f;
    if (wr != 0.f) {
        fl_obj = fl_cls = fa.a_bg * focal_weight(o.s1, fa.gamma) * o.ce0;         // target 0 of either term: nearly every row
        if (obj_t[row] != 0) fl_obj = fa.a_fg * focal_weight(o.s0, fa.gamma) * o.ce1;
        if (t > 0) fl_cls = fa.a_fg * focal_weight(f.m, fa.gamma) * f.ce;
    }
    ws[row] = make_float4(l1, fl_obj, 0.f, fl_cls);
}

// ---------------------------------------------------------------------------------------------------- selection
__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Sum over the workgroup in a fixed order: butterflies inside each wave, then the 16 wave totals in index order.
__device__ inline double block_sum(double v, double* red /*[SEL_WAVES]*/)
{
    v = wave_sum(v);
    __syncthreads();                                    // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < SEL_WAVES; ++i) t += red[i];
    return t;
}

// Count `digit` in hist for the lanes with `valid`.  The top digit of a mining key is nearly the same for every
// prior, so up to two rounds first peel the leading lane's digit off with one atomic for the whole wave.
// Integer atomics only: the counts do not depend on their order.
__device__ inline void hist_add(unsigned* hist, unsigned digit, bool valid)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long act = __ballot(valid);
        if (act == 0) return;
        const int leader = __ffsll((long long)act) - 1;
        const unsigned d0 = __shfl(digit, leader);
        const unsigned long long same = __ballot(valid && digit == d0);
        if (lane == leader) atomicAdd(&hist[d0], (unsigned)__popcll(same));
        if (digit == d0) valid = false;
    }
    if (valid) atomicAdd(&hist[digit], 1u);
}

template <bool LDS>
__global__ __launch_bounds__(SEL_THREADS) void loss_select_kernel(
    const float4* __restrict__ ws, const float2* __restrict__ conf_t, int P, int negpos_ratio,
    float* __restrict__ w_out, long long* __restrict__ num_pos_out, double* __restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) unsigned skeys[];    // [P] when LDS
    __shared__ unsigned hist[256];
    __shared__ double red[SEL_WAVES];
    __shared__ int wcnt[2][SEL_WAVES];
    __shared__ unsigned s_prefix, s_krem, s_eq;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)blockIdx.x * P;
    ws += base; conf_t += base; w_out += base;
    auto key_at = [&](int i) -> unsigned { return LDS ? skeys[i] : __float_as_uint(ws[i].z); };

    // num_pos = long(sum of weight * pos): fp64 in a fixed order, rounded once to fp32, truncated
    double acc = 0.0;
    for (int i = tid; i < P; i += SEL_THREADS) {
        const float2 ct = conf_t[i];
        if (ct.x > 0.f) acc += (double)ct.y;
        if (LDS) skeys[i] = __float_as_uint(ws[i].z);
    }
    const float possum = (float)block_sum(acc, red);
    const long long num_pos = (long long)possum;
    long long kk = (long long)negpos_ratio * num_pos;
    kk = kk < 0 ? 0 : (kk > P - 1 ? P - 1 : kk);
    const unsigned k = (unsigned)kk;                    // hard negatives to draw, < P

    // radix select: after the four passes `thr` is the k-th largest key, `krem` of the `eq` priors equal to it are drawn
    unsigned thr = 0, krem = k, eq = 0;
    if (k > 0) {
        unsigned mask = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();                            // also orders the skeys writes above before the first read
            for (int i0 = 0; i0 < P; i0 += SEL_THREADS) {
                const int i = i0 + tid;
                const unsigned key = i < P ? key_at(i) : 0u;
                hist_add(hist, (key >> shift) & 255u, i < P && (key & mask) == thr);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned rem = krem, d = 255;
                for (;; --d) {
                    const unsigned c = hist[d];
                    if (rem <= c || d == 0) { s_eq = c; break; }
                    rem -= c;
                }
                s_prefix = thr | (d << shift);
                s_krem = rem;
            }
            __syncthreads();
            thr = s_prefix; krem = s_krem; eq = s_eq;
            mask |= 255u << shift;
        }
    }
    const bool ranked = k > 0 && krem < eq;             // the cut-off falls inside a tie group: lowest indices first

    double sl = 0.0, sc = 0.0, so = 0.0;
    unsigned run = 0;                                   // priors equal to thr seen in earlier chunks
    int buf = 0;
    for (int i0 = 0; i0 < P; i0 += SEL_THREADS) {
        const int i = i0 + tid;
        const bool in = i < P;
        const unsigned key = in ? key_at(i) : 0u;
        const bool iseq = in && k > 0 && key == thr;
        bool neg = in && k > 0 && key > thr;
        if (!ranked) {
            neg = neg || iseq;
        } else {
            const unsigned long long mm = __ballot(iseq);
            if (lane == 0) wcnt[buf][wave] = __popcll(mm);
            __syncthreads();
            unsigned before = 0, total = 0;
            for (int v = 0; v < SEL_WAVES; ++v) {
                const unsigned c = (unsigned)wcnt[buf][v];
                before += v < wave ? c : 0u;
                total += c;
            }
            const unsigned rank = run + before + (unsigned)__popcll(mm & ((1ull << lane) - 1ull));
            neg = neg || (iseq && rank < krem);
            run += total;
            buf ^= 1;
        }
        if (in) {
            const float2 ct = conf_t[i];
            const bool pos = ct.x > 0.f;
            const float w = (pos || neg) ? ct.y : 0.f;
            w_out[i] = w;
            if (pos || w != 0.f) {
                const float4 v = ws[i];
                if (pos) sl += (double)(v.x * ct.y);
                if (w != 0.f) { so += (double)(v.y * w); sc += (double)(v.w * w); }
            }
        }
    }
    sl = block_sum(sl, red);
    sc = block_sum(sc, red);
    so = block_sum(so, red);
    if (tid == 0) {
        partial[blockIdx.x * 3 + 0] = sl;
        partial[blockIdx.x * 3 + 1] = sc;
        partial[blockIdx.x * 3 + 2] = so;
        num_pos_out[blockIdx.x] = num_pos;
    }
}

// The per-image pass of the focal form: nothing is selected, so there are no keys in LDS and no radix passes.  num_pos, the
// three sums and their block_sum order are loss_select_kernel's; w = weight for label >= 0 and 0 for an ignored row.
__global__ __launch_bounds__(SEL_THREADS) void loss_image_sum_kernel(
    const float4* __restrict__ ws, const float2* __restrict__ conf_t, int P, float* __restrict__ w_out,
    long long* __restrict__ num_pos_out, double* __restrict__ partial)
{
    __shared__ double red[SEL_WAVES];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * P;
    ws += base; conf_t += base; w_out += base;

    double acc = 0.0, sl = 0.0, sc = 0.0, so = 0.0;
    for (int i = tid; i < P; i += SEL_THREADS) {
        const float2 ct = conf_t[i];
        const bool pos = ct.x > 0.f;
        const float w = ct.x >= 0.f ? ct.y : 0.f;
        if (pos) acc += (double)ct.y;
        w_out[i] = w;
        if (pos || w != 0.f) {
            const float4 v = ws[i];
            if (pos) sl += (double)(v.x * ct.y);
            if (w != 0.f) { so += (double)(v.y * w); sc += (double)(v.w * w); }
        }
    }
    const float possum = (float)block_sum(acc, red);    // long(sum of weight * pos), as loss_select_kernel rounds it
    sl = block_sum(sl, red);
    sc = block_sum(sc, red);
    so = block_sum(so, red);
    if (tid == 0) {
        partial[blockIdx.x * 3 + 0] = sl;
        partial[blockIdx.x * 3 + 1] = sc;
        partial[blockIdx.x * 3 + 2] = so;
        num_pos_out[blockIdx.x] = (long long)possum;
    }
}

// sums = (sum loc, sum cls, sum obj) over the images in index order, n = sum of num_pos
__global__ void loss_finish_kernel(const double* __restrict__ partial, const long long* __restrict__ num_pos, int batch,
                                   float* __restrict__ sums, long long* __restrict__ n)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a = 0.0, b = 0.0, c = 0.0;
    long long t = 0;
    for (int i = 0; i < batch; ++i) {
        a += partial[i * 3 + 0]; b += partial[i * 3 + 1]; c += partial[i * 3 + 2];
        t += num_pos[i];
    }
    sums[0] = (float)a; sums[1] = (float)b; sums[2] = (float)c;
    n[0] = t;
}

// ---------------------------------------------------------------------------------------------------- backward
// With p = softmax(fused logits), s = softmax(obj), q = softmax(conf): p_0 = s_0 and p_k = s_1 q_k, so
//   d cls / d conf_k = [t >= 1] q_k - [t = k],   d cls / d obj = s - onehot(t >= 1),   d obj-loss / d obj = s - onehot(obj_t).
// A row with w = 0 (then weight * pos = 0 too) is written as zeros without looking at its logits.
template <int G, bool VEC, bool IOU>
__global__ __launch_bounds__(ROW_THREADS) void loss_bwd_kernel(
    const float4* __restrict__ loc, const float* __restrict__ conf, const float2* __restrict__ obj,
    const float4* __restrict__ loc_t, const float2* __restrict__ conf_t, const uint8_t* __restrict__ obj_t,
    const float* __restrict__ w, const float* __restrict__ g, long long rows, int nfg,
    float4* __restrict__ dloc, float* __restrict__ dconf, float2* __restrict__ dobj, LocArgs la)
{
    const int sub = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;                            // whole groups leave together; shuffles stay inside a group
    const float wr = w[row];
    const float2 ct = conf_t[row];
    const int t = class_target(ct.x, nfg);
    const float g0 = g[0], g1 = g[1], g2 = g[2];
    const float* crow = conf + row * nfg;
    float* drow = dconf + row * nfg;
    const int items = VEC ? nfg / 4 : nfg;

    if (wr != 0.f && t > 0) {
        const float4 v0 = load_item<VEC>(crow, sub, items);
        float m, s;
        row_max_sumexp<G, VEC>(crow, sub, items, v0, m, s);
        const float gw = g1 * wr;
        for (int i = sub; i < items; i += G) {
            const float4 v = i == sub ? v0 : load_item<VEC>(crow, i, items);
            const int c0 = VEC ? 4 * i : i;
            const float dx = gw * (expf(v.x - m) / s - (c0 == t - 1 ? 1.f : 0.f));
            if (VEC) {
                const float dy = gw * (expf(v.y - m) / s - (c0 + 1 == t - 1 ? 1.f : 0.f));
                const float dz = gw * (expf(v.z - m) / s - (c0 + 2 == t - 1 ? 1.f : 0.f));
                const float dw = gw * (expf(v.w - m) / s - (c0 + 3 == t - 1 ? 1.f : 0.f));
                reinterpret_cast<float4*>(drow)[i] = make_float4(dx, dy, dz, dw);
            } else {
                drow[i] = dx;
            }
        }
    } else {
        for (int i = sub; i < items; i += G) {
            if (VEC) reinterpret_cast<float4*>(drow)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            else drow[i] = 0.f;
        }
    }
    if (sub != 0) return;

    float4 dl = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ct.x > 0.f && ct.y != 0.f) {
        const float4 a = loc[row], b = loc_t[row];
        const float gl = g0 * ct.y;
        if (!IOU) {
            dl.x = gl * fminf(fmaxf(a.x - b.x, -1.f), 1.f);
            dl.y = gl * fminf(fmaxf(a.y - b.y, -1.f), 1.f);
            dl.z = gl * fminf(fmaxf(a.z - b.z, -1.f), 1.f);
            dl.w = gl * fminf(fmaxf(a.w - b.w, -1.f), 1.f);
        } else {
            const float4 p = la.priors[row % la.num_priors];
            const ctdet::IouRow ir = ctdet::iou_row_forward(a, b, p, la.var0, la.var1, la.kind);
            ctdet::iou_row_backward(ir, p, la.var0, la.var1, la.kind, gl, dl.x, dl.y, dl.z, dl.w);
        }
    }
    dloc[row] = dl;

    float2 dob = make_float2(0.f, 0.f);
    if (wr != 0.f) {
        const float2 o = obj[row];
        const float om = fmaxf(o.x, o.y);
        const float e0 = expf(o.x - om), e1 = expf(o.y - om);
        const float p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
        const bool ot = obj_t[row] != 0;
        const float go = g2 * wr, gc = g1 * wr;
        dob.x = go * (p0 - (ot ? 0.f : 1.f)) + gc * (p0 - (t == 0 ? 1.f : 0.f));
        dob.y = go * (p1 - (ot ? 1.f : 0.f)) + gc * (p1 - (t == 0 ? 0.f : 1.f));
    }
    dobj[row] = dob;
}

// The focal form: the same shape, each term times its factor c.  The class factor scales dconf, so every lane of a row
// of non-zero weight evaluates the objectness row; a background row (t = 0) writes zeros to dconf and does not read conf.
template <int G, bool VEC, bool IOU>
__global__ __launch_bounds__(ROW_THREADS) void focal_bwd_kernel(
    const float4* __restrict__ loc, const float* __restrict__ conf, const float2* __restrict__ obj,
    const float4* __restrict__ loc_t, const float2* __restrict__ conf_t, const uint8_t* __restrict__ obj_t,
    const float* __restrict__ w, const float* __restrict__ g, long long rows, int nfg,
    float4* __restrict__ dloc, float* __restrict__ dconf, float2* __restrict__ dobj, LocArgs la, FocalArgs fa)
{
    const int sub = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;                            // whole groups leave together; shuffles stay inside a group
    const float wr = w[row];
    const float2 ct = conf_t[row];
    const int t = class_target(ct.x, nfg);
    const float g0 = g[0], g1 = g[1], g2 = g[2];
    const float* crow = conf + row * nfg;
    float* drow = dconf + row * nfg;
    const int items = VEC ? nfg / 4 : nfg;

    ObjRow o = {0.f, 0.f, 0.f, 0.f};
    float c_bg = 0.f;                                   // the factor of a background target, of either term: nearly every row
    if (wr != 0.f) {
        o = obj_row(obj[row]);
        c_bg = focal_grad_factor(fa.a_bg, fa.gamma, o.s0, o.s1, o.ce0);
    }
    float c_cls = c_bg;
    if (wr != 0.f && t > 0) {
        const float4 v0 = load_item<VEC>(crow, sub, items);
        const FgRow f = fg_row<G, VEC>(crow, sub, items, v0, t - 1, o);
        c_cls = focal_grad_factor(fa.a_fg, fa.gamma, f.p, f.m, f.ce);
        write_dconf_row<G, VEC>(crow, drow, sub, items, v0, f.mx, f.s, t - 1, (g1 * wr) * c_cls);
    } else {
        zero_dconf_row<G, VEC>(drow, sub, items);
    }
    if (sub != 0) return;

    dloc[row] = loc_row_backward<IOU>(loc, loc_t, row, ct, g0, la);

    float2 dob = make_float2(0.f, 0.f);
    if (wr != 0.f) {
        const bool ot = obj_t[row] != 0;
        float c_obj = c_bg;
        if (ot) c_obj = focal_grad_factor(fa.a_fg, fa.gamma, o.s1, o.s0, o.ce1);
        const float go = (g2 * wr) * c_obj, gc = (g1 * wr) * c_cls;
        dob.x = go * (o.s0 - (ot ? 0.f : 1.f)) + gc * (o.s0 - (t == 0 ? 1.f : 0.f));
        dob.y = go * (o.s1 - (ot ? 1.f : 0.f)) + gc * (o.s1 - (t == 0 ? 0.f : 1.f));
    }
    dobj[row] = dob;
}

size_t ws_rows_bytes(int batch, int num_priors) { return ctdet::align_up((size_t)batch * num_priors * sizeof(float4), 256); }

// lanes per conf row: the smallest supported group that holds the row in one item per lane (64 = a whole wave, looping)
int group_for(int items) { return items <= 4 ? 4 : items <= 8 ? 8 : items <= 16 ? 16 : 64; }

}  // namespace

extern "C" size_t ct_multibox_loss_workspace_bytes(int batch, int num_priors, int num_classes)
{
    (void)num_classes;
    if (batch <= 0 || num_priors <= 0) return 0;
    return ws_rows_bytes(batch, num_priors) + ctdet::align_up((size_t)batch * 3 * sizeof(double), 256);
}

// launch KERNEL<G, VEC, IOU> for the row length nfg; `vec` (16-byte loads allowed), `rows`, `nfg`, `st` come from the caller
#define CT_LOSS_DISPATCH(KERNEL, IOU, ...)                                                                       \
    do {                                                                                                         \
        const int G = group_for(vec ? nfg / 4 : nfg);                                                            \
        const long long nblk = (rows + ROW_THREADS / G - 1) / (ROW_THREADS / G);                                 \
        CT_REQUIRE(nblk < 0x7FFFFFFFLL, "%s: too many priors", #KERNEL);                                         \
        const dim3 grid((unsigned)nblk), block(ROW_THREADS);                                                     \
        if (vec) {                                                                                               \
            if (G == 4) hipLaunchKernelGGL((KERNEL<4, true, IOU>), grid, block, 0, st, __VA_ARGS__);             \
            else if (G == 8) hipLaunchKernelGGL((KERNEL<8, true, IOU>), grid, block, 0, st, __VA_ARGS__);        \
            else if (G == 16) hipLaunchKernelGGL((KERNEL<16, true, IOU>), grid, block, 0, st, __VA_ARGS__);      \
            else hipLaunchKernelGGL((KERNEL<64, true, IOU>), grid, block, 0, st, __VA_ARGS__);                   \
        } else {                                                                                                 \
            if (G == 4) hipLaunchKernelGGL((KERNEL<4, false, IOU>), grid, block, 0, st, __VA_ARGS__);            \
            else if (G == 8) hipLaunchKernelGGL((KERNEL<8, false, IOU>), grid, block, 0, st, __VA_ARGS__);       \
            else if (G == 16) hipLaunchKernelGGL((KERNEL<16, false, IOU>), grid, block, 0, st, __VA_ARGS__);     \
            else hipLaunchKernelGGL((KERNEL<64, false, IOU>), grid, block, 0, st, __VA_ARGS__);                  \
        }                                                                                                        \
        CT_LAUNCH_CHECK(#KERNEL);                                                                                \
    } while (0)

namespace {

// the checks of the _loc entries, before any HIP call; `fn` names the entry in the message
int check_loc_args(const char* fn, const float* priors, int loc_loss, float var0, float var1)
{
    CT_REQUIRE(loc_loss >= CT_LOC_SMOOTH_L1 && loc_loss <= CT_LOC_CIOU,
               "%s: loc_loss=%d (0 smooth-L1, 1 iou, 2 giou, 3 diou, 4 ciou)", fn, loc_loss);
    CT_REQUIRE(std::isfinite(var0) && std::isfinite(var1) && var0 > 0.f && var1 > 0.f,
               "%s: variances (%g, %g) must be positive and finite", fn, (double)var0, (double)var1);
    if (loc_loss != CT_LOC_SMOOTH_L1) {
        CT_REQUIRE(priors != nullptr, "%s: loc_loss=%d needs priors (null pointer)", fn, loc_loss);
        CT_REQUIRE((reinterpret_cast<uintptr_t>(priors) & 15) == 0, "%s: priors must be 16-byte aligned", fn);
    }
    return CT_OK;
}

// the classification terms of a call: CT_CONF_CE, or CT_CONF_FOCAL with its constants
struct ConfArgs {
    int kind;
    FocalArgs focal;
};

// the checks of the _terms entries, before any HIP call -> la, ca
int check_terms(const char* fn, const ct_loss_terms* terms, LocArgs& la, ConfArgs& ca)
{
    CT_REQUIRE(terms != nullptr, "%s: terms is a null pointer", fn);
    if (const int rc = check_loc_args(fn, terms->priors, terms->loc_loss, terms->var0, terms->var1)) return rc;
    CT_REQUIRE(terms->conf_loss == CT_CONF_CE || terms->conf_loss == CT_CONF_FOCAL, "%s: conf_loss=%d (0 ce, 1 focal)", fn,
               terms->conf_loss);
    const float gamma = terms->focal_gamma, alpha = terms->focal_alpha;
    if (terms->conf_loss == CT_CONF_FOCAL) {
        CT_REQUIRE(std::isfinite(gamma) && gamma >= 0.f, "%s: focal_gamma=%g must be finite and >= 0", fn, (double)gamma);
        CT_REQUIRE(alpha <= 1.f, "%s: focal_alpha=%g must be in [0, 1], or negative for none", fn, (double)alpha);   // no NaN
    }
    la = {terms->loc_loss == CT_LOC_SMOOTH_L1 ? nullptr : (const float4*)terms->priors, 0, terms->loc_loss, terms->var0,
          terms->var1};
    ca = {terms->conf_loss, {gamma, alpha < 0.f ? 1.f : alpha, alpha < 0.f ? 1.f : 1.f - alpha}};
    return CT_OK;
}

// the shared launcher of the forward entries: three launches whatever la.kind and ca.kind
int loss_fwd(const char* fn, const float* loc, const float* conf, const float* obj, const float* loc_t,
             const float* conf_t, const uint8_t* obj_t, int batch, int num_priors, int num_classes, int negpos_ratio,
             float* sums, long long* num_pos, long long* n, float* w, void* ws, size_t ws_bytes, ct_stream_t stream,
             LocArgs la, const ConfArgs& ca)
{
    CT_REQUIRE(loc && conf && obj && loc_t && conf_t && obj_t && sums && num_pos && n && w && ws, "%s: null pointer", fn);
    CT_REQUIRE(batch > 0 && num_priors > 0, "%s: batch=%d num_priors=%d", fn, batch, num_priors);
    CT_REQUIRE(num_classes >= 2, "%s: num_classes=%d (at least background and one class)", fn, num_classes);
    CT_REQUIRE(negpos_ratio >= 0, "%s: negpos_ratio=%d", fn, negpos_ratio);
    const size_t need = ct_multibox_loss_workspace_bytes(batch, num_priors, num_classes);
    if (ws_bytes < need) return ctdet::fail(CT_ERR_WORKSPACE, "%s: workspace %zu < %zu", fn, ws_bytes, need);
    hipStream_t st = ctdet::as_stream(stream);
    const long long rows = (long long)batch * num_priors;
    const int nfg = num_classes - 1;
    float4* rows_ws = (float4*)ws;
    double* partial = (double*)((char*)ws + ws_rows_bytes(batch, num_priors));
    la.num_priors = num_priors;

    const bool vec = nfg % 4 == 0 && (reinterpret_cast<uintptr_t>(conf) & 15) == 0;
    if (ca.kind == CT_CONF_FOCAL) {
        if (la.kind == CT_LOC_SMOOTH_L1)
            CT_LOSS_DISPATCH(focal_prior_kernel, false, (const float4*)loc, conf, (const float2*)obj, (const float4*)loc_t,
                             (const float2*)conf_t, obj_t, rows, nfg, rows_ws, la, ca.focal);
        else
            CT_LOSS_DISPATCH(focal_prior_kernel, true, (const float4*)loc, conf, (const float2*)obj, (const float4*)loc_t,
                             (const float2*)conf_t, obj_t, rows, nfg, rows_ws, la, ca.focal);
        hipLaunchKernelGGL(loss_image_sum_kernel, dim3(batch), dim3(SEL_THREADS), 0, st, (const float4*)rows_ws,
                           (const float2*)conf_t, num_priors, w, num_pos, partial);
        CT_LAUNCH_CHECK("loss_image_sum_kernel");
    } else {
        if (la.kind == CT_LOC_SMOOTH_L1)
            CT_LOSS_DISPATCH(loss_prior_kernel, false, (const float4*)loc, conf, (const float2*)obj, (const float4*)loc_t,
                             (const float2*)conf_t, obj_t, rows, nfg, rows_ws, la);
        else
            CT_LOSS_DISPATCH(loss_prior_kernel, true, (const float4*)loc, conf, (const float2*)obj, (const float4*)loc_t,
                             (const float2*)conf_t, obj_t, rows, nfg, rows_ws, la);

        if (num_priors <= LDS_MAX_KEYS) {
            const size_t lds = (size_t)num_priors * sizeof(unsigned);
            static std::once_flag once;
            static hipError_t attr = hipSuccess;
            std::call_once(once, [] {
                attr = hipFuncSetAttribute((const void*)loss_select_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           LDS_MAX_KEYS * (int)sizeof(unsigned));
            });
            CT_HIP(attr);
            hipLaunchKernelGGL(loss_select_kernel<true>, dim3(batch), dim3(SEL_THREADS), lds, st, (const float4*)rows_ws,
                               (const float2*)conf_t, num_priors, negpos_ratio, w, num_pos, partial);
        } else {
            hipLaunchKernelGGL(loss_select_kernel<false>, dim3(batch), dim3(SEL_THREADS), 0, st, (const float4*)rows_ws,
                               (const float2*)conf_t, num_priors, negpos_ratio, w, num_pos, partial);
        }
        CT_LAUNCH_CHECK("loss_select_kernel");
    }
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)partial, (const long long*)num_pos,
                       batch, sums, n);
    CT_LAUNCH_CHECK("loss_finish_kernel");
    return CT_OK;
}

int loss_bwd(const char* fn, const float* loc, const float* conf, const float* obj, const float* loc_t,
             const float* conf_t, const uint8_t* obj_t, const float* w, const float* g, int batch, int num_priors,
             int num_classes, float* dloc, float* dconf, float* dobj, ct_stream_t stream, LocArgs la, const ConfArgs& ca)
{
    CT_REQUIRE(loc && conf && obj && loc_t && conf_t && obj_t && w && g && dloc && dconf && dobj, "%s: null pointer", fn);
    CT_REQUIRE(batch > 0 && num_priors > 0, "%s: batch=%d num_priors=%d", fn, batch, num_priors);
    CT_REQUIRE(num_classes >= 2, "%s: num_classes=%d (at least background and one class)", fn, num_classes);
    hipStream_t st = ctdet::as_stream(stream);
    const long long rows = (long long)batch * num_priors;
    const int nfg = num_classes - 1;
    la.num_priors = num_priors;
    const bool vec = nfg % 4 == 0 && ((reinterpret_cast<uintptr_t>(conf) | reinterpret_cast<uintptr_t>(dconf)) & 15) == 0;
    if (ca.kind == CT_CONF_FOCAL) {
        if (la.kind == CT_LOC_SMOOTH_L1)
            CT_LOSS_DISPATCH(focal_bwd_kernel, false, (const float4*)loc, conf, (const float2*)obj, (const float4*)loc_t,
                             (const float2*)conf_t, obj_t, w, g, rows, nfg, (float4*)dloc, dconf, (float2*)dobj, la, ca.focal);
        else
            CT_LOSS_DISPATCH(focal_bwd_kernel, true, (const float4*)loc, conf, (const float2*)obj, (const float4*)loc_t,
                             (const float2*)conf_t, obj_t, w, g, rows, nfg, (float4*)dloc, dconf, (float2*)dobj, la, ca.focal);
    } else if (la.kind == CT_LOC_SMOOTH_L1) {
        CT_LOSS_DISPATCH(loss_bwd_kernel, false, (const float4*)loc, conf, (const float2*)obj, (const float4*)loc_t,
                         (const float2*)conf_t, obj_t, w, g, rows, nfg, (float4*)dloc, dconf, (float2*)dobj, la);
    } else {
        CT_LOSS_DISPATCH(loss_bwd_kernel, true, (const float4*)loc, conf, (const float2*)obj, (const float4*)loc_t,
                         (const float2*)conf_t, obj_t, w, g, rows, nfg, (float4*)dloc, dconf, (float2*)dobj, la);
    }
    return CT_OK;
}

const LocArgs SMOOTH_L1_ARGS = {nullptr, 0, CT_LOC_SMOOTH_L1, 0.f, 0.f};
const ConfArgs CE_ARGS = {CT_CONF_CE, {0.f, 1.f, 1.f}};

}  // namespace

extern "C" int ct_multibox_loss_fwd(const float* loc, const float* conf, const float* obj, const float* loc_t,
                                    const float* conf_t, const uint8_t* obj_t, int batch, int num_priors,
                                    int num_classes, int negpos_ratio, float* sums, long long* num_pos, long long* n,
                                    float* w, void* ws, size_t ws_bytes, ct_stream_t stream)
{
    return loss_fwd("ct_multibox_loss_fwd", loc, conf, obj, loc_t, conf_t, obj_t, batch, num_priors, num_classes,
                    negpos_ratio, sums, num_pos, n, w, ws, ws_bytes, stream, SMOOTH_L1_ARGS, CE_ARGS);
}

extern "C" int ct_multibox_loss_bwd(const float* loc, const float* conf, const float* obj, const float* loc_t,
                                    const float* conf_t, const uint8_t* obj_t, const float* w, const float* g,
                                    int batch, int num_priors, int num_classes, float* dloc, float* dconf,
                                    float* dobj, ct_stream_t stream)
{
    return loss_bwd("ct_multibox_loss_bwd", loc, conf, obj, loc_t, conf_t, obj_t, w, g, batch, num_priors, num_classes,
                    dloc, dconf, dobj, stream, SMOOTH_L1_ARGS, CE_ARGS);
}

extern "C" int ct_multibox_loss_fwd_loc(const float* loc, const float* conf, const float* obj, const float* loc_t,
                                        const float* conf_t, const uint8_t* obj_t, int batch, int num_priors,
                                        int num_classes, int negpos_ratio, float* sums, long long* num_pos, long long* n,
                                        float* w, void* ws, size_t ws_bytes, ct_stream_t stream, const float* priors,
                                        int loc_loss, float var0, float var1)
{
    if (const int rc = check_loc_args("ct_multibox_loss_fwd_loc", priors, loc_loss, var0, var1)) return rc;
    const LocArgs la = {loc_loss == CT_LOC_SMOOTH_L1 ? nullptr : (const float4*)priors, 0, loc_loss, var0, var1};
    return loss_fwd("ct_multibox_loss_fwd_loc", loc, conf, obj, loc_t, conf_t, obj_t, batch, num_priors, num_classes,
                    negpos_ratio, sums, num_pos, n, w, ws, ws_bytes, stream, la, CE_ARGS);
}

extern "C" int ct_multibox_loss_bwd_loc(const float* loc, const float* conf, const float* obj, const float* loc_t,
                                        const float* conf_t, const uint8_t* obj_t, const float* w, const float* g,
                                        int batch, int num_priors, int num_classes, float* dloc, float* dconf,
                                        float* dobj, ct_stream_t stream, const float* priors, int loc_loss, float var0,
                                        float var1)
{
    if (const int rc = check_loc_args("ct_multibox_loss_bwd_loc", priors, loc_loss, var0, var1)) return rc;
    const LocArgs la = {loc_loss == CT_LOC_SMOOTH_L1 ? nullptr : (const float4*)priors, 0, loc_loss, var0, var1};
    return loss_bwd("ct_multibox_loss_bwd_loc", loc, conf, obj, loc_t, conf_t, obj_t, w, g, batch, num_priors,
                    num_classes, dloc, dconf, dobj, stream, la, CE_ARGS);
}

extern "C" int ct_multibox_loss_fwd_terms(const float* loc, const float* conf, const float* obj, const float* loc_t,
                                          const float* conf_t, const uint8_t* obj_t, int batch, int num_priors,
                                          int num_classes, int negpos_ratio, float* sums, long long* num_pos, long long* n,
                                          float* w, void* ws, size_t ws_bytes, ct_stream_t stream,
                                          const ct_loss_terms* terms)
{
    LocArgs la;
    ConfArgs ca;
    if (const int rc = check_terms("ct_multibox_loss_fwd_terms", terms, la, ca)) return rc;
    return loss_fwd("ct_multibox_loss_fwd_terms", loc, conf, obj, loc_t, conf_t, obj_t, batch, num_priors, num_classes,
                    negpos_ratio, sums, num_pos, n, w, ws, ws_bytes, stream, la, ca);
}

extern "C" int ct_multibox_loss_bwd_terms(const float* loc, const float* conf, const float* obj, const float* loc_t,
                                          const float* conf_t, const uint8_t* obj_t, const float* w, const float* g,
                                          int batch, int num_priors, int num_classes, float* dloc, float* dconf,
                                          float* dobj, ct_stream_t stream, const ct_loss_terms* terms)
{
    LocArgs la;
    ConfArgs ca;
    if (const int rc = check_terms("ct_multibox_loss_bwd_terms", terms, la, ca)) return rc;
    return loss_bwd("ct_multibox_loss_bwd_terms", loc, conf, obj, loc_t, conf_t, obj_t, w, g, batch, num_priors,
                    num_classes, dloc, dconf, dobj, stream, la, ca);
}
