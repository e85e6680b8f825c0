// Fused multi-tensor SGD step (train.py's `optimizer.step()` over the groups of utils/solver.py:6-33): weight decay,
// momentum, dampening, Nesterov and the parameter update of torch.optim.SGD in ONE pass over (param, grad, buf), for
// any number of tensors per call.  The tensor table and the first workgroup of every tensor travel in the kernel
// arguments (no device table, no staging copy, nothing read from the caller's array after the call returns), so a
// call is ceil(non-empty tensors / TENSORS_PER_LAUNCH) launches whatever the tensor sizes; a workgroup finds its
// tensor by a binary search over the prefix sums, which are scalar loads from the kernel-argument segment.
//
// Each workgroup owns one CHUNK of one tensor.  A tensor whose three pointers share their offset inside a 16-byte
// line is walked in 16-byte groups counted from the line that holds element 0: every whole group is a dwordx4 load /
// store, and only the first and the last group of the tensor can be partial (scalar, bounds-checked per element).
// Tensors whose pointers disagree are walked one dword per lane, still coalesced.  No byte outside
// [ptr, ptr + numel) is read or written; plain stores only.
//
// Every operation is rounded separately to fp32 (__fmul_rn / __fadd_rn / __fsub_rn, and -ffp-contract=off for the
// file), in the order include/ctdet.h states, so a NumPy float32 restatement reproduces the result bit for bit.
#include "ct_common.h"

#include <cstdint>

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = 8192;                 // elements per workgroup: 8 dwordx4 groups per lane, issued 4 at a time
constexpr int GROUPS = CHUNK / 4;           // 16-byte groups per chunk
constexpr int UNROLL = 4;
constexpr int TENSORS_PER_LAUNCH = 80;      // 80 * 40 B + 81 * 4 B + scalars = 3548 B of the 4096 B a launch may carry
constexpr int64_t MAX_NUMEL = 2147483647;

enum { F_FIRST = 1, F_VEC = 2, F_SHIFT = 4 /* bits 2-3: elements between the 16-byte line and element 0 */ };

struct Tensor {
    float* p;
    const float* g;
    float* b;
    int numel;
    float lr, wd;
    int flags;
};

struct Launch {
    Tensor t[TENSORS_PER_LAUNCH];
    int first_block[TENSORS_PER_LAUNCH + 1];
    int n;
    float momentum, one_minus_damp, grad_scale;
    int nesterov;
};
static_assert(sizeof(Tensor) == 40, "kernel-argument budget");
static_assert(sizeof(Launch) <= 4096, "kernel arguments are limited to 4 KiB");

struct Hyper {
    float lr, wd, momentum, omd, gs;
    bool first, nesterov;
};

// include/ctdet.h, ct_sgd_step: one rounding per line
__device__ inline void update(float& p, float g, float& b, const Hyper& h)
{
    g = __fmul_rn(g, h.gs);
    float d = g;
    if (h.wd != 0.f) d = __fadd_rn(g, __fmul_rn(h.wd, p));
    float step = d;
    if (h.momentum != 0.f) {
        b = h.first ? d : __fadd_rn(__fmul_rn(h.momentum, b), __fmul_rn(h.omd, d));
        step = h.nesterov ? __fadd_rn(d, __fmul_rn(h.momentum, b)) : b;
    }
    p = __fsub_rn(p, __fmul_rn(h.lr, step));
}

__device__ inline void update4(float4& p, float4 g, float4& b, const Hyper& h)
{
    update(p.x, g.x, b.x, h);
    update(p.y, g.y, b.y, h);
    update(p.z, g.z, b.z, h);
    update(p.w, g.w, b.w, h);
}

__global__ __launch_bounds__(THREADS) void sgd_multi_kernel(const Launch L)
{
    const int blk = blockIdx.x;
    int lo = 0, hi = L.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk >= L.first_block[mid]) lo = mid; else hi = mid;
    }
    const Tensor& T = L.t[lo];
    const int chunk = blk - L.first_block[lo];
    const int flags = T.flags;
    const int numel = T.numel;
    float* __restrict__ P = T.p;
    const float* __restrict__ G = T.g;
    float* __restrict__ B = T.b;
    Hyper h;
    h.lr = T.lr; h.wd = T.wd; h.momentum = L.momentum; h.omd = L.one_minus_damp; h.gs = L.grad_scale;
    h.first = flags & F_FIRST; h.nesterov = L.nesterov != 0;
    const bool has_buf = L.momentum != 0.f;
    const int tid = threadIdx.x;

    if (!(flags & F_VEC)) {
        // pointers disagree inside the 16-byte line: one dword per lane
        const int64_t base = (int64_t)chunk * CHUNK;
        for (int k = 0; k < CHUNK / THREADS; k += UNROLL) {
            float p[UNROLL], g[UNROLL], b[UNROLL];
            int64_t j[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                j[u] = base + (int64_t)(k + u) * THREADS + tid;
                if (j[u] < numel) {
                    p[u] = P[j[u]];
                    g[u] = G[j[u]];
                    b[u] = has_buf ? B[j[u]] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                if (j[u] < numel) {
                    update(p[u], g[u], b[u], h);
                    P[j[u]] = p[u];
                    if (has_buf) B[j[u]] = b[u];
                }
            }
        }
        return;
    }

    // Shifted coordinates: s = element index + shift, so s % 4 == 0 sits on a 16-byte line of all three arrays.
    // The tensor occupies s in [shift, end); group q covers s in [4q, 4q + 4).
    const int shift = (flags >> 2) & 3;
    const int64_t end = (int64_t)numel + shift;
    const int64_t q0 = (int64_t)chunk * GROUPS;
    const bool whole = (q0 * 4 >= shift) && ((q0 + GROUPS) * 4 <= end);
    if (whole) {
        for (int k = 0; k < GROUPS / THREADS; k += UNROLL) {
            float4 p[UNROLL], g[UNROLL], b[UNROLL];
            int64_t j[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                j[u] = (q0 + (int64_t)(k + u) * THREADS + tid) * 4 - shift;
                p[u] = *reinterpret_cast<const float4*>(P + j[u]);
                g[u] = *reinterpret_cast<const float4*>(G + j[u]);
                b[u] = has_buf ? *reinterpret_cast<const float4*>(B + j[u]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                update4(p[u], g[u], b[u], h);
                *reinterpret_cast<float4*>(P + j[u]) = p[u];
                if (has_buf) *reinterpret_cast<float4*>(B + j[u]) = b[u];
            }
        }
        return;
    }
    // first / last chunk of the tensor: whole groups stay 16-byte wide, a partial group goes element by element
    for (int k = 0; k < GROUPS / THREADS; ++k) {
        const int64_t s = (q0 + (int64_t)k * THREADS + tid) * 4;
        if (s >= end) break;
        if (s >= shift && s + 4 <= end) {
            const int64_t j = s - shift;
            float4 p = *reinterpret_cast<const float4*>(P + j);
            const float4 g = *reinterpret_cast<const float4*>(G + j);
            float4 b = has_buf ? *reinterpret_cast<const float4*>(B + j) : make_float4(0.f, 0.f, 0.f, 0.f);
            update4(p, g, b, h);
            *reinterpret_cast<float4*>(P + j) = p;
            if (has_buf) *reinterpret_cast<float4*>(B + j) = b;
        } else {
            for (int e = 0; e < 4; ++e) {
                const int64_t se = s + e;
                if (se < shift || se >= end) continue;
                const int64_t j = se - shift;
                float p = P[j];
                float b = has_buf ? B[j] : 0.f;
                update(p, G[j], b, h);
                P[j] = p;
                if (has_buf) B[j] = b;
            }
        }
    }
}

inline int line_offset(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

}  // namespace

extern "C" int ct_sgd_step(const ct_sgd_tensor* items, int n, float momentum, float dampening, int nesterov,
                           float grad_scale, ct_stream_t stream)
{
    using namespace ctdet;
    CT_REQUIRE(n >= 0, "ct_sgd_step: n = %d is negative", n);
    CT_REQUIRE(n == 0 || items != nullptr, "ct_sgd_step: items is NULL with n = %d", n);
    CT_REQUIRE(!nesterov || (momentum != 0.f && dampening == 0.f),
               "ct_sgd_step: nesterov needs a momentum and zero dampening (momentum %g, dampening %g)",
               (double)momentum, (double)dampening);
    for (int i = 0; i < n; ++i) {
        const ct_sgd_tensor& it = items[i];
        CT_REQUIRE(it.numel >= 0 && it.numel <= MAX_NUMEL, "ct_sgd_step: tensor %d has numel %lld (0 .. 2^31-1)", i,
                   (long long)it.numel);
        if (it.numel == 0) continue;        // a no-op whatever its pointers are (an empty tensor may have none)
        CT_REQUIRE(it.param && it.grad, "ct_sgd_step: tensor %d has a NULL %s", i, it.param ? "grad" : "param");
        CT_REQUIRE(momentum == 0.f || it.momentum_buf, "ct_sgd_step: tensor %d has no momentum_buf but momentum = %g",
                   i, (double)momentum);
        CT_REQUIRE(((reinterpret_cast<uintptr_t>(it.param) | reinterpret_cast<uintptr_t>(it.grad) |
                     reinterpret_cast<uintptr_t>(it.momentum_buf)) & 3) == 0,
                   "ct_sgd_step: tensor %d has a pointer that is not 4-byte aligned", i);
    }
    hipStream_t st = as_stream(stream);
    Launch L = {};
    L.momentum = momentum;
    L.one_minus_damp = 1.0f - dampening;
    L.grad_scale = grad_scale;
    L.nesterov = nesterov ? 1 : 0;
    const bool has_buf = momentum != 0.f;
    int i = 0;
    while (i < n) {
        int k = 0;
        int64_t blocks = 0;
        for (; i < n && k < TENSORS_PER_LAUNCH; ++i) {
            const ct_sgd_tensor& it = items[i];
            if (it.numel == 0) continue;
            const int off = line_offset(it.param);
            const bool vec = off == line_offset(it.grad) && (!has_buf || off == line_offset(it.momentum_buf));
            Tensor& t = L.t[k];
            t.p = it.param;
            t.g = it.grad;
            t.b = has_buf ? it.momentum_buf : nullptr;
            t.numel = (int)it.numel;
            t.lr = it.lr;
            t.wd = it.weight_decay;
            t.flags = (it.first_step ? F_FIRST : 0) | (vec ? F_VEC | off * F_SHIFT : 0);
            L.first_block[k] = (int)blocks;
            blocks += ceil_div<int64_t>(it.numel + (vec ? off : 0), CHUNK);
            ++k;
        }
        if (k == 0) break;
        for (int q = k; q <= TENSORS_PER_LAUNCH; ++q) L.first_block[q] = (int)blocks;
        L.n = k;
        CT_PROF("sgd_multi_kernel", st);
        hipLaunchKernelGGL(sgd_multi_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, L);
        CT_LAUNCH_CHECK("sgd_multi_kernel");
    }
    return CT_OK;
}

extern "C" int ct_sgd_tensors_per_launch(void) { return TENSORS_PER_LAUNCH; }
