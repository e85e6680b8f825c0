// Exponential moving average of the weights ("model averaging") next to the fused SGD step of ct_optim.hip:
//   ct_ema_begin      one thread: decides on the device whether this step is averaged (the non-finite guard of
//                     ct_grad_norm_clip skipped it or not), advances the update count and evaluates the warm-up decay;
//   ct_sgd_step_ema   ct_sgd_step / ct_sgd_step_clipped with one more array: the average is updated from the new
//                     parameter value while it is still in a register (7 array passes instead of 5 + 3);
//   ct_ema_update     the same line for tensors the optimizer did not touch (no gradient, BatchNorm statistics);
//   ct_tensor_swap    exchanges two sets of tensors in place (evaluate with the averaged weights, then swap back).
// The three multi-tensor kernels walk their tensors as sgd_multi_kernel does (ct_multi_tensor.h): the table travels in
// the kernel arguments, a workgroup owns one CHUNK of one tensor found by a binary search over prefix sums, tensors
// whose pointers share their offset inside a 16-byte line move in dwordx4 accesses with a scalar first / last group,
// any other tensor one dword per lane.  No byte outside [ptr, ptr + numel) is read or written; plain vector stores.
// Every operation is rounded separately to fp32 (-ffp-contract=off for the file), in the order include/ctdet.h states.
#include "ct_common.h"
#include "ct_multi_tensor.h"

#include <climits>
#include <cstdint>

namespace {

using namespace ctdet::mt;

// include/ctdet.h, ct_sgd_step_ema: ema = d * ema + (1 - d) * x, three roundings
__device__ inline float ema_of(float e, float x, float d, float om)
{
    return __fadd_rn(__fmul_rn(d, e), __fmul_rn(om, x));
}

template <class V> __device__ inline V ld(const float* p);
template <> __device__ inline float ld<float>(const float* p) { return *p; }
template <> __device__ inline float4 ld<float4>(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline void st(float* p, float v) { *p = v; }
__device__ inline void st(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
template <class V> __device__ inline V zero();
template <> __device__ inline float zero<float>() { return 0.f; }
template <> __device__ inline float4 zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// One chunk of one tensor.  Op supplies Regs<V>, load<V>(j), apply(Regs<V>&) and store(j, Regs<V>) for V = float and
// float4; j is the element index of the access, which for float4 sits on a 16-byte line of every array of the tensor.
// The accesses are those of sgd_multi_kernel: loads of UNROLL groups are issued before the first result is stored.
template <class Op>
__device__ inline void walk(const Op& op, int chunk, int numel, int flags, int tid)
{
    if (!(flags & F_VEC)) {
        // pointers disagree inside the 16-byte line: one dword per lane
        const int64_t base = (int64_t)chunk * CHUNK;
        for (int k = 0; k < CHUNK / THREADS; k += UNROLL) {
            typename Op::template Regs<float> r[UNROLL];
            int64_t j[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                j[u] = base + (int64_t)(k + u) * THREADS + tid;
                if (j[u] < numel) r[u] = op.template load<float>(j[u]);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                if (j[u] < numel) {
                    op.apply(r[u]);
                    op.store(j[u], r[u]);
                }
            }
        }
        return;
    }
    // Shifted coordinates: s = element index + shift, so s % 4 == 0 sits on a 16-byte line of every array.
    // The tensor occupies s in [shift, end); group q covers s in [4q, 4q + 4).
    const int shift = (flags >> 2) & 3;
    const int64_t end = (int64_t)numel + shift;
    const int64_t q0 = (int64_t)chunk * GROUPS;
    const bool whole = (q0 * 4 >= shift) && ((q0 + GROUPS) * 4 <= end);
    if (whole) {
        for (int k = 0; k < GROUPS / THREADS; k += UNROLL) {
            typename Op::template Regs<float4> r[UNROLL];
            int64_t j[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                j[u] = (q0 + (int64_t)(k + u) * THREADS + tid) * 4 - shift;
                r[u] = op.template load<float4>(j[u]);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                op.apply(r[u]);
                op.store(j[u], r[u]);
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
            typename Op::template Regs<float4> r = op.template load<float4>(j);
            op.apply(r);
            op.store(j, r);
        } else {
            for (int e = 0; e < 4; ++e) {
                const int64_t se = s + e;
                if (se < shift || se >= end) continue;
                const int64_t j = se - shift;
                typename Op::template Regs<float> r = op.template load<float>(j);
                op.apply(r);
                op.store(j, r);
            }
        }
    }
}

// flags of a tensor whose non-NULL pointers are `ptrs`: F_VEC and the shift when they agree inside the 16-byte line
template <int N>
inline int vec_flags(const void* const (&ptrs)[N])
{
    int off = -1;
    for (const void* p : ptrs) {
        if (!p) continue;
        if (off < 0) off = line_offset(p);
        else if (off != line_offset(p)) return 0;
    }
    return off < 0 ? 0 : (F_VEC | off * F_SHIFT);
}

inline int64_t chunks_of(int64_t numel, int flags)
{
    return ctdet::ceil_div<int64_t>(numel + ((flags & F_VEC) ? (flags >> 2) & 3 : 0), CHUNK);
}

// ------------------------------------------------------------------------------------------------ ct_ema_begin
__global__ void ema_begin_kernel(ct_ema_state* state, float decay, float warmup, const ct_clip_state* clip)
{
    // include/ctdet.h, ct_ema_begin: one rounding per line; plain loads and stores of the 16 bytes
    const int n = state->updates;
    const int applied = clip ? (clip->finite != 0 ? 1 : 0) : 1;
    if (!applied) {
        state->applied = 0;
        return;
    }
    float d = decay;
    if (warmup != 0.f) {
        const float nf = (float)n;
        const float num = __fadd_rn(1.0f, nf);
        const float den = __fadd_rn(warmup, nf);
        d = fminf(decay, __fdiv_rn(num, den));
    }
    state->updates = n == INT_MAX ? n : n + 1;
    state->decay = d;
    state->one_minus = __fsub_rn(1.0f, d);
    state->applied = 1;
}

// --------------------------------------------------------------------------------------------- ct_sgd_step_ema
constexpr int SGD_EMA_PER_LAUNCH = 77;      // 77 * 48 B + 78 * 4 B + scalars = 4048 B of the 4096 B a launch may carry

struct SgdEmaTensor {
    float* p;
    const float* g;
    float* b;
    float* e;
    int numel;
    float lr, wd;
    int flags;
};

struct SgdEmaLaunch {
    SgdEmaTensor t[SGD_EMA_PER_LAUNCH];
    int first_block[SGD_EMA_PER_LAUNCH + 1];
    int n;
    float momentum, one_minus_damp, grad_scale;
    int nesterov;
    const ct_clip_state* clip;              // sgd_multi_kernel_ema<true> only
    const ct_ema_state* ema;
};
static_assert(sizeof(SgdEmaTensor) == 48, "kernel-argument budget");
static_assert(sizeof(SgdEmaLaunch) <= 4096, "kernel arguments are limited to 4 KiB");

struct SgdEmaOp {
    float* __restrict__ P;
    const float* __restrict__ G;
    float* __restrict__ B;
    float* __restrict__ E;
    Hyper h;
    bool has_buf, averaged;
    float d, om;
    template <class V> struct Regs { V p, g, b, e; };

    template <class V> __device__ Regs<V> load(int64_t j) const
    {
        Regs<V> r;
        r.p = ld<V>(P + j);
        r.g = ld<V>(G + j);
        r.b = has_buf ? ld<V>(B + j) : zero<V>();
        r.e = averaged ? ld<V>(E + j) : zero<V>();
        return r;
    }
    __device__ void apply(Regs<float>& r) const
    {
        update(r.p, r.g, r.b, h);
        r.e = ema_of(r.e, r.p, d, om);
    }
    __device__ void apply(Regs<float4>& r) const
    {
        update4(r.p, r.g, r.b, h);
        r.e.x = ema_of(r.e.x, r.p.x, d, om);
        r.e.y = ema_of(r.e.y, r.p.y, d, om);
        r.e.z = ema_of(r.e.z, r.p.z, d, om);
        r.e.w = ema_of(r.e.w, r.p.w, d, om);
    }
    template <class V> __device__ void store(int64_t j, const Regs<V>& r) const
    {
        st(P + j, r.p);
        if (has_buf) st(B + j, r.b);
        if (averaged) st(E + j, r.e);
    }
};

// CLIP as in sgd_multi_kernel.  The average moves iff the step ran and ct_ema_begin opened an update.
template <bool CLIP>
__global__ __launch_bounds__(THREADS) void sgd_multi_kernel_ema(const SgdEmaLaunch L)
{
    const int blk = blockIdx.x;
    const int lo = owner_of(L.first_block, L.n, blk);
    const SgdEmaTensor& T = L.t[lo];
    const int chunk = blk - L.first_block[lo];
    const int flags = T.flags;
    const int numel = T.numel;
    const int tid = threadIdx.x;
    SgdEmaOp op;
    op.P = T.p; op.G = T.g; op.B = T.b; op.E = T.e;
    op.h.lr = T.lr; op.h.wd = T.wd; op.h.momentum = L.momentum; op.h.omd = L.one_minus_damp; op.h.gs = L.grad_scale;
    op.h.first = flags & F_FIRST; op.h.nesterov = L.nesterov != 0;
    op.has_buf = L.momentum != 0.f;

    if (CLIP) {
        if (L.clip->finite == 0) {
            // Skipped step, as in sgd_multi_kernel<true>: +0 to a first-step buffer, nothing else -- the average stays.
            if (op.has_buf && op.h.first) {
                const int shift = (flags & F_VEC) ? (flags >> 2) & 3 : 0;
                const int64_t s0 = (int64_t)chunk * CHUNK;
                const int64_t j0 = s0 > shift ? s0 - shift : 0;
                const int64_t j1 = s0 + CHUNK - shift < numel ? s0 + CHUNK - shift : numel;
                for (int64_t j = j0 + tid; j < j1; j += THREADS) op.B[j] = 0.f;
            }
            return;
        }
        op.h.gs = __fmul_rn(L.grad_scale, L.clip->coef);
    }
    op.averaged = L.ema->applied != 0;
    op.d = L.ema->decay;
    op.om = L.ema->one_minus;
    walk(op, chunk, numel, flags, tid);
}

// ------------------------------------------------------------------------- ct_ema_update and ct_tensor_swap
constexpr int PAIRS_PER_LAUNCH = 140;       // 140 * 24 B + 141 * 4 B + 16 B = 3940 B

struct Pair {
    float* a;                               // ema   | a
    float* b;                               // src   | b   (ema_multi_kernel only reads it)
    int numel;
    int flags;
};

struct PairLaunch {
    Pair t[PAIRS_PER_LAUNCH];
    int first_block[PAIRS_PER_LAUNCH + 1];
    int n;
    const ct_ema_state* ema;                // ema_multi_kernel only
};
static_assert(sizeof(Pair) == 24, "kernel-argument budget");
static_assert(sizeof(PairLaunch) <= 4096, "kernel arguments are limited to 4 KiB");

struct EmaOp {
    float* __restrict__ E;
    const float* __restrict__ S;
    float d, om;
    template <class V> struct Regs { V e, s; };

    template <class V> __device__ Regs<V> load(int64_t j) const
    {
        Regs<V> r;
        r.e = ld<V>(E + j);
        r.s = ld<V>(S + j);
        return r;
    }
    __device__ void apply(Regs<float>& r) const { r.e = ema_of(r.e, r.s, d, om); }
    __device__ void apply(Regs<float4>& r) const
    {
        r.e.x = ema_of(r.e.x, r.s.x, d, om);
        r.e.y = ema_of(r.e.y, r.s.y, d, om);
        r.e.z = ema_of(r.e.z, r.s.z, d, om);
        r.e.w = ema_of(r.e.w, r.s.w, d, om);
    }
    template <class V> __device__ void store(int64_t j, const Regs<V>& r) const { st(E + j, r.e); }
};

struct SwapOp {
    float* __restrict__ A;
    float* __restrict__ B;
    template <class V> struct Regs { V a, b; };

    template <class V> __device__ Regs<V> load(int64_t j) const
    {
        Regs<V> r;
        r.a = ld<V>(A + j);
        r.b = ld<V>(B + j);
        return r;
    }
    template <class V> __device__ void apply(Regs<V>&) const {}
    template <class V> __device__ void store(int64_t j, const Regs<V>& r) const
    {
        st(A + j, r.b);
        st(B + j, r.a);
    }
};

__global__ __launch_bounds__(THREADS) void ema_multi_kernel(const PairLaunch L)
{
    if (L.ema->applied == 0) return;        // the step was skipped: the averages stay
    const int blk = blockIdx.x;
    const int lo = owner_of(L.first_block, L.n, blk);
    const Pair& T = L.t[lo];
    EmaOp op;
    op.E = T.a; op.S = T.b;
    op.d = L.ema->decay;
    op.om = L.ema->one_minus;
    walk(op, blk - L.first_block[lo], T.numel, T.flags, threadIdx.x);
}

__global__ __launch_bounds__(THREADS) void tensor_swap_kernel(const PairLaunch L)
{
    const int blk = blockIdx.x;
    const int lo = owner_of(L.first_block, L.n, blk);
    const Pair& T = L.t[lo];
    SwapOp op;
    op.A = T.a; op.B = T.b;
    walk(op, blk - L.first_block[lo], T.numel, T.flags, threadIdx.x);
}

int check_state(const char* who, const ct_ema_state* state)
{
    CT_REQUIRE(state != nullptr, "%s: the ema state is NULL", who);
    CT_REQUIRE((reinterpret_cast<uintptr_t>(state) & 3) == 0, "%s: the ema state is not 4-byte aligned", who);
    return CT_OK;
}

// The launches of ct_ema_update (ema != nullptr) and ct_tensor_swap over pairs the caller has checked
template <class Item, class GetA, class GetB>
int launch_pairs(const Item* items, int n, const ct_ema_state* ema, GetA get_a, GetB get_b, ct_stream_t stream)
{
    using namespace ctdet;
    hipStream_t st = as_stream(stream);
    PairLaunch L = {};
    L.ema = ema;
    int i = 0;
    while (i < n) {
        int k = 0;
        int64_t blocks = 0;
        for (; i < n && k < PAIRS_PER_LAUNCH; ++i) {
            if (items[i].numel == 0) continue;
            Pair& t = L.t[k];
            t.a = get_a(items[i]);
            t.b = get_b(items[i]);
            t.numel = (int)items[i].numel;
            const void* const ptrs[2] = {t.a, t.b};
            t.flags = vec_flags(ptrs);
            L.first_block[k] = (int)blocks;
            blocks += chunks_of(t.numel, t.flags);
            ++k;
        }
        if (k == 0) break;
        for (int q = k; q <= PAIRS_PER_LAUNCH; ++q) L.first_block[q] = (int)blocks;
        L.n = k;
        if (ema) {
            CT_PROF("ema_multi_kernel", st);
            hipLaunchKernelGGL(ema_multi_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, L);
            CT_LAUNCH_CHECK("ema_multi_kernel");
        } else {
            CT_PROF("tensor_swap_kernel", st);
            hipLaunchKernelGGL(tensor_swap_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, L);
            CT_LAUNCH_CHECK("tensor_swap_kernel");
        }
    }
    return CT_OK;
}

// n and the table pointer, as every multi-tensor entry checks them
int check_table(const char* who, const void* items, int n)
{
    CT_REQUIRE(n >= 0, "%s: n = %d is negative", who, n);
    CT_REQUIRE(n == 0 || items != nullptr, "%s: items is NULL with n = %d", who, n);
    return CT_OK;
}

}  // namespace

extern "C" int ct_ema_begin(ct_ema_state* state_dev, float decay, float warmup, const ct_clip_state* clip_dev_or_null,
                            ct_stream_t stream)
{
    using namespace ctdet;
    const char* who = "ct_ema_begin";
    if (const int rc = check_state(who, state_dev)) return rc;
    CT_REQUIRE(decay >= 0.f && decay < 1.f, "%s: decay = %g is outside [0, 1)", who, (double)decay);
    CT_REQUIRE(warmup == 0.f || (warmup >= 1.f && warmup <= 3.0e38f), "%s: warmup = %g is neither 0 (off) nor >= 1", who,
               (double)warmup);
    CT_REQUIRE((reinterpret_cast<uintptr_t>(clip_dev_or_null) & 3) == 0, "%s: the clip state is not 4-byte aligned", who);
    hipStream_t st = as_stream(stream);
    CT_PROF("ema_begin_kernel", st);
    hipLaunchKernelGGL(ema_begin_kernel, dim3(1), dim3(1), 0, st, state_dev, decay, warmup, clip_dev_or_null);
    CT_LAUNCH_CHECK("ema_begin_kernel");
    return CT_OK;
}

extern "C" int ct_sgd_ema_tensors_per_launch(void) { return SGD_EMA_PER_LAUNCH; }

extern "C" int ct_sgd_step_ema(const ct_sgd_ema_tensor* items, int n, float momentum, float dampening, int nesterov,
                               float grad_scale, const ct_clip_state* clip, const ct_ema_state* ema_dev,
                               ct_stream_t stream)
{
    using namespace ctdet;
    const char* who = "ct_sgd_step_ema";
    if (const int rc = check_table(who, items, n)) return rc;
    CT_REQUIRE(!nesterov || (momentum != 0.f && dampening == 0.f),
               "%s: nesterov needs a momentum and zero dampening (momentum %g, dampening %g)", who, (double)momentum,
               (double)dampening);
    if (const int rc = check_state(who, ema_dev)) return rc;
    CT_REQUIRE((reinterpret_cast<uintptr_t>(clip) & 3) == 0, "%s: the clip state is not 4-byte aligned", who);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const ct_sgd_ema_tensor& it = items[i];
        CT_REQUIRE(it.numel >= 0 && it.numel <= MAX_NUMEL, "%s: tensor %d has numel %lld (0 .. 2^31-1)", who, i,
                   (long long)it.numel);
        if (it.numel == 0) continue;        // a no-op whatever its pointers are (an empty tensor may have none)
        CT_REQUIRE(it.param && it.grad, "%s: tensor %d has a NULL %s", who, i, it.param ? "grad" : "param");
        CT_REQUIRE(momentum == 0.f || it.momentum_buf, "%s: tensor %d has no momentum_buf but momentum = %g", who, i,
                   (double)momentum);
        CT_REQUIRE(it.ema, "%s: tensor %d has a NULL ema", who, i);
        CT_REQUIRE(((reinterpret_cast<uintptr_t>(it.param) | reinterpret_cast<uintptr_t>(it.grad) |
                     reinterpret_cast<uintptr_t>(it.momentum_buf) | reinterpret_cast<uintptr_t>(it.ema)) & 3) == 0,
                   "%s: tensor %d has a pointer that is not 4-byte aligned", who, i);
        total += ceil_div<int64_t>(it.numel + 3, CHUNK);
    }
    CT_REQUIRE(total <= INT_MAX, "%s: %lld chunks of %d elements are more than a call takes", who, (long long)total, CHUNK);
    hipStream_t st = as_stream(stream);
    SgdEmaLaunch L = {};
    L.momentum = momentum;
    L.one_minus_damp = 1.0f - dampening;
    L.grad_scale = grad_scale;
    L.nesterov = nesterov ? 1 : 0;
    L.clip = clip;
    L.ema = ema_dev;
    const bool has_buf = momentum != 0.f;
    int i = 0;
    while (i < n) {
        int k = 0;
        int64_t blocks = 0;
        for (; i < n && k < SGD_EMA_PER_LAUNCH; ++i) {
            const ct_sgd_ema_tensor& it = items[i];
            if (it.numel == 0) continue;
            SgdEmaTensor& t = L.t[k];
            t.p = it.param;
            t.g = it.grad;
            t.b = has_buf ? it.momentum_buf : nullptr;
            t.e = it.ema;
            t.numel = (int)it.numel;
            t.lr = it.lr;
            t.wd = it.weight_decay;
            const void* const ptrs[4] = {t.p, t.g, t.b, t.e};
            t.flags = (it.first_step ? F_FIRST : 0) | vec_flags(ptrs);
            L.first_block[k] = (int)blocks;
            blocks += chunks_of(t.numel, t.flags);
            ++k;
        }
        if (k == 0) break;
        for (int q = k; q <= SGD_EMA_PER_LAUNCH; ++q) L.first_block[q] = (int)blocks;
        L.n = k;
        if (clip) {
            CT_PROF("sgd_multi_kernel_ema_clipped", st);
            hipLaunchKernelGGL(sgd_multi_kernel_ema<true>, dim3((unsigned)blocks), dim3(THREADS), 0, st, L);
            CT_LAUNCH_CHECK("sgd_multi_kernel_ema_clipped");
        } else {
            CT_PROF("sgd_multi_kernel_ema", st);
            hipLaunchKernelGGL(sgd_multi_kernel_ema<false>, dim3((unsigned)blocks), dim3(THREADS), 0, st, L);
            CT_LAUNCH_CHECK("sgd_multi_kernel_ema");
        }
    }
    return CT_OK;
}

extern "C" int ct_ema_update(const ct_ema_tensor* items, int n, const ct_ema_state* ema_dev, ct_stream_t stream)
{
    const char* who = "ct_ema_update";
    if (const int rc = check_table(who, items, n)) return rc;
    if (const int rc = check_state(who, ema_dev)) return rc;
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const ct_ema_tensor& it = items[i];
        CT_REQUIRE(it.numel >= 0 && it.numel <= MAX_NUMEL, "%s: tensor %d has numel %lld (0 .. 2^31-1)", who, i,
                   (long long)it.numel);
        if (it.numel == 0) continue;
        CT_REQUIRE(it.ema && it.src, "%s: tensor %d has a NULL %s", who, i, it.ema ? "src" : "ema");
        CT_REQUIRE(((reinterpret_cast<uintptr_t>(it.ema) | reinterpret_cast<uintptr_t>(it.src)) & 3) == 0,
                   "%s: tensor %d has a pointer that is not 4-byte aligned", who, i);
        total += ctdet::ceil_div<int64_t>(it.numel + 3, CHUNK);
    }
    CT_REQUIRE(total <= INT_MAX, "%s: %lld chunks of %d elements are more than a call takes", who, (long long)total, CHUNK);
    return launch_pairs(items, n, ema_dev, [](const ct_ema_tensor& it) { return it.ema; },
                        [](const ct_ema_tensor& it) { return const_cast<float*>(it.src); }, stream);
}

extern "C" int ct_tensor_swap(const ct_swap_tensor* items, int n, ct_stream_t stream)
{
    const char* who = "ct_tensor_swap";
    if (const int rc = check_table(who, items, n)) return rc;
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const ct_swap_tensor& it = items[i];
        CT_REQUIRE(it.numel >= 0 && it.numel <= MAX_NUMEL, "%s: tensor %d has numel %lld (0 .. 2^31-1)", who, i,
                   (long long)it.numel);
        if (it.numel == 0) continue;
        CT_REQUIRE(it.a && it.b, "%s: tensor %d has a NULL %s", who, i, it.a ? "b" : "a");
        CT_REQUIRE(((reinterpret_cast<uintptr_t>(it.a) | reinterpret_cast<uintptr_t>(it.b)) & 3) == 0,
                   "%s: tensor %d has a pointer that is not 4-byte aligned", who, i);
        const uintptr_t a = reinterpret_cast<uintptr_t>(it.a), b = reinterpret_cast<uintptr_t>(it.b);
        const uintptr_t bytes = (uintptr_t)it.numel * sizeof(float);
        CT_REQUIRE(a != b, "%s: tensor %d has a == b", who, i);
        CT_REQUIRE(a + bytes <= b || b + bytes <= a, "%s: tensor %d has overlapping ranges", who, i);
        total += ctdet::ceil_div<int64_t>(it.numel + 3, CHUNK);
    }
    CT_REQUIRE(total <= INT_MAX, "%s: %lld chunks of %d elements are more than a call takes", who, (long long)total, CHUNK);
    return launch_pairs(items, n, nullptr, [](const ct_swap_tensor& it) { return it.a; },
                        [](const ct_swap_tensor& it) { return it.b; }, stream);
}
