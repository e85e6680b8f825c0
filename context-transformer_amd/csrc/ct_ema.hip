// Exponential moving average of the weights ("model averaging") next to the fused SGD step of ct_optim.hip:
//   ct_ema_begin      one thread: decides on the device whether this step is averaged (the non-finite guard of
//                     ct_grad_norm_clip skipped it or not), advances the update count and evaluates the warm-up decay;
//   ct_ema_update     ema = d * ema + (1 - d) * src for tensors the optimizer did not touch (no gradient, BatchNorm
//                     statistics); the parameters it did touch are averaged inside the step (ct_optim.hip, ct_sgd_step_ema);
//   ct_tensor_swap    exchanges two sets of tensors in place (evaluate with the averaged weights, then swap back).
// The two multi-tensor kernels are an Op each over walk() of ct_multi_tensor.h, which also packs their launch records
// and checks their arguments.  Every operation is rounded separately to fp32 (-ffp-contract=off for the file), in the
// order include/ctdet.h states.
#include "ct_common.h"
#include "ct_multi_tensor.h"

#include <climits>
#include <cstdint>

namespace {

using namespace ctdet::mt;

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
    template <class V> __device__ void apply(Regs<V>& r) const { r.e = ema_of(r.e, r.s, d, om); }
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

// ct_ema_update and ct_tensor_swap after their table checks: the checks of every pair -- `more` adds an entry's own --
// and the launches of `kernel`.  get(item, a, b) gives the two pointers, name_a / name_b are what the messages call them.
template <class Item, class Get, class More>
int pairs(const char* who, const Item* items, int n, const char* name, void (*kernel)(PairLaunch),
          const ct_ema_state* ema, const char* name_a, const char* name_b, Get get, More more, ct_stream_t stream)
{
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        float *a, *b;
        get(items[i], a, b);
        const Ptr ptrs[] = {{a, name_a, false}, {b, name_b, false}};
        if (const int rc = check_tensor(who, i, items[i].numel, ptrs)) return rc;
        if (const int rc = more(i, items[i])) return rc;
        total += max_chunks(items[i].numel);
    }
    if (const int rc = check_chunks(who, total)) return rc;
    hipStream_t st = ctdet::as_stream(stream);
    PairLaunch L = {};
    L.ema = ema;
    const auto fill = [&](PairLaunch& rec, int k, int i) -> int64_t {
        if (items[i].numel == 0) return 0;
        Pair& t = rec.t[k];
        get(items[i], t.a, t.b);
        t.numel = (int)items[i].numel;
        const void* const ptrs[2] = {t.a, t.b};
        t.flags = vec_flags(ptrs);
        return chunks_of(t.numel, t.flags);
    };
    return pack(L, n, fill, [&](const PairLaunch& rec, unsigned blocks) { return launch(name, kernel, rec, blocks, st); });
}

}  // namespace

extern "C" int ct_ema_begin(ct_ema_state* state_dev, float decay, float warmup, const ct_clip_state* clip_dev_or_null,
                            ct_stream_t stream)
{
    using namespace ctdet;
    const char* who = "ct_ema_begin";
    if (const int rc = check_state(who, state_dev, "the ema state")) return rc;
    CT_REQUIRE(decay >= 0.f && decay < 1.f, "%s: decay = %g is outside [0, 1)", who, (double)decay);
    CT_REQUIRE(warmup == 0.f || (warmup >= 1.f && warmup <= 3.0e38f), "%s: warmup = %g is neither 0 (off) nor >= 1", who,
               (double)warmup);
    if (const int rc = check_state(who, clip_dev_or_null, "the clip state", true)) return rc;
    hipStream_t st = as_stream(stream);
    CT_PROF("ema_begin_kernel", st);
    hipLaunchKernelGGL(ema_begin_kernel, dim3(1), dim3(1), 0, st, state_dev, decay, warmup, clip_dev_or_null);
    CT_LAUNCH_CHECK("ema_begin_kernel");
    return CT_OK;
}

extern "C" int ct_ema_update(const ct_ema_tensor* items, int n, const ct_ema_state* ema_dev, ct_stream_t stream)
{
    const char* who = "ct_ema_update";
    if (const int rc = check_table(who, items, n)) return rc;
    if (const int rc = check_state(who, ema_dev, "the ema state")) return rc;
    return pairs(who, items, n, "ema_multi_kernel", ema_multi_kernel, ema_dev, "ema", "src",
                 [](const ct_ema_tensor& it, float*& a, float*& b) { a = it.ema; b = const_cast<float*>(it.src); },
                 [](int, const ct_ema_tensor&) { return CT_OK; }, stream);
}

extern "C" int ct_tensor_swap(const ct_swap_tensor* items, int n, ct_stream_t stream)
{
    const char* who = "ct_tensor_swap";
    if (const int rc = check_table(who, items, n)) return rc;
    const auto apart = [&](int i, const ct_swap_tensor& it) -> int {
        if (it.numel == 0) return CT_OK;
        const uintptr_t a = reinterpret_cast<uintptr_t>(it.a), b = reinterpret_cast<uintptr_t>(it.b);
        const uintptr_t bytes = (uintptr_t)it.numel * sizeof(float);
        CT_REQUIRE(a != b, "%s: tensor %d has a == b", who, i);
        CT_REQUIRE(a + bytes <= b || b + bytes <= a, "%s: tensor %d has overlapping ranges", who, i);
        return CT_OK;
    };
    return pairs(who, items, n, "tensor_swap_kernel", tensor_swap_kernel, nullptr, "a", "b",
                 [](const ct_swap_tensor& it, float*& a, float*& b) { a = it.a; b = it.b; }, apart, stream);
}
