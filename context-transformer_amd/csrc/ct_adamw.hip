// Fused multi-tensor AdamW step (torch.optim.AdamW, amsgrad=False, maximize=False; decoupled weight decay), the second
// update rule on the chunk walker of ct_multi_tensor.h:
//   ct_adamw_begin    one thread per listed 32-byte step record: decides on the device whether this step counts (the
//                     non-finite guard of ct_grad_norm_clip skipped it or not), advances the binary64 running products
//                     beta1^step / beta2^step and leaves the two bias-correction terms in fp32 for the step;
//   ct_adamw_step     one pass over (param, grad, exp_avg, exp_avg_sq) and, with a weight average attached, the shadow,
//                     for any number of tensors per call: ceil(non-empty tensors / tensors per launch) launches.
// The walk over a tensor, the launch-record packing and the argument checks are those of ct_multi_tensor.h; this file
// holds the launch record, the Op and the begin kernel.
//
// Every operation is rounded separately to fp32 (__fmul_rn / __fadd_rn / __fsub_rn, and -ffp-contract=off for the
// file); the square root and the two divisions are the correctly rounded ones (the compiler's default for HIP, asked
// for by name in build.py), in the order include/ctdet.h states, so a NumPy float32 restatement reproduces the result
// bit for bit.  A skipped step (clip->finite == 0) returns before the first load: nothing is written.
#include "ct_common.h"
#include "ct_multi_tensor.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

namespace {

using namespace ctdet::mt;

enum { F_DECAY = 1 };                       // bit 0 of Tensor::flags (F_FIRST's place): weight_decay != 0

// ---------------------------------------------------------------------------------------------- ct_adamw_begin
constexpr int BEGIN_PER_LAUNCH = 1000;      // 1000 * 4 B + 40 B of scalars = 4040 B of the 4096 B a launch may carry

struct BeginLaunch {
    int index[BEGIN_PER_LAUNCH];
    int n;
    double beta1, beta2;
    ct_adam_state* states;
    const ct_clip_state* clip;
};
static_assert(sizeof(ct_adam_state) == 32, "ct_adam_state is 32 bytes");
static_assert(sizeof(BeginLaunch) <= 4096, "kernel arguments are limited to 4 KiB");

__global__ __launch_bounds__(THREADS) void adamw_begin_kernel(const BeginLaunch L)
{
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= L.n) return;
    // include/ctdet.h, ct_adamw_begin: one rounding per line; plain loads and stores of the 32 bytes
    ct_adam_state* s = L.states + L.index[i];
    const int ok = L.clip ? (L.clip->finite != 0 ? 1 : 0) : 1;
    if (!ok) {
        s->applied = 0;
        return;
    }
    const int step = s->step;
    const double b1p = (step == 0 ? 1.0 : s->beta1_pow) * L.beta1;
    const double b2p = (step == 0 ? 1.0 : s->beta2_pow) * L.beta2;
    const float bc1 = (float)(1.0 - b1p);
    const float bc2 = (float)(1.0 - b2p);
    s->beta1_pow = b1p;
    s->beta2_pow = b2p;
    s->step = step == INT_MAX ? step : step + 1;
    s->applied = 1;
    s->bc1 = bc1;
    s->rs2 = sqrtf(bc2);
}

// ----------------------------------------------------------------------------------------------- ct_adamw_step
constexpr int TENSORS_PER_LAUNCH = 59;      // 59 * 64 B + 60 * 4 B + 48 B of scalars and pointers = 4064 B

struct Tensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* e;                               // EMA only
    const ct_adam_state* state;
    int numel;
    float lr, lw;                           // lw = lr * weight_decay, rounded once on the host
    int flags;
};

struct Launch {
    Tensor t[TENSORS_PER_LAUNCH];
    int first_block[TENSORS_PER_LAUNCH + 1];
    int n;
    float beta1, beta2, om1, om2, eps, grad_scale;
    const ct_clip_state* clip;              // CLIP only
    const ct_ema_state* ema;                // EMA only
};
static_assert(sizeof(Tensor) == 64, "kernel-argument budget");
static_assert(sizeof(Launch) <= 4096, "kernel arguments are limited to 4 KiB");

struct AdamHyper {
    float lw, b1, b2, om1, om2, rs2, eps, a, gs;
    bool decay;
};

// include/ctdet.h, ct_adamw_step: one rounding per line
__device__ inline void adamw(float& p, float g, float& m, float& v, const AdamHyper& h)
{
    g = __fmul_rn(g, h.gs);
    if (h.decay) p = __fsub_rn(p, __fmul_rn(h.lw, p));
    m = __fadd_rn(__fmul_rn(h.b1, m), __fmul_rn(h.om1, g));
    v = __fadd_rn(__fmul_rn(h.b2, v), __fmul_rn(__fmul_rn(h.om2, g), g));
    const float den = __fadd_rn(__fdiv_rn(sqrtf(v), h.rs2), h.eps);
    p = __fsub_rn(p, __fmul_rn(h.a, __fdiv_rn(m, den)));
}

__device__ inline void adamw(float4& p, const float4& g, float4& m, float4& v, const AdamHyper& h)
{
    adamw(p.x, g.x, m.x, v.x, h);
    adamw(p.y, g.y, m.y, v.y, h);
    adamw(p.z, g.z, m.z, v.z, h);
    adamw(p.w, g.w, m.w, v.w, h);
}

// The update of one element or one 16-byte group for walk().  EMA = false never touches E, averaged, d or om.
template <bool EMA>
struct AdamwOp {
    float* __restrict__ P;
    const float* __restrict__ G;
    float* __restrict__ M;
    float* __restrict__ V;
    float* __restrict__ E;
    AdamHyper h;
    bool averaged;
    float d, om;
    template <class T> struct Regs { T p, g, m, v, e; };

    template <class T> __device__ Regs<T> load(int64_t j) const
    {
        Regs<T> r;
        r.p = ld<T>(P + j);
        r.g = ld<T>(G + j);
        r.m = ld<T>(M + j);
        r.v = ld<T>(V + j);
        if constexpr (EMA) r.e = averaged ? ld<T>(E + j) : zero<T>();
        else r.e = zero<T>();
        return r;
    }
    template <class T> __device__ void apply(Regs<T>& r) const
    {
        adamw(r.p, r.g, r.m, r.v, h);
        if constexpr (EMA) r.e = ema_of(r.e, r.p, d, om);
    }
    template <class T> __device__ void store(int64_t j, const Regs<T>& r) const
    {
        st(P + j, r.p);
        st(M + j, r.m);
        st(V + j, r.v);
        if constexpr (EMA) {
            if (averaged) st(E + j, r.e);
        }
    }
};

// CLIP reads the state ct_grad_norm_clip left on the device: coef goes into grad_scale once, and a non-finite norm
// skips the update.  EMA: the average moves iff the step ran and ct_ema_begin opened an update.
template <bool EMA, bool CLIP>
__global__ __launch_bounds__(THREADS) void adamw_multi_kernel(const Launch L)
{
    const int blk = blockIdx.x;
    const int lo = owner_of(L.first_block, L.n, blk);
    const Tensor& T = L.t[lo];
    AdamwOp<EMA> op;
    op.h.gs = L.grad_scale;
    if (CLIP) {
        if (L.clip->finite == 0) return;    // skipped step: nothing is written
        op.h.gs = __fmul_rn(L.grad_scale, L.clip->coef);
    }
    op.P = T.p; op.G = T.g; op.M = T.m; op.V = T.v;
    op.h.lw = T.lw; op.h.decay = (T.flags & F_DECAY) != 0;
    op.h.b1 = L.beta1; op.h.b2 = L.beta2; op.h.om1 = L.om1; op.h.om2 = L.om2; op.h.eps = L.eps;
    op.h.rs2 = T.state->rs2;
    op.h.a = __fdiv_rn(T.lr, T.state->bc1);
    if constexpr (EMA) {
        op.E = T.e;
        op.averaged = L.ema->applied != 0;
        op.d = L.ema->decay;
        op.om = L.ema->one_minus;
    }
    walk(op, blk - L.first_block[lo], T.numel, T.flags, threadIdx.x);
}

inline bool unit_interval(double b) { return b >= 0.0 && b < 1.0; }        // false for NaN

}  // namespace

extern "C" int ct_adamw_begin_indices_per_launch(void) { return BEGIN_PER_LAUNCH; }

extern "C" int ct_adamw_begin(ct_adam_state* states_dev, const int* index_host, int n, double beta1, double beta2,
                              const ct_clip_state* clip_dev_or_null, ct_stream_t stream)
{
    using namespace ctdet;
    const char* who = "ct_adamw_begin";
    CT_REQUIRE(n >= 0, "%s: n = %d is negative", who, n);
    CT_REQUIRE(unit_interval(beta1) && unit_interval(beta2), "%s: betas (%g, %g) are outside [0, 1)", who, beta1, beta2);
    if (const int rc = check_state(who, clip_dev_or_null, "the clip state", true)) return rc;
    CT_REQUIRE((reinterpret_cast<uintptr_t>(states_dev) & 7) == 0, "%s: states_dev is not 8-byte aligned", who);
    if (n == 0) return CT_OK;
    CT_REQUIRE(states_dev != nullptr, "%s: states_dev is NULL with n = %d", who, n);
    CT_REQUIRE(index_host != nullptr, "%s: index_host is NULL with n = %d", who, n);
    std::vector<int> sorted(index_host, index_host + n);
    std::sort(sorted.begin(), sorted.end());
    CT_REQUIRE(sorted[0] >= 0, "%s: index %d is negative", who, sorted[0]);
    for (int i = 1; i < n; ++i) CT_REQUIRE(sorted[i] != sorted[i - 1], "%s: index %d is listed twice", who, sorted[i]);
    hipStream_t st = as_stream(stream);
    BeginLaunch L = {};
    L.beta1 = beta1;
    L.beta2 = beta2;
    L.states = states_dev;
    L.clip = clip_dev_or_null;
    for (int i0 = 0; i0 < n; i0 += BEGIN_PER_LAUNCH) {
        L.n = std::min(BEGIN_PER_LAUNCH, n - i0);
        std::copy(index_host + i0, index_host + i0 + L.n, L.index);
        if (const int rc = launch("adamw_begin_kernel", adamw_begin_kernel, L, (unsigned)ceil_div(L.n, THREADS), st))
            return rc;
    }
    return CT_OK;
}

extern "C" int ct_adamw_tensors_per_launch(void) { return TENSORS_PER_LAUNCH; }

extern "C" int ct_adamw_step(const ct_adamw_tensor* items, int n, float beta1, float beta2, float eps, float grad_scale,
                             const ct_clip_state* clip, const ct_ema_state* ema, ct_stream_t stream)
{
    using namespace ctdet;
    const char* who = "ct_adamw_step";
    if (const int rc = check_table(who, items, n)) return rc;
    CT_REQUIRE(unit_interval(beta1) && unit_interval(beta2), "%s: betas (%g, %g) are outside [0, 1)", who, (double)beta1,
               (double)beta2);
    CT_REQUIRE(eps >= 0.f, "%s: eps = %g is negative or NaN", who, (double)eps);
    if (const int rc = check_state(who, clip, "the clip state", true)) return rc;
    if (const int rc = check_state(who, ema, "the ema state", true)) return rc;
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const ct_adamw_tensor& it = items[i];
        const Ptr ptrs[] = {{it.param, "param", false},
                            {it.grad, "grad", false},
                            {it.exp_avg, "exp_avg", false},
                            {it.exp_avg_sq, "exp_avg_sq", false},
                            {it.ema, "ema", ema == nullptr, "no ema but the call has an ema state"}};
        if (const int rc = check_tensor(who, i, it.numel, ptrs)) return rc;
        if (it.numel == 0) continue;
        CT_REQUIRE(it.ema == nullptr || ema != nullptr, "%s: tensor %d has an ema but the call has no ema state", who, i);
        CT_REQUIRE(it.state != nullptr, "%s: tensor %d has a NULL state", who, i);
        CT_REQUIRE((reinterpret_cast<uintptr_t>(it.state) & 7) == 0, "%s: tensor %d has a state that is not 8-byte aligned",
                   who, i);
        total += max_chunks(it.numel);
    }
    if (const int rc = check_chunks(who, total)) return rc;
    Launch L = {};
    L.beta1 = beta1;
    L.beta2 = beta2;
    L.om1 = (float)(1.0 - (double)beta1);
    L.om2 = (float)(1.0 - (double)beta2);
    L.eps = eps;
    L.grad_scale = grad_scale;
    L.clip = clip;
    L.ema = ema;
    const auto fill = [&](Launch& rec, int k, int i) -> int64_t {
        const ct_adamw_tensor& it = items[i];
        if (it.numel == 0) return 0;
        Tensor& t = rec.t[k];
        t.p = it.param;
        t.g = it.grad;
        t.m = it.exp_avg;
        t.v = it.exp_avg_sq;
        t.e = it.ema;
        t.state = it.state;
        t.numel = (int)it.numel;
        t.lr = it.lr;
        t.lw = it.lr * it.weight_decay;
        const void* const ptrs[5] = {t.p, t.g, t.m, t.v, t.e};
        t.flags = (it.weight_decay != 0.f ? F_DECAY : 0) | vec_flags(ptrs);
        return chunks_of(t.numel, t.flags);
    };
    const char* name = ema ? (clip ? "adamw_multi_kernel_ema_clipped" : "adamw_multi_kernel_ema")
                           : (clip ? "adamw_multi_kernel_clipped" : "adamw_multi_kernel");
    const auto kernel = ema ? (clip ? adamw_multi_kernel<true, true> : adamw_multi_kernel<true, false>)
                            : (clip ? adamw_multi_kernel<false, true> : adamw_multi_kernel<false, false>);
    hipStream_t st = as_stream(stream);
    return pack(L, n, fill, [&](const Launch& rec, unsigned blocks) { return launch(name, kernel, rec, blocks, st); });
}
