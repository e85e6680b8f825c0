// Fused multi-tensor SGD step (train.py's `optimizer.step()` over the groups of utils/solver.py:6-33): weight decay,
// momentum, dampening, Nesterov and the parameter update of torch.optim.SGD in ONE pass over (param, grad, buf), for
// any number of tensors per call -- ct_sgd_step, ct_sgd_step_clipped -- and, with one more array, the weight average
// updated from the new parameter value while it is still in a register (ct_sgd_step_ema: 7 array passes instead of
// 5 + 3).  A call is ceil(non-empty tensors / tensors per launch) launches whatever the tensor sizes.  The walk over a
// tensor, the launch-record packing and the argument checks are those of ct_multi_tensor.h; this file holds the two
// launch records, the one kernel both are walked by, and the gradient norm.
//
// Every operation is rounded separately to fp32 (__fmul_rn / __fadd_rn / __fsub_rn, and -ffp-contract=off for the
// file), in the order include/ctdet.h states, so a NumPy float32 restatement reproduces the result bit for bit.
//
// Gradient-norm clipping and the non-finite guard (ct_grad_norm_clip) sit in front of the same update.
// grad_norm_kernel is a reduction, not a map, so it keeps a read-only walk of its own over the same chunks, found by the
// same prefix-sum search: every workgroup squares and sums its chunk in binary64 (each product of two fp32 values is
// exact there), reduces across lanes and waves in a fixed order and stores ONE double to its own workspace slot;
// grad_norm_finish_kernel (one workgroup) sums the slots in a fixed order and writes {norm, coef, finite, nonfinite}
// to a 16-byte device state.  No atomics, no "last workgroup finishes": the same table gives the same bits.
// sgd_multi_kernel<., true> reads that state (two scalar loads), multiplies coef into grad_scale once, or -- when the
// norm was not finite -- leaves everything alone except the momentum buffers of first-step tensors, which it sets to +0.
#include "ct_common.h"
#include "ct_multi_tensor.h"

#include <cstdint>
#include <cstdio>
#include <type_traits>

namespace {

using namespace ctdet::mt;

constexpr int TENSORS_PER_LAUNCH = 80;      // 80 * 40 B + 81 * 4 B + scalars = 3548 B of the 4096 B a launch may carry
constexpr int SGD_EMA_PER_LAUNCH = 77;      // 77 * 48 B + 78 * 4 B + scalars = 4048 B

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
    const ct_clip_state* clip;              // CLIP only; appended, so the other offsets stay
};
static_assert(sizeof(Tensor) == 40, "kernel-argument budget");
static_assert(sizeof(Launch) <= 4096, "kernel arguments are limited to 4 KiB");

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
    const ct_clip_state* clip;              // CLIP only
    const ct_ema_state* ema;
};
static_assert(sizeof(SgdEmaTensor) == 48, "kernel-argument budget");
static_assert(sizeof(SgdEmaLaunch) <= 4096, "kernel arguments are limited to 4 KiB");

// The update of one element or one 16-byte group for walk().  EMA = false never touches E, averaged, d or om.
template <bool EMA>
struct SgdOp {
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
        if constexpr (EMA) r.e = averaged ? ld<V>(E + j) : zero<V>();
        else r.e = zero<V>();
        return r;
    }
    template <class V> __device__ void apply(Regs<V>& r) const
    {
        update(r.p, r.g, r.b, h);
        if constexpr (EMA) r.e = ema_of(r.e, r.p, d, om);
    }
    template <class V> __device__ void store(int64_t j, const Regs<V>& r) const
    {
        st(P + j, r.p);
        if (has_buf) st(B + j, r.b);
        if constexpr (EMA) {
            if (averaged) st(E + j, r.e);
        }
    }
};

// LaunchT = Launch is ct_sgd_step; SgdEmaLaunch is ct_sgd_step_ema, where the average moves iff the step ran and
// ct_ema_begin opened an update.  CLIP reads the state ct_grad_norm_clip left on the device: coef goes into grad_scale
// once, and a non-finite norm skips the update.
template <class LaunchT, bool CLIP>
__global__ __launch_bounds__(THREADS) void sgd_multi_kernel(const LaunchT L)
{
    constexpr bool EMA = std::is_same<LaunchT, SgdEmaLaunch>::value;
    const int blk = blockIdx.x;
    const int lo = owner_of(L.first_block, L.n, blk);
    const auto& T = L.t[lo];
    const int chunk = blk - L.first_block[lo];
    const int flags = T.flags;
    const int numel = T.numel;
    const int tid = threadIdx.x;
    SgdOp<EMA> op;
    op.P = T.p; op.G = T.g; op.B = T.b;
    op.h.lr = T.lr; op.h.wd = T.wd; op.h.momentum = L.momentum; op.h.omd = L.one_minus_damp; op.h.gs = L.grad_scale;
    op.h.first = flags & F_FIRST; op.h.nesterov = L.nesterov != 0;
    op.has_buf = L.momentum != 0.f;

    if (CLIP) {
        if (L.clip->finite == 0) {
            // Skipped step.  A first-step buffer is uninitialised memory the host is about to adopt as state: +0 to
            // the elements of this chunk (dword stores: the path is rare), nothing else is written.
            if (op.has_buf && op.h.first) {
                const int shift = (flags & F_VEC) ? (flags >> 2) & 3 : 0;
                const int64_t s0 = (int64_t)chunk * CHUNK;              // shifted coordinates, as in walk()
                const int64_t j0 = s0 > shift ? s0 - shift : 0;
                const int64_t j1 = s0 + CHUNK - shift < numel ? s0 + CHUNK - shift : numel;
                for (int64_t j = j0 + tid; j < j1; j += THREADS) op.B[j] = 0.f;
            }
            return;
        }
        op.h.gs = __fmul_rn(L.grad_scale, L.clip->coef);
    }
    if constexpr (EMA) {
        op.E = T.e;
        op.averaged = L.ema->applied != 0;
        op.d = L.ema->decay;
        op.om = L.ema->one_minus;
    }
    walk(op, chunk, numel, flags, tid);
}

// ------------------------------------------------------------------------------------------------ gradient norm
constexpr int GRADS_PER_LAUNCH = 220;       // 220 * (8 + 4) B + 221 * 4 B + 24 B = 3548 B, as much as Launch carries
constexpr int FINISH_THREADS = 1024;
constexpr int WAVE = 64;

struct NormLaunch {
    const float* g[GRADS_PER_LAUNCH];
    int numel[GRADS_PER_LAUNCH];
    int first_block[GRADS_PER_LAUNCH + 1];
    int n;
    int slot0;                              // workspace slot of this launch's workgroup 0
    double* slots;
};
static_assert(sizeof(NormLaunch) <= sizeof(Launch), "kernel-argument budget: no more than the update carries");

__device__ inline double sq(float v) { return (double)v * (double)v; }      // exact: 48 significant bits at most

// x + y + z + w of one group, left to right
__device__ inline double sq4(const float4& v) { return ((sq(v.x) + sq(v.y)) + sq(v.z)) + sq(v.w); }

// Sum over the workgroup in a fixed order: lanes by halving strides inside a wave, then the waves one after another.
// The result is valid in thread 0.
template <int NT>
__device__ inline double block_sum(double v)
{
    __shared__ double part[NT / WAVE];
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < NT / WAVE; ++w) s += part[w];
    }
    return s;
}

__global__ __launch_bounds__(THREADS) void grad_norm_kernel(const NormLaunch L)
{
    const int blk = blockIdx.x;
    const int lo = owner_of(L.first_block, L.n, blk);
    const int chunk = blk - L.first_block[lo];
    const int numel = L.numel[lo];
    const float* __restrict__ G = L.g[lo];
    const int tid = threadIdx.x;
    // Shifted coordinates as in walk(): s = element index + shift, s % 4 == 0 on a 16-byte line.  With one array there
    // is always such a shift.
    const int shift = (int)((reinterpret_cast<uintptr_t>(G) >> 2) & 3);
    const int64_t end = (int64_t)numel + shift;
    const int64_t q0 = (int64_t)chunk * GROUPS;
    const bool whole = (q0 * 4 >= shift) && ((q0 + GROUPS) * 4 <= end);
    double acc = 0.0;
    if (whole) {
        float4 g[GROUPS / THREADS];
#pragma unroll
        for (int k = 0; k < GROUPS / THREADS; ++k)
            g[k] = *reinterpret_cast<const float4*>(G + ((q0 + (int64_t)k * THREADS + tid) * 4 - shift));
#pragma unroll
        for (int k = 0; k < GROUPS / THREADS; ++k) acc += sq4(g[k]);
    } else {
        // first / last chunk of the tensor: a partial group goes element by element, nothing outside it is read
        for (int k = 0; k < GROUPS / THREADS; ++k) {
            const int64_t s = (q0 + (int64_t)k * THREADS + tid) * 4;
            if (s >= end) break;
            if (s >= shift && s + 4 <= end) {
                acc += sq4(*reinterpret_cast<const float4*>(G + (s - shift)));
            } else {
                double part = 0.0;
                for (int e = 0; e < 4; ++e) {
                    const int64_t se = s + e;
                    if (se >= shift && se < end) part += sq(G[se - shift]);
                }
                acc += part;
            }
        }
    }
    acc = block_sum<THREADS>(acc);
    if (tid == 0) L.slots[(int64_t)L.slot0 + blk] = acc;
}

__global__ __launch_bounds__(FINISH_THREADS) void grad_norm_finish_kernel(const double* __restrict__ slots, int n,
                                                                          float grad_scale, float max_norm,
                                                                          ct_clip_state* state)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += FINISH_THREADS) acc += slots[i];
    acc = block_sum<FINISH_THREADS>(acc);
    if (threadIdx.x == 0) {
        // include/ctdet.h, ct_grad_norm_clip: one rounding per line
        const float norm = (float)(sqrt(acc) * (double)fabsf(grad_scale));
        const bool finite = isfinite(norm);
        const float coef = finite ? fminf(1.0f, __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f))) : 0.0f;
        const int bad = state->nonfinite + (finite ? 0 : 1);
        state->norm = norm;
        state->coef = coef;
        state->finite = finite ? 1 : 0;
        state->nonfinite = bad;
    }
}

// one array: it is always walked in 16-byte groups
inline int64_t grad_chunks(const ct_grad_tensor& it)
{
    const void* const ptrs[1] = {it.grad};
    return it.numel ? chunks_of(it.numel, vec_flags(ptrs)) : 0;
}

// The argument checks both norm entry points share; *slots = the workgroups, and workspace slots, of the call
int check_grads(const char* who, const ct_grad_tensor* items, int n, int64_t* slots)
{
    if (const int rc = check_table(who, items, n)) return rc;
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const Ptr ptrs[] = {{items[i].grad, "grad", false}};
        if (const int rc = check_tensor(who, i, items[i].numel, ptrs)) return rc;
        total += grad_chunks(items[i]);
    }
    *slots = total;
    return check_chunks(who, total);
}

// The three step entry points: Launch / ct_sgd_tensor (ema == nullptr) and SgdEmaLaunch / ct_sgd_ema_tensor; `who`
// names the entry point in the messages, clip != nullptr takes the CLIP kernel
template <class LaunchT, class Item>
int sgd_step(const char* who, const Item* items, int n, float momentum, float dampening, int nesterov, float grad_scale,
             const ct_clip_state* clip, const ct_ema_state* ema, ct_stream_t stream)
{
    constexpr bool EMA = std::is_same<LaunchT, SgdEmaLaunch>::value;
    if (const int rc = check_table(who, items, n)) return rc;
    CT_REQUIRE(!nesterov || (momentum != 0.f && dampening == 0.f),
               "%s: nesterov needs a momentum and zero dampening (momentum %g, dampening %g)", who, (double)momentum,
               (double)dampening);
    LaunchT L = {};
    if constexpr (EMA) {
        if (const int rc = check_state(who, ema, "the ema state")) return rc;
        if (const int rc = check_state(who, clip, "the clip state", true)) return rc;
        L.ema = ema;
    }
    char no_buf[64];
    snprintf(no_buf, sizeof(no_buf), "no momentum_buf but momentum = %g", (double)momentum);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const Item& it = items[i];
        const float* e = nullptr;
        if constexpr (EMA) e = it.ema;
        const Ptr ptrs[] = {{it.param, "param", false},
                            {it.grad, "grad", false},
                            {it.momentum_buf, "momentum_buf", momentum == 0.f, no_buf},
                            {e, "ema", !EMA}};
        if (const int rc = check_tensor(who, i, it.numel, ptrs)) return rc;
        if constexpr (EMA) total += max_chunks(it.numel);
    }
    // ct_sgd_step has never limited the chunks of a call (a launch holds 80 * 2^18 at most), and still does not
    if constexpr (EMA) {
        if (const int rc = check_chunks(who, total)) return rc;
    }
    L.momentum = momentum;
    L.one_minus_damp = 1.0f - dampening;
    L.grad_scale = grad_scale;
    L.nesterov = nesterov ? 1 : 0;
    L.clip = clip;
    const bool has_buf = momentum != 0.f;
    const auto fill = [&](LaunchT& rec, int k, int i) -> int64_t {
        const Item& it = items[i];
        if (it.numel == 0) return 0;
        auto& t = rec.t[k];
        t.p = it.param;
        t.g = it.grad;
        t.b = has_buf ? it.momentum_buf : nullptr;
        const float* e = nullptr;
        if constexpr (EMA) e = t.e = it.ema;
        t.numel = (int)it.numel;
        t.lr = it.lr;
        t.wd = it.weight_decay;
        const void* const ptrs[4] = {t.p, t.g, t.b, e};
        t.flags = (it.first_step ? F_FIRST : 0) | vec_flags(ptrs);
        return chunks_of(t.numel, t.flags);
    };
    const char* name = EMA ? (clip ? "sgd_multi_kernel_ema_clipped" : "sgd_multi_kernel_ema")
                           : (clip ? "sgd_multi_kernel_clipped" : "sgd_multi_kernel");
    const auto kernel = clip ? sgd_multi_kernel<LaunchT, true> : sgd_multi_kernel<LaunchT, false>;
    hipStream_t st = ctdet::as_stream(stream);
    return pack(L, n, fill, [&](const LaunchT& rec, unsigned blocks) { return launch(name, kernel, rec, blocks, st); });
}

}  // namespace

extern "C" int ct_grad_norm_tensors_per_launch(void) { return GRADS_PER_LAUNCH; }

extern "C" size_t ct_grad_norm_workspace_bytes(const ct_grad_tensor* items, int n)
{
    int64_t slots = 0;
    if (check_grads("ct_grad_norm_workspace_bytes", items, n, &slots) != CT_OK) return 0;
    return sizeof(double) * (size_t)(slots > 0 ? slots : 1);
}

extern "C" int ct_grad_norm_clip(const ct_grad_tensor* items, int n, float grad_scale, float max_norm, void* workspace,
                                 size_t workspace_bytes, ct_clip_state* state_dev, ct_stream_t stream)
{
    const char* who = "ct_grad_norm_clip";
    int64_t slots = 0;
    if (const int rc = check_grads(who, items, n, &slots)) return rc;
    CT_REQUIRE(max_norm > 0.f, "%s: max_norm = %g must be positive (+inf: guard only)", who, (double)max_norm);
    if (const int rc = check_state(who, state_dev, "state_dev")) return rc;
    const size_t need = sizeof(double) * (size_t)(slots > 0 ? slots : 1);
    CT_REQUIRE(workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
               "%s: workspace is NULL or not 8-byte aligned", who);
    CT_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    hipStream_t st = ctdet::as_stream(stream);
    NormLaunch L = {};
    L.slots = static_cast<double*>(workspace);
    int64_t slot0 = 0;
    const auto fill = [&](NormLaunch& rec, int k, int i) {
        rec.g[k] = items[i].grad;
        rec.numel[k] = (int)items[i].numel;
        return grad_chunks(items[i]);
    };
    const int rc = pack(L, n, fill, [&](NormLaunch& rec, unsigned blocks) {
        rec.slot0 = (int)slot0;
        slot0 += blocks;
        return launch("grad_norm_kernel", grad_norm_kernel, rec, blocks, st);
    });
    if (rc != CT_OK) return rc;
    // slot0 == slots: every slot the finish reads was written by the launches above
    CT_PROF("grad_norm_finish_kernel", st);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(FINISH_THREADS), 0, st, L.slots, (int)slot0, grad_scale,
                       max_norm, state_dev);
    CT_LAUNCH_CHECK("grad_norm_finish_kernel");
    return CT_OK;
}

extern "C" int ct_sgd_step(const ct_sgd_tensor* items, int n, float momentum, float dampening, int nesterov,
                           float grad_scale, ct_stream_t stream)
{
    return sgd_step<Launch>("ct_sgd_step", items, n, momentum, dampening, nesterov, grad_scale, nullptr, nullptr, stream);
}

extern "C" int ct_sgd_step_clipped(const ct_sgd_tensor* items, int n, float momentum, float dampening, int nesterov,
                                   float grad_scale, const ct_clip_state* state_dev, ct_stream_t stream)
{
    const char* who = "ct_sgd_step_clipped";
    if (const int rc = check_state(who, state_dev, "state_dev")) return rc;
    return sgd_step<Launch>(who, items, n, momentum, dampening, nesterov, grad_scale, state_dev, nullptr, stream);
}

extern "C" int ct_sgd_step_ema(const ct_sgd_ema_tensor* items, int n, float momentum, float dampening, int nesterov,
                               float grad_scale, const ct_clip_state* clip, const ct_ema_state* ema_dev,
                               ct_stream_t stream)
{
    return sgd_step<SgdEmaLaunch>("ct_sgd_step_ema", items, n, momentum, dampening, nesterov, grad_scale, clip, ema_dev,
                                  stream);
}

extern "C" int ct_sgd_tensors_per_launch(void) { return TENSORS_PER_LAUNCH; }

extern "C" int ct_sgd_ema_tensors_per_launch(void) { return SGD_EMA_PER_LAUNCH; }
