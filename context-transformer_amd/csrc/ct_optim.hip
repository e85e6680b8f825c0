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
//
// Gradient-norm clipping and the non-finite guard (ct_grad_norm_clip, ct_sgd_step_clipped) sit in front of the same
// update.  grad_norm_kernel walks the gradients in the same chunks, found by the same prefix-sum search: every
// workgroup squares and sums its chunk in binary64 (each product of two fp32 values is exact there), reduces across
// lanes and waves in a fixed order and stores ONE double to its own workspace slot; grad_norm_finish_kernel (one
// workgroup) sums the slots in a fixed order and writes {norm, coef, finite, nonfinite} to a 16-byte device state.
// No atomics, no "last workgroup finishes": the same table gives the same bits.  sgd_multi_kernel<true> reads that
// state (two scalar loads), multiplies coef into grad_scale once, or -- when the norm was not finite -- leaves
// everything alone except the momentum buffers of first-step tensors, which it sets to +0.
#include "ct_common.h"
#include "ct_multi_tensor.h"

#include <climits>
#include <cstdint>

namespace {

using namespace ctdet::mt;                  // chunk geometry, update(), owner_of(), line_offset(): shared with ct_ema.hip

constexpr int TENSORS_PER_LAUNCH = 80;      // 80 * 40 B + 81 * 4 B + scalars = 3548 B of the 4096 B a launch may carry

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
    const ct_clip_state* clip;              // sgd_multi_kernel<true> only; appended, so the other offsets stay
};
static_assert(sizeof(Tensor) == 40, "kernel-argument budget");
static_assert(sizeof(Launch) <= 4096, "kernel arguments are limited to 4 KiB");

// CLIP = false is ct_sgd_step.  CLIP = true (ct_sgd_step_clipped) reads the state ct_grad_norm_clip left on the
// device: coef goes into grad_scale once, and a non-finite norm skips the update.
template <bool CLIP>
__global__ __launch_bounds__(THREADS) void sgd_multi_kernel(const Launch L)
{
    const int blk = blockIdx.x;
    const int lo = owner_of(L.first_block, L.n, blk);
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

    if (CLIP) {
        if (L.clip->finite == 0) {
            // Skipped step.  A first-step buffer is uninitialised memory the host is about to adopt as state: +0 to
            // the elements of this chunk (dword stores: the path is rare), nothing else is written.
            if (has_buf && h.first) {
                const int shift = (flags & F_VEC) ? (flags >> 2) & 3 : 0;
                const int64_t s0 = (int64_t)chunk * CHUNK;              // shifted coordinates, as below
                const int64_t j0 = s0 > shift ? s0 - shift : 0;
                const int64_t j1 = s0 + CHUNK - shift < numel ? s0 + CHUNK - shift : numel;
                for (int64_t j = j0 + tid; j < j1; j += THREADS) B[j] = 0.f;
            }
            return;
        }
        h.gs = __fmul_rn(L.grad_scale, L.clip->coef);
    }

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
    // Shifted coordinates as in sgd_multi_kernel: s = element index + shift, s % 4 == 0 on a 16-byte line.  With one
    // array there is always such a shift.
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

inline int64_t grad_chunks(const ct_grad_tensor& it)
{
    return ctdet::ceil_div<int64_t>(it.numel + line_offset(it.grad), CHUNK);
}

// The argument checks both norm entry points share; -> CT_OK or the recorded failure
int check_grads(const char* who, const ct_grad_tensor* items, int n, int64_t* slots)
{
    CT_REQUIRE(n >= 0, "%s: n = %d is negative", who, n);
    CT_REQUIRE(n == 0 || items != nullptr, "%s: items is NULL with n = %d", who, n);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const ct_grad_tensor& it = items[i];
        CT_REQUIRE(it.numel >= 0 && it.numel <= MAX_NUMEL, "%s: tensor %d has numel %lld (0 .. 2^31-1)", who, i,
                   (long long)it.numel);
        if (it.numel == 0) continue;        // an empty tensor may have no pointer
        CT_REQUIRE(it.grad, "%s: tensor %d has a NULL grad", who, i);
        CT_REQUIRE((reinterpret_cast<uintptr_t>(it.grad) & 3) == 0, "%s: tensor %d has a grad that is not 4-byte aligned",
                   who, i);
        total += grad_chunks(it);
    }
    CT_REQUIRE(total <= INT_MAX, "%s: %lld chunks of %d elements are more than a call takes", who, (long long)total, CHUNK);
    *slots = total;
    return CT_OK;
}

// ct_sgd_step (clip == nullptr) and ct_sgd_step_clipped; `who` names the entry point in the messages
int sgd_step(const char* who, const ct_sgd_tensor* items, int n, float momentum, float dampening, int nesterov,
             float grad_scale, const ct_clip_state* clip, ct_stream_t stream)
{
    using namespace ctdet;
    CT_REQUIRE(n >= 0, "%s: n = %d is negative", who, n);
    CT_REQUIRE(n == 0 || items != nullptr, "%s: items is NULL with n = %d", who, n);
    CT_REQUIRE(!nesterov || (momentum != 0.f && dampening == 0.f),
               "%s: nesterov needs a momentum and zero dampening (momentum %g, dampening %g)", who, (double)momentum,
               (double)dampening);
    for (int i = 0; i < n; ++i) {
        const ct_sgd_tensor& it = items[i];
        CT_REQUIRE(it.numel >= 0 && it.numel <= MAX_NUMEL, "%s: tensor %d has numel %lld (0 .. 2^31-1)", who, i,
                   (long long)it.numel);
        if (it.numel == 0) continue;        // a no-op whatever its pointers are (an empty tensor may have none)
        CT_REQUIRE(it.param && it.grad, "%s: tensor %d has a NULL %s", who, i, it.param ? "grad" : "param");
        CT_REQUIRE(momentum == 0.f || it.momentum_buf, "%s: tensor %d has no momentum_buf but momentum = %g", who, i,
                   (double)momentum);
        CT_REQUIRE(((reinterpret_cast<uintptr_t>(it.param) | reinterpret_cast<uintptr_t>(it.grad) |
                     reinterpret_cast<uintptr_t>(it.momentum_buf)) & 3) == 0,
                   "%s: tensor %d has a pointer that is not 4-byte aligned", who, i);
    }
    hipStream_t st = as_stream(stream);
    Launch L = {};
    L.momentum = momentum;
    L.one_minus_damp = 1.0f - dampening;
    L.grad_scale = grad_scale;
    L.nesterov = nesterov ? 1 : 0;
    L.clip = clip;
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
        if (clip) {
            CT_PROF("sgd_multi_kernel_clipped", st);
            hipLaunchKernelGGL(sgd_multi_kernel<true>, dim3((unsigned)blocks), dim3(THREADS), 0, st, L);
            CT_LAUNCH_CHECK("sgd_multi_kernel_clipped");
        } else {
            CT_PROF("sgd_multi_kernel", st);
            hipLaunchKernelGGL(sgd_multi_kernel<false>, dim3((unsigned)blocks), dim3(THREADS), 0, st, L);
            CT_LAUNCH_CHECK("sgd_multi_kernel");
        }
    }
    return CT_OK;
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
    using namespace ctdet;
    int64_t slots = 0;
    const int rc = check_grads("ct_grad_norm_clip", items, n, &slots);
    if (rc != CT_OK) return rc;
    CT_REQUIRE(max_norm > 0.f, "ct_grad_norm_clip: max_norm = %g must be positive (+inf: guard only)", (double)max_norm);
    CT_REQUIRE(state_dev != nullptr, "ct_grad_norm_clip: state_dev is NULL");
    CT_REQUIRE((reinterpret_cast<uintptr_t>(state_dev) & 3) == 0, "ct_grad_norm_clip: state_dev is not 4-byte aligned");
    const size_t need = sizeof(double) * (size_t)(slots > 0 ? slots : 1);
    CT_REQUIRE(workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
               "ct_grad_norm_clip: workspace is NULL or not 8-byte aligned");
    CT_REQUIRE(workspace_bytes >= need, "ct_grad_norm_clip: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    NormLaunch L = {};
    L.slots = static_cast<double*>(workspace);
    int64_t slot0 = 0;
    int i = 0;
    while (i < n) {
        int k = 0;
        int64_t blocks = 0;
        for (; i < n && k < GRADS_PER_LAUNCH; ++i) {
            const ct_grad_tensor& it = items[i];
            if (it.numel == 0) continue;
            L.g[k] = it.grad;
            L.numel[k] = (int)it.numel;
            L.first_block[k] = (int)blocks;
            blocks += grad_chunks(it);
            ++k;
        }
        if (k == 0) break;
        for (int q = k; q <= GRADS_PER_LAUNCH; ++q) L.first_block[q] = (int)blocks;
        L.n = k;
        L.slot0 = (int)slot0;
        CT_PROF("grad_norm_kernel", st);
        hipLaunchKernelGGL(grad_norm_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, L);
        CT_LAUNCH_CHECK("grad_norm_kernel");
        slot0 += blocks;
    }
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
    return sgd_step("ct_sgd_step", items, n, momentum, dampening, nesterov, grad_scale, nullptr, stream);
}

extern "C" int ct_sgd_step_clipped(const ct_sgd_tensor* items, int n, float momentum, float dampening, int nesterov,
                                   float grad_scale, const ct_clip_state* state_dev, ct_stream_t stream)
{
    CT_REQUIRE(state_dev != nullptr, "ct_sgd_step_clipped: state_dev is NULL");
    CT_REQUIRE((reinterpret_cast<uintptr_t>(state_dev) & 3) == 0, "ct_sgd_step_clipped: state_dev is not 4-byte aligned");
    return sgd_step("ct_sgd_step_clipped", items, n, momentum, dampening, nesterov, grad_scale, state_dev, stream);
}

extern "C" int ct_sgd_tensors_per_launch(void) { return TENSORS_PER_LAUNCH; }
