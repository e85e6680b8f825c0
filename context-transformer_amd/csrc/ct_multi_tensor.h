// What the multi-tensor element-wise kernels share (ct_optim.hip: the SGD step, with and without a weight average, and
// the gradient norm; ct_ema.hip: the average alone and the exchange; ct_adamw.hip: the AdamW step).
//
// Device side.  The tensor table and the first workgroup of every tensor travel in the kernel arguments (no device
// table, no staging copy, nothing read from the caller's array after the call returns); a workgroup finds its tensor
// by a binary search over the prefix sums (owner_of), which are scalar loads from the kernel-argument segment, and owns
// one CHUNK of it.  walk<Op> is the one place a map kernel's chunk is walked: a tensor whose pointers share their
// offset inside a 16-byte line is walked in 16-byte groups counted from the line that holds element 0 -- every whole
// group is a dwordx4 load / store, UNROLL of them in flight, and only the first and the last group of the tensor can be
// partial (scalar, bounds-checked per element); a tensor whose pointers disagree is walked one dword per lane, still
// coalesced.  No byte outside [ptr, ptr + numel) is read or written; plain vector stores only.  update() and ema_of()
// are the arithmetic of include/ctdet.h, one rounding per line, so that every kernel that applies them produces the
// same bits.
//
// Host side.  vec_flags / chunks_of are the rule that decides between the two walks and the chunk count that follows
// from it; check_table / check_tensor / check_chunks / check_state are the argument checks every entry point makes;
// pack() fills launch records from the caller's items and launch() sends one.
#pragma once

#include "ct_common.h"

#include <climits>
#include <cstdint>

namespace ctdet {
namespace mt {

constexpr int THREADS = 256;
constexpr int CHUNK = 8192;                 // elements per workgroup: 8 dwordx4 groups per lane, issued 4 at a time
constexpr int GROUPS = CHUNK / 4;           // 16-byte groups per chunk
constexpr int UNROLL = 4;
constexpr int64_t MAX_NUMEL = 2147483647;

enum { F_FIRST = 1, F_VEC = 2, F_SHIFT = 4 /* bits 2-3: elements between the 16-byte line and element 0 */ };

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

__device__ inline void update(float4& p, const float4& g, float4& b, const Hyper& h)
{
    update(p.x, g.x, b.x, h);
    update(p.y, g.y, b.y, h);
    update(p.z, g.z, b.z, h);
    update(p.w, g.w, b.w, h);
}

// include/ctdet.h, ct_sgd_step_ema: ema = d * ema + (1 - d) * x, three roundings
__device__ inline float ema_of(float e, float x, float d, float om)
{
    return __fadd_rn(__fmul_rn(d, e), __fmul_rn(om, x));
}

__device__ inline float4 ema_of(const float4& e, const float4& x, float d, float om)
{
    return make_float4(ema_of(e.x, x.x, d, om), ema_of(e.y, x.y, d, om), ema_of(e.z, x.z, d, om), ema_of(e.w, x.w, d, om));
}

// The tensor that owns workgroup `blk`: the last entry whose first workgroup is <= blk
template <int N>
__device__ inline int owner_of(const int (&first_block)[N], int n, int blk)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk >= first_block[mid]) lo = mid; else hi = mid;
    }
    return lo;
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
// The loads of UNROLL groups are issued before the first result is stored.
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

// ---------------------------------------------------------------------------------------------------- host side
// elements between the 16-byte line that holds *p and p
inline int line_offset(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

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
    return ceil_div<int64_t>(numel + ((flags & F_VEC) ? (flags >> 2) & 3 : 0), CHUNK);
}

// n and the table pointer, as every multi-tensor entry checks them; -> CT_OK or the recorded failure, as all checks
inline int check_table(const char* who, const void* items, int n)
{
    CT_REQUIRE(n >= 0, "%s: n = %d is negative", who, n);
    CT_REQUIRE(n == 0 || items != nullptr, "%s: items is NULL with n = %d", who, n);
    return CT_OK;
}

// One pointer of a tensor for check_tensor; if_null replaces "a NULL <name>" in the message
struct Ptr {
    const void* p;
    const char* name;
    bool may_be_null;
    const char* if_null = nullptr;
};

// numel, then the pointers in the order given, then their alignment.  A tensor of no elements is a no-op whatever its
// pointers are (an empty tensor may have none).
template <int N>
inline int check_tensor(const char* who, int i, int64_t numel, const Ptr (&ptrs)[N])
{
    CT_REQUIRE(numel >= 0 && numel <= MAX_NUMEL, "%s: tensor %d has numel %lld (0 .. 2^31-1)", who, i, (long long)numel);
    if (numel == 0) return CT_OK;
    uintptr_t bits = 0;
    for (const Ptr& f : ptrs) {
        if (!f.p && !f.may_be_null)
            return f.if_null ? fail(CT_ERR_INVALID, "%s: tensor %d has %s", who, i, f.if_null)
                             : fail(CT_ERR_INVALID, "%s: tensor %d has a NULL %s", who, i, f.name);
        bits |= reinterpret_cast<uintptr_t>(f.p);
    }
    CT_REQUIRE((bits & 3) == 0, "%s: tensor %d has a %s that is not 4-byte aligned", who, i, N == 1 ? ptrs[0].name : "pointer");
    return CT_OK;
}

// the most chunks a tensor of `numel` elements takes, whatever its pointers are
inline int64_t max_chunks(int64_t numel) { return numel ? ceil_div<int64_t>(numel + 3, CHUNK) : 0; }

inline int check_chunks(const char* who, int64_t total)
{
    CT_REQUIRE(total <= INT_MAX, "%s: %lld chunks of %d elements are more than a call takes", who, (long long)total, CHUNK);
    return CT_OK;
}

// A 16-byte device state (ct_clip_state, ct_ema_state); `what` names it in the messages
inline int check_state(const char* who, const void* state, const char* what, bool may_be_null = false)
{
    CT_REQUIRE(state != nullptr || may_be_null, "%s: %s is NULL", who, what);
    CT_REQUIRE((reinterpret_cast<uintptr_t>(state) & 3) == 0, "%s: %s is not 4-byte aligned", who, what);
    return CT_OK;
}

// Packs items 0 .. n-1 into launch records and sends each full one.  fill(L, k, i) writes entry k of L from item i and
// returns its chunk count, 0 for an empty tensor (skipped); go(L, blocks) launches `blocks` workgroups over L.
// first_block[k ..] of the last, shorter table is padded with the total, so the search never reads a stale sum.
template <class LaunchT, class Fill, class Go>
inline int pack(LaunchT& L, int n, Fill fill, Go go)
{
    constexpr int CAP = (int)(sizeof(L.first_block) / sizeof(int)) - 1;
    int i = 0;
    while (i < n) {
        int k = 0;
        int64_t blocks = 0;
        for (; i < n && k < CAP; ++i) {
            const int64_t chunks = fill(L, k, i);
            if (chunks == 0) continue;
            L.first_block[k++] = (int)blocks;
            blocks += chunks;
        }
        if (k == 0) break;
        for (int q = k; q <= CAP; ++q) L.first_block[q] = (int)blocks;
        L.n = k;
        if (const int rc = go(L, (unsigned)blocks)) return rc;
    }
    return CT_OK;
}

// One launch of THREADS-wide workgroups under the name the profile records and the error messages carry
template <class LaunchT>
inline int launch(const char* name, void (*kernel)(LaunchT), const LaunchT& L, unsigned blocks, hipStream_t st)
{
    CT_PROF(name, st);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(THREADS), 0, st, L);
    CT_LAUNCH_CHECK(name);
    return CT_OK;
}

}  // namespace mt
}  // namespace ctdet
