// What the multi-tensor element-wise kernels share (ct_optim.hip: the SGD step and the gradient norm; ct_ema.hip: the
// SGD step with a weight average, the average alone, the exchange): the chunk geometry, the search that gives a
// workgroup its tensor, the rule that decides between 16-byte and dword accesses, and the SGD recurrence itself, so
// that every kernel that applies it produces the same bits.
#pragma once

#include "ct_common.h"

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

__device__ inline void update4(float4& p, float4 g, float4& b, const Hyper& h)
{
    update(p.x, g.x, b.x, h);
    update(p.y, g.y, b.y, h);
    update(p.z, g.z, b.z, h);
    update(p.w, g.w, b.w, h);
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

// elements between the 16-byte line that holds *p and p
inline int line_offset(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

}  // namespace mt
}  // namespace ctdet
