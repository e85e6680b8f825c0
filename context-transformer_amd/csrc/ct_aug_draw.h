// The counter-based generator and the draw rules of the device input pipeline (include/ctdet.h GENERATOR, DRAW RULES),
// and the workgroup scan of its pack launches: what ct_aug_plan.hip and ct_affine.hip share.  Both compile with
// contraction off; ctdet/aug_plan_ref.py evaluates the same expressions in numpy.
#pragma once
#include <hip/hip_runtime.h>

namespace ctdet {
namespace aug {

struct Words { unsigned w[4]; };

// Philox4x32-10: key = seed, counter = (id lo, id hi, slot, lane)
__device__ inline Words philox(unsigned long long seed, unsigned long long sample_id, unsigned slot, unsigned lane)
{
    unsigned c0 = (unsigned)sample_id, c1 = (unsigned)(sample_id >> 32), c2 = slot, c3 = lane;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)c0 * 0xD2511F53u, p1 = (unsigned long long)c2 * 0xCD9E8D57u;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (unsigned)p1; c2 = n2; c3 = (unsigned)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Words o;
    o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

__device__ __forceinline__ double unit(unsigned w) { return (double)w * 2.3283064365386962890625e-10; }   // w * 2^-32
__device__ __forceinline__ double uniform(double a, double b, unsigned w) { return a + (b - a) * unit(w); }
__device__ __forceinline__ int randrange(int n, unsigned w) { return (int)(((unsigned long long)w * (unsigned)n) >> 32); }

constexpr int PACK_THREADS = 1024;

// inclusive scan over the workgroup's PACK_THREADS values (Hillis-Steele in LDS); IS_MAX: running maximum, else sum
template <bool IS_MAX>
__device__ inline int block_scan(int v, int* sh)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < PACK_THREADS; d <<= 1) {
        const int o = tid >= d ? sh[tid - d] : (IS_MAX ? -1 : 0);
        __syncthreads();
        v = IS_MAX ? max(v, o) : v + o;
        sh[tid] = v;
        __syncthreads();
    }
    return v;
}

}  // namespace aug
}  // namespace ctdet
