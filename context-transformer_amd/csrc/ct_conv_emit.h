// What the fp32-input direct convolutions (conv_igemm_f32 of ct_conv.hip, conv_x3_f32 of ct_conv_x3.hip) share on the device,
// written once: the finishing kernel of a split-K launch and the per-cout epilogue vectors staged through LDS.  Templates over the
// kernel-argument records (ConvArgs, X3Args), which agree in the member names used here.  The bf16 NHWC kernel has the transposed
// slab layout [Npix][M], bf16 residual / output and a finishing kernel of its own.
#pragma once
#include "ct_device.h"
#include "ct_f16x2.h"
#include <cmath>
#include <type_traits>

namespace ctdet {

// the record carries the f16x2 operand form's exponents (X3Args: eW, in_amax)
template <typename Args, typename = void>
struct has_f16x2_scale : std::false_type {};
template <typename Args>
struct has_f16x2_scale<Args, std::void_t<decltype(std::declval<const Args&>().eW)>> : std::true_type {};

// Per-cout epilogue vectors once per workgroup through LDS (the operand tiles are dead after the last barrier) instead of a
// per-lane global gather of scale / shift / floor for each of a lane's 64 outputs, which cost a third of the fixed time of a
// workgroup (1x1 16->1024 @19x19 bs 32, one k-step: 39.9 -> 25.8 us).  ev = [3][BM]: scale, shift, floor.  This is the entry of
// tile row i; the loop over the rows stays in the kernel (with it in here the compiler lays the kernel's blocks out differently),
// which synchronises before it reads.
template <int BM, typename Args>
__device__ __forceinline__ void stage_epilogue_vector(float* ev, const Args& a, int m0, int i)
{
    const int co = m0 + i;
    const bool in = co < a.M;
    ev[i] = in ? a.scale[co] : 0.f;
    ev[BM + i] = in ? a.shift[co] : 0.f;
    ev[2 * BM + i] = !in ? 0.f : a.lo ? a.lo[co] : (a.relu ? 0.f : -INFINITY);
}

// Finishing kernel of a split-K convolution: sum of the slabs in split order, then the arithmetic of the fused epilogue.
// f16x2 launches (a record with eW, non-null): the slabs hold sums scaled by 2^(eX[image] + eW).
template <typename Args>
__global__ __launch_bounds__(256) void conv_splitk_finish(const Args a)
{
    const int total = a.M * a.Npix;
    const bool track = a.out_amax != nullptr;
    const int rounds = (total + gridDim.x * 256 - 1) / (gridDim.x * 256);       // the same trip count for every lane (flush below)
    for (int it = 0; it < rounds; ++it) {
        const int idx = (it * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        float amax_run = 0.f;
        int img = -1;
        if (idx < total) {
            const int co = idx / a.Npix, P = idx - co * a.Npix;
            const int n = P / a.OHW, s = P - n * a.OHW;
            img = n;
            float sum = a.ws[idx];
            for (int k = 1; k < a.ksplit; ++k) sum += a.ws[(size_t)k * total + idx];
            if constexpr (has_f16x2_scale<Args>::value) {
                h2::pow2x2 ymul{1.f, 1.f};
                if (a.eW) ymul = h2::unscale_for(*a.eW, h2::image_exponent(a.in_amax, n, h2::kGrowthNone));
                sum = (sum * ymul.lo) * ymul.hi;
            }
            float v = sum * a.scale[co] + a.shift[co];
            if (a.res) v = v * a.res_scale + a.res[((size_t)n * a.res_ctot + a.res_coff + co) * a.OHW + s];
            if (a.lo) { const float fl = a.lo[co]; v = v < fl ? fl : v; }      // NaN propagates
            else if (a.relu) v = v < 0.f ? 0.f : v;
            if (track) h2::track_absmax(amax_run, v);
            if (a.nseg == 0) a.out[((size_t)n * a.out_ctot + a.out_coff + co) * a.OHW + s] = v;
            else scatter_segments(a, n, s, co, v);
        }
        if (track) h2::flush_absmax(a.out_amax, img, amax_run);      // every lane arrives here
    }
}

}  // namespace ctdet
