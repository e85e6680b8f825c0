// The claim / assign half the prediction-free and the prediction-aware matcher share (ct_atss.hip, ct_tal.hip): a selection
// kernel publishes one packed claim per positive with atomicMax into a zeroed [B,P] table, and one thread per (image, prior)
// turns the winning claim into the outputs ct_match_batched would write.  Both files are compiled with -ffp-contract=off.
#pragma once
#include "ct_box_math.h"
#include <cstdint>

#pragma clang fp contract(off)

namespace ctdet {

// A claim on a prior, ordered under atomicMax: forced over ordinary, then the larger IoU (a non-negative float's bits order
// like its value), then the lower box index.  Never 0, which stands for "no claim".
__device__ __forceinline__ unsigned long long pack_claim(bool forced, float iou, int g)
{
    return ((unsigned long long)(forced ? 1u : 0u) << 63) | ((unsigned long long)(__float_as_uint(iou) & 0x7FFFFFFFu) << 32) |
           (unsigned long long)(0xFFFFFFFFu - (unsigned)g);
}

// Prior p of image b: the winning claim, if any, becomes the matcher's outputs; every other prior gets zeros and (0, 1).
__device__ __forceinline__ void assign_claim(const float* __restrict__ truths, const int* __restrict__ gt_off,
                                             const float4* __restrict__ priors, int P, int b, int p,
                                             const unsigned long long* __restrict__ claims, float v0, float v1,
                                             float4* __restrict__ loc_t, float2* __restrict__ conf_t,
                                             uint8_t* __restrict__ obj_t, float* __restrict__ overlap)
{
    const size_t o = (size_t)b * P + p;
    const unsigned long long claim = claims[o];
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    float label = 0.f, weight = 1.f, ov = 0.f;
    if (claim != 0ull) {
        const int g = (int)(0xFFFFFFFFu - (unsigned)(claim & 0xFFFFFFFFull));
        const float* t = truths + (size_t)(gt_off[b] + g) * 6;
        ov = __uint_as_float((unsigned)(claim >> 32) & 0x7FFFFFFFu);
        label = t[4];
        weight = t[5];
        out = encode_box(make_float4(t[0], t[1], t[2], t[3]), priors[p], v0, v1);
    }
    loc_t[o] = out;
    conf_t[o] = make_float2(label, weight);
    obj_t[o] = label != 0.f ? 1 : 0;
    if (overlap) overlap[o] = ov;
}

}  // namespace ctdet
