// The box expressions the matchers share (ct_box.hip: jaccard / match, ct_atss.hip: the ATSS matcher), defined once so that
// both write the same bits.  Every file that includes this is compiled with -ffp-contract=off; the pragma below says the
// same for whatever follows the include: each fp32 operation keeps the reference's rounding (no FMA contraction).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace ctdet {

// utils/box_utils.py:29-68: inter / (area_a + area_b - inter), no +1
__device__ __forceinline__ float iou_plain(const float4 a, const float4 b)
{
    const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
    const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
    const float inter = w * h;
    const float area_a = (a.z - a.x) * (a.w - a.y);
    const float area_b = (b.z - b.x) * (b.w - b.y);
    return inter / (area_a + area_b - inter);
}

// utils/box_utils.py:5-14
__device__ __forceinline__ float4 point_form(const float4 p)
{
    return make_float4(p.x - p.z / 2.f, p.y - p.w / 2.f, p.x + p.z / 2.f, p.y + p.w / 2.f);
}

// utils/box_utils.py:135-156: the offsets that take centre-form prior p to point-form box m
__device__ __forceinline__ float4 encode_box(const float4 m, const float4 p, float v0, float v1)
{
    float4 o;
    o.x = ((m.x + m.z) / 2.f - p.x) / (v0 * p.z);
    o.y = ((m.y + m.w) / 2.f - p.y) / (v0 * p.w);
    o.z = logf((m.z - m.x) / p.z) / v1;
    o.w = logf((m.w - m.y) / p.w) / v1;
    return o;
}

}  // namespace ctdet
