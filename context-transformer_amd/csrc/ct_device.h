// Device-side helpers every kernel file shares, defined once: the buffer descriptor, the vector types, the split that
// defines the bf16x3 operand form, the accumulator row of the 32x32 MFMA and the multibox head scatter.  A translation unit pulls in what it uses with using-declarations.
#pragma once
#include <hip/hip_runtime.h>

namespace ctdet {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kInvalidOff = 0x7FFFFFF0;          // >= num_records of every descriptor -> loads 0
constexpr long long kMaxBufBytes = 0x7FFFFF00LL;  // descriptors stay below 2 GiB

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// x = hi + mid + lo exactly (3 x 8 significant bits by truncation); the upper halves of the three words are the pieces.
// The order of the two subtractions is the operand form: every packer and every kernel that splits must agree bit for bit.
__device__ __forceinline__ void split3(float x, unsigned& h, unsigned& m, unsigned& l)
{
    h = __builtin_bit_cast(unsigned, x) & 0xFFFF0000u;
    const float r1 = x - __builtin_bit_cast(float, h);
    m = __builtin_bit_cast(unsigned, r1) & 0xFFFF0000u;
    l = __builtin_bit_cast(unsigned, r1 - __builtin_bit_cast(float, m));
}

__device__ __forceinline__ int pack_hi(unsigned e0, unsigned e1)      // [bf16 e0 | bf16 e1 << 16]
{
    return (int)__builtin_amdgcn_perm(e1, e0, 0x07060302u);
}

// row of a 32x32 MFMA accumulator block that register r (0..15) of a lane in half hsel (lane >> 5) holds; the column is lane & 31
__device__ __forceinline__ constexpr int acc_row(int r, int hsel) { return (r & 3) + 8 * (r >> 2) + 4 * hsel; }

// One value of output channel co at pixel s of image n into the flattened multibox head buffers (ct_out_segment: channels-last
// per segment).  Args is any kernel-argument record with nseg and seg[3].
template <typename Args>
__device__ __forceinline__ void scatter_segments(const Args& a, int n, int s, int co, float v)
{
#pragma unroll
    for (int g = 0; g < 3; ++g)
        if (g < a.nseg && co >= a.seg[g].co_begin && co < a.seg[g].co_end)
            a.seg[g].ptr[(size_t)n * a.seg[g].img_stride + a.seg[g].base +
                         (size_t)s * a.seg[g].pix_stride + (co - a.seg[g].co_begin)] = v;
}

}  // namespace ctdet
