// Device-side helpers every kernel file shares, defined once: the buffer descriptor, the vector types, and the split that
// defines the bf16x3 operand form.  A translation unit pulls in what it uses with using-declarations.
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

}  // namespace ctdet
