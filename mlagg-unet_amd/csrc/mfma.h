// Operand vectors, 16-bit packing and the 32x32x16 matrix instruction, shared by every kernel that feeds the 16-bit matrix cores
// (K4lp, K5 and its variants, K18/K19 through bf16x3.h / opmode.h, the 16-bit map I/O of lpio.h).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));      // a native vector: arrays of HIP's uint4 struct land in scratch
typedef unsigned short u16;

// two fp32 -> one dword of two 16-bit values (round to nearest even), low half = first value
template <bool BF16>
__device__ __forceinline__ unsigned pack2(float a, float b)
{
    if (BF16) {
        const __hip_bfloat162 v = __float22bfloat162_rn(make_float2(a, b));
        return *reinterpret_cast<const unsigned *>(&v);
    }
    const __half2 v = __floats2half2_rn(a, b);
    return *reinterpret_cast<const unsigned *>(&v);
}

template <bool BF16>
__device__ __forceinline__ u16 cvt1(float a) { return (u16)(pack2<BF16>(a, 0.f) & 0xffff); }

template <bool BF16>
__device__ __forceinline__ uint4 pack8(const float *v)
{
    return make_uint4(pack2<BF16>(v[0], v[1]), pack2<BF16>(v[2], v[3]), pack2<BF16>(v[4], v[5]), pack2<BF16>(v[6], v[7]));
}

// v_mfma_f32_32x32x16_{bf16,f16}: a lane's operand is 8 consecutive k of one row (one dword pair per pack2)
template <bool BF16>
__device__ __forceinline__ f32x16 mfma16(const uint4 &a, const uint4 &b, f32x16 c)
{
    if (BF16)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8 *>(&a), *reinterpret_cast<const bf16x8 *>(&b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8 *>(&a), *reinterpret_cast<const f16x8 *>(&b), c, 0, 0, 0);
}

__device__ __forceinline__ f32x16 zero16()
{
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

// row index of accumulator register v in lane half kh (D layout of the 32x32 MFMA)
__device__ __forceinline__ int acc_row(int v, int kh) { return (v & 3) + 8 * (v >> 2) + 4 * kh; }

}  // namespace
