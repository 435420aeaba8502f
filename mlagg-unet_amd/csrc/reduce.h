// Wave-level reductions and fences shared by the kernels (wave64).  A reduction that differs from these in order, width or LDS
// layout stays with its kernel: sums here are bit-exact contracts, not conveniences.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// butterfly over the 64 lanes, widest step first: every lane ends with the same total
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the per-wave totals of a 256-thread workgroup (red[wave], written by lane 0 of each wave), added in a fixed order
__device__ __forceinline__ float sum4(const float *red) { return (red[0] + red[1]) + (red[2] + red[3]); }

// exchanges within a quad of lanes on the DPP path (no LDS crossbar): lane ^ 1, lane ^ 2
__device__ __forceinline__ float dpp_quad_xor1(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_quad_xor2(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
}
__device__ __forceinline__ float quad_sum(float v)
{
    v += dpp_quad_xor1(v);
    v += dpp_quad_xor2(v);
    return v;
}

}  // namespace
