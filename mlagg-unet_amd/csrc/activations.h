// Pointwise activations and their derivatives, one definition each for every kernel (fp32 in registers; fast exponential).
#pragma once
#include <hip/hip_runtime.h>

namespace {

// exact (erf) GELU, the reference's nn.GELU()
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad_f(float x)
{
    const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
    return cdf + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float silu_f(float x) { return x / (1.f + __expf(-x)); }
__device__ __forceinline__ float dsilu_f(float x)
{
    const float s = 1.f / (1.f + __expf(-x));
    return s * (1.f + x * (1.f - s));
}

// softplus(x) = max(x, 0) + log1p(exp(-|x|)), also returning e = exp(-|x|) (the sigmoid of x follows from it without a second
// exponential).  e is in (0, 1]; for small e the series e - e^2/2 + e^3/3 (truncation < e^4/4 <= 2.5e-9 at e = 0.01) avoids the
// cancellation of log(1 + e), elsewhere v_log_f32 on 1 + e is accurate to ~1 ulp of a value in [0.01, 0.69].  ~10 VALU ops instead
// of the ~100 of libm's expf + log1pf, which were 45 % of the forward kernels' instructions (round-1 PMC).
__device__ __forceinline__ float softplus1(float x, float &e)
{
    e = __expf(-fabsf(x));
    const float small = e * (1.f - e * (0.5f - e * (1.f / 3.f)));
    const float big = __builtin_amdgcn_logf(1.f + e) * 0.6931471805599453f;   // bare v_log_f32 (log2): 1 + e >= 1, no denormal path needed
    return fmaxf(x, 0.f) + (e < 0.01f ? small : big);
}
__device__ __forceinline__ float softplus_f(float x)
{
    float e;
    return softplus1(x, e);
}
// d softplus(x)/dx = sigmoid(x) from the VALUE sp = softplus(x) >= 0 (what the scan backward has in hand): 1 - exp(-sp).  Just
// below 1 fp32 is spaced 2^-24, so the subtraction alone carries an absolute error of 6e-8 however small the result: 3e-5 of
// sigmoid(-6.9), the dt-init floor, and all of it at x = -16.  Below sp = 0.1 the alternating series sp - sp^2/2 + sp^3/6 - sp^4/24
// (truncation < sp^4/120: 8e-7 relative at 0.1) has no cancellation; above, 6e-8 is under 7e-7 of a result of 0.095 or more.
__device__ __forceinline__ float softplus_grad_from_value(float sp)
{
    const float small = sp * (1.f - sp * (0.5f - sp * ((1.f / 6.f) - sp * (1.f / 24.f))));
    return sp < 0.1f ? small : 1.f - __expf(-sp);
}

}  // namespace
