// The step tail: gradient-norm clipping + the optimizer update for all parameters of the network in three launches (K11, K34, K35).
//
// Replaces `torch.nn.utils.clip_grad_norm_(parameters, 12)` + `optimizer.step()` of the train step (reference
// nnUNetTrainer.py:855-857): ATen runs a multi-tensor norm, a multi-tensor scale of every gradient and 15 multi-tensor AdamW
// launches at ~1.2 TB/s (0.9 ms per step for the 27 M parameters).  Here
//   1. sumsq : every work item (a <= 64 Ki-element chunk of one gradient) writes its fp32 sum of squares as one double partial;
//   2. reduce: one block adds the partials up in a fixed order (bit-reproducible) and, in the device form, advances the step counter;
//   3. update: the clip coefficient min(1, max_norm / (norm + 1e-6)) is formed ON THE DEVICE from that total -- no host
//              synchronisation -- and applied to the gradient as it is read.  The gradients themselves are left unscaled in memory
//              (torch rewrites them: 216 MB of extra traffic).
// Tensors are addressed through a device table of (param, grad, state 0, state 1, numel) rows and a work list of (tensor, chunk)
// pairs, both built by the host wrapper.  The update kernel is instantiated per kind (MLAGG_OPT_* of the header) and reads / writes
// only the state tensors its kind has.  HBM-bound: 4 bytes per parameter for the norm, and for the update
//   ADAMW          28  torch.optim.AdamW, amsgrad off (the optimizer of nnUNetTrainer_MLAgg_2D_dt_MS.py:137-147; K11)
//   SGD_NESTEROV   20  the base trainer's SGD with Nesterov momentum (nnUNetTrainer.py:448-452; K34)
//   ADAMW_AMSGRAD  36  nnUNetTrainerAdam's AdamW with amsgrad (K34)
//   ADAM_L2        28  nnUNetTrainerVanillaAdam's Adam with L2 decay (K34)
// ADAMW rounds its betas to float before anything is formed from them; the other Adam kinds form 1 - beta and the bias corrections
// from the double betas, as torch does.
//
// Loss-scaled form (K35, SCALED = true, all four kinds): the norm pass squares g / scale, the reduce decides what
// torch.amp.GradScaler decides on the host (found_inf, the skipped step, the new scale and growth tracker) and leaves the gradient
// multiplier (1 / scale) * clip coefficient for the update, which returns at once on a skipped step.  The gradients stay SCALED and
// unclipped in memory: torch's unscale_ rewrites every one of them, here no byte more moves than in the unscaled form.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlagg_hip.h"
#include "prof.h"
#include "reduce.h"

namespace {

constexpr int CHUNK = 65536;          // elements per work item
constexpr int OPT_TPB = 256;

struct TensorRow {                    // mirrors the int64 x 5 rows of the host table
    float *p;
    const float *g;
    float *m;
    float *v;
    long long n;
};

// 1 / scale as torch.amp.GradScaler forms it (_scale.double().reciprocal().float())
__device__ __forceinline__ float inv_scale_of(const float *__restrict__ scale) { return (float)(1.0 / (double)*scale); }

// SCALED: the gradients carry the loss scale *scale; the sum is that of the UNSCALED gradients (g / scale)^2, the norm the
// reference clips on (unscale_ comes before clip_grad_norm_).  An inf or NaN element, or a square beyond fp32, makes the partial non-finite.
template <bool SCALED>
__global__ void __launch_bounds__(OPT_TPB)
adamw_sumsq_kernel(const TensorRow *__restrict__ table, const int2 *__restrict__ work, double *__restrict__ sumsq,
             const float *__restrict__ scale)
{
    __shared__ float red[OPT_TPB / 64];
    const int2 w = work[blockIdx.x];
    const TensorRow t = table[w.x];
    const long long lo = (long long)w.y * CHUNK, hi = min(lo + CHUNK, t.n);
    const float *g = t.g + lo;
    const long long n = hi - lo;
    const float inv = SCALED ? inv_scale_of(scale) : 1.f;
    float s = 0.f;
    if ((((uintptr_t)g) & 15) == 0) {
        const long long n4 = n >> 2;
        for (long long i = threadIdx.x; i < n4; i += OPT_TPB) {
            float4 a = reinterpret_cast<const float4 *>(g)[i];
            if (SCALED) a.x *= inv, a.y *= inv, a.z *= inv, a.w *= inv;
            s += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
        }
        for (long long i = 4 * n4 + threadIdx.x; i < n; i += OPT_TPB) {
            const float a = SCALED ? g[i] * inv : g[i];
            s += a * a;
        }
    } else {
        for (long long i = threadIdx.x; i < n; i += OPT_TPB) {
            const float a = SCALED ? g[i] * inv : g[i];
            s += a * a;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    // one partial per work item, added up in a fixed order by the reduce kernels (a double atomic add made the clip
    // coefficient -- hence every parameter -- depend on the arrival order in the last bit)
    if (threadIdx.x == 0) sumsq[1 + blockIdx.x] = (double)sum4(red);
}

// the fixed-order total of the n_work partials behind sumsq[0]
__device__ __forceinline__ double sumsq_total(const double *__restrict__ sumsq, int n_work)
{
    __shared__ double red[OPT_TPB];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_work; i += OPT_TPB) s += sumsq[1 + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = OPT_TPB / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}

__global__ void __launch_bounds__(OPT_TPB)
adamw_sumsq_reduce_kernel(double *__restrict__ sumsq, int n_work, int *__restrict__ step_dev)
{
    // device-resident step counter (the hipGraph form of the step): advanced here, read by the update kernel behind this one
    if (step_dev && threadIdx.x == 0) *step_dev += 1;
    const double total = sumsq_total(sumsq, n_work);
    if (threadIdx.x == 0) sumsq[0] = total;
}

struct AdamArgs {
    float lr, beta1, beta2, eps, weight_decay, max_norm, bias_c1, bias_c2_sqrt;
};

// min(1, max_norm / (norm + 1e-6)) from the squared norm; 1 without clipping
__device__ __forceinline__ float clip_coef_of(float max_norm, double total)
{
    if (!(max_norm > 0.f)) return 1.f;
    const float norm = (float)sqrt(total);
    // a non-finite norm poisons EVERY parameter, as clip_grad_norm_'s NaN coefficient does (fminf(NaN, 1) = 1 would
    // keep stepping the finite gradients and hide the failure)
    return (norm == norm && norm < __builtin_huge_valf()) ? fminf(max_norm / (norm + 1e-6f), 1.f) : __builtin_nanf("");
}

// The reduce of the loss-scaled step: the same fixed-order total (of the unscaled squares), then, in one thread, everything
// torch.amp.GradScaler decides on the host between unscale_ and update:
//   found_inf  1 when the total is not finite (an inf or NaN gradient element; ALSO finite elements whose unscaled square, or a
//              work item's fp32 sum of such squares, leaves fp32 -- |g / scale|, or the norm of a 64 Ki-element chunk, above
//              1.8e19 -- where torch would step with a zero coefficient), else 0;
//   step_dev   advanced on a good step only (torch never calls the optimizer on a skipped one);
//   grad_mult  (1 / scale) * clip coefficient, formed from the scale the gradients were produced with: what the update kernel
//              multiplies every gradient by as it reads it;
//   scale, growth_tracker  torch._amp_update_scale_: backoff and tracker 0 on overflow; else count up and, at growth_interval,
//              grow if the product is finite and reset the tracker.
__global__ void __launch_bounds__(OPT_TPB)
scaled_sumsq_reduce_kernel(double *__restrict__ sumsq, int n_work, int *__restrict__ step_dev, float *__restrict__ scale,
                           int *__restrict__ growth_tracker, float *__restrict__ found_inf, float *__restrict__ grad_mult,
                           float max_norm, double growth_factor, double backoff_factor, int growth_interval)
{
    const double total = sumsq_total(sumsq, n_work);
    if (threadIdx.x != 0) return;
    sumsq[0] = total;
    const bool bad = !(total == total) || total >= __builtin_huge_val();
    const float old_scale = *scale;
    *found_inf = bad ? 1.f : 0.f;
    if (bad) {
        *grad_mult = 0.f;                                 // never read: the update kernel returns on found_inf
        *scale = (float)((double)old_scale * backoff_factor);
        *growth_tracker = 0;
        return;
    }
    *step_dev += 1;
    *grad_mult = (float)(1.0 / (double)old_scale) * clip_coef_of(max_norm, total);
    const int successful = *growth_tracker + 1;
    if (successful == growth_interval) {
        const float grown = (float)((double)old_scale * growth_factor);
        if (grown == grown && fabsf(grown) < __builtin_huge_valf()) *scale = grown;
        *growth_tracker = 0;
    } else {
        *growth_tracker = successful;
    }
}

// KIND (MLAGG_OPT_* of the header) and the state tensors of a row: SGD_NESTEROV m = momentum_buffer (v unused, may be null);
// ADAMW_AMSGRAD m, v and a third tensor max_exp_avg_sq, whose address comes from `extra` (one pointer per table row: the 5 x 8-byte
// row stays as it is); ADAMW and ADAM_L2 m, v.  a.beta1 carries the momentum of SGD.
template <int KIND>
__device__ __forceinline__ void opt_one(float &p, float g, float &m, float &v, float &vmax, const AdamArgs &a, float coef, float omb1,
                                        float omb2)
{
    g *= coef;
    if (KIND == MLAGG_OPT_SGD_NESTEROV) {
        g += a.weight_decay * p;                          // torch.optim.SGD: L2 decay, dampening 0
        m = a.beta1 * m + g;                              // a zero buffer gives torch's first step (buf = g)
        p -= a.lr * (g + a.beta1 * m);
        return;
    }
    if (KIND == MLAGG_OPT_ADAM_L2)
        g += a.weight_decay * p;
    else
        p *= 1.f - a.lr * a.weight_decay;
    m = a.beta1 * m + omb1 * g;                           // torch: exp_avg.lerp_(grad, 1 - beta1)
    v = a.beta2 * v + omb2 * g * g;
    float s = v;
    if (KIND == MLAGG_OPT_ADAMW_AMSGRAD) {
        vmax = (v > vmax || v != v) ? v : vmax;           // torch.maximum: a NaN moment stays a NaN
        s = vmax;
    }
    const float denom = sqrtf(s) / a.bias_c2_sqrt + a.eps;
    p -= (a.lr / a.bias_c1) * (m / denom);
}

// SCALED: a skipped step (found_inf set by the reduce) leaves parameters and state untouched; otherwise the gradient multiplier
// (1 / scale) * clip coefficient stands where the clip coefficient stood.  Gradients stay scaled and unclipped in memory.
template <int KIND, bool SCALED>
__global__ void __launch_bounds__(OPT_TPB)
opt_update_kernel(const TensorRow *__restrict__ table, float *const *__restrict__ extra, const int2 *__restrict__ work,
                  const double *__restrict__ sumsq, AdamArgs a, double beta1, double beta2, const float *__restrict__ lr_dev,
                  const int *__restrict__ step_dev, const float *__restrict__ found_inf, const float *__restrict__ grad_mult)
{
    constexpr bool SGD = KIND == MLAGG_OPT_SGD_NESTEROV, AMS = KIND == MLAGG_OPT_ADAMW_AMSGRAD, F32_BETAS = KIND == MLAGG_OPT_ADAMW;
    if (SCALED && *found_inf != 0.f) return;
    // ADAMW forms 1 - beta and the bias corrections from the betas rounded to float.  The other kinds form them from the betas in
    // double, as torch does: beta2 rounded to float first is 1.3e-8 off, its 1000th power 1.3e-5 (and 1.f - 0.999f is 1.3e-5 off
    // 0.001), and at a learning rate of 1e-2 that shows in the parameters
    if (F32_BETAS) beta1 = (double)a.beta1, beta2 = (double)a.beta2;
    if (lr_dev) {
        // learning rate and step live on the device (a captured launch cannot carry them as arguments): the same double-precision
        // bias corrections the launch-argument form passes in
        a.lr = *lr_dev;
        if (!SGD) {
            const double step = (double)*step_dev;
            a.bias_c1 = (float)(1.0 - pow(beta1, step));
            a.bias_c2_sqrt = (float)sqrt(1.0 - pow(beta2, step));
        }
    }
    const int2 w = work[blockIdx.x];
    const TensorRow t = table[w.x];
    const long long lo = (long long)w.y * CHUNK, hi = min(lo + CHUNK, t.n);
    const long long n = hi - lo;
    const float coef = SCALED ? *grad_mult : clip_coef_of(a.max_norm, *sumsq);
    const float omb1 = F32_BETAS ? 1.f - a.beta1 : (float)(1.0 - beta1), omb2 = F32_BETAS ? 1.f - a.beta2 : (float)(1.0 - beta2);
    // a kind reads and writes only the state tensors it has; the others alias m and are never touched
    float *p = t.p + lo, *m = t.m + lo, *v = SGD ? m : t.v + lo, *x = AMS ? extra[w.x] + lo : m;
    const float *g = t.g + lo;
    const bool al = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)x)) & 15) == 0;
    const long long n4 = al ? n >> 2 : 0;
    // Which product of beta * state + (1 - beta) * g [* g], and of p (1 - lr wd) - step, the compiler fuses into the FMA follows the
    // order in which the state and the gradient are loaded and whether an intermediate is stored, and the last bit of the moments
    // and parameters follows that choice.  ADAMW keeps the forms it has had since K11 (float4 loop: v loaded before g; tail: on the
    // elements in memory), the other kinds theirs (g behind m, in front of v; tail: on copies, g last): do not reorder the loads or
    // stores of either loop without comparing parameter bits
    for (long long i = threadIdx.x; i < n4; i += OPT_TPB) {
        float4 p4 = reinterpret_cast<float4 *>(p)[i], m4 = reinterpret_cast<float4 *>(m)[i];
        float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f), x4 = v4;
        if (F32_BETAS) v4 = reinterpret_cast<float4 *>(v)[i];
        const float4 g4 = reinterpret_cast<const float4 *>(g)[i];
        if (!SGD && !F32_BETAS) v4 = reinterpret_cast<float4 *>(v)[i];
        if (AMS) x4 = reinterpret_cast<float4 *>(x)[i];
        opt_one<KIND>(p4.x, g4.x, m4.x, v4.x, x4.x, a, coef, omb1, omb2);
        opt_one<KIND>(p4.y, g4.y, m4.y, v4.y, x4.y, a, coef, omb1, omb2);
        opt_one<KIND>(p4.z, g4.z, m4.z, v4.z, x4.z, a, coef, omb1, omb2);
        opt_one<KIND>(p4.w, g4.w, m4.w, v4.w, x4.w, a, coef, omb1, omb2);
        reinterpret_cast<float4 *>(p)[i] = p4;
        reinterpret_cast<float4 *>(m)[i] = m4;
        if (!SGD) reinterpret_cast<float4 *>(v)[i] = v4;
        if (AMS) reinterpret_cast<float4 *>(x)[i] = x4;
    }
    for (long long i = 4 * n4 + threadIdx.x; i < n; i += OPT_TPB) {
        if (F32_BETAS) {                                  // in memory, as K11's tail always worked
            float none = 0.f;
            opt_one<KIND>(p[i], g[i], m[i], v[i], none, a, coef, omb1, omb2);
            continue;
        }
        float pi = p[i], mi = m[i], vi = SGD ? 0.f : v[i], xi = AMS ? x[i] : 0.f;
        opt_one<KIND>(pi, g[i], mi, vi, xi, a, coef, omb1, omb2);
        p[i] = pi;
        m[i] = mi;
        if (!SGD) v[i] = vi;
        if (AMS) x[i] = xi;
    }
}

// The device-resident state of the loss-scaled step and the factors of its scale update.
struct ScaleState {
    float *scale;
    int *growth_tracker;
    float *found_inf, *grad_mult;
    double growth_factor, backoff_factor;
    int growth_interval;
};

template <int KIND>
void launch_update(const TensorRow *table, float *const *extra, const int2 *work, int n_work, const double *sumsq, const AdamArgs &a,
                   double beta1, double beta2, const float *lr_dev, const int *step_dev, const ScaleState *ss, hipStream_t st)
{
    if (ss)
        hipLaunchKernelGGL((opt_update_kernel<KIND, true>), dim3(n_work), dim3(OPT_TPB), 0, st, table, extra, work, sumsq, a, beta1,
                           beta2, lr_dev, step_dev, (const float *)ss->found_inf, (const float *)ss->grad_mult);
    else
        hipLaunchKernelGGL((opt_update_kernel<KIND, false>), dim3(n_work), dim3(OPT_TPB), 0, st, table, extra, work, sumsq, a, beta1,
                           beta2, lr_dev, step_dev, (const float *)nullptr, (const float *)nullptr);
}

// The launches of one step of `kind`.  lr_dev / step_dev null: the launch-argument form, with the 1-based `step` for the bias
// corrections of the Adam kinds; else the device form (`step` unused).  ss non-null: the loss-scaled step, device form only.
int step_launch(int kind, const void *tensor_table, const void *extra_table, const void *work_list, int n_work, double *sumsq, AdamArgs a,
                double beta1, double beta2, int step, const float *lr_dev, int *step_dev, const ScaleState *ss, void *stream)
{
    if (!tensor_table || !work_list || !sumsq) return MLAGG_E_NULLPTR;
    if (kind < MLAGG_OPT_SGD_NESTEROV || kind > MLAGG_OPT_ADAMW || (kind == MLAGG_OPT_ADAMW_AMSGRAD && !extra_table) || n_work <= 0)
        return MLAGG_E_UNSUPPORTED;
    if (ss && ss->growth_interval < 1) return MLAGG_E_UNSUPPORTED;
    if (!step_dev && kind != MLAGG_OPT_SGD_NESTEROV) {
        if (step < 1) return MLAGG_E_UNSUPPORTED;
        const bool f32_betas = kind == MLAGG_OPT_ADAMW;   // the rounding rule of opt_update_kernel
        a.bias_c1 = (float)(1.0 - pow(f32_betas ? (double)a.beta1 : beta1, (double)step));
        a.bias_c2_sqrt = (float)sqrt(1.0 - pow(f32_betas ? (double)a.beta2 : beta2, (double)step));
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const TensorRow *table = static_cast<const TensorRow *>(tensor_table);
    float *const *extra = static_cast<float *const *>(extra_table);
    const int2 *work = static_cast<const int2 *>(work_list);
    const bool clip = a.max_norm > 0.f;
    mlagg_prof::Scope mlagg_prof_scope(kind == MLAGG_OPT_ADAMW ? mlagg_prof::K_ADAMW : mlagg_prof::K_OPT_VARIANTS, st);
    if (ss) {
        // the norm pass always runs: it finds the overflow
        hipLaunchKernelGGL(adamw_sumsq_kernel<true>, dim3(n_work), dim3(OPT_TPB), 0, st, table, work, sumsq, (const float *)ss->scale);
        hipLaunchKernelGGL(scaled_sumsq_reduce_kernel, dim3(1), dim3(OPT_TPB), 0, st, sumsq, n_work, step_dev, ss->scale,
                           ss->growth_tracker, ss->found_inf, ss->grad_mult, a.max_norm, ss->growth_factor, ss->backoff_factor,
                           ss->growth_interval);
    } else {
        if (clip)
            hipLaunchKernelGGL(adamw_sumsq_kernel<false>, dim3(n_work), dim3(OPT_TPB), 0, st, table, work, sumsq, (const float *)nullptr);
        // device form: without clipping the reduce launch still runs (over zero partials) to advance the step counter
        if (clip || step_dev)
            hipLaunchKernelGGL(adamw_sumsq_reduce_kernel, dim3(1), dim3(OPT_TPB), 0, st, sumsq, clip ? n_work : 0, step_dev);
    }
    const auto update = kind == MLAGG_OPT_SGD_NESTEROV    ? launch_update<MLAGG_OPT_SGD_NESTEROV>
                        : kind == MLAGG_OPT_ADAMW_AMSGRAD ? launch_update<MLAGG_OPT_ADAMW_AMSGRAD>
                        : kind == MLAGG_OPT_ADAM_L2       ? launch_update<MLAGG_OPT_ADAM_L2>
                                                          : launch_update<MLAGG_OPT_ADAMW>;
    update(table, extra, work, n_work, sumsq, a, beta1, beta2, lr_dev, step_dev, ss, st);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int mlagg_adamw_chunk_elements(void) { return CHUNK; }

extern "C" int mlagg_optimizer_clip_step(int kind, const void *tensor_table, const void *extra_table, const void *work_list, int n_work,
                                         double *sumsq, float lr, double beta1, double beta2, float eps, float weight_decay,
                                         float max_norm, int step, void *stream)
{
    const AdamArgs a{lr, (float)beta1, (float)beta2, eps, weight_decay, max_norm, 1.f, 1.f};
    return step_launch(kind, tensor_table, extra_table, work_list, n_work, sumsq, a, beta1, beta2, step, nullptr, nullptr, nullptr,
                              stream);
}

extern "C" int mlagg_optimizer_clip_step_dev(int kind, const void *tensor_table, const void *extra_table, const void *work_list,
                                             int n_work, double *sumsq, const float *lr_dev, int *step_dev, double beta1, double beta2,
                                             float eps, float weight_decay, float max_norm, void *stream)
{
    if (!lr_dev || !step_dev) return MLAGG_E_NULLPTR;
    const AdamArgs a{0.f, (float)beta1, (float)beta2, eps, weight_decay, max_norm, 1.f, 1.f};
    return step_launch(kind, tensor_table, extra_table, work_list, n_work, sumsq, a, beta1, beta2, 0, lr_dev, step_dev, nullptr,
                              stream);
}

extern "C" int mlagg_scaled_clip_step_dev(int kind, const void *tensor_table, const void *extra_table, const void *work_list, int n_work,
                                          double *sumsq, const float *lr_dev, int *step_dev, float *scale, int *growth_tracker,
                                          float *found_inf, float *grad_mult, double beta1, double beta2, float eps, float weight_decay,
                                          float max_norm, double growth_factor, double backoff_factor, int growth_interval,
                                          void *stream)
{
    if (!lr_dev || !step_dev || !scale || !growth_tracker || !found_inf || !grad_mult) return MLAGG_E_NULLPTR;
    const AdamArgs a{0.f, (float)beta1, (float)beta2, eps, weight_decay, max_norm, 1.f, 1.f};
    const ScaleState ss{scale, growth_tracker, found_inf, grad_mult, growth_factor, backoff_factor, growth_interval};
    return step_launch(kind, tensor_table, extra_table, work_list, n_work, sumsq, a, beta1, beta2, 0, lr_dev, step_dev, &ss, stream);
}
