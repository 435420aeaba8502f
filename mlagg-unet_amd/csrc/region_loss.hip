// K29 -- statistics and gradient of the Dice + binary cross-entropy deep-supervision loss of region-based datasets (sigmoid heads),
// one pass each over the logits: the counterpart of K9 (loss.hip) for label managers with `has_regions`.
//
// Replaces, per deep-supervision level, the eager chain of DC_and_BCE_loss (reference loss/compound_losses.py:60-100): sigmoid, three
// masked products + spatial sums (MemoryEfficientSoftDiceLoss with do_bg=True, loss/dice.py:73-117), BCEWithLogitsLoss and the
// backward of all of them.
//
//   stats : per (sample b, head r)    I[b][r] = sum_p m_p sigmoid(z_r) t_r          ("intersect")
//                                      P[b][r] = sum_p m_p sigmoid(z_r)              ("sum_pred")
//                                      G[b][r] = sum_p m_p t_r                       ("sum_gt")
//           and the scalars            BCE     = sum_{b,r,p} m_p (softplus(z_r) - z_r t_r)      M = sum_{b,p} m_p
//   grad  : dz_r = m_p [ s (1 - s) (gI[b][r] t_r + gP[b][r]) + gBCE (s - t_r) ],   s = sigmoid(z_r)
// The few-element algebra between them (dice ratio, means, level weights, the data-parallel all-reduce of the batch-dice statistics)
// stays in torch on (levels, heads)-sized tensors: trainer.region_deep_supervision_loss.
//
// The target comes in two forms (template flag PLANES):
//   label map      (B, HW) float labels + member[256]: bit r of member[v] says that label v belongs to region r (np.isin: a value
//                  outside the table or in no region has no bits); m_p = [label != ignore], 1 everywhere without an ignore label.
//                  No (B, R, ...) one-hot tensor exists.
//   region planes  (B, R, HW) or, with an ignore label, (B, R + 1, HW) float: what ConvertSegmentationToRegionsTransform delivers;
//                  the last plane is then the ignore indicator and m_p = (1 - t_last) != 0 (compound_losses.py:85-89).
//
// Layout and schedule as K9: logits (B, R, HW) fp32 planes; a thread owns PPT consecutive-by-256 pixels of one sample, every plane is
// read as 1 KiB coalesced runs, the sigmoid is recomputed in the gradient pass.  One exponential per logit: softplus1 returns
// e = exp(-|z|) and sigmoid(z) = (z >= 0 ? 1 : e) / (1 + e), so every quantity stays finite for any finite z (|z| = 100: e = 0,
// sigmoid is exactly 0 or 1, softplus is max(z, 0)).  HBM-bound.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "activations.h"
#include "mlagg_hip.h"
#include "prof.h"
#include "reduce.h"

namespace {

constexpr int MAXR = 16;
constexpr int PPT = 4;            // pixels per thread
constexpr int TPB = 256;

struct RegionGeom {
    int B, R;
    long HW;
    int ignore;                   // label map: the label whose pixels take no part in the loss; planes: >= 0 says that plane R is the ignore plane; -1: none
};

__device__ __forceinline__ float sigmoid_from_e(float z, float e) { return (z >= 0.f ? 1.f : e) / (1.f + e); }

// the targets t[0 .. RB) and the mask of pixel p of one sample
template <bool PLANES, int RB>
__device__ __forceinline__ float load_target(const float *__restrict__ tb, const uint32_t *member, long p, const RegionGeom &g,
                                             float (&t)[RB])
{
    if (PLANES) {
#pragma unroll
        for (int r = 0; r < RB; ++r) t[r] = r < g.R ? tb[(size_t)r * g.HW + p] : 0.f;
        return g.ignore >= 0 ? (1.f - tb[(size_t)g.R * g.HW + p] != 0.f ? 1.f : 0.f) : 1.f;
    }
    const int v = (int)tb[p];
    const uint32_t bits = (unsigned)v < 256u ? member[v] : 0u;
#pragma unroll
    for (int r = 0; r < RB; ++r) t[r] = (float)(bits >> r & 1u);
    return g.ignore >= 0 && v == g.ignore ? 0.f : 1.f;
}

// Partial sums leave the workgroup as ONE row [I(R) | P(R) | G(R) | bce | m] of `part` and are added up in a fixed order by
// dice_bce_reduce_kernel: no float atomics, so the loss value -- and through the dice gradient every gradient of the step -- is
// bit-reproducible from run to run (see loss.hip).
template <bool PLANES, int RB>
__global__ void __launch_bounds__(TPB)
dice_bce_stats_kernel(const float *__restrict__ logits, const float *__restrict__ target, const uint32_t *__restrict__ member_g,
                      float *__restrict__ part, RegionGeom g)
{
    __shared__ float red[TPB / 64][3 * MAXR + 2];
    __shared__ uint32_t member[256];
    if (!PLANES) {
        member[threadIdx.x] = member_g[threadIdx.x];      // TPB == 256 entries
        __syncthreads();
    }
    const int b = blockIdx.y, R = g.R;
    const float *zb = logits + (size_t)b * R * g.HW;
    const float *tb = target + (size_t)b * (PLANES ? (size_t)(R + (g.ignore >= 0 ? 1 : 0)) : 1) * g.HW;
    float aI[RB], aP[RB], aG[RB], abce = 0.f, am = 0.f;
#pragma unroll
    for (int r = 0; r < RB; ++r) aI[r] = aP[r] = aG[r] = 0.f;

    const long p0 = (long)blockIdx.x * (TPB * PPT) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const long p = p0 + (long)j * TPB;
        if (p >= g.HW) break;
        float t[RB];
        const float m = load_target<PLANES, RB>(tb, member, p, g, t);
        am += m;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            if (r < R) {
                const float z = zb[(size_t)r * g.HW + p];
                float e;
                const float sp = softplus1(z, e);
                const float s = sigmoid_from_e(z, e);
                aP[r] += m * s;
                aI[r] += m * s * t[r];
                aG[r] += m * t[r];
                abce += m * (sp - z * t[r]);               // BCEWithLogitsLoss: softplus(z) - z t
            }
        }
    }
    // block reduction: wave butterflies, one LDS row per wave, the four rows added in a fixed order, one partial row per workgroup
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        if (r < R) {
            const float vI = wave_sum(aI[r]), vP = wave_sum(aP[r]), vG = wave_sum(aG[r]);
            if ((threadIdx.x & 63) == 0) { red[wv][r] = vI; red[wv][MAXR + r] = vP; red[wv][2 * MAXR + r] = vG; }
        }
    }
    abce = wave_sum(abce);
    am = wave_sum(am);
    if ((threadIdx.x & 63) == 0) { red[wv][3 * MAXR] = abce; red[wv][3 * MAXR + 1] = am; }
    __syncthreads();
    float *row = part + ((size_t)b * gridDim.x + blockIdx.x) * (3 * R + 2);
    if (threadIdx.x < 3 * R) {
        const int which = threadIdx.x / R, r = threadIdx.x - which * R, i = which * MAXR + r;
        row[threadIdx.x] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    } else if (threadIdx.x < 3 * R + 2) {
        const int i = 3 * MAXR + (threadIdx.x - 3 * R);
        row[threadIdx.x] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

// stats_ip (B, 2, R), stats_g (B, R) = column sums of the nblk partial rows of every sample; sums[0] = the sum of all bce partials,
// sums[1] = the sum of all mask partials.  One workgroup, fixed assignment and order: deterministic.
__global__ void __launch_bounds__(256)
dice_bce_reduce_kernel(const float *__restrict__ part, int nblk, float *__restrict__ stats_ip, float *__restrict__ stats_g,
                       float *__restrict__ sums, int B, int R)
{
    __shared__ float red[2][256];
    const int W = 3 * R + 2;
    for (int i = threadIdx.x; i < B * 3 * R; i += 256) {
        const int b = i / (3 * R), v = i - b * 3 * R;
        const float *p = part + (size_t)b * nblk * W + v;
        float s0 = 0.f, s1 = 0.f;
        int k = 0;
        for (; k + 1 < nblk; k += 2) { s0 += p[(size_t)k * W]; s1 += p[(size_t)(k + 1) * W]; }
        if (k < nblk) s0 += p[(size_t)k * W];
        const float s = s0 + s1;
        const int which = v / R, r = v - which * R;
        if (which < 2) stats_ip[((size_t)b * 2 + which) * R + r] = s;
        else stats_g[(size_t)b * R + r] = s;
    }
    float a = 0.f, c = 0.f;
    for (long i = threadIdx.x; i < (long)B * nblk; i += 256) {
        a += part[(size_t)i * W + 3 * R];
        c += part[(size_t)i * W + 3 * R + 1];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = c;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            red[0][threadIdx.x] += red[0][threadIdx.x + off];
            red[1][threadIdx.x] += red[1][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) sums[threadIdx.x] = red[threadIdx.x][0];
}

template <bool PLANES, int RB>
__global__ void __launch_bounds__(TPB)
dice_bce_grad_kernel(const float *__restrict__ logits, const float *__restrict__ target, const uint32_t *__restrict__ member_g,
                     const float *__restrict__ g_ip, const float *__restrict__ g_bce, float *__restrict__ dlogits, RegionGeom g)
{
    __shared__ uint32_t member[256];
    if (!PLANES) {
        member[threadIdx.x] = member_g[threadIdx.x];
        __syncthreads();
    }
    const int b = blockIdx.y, R = g.R;
    const float *zb = logits + (size_t)b * R * g.HW;
    const float *tb = target + (size_t)b * (PLANES ? (size_t)(R + (g.ignore >= 0 ? 1 : 0)) : 1) * g.HW;
    float *db = dlogits + (size_t)b * R * g.HW;
    float gI[RB], gP[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        gI[r] = r < R ? g_ip[((size_t)b * 2 + 0) * R + r] : 0.f;
        gP[r] = r < R ? g_ip[((size_t)b * 2 + 1) * R + r] : 0.f;
    }
    const float gb = g_bce[0];
    const long p0 = (long)blockIdx.x * (TPB * PPT) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const long p = p0 + (long)j * TPB;
        if (p >= g.HW) break;
        float t[RB];
        const float m = load_target<PLANES, RB>(tb, member, p, g, t);
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            if (r < R) {
                const float z = zb[(size_t)r * g.HW + p];
                const float e = __expf(-fabsf(z));
                const float s = sigmoid_from_e(z, e);
                const float ds = e / ((1.f + e) * (1.f + e));          // s (1 - s) without the cancellation of 1 - s near s = 1
                db[(size_t)r * g.HW + p] = m * (ds * (gI[r] * t[r] + gP[r]) + gb * (s - t[r]));
            }
        }
    }
}

int check(int B, int R, long HW)
{
    if (B <= 0 || B > 65535 || R < 1 || R > MAXR || HW <= 0) return MLAGG_E_UNSUPPORTED;
    return 0;
}

unsigned blocks_of(long HW) { return (unsigned)((HW + TPB * PPT - 1) / (TPB * PPT)); }

template <bool PLANES, int RB>
void launch_stats(hipStream_t st, const float *logits, const float *target, const uint32_t *member, float *part, const RegionGeom &g)
{
    hipLaunchKernelGGL((dice_bce_stats_kernel<PLANES, RB>), dim3(blocks_of(g.HW), g.B), dim3(TPB), 0, st, logits, target, member, part, g);
}

template <bool PLANES, int RB>
void launch_grad(hipStream_t st, const float *logits, const float *target, const uint32_t *member, const float *g_ip,
                 const float *g_bce, float *dlogits, const RegionGeom &g)
{
    hipLaunchKernelGGL((dice_bce_grad_kernel<PLANES, RB>), dim3(blocks_of(g.HW), g.B), dim3(TPB), 0, st, logits, target, member, g_ip,
                       g_bce, dlogits, g);
}

}  // namespace

extern "C" int mlagg_dice_bce_max_regions(void) { return MAXR; }

extern "C" size_t mlagg_dice_bce_stats_workspace_floats(int B, int R, long HW)
{
    if (B <= 0 || R <= 0 || HW <= 0) return 0;
    return (size_t)B * blocks_of(HW) * (3 * R + 2);
}

extern "C" int mlagg_dice_bce_stats(const float *logits, const float *target, const unsigned int *member, float *stats_ip,
                                    float *stats_g, float *sums, float *workspace, int B, int R, long HW, int ignore_label,
                                    void *stream)
{
    if (!logits || !target || !stats_ip || !stats_g || !sums || !workspace) return MLAGG_E_NULLPTR;
    if (int rc = check(B, R, HW)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RegionGeom g{B, R, HW, ignore_label < 0 ? -1 : ignore_label};
    MLAGG_TIMED(K_REGION_LOSS_STATS, st);
    if (member) {
        if (R <= 4) launch_stats<false, 4>(st, logits, target, member, workspace, g);
        else if (R <= 8) launch_stats<false, 8>(st, logits, target, member, workspace, g);
        else launch_stats<false, 16>(st, logits, target, member, workspace, g);
    } else {
        if (R <= 4) launch_stats<true, 4>(st, logits, target, member, workspace, g);
        else if (R <= 8) launch_stats<true, 8>(st, logits, target, member, workspace, g);
        else launch_stats<true, 16>(st, logits, target, member, workspace, g);
    }
    hipLaunchKernelGGL(dice_bce_reduce_kernel, dim3(1), dim3(256), 0, st, workspace, (int)blocks_of(HW), stats_ip, stats_g, sums, B, R);
    return (int)hipGetLastError();
}

extern "C" int mlagg_dice_bce_grad(const float *logits, const float *target, const unsigned int *member, const float *g_ip,
                                   const float *g_bce, float *dlogits, int B, int R, long HW, int ignore_label, void *stream)
{
    if (!logits || !target || !g_ip || !g_bce || !dlogits) return MLAGG_E_NULLPTR;
    if (int rc = check(B, R, HW)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RegionGeom g{B, R, HW, ignore_label < 0 ? -1 : ignore_label};
    MLAGG_TIMED(K_REGION_LOSS_GRAD, st);
    if (member) {
        if (R <= 4) launch_grad<false, 4>(st, logits, target, member, g_ip, g_bce, dlogits, g);
        else if (R <= 8) launch_grad<false, 8>(st, logits, target, member, g_ip, g_bce, dlogits, g);
        else launch_grad<false, 16>(st, logits, target, member, g_ip, g_bce, dlogits, g);
    } else {
        if (R <= 4) launch_grad<true, 4>(st, logits, target, member, g_ip, g_bce, dlogits, g);
        else if (R <= 8) launch_grad<true, 8>(st, logits, target, member, g_ip, g_bce, dlogits, g);
        else launch_grad<true, 16>(st, logits, target, member, g_ip, g_bce, dlogits, g);
    }
    return (int)hipGetLastError();
}
