// K9 -- statistics and gradient of the Dice + cross-entropy deep-supervision loss, one pass each over the logits.
//
// Replaces, per deep-supervision level, the eager chain of DC_and_CE_loss (reference loss/compound_losses.py:31-57):
// softmax, one-hot scatter, three masked products + spatial sums (MemoryEfficientSoftDiceLoss, loss/dice.py:73-117),
// log_softmax + nll (RobustCrossEntropyLoss, loss/robust_ce_loss.py:12-16) and the backward of all of them --
// 310 kernel launches and 2.5 ms per train step at config 2 (5 levels, 10 x 14 x 256^2 logits at level 0).
//
//   stats : per (sample b, class c)   I[b][c] = sum_p softmax(z)_c [y_p == c]      ("intersect")
//                                      P[b][c] = sum_p softmax(z)_c                 ("sum_pred")
//                                      G[b][c] = sum_p [y_p == c]                   ("sum_gt")
//           and the scalar            CE      = sum_{b,p} (logsumexp(z) - z_y)
//   grad  : dz_k = p_k (g_k - sum_c p_c g_c) + gCE (p_k - [y == k]),   g_c = gI[b][c] [y == c] + gP[b][c]
// The few-element algebra between them (dice ratio, means, level weights, the data-parallel all-reduce of the
// batch-dice statistics) stays in torch on (levels, classes)-sized tensors: trainer.deep_supervision_loss.
//
// K33 (further down) -- top-k cross-entropy, TopKLoss / DC_and_topk_loss (loss/robust_ce_loss.py:19-32, loss/compound_losses.py:103-151):
// the same two passes as template instances that also write / read the per-pixel cross-entropy, and between them an exact radix
// select of the k-th largest of the B HW values (topk_* kernels).
//
// Layout: logits (B, C, HW) fp32 NCHW planes, target (B, HW) float labels (as the nnU-Net pipeline delivers them).
// A thread owns PPT consecutive-by-256 pixels of one sample; every class plane is read as 1 KiB coalesced runs; the
// softmax is recomputed in the gradient pass (one more read of z instead of a write + read of the probabilities).
// HBM-bound: 4 (C + 1) bytes per pixel forward, 4 (2C + 1) backward.
#include <hip/hip_runtime.h>

#include "mlagg_hip.h"
#include "prof.h"
#include "reduce.h"

namespace {

constexpr int MAXC = 16;
constexpr int PPT = 4;            // pixels per thread
constexpr int TPB = 256;

struct LossGeom {
    int B, C;
    long HW;
    int ignore;                   // label value whose pixels take no part in the loss (DC_and_CE_loss(ignore_label=...)); -1: none
};

// Partial sums leave the workgroup as ONE row [I(C) | P(C) | G(C) | ce] of `part` and are added up in a fixed order by
// dice_ce_reduce_kernel: the first version accumulated them with float atomics (LDS, then global), which made the LOSS VALUE -- and
// through the dice gradient every gradient of the step -- differ in the last bits between two runs on identical inputs
// (tools/find_nondeterminism.py; profiles/round3_nondeterminism.log).
//
// The same pass serves K33 (top-k cross-entropy, below): CEPIX also writes every pixel's cross-entropy -- with label smoothing
// `eps` -- into ce_pix (B, HW), exactly 0 where the pixel is ignored; DICE = false (the pure top-k trainers) leaves the statistics
// out altogether.  K9 is the <false, true> instance: its arithmetic is the code below with nothing added.
template <bool CEPIX, bool DICE>
__global__ void __launch_bounds__(TPB)
dice_ce_stats_kernel(const float *__restrict__ logits, const float *__restrict__ target, float *__restrict__ part, LossGeom g,
                     float *__restrict__ ce_pix, float eps)
{
    __shared__ float red[TPB / 64][3 * MAXC + 1];
    const int b = blockIdx.y, C = g.C;
    const float *zb = logits + (size_t)b * C * g.HW;
    const float *tb = target + (size_t)b * g.HW;
    float aI[MAXC], aP[MAXC], aG[MAXC], ace = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) aI[c] = aP[c] = aG[c] = 0.f;

    const long p0 = (long)blockIdx.x * (TPB * PPT) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const long p = p0 + (long)j * TPB;
        if (p >= g.HW) break;
        float z[MAXC];
        float m = -3.0e38f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            z[c] = c < C ? zb[(size_t)c * g.HW + p] : -3.0e38f;
            m = fmaxf(m, z[c]);
        }
        const int y = (int)tb[p];
        float s = 0.f, zy = 0.f, zsum = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const float sh = z[c] - m;                     // shifted logit; zy keeps the one of the label
            zy = c == y ? sh : zy;
            if (CEPIX) zsum += c < C ? sh : 0.f;
            z[c] = c < C ? expf(sh) : 0.f;                 // z[] now holds exp(z - m)
            s += z[c];
        }
        const float inv = 1.f / s;
        const bool valid = y != g.ignore;                  // the loss mask of the reference (compound_losses.py:38-46)
        if (DICE) {
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const float pc = z[c] * inv;
                const bool hit = valid && c == y;
                aP[c] += valid ? pc : 0.f;
                aI[c] += hit ? pc : 0.f;
                aG[c] += hit ? 1.f : 0.f;
            }
            ace += valid ? logf(s) - zy : 0.f;             // -log softmax(z)_y (CrossEntropyLoss(ignore_index))
        }
        if (CEPIX) {
            // CrossEntropyLoss(reduction='none', label_smoothing=eps): (1 - eps)(lse - z_y) + (eps / C) sum_c (lse - z_c)
            const float lse = logf(s);
            const float nll = lse - zy, smooth = lse - zsum / (float)C;
            ce_pix[(size_t)b * g.HW + p] = valid ? (eps > 0.f ? (1.f - eps) * nll + eps * smooth : nll) : 0.f;
        }
    }
    if (!DICE) return;
    // block reduction: wave butterflies, one LDS row per wave, the four rows added in a fixed order, one partial row per workgroup
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        if (c < C) {
            const float vI = wave_sum(aI[c]), vP = wave_sum(aP[c]), vG = wave_sum(aG[c]);
            if ((threadIdx.x & 63) == 0) { red[wv][c] = vI; red[wv][MAXC + c] = vP; red[wv][2 * MAXC + c] = vG; }
        }
    }
    ace = wave_sum(ace);
    if ((threadIdx.x & 63) == 0) red[wv][3 * MAXC] = ace;
    __syncthreads();
    float *row = part + ((size_t)b * gridDim.x + blockIdx.x) * (3 * C + 1);
    if (threadIdx.x < 3 * C) {
        const int which = threadIdx.x / C, c = threadIdx.x - which * C, i = which * MAXC + c;
        row[threadIdx.x] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
    if (threadIdx.x == 3 * C) row[3 * C] = (red[0][3 * MAXC] + red[1][3 * MAXC]) + (red[2][3 * MAXC] + red[3][3 * MAXC]);
}

// stats_ip (B, 2, C), stats_g (B, C) = column sums of the nblk partial rows of every sample; ce_sum = sum of all ce partials.
// One workgroup, fixed assignment and order: deterministic.
__global__ void __launch_bounds__(256)
dice_ce_reduce_kernel(const float *__restrict__ part, int nblk, float *__restrict__ stats_ip, float *__restrict__ stats_g,
                      float *__restrict__ ce_sum, int B, int C)
{
    __shared__ float red[256];
    const int W = 3 * C + 1;
    for (int i = threadIdx.x; i < B * 3 * C; i += 256) {
        const int b = i / (3 * C), v = i - b * 3 * C;
        const float *p = part + (size_t)b * nblk * W + v;
        float s0 = 0.f, s1 = 0.f;
        int r = 0;
        for (; r + 1 < nblk; r += 2) { s0 += p[(size_t)r * W]; s1 += p[(size_t)(r + 1) * W]; }
        if (r < nblk) s0 += p[(size_t)r * W];
        const float s = s0 + s1;
        const int which = v / C, c = v - which * C;
        if (which < 2) stats_ip[((size_t)b * 2 + which) * C + c] = s;
        else stats_g[(size_t)b * C + c] = s;
    }
    float a = 0.f;
    for (long i = threadIdx.x; i < (long)B * nblk; i += 256) a += part[(size_t)i * W + 3 * C];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *ce_sum = red[0];
}

// The order-preserving integer image of a float: a < b as floats <=> ce_key(a) < ce_key(b) as unsigned, -0 and +0 map to one key.
__device__ __forceinline__ unsigned ce_key(float v)
{
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ce_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// what the select (below) leaves on the device for the gradient pass and for the host code: eight 4-byte words
struct TopkRecord {
    float t;                      // the k-th largest per-pixel cross-entropy
    float share;                  // (k - n_gt) / n_eq: the weight of every pixel that ties with t
    float topk_sum;               // sum of the k largest = sum_{ce > t} ce + (k - n_gt) t
    float topk_mean;              // topk_sum / k, TopKLoss.forward's result (robust_ce_loss.py:31-32)
    long long n_gt, n_eq;         // #{ce > t}, #{ce == t}
};

// TOPK = false: K9.  TOPK = true (K33): the cross-entropy term is the gradient of the mean of the k largest per-pixel values --
// g_ce[0] w_p / k ((1 - eps)(p_k - [y == k]) + eps (p_k - 1 / C)), w_p = 1 above the threshold, `share` on it, 0 below -- and
// DICE = false leaves the Dice term out (g_ip is not read).
template <bool TOPK, bool DICE>
__global__ void __launch_bounds__(TPB)
dice_ce_grad_kernel(const float *__restrict__ logits, const float *__restrict__ target, const float *__restrict__ g_ip,
                    const float *__restrict__ g_ce, float *__restrict__ dlogits, LossGeom g, const float *__restrict__ ce_pix,
                    const TopkRecord *__restrict__ rec, float eps, float inv_k)
{
    const int b = blockIdx.y, C = g.C;
    const float *zb = logits + (size_t)b * C * g.HW;
    const float *tb = target + (size_t)b * g.HW;
    float *db = dlogits + (size_t)b * C * g.HW;
    float gI[MAXC], gP[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        gI[c] = DICE && c < C ? g_ip[((size_t)b * 2 + 0) * C + c] : 0.f;
        gP[c] = DICE && c < C ? g_ip[((size_t)b * 2 + 1) * C + c] : 0.f;
    }
    const float gce = g_ce[0];
    unsigned tkey = 0u;
    float share = 0.f;
    if (TOPK) {
        tkey = ce_key(rec->t);
        share = rec->share;
    }
    const long p0 = (long)blockIdx.x * (TPB * PPT) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const long p = p0 + (long)j * TPB;
        if (p >= g.HW) break;
        float z[MAXC];
        float m = -3.0e38f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            z[c] = c < C ? zb[(size_t)c * g.HW + p] : -3.0e38f;
            m = fmaxf(m, z[c]);
        }
        const int y = (int)tb[p];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            z[c] = c < C ? expf(z[c] - m) : 0.f;
            s += z[c];
        }
        const float inv = 1.f / s;
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            z[c] *= inv;                                               // p_c
            dot += z[c] * (gP[c] + (c == y ? gI[c] : 0.f));
        }
        const bool valid = y != g.ignore;
        if (!TOPK) {
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                if (c < C) {
                    const float hit = c == y ? 1.f : 0.f;
                    const float dz = z[c] * (gP[c] + hit * gI[c] - dot) + gce * (z[c] - hit);
                    db[(size_t)c * g.HW + p] = valid ? dz : 0.f;
                }
            }
        } else {
            const unsigned key = ce_key(ce_pix[(size_t)b * g.HW + p]);
            const float w = gce * ((key > tkey ? 1.f : key == tkey ? share : 0.f) * inv_k);
            const float unif = eps / (float)C;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                if (c < C) {
                    const float hit = c == y ? 1.f : 0.f;
                    float dz = w * ((1.f - eps) * (z[c] - hit) + eps * z[c] - unif);
                    if (DICE) dz += z[c] * (gP[c] + hit * gI[c] - dot);
                    db[(size_t)c * g.HW + p] = valid ? dz : 0.f;
                }
            }
        }
    }
}

// ---- K33: exact selection of the k largest of the N = B HW per-pixel cross-entropies ------------------------------------------
// A radix select on ce_key: three passes over ce_pix, most significant digit first (11, 11 and 10 bits).  A pass counts, per value of
// its digit, the keys that agree with the digits chosen so far -- integer atomics into an LDS histogram, then one integer atomic per
// non-empty bin into the pass's global histogram: integer sums do not depend on the order of arrival.  A single workgroup then picks
// the bin that holds the k-th largest key.  After the last pick the key of the threshold t is complete, and so are the integer counts
// n_gt = #{ce > t} and n_eq = #{ce == t}.  One more pass sums the values above t: a double per workgroup, the partials added in a
// fixed order by one workgroup that also writes the TopkRecord.  Launches follow each other on the stream; no workgroup waits on
// another one, nothing is read back.
constexpr int SEL_TPB = 256;
constexpr int SEL_EPT = 16;                          // elements per thread
constexpr int SEL_EPW = SEL_TPB * SEL_EPT;           // elements per workgroup
constexpr int SEL_PASSES = 3;
constexpr int SEL_BINS = 2048;                       // bins of the widest digit
__host__ __device__ constexpr int sel_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__host__ __device__ constexpr int sel_bits(int pass) { return pass == 2 ? 10 : 11; }

struct SelState {                                    // device state between the passes
    unsigned long long k_rem;                        // rank of the threshold among the keys that agree with `prefix`
    unsigned long long n_gt;                         // keys known to lie above the threshold
    unsigned long long n_eq;                         // after the last pick: keys equal to the threshold
    unsigned prefix;                                 // digits of the threshold's key chosen so far
    unsigned pad;
};
// workspace, in 8-byte words: SelState | SEL_PASSES x SEL_BINS histogram counters | one double per workgroup of the sum pass
constexpr size_t SEL_STATE_WORDS = sizeof(SelState) / 8;
constexpr size_t SEL_HIST_WORDS = (size_t)SEL_PASSES * SEL_BINS;

__global__ void __launch_bounds__(SEL_TPB) topk_init_kernel(unsigned long long *__restrict__ ws, unsigned long long k)
{
    for (int i = threadIdx.x; i < (int)SEL_HIST_WORDS; i += SEL_TPB) ws[SEL_STATE_WORDS + i] = 0ull;
    if (threadIdx.x == 0) {
        SelState *s = reinterpret_cast<SelState *>(ws);
        s->k_rem = k;
        s->n_gt = 0ull;
        s->n_eq = 0ull;
        s->prefix = 0u;
        s->pad = 0u;
    }
}

template <int PASS>
__global__ void __launch_bounds__(SEL_TPB)
topk_hist_kernel(const float *__restrict__ ce_pix, long n, const SelState *__restrict__ state, unsigned long long *__restrict__ hist)
{
    constexpr int SHIFT = sel_shift(PASS), BINS = 1 << sel_bits(PASS);
    __shared__ unsigned h[BINS];
    for (int i = threadIdx.x; i < BINS; i += SEL_TPB) h[i] = 0u;
    __syncthreads();
    const unsigned prefix = PASS == 0 ? 0u : state->prefix;
    const long base = (long)blockIdx.x * SEL_EPW + threadIdx.x;
#pragma unroll
    for (int j = 0; j < SEL_EPT; ++j) {
        const long i = base + (long)j * SEL_TPB;
        if (i < n) {
            const unsigned key = ce_key(ce_pix[i]);
            // the digits above this pass's (64-bit shift: PASS 0 has none)
            const bool agrees = PASS == 0 || (((unsigned long long)(key ^ prefix)) >> (SHIFT + sel_bits(PASS))) == 0ull;
            if (agrees) atomicAdd(&h[(key >> SHIFT) & (BINS - 1)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BINS; i += SEL_TPB)
        if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// One workgroup: the bin d with  #{bins above d} < k_rem <= #{bins above d} + hist[d].  Thread t owns the PER consecutive bins from
// t * PER; an inclusive suffix scan over the threads' totals gives every thread the count above its bins.
template <int PASS>
__global__ void __launch_bounds__(SEL_TPB) topk_pick_kernel(SelState *__restrict__ state, const unsigned long long *__restrict__ hist)
{
    constexpr int BINS = 1 << sel_bits(PASS), PER = BINS / SEL_TPB;
    __shared__ unsigned long long suf[SEL_TPB];
    unsigned long long mine[PER], tot = 0ull;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        mine[j] = hist[threadIdx.x * PER + j];
        tot += mine[j];
    }
    suf[threadIdx.x] = tot;
    __syncthreads();
    for (int off = 1; off < SEL_TPB; off <<= 1) {
        const unsigned long long add = threadIdx.x + off < SEL_TPB ? suf[threadIdx.x + off] : 0ull;
        __syncthreads();
        suf[threadIdx.x] += add;
        __syncthreads();
    }
    const unsigned long long k_rem = state->k_rem;
    unsigned long long above = suf[threadIdx.x] - tot;                 // keys in the bins of the threads after this one
    __syncthreads();                                                   // every thread has read k_rem before one of them writes it
#pragma unroll
    for (int j = PER - 1; j >= 0; --j) {
        if (above < k_rem && k_rem <= above + mine[j]) {               // true for exactly one bin: 1 <= k_rem <= the total
            state->prefix |= (unsigned)(threadIdx.x * PER + j) << sel_shift(PASS);
            state->k_rem = k_rem - above;
            state->n_gt += above;
            state->n_eq = mine[j];
        }
        above += mine[j];
    }
}

__global__ void __launch_bounds__(SEL_TPB)
topk_sum_kernel(const float *__restrict__ ce_pix, long n, const SelState *__restrict__ state, double *__restrict__ part)
{
    __shared__ double red[SEL_TPB];
    const unsigned tkey = state->prefix;
    const long base = (long)blockIdx.x * SEL_EPW + threadIdx.x;
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < SEL_EPT; ++j) {
        const long i = base + (long)j * SEL_TPB;
        if (i < n) {
            const float v = ce_pix[i];
            a += ce_key(v) > tkey ? (double)v : 0.0;
        }
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int off = SEL_TPB / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(SEL_TPB)
topk_finish_kernel(const SelState *__restrict__ state, const double *__restrict__ part, long nblk, unsigned long long k,
                   TopkRecord *__restrict__ rec)
{
    __shared__ double red[SEL_TPB];
    double a = 0.0;
    for (long i = threadIdx.x; i < nblk; i += SEL_TPB) a += part[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int off = SEL_TPB / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float t = ce_unkey(state->prefix);
        const double rest = (double)(k - state->n_gt);                 // the part of the k that the ties at t fill: 1 <= rest <= n_eq
        const double total = red[0] + rest * (double)t;
        rec->t = t;
        rec->share = (float)(rest / (double)state->n_eq);
        rec->topk_sum = (float)total;
        rec->topk_mean = (float)(total / (double)k);
        rec->n_gt = (long long)state->n_gt;
        rec->n_eq = (long long)state->n_eq;
    }
}

template <int PASS>
void select_pass(const float *ce_pix, long n, unsigned long long *ws, hipStream_t st)
{
    SelState *state = reinterpret_cast<SelState *>(ws);
    unsigned long long *hist = ws + SEL_STATE_WORDS + (size_t)PASS * SEL_BINS;
    hipLaunchKernelGGL(topk_hist_kernel<PASS>, dim3((unsigned)((n + SEL_EPW - 1) / SEL_EPW)), dim3(SEL_TPB), 0, st, ce_pix, n, state,
                       hist);
    hipLaunchKernelGGL(topk_pick_kernel<PASS>, dim3(1), dim3(SEL_TPB), 0, st, state, hist);
}

int check(int B, int C, long HW)
{
    if (B <= 0 || B > 65535 || C < 2 || C > MAXC || HW <= 0) return MLAGG_E_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int mlagg_dice_ce_max_classes(void) { return MAXC; }

extern "C" size_t mlagg_dice_ce_stats_workspace_floats(int B, int C, long HW)
{
    if (B <= 0 || C <= 0 || HW <= 0) return 0;
    return (size_t)B * ((HW + TPB * PPT - 1) / (TPB * PPT)) * (3 * C + 1);
}

extern "C" int mlagg_dice_ce_stats(const float *logits, const float *target, float *stats_ip, float *stats_g, float *ce_sum,
                                   float *workspace, int B, int C, long HW, int ignore_label, void *stream)
{
    if (!logits || !target || !stats_ip || !stats_g || !ce_sum || !workspace) return MLAGG_E_NULLPTR;
    if (int rc = check(B, C, HW)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LossGeom g{B, C, HW, ignore_label};
    const unsigned nblk = (unsigned)((HW + TPB * PPT - 1) / (TPB * PPT));
    MLAGG_TIMED(K_LOSS_STATS, st);
    hipLaunchKernelGGL((dice_ce_stats_kernel<false, true>), dim3(nblk, B), dim3(TPB), 0, st, logits, target, workspace, g,
                       (float *)nullptr, 0.f);
    hipLaunchKernelGGL(dice_ce_reduce_kernel, dim3(1), dim3(256), 0, st, workspace, (int)nblk, stats_ip, stats_g, ce_sum, B, C);
    return (int)hipGetLastError();
}

extern "C" int mlagg_dice_ce_grad(const float *logits, const float *target, const float *g_ip, const float *g_ce,
                                  float *dlogits, int B, int C, long HW, int ignore_label, void *stream)
{
    if (!logits || !target || !g_ip || !g_ce || !dlogits) return MLAGG_E_NULLPTR;
    if (int rc = check(B, C, HW)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LossGeom g{B, C, HW, ignore_label};
    MLAGG_TIMED(K_LOSS_GRAD, st);
    hipLaunchKernelGGL((dice_ce_grad_kernel<false, true>), dim3((unsigned)((HW + TPB * PPT - 1) / (TPB * PPT)), B), dim3(TPB), 0, st,
                       logits, target, g_ip, g_ce, dlogits, g, (const float *)nullptr, (const TopkRecord *)nullptr, 0.f, 0.f);
    return (int)hipGetLastError();
}

// ---- K33 entry points -----------------------------------------------------------------------------------------------------------
extern "C" int mlagg_topk_ce_record_floats(void) { return (int)(sizeof(TopkRecord) / sizeof(float)); }

extern "C" int mlagg_topk_ce_select_elements_per_workgroup(void) { return SEL_EPW; }

extern "C" size_t mlagg_topk_ce_select_workspace_bytes(long n)
{
    if (n <= 0) return 0;
    return 8 * (SEL_STATE_WORDS + SEL_HIST_WORDS + (size_t)((n + SEL_EPW - 1) / SEL_EPW));
}

extern "C" int mlagg_topk_ce_stats(const float *logits, const float *target, float *stats_ip, float *stats_g, float *ce_sum,
                                   float *ce_pix, float *workspace, int B, int C, long HW, int ignore_label, float label_smoothing,
                                   void *stream)
{
    if (!logits || !target || !ce_pix) return MLAGG_E_NULLPTR;
    const bool dice = stats_ip || stats_g || ce_sum || workspace;
    if (dice && !(stats_ip && stats_g && ce_sum && workspace)) return MLAGG_E_NULLPTR;       // all four or none of them
    if (int rc = check(B, C, HW)) return rc;
    if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LossGeom g{B, C, HW, ignore_label};
    const unsigned nblk = (unsigned)((HW + TPB * PPT - 1) / (TPB * PPT));
    MLAGG_TIMED(K_TOPK_STATS, st);
    if (dice) {
        hipLaunchKernelGGL((dice_ce_stats_kernel<true, true>), dim3(nblk, B), dim3(TPB), 0, st, logits, target, workspace, g, ce_pix,
                           label_smoothing);
        hipLaunchKernelGGL(dice_ce_reduce_kernel, dim3(1), dim3(256), 0, st, workspace, (int)nblk, stats_ip, stats_g, ce_sum, B, C);
    } else {
        hipLaunchKernelGGL((dice_ce_stats_kernel<true, false>), dim3(nblk, B), dim3(TPB), 0, st, logits, target, (float *)nullptr, g,
                           ce_pix, label_smoothing);
    }
    return (int)hipGetLastError();
}

extern "C" int mlagg_topk_ce_select(const float *ce_pix, float *record, void *workspace, long n, long k, void *stream)
{
    if (!ce_pix || !record || !workspace) return MLAGG_E_NULLPTR;
    if (n <= 0 || k <= 0 || k > n) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long *ws = static_cast<unsigned long long *>(workspace);
    const long nblk = (n + SEL_EPW - 1) / SEL_EPW;
    if (nblk > 0x7fffffffL) return MLAGG_E_UNSUPPORTED;
    SelState *state = reinterpret_cast<SelState *>(ws);
    double *part = reinterpret_cast<double *>(ws + SEL_STATE_WORDS + SEL_HIST_WORDS);
    MLAGG_TIMED(K_TOPK_SELECT, st);
    hipLaunchKernelGGL(topk_init_kernel, dim3(1), dim3(SEL_TPB), 0, st, ws, (unsigned long long)k);
    select_pass<0>(ce_pix, n, ws, st);
    select_pass<1>(ce_pix, n, ws, st);
    select_pass<2>(ce_pix, n, ws, st);
    hipLaunchKernelGGL(topk_sum_kernel, dim3((unsigned)nblk), dim3(SEL_TPB), 0, st, ce_pix, n, state, part);
    hipLaunchKernelGGL(topk_finish_kernel, dim3(1), dim3(SEL_TPB), 0, st, state, part, nblk, (unsigned long long)k,
                       reinterpret_cast<TopkRecord *>(record));
    return (int)hipGetLastError();
}

extern "C" int mlagg_topk_ce_grad(const float *logits, const float *target, const float *ce_pix, const float *record,
                                  const float *g_ip, const float *g_topk, float *dlogits, int B, int C, long HW, long k,
                                  int ignore_label, float label_smoothing, void *stream)
{
    if (!logits || !target || !ce_pix || !record || !g_topk || !dlogits) return MLAGG_E_NULLPTR;
    if (int rc = check(B, C, HW)) return rc;
    if (k <= 0 || k > (long)B * HW || !(label_smoothing >= 0.f && label_smoothing <= 1.f)) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LossGeom g{B, C, HW, ignore_label};
    const dim3 grid((unsigned)((HW + TPB * PPT - 1) / (TPB * PPT)), B);
    const TopkRecord *rec = reinterpret_cast<const TopkRecord *>(record);
    const float inv_k = (float)(1.0 / (double)k);
    MLAGG_TIMED(K_TOPK_GRAD, st);
    if (g_ip)
        hipLaunchKernelGGL((dice_ce_grad_kernel<true, true>), grid, dim3(TPB), 0, st, logits, target, g_ip, g_topk, dlogits, g, ce_pix,
                           rec, label_smoothing, inv_k);
    else
        hipLaunchKernelGGL((dice_ce_grad_kernel<true, false>), grid, dim3(TPB), 0, st, logits, target, (const float *)nullptr, g_topk,
                           dlogits, g, ce_pix, rec, label_smoothing, inv_k);
    return (int)hipGetLastError();
}
