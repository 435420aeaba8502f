// K28 -- ensembling and model selection on the device (the reference's ensembling/ensemble.py and the counting of
// evaluation/evaluate_predictions.py).
//
// Entry points and their kernels (one launch each; no LDS and no atomics in the first, integer atomics only in the second):
//   mlagg_ensemble_mean
//     ens_mean_kernel          average_probabilities (:17-29) and the argmax of merge_files in one pass: a lane owns 4 consecutive voxels
//                              and walks the K class planes; per plane acc = float(m_0), acc = acc + float(m_i) in member order, then
//                              acc / float(M) as an IEEE division, which is numpy's arithmetic to the bit (additions only: nothing can
//                              contract).  The running best mean and its class stay in registers: the first class whose mean is the
//                              maximum wins, a NaN counts as a maximum and the first NaN wins (numpy's argmax).  The member table
//                              (address, element size) lies in device memory, so M is unbounded and the sum never leaves its register.
//                              A plane of a member is read with one 16-byte (fp32) or 8-byte (fp16) load per lane where its first voxel
//                              is aligned to that and 4 voxels remain, with scalar loads otherwise; the test is made per member and per
//                              plane (N % 4 != 0 misaligns every other plane) and is the same in every lane.  Two planes are in flight
//                              per lane.  The mean is written only when its buffer is given.
//   mlagg_ensemble_mean_regions
//     ens_mean_kernel<true>    the same mean, in the same order, for the sigmoid heads of a region-based label manager; the label is
//                              painted from it as convert_probabilities_to_segmentation does (label_handling.py:166-173): 0, then
//                              order[k] wherever mean_k > 0.5 for k = 0 .. K-1, the last match winning (a NaN mean does not fire).  The
//                              K entries of regions_class_order follow the member table in device memory.
//   mlagg_label_confusion
//     label_confusion_kernel   the (L + 1) x (L + 1) matrix of (reference bin, prediction bin) voxel counts, from which tp / fp / fn / tn
//                              of every label and region follow on the host (compute_tp_fp_fn_tn :77-86 with ignore_mask = seg_ref ==
//                              ignore_label).  A lane reads 16 voxels of both volumes per step (one 16-byte load each where both bases
//                              are aligned), collapses runs of equal (reference, prediction) bytes -- also across its steps -- and adds
//                              each run to an int32 counter in LDS; the bins are looked up only where a run starts.  A workgroup sees
//                              fewer than 2^31 voxels and flushes its non-zero counters with 64-bit integer atomic adds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlagg_hip.h"
#include "prof.h"

namespace {

constexpr int ENS_BLOCK = 256;
constexpr int ENS_RUN = 4;                             // voxels per lane and step
constexpr int LC_BLOCK = 256;
constexpr int LC_RUN = 16;                             // voxels per lane and step
constexpr int LC_MAX_BINS = MLAGG_CONFUSION_MAX_LABELS + 1;
constexpr long long MAX_BLOCKS = 2048;                 // 256 CUs x 8 workgroups; the rest of the volume by grid stride

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// the 4 (n < 4: the first n) values of one member's plane that start at element offset o, as fp32
__device__ __forceinline__ f32x4 load_run(long long addr, int elem, long long o, int n)
{
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (elem == 4) {
        const float *p = reinterpret_cast<const float *>(addr) + o;
        if (n == ENS_RUN && !(reinterpret_cast<uintptr_t>(p) & 15)) return *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
        for (int j = 0; j < ENS_RUN; ++j)
            if (j < n) v[j] = p[j];
    } else {
        const _Float16 *p = reinterpret_cast<const _Float16 *>(addr) + o;
        if (n == ENS_RUN && !(reinterpret_cast<uintptr_t>(p) & 7)) {
            const f16x4 h = *reinterpret_cast<const f16x4 *>(p);
            return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
        }
#pragma unroll
        for (int j = 0; j < ENS_RUN; ++j)
            if (j < n) v[j] = (float)p[j];
    }
    return v;
}

struct Best {
    f32x4 value;
    int index[ENS_RUN];
};

// the sum of one plane -> its mean, stored if asked, and the running argmax (REGIONS: the label `paint` wherever the mean is above 0.5)
template <bool REGIONS>
__device__ __forceinline__ void finish_plane(f32x4 acc, float fm, int k, long long o, int n, float *__restrict__ mean, Best &best,
                                             int paint)
{
#pragma unroll
    for (int j = 0; j < ENS_RUN; ++j) acc[j] = acc[j] / fm;
    if (mean) {
        float *p = mean + o;
        if (n == ENS_RUN && !(reinterpret_cast<uintptr_t>(p) & 15)) *reinterpret_cast<f32x4 *>(p) = acc;
        else {
#pragma unroll
            for (int j = 0; j < ENS_RUN; ++j)
                if (j < n) p[j] = acc[j];
        }
    }
    if constexpr (REGIONS) {
#pragma unroll
        for (int j = 0; j < ENS_RUN; ++j) best.index[j] = acc[j] > 0.5f ? paint : best.index[j];
        return;
    }
    if (k == 0) {
        best.value = acc;
        return;
    }
#pragma unroll
    for (int j = 0; j < ENS_RUN; ++j) {
        const float b = best.value[j], v = acc[j];
        if (b == b && (v > b || v != v)) {             // a NaN best is final; the first larger value or NaN replaces the best
            best.value[j] = v;
            best.index[j] = k;
        }
    }
}

template <bool REGIONS>
__global__ void __launch_bounds__(ENS_BLOCK) ens_mean_kernel(const long long *__restrict__ table, int M, int K, long long N,
                                                             uint8_t *__restrict__ labels, float *__restrict__ mean)
{
    const float fm = (float)M;
    const long long *order = table + 2 * (long long)M;          // REGIONS: regions_class_order behind the member table
    const long long runs = (N + ENS_RUN - 1) / ENS_RUN;
    for (long long r = (long long)blockIdx.x * ENS_BLOCK + threadIdx.x; r < runs; r += (long long)gridDim.x * ENS_BLOCK) {
        const long long v0 = r * ENS_RUN;
        const int n = (int)(N - v0 < ENS_RUN ? N - v0 : ENS_RUN);
        Best best;
#pragma unroll
        for (int j = 0; j < ENS_RUN; ++j) best.index[j] = 0;
        int k = 0;
        for (; k + 1 < K; k += 2) {
            const long long o0 = (long long)k * N + v0, o1 = o0 + N;
            f32x4 a = load_run(table[0], (int)table[1], o0, n);
            f32x4 b = load_run(table[0], (int)table[1], o1, n);
            for (int m = 1; m < M; ++m) {
                const long long addr = table[2 * m];
                const int elem = (int)table[2 * m + 1];
                const f32x4 x = load_run(addr, elem, o0, n), y = load_run(addr, elem, o1, n);
                a = a + x;
                b = b + y;
            }
            finish_plane<REGIONS>(a, fm, k, o0, n, mean, best, REGIONS ? (int)order[k] : 0);
            finish_plane<REGIONS>(b, fm, k + 1, o1, n, mean, best, REGIONS ? (int)order[k + 1] : 0);
        }
        if (k < K) {
            const long long o0 = (long long)k * N + v0;
            f32x4 a = load_run(table[0], (int)table[1], o0, n);
            for (int m = 1; m < M; ++m) a = a + load_run(table[2 * m], (int)table[2 * m + 1], o0, n);
            finish_plane<REGIONS>(a, fm, k, o0, n, mean, best, REGIONS ? (int)order[k] : 0);
        }
        uint8_t *out = labels + v0;
        if (n == ENS_RUN && !(reinterpret_cast<uintptr_t>(out) & 3))
            *reinterpret_cast<uint32_t *>(out) = (uint32_t)best.index[0] | (uint32_t)best.index[1] << 8 | (uint32_t)best.index[2] << 16 |
                                                 (uint32_t)best.index[3] << 24;
        else {
#pragma unroll
            for (int j = 0; j < ENS_RUN; ++j)
                if (j < n) out[j] = (uint8_t)best.index[j];
        }
    }
}

struct Run {
    int raw;                                           // (reference << 8) | prediction of the open run, -1: none
    int key;                                           // its counter, -1: not counted (ignored)
    int n;
};

__device__ __forceinline__ void count_voxel(Run &run, int r, int p, const uint8_t *lut, int pitch, int ignore, int *cnt)
{
    const int raw = r << 8 | p;
    if (raw != run.raw) {
        if (run.n && run.key >= 0) atomicAdd(&cnt[run.key], run.n);
        run.raw = raw;
        run.key = r == ignore ? -1 : (int)lut[r] * pitch + (int)lut[p];
        run.n = 0;
    }
    ++run.n;
}

__global__ void __launch_bounds__(LC_BLOCK) label_confusion_kernel(const uint8_t *__restrict__ ref, const uint8_t *__restrict__ pred,
                                                                   long long N, const uint8_t *__restrict__ table, int L, int ignore,
                                                                   int vec, unsigned long long *__restrict__ counts)
{
    __shared__ int cnt[LC_MAX_BINS * LC_MAX_BINS];
    __shared__ uint8_t lut[256];
    const int t = threadIdx.x, pitch = L + 1, entries = pitch * pitch;
    for (int e = t; e < entries; e += LC_BLOCK) cnt[e] = 0;
    for (int e = t; e < 256; e += LC_BLOCK) lut[e] = (uint8_t)min((int)table[e], L);          // a bin beyond L counts as "any other"
    __syncthreads();
    const long long units = (N + LC_RUN - 1) / LC_RUN;
    Run run{-1, -1, 0};
    for (long long u = (long long)blockIdx.x * LC_BLOCK + t; u < units; u += (long long)gridDim.x * LC_BLOCK) {
        const long long v0 = u * LC_RUN;
        if (vec && v0 + LC_RUN <= N) {
            const uint4 a = *reinterpret_cast<const uint4 *>(ref + v0), b = *reinterpret_cast<const uint4 *>(pred + v0);
            const uint32_t ra[4] = {a.x, a.y, a.z, a.w}, pa[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    count_voxel(run, (int)(ra[w] >> (8 * j) & 255), (int)(pa[w] >> (8 * j) & 255), lut, pitch, ignore, cnt);
        } else {
            const int n = (int)(N - v0 < LC_RUN ? N - v0 : LC_RUN);
            for (int j = 0; j < n; ++j) count_voxel(run, ref[v0 + j], pred[v0 + j], lut, pitch, ignore, cnt);
        }
    }
    if (run.n && run.key >= 0) atomicAdd(&cnt[run.key], run.n);
    __syncthreads();
    for (int e = t; e < entries; e += LC_BLOCK)
        if (cnt[e]) atomicAdd(&counts[e], (unsigned long long)cnt[e]);
}

template <bool REGIONS>
int ensemble_any(const long long *table, int M, int K, long long N, unsigned char *labels, float *mean, void *stream)
{
    if (M < 1 || K < (REGIONS ? 1 : 2) || K > MLAGG_ENSEMBLE_MAX_CLASSES || N < 1) return MLAGG_E_UNSUPPORTED;
    if (N > LLONG_MAX / ((long long)K * 4)) return MLAGG_E_UNSUPPORTED;
    if (!table || !labels) return MLAGG_E_NULLPTR;
    if (reinterpret_cast<uintptr_t>(table) & 7 || reinterpret_cast<uintptr_t>(mean) & 3) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long runs = (N + ENS_RUN - 1) / ENS_RUN;
    const long long blocks = (runs + ENS_BLOCK - 1) / ENS_BLOCK;
    MLAGG_TIMED(K_ENS_MEAN, st);
    hipLaunchKernelGGL(ens_mean_kernel<REGIONS>, dim3((unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS)), dim3(ENS_BLOCK), 0, st, table,
                       M, K, N, labels, mean);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int mlagg_ensemble_mean(const long long *table, int M, int K, long long N, unsigned char *labels, float *mean, void *stream)
{
    return ensemble_any<false>(table, M, K, N, labels, mean, stream);
}

extern "C" int mlagg_ensemble_mean_regions(const long long *table, int M, int K, long long N, unsigned char *labels, float *mean,
                                           void *stream)
{
    return ensemble_any<true>(table, M, K, N, labels, mean, stream);
}

extern "C" int mlagg_label_confusion(const unsigned char *ref, const unsigned char *pred, long long N, const unsigned char *table, int L,
                                     int ignore, long long *counts, void *stream)
{
    if (N < 1 || L < 0 || L > MLAGG_CONFUSION_MAX_LABELS || ignore < -1 || ignore > 255) return MLAGG_E_UNSUPPORTED;
    if (!ref || !pred || !table || !counts) return MLAGG_E_NULLPTR;
    if (reinterpret_cast<uintptr_t>(counts) & 7) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t entries = (size_t)(L + 1) * (L + 1);
    if (hipError_t e = hipMemsetAsync(counts, 0, entries * sizeof(long long), st)) return (int)e;
    const long long units = (N + LC_RUN - 1) / LC_RUN;
    long long blocks = (units + LC_BLOCK - 1) / LC_BLOCK;
    if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
    // a workgroup's int32 counters: it takes ceil(units / (blocks * LC_BLOCK)) steps of LC_BLOCK * LC_RUN voxels; keep that at 2^30 voxels
    const long long cap = (long long)LC_BLOCK * ((1LL << 30) / (LC_BLOCK * LC_RUN));
    const long long need = (units + cap - 1) / cap;
    if (blocks < need) blocks = need;
    if (blocks > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    const int vec = !((reinterpret_cast<uintptr_t>(ref) | reinterpret_cast<uintptr_t>(pred)) & 15);
    MLAGG_TIMED(K_LABEL_CONFUSION, st);
    hipLaunchKernelGGL(label_confusion_kernel, dim3((unsigned)blocks), dim3(LC_BLOCK), 0, st, ref, pred, N, table, L, ignore, vec,
                       reinterpret_cast<unsigned long long *>(counts));
    return (int)hipGetLastError();
}
