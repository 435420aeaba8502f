// K26 -- the segmentation side of preprocessing a TRAINING case, and the ordered selection of voxels by rank that the class
// locations and the dataset fingerprint need, for one (1, X, Y, Z) int16 label volume on the device.
//
// What it replaces, of the reference's DefaultPreprocessor.run_case with a seg_file
// (nnunetv2/preprocessing/preprocessors/default_preprocessor.py:38-124) and of the fingerprint extractor
// (nnunetv2/experiment_planning/dataset_fingerprint/fingerprint_extractor.py:39-103):
//   crop_to_nonzero's segmentation half (preprocessing/cropping/cropping.py:24-49): crop to the image's non-zero box, background
//   where the filled non-zero mask is off becomes -1;
//   resample_data_or_seg_to_shape(is_seg=True, order=1, order_z=0) (preprocessing/resampling/default_resampling.py:122-212 with
//   batchgenerators' resize_segmentation): per label, the indicator volume zoomed linearly and thresholded at 0.5, labels written
//   in ascending order;
//   np.argwhere(mask)[ranks] of _sample_foreground_locations (:134-161) and images[i][seg > 0][ranks] of
//   collect_foreground_intensities.
//
//   pt_seg_crop_kernel     crop + the -1 rule, any strides in, contiguous int16 out, label histogram in the same pass;
//   pt_seg_resize_kernel   every output voxel reads its 2 x 2 x 2 source voxels through the per-axis two-tap tables
//                          (export._axis_taps: 'linear', or 'nearest' for the low-resolution axis of a separate-z case, whose
//                          second weight is 0), sums in fp64 the weights of each distinct label among them and writes the largest
//                          label whose sum is >= 0.5, else 0: no indicator volume exists.  The products and sums run in scipy's
//                          order ((wx * wy) * wz, last axis fastest, contraction off).  Histogram of the output in the same pass;
//   pt_rank_count_kernel   per row of MLAGG_PP_RANK_BLOCK consecutive voxels and per group, the number of voxels whose label is
//                          in the group (wave ballot + popcount, one table row per workgroup, no atomics);
//   pt_rank_scan_kernel    exclusive scan of the table along the rows, one workgroup per group, and the totals;
//   pt_rank_select_kernel  one wave per requested rank: binary search of the row, ballot scan inside it to the voxel; writes the
//                          (0, x, y, z) coordinate and / or the fp32 value of every channel of a strided image at that voxel.
//
// Groups are label sets: groups[label + 1] (label -1 .. max_label) holds bit g when the label belongs to group g, at most
// MLAGG_PP_MAX_GROUPS of them.  Labels outside -1 .. max_label belong to no group and land in the histogram's last bin, which the
// caller checks.  Every count is an integer and every table row has one writer: two runs are bit-identical.  All volume offsets
// are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlagg_hip.h"
#include "prof.h"

namespace {

constexpr int PT_BLOCK = 256;
constexpr int PT_WAVE = 64;
constexpr int PT_WAVES = PT_BLOCK / PT_WAVE;
constexpr int PT_ROW = MLAGG_PP_RANK_BLOCK;          // voxels per table row
constexpr int PT_HIST_LDS = 4096;                    // histograms of up to this many bins are gathered in LDS first
constexpr unsigned PT_MAX_GRID = 4096;

static_assert(PT_ROW % PT_BLOCK == 0, "a table row is a whole number of workgroup sweeps");
static_assert(MLAGG_PP_MAX_GROUPS <= PT_WAVE, "lane g of a wave keeps group g's count");

typedef unsigned long long u64;

// bins 0 .. max_label + 1 hold the labels -1 .. max_label; bin max_label + 2 everything else
__device__ __forceinline__ int hist_bin(int label, int max_label)
{
    return (label >= -1 && label <= max_label) ? label + 1 : max_label + 2;
}

// A thread's run of equal bins is added once: most neighbours in a label volume are equal.
struct HistRun {
    int bin = -1;
    unsigned n = 0;
    __device__ __forceinline__ void flush(unsigned *lds, u64 *hist)
    {
        if (n == 0) return;
        if (lds) atomicAdd(lds + bin, n);
        else atomicAdd(hist + bin, (u64)n);
        n = 0;
    }
    __device__ __forceinline__ void add(int b, unsigned *lds, u64 *hist)
    {
        if (b != bin) {
            flush(lds, hist);
            bin = b;
        }
        ++n;
    }
};

__device__ __forceinline__ unsigned *hist_begin(unsigned *lds, int bins, const u64 *hist)
{
    if (!hist || bins > PT_HIST_LDS) return nullptr;
    for (int i = threadIdx.x; i < bins; i += PT_BLOCK) lds[i] = 0;
    __syncthreads();
    return lds;
}

__device__ __forceinline__ void hist_end(unsigned *lds, int bins, u64 *hist)
{
    if (!lds) return;
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += PT_BLOCK)
        if (lds[i]) atomicAdd(hist + i, (u64)lds[i]);
}

struct Win {
    int lo[3];
    int ext[3];
};

// ---------------------------------------------------------------------------------------------------------------------------
// crop + the -1 rule
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PT_BLOCK) pt_seg_crop_kernel(const short *__restrict__ seg, long long sx, long long sy, long long sz,
                                                               Win w, const uint8_t *__restrict__ mask, short *__restrict__ out,
                                                               long long V, int max_label, u64 *__restrict__ hist)
{
    __shared__ unsigned lds_hist[PT_HIST_LDS];
    const int bins = max_label + 3;
    unsigned *lds = hist_begin(lds_hist, bins, hist);
    HistRun run;
    const long long stride = (long long)gridDim.x * PT_BLOCK;
    for (long long f = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; f < V; f += stride) {
        long long r = f / w.ext[2];
        const int z = (int)(f - r * w.ext[2]);
        const int y = (int)(r % w.ext[1]);
        const int x = (int)(r / w.ext[1]);
        int v = seg[(long long)(w.lo[0] + x) * sx + (long long)(w.lo[1] + y) * sy + (long long)(w.lo[2] + z) * sz];
        if (v == 0 && !mask[f]) v = -1;
        out[f] = (short)v;
        if (hist) run.add(hist_bin(v, max_label), lds, hist);
    }
    if (hist) run.flush(lds, hist);
    hist_end(lds, bins, hist);
}

// ---------------------------------------------------------------------------------------------------------------------------
// resize_segmentation(order=1) without indicator volumes
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PT_BLOCK) pt_seg_resize_kernel(const short *__restrict__ in, int Y, int Z, const int *__restrict__ idx,
                                                                 const double *__restrict__ tw, short *__restrict__ out, int Xo, int Yo,
                                                                 int Zo, long long M, int max_label, u64 *__restrict__ hist)
{
#pragma clang fp contract(off)
    __shared__ unsigned lds_hist[PT_HIST_LDS];
    const int bins = max_label + 3;
    unsigned *lds = hist_begin(lds_hist, bins, hist);
    HistRun run;
    const long long stride = (long long)gridDim.x * PT_BLOCK;
    for (long long f = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; f < M; f += stride) {
        long long r = f / Zo;
        const int oz = (int)(f - r * Zo);
        const int oy = (int)(r % Yo);
        const int ox = (int)(r / Yo);
        const int rx = 2 * ox, ry = 2 * (Xo + oy), rz = 2 * (Xo + Yo + oz);
        short lab[8];
        double wt[8];
        bool same = true;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const long long row = ((long long)idx[rx + a] * Y + idx[ry + b]) * Z;
                const double wxy = tw[rx + a] * tw[ry + b];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int k = a * 4 + b * 2 + c;
                    lab[k] = in[row + idx[rz + c]];
                    wt[k] = wxy * tw[rz + c];
                    same = same && lab[k] == lab[0];
                }
            }
        }
        int best = 0;
        if (same) {
            best = lab[0];                               // its weights sum to 1 within rounding
        } else {
            bool found = false;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < 8; ++j) s += lab[j] == lab[i] ? wt[j] : 0.0;
                if (s >= 0.5 && (!found || lab[i] > best)) {
                    best = lab[i];
                    found = true;
                }
            }
        }
        out[f] = (short)best;
        if (hist) run.add(hist_bin(best, max_label), lds, hist);
    }
    if (hist) run.flush(lds, hist);
    hist_end(lds, bins, hist);
}

// ---------------------------------------------------------------------------------------------------------------------------
// ordered rank select
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 group_bits(const short *__restrict__ seg, long long v, long long N, const u64 *__restrict__ groups,
                                          int max_label)
{
    if (v >= N) return 0;
    const int l = seg[v];
    return (l >= -1 && l <= max_label) ? groups[l + 1] : 0;
}

// table[row * G + g] = number of voxels of row `row` (PT_ROW consecutive voxels) whose label is in group g
__global__ void __launch_bounds__(PT_BLOCK) pt_rank_count_kernel(const short *__restrict__ seg, long long N, const u64 *__restrict__ groups,
                                                                 int max_label, int G, long long *__restrict__ table)
{
    __shared__ int part[PT_WAVES][MLAGG_PP_MAX_GROUPS];
    const int lane = threadIdx.x % PT_WAVE, wave = threadIdx.x / PT_WAVE;
    const long long base = (long long)blockIdx.x * PT_ROW;
    int count = 0;                                       // lane g: group g
    for (int it = 0; it < PT_ROW / PT_BLOCK; ++it) {
        const u64 bits = group_bits(seg, base + it * PT_BLOCK + threadIdx.x, N, groups, max_label);
        for (int g = 0; g < G; ++g) {
            const u64 m = __ballot((bits >> g) & 1);
            if (lane == g) count += __popcll(m);
        }
    }
    if (lane < G) part[wave][lane] = count;
    __syncthreads();
    if ((int)threadIdx.x < G) {
        int s = 0;
        for (int w = 0; w < PT_WAVES; ++w) s += part[w][threadIdx.x];
        table[(long long)blockIdx.x * G + threadIdx.x] = s;
    }
}

// group blockIdx.x: table[., g] becomes its exclusive prefix sum along the rows, totals[g] the sum
__global__ void __launch_bounds__(PT_BLOCK) pt_rank_scan_kernel(long long *__restrict__ table, long long rows, int G,
                                                                long long *__restrict__ totals)
{
    __shared__ long long sums[PT_BLOCK];
    const int g = blockIdx.x;
    const long long per = (rows + PT_BLOCK - 1) / PT_BLOCK;
    const long long r0 = min((long long)threadIdx.x * per, rows), r1 = min(r0 + per, rows);
    long long s = 0;
    for (long long r = r0; r < r1; ++r) s += table[r * G + g];
    sums[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long acc = 0;
        for (int t = 0; t < PT_BLOCK; ++t) {
            const long long v = sums[t];
            sums[t] = acc;
            acc += v;
        }
        totals[g] = acc;
    }
    __syncthreads();
    long long acc = sums[threadIdx.x];
    for (long long r = r0; r < r1; ++r) {
        const long long v = table[r * G + g];
        table[r * G + g] = acc;
        acc += v;
    }
}

struct Img {
    const float *p;
    int C;
    long long sc, sx, sy, sz;
};

// one wave per rank: the voxel of C-order rank ranks[i] among those of group g.  coords[i] = (0, x, y, z), values[c * n + i] =
// img[c, x, y, z]; a rank outside [0, totals[g]) gives (-1, -1, -1, -1) and leaves the values alone.
__global__ void __launch_bounds__(PT_BLOCK) pt_rank_select_kernel(const short *__restrict__ seg, long long N, int Y, int Z,
                                                                  const u64 *__restrict__ groups, int max_label, int G, int g,
                                                                  const long long *__restrict__ table, long long rows,
                                                                  const long long *__restrict__ totals,
                                                                  const long long *__restrict__ ranks, long long n,
                                                                  long long *__restrict__ coords, Img img, float *__restrict__ values)
{
    const int lane = threadIdx.x % PT_WAVE;
    const long long i = (long long)blockIdx.x * PT_WAVES + threadIdx.x / PT_WAVE;
    if (i >= n) return;                                  // whole waves leave together
    const long long rank = ranks[i];
    if (rank < 0 || rank >= totals[g]) {
        if (coords && lane < 4) coords[i * 4 + lane] = -1;
        return;
    }
    long long lo = 0, hi = rows - 1;                     // the last row whose prefix is <= rank
    while (lo < hi) {
        const long long mid = (lo + hi + 1) / 2;
        if (table[mid * G + g] <= rank) lo = mid;
        else hi = mid - 1;
    }
    int rest = (int)(rank - table[lo * G + g]);
    const long long base = lo * PT_ROW;
    for (int it = 0; it < PT_ROW / PT_WAVE; ++it) {
        const long long v = base + it * PT_WAVE + lane;
        const bool in = (group_bits(seg, v, N, groups, max_label) >> g) & 1;
        const u64 m = __ballot(in);
        const int c = __popcll(m);
        if (rest < c) {
            if (in && __popcll(m & ((1ull << lane) - 1ull)) == rest) {
                const long long r = v / Z;
                const int z = (int)(v - r * Z);
                const int y = (int)(r % Y);
                const long long x = r / Y;
                if (coords) coords[i * 4 + 0] = 0, coords[i * 4 + 1] = x, coords[i * 4 + 2] = y, coords[i * 4 + 3] = z;
                if (values)
                    for (int ch = 0; ch < img.C; ++ch)
                        values[ch * n + i] = img.p[ch * img.sc + x * img.sx + y * img.sy + z * img.sz];
            }
            return;
        }
        rest -= c;
    }
}

unsigned capped_grid(long long n, long long per)
{
    const long long b = (n + per - 1) / per;
    return (unsigned)(b < 1 ? 1 : (b > PT_MAX_GRID ? PT_MAX_GRID : b));
}

}  // namespace

extern "C" size_t mlagg_pp_rank_rows(long long N) { return N < 1 ? 0 : (size_t)((N + PT_ROW - 1) / PT_ROW); }

extern "C" int mlagg_pp_seg_crop(const short *seg, int X, int Y, int Z, long long sx, long long sy, long long sz, const int *lo,
                                 const int *ext, const unsigned char *mask, short *out, int max_label, unsigned long long *hist,
                                 void *stream)
{
    if (!seg || !lo || !ext || !mask || !out) return MLAGG_E_NULLPTR;
    if (X < 1 || Y < 1 || Z < 1 || sx < 0 || sy < 0 || sz < 0 || max_label < 0 || max_label > 32767) return MLAGG_E_UNSUPPORTED;
    const int sh[3] = {X, Y, Z};
    Win w;
    for (int d = 0; d < 3; ++d) {
        if (lo[d] < 0 || ext[d] < 1 || lo[d] + ext[d] > sh[d]) return MLAGG_E_UNSUPPORTED;
        w.lo[d] = lo[d], w.ext[d] = ext[d];
    }
    const long long V = (long long)ext[0] * ext[1] * ext[2];
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_PT_SEG_CROP, st);
    if (hist) (void)hipMemsetAsync(hist, 0, sizeof(u64) * (max_label + 3), st);
    hipLaunchKernelGGL(pt_seg_crop_kernel, dim3(capped_grid(V, PT_BLOCK * 4LL)), dim3(PT_BLOCK), 0, st, seg, sx, sy, sz, w,
                       reinterpret_cast<const uint8_t *>(mask), out, V, max_label, hist);
    return (int)hipGetLastError();
}

extern "C" int mlagg_pp_seg_resize(const short *in, int X, int Y, int Z, const int *tap_idx, const double *tap_w, short *out, int Xo,
                                   int Yo, int Zo, int max_label, unsigned long long *hist, void *stream)
{
    if (!in || !tap_idx || !tap_w || !out) return MLAGG_E_NULLPTR;
    if (X < 1 || Y < 1 || Z < 1 || Xo < 1 || Yo < 1 || Zo < 1 || max_label < 0 || max_label > 32767) return MLAGG_E_UNSUPPORTED;
    if ((long long)Xo + Yo + Zo > 1073741823LL) return MLAGG_E_UNSUPPORTED;       // table rows are indexed with int
    const long long M = (long long)Xo * Yo * Zo;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_PT_SEG_RESIZE, st);
    if (hist) (void)hipMemsetAsync(hist, 0, sizeof(u64) * (max_label + 3), st);
    hipLaunchKernelGGL(pt_seg_resize_kernel, dim3(capped_grid(M, PT_BLOCK * 2LL)), dim3(PT_BLOCK), 0, st, in, Y, Z, tap_idx, tap_w, out,
                       Xo, Yo, Zo, M, max_label, hist);
    return (int)hipGetLastError();
}

extern "C" int mlagg_pp_rank_counts(const short *seg, long long N, const unsigned long long *groups, int max_label, int n_groups,
                                    long long *table, long long *totals, void *stream)
{
    if (!seg || !groups || !table || !totals) return MLAGG_E_NULLPTR;
    if (N < 1 || max_label < 0 || max_label > 32767 || n_groups < 1 || n_groups > MLAGG_PP_MAX_GROUPS) return MLAGG_E_UNSUPPORTED;
    const long long rows = (long long)mlagg_pp_rank_rows(N);
    if (rows > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_PT_RANK_COUNTS, st);
    hipLaunchKernelGGL(pt_rank_count_kernel, dim3((unsigned)rows), dim3(PT_BLOCK), 0, st, seg, N, groups, max_label, n_groups, table);
    hipLaunchKernelGGL(pt_rank_scan_kernel, dim3((unsigned)n_groups), dim3(PT_BLOCK), 0, st, table, rows, n_groups, totals);
    return (int)hipGetLastError();
}

extern "C" int mlagg_pp_rank_select(const short *seg, long long N, int Y, int Z, const unsigned long long *groups, int max_label,
                                    int n_groups, int group, const long long *table, const long long *totals, const long long *ranks,
                                    long long n_ranks, long long *coords, const float *image, int C, long long sc, long long sx,
                                    long long sy, long long sz, float *values, void *stream)
{
    if (!seg || !groups || !table || !totals || !ranks) return MLAGG_E_NULLPTR;
    if ((values != nullptr) != (image != nullptr) || (!coords && !values)) return MLAGG_E_NULLPTR;
    if (N < 1 || Y < 1 || Z < 1 || N % ((long long)Y * Z) != 0 || max_label < 0 || max_label > 32767 || n_groups < 1 ||
        n_groups > MLAGG_PP_MAX_GROUPS || group < 0 || group >= n_groups || n_ranks < 1)
        return MLAGG_E_UNSUPPORTED;
    if (image && (C < 1 || sc < 0 || sx < 0 || sy < 0 || sz < 0)) return MLAGG_E_UNSUPPORTED;
    const long long rows = (long long)mlagg_pp_rank_rows(N);
    const long long blocks = (n_ranks + PT_WAVES - 1) / PT_WAVES;
    if (rows > 2147483647LL || blocks > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_PT_RANK_SELECT, st);
    hipLaunchKernelGGL(pt_rank_select_kernel, dim3((unsigned)blocks), dim3(PT_BLOCK), 0, st, seg, N, Y, Z, groups, max_label, n_groups,
                       group, table, rows, totals, ranks, n_ranks, coords, Img{image, C, sc, sx, sy, sz}, values);
    return (int)hipGetLastError();
}
