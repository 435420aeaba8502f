// K30 -- the cascade training transforms on bit planes (nnU-Net's 3d_cascade_fullres input path).
//
// What it replaces: MoveSegAsOneHotToData, ApplyRandomBinaryOperatorTransform and
// RemoveRandomConnectedComponentFromOneHotEncodingTransform (training/data_augmentation/custom_transforms/cascade_transforms.py:
// 10-136), which materialise the previous stage's segmentation as fp32 one-hot channels and run skimage's binary_dilation / erosion /
// closing / opening with a ball footprint, and a connected-component labelling, on every channel on the host.
//
// Here a one-hot channel is a bit plane: (X, Y, W) 64-bit words, W = ceil(Z / 64), bit k of word w of row (x, y) is voxel z = 64 w + k.
// The padding bits of a row's last word are 0 at rest and every kernel below masks them after it has written.
//   cascade_pack_kernel     one wave per word: lane k reads voxel 64 w + k of the label map, one ballot per listed label;
//   cascade_unpack_kernel   planes -> fp32 0 / 1 channels of the network input;
//   cascade_morph_kernel    out[p] = OR over the footprint's offsets d of in[p + d], 0 outside the volume: each lane computes one output
//                           word of an 8 x 8 x 4-word tile whose input words (8 rows and one word of halo) are staged in LDS; per
//                           footprint row (dx, dy) and per run of set offsets [lo, lo + len) along z the lane aligns the 128 bits
//                           starting at 64 w + lo with a funnel shift and spreads the run by log-step OR-shifts.  Erosion is the same
//                           kernel on the complemented input (padding and outside: 0 after the complement, i.e. "1 outside") with
//                           the complemented output; the caller hands over the offsets of the dilation (-(i - c)) or the erosion
//                           (i - c);
//   cascade_commit_kernel   the reference's "was added" rule: plane c of a sample takes the result, res & ~before is cleared in the
//                           sample's other planes;
//   cascade_cc_*            26-connected components of every plane with the labelling of cc_label.h over a voxel source that reads
//                           the bits (tile-local union-find, merge across tile faces, compress, sizes), then per plane the number
//                           of components with size < thresh and, for a chosen rank k, the k-th such component in root order (a
//                           root is its component's minimum linear index: scipy's / skimage's label order), which is cleared, and
//                           optionally set in another plane.
// Integer atomics only; every result is independent of the schedule.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "cc_label.h"
#include "mlagg_hip.h"

namespace {

using namespace mlagg_cc;
typedef unsigned long long u64;

struct Labels {
    int v[MLAGG_CASCADE_MAX_LABELS];
};

__device__ __forceinline__ u64 tail_mask(int Z, int W, int w)
{
    const int r = Z & 63;
    return (w == W - 1 && r) ? ((1ull << r) - 1ull) : ~0ull;
}

// ---------------------------------------------------------------------------------------------------------------------------
// pack / unpack
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) cascade_pack_kernel(const T *__restrict__ seg, long long sample_stride, int L, Labels lab,
                                                           long long rows_per_sample, int Z, int W, long long n_words,
                                                           u64 *__restrict__ planes)
{
    const int lane = threadIdx.x & 63;
    const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);         // (b, row, w), uniform in the wave
    if (word >= n_words) return;
    const int w = (int)(word % W);
    const long long brow = word / W, b = brow / rows_per_sample, row = brow % rows_per_sample;
    const int z = w * 64 + lane;
    int v = INT_MIN;                                                               // no label of the list
    if (z < Z) {
        const T s = seg[b * sample_stride + row * Z + z];
        v = (int)s;
        if ((T)v != s) v = INT_MIN;                                                // a fractional float is no label
    }
    u64 mine = 0;
    for (int i = 0; i < L; ++i) {
        const u64 m = __ballot(v == lab.v[i]);
        if (lane == i) mine = m;
    }
    if (lane < L) planes[((b * L + lane) * rows_per_sample + row) * W + w] = mine;
}

__global__ void __launch_bounds__(256) cascade_unpack_kernel(const u64 *__restrict__ planes, int L, long long rows_per_sample, int Z,
                                                             int W, int C_total, int c0, long long n_vox, float *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;                 // (b, l, row, z)
    if (i >= n_vox) return;
    const int z = (int)(i % Z);
    const long long prow = i / Z, row = prow % rows_per_sample, bl = prow / rows_per_sample;
    const long long b = bl / L, l = bl % L;
    const u64 word = planes[prow * W + (z >> 6)];
    out[((b * C_total + c0 + l) * rows_per_sample + row) * Z + z] = (float)((word >> (z & 63)) & 1ull);
}

// ---------------------------------------------------------------------------------------------------------------------------
// morphology
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int MT = 8, MW = 4, MH = MLAGG_CASCADE_MAX_REACH;       // tile rows per axis, tile words, halo rows
constexpr int MR = MT + 2 * MH, MWH = MW + 2;                     // staged rows per axis, staged words per row
constexpr int MJ = 32;                                           // jobs per launch

struct MorphJobs {
    int src[MJ], dst[MJ], first_run[MJ], n_runs[MJ], complement[MJ];
};

// bits [r, r + 64) of the 128-bit value (hi : lo), 0 <= r < 64
__device__ __forceinline__ u64 funnel(u64 lo, u64 hi, int r)
{
    return r ? (lo >> r) | (hi << (64 - r)) : lo;
}

__global__ void __launch_bounds__(MT * MT * MW) cascade_morph_kernel(u64 *__restrict__ pool, long long plane_words, int X, int Y,
                                                                     int Z, int W, int ntx, int nty, int ntw,
                                                                     const int4 *__restrict__ runs, MorphJobs jobs)
{
    __shared__ u64 tile[MR][MR][MWH];
    const int j = blockIdx.y;
    const u64 *src = pool + (long long)jobs.src[j] * plane_words;
    u64 *dst = pool + (long long)jobs.dst[j] * plane_words;
    const bool comp = jobs.complement[j] != 0;
    const int4 *run = runs + jobs.first_run[j];
    const int n_runs = jobs.n_runs[j];
    const int tw = blockIdx.x % ntw, r = blockIdx.x / ntw;
    const int x0 = (r / nty) * MT, y0 = (r % nty) * MT, w0 = tw * MW;
    for (int i = threadIdx.x; i < MR * MR * MWH; i += MT * MT * MW) {
        const int sw = i % MWH, sy = (i / MWH) % MR, sx = i / (MWH * MR);
        const int x = x0 + sx - MH, y = y0 + sy - MH, w = w0 + sw - 1;
        u64 v = 0;
        if (x >= 0 && x < X && y >= 0 && y < Y && w >= 0 && w < W) {
            v = src[((long long)x * Y + y) * W + w];
            if (comp) v = ~v & tail_mask(Z, W, w);
        }
        tile[sx][sy][sw] = v;
    }
    __syncthreads();
    const int lw = threadIdx.x % MW, ly = (threadIdx.x / MW) % MT, lx = threadIdx.x / (MW * MT);
    const int x = x0 + lx, y = y0 + ly, w = w0 + lw;
    if (x >= X || y >= Y || w >= W) return;
    u64 acc = 0;
    for (int k = 0; k < n_runs; ++k) {
        const int4 q = run[k];                                    // (dx, dy, lo, len): uniform over the block
        if (q.x < -MH || q.x > MH || q.y < -MH || q.y > MH || q.z <= -64 || q.w < 1 || q.w > 64 || q.z + q.w > 64) continue;   // not staged
        const u64 *p = tile[lx + MH + q.x][ly + MH + q.y] + lw;
        const u64 a = p[0], b = p[1], c = p[2];
        u64 lo, hi;                                               // bits [64 w + q.z, + 128) of the row
        if (q.z >= 0) {
            lo = funnel(b, c, q.z);
            hi = funnel(c, 0ull, q.z);
        } else {
            lo = funnel(a, b, 64 + q.z);
            hi = funnel(b, c, 64 + q.z);
        }
        int m = 1;                                                // lo covers the OR of m consecutive offsets
        while (2 * m <= q.w) {
            lo |= funnel(lo, hi, m);
            hi |= hi >> m;
            m *= 2;
        }
        if (m < q.w) lo |= funnel(lo, hi, q.w - m);
        acc |= lo;
    }
    if (comp) acc = ~acc;
    dst[((long long)x * Y + y) * W + w] = acc & tail_mask(Z, W, w);
}

struct CommitJobs {
    int res[MJ], target[MJ], first[MJ];
};

__global__ void __launch_bounds__(256) cascade_commit_kernel(u64 *__restrict__ pool, long long plane_words, int L, CommitJobs jobs)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= plane_words) return;
    const int j = blockIdx.y;
    const int target = jobs.target[j], first = jobs.first[j];
    const u64 res = pool[(long long)jobs.res[j] * plane_words + i];
    const u64 added = res & ~pool[(long long)target * plane_words + i];
    pool[(long long)target * plane_words + i] = res;
    if (!added) return;
    for (int l = 0; l < L; ++l)
        if (first + l != target) pool[(long long)(first + l) * plane_words + i] &= ~added;
}

// ---------------------------------------------------------------------------------------------------------------------------
// connected components of the planes (grid.y = plane)
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int SEL_BLOCK = 256;

struct Planes {
    Geo g;
    int W;                                             // words per row
    long long plane_words;
};

// K30's voxel source: the class of a voxel is its bit
struct BitSource {
    const u64 *plane;
    int Y, W;

    __device__ __forceinline__ u64 word(int x, int y, int z) const
    {
        return plane[((long long)x * Y + y) * W + (z >> 6)] >> (z & 63);
    }

    // z is a multiple of 4: the four voxels lie in one word, and the padding bits beyond Z are 0
    __device__ __forceinline__ uint32_t classes4(int x, int y, int z) const
    {
        const uint32_t b = (uint32_t)word(x, y, z);
        return (b & 1u) | (b & 2u) << 7 | (b & 4u) << 14 | (b & 8u) << 21;
    }

    __device__ __forceinline__ uint32_t class1(int x, int y, int z) const
    {
        return (uint32_t)word(x, y, z) & 1u;
    }
};

__global__ void __launch_bounds__(CC_BLOCK) cascade_cc_local_kernel(const u64 *__restrict__ planes, Planes p, int *__restrict__ parent,
                                                                     int *__restrict__ size)
{
    label_tile(BitSource{planes + blockIdx.y * p.plane_words, p.g.Y, p.W}, p.g, parent, size);
}

__global__ void __launch_bounds__(CC_BLOCK) cascade_cc_merge_kernel(const u64 *__restrict__ planes, Planes p, int *__restrict__ parent)
{
    merge_tiles(BitSource{planes + blockIdx.y * p.plane_words, p.g.Y, p.W}, p.g, parent);
}

// per 256 voxels the number of valid roots (size < thresh); table[plane] = (non-empty, n_valid)
__global__ void __launch_bounds__(256) cascade_cc_count_kernel(const int *__restrict__ parent, const int *__restrict__ size, long long N,
                                                               double thresh, int *__restrict__ blockcnt, int *__restrict__ table)
{
    __shared__ int roots, valid;
    if (threadIdx.x == 0) roots = valid = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < N && parent[blockIdx.y * N + i] == i) {
        atomicAdd(&roots, 1);
        if ((double)size[blockIdx.y * N + i] < thresh) atomicAdd(&valid, 1);
    }
    __syncthreads();
    if (threadIdx.x) return;
    blockcnt[(long long)blockIdx.y * gridDim.x + blockIdx.x] = valid;
    if (roots) atomicOr(&table[2 * blockIdx.y], 1);
    if (valid) atomicAdd(&table[2 * blockIdx.y + 1], valid);
}

// target[plane] = the rank[plane]-th valid root in index order, -1 when rank < 0 or there is none
__global__ void __launch_bounds__(SEL_BLOCK) cascade_cc_select_kernel(const int *__restrict__ parent, const int *__restrict__ size,
                                                                      long long N, double thresh, const int *__restrict__ blockcnt,
                                                                      int n_blocks, const int *__restrict__ rank,
                                                                      int *__restrict__ target)
{
    __shared__ int sums[SEL_BLOCK];
    const int pl = blockIdx.x, t = threadIdx.x;
    const int k = rank[pl];
    if (k < 0) return;                                 // target[] is -1 from the memset
    blockcnt += (long long)pl * n_blocks;
    parent += pl * N;
    size += pl * N;
    const int span = (n_blocks + SEL_BLOCK - 1) / SEL_BLOCK;
    const int b0 = min(t * span, n_blocks), b1 = min(b0 + span, n_blocks);
    int s = 0;
    for (int b = b0; b < b1; ++b) s += blockcnt[b];
    sums[t] = s;
    __syncthreads();
    int before = 0;
    for (int i = 0; i < t; ++i) before += sums[i];
    if (!(before <= k && k < before + s)) return;      // exactly one lane owns rank k (none when k >= n_valid)
    for (int b = b0; b < b1; ++b) {
        const int c = blockcnt[b];
        if (k >= before + c) {
            before += c;
            continue;
        }
        for (long long i = (long long)b * 256; i < N && i < (long long)(b + 1) * 256; ++i) {
            if (parent[i] != i || !((double)size[i] < thresh)) continue;
            if (before == k) {
                target[pl] = (int)i;
                return;
            }
            ++before;
        }
    }
}

// one wave per word: clears the voxels of the target component, and sets them in plane pl + fill[pl] when fill[pl] != 0
__global__ void __launch_bounds__(256) cascade_cc_remove_kernel(u64 *__restrict__ planes, Planes p, const int *__restrict__ parent,
                                                                const int *__restrict__ target, const int *__restrict__ fill)
{
    const int pl = blockIdx.y, lane = threadIdx.x & 63;
    const int tg = target[pl];
    if (tg < 0) return;
    const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (word >= p.plane_words) return;
    const int w = (int)(word % p.W);
    const long long row = word / p.W;
    const int z = w * 64 + lane;
    const u64 m = __ballot(z < p.g.Z && parent[pl * p.g.N + row * p.g.Z + z] == tg);
    if (lane || !m) return;
    atomicAnd(&planes[pl * p.plane_words + word], ~m);
    if (fill[pl]) atomicOr(&planes[(pl + fill[pl]) * p.plane_words + word], m);
}

bool planes_geometry(int P, int X, int Y, int Z, Planes &p)
{
    if (!geometry(P, X, Y, Z, p.g)) return false;
    p.W = (Z + 63) / 64;
    p.plane_words = (long long)X * Y * p.W;
    return true;
}

}  // namespace

extern "C" int mlagg_cascade_pack(const void *seg, int elem_bytes, long long sample_stride, int B, int X, int Y, int Z, const int *labels,
                                  int L, unsigned long long *planes, void *stream)
{
    if (!seg || !labels || !planes) return MLAGG_E_NULLPTR;
    if (B < 1 || X < 1 || Y < 1 || Z < 1 || L < 1 || L > MLAGG_CASCADE_MAX_LABELS || (elem_bytes != 2 && elem_bytes != 4))
        return MLAGG_E_UNSUPPORTED;
    const long long rows = (long long)X * Y, W = (Z + 63) / 64, n_words = (long long)B * rows * W;
    if (sample_stride < rows * Z || (n_words + 3) / 4 > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    Labels lab;
    for (int i = 0; i < MLAGG_CASCADE_MAX_LABELS; ++i) lab.v[i] = i < L ? labels[i] : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n_words + 3) / 4));
    if (elem_bytes == 2)
        hipLaunchKernelGGL(cascade_pack_kernel<short>, grid, dim3(256), 0, st, static_cast<const short *>(seg), sample_stride, L, lab,
                           rows, Z, (int)W, n_words, planes);
    else
        hipLaunchKernelGGL(cascade_pack_kernel<float>, grid, dim3(256), 0, st, static_cast<const float *>(seg), sample_stride, L, lab,
                           rows, Z, (int)W, n_words, planes);
    return (int)hipGetLastError();
}

extern "C" int mlagg_cascade_unpack(const unsigned long long *planes, int B, int L, int X, int Y, int Z, float *out, int C_total, int c0,
                                    void *stream)
{
    if (!planes || !out) return MLAGG_E_NULLPTR;
    if (B < 1 || L < 1 || X < 1 || Y < 1 || Z < 1 || c0 < 0 || c0 + L > C_total) return MLAGG_E_UNSUPPORTED;
    const long long rows = (long long)X * Y, n_vox = (long long)B * L * rows * Z;
    if ((n_vox + 255) / 256 > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    hipLaunchKernelGGL(cascade_unpack_kernel, dim3((unsigned)((n_vox + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       planes, L, rows, Z, (Z + 63) / 64, C_total, c0, n_vox, out);
    return (int)hipGetLastError();
}

extern "C" int mlagg_cascade_morph(unsigned long long *pool, int n_planes, int X, int Y, int Z, const int *runs, int n_runs_total,
                                   const int *jobs, int n_jobs, void *stream)
{
    if (!pool || !runs || !jobs) return MLAGG_E_NULLPTR;
    Planes p;
    if (!planes_geometry(1, X, Y, Z, p) || n_planes < 2 || n_jobs < 1 || n_runs_total < 1) return MLAGG_E_UNSUPPORTED;
    for (int j = 0; j < n_jobs; ++j) {
        const int *q = jobs + 5 * j;                                 // (src, dst, first run, runs, complement)
        if (q[0] < 0 || q[0] >= n_planes || q[1] < 0 || q[1] >= n_planes || q[0] == q[1] || q[2] < 0 || q[3] < 1 ||
            (long long)q[2] + q[3] > n_runs_total)
            return MLAGG_E_UNSUPPORTED;
        for (int i = 0; i < j; ++i)                                  // a launch's outputs are nobody's input or output
            if (jobs[5 * i + 1] == q[1] || jobs[5 * i + 1] == q[0] || jobs[5 * i] == q[1]) return MLAGG_E_UNSUPPORTED;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ntx = (X + MT - 1) / MT, nty = (Y + MT - 1) / MT, ntw = (p.W + MW - 1) / MW;
    if ((long long)ntx * nty * ntw > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    for (int j0 = 0; j0 < n_jobs; j0 += MJ) {
        const int nj = n_jobs - j0 < MJ ? n_jobs - j0 : MJ;
        MorphJobs mj = {};
        for (int j = 0; j < nj; ++j) {
            const int *q = jobs + 5 * (j0 + j);
            mj.src[j] = q[0];
            mj.dst[j] = q[1];
            mj.first_run[j] = q[2];
            mj.n_runs[j] = q[3];
            mj.complement[j] = q[4] != 0;
        }
        hipLaunchKernelGGL(cascade_morph_kernel, dim3((unsigned)(ntx * nty * ntw), (unsigned)nj), dim3(MT * MT * MW), 0, st, pool,
                           p.plane_words, X, Y, Z, p.W, ntx, nty, ntw, reinterpret_cast<const int4 *>(runs), mj);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}

extern "C" int mlagg_cascade_commit(unsigned long long *pool, int n_planes, int X, int Y, int Z, int L, const int *jobs, int n_jobs,
                                    void *stream)
{
    if (!pool || !jobs) return MLAGG_E_NULLPTR;
    Planes p;
    if (!planes_geometry(1, X, Y, Z, p) || L < 1 || n_jobs < 1) return MLAGG_E_UNSUPPORTED;
    for (int j = 0; j < n_jobs; ++j) {
        const int *q = jobs + 3 * j;                                 // (result plane, target plane, the sample's first plane)
        if (q[0] < 0 || q[0] >= n_planes || q[2] < 0 || q[2] + L > n_planes || q[1] < q[2] || q[1] >= q[2] + L ||
            (q[0] >= q[2] && q[0] < q[2] + L))
            return MLAGG_E_UNSUPPORTED;
        for (int i = 0; i < j; ++i)                                  // one job per sample and launch
            if (jobs[3 * i + 2] < q[2] + L && q[2] < jobs[3 * i + 2] + L) return MLAGG_E_UNSUPPORTED;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((p.plane_words + 255) / 256);
    for (int j0 = 0; j0 < n_jobs; j0 += MJ) {
        const int nj = n_jobs - j0 < MJ ? n_jobs - j0 : MJ;
        CommitJobs cj = {};
        for (int j = 0; j < nj; ++j) {
            cj.res[j] = jobs[3 * (j0 + j)];
            cj.target[j] = jobs[3 * (j0 + j) + 1];
            cj.first[j] = jobs[3 * (j0 + j) + 2];
        }
        hipLaunchKernelGGL(cascade_commit_kernel, dim3(blocks, (unsigned)nj), dim3(256), 0, st, pool, p.plane_words, L, cj);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}

extern "C" size_t mlagg_cascade_cc_blocks(int X, int Y, int Z)
{
    return (size_t)(((long long)X * Y * Z + 255) / 256);
}

extern "C" int mlagg_cascade_cc_stats(const unsigned long long *planes, int P, int X, int Y, int Z, double thresh, int *parent,
                                      int *size, int *blockcnt, int *table, void *stream)
{
    if (!planes || !parent || !size || !blockcnt || !table) return MLAGG_E_NULLPTR;
    Planes p;
    if (!planes_geometry(P, X, Y, Z, p)) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipError_t e = hipMemsetAsync(table, 0, 2 * (size_t)P * sizeof(int), st)) return (int)e;
    const long long N = p.g.N;
    const dim3 tiles(tile_count(p.g), (unsigned)P), vox((unsigned)((N + 255) / 256), (unsigned)P);
    hipLaunchKernelGGL(cascade_cc_local_kernel, tiles, dim3(CC_BLOCK), 0, st, planes, p, parent, size);
    hipLaunchKernelGGL(cascade_cc_merge_kernel, tiles, dim3(CC_BLOCK), 0, st, planes, p, parent);
    hipLaunchKernelGGL(mlagg_uf::compress_kernel<>, vox, dim3(256), 0, st, parent, N);
    hipLaunchKernelGGL(mlagg_uf::size_kernel<>, vox, dim3(256), 0, st, parent, size, N);
    hipLaunchKernelGGL(cascade_cc_count_kernel, vox, dim3(256), 0, st, parent, size, N, thresh, blockcnt, table);
    return (int)hipGetLastError();
}

extern "C" int mlagg_cascade_cc_remove(unsigned long long *planes, int P, int X, int Y, int Z, double thresh, const int *parent,
                                       const int *size, const int *blockcnt, const int *rank, const int *fill, int *target,
                                       void *stream)
{
    if (!planes || !parent || !size || !blockcnt || !rank || !fill || !target) return MLAGG_E_NULLPTR;
    Planes p;
    if (!planes_geometry(P, X, Y, Z, p)) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipError_t e = hipMemsetAsync(target, 0xff, (size_t)P * sizeof(int), st)) return (int)e;
    hipLaunchKernelGGL(cascade_cc_select_kernel, dim3((unsigned)P), dim3(SEL_BLOCK), 0, st, parent, size, p.g.N, thresh, blockcnt,
                       (int)((p.g.N + 255) / 256), rank, target);
    hipLaunchKernelGGL(cascade_cc_remove_kernel, dim3((unsigned)((p.plane_words + 3) / 4), (unsigned)P), dim3(256), 0, st, planes, p,
                       parent, target, fill);
    return (int)hipGetLastError();
}
