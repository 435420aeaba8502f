// K27 -- cell-instance F1 evaluation on the device (the microscopy metric of the reference's evaluation/compute_cell_metric.py).
//
// What it replaces, per image: skimage.measure.label(seg == 1) (full, 8-neighbour connectivity, components numbered in raster order
// of their first pixel), dice(gt > 0, seg > 0), remove_boundary_cells + segmentation.relabel_sequential on both maps (every label
// seen in the 2-pixel ring is dropped, the rest renumbered 1..n in order), the numba pixel loop _label_overlap, and the IoU matrix
// with its threshold test.  The assignment itself stays on the host (cells.py): when no row and no column of {iou >= th} holds more
// than one edge the edge count is the answer, otherwise the edge list goes to a maximum bipartite matching.
//
// Entry points and their kernels (one launch each, no inter-workgroup waiting inside a kernel):
//   mlagg_cells_label
//     cl_local_kernel     tile-local union-find in LDS over a 32 x 64 pixel tile (512 lanes, 4 consecutive pixels each) with the four
//                         backward neighbours W, NW, N, NE; writes parent[v] = global index of v's tile root, -1 off the mask; with a
//                         gt map also the three dice counts |gt > 0|, |seg == fg|, |both| (LDS partials, one global add per block);
//     cl_merge_kernel     pixels on a tile edge unite their tree with the neighbour tiles' trees in the global parent array;
//     mlagg_uf::compress_kernel   parent[v] = find(v), the kernel the 3-D labellings use.  Links go towards the smaller index
//                         (unionfind.h), so every root is its component's minimum linear index = its first pixel in raster order,
//                         whatever the schedule.
//   mlagg_cells_relabel   order-preserving compaction of a key map (a label map, or parent + 1) to 1..n over a rectangular view:
//     cl_flag_kernel      present[key] = 1, and removed[key] = 1 for keys seen in the view's 2-pixel ring (plain byte stores of 1);
//     cl_scan_count / cl_scan_offsets / cl_scan_apply   exclusive scan of present & ~removed over the key domain -> newid[key];
//     cl_rewrite_kernel   out = newid[key].
//   mlagg_cells_overlap
//     cl_overlap_kernel   the dense (n_true + 1) x (n_pred + 1) pixel-count matrix and both area vectors in one pass: each lane walks
//                         16 pixels of a row and issues one integer atomic per run of equal labels; background runs are summed per
//                         block first, since they would all hit one address.
//   mlagg_cells_match
//     cl_match_kernel     iou = ov / (a_t + a_p - ov) in float64 (0 where that is 0 / 0), written out only when asked; per threshold
//                         the edge count and the largest row and column degree of {iou >= th}, rows and columns 0 excluded; or, on a
//                         second call for one threshold, the edge list itself (its order is the schedule's: the host sorts it).
// All atomics are integer atomics: every count is independent of the schedule and equal to the host path's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlagg_hip.h"
#include "prof.h"
#include "unionfind.h"

namespace {

using namespace mlagg_uf;

constexpr int TH = 32, TW = 64;                        // tile: rows x columns, x is the contiguous axis
constexpr int TP = TH * TW;                            // 2048 pixels
constexpr int CL_BLOCK = 512;                          // 4 consecutive pixels per lane
constexpr int SCAN_LANE = 16, SCAN_BLOCK = 256;
constexpr int SCAN_CHUNK = SCAN_LANE * SCAN_BLOCK;     // 4096 keys per block
constexpr int RUN = 16;                                // pixels per lane in cl_overlap_kernel
constexpr int MAX_T = MLAGG_CELLS_MAX_THRESHOLDS;

struct Img {
    const void *seg;
    int elem;                                          // bytes per pixel of seg: 1 (uint8) or 4 (int32)
    int fg;                                            // the foreground value
    int H, W;
    int nty, ntx;
    bool vec;                                          // uint8, W % 4 == 0 and a 4-byte aligned base: dword loads
};

__device__ __forceinline__ bool is_fg(const Img &m, long long o)
{
    const int v = m.elem == 1 ? (int)static_cast<const uint8_t *>(m.seg)[o] : static_cast<const int *>(m.seg)[o];
    return v == m.fg;
}

// foreground bits of the four pixels (y, x..x+3), 0 beyond W; y < H and x < W are the caller's
__device__ __forceinline__ uint32_t fg4(const Img &m, int y, int x)
{
    const long long o = (long long)y * m.W + x;
    uint32_t bits = 0;
    if (m.vec && x + 4 <= m.W) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(m.seg) + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) bits |= (uint32_t)((int)((w >> (8 * j)) & 255) == m.fg) << j;
        return bits;
    }
    for (int j = 0; j < 4 && x + j < m.W; ++j) bits |= (uint32_t)is_fg(m, o + j) << j;
    return bits;
}

__global__ void __launch_bounds__(CL_BLOCK) cl_local_kernel(Img m, const int *__restrict__ gt, int *__restrict__ parent,
                                                             int *__restrict__ counts)
{
    __shared__ int par[TP];
    __shared__ uint8_t msk[TP];
    __shared__ int dice[3];
    const int t = threadIdx.x;
    if (t < 3) dice[t] = 0;
    const int y0 = (blockIdx.x / m.ntx) * TH, x0 = (blockIdx.x % m.ntx) * TW;
    const int lx = (t & 15) * 4, ly = t >> 4;
    const int y = y0 + ly, x = x0 + lx;
    const bool row = y < m.H && x < m.W;
    const uint32_t bits = row ? fg4(m, y, x) : 0u;
    const int l0 = ly * TW + lx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        msk[l0 + j] = (bits >> j) & 1;
        par[l0 + j] = l0 + j;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!((bits >> j) & 1)) continue;
        const int cx = lx + j, me = l0 + j;
        if (cx > 0 && msk[me - 1]) lds_unite(par, me, me - 1);                         // W
        if (ly > 0) {
            if (cx > 0 && msk[me - TW - 1]) lds_unite(par, me, me - TW - 1);           // NW
            if (msk[me - TW]) lds_unite(par, me, me - TW);                             // N
            if (cx + 1 < TW && msk[me - TW + 1]) lds_unite(par, me, me - TW + 1);      // NE
        }
    }
    __syncthreads();
    int n_gt = 0, n_seg = 0, n_both = 0;
    if (row) {
        const long long o = (long long)y * m.W + x;
        for (int j = 0; j < 4 && x + j < m.W; ++j) {
            const bool f = (bits >> j) & 1;
            int p = -1;
            if (f) {
                const int r = lds_find(par, l0 + j);
                p = (int)((long long)(y0 + r / TW) * m.W + (x0 + r % TW));
            }
            parent[o + j] = p;
            if (gt) {
                const bool g = gt[o + j] > 0;
                n_gt += g;
                n_both += g && f;
            }
            n_seg += f;
        }
    }
    if (n_gt) atomicAdd(&dice[0], n_gt);
    if (n_seg) atomicAdd(&dice[1], n_seg);
    if (n_both) atomicAdd(&dice[2], n_both);
    __syncthreads();
    if (t < 3 && dice[t]) atomicAdd(&counts[t], dice[t]);
}

__global__ void __launch_bounds__(CL_BLOCK) cl_merge_kernel(Img m, int *__restrict__ parent)
{
    const int t = threadIdx.x;
    const int y0 = (blockIdx.x / m.ntx) * TH, x0 = (blockIdx.x % m.ntx) * TW;
    const int lx = (t & 15) * 4, ly = t >> 4;
    const int y = y0 + ly, x = x0 + lx;
    // only pixels of the first row and of the first and last column have backward neighbours in another tile
    if (!(ly == 0 || lx == 0 || lx + 4 == TW) || y >= m.H || x >= m.W) return;
    const uint32_t bits = fg4(m, y, x);
    for (int j = 0; j < 4 && x + j < m.W; ++j) {
        if (!((bits >> j) & 1)) continue;
        const int cx = lx + j, gx = x + j;
        const int me = (int)((long long)y * m.W + gx);
        if (cx == 0 && gx > 0 && is_fg(m, (long long)me - 1)) gunite(parent, me, me - 1);                       // W
        if (y > 0) {
            const long long up = (long long)me - m.W;
            if ((ly == 0 || cx == 0) && gx > 0 && is_fg(m, up - 1)) gunite(parent, me, (int)(up - 1));          // NW
            if (ly == 0 && is_fg(m, up)) gunite(parent, me, (int)up);                                           // N
            if ((ly == 0 || cx == TW - 1) && gx + 1 < m.W && is_fg(m, up + 1)) gunite(parent, me, (int)(up + 1));   // NE
        }
    }
}

// A rectangular view of a key map: key = keys[r * stride + c] + bias for r < h, c < w; the view stands for an Hr x Wr image (the
// rest of it is zero padding), whose 2-pixel ring is r < 2, r >= Hr - 2, c < 2, c >= Wr - 2.
struct View {
    const int *keys;
    int bias;
    long long stride;
    int h, w, Hr, Wr;
    long long D;                                       // keys lie in [0, D); 0 is the background
};

__global__ void __launch_bounds__(256) cl_flag_kernel(View v, int ring, uint8_t *__restrict__ present, uint8_t *__restrict__ removed)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)v.h * v.w) return;
    const int r = (int)(i / v.w), c = (int)(i % v.w);
    const long long k = (long long)v.keys[r * v.stride + c] + v.bias;
    if (k <= 0 || k >= v.D) return;
    present[k] = 1;
    if (ring && (r < 2 || r >= v.Hr - 2 || c < 2 || c >= v.Wr - 2)) removed[k] = 1;
}

__device__ __forceinline__ int kept(const uint8_t *present, const uint8_t *removed, long long k, long long D)
{
    return k > 0 && k < D && present[k] && !removed[k];
}

__global__ void __launch_bounds__(SCAN_BLOCK) cl_scan_count_kernel(const uint8_t *__restrict__ present,
                                                                    const uint8_t *__restrict__ removed, long long D,
                                                                    int *__restrict__ blocksum)
{
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const long long k0 = (long long)blockIdx.x * SCAN_CHUNK + threadIdx.x * SCAN_LANE;
    int s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_LANE; ++j) s += kept(present, removed, k0 + j, D);
    if (s) atomicAdd(&total, s);
    __syncthreads();
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
}

// exclusive scan of blocksum[0..nb) in place by one workgroup; total[0] = the sum
__global__ void __launch_bounds__(1024) cl_scan_offsets_kernel(int *__restrict__ blocksum, int nb, int *__restrict__ total)
{
    __shared__ int buf[1024];
    __shared__ int carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += 1024) {
        const int mine = base + t < nb ? blocksum[base + t] : 0;
        buf[t] = mine;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int add = t >= d ? buf[t - d] : 0;
            __syncthreads();
            buf[t] += add;
            __syncthreads();
        }
        const int c = carry;
        if (base + t < nb) blocksum[base + t] = c + buf[t] - mine;
        __syncthreads();
        if (t == 1023) carry = c + buf[1023];
        __syncthreads();
    }
    if (t == 0) total[0] = carry;
}

__global__ void __launch_bounds__(SCAN_BLOCK) cl_scan_apply_kernel(const uint8_t *__restrict__ present,
                                                                    const uint8_t *__restrict__ removed, long long D,
                                                                    const int *__restrict__ blocksum, int *__restrict__ newid)
{
    __shared__ int buf[SCAN_BLOCK];
    const int t = threadIdx.x;
    const long long k0 = (long long)blockIdx.x * SCAN_CHUNK + t * SCAN_LANE;
    int f[SCAN_LANE], s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_LANE; ++j) {
        f[j] = kept(present, removed, k0 + j, D);
        s += f[j];
    }
    buf[t] = s;
    __syncthreads();
    for (int d = 1; d < SCAN_BLOCK; d <<= 1) {
        const int add = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    int id = blocksum[blockIdx.x] + buf[t] - s;        // kept keys before this lane's first
#pragma unroll
    for (int j = 0; j < SCAN_LANE; ++j) {
        if (k0 + j < D) newid[k0 + j] = f[j] ? id + 1 : 0;
        id += f[j];
    }
}

__global__ void __launch_bounds__(256) cl_rewrite_kernel(View v, const int *__restrict__ newid, int *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)v.h * v.w) return;
    const int r = (int)(i / v.w), c = (int)(i % v.w);
    const long long k = (long long)v.keys[r * v.stride + c] + v.bias;
    out[i] = (k > 0 && k < v.D) ? newid[k] : 0;
}

__global__ void __launch_bounds__(256) cl_overlap_kernel(const int *__restrict__ g, const int *__restrict__ p, int h, int w,
                                                         int n_true, int n_pred, int *__restrict__ overlap,
                                                         int *__restrict__ area_t, int *__restrict__ area_p)
{
    __shared__ int bg[3];                              // (0, 0) pairs, gt background, prediction background of this block
    if (threadIdx.x < 3) bg[threadIdx.x] = 0;
    __syncthreads();
    const int segs = (w + RUN - 1) / RUN;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int z_pair = 0, z_t = 0, z_p = 0;
    if (i < (long long)h * segs) {
        const int r = (int)(i / segs), c0 = (int)(i % segs) * RUN;
        const long long o = (long long)r * w + c0;
        const int n = min(RUN, w - c0);
        const long long pitch = (long long)n_pred + 1;
        int cg = -1, cp = -1, n_pair = 0, n_g = 0, n_p = 0;
        for (int j = 0; j <= n; ++j) {
            int a = -1, b = -1;
            if (j < n) {
                a = g[o + j];
                b = p[o + j];
                if (a < 0 || a > n_true || b < 0 || b > n_pred) a = b = -2;       // outside the matrix: never counted
            }
            if (a != cg || b != cp) {
                if (n_pair && cg >= 0) {
                    if ((cg | cp) == 0) z_pair += n_pair;
                    else atomicAdd(&overlap[cg * pitch + cp], n_pair);
                }
                n_pair = 0;
            }
            if (a != cg) {
                if (n_g && cg >= 0) {
                    if (cg == 0) z_t += n_g;
                    else atomicAdd(&area_t[cg], n_g);
                }
                n_g = 0;
                cg = a;
            }
            if (b != cp) {
                if (n_p && cp >= 0) {
                    if (cp == 0) z_p += n_p;
                    else atomicAdd(&area_p[cp], n_p);
                }
                n_p = 0;
                cp = b;
            }
            ++n_pair;
            ++n_g;
            ++n_p;
        }
    }
    if (z_pair) atomicAdd(&bg[0], z_pair);
    if (z_t) atomicAdd(&bg[1], z_t);
    if (z_p) atomicAdd(&bg[2], z_p);
    __syncthreads();
    if (threadIdx.x == 0 && bg[0]) atomicAdd(&overlap[0], bg[0]);
    if (threadIdx.x == 1 && bg[1]) atomicAdd(&area_t[0], bg[1]);
    if (threadIdx.x == 2 && bg[2]) atomicAdd(&area_p[0], bg[2]);
}

struct Thresholds {
    double th[MAX_T];
    int n;
};

__global__ void __launch_bounds__(256) cl_match_kernel(const int *__restrict__ overlap, const int *__restrict__ area_t,
                                                       const int *__restrict__ area_p, int n_true, int n_pred, Thresholds T,
                                                       double *__restrict__ iou, int *__restrict__ degrees, int *__restrict__ stats,
                                                       int *__restrict__ edges, int edge_cap)
{
    const long long pitch = (long long)n_pred + 1, rows = (long long)n_true + 1;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * pitch) return;
    const int i = (int)(e / pitch), j = (int)(e % pitch);
    const long long ov = overlap[e];
    const long long den = (long long)area_t[i] + area_p[j] - ov;
    const double v = den == 0 ? 0.0 : (double)ov / (double)den;          // the reference's NaN (0 / 0) set to 0
    if (iou) iou[e] = v;
    if (i == 0 || j == 0) return;
    if (edges) {                                                         // the list of one threshold
        if (v >= T.th[0]) {
            const int slot = atomicAdd(&stats[3], 1);
            if (slot < edge_cap) {
                edges[2 * slot] = i - 1;
                edges[2 * slot + 1] = j - 1;
            }
        }
        return;
    }
    int *rowdeg = degrees, *coldeg = degrees + (long long)MAX_T * rows;
    for (int t = 0; t < T.n; ++t) {
        if (!(v >= T.th[t])) continue;
        atomicAdd(&stats[4 * t], 1);
        const int dr = atomicAdd(&rowdeg[t * rows + i], 1) + 1;
        const int dc = atomicAdd(&coldeg[t * pitch + j], 1) + 1;
        if (dr > 1) atomicMax(&stats[4 * t + 1], dr);
        if (dc > 1) atomicMax(&stats[4 * t + 2], dc);
    }
}

}  // namespace

extern "C" int mlagg_cells_label(const void *seg, int elem_bytes, int foreground, const int *gt, int H, int W, int *parent,
                                 int *counts, void *stream)
{
    if (H < 1 || W < 1 || (elem_bytes != 1 && elem_bytes != 4)) return MLAGG_E_UNSUPPORTED;
    const long long N = (long long)H * W;
    if (N > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    if (!seg || !parent || !counts) return MLAGG_E_NULLPTR;
    if (elem_bytes == 4 && (reinterpret_cast<uintptr_t>(seg) & 3)) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Img m;
    m.seg = seg;
    m.elem = elem_bytes;
    m.fg = foreground;
    m.H = H;
    m.W = W;
    m.nty = (H + TH - 1) / TH;
    m.ntx = (W + TW - 1) / TW;
    m.vec = elem_bytes == 1 && (W % 4) == 0 && !(reinterpret_cast<uintptr_t>(seg) & 3);
    const long long tiles = (long long)m.nty * m.ntx;
    if (hipError_t e = hipMemsetAsync(counts, 0, 3 * sizeof(int), st)) return (int)e;
    {
        MLAGG_TIMED(K_CL_LOCAL, st);
        hipLaunchKernelGGL(cl_local_kernel, dim3((unsigned)tiles), dim3(CL_BLOCK), 0, st, m, gt, parent, counts);
    }
    {
        MLAGG_TIMED(K_CL_MERGE, st);
        hipLaunchKernelGGL(cl_merge_kernel, dim3((unsigned)tiles), dim3(CL_BLOCK), 0, st, m, parent);
    }
    {
        MLAGG_TIMED(K_CL_COMPRESS, st);
        hipLaunchKernelGGL(mlagg_uf::compress_kernel<>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, parent, N);
    }
    return (int)hipGetLastError();
}

extern "C" size_t mlagg_cells_scan_blocks(long long D)
{
    return D < 1 ? 0 : (size_t)((D + SCAN_CHUNK - 1) / SCAN_CHUNK);
}

extern "C" int mlagg_cells_relabel(const int *keys, int bias, long long stride, int h, int w, int Hr, int Wr, int ring, long long D,
                                   unsigned char *flags, int *newid, int *blocksum, int *total, int *out, void *stream)
{
    if (h < 1 || w < 1 || Hr < h || Wr < w || stride < w || D < 1 || D > 2147483648LL) return MLAGG_E_UNSUPPORTED;
    if (ring && (Hr < 5 || Wr < 5)) return MLAGG_E_UNSUPPORTED;
    if ((long long)h * w > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    if (!keys || !flags || !newid || !blocksum || !total || !out) return MLAGG_E_NULLPTR;
    hipStream_t st = static_cast<hipStream_t>(stream);
    View v{keys, bias, stride, h, w, Hr, Wr, D};
    uint8_t *present = flags, *removed = flags + D;
    if (hipError_t e = hipMemsetAsync(flags, 0, (size_t)(2 * D), st)) return (int)e;
    const unsigned pblocks = (unsigned)(((long long)h * w + 255) / 256);
    const int nb = (int)mlagg_cells_scan_blocks(D);
    {
        MLAGG_TIMED(K_CL_FLAG, st);
        hipLaunchKernelGGL(cl_flag_kernel, dim3(pblocks), dim3(256), 0, st, v, ring, present, removed);
    }
    {
        MLAGG_TIMED(K_CL_SCAN, st);
        hipLaunchKernelGGL(cl_scan_count_kernel, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, present, removed, D, blocksum);
        hipLaunchKernelGGL(cl_scan_offsets_kernel, dim3(1), dim3(1024), 0, st, blocksum, nb, total);
        hipLaunchKernelGGL(cl_scan_apply_kernel, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, present, removed, D, blocksum, newid);
    }
    {
        MLAGG_TIMED(K_CL_REWRITE, st);
        hipLaunchKernelGGL(cl_rewrite_kernel, dim3(pblocks), dim3(256), 0, st, v, newid, out);
    }
    return (int)hipGetLastError();
}

extern "C" int mlagg_cells_overlap(const int *g, const int *p, int h, int w, int n_true, int n_pred, int *overlap, int *area_t,
                                   int *area_p, void *stream)
{
    if (h < 1 || w < 1 || n_true < 0 || n_pred < 0 || (long long)h * w > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    const long long entries = ((long long)n_true + 1) * ((long long)n_pred + 1);
    if (entries * 4 > MLAGG_CELLS_MAX_OVERLAP_BYTES) return MLAGG_E_UNSUPPORTED;
    if (!g || !p || !overlap || !area_t || !area_p) return MLAGG_E_NULLPTR;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipError_t e = hipMemsetAsync(overlap, 0, (size_t)entries * 4, st)) return (int)e;
    if (hipError_t e = hipMemsetAsync(area_t, 0, ((size_t)n_true + 1) * 4, st)) return (int)e;
    if (hipError_t e = hipMemsetAsync(area_p, 0, ((size_t)n_pred + 1) * 4, st)) return (int)e;
    const long long lanes = (long long)h * ((w + RUN - 1) / RUN);
    MLAGG_TIMED(K_CL_OVERLAP, st);
    hipLaunchKernelGGL(cl_overlap_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, g, p, h, w, n_true, n_pred, overlap,
                       area_t, area_p);
    return (int)hipGetLastError();
}

extern "C" int mlagg_cells_match(const int *overlap, const int *area_t, const int *area_p, int n_true, int n_pred,
                                 const double *thresholds, int n_thresholds, double *iou, int *degrees, int *stats, int *edges,
                                 int edge_cap, void *stream)
{
    if (n_true < 0 || n_pred < 0 || n_thresholds < 0 || n_thresholds > MAX_T) return MLAGG_E_UNSUPPORTED;
    if (edges && (n_thresholds != 1 || edge_cap < 1)) return MLAGG_E_UNSUPPORTED;
    const long long rows = (long long)n_true + 1, pitch = (long long)n_pred + 1;
    if (rows * pitch * 4 > MLAGG_CELLS_MAX_OVERLAP_BYTES) return MLAGG_E_UNSUPPORTED;
    if (!overlap || !area_t || !area_p || !stats || (n_thresholds && !thresholds) || (!edges && !degrees)) return MLAGG_E_NULLPTR;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Thresholds T;
    T.n = n_thresholds;
    for (int t = 0; t < MAX_T; ++t) T.th[t] = t < n_thresholds ? thresholds[t] : 0.0;
    if (hipError_t e = hipMemsetAsync(stats, 0, 4 * MAX_T * sizeof(int), st)) return (int)e;
    if (!edges)
        if (hipError_t e = hipMemsetAsync(degrees, 0, (size_t)(MAX_T * (rows + pitch)) * sizeof(int), st)) return (int)e;
    MLAGG_TIMED(K_CL_MATCH, st);
    hipLaunchKernelGGL(cl_match_kernel, dim3((unsigned)((rows * pitch + 255) / 256)), dim3(256), 0, st, overlap, area_t, area_p, n_true,
                       n_pred, T, iou, degrees, stats, edges, edge_cap);
    return (int)hipGetLastError();
}
