// K23 -- keep the largest connected component on the device (nnU-Net's postprocessing by connected components).
//
// What it replaces: remove_all_but_largest_component_from_segmentation (nnunetv2/postprocessing/remove_connected_components.py:
// 22-34), which unites the masks of the requested labels or regions into one boolean volume and hands it to acvl_utils'
// remove_all_but_largest_component: skimage.measure.label(connectivity=None) = full (26-neighbour) connectivity, np.bincount of the
// component ids, every component whose size equals the maximum is kept, the rest of the mask becomes background_label.
//
// One launch works on a uint8 label volume (X, Y, Z) and a 256-entry uint8 group table: group[label] = 0 leaves the voxel out of every
// mask, and two voxels are connected when they are 26-neighbours with the same non-zero group.  Mapping every listed label to group 1
// is the reference's united mask; mapping each label to itself labels every class at once (the per-class steps of
// determine_postprocessing), which is exact because removing one class's components never changes another class's components.
//
// Phases, one launch each, no inter-workgroup waiting inside a kernel:
//   cc_local_kernel    tile-local union-find in LDS (Playne-Hawick style: atomicMin links the larger root to the smaller one) over
//                      the 13 backward neighbours inside an 8 x 8 x 32 tile, read with one dword load of four labels per lane;
//                      writes parent[v] = the global index of v's tile root (-1 outside the mask), size[v] = the tile component's
//                      voxel count at its tile root (0 elsewhere), and the per-group voxel counts (LDS histogram, one global add
//                      per group and tile);
//   cc_merge_kernel    the voxels whose backward neighbours lie in another tile unite the two trees in the global parent array with
//                      the same atomicMin linking; a stale parent read from another XCD's L2 is always an ancestor in the same set,
//                      and a failed link returns the current value, so the loop converges;
//   cc_compress_kernel parent[v] = find(v): with links always towards the smaller index, every component's root is its minimum linear
//                      index, whatever the schedule;
//   cc_size_kernel     each tile root adds its tile count into its component root: one global integer atomic per tile component
//                      (the per-voxel adds were aggregated in LDS in cc_local_kernel), not one per voxel;
//   cc_max_kernel      every component root takes the per-group maximum of the sizes (LDS maximum per workgroup, then one
//                      atomicMax per group into 256 slots);
//   cc_write_kernel    out[v] = background when group != 0 and the component is smaller than its group's maximum, label otherwise
//                      (ties at the maximum are all kept), plus the per-group kept counts.
// Every result is an integer and independent of the schedule: bit-identical to the host path.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlagg_hip.h"
#include "prof.h"
#include "unionfind.h"

namespace {

using namespace mlagg_uf;

constexpr int TX = 8, TY = 8, TZ = 32;                 // tile; z is the contiguous axis
constexpr int TV = TX * TY * TZ;                       // 2048 voxels
constexpr int CC_BLOCK = 512;                          // 4 consecutive z voxels per lane
constexpr int NG = 256;                                // group slots

struct Vol {
    const uint8_t *lab;
    const uint8_t *group;
    int X, Y, Z;
    int ntx, nty, ntz;                                 // tiles per axis
    bool vec;                                          // Z % 4 == 0 and a 4-byte aligned base: dword label loads
};

struct Tile {
    int x0, y0, z0;
};

__device__ __forceinline__ Tile tile_of(const Vol &v, int b)
{
    const int tz = b % v.ntz, r = b / v.ntz;
    return Tile{(r / v.nty) * TX, (r % v.nty) * TY, tz * TZ};
}

// the 13 backward neighbours: (dx, dy, dz) lexicographically negative
__device__ __forceinline__ void backward(int i, int &dx, int &dy, int &dz)
{
    // i in [0, 13): i < 9 -> dx = -1 with (dy, dz) in {-1, 0, 1}^2; 9..11 -> dx = 0, dy = -1; 12 -> (0, 0, -1)
    if (i < 9) {
        dx = -1;
        dy = i / 3 - 1;
        dz = i % 3 - 1;
    } else if (i < 12) {
        dx = 0;
        dy = -1;
        dz = i - 10;
    } else {
        dx = 0;
        dy = 0;
        dz = -1;
    }
}

// four labels at (x, y, z..z+3) of the volume, 0 beyond Z; x < X and y < Y are the caller's
__device__ __forceinline__ uint32_t load4(const Vol &v, int x, int y, int z)
{
    const long long o = ((long long)x * v.Y + y) * v.Z + z;
    if (v.vec && z + 4 <= v.Z) return *reinterpret_cast<const uint32_t *>(v.lab + o);
    uint32_t w = 0;
    for (int j = 0; j < 4 && z + j < v.Z; ++j) w |= (uint32_t)v.lab[o + j] << (8 * j);
    return w;
}

__device__ __forceinline__ void lane_coords(int t, int &lx, int &ly, int &lz)
{
    lz = (t & 7) * 4;
    ly = (t >> 3) & 7;
    lx = t >> 6;
}

__global__ void __launch_bounds__(CC_BLOCK) cc_local_kernel(Vol v, int *__restrict__ parent, int *__restrict__ size,
                                                             int *__restrict__ count)
{
    __shared__ int par[TV];
    __shared__ int cnt[TV];
    __shared__ uint8_t grp[TV];
    __shared__ uint8_t gtab[NG];
    __shared__ int hist[NG];
    const int t = threadIdx.x;
    if (t < NG) {
        gtab[t] = v.group[t];
        hist[t] = 0;
    }
    const Tile T = tile_of(v, blockIdx.x);
    int lx, ly, lz;
    lane_coords(t, lx, ly, lz);
    const int x = T.x0 + lx, y = T.y0 + ly, z = T.z0 + lz;
    const bool row = x < v.X && y < v.Y && z < v.Z;
    const uint32_t w = row ? load4(v, x, y, z) : 0u;
    __syncthreads();
    const int l0 = (lx * TY + ly) * TZ + lz;
    uint8_t g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        g[j] = (row && z + j < v.Z) ? gtab[(w >> (8 * j)) & 255] : 0;
        grp[l0 + j] = g[j];
        par[l0 + j] = l0 + j;
        cnt[l0 + j] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!g[j]) continue;
        for (int i = 0; i < 13; ++i) {
            int dx, dy, dz;
            backward(i, dx, dy, dz);
            const int nx = lx + dx, ny = ly + dy, nz = lz + j + dz;
            if (nx < 0 || ny < 0 || ny >= TY || nz < 0 || nz >= TZ) continue;
            const int n = (nx * TY + ny) * TZ + nz;
            if (grp[n] == g[j]) lds_unite(par, l0 + j, n);
        }
    }
    __syncthreads();
    int root[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        root[j] = -1;
        if (g[j]) {
            root[j] = lds_find(par, l0 + j);
            atomicAdd(&cnt[root[j]], 1);
            atomicAdd(&hist[g[j]], 1);
        }
    }
    __syncthreads();
    if (row) {
        const long long o = ((long long)x * v.Y + y) * v.Z + z;
        for (int j = 0; j < 4 && z + j < v.Z; ++j) {
            int p = -1, s = 0;
            if (g[j]) {
                const int r = root[j];
                const int rx = r / (TY * TZ), ry = (r / TZ) % TY, rz = r % TZ;
                p = (int)(((long long)(T.x0 + rx) * v.Y + (T.y0 + ry)) * v.Z + (T.z0 + rz));
                if (r == l0 + j) s = cnt[r];
            }
            parent[o + j] = p;
            size[o + j] = s;
        }
    }
    if (t < NG && t > 0 && hist[t]) atomicAdd(&count[t], hist[t]);
}

__global__ void __launch_bounds__(CC_BLOCK) cc_merge_kernel(Vol v, int *__restrict__ parent)
{
    __shared__ uint8_t gtab[NG];
    const int t = threadIdx.x;
    if (t < NG) gtab[t] = v.group[t];
    const Tile T = tile_of(v, blockIdx.x);
    int lx, ly, lz;
    lane_coords(t, lx, ly, lz);
    const int x = T.x0 + lx, y = T.y0 + ly, z = T.z0 + lz;
    __syncthreads();
    // only lanes on a tile face have backward neighbours in another tile
    const bool face = lx == 0 || ly == 0 || ly == TY - 1 || lz == 0 || lz + 4 == TZ;
    if (!face || x >= v.X || y >= v.Y || z >= v.Z) return;
    const uint32_t w = load4(v, x, y, z);
    for (int j = 0; j < 4 && z + j < v.Z; ++j) {
        const int lzj = lz + j;
        if (!(lx == 0 || ly == 0 || ly == TY - 1 || lzj == 0 || lzj == TZ - 1)) continue;
        const uint8_t g = gtab[(w >> (8 * j)) & 255];
        if (!g) continue;
        const int me = (int)(((long long)x * v.Y + y) * v.Z + z + j);
        for (int i = 0; i < 13; ++i) {
            int dx, dy, dz;
            backward(i, dx, dy, dz);
            const int nlx = lx + dx, nly = ly + dy, nlz = lzj + dz;
            if (nlx >= 0 && nly >= 0 && nly < TY && nlz >= 0 && nlz < TZ) continue;      // same tile: done in cc_local_kernel
            const int nx = x + dx, ny = y + dy, nz = z + j + dz;
            if (nx < 0 || ny < 0 || ny >= v.Y || nz < 0 || nz >= v.Z) continue;
            const int n = (int)(((long long)nx * v.Y + ny) * v.Z + nz);
            if (gtab[v.lab[n]] == g) gunite(parent, me, n);
        }
    }
}

__global__ void __launch_bounds__(256) cc_compress_kernel(int *__restrict__ parent, int N)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int p = parent[i];
    if (p < 0 || p == i) return;
    int r = p, q = parent[r];
    while (q != r) {
        r = q;
        q = parent[r];
    }
    if (r != p) parent[i] = r;
}

__global__ void __launch_bounds__(256) cc_size_kernel(const int *__restrict__ parent, int *__restrict__ size, int N)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int s = size[i];
    if (s == 0) return;
    const int r = parent[i];
    if (r != i) atomicAdd(&size[r], s);               // a component root keeps its own tile count in place
}

__global__ void __launch_bounds__(256) cc_max_kernel(const uint8_t *__restrict__ lab, const uint8_t *__restrict__ group,
                                                     const int *__restrict__ parent, const int *__restrict__ size,
                                                     int *__restrict__ gmax, int N)
{
    __shared__ int m[NG];
    const int t = threadIdx.x;
    m[t] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + t;
    if (i < N && parent[i] == i) atomicMax(&m[group[lab[i]]], size[i]);
    __syncthreads();
    if (t > 0 && m[t]) atomicMax(&gmax[t], m[t]);
}

__global__ void __launch_bounds__(256) cc_write_kernel(const uint8_t *__restrict__ lab, const uint8_t *__restrict__ group,
                                                       const int *__restrict__ parent, const int *__restrict__ size,
                                                       const int *__restrict__ gmax, int *__restrict__ kept, uint8_t bg,
                                                       uint8_t *__restrict__ out, int N)
{
    __shared__ int h[NG];
    __shared__ uint8_t gtab[NG];
    const int t = threadIdx.x;
    h[t] = 0;
    gtab[t] = group[t];
    __syncthreads();
    const long long f0 = ((long long)blockIdx.x * 256 + t) * 4;
    if (f0 < N) {
        uint32_t w = 0, o = 0;
        const bool full = f0 + 4 <= N;
        if (full) w = *reinterpret_cast<const uint32_t *>(lab + f0);
        else for (int j = 0; f0 + j < N; ++j) w |= (uint32_t)lab[f0 + j] << (8 * j);
        for (int j = 0; j < 4 && f0 + j < N; ++j) {
            const uint32_t l = (w >> (8 * j)) & 255;
            const int g = gtab[l];
            uint32_t r = l;
            if (g) {
                if (size[parent[f0 + j]] < gmax[g]) r = bg;
                else atomicAdd(&h[g], 1);
            }
            o |= r << (8 * j);
        }
        if (full) *reinterpret_cast<uint32_t *>(out + f0) = o;
        else for (int j = 0; f0 + j < N; ++j) out[f0 + j] = (uint8_t)(o >> (8 * j));
    }
    __syncthreads();
    if (t > 0 && h[t]) atomicAdd(&kept[t], h[t]);
}

}  // namespace

extern "C" int mlagg_keep_largest_component(const unsigned char *labels, int X, int Y, int Z, const unsigned char *group,
                                            int background_label, int *parent, int *size, int *stats, unsigned char *out,
                                            void *stream)
{
    if (X < 1 || Y < 1 || Z < 1) return MLAGG_E_UNSUPPORTED;
    const long long N = (long long)X * Y * Z;
    if (N > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    if (!labels || !group || !parent || !size || !stats || !out) return MLAGG_E_NULLPTR;
    if (background_label < 0 || background_label > 255) return MLAGG_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(labels) & 3) || (reinterpret_cast<uintptr_t>(out) & 3)) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Vol v;
    v.lab = labels;
    v.group = group;
    v.X = X;
    v.Y = Y;
    v.Z = Z;
    v.ntx = (X + TX - 1) / TX;
    v.nty = (Y + TY - 1) / TY;
    v.ntz = (Z + TZ - 1) / TZ;
    v.vec = (Z % 4) == 0;
    const long long tiles = (long long)v.ntx * v.nty * v.ntz;
    const int n = (int)N;
    int *count = stats, *gmax = stats + NG, *kept = stats + 2 * NG;
    if (hipError_t e = hipMemsetAsync(stats, 0, 3 * NG * sizeof(int), st)) return (int)e;
    {
        MLAGG_TIMED(K_CC_LOCAL, st);
        hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)tiles), dim3(CC_BLOCK), 0, st, v, parent, size, count);
    }
    {
        MLAGG_TIMED(K_CC_MERGE, st);
        hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)tiles), dim3(CC_BLOCK), 0, st, v, parent);
    }
    const unsigned blocks = (unsigned)((N + 255) / 256);
    {
        MLAGG_TIMED(K_CC_COMPRESS, st);
        hipLaunchKernelGGL(cc_compress_kernel, dim3(blocks), dim3(256), 0, st, parent, n);
    }
    {
        MLAGG_TIMED(K_CC_SIZE, st);
        hipLaunchKernelGGL(cc_size_kernel, dim3(blocks), dim3(256), 0, st, parent, size, n);
    }
    {
        MLAGG_TIMED(K_CC_MAX, st);
        hipLaunchKernelGGL(cc_max_kernel, dim3(blocks), dim3(256), 0, st, labels, group, parent, size, gmax, n);
    }
    {
        MLAGG_TIMED(K_CC_WRITE, st);
        const unsigned wblocks = (unsigned)((N + 1023) / 1024);
        hipLaunchKernelGGL(cc_write_kernel, dim3(wblocks), dim3(256), 0, st, labels, group, parent, size, gmax, kept,
                           (uint8_t)background_label, out, n);
    }
    return (int)hipGetLastError();
}
