// 26-connected component labelling of (X, Y, Z) volumes, z contiguous, with the union-find of unionfind.h: the grid-level algorithm
// of K23 (components.hip) and K30 (cascade_aug.hip), defined once over a voxel source.
//
// A voxel source tells the class of a voxel, 0 meaning outside every mask; two voxels are connected when they are 26-neighbours
// with the same non-zero class.  It has two members, called only with x < X, y < Y, z < Z:
//   uint32_t classes4(int x, int y, int z)   the classes of (x, y, z..z+3), z a multiple of 4, as four bytes (voxel z + j in bits
//                                            [8 j, 8 j + 8)), 0 beyond Z;
//   uint32_t class1(int x, int y, int z)     the class of one voxel.
//
// Phases, one launch each with grid (tile_count(g), planes) and CC_BLOCK lanes, no inter-workgroup waiting inside a kernel; parent and
// size hold N int32 per plane:
//   label_tile      tile-local union-find in LDS over the 13 backward neighbours inside an 8 x 8 x 32 tile, four consecutive z voxels
//                   per lane; writes parent[v] = the global index of v's tile root (-1 outside the mask) and size[v] = the tile
//                   component's voxel count at its tile root (0 elsewhere);
//   merge_tiles     the voxels whose backward neighbours lie in another tile unite the two trees in the global parent array; a stale
//                   parent read from another XCD's L2 is always an ancestor in the same set, and a failed link returns the current
//                   value, so the loop converges;
//   then mlagg_uf::compress_kernel and mlagg_uf::size_kernel: every voxel points at its component's root, the component's minimum
//   linear index (its first voxel in raster order) whatever the schedule, and size[root] is the component's voxel count.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unionfind.h"

namespace mlagg_cc {

constexpr int TX = 8, TY = 8, TZ = 32;                 // tile; z is the contiguous axis
constexpr int TV = TX * TY * TZ;                       // 2048 voxels
constexpr int CC_BLOCK = 512;                          // 4 consecutive z voxels per lane

struct Geo {
    int X, Y, Z;
    int ntx, nty, ntz;                                 // tiles per axis
    long long N;
};

// false when the planes are outside the supported range: N <= 2^31 - 1 voxels (int32 parents), P <= 65535 planes (grid.y)
inline bool geometry(int P, int X, int Y, int Z, Geo &g)
{
    if (P < 1 || X < 1 || Y < 1 || Z < 1) return false;
    g.X = X;
    g.Y = Y;
    g.Z = Z;
    g.N = (long long)X * Y * Z;
    if (g.N > 2147483647LL || P > 65535) return false;
    g.ntx = (X + TX - 1) / TX;
    g.nty = (Y + TY - 1) / TY;
    g.ntz = (Z + TZ - 1) / TZ;
    return true;
}

inline unsigned tile_count(const Geo &g)
{
    return (unsigned)((long long)g.ntx * g.nty * g.ntz);
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

__device__ __forceinline__ void lane_coords(int t, int &lx, int &ly, int &lz)
{
    lz = (t & 7) * 4;
    ly = (t >> 3) & 7;
    lx = t >> 6;
}

__device__ __forceinline__ void tile_origin(const Geo &g, int b, int &x0, int &y0, int &z0)
{
    const int tz = b % g.ntz, r = b / g.ntz;
    x0 = (r / g.nty) * TX;
    y0 = (r % g.nty) * TY;
    z0 = tz * TZ;
}

// Returns the classes of the lane's four voxels (0 outside the volume), for what the caller counts besides.
template <typename Src>
__device__ __forceinline__ uint32_t label_tile(const Src &src, const Geo &g, int *__restrict__ parent, int *__restrict__ size)
{
    __shared__ int par[TV];
    __shared__ int cnt[TV];
    __shared__ uint8_t cls[TV];
    parent += blockIdx.y * g.N;
    size += blockIdx.y * g.N;
    int x0, y0, z0, lx, ly, lz;
    tile_origin(g, blockIdx.x, x0, y0, z0);
    lane_coords(threadIdx.x, lx, ly, lz);
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    const bool row = x < g.X && y < g.Y && z < g.Z;
    const uint32_t w = row ? src.classes4(x, y, z) : 0u;
    const int l0 = (lx * TY + ly) * TZ + lz;
    uint8_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = (uint8_t)(w >> (8 * j));
        cls[l0 + j] = c[j];
        par[l0 + j] = l0 + j;
        cnt[l0 + j] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!c[j]) continue;
        for (int i = 0; i < 13; ++i) {
            int dx, dy, dz;
            backward(i, dx, dy, dz);
            const int nx = lx + dx, ny = ly + dy, nz = lz + j + dz;
            if (nx < 0 || ny < 0 || ny >= TY || nz < 0 || nz >= TZ) continue;
            const int n = (nx * TY + ny) * TZ + nz;
            if (cls[n] == c[j]) mlagg_uf::lds_unite(par, l0 + j, n);
        }
    }
    __syncthreads();
    int root[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        root[j] = -1;
        if (c[j]) {
            root[j] = mlagg_uf::lds_find(par, l0 + j);
            atomicAdd(&cnt[root[j]], 1);
        }
    }
    __syncthreads();
    if (row) {
        const long long o = ((long long)x * g.Y + y) * g.Z + z;
        for (int j = 0; j < 4 && z + j < g.Z; ++j) {
            int p = -1, s = 0;
            if (c[j]) {
                const int r = root[j];
                const int rx = r / (TY * TZ), ry = (r / TZ) % TY, rz = r % TZ;
                p = (int)(((long long)(x0 + rx) * g.Y + (y0 + ry)) * g.Z + (z0 + rz));
                if (r == l0 + j) s = cnt[r];
            }
            parent[o + j] = p;
            size[o + j] = s;
        }
    }
    return w;
}

template <typename Src>
__device__ __forceinline__ void merge_tiles(const Src &src, const Geo &g, int *__restrict__ parent)
{
    parent += blockIdx.y * g.N;
    int x0, y0, z0, lx, ly, lz;
    tile_origin(g, blockIdx.x, x0, y0, z0);
    lane_coords(threadIdx.x, lx, ly, lz);
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    // only lanes on a tile face have backward neighbours in another tile
    const bool face = lx == 0 || ly == 0 || ly == TY - 1 || lz == 0 || lz + 4 == TZ;
    if (!face || x >= g.X || y >= g.Y || z >= g.Z) return;
    const uint32_t w = src.classes4(x, y, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {                      // a class is 0 beyond Z
        const int lzj = lz + j;
        if (!(lx == 0 || ly == 0 || ly == TY - 1 || lzj == 0 || lzj == TZ - 1)) continue;
        const uint32_t c = (w >> (8 * j)) & 255;
        if (!c) continue;
        const int me = (int)(((long long)x * g.Y + y) * g.Z + z + j);
        for (int i = 0; i < 13; ++i) {
            int dx, dy, dz;
            backward(i, dx, dy, dz);
            const int nlx = lx + dx, nly = ly + dy, nlz = lzj + dz;
            if (nlx >= 0 && nly >= 0 && nly < TY && nlz >= 0 && nlz < TZ) continue;      // same tile: done in label_tile
            const int nx = x + dx, ny = y + dy, nz = z + j + dz;
            if (nx < 0 || ny < 0 || ny >= g.Y || nz < 0 || nz >= g.Z) continue;
            if (src.class1(nx, ny, nz) == c) mlagg_uf::gunite(parent, me, (int)(((long long)nx * g.Y + ny) * g.Z + nz));
        }
    }
}

}  // namespace mlagg_cc
