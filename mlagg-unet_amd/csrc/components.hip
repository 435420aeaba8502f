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
// Phases, one launch each, no inter-workgroup waiting inside a kernel.  The labelling is cc_label.h's, over a voxel source that
// reads one dword of four labels per lane and looks them up in the group table in LDS:
//   cc_local_kernel    mlagg_cc::label_tile (tile-local union-find: parent[v] = the global index of v's tile root, size[v] = the
//                      tile component's voxel count at its tile root), and the per-group voxel counts (LDS histogram, one global
//                      add per group and tile);
//   cc_merge_kernel    mlagg_cc::merge_tiles across the tile faces;
//   mlagg_uf::compress_kernel, mlagg_uf::size_kernel   every voxel points at its component's root, which holds the component's size;
//   cc_max_kernel      every component root takes the per-group maximum of the sizes (LDS maximum per workgroup, then one
//                      atomicMax per group into 256 slots);
//   cc_write_kernel    out[v] = background when group != 0 and the component is smaller than its group's maximum, label otherwise
//                      (ties at the maximum are all kept), plus the per-group kept counts.
// Every result is an integer and independent of the schedule: bit-identical to the host path.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cc_label.h"
#include "mlagg_hip.h"
#include "prof.h"

namespace {

using namespace mlagg_cc;

constexpr int NG = 256;                                // group slots

// K23's voxel source: a voxel's class is the group of its label
struct GroupSource {
    const uint8_t *lab;
    const uint8_t *gtab;                               // the group table in LDS
    int Y, Z;
    bool vec;                                          // Z % 4 == 0 and a 4-byte aligned base: dword label loads

    __device__ __forceinline__ uint32_t classes4(int x, int y, int z) const
    {
        const long long o = ((long long)x * Y + y) * Z + z;
        uint32_t w = 0, c = 0;
        if (vec && z + 4 <= Z) w = *reinterpret_cast<const uint32_t *>(lab + o);
        else for (int j = 0; j < 4 && z + j < Z; ++j) w |= (uint32_t)lab[o + j] << (8 * j);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (z + j < Z) c |= (uint32_t)gtab[(w >> (8 * j)) & 255] << (8 * j);
        return c;
    }

    __device__ __forceinline__ uint32_t class1(int x, int y, int z) const
    {
        return gtab[lab[((long long)x * Y + y) * Z + z]];
    }
};

__global__ void __launch_bounds__(CC_BLOCK) cc_local_kernel(const uint8_t *__restrict__ lab, const uint8_t *__restrict__ group, bool vec,
                                                             Geo g, int *__restrict__ parent, int *__restrict__ size,
                                                             int *__restrict__ count)
{
    __shared__ uint8_t gtab[NG];
    __shared__ int hist[NG];
    const int t = threadIdx.x;
    if (t < NG) {
        gtab[t] = group[t];
        hist[t] = 0;
    }
    __syncthreads();
    const uint32_t w = label_tile(GroupSource{lab, gtab, g.Y, g.Z, vec}, g, parent, size);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t c = (w >> (8 * j)) & 255;
        if (c) atomicAdd(&hist[c], 1);
    }
    __syncthreads();
    if (t < NG && t > 0 && hist[t]) atomicAdd(&count[t], hist[t]);
}

__global__ void __launch_bounds__(CC_BLOCK) cc_merge_kernel(const uint8_t *__restrict__ lab, const uint8_t *__restrict__ group, bool vec,
                                                             Geo g, int *__restrict__ parent)
{
    __shared__ uint8_t gtab[NG];
    if (threadIdx.x < NG) gtab[threadIdx.x] = group[threadIdx.x];
    __syncthreads();
    merge_tiles(GroupSource{lab, gtab, g.Y, g.Z, vec}, g, parent);
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
    Geo g;
    if (!geometry(1, X, Y, Z, g)) return MLAGG_E_UNSUPPORTED;
    if (!labels || !group || !parent || !size || !stats || !out) return MLAGG_E_NULLPTR;
    if (background_label < 0 || background_label > 255) return MLAGG_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(labels) & 3) || (reinterpret_cast<uintptr_t>(out) & 3)) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = (Z % 4) == 0;
    const long long N = g.N;
    const int n = (int)N;
    int *count = stats, *gmax = stats + NG, *kept = stats + 2 * NG;
    if (hipError_t e = hipMemsetAsync(stats, 0, 3 * NG * sizeof(int), st)) return (int)e;
    {
        MLAGG_TIMED(K_CC_LOCAL, st);
        hipLaunchKernelGGL(cc_local_kernel, dim3(tile_count(g)), dim3(CC_BLOCK), 0, st, labels, group, vec, g, parent, size, count);
    }
    {
        MLAGG_TIMED(K_CC_MERGE, st);
        hipLaunchKernelGGL(cc_merge_kernel, dim3(tile_count(g)), dim3(CC_BLOCK), 0, st, labels, group, vec, g, parent);
    }
    const unsigned blocks = (unsigned)((N + 255) / 256);
    {
        MLAGG_TIMED(K_CC_COMPRESS, st);
        hipLaunchKernelGGL(mlagg_uf::compress_kernel<>, dim3(blocks), dim3(256), 0, st, parent, N);
    }
    {
        MLAGG_TIMED(K_CC_SIZE, st);
        hipLaunchKernelGGL(mlagg_uf::size_kernel<>, dim3(blocks), dim3(256), 0, st, parent, size, N);
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
