// Union-find on the device, shared by the 3-D labelling of cc_label.h (K23 components.hip, K30 cascade_aug.hip) and the 2-D one of
// K27 (cells.hip): Playne-Hawick linking, atomicMin always links the larger root to the smaller one, so every set's root is its
// minimum index whatever the schedule.  The find / unite helpers, and the two kernels that finish a labelling once every link is made.
#pragma once
#include <hip/hip_runtime.h>

namespace mlagg_uf {

// LDS reads in the union loops are atomic loads, so that hipcc re-reads what other lanes' atomicMin changed
__device__ __forceinline__ int lds_find(int *par, int a)
{
    int p = __hip_atomic_load(par + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (p != a) {
        a = p;
        p = __hip_atomic_load(par + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return a;
}

__device__ inline void lds_unite(int *par, int a, int b)
{
    while (true) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&par[b], a);
        if (old == b) return;
        b = old;
    }
}

__device__ __forceinline__ int gfind(const int *par, int a)
{
    int p = __hip_atomic_load(par + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != a) {
        a = p;
        p = __hip_atomic_load(par + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return a;
}

__device__ inline void gunite(int *par, int a, int b)
{
    while (true) {
        a = gfind(par, a);
        b = gfind(par, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&par[b], a);
        if (old == b) return;
        b = old;
    }
}

// The kernels below work on grid.y planes of N elements each, 256 per workgroup along grid.x.

// parent[v] = find(v); -1 (outside the mask) stays
template <int UNUSED = 0>              // a template only so that the header can hold the definition
__global__ void __launch_bounds__(256) compress_kernel(int *__restrict__ parent, long long N)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    parent += blockIdx.y * N;
    const int p = parent[i];
    if (p < 0 || p == i) return;
    int r = p, q = parent[r];
    while (q != r) {
        r = q;
        q = parent[r];
    }
    if (r != p) parent[i] = r;
}

// size[] holds partial counts at the roots of the trees that were united (0 elsewhere); after compress_kernel each adds its count
// into its set's root: one global integer atomic per partial count, not one per element
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) size_kernel(const int *__restrict__ parent, int *__restrict__ size, long long N)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    parent += blockIdx.y * N;
    size += blockIdx.y * N;
    const int s = size[i];
    if (s == 0) return;
    const int r = parent[i];
    if (r != i) atomicAdd(&size[r], s);               // a set's root keeps its own count in place
}

}  // namespace mlagg_uf
