// Union-find device helpers shared by K23 (components.hip) and K27 (cells.hip): Playne-Hawick linking, atomicMin always links the
// larger root to the smaller one, so every set's root is its minimum index whatever the schedule.
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

}  // namespace mlagg_uf
