// K36 -- the tail of the training / validation transform chain, one pass from the augmented (data, seg) to what the loss consumes.
//
// Replaces, per batch, the last four transforms of nnUNetTrainer.get_training_transforms (reference nnUNetTrainer.py:697-731; :742-757
// for validation, which has no mask):
//   MaskTransform                          (custom_transforms/masking.py:18-22)            data[:, c][seg[:, 0] < 0] = 0 for the listed c
//   RemoveLabelTransform(-1, 0)                                                            w = v < 0 ? 0 : v
//   ConvertSegmentationToRegionsTransform  (custom_transforms/region_based_training.py:23-38)  plane r = isin(w, regions[r]), the
//                                                                                          ignore label as one more "region"
//   DownsampleSegForDSTransform2, order 0                                                  one nearest-neighbour map per level
// The per-voxel maps commute with the nearest-neighbour gather, so every level reads the LABEL of its source voxel once and writes all
// its planes: no (B, R, *S) intermediate, no per-level torch.where / interpolate launches.
//
// Schedule: the grid is the concatenation of the levels' output index spaces.  A work item is a quad, four consecutive output voxels of
// one row (the contiguous axis) of one level; a workgroup's 256 items belong to one level (the level is found from blockIdx.x alone, so a
// wave never diverges over it).  Where the source index along the row is the identity (level 0, and any level that keeps that axis)
// the four labels are one 16-byte (fp32) or 8-byte (int16) load; the planes leave as 16-byte stores where the level's row length is a
// multiple of four and its base is aligned, as scalar stores otherwise (the last quad of a row is then partial).  The gathered levels
// read their source indices from small int32 tables built on the host (dataloading.nearest_index): the index rule is not restated here.
// Level-0 quads also write the mask: zeros are stored to data where the raw label is negative, nothing of data is read.
// 64-bit offsets throughout; no atomics, no LDS.  HBM-bound: 4 (or 2) bytes read and 4 R' bytes written per level-0 voxel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlagg_hip.h"
#include "prof.h"

namespace {

constexpr int TPB = 256;
constexpr int QUAD = 4;
constexpr unsigned F_VEC_STORE = 1u;      // level: 16-byte plane stores
constexpr unsigned F_VEC_SOURCE = 2u;     // level: the four labels of a quad are one vector load
constexpr unsigned F_VEC_MASK = 1u;       // batch: 16-byte zero stores to data

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short i16x4 __attribute__((ext_vector_type(4)));

struct TailLevel {
    const int *tab[3];                    // source index per output index along (z, y, x); NULL: the identity
    float *out;
    long long items;                      // B * size[0] * size[1] * quads
    int size[3];                          // 2-D: size[0] == 1
    int quads;                            // ceil(size[2] / 4)
    unsigned first_block;
    unsigned flags;
};

struct TailParams {
    TailLevel lev[MLAGG_TAIL_MAX_LEVELS];
    float *data;
    const void *seg;
    const uint32_t *member;
    unsigned long long mask_bits;         // bit c: channel c of data is masked
    int B, C, Sc, L, R, planes, ignore;
    int size[3];
    unsigned flags;
};

__device__ __forceinline__ int source_index(const int *tab, int i, int n)
{
    return tab ? min(max(tab[i], 0), n - 1) : i;
}

__device__ __forceinline__ void load_quad(const float *p, float (&v)[QUAD])
{
    const f32x4 t = *reinterpret_cast<const f32x4 *>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

__device__ __forceinline__ void load_quad(const short *p, float (&v)[QUAD])
{
    const i16x4 t = *reinterpret_cast<const i16x4 *>(p);
    v[0] = (float)t.x; v[1] = (float)t.y; v[2] = (float)t.z; v[3] = (float)t.w;
}

// n <= 4 values of a quad; vec: n == 4 and p is 16-byte aligned
__device__ __forceinline__ void store_quad(float *p, const float (&v)[QUAD], int n, bool vec)
{
    if (vec) {
        f32x4 t;
        t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
        *reinterpret_cast<f32x4 *>(p) = t;
    } else {
#pragma unroll
        for (int j = 0; j < QUAD; ++j)
            if (j < n) p[j] = v[j];
    }
}

// np.isin(w, regions[r]) for every r: only an integer label in 0 .. 255 can belong to a region
__device__ __forceinline__ uint32_t member_bits(const uint32_t *__restrict__ member, float w)
{
    if (!(w >= 0.f && w < 256.f)) return 0u;
    const int i = (int)w;
    return (float)i == w ? member[i] : 0u;
}

template <typename SegT, bool REGIONS>
__global__ void __launch_bounds__(TPB)
batch_tail_kernel(const TailParams p)
{
    int l = 0;
#pragma unroll
    for (int i = 1; i < MLAGG_TAIL_MAX_LEVELS; ++i)
        if (i < p.L && blockIdx.x >= p.lev[i].first_block) l = i;
    const TailLevel &lv = p.lev[l];
    const long long item = (long long)(blockIdx.x - lv.first_block) * TPB + threadIdx.x;
    if (item >= lv.items) return;

    const int Dl = lv.size[0], Hl = lv.size[1], Wl = lv.size[2];
    const int D = p.size[0], H = p.size[1], W = p.size[2];
    const int q = (int)(item % lv.quads);
    long long row = item / lv.quads;
    const int y = (int)(row % Hl);
    row /= Hl;
    const int z = (int)(row % Dl);
    const int b = (int)(row / Dl);
    const int x0 = QUAD * q;
    const int n = min(QUAD, Wl - x0);

    // the labels of the quad's source voxels (channel 0 of seg)
    const int zs = source_index(lv.tab[0], z, D), ys = source_index(lv.tab[1], y, H);
    const SegT *srow = static_cast<const SegT *>(p.seg) + ((((long long)b * p.Sc) * D + zs) * H + ys) * W;
    float v[QUAD];
    if (lv.flags & F_VEC_SOURCE) {
        load_quad(srow + x0, v);
    } else {
#pragma unroll
        for (int j = 0; j < QUAD; ++j) v[j] = j < n ? (float)srow[source_index(lv.tab[2], x0 + j, W)] : 0.f;
    }

    // MaskTransform: level 0 is the identity here (checked by the launcher), so the quad's voxels are its own sources
    if (l == 0 && p.mask_bits) {
        bool any = false, all = n == QUAD;
#pragma unroll
        for (int j = 0; j < QUAD; ++j) {
            const bool neg = j < n && v[j] < 0.f;
            any |= neg;
            all &= neg;
        }
        if (any) {
            const long long plane = (long long)D * H * W;
            float *d0 = p.data + (long long)b * p.C * plane + ((long long)z * H + y) * W + x0;
            const float zero[QUAD] = {0.f, 0.f, 0.f, 0.f};
            for (unsigned long long bits = p.mask_bits; bits; bits &= bits - 1) {
                float *d = d0 + (long long)(__ffsll(bits) - 1) * plane;
                if (all && (p.flags & F_VEC_MASK)) {
                    store_quad(d, zero, QUAD, true);
                } else {
#pragma unroll
                    for (int j = 0; j < QUAD; ++j)
                        if (j < n && v[j] < 0.f) d[j] = 0.f;
                }
            }
        }
    }

    // RemoveLabelTransform
    float w[QUAD];
#pragma unroll
    for (int j = 0; j < QUAD; ++j) w[j] = v[j] < 0.f ? 0.f : v[j];

    const long long lplane = (long long)Dl * Hl * Wl;
    float *o = lv.out + (long long)b * p.planes * lplane + ((long long)z * Hl + y) * Wl + x0;
    const bool vec = (lv.flags & F_VEC_STORE) != 0;
    if (!REGIONS) {
        store_quad(o, w, n, vec);
        return;
    }
    uint32_t bits[QUAD];
#pragma unroll
    for (int j = 0; j < QUAD; ++j) bits[j] = j < n ? member_bits(p.member, w[j]) : 0u;
    float t[QUAD];
    for (int r = 0; r < p.R; ++r) {
#pragma unroll
        for (int j = 0; j < QUAD; ++j) t[j] = (float)(bits[j] >> r & 1u);
        store_quad(o + (long long)r * lplane, t, n, vec);
    }
    if (p.ignore >= 0) {
        const float ign = (float)p.ignore;
#pragma unroll
        for (int j = 0; j < QUAD; ++j) t[j] = w[j] == ign ? 1.f : 0.f;
        store_quad(o + (long long)p.R * lplane, t, n, vec);
    }
}

bool aligned(const void *ptr, size_t bytes) { return reinterpret_cast<uintptr_t>(ptr) % bytes == 0; }

}  // namespace

extern "C" int mlagg_batch_tail(float *data, int B, int C, const void *seg, int seg_kind, int Sc, int nd, const int *sizes,
                                const int *mask_channels, int n_mask, int L, const int *level_sizes, const void *const *tables,
                                void *const *out, const unsigned int *member, int R, int ignore_label, void *stream)
{
    if (!seg || !sizes || !level_sizes || !tables || !out || (n_mask > 0 && (!data || !mask_channels))) return MLAGG_E_NULLPTR;
    if (B < 1 || C < 1 || Sc < 1 || (nd != 2 && nd != 3) || L < 1 || L > MLAGG_TAIL_MAX_LEVELS || n_mask < 0 || ignore_label < -1 ||
        (seg_kind != MLAGG_TAIL_SEG_F32 && seg_kind != MLAGG_TAIL_SEG_INT16) || (member && (R < 1 || R > MLAGG_TAIL_MAX_REGIONS)))
        return MLAGG_E_UNSUPPORTED;
    TailParams p = {};
    p.data = data;
    p.seg = seg;
    p.member = member;
    p.B = B; p.C = C; p.Sc = Sc; p.L = L;
    p.R = member ? R : 0;
    p.ignore = member ? ignore_label : -1;
    p.planes = member ? R + (ignore_label >= 0 ? 1 : 0) : 1;
    p.size[0] = 1;
    for (int a = 0; a < nd; ++a) {
        if (sizes[a] < 1) return MLAGG_E_UNSUPPORTED;
        p.size[3 - nd + a] = sizes[a];
    }
    for (int i = 0; i < n_mask; ++i) {
        if (mask_channels[i] < 0 || mask_channels[i] >= C || mask_channels[i] >= 64) return MLAGG_E_UNSUPPORTED;
        p.mask_bits |= 1ull << mask_channels[i];
    }
    const int W = p.size[2];
    if (W % QUAD == 0 && data && aligned(data, 16)) p.flags |= F_VEC_MASK;
    const size_t seg_vec_bytes = seg_kind == MLAGG_TAIL_SEG_F32 ? 16 : 8;
    long long blocks = 0;
    for (int l = 0; l < L; ++l) {
        TailLevel &lv = p.lev[l];
        if (!out[l]) return MLAGG_E_NULLPTR;
        lv.out = static_cast<float *>(out[l]);
        lv.size[0] = 1;
        for (int a = 0; a < nd; ++a) {
            const int s = level_sizes[l * nd + a];
            const int *tab = static_cast<const int *>(tables[l * nd + a]);
            if (s < 1 || (!tab && s != sizes[a])) return MLAGG_E_UNSUPPORTED;
            if (l == 0 && tab && p.mask_bits) return MLAGG_E_UNSUPPORTED;     // the mask is written by level 0 as the identity
            lv.size[3 - nd + a] = s;
            lv.tab[3 - nd + a] = tab;
        }
        lv.quads = (lv.size[2] + QUAD - 1) / QUAD;
        lv.items = (long long)B * lv.size[0] * lv.size[1] * lv.quads;
        if (lv.size[2] % QUAD == 0 && aligned(lv.out, 16)) lv.flags |= F_VEC_STORE;
        if (!lv.tab[2] && W % QUAD == 0 && aligned(seg, seg_vec_bytes)) lv.flags |= F_VEC_SOURCE;
        lv.first_block = (unsigned)blocks;
        blocks += (lv.items + TPB - 1) / TPB;
        if (blocks > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_BATCH_TAIL, st);
    const dim3 grid((unsigned)blocks), block(TPB);
    if (seg_kind == MLAGG_TAIL_SEG_F32) {
        if (member) hipLaunchKernelGGL((batch_tail_kernel<float, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((batch_tail_kernel<float, false>), grid, block, 0, st, p);
    } else {
        if (member) hipLaunchKernelGGL((batch_tail_kernel<short, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((batch_tail_kernel<short, false>), grid, block, 0, st, p);
    }
    return (int)hipGetLastError();
}
