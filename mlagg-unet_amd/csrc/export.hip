// K21 -- prediction export on the device: order-1 resampling of the logits back to the cropped original shape, and the fused export
// (resample, softmax, argmax, paste into the uncropped volume, transpose back) that writes uint8 labels and, optionally, probabilities.
//
// What it replaces: the reference's export_prediction_from_softmax (nnunetv2/inference/export_prediction.py:10-69), which copies the
// logits to the host and, in float64 on the CPU with one Python call per channel (and per slice on anisotropic data),
//   resamples them with resample_data_or_seg_to_shape(is_seg=False, order=1, order_z=0)
//            (preprocessing/resampling/default_resampling.py:76-200: skimage resize = ndi.zoom(order=1, mode='nearest',
//            grid_mode=True) and, for separate z, map_coordinates(order=0, mode='nearest') along the low-resolution axis),
//   applies softmax and argmax (utilities/label_handling/label_handling.py:128-182),
//   pastes the labels (and the probabilities, :184-201) into shape_before_cropping at bbox_used_for_cropping,
//   and transposes them by transpose_backward.
//   resample_linear_kernel   the resampling alone: (C, X, Y, Z) -> (C, X', Y', Z') fp32 (export.resample_logits_to_shape, and the
//                            first step of the export for more than 32 classes);
//   export_kernel<KB>        everything at once for K <= KB classes, without materialising the resampled logits.  REGIONS: the
//                            heads of a region-based label manager -- fp32 sigmoid per head instead of the softmax, and the label
//                            painted in regions_class_order (label 0, then order[i] wherever sigmoid_i > 0.5 for i = 0 .. K-1: the
//                            last match wins, label_handling.py:166-173) instead of the argmax.
//
// The coordinates are not computed here: the host builds one table per output axis in float64 with the reference's expressions
// (export._axis_taps) -- two source indices and their two weights -- and the kernels only gather and blend.  An order-0 or unchanged
// axis has the entry (i, i, 1, 0).  The blend is separable in a fixed order, in fp64, rounded once to fp32: along z for each of the
// four (x, y) taps, then along y, then along x; the host path (export._resample_host) runs the same products and sums in torch
// float64, so both give the same fp32 logits bit for bit, and the reference's float64 result to within its summation order.
// `#pragma clang fp contract(off)` keeps hipcc from fusing the products into FMAs.  The logits may have any strides (the 2-D sliding
// window returns a view); all volume offsets are 64-bit; no atomics, so every result is bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mlagg_hip.h"
#include "prof.h"

namespace {

constexpr int EX_BLOCK = 256;
constexpr int EX_VEC = 4;              // consecutive output elements per lane: one dwordx4 (resample) or one packed dword (labels)

struct Src {
    const float *p;
    long long sc, sx, sy, sz;          // element strides of the logits
};

struct Taps {
    const int *idx;                    // (X' + Y' + Z', 2): x entries, then y, then z
    const double *w;                   // (X' + Y' + Z', 2)
    int yoff, zoff;                    // X', X' + Y'
};

// one output voxel (ox, oy, oz) of channel base `c`; ix/iy/iz and wx/wy/wz are the table entries of its three coordinates
__device__ __forceinline__ float interp(const float *__restrict__ c, long long sx, long long sy, long long sz, int2 ix, int2 iy, int2 iz,
                                        double2 wx, double2 wy, double2 wz)
{
#pragma clang fp contract(off)
    const long long z0 = iz.x * sz, z1 = iz.y * sz;
    double rx[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const float *px = c + (long long)(a ? ix.y : ix.x) * sx;
        double ry[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float *p = px + (long long)(b ? iy.y : iy.x) * sy;
            const double v0 = p[z0], v1 = p[z1];
            ry[b] = v0 * wz.x + v1 * wz.y;
        }
        rx[a] = ry[0] * wy.x + ry[1] * wy.y;
    }
    return (float)(rx[0] * wx.x + rx[1] * wx.y);
}

__device__ __forceinline__ int2 tap_idx(const Taps &t, int e) { return reinterpret_cast<const int2 *>(t.idx)[e]; }
__device__ __forceinline__ double2 tap_w(const Taps &t, int e) { return reinterpret_cast<const double2 *>(t.w)[e]; }

// flat output element f = 4 * lane + j of (C, X', Y', Z')
__global__ void __launch_bounds__(EX_BLOCK) resample_linear_kernel(Src s, Taps t, float *__restrict__ out, int Xo, int Yo, int Zo,
                                                                   long long M)
{
    const long long f0 = ((long long)blockIdx.x * EX_BLOCK + threadIdx.x) * EX_VEC;
    if (f0 >= M) return;
    long long r = f0 / Zo;
    int z = (int)(f0 - r * Zo);
    int y = (int)(r % Yo);
    r /= Yo;
    int x = (int)(r % Xo);
    int c = (int)(r / Xo);
    float v[EX_VEC];
#pragma unroll
    for (int j = 0; j < EX_VEC; ++j) {
        v[j] = 0.f;
        if (f0 + j < M) {
            v[j] = interp(s.p + (long long)c * s.sc, s.sx, s.sy, s.sz, tap_idx(t, x), tap_idx(t, t.yoff + y), tap_idx(t, t.zoff + z),
                          tap_w(t, x), tap_w(t, t.yoff + y), tap_w(t, t.zoff + z));
        }
        if (++z == Zo) {
            z = 0;
            if (++y == Yo) {
                y = 0;
                if (++x == Xo) {
                    x = 0;
                    ++c;
                }
            }
        }
    }
    if (f0 + EX_VEC <= M) {
        *reinterpret_cast<float4 *>(out + f0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < EX_VEC && f0 + j < M; ++j) out[f0 + j] = v[j];
    }
}

struct Geometry {
    int lo[3];                         // bbox lower corner, pre-transpose axis order
    int ext[3];                        // bbox extent = the resampled shape (X', Y', Z')
    int inv[3];                        // inv[d]: the output axis that holds pre-transpose axis d
    int Q[3];                          // output (transposed, uncropped) shape
};

__device__ __forceinline__ int pick(int q0, int q1, int q2, int i) { return i == 0 ? q0 : (i == 1 ? q1 : q2); }

struct Order {
    uint8_t label[32];                 // regions_class_order: the label head i paints (REGIONS only)
};

// flat output voxel f = 4 * lane + j of the transposed, uncropped volume Q; KB >= K logits live in registers
template <int KB, bool REGIONS>
__global__ void __launch_bounds__(EX_BLOCK) export_kernel(Src s, Taps t, Geometry g, Order order, int K, uint8_t *__restrict__ labels,
                                                          float *__restrict__ probs, long long N)
{
#pragma clang fp contract(off)
    const long long f0 = ((long long)blockIdx.x * EX_BLOCK + threadIdx.x) * EX_VEC;
    if (f0 >= N) return;
    long long r = f0 / g.Q[2];
    int q2 = (int)(f0 - r * g.Q[2]);
    int q1 = (int)(r % g.Q[1]);
    int q0 = (int)(r / g.Q[1]);
    uint32_t packed = 0;
    for (int j = 0; j < EX_VEC && f0 + j < N; ++j) {
        const long long f = f0 + j;
        const int ox = pick(q0, q1, q2, g.inv[0]) - g.lo[0];
        const int oy = pick(q0, q1, q2, g.inv[1]) - g.lo[1];
        const int oz = pick(q0, q1, q2, g.inv[2]) - g.lo[2];
        if ((unsigned)ox < (unsigned)g.ext[0] && (unsigned)oy < (unsigned)g.ext[1] && (unsigned)oz < (unsigned)g.ext[2]) {
            const int2 ix = tap_idx(t, ox), iy = tap_idx(t, t.yoff + oy), iz = tap_idx(t, t.zoff + oz);
            const double2 wx = tap_w(t, ox), wy = tap_w(t, t.yoff + oy), wz = tap_w(t, t.zoff + oz);
            if constexpr (REGIONS) {
                // torch.sigmoid per head in fp32 (label_handling.py:46-47, 128-144); a logit of exactly 0 gives 0.5, which does not fire
                uint32_t lab = 0;
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    if (k < K) {
                        const float z = interp(s.p + (long long)k * s.sc, s.sx, s.sy, s.sz, ix, iy, iz, wx, wy, wz);
                        const float p = 1.f / (1.f + expf(-z));
                        lab = p > 0.5f ? (uint32_t)order.label[k] : lab;
                        if (probs) probs[(long long)k * N + f] = p;
                    }
                }
                packed |= lab << (8 * j);
            } else {
                float l[KB];
                float m = -INFINITY;
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    if (k < K) {
                        l[k] = interp(s.p + (long long)k * s.sc, s.sx, s.sy, s.sz, ix, iy, iz, wx, wy, wz);
                        m = fmaxf(m, l[k]);
                    }
                }
                // softmax over the classes in fp32 (torch.softmax(x, 0) of label_handling.py:128-144), then the first maximum of the
                // probabilities (numpy's argmax(0), :172)
                float sum = 0.f;
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    if (k < K) {
                        l[k] = expf(l[k] - m);
                        sum = sum + l[k];
                    }
                }
                float best = 0.f;
                int arg = 0;
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    if (k < K) {
                        l[k] = l[k] / sum;
                        if (k == 0 || l[k] > best) {
                            best = l[k];
                            arg = k;
                        }
                        if (probs) probs[(long long)k * N + f] = l[k];
                    }
                }
                packed |= (uint32_t)arg << (8 * j);
            }
        } else if (probs) {
            for (int k = 0; k < K; ++k) probs[(long long)k * N + f] = 0.f;          // revert_cropping: zeros in every channel
        }
        if (++q2 == g.Q[2]) {
            q2 = 0;
            if (++q1 == g.Q[1]) {
                q1 = 0;
                ++q0;
            }
        }
    }
    if (f0 + EX_VEC <= N) {
        *reinterpret_cast<uint32_t *>(labels + f0) = packed;
    } else {
        for (int j = 0; f0 + j < N; ++j) labels[f0 + j] = (uint8_t)(packed >> (8 * j));
    }
}

template <int KB, bool REGIONS>
void launch_export(dim3 grid, hipStream_t st, const Src &s, const Taps &t, const Geometry &g, const Order &order, int K, uint8_t *labels,
                   float *probs, long long N)
{
    hipLaunchKernelGGL((export_kernel<KB, REGIONS>), grid, dim3(EX_BLOCK), 0, st, s, t, g, order, K, labels, probs, N);
}

int check_source(const float *in, int C, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz, const int *idx,
                 const double *w)
{
    if (!in || !idx || !w) return MLAGG_E_NULLPTR;
    if (C < 1 || X < 1 || Y < 1 || Z < 1 || sc < 0 || sx < 0 || sy < 0 || sz < 0) return MLAGG_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(idx) & 7) || (reinterpret_cast<uintptr_t>(w) & 15)) return MLAGG_E_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int mlagg_resample_linear(const float *in, int C, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz,
                                     const int *tap_idx, const double *tap_w, float *out, int Xo, int Yo, int Zo, void *stream)
{
    if (int rc = check_source(in, C, X, Y, Z, sc, sx, sy, sz, tap_idx, tap_w)) return rc;
    if (!out) return MLAGG_E_NULLPTR;
    if (Xo < 1 || Yo < 1 || Zo < 1 || (reinterpret_cast<uintptr_t>(out) & 15)) return MLAGG_E_UNSUPPORTED;
    const long long M = (long long)C * Xo * Yo * Zo;
    const long long blocks = (M + (long long)EX_BLOCK * EX_VEC - 1) / ((long long)EX_BLOCK * EX_VEC);
    if (blocks > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_RESAMPLE_LINEAR, st);
    const Src s{in, sc, sx, sy, sz};
    const Taps t{tap_idx, tap_w, Xo, Xo + Yo};
    hipLaunchKernelGGL(resample_linear_kernel, dim3((unsigned)blocks), dim3(EX_BLOCK), 0, st, s, t, out, Xo, Yo, Zo, M);
    return (int)hipGetLastError();
}

namespace {

// regions_class_order == NULL: softmax + argmax; else K labels in 0..255, sigmoid + painting
int export_any(const float *logits, int K, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz,
               const int *tap_idx, const double *tap_w, int Xc, int Yc, int Zc, const int *box_lo, const int *shape, const int *perm,
               const int *regions_class_order, unsigned char *labels, float *probs, void *stream)
{
    if (int rc = check_source(logits, K, X, Y, Z, sc, sx, sy, sz, tap_idx, tap_w)) return rc;
    if (!box_lo || !shape || !perm || !labels) return MLAGG_E_NULLPTR;
    if (K > 32 || Xc < 1 || Yc < 1 || Zc < 1 || (reinterpret_cast<uintptr_t>(labels) & 3)) return MLAGG_E_UNSUPPORTED;
    Geometry g;
    const int ext[3] = {Xc, Yc, Zc};
    int seen = 0;
    for (int d = 0; d < 3; ++d) {
        if (shape[d] < 1 || box_lo[d] < 0 || box_lo[d] + ext[d] > shape[d]) return MLAGG_E_UNSUPPORTED;
        if (perm[d] < 0 || perm[d] > 2 || (seen & (1 << perm[d]))) return MLAGG_E_UNSUPPORTED;
        seen |= 1 << perm[d];
        g.lo[d] = box_lo[d];
        g.ext[d] = ext[d];
    }
    for (int i = 0; i < 3; ++i) {
        g.Q[i] = shape[perm[i]];
        g.inv[perm[i]] = i;
    }
    const long long N = (long long)shape[0] * shape[1] * shape[2];
    const long long blocks = (N + (long long)EX_BLOCK * EX_VEC - 1) / ((long long)EX_BLOCK * EX_VEC);
    if (blocks > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_EXPORT_SEG, st);
    const Src s{logits, sc, sx, sy, sz};
    const Taps t{tap_idx, tap_w, Xc, Xc + Yc};
    const dim3 grid((unsigned)blocks);
    uint8_t *lab = reinterpret_cast<uint8_t *>(labels);
    Order order{};
    if (regions_class_order) {
        for (int k = 0; k < K; ++k) {
            if (regions_class_order[k] < 0 || regions_class_order[k] > 255) return MLAGG_E_UNSUPPORTED;
            order.label[k] = (uint8_t)regions_class_order[k];
        }
        if (K <= 4) launch_export<4, true>(grid, st, s, t, g, order, K, lab, probs, N);
        else if (K <= 8) launch_export<8, true>(grid, st, s, t, g, order, K, lab, probs, N);
        else if (K <= 16) launch_export<16, true>(grid, st, s, t, g, order, K, lab, probs, N);
        else launch_export<32, true>(grid, st, s, t, g, order, K, lab, probs, N);
    } else {
        if (K <= 4) launch_export<4, false>(grid, st, s, t, g, order, K, lab, probs, N);
        else if (K <= 8) launch_export<8, false>(grid, st, s, t, g, order, K, lab, probs, N);
        else if (K <= 16) launch_export<16, false>(grid, st, s, t, g, order, K, lab, probs, N);
        else launch_export<32, false>(grid, st, s, t, g, order, K, lab, probs, N);
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int mlagg_export_segmentation(const float *logits, int K, int X, int Y, int Z, long long sc, long long sx, long long sy,
                                         long long sz, const int *tap_idx, const double *tap_w, int Xc, int Yc, int Zc,
                                         const int *box_lo, const int *shape, const int *perm, unsigned char *labels, float *probs,
                                         void *stream)
{
    return export_any(logits, K, X, Y, Z, sc, sx, sy, sz, tap_idx, tap_w, Xc, Yc, Zc, box_lo, shape, perm, nullptr, labels, probs, stream);
}

extern "C" int mlagg_export_segmentation_regions(const float *logits, int K, int X, int Y, int Z, long long sc, long long sx, long long sy,
                                                 long long sz, const int *tap_idx, const double *tap_w, int Xc, int Yc, int Zc,
                                                 const int *box_lo, const int *shape, const int *perm, const int *regions_class_order,
                                                 unsigned char *labels, float *probs, void *stream)
{
    if (!regions_class_order) return MLAGG_E_NULLPTR;
    return export_any(logits, K, X, Y, Z, sc, sx, sy, sz, tap_idx, tap_w, Xc, Yc, Zc, box_lo, shape, perm, regions_class_order, labels,
                      probs, stream);
}
