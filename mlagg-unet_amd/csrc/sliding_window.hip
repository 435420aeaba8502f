// K20 -- 3-D sliding-window inference: tile gather with mirror variants, Gaussian fold, finalize (+ argmax).
// K32 -- the same gather for a cascaded stage: the one-hot channels of the previous stage's label map are written next to the
//        image channels of every tile, from the label map itself (no one-hot volume).
//
// What it replaces: the per-tile tensor traffic of the reference's predict_sliding_window_return_logits for 3-D tiles
// (nnunetv2/inference/sliding_window_prediction.py:60-210):
//   gather   `data[sl][None]` (:193) and the flipped input copies of maybe_mirror_and_predict (:87-115), for a whole chunk of tiles
//            and every mirror variant in one launch;
//   fold     the flipped output copies and their sum (:97-114), `/= num_predictons` (:115), `* gaussian` and the accumulation into
//            predicted_logits / n_predictions (:200-201), one launch per tile so the overlapping tiles accumulate in tile order;
//   finalize `predicted_logits /= n_predictions` (:203) and the crop of the padding (:206), into a contiguous tensor, optionally
//            with the argmax labels of the segmentation.
//   gather_onehot  the gather on `np.vstack((data, seg_onehot))` of the cascade's second stage (predict_from_raw_data.py:57-60,
//            convert_labelmap_to_one_hot label_handling.py:266-270, nnUNetTrainer.py:1099-1101) without that stack: a tile's image
//            rows are copied as in gather, and one block per (variant, tile, x, y) row of the LABEL MAP reads its Z run once and
//            writes the L rows `label == labels[i]` of the one-hot channels.
//
// Layouts (fp32, Z the contiguous axis everywhere):
//   volume (C, X, Y, Z) padded input; chunk input / output (V * n, C|K, tx, ty, tz), variant-major then tile;
//   acc (K, X, Y, Z), w (X, Y, Z) accumulators; logits (K, X0, Y0, Z0) cropped; labels (X0, Y0, Z0) int64.
// A variant is a bitmask of flipped tile axes (bit a: axis a).  Flipping reads a Z run in reverse: the same 128-byte lines as
// the forward run, so every access below is coalesced.  One wave per (x, y) row of a tile walks its Z run; offsets are 64-bit.
// Arithmetic is the reference's order with fp32 accumulators and no contracted FMA: the result is bit-identical to the same torch
// composition on the device and independent of the chunking.  `#pragma clang fp contract(off)` in the kernel bodies, not
// __fadd_rn / __fmul_rn: the HIP headers define those as plain `x * y` / `x + y`, which hipcc's default -ffp-contract=fast fused
// into v_fmac_f32 once inlined.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mlagg_hip.h"
#include "prof.h"

namespace {

constexpr int SW_WAVE = 64;
constexpr int SW_MAX_V = 8;
constexpr int SW_MAX_TILES = 64;       // tiles per gather launch (the entry splits larger chunks)

struct GatherArgs {
    int ox[SW_MAX_TILES], oy[SW_MAX_TILES], oz[SW_MAX_TILES];
    int flips[SW_MAX_V];
};

// one block per output row (b, c, x, y): b = v * nsub + i over the variants and the nsub tiles of this launch
__global__ void __launch_bounds__(SW_WAVE) sw_gather_kernel(const float *__restrict__ vol, float *__restrict__ out, GatherArgs a,
                                                            int C, int X, int Y, int Z, int tx, int ty, int tz, int n, int i0, int nsub)
{
    int r = blockIdx.x;
    const int y = r % ty;
    r /= ty;
    const int x = r % tx;
    r /= tx;
    const int c = r % C;
    const int b = r / C;
    const int v = b / nsub, i = b % nsub;
    const int m = a.flips[v];
    const int sx = a.ox[i] + ((m & 1) ? tx - 1 - x : x);
    const int sy = a.oy[i] + ((m & 2) ? ty - 1 - y : y);
    const float *src = vol + (((size_t)c * X + sx) * Y + sy) * (size_t)Z + a.oz[i];
    float *dst = out + ((((size_t)v * n + i0 + i) * C + c) * tx + x) * (size_t)ty * tz + (size_t)y * tz;
    if (m & 4) {
        for (int z = threadIdx.x; z < tz; z += SW_WAVE) dst[z] = src[tz - 1 - z];
    } else {
        for (int z = threadIdx.x; z < tz; z += SW_WAVE) dst[z] = src[z];
    }
}

struct OneHotArgs {
    unsigned char labels[MLAGG_CASCADE_MAX_LABELS];
};

// one block per row (b, c, x, y) with c in 0 .. C: c < C is sw_gather_kernel's copy of image channel c into a (C + L)-channel tile;
// c == C owns the same row of the label map (S: int8, uint8 or int16, any byte alignment: one element per lane) and writes the
// rows of output channels C .. C + L - 1, so every label is read once for its L outputs.  Coalesced 256-byte stores per channel row.
template <typename S>
__global__ void __launch_bounds__(SW_WAVE) sw_gather_onehot_kernel(const float *__restrict__ vol, const S *__restrict__ seg,
                                                                   float *__restrict__ out, GatherArgs a, OneHotArgs h, int C, int L,
                                                                   int X, int Y, int Z, int tx, int ty, int tz, int n, int i0,
                                                                   int nsub)
{
    int r = blockIdx.x;
    const int y = r % ty;
    r /= ty;
    const int x = r % tx;
    r /= tx;
    const int c = r % (C + 1);
    const int b = r / (C + 1);
    const int v = b / nsub, i = b % nsub;
    const int m = a.flips[v];
    const int sx = a.ox[i] + ((m & 1) ? tx - 1 - x : x);
    const int sy = a.oy[i] + ((m & 2) ? ty - 1 - y : y);
    const size_t T = (size_t)tx * ty * tz;
    float *dst = out + (((size_t)v * n + i0 + i) * (C + L) + c) * T + ((size_t)x * ty + y) * tz;
    if (c < C) {
        const float *src = vol + (((size_t)c * X + sx) * Y + sy) * (size_t)Z + a.oz[i];
        if (m & 4) {
            for (int z = threadIdx.x; z < tz; z += SW_WAVE) dst[z] = src[tz - 1 - z];
        } else {
            for (int z = threadIdx.x; z < tz; z += SW_WAVE) dst[z] = src[z];
        }
        return;
    }
    const S *src = seg + ((size_t)sx * Y + sy) * (size_t)Z + a.oz[i];
    for (int z = threadIdx.x; z < tz; z += SW_WAVE) {
        const int label = (int)src[(m & 4) ? tz - 1 - z : z];
        for (int k = 0; k < L; ++k) dst[(size_t)k * T + z] = label == (int)h.labels[k] ? 1.0f : 0.0f;
    }
}

struct FoldArgs {
    int flips[SW_MAX_V];
};

// one block per tile row (x, y); every lane owns voxel p = (x, y, z) of the tile for all K classes
__global__ void __launch_bounds__(SW_WAVE) sw_fold_kernel(const float *__restrict__ out, const float *__restrict__ gauss,
                                                          float *__restrict__ acc, float *__restrict__ w, FoldArgs a, int tile, int n,
                                                          int V, int K, int tx, int ty, int tz, int ox, int oy, int oz, int X, int Y,
                                                          int Z)
{
#pragma clang fp contract(off)
    const int y = blockIdx.x % ty, x = blockIdx.x / ty;
    const size_t T = (size_t)tx * ty * tz;
    const size_t plane = (size_t)X * Y * Z;
    const size_t vstride = (size_t)n * K * T;              // one variant block of the chunk output
    const float *base = out + (size_t)tile * K * T;
    size_t roff[SW_MAX_V];                                 // row (x, y) of variant v after its flip, without the Z part
    for (int v = 0; v < V; ++v) {
        const int m = a.flips[v];
        const int fx = (m & 1) ? tx - 1 - x : x, fy = (m & 2) ? ty - 1 - y : y;
        roff[v] = (size_t)v * vstride + ((size_t)fx * ty + fy) * tz;
    }
    const float inv = 1.0f / (float)V;                     // V is a power of two: the product equals the division exactly
    const float *grow = gauss + ((size_t)x * ty + y) * tz;
    const size_t dst = ((size_t)(ox + x) * Y + (oy + y)) * Z + oz;
    for (int z = threadIdx.x; z < tz; z += SW_WAVE) {
        const float g = grow[z];
        for (int k = 0; k < K; ++k) {
            const float *ok = base + (size_t)k * T;
            float s = ok[roff[0] + ((a.flips[0] & 4) ? tz - 1 - z : z)];
            for (int v = 1; v < V; ++v) s = s + ok[roff[v] + ((a.flips[v] & 4) ? tz - 1 - z : z)];
            s = s * inv;
            float *pa = acc + (size_t)k * plane + dst + z;
            const float t = s * g;
            *pa = *pa + t;
        }
        w[dst + z] = w[dst + z] + g;
    }
}

// one block per output row (x, y) of the cropped region
__global__ void __launch_bounds__(SW_WAVE) sw_finalize_kernel(const float *__restrict__ acc, const float *__restrict__ w,
                                                              float *__restrict__ logits, long long *__restrict__ labels, int K, int X,
                                                              int Y, int Z, int lx, int ly, int lz, int X0, int Y0, int Z0)
{
#pragma clang fp contract(off)
    const int y = blockIdx.x % Y0, x = blockIdx.x / Y0;
    const size_t plane = (size_t)X * Y * Z, plane0 = (size_t)X0 * Y0 * Z0;
    const size_t src = ((size_t)(lx + x) * Y + (ly + y)) * Z + lz;
    const size_t dst = ((size_t)x * Y0 + y) * Z0;
    for (int z = threadIdx.x; z < Z0; z += SW_WAVE) {
        const float wv = w[src + z];
        float best = 0.f;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            const float l = acc[(size_t)k * plane + src + z] / wv;      // correctly rounded (hipcc's default)
            logits[(size_t)k * plane0 + dst + z] = l;
            // torch.argmax: the first maximum; a NaN counts as the maximum (the first NaN wins)
            if (k == 0 || (!isnan(best) && (l > best || isnan(l)))) {
                best = l;
                arg = k;
            }
        }
        if (labels) labels[dst + z] = arg;
    }
}

int check_flips(const int *flips, int V)
{
    if (!flips) return MLAGG_E_NULLPTR;
    if (V < 1 || V > SW_MAX_V || (V & (V - 1))) return MLAGG_E_UNSUPPORTED;
    for (int v = 0; v < V; ++v)
        if (flips[v] < 0 || flips[v] > 7) return MLAGG_E_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int mlagg_sw_gather(const float *vol, int C, int X, int Y, int Z, const int *origins, int n, const int *flips, int V,
                               float *out, int tx, int ty, int tz, void *stream)
{
    if (!vol || !out || !origins) return MLAGG_E_NULLPTR;
    if (int rc = check_flips(flips, V)) return rc;
    if (C < 1 || X < 1 || Y < 1 || Z < 1 || n < 1 || tx < 1 || ty < 1 || tz < 1) return MLAGG_E_UNSUPPORTED;
    for (int i = 0; i < n; ++i) {
        const int *o = origins + 3 * i;
        if (o[0] < 0 || o[1] < 0 || o[2] < 0 || o[0] + tx > X || o[1] + ty > Y || o[2] + tz > Z) return MLAGG_E_UNSUPPORTED;
    }
    if ((long long)V * SW_MAX_TILES * C * tx * ty > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_SW_GATHER, st);
    GatherArgs a;
    for (int v = 0; v < V; ++v) a.flips[v] = flips[v];
    for (int v = V; v < SW_MAX_V; ++v) a.flips[v] = 0;
    for (int i0 = 0; i0 < n; i0 += SW_MAX_TILES) {
        const int nsub = n - i0 < SW_MAX_TILES ? n - i0 : SW_MAX_TILES;
        for (int i = 0; i < nsub; ++i) {
            a.ox[i] = origins[3 * (i0 + i)];
            a.oy[i] = origins[3 * (i0 + i) + 1];
            a.oz[i] = origins[3 * (i0 + i) + 2];
        }
        const unsigned rows = (unsigned)((long long)V * nsub * C * tx * ty);
        hipLaunchKernelGGL(sw_gather_kernel, dim3(rows), dim3(SW_WAVE), 0, st, vol, out, a, C, X, Y, Z, tx, ty, tz, n, i0, nsub);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}

extern "C" int mlagg_sw_gather_onehot(const float *vol, int C, const void *seg, int seg_kind, const int *labels, int L, int X, int Y,
                                      int Z, const int *origins, int n, const int *flips, int V, float *out, int tx, int ty, int tz,
                                      void *stream)
{
    if (!vol || !out || !origins || !seg || !labels) return MLAGG_E_NULLPTR;
    if (int rc = check_flips(flips, V)) return rc;
    if (C < 1 || X < 1 || Y < 1 || Z < 1 || n < 1 || tx < 1 || ty < 1 || tz < 1) return MLAGG_E_UNSUPPORTED;
    if (seg_kind != MLAGG_SEG_INT8 && seg_kind != MLAGG_SEG_UINT8 && seg_kind != MLAGG_SEG_INT16) return MLAGG_E_UNSUPPORTED;
    if (L < 1 || L > MLAGG_CASCADE_MAX_LABELS) return MLAGG_E_UNSUPPORTED;
    OneHotArgs h;
    for (int k = 0; k < MLAGG_CASCADE_MAX_LABELS; ++k) {
        if (k < L && (labels[k] < 1 || labels[k] > 255)) return MLAGG_E_UNSUPPORTED;
        h.labels[k] = k < L ? (unsigned char)labels[k] : 0;
    }
    for (int i = 0; i < n; ++i) {
        const int *o = origins + 3 * i;
        if (o[0] < 0 || o[1] < 0 || o[2] < 0 || o[0] + tx > X || o[1] + ty > Y || o[2] + tz > Z) return MLAGG_E_UNSUPPORTED;
    }
    if ((long long)V * SW_MAX_TILES * (C + 1) * tx * ty > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_SW_GATHER_ONEHOT, st);
    GatherArgs a;
    for (int v = 0; v < SW_MAX_V; ++v) a.flips[v] = v < V ? flips[v] : 0;
    for (int i0 = 0; i0 < n; i0 += SW_MAX_TILES) {
        const int nsub = n - i0 < SW_MAX_TILES ? n - i0 : SW_MAX_TILES;
        for (int i = 0; i < nsub; ++i) {
            a.ox[i] = origins[3 * (i0 + i)];
            a.oy[i] = origins[3 * (i0 + i) + 1];
            a.oz[i] = origins[3 * (i0 + i) + 2];
        }
        for (int i = nsub; i < SW_MAX_TILES; ++i) a.ox[i] = a.oy[i] = a.oz[i] = 0;
        const dim3 grid((unsigned)((long long)V * nsub * (C + 1) * tx * ty)), block(SW_WAVE);
        if (seg_kind == MLAGG_SEG_INT8)
            hipLaunchKernelGGL(sw_gather_onehot_kernel<signed char>, grid, block, 0, st, vol, static_cast<const signed char *>(seg),
                               out, a, h, C, L, X, Y, Z, tx, ty, tz, n, i0, nsub);
        else if (seg_kind == MLAGG_SEG_UINT8)
            hipLaunchKernelGGL(sw_gather_onehot_kernel<unsigned char>, grid, block, 0, st, vol,
                               static_cast<const unsigned char *>(seg), out, a, h, C, L, X, Y, Z, tx, ty, tz, n, i0, nsub);
        else
            hipLaunchKernelGGL(sw_gather_onehot_kernel<short>, grid, block, 0, st, vol, static_cast<const short *>(seg), out, a, h,
                               C, L, X, Y, Z, tx, ty, tz, n, i0, nsub);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}

extern "C" int mlagg_sw_fold(const float *out, int tile, int n, const int *flips, int V, int K, const float *gauss, int tx, int ty,
                             int tz, int ox, int oy, int oz, float *acc, float *w, int X, int Y, int Z, void *stream)
{
    if (!out || !gauss || !acc || !w) return MLAGG_E_NULLPTR;
    if (int rc = check_flips(flips, V)) return rc;
    if (n < 1 || tile < 0 || tile >= n || K < 1 || tx < 1 || ty < 1 || tz < 1 || X < 1 || Y < 1 || Z < 1) return MLAGG_E_UNSUPPORTED;
    if (ox < 0 || oy < 0 || oz < 0 || ox + tx > X || oy + ty > Y || oz + tz > Z) return MLAGG_E_UNSUPPORTED;
    if ((long long)tx * ty > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_SW_FOLD, st);
    FoldArgs a;
    for (int v = 0; v < SW_MAX_V; ++v) a.flips[v] = v < V ? flips[v] : 0;
    hipLaunchKernelGGL(sw_fold_kernel, dim3((unsigned)(tx * ty)), dim3(SW_WAVE), 0, st, out, gauss, acc, w, a, tile, n, V, K, tx, ty,
                       tz, ox, oy, oz, X, Y, Z);
    return (int)hipGetLastError();
}

extern "C" int mlagg_sw_finalize(const float *acc, const float *w, int K, int X, int Y, int Z, int lx, int ly, int lz, int X0, int Y0,
                                 int Z0, float *logits, long long *labels, void *stream)
{
    if (!acc || !w || !logits) return MLAGG_E_NULLPTR;
    if (K < 1 || X < 1 || Y < 1 || Z < 1 || X0 < 1 || Y0 < 1 || Z0 < 1) return MLAGG_E_UNSUPPORTED;
    if (lx < 0 || ly < 0 || lz < 0 || lx + X0 > X || ly + Y0 > Y || lz + Z0 > Z) return MLAGG_E_UNSUPPORTED;
    if ((long long)X0 * Y0 > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_SW_FINALIZE, st);
    hipLaunchKernelGGL(sw_finalize_kernel, dim3((unsigned)(X0 * Y0)), dim3(SW_WAVE), 0, st, acc, w, logits, labels, K, X, Y, Z, lx, ly,
                       lz, X0, Y0, Z0);
    return (int)hipGetLastError();
}
