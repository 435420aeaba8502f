// K25 -- 3-D spatial augmentation on the device: rotation + isotropic scaling of a training batch, cubic B-spline data and
// trilinear per-label segmentation, or the centre crop of the samples the draw left alone.
//
// What it replaces: batchgenerators' augment_spatial / interpolate_img for a 3-D patch (the SpatialTransform of
// nnUNetTrainer.get_training_transforms, nnUNetTrainer.py:666-677: order 3 data with cval 0, order 1 segmentation with cval -1,
// random_crop False), i.e. scipy.ndimage.map_coordinates once per channel and once per label indicator of every sample.
//
// Layouts: vol (B, C, Xi, Yi, Zi) fp32 -- per sample the cubic B-spline coefficients (mirror boundary) where it is resampled,
// the raw data where it is cropped; lab (B, 1, Xi, Yi, Zi) int16, the loader's labels as they are (-1 padding included);
// out (B, C, Xo, Yo, Zo) fp32, out_lab (B, 1, Xo, Yo, Zo) fp32.  Z is the contiguous axis everywhere.
// One lane per output voxel, the flat output index split with z fastest: a wave's stores are one or two contiguous runs and
// its 64 lanes read neighbouring coefficient lines (a rotation by <= 30 degrees and a zoom <= 1.4 keep a wave's footprint
// within a few 128-byte lines per tap row), which L1 / L2 serve.  Per voxel the coordinate (fp64 affine, as the float64
// reference builds it), the 4 + 4 + 4 separable weights and mirror indices are computed once and reused for every channel.
// Segmentation: the 8 trilinear taps' labels and weights; each distinct label's indicator is the sum of its taps' weights (taps
// in scipy's order), the largest label whose indicator reaches 0.5 wins, 0 where none does or outside the input.
// No atomics, no reductions across lanes: repeated calls are bit-identical.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mlagg_hip.h"
#include "prof.h"

namespace {

constexpr int A3_BLOCK = 256;
constexpr int A3_MAX_B = 16;           // samples per launch (the entry splits larger batches)

struct Aug3dArgs {
    double A[A3_MAX_B][12];            // row j: input coordinate j = A[4j + 3] + A[4j] x + A[4j + 1] y + A[4j + 2] z
    int resample[A3_MAX_B];
};

__device__ __forceinline__ int mirror_index(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i > n - 1 ? 2 * (n - 1) - i : i;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

__device__ __forceinline__ void cubic_weights(float t, float w[4])
{
    const float t2 = t * t, t3 = t2 * t, u = 1.0f - t;
    w[0] = u * u * u / 6.0f;
    w[1] = (3.0f * t3 - 6.0f * t2 + 4.0f) / 6.0f;
    w[2] = (-3.0f * t3 + 3.0f * t2 + 3.0f * t + 1.0f) / 6.0f;
    w[3] = t3 / 6.0f;
}

// The per-label vote of interpolate_img(is_seg): each distinct label's indicator is the sum of its taps' weights (taps in scipy's
// order), the largest label whose indicator reaches 0.5 wins, 0 where none does.  N = 8 (trilinear, K25) or 4 (bilinear, K31).
template <int N>
__device__ __forceinline__ float label_vote(const int (&l)[N], const float (&w)[N])
{
    int best = 0;
    bool hit = false;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        bool first = true;
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (j < k && l[j] == l[k]) first = false;
            if (l[j] == l[k]) sum += w[j];
        }
        if (first && sum >= 0.5f && (!hit || l[k] > best)) {
            best = l[k];
            hit = true;
        }
    }
    return hit ? (float)best : 0.0f;
}

__global__ void __launch_bounds__(A3_BLOCK) aug3d_resample_kernel(const float *__restrict__ vol, const short *__restrict__ lab,
                                                                  float *__restrict__ out, float *__restrict__ out_lab, Aug3dArgs a,
                                                                  int C, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo,
                                                                  long long nvox)
{
    const long long i = (long long)blockIdx.x * A3_BLOCK + threadIdx.x;
    if (i >= nvox) return;
    const int z = (int)(i % Zo);
    long long r = i / Zo;
    const int y = (int)(r % Yo);
    r /= Yo;
    const int x = (int)(r % Xo);
    const int b = (int)(r / Xo);
    const size_t in_plane = (size_t)Xi * Yi * Zi, out_plane = (size_t)Xo * Yo * Zo;
    const size_t o = ((size_t)x * Yo + y) * Zo + z;
    const float *vb = vol + (size_t)b * C * in_plane;
    float *ob = out + (size_t)b * C * out_plane + o;
    if (!a.resample[b]) {                                  // centre crop (crop_type "center"), bit for bit
        const size_t s = ((size_t)(x + (Xi - Xo) / 2) * Yi + (y + (Yi - Yo) / 2)) * Zi + z + (Zi - Zo) / 2;
        for (int c = 0; c < C; ++c) ob[(size_t)c * out_plane] = vb[(size_t)c * in_plane + s];
        if (lab) out_lab[(size_t)b * out_plane + o] = (float)lab[(size_t)b * in_plane + s];
        return;
    }
    const double *A = a.A[b];
    const double px = A[3] + A[0] * x + A[1] * y + A[2] * z;
    const double py = A[7] + A[4] * x + A[5] * y + A[6] * z;
    const double pz = A[11] + A[8] * x + A[9] * y + A[10] * z;
    if (!(px >= 0.0 && px <= Xi - 1 && py >= 0.0 && py <= Yi - 1 && pz >= 0.0 && pz <= Zi - 1)) {   // mode "constant"
        for (int c = 0; c < C; ++c) ob[(size_t)c * out_plane] = 0.0f;
        if (lab) out_lab[(size_t)b * out_plane + o] = 0.0f;
        return;
    }
    const double fx = floor(px), fy = floor(py), fz = floor(pz);
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    const float tx = (float)(px - fx), ty = (float)(py - fy), tz = (float)(pz - fz);
    float wx[4], wy[4], wz[4];
    cubic_weights(tx, wx);
    cubic_weights(ty, wy);
    cubic_weights(tz, wz);
    int jx[4], jy[4], jz[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        jx[k] = mirror_index(ix - 1 + k, Xi);
        jy[k] = mirror_index(iy - 1 + k, Yi);
        jz[k] = mirror_index(iz - 1 + k, Zi);
    }
    for (int c = 0; c < C; ++c) {
        const float *vc = vb + (size_t)c * in_plane;
        float acc = 0.0f;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float sy = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float *row = vc + ((size_t)jx[p] * Yi + jy[q]) * Zi;
                const float sz = wz[0] * row[jz[0]] + wz[1] * row[jz[1]] + wz[2] * row[jz[2]] + wz[3] * row[jz[3]];
                sy += wy[q] * sz;
            }
            acc += wx[p] * sy;
        }
        ob[(size_t)c * out_plane] = acc;
    }
    if (lab) {
        const short *lb = lab + (size_t)b * in_plane;
        const int kx[2] = {mirror_index(ix, Xi), mirror_index(ix + 1, Xi)};
        const int ky[2] = {mirror_index(iy, Yi), mirror_index(iy + 1, Yi)};
        const int kz[2] = {mirror_index(iz, Zi), mirror_index(iz + 1, Zi)};
        const float lx[2] = {1.0f - tx, tx}, ly[2] = {1.0f - ty, ty}, lz[2] = {1.0f - tz, tz};
        int l[8];
        float w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p = k >> 2, q = (k >> 1) & 1, s = k & 1;
            l[k] = lb[((size_t)kx[p] * Yi + ky[q]) * Zi + kz[s]];
            w[k] = lx[p] * ly[q] * lz[s];
        }
        out_lab[(size_t)b * out_plane + o] = label_vote(l, w);
    }
}

// K31 -- the same transform for an anisotropic patch ("dummy 2-D" augmentation): every slice x of (B, C, X, Y, Z) is resampled in
// its own (y, z) plane with one rotation / scale per sample, X is never resampled.
//
// What it replaces: Convert3DTo2DTransform + the 2-D SpatialTransform on (B, C * X, Y, Z) + Convert2DTo3DTransform
// (nnUNetTrainer.get_training_transforms with do_dummy_2d_data_aug, nnUNetTrainer.py:658-680): map_coordinates once per slice of
// every channel and of every label indicator.  16 cubic taps on coefficients prefiltered along Y and Z only, 4 bilinear label
// taps; the arithmetic (fp64 coordinate, fp32 fractions, inside test, tap order, vote) is K25's with the x axis removed.
//
// Work decomposition: the rotation range is +-180 degrees, so a z-fastest wave would read 64 different rows per tap near 90
// degrees.  Here a wave owns an 8 x 8 (y, z) output tile -- lane = 8 (y & 7) + (z & 7) -- whose input footprint is a rotated
// square of at most 8 * 1.4 * sqrt(2) + 3 = 19 rows of about as many columns at any angle: a few tens of 128-byte lines, shared by
// the 16 taps of its 64 lanes.  A block is 2 x 2 such tiles (16 x 16 outputs).  A lane computes its coordinate, the 4 + 4 weights
// and the 16 mirror-indexed tap offsets of the plane once and keeps them in registers for a chunk of slices and all channels
// (blockIdx.y = chunk, blockIdx.z = sample): per slice and channel 16 loads and 16 multiply-adds remain.  The entry sizes the
// chunk (planar_chunk): at least 4 slices where X allows, so the set-up is paid once per several slices, at most 16, and smaller
// than X while the grid has fewer than 1024 blocks, so that thin volumes still fill the machine.  The footprint is read through
// L1 / L2 as it is; it is not staged in LDS.  Stores are 32-byte runs, 8 per wave and plane.
// No atomics, no reductions across lanes: repeated calls are bit-identical.
constexpr int PL_TILE = 16;            // block tile edge: 2 x 2 waves of 8 x 8 outputs

struct PlanarArgs {
    double A[A3_MAX_B][6];             // input y = A[2] + A[0] y + A[1] z, input z = A[5] + A[3] y + A[4] z
    int resample[A3_MAX_B];
};

__global__ void __launch_bounds__(A3_BLOCK) aug3d_planar_kernel(const float *__restrict__ vol, const short *__restrict__ lab,
                                                                float *__restrict__ out, float *__restrict__ out_lab, PlanarArgs a,
                                                                int C, int X, int Yi, int Zi, int Yo, int Zo, int chunk, int tiles_z)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y = (int)(blockIdx.x / tiles_z) * PL_TILE + (wave >> 1) * 8 + (lane >> 3);
    const int z = (int)(blockIdx.x % tiles_z) * PL_TILE + (wave & 1) * 8 + (lane & 7);
    if (y >= Yo || z >= Zo) return;
    const int b = blockIdx.z;
    const int x0 = blockIdx.y * chunk, x1 = x0 + chunk < X ? x0 + chunk : X;
    const size_t in_slice = (size_t)Yi * Zi, out_slice = (size_t)Yo * Zo;
    const float *vb = vol + (size_t)b * C * X * in_slice;
    const short *lb = lab ? lab + (size_t)b * X * in_slice : nullptr;
    float *ob = out + (size_t)b * C * X * out_slice + (size_t)y * Zo + z;
    float *olb = lab ? out_lab + (size_t)b * X * out_slice + (size_t)y * Zo + z : nullptr;
    if (!a.resample[b]) {                                  // centre crop over (y, z), bit for bit
        const int s = (y + (Yi - Yo) / 2) * Zi + z + (Zi - Zo) / 2;
        for (int x = x0; x < x1; ++x) {
            for (int c = 0; c < C; ++c) ob[((size_t)c * X + x) * out_slice] = vb[((size_t)c * X + x) * in_slice + s];
            if (lab) olb[(size_t)x * out_slice] = (float)lb[(size_t)x * in_slice + s];
        }
        return;
    }
    const double *A = a.A[b];
    const double py = A[2] + A[0] * y + A[1] * z;
    const double pz = A[5] + A[3] * y + A[4] * z;
    if (!(py >= 0.0 && py <= Yi - 1 && pz >= 0.0 && pz <= Zi - 1)) {                                   // mode "constant"
        for (int x = x0; x < x1; ++x) {
            for (int c = 0; c < C; ++c) ob[((size_t)c * X + x) * out_slice] = 0.0f;
            if (lab) olb[(size_t)x * out_slice] = 0.0f;
        }
        return;
    }
    const double fy = floor(py), fz = floor(pz);
    const int iy = (int)fy, iz = (int)fz;
    const float ty = (float)(py - fy), tz = (float)(pz - fz);
    if (C > 0) {
        float wy[4], wz[4];
        cubic_weights(ty, wy);
        cubic_weights(tz, wz);
        int off[16];                                       // tap (q, r) of the plane: row jy[q], column jz[r]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = mirror_index(iy - 1 + q, Yi) * Zi;
#pragma unroll
            for (int r = 0; r < 4; ++r) off[4 * q + r] = row + mirror_index(iz - 1 + r, Zi);
        }
        for (int x = x0; x < x1; ++x)
            for (int c = 0; c < C; ++c) {
                const float *vs = vb + ((size_t)c * X + x) * in_slice;
                float acc = 0.0f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float sz = wz[0] * vs[off[4 * q]] + wz[1] * vs[off[4 * q + 1]] + wz[2] * vs[off[4 * q + 2]] +
                                     wz[3] * vs[off[4 * q + 3]];
                    acc += wy[q] * sz;
                }
                ob[((size_t)c * X + x) * out_slice] = acc;
            }
    }
    if (lab) {
        const int ky[2] = {mirror_index(iy, Yi) * Zi, mirror_index(iy + 1, Yi) * Zi};
        const int kz[2] = {mirror_index(iz, Zi), mirror_index(iz + 1, Zi)};
        const float ly[2] = {1.0f - ty, ty}, lz[2] = {1.0f - tz, tz};
        float w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = ly[k >> 1] * lz[k & 1];
        for (int x = x0; x < x1; ++x) {
            const short *ls = lb + (size_t)x * in_slice;
            int l[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) l[k] = ls[ky[k >> 1] + kz[k & 1]];
            olb[(size_t)x * out_slice] = label_vote(l, w);
        }
    }
}

// Slices per block: see the header comment of K31.
int planar_chunk(int X, long long blocks_per_chunk)
{
    long long chunk = (long long)X * blocks_per_chunk / 1024;
    chunk = chunk < 4 ? 4 : (chunk > 16 ? 16 : chunk);
    chunk = chunk > X ? X : chunk;
    const int n = (X + (int)chunk - 1) / (int)chunk;       // even the chunks out: 5 slices in chunks of 4 become 3 + 2
    return (X + n - 1) / n;
}

}  // namespace

extern "C" int mlagg_aug3d_resample(const float *vol, const short *lab, int B, int C, int Xi, int Yi, int Zi, const double *affine,
                                    const int *resample, float *out, float *out_lab, int Xo, int Yo, int Zo, void *stream)
{
    if ((C > 0 && (!vol || !out)) || !affine || !resample || (lab && !out_lab)) return MLAGG_E_NULLPTR;
    if (B < 1 || C < 0 || (C == 0 && !lab) || Xi < 1 || Yi < 1 || Zi < 1 || Xo < 1 || Yo < 1 || Zo < 1) return MLAGG_E_UNSUPPORTED;
    for (int b = 0; b < B; ++b)                            // a cropped sample reads the centre of its input
        if (!resample[b] && (Xo > Xi || Yo > Yi || Zo > Zi)) return MLAGG_E_UNSUPPORTED;
    if ((long long)A3_MAX_B * Xo * Yo * Zo > (1LL << 38)) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_AUG3D_RESAMPLE, st);
    const size_t in_plane = (size_t)Xi * Yi * Zi, out_plane = (size_t)Xo * Yo * Zo;
    for (int b0 = 0; b0 < B; b0 += A3_MAX_B) {
        const int nb = B - b0 < A3_MAX_B ? B - b0 : A3_MAX_B;
        Aug3dArgs a;
        for (int b = 0; b < A3_MAX_B; ++b) {
            for (int k = 0; k < 12; ++k) a.A[b][k] = b < nb ? affine[12 * (b0 + b) + k] : 0.0;
            a.resample[b] = b < nb ? (resample[b0 + b] != 0) : 0;
        }
        const long long nvox = (long long)nb * out_plane;
        const unsigned blocks = (unsigned)((nvox + A3_BLOCK - 1) / A3_BLOCK);
        hipLaunchKernelGGL(aug3d_resample_kernel, dim3(blocks), dim3(A3_BLOCK), 0, st, vol + (size_t)b0 * C * in_plane,
                           lab ? lab + (size_t)b0 * in_plane : nullptr, out + (size_t)b0 * C * out_plane,
                           lab ? out_lab + (size_t)b0 * out_plane : nullptr, a, C, Xi, Yi, Zi, Xo, Yo, Zo, nvox);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}

extern "C" int mlagg_aug3d_resample_planar(const float *vol, const short *lab, int B, int C, int X, int Yi, int Zi,
                                           const double *affine, const int *resample, float *out, float *out_lab, int Yo, int Zo,
                                           void *stream)
{
    if ((C > 0 && (!vol || !out)) || !affine || !resample || (lab && !out_lab)) return MLAGG_E_NULLPTR;
    if (B < 1 || C < 0 || (C == 0 && !lab) || X < 1 || Yi < 1 || Zi < 1 || Yo < 1 || Zo < 1) return MLAGG_E_UNSUPPORTED;
    for (int b = 0; b < B; ++b)                            // a cropped sample reads the centre of its input planes
        if (!resample[b] && (Yo > Yi || Zo > Zi)) return MLAGG_E_UNSUPPORTED;
    if ((long long)Yi * Zi > INT32_MAX || (long long)Yo * Zo > INT32_MAX) return MLAGG_E_UNSUPPORTED;   // in-plane offsets are ints
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_AUG3D_PLANAR, st);
    const size_t in_vol = (size_t)X * Yi * Zi, out_vol = (size_t)X * Yo * Zo;
    const int tiles_y = (Yo + PL_TILE - 1) / PL_TILE, tiles_z = (Zo + PL_TILE - 1) / PL_TILE;
    for (int b0 = 0; b0 < B; b0 += A3_MAX_B) {
        const int nb = B - b0 < A3_MAX_B ? B - b0 : A3_MAX_B;
        PlanarArgs a;
        for (int b = 0; b < A3_MAX_B; ++b) {
            for (int k = 0; k < 6; ++k) a.A[b][k] = b < nb ? affine[6 * (b0 + b) + k] : 0.0;
            a.resample[b] = b < nb ? (resample[b0 + b] != 0) : 0;
        }
        const int chunk = planar_chunk(X, (long long)nb * tiles_y * tiles_z);
        const int chunks = (X + chunk - 1) / chunk;
        if (chunks > 65535) return MLAGG_E_UNSUPPORTED;
        hipLaunchKernelGGL(aug3d_planar_kernel, dim3((unsigned)tiles_y * tiles_z, chunks, nb), dim3(A3_BLOCK), 0, st,
                           C ? vol + (size_t)b0 * C * in_vol : nullptr, lab ? lab + (size_t)b0 * in_vol : nullptr,
                           C ? out + (size_t)b0 * C * out_vol : nullptr, lab ? out_lab + (size_t)b0 * out_vol : nullptr, a, C, X, Yi,
                           Zi, Yo, Zo, chunk, tiles_z);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}
