// K22 -- case preprocessing on the device: the non-zero box, crop + per-channel normalisation, and the cubic (order-3) resampling
// to the plan's spacing, for one raw (c, x, y, z) fp32 volume.
//
// What it replaces: the reference's DefaultPreprocessor.run_case (nnunetv2/preprocessing/preprocessors/default_preprocessor.py:38-124)
// for a test case, which on the CPU
//   crops to the box of the filled non-zero mask (preprocessing/cropping/cropping.py),
//   normalises every channel in fp32 (preprocessing/normalization/default_normalization_schemes.py),
//   and resamples with resample_data_or_seg_to_shape(order=3, order_z=0) (preprocessing/resampling/default_resampling.py:76-200):
//   skimage resize(order=3, mode='edge') = ndi.zoom(order=3, mode='nearest', grid_mode=True) clipped to the input's range, per
//   channel (3-D) or per slice along the low-resolution axis, followed by map_coordinates(order=0 | 1) along that axis.
//
//   pp_box_kernel         per-axis min / max of the coordinates of non-zero voxels, any strides (integer atomics);
//   pp_stats_kernel       per-channel fp64 partial sums (shifted by the window's first value), count, min and max of the cropped
//                         window, optionally under a mask; pp_stats_final_kernel folds them in a fixed order into the scheme's
//                         fp32 constants (ZScore mean / std, RescaleTo01 min / range);
//   pp_normalize_kernel   crop + scheme in fp32, contiguous (C, X, Y, Z) out;
//   pp_minmax_kernel      min / max of every clip domain (a channel, or one slice along the low-resolution axis), ordered-int atomics;
//   pp_cubic_kernel       one axis of the cubic B-spline zoom: lines of that axis staged in LDS, prefiltered, evaluated at 4 taps;
//   pp_gather_kernel      order-0 / order-1 blend along the low-resolution axis of separate-z resampling, rounded to fp32.
//
// The cubic zoom is scipy's, restated separably: every line is edge-padded by 12 (_prepad_for_spline_filter) through index
// clamping, prefiltered with the cubic B-spline's inverse filter (pole z = sqrt(3) - 2) under the reflect boundary that
// spline_filter1d(mode='nearest') uses, and evaluated at c = (o + 0.5) * n_in / n_out - 0.5 + 12 with the four B-spline weights.
// The prefilter is the FIR form h[k] = 6z / (z^2 - 1) * z^|k|, |k| <= 30 (|z|^31 < 2e-18), on the reflect-extended padded line, so
// every coefficient is independent and the whole line runs in parallel.  Filtering and evaluating along one axis commute with the
// same along another, so the axes run one pass each, in fp64; the host builds the tap tables (preprocessing._cubic_taps).
// Every sum has a fixed order and every atomic is an integer min / max: results are bit-reproducible.  `#pragma clang fp
// contract(off)` keeps the fp32 normalisation exactly the reference's sequence of roundings.  All volume offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mlagg_hip.h"
#include "prof.h"

namespace {

constexpr int PP_BLOCK = 256;
constexpr int PP_STATS_BLOCKS = MLAGG_PP_STATS_PARTIALS;   // partials per channel (fixed: the fold order does not depend on the device)
constexpr int PP_PAD = 12;             // scipy's _prepad_for_spline_filter
constexpr int PP_FIR = 30;             // prefilter half-width
constexpr int PP_LDS_BYTES = 65536;

struct Src {
    const float *p;
    long long sc, sx, sy, sz;
};

__device__ __forceinline__ unsigned ord_enc(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float ord_dec(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// ---------------------------------------------------------------------------------------------------------------------------
// non-zero box
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void pp_box_init_kernel(int *box)
{
    if (threadIdx.x < 3) box[threadIdx.x] = 0x7fffffff;
    else if (threadIdx.x < 6) box[threadIdx.x] = -1;
}

__global__ void __launch_bounds__(PP_BLOCK) pp_box_kernel(Src s, int X, int Y, int Z, long long N, int *box)
{
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
    const long long stride = (long long)gridDim.x * PP_BLOCK;
    for (long long f = (long long)blockIdx.x * PP_BLOCK + threadIdx.x; f < N; f += stride) {
        long long r = f / Z;
        const int z = (int)(f - r * Z);
        const int y = (int)(r % Y);
        r /= Y;
        const int x = (int)(r % X);
        const long long c = r / X;
        if (s.p[c * s.sc + x * s.sx + y * s.sy + z * s.sz] != 0.f) {
            lo[0] = min(lo[0], x), lo[1] = min(lo[1], y), lo[2] = min(lo[2], z);
            hi[0] = max(hi[0], x), hi[1] = max(hi[1], y), hi[2] = max(hi[2], z);
        }
    }
    __shared__ int red[6][PP_BLOCK];
    for (int d = 0; d < 3; ++d) red[d][threadIdx.x] = lo[d], red[3 + d][threadIdx.x] = hi[d];
    __syncthreads();
    for (int h = PP_BLOCK / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            for (int d = 0; d < 3; ++d) {
                red[d][threadIdx.x] = min(red[d][threadIdx.x], red[d][threadIdx.x + h]);
                red[3 + d][threadIdx.x] = max(red[3 + d][threadIdx.x], red[3 + d][threadIdx.x + h]);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) {
        if (red[3 + threadIdx.x][0] >= 0) atomicMin(box + threadIdx.x, red[threadIdx.x][0]);
    } else if (threadIdx.x < 6) {
        if (red[threadIdx.x][0] >= 0) atomicMax(box + threadIdx.x, red[threadIdx.x][0]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// crop window: statistics and normalisation
// ---------------------------------------------------------------------------------------------------------------------------
struct Window {
    int lo[3];
    int ext[3];
};

__device__ __forceinline__ long long window_offset(const Src &s, const Window &w, long long c, long long f, long long &sp)
{
    long long r = f / w.ext[2];
    const int z = (int)(f - r * w.ext[2]);
    const int y = (int)(r % w.ext[1]);
    const int x = (int)(r / w.ext[1]);
    sp = f;
    return c * s.sc + (long long)(w.lo[0] + x) * s.sx + (long long)(w.lo[1] + y) * s.sy + (long long)(w.lo[2] + z) * s.sz;
}

// partials[(c * PP_STATS_BLOCKS + b) * 5 + {0..4}] = sum (x - x0), sum (x - x0)^2, count, min, max over block b's share of the
// window of channel c (voxels with mask != 0 when a mask is given; x0 = the window's first voxel)
__global__ void __launch_bounds__(PP_BLOCK) pp_stats_kernel(Src s, Window w, int c, const uint8_t *__restrict__ mask,
                                                            double *__restrict__ partials)
{
    const long long V = (long long)w.ext[0] * w.ext[1] * w.ext[2];
    long long sp;
    const double x0 = s.p[window_offset(s, w, c, 0, sp)];
    double s1 = 0.0, s2 = 0.0, n = 0.0, mn = INFINITY, mx = -INFINITY;
    for (long long f = (long long)blockIdx.x * PP_BLOCK + threadIdx.x; f < V; f += (long long)PP_STATS_BLOCKS * PP_BLOCK) {
        const long long off = window_offset(s, w, c, f, sp);
        if (mask && !mask[sp]) continue;
        const double v = s.p[off];
        const double d = v - x0;
        s1 += d;
        s2 += d * d;
        n += 1.0;
        mn = fmin(mn, v);
        mx = fmax(mx, v);
    }
    __shared__ double red[5][PP_BLOCK];
    red[0][threadIdx.x] = s1, red[1][threadIdx.x] = s2, red[2][threadIdx.x] = n, red[3][threadIdx.x] = mn, red[4][threadIdx.x] = mx;
    __syncthreads();
    for (int h = PP_BLOCK / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            const int t = threadIdx.x;
            red[0][t] += red[0][t + h];
            red[1][t] += red[1][t + h];
            red[2][t] += red[2][t + h];
            red[3][t] = fmin(red[3][t], red[3][t + h]);
            red[4][t] = fmax(red[4][t], red[4][t + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 5) partials[((long long)c * PP_STATS_BLOCKS + blockIdx.x) * 5 + threadIdx.x] = red[threadIdx.x][0];
}

// one thread: fold channel c's partials in order; stats[c * 4] = fp64 (mean, std, min, max); params[c * 4 + 0 | 3] for RescaleTo01
// (min, max(range, 1e-8)), params[c * 4 + 2 | 3] for ZScore (mean, max(std, 1e-8)), all rounded to fp32 as numpy holds them
__global__ void pp_stats_final_kernel(const double *__restrict__ partials, Src s, Window w, int c, int scheme,
                                      float *__restrict__ params, double *__restrict__ stats)
{
#pragma clang fp contract(off)
    long long sp;
    const double x0 = s.p[window_offset(s, w, c, 0, sp)];
    double s1 = 0.0, s2 = 0.0, n = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int b = 0; b < PP_STATS_BLOCKS; ++b) {
        const double *q = partials + ((long long)c * PP_STATS_BLOCKS + b) * 5;
        s1 += q[0];
        s2 += q[1];
        n += q[2];
        mn = fmin(mn, q[3]);
        mx = fmax(mx, q[4]);
    }
    const double dm = s1 / n;
    const double mean = x0 + dm;
    const double std = sqrt(fmax(s2 / n - dm * dm, 0.0));
    stats[c * 4 + 0] = mean, stats[c * 4 + 1] = std, stats[c * 4 + 2] = mn, stats[c * 4 + 3] = mx;
    if (scheme == MLAGG_PP_ZSCORE || scheme == MLAGG_PP_ZSCORE_MASKED) {
        const float sf = (float)std;
        params[c * 4 + 2] = (float)mean;
        params[c * 4 + 3] = ((double)sf >= 1e-8) ? sf : (float)1e-8;          // max(std, 1e-8) with an fp32 std
    } else if (scheme == MLAGG_PP_RESCALE01) {
        const float r = __fsub_rn((float)mx, (float)mn);
        params[c * 4 + 0] = (float)mn;
        params[c * 4 + 3] = fmaxf(r, (float)1e-8);                            // np.clip(image.max(), a_min=1e-8)
    }
}

__global__ void __launch_bounds__(PP_BLOCK) pp_normalize_kernel(Src s, Window w, int C, const int *__restrict__ schemes,
                                                                const float *__restrict__ params, const uint8_t *__restrict__ mask,
                                                                float *__restrict__ out, long long V)
{
#pragma clang fp contract(off)
    const long long g = (long long)blockIdx.x * PP_BLOCK + threadIdx.x;
    if (g >= V * C) return;
    const long long c = g / V;
    long long sp;
    const float x = s.p[window_offset(s, w, c, g - c * V, sp)];
    const float *pr = params + c * 4;
    float v = x;
    switch (schemes[c]) {
    case MLAGG_PP_CT: v = __fdiv_rn(__fsub_rn(fminf(fmaxf(x, pr[0]), pr[1]), pr[2]), pr[3]); break;
    case MLAGG_PP_ZSCORE: v = __fdiv_rn(__fsub_rn(x, pr[2]), pr[3]); break;
    case MLAGG_PP_ZSCORE_MASKED: v = mask[sp] ? __fdiv_rn(__fsub_rn(x, pr[2]), pr[3]) : x; break;
    case MLAGG_PP_RESCALE01: v = __fdiv_rn(__fsub_rn(x, pr[0]), pr[3]); break;
    case MLAGG_PP_RGB01: v = __fdiv_rn(x, 255.f); break;
    default: break;
    }
    out[g] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// clip domains: domain d = c * D + i holds the voxels of channel c whose coordinate along the domain axis is i (D = 1: the whole
// channel).  A channel of V voxels is (outer, D, inner) around that axis.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PP_BLOCK) pp_minmax_kernel(const float *__restrict__ x, long long V, int D, long long inner,
                                                             int chunks, unsigned *__restrict__ lo, unsigned *__restrict__ hi)
{
    const int d = blockIdx.x / chunks, k = blockIdx.x % chunks;
    const int c = d / D, i = d % D;
    const long long P = V / D;
    const float *base = x + (long long)c * V + (long long)i * inner;
    unsigned a = 0xffffffffu, b = 0u;
    for (long long j = (long long)k * PP_BLOCK + threadIdx.x; j < P; j += (long long)chunks * PP_BLOCK) {
        const long long o = j / inner;
        const unsigned e = ord_enc(base[o * D * inner + (j - o * inner)]);
        a = min(a, e);
        b = max(b, e);
    }
    __shared__ unsigned red[2][PP_BLOCK];
    red[0][threadIdx.x] = a, red[1][threadIdx.x] = b;
    __syncthreads();
    for (int h = PP_BLOCK / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            red[0][threadIdx.x] = min(red[0][threadIdx.x], red[0][threadIdx.x + h]);
            red[1][threadIdx.x] = max(red[1][threadIdx.x], red[1][threadIdx.x + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMin(lo + d, red[0][0]);
        atomicMax(hi + d, red[1][0]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// one axis of the cubic zoom.  The volume is (outer, n_in, inner) around the axis; a block takes TI lines: TI consecutive `inner`
// positions of one outer index (inner > 1, loads coalesced across lines), or TI consecutive outer indices (inner == 1, the lines
// are one contiguous run).  LDS: raw[TI][n_in], coef[TI][M] in fp64.
// ---------------------------------------------------------------------------------------------------------------------------
struct Fir {
    double h[PP_FIR + 1];              // h[|k|]
};

struct Clip {
    const unsigned *lo, *hi;           // ordered-int min / max per domain, or NULL: no clip
    long long cstride;                 // output elements per channel
    long long dstride;                 // output elements per step of the domain axis
    int D;                             // domain axis extent (1: per channel)
};

template <typename Tin, typename Tout>
__global__ void __launch_bounds__(PP_BLOCK) pp_cubic_kernel(const Tin *__restrict__ in, Tout *__restrict__ out, long long outer,
                                                            long long inner, int n_in, int n_out, int TI, const int *__restrict__ start,
                                                            const double *__restrict__ wt, int P0, int M, Fir fir, Clip clip)
{
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    double *raw = lds;                              // [TI][n_in]
    double *coef = lds + (long long)TI * n_in;      // [TI][M]
    long long ob, t0;
    int cnt;
    if (inner > 1) {
        const long long nt = (inner + TI - 1) / TI;
        ob = blockIdx.x / nt;
        t0 = (blockIdx.x - ob * nt) * TI;
        cnt = (int)min((long long)TI, inner - t0);
    } else {
        ob = (long long)blockIdx.x * TI;
        t0 = 0;
        cnt = (int)min((long long)TI, outer - ob);
    }
    const int nin_all = cnt * n_in;
    if (inner > 1) {
        const Tin *base = in + ob * n_in * inner + t0;
        for (int k = threadIdx.x; k < n_in * TI; k += PP_BLOCK) {
            const int i = k / TI, j = k - i * TI;
            if (j < cnt) raw[j * n_in + i] = (double)base[(long long)i * inner + j];
        }
    } else {
        const Tin *base = in + ob * n_in;
        for (int k = threadIdx.x; k < nin_all; k += PP_BLOCK) raw[k] = (double)base[k];
    }
    __syncthreads();
    const int N = n_in + 2 * PP_PAD;
    for (int k = threadIdx.x; k < cnt * M; k += PP_BLOCK) {
        const int j = k / M, m = k - j * M;
        const double *r = raw + j * n_in;
        const int p = P0 + m;
        double acc = 0.0;
        for (int q = -PP_FIR; q <= PP_FIR; ++q) {
            int u = p + q;
            u = u < 0 ? -u - 1 : (u >= N ? 2 * N - 1 - u : u);          // reflect: d c b a | a b c d
            u = min(max(u - PP_PAD, 0), n_in - 1);                      // the 12-value edge padding
            acc = acc + fir.h[q < 0 ? -q : q] * r[u];
        }
        coef[k] = acc;
    }
    __syncthreads();
    const int nout_all = cnt * n_out;
    for (int k = threadIdx.x; k < nout_all; k += PP_BLOCK) {
        int j, o;
        if (inner > 1) {
            o = k / cnt;
            j = k - o * cnt;
        } else {
            j = k / n_out;
            o = k - j * n_out;
        }
        const double *cf = coef + j * M + (start[o] - P0);
        const double *wo = wt + 4LL * o;
        double v = wo[0] * cf[0] + wo[1] * cf[1] + wo[2] * cf[2] + wo[3] * cf[3];
        const long long f = inner > 1 ? (ob * n_out + o) * inner + t0 + j : (ob + j) * n_out + o;
        if (clip.lo) {
            const long long dom = (f / clip.cstride) * clip.D + (f / clip.dstride) % clip.D;
            v = fmin(fmax(v, (double)ord_dec(clip.lo[dom])), (double)ord_dec(clip.hi[dom]));
        }
        out[f] = (Tout)v;
    }
}

// order-0 / order-1 blend along one axis: in (outer, n_in, inner) fp64 -> out (outer, n_out, inner) fp32
__global__ void __launch_bounds__(PP_BLOCK) pp_gather_kernel(const double *__restrict__ in, float *__restrict__ out, long long inner,
                                                             int n_in, int n_out, const int *__restrict__ idx,
                                                             const double *__restrict__ w, long long M)
{
#pragma clang fp contract(off)
    const long long f = (long long)blockIdx.x * PP_BLOCK + threadIdx.x;
    if (f >= M) return;
    const long long r = f / inner;
    const long long t = f - r * inner;
    const int o = (int)(r % n_out);
    const long long ob = r / n_out;
    const double *base = in + ob * n_in * inner + t;
    out[f] = (float)(base[(long long)idx[2 * o] * inner] * w[2 * o] + base[(long long)idx[2 * o + 1] * inner] * w[2 * o + 1]);
}

int grid_of(long long n, long long per, unsigned *grid)
{
    const long long b = (n + per - 1) / per;
    if (b < 1 || b > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    *grid = (unsigned)b;
    return 0;
}

int check_src(const float *in, int C, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz)
{
    if (!in) return MLAGG_E_NULLPTR;
    if (C < 1 || X < 1 || Y < 1 || Z < 1 || sc < 0 || sx < 0 || sy < 0 || sz < 0) return MLAGG_E_UNSUPPORTED;
    return 0;
}

int check_window(int X, int Y, int Z, const int *lo, const int *ext, Window *w)
{
    if (!lo || !ext) return MLAGG_E_NULLPTR;
    const int sh[3] = {X, Y, Z};
    for (int d = 0; d < 3; ++d) {
        if (lo[d] < 0 || ext[d] < 1 || lo[d] + ext[d] > sh[d]) return MLAGG_E_UNSUPPORTED;
        w->lo[d] = lo[d];
        w->ext[d] = ext[d];
    }
    return 0;
}

}  // namespace

extern "C" int mlagg_pp_cubic_lines_per_block(int n_in, int M)
{
    if (n_in < 1 || M < 1) return 0;
    const long long per_line = 8LL * (n_in + M);
    int ti = 0;
    for (int t = 1; t <= 32; t *= 2)
        if (t * per_line <= PP_LDS_BYTES) ti = t;
    return ti;
}

extern "C" int mlagg_pp_nonzero_box(const float *in, int C, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz,
                                    int *box, void *stream)
{
    if (int rc = check_src(in, C, X, Y, Z, sc, sx, sy, sz)) return rc;
    if (!box) return MLAGG_E_NULLPTR;
    const long long N = (long long)C * X * Y * Z;
    unsigned grid;
    if (int rc = grid_of(N, PP_BLOCK * 8LL, &grid)) return rc;
    grid = grid > 4096u ? 4096u : grid;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_PP_BOX, st);
    hipLaunchKernelGGL(pp_box_init_kernel, dim3(1), dim3(64), 0, st, box);
    hipLaunchKernelGGL(pp_box_kernel, dim3(grid), dim3(PP_BLOCK), 0, st, Src{in, sc, sx, sy, sz}, X, Y, Z, N, box);
    return (int)hipGetLastError();
}

extern "C" int mlagg_pp_channel_stats(const float *in, int C, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz,
                                      const int *lo, const int *ext, int c, int scheme, const unsigned char *mask, double *partials,
                                      float *params, double *stats, void *stream)
{
    if (int rc = check_src(in, C, X, Y, Z, sc, sx, sy, sz)) return rc;
    Window w;
    if (int rc = check_window(X, Y, Z, lo, ext, &w)) return rc;
    if (!partials || !params || !stats) return MLAGG_E_NULLPTR;
    if (c < 0 || c >= C || (scheme == MLAGG_PP_ZSCORE_MASKED && !mask)) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_PP_STATS, st);
    const Src s{in, sc, sx, sy, sz};
    const uint8_t *m = scheme == MLAGG_PP_ZSCORE_MASKED ? reinterpret_cast<const uint8_t *>(mask) : nullptr;
    hipLaunchKernelGGL(pp_stats_kernel, dim3(PP_STATS_BLOCKS), dim3(PP_BLOCK), 0, st, s, w, c, m, partials);
    hipLaunchKernelGGL(pp_stats_final_kernel, dim3(1), dim3(1), 0, st, partials, s, w, c, scheme, params, stats);
    return (int)hipGetLastError();
}

extern "C" int mlagg_pp_normalize(const float *in, int C, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz,
                                  const int *lo, const int *ext, const int *schemes, const float *params, const unsigned char *mask,
                                  float *out, void *stream)
{
    if (int rc = check_src(in, C, X, Y, Z, sc, sx, sy, sz)) return rc;
    Window w;
    if (int rc = check_window(X, Y, Z, lo, ext, &w)) return rc;
    if (!schemes || !params || !out) return MLAGG_E_NULLPTR;
    const long long V = (long long)w.ext[0] * w.ext[1] * w.ext[2];
    unsigned grid;
    if (int rc = grid_of(V * C, PP_BLOCK, &grid)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_PP_NORMALIZE, st);
    hipLaunchKernelGGL(pp_normalize_kernel, dim3(grid), dim3(PP_BLOCK), 0, st, Src{in, sc, sx, sy, sz}, w, C, schemes, params,
                       reinterpret_cast<const uint8_t *>(mask), out, V);
    return (int)hipGetLastError();
}

extern "C" int mlagg_pp_clip_ranges(const float *x, int C, int X, int Y, int Z, int axis, unsigned *lo, unsigned *hi, void *stream)
{
    if (!x || !lo || !hi) return MLAGG_E_NULLPTR;
    if (C < 1 || X < 1 || Y < 1 || Z < 1 || axis < -1 || axis > 2) return MLAGG_E_UNSUPPORTED;
    const int sh[3] = {X, Y, Z};
    const long long V = (long long)X * Y * Z;
    const int D = axis < 0 ? 1 : sh[axis];
    const long long inner = axis < 0 ? V : (axis == 0 ? (long long)Y * Z : (axis == 1 ? (long long)Z : 1LL));
    const long long P = V / D;
    long long chunks = (P + 16LL * PP_BLOCK - 1) / (16LL * PP_BLOCK);
    chunks = chunks > 64 ? 64 : chunks;
    if ((long long)C * D * chunks > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_PP_MINMAX, st);
    (void)hipMemsetAsync(lo, 0xff, sizeof(unsigned) * C * D, st);
    (void)hipMemsetAsync(hi, 0, sizeof(unsigned) * C * D, st);
    hipLaunchKernelGGL(pp_minmax_kernel, dim3((unsigned)(C * D * chunks)), dim3(PP_BLOCK), 0, st, x, V, D, inner, (int)chunks, lo, hi);
    return (int)hipGetLastError();
}

extern "C" int mlagg_pp_cubic_axis(const void *in, int in_f64, void *out, int out_f64, long long outer, int n_in, long long inner,
                                   int n_out, const int *start, const double *w, int P0, int M, const double *fir,
                                   const unsigned *clip_lo, const unsigned *clip_hi, long long clip_cstride, long long clip_dstride,
                                   int clip_D, void *stream)
{
    if (!in || !out || !start || !w || !fir) return MLAGG_E_NULLPTR;
    if (outer < 1 || inner < 1 || n_in < 1 || n_out < 1 || M < 4 || P0 < 0) return MLAGG_E_UNSUPPORTED;
    if (P0 + M > n_in + 2 * PP_PAD) return MLAGG_E_UNSUPPORTED;                    // taps inside the padded line
    if ((clip_lo == nullptr) != (clip_hi == nullptr)) return MLAGG_E_NULLPTR;
    if (clip_lo && (clip_cstride < 1 || clip_dstride < 1 || clip_D < 1)) return MLAGG_E_UNSUPPORTED;
    const int TI = mlagg_pp_cubic_lines_per_block(n_in, M);
    if (TI < 1) return MLAGG_E_UNSUPPORTED;                                       // the line does not fit the LDS plan
    const long long blocks = inner > 1 ? outer * ((inner + TI - 1) / TI) : (outer + TI - 1) / TI;
    if (blocks > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    Fir f;
    for (int k = 0; k <= PP_FIR; ++k) f.h[k] = fir[k];
    const Clip clip{clip_lo, clip_hi, clip_cstride, clip_dstride, clip_D};
    const size_t lds = sizeof(double) * (size_t)TI * (n_in + M);
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_PP_CUBIC, st);
    const dim3 grid((unsigned)blocks), block(PP_BLOCK);
    if (!in_f64 && out_f64)
        hipLaunchKernelGGL((pp_cubic_kernel<float, double>), grid, block, lds, st, static_cast<const float *>(in),
                           static_cast<double *>(out), outer, inner, n_in, n_out, TI, start, w, P0, M, f, clip);
    else if (in_f64 && out_f64)
        hipLaunchKernelGGL((pp_cubic_kernel<double, double>), grid, block, lds, st, static_cast<const double *>(in),
                           static_cast<double *>(out), outer, inner, n_in, n_out, TI, start, w, P0, M, f, clip);
    else if (in_f64 && !out_f64)
        hipLaunchKernelGGL((pp_cubic_kernel<double, float>), grid, block, lds, st, static_cast<const double *>(in),
                           static_cast<float *>(out), outer, inner, n_in, n_out, TI, start, w, P0, M, f, clip);
    else
        hipLaunchKernelGGL((pp_cubic_kernel<float, float>), grid, block, lds, st, static_cast<const float *>(in),
                           static_cast<float *>(out), outer, inner, n_in, n_out, TI, start, w, P0, M, f, clip);
    return (int)hipGetLastError();
}

extern "C" int mlagg_pp_gather_axis(const double *in, float *out, long long outer, int n_in, long long inner, int n_out, const int *idx,
                                    const double *w, void *stream)
{
    if (!in || !out || !idx || !w) return MLAGG_E_NULLPTR;
    if (outer < 1 || inner < 1 || n_in < 1 || n_out < 1) return MLAGG_E_UNSUPPORTED;
    const long long M = outer * n_out * inner;
    unsigned grid;
    if (int rc = grid_of(M, PP_BLOCK, &grid)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_PP_GATHER, st);
    hipLaunchKernelGGL(pp_gather_kernel, dim3(grid), dim3(PP_BLOCK), 0, st, in, out, inner, n_in, n_out, idx, w, M);
    return (int)hipGetLastError();
}
