// K24 -- normalized surface Dice (NSD) on the device.
//
// What it replaces: evaluation/SurfaceDice.py compute_surface_distances (:280-425) followed by compute_surface_dice_at_tolerance
// (:470-479), called once per organ by the *_NSD_Eval.py scripts.  Per organ the reference crops the union bounding box with one zero
// plane on the high side of every axis, computes the 2x2x2 neighbour code of every voxel with scipy.ndimage.correlate (an even kernel
// has its origin at index 1, so voxel p reads the masks at p-1 .. p), marks the codes other than 0 and 255 as surface voxels ("surfels"),
// runs two float64 distance_transform_edt over the complements of the surfel sets, and sums the per-code areas of the surfels whose
// distance to the other surface is <= tol.
//
// Here every label of a case is handled by the same launches; each label has a crop (origin, mask extents n, dims D = n + 1) laid
// end to end in one workspace, and a kernel finds its label by a binary search over the crops' offsets.
//   sf_init_kernel / sf_stats_kernel   one pass over the two label volumes: per label the gt and prediction voxel counts, the union
//                      bounding box and the gt's z range (run-length per thread, LDS atomics, one global atomic per block and slot);
//                      the host reads these 256 x 10 ints back once and lays out the crops;
//   sf_codes_kernel    gt and prediction neighbour codes of every crop voxel (reads outside the mask extents are 0, which is also how a
//                      slab organ's cut to [z_lower, z_upper) is applied), plus integer counts of the surfels;
//   sf_zpass_kernel    exact Euclidean feature transform, pass 1: one wave per line along the contiguous axis, the nearest surfel by a
//                      wave prefix-max / suffix-min scan;
//   sf_ypass_kernel    pass 2: one wave per line along y, Felzenszwalb-Huttenlocher lower envelope of the parabolas
//                      s1^2 (y - q)^2 + ((z - fz(q)) s2)^2 in float64, built in LDS; writes the nearest feature's packed (y, z);
//   sf_xpass_kernel    pass 3: the same along x for one feature set, evaluated only at the other mask's surfels: the distance is
//                      scipy's sqrt(((dx s0)^2 + (dy s1)^2) + (dz s2)^2) from the integer feature offset (no FMA contraction), and the
//                      line's surfel area and area within tol are summed in a fixed lane order into one partial per line; optionally
//                      every (distance, area) pair is appended to a per-label list (compute_surface_distances sorts them afterwards);
//   sf_sum_kernel      per label and direction a fixed-order sum of the line partials: a repeated call is bit-identical.
// A set without surfels leaves every distance at +inf, as the reference's np.Inf map does.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mlagg_hip.h"
#include "prof.h"

namespace {

constexpr int SF_STATS_BLOCK = 256;
constexpr int SF_SEG = 16;                    // z voxels per thread in sf_stats_kernel
constexpr int SF_NSLOT = MLAGG_SURFACE_STATS_PER_LABEL;
constexpr int SF_DESC = MLAGG_SURFACE_DESC_FIELDS;
constexpr int SF_WAVE = 64;
constexpr int SF_GRID_CAP = 1 << 20;          // grid-stride loops above this many workgroups
constexpr int SF_MAX_LABELS = 255;

// desc fields (int64 each, per label)
enum { D_LABEL = 0, D_O0, D_O1, D_O2, D_N0, D_N1, D_N2, D_VOX, D_ZL, D_YL, D_XL, D_PAIR_GT, D_PAIR_PRED };

struct Crop {
    int label;
    int o0, o1, o2;
    int n0, n1, n2;
    int D0, D1, D2;
    long long vox;
};

__device__ __forceinline__ Crop crop_of(const long long *desc, int i)
{
    const long long *d = desc + (long long)i * SF_DESC;
    Crop c;
    c.label = (int)d[D_LABEL];
    c.o0 = (int)d[D_O0];
    c.o1 = (int)d[D_O1];
    c.o2 = (int)d[D_O2];
    c.n0 = (int)d[D_N0];
    c.n1 = (int)d[D_N1];
    c.n2 = (int)d[D_N2];
    c.D0 = c.n0 + 1;
    c.D1 = c.n1 + 1;
    c.D2 = c.n2 + 1;
    c.vox = d[D_VOX];
    return c;
}

// the last label whose range (desc field f) starts at or before idx
__device__ __forceinline__ int find_label(const long long *desc, int nl, int f, long long idx)
{
    int lo = 0, hi = nl - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(long long)mid * SF_DESC + f] <= idx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool is_border(uint8_t c)
{
    return c != 0 && c != 255;
}

// --------------------------------------------------------------------------------------------------------------------------------
// per-label statistics
// --------------------------------------------------------------------------------------------------------------------------------
__global__ void sf_init_kernel(int *stats)
{
    const int l = threadIdx.x;
    int *s = stats + l * SF_NSLOT;
    s[0] = 0, s[1] = 0;
    s[2] = 0x7fffffff, s[3] = -1, s[4] = 0x7fffffff, s[5] = -1, s[6] = 0x7fffffff, s[7] = -1;
    s[8] = 0x7fffffff, s[9] = -1;
}

__device__ __forceinline__ void flush_run(int *h, int lab, int n, int x, int y, int z0, int z1, bool gt)
{
    int *s = h + lab * SF_NSLOT;
    atomicAdd(&s[gt ? 0 : 1], n);
    atomicMin(&s[2], x), atomicMax(&s[3], x);
    atomicMin(&s[4], y), atomicMax(&s[5], y);
    atomicMin(&s[6], z0), atomicMax(&s[7], z1);
    if (gt) atomicMin(&s[8], z0), atomicMax(&s[9], z1);
}

__global__ void __launch_bounds__(SF_STATS_BLOCK) sf_stats_kernel(const uint8_t *__restrict__ gt, const uint8_t *__restrict__ pred,
                                                                  int X, int Y, int Z, const uint8_t *__restrict__ wanted,
                                                                  int *__restrict__ stats)
{
    __shared__ int h[256 * SF_NSLOT];
    __shared__ uint8_t want[256];
    const int t = threadIdx.x;
    want[t] = wanted[t];
    {
        int *s = h + t * SF_NSLOT;
        s[0] = 0, s[1] = 0;
        s[2] = 0x7fffffff, s[3] = -1, s[4] = 0x7fffffff, s[5] = -1, s[6] = 0x7fffffff, s[7] = -1;
        s[8] = 0x7fffffff, s[9] = -1;
    }
    __syncthreads();
    const int nseg = (Z + SF_SEG - 1) / SF_SEG;
    const long long work = (long long)X * Y * nseg;
    const long long stride = (long long)gridDim.x * SF_STATS_BLOCK;
    for (long long w = (long long)blockIdx.x * SF_STATS_BLOCK + t; w < work; w += stride) {
        const long long row = w / nseg;
        const int z0 = (int)(w - row * nseg) * SF_SEG;
        const int z1 = min(Z, z0 + SF_SEG);
        const int x = (int)(row / Y), y = (int)(row % Y);
        const long long base = row * Z;
        int cg = 0, ng = 0, sg = z0, cp = 0, np = 0, sp = z0;
        for (int z = z0; z < z1; ++z) {
            const int g = gt[base + z], p = pred[base + z];
            if (g != cg) {
                if (ng && want[cg]) flush_run(h, cg, ng, x, y, sg, z - 1, true);
                cg = g, ng = 0, sg = z;
            }
            ++ng;
            if (p != cp) {
                if (np && want[cp]) flush_run(h, cp, np, x, y, sp, z - 1, false);
                cp = p, np = 0, sp = z;
            }
            ++np;
        }
        if (ng && want[cg]) flush_run(h, cg, ng, x, y, sg, z1 - 1, true);
        if (np && want[cp]) flush_run(h, cp, np, x, y, sp, z1 - 1, false);
    }
    __syncthreads();
    const int *s = h + t * SF_NSLOT;
    if (s[0] == 0 && s[1] == 0) return;
    int *g = stats + t * SF_NSLOT;
    if (s[0]) atomicAdd(&g[0], s[0]);
    if (s[1]) atomicAdd(&g[1], s[1]);
    atomicMin(&g[2], s[2]), atomicMax(&g[3], s[3]);
    atomicMin(&g[4], s[4]), atomicMax(&g[5], s[5]);
    atomicMin(&g[6], s[6]), atomicMax(&g[7], s[7]);
    if (s[0]) atomicMin(&g[8], s[8]), atomicMax(&g[9], s[9]);
}

// --------------------------------------------------------------------------------------------------------------------------------
// neighbour codes
// --------------------------------------------------------------------------------------------------------------------------------
struct Volumes {
    const uint8_t *gt, *pred;
    int X, Y, Z;
};

__global__ void __launch_bounds__(256) sf_codes_kernel(Volumes V, const long long *__restrict__ desc, int nl, long long total,
                                                       uint8_t *__restrict__ codes, int *__restrict__ counts)
{
    const long long stride = (long long)gridDim.x * 256;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total; v += stride) {
        const int i = find_label(desc, nl, D_VOX, v);
        const Crop c = crop_of(desc, i);
        const long long r = v - c.vox;
        const int z = (int)(r % c.D2);
        const long long q = r / c.D2;
        const int y = (int)(q % c.D1), x = (int)(q / c.D1);
        int cg = 0, cp = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int a = x - 1 + (k >> 2), b = y - 1 + ((k >> 1) & 1), e = z - 1 + (k & 1);
            if (a < 0 || b < 0 || e < 0 || a >= c.n0 || b >= c.n1 || e >= c.n2) continue;
            const long long o = ((long long)(c.o0 + a) * V.Y + (c.o1 + b)) * V.Z + (c.o2 + e);
            const int bit = 1 << (7 - k);                // kernel [[[128,64],[32,16]],[[8,4],[2,1]]]: corner (i,j,k) -> 2^(7-(4i+2j+k))
            if (V.gt[o] == c.label) cg |= bit;
            if (V.pred[o] == c.label) cp |= bit;
        }
        codes[v] = (uint8_t)cg;
        codes[total + v] = (uint8_t)cp;
        // surfel counts: one atomic per wave where the active lanes share a label, else per lane
        const unsigned long long act = __ballot(1);
        const int first = __ffsll((long long)act) - 1;
        const unsigned long long bg = __ballot(is_border((uint8_t)cg)), bp = __ballot(is_border((uint8_t)cp));
        if (__all(i == __shfl(i, first, SF_WAVE))) {
            if ((int)(threadIdx.x & (SF_WAVE - 1)) == first) {
                if (bg) atomicAdd(&counts[2 * i], __popcll(bg));
                if (bp) atomicAdd(&counts[2 * i + 1], __popcll(bp));
            }
        } else {
            if (is_border((uint8_t)cg)) atomicAdd(&counts[2 * i], 1);
            if (is_border((uint8_t)cp)) atomicAdd(&counts[2 * i + 1], 1);
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------------------
// pass 1: nearest surfel along z (one wave per line, both masks)
// --------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sf_zpass_kernel(const uint8_t *__restrict__ codes, const long long *__restrict__ desc, int nl,
                                                       long long total, long long zlines, int *__restrict__ ft)
{
    const int lane = threadIdx.x & (SF_WAVE - 1);
    const long long waves = (long long)gridDim.x * (256 / SF_WAVE);
    for (long long w = (long long)blockIdx.x * (256 / SF_WAVE) + (threadIdx.x / SF_WAVE); w < 2 * zlines; w += waves) {
        const int m = w >= zlines;
        const long long gl = w - (m ? zlines : 0);
        const int i = find_label(desc, nl, D_ZL, gl);
        const Crop c = crop_of(desc, i);
        const long long l = gl - desc[(long long)i * SF_DESC + D_ZL];
        const long long base = c.vox + l * c.D2;        // line (x, y) = (l / D1, l % D1), contiguous along z
        const uint8_t *cd = codes + (long long)m * total + base;
        int *out = ft + (long long)m * total + base;
        // forward: the last surfel at or before z
        int carry = -1;
        for (int z0 = 0; z0 < c.D2; z0 += SF_WAVE) {
            const int z = z0 + lane;
            int v = (z < c.D2 && is_border(cd[z])) ? z : -1;
            for (int d = 1; d < SF_WAVE; d <<= 1) {
                const int u = __shfl_up(v, d, SF_WAVE);
                if (lane >= d) v = max(v, u);
            }
            v = max(v, carry);
            if (z < c.D2) out[z] = v;
            carry = __shfl(v, SF_WAVE - 1, SF_WAVE);
        }
        // backward: the first surfel at or after z; keep the nearer one (a tie is equally near)
        carry = 0x7fffffff;
        const int last = ((c.D2 - 1) / SF_WAVE) * SF_WAVE;
        for (int z0 = last; z0 >= 0; z0 -= SF_WAVE) {
            const int z = z0 + lane;
            int v = (z < c.D2 && is_border(cd[z])) ? z : 0x7fffffff;
            for (int d = 1; d < SF_WAVE; d <<= 1) {
                const int u = __shfl_down(v, d, SF_WAVE);
                if (lane + d < SF_WAVE) v = min(v, u);
            }
            v = min(v, carry);
            if (z < c.D2) {
                const int prev = out[z];
                int f = -1;
                if (prev >= 0 && (v == 0x7fffffff || z - prev <= v - z)) f = prev;
                else if (v != 0x7fffffff) f = v;
                out[z] = f;
            }
            carry = __shfl(v, 0, SF_WAVE);
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------------------
// lower envelope of the parabolas w (p - q)^2 + f(q) over the sites of one line, in LDS (lane 0 builds it, all lanes query it)
// --------------------------------------------------------------------------------------------------------------------------------
struct Env {
    double *f;      // [n] key of each position, +inf where there is no site
    int *aux;       // [n] the site's feature (packed coordinates)
    int *v;         // [n] envelope sites
    double *zb;     // [n + 1] breakpoints
};

__device__ __forceinline__ Env env_of(unsigned char *lds, int nmax)
{
    Env e;
    e.f = reinterpret_cast<double *>(lds);
    e.zb = e.f + nmax;
    e.aux = reinterpret_cast<int *>(e.zb + nmax + 1);
    e.v = e.aux + nmax;
    return e;
}

// returns the number of parabolas in the envelope
__device__ int env_build(const Env &e, int n, double w)
{
    int k = -1;
    for (int q = 0; q < n; ++q) {
        const double fq = e.f[q];
        if (isinf(fq)) continue;
        const double hq = fq + w * (double)q * (double)q;
        if (k < 0) {
            k = 0;
            e.v[0] = q;
            e.zb[0] = -INFINITY;
            continue;
        }
        double s;
        while (true) {
            const int p = e.v[k];
            s = (hq - (e.f[p] + w * (double)p * (double)p)) / (2.0 * w * (double)(q - p));
            if (k > 0 && s <= e.zb[k]) --k;
            else break;
        }
        ++k;
        e.v[k] = q;
        e.zb[k] = s;
    }
    return k + 1;
}

// the envelope's site nearest to position x (K >= 1)
__device__ __forceinline__ int env_query(const Env &e, int K, int x)
{
    int lo = 0, hi = K - 1;                        // the largest k with zb[k] <= x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (e.zb[mid] <= (double)x) lo = mid;
        else hi = mid - 1;
    }
    return e.v[lo];
}

// --------------------------------------------------------------------------------------------------------------------------------
// pass 2: along y; ft (x, y, z) = nearest z  ->  packed fy * D2 + fz, in place
// --------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SF_WAVE) sf_ypass_kernel(const long long *__restrict__ desc, int nl, long long total, long long ylines,
                                                           int nmax, double s1, double s2, int *__restrict__ ft)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sf_lds[];
    const Env e = env_of(sf_lds, nmax);
    __shared__ int nenv;
    const int lane = threadIdx.x;
    const double w = s1 * s1;
    for (long long b = blockIdx.x; b < 2 * ylines; b += gridDim.x) {
        const int m = b >= ylines;
        const long long gl = b - (m ? ylines : 0);
        const int i = find_label(desc, nl, D_YL, gl);
        const Crop c = crop_of(desc, i);
        const long long l = gl - desc[(long long)i * SF_DESC + D_YL];
        const int x = (int)(l / c.D2), z = (int)(l % c.D2);
        int *line = ft + (long long)m * total + c.vox + (long long)x * c.D1 * c.D2 + z;    // stride D2 along y
        for (int y = lane; y < c.D1; y += SF_WAVE) {
            const int fz = line[(long long)y * c.D2];
            double f = INFINITY;
            if (fz >= 0) {
                const double dz = (double)(z - fz) * s2;
                f = dz * dz;
            }
            e.f[y] = f;
            e.aux[y] = fz;
        }
        __syncthreads();
        if (lane == 0) nenv = env_build(e, c.D1, w);
        __syncthreads();
        const int K = nenv;
        for (int y = lane; y < c.D1; y += SF_WAVE) {
            int out = -1;
            if (K > 0) {
                const int q = env_query(e, K, y);
                out = q * c.D2 + e.aux[q];
            }
            line[(long long)y * c.D2] = out;
        }
        __syncthreads();
    }
}

// --------------------------------------------------------------------------------------------------------------------------------
// pass 3: along x, evaluated at the other mask's surfels, with the per-line sums
// --------------------------------------------------------------------------------------------------------------------------------
struct Reduce {
    const uint8_t *codes;
    const int *ft;
    const long long *desc;
    const double *tol;
    const double *area;
    double *partial;        // [2][xlines][2]: surfel area, area within tol
    double *pairs;          // optional: (distance, area) pairs at desc[D_PAIR_GT / D_PAIR_PRED] + counter
    int *pair_count;        // [nl][2]
    long long total, xlines;
    int nl, nmax;
    double s0, s1, s2;
};

__device__ __forceinline__ double surface_distance(int dx, int dy, int dz, double s0, double s1, double s2)
{
#pragma clang fp contract(off)
    const double a = (double)dx * s0, b = (double)dy * s1, c = (double)dz * s2;
    return sqrt((a * a + b * b) + c * c);             // scipy: dt *= sampling; dt *= dt; add.reduce over the axes; sqrt
}

__global__ void __launch_bounds__(SF_WAVE) sf_xpass_kernel(Reduce R)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sf_lds[];
    const Env e = env_of(sf_lds, R.nmax);
    __shared__ int nenv;
    __shared__ double sarea[256];
    const int lane = threadIdx.x;
    for (int k = lane; k < 256; k += SF_WAVE) sarea[k] = R.area[k];
    const double w = R.s0 * R.s0;
    for (long long b = blockIdx.x; b < 2 * R.xlines; b += gridDim.x) {
        const int dir = b >= R.xlines;                 // 0: gt surfels against the prediction's surface, 1: the reverse
        const int fm = 1 - dir;                        // feature set
        const long long gl = b - (dir ? R.xlines : 0);
        const int i = find_label(R.desc, R.nl, D_XL, gl);
        const Crop c = crop_of(R.desc, i);
        const long long l = gl - R.desc[(long long)i * SF_DESC + D_XL];
        const int y = (int)(l / c.D2), z = (int)(l % c.D2);
        const long long plane = (long long)c.D1 * c.D2;
        const long long off = c.vox + (long long)y * c.D2 + z;                 // stride plane along x
        const int *line = R.ft + (long long)fm * R.total + off;
        const uint8_t *q = R.codes + (long long)dir * R.total + off;
        for (int x = lane; x < c.D0; x += SF_WAVE) {
            const int p = line[(long long)x * plane];
            double f = INFINITY;
            if (p >= 0) {
                const double dy = (double)(y - p / c.D2) * R.s1, dz = (double)(z - p % c.D2) * R.s2;
                f = dy * dy + dz * dz;
            }
            e.f[x] = f;
            e.aux[x] = p;
        }
        __syncthreads();
        if (lane == 0) nenv = env_build(e, c.D0, w);
        __syncthreads();
        const int K = nenv;
        const double tol = R.tol[i];
        double sa = 0.0, sw = 0.0;
        for (int x = lane; x < c.D0; x += SF_WAVE) {
            const uint8_t code = q[(long long)x * plane];
            if (!is_border(code)) continue;
            double d = INFINITY;
            if (K > 0) {
                const int fx = env_query(e, K, x);
                const int p = e.aux[fx];
                d = surface_distance(fx - x, p / c.D2 - y, p % c.D2 - z, R.s0, R.s1, R.s2);
            }
            const double a = sarea[code];
            sa += a;
            if (d <= tol) sw += a;
            if (R.pairs) {
                const long long at = R.desc[(long long)i * SF_DESC + (dir ? D_PAIR_PRED : D_PAIR_GT)] +
                                     atomicAdd(&R.pair_count[2 * i + dir], 1);
                R.pairs[2 * at] = d;
                R.pairs[2 * at + 1] = a;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            sa += __shfl_xor(sa, o, SF_WAVE);
            sw += __shfl_xor(sw, o, SF_WAVE);
        }
        if (lane == 0) {
            R.partial[2 * b] = sa;
            R.partial[2 * b + 1] = sw;
        }
        __syncthreads();
    }
}

// per label and direction: sums[4 * i + 2 * dir + {0, 1}] = fixed-order sum of the label's line partials
__global__ void __launch_bounds__(256) sf_sum_kernel(const double *__restrict__ partial, const long long *__restrict__ desc, int nl,
                                                     long long xlines, double *__restrict__ sums)
{
    __shared__ double red[2][256];
    const int i = blockIdx.x >> 1, dir = blockIdx.x & 1, t = threadIdx.x;
    const long long l0 = desc[(long long)i * SF_DESC + D_XL];
    const long long l1 = i + 1 < nl ? desc[(long long)(i + 1) * SF_DESC + D_XL] : xlines;
    const double *p = partial + 2 * ((long long)dir * xlines);
    double a = 0.0, b = 0.0;
    for (long long l = l0 + t; l < l1; l += 256) {
        a += p[2 * l];
        b += p[2 * l + 1];
    }
    red[0][t] = a;
    red[1][t] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            red[0][t] += red[0][t + s];
            red[1][t] += red[1][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        sums[4 * i + 2 * dir] = red[0][0];
        sums[4 * i + 2 * dir + 1] = red[1][0];
    }
}

__host__ size_t env_lds_bytes(int nmax)
{
    return (size_t)nmax * (sizeof(double) + 2 * sizeof(int)) + (size_t)(nmax + 1) * sizeof(double);
}

unsigned grid_of(long long n)
{
    return (unsigned)(n < SF_GRID_CAP ? (n > 0 ? n : 1) : SF_GRID_CAP);
}

}  // namespace

extern "C" int mlagg_surface_stats(const unsigned char *gt, const unsigned char *pred, int X, int Y, int Z, const unsigned char *wanted,
                                   int *stats, void *stream)
{
    if (X < 1 || Y < 1 || Z < 1) return MLAGG_E_UNSUPPORTED;
    if (!gt || !pred || !wanted || !stats) return MLAGG_E_NULLPTR;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long work = (long long)X * Y * ((Z + SF_SEG - 1) / SF_SEG);
    {
        MLAGG_TIMED(K_SF_STATS, st);
        hipLaunchKernelGGL(sf_init_kernel, dim3(1), dim3(256), 0, st, stats);
        const long long blocks = (work + SF_STATS_BLOCK - 1) / SF_STATS_BLOCK;
        // at most 2048 blocks: each block ends in up to 256 x 10 global atomics
        hipLaunchKernelGGL(sf_stats_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(SF_STATS_BLOCK), 0, st, gt, pred,
                           X, Y, Z, wanted, stats);
    }
    return (int)hipGetLastError();
}

extern "C" int mlagg_surface_prepare(const unsigned char *gt, const unsigned char *pred, int X, int Y, int Z, const long long *desc,
                                     int n_labels, long long total, long long max_crop, long long zlines, long long ylines,
                                     int nmax_y, double s1, double s2, unsigned char *codes, int *ft, int *counts, void *stream)
{
    if (X < 1 || Y < 1 || Z < 1 || n_labels < 1 || n_labels > SF_MAX_LABELS || total < 1) return MLAGG_E_UNSUPPORTED;
    if (max_crop < 1 || max_crop > 2147483647LL) return MLAGG_E_UNSUPPORTED;
    if (nmax_y < 1 || nmax_y > MLAGG_SURFACE_MAX_LINE) return MLAGG_E_UNSUPPORTED;
    if (!gt || !pred || !desc || !codes || !ft || !counts) return MLAGG_E_NULLPTR;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipError_t e = hipMemsetAsync(counts, 0, 2 * n_labels * sizeof(int), st)) return (int)e;
    const Volumes V{gt, pred, X, Y, Z};
    {
        MLAGG_TIMED(K_SF_CODES, st);
        hipLaunchKernelGGL(sf_codes_kernel, dim3(grid_of((total + 255) / 256)), dim3(256), 0, st, V, desc, n_labels, total, codes,
                           counts);
    }
    {
        MLAGG_TIMED(K_SF_ZPASS, st);
        hipLaunchKernelGGL(sf_zpass_kernel, dim3(grid_of((2 * zlines + 3) / 4)), dim3(256), 0, st, codes, desc, n_labels, total,
                           zlines, ft);
    }
    {
        MLAGG_TIMED(K_SF_YPASS, st);
        hipLaunchKernelGGL(sf_ypass_kernel, dim3(grid_of(2 * ylines)), dim3(SF_WAVE), env_lds_bytes(nmax_y), st, desc, n_labels,
                           total, ylines, nmax_y, s1, s2, ft);
    }
    return (int)hipGetLastError();
}

extern "C" int mlagg_surface_reduce(const unsigned char *codes, const int *ft, const long long *desc, int n_labels, long long total,
                                    long long xlines, int nmax_x, const double *tol, const double *area, double s0, double s1,
                                    double s2, double *partial, double *sums, double *pairs, int *pair_count, void *stream)
{
    if (n_labels < 1 || n_labels > SF_MAX_LABELS || total < 1 || xlines < 1) return MLAGG_E_UNSUPPORTED;
    if (nmax_x < 1 || nmax_x > MLAGG_SURFACE_MAX_LINE) return MLAGG_E_UNSUPPORTED;
    if (!codes || !ft || !desc || !tol || !area || !partial || !sums) return MLAGG_E_NULLPTR;
    if (pairs && !pair_count) return MLAGG_E_NULLPTR;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pairs)
        if (hipError_t e = hipMemsetAsync(pair_count, 0, 2 * n_labels * sizeof(int), st)) return (int)e;
    Reduce R;
    R.codes = codes;
    R.ft = ft;
    R.desc = desc;
    R.tol = tol;
    R.area = area;
    R.partial = partial;
    R.pairs = pairs;
    R.pair_count = pair_count;
    R.total = total;
    R.xlines = xlines;
    R.nl = n_labels;
    R.nmax = nmax_x;
    R.s0 = s0;
    R.s1 = s1;
    R.s2 = s2;
    {
        MLAGG_TIMED(K_SF_XPASS, st);
        hipLaunchKernelGGL(sf_xpass_kernel, dim3(grid_of(2 * xlines)), dim3(SF_WAVE), env_lds_bytes(nmax_x), st, R);
    }
    {
        MLAGG_TIMED(K_SF_SUM, st);
        hipLaunchKernelGGL(sf_sum_kernel, dim3(2 * n_labels), dim3(256), 0, st, partial, desc, n_labels, xlines, sums);
    }
    return (int)hipGetLastError();
}
