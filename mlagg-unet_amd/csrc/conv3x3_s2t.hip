// K19t -- the 3 x 3, stride-2, padding-1 transposed convolution of PatchExpand (nnUNetTrainer_MLAgg_2D_dt_MS.py:479-546, conv1 at
// :506-513) and its two gradients, on channel-major maps with the operand forms of K19 (opmode.h: three bf16 pieces for the fp32 step,
// one rounded operand in the 16-bit modes).
//
// Parity algebra.  y = conv_transpose2d(x, W, stride 2, padding 1) is (2H - 1) x (2W - 1); output row u = 2m reads tap ky = 1 of input
// row m, u = 2m - 1 reads ky = 0 of row m and ky = 2 of row m - 1 (columns alike).  So input pixel (m, n) owns four output pixels --
// (2m, 2n), (2m, 2n - 1), (2m - 1, 2n), (2m - 1, 2n - 1): the parity classes with 1, 2, 2 and 4 taps -- and every class reads only the
// shifts x[m - {0, 1}][n - {0, 1}].  The forward is one GEMM over the H x W input grid (rows = output channels, columns = input pixels,
// contraction = input channel) with nine (tap, class) products; a class with a negative output row or column is the pad's and is not
// stored.  The data gradient dx = conv2d(dy, W, stride 2, padding 1) is the same GEMM shape with rows = input channels, contraction =
// output channel, and tap (ky, kx) reading dy[2m - 1 + ky][2n - 1 + kx] (zero outside (2H - 1) x (2W - 1)).
//
// Forward / data gradient kernel (one template, MODE): K19's structure -- a lane owns one pixel of the input grid, a stage is one
// 16-channel block x one kernel row ky (three taps), the three taps' weights for the workgroup's 32 TO rows are shared by four waves in
// LDS (double-buffered, pre-split weight image [piece][tap][row][k] in the caller's workspace), the source elements a stage needs are
// loaded with buffer loads whose out-of-range offsets return 0 (no padded copies) and split ONCE.  Forward: kernel rows 0 and 1 read
// the same input row m (the pair x[m][n - 1], x[m][n] is split once and serves six taps), kernel row 2 reads row m - 1; tap kx = 0 / 1
// reads x[.][n] into column classes 2n - 1 / 2n, kx = 2 reads x[.][n - 1] into 2n - 1.  All four class accumulators live in the same
// wave, so the unequal tap counts per class cost nothing: every stage issues 3 taps x TO MFMA groups.  Data gradient: the three
// elements dy[2m - 1 + ky][2n - 1 .. 2n + 1] per kernel row, tap kx reads element kx; dy may be a strided view (the interior of the
// padded gradient).
//
// Weight gradient: dW[i][o][ky][kx] = sum_{b, m, n} x[b][i][m][n] dy[b][o][2m - 1 + ky][2n - 1 + kx].  Contraction = input pixels, in
// blocks of 16 consecutive pixels of ONE input row (the block's row and first column are wave-uniform: row validity per kernel row is
// a uniform branch); a wave owns 32 input x 32 output channels x the nine taps (144 accumulators).  Per block a lane reads its 8 x
// values (A, split once) and per kernel row the 17 dy values 2n - 1 .. 2n + 15 of its output channel: the 8 even columns are the
// kx = 1 operand, the 9 odd ones split as pairs give kx = 0 (pairs 0-3) and kx = 2 (the same pairs shifted by one element: one
// v_alignbit_b32 per dword).  Partials [part][i][o][tap] are summed in a fixed order (no atomics, run-to-run identical).
#include <hip/hip_runtime.h>

#include "mlagg_hip.h"
#include "prof.h"
#include "internal.h"
#include "opmode.h"

namespace {

constexpr unsigned OOB = 0x80000000u;          // a buffer offset past the 2 GB range of every resource here: the load returns 0
constexpr int WAVES = 4;

// img[q][t][r][k] = piece q of tap t of the (R x K) product matrix: forward (R = O, K = I) w[k][r][t], data gradient (R = I, K = O)
// w[r][k][t]; w is the layer's (I, O, 3, 3) weight in both
template <int DT>
__global__ void __launch_bounds__(256)
s2t_weight_image_kernel(const float *__restrict__ w, unsigned short *__restrict__ img, int R, int K, int dgrad)
{
    const int n = 9 * R * K;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int k = idx % K, r = (idx / K) % R, t = idx / (K * R);
    const float v = dgrad ? w[((size_t)r * K + k) * 9 + t] : w[((size_t)k * R + r) * 9 + t];
    unsigned short p[3];
    opmode::pieces<DT>(v, p);
#pragma unroll
    for (int q = 0; q < opmode::Form<DT>::NQ; ++q) img[(size_t)q * n + idx] = p[q];
}

struct S2Geom {
    int B, R, K, H, W, P;            // R = output rows of the product, K = contraction channels, H x W = the input grid, P = H W
    long src_batch, src_chan, src_row;   // source map (x or dy): floats between samples / channels / rows
    long dst_batch;                  // destination map (y or dx), contiguous channels and rows
};

// MODE 0: forward (source x, destination y (2H - 1) x (2W - 1)); MODE 1: data gradient (source dy, destination dx H x W)
template <int MODE, int TO, int DT>
__global__ void __launch_bounds__(64 * WAVES, 2)
s2t_gemm_kernel(const float *__restrict__ S, const unsigned short *__restrict__ Wimg, float *__restrict__ D, S2Geom g)
{
    constexpr int ROWS = 32 * TO;
    constexpr int NQ = opmode::Form<DT>::NQ, NT = opmode::Form<DT>::NT;
    constexpr int NE = MODE == 0 ? 2 : 3;               // source elements per stage: forward (n - 1, n), data gradient 2n - 1 .. 2n + 1
    constexpr int NC = MODE == 0 ? 4 : 1;               // accumulator classes
    constexpr int STAGE = 3 * NQ * ROWS * 2;            // uint4 per stage
    constexpr int WL = (STAGE + 64 * WAVES - 1) / (64 * WAVES);
    __shared__ u32x4 sW[2][STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, kh = lane >> 5;
    const int pnat = (blockIdx.x * WAVES + wave) * 32 + col, r0 = blockIdx.y * ROWS, b = blockIdx.z;
    const int pc = min(pnat, g.P - 1);                  // past the end of the grid: the last pixel again, nothing stored
    const int m = pc / g.W, n = pc - m * g.W;
    // Six partial products into one fp32 chain round 6 x 9 K times: on the data gradient of up_2 (9 x 384 terms) that was 2.5e-6 of the
    // output's max.  Where the registers allow, the five small products (2^-8 and less of the main one) sum in accumulators of their
    // own and the main chain rounds 9 K times: the error of a plain fp32 sum.
    constexpr bool SPLIT = NT == 6 && NC * TO <= 4;
    constexpr int NA = SPLIT ? 2 : 1;
    f32x16 acc[NA][NC][TO];
#pragma unroll
    for (int s = 0; s < NA; ++s)
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int a = 0; a < TO; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[s][c][a][r] = 0.f;
    // per kernel row ky and element e: the lane's byte offset (channel rows 8 kh .. of the block), OOB where the element is padding
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(S + (size_t)b * g.src_batch), 0, 0x7fffffff, 0x00020000);
    unsigned off[3][NE];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            int row, cl;
            bool ok;
            if constexpr (MODE == 0) {
                row = ky == 2 ? m - 1 : m;
                cl = n - 1 + e;
                ok = row >= 0 && cl >= 0;
            } else {
                row = 2 * m - 1 + ky;
                cl = 2 * n - 1 + e;
                ok = row >= 0 && row < 2 * g.H - 1 && cl >= 0 && cl < 2 * g.W - 1;
            }
            off[ky][e] = ok ? 4u * (unsigned)(8 * kh * g.src_chan + (long)row * g.src_row + cl) : OOB;
        }
    const size_t img = (size_t)9 * g.R * g.K, tstride = (size_t)g.R * g.K;
    const int nblk = g.K / 16, nstage = 3 * nblk;
    unsigned wsrc[WL];
#pragma unroll
    for (int i = 0; i < WL; ++i) {
        const int e = min(tid + 64 * WAVES * i, STAGE - 1);
        const int h = e & 1, row = (e >> 1) % ROWS, q = ((e >> 1) / ROWS) % NQ, tt = (e >> 1) / (NQ * ROWS);
        wsrc[i] = 2u * (unsigned)(q * img + tt * tstride + (size_t)min(r0 + row, g.R - 1) * g.K + 8 * h);
    }
    u32x4 wreg[WL];
#define S2T_WFETCH(S_)                                                                                                        \
    {                                                                                                                         \
        const int sc_ = min((S_), nstage - 1), blk_ = sc_ / 3, ky_ = sc_ - 3 * blk_;                                          \
        const char *base_ = reinterpret_cast<const char *>(Wimg + (size_t)(3 * ky_) * tstride + 16 * blk_);                  \
        _Pragma("unroll") for (int i_ = 0; i_ < WL; ++i_) wreg[i_] = *reinterpret_cast<const u32x4 *>(base_ + (size_t)wsrc[i_]); \
    }
#define S2T_WSTORE(BUF)                                                                                                       \
    {                                                                                                                         \
        _Pragma("unroll") for (int i_ = 0; i_ < WL; ++i_) sW[(BUF)][min(tid + 64 * WAVES * i_, STAGE - 1)] = wreg[i_];        \
    }
    float raw[2][NE][8];
    uint4 src[NE][3];
    // the forward's kernel row 1 reads what kernel row 0 read: no fetch, and the split source of row 0 is reused
    auto xfetch = [&](float (&R)[NE][8], int blk_, int ky) __attribute__((always_inline)) {
        if (MODE == 0 && ky == 1) return;
        const int blk = min(blk_, nblk - 1);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const unsigned so = 4u * (unsigned)((16 * blk + r) * g.src_chan);
#pragma unroll
            for (int e = 0; e < NE; ++e) R[e][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srs, off[ky][e], so, 0));
        }
    };
    auto consume = [&](const u32x4 *wst, const float (&R)[NE][8], int ky) __attribute__((always_inline)) {
        if (!(MODE == 0 && ky == 1)) {
#pragma unroll
            for (int e = 0; e < NE; ++e) opmode::split8<DT>(R[e], src[e]);
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            uint4 aq[TO][3];
#pragma unroll
            for (int a = 0; a < TO; ++a)
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const u32x4 v = wst[(kx * NQ + q) * ROWS * 2 + (32 * a + col) * 2 + kh];
                    aq[a][q] = make_uint4(v.x, v.y, v.z, v.w);
                }
            // forward: element 1 = x[.][n], element 0 = x[.][n - 1]; class = 2 (row class 2m) + (column class 2n)
            const int e = MODE == 0 ? (kx == 2 ? 0 : 1) : kx;
            const int c = MODE == 0 ? 2 * (ky == 1) + (kx == 1) : 0;
#pragma unroll
            for (int term = 0; term < NT; ++term)
#pragma unroll
                for (int a = 0; a < TO; ++a) {
                    f32x16 &d = acc[SPLIT && term < NT - 1 ? 1 : 0][c][a];          // the last term is hi . hi
                    d = opmode::mfma<DT>(aq[a][opmode::Form<DT>::termA(term)], src[e][opmode::Form<DT>::termB(term)], d);
                }
        }
    };
    auto stage = [&](int blk_, int ky, int par) __attribute__((always_inline)) {          // stage s = 3 blk + ky, par = s & 1
        S2T_WFETCH(3 * blk_ + ky + 1)
        xfetch(raw[par ^ 1], ky == 2 ? blk_ + 1 : blk_, ky == 2 ? 0 : ky + 1);
        consume(sW[par], raw[par], ky);
        S2T_WSTORE(par ^ 1)
        __syncthreads();
    };
    S2T_WFETCH(0)
    S2T_WSTORE(0)
    xfetch(raw[0], 0, 0);
    __syncthreads();
    int blk = 0;
#pragma unroll 1
    for (; blk + 2 <= nblk; blk += 2) {
#pragma unroll
        for (int r = 0; r < 3; ++r) stage(blk, r, r & 1);
#pragma unroll
        for (int r = 0; r < 3; ++r) stage(blk + 1, r, (r + 1) & 1);
    }
    if (blk < nblk) {
#pragma unroll
        for (int r = 0; r < 3; ++r) stage(blk, r, r & 1);
    }
#undef S2T_WFETCH
#undef S2T_WSTORE
    if (pnat >= g.P) return;
    if constexpr (SPLIT) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int a = 0; a < TO; ++a) acc[0][c][a] += acc[1][c][a];
    }
    if constexpr (MODE == 0) {
        const int OW = 2 * g.W - 1;
        const long OP = (long)(2 * g.H - 1) * OW;
        float *yb = D + (size_t)b * g.dst_batch;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int u = (c & 2) ? 2 * m : 2 * m - 1, v = (c & 1) ? 2 * n : 2 * n - 1;
            if (u < 0 || v < 0) continue;                    // the pad's row / column
#pragma unroll
            for (int a = 0; a < TO; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = r0 + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    if (o < g.R) yb[(size_t)o * OP + (long)u * OW + v] = acc[0][c][a][r];
                }
        }
    } else {
        float *xb = D + (size_t)b * g.dst_batch + pc;
#pragma unroll
        for (int a = 0; a < TO; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = r0 + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (o < g.R) xb[(size_t)o * g.P] = acc[0][0][a][r];
            }
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
struct SWGeom {
    int B, O, I, H, W, P;
    long x_batch, dy_batch, dy_chan, dy_row;
    int cw;                          // 16-pixel blocks per input row
    int per_part, nparts;            // blocks per partial sum, partial sums per sample
};

template <int DT>
__global__ void __launch_bounds__(64)
s2t_wgrad_kernel(const float *__restrict__ X, const float *__restrict__ dY, float *__restrict__ part, SWGeom g)
{
    constexpr int NQ = opmode::Form<DT>::NQ, NT = opmode::Form<DT>::NT;
    const int lane = threadIdx.x, col = lane & 31, kh = lane >> 5;
    const int b = blockIdx.x / g.nparts, s = blockIdx.x % g.nparts;
    const int i0 = blockIdx.z * 32, o0 = blockIdx.y * 32;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int ic = min(i0 + col, g.I - 1), oc = min(o0 + col, g.O - 1);
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(X + (size_t)b * g.x_batch), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(dY + (size_t)b * g.dy_batch), 0, 0x7fffffff, 0x00020000);
    const unsigned xbase = 4u * (unsigned)((long)ic * g.P), dbase = 4u * (unsigned)((long)oc * g.dy_chan);
    const int nb_total = g.H * g.cw;
    const int bb = s * g.per_part, be = min(bb + g.per_part, nb_total);
#pragma unroll 1
    for (int blk = bb; blk < be; ++blk) {
        const int m = blk / g.cw, n = (blk - m * g.cw) * 16 + 8 * kh;   // m uniform; the lane's 8 pixels n .. n + 7
        float xf[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool ok = n + k < g.W;
            xf[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, ok ? xbase + 4u * (unsigned)(m * g.W + n + k) : OOB, 0, 0));
        }
        uint4 aq[3];
        opmode::split8<DT>(xf, aq);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int u = 2 * m - 1 + ky;
            if (u < 0 || u >= 2 * g.H - 1) continue;        // uniform: the dy row is padding
            // dy columns 2n - 1 + j, j = 0 .. 16: odd columns (even j) in ev[.], even columns (odd j) in od[.] -- named by j's parity
            float f0[9], f1[8];
            const unsigned rb = dbase + 4u * (unsigned)((long)u * g.dy_row);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int v = 2 * (n + k) - 1;               // x pixel n + k (kx = 0) / n + k - 1 (kx = 2)
                const bool ok = v >= 0 && v < 2 * g.W - 1;
                f0[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(drs, ok ? rb + 4u * (unsigned)v : OOB, 0, 0));
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int v = 2 * (n + k);
                const bool ok = v < 2 * g.W - 1;
                f1[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(drs, ok ? rb + 4u * (unsigned)v : OOB, 0, 0));
            }
            unsigned d[3][5];                                // [piece][pair]: (f0[0], f0[1]) .. (f0[8], 0)
            opmode::split<DT>(f0[0], f0[1], d[0][0], d[1][0], d[2][0]);
            opmode::split<DT>(f0[2], f0[3], d[0][1], d[1][1], d[2][1]);
            opmode::split<DT>(f0[4], f0[5], d[0][2], d[1][2], d[2][2]);
            opmode::split<DT>(f0[6], f0[7], d[0][3], d[1][3], d[2][3]);
            opmode::split<DT>(f0[8], 0.f, d[0][4], d[1][4], d[2][4]);
            uint4 bq[3][3];
            opmode::split8<DT>(f1, bq[1]);                   // kx = 1: columns 2 (n + k)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                bq[0][q] = make_uint4(d[q][0], d[q][1], d[q][2], d[q][3]);                          // kx = 0: columns 2 (n + k) - 1
                bq[2][q] = make_uint4(__builtin_amdgcn_alignbit(d[q][1], d[q][0], 16), __builtin_amdgcn_alignbit(d[q][2], d[q][1], 16),
                                      __builtin_amdgcn_alignbit(d[q][3], d[q][2], 16), __builtin_amdgcn_alignbit(d[q][4], d[q][3], 16));
            }
#pragma unroll
            for (int term = 0; term < NT; ++term)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    acc[3 * ky + kx] = opmode::mfma<DT>(aq[opmode::Form<DT>::termA(term)], bq[kx][opmode::Form<DT>::termB(term)], acc[3 * ky + kx]);
        }
    }
    // partial [part][i][o][tap]: D row -> input channel, column = lane -> output channel
    float *prow = part + (size_t)blockIdx.x * ((size_t)9 * g.O * g.I);
    const int o = o0 + col;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (o < g.O && i < g.I) prow[((size_t)i * g.O + o) * 9 + t] = acc[t][r];
        }
}

int make_swgeom(SWGeom &g, int B, int O, int I, int H, int W)
{
    g.B = B; g.O = O; g.I = I; g.H = H; g.W = W; g.P = H * W;
    g.cw = (W + 15) / 16;
    const int nb = H * g.cw;
    const int tiles = ((O + 31) / 32) * ((I + 31) / 32);
    // about 2048 waves in all, at least 4 blocks per partial sum; partial sums under 256 MB
    int per_sample = (2048 + B * tiles - 1) / (B * tiles);
    const long cap = (256L << 20) / (4L * 9 * O * I) / B;
    if (per_sample > cap) per_sample = (int)cap;
    if (per_sample < 1) per_sample = 1;
    int per = (nb + per_sample - 1) / per_sample;
    if (per < 4) per = 4;
    g.per_part = per;
    g.nparts = (nb + per - 1) / per;
    return 0;
}

bool shape_ok(int O, int I, int H, int W)
{
    if (O <= 0 || I <= 0 || H <= 0 || W <= 0 || (O % 16) || (I % 16)) return false;
    const long P = (long)H * W;
    // every sample of x, dy (the (2H - 1) x (2W - 1) map, or a view into a 2H x 2W one) and dx is one buffer resource: byte offsets under 2 GB
    return P <= (1L << 26) && (long)I * P * 4 < (1L << 31) - 64 && (long)O * 4 * P * 4 < (1L << 31) - 64 && (long)max(O, I) * P * 4 < (1L << 31) - 64;
}

// TO of s2t_gemm_kernel: 64-row tiles where the rows fill them, else 32 (the forward of up_0 has 96 output channels)
int gemm_tile(int R) { return R % 64 == 0 ? 2 : 1; }

template <int MODE, int TO>
void launch_gemm(const float *src, const unsigned short *img, float *dst, const S2Geom &g, int dt, hipStream_t st)
{
    const dim3 grid((g.P + 32 * WAVES - 1) / (32 * WAVES), (g.R + 32 * TO - 1) / (32 * TO), g.B);
    if (dt == MLAGG_DTYPE_BF16)
        hipLaunchKernelGGL((s2t_gemm_kernel<MODE, TO, MLAGG_DTYPE_BF16>), grid, dim3(64 * WAVES), 0, st, src, img, dst, g);
    else if (dt == MLAGG_DTYPE_F16)
        hipLaunchKernelGGL((s2t_gemm_kernel<MODE, TO, MLAGG_DTYPE_F16>), grid, dim3(64 * WAVES), 0, st, src, img, dst, g);
    else
        hipLaunchKernelGGL((s2t_gemm_kernel<MODE, TO, MLAGG_DTYPE_BF16X3>), grid, dim3(64 * WAVES), 0, st, src, img, dst, g);
}

int gemm(int mode, const float *src, long src_batch, long src_chan, long src_row, const float *w, float *dst, long dst_batch, void *ws,
         int B, int O, int I, int H, int W, int dt, void *stream)
{
    if (!src || !w || !dst || !ws) return MLAGG_E_NULLPTR;
    if (!opmode::valid(dt) || B <= 0 || B > 65535 || !shape_ok(O, I, H, W)) return MLAGG_E_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(ws) & 15) return MLAGG_E_UNSUPPORTED;
    const long P = (long)H * W;
    S2Geom g{B, mode ? I : O, mode ? O : I, H, W, (int)P, src_batch, src_chan, src_row, dst_batch};
    if (mode == 0) {
        if (src_chan != P || src_row != W || src_batch < (long)I * P || dst_batch < (long)O * (2 * H - 1) * (2 * W - 1)) return MLAGG_E_UNSUPPORTED;
    } else {
        if (src_row < 2 * W - 1 || src_chan < (long)(2 * H - 2) * src_row + 2 * W - 1 || src_batch < (long)O * src_chan || dst_batch < (long)I * P)
            return MLAGG_E_UNSUPPORTED;
        if ((long)O * src_chan * 4 >= (1L << 31) - 64) return MLAGG_E_UNSUPPORTED;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_CONV3X3, st);
    unsigned short *img = static_cast<unsigned short *>(ws);
    const int n = 9 * O * I;
    const dim3 igrid((n + 255) / 256);
    if (dt == MLAGG_DTYPE_BF16)
        hipLaunchKernelGGL(s2t_weight_image_kernel<MLAGG_DTYPE_BF16>, igrid, dim3(256), 0, st, w, img, g.R, g.K, mode);
    else if (dt == MLAGG_DTYPE_F16)
        hipLaunchKernelGGL(s2t_weight_image_kernel<MLAGG_DTYPE_F16>, igrid, dim3(256), 0, st, w, img, g.R, g.K, mode);
    else
        hipLaunchKernelGGL(s2t_weight_image_kernel<MLAGG_DTYPE_BF16X3>, igrid, dim3(256), 0, st, w, img, g.R, g.K, mode);
    const bool wide = gemm_tile(g.R) == 2;
    if (mode == 0) {
        if (wide) launch_gemm<0, 2>(src, img, dst, g, dt, st);
        else launch_gemm<0, 1>(src, img, dst, g, dt, st);
    } else {
        if (wide) launch_gemm<1, 2>(src, img, dst, g, dt, st);
        else launch_gemm<1, 1>(src, img, dst, g, dt, st);
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int mlagg_conv3x3_s2t_supported(int O, int I, int H, int W) { return shape_ok(O, I, H, W) ? 1 : 0; }

extern "C" size_t mlagg_conv3x3_s2t_workspace_bytes(int O, int I) { return O > 0 && I > 0 ? (size_t)3 * 9 * O * I * 2 : 0; }

extern "C" int mlagg_conv3x3_s2t_fwd(const float *x, long x_batch, const float *w, float *y, long y_batch, void *workspace, int B, int O,
                                     int I, int H, int W, int dtype, void *stream)
{
    return gemm(0, x, x_batch, (long)H * W, W, w, y, y_batch, workspace, B, O, I, H, W, dtype, stream);
}

extern "C" int mlagg_conv3x3_s2_dgrad(const float *dy, long dy_batch, long dy_chan_stride, long dy_row_stride, const float *w, float *dx,
                                      long dx_batch, void *workspace, int B, int O, int I, int H, int W, int dtype, void *stream)
{
    return gemm(1, dy, dy_batch, dy_chan_stride, dy_row_stride, w, dx, dx_batch, workspace, B, O, I, H, W, dtype, stream);
}

extern "C" size_t mlagg_conv3x3_s2t_wgrad_workspace_floats(int B, int O, int I, int H, int W)
{
    if (B <= 0 || !shape_ok(O, I, H, W)) return 0;
    SWGeom g;
    make_swgeom(g, B, O, I, H, W);
    return (size_t)B * g.nparts * 9 * O * I;
}

extern "C" int mlagg_conv3x3_s2t_tile(int R) { return R > 0 ? gemm_tile(R) : 0; }

extern "C" int mlagg_conv3x3_s2t_wgrad_geometry(int B, int O, int I, int H, int W, int *out3)
{
    if (!out3) return MLAGG_E_NULLPTR;
    if (B <= 0 || B > (1 << 20) || !shape_ok(O, I, H, W)) return MLAGG_E_UNSUPPORTED;
    SWGeom g;
    make_swgeom(g, B, O, I, H, W);
    out3[0] = g.cw; out3[1] = g.per_part; out3[2] = g.nparts;
    return 0;
}

extern "C" int mlagg_conv3x3_s2t_wgrad(const float *x, long x_batch, const float *dy, long dy_batch, long dy_chan_stride, long dy_row_stride,
                                       float *dW, float *workspace, int B, int O, int I, int H, int W, int dtype, void *stream)
{
    if (!x || !dy || !dW || !workspace) return MLAGG_E_NULLPTR;
    if (!opmode::valid(dtype) || B <= 0 || B > (1 << 20) || !shape_ok(O, I, H, W)) return MLAGG_E_UNSUPPORTED;
    if (x_batch < (long)I * H * W || dy_row_stride < 2 * W - 1 || dy_chan_stride < (long)(2 * H - 2) * dy_row_stride + 2 * W - 1 ||
        dy_batch < (long)O * dy_chan_stride || (long)O * dy_chan_stride * 4 >= (1L << 31) - 64)
        return MLAGG_E_UNSUPPORTED;
    SWGeom g;
    make_swgeom(g, B, O, I, H, W);
    g.x_batch = x_batch;
    g.dy_batch = dy_batch;
    g.dy_chan = dy_chan_stride;
    g.dy_row = dy_row_stride;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MLAGG_TIMED(K_CONV3X3, st);
    const dim3 grid(B * g.nparts, (O + 31) / 32, (I + 31) / 32);
    if (dtype == MLAGG_DTYPE_BF16)
        hipLaunchKernelGGL(s2t_wgrad_kernel<MLAGG_DTYPE_BF16>, grid, dim3(64), 0, st, x, dy, workspace, g);
    else if (dtype == MLAGG_DTYPE_F16)
        hipLaunchKernelGGL(s2t_wgrad_kernel<MLAGG_DTYPE_F16>, grid, dim3(64), 0, st, x, dy, workspace, g);
    else
        hipLaunchKernelGGL(s2t_wgrad_kernel<MLAGG_DTYPE_BF16X3>, grid, dim3(64), 0, st, x, dy, workspace, g);
    // dW (I, O, 3, 3) = the column sums of the partial rows [part][i][o][tap], in a fixed order
    const int n = 9 * O * I;
    hipLaunchKernelGGL(mlagg_internal::column_sum_kernel<false>, dim3((n + 63) / 64), dim3(1024), 0, st, workspace, B * g.nparts, n, n, dW);
    return (int)hipGetLastError();
}
