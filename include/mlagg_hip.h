/*
 * mlagg_hip.h -- C ABI of libmlagg_hip.so (MI355X / gfx950 kernels for the MLAgg-UNet 2D hot path).
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes, no torch types; every buffer is owned by the caller, the
 *     library never allocates, frees or synchronises (safe inside hipGraph capture);
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream);
 *   - return 0 on success, a negative MLAGG_E_* code for a rejected argument, or a positive
 *     hipError_t from the launch.  The Python host turns any non-zero return into RuntimeError,
 *     the only exception type nnU-Net handles
 *     (mlagg/nnunetv2/training/nnUNetTrainer/variants/benchmarking/nnUNetTrainerBenchmark_5epochs.py:25-29);
 *   - all tensors fp32, contiguous in the stated layout; re-entrant; callable from autograd's
 *     backward thread.
 */
#ifndef MLAGG_HIP_H
#define MLAGG_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLAGG_E_UNSUPPORTED (-1) /* shape outside what the kernels are built for */
#define MLAGG_E_NULLPTR     (-2)
#define MLAGG_E_WORKSPACE   (-3)

/* arithmetic type of the mixed-precision entry points (tensors stay fp32 in memory; see mlagg_linear_lp_*) */
#define MLAGG_DTYPE_F32  0
#define MLAGG_DTYPE_BF16 1
#define MLAGG_DTYPE_F16  2
#define MLAGG_DTYPE_BF16X3 3 /* GEMM arithmetic only: fp32 operands as three bf16 pieces each, six partial products (fp32-accurate) */

const char *mlagg_version(void);
const char *mlagg_error_string(int code);

/* Per-kernel HIP-event timing for bench.py's roofline line (diagnostics; off by default, zero cost).
 * select: -1 off, -2 every kernel, otherwise one kernel id in [0, mlagg_profile_kernel_count()).
 * collect: synchronises with the recorded events (so NOT graph-capturable), writes the summed
 * milliseconds and launch counts per kernel id into ms[count] / counts[count] and resets. */
int mlagg_profile_kernel_count(void);
const char *mlagg_profile_kernel_name(int id);
int mlagg_profile_select(int id);
int mlagg_profile_collect(double *ms, int *counts);

/* ------------------------------------------------------------------------------------------
 * K1: selective scan.  Replaces mamba-ssm's `selective_scan_cuda.fwd/bwd` behind
 * `selective_scan_fn(u, delta, A, B, C, D, z=None, delta_bias, delta_softplus=True)` as called at
 * mlagg/nnunetv2/training/nnUNetTrainer/variants/mamba/MambaSkip.py:445-451 (ABI mirrored at
 * .../variants/mamba/vmamba/csms6s.py:224,235-238).
 *   u, delta, out      (batch, dim, L)        dim = G * H, channel d uses group d / H
 *   A                  (dim, N)               N must be 16
 *   B, C               (batch, G, N, L)
 *   D, delta_bias      (dim) or NULL
 *   chunk_state        workspace AND saved-for-backward tensor, mlagg_selscan_state_floats() floats:
 *                      [batch][nchunks][dim][N] states entering each 64-step chunk, followed by
 *                      [batch][nchunks][dim] per-chunk sums of softplus'd delta and
 *                      [batch][nchunks][7][dim][N] states entering the 2nd..8th 8-step tile of each chunk.
 * ------------------------------------------------------------------------------------------ */
size_t mlagg_selscan_state_floats(int batch, int dim, int L, int N);
int mlagg_selscan_fwd(const float *u, const float *delta, const float *A, const float *B, const float *C,
                      const float *D, const float *delta_bias, float *out, float *chunk_state,
                      int batch, int dim, int L, int N, int G, int delta_softplus, void *stream);

/* Backward.  `workspace` needs mlagg_selscan_bwd_workspace_floats() floats (reverse chunk carries and
 * per-chunk partial sums of dA / dD / ddelta_bias, reduced deterministically inside the call).
 * dD / ddelta_bias may be NULL when D / delta_bias are NULL. */
size_t mlagg_selscan_bwd_workspace_floats(int batch, int dim, int L, int N);
int mlagg_selscan_bwd(const float *u, const float *delta, const float *A, const float *B, const float *C,
                      const float *D, const float *delta_bias, const float *dout, const float *chunk_state,
                      float *du, float *ddelta, float *dA, float *dB, float *dC, float *dD,
                      float *ddelta_bias, float *workspace,
                      int batch, int dim, int L, int N, int G, int delta_softplus, void *stream);

/* K1, low-rank delta form: the scan with SS2D_skip's dt projection folded in.  Replaces the pair
 *   dts = einsum("b k r l, k d r -> b k d l", dts_r, dt_projs_weight)            (MambaSkip.py:430-436)
 *   selective_scan_fn(xs, dts, As, Bs, Cs, Ds, delta_bias=..., delta_softplus=True)  (MambaSkip.py:445-451)
 * dtr (batch, G, R, L): the rank-R rows of group g (scan order); Wdt (dim, R): row d = projection of channel d
 * (dt_projs_weight viewed as (K*d_inner, R)); 1 <= R <= 4.  delta (batch, dim, L) never exists in memory.
 * Backward overwrites du (batch, dim, L), ddtr (batch, G, R, L), dWdt (dim, R), dA, dB, dC and, when non-NULL,
 * dD, ddelta_bias; chunk_state / workspace sizes as for mlagg_selscan_fwd / _bwd. */
int mlagg_selscan_lowrank_fwd(const float *u, const float *dtr, const float *Wdt, int R, const float *A, const float *B,
                              const float *C, const float *D, const float *delta_bias, float *out, float *chunk_state,
                              int batch, int dim, int L, int N, int G, int delta_softplus, void *stream);
int mlagg_selscan_lowrank_bwd(const float *u, const float *dtr, const float *Wdt, int R, const float *A, const float *B,
                              const float *C, const float *D, const float *delta_bias, const float *dout,
                              const float *chunk_state, float *du, float *ddtr, float *dWdt, float *dA, float *dB,
                              float *dC, float *dD, float *ddelta_bias, float *workspace, int batch, int dim, int L,
                              int N, int G, int delta_softplus, void *stream);
/* What the K1 launchers choose for (dim, L, G) in the direct form (R = 0) or the low-rank form of rank R (host only, nothing is
 * launched; the launchers decide through the same code, MLAGG_SELSCAN_BWD_BLOCKED included): form * 2 + fast, or
 * MLAGG_E_UNSUPPORTED for a geometry the launchers refuse (and for R outside 0..4).
 *   fast: 1 when the forward and the backward's local pass run the instantiation without range checks (32-channel blocks that
 *         divide the group of H = dim / G channels, L % 4 == 0);
 *   form: the backward's main kernel.  0: channel blocks (H > 96, or the override), dB / dC / d(dtr) by float atomics when a group
 *         has more than one block.  1..5: one wave per group, selscan_bwd_group_kernel<RT, VEC, FULL, WHOLE> with RT the
 *         compile-time rank (0: direct form, 3: rank 3, 4: any rank, read at run time), VEC: L % 4 == 0, FULL: H % 16 == 0,
 *         WHOLE: L % 64 == 0 --
 *           1 <0 or 3, true, true, true>    2 <0 or 3, true, true, false>    3 <4, true, true, false>
 *           4 <0 or 4, true, false, false>  5 <0 or 4, false, false, false> */
int mlagg_selscan_path(int dim, int L, int G, int R);

/* ------------------------------------------------------------------------------------------
 * K3: 3x3-window differential attention + RMSNorm + LePE, the `local=True` branch of
 * AggregatedAttention.forward (mlagg/.../nnUNetTrainer_MLAgg_2D_dt_MS.py:693-717, 779-782).
 * Token-major inputs: q (batch, H*W, d) and kv (batch, H*W, 2d) straight out of the q / kv
 * Linear layers (row strides in floats given explicitly, so strided views need no copy).
 *   d = nh * 48, head h: q1 = q[.., 48h .. 48h+23], q2 = q[.., 48h+24 .. 48h+47]   (T:687, 712-713)
 *   k likewise in kv[.., 0 .. d), v = kv[.., d + 48h .. d + 48h + 47]               (T:690, 702-703)
 *   out[t, 48h+e] = 0.2 * w_subln[e] * rmsnorm_e( sum_j (s1_j - lam * s2_j) v_j[e] )
 *                   + lepe_b[48h+e] + sum_j lepe_w[48h+e][j] v_j[48h+e]
 *   s1 = softmax_j(scale * q1.k1_j), s2 = softmax_j(scale * q2.k2_j) over the in-image 3x3 window.
 *   `lam` is read from device memory (1 float) so the call stays graph-capturable.
 * ------------------------------------------------------------------------------------------ */
int mlagg_local_attn_fwd(const float *q, int q_stride, const float *kv, int kv_stride,
                         const float *lam, const float *subln_w, const float *lepe_w, const float *lepe_b,
                         float *out, int out_stride, int batch, int H, int W, int nh, float scale,
                         void *stream);
/* Backward: gather form, no atomics on dq/dkv.  `workspace` = mlagg_local_attn_bwd_workspace_floats().
 * dlam / dsubln_w are ACCUMULATED into (caller zero-fills); dlepe_w / dlepe_b are written. */
size_t mlagg_local_attn_bwd_workspace_floats(int batch, int H, int W, int nh);
int mlagg_local_attn_bwd(const float *q, int q_stride, const float *kv, int kv_stride,
                         const float *lam, const float *subln_w, const float *lepe_w,
                         const float *dout, int dout_stride,
                         float *dq, int dq_stride, float *dkv, int dkv_stride,
                         float *dlam, float *dsubln_w, float *dlepe_w, float *dlepe_b, float *workspace,
                         int batch, int H, int W, int nh, float scale, void *stream);

/* ------------------------------------------------------------------------------------------
 * K4: pooled differential attention + RMSNorm, the `local=False` branch (T:733-760 variant A via
 * flash_attn_func, T:762-777 variant B); supersedes the four `flash_attn_func(q_j, k_j, v_i)` calls.
 *   q (batch, N, d) unscaled projection; kp, vp (batch, P, d) pooled keys / values (kv(x_) halves);
 *   `scale` is the total logit scale: head_dim^-0.5 for variant B, 1/head_dim for variant A.
 *   out[t, 48h+e] = 0.2 * w_subln[e] * rmsnorm_e( sum_p (s1_p - lam * s2_p) vp[p, 48h+e] )
 * ------------------------------------------------------------------------------------------ */
int mlagg_pooled_attn_fwd(const float *q, int q_stride, const float *kp, int kp_stride,
                          const float *vp, int vp_stride, const float *lam, const float *subln_w,
                          float *out, int out_stride,
                          float *lse,   /* (batch, N, nh, 2) log-sum-exp of both maps, or NULL (inference) */
                          float *o_pre, /* (batch, N, d) output before the RMSNorm, or NULL (inference) */
                          int batch, int N, int P, int nh, float scale, void *stream);
/* Backward needs the forward's lse / o_pre and mlagg_pooled_attn_bwd_workspace_floats() of scratch.
 * dq / dkp / dvp are overwritten; dlam / dsubln_w are ACCUMULATED into (caller zero-fills). */
size_t mlagg_pooled_attn_bwd_workspace_floats(int batch, int N, int P, int nh);
int mlagg_pooled_attn_bwd(const float *q, int q_stride, const float *kp, int kp_stride,
                          const float *vp, int vp_stride, const float *lam, const float *subln_w,
                          const float *dout, int dout_stride, const float *lse, const float *o_pre,
                          float *dq, int dq_stride, float *dkp, int dkp_stride, float *dvp, int dvp_stride,
                          float *dlam, float *dsubln_w, float *workspace,
                          int batch, int N, int P, int nh, float scale, void *stream);

/* ------------------------------------------------------------------------------------------
 * K2: depthwise 3x3 convolution (zero padding 1, stride 1) + bias (+ SiLU when `silu`), token-major
 * x, y (batch, H*W, C) with row strides in floats; w (C, 9) = Conv2d weight (C, 1, 3, 3) flattened.
 * Replaces nn.Conv2d(groups=C) at nnUNetTrainer_MLAgg_2D_dt_MS.py:890 (dwc + SiLU), T:781-782 (LePE of
 * the pooled branch), MambaSkip.py:521-523 (conv2d + SiLU) and M:553 (ConvolutionalGLU.dwconv).
 *   pre: (batch, H*W, C) contiguous pre-activation saved for backward when silu (NULL otherwise /
 *        inference).  Backward WRITES dw (C, 9) and dbias (C) (no zero-fill needed).
 *   res: NULL, or (batch, H*W, C) contiguous, added to the output (silu == 0 only): x + lepe(v) of T:782 in the same pass.
 * ------------------------------------------------------------------------------------------ */
int mlagg_dwconv3x3_fwd(const float *x, int x_stride, const float *w, const float *bias, const float *res, float *y,
                        int y_stride, float *pre, int batch, int H, int W, int C, int silu, void *stream);
size_t mlagg_dwconv3x3_bwd_workspace_floats(int batch, int H, int W, int C);
/* Gated form: y = SiLU(conv(x) + bias) * gate -- `self.fc2(self.act(self.dwconv(x, H, W)) * v)` of ConvolutionalGLU (MambaSkip.py:559-577)
 * with the product in the convolution's epilogue; gate (batch, H*W, C) with row stride gate_stride (the v half of fc1's output).  Backward
 * also writes dgate = dy * SiLU(pre) (row stride dgate_stride).  Workspace as for mlagg_dwconv3x3_bwd. */
int mlagg_dwconv3x3_gated_fwd(const float *x, int x_stride, const float *w, const float *bias, const float *gate, int gate_stride, float *y,
                              int y_stride, float *pre, int batch, int H, int W, int C, void *stream);
int mlagg_dwconv3x3_gated_bwd(const float *x, int x_stride, const float *w, const float *dy, int dy_stride, const float *pre,
                              const float *gate, int gate_stride, float *dx, int dx_stride, float *dgate, int dgate_stride, float *dw,
                              float *dbias, float *workspace, int batch, int H, int W, int C, void *stream);
int mlagg_dwconv3x3_bwd(const float *x, int x_stride, const float *w, const float *dy, int dy_stride,
                        const float *pre, float *dx, int dx_stride, float *dw, float *dbias, float *workspace,
                        int batch, int H, int W, int C, int silu, void *stream);

/* ------------------------------------------------------------------------------------------
 * K5w: weight / bias gradient of a token-major Linear,  dW (O, I) = dy^T x,  db (O) = column sums of dy,
 * with dy (M, O) and x (M, I) (row strides in floats), M = batch * tokens.  Replaces the library GEMM in the
 * backward of the nn.Linear layers at nnUNetTrainer_MLAgg_2D_dt_MS.py:687-690, 887-907 and
 * MambaSkip.py:518, 538, 572-575 (split-K over tokens on fp32 MFMA).  dW / db are overwritten.
 * ------------------------------------------------------------------------------------------ */
/* K5: the same layers' forward y (M, N) = x (M, K) . w (N, K)^T + bias and input gradient
 * dx (M, I) = dy (M, O) . w (O, I) on fp32 MFMA (w contiguous; x / y / dy / dx with row strides; K and I % 4 == 0). */
int mlagg_linear_fwd(const float *x, int x_stride, const float *w, const float *bias, float *y, int y_stride,
                     int M, int N, int K, void *stream);
int mlagg_linear_dgrad(const float *dy, int dy_stride, const float *w, float *dx, int dx_stride, int M, int O, int I,
                       void *stream);
/* Mixed precision: the same two products with the operands rounded to bf16 / fp16 (dtype = MLAGG_DTYPE_BF16 / _F16) on
 * their way into the matrix cores and fp32 accumulation -- what torch.autocast makes of nn.Linear in the reference's
 * default train step (mlagg/nnunetv2/training/nnUNetTrainer/nnUNetTrainer.py:848-851; fp16 + GradScaler :152, bf16 in
 * BASELINE configs[2]).  x, w, y / dy, dx stay fp32 in memory, same layouts and strides as above.
 * dtype = MLAGG_DTYPE_BF16X3: the fp32 layers on the 16-bit matrix instructions -- each fp32 operand as three bf16 pieces, six
 * partial products accumulated in fp32 (error 2^-24 of a product: as accurate as the fp32 instruction, 2.7x its rate). */
int mlagg_linear_lp_fwd(const float *x, int x_stride, const float *w, const float *bias, float *y, int y_stride,
                        int M, int N, int K, int dtype, void *stream);
int mlagg_linear_lp_dgrad(const float *dy, int dy_stride, const float *w, float *dx, int dx_stride, int M, int O, int I,
                          int dtype, void *stream);
size_t mlagg_linear_wgrad_workspace_floats(int M, int O, int I);
/* The launch geometry of K5w for contiguous operands (host arithmetic, what the launcher itself decides with): out5 = {to, ti: 32-wide
 * tiles per wave along O and I; slab: tokens per wave; nslabs; ogroups * 65536 + igroups: 96-wide column groups}.  0, or the error of
 * the launch for these sizes. */
int mlagg_linear_wgrad_geometry(int M, int O, int I, int *out5);
int mlagg_linear_wgrad(const float *dy, int dy_stride, const float *x, int x_stride, float *dW, float *db,
                       float *workspace, int M, int O, int I, void *stream);
/* The same gradient with every fp32 operand as three bf16 pieces on v_mfma_f32_32x32x16_bf16 (six partial products, fp32
 * accumulation: the error of the fp32 instruction at 2.7x less matrix-pipe time; same workspace, same layouts). */
int mlagg_linear_wgrad_x3(const float *dy, int dy_stride, const float *x, int x_stride, float *dW, float *db, float *workspace,
                          int M, int O, int I, void *stream);

/* ------------------------------------------------------------------------------------------
 * Boundary #3: `flash_attn.flash_attn_func(q, k, v, causal=False)` as called four times per pooled AggregatedAttention
 * (nnUNetTrainer_MLAgg_2D_dt_MS.py:173, 745-750): out = softmax(q k^T * softmax_scale) v per (batch, head), 16-bit
 * tensors (dtype = MLAGG_DTYPE_BF16 / _F16), fp32 arithmetic.  Serves mlagg_unet_amd.shims.flash_attn_func (the
 * reference's own model file running unmodified); the product network uses the fused K4 launch instead.
 *   q, out, dout, dq  (B, N, nh, head_dim)     head_dim must be 24 (every MLAgg-UNet stage), P <= 512
 *   k, v              (B, P, nh, head_dim)
 *   lse               (B, nh, N) fp32, written by fwd when not NULL (needed by bwd)
 *   workspace         mlagg_flash_attn_bwd_workspace_floats() floats; after bwd its LAST B*P*nh*2*head_dim floats hold
 *                     the fp32 gradients (B, P, nh, 2, head_dim): [..., 0, :] = dk, [..., 1, :] = dv
 * ------------------------------------------------------------------------------------------ */
int mlagg_flash_attn_fwd(const void *q, const void *k, const void *v, void *out, float *lse, int B, int N, int P, int nh,
                         int head_dim, float softmax_scale, int dtype, void *stream);
size_t mlagg_flash_attn_bwd_workspace_floats(int B, int N, int P, int nh, int head_dim);
int mlagg_flash_attn_bwd(const void *q, const void *k, const void *v, const void *out, const void *dout, const float *lse,
                         void *dq, float *workspace, int B, int N, int P, int nh, int head_dim, float softmax_scale,
                         int dtype, void *stream);

/* ------------------------------------------------------------------------------------------
 * K6: LayerNorm over the last dimension of token-major rows, x (rows, C) with row stride x_stride,
 * y (rows, C) contiguous.  Replaces nn.LayerNorm at nnUNetTrainer_MLAgg_2D_dt_MS.py:723, 887, 907, 984-1001 and
 * MambaSkip.py:536, 741-742.  Built for C in {48, 96, 192, 384, 768} (mlagg_layernorm_supported).
 *   stats: (rows, 2) mean / rstd saved for backward (NULL for inference).
 *   backward overwrites dx (rows, C), dgamma (C), dbeta (C or NULL).
 * ------------------------------------------------------------------------------------------ */
int mlagg_layernorm_supported(int C);
int mlagg_layernorm_fwd(const float *x, int x_stride, const float *gamma, const float *beta, float *y,
                        float *stats, int rows, int C, float eps, void *stream);
size_t mlagg_layernorm_bwd_workspace_floats(int rows, int C);
int mlagg_layernorm_bwd(const float *x, int x_stride, const float *dy, int dy_stride, const float *gamma,
                        const float *stats, float *dx, float *dgamma, float *dbeta, float *workspace,
                        int rows, int C, void *stream);
/* K6 with the residual junction in front of the norm in the same pass (nnUNetTrainer_MLAgg_2D_dt_MS.py:905-907: x = shortcut +
 * drop_path(out_proj(..)); x = x + drop_path(mlp(norm2(x))) -- and norm1 of the next block of the stage, T:887):
 *   xsum = skip + branch * scale[row / rows_per_sample],   y = LayerNorm(xsum) * gamma + beta
 * skip, branch, xsum, y (rows, C) contiguous; scale: one stochastic-depth factor per sample (rows_per_sample rows each), NULL = 1.
 * Backward: dskip = LayerNorm'(dy) + dres (dres: gradient reaching xsum from its other consumers, NULL = none), dbranch = dskip *
 * scale (NULL exactly when scale is: the two gradients coincide); workspace: mlagg_layernorm_bwd_workspace_floats(rows, C). */
int mlagg_residual_layernorm_fwd(const float *skip, const float *branch, const float *scale, const float *gamma, const float *beta,
                                 float *xsum, float *y, float *stats, int rows, int rows_per_sample, int C, float eps, void *stream);
int mlagg_residual_layernorm_bwd(const float *xsum, const float *dy, int dy_stride, const float *dres, const float *scale,
                                 const float *gamma, const float *stats, float *dskip, float *dbranch, float *dgamma, float *dbeta,
                                 float *workspace, int rows, int rows_per_sample, int C, void *stream);

/* ------------------------------------------------------------------------------------------
 * K2v: depthwise 3x3x3 convolution (zero padding 1, stride 1) + bias (+ SiLU when `silu`) on token-major volumes:
 * x, y (batch, D*H*W, C) with row strides in floats (multiples of 4, C % 4 == 0); w (C, 27) = Conv3d weight (C, 1, 3, 3, 3)
 * flattened, tap index kd * 9 + kh * 3 + kw.  Replaces the depthwise nn.Conv3d + SiLU of SS3D
 * (variants/mamba/UMambaEnc_SS3D.py:166-174, 331-333).  pre: (batch, D*H*W, C) contiguous pre-activation saved for
 * backward when silu (NULL otherwise / inference).  Backward writes dx, dw (C, 27) and dbias (C, may be NULL).
 * ------------------------------------------------------------------------------------------ */
int mlagg_dwconv3d_fwd(const float *x, int x_stride, const float *w, const float *bias, float *y, int y_stride,
                       float *pre, int batch, int D, int H, int W, int C, int silu, void *stream);
size_t mlagg_dwconv3d_bwd_workspace_floats(int batch, int D, int H, int W, int C);
int mlagg_dwconv3d_bwd(const float *x, int x_stride, const float *w, const float *dy, int dy_stride, const float *pre,
                       float *dx, int dx_stride, float *dw, float *dbias, float *workspace, int batch, int D, int H,
                       int W, int C, int silu, void *stream);

/* ------------------------------------------------------------------------------------------
 * K2n: depthwise 3x3 convolution on NCHW maps (zero padding 1, stride 1 or 2) + bias.  x (B, C, H, W),
 * y (B, C, Ho, Wo), w (C, 9).  Replaces nn.Conv2d(groups=C) of MedNeXtBlock.conv1 / MedNeXtDownBlock.conv1
 * (nnUNetTrainer_MLAgg_2D_dt_MS.py:256-263, 310, 349-356).  Backward overwrites dx, dw (C, 9), dbias (C or NULL).
 * ------------------------------------------------------------------------------------------ */
int mlagg_dwconv3x3_nchw_fwd(const float *x, const float *w, const float *bias, float *y, int B, int C, int H, int W,
                             int stride, void *stream);
size_t mlagg_dwconv3x3_nchw_bwd_workspace_floats(int B, int C, int H, int W, int stride);
int mlagg_dwconv3x3_nchw_bwd(const float *x, const float *w, const float *dy, float *dx, float *dw, float *dbias,
                             float *workspace, int B, int C, int H, int W, int stride, void *stream);
/* ... dx = data gradient + dres (NULL: none): the gradient of the block's residual connection on the same map (`x1 = x + ...`,
 * T:256-300) summed inside the kernel; needs stride 1 and W % 4 == 0. */
int mlagg_dwconv3x3_nchw_bwd_res(const float *x, const float *w, const float *dy, const float *dres, float *dx, float *dw, float *dbias,
                                 float *workspace, int B, int C, int H, int W, int stride, void *stream);

/* ------------------------------------------------------------------------------------------
 * K1': cross-scan / cross-merge of SS2D_skip.forward_corev0 (MambaSkip.py:414-422 and 455-471 + 534).
 *   tok: token-major (B, L_cat, tok_stride floats per token); direction k reads/writes CB channels at
 *        column k * blk_stride (nblk = 4) or at column 0 for every direction (nblk = 1);
 *   seq: (B, 4 * CB, L_cat), row k * CB + c = direction k in scan order (k=0 row-major, 1 column-major,
 *        2/3 their reversals; scales concatenated in order).  H, W: host arrays of the nscale (<= 4) map sizes.
 * cross_scan: tok -> seq.  cross_merge: the adjoint, seq -> tok (sums the four directions when nblk = 1).
 * ------------------------------------------------------------------------------------------ */
int mlagg_cross_scan(const float *tok, int tok_stride, int blk_stride, float *seq, int B, int nscale,
                     const int *H, const int *W, int CB, int nblk, void *stream);
int mlagg_cross_merge(const float *seq, float *tok, int tok_stride, int blk_stride, int B, int nscale,
                      const int *H, const int *W, int CB, int nblk, void *stream);

/* ------------------------------------------------------------------------------------------
 * K18: 1 x 1 convolutions (stride 1, no padding, groups 1) on channel-major maps, fp32 operands as three bf16 pieces on the 16-bit
 * matrix instructions (six partial products, fp32 accumulation: the accuracy of the fp32 instruction).  Replaces the library
 * convolution behind nn.Conv2d(kernel_size=1) at nnUNetTrainer_MLAgg_2D_dt_MS.py:279-316 (MedNeXtBlock conv2 / conv3), :319-367
 * (down / up blocks) and :972-1001 (Project).
 *   fwd:   y (B, O, P) = w (O, I) . x (B, I, P) (+ bias[o], NULL: none); P = H * W pixels; x_batch / y_batch: floats between
 *          samples (a channel slice of a wider map is a valid operand).  The data gradient is the same call on w^T (I, O) and dy.
 *   wgrad: dW (O, I) = sum_b dy (B, O, P) . x (B, I, P)^T, overwritten; workspace: mlagg_conv1x1_wgrad_workspace_floats floats.
 * Supported (mlagg_conv1x1_supported): contraction I % 16 == 0, P % 16 == 0, P >= 96; anything else MLAGG_E_UNSUPPORTED (the
 * caller keeps the library convolution).
 * ------------------------------------------------------------------------------------------ */
int mlagg_conv1x1_supported(int O, int I, long P);
int mlagg_conv1x1_fwd(const float *x, long x_batch, const float *w, const float *bias, float *y, long y_batch, int B, int O, int I,
                      long P, void *stream);
size_t mlagg_conv1x1_wgrad_workspace_floats(int B, int O, int I, long P);
int mlagg_conv1x1_wgrad(const float *dy, long dy_batch, const float *x, long x_batch, float *dW, float *workspace, int B, int O,
                        int I, long P, void *stream);
/* The same two products in the operand form `dtype`: MLAGG_DTYPE_BF16X3 = the calls above; MLAGG_DTYPE_BF16 / MLAGG_DTYPE_F16 = the
 * reference's autocast train step (nnUNetTrainer.py:848; BASELINE configs[2] / [4]), where the convolution's operands are rounded to
 * 16 bits and the sums are fp32: operands rounded ONCE in registers (nearest even), one product; x, w, y / dW stay fp32 in memory. */
int mlagg_conv1x1_fwd_lp(const float *x, long x_batch, const float *w, const float *bias, float *y, long y_batch, int B, int O, int I,
                         long P, int dtype, void *stream);
int mlagg_conv1x1_wgrad_lp(const float *dy, long dy_batch, const float *x, long x_batch, float *dW, float *workspace, int B, int O,
                           int I, long P, int dtype, void *stream);
/* Forward form with a ragged contraction: x has I_valid <= I channels, w is (O, I) with I % 16 == 0 and zero columns from I_valid on
 * (the segmentation heads, nnUNetTrainer_MLAgg_2D_dt_MS.py:549-561 OutBlock: the data gradient of a 14-class head contracts over 14). */
int mlagg_conv1x1_fwd_ragged(const float *x, long x_batch, const float *w, const float *bias, float *y, long y_batch, int B, int O, int I,
                             int I_valid, long P, int dtype, void *stream);
/* ... accumulate != 0: y += w . x.  The data gradient of the second convolution that reads a map (UnetResBlock's conv3 beside conv1 on the
 * same input, MONAI structure behind T:1340-1368) is added to the first one's inside the kernel instead of by an add_ over the map. */
int mlagg_conv1x1_fwd_acc(const float *x, long x_batch, const float *w, const float *bias, float *y, long y_batch, int B, int O, int I,
                          int I_valid, long P, int dtype, int accumulate, void *stream);
/* The tile the launchers choose (host only, nothing is launched; the launchers call the same code, MLAGG_K18_TILE included): to * 4 + tp
 * of the forward form for O output channels -- (32 to) channels x (32 tp) pixels per wave -- and to * 4 + ti of the weight gradient. */
int mlagg_conv1x1_fwd_tile(int O);
int mlagg_conv1x1_wgrad_tile(int O, int I);

/* ------------------------------------------------------------------------------------------
 * K19: dense 3 x 3 convolutions (stride 1, zero padding 1, groups 1) on channel-major maps as nine shifted GEMMs on the 16-bit matrix
 * instructions (fp32 operands as three bf16 pieces, six partial products, fp32 accumulation).  Replaces the library convolution
 * behind nn.Conv2d(kernel_size=3, padding=1) in UnetResBlock conv1 / conv2 (nnUNetTrainer_MLAgg_2D_dt_MS.py:1340-1368 via
 * UnetrBasicBlock / UnetrUpBlock), Project (T:972-1001) and the MSMM conv branches (MambaSkip.py:706-712): forward, and -- with
 * `transposed`, on the layer's forward weight (I_layer = O here) and its output gradient -- the data gradient.
 *   y (B, O, H, W) = conv3x3(x (B, I, H, W), w) (+ bias[o], NULL: none); x_batch / y_batch: floats between samples;
 *   workspace: mlagg_conv3x3_workspace_bytes(O, I) bytes, 16-byte aligned (the pre-split weight image, rebuilt by every call).
 * Supported (mlagg_conv3x3_supported): contraction I % 16 == 0, H * W >= 96.
 * ------------------------------------------------------------------------------------------ */
int mlagg_conv3x3_supported(int O, int I, int H, int W);
size_t mlagg_conv3x3_workspace_bytes(int O, int I);
int mlagg_conv3x3_fwd(const float *x, long x_batch, const float *w, int transposed, const float *bias, float *y, long y_batch,
                      void *workspace, int B, int O, int I, int H, int W, void *stream);
/* The same kernel for 3 x 3 x 3 convolutions (stride 1, padding 1) on (B, C, D, H, W) volumes -- nine kernel rows (kz, ky) of three
 * taps: the forward / data gradient of `nn.Conv3d(kernel_size=3, padding=1)` in the 3-D network (variants/mamba/UMambaEnc_SS3D.py:49-66
 * BasicResBlock / BasicBlockD convolutions, :477-513, 589-637, 744-779), straight on the unpadded volumes; w (O, I, 3, 3, 3).
 * workspace: mlagg_conv3x3x3_workspace_bytes(O, I). */
int mlagg_conv3x3x3_supported(int O, int I, int D, int H, int W);
size_t mlagg_conv3x3x3_workspace_bytes(int O, int I);
int mlagg_conv3x3x3_fwd(const float *x, long x_batch, const float *w, int transposed, const float *bias, float *y, long y_batch,
                        void *workspace, int B, int O, int I, int D, int H, int W, void *stream);
/* Weight gradient of the same convolution: dW (O, I, 3, 3) = sum_b sum_p dy (B, O, H, W) [.] x (B, I, H, W) shifted by the tap,
 * overwritten (inside `convolution_backward` of the layers above); W % 8 == 0 and H W % 16 == 0 (mlagg_conv3x3_wgrad_supported); workspace:
 * mlagg_conv3x3_wgrad_workspace_floats floats.  dy 16-byte aligned. */
int mlagg_conv3x3_wgrad_supported(int O, int I, int H, int W);
/* ... and of the 3 x 3 x 3 convolution: dW (O, I, 3, 3, 3) from dy (B, O, D, H, W) and x (B, I, D, H, W), unpadded volumes (one wave
 * per kernel slice kz); W % 8 == 0 and D H W % 16 == 0 (mlagg_conv3x3x3_wgrad_supported), else the caller keeps K15. */
int mlagg_conv3x3x3_wgrad_supported(int O, int I, int D, int H, int W);
size_t mlagg_conv3x3x3_wgrad_workspace_floats(int B, int O, int I, int D, int H, int W);
int mlagg_conv3x3x3_wgrad(const float *dy, long dy_batch, const float *x, long x_batch, float *dW, float *workspace, int B, int O,
                          int I, int D, int H, int W, void *stream);
size_t mlagg_conv3x3_wgrad_workspace_floats(int B, int O, int I, int H, int W);
int mlagg_conv3x3_wgrad(const float *dy, long dy_batch, const float *x, long x_batch, float *dW, float *workspace, int B, int O,
                        int I, int H, int W, void *stream);
/* The 3 x 3 products in the operand form `dtype` (see mlagg_conv1x1_fwd_lp; workspaces as above). */
int mlagg_conv3x3_fwd_lp(const float *x, long x_batch, const float *w, int transposed, const float *bias, float *y, long y_batch,
                         void *workspace, int B, int O, int I, int H, int W, int dtype, void *stream);
int mlagg_conv3x3_wgrad_lp(const float *dy, long dy_batch, const float *x, long x_batch, float *dW, float *workspace, int B, int O,
                           int I, int H, int W, int dtype, void *stream);
/* What the launchers choose (host only, nothing is launched; the launchers call the same code, MLAGG_K19_TILE / MLAGG_K19W16 included):
 *   fwd_tile:   to * 4 + tp of the forward form for O output channels on a (D, H, W) map (D = 1: 2-D) -- (32 to) channels x (32 tp)
 *               pixels per wave;
 *   wgrad_form: form * 4 + ti of the weight gradient in the operand form `dtype`.  form 0: 32 x 32 tiles, nine taps per wave (every
 *               volume, D > 1), ti reported as 0; form 1: (48 x 16 ti)-channel tiles, fragment-shaped loads; form 2: the same tiles,
 *               operands staged through LDS in full lines (needs a 16-byte-aligned x, else the launcher runs form 1).
 *               MLAGG_E_UNSUPPORTED for a `dtype` that is no operand form. */
int mlagg_conv3x3_fwd_tile(int O, int D, int H, int W);
int mlagg_conv3x3_wgrad_form(int O, int I, int D, int dtype);

/* ------------------------------------------------------------------------------------------
 * K19t: the 3 x 3, stride-2, padding-1 transposed convolution of PatchExpand (nnUNetTrainer_MLAgg_2D_dt_MS.py:506-513, conv1 =
 * nn.ConvTranspose2d(cin, cout, 3, stride=2, padding=1)) and its two gradients, in the operand form `dtype` (MLAGG_DTYPE_BF16X3: fp32
 * layers; MLAGG_DTYPE_BF16 / _F16: the 16-bit modes, see mlagg_conv1x1_fwd_lp).  w is the layer's (I, O, 3, 3) weight.
 *   forward: y (B, O, 2H - 1, 2W - 1) = conv_transpose2d(x (B, I, H, W), w), what the library returns (PatchExpand's pad stays);
 *   data gradient: dx (B, I, H, W) = conv2d(dy, w, stride 2, padding 1), dy (B, O, 2H - 1, 2W - 1) at any channel / row stride (the
 *   interior of the padded gradient qualifies); weight gradient: dW (I, O, 3, 3), overwritten.
 *   workspace: mlagg_conv3x3_s2t_workspace_bytes(O, I) bytes, 16-byte aligned (the pre-split weight image) for the forward / data
 *   gradient; mlagg_conv3x3_s2t_wgrad_workspace_floats floats for the weight gradient.
 * Supported (mlagg_conv3x3_s2t_supported): O % 16 == 0 and I % 16 == 0, every sample of x, dy and dx under 2 GB.
 * ------------------------------------------------------------------------------------------ */
int mlagg_conv3x3_s2t_supported(int O, int I, int H, int W);
size_t mlagg_conv3x3_s2t_workspace_bytes(int O, int I);
int mlagg_conv3x3_s2t_fwd(const float *x, long x_batch, const float *w, float *y, long y_batch, void *workspace, int B, int O, int I,
                          int H, int W, int dtype, void *stream);
int mlagg_conv3x3_s2_dgrad(const float *dy, long dy_batch, long dy_chan_stride, long dy_row_stride, const float *w, float *dx,
                           long dx_batch, void *workspace, int B, int O, int I, int H, int W, int dtype, void *stream);
size_t mlagg_conv3x3_s2t_wgrad_workspace_floats(int B, int O, int I, int H, int W);
int mlagg_conv3x3_s2t_wgrad(const float *x, long x_batch, const float *dy, long dy_batch, long dy_chan_stride, long dy_row_stride,
                            float *dW, float *workspace, int B, int O, int I, int H, int W, int dtype, void *stream);
/* Host arithmetic, what the launchers themselves decide with.  mlagg_conv3x3_s2t_tile: the 32-row tiles per workgroup (1 or 2) of the
 * forward (R = O) / data gradient (R = I) kernel.  mlagg_conv3x3_s2t_wgrad_geometry: out3 = {cw: 16-pixel blocks per input row;
 * per_part: blocks per partial sum; nparts: partial sums per sample}; 0, or the error of the launch for these sizes. */
int mlagg_conv3x3_s2t_tile(int R);
int mlagg_conv3x3_s2t_wgrad_geometry(int B, int O, int I, int H, int W, int *out3);

/* ------------------------------------------------------------------------------------------
 * K17: key / value reduction of the pooled attention branch, pooled (B, (H/r)(W/r), d) = r x r window mean of GELU(s), s (B, H W, d)
 * token-major at row stride s_stride (a column block of the stacked q | v | sr projection).  Replaces nn.GELU + nn.AdaptiveAvgPool2d
 * at nnUNetTrainer_MLAgg_2D_dt_MS.py:722 (modules at :668, :671) for H % r == W % r == 0 (other sizes: MLAGG_E_UNSUPPORTED, the
 * caller keeps the library's adaptive pooling).  Backward overwrites ds (B, H W, d) at row stride ds_stride.
 * ------------------------------------------------------------------------------------------ */
int mlagg_gelu_pool_fwd(const float *s, int s_stride, float *pooled, int batch, int H, int W, int d, int r, void *stream);
int mlagg_gelu_pool_bwd(const float *s, int s_stride, const float *dpooled, float *ds, int ds_stride, int batch, int H, int W, int d,
                        int r, void *stream);

/* ------------------------------------------------------------------------------------------
 * K7: gate of the MLLA block, out (rows, 2h) = concat(a0, a1) * SiLU(act) with a0, a1 (rows, h) contiguous and
 * act (rows, 2h) at row stride act_stride.  Replaces SiLU + torch.cat + product at
 * nnUNetTrainer_MLAgg_2D_dt_MS.py:888, 899, 902.  Backward overwrites da0, da1 (rows, h) and dact (rows, 2h).
 * ------------------------------------------------------------------------------------------ */
int mlagg_gate_fwd(const float *a0, const float *a1, const float *act, int act_stride, float *out, long rows, int h,
                   void *stream);
int mlagg_gate_bwd(const float *dout, int dout_stride, const float *a0, const float *a1, const float *act, int act_stride,
                   float *da0, float *da1, float *dact, int dact_stride, long rows, int h, void *stream);

/* ------------------------------------------------------------------------------------------
 * K8: small fused ops.
 * diff_lambda: lam[0] = exp(<q1, k1>) - exp(<q2, k2>) + lambda_init over n-element vectors (the differential-attention
 * lambda of nnUNetTrainer_MLAgg_2D_dt_MS.py:709-711 / 770-772); saved_exp[2] receives the two exponentials for the
 * backward, which overwrites dq1, dk1, dq2, dk2 (n each) from dlam[0].
 * scaled_residual: out = skip + branch * scale[b] for b in [0, batch), per_sample floats per sample (multiple of 4),
 * everything contiguous -- the residual under timm DropPath (T:903, 907; MambaSkip.py:741, 745), scale = mask / keep.
 * skip == NULL computes out = branch * scale[b] (the branch gradient).
 * ------------------------------------------------------------------------------------------ */
int mlagg_diff_lambda_fwd(const float *q1, const float *k1, const float *q2, const float *k2, float lambda_init, int n,
                          float *lam, float *saved_exp, void *stream);
int mlagg_diff_lambda_bwd(const float *dlam, const float *q1, const float *k1, const float *q2, const float *k2,
                          const float *saved_exp, int n, float *dq1, float *dk1, float *dq2, float *dk2, void *stream);
int mlagg_scaled_residual(const float *skip, const float *branch, const float *scale, float *out, int batch,
                          long per_sample, void *stream);
/* transpose_2d: dst[b][c][r] = src[b][r][c], (batch, R, C) -> contiguous (batch, C, R); src matrices contiguous, src_batch_stride
 * elements apart (0 = R * C; a channel slice of an NCHW map has a larger one): the NCHW <-> token-major flips
 * (`x.flatten(2).transpose(1, 2)` / its inverse at nnUNetTrainer_MLAgg_2D_dt_MS.py:878-880, 910; MambaSkip.py:727-733, 747-751). */
int mlagg_transpose_2d(const float *src, long src_batch_stride, float *dst, int batch, int R, int C, void *stream);
/* ... with the results dst_batch_stride floats apart (0 = R * C): the gradient of a channel slice of an NCHW map written where the
 * map's gradient lives (the halves of `x.split([48, C - 48], dim=1)` in MambaSkip.py:727-733 share one gradient buffer). */
int mlagg_transpose_2d_into(const float *src, long src_batch_stride, float *dst, long dst_batch_stride, int batch, int R, int C,
                            void *stream);
/* pixel_shuffle2: dst (B, O, 2 H, 2 W)[b][o][2 i + a][2 j + c] = src (B, 4 O, H, W)[b][(2 a + c) O + o][i][j]; inverse != 0: the other
 * way round (src is the (B, O, 2 H, 2 W) map).  Around K18 this is the kernel-2 / stride-2 transposed convolution of UnetrUpBlock
 * (nnUNetTrainer_MLAgg_2D_dt_MS.py:1340-1368) and its backward.  W even, both pointers 16-byte aligned, contiguous maps. */
int mlagg_pixel_shuffle2(const float *src, float *dst, int B, int O, int H, int W, int inverse, void *stream);
/* ... the inverse with the (B, O, 2 H, 2 W) source a channel slice of a wider map: src_batch floats between samples (0: contiguous) */
int mlagg_pixel_unshuffle2_strided(const float *src, long src_batch, float *dst, int B, int O, int H, int W, void *stream);
/* Bias gradients.  channel_sum: out[c] = sum over batch and pixels of an NCHW gradient map g (B, C, HW) -- the bias gradient of
 * the convolutions around the path (torch computes it with a generic reduction inside convolution_backward); workspace:
 * mlagg_channel_sum_workspace_floats(B, C) floats.  column_sum: out[c] = sum_r x[r][c], x (rows, cols) at row stride x_stride --
 * the bias gradient of the Linear layers whose GEMMs go to the library (few tokens); workspace: mlagg_column_sum_workspace_floats(rows,
 * cols) floats (0 for short matrices; NULL: single launch, one workgroup per 64 columns). */
size_t mlagg_channel_sum_workspace_floats(int B, int C);
int mlagg_channel_sum(const float *g, float *out, float *workspace, int B, int C, long HW, void *stream);
size_t mlagg_column_sum_workspace_floats(int rows, int cols);
int mlagg_column_sum(const float *x, int x_stride, float *out, float *workspace, int rows, int cols, void *stream);

/* ------------------------------------------------------------------------------------------
 * K1' for volumes: cross-scan / cross-merge by permutation table, the re-ordering of the 3-D selective scan
 * (`SS3D.forward_corev0`, mlagg/nnunetv2/training/nnUNetTrainer/variants/mamba/UMambaEnc_SS3D.py:244-296: K = 12 directions
 * = six axis orders of (D, H, W) and their reversals; the stack / permute / flip / cat chains at :251-259 and :284-295).
 *   idx  (K, L) int32: natural (d, h, w) position of scan step l of direction k
 *   scan   seq[b][k * CB + c][l] = tok[b][idx[k][l]][k * blk_stride + c]       tok (B, L, *) rows of tok_stride floats
 *   merge  the transpose; blk_stride = 0 sums the K directions into the same CB columns (tok_stride must equal CB; float
 *          atomics: the sum order is not fixed)
 * ------------------------------------------------------------------------------------------ */
int mlagg_index_scan(const float *tok, long tok_stride, int blk_stride, const int *idx, float *seq, int B, int L, int K, int CB,
                     void *stream);
int mlagg_index_merge(const float *seq, const int *idx, float *tok, long tok_stride, int blk_stride, int B, int L, int K, int CB,
                      void *stream);
/* out (rows, CB) = sum of the K column blocks of wide (rows, K * CB), in a fixed order (CB % 4 == 0): with
 * mlagg_index_merge(blk_stride = CB) the deterministic form of the summed merge (torch.sum(y, dim=1), UMambaEnc_SS3D.py:338). */
int mlagg_block_sum(const float *wide, float *out, long rows, int K, int CB, void *stream);

/* ------------------------------------------------------------------------------------------
 * K1f: the whole of SS2D_skip.forward_corev0 behind x_proj (reference MambaSkip.py:405-473) + the four-way sum of M:534 on
 * TOKEN-MAJOR tensors: the four scan orders of every scale (M:414-422), the dt einsum (M:430-436), `selective_scan_fn(xs, dts,
 * As, Bs, Cs, Ds, z=None, delta_bias, delta_softplus=True)` (M:445-451) and the inverse re-orderings (M:455-471) in the scan
 * kernels' own address arithmetic -- no scan-order copy of x, of the projections or of any gradient exists.
 * Fixed shape (every MLAgg-UNet configuration): 4 directions, d_inner 96, d_state 16, dt_rank 3; L % 4 == 0
 * (mlagg_msmm_scan_supported says whether a shape qualifies; others take mlagg_cross_scan + mlagg_selscan_lowrank_*).
 *   xc    (B, L, 96)   conv outputs of all scales concatenated, natural token order (u of all four directions)
 *   xdbl  (B, L, 144)  x_proj output with the weight rows laid out per direction as [dt0 dt1 dt2 0 | B(16) | C(16)]
 *   idx   (4, L) int32 token visited by direction k at scan position t (k = 0: row-major, 1: column-major, 2 / 3: their reversals
 *         inside every scale; scales concatenated in the same order for every direction); every entry must be in [0, L)
 *   Wdt (384, 3) dt_projs_weight; A (384, 16) = -exp(A_logs); D (384) or NULL; delta_bias (384) or NULL
 *   y     (B, L, 96)   sum over the four directions at the token's natural position
 *   state saved for backward (mlagg_msmm_scan_state_floats); workspace: the per-direction outputs before the sum
 * Backward overwrites dxc (B, L, 96), dxdbl (B, L, 144: every column, the pad columns with zeros), dWdt, dA and, when non-NULL,
 * dD, ddelta_bias.  No atomics: bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
int mlagg_msmm_scan_supported(int d_inner, int d_state, int dt_rank, int directions, int L);
size_t mlagg_msmm_scan_state_floats(int batch, int L);
size_t mlagg_msmm_scan_fwd_workspace_floats(int batch, int L);
size_t mlagg_msmm_scan_bwd_workspace_floats(int batch, int L);
int mlagg_msmm_scan_fwd(const float *xc, const float *xdbl, const int *idx, const float *Wdt, const float *A, const float *D,
                        const float *delta_bias, float *y, float *state, float *workspace, int batch, int L, void *stream);
int mlagg_msmm_scan_bwd(const float *xc, const float *xdbl, const int *idx, const float *Wdt, const float *A, const float *D,
                        const float *delta_bias, const float *dy, const float *state, float *dxc, float *dxdbl, float *dWdt,
                        float *dA, float *dD, float *ddelta_bias, float *workspace, int batch, int L, void *stream);

/* ------------------------------------------------------------------------------------------
 * K1s: selective scan with ONE state per channel on token-major volumes, scan orders applied inside the kernels.
 * Replaces, for the reference's 3-D network (variants/mamba/UMambaEnc_SS3D.py: `SS3D` built with d_state = 1 at :640-655),
 * everything of `SS3D.forward_corev0` (:244-296) behind x_proj: the copies that build the K = 12 scan sequences of u
 * (:251-259), the dt einsum (:264), `selective_scan_fn(xs, dts, As, Bs, Cs, Ds, z=None, delta_bias, delta_softplus=True)`
 * (:277-283) and the inverse permutations (:285-296); the caller finishes `torch.sum(y, dim=1)` (:338) with mlagg_block_sum.
 *   tok   (B, L, C) conv output u in natural (d, h, w) token order, rows of tok_stride floats; C % 64 == 0
 *   idx   (K, L) int32: token visited at step l of direction k
 *   dtr   (B, K, R, L), Bs, Cs (B, K, L): x_proj's output in scan order (mlagg_index_scan); R in {1, 2, 3, 4, 8, 16, 20}
 *   Wdt   (K*C, R) dt_projs_weight; A (K*C) = -exp(A_logs); D (K*C); bias (K*C) dt_projs_bias
 *   yk    (B, L, K, C): y of direction k at the natural position of its token
 *   state saved for backward, mlagg_selscan1_state_floats() floats: chunk-entry states, chunk sums of delta, states entering
 *         every 16-step tile
 * Backward: dout (B, L, C) (rows of dout_stride floats) = gradient of the K-way sum; writes duk (B, L, K, C) (the caller sums the
 * K blocks), ddtr / dBs / dCs in scan order, and dparams (K*C, 3 + R) = [dA | dD | dbias | dWdt] per channel.
 * mlagg_selscan1_chunk: the chunk length the kernels cut L into (diagnostics).
 * ------------------------------------------------------------------------------------------ */
int mlagg_selscan1_chunk(int B, int L, int K);
size_t mlagg_selscan1_state_floats(int B, int L, int C, int K);
int mlagg_selscan1_fwd(const float *tok, long tok_stride, const int *idx, const float *dtr, const float *Bs, const float *Cs,
                       const float *Wdt, int R, const float *A, const float *D, const float *bias, float *yk, float *state,
                       int B, int L, int C, int K, void *stream);
size_t mlagg_selscan1_bwd_workspace_floats(int B, int L, int C, int K, int R);
int mlagg_selscan1_bwd(const float *tok, long tok_stride, const int *idx, const float *dtr, const float *Bs, const float *Cs,
                       const float *Wdt, int R, const float *A, const float *D, const float *bias, const float *dout,
                       long dout_stride, const float *state, float *duk, float *ddtr, float *dBs, float *dCs, float *dparams,
                       float *workspace, int B, int L, int C, int K, void *stream);

/* ------------------------------------------------------------------------------------------
 * K13: epilogue of the library convolutions on NCHW maps (B, C, HW): y = act(x + bias[c] + res), act 0 = none (in place on
 * x, y ignored), 1 = GELU (erf form; x is overwritten with the pre-activation, y receives the result).  Replaces the
 * bias add / GELU / residual add chain behind the convolutions of MedNeXtBlock, MedNeXtDownBlock, PatchExpand and project
 * (nnUNetTrainer_MLAgg_2D_dt_MS.py:307-324, 358-366, 498-546, 984-1001).  bias, res may be NULL.
 * Backward of the GELU form: dpre = dy * gelu'(pre), dbias[c] = sum of dpre over batch and pixels (NULL to skip;
 * workspace: mlagg_channel_sum_workspace_floats(B, C) floats).
 * ------------------------------------------------------------------------------------------ */
int mlagg_channel_epilogue_fwd(float *x, const float *bias, const float *res, float *y, int B, int C, long HW, int act,
                               void *stream);
int mlagg_channel_gelu_bwd(const float *pre, const float *dy, float *dpre, float *dbias, float *workspace, int B, int C,
                           long HW, void *stream);
/* The same epilogue in the 16-bit modes, with the element type of every map in memory as an argument (MLAGG_DTYPE_*; HW % 4 == 0):
 * x is the bf16 / fp16 output of the library convolution and is left untouched, y = act(x + bias[c] + res) is written in y_dtype
 * (16-bit when only the next 16-bit convolution reads it, fp32 when it joins the residual stream): no cast kernels on either side
 * of the convolution.  Backward: dx = dy * act'(x + bias + res) in dx_dtype (the convolution's gradient operand) and dbias in one
 * pass (act 0: x / bias / res may be NULL).  Arithmetic fp32. */
int mlagg_channel_epilogue_lp_fwd(const void *x, int x_dtype, const float *bias, const void *res, int res_dtype, void *y, int y_dtype,
                                  int B, int C, long HW, int act, void *stream);
int mlagg_channel_epilogue_lp_bwd(const void *x, int x_dtype, const float *bias, const void *res, int res_dtype, const void *dy,
                                  int dy_dtype, void *dx, int dx_dtype, float *dbias, float *workspace, int B, int C, long HW, int act,
                                  void *stream);

/* ------------------------------------------------------------------------------------------
 * K9: Dice + cross-entropy statistics and gradient of one deep-supervision level.  Replaces softmax, one-hot scatter,
 * masked products, spatial sums, log_softmax + nll and all their backward kernels of DC_and_CE_loss
 * (loss/compound_losses.py:31-57, loss/dice.py:73-117, loss/robust_ce_loss.py:12-16).
 * logits (B, C, HW) fp32, 2 <= C <= mlagg_dice_ce_max_classes(); target (B, HW) float labels in [0, C).
 * stats: stats_ip[b][0][c] = sum_p softmax_c [y == c], stats_ip[b][1][c] = sum_p softmax_c,
 * stats_g[b][c] = sum_p [y == c], ce_sum[0] = sum_{b,p} -log softmax_y.
 * grad: dlogits = d(loss)/d(logits) for upstream gradients g_ip (B, 2, C) of stats_ip and g_ce[0] of ce_sum (device scalars:
 * no host synchronisation).
 * ignore_label >= 0: pixels carrying that label take no part in any sum and get a zero gradient -- the loss mask of
 * DC_and_CE_loss(ignore_label=...) (loss/compound_losses.py:38-50; the number of valid pixels is sum_{b,c} stats_g); -1: none.
 */
int mlagg_dice_ce_max_classes(void);
/*
 * stats OVERWRITES its three outputs: per-workgroup partial rows in `workspace` (mlagg_dice_ce_stats_workspace_floats floats) are
 * summed in a fixed order -- the value of the loss is bit-reproducible from run to run.
 * ------------------------------------------------------------------------------------------ */
size_t mlagg_dice_ce_stats_workspace_floats(int B, int C, long HW);
int mlagg_dice_ce_stats(const float *logits, const float *target, float *stats_ip, float *stats_g, float *ce_sum,
                        float *workspace, int B, int C, long HW, int ignore_label, void *stream);
int mlagg_dice_ce_grad(const float *logits, const float *target, const float *g_ip, const float *g_ce, float *dlogits, int B,
                       int C, long HW, int ignore_label, void *stream);

/* ------------------------------------------------------------------------------------------
 * K33: top-k cross-entropy of one deep-supervision level -- TopKLoss (loss/robust_ce_loss.py:19-32: the mean of the k largest
 * per-pixel cross-entropies, k = int(N kpercent / 100) of the N = B HW pixels, ignored ones counted) alone or, with the Dice
 * statistics of K9 from the same pass, DC_and_topk_loss (loss/compound_losses.py:103-151) -- the losses of the reference's
 * nnUNetTrainerTopk10Loss, nnUNetTrainerTopk10LossLS01 and nnUNetTrainerDiceTopK10Loss (variants/loss/nnUNetTrainerTopkLoss.py).
 * Replaces log_softmax + nll, the device-wide torch.topk, the mean and their backward kernels.  Tensors and layout as K9's.
 *
 * stats:  one pass over the logits.  ce_pix (B HW) receives CrossEntropyLoss(reduction='none', ignore_index, label_smoothing) per pixel:
 *         (1 - e)(lse - z_y) + (e / C) sum_c (lse - z_c), exactly 0.0f where the pixel carries ignore_label.  stats_ip, stats_g, ce_sum
 *         and workspace (mlagg_dice_ce_stats_workspace_floats floats) are K9's, with K9's ignore semantics and fixed-order partial rows
 *         (ce_sum is the plain, unsmoothed sum); all four NULL (the pure top-k trainers): the Dice work is skipped.
 * select: the exact k-th largest value t of ce_pix (n = B HW values, 1 <= k <= n; the host refuses k = 0, where the reference
 *         returns NaN) by a radix select on an order-preserving integer image of the floats (-0 and +0 are one key): per digit one
 *         histogram launch (integer atomics, LDS then global: independent of the order of arrival) and one single-workgroup launch
 *         that picks the bin; then the values above t are summed as one double per workgroup, added in a fixed order.  record
 *         (mlagg_topk_ce_record_floats() = 8 four-byte words, 8-byte aligned) receives
 *             float t | float share = (k - n_gt) / n_eq | float topk_sum = sum_{ce > t} ce + (k - n_gt) t | float topk_sum / k |
 *             int64 n_gt = #{ce > t} | int64 n_eq = #{ce == t}.
 *         workspace: mlagg_topk_ce_select_workspace_bytes(n) bytes, 8-byte aligned.  No workgroup waits on another one, no float
 *         atomics, nothing is read back: bit-reproducible and capturable.
 * grad:   dlogits = p_k (g_k - sum_c p_c g_c)  [K9's Dice term, g_c = gI[b][c] [y == c] + gP[b][c]; left out when g_ip is NULL]
 *                   + g_topk[0] w_p / k ((1 - e)(p_k - [y == k]) + e (p_k - 1 / C)),
 *         w_p = 1 where ce_pix > t, share where ce_pix == t, 0 below; ignored pixels get 0.  g_ip, g_topk: device tensors as in
 *         mlagg_dice_ce_grad (g_topk is the upstream gradient of topk_sum / k).
 * Ties at the threshold share the weight that remains, k - n_gt, equally: a valid subgradient of the sum of the k largest values,
 * free of any order and the same in every run.  torch.topk's choice among equal values is unspecified and differs between its own
 * back ends, so gradients of tied pixels may differ from a torch run; the value does not.
 * MLAGG_E_NULLPTR for a missing pointer, MLAGG_E_UNSUPPORTED for C outside 2 .. mlagg_dice_ce_max_classes(), k outside 1 .. n or a
 * label smoothing outside [0, 1].
 * ------------------------------------------------------------------------------------------ */
int mlagg_topk_ce_record_floats(void);
int mlagg_topk_ce_select_elements_per_workgroup(void);
size_t mlagg_topk_ce_select_workspace_bytes(long n);
int mlagg_topk_ce_stats(const float *logits, const float *target, float *stats_ip, float *stats_g, float *ce_sum, float *ce_pix,
                        float *workspace, int B, int C, long HW, int ignore_label, float label_smoothing, void *stream);
int mlagg_topk_ce_select(const float *ce_pix, float *record, void *workspace, long n, long k, void *stream);
int mlagg_topk_ce_grad(const float *logits, const float *target, const float *ce_pix, const float *record, const float *g_ip,
                       const float *g_topk, float *dlogits, int B, int C, long HW, long k, int ignore_label, float label_smoothing,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * K10: per-plane normalisation of an NCHW map fused with the activation that follows it:
 *   y = act((x - mean_bc) * rstd_bc * gamma_c + beta_c),  statistics over the HW pixels of each (batch, channel) plane.
 * gamma / beta (C) may be NULL (1 / 0).  act: 0 none, 1 LeakyReLU(slope), 2 SiLU.  res (B, C, HW) or NULL is added before the
 * activation (the residual sum of the UnetResBlock, MambaSkip.py:662-666): y = act(norm(x) + res); backward then also writes
 * dres (may be NULL).  Replaces nn.GroupNorm(C, C)
 * (nnUNetTrainer_MLAgg_2D_dt_MS.py:268-270, 357, 500-502), nn.InstanceNorm2d + LeakyReLU(0.01) of the MONAI UnetResBlock
 * (T:1339-1357; structure at MambaSkip.py:581-667) and nn.InstanceNorm2d(affine) + SiLU (MambaSkip.py:700-706).
 * stats (B*C, 2) receives mean and rstd for the backward, which overwrites dx and, when non-NULL, dgamma / dbeta (C);
 * also nn.InstanceNorm3d(affine) + LeakyReLU of the 3-D network (variants/mamba/UMambaEnc_SS3D.py:477-513): planes of 256 Ki
 * elements and more are cut into 16 Ki-element segments, one workgroup each, with exact pooled statistics.
 * workspace: mlagg_plane_norm_fwd_workspace_floats / _bwd_workspace_floats(B, C, HW) floats (forward: 0 floats -- NULL allowed --
 * unless the planes are cut into segments; backward: needed with dgamma / dbeta or segments).
 * ------------------------------------------------------------------------------------------ */
size_t mlagg_plane_norm_fwd_workspace_floats(int B, int C, long HW);
/* x_dtype / res_dtype / y_dtype (forward), x_dtype / dy_dtype / res_dtype (backward; dx has x's type, dres res's): MLAGG_DTYPE_F32,
 * _BF16 or _F16 -- the element type of each map IN MEMORY (arithmetic and statistics are fp32).  In the 16-bit modes a map that only
 * a 16-bit library convolution reads or wrote is kept 16-bit (the reference's autocast tensors, nnUNetTrainer.py:848): no cast
 * kernels around the convolutions, half the bytes through this kernel. */
int mlagg_plane_norm_fwd(const void *x, const float *gamma, const float *beta, const void *res, void *y, float *stats,
                         float *workspace, int B, int C, long HW, float eps, int act, float slope, int x_dtype, int res_dtype,
                         int y_dtype, void *stream);
size_t mlagg_plane_norm_bwd_workspace_floats(int B, int C, long HW);
int mlagg_plane_norm_bwd(const void *x, const void *dy, const float *gamma, const float *beta, const void *res, const float *stats,
                         void *dx, void *dres, float *dgamma, float *dbeta, float *workspace, int B, int C, long HW, int act,
                         float slope, int x_dtype, int dy_dtype, int res_dtype, void *stream);
/* ... with dy a channel slice of a wider map (the halves of `torch.cat([up, skip], 1)`'s gradient, T:1360-1366): dy_batch elements
 * between samples, a multiple of HW (0: contiguous) -- no copy of the slice in front of the kernel. */
int mlagg_plane_norm_bwd_strided(const void *x, const void *dy, long dy_batch, const float *gamma, const float *beta, const void *res,
                                 const float *stats, void *dx, void *dres, float *dgamma, float *dbeta, float *workspace, int B, int C,
                                 long HW, int act, float slope, int x_dtype, int dy_dtype, int res_dtype, void *stream);

/* ------------------------------------------------------------------------------------------
 * K4lp: pooled differential attention on the 16-bit matrix cores (fp32 tensors in memory; q * scale, k, v, the softmax weights and
 * d(o) rounded to bf16 / fp16 operands, fp32 sums / softmax / RMSNorm).  Replaces, under the reference's autocast step, the four
 * `flash_attn_func(q_j, k_j, v_i, causal=False)` launches of the pooled branch, the lambda subtraction, RMSNorm and 0.2 gain
 * (nnUNetTrainer_MLAgg_2D_dt_MS.py:733-760) and their backward.  Layouts and strides as mlagg_pooled_attn_fwd / _bwd; P <= 320.
 * Saved for backward: lse (B, N, nh, 2) and the two maps' own outputs o1 = P1 v, o2 = P2 v (B, N, d) (NULL, NULL, NULL: inference).
 * dtype: MLAGG_DTYPE_BF16 / MLAGG_DTYPE_F16.  Backward overwrites dq, dkp, dvp, dlam[1], dsubln_w[48]; fixed summation order.
 * ------------------------------------------------------------------------------------------ */
int mlagg_pooled_attn_lp_fwd(const float *q, int q_stride, const float *kp, int kp_stride, const float *vp, int vp_stride,
                             const float *lam, const float *subln_w, float *out, int out_stride, float *lse, float *o1, float *o2,
                             int batch, int N, int P, int nh, float scale, int dtype, void *stream);
size_t mlagg_pooled_attn_lp_bwd_workspace_floats(int batch, int N, int P, int nh);
int mlagg_pooled_attn_lp_bwd(const float *q, int q_stride, const float *kp, int kp_stride, const float *vp, int vp_stride,
                             const float *lam, const float *subln_w, const float *dout, int dout_stride, const float *lse,
                             const float *o1, const float *o2, float *dq, int dq_stride, float *dkp, int dkp_stride, float *dvp,
                             int dvp_stride, float *dlam, float *dsubln_w, float *workspace, int batch, int N, int P, int nh,
                             float scale, int dtype, void *stream);

/* ------------------------------------------------------------------------------------------
 * K15: weight gradient of the full convolutions on channel-major maps as tap GEMMs on the fp32 matrix cores.  Replaces MIOpen's
 * weight-gradient solvers behind the backward of `nn.Conv3d` / `nn.Conv2d` (kernel 3 with padding 1, or kernel 1; stride 1 or 2) of
 * the 3-D network's BasicResBlock / BasicBlockD / UpsampleLayer / seg layers (variants/mamba/UMambaEnc_SS3D.py:49-66, 477-513,
 * 589-637, 744-779) and of the 2-D network's 3x3 / 1x1 convolutions (nnUNetTrainer_MLAgg_2D_dt_MS.py:976-977, 278-296; MambaSkip.py:703).
 *   mlagg_conv_pad_geometry: box (Dq, Hq, Wq) and guard (floats in front of and behind every channel row) of the padded copies for an
 *       input of (D, H, W) voxels (D = 1: a 2-D map, stride 1 only).
 *   mlagg_volume_pad: src (B, C, D, H, W) -> dst (B, phases, C, 2 * guard + Dq * Hq * Wq): zero-padded copy (stride 1: one phase, data
 *       at origin 1) or the 8 parity phases of the zero-padded input (stride 2).  as_output = 1: an output-sized map (out_D, out_H,
 *       out_W) laid into the box of the input geometry (D, H, W) with a zero ring (origin 1 for stride 1, 0 for stride 2).
 *   wide = 1 (stride 1, W % 4 == 0): the data starts at x = 4 (Wq = W + 8): aligned groups of 4 padded voxels are aligned groups of 4
 *       data voxels -- the geometry mlagg_conv_taps needs; K15 works on either.
 *   mlagg_conv_wgrad_taps: dW (O, I, ntaps) (+)= sum_{b, q < Q} A[b][o][q] * B[b][i][q + tap_off[t]].  Q and the row strides are
 *       multiples of 4 floats (Q of 8), tap_off is a HOST array of ntaps <= 27 element offsets; workspace of
 *       mlagg_conv_wgrad_taps_workspace_floats() floats.  fp32 in, fp32 MFMA (exact products), fixed summation order.
 * ------------------------------------------------------------------------------------------ */
int mlagg_conv_pad_geometry(int D, int H, int W, int stride, int wide, int *Dq, int *Hq, int *Wq, long *guard);
int mlagg_volume_pad(const float *src, float *dst, int B, int C, int D, int H, int W, int stride, int wide, int as_output, int out_D,
                     int out_H, int out_W, void *stream);
size_t mlagg_conv_wgrad_taps_workspace_floats(int batch, long Q, int O, int I, int ntaps);
/* K16: forward / data gradient of the same convolutions (stride 1; kernel 3 pad 1 or kernel 1) on the padded copy (wide form):
 * y (B, O, D, H, W) = sum_t sum_i weight[o * w_so + i * w_si + t'] * xp[b][i][q + tap_off[t]], t' = t (flip 0) or ntaps - 1 - t (flip 1: the data
 * gradient, with w_so / w_si exchanged by the caller).  Replaces MIOpen's Conv3d forward / backward-data behind BasicResBlock / BasicBlockD /
 * UpsampleLayer / seg layers of the 3-D network (UMambaEnc_SS3D.py:49-66, 477-513, 589-637, 744-779).  fp32 MFMA, exact products. */
int mlagg_conv_taps(const float *xp, long x_batch, long x_row, const float *weight, long w_so, long w_si, int flip, const long *tap_off,
                    int ntaps, float *y, int B, int O, int I, int D, int H, int W, void *stream);
int mlagg_conv_wgrad_taps(const float *A, long a_batch, long a_row, const float *B, long b_batch, long b_row, const long *tap_off,
                          int ntaps, long Q, int O, int I, int batch, float *dW, int accumulate, float *workspace, void *stream);
/* The launch geometry of mlagg_conv_wgrad_taps (host arithmetic, what the launcher itself decides with): out5 = {slab: voxels per
 * wave; nslabs; tap groups of at most nine taps; 32-wide tiles along O; along I}.  0, or the error of the launch for these sizes. */
int mlagg_conv_wgrad_taps_geometry(int batch, long Q, int O, int I, int ntaps, int *out5);
/* The launch geometry of mlagg_conv_taps: out4 = {Q: voxels of the padded box; workgroups of 512 voxels; 32-row output tiles; bytes
 * of the LDS weight image}.  0, or the error of the launch for these sizes. */
int mlagg_conv_taps_geometry(int O, int I, int D, int H, int W, int ntaps, long *out4);

/* ------------------------------------------------------------------------------------------
 * K5, round-4 form (csrc/linear_x3.hip): y (M, N) = x (M, K) . W (N, K)^T for token-major activations, fp32 in / out, split-bf16
 * products (three exact bf16 pieces per operand, six partial products, fp32 accumulation: the error of an fp32 GEMM).  Replaces the
 * forward and data-gradient GEMMs behind every token-major nn.Linear of the path (nnUNetTrainer_MLAgg_2D_dt_MS.py:176-192, 687-690,
 * 719-723, 887-907; MambaSkip.py:518, 538, 559-577) at every token count.
 * The weight operand is an IMAGE: mlagg_weight_image lays the three bf16 pieces of W (N, K) out as img[piece][n][k] with rows padded
 * with zeros to a multiple of 32 (mlagg_weight_image_bytes(N, K) bytes) and, if img_t is non-NULL, the same for W^T (K, N)
 * (mlagg_weight_image_bytes(K, N) bytes): the operand of the data gradient dx (M, K) = dy (M, N) . W = mlagg_linear_x3(dy, img_t, ...,
 * N_gemm = K, K_gemm = N).  mlagg_weight_images builds the images of a whole network in one launch from a device table of rows
 * {const float *w; void *img; void *img_t; int32 N, K, w_stride, pad} (40 bytes each); max_tiles >= ceil(N / 32) * ceil(K / 32) of
 * every row.  K % 8 == 0 (mlagg_linear_x3_supported).
 * epilogue 0: y = x W^T + bias (bias may be NULL); 1: y = x W^T + bias AND y_act = GELU(y) (exact, erf: Mlp fc1 + nn.GELU, T:188-190);
 * 2: y = (x W^T) * GELU'(pre) (the data gradient that flows back through that GELU; bias ignored).
 * ------------------------------------------------------------------------------------------ */
size_t mlagg_weight_image_bytes(int rows, int cols);
int mlagg_weight_image(const float *w, int w_stride, void *img, void *img_t, int N, int K, void *stream);
int mlagg_weight_images(const void *jobs, int n_jobs, int max_tiles, void *stream);
int mlagg_linear_x3_supported(int M, int N, int K);
/* nw * 10 + tn of the default dispatch (workgroup = nw waves of 32 rows x tn column tiles of 32: 22, 42, 23 or 43; host arithmetic, the
 * launcher's own rule), MLAGG_E_UNSUPPORTED where mlagg_linear_x3_supported is 0. */
int mlagg_linear_x3_tile(int M, int N, int K);
int mlagg_linear_x3(const float *x, int x_stride, const void *w_image, const float *bias, float *y, int y_stride, float *y_act,
                    const float *pre, int pre_stride, int M, int N, int K, int epilogue, void *stream);

/* ------------------------------------------------------------------------------------------
 * K11 / K34 / K35: clip_grad_norm_(parameters, 12) + optimizer.step() of the train step (nnUNetTrainer.py:855-857) for every
 * parameter in three launches: sum of squares per work item, their fixed-order total, update.
 * tensor_table: device array of rows {param*, grad*, state0*, state1*, int64 numel} (5 x 8 bytes each): state0 is exp_avg or
 * SGD's momentum_buffer, state1 exp_avg_sq (not read by SGD: may be null).  extra_table: device array of one pointer per table row,
 * the third state tensor max_exp_avg_sq of ADAMW_AMSGRAD; not read by the other kinds (may be null).
 * work_list: device array of int32 pairs (tensor index, chunk index), one per mlagg_adamw_chunk_elements() elements.  The float4
 * path is taken by a work item whose param, grad and state pointers (those its kind has) are all 16-byte aligned.
 * sumsq: 1 + n_work device doubles (scratch: [0] the squared global norm, then one partial per work item, summed in a fixed
 * order: bit-reproducible).  max_norm > 0: gradients are scaled by coef = min(1, max_norm / (||g||_2 + 1e-6)) as they are
 * read (the global norm is formed on the device; no host synchronisation; gradients in memory stay unscaled); <= 0: no clipping.
 * kind:
 *   MLAGG_OPT_SGD_NESTEROV   torch.optim.SGD(momentum, nesterov=True, dampening 0, L2 weight decay): the base trainer's optimizer
 *                            (nnUNetTrainer.py:448-452; K34).  g = coef g + wd p; buf = momentum buf + g; p -= lr (g + momentum buf);
 *                            a zero buffer gives torch's first step (buf = g).  beta1 carries the momentum; beta2, eps, step unused.
 *   MLAGG_OPT_ADAMW_AMSGRAD  torch.optim.AdamW(amsgrad=True) of nnUNetTrainerAdam (variants/optimizer/nnUNetTrainerAdam.py; K34):
 *                            decoupled decay; vmax = max(vmax, v); denom = sqrt(vmax) / sqrt(bias_c2) + eps.
 *   MLAGG_OPT_ADAM_L2        torch.optim.Adam of nnUNetTrainerVanillaAdam (K34): g = coef g + wd p before the moments, no decoupled
 *                            decay.
 *   MLAGG_OPT_ADAMW          torch.optim.AdamW, amsgrad off, of nnUNetTrainer_MLAgg_2D_dt_MS.py:137-147 (K11): decoupled decay;
 *                            extra_table is not read.
 * beta1, beta2 are doubles.  ADAMW rounds them to float first and forms everything from the float values: the moment weights beta and
 * 1.f - beta, the bias corrections 1 - pow((double)(float)beta, step).  ADAMW_AMSGRAD and ADAM_L2 form the bias corrections
 * 1 - beta^step from the doubles, as torch does (beta2 = 0.999 rounded to float is 1.3e-8 off, its 1000th power 1.3e-5, which a
 * learning rate of 1e-2 carries into the parameters), and use beta and 1 - beta each rounded to float from the double in the moment
 * updates, the weights torch hands to its kernels.
 * mlagg_optimizer_clip_step is the launch-argument form: step is the 1-based step count for the bias corrections (>= 1 for the Adam
 * kinds; ignored by SGD).  mlagg_optimizer_clip_step_dev is the form for a hipGraph capture of the whole train step (B:833-863
 * replayed as one graph): nothing that changes between steps is a launch argument.  lr_dev: one device float (the schedule writes it
 * between replays, B:825); step_dev: one device int32, advanced by the call for every kind before the bias corrections read it (SGD
 * does not read it: it counts the steps that replays have taken).  With max_norm <= 0 the norm pass is skipped, the counter still
 * moves.
 *
 * mlagg_scaled_clip_step_dev (K35) is the device form with fp16 loss scaling (torch.amp.GradScaler of the reference's default train
 * step, nnUNetTrainer.py:152, :848-858: scaled backward, unscale_, clip_grad_norm_ 12, step, update) fused into the same three
 * launches, for every kind, with nothing decided on the host.  The gradients of the table carry the loss scale.  Device-resident
 * state, one element each:
 *   scale (float), growth_tracker (int32), found_inf (float, 0 or 1 as torch keeps it); grad_mult: one scratch float.
 * 1. sum of squares of the UNSCALED gradients, (g * inv)^2 with inv = (float)(1.0 / (double)scale): the norm the reference clips on;
 * 2. reduce (fixed order): found_inf = the total is not finite -- any inf / NaN element, and (the one deviation from torch, which
 *    would step with a zero coefficient) finite elements whose unscaled square, or a work item's fp32 sum of such squares, leaves
 *    fp32 (|g / scale|, or the norm of a 64 Ki-element chunk of it, above 1.8e19); a good step advances step_dev, a skipped one does not; grad_mult = inv * min(1, max_norm / (norm + 1e-6)) (inv alone with max_norm <= 0);
 *    then torch._amp_update_scale_: overflow: scale *= backoff_factor, tracker 0; else the tracker counts up and at growth_interval
 *    scale *= growth_factor if that is finite, tracker 0;
 * 3. update: returns at once when found_inf is set (parameters and state stay bit-identical), else the arithmetic of the kind with
 *    grad_mult where the clip coefficient stood.  Gradients stay SCALED and unclipped in memory.
 * With scale 1.0 and no overflow the results equal those of the unscaled entry points bit for bit.
 * ------------------------------------------------------------------------------------------ */
#define MLAGG_OPT_SGD_NESTEROV 0
#define MLAGG_OPT_ADAMW_AMSGRAD 1
#define MLAGG_OPT_ADAM_L2 2
#define MLAGG_OPT_ADAMW 3
int mlagg_adamw_chunk_elements(void);
int mlagg_optimizer_clip_step(int kind, const void *tensor_table, const void *extra_table, const void *work_list, int n_work,
                              double *sumsq, float lr, double beta1, double beta2, float eps, float weight_decay, float max_norm, int step,
                              void *stream);
int mlagg_optimizer_clip_step_dev(int kind, const void *tensor_table, const void *extra_table, const void *work_list, int n_work,
                                  double *sumsq, const float *lr_dev, int *step_dev, double beta1, double beta2, float eps,
                                  float weight_decay, float max_norm, void *stream);
int mlagg_scaled_clip_step_dev(int kind, const void *tensor_table, const void *extra_table, const void *work_list, int n_work,
                               double *sumsq, const float *lr_dev, int *step_dev, float *scale, int *growth_tracker, float *found_inf,
                               float *grad_mult, double beta1, double beta2, float eps, float weight_decay, float max_norm,
                               double growth_factor, double backoff_factor, int growth_interval, void *stream);

/* ------------------------------------------------------------------------------------------
 * K20: 3-D sliding-window inference (reference nnunetv2/inference/sliding_window_prediction.py:60-210 for a 3-D tile_size).
 * fp32 throughout, Z the contiguous axis, 64-bit volume offsets.  flips: HOST array of the V mirror variants (V in {1, 2, 4, 8}),
 * each a bitmask of flipped tile axes (bit a = axis a), in the reference's order none, 0, 1, 2, (0,1), (0,2), (1,2), (0,1,2)
 * restricted to the requested axes (maybe_mirror_and_predict :87-115).
 *   gather:   vol (C, X, Y, Z) padded input -> out (V * n, C, tx, ty, tz), variant-major then tile, variant v flipped along its axes.
 *             origins: HOST array of n (x, y, z) tile origins; every tile must lie inside the volume.  Replaces `data[sl][None]`
 *             (:193) and the torch.flip input copies of :97-114.
 *   fold:     for tile `tile` of a chunk output out (V * n, K, tx, ty, tz) at origin (ox, oy, oz): s = out_0 + flip_1(out_1) + ...
 *             in variant order, s /= V, acc[k, o + p] += s * gauss[p], w[o + p] += gauss[p]; acc (K, X, Y, Z), w (X, Y, Z).  Replaces
 *             the flipped output copies and their sum (:97-115) and the accumulation (:200-201).  One call per tile, in tile order:
 *             the overlapping tiles accumulate in the reference's order, whatever the chunking.
 *   finalize: logits (K, X0, Y0, Z0) = acc / w on the region starting at (lx, ly, lz), contiguous (:203, :206); labels
 *             (X0, Y0, Z0) int64 = argmax over K with torch.argmax's first-maximum rule, or NULL.
 *
 * K32: the gather of a cascaded stage (3d_cascade_fullres).  The reference stacks the one-hot encoding of the previous stage's
 * segmentation below the image channels, `np.vstack((data, seg_onehot))` with `result[i] = seg == l`
 * (inference/predict_from_raw_data.py:47-67, utilities/label_handling/label_handling.py:266-270, and nnUNetTrainer.py:1099-1101 in
 * validation; the segmentation comes from inference/export_prediction.py:74-106), and cuts tiles from that volume of 4 L X Y Z bytes.
 *   gather_onehot: vol (C, X, Y, Z) fp32 and seg (X, Y, Z) contiguous labels of seg_kind (MLAGG_SEG_INT8 / _UINT8 / _INT16, read as
 *             they are: any byte alignment, no conversion pass) -> out (V * n, C + L, tx, ty, tz).  Channels 0 .. C-1 are those of
 *             gather, bit for bit; channel C + i is 1.0f where the label at the same (flipped) source voxel equals labels[i], else
 *             0.0f.  labels: HOST array of L values in 1 .. 255, 1 <= L <= MLAGG_CASCADE_MAX_LABELS (64).  origins, flips, V as in
 *             gather.  Every label is read once for its L outputs; the one-hot volume never exists.
 * No atomics: bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
#define MLAGG_SEG_INT8  0
#define MLAGG_SEG_UINT8 1
#define MLAGG_SEG_INT16 2
int mlagg_sw_gather_onehot(const float *vol, int C, const void *seg, int seg_kind, const int *labels, int L, int X, int Y, int Z,
                           const int *origins, int n, const int *flips, int V, float *out, int tx, int ty, int tz, void *stream);
int mlagg_sw_gather(const float *vol, int C, int X, int Y, int Z, const int *origins, int n, const int *flips, int V, float *out,
                    int tx, int ty, int tz, void *stream);
int mlagg_sw_fold(const float *out, int tile, int n, const int *flips, int V, int K, const float *gauss, int tx, int ty, int tz,
                  int ox, int oy, int oz, float *acc, float *w, int X, int Y, int Z, void *stream);
int mlagg_sw_finalize(const float *acc, const float *w, int K, int X, int Y, int Z, int lx, int ly, int lz, int X0, int Y0, int Z0,
                      float *logits, long long *labels, void *stream);

/* ------------------------------------------------------------------------------------------
 * K21: prediction export on the device (reference nnunetv2/inference/export_prediction.py:10-69 with the default
 * resample_data_or_seg_to_shape(is_seg=False, order=1, order_z=0), preprocessing/resampling/default_resampling.py:76-200).
 * Logits (C|K, X, Y, Z) fp32 with element strides (sc, sx, sy, sz) >= 0: any view.  tap_idx (X' + Y' + Z', 2) int32 and
 * tap_w (X' + Y' + Z', 2) fp64 are DEVICE tables built by export._axis_taps: for output index o of an axis, the two source
 * indices (inside the input's extent along that axis) and their weights; x entries first, then y, then z.  The kernels blend the
 * eight taps separably (z, then y, then x) in fp64 and round once to fp32.
 *   resample_linear:     out (C, X', Y', Z') contiguous fp32 (16-byte aligned).  Replaces resample_data_or_seg_to_shape (:76-200).
 *   export_segmentation: K <= 32 classes; box_lo, shape, perm are HOST arrays of 3: the bbox's lower corner and
 *                        shape_before_cropping in the preprocessed axis order, and transpose_backward.  The box has extent
 *                        (X', Y', Z').  labels (shape[perm[0]], shape[perm[1]], shape[perm[2]]) uint8 (4-byte aligned) = argmax
 *                        of the fp32 softmax of the resampled logits inside the box, 0 outside; probs (K, same) fp32 or NULL,
 *                        0 outside the box.  Replaces the resampling, convert_logits_to_segmentation, the paste, revert_cropping
 *                        and the transposes of export_prediction.py:36-63.
 * No atomics: bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
int mlagg_resample_linear(const float *in, int C, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz,
                          const int *tap_idx, const double *tap_w, float *out, int Xo, int Yo, int Zo, void *stream);
int mlagg_export_segmentation(const float *logits, int K, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz,
                              const int *tap_idx, const double *tap_w, int Xc, int Yc, int Zc, const int *box_lo, const int *shape,
                              const int *perm, unsigned char *labels, float *probs, void *stream);
/* export_segmentation_regions: the same resampling, paste and transpose for the K <= 32 sigmoid heads of a region-based label manager
 * (label_handling.py:46-47, 166-173): per voxel the fp32 sigmoid of every resampled logit; the label starts at 0 and takes
 * regions_class_order[i] where sigmoid_i > 0.5, for i = 0 .. K-1 in order (the last match wins; a logit of exactly 0 does not fire).
 * regions_class_order is a HOST array of K values in 0 .. 255; probs (optional) are the sigmoids, 0 outside the box. */
int mlagg_export_segmentation_regions(const float *logits, int K, int X, int Y, int Z, long long sc, long long sx, long long sy,
                                      long long sz, const int *tap_idx, const double *tap_w, int Xc, int Yc, int Zc, const int *box_lo,
                                      const int *shape, const int *perm, const int *regions_class_order, unsigned char *labels,
                                      float *probs, void *stream);

/* ------------------------------------------------------------------------------------------
 * K22: case preprocessing on the device (reference nnunetv2/preprocessing/preprocessors/default_preprocessor.py:38-124 for a
 * test case: crop to non-zero (preprocessing/cropping/cropping.py), normalise (normalization/default_normalization_schemes.py),
 * resample_data_or_seg_to_shape(order=3, order_z=0 | 1) (resampling/default_resampling.py:76-200)).  The raw input is
 * (C, X, Y, Z) fp32 with element strides (sc, sx, sy, sz) >= 0 (the transpose_forward view); lo / ext are HOST arrays of 3:
 * the crop window's lower corner and extent.
 *   nonzero_box:     box (6 ints, DEVICE) = min x, y, z and max x, y, z of the voxels != 0 in any channel ((INT_MAX, -1) when
 *                    there are none).  Integer atomics: deterministic.
 *   channel_stats:   channel c of the window (voxels with mask != 0 for MLAGG_PP_ZSCORE_MASKED; mask (ext) uint8, contiguous):
 *                    stats[c * 4 .. + 3] = fp64 mean, std, min, max; for ZScore params[c * 4 + 2 | 3] = fp32 mean and
 *                    max(std, 1e-8), for RescaleTo01 params[c * 4 + 0 | 3] = min and max(max - min, 1e-8).  partials:
 *                    C * MLAGG_PP_STATS_PARTIALS * 5 doubles of workspace.  Fixed summation order: bit-reproducible.
 *   normalize:       out (C, ext) contiguous fp32 = scheme schemes[c] (DEVICE int array of C) of the window in fp32, with
 *                    params[c * 4 ..] (DEVICE): CT (lo, hi, mean, den) = (clip(x, lo, hi) - mean) / den; ZScore (.., .., mean, den);
 *                    masked ZScore the same where mask != 0, x elsewhere; RescaleTo01 (min, .., .., den); RGBTo01 x / 255.
 *   clip_ranges:     lo / hi (C * D ordered-int encoded fp32) = min / max of x (C, X, Y, Z) contiguous per channel (axis -1,
 *                    D = 1) or per channel and slice along axis (D = its extent): the ranges skimage's resize clips to.
 *   cubic_axis:      one axis of ndi.zoom(order=3, mode='nearest', grid_mode=True) in fp64 on (outer, n_in, inner) contiguous
 *                    fp32 | fp64 -> (outer, n_out, inner) fp32 | fp64: out[o] = sum_k w[4 o + k] * coef[start[o] + k], where coef
 *                    is the line edge-padded by 12, prefiltered by the HOST array fir[0..30] (h[|k|]) with the reflect boundary; start / w are
 *                    DEVICE tables, every start[o] in [P0, P0 + M - 4], P0 + M <= n_in + 24; clip_lo / clip_hi (clip_ranges
 *                    output or NULL) clip the output element f to domain (f / clip_cstride) * clip_D + (f / clip_dstride) % clip_D.
 *                    Lines longer than the LDS plan allows (mlagg_pp_cubic_lines_per_block == 0) are MLAGG_E_UNSUPPORTED.
 *   gather_axis:     (outer, n_in, inner) fp64 -> (outer, n_out, inner) fp32: in[idx[2 o]] * w[2 o] + in[idx[2 o + 1]] * w[2 o + 1]
 *                    (export._axis_taps tables, DEVICE): map_coordinates(order=0 | 1, mode='nearest') along the low-resolution
 *                    axis of separate-z resampling (:172-184).
 * All volume offsets are 64-bit.
 * ------------------------------------------------------------------------------------------ */
#define MLAGG_PP_NONE          0
#define MLAGG_PP_CT            1
#define MLAGG_PP_ZSCORE        2
#define MLAGG_PP_ZSCORE_MASKED 3
#define MLAGG_PP_RESCALE01     4
#define MLAGG_PP_RGB01         5
#define MLAGG_PP_STATS_PARTIALS 256
int mlagg_pp_nonzero_box(const float *in, int C, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz, int *box,
                         void *stream);
int mlagg_pp_channel_stats(const float *in, int C, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz,
                           const int *lo, const int *ext, int c, int scheme, const unsigned char *mask, double *partials,
                           float *params, double *stats, void *stream);
int mlagg_pp_normalize(const float *in, int C, int X, int Y, int Z, long long sc, long long sx, long long sy, long long sz,
                       const int *lo, const int *ext, const int *schemes, const float *params, const unsigned char *mask, float *out,
                       void *stream);
int mlagg_pp_clip_ranges(const float *x, int C, int X, int Y, int Z, int axis, unsigned *lo, unsigned *hi, void *stream);
int mlagg_pp_cubic_lines_per_block(int n_in, int M);
int mlagg_pp_cubic_axis(const void *in, int in_f64, void *out, int out_f64, long long outer, int n_in, long long inner, int n_out,
                        const int *start, const double *w, int P0, int M, const double *fir, const unsigned *clip_lo,
                        const unsigned *clip_hi, long long clip_cstride, long long clip_dstride, int clip_D, void *stream);
int mlagg_pp_gather_axis(const double *in, float *out, long long outer, int n_in, long long inner, int n_out, const int *idx,
                         const double *w, void *stream);

/* ------------------------------------------------------------------------------------------
 * K26: the segmentation of a TRAINING case and ordered rank selection on the device (reference default_preprocessor.py:38-124
 * with a seg_file, and experiment_planning/dataset_fingerprint/fingerprint_extractor.py:39-103).  Label volumes are int16;
 * max_label (0..32767) is the largest label the caller expects.  hist (max_label + 3 counters, DEVICE, or NULL) is zeroed and
 * filled in the same pass: hist[l + 1] = voxels of label l for l = -1 .. max_label, hist[max_label + 2] = voxels of any other
 * label (the caller's error check).
 *   seg_crop:     seg (X, Y, Z) with element strides (sx, sy, sz) >= 0 (the transpose_forward view); lo / ext HOST arrays of 3 (the
 *                 K22 crop window); mask (ext) uint8 contiguous, the filled non-zero mask.  out (ext) contiguous = the window of
 *                 seg, with -1 where seg == 0 and mask == 0 (cropping.py:24-49, crop_to_nonzero with a segmentation).
 *   seg_resize:   in (X, Y, Z) contiguous -> out (Xo, Yo, Zo) contiguous: batchgenerators' resize_segmentation(order=1) as
 *                 resample_data_or_seg (default_resampling.py:122-212) calls it.  tap_idx / tap_w: DEVICE tables of
 *                 (Xo + Yo + Zo, 2) ints / doubles, the two source indices (inside the axis) and weights of every output index,
 *                 axis after axis (export._axis_taps 'linear'; 'nearest' for the low-resolution axis of a separate-z case, whose
 *                 second weight is 0, which is the in-plane rule on the slice map_coordinates(order=0) picks).  out = the largest
 *                 label whose fp64 weight sum over the 8 source voxels is >= 0.5, else 0 (the reference starts from zeros and
 *                 writes the labels in ascending order, -1 included).
 *   rank_rows:    rows of the rank table for N voxels: ceil(N / MLAGG_PP_RANK_BLOCK).
 *   rank_counts:  seg (N) contiguous; groups (max_label + 2 DEVICE 64-bit words): bit g of groups[l + 1] set when label l
 *                 (-1 .. max_label) is in group g < n_groups <= MLAGG_PP_MAX_GROUPS.  table (rank_rows(N), n_groups) int64 =
 *                 per group, the number of group voxels in the rows before this one (exclusive scan of the per-row counts);
 *                 totals (n_groups) = the voxels of each group.  No atomics: bit-reproducible.
 *   rank_select:  for i < n_ranks: the voxel of C-order rank ranks[i] (DEVICE) among the voxels of `group`, i.e.
 *                 np.argwhere(mask)[ranks] (default_preprocessor.py:134-161).  coords (n_ranks, 4) int64 = (0, x, y, z) with
 *                 (Y, Z) the two last extents of seg, or NULL; values (C, n_ranks) fp32 = image[c, x, y, z] of an image with
 *                 element strides (sc, sx, sy, sz) >= 0 (images[c][mask][ranks], fingerprint_extractor.py:58-67), or NULL with
 *                 image NULL.  A rank outside [0, totals[group]) gives coords of -1 and no value.
 * All volume offsets are 64-bit.
 * ------------------------------------------------------------------------------------------ */
#define MLAGG_PP_RANK_BLOCK 2048
#define MLAGG_PP_MAX_GROUPS 64
int mlagg_pp_seg_crop(const short *seg, int X, int Y, int Z, long long sx, long long sy, long long sz, const int *lo, const int *ext,
                      const unsigned char *mask, short *out, int max_label, unsigned long long *hist, void *stream);
int mlagg_pp_seg_resize(const short *in, int X, int Y, int Z, const int *tap_idx, const double *tap_w, short *out, int Xo, int Yo,
                        int Zo, int max_label, unsigned long long *hist, void *stream);
size_t mlagg_pp_rank_rows(long long N);
int mlagg_pp_rank_counts(const short *seg, long long N, const unsigned long long *groups, int max_label, int n_groups,
                         long long *table, long long *totals, void *stream);
int mlagg_pp_rank_select(const short *seg, long long N, int Y, int Z, const unsigned long long *groups, int max_label, int n_groups,
                         int group, const long long *table, const long long *totals, const long long *ranks, long long n_ranks,
                         long long *coords, const float *image, int C, long long sc, long long sx, long long sy, long long sz,
                         float *values, void *stream);

/* ------------------------------------------------------------------------------------------
 * K23: keep the largest connected component (reference nnunetv2/postprocessing/remove_connected_components.py:22-34,
 * remove_all_but_largest_component_from_segmentation, with acvl_utils' remove_all_but_largest_component: full connectivity, every
 * component of the maximal size kept).  labels (X, Y, Z) contiguous uint8, X * Y * Z <= 2^31 - 1 (else MLAGG_E_UNSUPPORTED before
 * any launch), 4-byte aligned; group (256) uint8 DEVICE table: group[label] = 0 outside every mask, else the voxel's group.  Two
 * voxels are connected when they are 26-neighbours with the same non-zero group: all listed labels -> 1 is the reference's
 * united mask (foreground or a region); label -> label labels every class at once.
 *   out (X, Y, Z) uint8 (4-byte aligned) = background_label (0..255) where group != 0 and the voxel's component is smaller than
 *   the largest of its group; labels elsewhere.  parent, size: X * Y * Z int32 each of workspace.  stats (3 * 256 int32, DEVICE)
 *   = per group: voxel count, largest component size, voxels kept (slot 0 unused).
 * Six launches, integer atomics only: the result does not depend on the schedule.
 * ------------------------------------------------------------------------------------------ */
int mlagg_keep_largest_component(const unsigned char *labels, int X, int Y, int Z, const unsigned char *group, int background_label,
                                 int *parent, int *size, int *stats, unsigned char *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * K24: normalized surface Dice (reference evaluation/SurfaceDice.py:280-425 compute_surface_distances, :470-479
 * compute_surface_dice_at_tolerance, and the per-organ loops of evaluation/{abdomen,BTCV,ACDC,endoscopy}_NSD_Eval.py :90-110).
 * gt, pred (X, Y, Z) contiguous uint8 label volumes indexed [x, y, z].  Three calls per case, two small read-backs by the caller:
 *
 * mlagg_surface_stats: wanted (256) uint8 DEVICE table (1 for the labels to measure, label 0 never); stats (256 x 10 int32, DEVICE)
 *   per label value l: stats[10 l + 0..9] = gt voxels, prediction voxels, union box x min / max, y min / max, z min / max (min
 *   INT_MAX and max -1 when empty), gt z min / max.  One pass over both volumes (per-block LDS partials, one atomic per block).
 *
 * mlagg_surface_prepare: desc (n_labels x 16 int64, DEVICE), per label: label, crop origin o0..o2 in the volume, mask extents n0..n2
 *   (the union box, a slab label's cut to the gt's [z_lower, z_upper) included), then the exclusive prefix offsets of the crop
 *   voxels (D0 D1 D2, D = n + 1: the reference's zero plane on the high side), of the z lines (D0 D1), the y lines (D0 D2) and the
 *   x lines (D1 D2), and of the (distance, area) pairs of the gt and the prediction surfels (used by mlagg_surface_reduce when it
 *   compacts).  total / zlines / ylines: the sums; max_crop: the largest crop's voxel count.  Every crop <= 2^31 - 1 voxels and
 *   every D <= MLAGG_SURFACE_MAX_LINE (nmax_y: the largest D1), else MLAGG_E_UNSUPPORTED before any launch.
 *   codes (2 x total uint8) = the 2x2x2 neighbour codes of the gt, then of the prediction; ft (2 x total int32) = the exact
 *   feature transform of each surfel set after the z and y passes (packed fy * D2 + fz of the nearest feature in the x plane, -1
 *   where that plane has none); counts (n_labels x 2 int32) = surfels of the gt and the prediction.  s1, s2: spacing (mm).
 *
 * mlagg_surface_reduce: the x pass at the other mask's surfels.  tol (n_labels float64, DEVICE), area (256 float64, DEVICE: the
 *   surfel area of every code at this spacing).  partial: 4 x xlines float64 of workspace.  sums (n_labels x 4 float64) = gt surfel
 *   area, gt area within tol of the prediction's surface, prediction surfel area, prediction area within tol of the gt's surface,
 *   each a fixed-order sum (bit-identical on a repeated call).  pairs (optional, NULL: off): (distance, area) float64 pairs of every
 *   surfel at desc's pair offsets, in no particular order (pair_count: n_labels x 2 int32 of workspace).  Distance +inf where the
 *   other mask has no surfel.  Inference only: no graph capture.
 * ------------------------------------------------------------------------------------------ */
#define MLAGG_SURFACE_STATS_PER_LABEL 10
#define MLAGG_SURFACE_DESC_FIELDS 16
#define MLAGG_SURFACE_MAX_LINE 2560
int mlagg_surface_stats(const unsigned char *gt, const unsigned char *pred, int X, int Y, int Z, const unsigned char *wanted,
                        int *stats, void *stream);
int mlagg_surface_prepare(const unsigned char *gt, const unsigned char *pred, int X, int Y, int Z, const long long *desc, int n_labels,
                          long long total, long long max_crop, long long zlines, long long ylines, int nmax_y, double s1, double s2, unsigned char *codes,
                          int *ft, int *counts, void *stream);
int mlagg_surface_reduce(const unsigned char *codes, const int *ft, const long long *desc, int n_labels, long long total,
                         long long xlines, int nmax_x, const double *tol, const double *area, double s0, double s1, double s2,
                         double *partial, double *sums, double *pairs, int *pair_count, void *stream);

/* ------------------------------------------------------------------------------------------
 * K25: 3-D spatial augmentation of a training batch (batchgenerators augment_spatial / interpolate_img for a 3-D patch, the
 * SpatialTransform of nnUNetTrainer.get_training_transforms, nnUNetTrainer.py:666-677; no elastic deformation, random_crop False).
 * vol (B, C, Xi, Yi, Zi) fp32: per sample the cubic B-spline coefficients (scipy's "mirror" prefilter) where resample[b] != 0, the
 * raw data where it is 0.  lab (B, 1, Xi, Yi, Zi) int16 labels as the loader delivers them (-1 padding included), or NULL.
 * affine: HOST array of B x 12 float64, row-major 3 x 4 per sample: input coordinate j = A[j][3] + A[j][0] x + A[j][1] y + A[j][2] z
 * for output voxel (x, y, z).  resample: HOST array of B ints.
 *   resampled sample: out = cubic B-spline of vol at that coordinate (taps mirror-indexed), 0 where the coordinate leaves
 *                     [0, n - 1] on any axis; out_lab = the largest label whose trilinear indicator (8 taps, mirror-indexed) is
 *                     >= 0.5, 0 where none is or outside.
 *   cropped sample:   out / out_lab = the centre crop starting at ((Xi - Xo) / 2, (Yi - Yo) / 2, (Zi - Zo) / 2); needs Xo <= Xi ...
 * out (B, C, Xo, Yo, Zo) fp32, out_lab (B, 1, Xo, Yo, Zo) fp32 (required with lab).  All contiguous.  No atomics: bit-reproducible.
 * C = 0 with lab: labels only (vol and out are not read or written, and may be NULL): a further seg channel of the same batch.
 * ------------------------------------------------------------------------------------------ */
int mlagg_aug3d_resample(const float *vol, const short *lab, int B, int C, int Xi, int Yi, int Zi, const double *affine,
                         const int *resample, float *out, float *out_lab, int Xo, int Yo, int Zo, void *stream);

/* ------------------------------------------------------------------------------------------
 * K31: the same transform for an anisotropic patch, "dummy 2-D" augmentation (Convert3DTo2DTransform, the 2-D SpatialTransform on
 * (B, C * X, Y, Z) and Convert2DTo3DTransform of nnUNetTrainer.get_training_transforms, nnUNetTrainer.py:658-680, chosen by
 * do_dummy_2d_data_aug, nnUNetTrainer.py:380): every slice x is resampled in its own (y, z) plane, X is never resampled.
 * vol (B, C, X, Yi, Zi) fp32: per sample the cubic B-spline coefficients prefiltered along Y and Z ONLY where resample[b] != 0, the
 * raw data where it is 0.  lab (B, 1, X, Yi, Zi) int16 or NULL.  affine: HOST array of B x 6 float64, row-major 2 x 3 per sample:
 * input y = A[0][2] + A[0][0] y + A[0][1] z, input z = A[1][2] + A[1][0] y + A[1][1] z for output pixel (y, z) of every slice and
 * channel.  resample: HOST array of B ints.
 *   resampled sample: out = cubic B-spline of the slice at that coordinate (16 taps, mirror-indexed), 0 where the coordinate leaves
 *                     [0, n - 1] on either axis; out_lab = the largest label whose bilinear indicator (4 taps) is >= 0.5, 0 where
 *                     none is or outside.  The arithmetic is K25's with the x axis removed.
 *   cropped sample:   out / out_lab = the centre crop starting at ((Yi - Yo) / 2, (Zi - Zo) / 2) of every slice; needs Yo <= Yi ...
 * out (B, C, X, Yo, Zo) fp32, out_lab (B, 1, X, Yo, Zo) fp32 (required with lab).  All contiguous; Yi * Zi and Yo * Zo < 2^31.
 * No atomics: bit-reproducible.  C = 0 with lab: labels only (vol and out may be NULL), as K25.
 * ------------------------------------------------------------------------------------------ */
int mlagg_aug3d_resample_planar(const float *vol, const short *lab, int B, int C, int X, int Yi, int Zi, const double *affine,
                                const int *resample, float *out, float *out_lab, int Yo, int Zo, void *stream);

/* ------------------------------------------------------------------------------------------
 * K27: cell-instance F1 evaluation (reference evaluation/compute_cell_metric.py: skimage.measure.label(seg == 1), dice,
 * remove_boundary_cells, relabel_sequential, _label_overlap, _intersection_over_union and the threshold test of _true_positive).
 * All maps are contiguous int32 (H, W) unless said otherwise, H * W <= 2^31 - 1, labels >= 0.  Integer atomics only: every result
 * is independent of the schedule.
 *
 * mlagg_cells_label: seg (H, W) of elem_bytes 1 (uint8) or 4 (int32); parent (H * W int32) = the linear index of the first pixel in
 *   raster order of the pixel's 8-connected component of {seg == foreground}, -1 elsewhere.  gt (optional, NULL: off): counts
 *   (3 int32, DEVICE) = |gt > 0|, |seg == foreground|, |both|; without gt only counts[1].  Three launches.
 *
 * mlagg_cells_relabel: order-preserving compaction over a view.  key = keys[r * stride + c] + bias for r < h, c < w (bias 1 turns a
 *   parent map into keys, 0 is the background); keys lie in [0, D), D <= 2^31.  The view stands for an Hr x Wr image whose other
 *   pixels are zero padding (Hr >= h, Wr >= w).  ring != 0: every key seen in that image's 2-pixel ring (rows 0, 1, Hr - 2, Hr - 1,
 *   columns alike; needs Hr, Wr >= 5) is dropped, as remove_boundary_cells does.  out (h x w contiguous) = 1 + the number of kept
 *   smaller keys for a kept key, 0 otherwise; total[0] = the number of kept keys.  Workspace: flags (2 * D bytes), newid (D int32),
 *   blocksum (mlagg_cells_scan_blocks(D) int32).  Five launches.
 *
 * mlagg_cells_overlap: overlap ((n_true + 1) x (n_pred + 1) int32) = pixel counts of every (g, p) label pair, area_t (n_true + 1)
 *   and area_p (n_pred + 1) = its row and column sums; pixels with a label outside the matrix are not counted.  The matrix may take
 *   at most MLAGG_CELLS_MAX_OVERLAP_BYTES (else MLAGG_E_UNSUPPORTED before any launch).
 *
 * mlagg_cells_match: iou (optional, (n_true + 1) x (n_pred + 1) float64) = ov / (area_t + area_p - ov), 0 where that is 0 / 0.
 *   thresholds: HOST array of n_thresholds <= MLAGG_CELLS_MAX_THRESHOLDS float64.  edges == NULL: stats (4 x
 *   MLAGG_CELLS_MAX_THRESHOLDS int32, DEVICE), per threshold t: stats[4 t + 0..2] = the number of pairs i, j >= 1 with iou >= th, the
 *   largest number of them in one row and in one column (0 for "at most one"); degrees: MLAGG_CELLS_MAX_THRESHOLDS x (n_true +
 *   n_pred + 2) int32 of workspace.  edges != NULL (n_thresholds == 1): edges (edge_cap x 2 int32) = the pairs (i - 1, j - 1) in no
 *   particular order, stats[3] = their number.
 * ------------------------------------------------------------------------------------------ */
#define MLAGG_CELLS_MAX_THRESHOLDS 8
#define MLAGG_CELLS_MAX_OVERLAP_BYTES 1073741824
int mlagg_cells_label(const void *seg, int elem_bytes, int foreground, const int *gt, int H, int W, int *parent, int *counts,
                      void *stream);
size_t mlagg_cells_scan_blocks(long long D);
int mlagg_cells_relabel(const int *keys, int bias, long long stride, int h, int w, int Hr, int Wr, int ring, long long D,
                        unsigned char *flags, int *newid, int *blocksum, int *total, int *out, void *stream);
int mlagg_cells_overlap(const int *g, const int *p, int h, int w, int n_true, int n_pred, int *overlap, int *area_t, int *area_p,
                        void *stream);
int mlagg_cells_match(const int *overlap, const int *area_t, const int *area_p, int n_true, int n_pred, const double *thresholds,
                      int n_thresholds, double *iou, int *degrees, int *stats, int *edges, int edge_cap, void *stream);

/* ------------------------------------------------------------------------------------------
 * K28: ensembling and model selection (reference ensembling/ensemble.py and evaluation/evaluate_predictions.py).
 *
 * mlagg_ensemble_mean: average_probabilities (ensemble.py:17-29) and the argmax that merge_files (:32-46) takes of it, in one pass.
 *   table (DEVICE, M x 2 int64): per member the device address of its contiguous (K, N) array and its element size in bytes, 4 (fp32)
 *   or 2 (fp16); the address is a multiple of the element size.  M >= 1 (unbounded), 2 <= K <= MLAGG_ENSEMBLE_MAX_CLASSES, N >= 1.
 *   Per voxel and class: acc = float(m_0); acc = acc + float(m_i), i = 1 .. M - 1 in table order; acc = acc / float(M) (IEEE fp32
 *   division): numpy's arithmetic to the bit.  labels (N uint8) = the first class whose mean is the maximum; a NaN counts as a maximum
 *   and the first NaN wins (numpy's argmax).  mean (optional, NULL: not written; (K, N) fp32) = the means.  No atomics, no LDS.
 *
 * mlagg_ensemble_mean_regions: the same mean, in the same order, of the sigmoid probabilities of a region-based label manager; the
 *   label is what convert_probabilities_to_segmentation paints from it (label_handling.py:166-173): 0, then order[k] where mean_k > 0.5
 *   for k = 0 .. K-1 in order (the last match wins).  table (DEVICE, (2 M + K) int64): the M member rows, then the K labels of
 *   regions_class_order (0 .. 255).  1 <= K <= MLAGG_ENSEMBLE_MAX_CLASSES.
 *
 * mlagg_label_confusion: the counting of compute_metrics (evaluate_predictions.py:77-120).  ref, pred (N uint8); table (DEVICE, 256
 *   uint8) maps a label value to a bin 0 .. L, where L (<= MLAGG_CONFUSION_MAX_LABELS) stands for "any other value" (entries above L
 *   count as L).  ignore (-1: none): voxels whose REFERENCE value equals it are dropped (ignore_mask = seg_ref == ignore_label).
 *   counts ((L + 1) x (L + 1) int64, zeroed here) = voxels per (reference bin, prediction bin).  tp / fp / fn / tn of a label or a
 *   region R are sums over it: tp = sum cm[a in R, b in R], fn = sum cm[a in R, b not in R], fp = sum cm[a not in R, b in R], tn =
 *   the rest.  int32 counters in LDS per workgroup, flushed with 64-bit integer atomic adds: independent of the schedule.
 * Inference only: no graph capture is needed, though neither entry allocates or synchronises.
 * ------------------------------------------------------------------------------------------ */
#define MLAGG_ENSEMBLE_MAX_CLASSES 256
#define MLAGG_CONFUSION_MAX_LABELS 63
int mlagg_ensemble_mean(const long long *table, int M, int K, long long N, unsigned char *labels, float *mean, void *stream);
int mlagg_ensemble_mean_regions(const long long *table, int M, int K, long long N, unsigned char *labels, float *mean, void *stream);
int mlagg_label_confusion(const unsigned char *ref, const unsigned char *pred, long long N, const unsigned char *table, int L,
                          int ignore, long long *counts, void *stream);

/* ------------------------------------------------------------------------------------------
 * K29: Dice + binary cross-entropy statistics and gradient of one deep-supervision level of a region-based dataset (sigmoid heads).
 * Replaces sigmoid, the masked products and spatial sums, BCEWithLogitsLoss and all their backward kernels of DC_and_BCE_loss
 * (loss/compound_losses.py:60-100 with MemoryEfficientSoftDiceLoss(do_bg=True), loss/dice.py:73-117), as the trainer builds it for
 * label managers with regions (nnUNetTrainer.py:330-336).
 * logits (B, R, HW) fp32, 1 <= R <= mlagg_dice_bce_max_regions() (otherwise MLAGG_E_UNSUPPORTED).  The target has two forms:
 *   member != NULL  target (B, HW) float labels; member (DEVICE, 256 uint32): bit r of member[v] says that label v belongs to region r
 *                   (np.isin: a label outside 0 .. 255 or in no region has no bits).  ignore_label >= 0: pixels carrying that label
 *                   have the mask m = 0; -1: none (every pixel counts, also one with a negative label, which is in no region).  What ConvertSegmentationToRegionsTransform would write is never materialised.
 *   member == NULL  target (B, R, HW) float region planes, or (B, R + 1, HW) when ignore_label >= 0: the last plane is then the
 *                   ignore indicator and m = (1 - t_last) != 0 (compound_losses.py:85-89).
 * stats: stats_ip[b][0][r] = sum_p m s_r t_r, stats_ip[b][1][r] = sum_p m s_r, stats_g[b][r] = sum_p m t_r with s = sigmoid(z);
 * sums[0] = sum_{b,r,p} m (softplus(z_r) - z_r t_r) (BCEWithLogitsLoss, unreduced), sums[1] = sum_{b,p} m (the denominator of
 * compound_losses.py:96, without a factor R).  Every value is finite for any finite logit.
 * grad: dlogits = m [ s (1 - s) (g_ip[b][0][r] t_r + g_ip[b][1][r]) + g_bce[0] (s - t_r) ] for upstream gradients g_ip (B, 2, R) of
 * stats_ip and g_bce[0] of sums[0] (device scalars: no host synchronisation).
 */
int mlagg_dice_bce_max_regions(void);
/*
 * stats OVERWRITES its outputs: per-workgroup partial rows in `workspace` (mlagg_dice_bce_stats_workspace_floats floats) are summed in
 * a fixed order, no float atomics -- the value of the loss is bit-reproducible from run to run.
 * ------------------------------------------------------------------------------------------ */
size_t mlagg_dice_bce_stats_workspace_floats(int B, int R, long HW);
int mlagg_dice_bce_stats(const float *logits, const float *target, const unsigned int *member, float *stats_ip, float *stats_g,
                         float *sums, float *workspace, int B, int R, long HW, int ignore_label, void *stream);
int mlagg_dice_bce_grad(const float *logits, const float *target, const unsigned int *member, const float *g_ip, const float *g_bce,
                        float *dlogits, int B, int R, long HW, int ignore_label, void *stream);

/* ------------------------------------------------------------------------------------------
 * K30: the cascade training transforms on bit planes (reference training/data_augmentation/custom_transforms/cascade_transforms.py,
 * as nnUNetTrainer.get_training_transforms chains them, nnUNetTrainer.py:703-718).  A plane is (X, Y, W) 64-bit words, W =
 * ceil(Z / 64): bit k of word w of row (x, y) is voxel (x, y, 64 w + k).  The padding bits of a row's last word are 0 on input and
 * on output of every entry.  X * Y * Z <= 2^31 - 1.  Integer atomics only: every result is independent of the schedule.
 *
 * mlagg_cascade_pack: MoveSegAsOneHotToData (cascade_transforms.py:23-31) without the fp32 one-hot.  seg: B label maps (X, Y, Z) of
 *   elem_bytes 2 (int16) or 4 (fp32), sample b at seg + b * sample_stride elements; labels: HOST array of L <=
 *   MLAGG_CASCADE_MAX_LABELS ints.  planes (B, L, X, Y, W): plane i = (seg == labels[i]).
 * mlagg_cascade_unpack: planes (B, L, X, Y, W) -> out[:, c0 .. c0 + L - 1] of out (B, C_total, X, Y, Z) fp32, as 0 / 1 (:31).
 *
 * mlagg_cascade_morph: binary dilation / erosion with an arbitrary small footprint (ApplyRandomBinaryOperatorTransform's
 *   skimage.morphology.binary_* calls, :118-124).  pool: n_planes planes; jobs: HOST array of n_jobs x 5 ints (source plane, destination
 *   plane, first run, number of runs, complement), all jobs in parallel: no job's destination is a source or destination of another,
 *   or its own source.  runs (DEVICE, n_runs_total x 4 int32): (dx, dy, lo, len) = the offsets (dx, dy, lo .. lo + len - 1), |dx|,
 *   |dy| <= MLAGG_CASCADE_MAX_REACH, |lo| < 64, 1 <= len <= 64, lo + len <= 64: the 128 bits a lane aligns per run (a run outside that is
 *   skipped).
 *     complement == 0: dst[p] = OR over the offsets d of src[p + d], 0 outside the volume.  With d = -(i - c) over the set entries
 *                      i of a footprint S (centre c = n // 2): scipy.ndimage.binary_dilation(src, S).
 *     complement != 0: dst[p] = AND over the offsets d of src[p + d], 1 outside.  With d = i - c:
 *                      binary_erosion(src, S, border_value=True).
 *   Closing = the erosion of the dilation, opening = the dilation of the erosion: two calls.
 * mlagg_cascade_commit: the "was added" rule (:126-134).  jobs: HOST array of n_jobs x 3 ints (result plane, target plane, first
 *   plane of the target's sample), one job per sample: the target takes the result, and result & ~(the target before) is cleared
 *   in the other L - 1 planes first .. first + L - 1.  The result plane lies outside the sample.
 *
 * mlagg_cascade_cc_stats: RemoveRandomConnectedComponentFromOneHotEncodingTransform's labelling (:65-72) of P <= 65535 planes, 26-
 *   connected.  parent (P x X Y Z int32) = the minimum linear index of the voxel's component (its rank among the roots is skimage's
 *   label order), -1 where the plane is 0; size (P x X Y Z int32) = at a root its component's voxel count; blockcnt (P x
 *   mlagg_cascade_cc_blocks(X, Y, Z) int32) workspace; table (P x 2 int32, DEVICE) = (plane non-empty, number of components with
 *   (double)size < thresh).  Five launches.
 * mlagg_cascade_cc_remove: with the arrays of mlagg_cascade_cc_stats and the same thresh: rank (DEVICE, P int32) = per plane -1 or k:
 *   the k-th component with size < thresh in root order is cleared (:77-78); fill (DEVICE, P int32): when non-zero, the same voxels
 *   are set in plane p + fill[p] (:79-83).  target (P int32) workspace.  Two launches.
 * ------------------------------------------------------------------------------------------ */
#define MLAGG_CASCADE_MAX_LABELS 64
#define MLAGG_CASCADE_MAX_REACH 8
int mlagg_cascade_pack(const void *seg, int elem_bytes, long long sample_stride, int B, int X, int Y, int Z, const int *labels, int L,
                       unsigned long long *planes, void *stream);
int mlagg_cascade_unpack(const unsigned long long *planes, int B, int L, int X, int Y, int Z, float *out, int C_total, int c0,
                         void *stream);
int mlagg_cascade_morph(unsigned long long *pool, int n_planes, int X, int Y, int Z, const int *runs, int n_runs_total, const int *jobs,
                        int n_jobs, void *stream);
int mlagg_cascade_commit(unsigned long long *pool, int n_planes, int X, int Y, int Z, int L, const int *jobs, int n_jobs, void *stream);
size_t mlagg_cascade_cc_blocks(int X, int Y, int Z);
int mlagg_cascade_cc_stats(const unsigned long long *planes, int P, int X, int Y, int Z, double thresh, int *parent, int *size,
                           int *blockcnt, int *table, void *stream);
int mlagg_cascade_cc_remove(unsigned long long *planes, int P, int X, int Y, int Z, double thresh, const int *parent, const int *size,
                            const int *blockcnt, const int *rank, const int *fill, int *target, void *stream);

/* ------------------------------------------------------------------------------------------
 * K36: the tail of the training / validation transform chain in one launch, from the augmented (data, seg) to what the loss consumes:
 * MaskTransform (custom_transforms/masking.py:18-22), RemoveLabelTransform(-1, 0), ConvertSegmentationToRegionsTransform
 * (custom_transforms/region_based_training.py:23-38) and DownsampleSegForDSTransform2 with order 0, as nnUNetTrainer.py:697-731
 * (training) and :742-757 (validation, no mask) chain them.  nd = 2 or 3 spatial axes.
 *   data (B, C, *S) fp32, DEVICE, written in place: data[b, c, p] = 0 where seg[b, 0, p] < 0 (the value BEFORE the mapping below) for
 *        every c of mask_channels (HOST array of n_mask ints in 0 .. min(C, 64) - 1; n_mask == 0: data is not touched and may be NULL).
 *        No other element of data is written, none is read.  A mask needs level 0 to be the identity (all its tables NULL).
 *   seg  (B, Sc, *S), DEVICE, fp32 (seg_kind MLAGG_TAIL_SEG_F32) or int16 (MLAGG_TAIL_SEG_INT16); only channel 0 is read.
 *   sizes: HOST array of nd ints S.  level_sizes: HOST array of L x nd ints S_l, 1 <= L <= MLAGG_TAIL_MAX_LEVELS.
 *   tables: HOST array of L x nd DEVICE pointers: tables[l * nd + a] holds S_l[a] int32 source indices into axis a (output voxel i of
 *        level l copies source voxel table[i]; an index outside 0 .. S[a] - 1 is clamped into it).  NULL: the identity on that axis,
 *        which needs S_l[a] == S[a].
 *   out: HOST array of L DEVICE pointers to fp32 maps, every element of which is written:
 *        member == NULL  (label mode)  (B, 1, *S_l): w = v < 0 ? 0 : v of the source voxel.
 *        member != NULL  (region mode) (B, R', *S_l), R' = R + (ignore_label >= 0), 1 <= R <= MLAGG_TAIL_MAX_REGIONS.  member (DEVICE,
 *                        256 uint32): bit r of member[w] says that label w belongs to region r (np.isin; a label that is no integer in
 *                        0 .. 255 has no bits).  Plane r < R is 1.0f where that bit is set, else 0.0f; plane R is w == ignore_label.
 *                        The layout K29 takes with member == NULL.
 * One launch: the grid is the concatenation of the levels' output index spaces, a thread owns four consecutive output voxels of one
 * row of one level and writes all their planes (16-byte loads and stores where the row length and the alignment allow; scalar ones
 * otherwise); level-0 threads also write the mask.  64-bit offsets, no atomics, no LDS, no workspace, no synchronisation.
 * ------------------------------------------------------------------------------------------ */
#define MLAGG_TAIL_SEG_F32   0
#define MLAGG_TAIL_SEG_INT16 1
#define MLAGG_TAIL_MAX_LEVELS 8
#define MLAGG_TAIL_MAX_REGIONS 32
int mlagg_batch_tail(float *data, int B, int C, const void *seg, int seg_kind, int Sc, int nd, const int *sizes,
                     const int *mask_channels, int n_mask, int L, const int *level_sizes, const void *const *tables, void *const *out,
                     const unsigned int *member, int R, int ignore_label, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MLAGG_HIP_H */
