"""GPU parity of the HIP token mixers and of the assembled network against the CPU oracle and the
golden vectors captured from the reference (tolerance: north_star's 1e-3 on logits, tighter per op)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mlagg_oracle as O

gpu = pytest.mark.gpu
DEV = "cuda:0"


def _close(got, ref, atol, rtol, name=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    np.testing.assert_allclose(got, ref, atol=atol * max(1.0, float(np.abs(ref).max())), rtol=rtol, err_msg=name)


def _param_grads_close(prod, orac, atol=2e-4, rtol=2e-3):
    og = {n: p.grad for n, p in orac.named_parameters() if p.grad is not None}
    pg = {n: p.grad for n, p in prod.named_parameters() if p.grad is not None}
    assert set(og) == set(pg), set(og) ^ set(pg)
    for n in og:
        _close(pg[n], og[n], atol, rtol, n)


@gpu
@pytest.mark.parametrize("C,H,W,silu", [(96, 16, 12, True), (48, 7, 9, False), (128, 32, 32, True), (4, 1, 1, False)])
def test_dwconv3x3_matches_conv2d(C, H, W, silu):
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(C + H)
    B = 2
    x = torch.randn(B, H * W, C, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.3
    b = torch.randn(C, generator=g) * 0.1
    gy = torch.randn(B, H * W, C, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    img = xr.view(B, H, W, C).permute(0, 3, 1, 2)
    ref = F.conv2d(img, wr, br, padding=1, groups=C)
    ref = (F.silu(ref) if silu else ref).permute(0, 2, 3, 1).reshape(B, H * W, C)
    ref.backward(gy)
    xg, wg, bg = [t.clone().to(DEV).requires_grad_(True) for t in (x, w, b)]
    out = ops.dwconv3x3_nlc(xg, wg, bg, H, W, silu=silu)
    out.backward(gy.to(DEV))
    _close(out, ref, 1e-5, 1e-5, "y")
    _close(xg.grad, xr.grad, 1e-5, 1e-4, "dx")
    _close(wg.grad, wr.grad, 1e-5, 1e-4, "dw")
    _close(bg.grad, br.grad, 1e-5, 1e-4, "db")


@gpu
@pytest.mark.parametrize("C,H,W,packed", [(256, 16, 12, True), (128, 7, 9, False), (512, 32, 32, True), (4, 1, 1, False)])
def test_gated_dwconv3x3_matches_conv2d_times_gate(C, H, W, packed):
    """ops.dwconv3x3_gated = SiLU(dwconv(x) + b) * v (ConvolutionalGLU, MambaSkip.py:559-577) against torch float64 on the host: output,
    dx, d(gate), dw, db; `packed`: x and the gate are the two column halves of one projection output, gradients written into its arena."""
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(C + H)
    B = 2
    xv = torch.randn(B, H * W, 2 * C, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.3
    b = torch.randn(C, generator=g) * 0.1
    gy = torch.randn(B, H * W, C, generator=g)
    xr, wr, br = xv.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    img = xr[..., :C].reshape(B, H, W, C).permute(0, 3, 1, 2)
    ref = F.silu(F.conv2d(img, wr, br, padding=1, groups=C)).permute(0, 2, 3, 1).reshape(B, H * W, C) * xr[..., C:]
    ref.backward(gy.double())
    xg, wg, bg = [t.clone().to(DEV).requires_grad_(True) for t in (xv, w, b)]
    if packed:
        a, v = ops.split_cols(xg * 1.0, (C, C))
    else:
        a, v = (xg * 1.0)[..., :C].contiguous(), (xg * 1.0)[..., C:].contiguous()
    out = ops.dwconv3x3_gated(a, v, wg, bg, H, W)
    out.backward(gy.to(DEV))
    _close(out, ref.float(), 1e-5, 1e-5, "y")
    _close(xg.grad[..., :C], xr.grad[..., :C].float(), 1e-5, 1e-4, "dx")
    _close(xg.grad[..., C:], xr.grad[..., C:].float(), 1e-5, 1e-4, "dgate")
    _close(wg.grad, wr.grad.float(), 2e-5, 1e-4, "dw")
    _close(bg.grad, br.grad.float(), 2e-5, 1e-4, "db")


@gpu
def test_residual_block_gradient_is_summed_inside_the_depthwise_backward(monkeypatch):
    """MedNeXtBlock (T:256-300): the block input feeds conv1 and the residual sum; ops.dwconv3x3_nchw_res hands both gradients to
    K2n's data-gradient kernel.  Output, input gradient and all parameter gradients equal the plain form (autograd's add_ behind the
    kernel); the input gradient's two terms are summed in the other order."""
    from mlagg_unet_amd import model, ops
    torch.manual_seed(3)
    blk = model.MedNeXtBlock(96, 96, 2).to(DEV)
    x = torch.randn(2, 96, 24, 32, device=DEV)
    gy = torch.randn(2, 96, 24, 32, device=DEV)
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "DWC_RES", fused)
        xs = x.clone().requires_grad_(True)
        for p in blk.parameters():
            p.grad = None
        y = blk(xs * 1.0)
        y.backward(gy)
        outs.append((y.detach(), xs.grad, [p.grad.clone() for p in blk.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0])
    assert float((outs[0][1] - outs[1][1]).abs().max()) < 1e-5 * float(outs[1][1].abs().max())
    for a, b in zip(outs[0][2], outs[1][2]):                   # (the library's 1 x 1 weight-gradient solvers at this size use atomics: no bit equality)
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    assert ops.dwconv3x3_nchw_res(x, blk.conv1.weight, blk.conv1.bias) is None          # no gradient wanted: the plain form


@gpu
def test_dwconv3x3_adds_the_residual_in_the_same_pass():
    """res of ops.dwconv3x3_nlc (x + lepe(v), T:782): output and all four gradients equal conv + add."""
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(3)
    B, H, W, C = 2, 9, 12, 96
    x, r = torch.randn(B, H * W, C, generator=g).to(DEV), torch.randn(B, H * W, C, generator=g).to(DEV)
    w, b = (torch.randn(C, 1, 3, 3, generator=g) * 0.3).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
    gy = torch.randn(B, H * W, C, generator=g).to(DEV)
    outs = []
    for fused in (True, False):
        xs, rs, ws, bs = [t.clone().requires_grad_(True) for t in (x, r, w, b)]
        y = ops.dwconv3x3_nlc(xs, ws, bs, H, W, silu=False, res=rs) if fused else rs + ops.dwconv3x3_nlc(xs, ws, bs, H, W, silu=False)
        y.backward(gy)
        outs.append((y, xs.grad, rs.grad, ws.grad, bs.grad))
    for a, bb in zip(*outs):
        _close(a, bb, 1e-6, 1e-6)
    with pytest.raises(RuntimeError):
        ops.dwconv3x3_nlc(x, w, b, H, W, silu=True, res=r)


@gpu
@pytest.mark.parametrize("H,W,d,r", [(16, 16, 48, 8), (8, 12, 96, 4), (6, 10, 192, 2), (4, 4, 384, 1)])
def test_gelu_pool_matches_torch(H, W, d, r):
    """K17 against nn.GELU + nn.AdaptiveAvgPool2d (T:722) in float64, on a column block of a wider row (as in the model)."""
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(H * W + d)
    B = 3
    wide = torch.randn(B, H * W, 3 * d, generator=g) * 2.0
    gy = torch.randn(B, (H // r) * (W // r), d, generator=g)
    ref_in = wide[..., 2 * d:].double().requires_grad_(True)
    img = F.gelu(ref_in).view(B, H, W, d).permute(0, 3, 1, 2)
    ref = torch.nn.AdaptiveAvgPool2d((H // r, W // r))(img).flatten(2).transpose(1, 2)
    ref.backward(gy.double())
    wg = wide.to(DEV).requires_grad_(True)
    out = ops.gelu_pool((wg * 1.0)[..., 2 * d:], H, W, r)
    out.backward(gy.to(DEV))
    _close(out, ref.float(), 2e-6, 1e-5, "pooled")
    _close(wg.grad[..., 2 * d:], ref_in.grad.float(), 2e-6, 1e-5, "ds")
    assert float(wg.grad[..., :2 * d].abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        ops.gelu_pool(wg[..., 2 * d:], H, W, r + 7)


def _attn_pair(local, dim, res, nh, sr, variant, seed):
    from mlagg_unet_amd import model as PM
    torch.manual_seed(seed)
    orac = O.AggregatedAttention(dim, res, nh, local, sr, variant)
    O.deterministic_fill_(orac.state_dict(), seed=seed)
    prod = PM.AggregatedAttention(dim, res, nh, local, sr, variant)
    prod.load_state_dict(orac.state_dict())
    return orac, prod.to(DEV)


@gpu
@pytest.mark.parametrize("local", [True, False])
@pytest.mark.parametrize("dim,res,nh,sr,variant", [
    (48, (16, 16), 1, 4, "B"),     # stage-0 geometry (one head pair)
    (192, (6, 10), 4, 2, "B"),     # 4 heads, non-square, tile edges inside the image
    (96, (9, 8), 2, 4, "A"),       # variant A scaling; 9 % 4 != 0 -> adaptive-pool fallback (pooled branch)
    (48, (1, 3), 1, 1, "B"),       # degenerate window: every token on the border
])
def test_aggregated_attention_matches_oracle(local, dim, res, nh, sr, variant):
    if not local and (res[0] // sr == 0 or res[1] // sr == 0):
        pytest.skip("no pooled keys")
    orac, prod = _attn_pair(local, dim, res, nh, sr, variant, seed=11)
    g = torch.Generator().manual_seed(5)
    B, N = 2, res[0] * res[1]
    x = torch.randn(B, N, dim, generator=g)
    gy = torch.randn(B, N, dim, generator=g)
    xo = x.clone().requires_grad_(True)
    yo = orac(xo, *res)
    yo.backward(gy)
    xp = x.clone().to(DEV).requires_grad_(True)
    yp = prod(xp)
    yp.backward(gy.to(DEV))
    _close(yp, yo, 2e-5, 1e-4, "out")
    _close(xp.grad, xo.grad, 5e-5, 1e-3, "dx")
    _param_grads_close(prod, orac)


@gpu
@pytest.mark.parametrize("variant", ["B", "A"])
@pytest.mark.parametrize("tag", ["s0", "s2"])
def test_mllablock_matches_reference_golden(golden_dir, tag, variant):
    from mlagg_unet_amd import model as PM
    g = np.load(os.path.join(golden_dir, f"mllablock_{tag}_variant{variant}.npz"))
    blk = PM.MLLABlock(int(g["dim"]), tuple(int(v) for v in g["res"]), int(g["heads"]), 2, 0.0, int(g["sr"]), variant)
    sd = blk.state_dict()
    O.deterministic_fill_(sd, seed=7)
    blk = blk.to(DEV).eval()
    x = torch.from_numpy(g["x"]).to(DEV).requires_grad_(True)
    y = blk(x)
    _close(y, g["y"], 5e-5, 1e-4, "y")
    y.backward(torch.from_numpy(g["gy"]).to(DEV))
    _close(x.grad, g["gx"], 1e-4, 1e-3, "gx")
    norms = {n: float(p.grad.double().norm()) for n, p in blk.named_parameters() if p.grad is not None}
    for n, ref in zip(g["grad_names"], g["grad_norms"]):
        assert abs(norms[str(n)] - ref) <= 2e-3 * max(ref, 1e-3), (n, norms[str(n)], ref)


@gpu
def test_msmm_matches_reference_golden(golden_dir):
    from mlagg_unet_amd import model as PM
    g = np.load(os.path.join(golden_dir, "msmm_nonsquare.npz"))
    layer = PM.VSS_Conv_Layer([96, 192, 384, 768], 48, depth=1, drop_path=0.1)
    O.deterministic_fill_(layer.state_dict(), seed=3)
    layer = layer.to(DEV).eval()
    xs = [torch.from_numpy(g[f"x{i}"]).to(DEV).requires_grad_(True) for i in range(4)]
    ys = layer(xs)
    for i, y in enumerate(ys):
        _close(y, g[f"y{i}"], 5e-5, 1e-4, f"y{i}")
    torch.autograd.backward(ys, [torch.from_numpy(g[f"gy{i}"]).to(DEV) for i in range(4)])
    for i, x in enumerate(xs):
        _close(x.grad, g[f"gx{i}"], 1e-4, 1e-3, f"gx{i}")
    sa = layer.blocks[0].self_attention
    for p, key in ((sa.A_logs, "g_A_logs"), (sa.Ds, "g_Ds"), (sa.dt_projs_bias, "g_dt_bias"),
                   (sa.x_proj_weight, "g_x_proj"), (sa.dt_projs_weight, "g_dt_w")):
        _close(p.grad, g[key], 2e-4, 2e-3, key)


@gpu
@pytest.mark.parametrize("variant", ["B", "A"])
def test_full_model_logits_match_reference_golden(golden_dir, variant):
    """north_star: segmentation logits within 1e-3 (fp32) of the reference on identical inputs."""
    from mlagg_unet_amd import model as PM
    g = np.load(os.path.join(golden_dir, f"full_model_64_variant{variant}.npz"))
    img = tuple(int(v) for v in g["img"])
    m = PM.build_network_architecture(img, 1, 14, True, variant)
    O.deterministic_fill_(m.state_dict())
    m = m.to(DEV).eval()
    data, target = O.synthetic_batch(1, 1, *img, 14, seed=int(g["data_seed"]))
    out = m(data.to(DEV))
    for i, o in enumerate(out):
        assert float((o.cpu() - torch.from_numpy(g[f"out{i}"])).abs().max()) < 1e-3, i
    from mlagg_unet_amd import trainer as TR
    loss = TR.deep_supervision_loss(out, [t.to(DEV) for t in target], batch_dice=True)
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-4
    loss.backward()
    norms = {n: float(p.grad.double().norm()) for n, p in m.named_parameters() if p.grad is not None}
    assert "dummy_tensor" not in norms
    for n, ref in zip(g["grad_names"], g["grad_norms"]):
        assert abs(norms[str(n)] - ref) <= 5e-3 * max(ref, 1e-3), (n, norms[str(n)], ref)


@gpu
def test_shims_expose_reference_import_names():
    """Plugin boundaries #2/#3: the names the reference imports resolve to the MI355X implementations."""
    from mlagg_unet_amd import shims
    shims.install()
    from flash_attn import flash_attn_func
    from mamba_ssm.ops.selective_scan_interface import selective_scan_fn
    g = torch.Generator().manual_seed(2)
    q = torch.randn(2, 50, 3, 24, generator=g).half()           # flash-attn takes fp16 / bf16 only (SURVEY finding 5)
    k = torch.randn(2, 16, 3, 24, generator=g).half()
    v = torch.randn(2, 16, 3, 24, generator=g).half()
    ref = O.softmax_attention_oracle(q.float(), k.float(), v.float())
    got = flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=False)
    assert got.dtype == torch.float16
    _close(got.float(), ref, 2e-3, 2e-3, "flash shim")
    u = torch.randn(1, 8, 40, generator=g)
    A = -torch.rand(8, 16, generator=g)
    Bm = torch.randn(1, 2, 16, 40, generator=g)
    y = selective_scan_fn(u.to(DEV), (u * 0.1).to(DEV), A.to(DEV), Bm.to(DEV), Bm.to(DEV), None, None, None, True)
    yr = O.selective_scan_oracle(u, u * 0.1, A, Bm, Bm, None, None, None, True)
    _close(y, yr, 1e-5, 1e-4, "scan shim")


@gpu
@pytest.mark.parametrize("M,O,I,bias", [(9000, 96, 96, True), (8200, 48, 96, True), (8193, 256, 48, True),
                                        (12001, 192, 384, False), (8192, 35, 50, True)])
def test_linear_wgrad_matches_torch(M, O, I, bias):
    """K5w (split-K MFMA weight gradient) against torch's matmul in float64."""
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, I, generator=g)
    w = torch.randn(O, I, generator=g) * 0.1
    b = torch.randn(O, generator=g) if bias else None
    gy = torch.randn(M, O, generator=g)
    xg = x.to(DEV).requires_grad_(True)
    wg = w.to(DEV).requires_grad_(True)
    bg = b.to(DEV).requires_grad_(True) if bias else None
    y = ops.linear(xg, wg, bg)
    y.backward(gy.to(DEV))
    dW = gy.double().t() @ x.double()
    _close(wg.grad, dW.float(), 2e-6, 1e-4, "dW")
    if bias:
        _close(bg.grad, gy.double().sum(0).float(), 2e-6, 1e-4, "db")
    _close(xg.grad, (gy.double() @ w.double()).float(), 1e-5, 1e-4, "dx")


@gpu
@pytest.mark.parametrize("rows,C,strided", [(1000, 48, False), (4097, 96, True), (513, 192, False), (130, 384, True),
                                             (77, 768, False), (5, 96, False),
                                             # the widths of the 3-D network (UMambaEnc_SS3D.py features and their 2x expansions)
                                             (3000, 32, False), (1025, 64, True), (700, 128, False), (300, 256, True),
                                             (129, 320, False), (65, 512, False), (33, 640, True)])
def test_layernorm_matches_torch(rows, C, strided):
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(rows + C)
    wide = torch.randn(rows, 2 * C, generator=g) * 2 + 0.5
    x = wide[:, C:] if strided else wide[:, :C].contiguous()
    w = torch.randn(C, generator=g) * 0.2 + 1
    b = torch.randn(C, generator=g) * 0.1
    gy = torch.randn(rows, C, generator=g)
    xr = x.clone().double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    F.layer_norm(xr, (C,), wr, br, 1e-5).backward(gy.double())
    wide_g = wide.to(DEV)
    xg = (wide_g[:, C:] if strided else wide_g[:, :C].contiguous()).detach().requires_grad_(True)
    wg, bg = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = ops.layer_norm(xg, wg, bg, 1e-5)
    y.backward(gy.to(DEV))
    _close(y, F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5).float(), 2e-6, 1e-5, "y")
    _close(xg.grad, xr.grad.float(), 5e-6, 1e-4, "dx")
    _close(wg.grad, wr.grad.float(), 5e-6, 1e-4, "dgamma")
    _close(bg.grad, br.grad.float(), 5e-6, 1e-4, "dbeta")


@gpu
@pytest.mark.parametrize("C,H,W,stride", [(96, 16, 12, 1), (48, 9, 7, 2), (8, 128, 128, 2), (5, 1, 1, 1), (7, 2, 3, 2), (4, 7, 8, 1), (3, 33, 36, 1)])
def test_dwconv3x3_nchw_matches_conv2d(C, H, W, stride):
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(C * H + stride)
    B = 2
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.3
    b = torch.randn(C, generator=g) * 0.1
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.conv2d(xr, wr, br, stride=stride, padding=1, groups=C)
    gy = torch.randn(ref.shape, generator=g)
    ref.backward(gy)
    xg, wg, bg = [t.clone().to(DEV).requires_grad_(True) for t in (x, w, b)]
    out = ops.dwconv3x3_nchw(xg, wg, bg, stride)
    out.backward(gy.to(DEV))
    _close(out, ref, 1e-5, 1e-5, "y")
    _close(xg.grad, xr.grad, 1e-5, 1e-4, "dx")
    _close(wg.grad, wr.grad, 1e-5, 1e-4, "dw")
    _close(bg.grad, br.grad, 1e-5, 1e-4, "db")


@gpu
def test_diff_lambda_matches_torch():
    """K8: lambda = exp(<q1,k1>) - exp(<q2,k2>) + lambda_init (reference T:709-711), forward and gradients."""
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(12)
    vs = [(torch.randn(24, generator=g) * 0.5).to(DEV).requires_grad_(True) for _ in range(4)]
    ref = [v.detach().clone().requires_grad_(True) for v in vs]
    lam = ops.diff_lambda(*vs, 0.8)
    want = torch.exp(torch.sum(ref[0] * ref[1])) - torch.exp(torch.sum(ref[2] * ref[3])) + 0.8
    assert abs(float(lam) - float(want)) < 1e-6
    (lam * 1.7).backward()
    (want * 1.7).backward()
    for a, b in zip(vs, ref):
        assert float((a.grad - b.grad).abs().max()) < 1e-6


@gpu
def test_scaled_residual_matches_addcmul():
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(13)
    skip = torch.randn(5, 37, 48, generator=g).to(DEV).requires_grad_(True)
    br = torch.randn(5, 37, 48, generator=g).to(DEV).requires_grad_(True)
    scale = torch.tensor([0.0, 1.25, 1.25, 0.0, 1.25], device=DEV)
    out = ops.scaled_residual(skip, br, scale)
    want = torch.addcmul(skip.detach(), br.detach(), scale.view(5, 1, 1))
    assert torch.equal(out, want) or float((out - want).abs().max()) < 1e-6
    gy = torch.randn(5, 37, 48, generator=g).to(DEV)
    out.backward(gy)
    assert torch.equal(skip.grad, gy)
    assert float((br.grad - gy * scale.view(5, 1, 1)).abs().max()) == 0.0


@gpu
def test_drop_path_pool_draws_all_masks_in_one_launch():
    """Training-mode forward: the first pass records the DropPath call order, later passes take their masks from one
    (n_calls, B) table; per-call keep probabilities follow the reference schedule (T:1096, 1235)."""
    from mlagg_unet_amd import model as PM
    torch.manual_seed(0)
    m = PM.build_network_architecture((64, 64), 1, 3, True, "B").to(DEV).train()
    x = torch.rand(4, 1, 64, 64, device=DEV)
    m(x)
    pool = m._dp_pool
    # 8 encoder blocks x 2 residuals, the first block has rate 0 (no mask): 14 calls; MSMM block: 1 + 4 calls at 0.1
    assert len(pool.order) == 19 and abs(pool.order[-1] - 0.9) < 1e-12
    assert all(abs(a - b) < 1e-6 for a, b in zip(pool.order[:2], [1 - 0.1 / 7] * 2))
    out1 = m(x)[0]
    assert pool.masks.shape == (19, 4) and pool.pos == 19
    vals = torch.unique(pool.masks[-1])
    assert all(float(v) == 0.0 or abs(float(v) - 1 / 0.9) < 1e-6 for v in vals)
    out2 = m(x)[0]
    assert torch.isfinite(out1).all() and not torch.equal(out1, out2)          # fresh masks every pass
    m.eval()
    with torch.no_grad():
        assert float((m(x)[0] - m(x)[0]).abs().max()) < 1e-4                   # no masks in eval


@gpu
@pytest.mark.parametrize("ncls,size,batch_dice", [(14, 64, True), (14, 64, False), (4, 40, True), (2, 24, False)])
def test_fused_dice_ce_loss_matches_eager(ncls, size, batch_dice):
    """K9 + the vectorised level algebra == the level-by-level torch composition of DC_and_CE_loss (the form pinned to
    the reference's loss classes by tests/golden/loss.npz on the CPU), value and gradient of every level."""
    from mlagg_unet_amd import trainer as TR
    g = torch.Generator().manual_seed(21)
    outs = [(torch.randn(3, ncls, size >> s, (size >> s) + (3 if s == 0 else 0), generator=g) * 2).to(DEV) for s in range(5)]
    tgts = [torch.round(torch.rand(3, 1, o.shape[2], o.shape[3], generator=g) * (ncls - 1)).to(DEV) for o in outs]
    a = [o.clone().requires_grad_(True) for o in outs]
    b = [o.clone().requires_grad_(True) for o in outs]
    fused = TR.deep_supervision_loss(a, tgts, batch_dice=batch_dice)
    eager = TR.deep_supervision_loss_eager(b, tgts, batch_dice=batch_dice)
    assert abs(float(fused) - float(eager)) < 2e-6 * max(1.0, abs(float(eager)))
    fused.backward()
    eager.backward()
    for x, y in zip(a, b):
        assert float((x.grad - y.grad).abs().max()) < 1e-7 + 1e-5 * float(y.grad.abs().max())


@gpu
def test_fused_loss_extreme_logits_stay_finite():
    from mlagg_unet_amd import trainer as TR
    z = torch.zeros(1, 3, 8, 8, device=DEV)
    z[:, 0] = 200.0                                    # label's logit 200 below the max: exp underflows, CE must not
    t = torch.ones(1, 1, 8, 8, device=DEV)
    zz = z.clone().requires_grad_(True)
    loss = TR.deep_supervision_loss([zz], [t])
    want = TR.deep_supervision_loss_eager([z], [t])
    assert torch.isfinite(loss) and abs(float(loss) - float(want)) < 1e-3
    loss.backward()
    assert torch.isfinite(zz.grad).all()


@gpu
@pytest.mark.parametrize("B,R,C", [(2, 64, 64), (3, 130, 48), (1, 7, 5), (2, 33, 96), (1, 4096, 192)])
def test_transpose_2d_bit_exact(B, R, C):
    from mlagg_unet_amd import ops
    x = torch.randn(B, R, C, generator=torch.Generator().manual_seed(R)).to(DEV)
    assert torch.equal(ops.transpose_2d(x), x.transpose(1, 2).contiguous())
    if R % 4 == 0:                                   # a channel slice of a wider NCHW map: larger batch stride, no copy
        wide = torch.randn(B, 2 * R, C, generator=torch.Generator().manual_seed(C)).to(DEV)
        sl = wide[:, :R]
        assert torch.equal(ops.transpose_2d(sl), sl.transpose(1, 2).contiguous())


@gpu
@pytest.mark.parametrize("shape", [(3, 7, 12, 20), (2, 5, 9, 7), (1, 96, 64, 64)])
def test_channel_bias_and_column_sum(shape):
    """Conv2d / ConvTranspose2d of the product model add their bias through K8 (gradient = plane sums)."""
    from mlagg_unet_amd import model as PM, ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    conv = PM.Conv2d(C, C + 1, 3, padding=1).to(DEV)
    ref = torch.nn.Conv2d(C, C + 1, 3, padding=1).to(DEV)
    ref.load_state_dict(conv.state_dict())
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = conv(xa), ref(xb)
    assert float((ya - yb).abs().max()) < 1e-5
    gy = torch.randn(ya.shape, generator=g).to(DEV)
    ya.backward(gy)
    yb.backward(gy)
    assert float((conv.bias.grad - ref.bias.grad).abs().max()) < 1e-4 * max(1.0, float(ref.bias.grad.abs().max()))
    assert float((conv.weight.grad - ref.weight.grad).abs().max()) < 1e-3 and float((xa.grad - xb.grad).abs().max()) < 1e-4
    ct, rt = PM.ConvTranspose2d(C, 4, 3, stride=2, padding=1).to(DEV), torch.nn.ConvTranspose2d(C, 4, 3, stride=2, padding=1).to(DEV)
    rt.load_state_dict(ct.state_dict())
    za, zb = ct(x), rt(x)
    assert float((za - zb).abs().max()) < 1e-5
    za.sum().backward()
    zb.sum().backward()
    assert float((ct.bias.grad - rt.bias.grad).abs().max()) < 1e-3 * float(rt.bias.grad.abs().max())
    m = torch.randn(257, C, generator=g).to(DEV)
    assert float((ops.column_sum(m) - m.sum(0)).abs().max()) < 1e-4
    wide = torch.randn(100, 3 * C, generator=g).to(DEV)
    assert float((ops.column_sum(wide[:, C:2 * C]) - wide[:, C:2 * C].sum(0)).abs().max()) < 1e-4
    tall = torch.randn(7840 + C, 3 * C, generator=g).to(DEV)         # row slabs + a second launch (ragged last slab)
    got, want = ops.column_sum(tall[:, C:2 * C]), tall[:, C:2 * C].double().sum(0)
    assert float((got.double() - want).abs().max()) < 2e-3 and torch.equal(got, ops.column_sum(tall[:, C:2 * C]))


@gpu
@pytest.mark.parametrize("B,C,H,W", [(3, 6, 16, 12), (2, 5, 7, 9), (1, 48, 64, 64)])
@pytest.mark.parametrize("kind", ["group", "instance_leaky", "instance_affine_silu"])
def test_plane_norm_matches_torch(B, C, H, W, kind):
    """K10 against nn.GroupNorm(C, C) / nn.InstanceNorm2d (+ LeakyReLU 0.01 / SiLU), forward and all gradients."""
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(H)
    x = (torch.randn(B, C, H, W, generator=g) * 2 + 0.5).to(DEV)
    gamma = (torch.randn(C, generator=g) * 0.5 + 1).to(DEV)
    beta = torch.randn(C, generator=g).to(DEV)
    gy = torch.randn(B, C, H, W, generator=g).to(DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    if kind == "group":
        ga, ba = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        gb, bb = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        ya = ops.plane_norm(xa, ga, ba, 1e-5)
        yb = F.group_norm(xb, C, gb, bb, 1e-5)
    elif kind == "instance_leaky":
        ga = ba = gb = bb = None
        ya = ops.plane_norm(xa, None, None, 1e-5, ops.ACT_LEAKY, 0.01)
        yb = F.leaky_relu(F.instance_norm(xb, eps=1e-5), 0.01)
    else:
        ga, ba = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        gb, bb = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        ya = ops.plane_norm(xa, ga, ba, 1e-5, ops.ACT_SILU)
        yb = F.silu(F.instance_norm(xb, weight=gb, bias=bb, eps=1e-5))
    assert float((ya - yb).abs().max()) < 2e-5
    ya.backward(gy)
    yb.backward(gy)
    assert float((xa.grad - xb.grad).abs().max()) < 5e-5 * max(1.0, float(xb.grad.abs().max()))
    if ga is not None:
        assert float((ga.grad - gb.grad).abs().max()) < 1e-4 * max(1.0, float(gb.grad.abs().max()))
        assert float((ba.grad - bb.grad).abs().max()) < 1e-4 * max(1.0, float(bb.grad.abs().max()))


@gpu
def test_plane_norm_residual_before_activation():
    """y = leaky(IN(x) + res): the tail of the MONAI UnetResBlock, forward and both gradients."""
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 6, 20, 12, generator=g).to(DEV)
    r = torch.randn(2, 6, 20, 12, generator=g).to(DEV)
    gy = torch.randn(2, 6, 20, 12, generator=g).to(DEV)
    xa, ra = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    xb, rb = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    ya = ops.plane_norm(xa, None, None, 1e-5, ops.ACT_LEAKY, 0.01, ra)
    yb = F.leaky_relu(F.instance_norm(xb, eps=1e-5) + rb, 0.01)
    assert float((ya - yb).abs().max()) < 2e-5
    ya.backward(gy)
    yb.backward(gy)
    assert float((xa.grad - xb.grad).abs().max()) < 5e-5 and float((ra.grad - rb.grad).abs().max()) < 1e-6


@gpu
@pytest.mark.parametrize("res", [False, True])
def test_plane_norm_segmented_planes_match_torch(res):
    """Planes of 256 Ki elements and more (InstanceNorm3d(affine) + LeakyReLU of the 3-D network, UMambaEnc_SS3D.py:477-513) are cut
    into 16 Ki-element segments with pooled statistics: against F.instance_norm in float64, a ragged last segment, an offset far
    larger than the spread (the case a sum-of-squares variance would lose), with and without the residual."""
    from mlagg_unet_amd import _lib, ops
    B, C, dims = 2, 3, (10, 164, 164)                     # 268 960 voxels: 17 segments, the last one 6 816 elements
    assert _lib.lib().mlagg_plane_norm_fwd_workspace_floats(B, C, dims[0] * dims[1] * dims[2]) == B * C * 17 * 3
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, *dims, generator=g) * 0.5 + 40.0
    r = torch.randn(B, C, *dims, generator=g)
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g)
    gy = torch.randn(B, C, *dims, generator=g)
    xb, rb = x.double().requires_grad_(True), r.double().requires_grad_(True)
    gb, bb = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yb = F.instance_norm(xb, weight=gb, bias=bb, eps=1e-5)
    yb = F.silu(yb + rb if res else yb)          # a smooth activation: behind LeakyReLU a handful of the 1.6 M elements sit within
    yb.backward(gy.double())                     # rounding distance of 0 and flip slope between any two fp32 evaluations
    xa, ra = x.to(DEV).requires_grad_(True), r.to(DEV).requires_grad_(True)
    ga, ba = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    ya = ops.plane_norm(xa, ga, ba, 1e-5, ops.ACT_SILU, 0.0, ra if res else None)
    ya.backward(gy.to(DEV))
    assert float((ya.detach().cpu().double() - yb.detach()).abs().max()) < 1e-3          # x / std ~ 80: 1e-5 relative of the input
    for name, a, b in (("dx", xa.grad, xb.grad), ("dgamma", ga.grad, gb.grad), ("dbeta", ba.grad, bb.grad)) + \
            ((("dres", ra.grad, rb.grad),) if res else ()):
        assert float((a.cpu().double() - b).abs().max()) <= 5e-4 * float(b.abs().max()), name


@gpu
@pytest.mark.parametrize("max_norm", [12.0, 0.05, 0.0])
def test_clip_adamw_matches_torch(max_norm):
    """K11 against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW over several steps (clip active, inactive, off)."""
    from mlagg_unet_amd import trainer as TR
    g = torch.Generator().manual_seed(9)
    shapes = [(7,), (33, 5), (1,), (300, 257), (96, 1, 3, 3), (70001,)]
    pa = [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    unused = torch.nn.Parameter(torch.ones(1, device=DEV))                      # like dummy_tensor: never gets a gradient
    oa = TR.ClipAdamW(pa + [unused], 5e-4, eps=1e-4, weight_decay=3e-5)
    ob = torch.optim.AdamW(pb, 5e-4, eps=1e-4, weight_decay=3e-5)
    for it in range(4):
        grads = [torch.randn(s, generator=g).to(DEV) * (0.1 + it) for s in shapes]
        for p, q, gr in zip(pa, pb, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        oa.step(max_norm=max_norm)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(pb, max_norm)
        ob.step()
        for p, gr in zip(pa, grads):
            assert torch.equal(p.grad, gr)                                       # gradients stay unscaled in memory
        if max_norm > 0:
            want = torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads))
            assert abs(float(oa.grad_norm()) - float(want)) < 1e-5 * float(want)
    for p, q in zip(pa, pb):
        assert float((p - q).abs().max()) < 2e-6, float((p - q).abs().max())
    sa, sb = oa.state_dict(), ob.state_dict()
    assert float(sa["state"][3]["step"]) == 4.0 == float(sb["state"][3]["step"])
    v_ref = sb["state"][3]["exp_avg_sq"]
    assert float((sa["state"][3]["exp_avg_sq"] - v_ref).abs().max()) < 1e-4 * float(v_ref.abs().max())   # (g * coef)^2 rounding
    assert float(unused) == 1.0 and 6 not in sa["state"]


@gpu
@pytest.mark.parametrize("max_norm", [12.0, 0.0])
def test_capturable_clip_adamw_is_bit_identical_to_the_eager_form_and_replays(max_norm):
    """The hipGraph form of K11 (step counter and a copy of the learning rate device-resident, mlagg_optimizer_clip_step_dev with MLAGG_OPT_ADAMW): bit-identical parameters to
    the launch-argument form over eager steps, a captured step replays with a NEW learning rate and advancing bias corrections, and the
    state_dict carries the device counter."""
    from mlagg_unet_amd import trainer as TR
    g = torch.Generator().manual_seed(21)
    shapes = [(7,), (33, 5), (300, 257), (70001,)]
    pa = [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa = TR.ClipAdamW(pa, 5e-4, eps=1e-4, weight_decay=3e-5, capturable=True)
    ob = TR.ClipAdamW(pb, 5e-4, eps=1e-4, weight_decay=3e-5)
    assert type(oa.param_groups[0]["lr"]) is float                               # the device copy lives outside param_groups
    static = [torch.zeros(s, device=DEV) for s in shapes]                        # gradients at fixed addresses, as inside a graph
    for p, st in zip(pa, static):
        p.grad = st
    grads = [[torch.randn(s, generator=g).to(DEV) * (0.5 + it) for s in shapes] for it in range(6)]
    lrs = [5e-4, 5e-4, 3e-4, 3e-4, 1e-4, 7e-5]

    def feed(it):
        for st, q, gr in zip(static, pb, grads[it]):
            st.copy_(gr)
            q.grad = gr.clone()
        oa.param_groups[0]["lr"] = lrs[it]
        oa.sync_lr()                                                             # a raw graph.replay() runs no host code of ours
        ob.param_groups[0]["lr"] = lrs[it]

    for it in range(2):                                                          # eager calls of the capturable form
        feed(it)
        oa.step(max_norm=max_norm)
        ob.step(max_norm=max_norm)
    for p, q in zip(pa, pb):
        assert torch.equal(p, q)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    feed(2)
    with torch.cuda.graph(graph):
        oa.step(max_norm=max_norm)
    ob_steps = 2
    # the capture itself executes nothing: parameters unchanged until the first replay
    for it in range(2, 6):
        feed(it)
        graph.replay()
        ob.step(max_norm=max_norm)
        ob_steps += 1
        for p, q in zip(pa, pb):
            assert torch.equal(p, q), it
    assert oa.steps_done() == ob_steps == 6
    assert float(oa.state_dict()["state"][0]["step"]) == 6.0


@gpu
def test_clip_adamw_checkpoint_round_trip_and_failure_modes():
    """state_dict after 2 steps loads into a fresh ClipAdamW AND into torch.optim.AdamW (the reference's checkpoint format,
    nnUNetTrainer.save_checkpoint B:1023-1043); one more step in each lands on the same parameters.  A non-finite gradient
    poisons every parameter as clip_grad_norm_'s NaN coefficient does; two parameter groups and a changing set of
    parameters with gradients are refused."""
    from mlagg_unet_amd import trainer as TR
    g = torch.Generator().manual_seed(11)
    shapes = [(5,), (64, 9), (300, 129)]

    def params():
        gg = torch.Generator().manual_seed(3)
        return [torch.nn.Parameter(torch.randn(s, generator=gg).to(DEV)) for s in shapes]
    pa = params()
    oa = TR.ClipAdamW(pa, 5e-4, eps=1e-4, weight_decay=3e-5)
    grads = [[torch.randn(s, generator=g).to(DEV) for s in shapes] for _ in range(3)]
    for it in range(2):
        for p, gr in zip(pa, grads[it]):
            p.grad = gr.clone()
        oa.step(max_norm=12.0)
    sd = oa.state_dict()
    pb, pc = [torch.nn.Parameter(p.detach().clone()) for p in pa], [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ob = TR.ClipAdamW(pb, 5e-4, eps=1e-4, weight_decay=3e-5)
    oc = torch.optim.AdamW(pc, 5e-4, eps=1e-4, weight_decay=3e-5)
    import copy
    ob.load_state_dict(copy.deepcopy(sd))        # as after torch.save / torch.load: load_state_dict itself keeps same-device
    oc.load_state_dict(copy.deepcopy(sd))        # tensors by reference, which would alias the three optimizers' moments
    for ps, opt in ((pa, oa), (pb, ob), (pc, oc)):
        for p, gr in zip(ps, grads[2]):
            p.grad = gr.clone()
        if opt is oc:
            torch.nn.utils.clip_grad_norm_(pc, 12.0)
            opt.step()
        else:
            opt.step(max_norm=12.0)
    for x, y, z in zip(pa, pb, pc):
        assert torch.equal(x, y)                                                  # resumed == uninterrupted, bit for bit
        assert float((x - z).abs().max()) < 2e-6
    assert float(ob.state_dict()["state"][0]["step"]) == 3.0 == float(oc.state_dict()["state"][0]["step"])
    # closure: evaluated, its value returned
    for p, gr in zip(pa, grads[0]):
        p.grad = gr.clone()
    assert oa.step(lambda: 7.5, max_norm=12.0) == 7.5
    # non-finite gradient norm: every parameter becomes NaN (torch: the clip coefficient is NaN)
    pa[1].grad[0, 0] = float("nan")
    oa.step(max_norm=12.0)
    assert all(bool(torch.isnan(p).all()) for p in pa)
    # refused configurations
    with pytest.raises(RuntimeError):
        TR.ClipAdamW([{"params": pb[:1]}, {"params": pb[1:]}])
    pb[0].grad = None
    with pytest.raises(RuntimeError):
        ob.step(max_norm=12.0)


@gpu
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("B,C,H,W,with_res,with_bias", [(2, 96, 32, 32, True, True), (3, 7, 5, 9, False, True), (1, 192, 16, 16, True, False)])
def test_channel_epilogue_matches_torch(act, B, C, H, W, with_res, with_bias):
    """K13: act(conv_out + bias + res) and its backward (d(pre), d(res), d(bias)) against torch in double precision."""
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(B * C + act)
    x = torch.randn(B, C, H, W, generator=g)
    b = torch.randn(C, generator=g) if with_bias else None
    r = torch.randn(B, C, H, W, generator=g) if with_res else None
    gy = torch.randn(B, C, H, W, generator=g)
    xr = x.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if with_bias else None
    rr = r.double().requires_grad_(True) if with_res else None
    pre = xr + (br.view(1, -1, 1, 1) if with_bias else 0) + (rr if with_res else 0)
    yr = torch.nn.functional.gelu(pre) if act else pre
    yr.backward(gy.double())
    xg = x.to(DEV).requires_grad_(True)
    bg = b.to(DEV).requires_grad_(True) if with_bias else None
    rg = r.to(DEV).requires_grad_(True) if with_res else None
    y = ops.channel_epilogue(xg * 1.0, bg, rg, act)          # * 1.0: a fresh map, as a convolution output is
    y.backward(gy.to(DEV))
    _close(y, yr.float(), 1e-5, 1e-5, "epilogue y")
    _close(xg.grad, xr.grad.float(), 1e-5, 1e-5, "epilogue dx")
    if with_res:
        _close(rg.grad, rr.grad.float(), 1e-5, 1e-5, "epilogue dres")
    if with_bias:
        _close(bg.grad, br.grad.float(), 2e-4, 1e-4, "epilogue dbias")


@gpu
def test_full_size_round_trips_of_the_data_movement_and_attention_ops():
    """Headline shapes (batch 10, 256 x 256 -> four MSMM scales, L_cat = 21760) through properties that need no oracle:
    cross_merge(cross_scan(x)) = 4 x bit for bit (each direction is a permutation, the merge a sum of four equal values);
    direction 0 of scale 0 is the plain row-major map; the pooled attention does not depend on the order of the pooled
    keys (softmax-sum invariance); the token-major projection is linear."""
    from mlagg_unet_amd import ops
    HW = [(128, 128), (64, 64), (32, 32), (16, 16)]
    Lc = sum(h * w for h, w in HW)
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(10, Lc, 96, device=DEV, generator=g)
    seq = ops.cross_scan(x, HW, 96, 1)
    assert seq.shape == (10, 4 * 96, Lc)
    assert torch.equal(seq[:, :96, :128 * 128].transpose(1, 2), x[:, :128 * 128])                  # k = 0, scale 0: identity order
    assert torch.equal(seq[:, 2 * 96:3 * 96, :128 * 128].flip(-1), seq[:, :96, :128 * 128])        # k = 2 = reversed k = 0
    back = ops.cross_merge(seq, HW, 96)
    assert torch.equal(back, 4.0 * x)
    # K4: key order invariance at stage-0 size (N = 16384 tokens, P = 64 pooled keys, one head pair, d = 48)
    N, P, nh, d = 128 * 128, 64, 1, 48
    q = torch.randn(10, N, d, device=DEV, generator=g)
    k = torch.randn(10, P, d, device=DEV, generator=g)
    v = torch.randn(10, P, d, device=DEV, generator=g)
    lam = torch.tensor([0.3], device=DEV)
    w = torch.ones(48, device=DEV)
    o1 = ops.pooled_diff_attn(q, k, v, lam, w, nh, 24 ** -0.5)
    perm = torch.randperm(P, device=DEV, generator=g)
    o2 = ops.pooled_diff_attn(q, k[:, perm].contiguous(), v[:, perm].contiguous(), lam, w, nh, 24 ** -0.5)
    assert float((o1 - o2).abs().max()) < 1e-5 * max(1.0, float(o1.abs().max()))
    # K5: linearity of the 163840-token projection
    W_ = torch.randn(192, 96, device=DEV, generator=g) * 0.1
    b_ = torch.randn(192, device=DEV, generator=g)
    xa, xb = x[:, :16384].contiguous(), torch.randn(10, 16384, 96, device=DEV, generator=g)
    ya, yb = ops.linear(xa, W_, b_), ops.linear(xb, W_, b_)
    yab = ops.linear(2.0 * xa - xb, W_, b_)
    assert float((yab - (2.0 * ya - yb)).abs().max()) < 1e-4 * float(ya.abs().max())      # W(2a - b) + c = 2(Wa + c) - (Wb + c)


@gpu
@pytest.mark.parametrize("batch_dice", [True, False])
def test_fused_loss_with_ignore_label_matches_reference_golden(batch_dice):
    """K9 with the ignore label of partially annotated datasets: pixels carrying it are left out of the dice sums and of the
    cross-entropy mean and get no gradient (reference DC_and_CE_loss(ignore_label=5), tests/golden/loss_ignore.npz)."""
    import os
    import numpy as np
    from mlagg_unet_amd import trainer as TR
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "loss_ignore.npz"))
    g = torch.Generator().manual_seed(23)
    outs = [torch.randn(3, 5, 32 >> s, 32 >> s, generator=g) for s in range(5)]
    tg = []
    for s in range(5):
        t_ = torch.round(torch.rand(3, 1, 32 >> s, 32 >> s, generator=g) * 4)
        t_[torch.rand(t_.shape, generator=g) < 0.3] = 5.0
        tg.append(t_)
    tg[3][0] = 5.0
    tg[4][:] = 5.0
    zs = [o.to(DEV).requires_grad_(True) for o in outs]
    loss = TR.deep_supervision_loss(zs, [t_.to(DEV) for t_ in tg], batch_dice=batch_dice, ignore_label=5)
    assert abs(float(loss.detach()) - float(G[f"loss_batch_dice_{int(batch_dice)}"])) < 2e-6
    loss.backward()
    for s, z in enumerate(zs):
        want = torch.from_numpy(G[f"grad{s}_batch_dice_{int(batch_dice)}"])
        assert float((z.grad.cpu() - want).abs().max()) < 1e-7
    assert float(zs[4].grad.abs().max()) == 0.0                    # the fully ignored level: no gradient at all
    assert float(zs[0].grad.cpu()[(tg[0] == 5).expand(-1, 5, -1, -1)].abs().max()) == 0.0


@gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hw", [(24, 20), (7, 9), (260, 260)])          # vector path, scalar path (odd plane), register-resident limit passed
def test_plane_norm_16_bit_maps(dt, hw):
    """K10 with 16-bit maps in memory (16-bit modes: convolution output in, next convolution's input out, residual in either type):
    against float64 arithmetic on the SAME 16-bit inputs, outputs within one rounding of the output type; gradients come back in
    the inputs' own types."""
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(hw[0])
    B, C = 2, 5
    x = (torch.randn(B, C, *hw, generator=g) * 2 + 0.5).to(dt)
    r = torch.randn(B, C, *hw, generator=g)                              # fp32 residual
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    gy = torch.randn(B, C, *hw, generator=g).to(dt)
    xb, rb = x.double().requires_grad_(True), r.double().requires_grad_(True)
    gb, bb = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yb = F.silu(F.instance_norm(xb, weight=gb, bias=bb, eps=1e-5) + rb)
    yb.backward(gy.double())
    xa, ra = x.to(DEV).requires_grad_(True), r.to(DEV).requires_grad_(True)
    ga, ba = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    ya = ops.plane_norm(xa, ga, ba, 1e-5, ops.ACT_SILU, 0.0, ra, out_dtype=dt)
    assert ya.dtype == dt
    ya.backward(gy.to(DEV))
    eps16 = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    assert float((ya.detach().cpu().double() - yb.detach()).abs().max()) <= eps16 * float(yb.abs().max()) * 1.01 + 1e-6
    assert xa.grad.dtype == dt and ra.grad.dtype == torch.float32
    assert float((xa.grad.cpu().double() - xb.grad).abs().max()) <= 2 * eps16 * float(xb.grad.abs().max()) + 1e-6
    assert float((ra.grad.cpu().double() - rb.grad).abs().max()) <= 1e-5 * float(rb.grad.abs().max()) + 1e-6
    assert float((ga.grad.cpu().double() - gb.grad).abs().max()) <= 1e-4 * float(gb.grad.abs().max()) + 1e-5
    assert float((ba.grad.cpu().double() - bb.grad).abs().max()) <= 1e-4 * float(bb.grad.abs().max()) + 1e-5


@gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("act", ["none", "gelu"])
def test_channel_epilogue_16_bit_maps(dt, act):
    """K13 in the 16-bit modes: y = act(x16 + bias + res) with x16 untouched, y in the requested type; backward dx in x's type,
    d(bias), d(res) in res's type."""
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(3)
    B, C, H, W = 2, 6, 12, 20
    x = torch.randn(B, C, H, W, generator=g).to(dt)
    bias = torch.randn(C, generator=g)
    r = torch.randn(B, C, H, W, generator=g) if act == "none" else None
    out_dt = torch.float32 if act == "none" else dt
    gy = torch.randn(B, C, H, W, generator=g).to(out_dt)
    xb, bb = x.double().requires_grad_(True), bias.double().requires_grad_(True)
    rb = None if r is None else r.double().requires_grad_(True)
    pre = xb + bb.view(1, -1, 1, 1) + (0 if rb is None else rb)
    yb = F.gelu(pre) if act == "gelu" else pre
    yb.backward(gy.double())
    xa, ba = x.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    ra = None if r is None else r.to(DEV).requires_grad_(True)
    x_before = xa.detach().clone()
    ya = ops.channel_epilogue_lp(xa, ba, ra, ops.EPI_GELU if act == "gelu" else ops.EPI_NONE, out_dt)
    ya.backward(gy.to(DEV))
    eps16 = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    out_eps = eps16 if out_dt == dt else 1e-6
    assert ya.dtype == out_dt and torch.equal(xa.detach(), x_before)
    assert float((ya.detach().cpu().double() - yb.detach()).abs().max()) <= out_eps * float(yb.abs().max()) * 1.01 + 1e-6
    assert xa.grad.dtype == dt
    assert float((xa.grad.cpu().double() - xb.grad).abs().max()) <= 2 * eps16 * float(xb.grad.abs().max()) + 1e-6
    # the bias sum runs over the fp32 values BEFORE they are rounded to x's type
    assert float((ba.grad.cpu().double() - bb.grad).abs().max()) <= 1e-4 * float(bb.grad.abs().max()) + 1e-4
    if ra is not None:
        assert ra.grad.dtype == torch.float32 and float((ra.grad.cpu().double() - rb.grad).abs().max()) < 1e-6


@gpu
def test_split_cols_gradient_buffer_equals_concatenated_gradients():
    """ops.split_cols: kernels that claim a piece write its gradient into the shared buffer; a piece used twice, a piece that feeds a
    plain torch op and a piece nobody uses all end with the gradient torch's own split + cat produce."""
    from mlagg_unet_amd import ops
    torch.manual_seed(5)
    B, H, W, C = 2, 16, 16, 96
    h = C // 2
    base = torch.randn(B, H * W, 2 * C + 48, device=DEV)
    w_dw = torch.randn(h, 1, 3, 3, device=DEV) * 0.3
    b_dw = torch.randn(h, device=DEV) * 0.1
    a0, a1 = torch.randn(B, H * W, h, device=DEV), torch.randn(B, H * W, h, device=DEV)

    def run(splitter):
        t = base.clone().requires_grad_(True)
        t2 = t * 1.0                                    # a non-leaf, like a projection output
        act, xa, za, _unused = splitter(t2, (C, h, h, 48))
        g = ops.gate(a0, a1, act)                       # claims `act`
        d1 = ops.dwconv3x3_nlc(xa, w_dw, b_dw, H, W, silu=True)         # claims `xa`
        d2 = ops.dwconv3x3_nlc(xa, w_dw, b_dw, H, W, silu=False)        # second consumer of the same piece
        e = F.gelu(za)                                  # torch op: gradient copied into the buffer
        loss = (g * g).sum() + (d1 * 0.5).sum() + (d2 * d2).sum() + (e * 1.5).sum()
        loss.backward()
        return t.grad

    g_arena = run(ops.split_cols)
    g_plain = run(lambda t, sizes: t.split(list(sizes), dim=-1))
    assert torch.equal(g_arena, g_plain)
    assert float(g_arena[..., 2 * C:].abs().max()) == 0.0


@gpu
@pytest.mark.parametrize("C,N,with_scale,use_sum", [(96, 60, True, True), (192, 33, False, True), (768, 7, True, False), (48, 128, False, False)])
def test_residual_layer_norm_matches_torch(C, N, with_scale, use_sum):
    """ops.residual_layer_norm = (skip + branch * scale[sample], LayerNorm of it); every gradient against float64 torch, with and
    without a second consumer of the sum."""
    from mlagg_unet_amd import ops
    g = torch.Generator().manual_seed(C + N)
    B = 3
    skip, branch = torch.randn(B, N, C, generator=g), torch.randn(B, N, C, generator=g)
    scale = torch.tensor([0.0, 1.25, 1.25]) if with_scale else None
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    gy, gx = torch.randn(B, N, C, generator=g), torch.randn(B, N, C, generator=g)
    rs, rb, rw, rbias = [t.double().requires_grad_(True) for t in (skip, branch, w, b)]
    xs = rs + (rb * scale.double().view(-1, 1, 1) if with_scale else rb)
    yr = F.layer_norm(xs, (C,), rw, rbias, 1e-5)
    ((yr * gy.double()).sum() + ((xs * gx.double()).sum() if use_sum else 0.0)).backward()
    ps, pb, pw, pbias = [t.to(DEV).requires_grad_(True) for t in (skip, branch, w, b)]
    xp, yp = ops.residual_layer_norm(ps, pb, None if scale is None else scale.to(DEV), pw, pbias, 1e-5)
    ((yp * gy.to(DEV)).sum() + ((xp * gx.to(DEV)).sum() if use_sum else 0.0)).backward()
    _close(xp, xs.float(), 1e-6, 1e-6, "xsum")
    _close(yp, yr.float(), 2e-6, 1e-5, "y")
    for name, got, want in (("dskip", ps.grad, rs.grad), ("dbranch", pb.grad, rb.grad), ("dgamma", pw.grad, rw.grad),
                            ("dbeta", pbias.grad, rbias.grad)):
        _close(got, want.float(), 5e-6, 1e-4, name)


@gpu
@pytest.mark.parametrize("M,N,K", [(16384, 192, 96), (20000, 140, 96), (16500, 96, 140), (16384, 48, 1536), (130, 100, 52)])
def test_linear_bf16x3_is_as_accurate_as_the_fp32_instruction(M, N, K):
    """K5 on the 16-bit matrix instructions (MLAGG_DTYPE_BF16X3: fp32 operands as three bf16 pieces, six partial products): forward
    and, on the transposed weight, the data gradient -- against float64, with the error bound of the fp32-MFMA kernel (and within
    1.5x of the error that kernel makes on the same inputs).  Ragged M, N and a K that is not a multiple of the 16-deep instruction."""
    from mlagg_unet_amd import _lib
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(M + N + K)
    x = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))).to(DEV)        # rows of very different scale
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    y3, y1 = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    _lib.check(lib.mlagg_linear_lp_fwd(x.data_ptr(), K, w.data_ptr(), b.data_ptr(), y3.data_ptr(), N, M, N, K, 3, st), "x3")
    _lib.check(lib.mlagg_linear_fwd(x.data_ptr(), K, w.data_ptr(), b.data_ptr(), y1.data_ptr(), N, M, N, K, st), "fp32")
    ref = torch.addmm(b.double(), x.double(), w.double().t())
    scale = ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)             # per row: the rows differ by orders of magnitude
    e3, e1 = float(((y3.double() - ref).abs() / scale).max()), float(((y1.double() - ref).abs() / scale).max())
    assert e3 < 3e-6 and e3 < 1.5 * e1 + 1e-7, (e3, e1)
    from mlagg_unet_amd import ops
    assert ops.K5_X3
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    gy = torch.randn(M, N, generator=g).to(DEV)
    ops.LinearFn.apply(xg, wg, b).backward(gy)                # M >= 16384: x3 forward and x3 data gradient on W^T; else the library
    dref = gy.double() @ w.double()
    assert float((xg.grad.double() - dref).abs().max() / dref.abs().max()) < 3e-6


@gpu
@pytest.mark.parametrize("M,O,I", [(16384, 192, 96), (9000, 140, 96), (8195, 48, 144), (8192, 100, 52), (40000, 96, 140), (8200, 36, 256)])
def test_linear_wgrad_bf16x3_matches_float64(M, O, I):
    """K5w on the 16-bit matrix instructions (mlagg_linear_wgrad_x3): dW and db against float64 with the fp32 kernel's bound, on
    widths that are not multiples of the 96-column groups (clamped lanes), ragged token counts and strided operands."""
    from mlagg_unet_amd import _lib
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(M + O + I)
    dyw = torch.randn(M, O + 8, generator=g).to(DEV)
    xw = (torch.randn(M, I + 4, generator=g) * torch.exp(0.5 * torch.randn(M, 1, generator=g))).to(DEV)
    dy, x = dyw[:, 4:4 + O], xw[:, :I]
    ws = torch.empty(lib.mlagg_linear_wgrad_workspace_floats(M, O, I), device=DEV)
    out = {}
    for name, fn in (("x3", lib.mlagg_linear_wgrad_x3), ("fp32", lib.mlagg_linear_wgrad)):
        dW, db = torch.full((O, I), float("nan"), device=DEV), torch.full((O,), float("nan"), device=DEV)
        _lib.check(fn(dy.data_ptr(), dyw.stride(0), x.data_ptr(), xw.stride(0), dW.data_ptr(), db.data_ptr(), ws.data_ptr(), M, O, I, st),
                   name)
        out[name] = (dW, db)
    ref = dy.double().t() @ x.double()
    e3 = float((out["x3"][0].double() - ref).abs().max() / ref.abs().max())
    e1 = float((out["fp32"][0].double() - ref).abs().max() / ref.abs().max())
    assert e3 < 2e-6 and e3 < 1.5 * e1 + 1e-7, (e3, e1)
    bref = dy.double().sum(0)
    assert float((out["x3"][1].double() - bref).abs().max()) < 1e-3 * max(1.0, float(bref.abs().max()))


@gpu
@pytest.mark.parametrize("M,O,I", [(16384, 192, 96), (9000, 140, 96), (8200, 52, 100)])
def test_linear_lp_dgrad_abi_in_split_bf16_mode(M, O, I):
    """`mlagg_linear_lp_dgrad(..., MLAGG_DTYPE_BF16X3)`: the data gradient on the UNtransposed weight (the entry point a binding may
    call directly; the model itself runs the forward kernel on W^T) against float64, ragged M / O / I."""
    from mlagg_unet_amd import _lib
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(M + O)
    dy = torch.randn(M, O, generator=g).to(DEV)
    w = (torch.randn(O, I, generator=g) * O ** -0.5).to(DEV)
    dx = torch.full((M, I), float("nan"), device=DEV)
    _lib.check(lib.mlagg_linear_lp_dgrad(dy.data_ptr(), O, w.data_ptr(), dx.data_ptr(), I, M, O, I, 3, st), "dgrad x3")
    ref = dy.double() @ w.double()
    assert float((dx.double() - ref).abs().max() / ref.abs().max()) < 3e-6
