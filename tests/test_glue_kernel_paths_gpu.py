"""GPU: the glue kernels K1' 2-D / 3-D, K8, K13 and K17 against the float64 references of tests/_glue_kernel_cases.py at the sizes where
their code changes path (tests/test_glue_kernel_paths_cpu.py shows which case enters which path and that the cases are well
conditioned).  One test per op family; each runs the op through mlagg_unet_amd.ops forward and backward on the device and compares
every output and EVERY gradient; where an op writes into a slice of a wider buffer the rest of it must come back untouched."""
import pytest
import torch

from tests import _glue_kernel_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0


def _ids(cases):
    return [M.case_id(c) for c in cases]


def _dev(t):
    return t.to(DEV)


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


def _poison(*floats):
    """Fill and free blocks of `floats` floats of device memory with NaN: the next allocations of those sizes are likely to be handed
    them, so a column a backward kernel does not write shows up."""
    junk = [torch.full((max(int(n), 1),), float("nan"), device=DEV) for n in floats for _ in range(3)]
    del junk


def _check(case, got):
    ref, yards = M.reference_and_yardstick(case)
    tols = M.bounds(case, ref, yards)
    aux = M.aux(case, ref)
    assert set(got) == set(tols), set(got) ^ set(tols)
    failed = []
    for q, tol in tols.items():
        assert got[q].shape == ref[q].shape, (q, got[q].shape, ref[q].shape)
        err, excess = M.error(got[q].float(), ref[q], tol, aux.get(q))
        print(f"{M.family(case)} {M.case_id(case)} {q}: error {err:.2e} ({tol.kind} {tol.a:.2e}, {tol.r:.0e})")
        if not excess <= 0.0:                                                     # (a NaN fails too)
            failed.append((q, err, tol))
    assert not failed, failed


@pytest.mark.parametrize("case", M.XSCAN_CASES, ids=_ids(M.XSCAN_CASES))
def test_cross_scan_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    HW = list(case.HW)
    if case.op == "scan":
        tok = _leaf(t["tok"])
        seq = ops.cross_scan(tok, HW, case.CB, 1)
        seq.backward(_dev(t["d_seq"]))
        _check(case, dict(seq=seq, dtok=tok.grad))
    elif case.op == "merge":
        seq = _leaf(t["seq"])
        tok = ops.cross_merge(seq, HW, case.CB)
        tok.backward(_dev(t["d_tok"]))
        _check(case, dict(tok=tok, dseq=seq.grad))
    else:
        x = _leaf(t["xdbl"])
        dtr, Bs, Cs = ops.cross_scan_bc(x, HW, M.XS_R, M.XS_N)
        cot = [_dev(t["d_dtr"]), _dev(t["d_Bs"]), _dev(t["d_Cs"])]
        _poison(x.numel())                                                        # the backward must write all 140 columns itself
        torch.autograd.backward([dtr, Bs, Cs], cot)
        _check(case, dict(dtr=dtr, Bs=Bs, Cs=Cs, dxdbl=x.grad))


@pytest.mark.parametrize("case", M.ISCAN_CASES, ids=_ids(M.ISCAN_CASES))
def test_index_scan_paths_match_float64(case):
    from mlagg_unet_amd import ops, ss3d
    t = M.inputs(case)
    idx = M.iscan_orders(case).to(torch.int32).to(DEV)
    if case.dims is not None:
        assert torch.equal(idx, ss3d.scan_orders_3d(*case.dims, DEV))
    _, blk, col0 = M.iscan_layout(case)
    if case.op in ("scan", "scanblk"):
        tok = _leaf(t["tok"])
        seq = ops.index_scan(tok, idx, case.CB, blk, col0)
        seq.backward(_dev(t["d_seq"]))
        _check(case, dict(seq=seq, dtok=tok.grad))
    elif case.op == "merge":
        seq = _leaf(t["seq"])
        tok = ops.index_merge(seq, idx, case.CB)                                  # the atomic form: compared by its bound only
        tok.backward(_dev(t["d_tok"]))
        _check(case, dict(tok=tok, dseq=seq.grad))
    else:
        x = _leaf(t["xdbl"])
        dtr, Bs, Cs = ops.index_scan_bc(x, idx, case.CB)
        cot = [_dev(t["d_dtr"]), _dev(t["d_Bs"]), _dev(t["d_Cs"])]
        _poison(x.numel())                                                        # the backward must write every column
        torch.autograd.backward([dtr, Bs, Cs], cot)
        _check(case, dict(dtr=dtr, Bs=Bs, Cs=Cs, dxdbl=x.grad))


@pytest.mark.parametrize("case", M.MOVE_CASES, ids=_ids(M.MOVE_CASES))
def test_transpose_paths_are_bit_exact(case):
    from mlagg_unet_amd import ops
    x = _dev(M.inputs(case)["x"])
    R, C = case.R, case.C
    if case.op == "plain":
        y = ops.transpose_2d(x)
    elif case.op == "half":                                                       # the first half of a (B, 2 R, C) tensor: a larger batch stride
        wide = torch.cat([x, torch.full_like(x, SENTINEL)], 1)
        src = wide[:, :R]
        assert src.stride(0) == 2 * R * C
        y = ops.transpose_2d(src)
    else:                                                                         # into the channels [4, 4 + C) of a wider map
        wide = torch.full((M.MOVE_B, C + M.MOVE_PAD, R), SENTINEL, device=DEV)
        y = ops.transpose_2d_into(x, wide[:, M.MOVE_C0:M.MOVE_C0 + C])
        assert y.data_ptr() == wide[:, M.MOVE_C0:].data_ptr()
        assert bool((wide[:, :M.MOVE_C0] == SENTINEL).all()) and bool((wide[:, M.MOVE_C0 + C:] == SENTINEL).all())
    _check(case, dict(y=y))


@pytest.mark.parametrize("case", M.SHUF_CASES, ids=_ids(M.SHUF_CASES))
def test_pixel_shuffle_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    B, O, H, W = M.SHUF_B, case.O, case.H, case.W
    if case.op != "convt":
        _check(case, dict(y=ops._pixel_shuffle2(_dev(t["x"]), B, O, H, W, case.op == "inv")))
        return
    x, w = _leaf(t["x"]), _leaf(t["w"])
    y = ops.conv_t2x2(x, w)
    wide = torch.full((B, 2 * O, 2 * H, 2 * W), SENTINEL, device=DEV)            # dy: a channel half of cat([up, skip])'s gradient
    wide[:, :O] = _dev(t["d_y"])
    assert ops._map_slice(wide[:, :O], "dy")[1] == wide.stride(0)                 # read where it is: the strided inverse shuffle
    y.backward(wide[:, :O])
    _check(case, dict(y=y, dx=x.grad, dw=w.grad))


@pytest.mark.parametrize("case", M.SUM_CASES, ids=_ids(M.SUM_CASES))
def test_channel_sum_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    x, b = _leaf(t["x"]), _leaf(t["bias"])
    y = ops.channel_bias(x * 1.0, b) if case.op == "bias" else ops.channel_epilogue(x * 1.0, b, None, ops.EPI_NONE)
    y.backward(_dev(t["d_y"]))
    _check(case, dict(y=y, dx=x.grad, dbias=b.grad))


@pytest.mark.parametrize("case", M.COL_CASES, ids=_ids(M.COL_CASES))
def test_column_sum_paths_match_float64(case):
    from mlagg_unet_amd import ops
    x = _dev(M.inputs(case)["x"])
    if case.wide:                                                                 # the middle column block of a row three times as wide
        full = torch.full((case.rows, 3 * case.cols), SENTINEL, device=DEV)
        full[:, case.cols:2 * case.cols] = x
        x = full[:, case.cols:2 * case.cols]
        assert x.stride(0) == 3 * case.cols
    _check(case, dict(sum=ops.column_sum(x)))


@pytest.mark.parametrize("case", M.RESID_CASES, ids=_ids(M.RESID_CASES))
def test_scaled_residual_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    skip, branch = _leaf(t["skip"]), _leaf(t["branch"])
    y = ops.scaled_residual(skip, branch, torch.tensor(case.scales, device=DEV))
    y.backward(_dev(t["d_y"]))
    zero = [i for i, s in enumerate(case.scales) if s == 0.0]
    _check(case, dict(y=y, y_zero=y[zero], dskip=skip.grad, dbranch=branch.grad))


@pytest.mark.parametrize("case", M.LAMBDA_CASES, ids=_ids(M.LAMBDA_CASES))
def test_diff_lambda_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    vs = [_leaf(t[k]) for k in ("q1", "k1", "q2", "k2")]
    lam = ops.diff_lambda(*vs, M.LAMBDA_INIT)
    lam.backward(torch.tensor(M.LAMBDA_DY, device=DEV))
    _check(case, dict(lam=lam, dq1=vs[0].grad, dk1=vs[1].grad, dq2=vs[2].grad, dk2=vs[3].grad))


@pytest.mark.parametrize("case", M.EPI_CASES, ids=_ids(M.EPI_CASES))
def test_channel_epilogue_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    x = _leaf(t["x"])
    b = _leaf(t["bias"]) if case.bias else None
    r = _leaf(t["res"]) if case.res else None
    y = ops.channel_epilogue(x * 1.0, b, r, ops.EPI_GELU if case.act == "gelu" else ops.EPI_NONE)     # * 1.0: a fresh map, as a convolution output is
    y.backward(_dev(t["d_y"]))
    got = dict(y=y, dx=x.grad)
    if case.bias:
        got["dbias"] = b.grad
    if case.res:
        got["dres"] = r.grad
    _check(case, got)


@pytest.mark.parametrize("case", M.EPILP_CASES, ids=_ids(M.EPILP_CASES))
def test_channel_epilogue_16_bit_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    xdt, rdt, ydt = M.epilp_types(case)
    x = _leaf(t["x"].to(xdt))
    b = _leaf(t["bias"]) if case.bias else None
    r = _leaf(t["res"].to(rdt)) if rdt is not None else None
    before = x.detach().clone()
    y = ops.channel_epilogue_lp(x, b, r, ops.EPI_GELU if case.act == "gelu" else ops.EPI_NONE, ydt)
    y.backward(_dev(t["d_y"].to(ydt)))
    assert y.dtype == ydt and x.grad.dtype == xdt and torch.equal(x.detach(), before)                # x is left as it was
    got = dict(y=y, dx=x.grad)
    if case.bias:
        assert b.grad.dtype == torch.float32
        got["dbias"] = b.grad
    if r is not None:
        assert r.grad.dtype == rdt
        got["dres"] = r.grad
    _check(case, got)


@pytest.mark.parametrize("case", M.POOL_CASES, ids=_ids(M.POOL_CASES))
def test_gelu_pool_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    B, H, W, d, r = case.B, case.H, case.W, case.d, case.r
    g = torch.Generator().manual_seed(d + r)
    wide = torch.randn(B, H * W, 3 * d, generator=g)
    wide[..., 2 * d:] = t["s"]                                                    # the third column block of a row 3 d wide: s_stride > d
    wg = _leaf(wide)
    dp = _dev(t["d_pooled"])
    if case.via == "block":
        s = (wg * 1.0)[..., 2 * d:]
        assert ops._rows(s, "s")[1] == 3 * d                                      # taken where it is, not copied
        pooled = ops.gelu_pool(s, H, W, r)
        pooled.backward(dp)
        assert float(wg.grad[..., :2 * d].abs().max()) == 0.0
        ds = wg.grad[..., 2 * d:]
    else:                                                                         # the gradient goes into the split's shared buffer: ds_stride > d
        _, _, s = ops.split_cols(wg * 1.0, (d, d, d))
        slot = s._mlagg_slot
        buf = slot.arena.buffer()
        buf.fill_(SENTINEL)
        pooled = ops.gelu_pool(s, H, W, r)
        assert slot.claimed
        (ds,) = torch.autograd.grad(pooled, s, dp)
        assert slot.arena.buf is buf and torch.equal(buf[..., 2 * d:], ds) and buf.stride(1) == 3 * d
        assert bool((buf[..., :2 * d] == SENTINEL).all())                         # nothing written beside the slot
    _check(case, dict(pooled=pooled, ds=ds))


def test_refusals_are_raised_before_any_launch():
    from mlagg_unet_amd import ops
    refusals = dict(M.REFUSALS)
    H, W, d, r = refusals["gelu_pool"]
    with pytest.raises(RuntimeError):                                             # r * d / 4 = 384 threads per window
        ops.gelu_pool(torch.randn(2, H * W, d, device=DEV), H, W, r)
    CB = refusals["index_scan"]
    with pytest.raises(RuntimeError):                                             # the LDS tile of 513 channels
        ops.index_scan(torch.randn(1, 4, CB, device=DEV), torch.arange(4, dtype=torch.int32, device=DEV).view(1, 4), CB)
    per = refusals["scaled_residual"]
    with pytest.raises(RuntimeError):                                             # samples that are no whole float4
        ops.scaled_residual(torch.randn(2, per, device=DEV), torch.randn(2, per, device=DEV), torch.ones(2, device=DEV))
    O, H, W = refusals["pixel_shuffle2"]
    with pytest.raises(RuntimeError):                                             # odd width: no pixel pairs
        ops._pixel_shuffle2(torch.randn(1, 4 * O, H, W, device=DEV), 1, O, H, W, False)
