"""GPU: K2 / K2n / K2v, K6 and K10 against the float64 references of tests/_map_kernel_cases.py at the sizes where their dispatch
changes path (tests/test_map_kernel_paths_cpu.py shows which case enters which path and that the cases are well conditioned).
One test per op family; each runs the op forward and backward on the device and compares the output and EVERY gradient."""
import pytest
import torch

from tests import _map_kernel_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(cases):
    return [M.case_id(c) for c in cases]


def _dev(t):
    return t.to(DEV)


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


def _padded(t, pad):
    """`t` (..., C) as the column block [4, 4 + C) of a wider random row: (the wide leaf, the block)."""
    g = torch.Generator().manual_seed(t.shape[-1] + pad)
    wide = torch.randn(*t.shape[:-1], t.shape[-1] + pad, generator=g)
    wide[..., 4:4 + t.shape[-1]] = t
    wide = _leaf(wide)
    return wide, wide[..., 4:4 + t.shape[-1]]


def _padded_grad(wide, C):
    """The block's gradient; nothing may have been written beside it."""
    g = wide.grad
    assert float(g[..., :4].abs().max()) == 0.0 and float(g[..., 4 + C:].abs().max()) == 0.0
    return g[..., 4:4 + C]


def _check(case, got):
    ref, yard = M.reference_and_yardstick(case)
    tols = M.bounds(case, ref, yard)
    assert set(got) == set(tols), set(got) ^ set(tols)
    failed = []
    for q, tol in tols.items():
        assert got[q].shape == ref[q].shape, (q, got[q].shape, ref[q].shape)
        err, excess = M.error(got[q], ref[q], tol, M.mask_for(case, q, ref))
        print(f"{M.family(case)} {M.case_id(case)} {q}: error {err:.2e} ({tol.kind} {tol.a:.2e}, {tol.r:.0e})")
        if not excess <= 0.0:                                                     # (a NaN fails too)
            failed.append((q, err, tol))
    assert not failed, failed


@pytest.mark.parametrize("case", M.K2_CASES, ids=_ids(M.K2_CASES))
def test_dwconv3x3_nlc_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    B, H, W, C = case.B, case.H, case.W, case.C
    w, b = _leaf(t["w"]), _leaf(t["b"])
    got = {}
    if case.form in ("gated", "packed"):
        arena = _leaf(torch.cat([t["x"], t["v"], torch.ones(B, H * W, 8)], -1))  # x | gate | 8 columns nobody uses
        if case.form == "packed":
            a, v, _ = ops.split_cols(arena * 1.0, (C, C, 8))
            assert getattr(a, "_mlagg_slot", None) is not None and getattr(v, "_mlagg_slot", None) is not None
        else:
            a, v = (arena * 1.0)[..., :C].contiguous(), (arena * 1.0)[..., C:2 * C].contiguous()
        y = ops.dwconv3x3_gated(a, v, w, b, H, W)
        y.backward(_dev(t["d_y"]))
        assert float(arena.grad[..., 2 * C:].abs().max()) == 0.0                  # outside the two column blocks: exactly zero
        got.update(dx=arena.grad[..., :C], dv=arena.grad[..., C:2 * C])
    else:
        wide, x = _padded(t["x"], case.pad) if case.pad else (None, _leaf(t["x"]))
        assert not case.pad or ops._rows(x, "x")[1] == C + case.pad              # taken where it is, not copied
        r = _leaf(t["r"]) if case.form == "res" else None
        y = ops.dwconv3x3_nlc(x, w, b, H, W, silu=case.form == "silu", res=r)
        y.backward(_dev(t["d_y"]))
        got["dx"] = _padded_grad(wide, C) if case.pad else x.grad
        if r is not None:
            got["dr"] = r.grad
    got.update(y=y, dw=w.grad, db=b.grad)
    _check(case, got)


@pytest.mark.parametrize("case", M.K2N_CASES, ids=_ids(M.K2N_CASES))
def test_dwconv3x3_nchw_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    x, w, b = _leaf(t["x"]), _leaf(t["w"]), _leaf(t["b"])
    if case.form == "res":
        out = ops.dwconv3x3_nchw_res(x, w, b)
        assert out is not None
        y, xres = out
        torch.autograd.backward([y, xres], [_dev(t["d_y"]), _dev(t["d_xres"])])
        _check(case, dict(y=y, xres=xres, dx=x.grad, dw=w.grad, db=b.grad))
    else:
        y = ops.dwconv3x3_nchw(x, w, b, case.stride)
        y.backward(_dev(t["d_y"]))
        _check(case, dict(y=y, dx=x.grad, dw=w.grad, db=b.grad))


@pytest.mark.parametrize("case", M.K2V_CASES, ids=_ids(M.K2V_CASES))
def test_dwconv3d_nlc_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    w = _leaf(t["w"])
    b = _leaf(t["b"]) if case.bias else None
    wide, x = _padded(t["x"], case.pad) if case.pad else (None, _leaf(t["x"]))
    assert not case.pad or ops._rows(x, "x")[1] == case.C + case.pad
    y = ops.dwconv3d_nlc(x, w, b, case.dims, silu=case.silu)
    y.backward(_dev(t["d_y"]))
    got = dict(y=y, dx=_padded_grad(wide, case.C) if case.pad else x.grad, dw=w.grad)
    if case.bias:
        got["db"] = b.grad
    _check(case, got)


@pytest.mark.parametrize("case", M.K6_CASES, ids=_ids(M.K6_CASES))
def test_layer_norm_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    C = case.C
    w, b = _leaf(t["w"]), _leaf(t["b"])
    if case.form == "res":
        skip, branch = _leaf(t["skip"]), _leaf(t["branch"])
        xsum, y = ops.residual_layer_norm(skip, branch, _dev(torch.tensor(M.K6_RES_SCALE)), w, b, M.EPS)
        if case.use_sum:                                                          # a second consumer of the sum
            torch.autograd.backward([y, xsum], [_dev(t["d_y"]), _dev(t["d_xsum"])])
        else:
            y.backward(_dev(t["d_y"]))
        _check(case, dict(xsum=xsum, y=y, dskip=skip.grad, dbranch=branch.grad, dw=w.grad, db=b.grad))
        return

    def second_half(v):                                                           # the columns [C, 2C) of a row twice as wide
        return _dev(torch.cat([torch.full_like(v, 7.0), v], 1))[:, C:]

    x = (second_half(t["x"]) if case.strided_x else _dev(t["x"])).detach().requires_grad_(True)
    dy = second_half(t["d_y"]) if case.strided_dy else _dev(t["d_y"])
    assert x.is_contiguous() != case.strided_x and dy.is_contiguous() != case.strided_dy
    y = ops.layer_norm(x, w, b, M.EPS)
    y.backward(dy)
    _check(case, dict(y=y, dx=x.grad, dw=w.grad, db=b.grad))


@pytest.mark.parametrize("case", M.K10_CASES, ids=_ids(M.K10_CASES))
def test_plane_norm_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    dt = M.DTYPES[case.dtype]
    x = _leaf(t["x"].to(dt))
    gamma, beta = (_leaf(t["gamma"]), _leaf(t["beta"])) if case.affine else (None, None)
    r = _leaf(t["r"]) if case.res else None
    dy = _dev(t["d_y"].to(dt))
    if case.dy_slice:                                                             # planes 1 .. C of a map two planes wider
        wide = torch.full((M.K10_B, M.K10_C + 2) + tuple(case.dims), 7.0, device=DEV)
        wide[:, 1:1 + M.K10_C] = dy
        dy = wide[:, 1:1 + M.K10_C]
        assert ops._map_slice(dy, "dy")[1] == wide.stride(0)                      # read where it is
    act = {"none": ops.ACT_NONE, "leaky": ops.ACT_LEAKY, "silu": ops.ACT_SILU}[case.act]
    y = ops.plane_norm(x, gamma, beta, M.EPS, act, M.LEAKY_SLOPE if case.act == "leaky" else 0.0, r, out_dtype=dt)
    assert y.dtype == dt
    y.backward(dy)
    assert x.grad.dtype == dt
    got = dict(y=y, dx=x.grad)
    if case.affine:
        got.update(dgamma=gamma.grad, dbeta=beta.grad)
    if case.res:
        assert r.grad.dtype == torch.float32
        got["dr"] = r.grad
    _check(case, got)
