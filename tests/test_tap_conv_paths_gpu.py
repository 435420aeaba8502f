"""GPU: K15, K16, K19t and the padded copies of mlagg_volume_pad against the float64 references of tests/_tap_conv_cases.py at the
shapes where their launchers and loops change slab, tail, tile, chunk or guard (tests/test_tap_conv_paths_cpu.py shows which case
enters which path, that the path predicates are the launchers' own answers, and that the cases are well conditioned).  Each case runs
the op through ops forward and backward with every product on the kernel the case is about, checks on the recorded launches that the
intended entry points ran with the operands where they lie, and compares y, dx and dW with the reference.  Every weight gradient runs
twice behind NaN-filled freed memory: finite (no partial row, no guard float left unwritten) and bit-identical (fixed-order sums)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import _tap_conv_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(cases):
    return [c.id for c in cases]


@pytest.fixture
def launches(monkeypatch):
    """Every entry point ops launches, in order: [(name, args)]."""
    from mlagg_unet_amd import ops
    seen, real = [], ops._launch

    def record(name, *args):
        seen.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(ops, "_launch", record)
    return seen


@pytest.fixture
def no_floor(monkeypatch):
    """Every product of the transposed convolution on K19t, at any size."""
    from mlagg_unet_amd import ops
    monkeypatch.setattr(ops, "K19_MIN_PIXELS", 0)
    monkeypatch.setattr(ops, "LP_K_MIN_PIXELS", 0)
    monkeypatch.setattr(ops, "K19T_WGRAD", True)


def _poison(*floats):
    """Fill and free blocks of `floats` floats of device memory with NaN: the next allocations of those sizes are likely to be handed
    them."""
    junk = [torch.full((max(int(n), 1),), float("nan"), device=DEV) for n in floats]
    del junk


def _names(launches):
    return [n for n, _ in launches]


def _calls(launches, name):
    return [a for n, a in launches if n == name]


def _box(case, wide):
    """(row floats, Q8, phases of the input copy) of a convolution case's padded copies."""
    d3 = M.dims3(case.dims)
    _, _, _, guard = M.pad_geometry(*d3, case.stride, wide)
    Q, Q8 = M.box_q(*d3, case.stride, wide)
    return 2 * guard + Q, Q8, (8 if case.stride == 2 else 1)


def _scratch_sizes(case, wide):
    """Floats of the buffers a backward allocates: K15's workspace and the two padded copies."""
    from mlagg_unet_amd import _lib
    row, Q8, nph = _box(case, wide)
    ws = _lib.lib().mlagg_conv_wgrad_taps_workspace_floats(case.B, Q8, case.O, case.I, M.ntaps(case))
    assert ws > 0
    return ws, case.B * nph * case.I * row, case.B * case.O * row


def _check_wgrad_launch(case, a, wide):
    """mlagg_conv_wgrad_taps(A, a_batch, a_row, B, b_batch, b_row, off, ntaps, Q, O, I, batch, dW, accumulate, ws): the strides of
    the padded copies, the whole 8-voxel steps over the box, overwrite."""
    row, Q8, nph = _box(case, wide)
    assert (a[1], a[2], a[4], a[5]) == (case.O * row, row, nph * case.I * row, row), a[:6]
    assert (a[7], a[8], a[9], a[10], a[11], a[13]) == (M.ntaps(case), Q8, case.O, case.I, case.B, 0), a[7:14]


def _check(case, got, ref, yard):
    tols = dict(M.bounds(case))
    tols["dW"] = M.dw_bound(case, ref["dW"], yard["dW"])
    failed = []
    for q in M.compared(case):
        assert got[q].shape == ref[q].shape, (q, got[q].shape, ref[q].shape)
        err = M.error(got[q], ref[q])
        print(f"{case.id} {q}: error {err:.2e} (bound {tols[q]:.1e})")
        if not err < tols[q]:                                                      # (a NaN fails too)
            failed.append((q, err, tols[q]))
    assert not failed, failed
    for idx in M.zero_taps(case):
        assert float(got["dW"][(slice(None), slice(None)) + idx].abs().max()) == 0.0, f"kernel plane / row {idx} sees padding only"


def _run_conv(case, launches):
    """{quantity: device tensor} of a K15 / K16 case, the launches checked."""
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    nd, d3 = len(case.dims), M.dims3(case.dims)
    x, w, dy = t["x"].to(DEV), t["w"].to(DEV), t["dy"].to(DEV)
    stride, padding = (case.stride,) * nd, (case.k // 2,) * nd
    wide = case.family == "k16"
    sizes = _scratch_sizes(case, wide)
    pad_common = (case.stride, int(wide))

    if case.family == "k15":
        assert ops.conv_wgrad_supported(x, w, stride, padding)
        _poison(*sizes)
        dW = ops.conv_weight_grad(x, dy, case.k, case.stride).view(w.shape)
        n_first = len(launches)
        _poison(*sizes)
        dW2 = ops.conv_weight_grad(x, dy, case.k, case.stride).view(w.shape)
        torch.cuda.synchronize()
        assert _names(launches) == ["mlagg_volume_pad", "mlagg_volume_pad", "mlagg_conv_wgrad_taps"] * 2
        px, pdy, wg = (a for _, a in launches[:n_first])
        assert px[0] == x.data_ptr() and px[2:] == (case.B, case.I) + d3 + pad_common + (0, 0, 0, 0)
        assert pdy[0] == dy.data_ptr() and pdy[2:] == (case.B, case.O) + d3 + pad_common + (1,) + M.dims3(M.y_dims(case))
        _check_wgrad_launch(case, wg, False)
        got = dict(dW=dW)
    else:
        plan = ops.conv_nd_plan(x, w, stride, padding)
        assert plan == (("K16", "K16", "K15") if wide else (None, None, "K15")), plan
        x.requires_grad_(True)
        w.requires_grad_(True)
        y = ops.conv_nd(x, w, stride, padding)
        n_fwd = len(launches)
        _poison(*sizes)
        dx, dW = torch.autograd.grad(y, (x, w), dy, retain_graph=True)
        n_first = len(launches)
        # once more (a K16 layer from its forward on: its backward gives the shared padded copy of x up)
        y2 = ops.conv_nd(x, w, stride, padding) if wide else y
        _poison(*sizes)
        dW2, = torch.autograd.grad(y2, (w,), dy)
        torch.cuda.synchronize()
        assert torch.equal(y2, y)
        fwd, bwd = launches[:n_fwd], launches[n_fwd:n_first]
        if wide:
            # forward: the wide copy of x and K16 on it; backward: the wide copy of dy, K16 on it with the taps flipped, and K15 on both
            assert _names(fwd) == ["mlagg_volume_pad", "mlagg_conv_taps"]
            assert sorted(_names(bwd)) == ["mlagg_conv_taps", "mlagg_conv_wgrad_taps", "mlagg_volume_pad"]
            px, ct = fwd[0][1], fwd[1][1]
            pdy, ctb, wg = (_calls(bwd, n)[0] for n in ("mlagg_volume_pad", "mlagg_conv_taps", "mlagg_conv_wgrad_taps"))
            row = _box(case, True)[0]
            assert px[2:] == (case.B, case.I) + d3 + (1, 1, 0, 0, 0, 0) and pdy[2:] == (case.B, case.O) + d3 + (1, 1, 1) + d3
            # mlagg_conv_taps(xp, x_batch, x_row, weight, w_so, w_si, flip, off, ntaps, y, B, O, I, D, H, W)
            assert ct[1:3] == (case.I * row, row) and ct[6] == 0 and ct[8] == M.ntaps(case) and ct[10:] == (case.B, case.O, case.I) + d3
            assert ctb[1:3] == (case.O * row, row) and ctb[6] == 1 and ctb[10:] == (case.B, case.I, case.O) + d3
            # K15 reads the copies K16 read: no third and fourth copy
            assert (wg[0], wg[3]) == (ctb[0], ct[0])
            assert _names(launches[n_first:]).count("mlagg_conv_wgrad_taps") == 1
        else:
            assert _names(fwd) == [] and _names(bwd) == ["mlagg_volume_pad", "mlagg_volume_pad", "mlagg_conv_wgrad_taps"]
            wg = bwd[2][1]
            assert bwd[0][1][2:] == (case.B, case.I) + d3 + pad_common + (0, 0, 0, 0)
        _check_wgrad_launch(case, wg, wide)
        got = dict(y=y.detach(), dx=dx, dW=dW)
    assert bool(torch.isfinite(dW).all()), "a partial row of the workspace or a guard float was read but never written"
    assert torch.equal(dW, dW2), "two runs of the weight gradient differ"
    return got


def _run_and_check(case, launches):
    ref, yard = M.reference(case), M.yardstick(case)
    got = _run_conv(case, launches)
    if case.family == "k15_nd":                                                    # y and dx are the library's: finite, not compared
        assert bool(torch.isfinite(got["y"]).all()) and bool(torch.isfinite(got["dx"]).all())
    _check(case, got, ref, yard)


@pytest.mark.parametrize("case", M.K15_CASES, ids=_ids(M.K15_CASES))
def test_k15_weight_gradient_slabs_tails_and_tiles_match_float64(case, launches):
    """Largest error on the MI355X: dW 4.2e-7 (A5) of the maximum."""
    _run_and_check(case, launches)


@pytest.mark.parametrize("case", M.K15_ND_CASES, ids=_ids(M.K15_ND_CASES))
def test_k15_behind_conv_nd_matches_float64(case, launches):
    """Largest error on the MI355X: dW 4.8e-7 (N3) of the maximum."""
    _run_and_check(case, launches)


@pytest.mark.parametrize("case", M.K16_CASES, ids=_ids(M.K16_CASES))
def test_k16_workgroups_chunks_and_tiles_match_float64(case, launches):
    """Largest errors on the MI355X: y 1.2e-6 (T4), dx 1.1e-6 (T3), dW 2.9e-7 (T7) of the maximum.  T7 is the one-slice volume that
    conv_nd_plan sent to K19, whose launcher refuses it."""
    _run_and_check(case, launches)


@pytest.mark.parametrize("cid", M.ACCUMULATE_CASES)
def test_k15_accumulates_into_the_weight_gradient(cid):
    """mlagg_conv_wgrad_taps with accumulate = 1 on the C ABI: dW0 + dW, and once more on the same buffer, each step against float64."""
    from mlagg_unet_amd import _lib, ops
    case = M.by_id(cid)
    ref, yard = M.reference(case), M.yardstick(case)
    bound = M.dw_bound(case, ref["dW"], yard["dW"])
    t = M.inputs(case)
    d3 = M.dims3(case.dims)
    xp = ops._Padded(t["x"].to(DEV), d3, case.stride, False)
    dyp = ops._Padded(t["dy"].to(DEV), d3, case.stride, False, as_output_of=xp)
    taps = ops._tap_offsets(case.k, len(case.dims), case.stride, xp.Hq, xp.Wq, case.I, xp.row)
    n, Q8 = len(taps), (xp.Q + 7) & ~7
    assert n == M.ntaps(case)
    off = (ctypes.c_long * n)(*taps)
    g = torch.Generator().manual_seed(n + case.O)
    dW0 = torch.randn(case.O, case.I, n, generator=g) * float(ref["dW"].abs().max())
    buf = dW0.to(DEV)
    want = dW0.double()
    scale = float(ref["dW"].abs().max())
    for step in (1, 2):
        ws = torch.full((_lib.lib().mlagg_conv_wgrad_taps_workspace_floats(case.B, Q8, case.O, case.I, n),), float("nan"), device=DEV)
        ops._launch("mlagg_conv_wgrad_taps", dyp.ptr(), case.O * dyp.row, dyp.row, xp.ptr(), xp.nph * case.I * xp.row, xp.row, off, n, Q8,
                    case.O, case.I, case.B, buf.data_ptr(), 1, ws.data_ptr())
        torch.cuda.synchronize()
        want = want + ref["dW"].reshape(case.O, case.I, n)
        err = float((buf.cpu().double() - want).abs().max()) / scale
        print(f"{cid} accumulate step {step}: error {err:.2e} (bound {bound:.1e})")
        assert err < bound, (step, err, bound)
        want = buf.cpu().double()                                                  # the next step adds to what is there


@pytest.mark.parametrize("row", M.PAD_CASES, ids=[r[0] for r in M.PAD_CASES])
def test_volume_pad_writes_the_whole_row_exactly(row):
    """mlagg_volume_pad into NaN-filled memory: every float of every row -- the guards, the zero ring, the data -- equals the host
    construction, and nothing beside the rows is written."""
    from mlagg_unet_amd import ops
    name, B, C, dims, stride, wide, out = row
    g = torch.Generator().manual_seed(len(name) + sum(dims))
    src = torch.randn(B, C, *(out or dims), generator=g)
    want = M.padded_rows(src, dims, stride, wide, out is not None)
    n, margin = want.numel(), 64
    big = torch.full((n + 2 * margin,), float("nan"), device=DEV)
    dst = big[margin:margin + n]
    ops._launch("mlagg_volume_pad", src.to(DEV).data_ptr(), dst.data_ptr(), B, C, *dims, stride, wide, int(out is not None), *(out or (0, 0, 0)))
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu().view(want.shape), want)
    assert bool(torch.isnan(big[:margin]).all()) and bool(torch.isnan(big[margin + n:]).all()), "written beside the rows"


def test_volume_pad_refuses_what_it_cannot_lay_out():
    from mlagg_unet_amd import _lib
    lib = _lib.lib()
    src, dst = torch.zeros(4096, device=DEV), torch.zeros(65536, device=DEV)
    for dims, stride, wide, out in M.PAD_REFUSED:
        rc = lib.mlagg_volume_pad(src.data_ptr(), dst.data_ptr(), 1, 1, *dims, stride, wide, int(out is not None), *(out or (0, 0, 0)), _lib.stream())
        assert rc == _lib.CONSTANTS["MLAGG_E_UNSUPPORTED"], (dims, stride, wide, out, rc)
    torch.cuda.synchronize()
    assert float(dst.abs().max()) == 0.0


@pytest.mark.parametrize("case", M.K19T_CASES, ids=_ids(M.K19T_CASES))
def test_k19t_tiles_loops_and_parts_match_float64(case, launches, no_floor):
    """Largest errors on the MI355X: form 3 y 7.6e-7, dx 4.7e-7 (P11), dW 2.3e-7 (P5);
    forms 1 and 2 y 1.9e-7, dx 3.3e-7, dW 1.2e-7 of the maximum."""
    from mlagg_unet_amd import _lib, ops
    ref, yard = M.reference(case), M.yardstick(case)
    t = M.inputs(case)
    B, I, O, (H, W) = case.B, case.I, case.O, case.dims
    assert ops._s2t_plan(O, I, H, W, case.form) == ("K19t", "K19t", "K19t")
    w = t["w"].to(DEV).requires_grad_(True)
    ws_floats = _lib.lib().mlagg_conv3x3_s2t_wgrad_workspace_floats(B, O, I, H, W)
    assert ws_floats > 0
    if case.sliced == "views":
        g = torch.Generator().manual_seed(H * W)
        wider = torch.randn(B, I + M.SLICE_EXTRA, H, W, generator=g)
        wider[:, M.SLICE_AT:M.SLICE_AT + I] = t["x"]
        x = wider.to(DEV)[:, M.SLICE_AT:M.SLICE_AT + I].detach().requires_grad_(True)
        full = torch.randn(B, O, 2 * H, 2 * W, generator=g)
        full[:, :, 1:, 1:] = t["dy"]
        full = full.to(DEV)
        y = ops.conv3x3_s2t(x, w, case.form)
        dy = full[:, :, 1:, 1:]                                                     # the interior of the padded gradient, where it lies
        x_batch, dy_strides = x.stride(0), (O * 4 * H * W, 4 * H * W, 2 * W)
        assert x_batch > I * H * W and dy.stride()[:3] == dy_strides and not dy.is_contiguous()
        n_fwd = len(launches)
        wd = w.detach()
        dx = ops._k19t_dgrad(dy, wd, O, I, H, W, case.form)
        _poison(ws_floats)
        dW = ops._k19t_wgrad(x.detach(), x_batch, dy, O, I, H, W, case.form)
        n_first = len(launches)
        _poison(ws_floats)
        dW2 = ops._k19t_wgrad(x.detach(), x_batch, dy, O, I, H, W, case.form)
        # and through PatchExpand's pad, whatever layout autograd hands the kernels: the same sums in the same order
        dxa, dWa = torch.autograd.grad(F.pad(y, (1, 0, 1, 0)), (x, w), full)
        assert torch.equal(dxa, dx) and torch.equal(dWa, dW)
    else:
        x = t["x"].to(DEV).requires_grad_(True)
        y = ops.conv3x3_s2t(x, w, case.form)
        dy = t["dy"].to(DEV)
        x_batch, dy_strides = I * H * W, (O * (2 * H - 1) * (2 * W - 1), (2 * H - 1) * (2 * W - 1), 2 * W - 1)
        n_fwd = len(launches)
        _poison(ws_floats)
        dx, dW = torch.autograd.grad(y, (x, w), dy, retain_graph=True)
        n_first = len(launches)
        _poison(ws_floats)
        dW2, = torch.autograd.grad(y, (w,), dy)
    torch.cuda.synchronize()
    assert _names(launches[:n_fwd]) == ["mlagg_conv3x3_s2t_fwd"] and launches[0][1][1] == x_batch
    assert sorted(_names(launches[n_fwd:n_first])) == ["mlagg_conv3x3_s2_dgrad", "mlagg_conv3x3_s2t_wgrad"]
    dg, wg = _calls(launches, "mlagg_conv3x3_s2_dgrad")[0], _calls(launches, "mlagg_conv3x3_s2t_wgrad")[0]
    assert dg[1:4] == dy_strides and (wg[1],) + wg[3:6] == (x_batch,) + dy_strides, (dg[1:4], wg[1:6])
    assert dg[-1] == wg[-1] == launches[0][1][-1] == case.form
    assert bool(torch.isfinite(dW).all()), "a partial row of the workspace was read but never written"
    assert torch.equal(dW, dW2), "two runs of the weight gradient differ"
    _check(case, dict(y=y.detach(), dx=dx, dW=dW), ref, yard)
