"""GPU: K18 and K19 against the float64 references of tests/_conv_kernel_cases.py at the shapes where their launchers change tile,
form or slab geometry (tests/test_conv_kernel_paths_cpu.py shows which case enters which path, that the path predicates are the
launchers' own answers, and that the cases are well conditioned).  One test per family; each case runs the op through ops forward
and backward with every supported product planned onto the kernel, checks on the recorded launches that the kernel entry points ran
with the operands where they are, and compares y, dx and dW with the reference.  The weight gradient runs twice behind NaN-filled
memory: finite (no partial row left unwritten) and bit-identical (fixed-order reductions)."""
import pytest
import torch

from tests import _conv_kernel_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(cases):
    return [c.id for c in cases]


def _block_of_wider(t, seed):
    """`t` (B, C, ...) as the channel block [8, 8 + C) of a random map 16 channels wider, on the device: (the wide map, the block)."""
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(t.shape[0], t.shape[1] + M.SLICE_EXTRA, *t.shape[2:], generator=g)
    wide[:, M.SLICE_AT:M.SLICE_AT + t.shape[1]] = t
    wide = wide.to(DEV)
    return wide, wide[:, M.SLICE_AT:M.SLICE_AT + t.shape[1]]


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


def _poison(floats):
    """Fill and free `floats` floats of device memory with NaN: the next allocation of that size is likely to be handed them."""
    junk = torch.full((max(int(floats), 1),), float("nan"), device=DEV)
    del junk


def _names(launches):
    return [n for n, _ in launches]


def _run(case, launches):
    """{quantity: device tensor} of one case, the launches checked."""
    from mlagg_unet_amd import _lib, ops
    lib = _lib.lib()
    t = M.inputs(case)
    B, I, O, P = case.B, case.I, case.O, M.pixels(case.dims)
    on = M.on_kernel(case)
    xw = dyw = None
    if case.sliced == "x":
        xw, x = _block_of_wider(t["x"], 1)
        assert ops._planes(x, "x")[1] == xw.stride(0) > I * P                      # taken where it is, not copied
        x = x.detach()
    else:
        x = t["x"].to(DEV)
    w = t["w"].to(DEV)
    if case.sliced == "dy":
        dyw, dy = _block_of_wider(t["dy"], 2)
        assert ops._planes(dy, "dy")[1] == dyw.stride(0) > O * P
    else:
        dy = t["dy"].to(DEV)
    x_batch, dy_batch = (xw.stride(0) if xw is not None else I * P), (dyw.stride(0) if dyw is not None else O * P)

    if len(case.dims) == 3:
        assert case.family == "k19_fwd" and case.form == 3 and all(on.values())
        fwd_name, wgrad_name, ws_floats = "mlagg_conv3x3x3_fwd", "mlagg_conv3x3x3_wgrad", lib.mlagg_conv3x3x3_wgrad_workspace_floats(B, O, I, *case.dims)

        def op(xx, ww):
            assert ops.conv_nd_plan(xx, ww, (1, 1, 1), (1, 1, 1)) == ("K19", "K19", "K19")
            return ops.conv_nd(xx, ww, (1, 1, 1), (1, 1, 1))
    elif case.family == "k18":
        plan = tuple("K18" if on[q] else None for q in ("y", "dx", "dW"))
        assert plan == ("K18", "K18", "K18")
        fwd_name, wgrad_name, ws_floats = "mlagg_conv1x1_fwd_acc", "mlagg_conv1x1_wgrad_lp", lib.mlagg_conv1x1_wgrad_workspace_floats(B, O, I, P)

        def op(xx, ww):
            return ops.Conv1x1Fn.apply(xx, ww, case.form, plan)
    else:
        H, W = case.dims
        assert on == dict(y=bool(lib.mlagg_conv3x3_supported(O, I, H, W)), dx=bool(lib.mlagg_conv3x3_supported(I, O, H, W)),
                          dW=bool(lib.mlagg_conv3x3_wgrad_supported(O, I, H, W)))
        plan = tuple("K19" if on[q] else None for q in ("y", "dx", "dW"))
        assert plan[0 if case.family == "k19_fwd" else 2] == "K19", plan           # the product the case is about
        fwd_name, wgrad_name = "mlagg_conv3x3_fwd_lp", "mlagg_conv3x3_wgrad_lp"
        ws_floats = lib.mlagg_conv3x3_wgrad_workspace_floats(B, O, I, H, W) if on["dW"] else 0

        def op(xx, ww):
            return ops.Conv3x3Fn.apply(xx, ww, case.form, None, plan)
    assert not on["dW"] or ws_floats > 0

    if not case.backward:
        with torch.no_grad():
            y = op(x, w)
        assert _names(launches) == [fwd_name] and launches[0][1][1] == x_batch
        return dict(y=y)

    x.requires_grad_(True)
    w.requires_grad_(True)
    y = op(x, w)
    n_fwd = len(launches)
    _poison(ws_floats)
    dx, dW = torch.autograd.grad(y, (x, w), dy, retain_graph=True)
    n_first = len(launches)
    _poison(ws_floats)
    dW2, = torch.autograd.grad(y, (w,), dy)
    torch.cuda.synchronize()

    # the kernels ran, on the operands where they are (the second backward repeats the data gradient too: what a node computes is
    # settled when it is recorded)
    fwd_calls = [a for n, a in launches if n == fwd_name]
    wgrad_calls = [a for n, a in launches if n == wgrad_name]
    # launches per product: one, but a volume's contraction runs in blocks of at most ops.K19_3D_CHAIN_CH channels
    per_y, per_dx = (len(ops._k19_3d_blocks(I)), len(ops._k19_3d_blocks(O))) if len(case.dims) == 3 else (1, 1)
    assert len(fwd_calls) == per_y * int(on["y"]) + 2 * per_dx * int(on["dx"]) and len(wgrad_calls) == 2 * int(on["dW"]), _names(launches)
    if on["y"]:
        assert _names(launches[:n_fwd]) == [fwd_name] * per_y and fwd_calls[0][1] == x_batch
    if on["dx"]:
        assert fwd_name in _names(launches[n_fwd:n_first]) and fwd_name in _names(launches[n_first:])
        assert fwd_calls[-1][1] == fwd_calls[-2][1] == dy_batch
    for a in wgrad_calls:
        assert (a[1], a[3]) == (dy_batch, x_batch), (a[1], a[3])
    if on["dW"]:
        assert bool(torch.isfinite(dW).all()), "a partial row of the workspace was read but never written"
        assert torch.equal(dW, dW2), "two runs of the weight gradient differ"
        for ky in M.zero_rows(case):
            assert float(dW[:, :, ky].abs().max()) == 0.0, f"kernel row {ky} of a one-row image"
    return dict(y=y.detach(), dx=dx, dW=dW)


def _check(case, got):
    ref, tols = M.reference(case), M.bounds(case)
    failed = []
    for q in got:
        assert got[q].shape == ref[q].shape, (q, got[q].shape, ref[q].shape)
        err = M.error(got[q], ref[q])
        if q in M.compared(case):
            print(f"{case.id} {q}: error {err:.2e} (bound {tols[q]:.1e})")
            if not err < tols[q]:                                                  # (a NaN fails too)
                failed.append((q, err, tols[q]))
        else:
            print(f"{case.id} {q}: error {err:.2e} (on the library: not compared)")
            assert bool(torch.isfinite(got[q]).all()), q
    assert set(M.compared(case)) <= set(got) and not failed, failed


def _sentinel_check(case, y):
    """The forward once more into the channel block [4, 4 + O) of a buffer filled with a sentinel: the block equals `y` and the planes
    beside it keep every bit."""
    from mlagg_unet_amd import ops
    t = M.inputs(case)
    B, I, O, P = case.B, case.I, case.O, M.pixels(case.dims)
    x, w = t["x"].to(DEV), t["w"].to(DEV)
    wide = torch.full((B, O + 8) + case.dims, -12345.678, device=DEV)
    before = wide.clone()
    out = wide[:, 4:4 + O]
    if case.family == "k18":
        assert B == 1                                                              # _conv1x1_k18 writes samples O * P apart
        ops._conv1x1_k18(x, I * P, w.reshape(O, I).contiguous(), out, B, O, I, P, case.form)
    else:
        H, W = case.dims
        ops._conv3x3_k19(x, I * P, w, False, O, I, H, W, case.form, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, y), "the channel block differs from the contiguous output"
    assert torch.equal(wide[:, :4], before[:, :4]) and torch.equal(wide[:, 4 + O:], before[:, 4 + O:]), "written beside the output"


@pytest.mark.parametrize("case", M.K19_FWD_CASES, ids=_ids(M.K19_FWD_CASES))
def test_conv3x3_forward_tiles_match_float64(case, launches):
    """Largest errors on the MI355X: y 8.1e-7, dx 1.3e-6, dW 3.1e-7 of the maximum.

    F16 is the case that found the length of K19's accumulator chains: its data gradient contracts 96 channels x 27 taps = 2592 products,
    which the kernel adds into one fp32 chain, and measured 2.65e-6 against the 2e-6 bound (864 products, F1: 9.7e-7; 1728, F4: 1.3e-6;
    on the host an fp32 chain with one rounding per product errs by 2.08e-6 on these inputs, one with a rounding per 16 products by
    5.3e-7).  ops._conv3x3x3_k19 now runs a volume's contraction in blocks of at most ops.K19_3D_CHAIN_CH channels and adds the partial
    outputs: 8.1e-7."""
    got = _run(case, launches)
    _check(case, got)
    if case.id in M.SENTINEL_CASES:
        _sentinel_check(case, got["y"])


@pytest.mark.parametrize("case", M.K19_WGRAD_CASES, ids=_ids(M.K19_WGRAD_CASES))
def test_conv3x3_weight_gradient_slabs_match_float64(case, launches):
    got = _run(case, launches)
    assert "dW" in M.compared(case)
    _check(case, got)


@pytest.mark.parametrize("case", M.K18_CASES, ids=_ids(M.K18_CASES))
def test_conv1x1_tiles_and_slabs_match_float64(case, launches):
    got = _run(case, launches)
    assert M.compared(case) == ["y", "dx", "dW"]
    _check(case, got)
    if case.id in M.SENTINEL_CASES:
        _sentinel_check(case, got["y"])
