"""GPU: the token-major projections -- K5 on weight images, the image builders, K5w (both kernels), the round-3 K5 in its three modes
and the fp32 K5 -- against the float64 references of tests/_linear_kernel_cases.py at the sizes where their launchers change tile, slab
or pipeline path (tests/test_linear_kernel_paths_cpu.py shows which case enters which path, that the path predicates are the launchers'
own answers, that the cases are well conditioned and what index errors they catch).

Every case runs through the C ABI (family `ops`: through ops.linear / ops.mlp) into outputs pre-filled with NaN, the workspace too;
a strided output is the column block of a wider tensor whose other columns hold a sentinel and must keep every bit.  Every case runs
twice into the same buffers with a different case in between: the two results are bitwise equal (no stale LDS or workspace state;
K5w has no atomics).  Each compared quantity prints `family id quantity: error (bound)`."""
import pytest
import torch

from tests import _linear_kernel_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _ids(cases):
    return [c.id for c in cases]


def _lib():
    from mlagg_unet_amd import _lib
    return _lib.lib(), _lib.stream()


def _ptr(t):
    return None if t is None else t.data_ptr()


class Out:
    """An output (rows, cols): contiguous (with `tail` more columns behind it), or (strided) the column block LAYOUT[key] of a wider
    tensor."""

    def __init__(self, rows, cols, key, strided, tail=0):
        first, extra = M.LAYOUT[key] if strided else (0, tail)
        self.wide = torch.empty(rows, cols + extra, device=DEV)
        self.view = self.wide[:, first:first + cols]
        self.stride = cols + extra

    def fill(self):
        self.wide.fill_(M.SENTINEL)
        self.view.fill_(NAN)

    def check(self, name):
        assert not bool(torch.isnan(self.view).any()), f"{name}: an element of the output was never written"
        keep = torch.ones(self.wide.shape[1], dtype=torch.bool, device=DEV)
        first = self.view.storage_offset()
        keep[first:first + self.view.shape[1]] = False
        beside = self.wide[:, keep]
        assert torch.equal(beside, torch.full_like(beside, M.SENTINEL)), f"{name}: written beside the output"


def _place(t, key, strided):
    """An input on the device: contiguous, or the column block LAYOUT[key] of a sentinel-filled wider tensor.  (view, row stride)."""
    if not strided:
        return t.to(DEV).contiguous(), t.shape[1]
    first, extra = M.LAYOUT[key]
    wide = torch.full((t.shape[0], t.shape[1] + extra), M.SENTINEL)
    wide[:, first:first + t.shape[1]] = t
    wide = wide.to(DEV)
    return wide[:, first:first + t.shape[1]], wide.shape[1]


class Job:
    """One case on the device: `outs` {quantity: Out}, `scratch` tensors filled with NaN before every run, `launch()`."""

    def __init__(self, case):
        self.case, self.outs, self.scratch, self.steps = case, {}, [], []

    def run(self):
        for o in self.outs.values():
            o.fill()
        for s in self.scratch:
            s.fill_(NAN)
        for step in self.steps:
            step()
        torch.cuda.synchronize()
        return {q: o.view.clone() for q, o in self.outs.items()}


def _check_rc(rc, what):
    from mlagg_unet_amd import _lib
    _lib.check(rc, what)


def _images(w, want_img=True, want_t=True, w_stride=None):
    lib, st = _lib()
    N, K = w.shape
    img = torch.full((lib.mlagg_weight_image_bytes(N, K),), 0xFF, dtype=torch.uint8, device=DEV) if want_img else None
    imgT = torch.full((lib.mlagg_weight_image_bytes(K, N),), 0xFF, dtype=torch.uint8, device=DEV) if want_t else None
    _check_rc(lib.mlagg_weight_image(w.data_ptr(), w_stride or w.stride(0), _ptr(img), _ptr(imgT), N, K, st), "mlagg_weight_image")
    return img, imgT


# ---------------------------------------------------------------------------------------------------------------------
# the jobs of each family
# ---------------------------------------------------------------------------------------------------------------------
def _x3_job(case):
    lib, _ = _lib()
    t = M.inputs(case)
    Mr, N, K = case.M, case.N, case.K
    job = Job(case)
    x, xs = _place(t["x"], "x", case.strided)
    dgrad = M.runs_dgrad(case)
    img, imgT = _images(t["w"].to(DEV), True, dgrad)
    b = t["b"].to(DEV) if case.bias else None
    epi = int(case.mode[1])
    y = job.outs["y"] = Out(Mr, N, "y", case.strided)
    act = None
    if epi == 1:
        act = job.outs["y_act"] = Out(Mr, N, "y_act", case.strided)
    pre, ps = _place(t["pre"], "pre", case.strided) if epi == 2 else (None, 0)
    assert not case.strided or (xs != K and xs % 4 == 0 and y.stride != N and (epi != 2 or ps not in (N, y.stride)))
    assert lib.mlagg_linear_x3_tile(Mr, N, K) == 10 * M.x3_tile(Mr, N)[0] + M.x3_tile(Mr, N)[1]
    keep = [x, img, imgT, b, pre]

    def forward():
        _, st = _lib()
        _check_rc(lib.mlagg_linear_x3(x.data_ptr(), xs, img.data_ptr(), _ptr(b), y.view.data_ptr(), y.stride,
                                      act.view.data_ptr() if act else None, _ptr(pre), ps, Mr, N, K, epi, st), "mlagg_linear_x3")
    job.steps.append(forward)
    if dgrad:
        dy, dys = _place(t["dy"], "dy", case.strided)
        dx = job.outs["dx"] = Out(Mr, K, "dx", case.strided)
        keep.append(dy)

        def backward():
            _, st = _lib()
            _check_rc(lib.mlagg_linear_x3(dy.data_ptr(), dys, imgT.data_ptr(), None, dx.view.data_ptr(), dx.stride, None, None, 0,
                                          Mr, K, N, 0, st), "mlagg_linear_x3 (data gradient)")
        job.steps.append(backward)
    job.keep = keep
    return job


def _wgrad_job(case):
    lib, _ = _lib()
    t = M.inputs(case)
    Mr, O, I = case.M, case.N, case.K
    job = Job(case)
    if case.strided:
        dy, dys = _place(t["dy"], "dy", True)
        xw = torch.full((Mr, I + 1), M.SENTINEL)
        xw[:, :I] = t["x"]
        xw = xw.to(DEV)
        x, xs = xw[:, :I], I + 1                                                   # an odd row stride: legal for K5w
    else:
        (dy, dys), (x, xs) = _place(t["dy"], "dy", False), _place(t["x"], "x", False)
    n = O * I + (O if case.bias else 0)
    ws = torch.empty(lib.mlagg_linear_wgrad_workspace_floats(Mr, O, I), device=DEV)
    assert ws.numel() == M.wgrad_geometry(Mr, O, I).nslabs * (O * I + O)
    job.scratch.append(ws)
    for suffix, entry in (("", lib.mlagg_linear_wgrad), ("_x3", lib.mlagg_linear_wgrad_x3)):
        out = job.outs["flat" + suffix] = Out(1, n, "y", False, tail=O + 16)          # dW | db | a sentinel tail, in one row

        def step(entry=entry, out=out):
            _, st = _lib()
            _check_rc(entry(dy.data_ptr(), dys, x.data_ptr(), xs, out.view.data_ptr(), out.view.data_ptr() + 4 * O * I if case.bias else None,
                            ws.data_ptr(), Mr, O, I, st), "mlagg_linear_wgrad")
        job.steps.append(step)
    job.keep = [dy, x]
    return job


def _wgrad_quantities(case, got):
    O, I = case.N, case.K
    out = {}
    for suffix in ("", "_x3"):
        flat = got["flat" + suffix][0]
        out["dW" + suffix] = flat[:O * I].view(O, I)
        if case.bias:
            out["db" + suffix] = flat[O * I:]
    return out


def _lp_job(case):
    lib, _ = _lib()
    t = M.inputs(case)
    Mr, N, K = case.M, case.N, case.K
    job = Job(case)
    code = None if case.family == "fp32" else {"bf16": 1, "fp16": 2, "bf16x3": 3}[case.mode]
    x, xs = _place(t["x"], "x", case.strided)
    w, wd = t["w"].to(DEV), t["wd"].to(DEV)
    b = t["b"].to(DEV) if case.bias else None
    y = job.outs["y"] = Out(Mr, N, "y", case.strided)
    dy, dys = _place(t["dy"], "dy", case.strided)
    dx = job.outs["dx"] = Out(Mr, N, "dx", case.strided)
    dgrad = M.runs_dgrad(case)

    def forward():
        _, st = _lib()
        args = (x.data_ptr(), xs, w.data_ptr(), _ptr(b), y.view.data_ptr(), y.stride, Mr, N, K)
        _check_rc(lib.mlagg_linear_fwd(*args, st) if code is None else lib.mlagg_linear_lp_fwd(*args, code, st), "forward")

    def backward():                                                                # dx (M, I = N) = dy (M, O = K) . wd (O, I)
        _, st = _lib()
        args = (dy.data_ptr(), dys, wd.data_ptr(), dx.view.data_ptr(), dx.stride, Mr, K, N)
        rc = lib.mlagg_linear_dgrad(*args, st) if code is None else lib.mlagg_linear_lp_dgrad(*args, code, st)
        if dgrad:
            _check_rc(rc, "data gradient")
        else:                                                                      # I % 4 != 0: refused, nothing launched
            assert rc == -1, rc
    job.steps += [forward, backward]
    job.keep = [x, w, wd, b, dy]
    return job


JOBS = {"x3": _x3_job, "wgrad": _wgrad_job, "lp": _lp_job, "fp32": _lp_job}
OTHER = {"x3": ("X-65", "X-129"), "wgrad": ("W-31x33", "W-m17"), "lp": ("L-129x95x36-bf16x3", "L-127x32x28-bf16"),
         "fp32": ("P-129x95x36", "P-127x32x28")}


def _both_ways(case):
    """The case, a different case, the case again into the same buffers: {quantity: tensor} of the first run, bitwise equal to the second."""
    job = JOBS[case.family](case)
    first = job.run()
    other = M.by_id(next(cid for cid in OTHER[case.family] if cid != case.id))
    JOBS[other.family](other).run()
    second = job.run()
    for q in first:
        assert torch.equal(first[q], second[q]) or (bool(torch.isnan(first[q]).all()) and bool(torch.isnan(second[q]).all())), \
            f"{q}: the second run, after {other.id}, differs from the first"
    return job, first


def _compare(case, got):
    ref, tols = M.reference(case), M.bounds(case)
    failed = []
    for q, v in got.items():
        base = q.split("_x3")[0]
        tol = tols[base]
        assert tuple(v.shape) == tuple(ref[base].shape), (q, v.shape, ref[base].shape)
        err = M.error(v, ref[base], tol.kind)
        print(f"{case.family} {case.id} {q}: error {err:.2e} ({tol.kind} bound {tol.a:.1e})")
        if not err < tol.a:                                                        # (a NaN fails too)
            failed.append((q, err, tol))
    assert not failed, failed


# ---------------------------------------------------------------------------------------------------------------------
# K5 on weight images
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.X3_CASES, ids=_ids(M.X3_CASES))
def test_linear_x3_paths_match_float64(case):
    job, got = _both_ways(case)
    for q, o in job.outs.items():
        o.check(f"{case.id} {q}")
    assert set(got) == set(M.compared(case))
    _compare(case, got)


@pytest.mark.parametrize("shape", M.X3_REFUSED, ids=[f"k{s[2]}" for s in M.X3_REFUSED])
def test_linear_x3_refuses_a_contraction_that_is_no_multiple_of_8(shape):
    lib, st = _lib()
    Mr, N, K = shape
    x, y = torch.randn(Mr, 8, device=DEV), torch.full((Mr, N), NAN, device=DEV)
    img = torch.zeros(lib.mlagg_weight_image_bytes(N, 32), dtype=torch.uint8, device=DEV)
    assert lib.mlagg_linear_x3_supported(Mr, N, K) == 0 and lib.mlagg_linear_x3_tile(Mr, N, K) == -1
    assert lib.mlagg_linear_x3(x.data_ptr(), 8, img.data_ptr(), None, y.data_ptr(), N, None, None, 0, Mr, N, K, 0, st) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()), "a refused call wrote its output"


# ---------------------------------------------------------------------------------------------------------------------
# weight images
# ---------------------------------------------------------------------------------------------------------------------
def _decode(buf, rows, cols):
    cp = (cols + 31) // 32 * 32
    return (buf.view(torch.int16).view(3, rows, cp).to(torch.int32) << 16).view(torch.float32)


def _row_block(w):
    """`w` (N, K) as the rows [2, 2 + N), columns [3, 3 + K) of a sentinel-filled wider matrix: w_stride = K + 5 > K."""
    wide = torch.full((w.shape[0] + 3, w.shape[1] + 5), M.SENTINEL)
    wide[2:2 + w.shape[0], 3:3 + w.shape[1]] = w
    wide = wide.to(DEV)
    return wide[2:2 + w.shape[0], 3:3 + w.shape[1]]


@pytest.mark.parametrize("case", M.IMG_CASES, ids=_ids(M.IMG_CASES))
def test_weight_image_is_the_exact_split_of_a_row_block(case):
    N, K = case.N, case.K
    w = _row_block(M.inputs(case)["w"])
    assert w.stride(0) == K + 5 and torch.equal(w.cpu(), M.inputs(case)["w"])
    want_img, want_t = case.mode in ("img", "both"), case.mode in ("imgT", "both")
    img, imgT = _images(w, want_img, want_t)
    other = next(c for c in M.IMG_CASES if (c.N, c.K) != (N, K) and c.mode == "both")
    _images(_row_block(M.inputs(other)["w"]))
    img2, imgT2 = _images(w, want_img, want_t)
    torch.cuda.synchronize()
    if want_img:
        p = _decode(img, N, K)
        assert torch.equal(p.sum(0)[:, :K], w) and float(p[:, :, K:].abs().max() if K % 32 else 0.0) == 0.0
        assert torch.equal(img, img2)
    if want_t:
        pt = _decode(imgT, K, N)
        assert torch.equal(pt.sum(0)[:, :N], w.t()) and float(pt[:, :, N:].abs().max() if N % 32 else 0.0) == 0.0
        assert torch.equal(imgT, imgT2)


def test_batched_image_build_equals_the_single_builds():
    """All five shapes as the jobs of ONE mlagg_weight_images launch: 40-byte rows {w, img, img_t, int32 N, K, w_stride, pad};
    max_tiles is the largest job's count (12), so every other job leaves workgroups idle."""
    lib, st = _lib()
    cases = [M.by_id(f"I-{N}x{K}-both") for N, K in M.IMG_SHAPES]
    ws = [_row_block(M.inputs(c)["w"]) for c in cases]
    single = [_images(w) for w in ws]
    bufs = [(torch.full_like(a, 0xFF), torch.full_like(b, 0xFF)) for a, b in single]
    rows = [[w.data_ptr(), a.data_ptr(), b.data_ptr(), c.N | (c.K << 32), w.stride(0)] for w, (a, b), c in zip(ws, bufs, cases)]
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    assert table.element_size() * table.shape[1] == 40
    tiles = [M.image_tiles(c.N, c.K) for c in cases]
    _check_rc(lib.mlagg_weight_images(table.data_ptr(), len(cases), max(tiles), st), "mlagg_weight_images")
    torch.cuda.synchronize()
    assert max(tiles) > min(tiles)
    for c, (a, b), (sa, sb) in zip(cases, bufs, single):
        assert torch.equal(a, sa) and torch.equal(b, sb), c.id


# ---------------------------------------------------------------------------------------------------------------------
# K5w
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.WGRAD_CASES, ids=_ids(M.WGRAD_CASES))
def test_linear_wgrad_paths_match_float64(case):
    job, got = _both_ways(case)
    O, I = case.N, case.K
    for q, o in job.outs.items():
        assert not bool(torch.isnan(o.view).any()), f"{case.id} {q}: a partial row of the workspace was read but never written"
        tail = o.wide[0, o.view.shape[1]:]
        assert torch.equal(tail, torch.full_like(tail, M.SENTINEL)), f"{case.id} {q}: written past the {'bias' if case.bias else 'weight'} gradient"
    quantities = _wgrad_quantities(case, got)
    assert {q.split("_x3")[0] for q in quantities} == set(M.compared(case) if case.bias else ["dW"])
    _compare(case, quantities)


# ---------------------------------------------------------------------------------------------------------------------
# the round-3 K5 (three modes) and the fp32 K5
# ---------------------------------------------------------------------------------------------------------------------
def _lp_test(case):
    job, got = _both_ways(case)
    job.outs["y"].check(f"{case.id} y")
    if M.runs_dgrad(case):
        job.outs["dx"].check(f"{case.id} dx")
    else:
        assert bool(torch.isnan(got.pop("dx")).all()), "a refused data gradient wrote its output"
    assert set(got) == set(M.compared(case))
    _compare(case, got)


@pytest.mark.parametrize("case", M.LP_CASES, ids=_ids(M.LP_CASES))
def test_linear_lp_paths_match_float64(case):
    _lp_test(case)


@pytest.mark.parametrize("case", M.FP32_CASES, ids=_ids(M.FP32_CASES))
def test_linear_fp32_paths_match_float64(case):
    _lp_test(case)


@pytest.mark.parametrize("shape", M.LP_REFUSED, ids=[f"k{s[2]}" for s in M.LP_REFUSED])
def test_round3_kernels_refuse_a_contraction_that_is_no_multiple_of_4(shape):
    lib, st = _lib()
    Mr, N, K = shape
    x, w, y = torch.randn(Mr, 32, device=DEV), torch.randn(N, 32, device=DEV), torch.full((Mr, N), NAN, device=DEV)
    args = (x.data_ptr(), 32, w.data_ptr(), None, y.data_ptr(), N, Mr, N, K)
    assert lib.mlagg_linear_fwd(*args, st) == -1
    for code in (1, 2, 3):
        assert lib.mlagg_linear_lp_fwd(*args, code, st) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()), "a refused call wrote its output"


# ---------------------------------------------------------------------------------------------------------------------
# through ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    """Every entry point ops launches, in order: [name]."""
    from mlagg_unet_amd import ops
    seen, real = [], ops._launch

    def record(name, *args):
        seen.append(name)
        return real(name, *args)

    monkeypatch.setattr(ops, "_launch", record)
    return seen


def _poison(floats):
    """Fill and free `floats` floats of device memory with NaN: the next allocation of that size is likely to be handed them."""
    junk = torch.full((max(int(floats), 1),), NAN, device=DEV)
    del junk


def _ops_run(case, monkeypatch):
    import contextlib
    from mlagg_unet_amd import ops
    lib, _ = _lib()
    t = M.inputs(case)
    Mr, O, I = case.M, case.N, case.K
    shape = (3, Mr // 3)
    if case.strided:
        wide = torch.full(shape + (I + 1,), M.SENTINEL)
        wide[..., 1:] = t["x"].view(*shape, I)
        x = wide.to(DEV).requires_grad_(True)[..., 1:]
        assert x.data_ptr() % 16 and ops._mfma_rows(x, "x")[0].data_ptr() != x.data_ptr()        # the copy branch
        dyw = torch.full(shape + (O + 8,), M.SENTINEL)
        dyw[..., 4:4 + O] = t["dy"].view(*shape, O)
        dy = dyw.to(DEV)[..., 4:4 + O]
        assert not dy.is_contiguous() and ops._mfma_rows(dy, "dy")[1] == O + 8                   # taken where it is
    else:
        x, dy = t["x"].view(*shape, I).to(DEV).requires_grad_(True), t["dy"].view(*shape, O).to(DEV)
    if case.mode == "mlp":
        monkeypatch.setattr(ops, "X3_MIN_ROWS", 1)
        monkeypatch.setattr(ops, "WGRAD_MIN_ROWS", 1)
        ps = [t[k].to(DEV).requires_grad_(True) for k in ("w", "b", "w2", "b2")]
        assert ops.mlp_supported(x, ps[0], ps[2])
        _poison(Mr * 2 * I)
        y = ops.mlp(x, *ps)
        _poison(lib.mlagg_linear_wgrad_workspace_floats(Mr, 2 * I, I))
        g = torch.autograd.grad(y, [x] + ps, dy)
        return dict(zip(("y", "dx", "dW1", "db1", "dW2", "db2"), (y.detach(),) + g))
    plan, precision = M.PLANS[case.mode]
    w = t["w"].to(DEV).requires_grad_(True)
    b = t["b"].to(DEV).requires_grad_(True) if case.bias else None
    with ops.compute_precision(precision) if precision else contextlib.nullcontext():
        _poison(Mr * O)
        y = ops.linear(x, w, b, plan=plan)
        _poison(lib.mlagg_linear_wgrad_workspace_floats(Mr, O, I))
        g = torch.autograd.grad(y, [x, w] + ([b] if case.bias else []), dy)
    return dict(zip(("y", "dx", "dW", "db"), (y.detach(),) + g))


@pytest.mark.parametrize("case", M.OPS_CASES, ids=_ids(M.OPS_CASES))
def test_ops_linear_and_mlp_on_planned_kernels_match_float64(case, launches, monkeypatch):
    first = _ops_run(case, monkeypatch)
    n = len(launches)
    other = M.by_id("O-k5" if case.id != "O-k5" else "O-x3")
    _ops_run(other, monkeypatch)
    del launches[n:]
    second = _ops_run(case, monkeypatch)
    torch.cuda.synchronize()
    for q in first:
        assert torch.equal(first[q], second[q]), f"{q}: the second run, after {other.id}, differs from the first"
    # the planned kernels ran
    if case.mode == "mlp":
        assert launches.count("mlagg_linear_x3") == 8 and launches.count("mlagg_linear_wgrad_x3") == 4, launches
    else:
        plan, precision = M.PLANS[case.mode]
        fwd = "mlagg_linear_x3" if plan[0] == "K5x3" else "mlagg_linear_lp_fwd"
        dgrad = None if plan[1] is None else (fwd if precision is None else "mlagg_linear_lp_dgrad")
        assert launches.count(fwd) == 2 * (1 + (dgrad == fwd)) and launches.count("mlagg_linear_wgrad_x3") == 2, launches
        assert dgrad in (None, fwd) or launches.count(dgrad) == 2, launches
    got = {q: v.reshape(-1, v.shape[-1]) if v.dim() == 3 else v for q, v in first.items()}
    if not M.runs_dgrad(case):
        assert bool(torch.isfinite(got.pop("dx")).all())                           # the library's: not compared
    assert set(got) == set(M.compared(case))
    _compare(case, got)


def test_ops_linear_raises_where_a_planned_kernel_cannot_serve_the_shape():
    """No quiet fallback: the data gradient of O = 33 planned onto K5x3 (contraction 33, no multiple of 8) raises."""
    from mlagg_unet_amd import ops
    case = M.by_id("O-x3-33")
    t = M.inputs(case)
    x, w = t["x"].to(DEV).requires_grad_(True), t["w"].to(DEV).requires_grad_(True)
    y = ops.linear(x, w, None, plan=M.PLANS["x3"][0])
    with pytest.raises(RuntimeError):
        torch.autograd.grad(y, (x, w), t["dy"].to(DEV))
    torch.cuda.synchronize()
