"""Cases, references and path predicates for the token-major projections -- K5 on weight images (csrc/linear_x3.hip), its image
builders, K5w (csrc/linear_wgrad.hip, both kernels), the round-3 K5 (csrc/linear_lp.hip, three modes) and the fp32 K5 (csrc/linear.hip)
-- at the sizes where their launchers change tile, slab or pipeline path: shared by tests/test_linear_kernel_paths_cpu.py and
tests/test_linear_kernel_paths_gpu.py.

A CASE is a LinCase (id, family, M, N, K, mode, bias, strided, regime).  `family`:
    x3     mlagg_linear_x3 on (M, N, K); mode "e0" / "e1" / "e2" = the epilogue.  Mode "e0" with a bias also runs the data gradient
           dx (M, K) = dy (M, N) . W on the image of W^T where N % 8 == 0.
    img    mlagg_weight_image of W (N, K); mode "img" / "imgT" / "both" = the images asked for.  Compared exactly (no bound).
    wgrad  mlagg_linear_wgrad AND mlagg_linear_wgrad_x3 on dy (M, O = N), x (M, I = K); bias False: db == NULL.
    lp     mlagg_linear_lp_fwd on (M, N, K) and mlagg_linear_lp_dgrad with O = K, I = N (refused where N % 4 != 0); mode "bf16" / "fp16"
           / "bf16x3" = the dtype.       fp32: the same through mlagg_linear_fwd / _dgrad.
    ops    ops.linear(x, w, b, plan=PLANS[mode][0]) under PLANS[mode][1], x of shape (3, M / 3, K); mode "mlp": ops.mlp with 2 K hidden.
`strided`: every operand and output is the column block of a tensor a few columns wider (LAYOUT: first column, extra columns) filled
with SENTINEL; for `wgrad` dy is the block [4, 4 + O) of a wider tensor and x has the odd row stride I + 1.  `regime` "unit": x rows
scaled by exp(randn); "wide": by 2^u, u uniform in [-40, 40] (far from the fp32 / bf16 denormals, which are not claimed).  Inputs come
from a generator seeded with zlib.crc32 of the case id: unit-variance x (before the row scales), dy and pre; weights scaled by
K ** -0.5.  The x3 cases with N = 96, 960 or 12288 are about the forward's tile; their data gradient contracts over those N, and
the fp32 sum of that many dense terms is, against the largest of a row's K = 8 .. 72 results and over up to 130945 rows, no longer
within half the bound on the host either (1.2e-6 .. 2.3e-6).  Where N > 72 their dy therefore keeps each element with probability
16 / N (zero otherwise): every row still runs through every k chunk of the image of W^T, all N columns are read, and a result sums
about 16 products.

`reference(case)` is the operation in float64 on the host -- of the operands rounded to the 16-bit type in the 16-bit modes (the exact
products of what the kernels multiply; they sum in fp32), the erf GELU and its derivative for epilogues 1 and 2.  `yardstick(case)`
is the same operation in plain fp32 on the host: it shows how well conditioned a case is, it is not the truth.  `bounds(case)` are the
project's bounds for these kernels, not measurements of them (Tol kind "row": max over rows of max |got - ref| / max |ref| of the row;
"max": max |got - ref| / max |ref|; "db": max |got - ref| / max(1, max |ref|)):
    x3 / bf16x3 / fp32 forward and data gradient   3e-6 row      (tests/test_linear_x3_gpu.py)
    dW                                             2e-6 max      (tests/test_blocks_gpu.py)
    epilogue 1 (y, y_act) / epilogue 2, mlp        1e-5 / 2e-5 max  (test_mlp_fused_matches_float64)
    bf16 / fp16                                    2e-5 max, against the rounded-operand product (tests/test_mixed_precision_gpu.py)
    db                                             DB_BOUND db   (below)

PATH PREDICATES are pure functions restating a launcher's decision; each names the source function it mirrors, and the CPU test
compares them with the library's host queries (mlagg_linear_x3_tile, mlagg_linear_x3_supported, mlagg_linear_wgrad_geometry,
mlagg_linear_wgrad_workspace_floats, mlagg_weight_image_bytes) over the cases and a sweep.  They describe the DEFAULT dispatch:
OVERRIDES lists the environment variables that change it.

Plain-fp32 yardstick errors of the compared quantities, largest over the group's cases, measured on the host with YARDSTICK_THREADS
threads (in each quantity's own metric):

    cases                     y        y_act    dx       dW       db
    x3 epilogue 0             5.6e-07           6.9e-07
    x3 epilogue 1             1.9e-07  1.9e-07
    x3 epilogue 2             1.5e-07
    wgrad                                                6.3e-07  3.7e-07
    lp bf16x3                 4.8e-07           4.9e-07
    lp bf16                   1.2e-07           1.4e-07
    lp fp16                   2.4e-07           3.0e-07
    fp32                      4.2e-07           5.0e-07
    ops x3 / x3-lib           4.8e-07           5.9e-07  6.5e-07  1.6e-07
    ops k5 / k5-lib           4.6e-07           3.7e-07  6.4e-07  1.3e-07
    ops k5-bf16 / k5-fp16     1.2e-07           2.4e-07  6.9e-07  1.3e-07
    ops mlp                   1.9e-07           4.1e-07  5.4e-07  2.2e-07      (dW, db: the larger of the two layers)

db: the ceiling is 1e-3 * max(1, max |ref|).  The largest yardstick error of db over all wgrad cases (fp32 `sum(0)`) is DB_YARD =
3.7e-7 in that metric (W-slab80), below a tenth of the ceiling, so the bound is DB_BOUND = 8 x that = 2.96e-6.
"""
import collections
import functools
import zlib

import torch

LinCase = collections.namedtuple("LinCase", "id family M N K mode bias strided regime")
Tol = collections.namedtuple("Tol", "kind a")
OVERRIDES = ("MLAGG_X3_TILE", "MLAGG_K5W_WAVES", "MLAGG_K5_X3", "MLAGG_X3_MIN_ROWS", "MLAGG_WGRAD_MIN_ROWS", "MLAGG_K5_MIN_ROWS",
             "MLAGG_LP_K5_MIN_ROWS")
SENTINEL = -12345.678
# a strided operand: columns [first, first + C) of a tensor `extra` columns wider.  x blocks start at a multiple of 4 floats and have a
# row stride that is one (the ABI of the MFMA kernels); y and y_act share one stride (the ABI), pre has another
LAYOUT = dict(x=(4, 8), y=(3, 5), y_act=(3, 5), pre=(2, 7), dy=(4, 8), dx=(3, 5))
DY_DENSE_MAX, DY_TERMS = 72, 16                     # the longest contraction with dense rows; products per row beyond it
LP_TYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
PLANS = {"x3": (("K5x3", "K5x3", "K5w"), None), "x3-lib": (("K5x3", None, "K5w"), None),
         "k5": (("K5", "K5", "K5w"), None), "k5-lib": (("K5", None, "K5w"), None),
         "k5-bf16": (("K5", "K5", "K5w"), "bf16"), "k5-fp16": (("K5", "K5", "K5w"), "fp16")}


# =====================================================================================================================
# path predicates
# =====================================================================================================================
# ---- K5 on weight images (csrc/linear_x3.hip) ---------------------------------------------------------------------------------
X3_NW2_MAX_ROWS, X3_TN3_MIN_GROUPS = 1024, 1024


def x3_supported(M, N, K):
    """mlagg_linear_x3_supported."""
    return M > 0 and N > 0 and K > 0 and K % 8 == 0 and 3 * N * (-(-K // 32) * 32) < 1 << 32


def x3_tile(M, N):
    """(nw, tn) of x3_tile(): workgroups of nw waves x 32 rows, tn column tiles of 32 per wave."""
    nw = 2 if M <= X3_NW2_MAX_ROWS else 4
    tn = 3 if N % 96 == 0 and -(-M // 128) * (N // 96) >= X3_TN3_MIN_GROUPS else 2
    return nw, tn


def x3_grid(M, N, tile):
    """(workgroups, rows of the last row block, live columns of the last column tile group): launch_x3."""
    nw, tn = tile
    bm, bn = 32 * nw, 32 * tn
    gx, gy = -(-M // bm), -(-N // bn)
    return gx * gy, M - (gx - 1) * bm, N - (gy - 1) * bn


def x3_chunks(K):
    """(Kp / 32, width of the k tail: K % 32, 0 = the last chunk is whole): linear_x3_kernel's chunk loop over the padded image rows."""
    return -(-K // 32), K % 32


def image_bytes(rows, cols):
    """mlagg_weight_image_bytes: three bf16 pieces, rows padded to a multiple of 32 columns."""
    return 3 * rows * (-(-cols // 32) * 32) * 2


def image_tiles(N, K):
    """32 x 32 tiles of one image job (weight_images_kernel)."""
    return -(-K // 32) * -(-N // 32)


# ---- K5w (csrc/linear_wgrad.hip make_geom, wave_tiles) ---------------------------------------------------------------------------
K5W_WAVES, K5W_MIN_SLAB = 1024, 64
WGeometry = collections.namedtuple("WGeometry", "to ti slab nslabs ogroups igroups")


def _ceil(a, b):
    return -(-a // b)


def wgrad_geometry(M, O, I):
    """make_geom + wave_tiles: 96-wide column groups, slabs of at least 64 tokens (a multiple of 16) so that slabs x groups reach 1024
    waves; (to, ti) 32-wide tiles per wave: 3 where a dimension has more than one group, else what it needs."""
    og, ig = -(-O // 96), -(-I // 96)
    slab = max(K5W_MIN_SLAB, _ceil(_ceil(M * og * ig, K5W_WAVES), 16) * 16)
    return WGeometry(3 if og > 1 else -(-O // 32), 3 if ig > 1 else -(-I // 32), slab, -(-M // slab), og, ig)


def wgrad_last_slab(M, slab):
    """Tokens of the last slab."""
    return M - (-(-M // slab) - 1) * slab


def wgrad_pipeline(tokens, kernel):
    """(nfull, remainder class, tail tokens) of a slab of `tokens` tokens: linear_wgrad_x3_kernel ("x3") takes whole blocks of 16 through
    three buffers (class: nfull % 3) and one clamped partial block; linear_wgrad_kernel ("fp32") blocks of 8 through two buffers (class:
    nfull % 2) and tail pairs."""
    step, bufs = (16, 3) if kernel == "x3" else (8, 2)
    return tokens // step, tokens // step % bufs, tokens % step


def reduce_passes(nslabs):
    """linear_wgrad_reduce_kernel, row group 0 of its 16 (the one with the most slabs): (passes of the loop unrolled over four row-group
    rounds [stride 64: while r + 48 < nslabs], single rounds after it [stride 16], row groups that still have a slab in the last single
    round [1 .. 16; 0: there is none])."""
    r, four = 0, 0
    while r + 48 < nslabs:
        r, four = r + 64, four + 1
    rest = max(0, nslabs - r)
    return four, -(-rest // 16), (rest - 1) % 16 + 1 if rest else 0


# ---- round-3 K5 and fp32 K5 (csrc/linear_lp.hip, csrc/linear.hip launch) -----------------------------------------------------------
def lp_grid(M, N, K):
    """(workgroups, rows of the last 128-row block, live columns of the last 96-column group, k chunks, width of the k tail)."""
    gx, gy = -(-M // 128), -(-N // 96)
    return gx * gy, M - (gx - 1) * 128, N - (gy - 1) * 96, -(-K // 32), K % 32


def lp_supported(M, N, K):
    """check() of both files, for contiguous operands."""
    return M > 0 and N > 0 and K > 0 and K % 4 == 0


def lp_dgrad_supported(M, O, I):
    return lp_supported(M, I, O) and I % 4 == 0


# =====================================================================================================================
# cases
# =====================================================================================================================
def _case(id, family, M, N, K, mode, bias=True, strided=False, regime="unit"):
    return LinCase(id, family, M, N, K, mode, bias, strided, regime)


X3_KS = (8, 32, 40, 64, 72)
X3_EPILOGUE_SHAPES = [("22", 200, 72, 40), ("42", 1100, 72, 40), ("43", 13060, 960, 8), ("23", 1000, 12288, 8)]
X3_EPILOGUE_MODES = [("e0", "e0", True), ("e0nb", "e0", False), ("e1", "e1", True), ("e2", "e2", False)]
X3_CASES = [
    _case("X-1024", "x3", 1024, 64, 32, "e0"),                          # <2,2>, the last row count of the 64-row workgroups
    _case("X-1025", "x3", 1025, 64, 32, "e0"),                          # <4,2>, the last workgroup has one row
    _case("X-1x1", "x3", 1, 1, 8, "e0"),
    _case("X-65", "x3", 65, 33, 40, "e0"),
    _case("X-63", "x3", 63, 32, 8, "e0"),                               # the second column tile is entirely past N (the `break`)
    _case("X-129", "x3", 129, 65, 72, "e0"),
    _case("X-200", "x3", 200, 97, 64, "e0"),
    _case("X-t3-on", "x3", 13057, 960, 8, "e0"),                        # 103 row blocks x 10 = 1030 workgroups: <4,3>
    _case("X-t3-off", "x3", 13056, 960, 8, "e0"),                       # 102 x 10 = 1020: <4,2>
    _case("X-t3-rows", "x3", 130945, 96, 8, "e0"),                      # 1024 row blocks, the last with one row: <4,3>
    _case("X-w2-on", "x3", 1024, 12288, 8, "e0"),                       # 8 x 128 = 1024: <2,3>
    _case("X-w2-off", "x3", 896, 12288, 8, "e0"),                       # 7 x 128 = 896: <2,2>
] + [_case(f"X-42-k{K}", "x3", 1100, 40, K, "e0") for K in X3_KS] + [_case(f"X-43-k{K}", "x3", 13057, 960, K, "e0") for K in X3_KS if K != 8] + [
    _case(f"X-{v}-{n}", "x3", M, N, K, mode, bias, True) for v, M, N, K in X3_EPILOGUE_SHAPES for n, mode, bias in X3_EPILOGUE_MODES]
X3_REFUSED = [(64, 64, 4), (64, 64, 12)]                                # K % 8 != 0: the error, no launch

IMG_SHAPES = [(1, 8), (33, 40), (70, 48), (96, 8), (97, 72)]
IMG_CASES = [_case(f"I-{N}x{K}-{mode}", "img", 0, N, K, mode, False, True) for N, K in IMG_SHAPES for mode in ("img", "imgT", "both")]

WGRAD_WIDTHS = [(o, i) for o in (32, 64, 96) for i in (32, 64, 96)] + [(1, 1), (31, 33), (33, 31), (65, 95)]
WGRAD_CLAMP = [(97, 32), (32, 97), (98, 194), (193, 98)]
WGRAD_MS = (1, 2, 15, 16, 17, 40, 63, 64, 65, 71, 127)
WGRAD_NSLABS = (15, 16, 17, 63, 64, 65, 66)
WGRAD_CASES = (
    [_case(f"W-{o}x{i}", "wgrad", 200, o, i, "both", True, (o, i) in ((31, 33), (65, 95))) for o, i in WGRAD_WIDTHS]
    + [_case(f"W-clamp-{o}x{i}", "wgrad", 200, o, i, "both", (o, i) != (97, 32), o > 97) for o, i in WGRAD_CLAMP]
    + [_case(f"W-m{m}", "wgrad", m, 33, 65, "both", m != 65, m == 17) for m in WGRAD_MS]
    + [_case(f"W-s{n}", "wgrad", 64 * n - 7, 32, 32, "both") for n in WGRAD_NSLABS]
    + [_case("W-s17-35x50", "wgrad", 64 * 17 - 7, 35, 50, "both"),           # n = O I + O = 1785, no multiple of the reducer's 64 columns
       _case("W-slab80", "wgrad", 70001, 32, 32, "both"),                      # slab 80 (5 blocks), 876 slabs, the last of one token
       _case("W-slab96", "wgrad", 98297, 32, 32, "both"),                      # slab 96 (6 blocks), 1024 slabs, the last of 89 tokens
       _case("W-wide", "wgrad", 127, 33, 65, "both", True, False, "wide")])

LP_TRIPLES = [(1, 1, 4), (127, 32, 28), (128, 33, 32), (129, 95, 36), (257, 96, 68), (1, 97, 32), (127, 100, 68), (128, 96, 4),
              (129, 33, 28), (257, 32, 36), (257, 100, 32), (128, 95, 68)]
LP_MODES = ("bf16", "fp16", "bf16x3")
LP_CASES = [_case(f"L-{M}x{N}x{K}-{mode}", "lp", M, N, K, mode, True, True) for M, N, K in LP_TRIPLES for mode in LP_MODES] + [
    _case("L-wide-bf16x3", "lp", 129, 95, 36, "bf16x3", False, True, "wide")]
FP32_CASES = [_case(f"P-{M}x{N}x{K}", "fp32", M, N, K, "fp32", True, True) for M, N, K in LP_TRIPLES] + [
    _case("P-wide", "fp32", 129, 95, 36, "fp32", False, True, "wide")]
LP_REFUSED = [(64, 32, 6), (64, 32, 30)]                                # K % 4 != 0

# ops: M tokens = 3 x (M / 3); `strided`: x is a column slice whose pointer is not 16-byte aligned AND dy is a column block of a wider
# gradient (the copy branch and the strided branch of ops._mfma_rows)
OPS_CASES = [
    _case("O-x3", "ops", 201, 64, 40, "x3"),
    _case("O-x3-33", "ops", 201, 33, 40, "x3-lib"),                      # O % 8 != 0: the data gradient is the library's
    _case("O-x3-slices", "ops", 201, 64, 40, "x3", True, True),
    _case("O-x3-nobias", "ops", 201, 96, 72, "x3", False, True),
    _case("O-k5", "ops", 201, 36, 40, "k5"),
    _case("O-k5-33", "ops", 201, 33, 40, "k5-lib"),
    _case("O-k5-slices", "ops", 201, 36, 40, "k5", True, True),
    _case("O-k5-bf16", "ops", 201, 36, 40, "k5-bf16"),
    _case("O-k5-fp16", "ops", 201, 36, 40, "k5-fp16", False),
    _case("O-mlp", "ops", 225, 40, 40, "mlp"),
]
X3_WIDE = _case("X-wide", "x3", 200, 97, 64, "e0", False, True, "wide")
X3_CASES.append(X3_WIDE)

CASES = {"x3": X3_CASES, "img": IMG_CASES, "wgrad": WGRAD_CASES, "lp": LP_CASES, "fp32": FP32_CASES, "ops": OPS_CASES}
ALL_CASES = [c for f in CASES.values() for c in f]
NUMERIC_CASES = [c for c in ALL_CASES if c.family != "img"]


def by_id(cid):
    return next(c for c in ALL_CASES if c.id == cid)


def runs_dgrad(case):
    """Does the case run a data gradient on the kernel under test?"""
    if case.family == "x3":
        return case.mode == "e0" and case.bias and case.regime == "unit" and case.N % 8 == 0
    if case.family in ("lp", "fp32"):
        return lp_dgrad_supported(case.M, case.K, case.N)
    if case.family == "ops":
        return case.mode == "mlp" or PLANS[case.mode][0][1] is not None
    return False


# =====================================================================================================================
# inputs, reference, yardstick
# =====================================================================================================================
def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case.id.encode()))


def inputs(case):
    """float32 host tensors of a case (contiguous; the device test lays the strided ones out)."""
    g = _gen(case)
    M, N, K = case.M, case.N, case.K
    rn = lambda *s: torch.randn(*s, generator=g)                                             # noqa: E731
    if case.family == "img":
        return dict(w=rn(N, K) * torch.exp(2 * rn(N, 1)))
    scale = torch.exp(rn(M, 1)) if case.regime == "unit" else torch.exp2(80 * torch.rand(M, 1, generator=g) - 40)
    t = dict(x=rn(M, K) * scale)
    if case.family == "wgrad":
        t["dy"] = rn(M, N)
        return t
    t["w"] = rn(N, K) * K ** -0.5
    if case.bias:
        t["b"] = rn(N)
    if case.family == "x3":
        if case.mode == "e2":
            t["pre"] = rn(M, N)
        if runs_dgrad(case):
            t["dy"] = rn(M, N)
            if N > DY_DENSE_MAX:                                                            # see the module docstring
                t["dy"] = t["dy"] * (torch.rand(M, N, generator=g) < DY_TERMS / N)
    elif case.family in ("lp", "fp32"):
        t["wd"] = rn(K, N) * K ** -0.5                                                      # data gradient: dy (M, O = K) . wd (O, I = N)
        t["dy"] = rn(M, K)
    elif case.mode == "mlp":
        t.update(w=rn(2 * K, K) * K ** -0.5, b=rn(2 * K) * 0.1, w2=rn(N, 2 * K) * (2 * K) ** -0.5, b2=rn(N) * 0.1, dy=rn(M, N))
    else:
        t["dy"] = rn(M, N)
    return t


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))


def gelu_grad(v):
    return 0.5 * (1.0 + torch.erf(v * 0.7071067811865476)) + v * torch.exp(-0.5 * v * v) * 0.3989422804014327


def _rounding(case):
    """The 16-bit type the case's forward and data-gradient operands are rounded to, or None."""
    if case.family == "lp":
        return LP_TYPE.get(case.mode)
    if case.family == "ops" and case.mode != "mlp":
        return LP_TYPE.get(PLANS[case.mode][1])
    return None


def evaluate(case, dtype, t=None):
    """{quantity: tensor} of a case in `dtype` on the host, from the operands as the mode holds them."""
    t = inputs(case) if t is None else t
    rt = _rounding(case)
    c = lambda v: v.to(dtype)                                                               # noqa: E731
    r = (lambda v: v.to(rt).to(dtype)) if rt is not None else c                              # noqa: E731
    out = {}
    if case.family == "wgrad":
        out["dW"] = c(t["dy"]).t() @ c(t["x"])
        out["db"] = c(t["dy"]).sum(0)
        return out
    if case.family == "ops" and case.mode == "mlp":
        x, w1, b1, w2, b2, dy = (c(t[k]) for k in ("x", "w", "b", "w2", "b2", "dy"))
        pre = x @ w1.t() + b1
        act = gelu(pre)
        out["y"] = act @ w2.t() + b2
        dpre = (dy @ w2) * gelu_grad(pre)
        out.update(dx=dpre @ w1, dW1=dpre.t() @ x, db1=dpre.sum(0), dW2=dy.t() @ act, db2=dy.sum(0))
        return out
    acc = r(t["x"]) @ r(t["w"]).t()
    y = acc + c(t["b"]) if case.bias else acc
    if case.family == "x3" and case.mode == "e2":
        out["y"] = acc * gelu_grad(c(t["pre"]))
        return out
    out["y"] = y
    if case.family == "x3" and case.mode == "e1":
        out["y_act"] = gelu(y)
    if case.family in ("lp", "fp32"):
        out["dx"] = r(t["dy"]) @ r(t["wd"])                                                  # compared where runs_dgrad
    elif "dy" in t:
        out["dx"] = r(t["dy"]) @ r(t["w"])
    if case.family == "ops":
        out["dW"] = c(t["dy"]).t() @ c(t["x"])                                               # weight gradients stay fp32 in every mode
        if case.bias:
            out["db"] = c(t["dy"]).sum(0)
    return out


@functools.lru_cache(maxsize=4)
def reference(case):
    """The float64 reference of a case; computed once, never modified."""
    return evaluate(case, torch.float64)


YARDSTICK_THREADS = 16


def yardstick(case):
    """The plain-fp32 yardstick of a case, with YARDSTICK_THREADS threads to be the same number on every machine."""
    before = torch.get_num_threads()
    torch.set_num_threads(YARDSTICK_THREADS)
    try:
        return evaluate(case, torch.float32)
    finally:
        torch.set_num_threads(before)


DB_CEILING = 1e-3
DB_YARD = 3.7e-7
DB_BOUND = 8 * DB_YARD


def compared(case):
    """The quantities the device test compares with the reference at the bounds below."""
    q = list(bounds(case))
    if not runs_dgrad(case):
        q = [n for n in q if n != "dx"]
    return q


def bounds(case):
    """{quantity: Tol} -- see the module docstring for where each comes from."""
    if case.family == "wgrad":
        return dict(dW=Tol("max", 2e-6), db=Tol("db", DB_BOUND))
    if case.family == "ops" and case.mode == "mlp":
        return dict(y=Tol("max", 1e-5), dx=Tol("max", 2e-5), dW1=Tol("max", 2e-5), db1=Tol("max", 2e-5), dW2=Tol("max", 2e-5),
                    db2=Tol("max", 2e-5))
    if case.family == "x3" and case.mode == "e1":
        return dict(y=Tol("max", 1e-5), y_act=Tol("max", 1e-5))
    if case.family == "x3" and case.mode == "e2":
        return dict(y=Tol("max", 2e-5))
    tol = Tol("max", 2e-5) if _rounding(case) is not None else Tol("row", 3e-6)
    out = dict(y=tol, dx=tol)
    if case.family == "ops":
        out["dW"] = Tol("max", 2e-6)
        if case.bias:
            out["db"] = Tol("db", DB_BOUND)
    return out


def error(got, ref, kind):
    """The error of `got` against `ref` in the metric `kind` (a NaN in `got` gives NaN, which no bound admits)."""
    d = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
    if kind == "row":
        return float((d.amax(dim=-1) / ref.abs().amax(dim=-1).clamp_min(1e-300)).max())
    if kind == "db":
        return float(d.max() / max(1.0, float(ref.abs().max())))
    return float(d.max() / ref.abs().max())


# =====================================================================================================================
# simulated defects (applied to the float64 evaluation; tests/test_linear_kernel_paths_cpu.py shows each lands far outside the bound)
# =====================================================================================================================
def defective(case, defect):
    """{quantity: float64 tensor} of the case as a kernel with the named index error would compute it."""
    t = {k: v.double() for k, v in inputs(case).items()}
    ref = {k: v.clone() for k, v in reference(case).items()}
    M, N, K = case.M, case.N, case.K
    if case.family == "x3":
        tile = x3_tile(M, N)
        if defect == "last_rows":                      # the rows of the last ragged row block dropped
            ref["y"][M - x3_grid(M, N, tile)[1]:] = 0.0
        elif defect == "k_tail":                       # the k tail chunk dropped
            keep = K - (K % 32 or 32)
            cut = dict(t, x=t["x"][:, :keep], w=t["w"][:, :keep])
            ref["y"] = cut["x"] @ cut["w"].t() + (t["b"] if case.bias else 0.0)
        elif defect == "third_tile":                   # the third column tile dropped
            assert tile[1] == 3
            cols = torch.arange(N) % 96 >= 64
            for q in ("y", "y_act"):
                if q in ref:
                    ref[q][:, cols] = 0.0
        elif defect == "pre_stride":                   # `pre` read with y_stride instead of pre_stride
            assert case.mode == "e2" and case.strided
            first, extra = LAYOUT["pre"]
            wide = torch.full((M, N + extra), SENTINEL, dtype=torch.float64)
            wide[:, first:first + N] = t["pre"]
            ys = N + LAYOUT["y"][1]
            flat = torch.cat([wide.reshape(-1)[first:], torch.full((M * ys,), SENTINEL, dtype=torch.float64)])
            pre = flat[:M * ys].reshape(M, ys)[:, :N]
            ref["y"] = (t["x"] @ t["w"].t()) * gelu_grad(pre)
        else:
            raise KeyError(defect)
        return ref
    assert case.family == "wgrad"
    g = wgrad_geometry(M, N, K)
    keep = torch.ones(M, dtype=torch.bool)
    if defect == "last_slab":                          # the last slab dropped
        keep[(g.nslabs - 1) * g.slab:] = False
    elif defect == "odd_token":                        # the odd last token of a slab dropped
        assert M % 2 == 1
        keep[M - 1] = False
    elif defect == "reduce64":                         # slabs >= 64 dropped from the reduction
        keep[64 * g.slab:] = False
    elif defect == "clamp_prev":                       # the clamped lanes' columns written to the previous group's
        dW = ref["dW"]
        for dim, size, tiles in ((0, N, g.to), (1, K, g.ti)):
            live = size % 96
            if size > 96 and 0 < live < tiles:
                src = dW.narrow(dim, size - live, live).clone()
                dW.narrow(dim, size - tiles, live).copy_(src)
                dW.narrow(dim, size - live, live).zero_()
        return ref
    else:
        raise KeyError(defect)
    ref["dW"] = t["dy"][keep].t() @ t["x"][keep]
    ref["db"] = t["dy"][keep].sum(0)
    return ref
