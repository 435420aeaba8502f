"""The cases of tests/_linear_kernel_cases.py are what they claim to be, checked without a GPU.

The path predicates agree with the library's host queries -- the launchers' own decisions (mlagg_linear_x3_tile,
mlagg_linear_x3_supported, mlagg_linear_wgrad_geometry, mlagg_linear_wgrad_workspace_floats, mlagg_weight_image_bytes) -- over the cases
and a sweep; the case tables reach every tile variant, every <TO, TI>, every slab / pipeline / reduction class and both sides of every
threshold (taking a boundary case out of a table fails here); every reference value is finite and the plain-fp32 yardstick stays
within HALF of the bounds the device test uses, i.e. the inputs are well conditioned and a failure on the device means the kernel;
simulated index errors, applied to the float64 evaluation, land at least ten times outside the bound of the case meant to catch them."""
import ctypes
import os

import pytest
import torch

from tests import _linear_kernel_cases as M


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    from mlagg_unet_amd import _lib
    return _lib.lib()


def _find(cid):
    return M.by_id(cid)


def _geometry(lib, m, o, i):
    out = (ctypes.c_int * 5)()
    rc = lib.mlagg_linear_wgrad_geometry(m, o, i, ctypes.addressof(out))
    return rc, list(out)


# ---------------------------------------------------------------------------------------------------------------------
# the tables describe the default dispatch
# ---------------------------------------------------------------------------------------------------------------------
def test_no_dispatch_override_is_set():
    on = [v for v in M.OVERRIDES if v in os.environ]
    assert not on, f"{on} set: the case tables of tests/_linear_kernel_cases.py describe the launchers' DEFAULT choices; unset to run them"


# ---------------------------------------------------------------------------------------------------------------------
# predicates against the library
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_M = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1151, 1152, 1153, 2048, 8191, 8192, 10240,
           13056, 13057, 65535, 65536, 65537, 70001, 98297, 130944, 130945, 131071, 131072, 131073, 163840, 327680]
SWEEP_W = list(range(1, 201)) + [960, 12288]


def test_x3_tile_and_support_match_the_launcher(lib):
    def same(m, n, k):
        ok = M.x3_supported(m, n, k)
        assert bool(lib.mlagg_linear_x3_supported(m, n, k)) == ok, (m, n, k)
        nw, tn = M.x3_tile(m, n)
        assert lib.mlagg_linear_x3_tile(m, n, k) == (nw * 10 + tn if ok else -1), (m, n, k)
    for c in M.X3_CASES:
        same(c.M, c.N, c.K)
        same(c.M, c.K, c.N)                                                        # the data gradient (refused where N % 8 != 0)
    for m, n, k in M.X3_REFUSED:
        assert not M.x3_supported(m, n, k)
        same(m, n, k)
    assert {m <= 1024 for m in SWEEP_M} == {m >= 130945 for m in SWEEP_M} == {True, False}
    for m in SWEEP_M:
        for n in SWEEP_W:
            same(m, n, 8)
    for k in (0, 4, 8, 12, 16, 36, 40, 1536):
        same(4096, 96, k)
    same(0, 8, 8), same(8, 0, 8), same(8, 1 << 26, 32)                              # the image of more than 2^32 elements


def test_weight_image_sizes_match_the_library(lib):
    for n in SWEEP_W:
        for k in (1, 8, 31, 32, 33, 40, 72, 96, 1536):
            assert lib.mlagg_weight_image_bytes(n, k) == M.image_bytes(n, k), (n, k)
    for c in M.IMG_CASES:
        assert M.image_tiles(c.N, c.K) * 32 * 32 * 6 >= M.image_bytes(c.N, c.K) > 0


def test_wgrad_geometry_and_workspace_match_the_launcher(lib):
    def same(m, o, i):
        g = M.wgrad_geometry(m, o, i)
        rc, out = _geometry(lib, m, o, i)
        assert rc == 0 and out == [g.to, g.ti, g.slab, g.nslabs, g.ogroups * 65536 + g.igroups], (m, o, i, out, g)
        assert lib.mlagg_linear_wgrad_workspace_floats(m, o, i) == g.nslabs * (o * i + o), (m, o, i)
        assert g.slab % 16 == 0 and g.slab >= 64 and (g.nslabs - 1) * g.slab + M.wgrad_last_slab(m, g.slab) == m
        assert 0 < M.wgrad_last_slab(m, g.slab) <= g.slab
    for c in M.WGRAD_CASES:
        same(c.M, c.N, c.K)
    for m in SWEEP_M:
        for o in SWEEP_W:
            same(m, o, 32)
            same(m, 97, o)
    for o in (1, 32, 33, 64, 65, 96, 97, 192, 193, 384):
        for i in (1, 32, 33, 64, 65, 96, 97, 192, 193, 384):
            same(163840, o, i)
    for bad in ((0, 8, 8), (8, 0, 8), (8, 8, 0)):
        assert _geometry(lib, *bad)[0] == -1 and lib.mlagg_linear_wgrad_workspace_floats(*bad) == 0
    assert lib.mlagg_linear_wgrad_geometry(8, 8, 8, None) == -2


def test_the_refusals_of_the_round3_kernels_are_what_the_cases_expect():
    for c in M.LP_CASES + M.FP32_CASES:
        assert M.lp_supported(c.M, c.N, c.K)
        assert M.runs_dgrad(c) == (c.N % 4 == 0)
    assert all(not M.lp_supported(*s) for s in M.LP_REFUSED)
    assert {M.runs_dgrad(c) for c in M.LP_CASES} == {M.runs_dgrad(c) for c in M.FP32_CASES} == {True, False}


# ---------------------------------------------------------------------------------------------------------------------
# coverage: what the tables must reach (each line names the boundary case that provides it)
# ---------------------------------------------------------------------------------------------------------------------
def _tile(cid):
    c = _find(cid)
    return M.x3_tile(c.M, c.N)


def _grid(cid):
    c = _find(cid)
    return M.x3_grid(c.M, c.N, M.x3_tile(c.M, c.N))


def test_x3_cases_cover_every_variant_and_both_sides_of_each_threshold():
    # M = 1024 / 1025: <2,2> / <4,2>, the latter's last workgroup with one row
    assert (_find("X-1024").M, _find("X-1025").M) == (1024, 1025) and _tile("X-1024") == (2, 2) and _tile("X-1025") == (4, 2)
    assert _grid("X-1025")[1] == 1 and _grid("X-1024")[1] == 64
    # tiny and ragged
    assert (_find("X-1x1").M, _find("X-1x1").N, _find("X-1x1").K) == (1, 1, 8)
    c = _find("X-63")
    assert _tile("X-63") == (2, 2) and c.N == 32 and _grid("X-63") == (1, 63, 32)                   # one live tile of the two: the break
    assert _grid("X-65") == (2, 1, 33) and _grid("X-129") == (6, 1, 1) and _grid("X-200") == (8, 8, 33)
    # the 1024-workgroup threshold of the 96-column tile at nw = 4: on, off, and reached by the rows alone
    c = _find("X-t3-on")
    assert -(-c.M // 128) * (c.N // 96) == 1030 and _tile("X-t3-on") == (4, 3)
    c = _find("X-t3-off")
    assert -(-c.M // 128) * (c.N // 96) == 1020 and _tile("X-t3-off") == (4, 2)
    c = _find("X-t3-rows")
    assert -(-c.M // 128) * (c.N // 96) == 1024 and _tile("X-t3-rows") == (4, 3) and _grid("X-t3-rows") == (1024, 1, 96)
    # ... and at nw = 2
    c = _find("X-w2-on")
    assert c.M == 1024 and -(-c.M // 128) * (c.N // 96) == 1024 and _tile("X-w2-on") == (2, 3)
    c = _find("X-w2-off")
    assert -(-c.M // 128) * (c.N // 96) == 896 and _tile("X-w2-off") == (2, 2)
    # every variant the default rule can reach, counting the data gradients that run
    tiles = {M.x3_tile(c.M, c.N) for c in M.X3_CASES} | {M.x3_tile(c.M, c.K) for c in M.X3_CASES if M.runs_dgrad(c)}
    assert tiles == {(2, 2), (4, 2), (2, 3), (4, 3)}
    # every k-tail class on <4,2> and on <4,3>: one partial chunk (no prefetch), whole chunks, whole + partial
    for v, tile in (("42", (4, 2)), ("43", (4, 3))):
        ks = {}
        for K in M.X3_KS:
            c = _find(f"X-{v}-k{K}") if (v, K) != ("43", 8) else _find("X-t3-on")
            assert M.x3_tile(c.M, c.N) == tile and c.K == K
            ks[K] = M.x3_chunks(K)
        assert ks == {8: (1, 8), 32: (1, 0), 40: (2, 8), 64: (2, 0), 72: (3, 8)}
    assert all(not M.x3_supported(*s) for s in M.X3_REFUSED) and {s[2] for s in M.X3_REFUSED} == {4, 12}
    # every epilogue (0 with and without bias, 1, 2) on every variant, strided, with a ragged last row block
    seen = set()
    for v, m, n, k in M.X3_EPILOGUE_SHAPES:
        tile = M.x3_tile(m, n)
        assert f"{tile[0]}{tile[1]}" == v and 0 < M.x3_grid(m, n, tile)[1] < 32 * tile[0]
        for name, mode, bias in M.X3_EPILOGUE_MODES:
            c = _find(f"X-{v}-{name}")
            assert (c.M, c.N, c.K, c.mode, c.bias, c.strided) == (m, n, k, mode, bias, True)
            seen.add((tile, mode, bias))
    assert seen == {(t, m, b) for t in ((2, 2), (4, 2), (2, 3), (4, 3)) for m, b in (("e0", True), ("e0", False), ("e1", True), ("e2", False))}
    lay = M.LAYOUT
    assert lay["x"][0] % 4 == 0 and lay["x"][1] % 4 == 0 and lay["y"] == lay["y_act"] and lay["pre"][1] != lay["y"][1]
    assert _find("X-wide").regime == "wide" and not M.runs_dgrad(_find("X-wide"))


def test_image_cases_cover_the_shapes_and_the_three_requests():
    assert {(c.N, c.K) for c in M.IMG_CASES} == {(1, 8), (33, 40), (70, 48), (96, 8), (97, 72)}
    for n, k in M.IMG_SHAPES:
        assert {c.mode for c in M.IMG_CASES if (c.N, c.K) == (n, k)} == {"img", "imgT", "both"}
    tiles = [M.image_tiles(n, k) for n, k in M.IMG_SHAPES]
    assert max(tiles) == 12 and min(tiles) == 1 and len(set(tiles)) >= 4                        # the batched build leaves workgroups idle


def _wg(cid):
    c = _find(cid)
    return M.wgrad_geometry(c.M, c.N, c.K)


def test_wgrad_cases_cover_every_tile_pair_and_the_slab_geometry():
    geo = {c.id: M.wgrad_geometry(c.M, c.N, c.K) for c in M.WGRAD_CASES}
    last = {c.id: M.wgrad_last_slab(c.M, geo[c.id].slab) for c in M.WGRAD_CASES}
    # all nine <TO, TI>, each at full width; the ragged widths; the clamp edges 96 k + 1 and 96 k + 2 on either side
    for o in (32, 64, 96):
        for i in (32, 64, 96):
            assert (geo[f"W-{o}x{i}"].to, geo[f"W-{o}x{i}"].ti) == (o // 32, i // 32)
    assert {(g.to, g.ti) for g in geo.values()} == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)}
    assert (geo["W-1x1"].to, geo["W-31x33"].ti, geo["W-33x31"].to, geo["W-65x95"].to, geo["W-65x95"].ti) == (1, 2, 2, 3, 3)
    for cid, og, ig in (("W-clamp-97x32", 2, 1), ("W-clamp-32x97", 1, 2), ("W-clamp-98x194", 2, 3), ("W-clamp-193x98", 3, 2)):
        c, g = _find(cid), geo[cid]
        assert (g.ogroups, g.igroups) == (og, ig) and {c.N % 96, c.K % 96} <= {1, 2, 32}
    assert {_find(cid).N % 96 for cid in geo if cid.startswith("W-clamp")} >= {1, 2} <= {_find(cid).K % 96 for cid in geo if cid.startswith("W-clamp")}
    # M around one slab: one slab, a second slab of one token, odd M
    ms = {c.M: c for c in M.WGRAD_CASES if c.id.startswith("W-m")}
    assert set(ms) == {1, 2, 15, 16, 17, 40, 63, 64, 65, 71, 127} and all((c.N, c.K) == (33, 65) for c in ms.values())
    assert geo["W-m64"].nslabs == 1 and geo["W-m65"].nslabs == 2 and last["W-m65"] == 1 and geo["W-m1"].slab == 64
    # nslabs against the reducer's strides of 16 and 64
    for n in M.WGRAD_NSLABS:
        assert geo[f"W-s{n}"].nslabs == n and geo[f"W-s{n}"].slab == 64 and last[f"W-s{n}"] == 57
    passes = {n: M.reduce_passes(n) for n in M.WGRAD_NSLABS}
    assert passes == {15: (0, 1, 15), 16: (0, 1, 16), 17: (0, 2, 1), 63: (1, 0, 0), 64: (1, 0, 0), 65: (1, 1, 1), 66: (1, 1, 2)}
    c = _find("W-s17-35x50")
    assert geo[c.id].nslabs == 17 and (c.N * c.K + c.N) % 64 != 0
    # slabs above the floor, the pipelines' remainder classes
    assert (geo["W-slab80"].slab, geo["W-slab80"].nslabs, last["W-slab80"]) == (80, 876, 1)
    assert (geo["W-slab96"].slab, geo["W-slab96"].nslabs, last["W-slab96"]) == (96, 1024, 89)
    assert M.wgrad_pipeline(80, "x3")[:2] == (5, 2) and M.wgrad_pipeline(96, "x3")[:2] == (6, 0) and M.wgrad_pipeline(64, "x3")[:2] == (4, 1)
    lengths = {min(g.slab, _find(cid).M) for cid, g in geo.items()} | set(last.values())
    assert {M.wgrad_pipeline(n, "x3")[1] for n in lengths if n >= 16} == {0, 1, 2}
    assert {M.wgrad_pipeline(n, "fp32")[1] for n in lengths if n >= 8} == {0, 1}
    assert {M.wgrad_pipeline(n, "x3")[0] for n in lengths} >= {0, 1, 2, 3, 4, 5, 6}
    assert {n % 16 for n in last.values()} >= {0, 1, 7, 8, 9, 15}
    assert {n % 2 for n in last.values()} == {0, 1}
    # db == NULL on two cases, strides on a few, the wide regime
    assert sorted(c.id for c in M.WGRAD_CASES if not c.bias) == ["W-clamp-97x32", "W-m65"]
    assert sum(c.strided for c in M.WGRAD_CASES) >= 4 and {geo[c.id].to for c in M.WGRAD_CASES if c.strided} >= {2, 3} <= {geo[c.id].ti for c in M.WGRAD_CASES if c.strided}
    assert _find("W-wide").regime == "wide"


def test_round3_cases_cover_the_grid_edges_in_every_mode():
    assert {t[0] for t in M.LP_TRIPLES} == {1, 127, 128, 129, 257}
    assert {t[1] for t in M.LP_TRIPLES} == {1, 32, 33, 95, 96, 97, 100}
    assert {t[2] for t in M.LP_TRIPLES} == {4, 28, 32, 36, 68}
    for t in M.LP_TRIPLES:
        assert {c.mode for c in M.LP_CASES if (c.M, c.N, c.K) == t and c.regime == "unit"} == set(M.LP_MODES)
        assert [c for c in M.FP32_CASES if (c.M, c.N, c.K) == t]
    grids = [M.lp_grid(*t) for t in M.LP_TRIPLES]
    assert {g[1] for g in grids} >= {1, 127, 128} and {g[2] for g in grids} >= {1, 32, 33, 95, 96, 4} and {g[4] for g in grids} >= {0, 4, 28}
    assert {g[0] for g in grids} >= {1, 2, 3, 6} and {g[3] for g in grids} == {1, 2, 3}
    # the data gradient (O = K, I = N): ragged second column group, k tail
    dg = [M.lp_grid(t[0], t[1], t[2]) for t in M.LP_TRIPLES if t[1] % 4 == 0]
    assert any(g[2] == 4 and g[0] > 1 for g in dg)
    assert all(c.strided for c in M.LP_CASES + M.FP32_CASES)
    assert _find("L-wide-bf16x3").regime == _find("P-wide").regime == "wide"


def test_ops_cases_cover_both_plans_the_modes_and_the_operand_branches():
    modes = [c.mode for c in M.OPS_CASES]
    assert 8 <= len(M.OPS_CASES) <= 10 and set(modes) == set(M.PLANS) | {"mlp"}
    assert M.PLANS["x3"][0] == ("K5x3", "K5x3", "K5w") and M.PLANS["k5"][0] == ("K5", "K5", "K5w")
    assert {M.PLANS[m][1] for m in modes if m != "mlp"} == {None, "bf16", "fp16"}
    assert any(c.strided and c.mode == "x3" for c in M.OPS_CASES) and any(c.strided and c.mode == "k5" for c in M.OPS_CASES)
    assert any(not c.bias for c in M.OPS_CASES) and all(c.M % 3 == 0 and c.M % 32 for c in M.OPS_CASES)
    for c in M.OPS_CASES:                                                          # a planned data gradient is one the kernel serves
        if c.mode != "mlp" and M.PLANS[c.mode][0][1] is not None:
            assert c.N % (8 if c.mode.startswith("x3") else 4) == 0, c.id
    assert any(c.N == 33 for c in M.OPS_CASES)


def test_case_ids_are_unique():
    ids = [c.id for c in M.ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert all(c.regime in ("unit", "wide") for c in M.ALL_CASES)


# ---------------------------------------------------------------------------------------------------------------------
# references and yardstick
# ---------------------------------------------------------------------------------------------------------------------
def _group(case):
    if case.family == "x3":
        return f"x3 {'epilogue ' + case.mode[1] if case.mode != 'e0' else 'epilogue 0'}"
    if case.family in ("lp", "ops"):
        return f"{case.family} {case.mode}"
    return case.family


_TABLE = {}


@pytest.mark.parametrize("case", M.NUMERIC_CASES, ids=[c.id for c in M.NUMERIC_CASES])
def test_reference_is_finite_and_the_plain_fp32_yardstick_is_within_half_the_bounds(case):
    ref, yard = M.reference(case), M.yardstick(case)
    tols = M.bounds(case)
    assert set(ref) == set(yard) and set(M.compared(case)) <= set(ref) and M.compared(case)
    for q in ref:
        assert ref[q].dtype == torch.float64 and yard[q].dtype == torch.float32
        assert bool(torch.isfinite(ref[q]).all()) and bool(torch.isfinite(yard[q]).all()), q
        if q not in M.compared(case):
            continue
        err = M.error(yard[q], ref[q], tols[q].kind)
        print(f"YARDSTICK {case.id} {q} {err:.2e} bound {tols[q].a:.1e} ({tols[q].kind})")
        key = (_group(case), q)
        _TABLE[key] = max(_TABLE.get(key, 0.0), err)
        assert err <= 0.5 * tols[q].a, (q, err, tols[q])


def test_print_the_yardstick_table_and_check_the_db_bound():
    """The table of the case file's docstring, and its db bound: 8 x the largest fp32 `sum(0)` error over the wgrad cases where that
    is below a tenth of the ceiling."""
    worst = 0.0
    for c in M.WGRAD_CASES:
        worst = max(worst, M.error(M.yardstick(c)["db"], M.reference(c)["db"], "db"))
    print(f"largest db yardstick error over the wgrad cases: {worst:.2e}")
    for (group, q), err in sorted(_TABLE.items()):
        print(f"    {group:<22} {q:<6} {err:.1e}")
    assert worst < 0.1 * M.DB_CEILING and M.DB_YARD > 0.0
    assert 0.25 * M.DB_YARD <= worst <= 0.5 * M.DB_BOUND, (worst, M.DB_YARD)       # the recorded figure is of the measured size
    assert M.DB_BOUND == 8 * M.DB_YARD <= M.DB_CEILING


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: simulated index errors land at least ten times outside the bound of the case meant to catch them
# ---------------------------------------------------------------------------------------------------------------------
DEFECTS = [
    ("last_rows", "y", ["X-1025", "X-65", "X-129", "X-t3-rows", "X-22-e0", "X-42-e1", "X-43-e2", "X-23-e0nb"]),
    ("k_tail", "y", ["X-42-k8", "X-42-k40", "X-42-k72", "X-43-k40", "X-43-k72", "X-t3-on", "X-42-k32", "X-42-k64"]),
    ("third_tile", "y", ["X-t3-on", "X-t3-rows", "X-w2-on", "X-43-e0", "X-23-e1", "X-43-k72"]),
    ("third_tile", "y_act", ["X-43-e1", "X-23-e1"]),
    ("pre_stride", "y", ["X-22-e2", "X-42-e2", "X-43-e2", "X-23-e2"]),
    ("last_slab", "dW", ["W-m65", "W-m71", "W-m127", "W-s15", "W-s17", "W-s65", "W-32x32", "W-slab96"]),
    ("last_slab", "db", ["W-m71", "W-m127", "W-s65"]),
    ("odd_token", "dW", ["W-m1", "W-m15", "W-m17", "W-m63", "W-m65", "W-m71", "W-m127", "W-s16"]),
    ("reduce64", "dW", ["W-s65", "W-s66", "W-slab80", "W-slab96"]),
    ("reduce64", "db", ["W-s65", "W-s66", "W-slab80", "W-slab96"]),
    ("clamp_prev", "dW", ["W-clamp-97x32", "W-clamp-32x97", "W-clamp-98x194", "W-clamp-193x98"]),
]


@pytest.mark.parametrize("defect,q,ids", DEFECTS, ids=[f"{d}-{q}" for d, q, _ in DEFECTS])
def test_simulated_defects_land_ten_times_outside_the_bound(defect, q, ids):
    for cid in ids:
        case = _find(cid)
        tol = M.bounds(case)[q]
        err = M.error(M.defective(case, defect)[q], M.reference(case)[q], tol.kind)
        print(f"DEFECT {defect} {cid} {q}: {err:.2e} against the bound {tol.a:.1e}")
        assert err >= 10 * tol.a, (defect, cid, q, err, tol)
