"""The cases of tests/_map_kernel_cases.py are what they claim to be, checked without a GPU.

The path predicates agree with the library's host queries (workspace sizes, supported widths); the case tables reach every path a
predicate can return and both sides of every threshold (taking a boundary case out of a table fails here); every reference value is finite; the plain-fp32 yardstick meets the bounds the device test uses, i.e. the inputs are well
conditioned and a failure on the device means the kernel; the LeakyReLU exclusion stays under its cap, and what it leaves in
cannot fail through a slope that flips."""
import pytest
import torch

from tests import _map_kernel_cases as M


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    from mlagg_unet_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------
# predicates against the library
# ---------------------------------------------------------------------------------------------------------------------
def test_k10_predicates_match_the_workspace_queries(lib):
    sizes = {M.k10_hw(c) for c in M.K10_CASES} | {4 * n for n in range(65530, 65545)} | {262143, 262145, 16 * 16384 + 4 * 4096, 2457600}
    for HW in sorted(sizes):
        S = M.k10_segments(HW)
        assert lib.mlagg_plane_norm_fwd_workspace_floats(M.K10_B, M.K10_C, HW) == M.K10_B * M.K10_C * S * 3, HW
        assert lib.mlagg_plane_norm_bwd_workspace_floats(M.K10_B, M.K10_C, HW) == M.K10_B * M.K10_C * (2 + 2 * S), HW
        assert (M.k10_fwd_path(HW) == "segmented") == (S > 0) == (M.k10_bwd_path(HW) == "segmented")
    assert M.k10_segments(262144) == 16 and M.k10_segments(262148) == 17 and M.k10_segments(262140) == 0


def test_k6_predicates_match_the_library(lib):
    for C in range(1, 1025):
        assert bool(lib.mlagg_layernorm_supported(C)) == (C in M.K6_ROW_SHAPES), C
    assert len(M.K6_ROW_SHAPES) == 12 and all(4 * lpr * f4 == C for C, (lpr, f4) in M.K6_ROW_SHAPES.items())
    for C in M.K6_ROW_SHAPES:
        rows_seen = {c.rows for c in M.K6_CASES if c.C == C} | {1023 * M.k6_rpb(C) + 1, 1024 * M.k6_rpb(C), 1024 * M.k6_rpb(C) + 1, 163840}
        for rows in sorted(rows_seen):
            assert lib.mlagg_layernorm_bwd_workspace_floats(rows, C) == M.k6_grid(rows, C) * 2 * C, (rows, C)
            trips = M.k6_trips(rows, C)
            assert len(trips) == M.k6_grid(rows, C) and min(trips) >= 1            # every launched workgroup has a row
            assert sum(min(M.k6_rpb(C), max(0, rows - (wg + k * len(trips)) * M.k6_rpb(C))) for wg, n in enumerate(trips) for k in range(n)) == rows
    # the capped grid of the issue: the looping cases fill it
    for C in M.K6_LOOP_WIDTHS:
        assert lib.mlagg_layernorm_bwd_workspace_floats(M.k6_loop_rows(C), C) == 1024 * 2 * C


def test_k2_predicates_match_the_workspace_query(lib):
    for c in M.K2_CASES:
        rows = M.k2_partial_rows(c.B, c.H)
        assert lib.mlagg_dwconv3x3_bwd_workspace_floats(c.B, c.H, c.W, c.C) == rows * c.C * 10 + c.B * c.H * c.W * c.C
        shapes = M.k2_wgrad_wave_shapes(c.W)
        assert sum(4 * g + t for g, t in shapes) == c.W and sum(M.k2_wgrad_channel_blocks(c.C)) == c.C


def test_k2n_predicates_match_the_workspace_query(lib):
    for c in M.K2N_CASES:
        slices = M.k2n_wgrad_slices(c.H, c.W, c.stride)
        assert lib.mlagg_dwconv3x3_nchw_bwd_workspace_floats(c.B, c.C, c.H, c.W, c.stride) == c.B * len(slices) * c.C * 10
        Ho, Wo = M.k2n_out(c.H, c.W, c.stride)
        assert sum(slices) == (c.H * c.W // 4 if M.k2n_path(c.W, c.stride) == "s1_strip" else Ho * Wo)


def test_k2v_predicates_match_the_workspace_query(lib):
    for c in M.K2V_CASES:
        D, H, W = c.dims
        L = D * H * W
        (_, _), (chunks, last) = M.k2v_blocks(L)
        assert lib.mlagg_dwconv3d_bwd_workspace_floats(c.B, D, H, W, c.C) == c.B * chunks * c.C * 28 + c.B * L * c.C
        assert (chunks - 1) * M.K2V_WTOK + last == L and 1 <= last <= M.K2V_WTOK


# ---------------------------------------------------------------------------------------------------------------------
# coverage: what the tables must reach (each line names the boundary case that provides it)
# ---------------------------------------------------------------------------------------------------------------------
def test_k10_cases_cover_every_path_and_threshold():
    fp32 = [c for c in M.K10_CASES if c.dtype == "fp32" and not c.offset and not c.res and not c.dy_slice]
    want = {16380: "reg256", 16384: "reg256", 16388: "reg1024", 65536: "reg1024", 65540: "stream_vec", 65539: "stream_scalar",
            262140: "stream_vec", 262144: "segmented", 262148: "segmented"}
    for HW, path in want.items():                                                 # the threshold and one float4 either side of it
        assert M.k10_fwd_path(HW) == path
        for act in ("none", "silu"):
            assert any(M.k10_hw(c) == HW and c.act == act and c.affine for c in fp32), (HW, act)
    assert {M.k10_hw(c) for c in fp32 if c.act == "none"} >= {1, 2, 3, 4, 8}
    assert (256, 256) in [c.dims for c in fp32]                                   # the maps of the headline configuration
    fwd_paths = {"reg256", "reg1024", "stream_vec", "stream_scalar", "segmented"}
    bwd_paths = {"stream_vec", "stream_scalar", "segmented"}
    for name, sel in (("leaky", lambda c: c.act == "leaky" and not c.affine), ("residual", lambda c: c.res and c.dtype == "fp32" and not c.offset)):
        assert {M.k10_fwd_path(M.k10_hw(c)) for c in M.K10_CASES if sel(c)} == fwd_paths, name
        assert {M.k10_bwd_path(M.k10_hw(c)) for c in M.K10_CASES if sel(c)} == bwd_paths, name
    assert {M.k10_hw(c) for c in M.K10_CASES if c.dy_slice} == {65536, 262144}
    assert {M.k10_hw(c) for c in M.K10_CASES if c.offset} == {65536, 262140}
    assert {(M.k10_hw(c), c.dtype) for c in M.K10_CASES if c.dtype != "fp32"} == {(hw, dt) for hw in (65536, 262144) for dt in ("bf16", "fp16")}
    # a ragged last segment: one float4 in the 17th
    assert any(M.k10_hw(c) % M.K10_SEG == 4 for c in M.K10_CASES)


def test_k6_cases_cover_every_width_and_the_looping_grid():
    for C in M.K6_ROW_SHAPES:
        rpb = M.k6_rpb(C)
        assert {c.rows for c in M.K6_CASES if c.C == C and c.form == "plain"} >= {1, rpb - 1, rpb, rpb + 1} - {0}, C
    for C in M.K6_LOOP_WIDTHS:
        looping = [c for c in M.K6_CASES if c.C == C and c.form == "plain" and c.rows == 1024 * M.k6_rpb(C) + M.k6_rpb(C) + 1]
        assert looping, C
        trips = M.k6_trips(looping[0].rows, C)
        assert len(trips) == 1024 and set(trips) == {1, 2} and trips[:2] == [2, 2] and trips[2] == 1          # the last row alone in workgroup 1
    assert {M.K6_ROW_SHAPES[C][0] for C in M.K6_LOOP_WIDTHS} == {64, 32, 16, 8, 4}                      # every lane-group size loops
    assert any(c.strided_x and c.strided_dy and max(M.k6_trips(c.rows, c.C)) >= 2 for c in M.K6_CASES)
    res = [c for c in M.K6_CASES if c.form == "res"]
    assert {c.use_sum for c in res} == {True, False}
    for c in res:
        assert c.rows % 3 == 0 and c.rows > 1024 * M.k6_rpb(c.C) and set(M.k6_trips(c.rows, c.C)) == {1, 2}
        assert (c.rows // 3) % M.k6_rpb(c.C) != 0 and 0.0 in M.K6_RES_SCALE        # a sample boundary inside a workgroup's rows


def test_k2_cases_cover_the_wave_shapes_blocks_and_reduce_rows():
    plain = [c for c in M.K2_CASES if c.form == "plain" and not c.pad]
    shapes = {c.W: [M.k2_wave_kind(s) for s in M.k2_wgrad_wave_shapes(c.W)] for c in plain}
    assert shapes[20] == ["groups+tail"] * 4                                      # a group followed by a tail
    assert shapes[30] == ["groups"] * 3 + ["groups+tail"] and M.k2_wgrad_wave_shapes(30)[3] < M.k2_wgrad_wave_shapes(30)[0]
    assert shapes[17] == ["groups+tail"] * 3 + ["tail"]
    assert shapes[2] == ["tail", "tail", "empty", "empty"] and shapes[3] == ["tail"] * 3 + ["empty"]
    assert shapes[5] == ["tail"] * 3 + ["empty"] and M.k2_wgrad_wave_shapes(5) == [(0, 2), (0, 2), (0, 1), (0, 0)]
    assert shapes[16] == ["groups"] * 4 and shapes[33] == ["groups+tail"] * 4
    assert {k for v in shapes.values() for k in v} == {"empty", "tail", "groups", "groups+tail"}
    # channel blocks: one quad in a second 32-block (36) and in a second 64-block (68); whole blocks (32, 64)
    assert {36, 68, 100, 32, 64, 4} <= {c.C for c in plain}
    assert M.k2_wgrad_channel_blocks(68) == [64, 4] and M.k2_tile_grid(1, 1, 36)[0][2] == 2
    # tiles: exactly one, and one row and one column past one
    assert any(M.k2_tile_grid(c.H, c.W, c.C) == ((1, 1, 1), (False, False, False)) for c in plain)
    assert any(c.H % M.K2_TY == 1 and c.W % M.K2_TX == 1 and c.H > M.K2_TY and c.W > 2 * M.K2_TX for c in plain)
    rows = {M.k2_partial_rows(c.B, c.H) for c in plain}
    assert rows >= {16, 17, 33, 48, 51}
    assert set().union(*(M.k2_reduce_shapes(r) for r in rows)) == {(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)}
    # every geometry plain and with SiLU; residual and both gated forms on the first six; one strided input
    geoms = {(c.B, c.H, c.W, c.C) for c in plain}
    assert len(geoms) == 12 and geoms == {(c.B, c.H, c.W, c.C) for c in M.K2_CASES if c.form == "silu" and not c.pad}
    for form in ("res", "gated", "packed"):
        assert {(c.B, c.H, c.W, c.C) for c in M.K2_CASES if c.form == form} >= {g for g, _ in M.K2_GEOMETRIES[:6]}
    assert any(c.pad == 8 for c in M.K2_CASES)


def test_k2n_cases_cover_the_paths_and_slices():
    plain = [c for c in M.K2N_CASES if c.form == "plain"]
    for path in ("s1_strip", "s1_generic", "s2"):
        mine = [c for c in plain if M.k2n_path(c.W, c.stride) == path]
        ns = [M.k2n_wgrad_slices(c.H, c.W, c.stride) for c in mine]
        assert any(len(s) == 1 for s in ns), path
        assert any(len(s) == 2 and s[1] == s[0] - 1 for s in ns), path            # a ragged last slice
        blocks = [M.k2n_data_blocks(c.H, c.W, c.stride) for c in mine]
        assert any(f == 1 for f, _ in blocks) and any(f > 1 for f, _ in blocks), path
    assert any(c.W == 4 and c.stride == 1 for c in plain)                         # one strip per row: both neighbours outside
    assert any(c.H == 1 and M.k2n_path(c.W, c.stride) == "s1_strip" for c in plain)
    assert any(c.H * (c.W // 4) > 256 and M.k2n_path(c.W, c.stride) == "s1_strip" for c in plain)
    s2 = {(c.H % 2, c.W % 2) for c in plain if c.stride == 2}
    assert s2 == {(0, 0), (1, 0), (0, 1), (1, 1)}                                 # even / odd extents: the last tap row / column in or out
    res = [c for c in M.K2N_CASES if c.form == "res"]
    assert {(c.C, c.H, c.W) for c in res} >= {(6, 5, 4), (4, 40, 28)} and all(M.k2n_path(c.W, c.stride) == "s1_strip" for c in res)
    assert any(len(M.k2n_wgrad_slices(c.H, c.W, 1)) == 2 for c in res)


def test_k2v_cases_sit_on_the_workgroup_edges():
    Ls = {c.dims[0] * c.dims[1] * c.dims[2] for c in M.K2V_CASES}
    assert Ls == {63, 64, 65, 255, 256, 257, 513}
    assert {M.k2v_edge(L, M.K2V_TOK) for L in Ls} >= {"under", "on", "over"}
    assert {M.k2v_edge(L, M.K2V_WTOK) for L in (255, 256, 257, 513)} == {"under", "on", "over"}
    assert {c.C for c in M.K2V_CASES} == {4, 64, 68, 96}
    for d, C in M.K2V_DIMS:
        assert {(c.bias, c.silu) for c in M.K2V_CASES if c.dims == d and c.C == C and not c.pad} == {(a, b) for a in (True, False) for b in (True, False)}
    assert any(c.pad for c in M.K2V_CASES)


# ---------------------------------------------------------------------------------------------------------------------
# references and yardstick
# ---------------------------------------------------------------------------------------------------------------------
ALL_CASES = [c for fam in ("k2", "k2n", "k2v", "k6", "k10") for c in M.CASES[fam]]


def test_case_ids_are_unique():
    ids = [M.family(c) + "-" + M.case_id(c) for c in ALL_CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("case", ALL_CASES, ids=[M.family(c) + "-" + M.case_id(c) for c in ALL_CASES])
def test_reference_is_finite_and_the_plain_fp32_yardstick_meets_the_bounds(case):
    ref, yard = M.reference_and_yardstick(case)
    tols = M.bounds(case, ref, yard)
    assert set(tols) == set(M.compared(case, ref)) and "y" in tols and len(tols) >= 2
    for q, tol in tols.items():
        assert ref[q].dtype == torch.float64 and yard[q].dtype == torch.float32
        assert bool(torch.isfinite(ref[q]).all()) and bool(torch.isfinite(yard[q]).all()), q
        mask = M.mask_for(case, q, ref)
        if mask is not None:
            excluded = 1.0 - float(mask.double().mean())
            print(f"{M.family(case)} {M.case_id(case)} {q}: {excluded:.2e} of the elements within {M.LEAKY_MIN_PRE} of the LeakyReLU kink")
            assert excluded <= M.LEAKY_MAX_EXCLUDED, (q, excluded)
            if q == "dx":              # ... and a slope taken on the other side of 0 moves the compared elements by less than half the bound
                shift = M.leaky_flip_shift(case, ref)
                print(f"{M.family(case)} {M.case_id(case)} dx: a flipped slope moves the other elements by at most {shift:.2e}")
                assert shift <= 0.5 * tol.a * max(1.0, float(ref[q].abs().max())), (shift, tol)
        err, excess = M.error(yard[q], ref[q], tol, mask)
        print(f"YARDSTICK {M.family(case)} {M.case_id(case)} {q} {tol.kind} {err:.2e} bound {tol.a:.2e}")
        assert excess <= 0.0, (q, err, tol)
        if tol.widen:                  # a widened bound stays far below what a dropped or doubled row or plane would cause (see below)
            assert tol.a <= 5e-4, (q, tol)


def _xhat(x):
    mean = x.mean(1, keepdim=True)
    return (x - mean) / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + M.EPS)


def test_a_lost_second_trip_is_far_outside_the_widened_bounds():
    """What the bounds on the summed gradients still catch at the largest sum: a looping K6 case whose second trip (the rows from
    1024 * RPB on, 65 of 65 601) is left out of d(gamma) / d(beta)."""
    case = next(c for c in M.K6_CASES if c.form == "plain" and c.C == 48 and c.rows == M.k6_loop_rows(48))
    ref, yard = M.reference_and_yardstick(case)
    t = {k: v.double() for k, v in M.inputs(case).items()}
    first_trip = 1024 * M.k6_rpb(48)
    tols = M.bounds(case, ref, yard)
    for q, full in (("dw", t["d_y"] * _xhat(t["x"])), ("db", t["d_y"])):
        assert M.error(full.sum(0), ref[q], tols[q])[1] <= 0.0, q
        err, excess = M.error(full[:first_trip].sum(0), ref[q], tols[q])
        assert excess > 0.0 and err > 100 * tols[q].a, (q, err, tols[q])
