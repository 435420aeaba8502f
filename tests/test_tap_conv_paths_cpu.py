"""The cases of tests/_tap_conv_cases.py are what they claim to be, checked without a GPU.

The path predicates agree with the library's host queries -- the launchers' own geometry (mlagg_conv_pad_geometry,
mlagg_conv_wgrad_taps_geometry, mlagg_conv_taps_geometry, mlagg_conv3x3_s2t_tile, mlagg_conv3x3_s2t_wgrad_geometry, the workspace
sizes) -- over the cases and a sweep; the case tables reach every slab, tail, tile, chunk and guard value listed in the coverage tests
(taking a boundary case out of a table fails here); the plan of every conv_nd case is the intended one; the host construction of the
padded copies obeys the properties the tap GEMMs rely on; and the plain-fp32 yardstick stays inside the UN-widened bounds the device
test uses, i.e. the inputs are well conditioned and a failure on the device means the kernel."""
import ctypes
import types

import pytest
import torch

from tests import _tap_conv_cases as M


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    from mlagg_unet_amd import _lib
    return _lib.lib()


def _pad_query(lib, D, H, W, stride, wide):
    Dq, Hq, Wq, guard = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    rc = lib.mlagg_conv_pad_geometry(D, H, W, stride, wide, ctypes.byref(Dq), ctypes.byref(Hq), ctypes.byref(Wq), ctypes.byref(guard))
    return None if rc else (Dq.value, Hq.value, Wq.value, guard.value)


def _k15_query(lib, batch, Q8, O, I, ntaps):
    out = (ctypes.c_int * 5)()
    rc = lib.mlagg_conv_wgrad_taps_geometry(batch, Q8, O, I, ntaps, out)
    return None if rc else tuple(out)


def _k16_query(lib, O, I, D, H, W, ntaps):
    out = (ctypes.c_long * 4)()
    rc = lib.mlagg_conv_taps_geometry(O, I, D, H, W, ntaps, out)
    return None if rc else tuple(out)


def _k19t_query(lib, B, O, I, H, W):
    out = (ctypes.c_int * 3)()
    rc = lib.mlagg_conv3x3_s2t_wgrad_geometry(B, O, I, H, W, out)
    return None if rc else tuple(out)


def _k15_geometry(c, wide=False):
    Q, Q8 = M.box_q(*M.dims3(c.dims), c.stride, wide)
    return Q, Q8, M.k15_geometry(c.B, Q8, c.O, c.I, M.ntaps(c))


def _dev(shape):
    """Something conv_nd_plan takes for an fp32 device map of this shape (no GPU here)."""
    return types.SimpleNamespace(is_cuda=True, dtype=torch.float32, shape=torch.Size(shape), dim=lambda: len(shape))


# ---------------------------------------------------------------------------------------------------------------------
# predicates against the library
# ---------------------------------------------------------------------------------------------------------------------
def test_pad_geometry_matches_the_library(lib):
    shapes = [M.dims3(c.dims) for c in M.ALL_CASES if c.family != "k19t"] + [d for _, _, _, d, _, _, _ in M.PAD_CASES]
    shapes += [(D, H, W) for D in (1, 2, 3, 6) for H in (1, 2, 5, 8) for W in range(1, 18)]
    seen = set()
    for D, H, W in shapes:
        for stride in (1, 2, 3):
            for wide in (0, 1):
                want = M.pad_geometry(D, H, W, stride, wide)
                assert _pad_query(lib, D, H, W, stride, wide) == want, (D, H, W, stride, wide)
                seen.add((stride, wide, want is None))
                if want:
                    Dq, Hq, Wq, guard = want
                    # what the kernels rely on: float4 rows, 8-voxel steps, and every tap shift (one plane + one row + one voxel
                    # either way, from a walk that may overhang Q by up to 7 voxels) inside the guard
                    assert Wq % 4 == 0 and guard % 8 == 0 and guard >= Hq * Wq + Wq + 1 + 7
    assert {(1, 0, False), (1, 1, False), (1, 1, True), (2, 0, False), (2, 0, True), (2, 1, True), (3, 0, True)} <= seen
    assert _pad_query(lib, 0, 4, 4, 1, 0) is None and _pad_query(lib, 4, 4, 0, 1, 0) is None


def test_k15_geometry_matches_the_launcher(lib):
    def same(batch, Q8, O, I, ntaps):
        g = M.k15_geometry(batch, Q8, O, I, ntaps)
        assert _k15_query(lib, batch, Q8, O, I, ntaps) == (g.slab, g.nslabs, g.ngroups, g.otiles, g.itiles), (batch, Q8, O, I, ntaps)
        assert lib.mlagg_conv_wgrad_taps_workspace_floats(batch, Q8, O, I, ntaps) == g.rows * ntaps * O * I
        assert (g.nslabs - 1) * g.slab + 8 * g.last_steps == Q8 and 0 < g.last_steps <= g.full_steps
        assert sum(M.k15_tap_groups(ntaps)) == ntaps and len(M.k15_tap_groups(ntaps)) == g.ngroups
    for c in M.K15_CASES + M.K15_ND_CASES + M.K16_CASES:
        Q, Q8, _ = _k15_geometry(c, wide=c.family == "k16")
        same(c.B, Q8, c.O, c.I, M.ntaps(c))
    slabs = set()
    for batch in (1, 2, 5):
        for Q8 in (8, 256, 264, 2048, 7688, 65536, 65544, 96 * 160 * 160 // 8 * 8, 98 * 162 * 168):
            for O, I in ((1, 1), (31, 33), (32, 32), (96, 64), (320, 320)):
                for ntaps in (1, 8, 9, 10, 27):
                    same(batch, Q8, O, I, ntaps)
                    slabs.add(M.k15_geometry(batch, Q8, O, I, ntaps).slab)
    assert slabs == {256, 512, 1024, 2048, 4096, 8192}
    assert _k15_query(lib, 1, 260, 4, 4, 27) is None and _k15_query(lib, 1, 264, 4, 4, 28) is None     # Q % 8, more than 27 taps
    assert lib.mlagg_conv_wgrad_taps_workspace_floats(1, 260, 4, 4, 27) == 0 == lib.mlagg_conv_wgrad_taps_workspace_floats(1, 264, 4, 4, 28)
    assert [M.k15_tap_groups(n) for n in (1, 9, 27)] == [[1], [9], [9, 9, 9]]


def test_k16_geometry_matches_the_launcher(lib):
    def same(O, I, D, H, W, ntaps):
        g = M.k16_geometry(O, I, D, H, W, ntaps)
        assert _k16_query(lib, O, I, D, H, W, ntaps) == (g.Q, g.nwg, g.otiles, g.lds), (O, I, D, H, W, ntaps)
        assert g.nwg * M.K16_WG_VOX - g.past == g.Q and 0 <= g.past < M.K16_WG_VOX and g.Q % 4 == 0
        inside = M.k16_inside(D, H, W)
        assert 4 * len(inside) == D * H * W and len(set(inside)) == len(inside)               # every data voxel, once
    for c in M.K16_CASES:
        same(c.O, c.I, *c.dims, M.ntaps(c))
    for O, I in ((1, 8), (33, 9), (64, 65)):
        for D, H, W in ((1, 3, 4), (2, 6, 8), (3, 11, 8), (5, 7, 12), (9, 13, 16)):
            for ntaps in (1, 27):
                same(O, I, D, H, W, ntaps)
    assert _k16_query(lib, 8, 8, 2, 3, 6, 27) is None                                         # W % 4


def test_k19t_tile_and_weight_gradient_geometry_match_the_launcher(lib):
    for R in range(1, 400):
        assert lib.mlagg_conv3x3_s2t_tile(R) == M.k19t_tile(R)
    assert lib.mlagg_conv3x3_s2t_tile(0) == 0
    shapes = [(B, O, I) + d for _, B, I, O, d, _ in M.K19T_SHAPES]
    shapes += [(2, 96, 192, 64, 64), (2, 192, 384, 32, 32), (10, 384, 768, 16, 16), (2, 96, 96, 30, 256), (1, 16, 16, 1, 1), (64, 768, 768, 40, 40),
               (3, 48, 16, 3, 37), (1, 16, 16, 640, 512)]
    flags = set()
    for B, O, I, H, W in shapes:
        g = M.k19t_wgrad_geometry(B, O, I, H, W)
        assert _k19t_query(lib, B, O, I, H, W) == (g.cw, g.per_part, g.nparts), (B, O, I, H, W)
        assert lib.mlagg_conv3x3_s2t_wgrad_workspace_floats(B, O, I, H, W) == B * g.nparts * 9 * O * I
        assert (g.nparts - 1) * g.per_part + g.last_part == H * g.cw and 0 < g.last_part <= g.per_part
        flags.add((g.capped, g.clamped))
    assert {(False, True), (False, False), (True, False)} <= flags                             # floor of 4; neither; the 256 MB cap
    assert _k19t_query(lib, 1, 24, 16, 4, 4) is None                                          # O % 16


# ---------------------------------------------------------------------------------------------------------------------
# the plans: which kernels the conv_nd cases run on; a one-slice volume is the tap GEMMs'
# ---------------------------------------------------------------------------------------------------------------------
def test_the_plan_of_every_conv_nd_case(lib):
    from mlagg_unet_amd import ops
    for c in M.K15_CASES + M.K15_ND_CASES + M.K16_CASES:
        nd = len(c.dims)
        args = (_dev((c.B, c.I) + c.dims), torch.empty(c.O, c.I, *([c.k] * nd)), (c.stride,) * nd, (c.k // 2,) * nd)
        assert ops.conv_wgrad_supported(*args), c.id
        plan = ops.conv_nd_plan(*args)
        if c.family == "k16":
            assert plan == ("K16", "K16", "K15"), (c.id, plan)
        elif c.family == "k15_nd":
            assert plan == (None, None, "K15"), (c.id, plan)
    # k = 3 reaches K16 only past K19: I % 16 != 0, under 96 voxels, or one slice
    why = {c.id: (c.I % 16 != 0, M.pixels(c.dims) < 96, c.dims[0] == 1) for c in M.K16_CASES if c.k == 3}
    assert {w for w in why.values() if sum(w) == 1} == {(True, False, False), (False, True, False), (False, False, True)}, why


def test_one_slice_volumes_are_not_planned_onto_k19(lib):
    """mlagg_conv3x3x3_fwd refuses D <= 1; the query must say so (it accepted D == 1, and conv_nd then raised)."""
    assert lib.mlagg_conv3x3x3_supported(16, 16, 2, 6, 8) and not lib.mlagg_conv3x3x3_supported(16, 16, 1, 12, 8)
    assert not lib.mlagg_conv3x3x3_supported(32, 32, 1, 64, 64) and not lib.mlagg_conv3x3x3_wgrad_supported(32, 32, 1, 64, 64)


# ---------------------------------------------------------------------------------------------------------------------
# coverage: what the tables must reach (each line names the case that provides it)
# ---------------------------------------------------------------------------------------------------------------------
def test_k15_cases_cover_the_slab_tail_tile_and_reduce_paths():
    ids = [c.id for c in M.ALL_CASES]
    assert len(set(ids)) == len(ids)
    geo = {c.id: _k15_geometry(c, wide=c.family == "k16") for c in M.K15_CASES + M.K15_ND_CASES + M.K16_CASES}
    Q, Q8, g = geo["A1"]
    assert M.by_id("A1").dims == (4, 9, 2) and Q == Q8 == 264 and Q8 % 256 == 8 and (g.nslabs, g.last_steps) == (2, 1)
    Q, Q8, g = geo["A2"]
    assert Q % 8 == 4 and Q8 == Q + 4 and g.nslabs == 1 and len(M.by_id("A2").dims) == 2 and M.ntaps(M.by_id("A2")) == 9
    assert (g.otiles, g.itiles, g.last_o, g.last_i) == (1, 2, 31, 1)
    Q, Q8, g = geo["A3"]
    assert (g.ngroups, g.otiles, g.last_o, g.last_i) == (3, 2, 1, 31)
    Q, Q8, g = geo["A4"]
    assert M.k15_tap_groups(M.ntaps(M.by_id("A4"))) == [1] and (M.by_id("A4").O, M.by_id("A4").I) == (1, 32)
    assert (M.by_id("A5").O, M.by_id("A5").I) == (32, 1) and M.ntaps(M.by_id("A5")) == 9
    Q, Q8, g = geo["A6"]
    assert g.slab == 512 and g.otiles * g.itiles == 64 and M.ntaps(M.by_id("A6")) == 1 and g.last_steps == 1 and g.full_steps == 64
    assert [geo[n][2].rows for n in ("A2", "A8", "A9", "A10", "A7")] == [1, 16, 17, 32, 33]
    assert M.k15_reduce_shapes(1) == {(0, 1), (0, 0)} and M.k15_reduce_shapes(16) == {(0, 1)} and M.k15_reduce_shapes(17) == {(1, 0), (0, 1)}
    assert M.k15_reduce_shapes(32) == {(1, 0)} and M.k15_reduce_shapes(33) == {(1, 1), (1, 0)}
    c = M.by_id("A11")
    assert c.dims[0] == 1 and len(c.dims) == 3 and c.stride == 1 and M.zero_taps(c) == [(0,), (2,)]
    # the tails of the double-buffered loop, in a LAST slab behind full ones and in a single slab
    last = {M.k15_tail(g.last_steps) for _, _, g in geo.values() if g.nslabs > 1}
    assert last == {"one", "two", "odd", "even"}, last
    assert (geo["T3"][2].nslabs, geo["T3"][2].last_steps) == (5, 2) and (geo["N2"][2].nslabs, geo["N2"][2].last_steps) == (4, 3)
    # ... and with data in them: a volume's short last slab lies in the zero ring of its last plane (A1, the reduce rows of A7), so
    # each short tail and the reduce kernel's tail row are also entered by a narrow 2-D map whose last slab holds its last data rows
    def first_of_last_slab(n):
        return (geo[n][2].nslabs - 1) * geo[n][2].slab
    live = {n: M.k15_last_data_voxel(M.by_id(n).dims, M.by_id(n).stride) >= first_of_last_slab(n) for n in ("A1", "A7", "A12", "A13", "A14", "A15")}
    assert live == dict(A1=False, A7=False, A12=True, A13=True, A14=True, A15=True), live
    assert [M.k15_tail(geo[n][2].last_steps) for n in ("A12", "A13", "A14")] == ["one", "two", "odd"]
    for n in ("A12", "A13", "A14"):                                                  # the last step of the walk holds data
        assert M.k15_last_data_voxel(M.by_id(n).dims, 1) >= geo[n][1] - 8
    assert geo["A15"][2].rows == 33 and M.by_id("A15").B == 3
    assert {M.k15_tail(g.last_steps) for _, _, g in geo.values() if g.nslabs == 1} >= {"two", "even"}
    assert all(M.k15_tail(g.full_steps) == "even" for _, _, g in geo.values())
    # Q % 8 == 4 on the wide copies too (K15 behind K16)
    assert geo["T4"][0] % 8 == 4
    # channel counts, taps, strides
    k15 = M.K15_CASES + M.K15_ND_CASES
    assert {1, 31, 32, 33} <= {c.O for c in k15} and {1, 31, 32, 33} <= {c.I for c in k15}
    assert {(len(c.dims), c.k) for c in k15} == {(2, 1), (2, 3), (3, 1), (3, 3)}
    assert {M.ntaps(c) for c in k15} == {1, 9, 27}
    s2 = [c for c in M.K15_CASES if c.stride == 2]
    assert {c.k for c in s2} == {1, 3} and {c.k for c in s2 if c.dims == (2, 2, 2)} == {1, 3}
    for axis in range(3):
        for k in (1, 3):
            assert {c.dims[axis] % 2 for c in s2 if c.k == k} == {0, 1}, (axis, k)
    assert {M.k15_reduce_last_block(M.ntaps(c), c.O, c.I) == 0 for c in k15} == {True, False}
    assert {c.stride for c in M.K15_ND_CASES} == {1, 2} and {len(c.dims) for c in M.K15_ND_CASES} == {2, 3}
    assert all(M.by_id(cid).family == "k15" for cid in M.ACCUMULATE_CASES) and {M.by_id(cid).stride for cid in M.ACCUMULATE_CASES} == {1, 2}


def test_k16_cases_cover_the_workgroup_chunk_and_tile_paths():
    geo = {c.id: M.k16_geometry(c.O, c.I, *c.dims, M.ntaps(c)) for c in M.K16_CASES}
    assert geo["T1"].Q == 512 and geo["T1"].past == 0 and geo["T1"].nwg == 1
    assert geo["T2"].nwg == 1 and geo["T2"].past > 0 and geo["T2"].odd_clamp
    assert M.by_id("T3").dims == (3, 11, 8) and geo["T3"].Q % 512 == 16 and geo["T3"].past == 496 and geo["T3"].nwg == 3
    assert (geo["T4"].chunks, geo["T4"].last_chunk, geo["T4"].last_o) == (3, 1, 1)
    assert (geo["T5"].chunks, geo["T5"].last_chunk, geo["T5"].otiles, geo["T5"].last_o) == (2, 32, 2, 1)
    assert M.by_id("T7").dims[0] == 1 and M.by_id("T7").I % 16 == 0 and M.pixels(M.by_id("T7").dims) >= 96
    assert M.by_id("T8").I % 16 == 0 and M.pixels(M.by_id("T8").dims) < 96
    cases = M.K16_CASES
    assert {c.I for c in cases} >= {8, 9, 32, 33, 64, 65} and {c.O for c in cases} >= {1, 31, 32, 33}
    assert {c.dims[2] for c in cases} == {4, 8, 12} and {c.k for c in cases} == {1, 3}
    assert {g.big_lds for g in geo.values()} == {True, False} and {g.lds for g in geo.values()} == {4096, 108 * 1024}
    assert {g.odd_clamp for g in geo.values()} == {True, False} and {g.last_o for g in geo.values()} >= {1, 31, 32}
    assert {g.last_chunk for g in geo.values()} >= {1, 8, 9, 32}
    # lanes inside the data box: some rows of lanes are all outside (the ring), some workgroups mix both
    for c in cases:
        inside = M.k16_inside(*c.dims)
        assert 0 < 4 * len(inside) < geo[c.id].Q


def test_k19t_cases_cover_the_tile_loop_pixel_and_part_paths():
    shapes = {n: (B, I, O) + d for n, B, I, O, d, _ in M.K19T_SHAPES}
    for n in shapes:
        assert {c.form for c in M.K19T_CASES if c.id.startswith(n + "-f")} == {3, 1, 2}, n      # every operand form on every shape
    fwd = {n: M.k19t_gemm(0, O, I, H * W, 3) for n, (B, I, O, H, W) in shapes.items()}
    dg = {n: M.k19t_gemm(1, O, I, H * W, 3) for n, (B, I, O, H, W) in shapes.items()}
    wg = {n: M.k19t_wgrad_geometry(B, O, I, H, W) for n, (B, I, O, H, W) in shapes.items()}
    for side, R in ((fwd, 2), (dg, 1)):
        assert {s[R] for s in shapes.values()} == {16, 32, 48, 64, 96}
        assert {g.nblk for g in side.values()} >= {1, 2, 3} and {g.loop for g in side.values()} >= {"tail", "pair", "pair+tail"}
        assert {g.to for g in side.values()} == {1, 2}
        # R = 16 and R = 48 leave a half-empty 32-row tile
        assert {s[R] for n, s in shapes.items() if side[n].last_rows == 16} == {16, 48}
    assert {s[3] for s in shapes.values()} == {1, 2, 3} and {s[4] for s in shapes.values()} >= {1, 8, 15, 16, 17, 33}
    assert {s[3] * s[4] for s in shapes.values()} >= {31, 33, 127, 129}
    assert fwd["P3"].last_wave == 1 and fwd["P6"].wgs == 2 and fwd["P6"].last_wg == 1 and fwd["P5"].last_wg == 127
    # accumulators: forward TO = 1 split, forward TO = 2 not (at a ragged pixel count), data gradient always, fp32 form only
    assert fwd["P4"].split and not fwd["P5"].split and fwd["P5"].to == 2 and shapes["P5"][3] * shapes["P5"][4] % 32 != 0
    assert all(g.split for g in dg.values()) and {g.to for g in dg.values()} == {1, 2}
    assert not M.k19t_gemm(0, 32, 32, 64, 1).split and not M.k19t_gemm(1, 32, 32, 64, 2).split
    # weight gradient
    assert {g.cw for g in wg.values()} >= {1, 2, 3, 8}
    assert {g.last_block for g in wg.values()} >= {1, 8, 15, 16} and {g.half1 for g in wg.values()} >= {0, 7, 8}
    assert any(g.nparts > 1 and g.last_part < g.per_part for g in wg.values()) and wg["P7"][1:4] == (4, 3, 1)
    assert all(g.clamped and not g.capped and g.per_part == 4 for g in wg.values())
    c = M.by_id("P11-f3")
    g = M.k19t_wgrad_geometry(c.B, c.O, c.I, *c.dims)
    assert not g.clamped and not g.capped and (g.per_part, g.nparts, g.last_part) == (5, 14, 1)
    assert M.k19t_gemm(0, c.O, c.I, M.pixels(c.dims), 3)[:5] == (2, 2, 64, 8, "pairs") and M.pixels(c.dims) % 128 == 32
    assert M.k19t_padding_rows(1, 0) == (0, 2) and M.k19t_padding_rows(3, 0) == (0,) and M.k19t_padding_rows(3, 2) == (2,)
    assert M.k19t_padding_rows(3, 1) == () and M.k19t_padding_rows(2, 1) == (2,)
    assert M.zero_taps(M.by_id("P1-f3")) == [(0,), (2,)] and M.zero_taps(M.by_id("P2-f3")) == []
    # the views: a ragged map, not only the 12 x 20 one of tests/test_conv3x3_s2t_gpu.py
    views = [s for n, s in shapes.items() if any(c.sliced == "views" for c in M.K19T_CASES if c.id.startswith(n + "-f"))]
    assert len(views) >= 2 and any(s[4] % 16 for s in views)


# ---------------------------------------------------------------------------------------------------------------------
# the padded copies, built on the host
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", M.PAD_CASES, ids=[r[0] for r in M.PAD_CASES])
def test_host_padded_rows_hold_every_voxel_once_between_zero_guards(row):
    name, B, C, dims, stride, wide, out = row
    g = torch.Generator().manual_seed(len(name) + sum(dims))
    src = torch.randn(B, C, *(out or dims), generator=g).double()
    rows = M.padded_rows(src, dims, stride, wide, out is not None)
    Dq, Hq, Wq, guard = M.pad_geometry(*dims, stride, wide)
    assert rows.shape == (B, 1 if (stride == 1 or out) else 8, C, 2 * guard + Dq * Hq * Wq)
    assert float(rows[..., :guard].abs().max()) == 0.0 and float(rows[..., -guard:].abs().max()) == 0.0
    assert torch.equal(rows.sum(dim=(1, 3)), src.sum(dim=(2, 3, 4)))                       # every voxel once (sums of the same values
    assert int((rows != 0).sum()) == int((src != 0).sum())                                 # in another order: compare counts too)


@pytest.mark.parametrize("dims,k,stride,wide", [((3, 4, 5), 3, 1, 0), ((2, 3, 4), 3, 1, 1), ((1, 4, 5), 3, 1, 0), ((4, 5, 3), 3, 2, 0),
                                                ((2, 2, 2), 3, 2, 0), ((5, 4, 6), 1, 2, 0), ((3, 4, 5), 1, 1, 0), ((4, 5), 3, 1, 0)])
def test_tap_sums_over_the_host_rows_are_the_weight_gradient(dims, k, stride, wide):
    """padded_rows is the layout the tap GEMMs need, not merely the one mlagg_volume_pad writes: the sums over q of
    dyp[o][q] * xp[i][q + off_t] on the host-built rows, with ops._tap_offsets' shifts, over Q8 voxels (the overhang included), are
    float64 conv's weight gradient."""
    from mlagg_unet_amd import ops
    import torch.nn.functional as F
    nd, B, I, O = len(dims), 2, 3, 2
    g = torch.Generator().manual_seed(sum(dims) + k + stride)
    x = torch.randn(B, I, *dims, generator=g).double()
    w = torch.randn(O, I, *([k] * nd), generator=g).double().requires_grad_(True)
    y = (F.conv3d if nd == 3 else F.conv2d)(x, w, None, stride, k // 2)
    dy = torch.randn(y.shape, generator=g).double()
    y.backward(dy)
    d3 = M.dims3(dims)
    Dq, Hq, Wq, guard = M.pad_geometry(*d3, stride, wide)
    Q, Q8 = M.box_q(*d3, stride, wide)
    row = 2 * guard + Q
    xp = M.padded_rows(x.reshape(B, I, *d3), d3, stride, wide, False)
    dyp = M.padded_rows(dy.reshape(B, O, *M.dims3(y.shape[2:])), d3, stride, wide, True)
    taps = ops._tap_offsets(k, nd, stride, Hq, Wq, I, row)
    dW = torch.zeros(O, I, len(taps), dtype=torch.float64)
    for b in range(B):
        flat, a = xp[b].reshape(-1), dyp[b, 0].reshape(-1)
        for t, off in enumerate(taps):
            for i in range(I):
                for o in range(O):
                    dW[o, i, t] += a[o * row + guard:o * row + guard + Q8] @ flat[i * row + guard + off:i * row + guard + off + Q8]
    assert float((dW.view(w.shape) - w.grad).abs().max()) < 1e-12


def test_pad_cases_cover_the_forms():
    forms = {(stride, wide, out is not None) for _, _, _, _, stride, wide, out in M.PAD_CASES}
    assert forms == {(1, 0, False), (1, 0, True), (1, 1, False), (1, 1, True), (2, 0, False), (2, 0, True)}
    s2 = [d for _, _, _, d, stride, _, out in M.PAD_CASES if stride == 2 and out is None]
    assert all({d[a] % 2 for d in s2} == {0, 1} for a in range(3))
    assert any(d[0] == 1 for _, _, _, d, _, _, _ in M.PAD_CASES)                           # a 2-D map
    for dims, stride, wide, out in M.PAD_REFUSED:
        geo = M.pad_geometry(*dims, stride, wide)
        if out is None:
            assert geo is None, (dims, stride, wide)
        else:
            org = (1 if stride == 1 and dims[0] > 1 else 0, 1 if stride == 1 else 0, (4 if wide else 1) if stride == 1 else 0)
            assert geo is not None and any(o + g0 > q for o, g0, q in zip(out, org, geo[:3])), (dims, out)


# ---------------------------------------------------------------------------------------------------------------------
# references and yardstick
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.ALL_CASES, ids=[c.id for c in M.ALL_CASES])
def test_reference_is_finite_and_the_plain_fp32_yardstick_is_within_the_bounds(case):
    ref, yard = M.reference(case), M.yardstick(case)
    tols = M.bounds(case)
    for q in ("y", "dx", "dW"):
        assert ref[q].dtype == torch.float64 and yard[q].dtype == torch.float32 and ref[q].shape == yard[q].shape
        assert bool(torch.isfinite(ref[q]).all()) and bool(torch.isfinite(yard[q]).all()), q
        err = M.error(yard[q], ref[q])
        used = q in M.compared(case)
        print(f"YARDSTICK {case.id} {q} {err:.2e} bound {tols[q]:.1e}{'' if used else ' (not compared on the device)'}")
        assert not used or err <= tols[q], (q, err, tols[q])
    # the widened bound of the weight gradient never passes the bound of tests/test_conv_wgrad_gpu.py
    assert tols["dW"] <= M.dw_bound(case, ref["dW"], yard["dW"]) <= 2e-5 + 1e-5 / float(ref["dW"].abs().max())
    for idx in M.zero_taps(case):
        sel = (slice(None), slice(None)) + idx
        assert float(ref["dW"][sel].abs().max()) == 0.0 and float(ref["dW"].abs().max()) > 0.0
