"""The cases of tests/_glue_kernel_cases.py are what they claim to be, checked without a GPU.

The path predicates agree with the library's host queries where one exists; the case tables reach every value a predicate can return
and both sides of every threshold (taking a boundary case out of a table fails here); the 2-D K1' reference restates the scan orders
of tests/test_msmm_scan_gpu.py independently; every reference value is finite; the plain-fp32 yardstick meets the bounds the device
test uses, i.e. the inputs are well conditioned and a failure on the device means the kernel; the derived sum bounds hold for the
yardstick in more than one summation order."""
import itertools

import pytest
import torch

from tests import _glue_kernel_cases as M


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    from mlagg_unet_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------
# predicates against the library
# ---------------------------------------------------------------------------------------------------------------------
def test_column_and_channel_sum_predicates_match_the_workspace_queries(lib):
    rows = sorted({c.rows for c in M.COL_CASES} | {r + d for r in range(512, 8193, 512) for d in (-1, 0, 1)} | {7840, 163840})
    cols = sorted({c.cols for c in M.COL_CASES} | {64 * g + d for g in (1, 2, 3, 42, 43, 64, 85, 86, 127, 128, 129) for d in (-1, 0, 1)})
    for r, c in itertools.product(rows, cols):
        slabs, per = M.column_sum_slabs(r, c)
        assert lib.mlagg_column_sum_workspace_floats(r, c) == (slabs * c if slabs > 1 else 0), (r, c)
        assert (slabs - 1) * per < r <= slabs * per and (slabs == 1 or (r >= 2048 and c <= 127 * 64)), (r, c)      # no empty slab
    assert lib.mlagg_column_sum_workspace_floats(0, 5) == 0 and lib.mlagg_column_sum_workspace_floats(5, 0) == 0
    for c in M.SUM_CASES:
        assert lib.mlagg_channel_sum_workspace_floats(c.B, c.C) == c.B * c.C


# ---------------------------------------------------------------------------------------------------------------------
# coverage: what the tables must reach (each line names the boundary case that provides it)
# ---------------------------------------------------------------------------------------------------------------------
def test_xscan_cases_cover_every_path_and_edge():
    for op in ("scan", "merge"):
        mine = [c for c in M.XSCAN_CASES if c.op == op]
        vec = {c.HW: M.xscan_vec4(c.HW) for c in mine}
        want = {((16, 16),): [True], ((20, 36),): [True], ((17, 33),): [False], ((6, 8),): [False], ((8, 6),): [False], ((5, 3),): [False], ((1, 1),): [False], ((1, 64),): [False],
                ((64, 1),): [False], ((8, 8), (6, 6), (4, 4)): [True, False, True],              # both paths in one launch, Lc = 116
                ((6, 6), (8, 8)): [False, True],                                                 # vec4 at the 4-aligned offset 36
                ((5, 5), (8, 8)): [False, False],                                                # an 8 x 8 scale, scalar through its offset 25
                ((8, 8), (3, 3)): [False, False],                                                # ... through Lc = 73
                ((32, 32), (16, 16), (8, 8), (4, 4)): [True] * 4}
        assert vec == want, op
        alone = {(h % 4 != 0, w % 4 != 0) for hw in vec for h, w in hw if len(hw) == 1 and (h * w) % 4 == 0 and not M.xscan_vec4(hw)[0]}
        assert alone >= {(True, False), (False, True)}                            # scalar through H alone ((6, 8), (1, 64)), through W alone
        assert M.xscan_offsets(((8, 8), (6, 6), (4, 4))) == ([0, 64, 100], 116) and M.xscan_offsets(((6, 6), (8, 8)))[0][1] % 4 == 0
        tiles = {c.HW: M.xscan_tiles(c.HW) for c in mine}
        assert tiles[((16, 16),)] == ([0, 1], [(False, False)])                                   # exactly one tile
        assert tiles[((20, 36),)] == ([0, 6], [(True, True)]) and tiles[((17, 33),)] == ([0, 6], [(True, True)])      # ragged by 4, by 1
        assert tiles[((1, 64),)][0] == [0, 4] and tiles[((64, 1),)][0] == [0, 4]                  # 1-row and 1-column maps: four tiles
        assert tiles[((32, 32), (16, 16), (8, 8), (4, 4))][0] == [0, 4, 5, 6, 7]                  # every tile0 entry is looked up
        assert tiles[((8, 8), (6, 6), (4, 4))][0] == [0, 1, 2, 3]
        assert {c.CB for c in mine} == {3, 16, 32, 36, 96}
        assert {tuple(M.xscan_channel_blocks(c.CB)) for c in mine} == {(3,), (16,), (32,), (32, 4), (32, 32, 32)}
        # a ragged channel block on a vec4, a scalar and a multi-scale geometry
        assert {tuple(M.xscan_vec4(c.HW)) for c in mine if c.CB % 32} >= {(True,), (False,), (True, True, True, True)}
    assert {c.HW for c in M.XSCAN_CASES if c.op == "scan"} == {c.HW for c in M.XSCAN_CASES if c.op == "merge"} == {g for g, _ in M.XS_GEOMETRIES}
    bc = [c for c in M.XSCAN_CASES if c.op == "bc"]
    assert {tuple(M.xscan_vec4(c.HW)) for c in bc} == {(True,), (False,), (True, False, True)}
    assert M.XS_PER == 35 and (M.XS_R * 4) % 16 != 0                                              # column offsets 3 and 19: not 16-byte aligned


def test_iscan_cases_cover_every_path_and_edge():
    for op in ("scan", "merge"):
        mine = [c for c in M.ISCAN_CASES if c.op == op and c.dims is None]
        assert {M.iscan_tile(c.L) for c in mine} >= {(1, 1), (1, 63), (1, 64), (2, 1), (3, 1)}
        assert {c.L % 64 for c in mine} >= {1, 63, 0}
        for L in M.IS_LENGTHS:                                                                    # every form at every tail
            assert {(c.K, c.CB) for c in mine if c.L == L} >= set(M.IS_FORMS), (op, L)
            assert {M.imerge_form(c.K, c.CB) for c in mine if c.L == L} == {"wide+block_sum", "atomic", "plain"}
        trips = {(c.L, c.CB): M.iscan_trips(M.iscan_tile(c.L)[1], c.CB) for c in mine}
        assert trips[(32, 64)] == 1 and 32 * 64 == 2048 and trips[(33, 64)] == 2                   # exactly one trip; one element run past it
        assert trips[(65, 512)] == 1 and M.iscan_trips(64, 512) == 16                             # (the first tile of L = 65 has 64 steps)
        assert {M.iscan_lds_bytes(c.CB)[1] for c in mine} == {True, False} and all(M.iscan_lds_bytes(c.CB)[2] for c in mine)
        assert M.iscan_lds_bytes(512) == (133120, True, True) and M.iscan_lds_bytes(190)[1] and not M.iscan_lds_bytes(189)[1]
        assert {c.CB for c in mine} >= {1, 512} and {c.K for c in mine} >= {1, 2, 3, 12}
        wide = {c.K for c in mine if M.imerge_form(c.K, c.CB) == "wide+block_sum"}
        assert wide == {2, 3, 12} and {M.block_sum_shape(K) for K in wide} == {(1, 0), (1, 1), (6, 0)}     # a pair, a pair + the odd one, six pairs
        assert any(c.dims is not None and c.K == 12 for c in M.ISCAN_CASES if c.op == op)          # the axis orders of a volume
    assert not M.iscan_lds_bytes(513)[2]
    blk = [c for c in M.ISCAN_CASES if c.op == "scanblk"]
    assert blk and all(M.iscan_layout(c)[1] > c.CB and M.iscan_layout(c)[2] > 0 for c in blk)
    assert M.iscan_layout(M.IScanCase("scanblk", 65, 12, 4, None)) == (108, 9, 3)                  # index_scan(wide, idx, 4, 9, 3)
    assert {c.CB for c in blk} >= {1, 4, 64}
    bc = [c for c in M.ISCAN_CASES if c.op == "bc"]
    assert {c.CB for c in bc} == {1, 3, 20} and {c.K for c in bc} >= {1, 2, 12} and {c.L % 64 for c in bc} >= {0, 1, 63}
    for c in M.ISCAN_CASES:                                                                        # every table is K permutations of L tokens
        idx = M.iscan_orders(c)
        assert idx.shape == (c.K, c.L) and all(torch.equal(idx[k].sort().values, torch.arange(c.L)) for k in range(c.K))


def test_k8_movement_cases_cover_every_form():
    plain = [c for c in M.MOVE_CASES if c.op == "plain"]
    forms = {(c.R, c.C): M.transpose_forms(c.R, c.C) for c in plain}
    assert {f[0] for f in forms.values()} == {(True, True), (True, False), (False, True), (False, False)}
    assert forms[(64, 64)] == ((True, True), (1, 1), (False, False))                              # exactly one tile
    assert forms[(63, 65)] == ((False, False), (2, 1), (True, True)) and forms[(65, 63)] == ((False, False), (1, 2), (True, True))
    assert forms[(3, 8)][0] == (True, False) and forms[(8, 3)][0] == (False, True)
    assert forms[(1, 130)][1] == (3, 1) and forms[(130, 1)][1] == (1, 3) and forms[(128, 48)][1] == (1, 2) and (1, 1) in forms
    assert {(c.R, c.C) for c in M.MOVE_CASES if c.op == "half"} == {s for s in forms if s[0] % 4 == 0} and len(forms) == 10
    assert {(c.R, c.C) for c in M.MOVE_CASES if c.op == "into"} == set(forms)
    assert M.MOVE_C0 % 4 == 0 and M.MOVE_PAD > M.MOVE_C0                                          # the slice starts 16-byte aligned for any R
    for op in ("fwd", "inv"):
        mine = [c for c in M.SHUF_CASES if c.op == op]
        assert {M.shuffle_threads(c.O, c.H, c.W) for c in mine} == {(1, 1), (255, 1), (256, 1), (257, 2)}
        assert any(c.W == 2 for c in mine) and any(c.H == 1 for c in mine) and all(c.W % 2 == 0 for c in mine)
    convt = [c for c in M.SHUF_CASES if c.op == "convt"]
    assert convt and any(M.shuffle_threads(c.O, c.H, c.W)[1] > 1 for c in convt)


def test_k8_reduction_cases_cover_every_path_and_threshold():
    want = {1: (0, 0, False, 1), 3: (0, 0, False, 3), 1020: (255, 1, False, 0), 1023: (0, 0, False, 1023), 1024: (256, 1, False, 0),
            1028: (257, 1, True, 0), 2048: (512, 1, True, 0), 2052: (513, 2, False, 0)}
    bias = [c for c in M.SUM_CASES if c.op == "bias"]
    for HW, shape in want.items():                                                # the second load dead at 256 float4, live at 257
        assert M.plane_sum_shape(HW) == shape and any(c.HW == HW for c in bias), HW
    assert {c.C for c in bias} == {1, 63, 64, 65} and {c.B for c in bias} == {1, 16, 17, 33}
    epi = [c for c in M.SUM_CASES if c.op == "epi"]
    assert {M.plane_sum_shape(c.HW)[1:] for c in epi} >= {(1, True, 0), (2, False, 0), (0, False, 1023), (1, False, 0)}
    assert {c.C for c in epi} == {1, 63, 64, 65} and {c.B for c in epi} == {1, 16, 17, 33}
    # the second-stage column sum over the B partial rows: under, on and over its 16 row groups, and a second trip of its pair loop
    slabs = {(c.rows, c.cols): M.column_sum_slabs(c.rows, c.cols) for c in M.COL_CASES if not c.wide}
    assert slabs[(2047, 65)] == (1, 2047) and slabs[(2047, 384)] == (1, 2047)                     # one row under the threshold
    assert slabs[(2048, 384)] == (4, 512) and slabs[(2048, 64)] == (4, 512)                       # on it: whole slabs
    assert slabs[(2049, 1)] == (4, 513) and slabs[(2049, 65)] == (4, 513)                         # one over: the last slab has 510 rows
    assert slabs[(2561, 63)] == (5, 513)                                                          # rows / 512 = 5, the last slab 509 rows
    assert slabs[(2048, 8128)] == (2, 1024) and slabs[(2048, 8129)] == (1, 2048)                  # 127 and 128 column groups
    assert {r for r, _ in slabs} >= {1, 16, 17, 2047, 2048, 2049, 2561} and {c for _, c in slabs} >= {1, 63, 64, 65, 384}
    wide = [M.column_sum_slabs(c.rows, c.cols)[0] for c in M.COL_CASES if c.wide]
    assert 1 in wide and 4 in wide and 5 in wide
    for c in M.COL_CASES:                                                         # a floor in place of the ceiling would drop rows
        s, per = M.column_sum_slabs(c.rows, c.cols)
        if c.rows in (2049, 2561):
            assert s > 1 and s * (c.rows // s) < c.rows
    grids = {c.per: M.row_scale_grid(len(c.scales) * c.per // 4) for c in M.RESID_CASES}
    assert grids[4] == (1, False) and grids[1776] == (9, False) and grids[M.RESID_BIG] == (8192, True)
    assert M.row_scale_grid(8192 * 256) == (8192, False) and M.row_scale_grid(8192 * 256 + 1) == (8192, True)
    assert 2 * M.RESID_BIG // 4 - 8192 * 256 == 258 and all(0.0 in c.scales and max(c.scales) > 0 for c in M.RESID_CASES)
    assert M.RESID_CASES[-1].scales[-1] != 0.0                                    # the second trip lands on a scaled sample
    assert {c.n for c in M.LAMBDA_CASES} == {1, 24, 63, 64, 65, 130} and {c.dot for c in M.LAMBDA_CASES} == {1.0, 8.0}
    for c in M.LAMBDA_CASES:
        t = M.inputs(c)
        assert abs(float((t["q1"].double() * t["k1"].double()).sum()) - c.dot) < 1e-3 * c.dot
        assert abs(float((t["q2"].double() * t["k2"].double()).sum()) - 0.9 * c.dot) < 1e-3 * c.dot


def test_k13_cases_cover_the_tails_the_clamps_and_the_type_combinations():
    assert {c.HW for c in M.EPI_CASES} == {1, 45, 1020, 1024, 1028}
    assert {M.epilogue_fp32_shape(c.HW) for c in M.EPI_CASES} == {(0, 1), (0, 45), (255, 0), (256, 0), (257, 0)}
    full = {(c.act, c.bias, c.res) for c in M.EPI_CASES if c.HW == 1028 and c.scale == 1.0}
    assert full == set(itertools.product(("none", "gelu"), (True, False), (True, False)))
    for HW in (1, 45, 1020, 1024):
        assert {c.act for c in M.EPI_CASES if c.HW == HW} == {"none", "gelu"}, HW
    assert any(c.scale == 3.0 and c.act == "gelu" for c in M.EPI_CASES)
    n, s, a = "none", "some", "all"
    want = {4: (1, (n, a, a, a)), 1020: (1, (n, a, a, a)), 1024: (1, (n, a, a, a)), 1028: (1, (n, s, a, a)), 4092: (1, (n, n, n, s)),
            4096: (1, (n, n, n, n)), 4100: (2, (n, a, a, a))}
    for HW, shape in want.items():
        assert M.epilogue_lp_trips(HW) == shape and any(c.HW == HW for c in M.EPILP_CASES), HW
    assert {c.HW for c in M.EPILP_CASES} == set(want)
    combos = {tuple(c)[1:] for c in M.EPILP_CASES}
    assert combos == set(itertools.product(("bf16", "fp16"), ("none", "fp32", "same"), ("same", "fp32"), (True, False), ("none", "gelu")))
    assert len(M.EPILP_CASES) == 48
    for HW in want:                                                               # every size with GELU and without, with a residual and d(bias)
        mine = [c for c in M.EPILP_CASES if c.HW == HW]
        assert {c.act for c in mine} == {"none", "gelu"} and any(c.bias for c in mine) and any(c.rdt != "none" for c in mine), HW


def test_k17_cases_cover_the_lane_layouts():
    geo = {(c.B, c.H, c.W, c.d, c.r): M.gelu_pool_geometry(c.B, c.H, c.W, c.d, c.r) for c in M.POOL_CASES}
    g = lambda per, cells, dead, wgs, last: dict(per=per, cells=cells, dead=dead, wgs=wgs, last_live=last, supported=True)     # noqa: E731
    assert geo[(2, 16, 16, 48, 8)] == g(96, 2, 64, 4, 2)
    assert geo[(2, 4, 4, 4, 1)] == g(1, 256, 0, 1, 32)                            # a thread per window, 32 of 256 cells live
    assert geo[(2, 6, 9, 20, 3)] == g(15, 17, 1, 1, 12)                           # one dead lane
    assert geo[(3, 12, 9, 20, 3)] == g(15, 17, 1, 3, 2)                           # a ragged last workgroup behind full ones
    assert geo[(2, 8, 8, 128, 8)] == g(256, 1, 0, 2, 1) and geo[(2, 2, 6, 1024, 1)] == g(256, 1, 0, 24, 1)       # the limit, r = 8 and r = 1
    assert geo[(2, 8, 12, 96, 4)] == g(96, 2, 64, 6, 2) and geo[(1, 2, 2, 8, 2)] == g(4, 64, 0, 1, 1)
    assert not M.gelu_pool_geometry(2, 8, 8, 192, 8)["supported"] and M.gelu_pool_geometry(2, 8, 8, 192, 8)["per"] == 384
    assert not M.gelu_pool_geometry(2, 1, 1, 1028, 1)["supported"]                # per = 257
    assert {c.via for c in M.POOL_CASES} == {"block", "split"} and any(c.scale == 6.0 for c in M.POOL_CASES)


def test_refusals_are_what_the_predicates_call_unsupported():
    ops = dict(M.REFUSALS)
    assert not M.gelu_pool_geometry(2, *ops["gelu_pool"])["supported"]
    assert not M.iscan_lds_bytes(ops["index_scan"])[2] and M.iscan_lds_bytes(ops["index_scan"] - 1)[2]
    assert ops["scaled_residual"] % 4 != 0 and ops["pixel_shuffle2"][2] % 2 == 1


# ---------------------------------------------------------------------------------------------------------------------
# the 2-D reference is an independent restatement of the scan orders
# ---------------------------------------------------------------------------------------------------------------------
def test_xscan_reference_equals_the_reference_orders_of_the_msmm_scan_test():
    from tests._selscan_regime_cases import reference_orders
    from tests.test_msmm_scan_gpu import CASES
    for _, HW in CASES + [(1, list(c.HW)) for c in M.XSCAN_CASES if c.op == "scan" and c.CB == 96]:
        L = sum(h * w for h, w in HW)
        tok = torch.arange(L, dtype=torch.float64).view(1, L, 1)
        seq = M.xscan_sequences(tok, HW)                                          # (1, 4, 1, L): the token each scan step reads
        assert torch.equal(seq[0, :, 0].long(), reference_orders(HW)), HW
        marks = torch.randn(1, 4, L, dtype=torch.float64)                         # merge: step l of direction k lands on token order[k][l]
        want = torch.zeros(L, dtype=torch.float64)
        for k in range(4):
            want.index_add_(0, reference_orders(HW)[k], marks[0, k])
        assert torch.allclose(M.xscan_merge(marks, HW)[0, :, 0], want, rtol=0, atol=1e-12), HW


# ---------------------------------------------------------------------------------------------------------------------
# references and yardstick
# ---------------------------------------------------------------------------------------------------------------------
ALL_CASES = [c for fam in M.CASES for c in M.CASES[fam]]
ALL_IDS = [M.family(c) + "-" + M.case_id(c) for c in ALL_CASES]


def test_case_ids_are_unique():
    assert len(set(ALL_IDS)) == len(ALL_IDS)


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_reference_is_finite_and_the_plain_fp32_yardstick_meets_the_bounds(case):
    ref, yards = M.reference_and_yardstick(case)
    tols = M.bounds(case, ref, yards)
    aux = M.aux(case, ref)
    assert set(tols) == set(M.compared(case, ref)) and set(tols) <= set(M.tolerances(case)) and tols
    for q, tol in tols.items():
        assert ref[q].dtype == torch.float64 and bool(torch.isfinite(ref[q]).all()), q
        for yard in yards:
            assert yard[q].dtype == torch.float32 and bool(torch.isfinite(yard[q]).all()), q
            err, excess = M.error(yard[q], ref[q], tol, aux.get(q))
            print(f"YARDSTICK {M.family(case)} {M.case_id(case)} {q} {tol.kind} {err:.2e} bound {tol.a:.2e} {tol.r:.0e}")
            assert excess <= 0.0, (q, err, tol)
        if tol.widen:                  # a widened bound stays far below what a dropped or doubled term would cause (see below)
            assert tol.a <= 5e-4, (q, tol)


MERGES = [c for c in M.XSCAN_CASES + M.ISCAN_CASES if c.op == "merge"]


@pytest.mark.parametrize("case", MERGES, ids=[M.family(c) + "-" + M.case_id(c) for c in MERGES])
def test_the_sum_bound_holds_in_either_summation_order(case):
    ref = M.evaluate(case, torch.float64)
    aux = M.aux(case, ref)
    tol = M.tolerances(case)["tok"]
    firsts = [M.evaluate(case, torch.float32, order)["tok"] for order in (0, 1)]
    for got in firsts:
        assert M.error(got, ref["tok"], tol, aux["tok"])[1] <= 0.0
    if tol.kind == "sum" and case.CB * (case.L if M.family(case) == "iscan" else M.xscan_len(case)) >= 64:
        assert tol.a == (4 if M.family(case) == "xscan" else case.K)
        assert not torch.equal(firsts[0], firsts[1]) or tol.a <= 2                # the two orders do differ: the bound is not an equality


def test_lost_terms_are_far_outside_the_bounds():
    """What the bounds on the sums still catch: a direction missing from a merge, and a row missing from a slabbed column sum (what a
    floor in place of the ceiling in the slab height would lose)."""
    case = M.IScanCase("merge", 65, 12, 5, None)
    ref = M.evaluate(case, torch.float64)
    t = {k: v.double() for k, v in M.inputs(case).items()}
    t["seq"][:, 11 * 5:] = 0.0                                                    # direction 11 never arrives
    got = M.compose(case, t)["tok"]
    assert M.error(got, ref["tok"], M.tolerances(case)["tok"], M.aux(case, ref)["tok"])[1] > 0.0
    case = M.ColCase(2049, 65, False)
    ref, yards = M.reference_and_yardstick(case)
    tol = M.bounds(case, ref, yards)["sum"]
    x = M.inputs(case)["x"].double()
    assert M.error(x.sum(0), ref["sum"], tol)[1] <= 0.0 and M.error(x[:2048].sum(0), ref["sum"], tol)[1] > 0.0
