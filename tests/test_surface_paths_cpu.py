"""Host side of the K24 path-boundary tests (tests/_surface_path_cases.py): the table reaches every path value it lists, the scipy
reference agrees with a brute-force search, the package's host path and crop layout agree with the references on every case, and
the inputs keep clear of their tolerances."""
import numpy as np
import pytest
import scipy.ndimage as ndi

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import surface
from tests import _surface_path_cases as C

KEYS = ("distances_gt_to_pred", "distances_pred_to_gt", "surfel_areas_gt", "surfel_areas_pred")


def _ids(cases):
    return [C.case_id(c) for c in cases]


def _crops():
    """[(case, D, [gt border, prediction border])] of every crop the device runs, with the label calls' (pairs=True) crops."""
    out = []
    for case in C.MASK_CASES:
        ref = C.mask_reference(case)
        if ref is not None:
            out.append((case, tuple(k + 1 for k in ref.n), ref.borders))
    for case in C.GROUPS["labels"]:
        for o in C.label_reference(case, True).values():
            if o.ref is not None:
                out.append((case, tuple(k + 1 for k in o.ref.n), o.ref.borders))
    return out


def test_the_table_reaches_every_path_value():
    crops = _crops()
    raw_D = [tuple(k + 1 for k in n) for _, n in C.RAW_CROPS]
    # sf_stats_kernel
    stats = C.GROUPS["stats"]
    assert {c.shape[2]: C.stats_segments(c.shape[2]) for c in stats if c.name != "second_stride"} == C.REACH["stats_segments"]
    assert {C.stats_grid_stride(c.shape) for c in stats} == C.REACH["stats_grid_stride"]
    z33 = next(c for c in stats if c.name == "z33")
    gt, seg = C.volumes(z33)
    assert C.stats_seam_runs(gt, z33.wanted) >= 3 and C.stats_seam_runs(seg, z33.wanted) >= 2
    assert gt[1, 2, 9] != 1 and (gt[1, 2, 10:21] == 1).all() and gt[1, 2, 21] != 1          # z 10..20: two flushes, two threads
    for c in stats:
        gt, seg = C.volumes(c)
        assert 7 in np.unique(gt) and 7 not in c.wanted                                       # present, not wanted
    big = next(c for c in stats if c.name == "second_stride")
    gt, _ = C.volumes(big)
    first_rows = C.SF_STATS_MAX_BLOCKS * C.SF_STATS_BLOCK // C.stats_segments(big.shape[2])
    rows1 = np.nonzero((gt == 1).any(axis=2).reshape(-1))[0]
    rows2 = np.nonzero((gt == 2).any(axis=2).reshape(-1))[0]
    assert rows1.min() >= first_rows and rows2.max() < first_rows
    # sf_codes_kernel
    uniform = set()
    for case in C.MASK_CASES:
        ref = C.mask_reference(case)
        if ref is not None:
            vox = int(np.prod([k + 1 for k in ref.n]))
            uniform.add(C.codes_mixed_waves([vox]) == 0 and vox % C.SF_WAVE == 0)
    for case in C.GROUPS["labels"]:
        vox = [int(np.prod([k + 1 for k in o.ref.n])) for o in C.label_reference(case).values() if o.ref is not None]
        assert len(vox) >= 3 and sum(1 for v in vox if v % C.SF_WAVE) >= 2 and C.codes_mixed_waves(vox) >= 2
        uniform.add(C.codes_mixed_waves(vox) == 0)
    assert uniform == C.REACH["codes_all_waves_uniform"]
    # sf_zpass_kernel
    D2s = {D[2] for _, D, _ in crops} | {D[2] for D in raw_D}
    assert C.REACH["zpass_D2"] <= D2s
    assert {C.zpass_chunks(d) for d in D2s} >= C.REACH["zpass_chunks"]
    hops = {}
    for case, D, borders in crops:
        if case.group == "carries" and D[2] >= 129:
            for m in (0, 1):
                hops[(case.name, m)] = C.zpass_hops(borders[m])
    assert hops[("low_z_128", 1)][0] == 2 and hops[("low_z_128", 1)][2]            # surfels at z 0..1 only, read at z = 128; empty lines
    assert hops[("low_z_128", 0)][1] == 1                                          # D2 = 129: the surfels at 127, 128 span two chunks
    assert hops[("low_z_129", 0)][1] == 2 and hops[("high_z_129", 1)][1] == 2      # D2 = 130: surfels at 128, 129 only, read at z = 0
    assert hops[("high_z_128", 0)][0] == 2
    # the y and x passes
    D1s, D0s = {D[1] for _, D, _ in crops} | {D[1] for D in raw_D}, {D[0] for _, D, _ in crops} | {D[0] for D in raw_D}
    assert C.REACH["trips_D"] <= D1s and C.REACH["trips_D"] <= D0s
    assert C.MAX_LINE in D1s and C.MAX_LINE in D0s
    ysites, xsites, full_y, full_x = set(), set(), False, False
    for case, D, borders in crops:
        for b in borders:
            ys, xs = C.line_sites(b)
            ysites |= ys
            xsites.add(xs)
            full_y |= D[1] in ys and D[1] > C.SF_WAVE
            full_x |= xs == D[0] and D[0] > C.SF_WAVE
    assert 0 in ysites and 0 in xsites and 2 in ysites and 2 in xsites and full_y and full_x
    for case in C.GROUPS["labels"]:                                               # D < nmax in a multi-label call
        Ds = [tuple(k + 1 for k in o.ref.n) for o in C.label_reference(case).values() if o.ref is not None]
        assert min(D[1] for D in Ds) < max(D[1] for D in Ds) and min(D[0] for D in Ds) < max(D[0] for D in Ds)
        assert all(len({D[a] for D in Ds}) == len(Ds) for a in range(3)) or case.name != "three"
    # sf_sum_kernel and the pair offsets: which label (position in the call) has how many lines
    eight = C.label_reference(C.GROUPS["labels"][0])
    kinds = [C.sum_lines(tuple(k + 1 for k in o.ref.n)) for o in eight.values() if o.ref is not None]
    assert set(kinds) == C.REACH["sum_lines"] and set(kinds[1:]) == C.REACH["sum_lines"]      # also with l0 != 0
    counts = [(int(o.ref.borders[0].sum()), int(o.ref.borders[1].sum())) for o in C.label_reference(C.GROUPS["labels"][0], True).values()
              if o.ref is not None]
    assert len(counts) >= 4 and all(sum(c) > 0 for c in counts[:3])                         # pair offsets of labels 2 and 3 non-zero


def test_two_site_envelope_queried_from_the_far_end():
    """carries along y: the y lines through the low cluster have the adjacent sites 0 and 1 only (the smallest envelope a mask can
    give, see UNCOVERED); the envelope built as csrc/surface.hip builds it keeps both, and the far end is served by the second."""
    case = next(c for c in C.GROUPS["carries"] if c.name == "low_y_128")
    ref = C.mask_reference(case)
    b = ref.borders[1]
    D1 = b.shape[1]
    assert D1 == 129
    x, z = 1, 1
    has = b[x].any(axis=1)                                                          # sites of the y lines of plane x
    assert has[:2].all() and not has[2:].any() and b[x, 0, z] and b[x, 1, z]
    s1, s2 = float(case.spacing[1]), float(case.spacing[2])
    v, zb = C.env_build([0.0, 0.0] + [np.inf] * (D1 - 2), s1 * s1)
    assert v == [0, 1] and zb[1] == 0.5
    want = ndi.distance_transform_edt(~b[x], sampling=[s1, s2])
    assert want[D1 - 1, z] == pytest.approx((D1 - 2) * s1, rel=1e-12)


def test_check_ft_accepts_scipy_and_rejects_an_off_by_one():
    case = C.GROUPS["lines"][0]
    ref = C.mask_reference(case)
    b = ref.borders[0]
    D = b.shape
    ft = np.empty(D, np.int64)
    for x in range(D[0]):
        _, (iy, iz) = ndi.distance_transform_edt(~b[x], sampling=case.spacing[1:], return_indices=True)
        ft[x] = iy * D[2] + iz
    assert C.check_ft(ft, b, case.spacing) <= C.REL_DIST
    bad = ft.copy()
    far = np.argwhere(~b)[-1]
    bad[tuple(far)] = np.ravel_multi_index(tuple(np.argwhere(b[far[0]])[0]), D[1:]) if ft[tuple(far)] != np.ravel_multi_index(
        tuple(np.argwhere(b[far[0]])[0]), D[1:]) else np.ravel_multi_index(tuple(np.argwhere(b[far[0]])[-1]), D[1:])
    try:
        err = C.check_ft(bad, b, case.spacing)
    except AssertionError:
        err = 1.0
    assert err > C.REL_DIST


BRUTE_GROUPS = C.MASK_GROUPS + ("labels",)


@pytest.mark.parametrize("group", BRUTE_GROUPS)
def test_reference_agrees_with_brute_force(group):
    """(the stats group has no distances)"""
    refs = []
    if group == "labels":
        for case in C.GROUPS[group]:
            refs += [(case, o.ref) for o in C.label_reference(case, True).values() if o.ref is not None]
    else:
        refs = [(case, C.mask_reference(case)) for case in C.GROUPS[group]]
    done = 0
    for case, ref in refs:
        if ref is None or C.brute_cost(ref) > C.BRUTE_CAP:
            continue
        done += 1
        assert C.rel_err(C.brute_force(ref.borders[0], ref.borders[1], case.spacing), ref.d_gt) <= C.REL_DIST, C.case_id(case)
        assert C.rel_err(C.brute_force(ref.borders[1], ref.borders[0], case.spacing), ref.d_pred) <= C.REL_DIST, C.case_id(case)
    assert done >= 1


@pytest.mark.parametrize("case", C.MASK_CASES, ids=_ids(C.MASK_CASES))
def test_host_distances_match_reference(case):
    g, p = C.masks(case)
    ref = C.mask_reference(case)
    got = surface._host_surface_distances(C.device_form(g, case.form), C.device_form(p, case.form), case.spacing)
    (d_gt, a_gt), (d_pred, a_pred) = C.sort_pairs(ref.d_gt, ref.a_gt), C.sort_pairs(ref.d_pred, ref.a_pred)
    want = dict(zip(KEYS, (d_gt, d_pred, a_gt, a_pred)))
    for k in KEYS:
        assert C.rel_err(got[k], want[k]) <= C.REL_DIST, k
    s = C.reference_stats(g, p, [1])[1].tolist()                                    # a bool mask is label 1; the box is the reference's
    assert s[:2] == [int(g.sum()), int(p.sum())] and s[2:8:2] == list(ref.lo) and s[3:8:2] == [l + k - 1 for l, k in zip(ref.lo, ref.n)]
    for tol in case.tols:
        assert C.tolerance_gap_ok(ref, tol, (3.0,) if case.group == "inclusive_tol" else ()), tol
        a_gt, w_gt, a_pred, w_pred = C._sums(ref, tol)
        with np.errstate(divide="ignore", invalid="ignore"):
            want_nsd = float(np.float64(w_gt + w_pred) / np.float64(a_gt + a_pred))
        assert abs(surface.compute_surface_dice_at_tolerance(got, tol) - want_nsd) <= C.REL_SUM * max(want_nsd, 1e-300)


def test_inclusive_tolerance_is_decided_by_the_reference():
    case = C.GROUPS["inclusive_tol"][0]
    ref = C.mask_reference(case)
    at = float(ref.a_gt[ref.d_gt == 3.0].sum()) + float(ref.a_pred[ref.d_pred == 3.0].sum())
    assert at > 0 and (ref.d_gt == 3.0).sum() >= 64
    hi, lo = C._sums(ref, case.tols[0]), C._sums(ref, case.tols[1])
    assert (hi[1] + hi[3]) - (lo[1] + lo[3]) == pytest.approx(at, rel=1e-12)


@pytest.mark.parametrize("case", C.GROUPS["labels"], ids=_ids(C.GROUPS["labels"]))
def test_host_case_nsd_and_layout_match_reference(case):
    gt, seg = C.volumes(case)
    tol = C.tolerances(case)
    want = C.label_reference(case)
    got = surface._host_case_nsd(gt, seg, case.spacing, tol, case.slabs)
    assert list(got) == list(want)
    for organ, o in want.items():
        C.check_rounded(got[organ], o.nsd)
        if o.ref is not None:
            assert C.tolerance_gap_ok(o.ref, float(tol[organ])), organ
    if case.name == "eight":
        assert [o.fixed for o in want.values()] == [None, None, None, None, 0, 1, None, None]
        assert want["organ8"].nsd == 0.0 and want["organ4"].nsd == 0.0 and 0.0 < want["organ7"].nsd < 1.0
        lo, hi = want["organ7"].zcut
        assert (seg[:, :, :lo] == 7).any() and (seg[:, :, hi:] == 7).any()                   # label voxels the cut must read as 0
    # the crops surface._device_layout makes of the statistics
    labels = list(range(1, len(tol) + 1))
    stats = C.reference_stats(gt, seg, labels).tolist()
    for measure_empty_gt in (False, True):
        want = C.label_reference(case, measure_empty_gt)
        rows, fixed = surface._device_layout(stats, labels, [lab in case.slabs for lab in labels], measure_empty_gt)
        assert fixed == [o.fixed for o in want.values()]
        measured = [o for o in want.values() if o.fixed is None]
        assert len(rows) == len(measured)
        vox = zl = yl = xl = 0
        for row, o in zip(rows, measured):
            lab, lo, n = row[0], row[1:4], row[4:7]
            assert lab == o.label and row[7:11] == [vox, zl, yl, xl] and len(row) == 16
            D = [k + 1 for k in n]
            vox, zl, yl, xl = vox + D[0] * D[1] * D[2], zl + D[0] * D[1], yl + D[0] * D[2], xl + D[1] * D[2]
            rlo = list(o.ref.lo)
            if o.zcut is not None:
                rlo[2] += o.zcut[0]
                s = stats[lab]
                assert lo[2] == max(s[6], o.zcut[0]) and lo[2] + n[2] == min(s[7] + 1, o.zcut[1])     # the cut, within the union
                assert lo[2] >= o.zcut[0] and lo[2] + n[2] <= o.zcut[1]
            else:
                assert lo == rlo and n == list(o.ref.n)
            assert all(a <= b and a + k >= b + m for a, k, b, m in zip(lo, n, rlo, o.ref.n))
            C.embed(o.ref, o.zcut, lo, n)
    if case.name == "eight":
        row7 = next(r for r in rows if r[0] == 7)
        assert (row7[3], row7[3] + row7[6]) == C.label_reference(case)["organ7"].zcut


def test_empty_slab_is_refused():
    gt = np.zeros((10, 10, 8), np.uint8)
    seg = np.zeros_like(gt)
    gt[4, 4, 3] = 1
    seg[4, 4, 3:5] = 1
    with pytest.raises(ValueError, match="empty"):
        C.reference_case(gt, seg, (1, 1, 1), {"a": 1.0}, (1,))
    with pytest.raises(ValueError, match="empty"):
        surface._host_case_nsd(gt, seg, (1, 1, 1), {"a": 1.0}, (1,))
    with pytest.raises(ValueError, match="empty"):
        surface._device_layout(C.reference_stats(gt, seg, [1]).tolist(), [1], [True])


def test_reference_stats_by_hand():
    gt = np.zeros((3, 4, 20), np.uint8)
    seg = np.zeros_like(gt)
    gt[1, 2, 10:18] = 5
    seg[2, 1, 3] = 5
    seg[0, 0, 0] = 9
    s = C.reference_stats(gt, seg, [5, 6])
    assert s[5].tolist() == [8, 1, 1, 2, 1, 2, 3, 17, 10, 17]
    assert s[6].tolist() == s[9].tolist() == [0, 0, C.INT_MAX, -1, C.INT_MAX, -1, C.INT_MAX, -1, C.INT_MAX, -1]
