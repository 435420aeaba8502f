"""GPU: K24 (csrc/surface.hip) against the references of tests/_surface_path_cases.py at the sizes where its launchers and loops
change path (tests/test_surface_paths_cpu.py shows which case enters which path).  Statistics, neighbour codes and surfel counts are
compared exactly, the feature transform after the z and y passes plane by plane, the distance lists and pair slices to 1e-12, the
sums and their ratios to 1e-9, the rounded NSD with the host test's rule.  Every test prints the errors it measured."""
import warnings

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import ops, surface
from tests import _surface_path_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("distances_gt_to_pred", "distances_pred_to_gt", "surfel_areas_gt", "surfel_areas_pred")


def _ids(cases):
    return [C.case_id(c) for c in cases]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a copy: the cases are read-only)


def _bound(case, quantity, default):
    return C.EXCEPTIONS.get((case, quantity), default)


def _stats(gt, seg, wanted):
    w = torch.zeros(256, dtype=torch.uint8)
    w[list(wanted)] = 1
    got = ops.surface_stats(gt, seg, w.to(DEV)).cpu().numpy()
    return got


def _check_prepare(case, gt, seg, rows, organs):
    """codes, counts and the packed feature transform of every crop of `rows` against the references `organs` (Ref, zcut)."""
    desc = torch.tensor(rows, dtype=torch.int64)
    codes, ft, counts, _, layout = ops.surface_prepare(gt, seg, desc, [float(v) for v in case.spacing])
    total = layout["total"]
    codes, ft, counts = codes.cpu().numpy().reshape(2, total), ft.cpu().numpy().reshape(2, total), counts.cpu().numpy()
    worst = 0.0
    for i, (row, (ref, zcut)) in enumerate(zip(rows, organs)):
        lo, n, vox = row[1:4], row[4:7], row[7]
        D = tuple(k + 1 for k in n)
        want_codes, borders = C.embed(ref, zcut, lo, n)
        nv = D[0] * D[1] * D[2]
        for m in (0, 1):
            assert np.array_equal(codes[m, vox:vox + nv].reshape(D), want_codes[m]), (C.case_id(case), row[0], "codes", m)
            assert int(counts[i, m]) == int(borders[m].sum()) == int(ref.borders[m].sum()), (C.case_id(case), row[0], "counts", m)
            worst = max(worst, C.check_ft(ft[m, vox:vox + nv], borders[m], case.spacing))
    print(f"{C.case_id(case)} ft in-plane distance: error {worst:.2e}")
    assert worst <= _bound(case, "ft", C.REL_DIST)


def _check_sums(case, got, want, what):
    """four sums and the two within / area ratios, 1e-9 relative; a zero must be a zero"""
    worst = C.rel_err(got, want)
    for a, w in ((0, 1), (2, 3)):
        if want[a] > 0:
            worst = max(worst, C.rel_err([got[w] / got[a]], [want[w] / want[a]]))
    print(f"{C.case_id(case)} {what} sums: error {worst:.2e}")
    assert worst <= _bound(case, "sums", C.REL_SUM), (what, got, want)


@pytest.mark.parametrize("case", C.GROUPS["stats"], ids=_ids(C.GROUPS["stats"]))
def test_stats_paths_are_exact(case):
    gt, seg = C.volumes(case)
    got = _stats(_dev(gt), _dev(seg), case.wanted)
    want = C.reference_stats(gt, seg, case.wanted)
    assert got.shape == (256, 10)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(l), int(s), int(got[l, s]), int(want[l, s])) for l, s in bad[:8]]


@pytest.mark.parametrize("case", C.MASK_CASES, ids=_ids(C.MASK_CASES))
def test_mask_paths_match_reference(case):
    g, p = C.masks(case)
    ref = C.mask_reference(case)
    g8, p8 = _dev(g.astype(np.uint8)), _dev(p.astype(np.uint8))
    # statistics and the prepared state of the one-label call
    stats = _stats(g8, p8, [1])
    assert np.array_equal(stats, C.reference_stats(g, p, [1]))
    rows, fixed = surface._device_layout(stats.tolist(), [1], [False], measure_empty_gt=True)
    assert fixed == [None] and rows[0][1:7] == [*ref.lo, *ref.n]
    _check_prepare(case, g8, p8, rows, [(ref, None)])
    # the dict, from the masks in the case's form
    fg, fp = _dev(C.device_form(g, case.form)), _dev(C.device_form(p, case.form))
    if case.form == "view":                                     # every second plane of a volume twice as long: non-contiguous
        wide_g, wide_p = torch.zeros((*g.shape[:2], 2 * g.shape[2]), dtype=torch.uint8, device=DEV), None
        wide_p = torch.ones_like(wide_g)
        wide_g[:, :, ::2], wide_p[:, :, ::2] = fg, fp
        fg, fp = wide_g[:, :, ::2], wide_p[:, :, ::2]
        assert not fg.is_contiguous() and not fp.is_contiguous()
    sd = surface.compute_surface_distances(fg, fp, case.spacing)
    (d_gt, a_gt), (d_pred, a_pred) = C.sort_pairs(ref.d_gt, ref.a_gt), C.sort_pairs(ref.d_pred, ref.a_pred)
    worst = 0.0
    for k, want in zip(KEYS, (d_gt, d_pred, a_gt, a_pred)):
        assert sd[k].is_cuda and sd[k].dtype == torch.float64
        worst = max(worst, C.rel_err(sd[k].cpu().numpy(), want))
    print(f"{C.case_id(case)} distances and areas: error {worst:.2e}")
    assert worst <= _bound(case, "distances", C.REL_DIST)
    # the fused sums and the rounded NSD at every tolerance
    within = []
    for tol in case.tols:
        want = C._sums(ref, tol)
        fixed, sums, _, _ = surface._device_run(g8, p8, case.spacing, [1], [float(tol)], [False])
        with np.errstate(divide="ignore", invalid="ignore"):
            nsd = float(np.float64(want[1] + want[3]) / np.float64(want[0] + want[2]))
        got = surface.case_nsd(g8, p8, case.spacing, {"organ": tol})
        if not g.any():
            assert fixed == [0] and sums is None and got == {"organ": 0}
            continue
        assert fixed == [None]
        sums = sums.cpu().numpy()[0]
        _check_sums(case, sums, want, f"tol {tol!r}")
        within.append(sums[1] + sums[3])
        C.check_rounded(got["organ"], nsd)
    if case.group == "inclusive_tol":                            # d == tol counts, the next double below does not
        at = float(ref.a_gt[ref.d_gt == case.tols[0]].sum()) + float(ref.a_pred[ref.d_pred == case.tols[0]].sum())
        assert at > 0 and C.rel_err([within[0] - within[1]], [at]) <= C.REL_SUM, (within, at)


@pytest.mark.parametrize("case", C.GROUPS["labels"], ids=_ids(C.GROUPS["labels"]))
def test_label_paths_match_reference(case):
    gt, seg = C.volumes(case)
    dgt, dseg = _dev(gt), _dev(seg)
    tol = C.tolerances(case)
    labels = list(range(1, len(tol) + 1))
    slabs = [lab in case.slabs for lab in labels]
    tols = [float(t) for t in tol.values()]
    stats = _stats(dgt, dseg, labels)
    assert np.array_equal(stats, C.reference_stats(gt, seg, labels))
    for pairs in (False, True):
        want = C.label_reference(case, measure_empty_gt=pairs)
        measured = [o for o in want.values() if o.fixed is None]
        rows, fixed = surface._device_layout(stats.tolist(), labels, slabs, measure_empty_gt=pairs)
        assert fixed == [o.fixed for o in want.values()]
        _check_prepare(case, dgt, dseg, rows, [(o.ref, o.zcut) for o in measured])
        fixed, sums, plist, counts = surface._device_run(dgt, dseg, case.spacing, labels, tols, slabs, pairs=pairs)
        assert fixed == [o.fixed for o in want.values()]
        sums = sums.cpu().numpy()
        assert sums.shape == (len(measured), 4)
        for k, o in enumerate(measured):
            _check_sums(case, sums[k], o.sums, f"label {o.label} pairs={pairs}")
        if not pairs:
            continue
        counts = counts.numpy()
        assert counts.tolist() == [[int(o.ref.borders[0].sum()), int(o.ref.borders[1].sum())] for o in measured]
        assert plist.shape == (int(counts.sum()), 2)
        at, worst = 0, 0.0
        for k, o in enumerate(measured):                         # label k's slices: its gt surfels, then its prediction's
            for m, (d, a) in enumerate(((o.ref.d_gt, o.ref.a_gt), (o.ref.d_pred, o.ref.a_pred))):
                part = plist[at:at + int(counts[k, m])]
                at += int(counts[k, m])
                gd, ga = surface._device_sort(part[:, 0], part[:, 1])
                wd, wa = C.sort_pairs(d, a)
                worst = max(worst, C.rel_err(gd.cpu().numpy(), wd), C.rel_err(ga.cpu().numpy(), wa))
        print(f"{C.case_id(case)} pair slices: error {worst:.2e}")
        assert worst <= _bound(case, "pairs", C.REL_DIST)
    got = surface.case_nsd(dgt, dseg, case.spacing, tol, case.slabs)
    want = C.label_reference(case)
    assert list(got) == list(want)
    for organ, o in want.items():
        C.check_rounded(got[organ], o.nsd)


def test_lines_of_length_one():
    """Crops with D = 1 on an axis (no mask voxel inside) next to an ordinary one, through ops.surface_prepare / surface_reduce: zero
    codes, no feature, zero sums; the ordinary crop last in the list is the reference's."""
    vol = np.zeros((8, 8, 8), np.uint8)
    vol[3:5, 3:5, 3:5] = 1
    seg = np.zeros_like(vol)
    seg[3:5, 3:5, 4:5] = 1
    rows = C.raw_desc()
    spacing = C.ANISO
    ref = C.reference(vol, seg, spacing)
    assert (ref.lo, ref.n) == C.RAW_CROPS[-1]
    dvol, dseg = _dev(vol), _dev(seg)
    state = ops.surface_prepare(dvol, dseg, torch.tensor(rows, dtype=torch.int64), list(spacing))
    codes, ft, counts, _, layout = state
    total = layout["total"]
    first = rows[-1][7]
    assert not codes.view(2, total)[:, :first].any() and bool((ft.view(2, total)[:, :first] == -1).all())
    assert counts.cpu().tolist() == [[0, 0]] * (len(rows) - 1) + [[int(ref.borders[0].sum()), int(ref.borders[1].sum())]]
    D = tuple(k + 1 for k in ref.n)
    for m in (0, 1):
        assert np.array_equal(codes.view(2, total)[m, first:].cpu().numpy().reshape(D), ref.codes[m])
        assert C.check_ft(ft.view(2, total)[m, first:].cpu().numpy(), ref.borders[m], spacing) <= C.REL_DIST
    tol = torch.full((len(rows),), 1.0, dtype=torch.float64, device=DEV)
    area = torch.from_numpy(C.area_table(spacing)).to(DEV)
    sums, _ = ops.surface_reduce(state, tol, area, list(spacing))
    sums = sums.cpu().numpy()
    assert not sums[:-1].any()
    assert C.rel_err(sums[-1], C._sums(ref, 1.0)) <= C.REL_SUM


def test_empty_slab_is_refused_on_the_device():
    gt = torch.zeros((10, 10, 8), dtype=torch.uint8, device=DEV)
    gt[4, 4, 3] = 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="empty"):
            surface.case_nsd(gt, gt.clone(), (1, 1, 1), {"a": 1.0}, (1,))
