"""NSD on the host: the constructed surfel area table, compute_surface_distances, the four metrics and case_nsd against
tests/golden/surface.npz (the reference's own SurfaceDice.py)."""
import math
import warnings

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import evaluation, surface
from tests import _surface_cases as C

G = np.load(C.golden_path())
MASKS = {name: (g, p, s) for name, g, p, s in C.mask_cases()}
KEYS = ("distances_gt_to_pred", "distances_pred_to_gt", "surfel_areas_gt", "surfel_areas_pred")


def _close(got, want, rel):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=rel, atol=0)
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)])


@pytest.mark.parametrize("i", range(len(C.AREA_SPACINGS)))
def test_area_table_matches_reference(i):
    got = surface.surface_area_table(C.AREA_SPACINGS[i])
    assert got.shape == (256,) and got.dtype == np.float64
    np.testing.assert_allclose(got, G[f"area/{i}"], rtol=1e-12, atol=1e-12)


def test_area_table_symmetries():
    """a code and its complement have the same area; codes 0 and 255 have none"""
    t = surface.surface_area_table((0.3, 2.9, 1.7))
    assert t[0] == 0 and t[255] == 0
    np.testing.assert_allclose(t, t[::-1], rtol=1e-14)


@pytest.mark.parametrize("name", list(MASKS))
def test_compute_surface_distances_host(name):
    g, p, s = MASKS[name]
    sd = surface.compute_surface_distances(g, p, s)
    for k in KEYS:
        _close(sd[k], G[f"mask/{name}/{k}"], 1e-12)


@pytest.mark.parametrize("name", list(MASKS))
def test_metrics_host(name):
    g, p, s = MASKS[name]
    sd = surface.compute_surface_distances(torch.from_numpy(g), torch.from_numpy(p), s)      # CPU tensors: the host path
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _close([surface.compute_surface_dice_at_tolerance(sd, t) for t in C.TOLERANCES], G[f"mask/{name}/dice"], 1e-9)
        _close([surface.compute_surface_overlap_at_tolerance(sd, t) for t in C.TOLERANCES], G[f"mask/{name}/overlap"], 1e-9)
        _close(surface.compute_average_surface_distance(sd), G[f"mask/{name}/average"], 1e-9)
        _close([surface.compute_robust_hausdorff(sd, q) for q in C.PERCENTS], G[f"mask/{name}/hausdorff"], 1e-12)


def _check_rounded(got, name, organs):
    nsd, rounded = G[f"label/{name}/nsd"], G[f"label/{name}/nsd_rounded"]
    assert list(got) == list(organs)
    for v, exact, want in zip(got.values(), nsd, rounded):
        near_boundary = abs((exact * 1e4) % 1 - 0.5) < 1e-5
        if not near_boundary:
            assert v == want, (name, got, rounded)
        else:
            assert abs(v - want) <= 1e-4 + 1e-12


@pytest.mark.parametrize("case", C.label_cases(), ids=lambda c: c[0])
def test_case_nsd_host(case):
    name, gt, seg, sp, tol, slabs = case
    _check_rounded(surface.case_nsd(gt, seg, sp, tol, slabs), name, tol)


def test_case_nsd_empty_slab_is_refused_host():
    gt = np.zeros((10, 10, 8), np.uint8)
    seg = np.zeros_like(gt)
    gt[4, 4, 3] = 5
    seg[4, 4, 3:5] = 5
    with pytest.raises(ValueError, match="empty"):
        surface.case_nsd(gt, seg, (1, 1, 1), surface.BTCV_NSD_TOLERANCES, surface.BTCV_SLAB_LABELS)


def test_presets_and_mean():
    assert list(surface.BTCV_NSD_TOLERANCES) == list(surface.BTCV_ORGANS) and len(surface.BTCV_ORGANS) == 13
    assert surface.BTCV_SLAB_LABELS == (5, 8, 9)
    assert [surface.BTCV_ORGANS[i - 1] for i in surface.BTCV_SLAB_LABELS] == ["Esophagus", "Aorta", "IVC"]
    assert list(surface.ABDOMEN_NSD_TOLERANCES) == list(evaluation.ABDOMEN_ORGANS)
    assert [surface.ABDOMEN_NSD_TOLERANCES[o] for o in ("Liver", "Duodenum", "Aorta")] == [5, 7, 2]
    assert list(surface.ACDC_NSD_TOLERANCES.values()) == [3, 3, 3]
    cols, mean = surface.mean_nsd([{"a": 1.0, "b": 0.5}, {"a": 0.5, "b": float("nan")}])
    assert cols == {"a": 0.75, "b": 0.5} and mean == 0.625


def test_empty_dict_metrics():
    sd = surface.compute_surface_distances(np.zeros((4, 4, 4), bool), np.zeros((4, 4, 4), bool), (1, 1, 1))
    assert all(len(sd[k]) == 0 for k in KEYS)
    assert math.isinf(surface.compute_robust_hausdorff(sd, 95))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert math.isnan(surface.compute_surface_dice_at_tolerance(sd, 1.0))
