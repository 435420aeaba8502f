"""K24 (csrc/surface.hip) on the MI355X: compute_surface_distances and case_nsd against tests/golden/surface.npz (the reference's
SurfaceDice.py) and against the host path on a BTCV-sized case; repeatability, untouched inputs, refused sizes."""
import warnings

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import _lib, ops, surface
from tests import _surface_cases as C
from tests.test_surface_cpu import G, KEYS, MASKS, _check_rounded, _close

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name", list(MASKS))
def test_k24_surface_distances_golden(name):
    g, p, s = MASKS[name]
    sd = surface.compute_surface_distances(torch.from_numpy(g).to(DEV), torch.from_numpy(p).to(DEV), s)
    for k in KEYS:
        assert sd[k].is_cuda and sd[k].dtype == torch.float64
        _close(sd[k].cpu().numpy(), G[f"mask/{name}/{k}"], 1e-12)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _close([surface.compute_surface_dice_at_tolerance(sd, t) for t in C.TOLERANCES], G[f"mask/{name}/dice"], 1e-9)
        _close([surface.compute_surface_overlap_at_tolerance(sd, t) for t in C.TOLERANCES], G[f"mask/{name}/overlap"], 1e-9)
        _close(surface.compute_average_surface_distance(sd), G[f"mask/{name}/average"], 1e-9)
        _close([surface.compute_robust_hausdorff(sd, q) for q in C.PERCENTS], G[f"mask/{name}/hausdorff"], 1e-12)


@pytest.mark.parametrize("case", C.label_cases(), ids=lambda c: c[0])
def test_k24_case_nsd_golden(case):
    name, gt, seg, sp, tol, slabs = case
    got = surface.case_nsd(torch.from_numpy(gt).to(DEV), torch.from_numpy(seg).to(DEV), sp, tol, slabs)
    _check_rounded(got, name, tol)
    # the fused sums give the unrounded NSD of the golden
    labels = list(range(1, len(tol) + 1))
    fixed, sums, _, _ = surface._device_run(torch.from_numpy(gt).to(DEV), torch.from_numpy(seg).to(DEV), sp, labels,
                                            [float(t) for t in tol.values()], [lab in slabs for lab in labels])
    sums, k = sums.cpu().numpy(), 0
    for i, f in enumerate(fixed):
        if f is None:
            a_gt, w_gt, a_pred, w_pred = sums[k]
            k += 1
            assert abs((w_gt + w_pred) / (a_gt + a_pred) - G[f"label/{name}/nsd"][i]) < 1e-9


@pytest.fixture(scope="module")
def btcv():
    gt, seg = C.btcv_sized_case()
    return gt, seg, torch.from_numpy(gt).to(DEV), torch.from_numpy(seg).to(DEV)


def test_k24_btcv_sized_against_host(btcv):
    gt, seg, dgt, dseg = btcv
    sp = (np.float32(0.78125), np.float32(0.78125), np.float32(3.0))
    got = surface.case_nsd(dgt, dseg, sp, surface.BTCV_NSD_TOLERANCES, surface.BTCV_SLAB_LABELS)
    want = surface.case_nsd(gt, seg, sp, surface.BTCV_NSD_TOLERANCES, surface.BTCV_SLAB_LABELS)
    assert list(got) == list(want)
    for o in got:
        assert abs(got[o] - want[o]) <= 1e-4 + 1e-12, (o, got[o], want[o])
    # the full dict of the largest organ, device against host
    lab = int(np.argmax(np.bincount(gt.ravel(), minlength=14)[1:])) + 1
    d = surface.compute_surface_distances(dgt == lab, dseg == lab, sp)
    h = surface.compute_surface_distances(gt == lab, seg == lab, sp)
    for k in KEYS:
        _close(d[k].cpu().numpy(), h[k], 1e-12)


def test_k24_bit_identical_and_inputs_untouched(btcv):
    _, _, dgt, dseg = btcv
    g0, s0 = dgt.clone(), dseg.clone()
    sp = (0.78125, 0.78125, 3.0)
    labels = list(range(1, 14))
    run = lambda: surface._device_run(dgt, dseg, sp, labels, [3.0] * 13, [lab in (5, 8, 9) for lab in labels])[1]  # noqa: E731
    a, b = run(), run()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(dgt, g0) and torch.equal(dseg, s0)


def test_k24_size_limits_refused():
    lib = _lib.lib()
    # the C entry refuses a crop over 2^31 - 1 voxels before any launch (every pointer is a dummy: nothing may run)
    dummy = torch.zeros(64, dtype=torch.int64, device=DEV)
    p = dummy.data_ptr()
    rc = lib.mlagg_surface_prepare(p, p, 4, 4, 4, p, 1, 2 ** 31, 2 ** 31, 16, 16, 4, 1.0, 1.0, p, p, p, ops._stream())
    assert rc == -1
    rc = lib.mlagg_surface_prepare(p, p, 4, 4, 4, p, 1, 64, 64, 16, 16, ops.SURFACE_MAX_LINE + 1, 1.0, 1.0, p, p, p, ops._stream())
    assert rc == -1
    rc = lib.mlagg_surface_reduce(p, p, p, 1, 64, 16, ops.SURFACE_MAX_LINE + 1, p, p, 1.0, 1.0, 1.0, p, p, None, None, ops._stream())
    assert rc == -1
    # the wrapper refuses a layout with a crop of 1301^3 > 2^31 - 1 voxels
    gt = torch.zeros((2, 2, 2), dtype=torch.uint8, device=DEV)
    desc = torch.tensor([[1, 0, 0, 0, 1300, 1300, 1300, 0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="2147483647"):
        ops.surface_prepare(gt, gt, desc, (1, 1, 1))
    desc = torch.tensor([[1, 0, 0, 0, 1, 1, ops.SURFACE_MAX_LINE, 0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="crop axis"):
        ops.surface_prepare(gt, gt, desc, (1, 1, 1))


def test_k24_empty_slab_refused():
    gt = torch.zeros((10, 10, 8), dtype=torch.uint8, device=DEV)
    gt[4, 4, 3] = 5
    with pytest.raises(ValueError, match="empty"):
        surface.case_nsd(gt, gt.clone(), (1, 1, 1), surface.BTCV_NSD_TOLERANCES, surface.BTCV_SLAB_LABELS)
