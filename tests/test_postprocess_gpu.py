"""Keep-largest-component postprocessing on the device (K23, csrc/components.hip, behind mlagg_unet_amd.postprocessing): fixture
parity with the reference (tests/golden/postprocess.npz) in both group modes, a synthetic BTCV-sized prediction against the host
path, union-find shapes that cross every tile, the size limit, and determine_postprocessing on device tensors."""
import json
import os

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import _lib, ops
from mlagg_unet_amd import postprocessing as PP
from tests import _postprocess_cases as C
from tests.test_postprocess_cpu import cv_inputs, reference_json

gpu = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "postprocess.npz"))


def _device_and_host(x, groups, background_label=0):
    """K23 and the host path on the same volume and group map; returns (device result, stats) as numpy, host result"""
    d = torch.from_numpy(x).to(DEV)
    got, stats = PP._keep_largest_device(d, groups, background_label)
    assert torch.equal(d.cpu(), torch.from_numpy(x))                     # the input is not modified
    return got.cpu().numpy(), stats.cpu().numpy(), PP._keep_largest_host(x, groups, background_label)


def _check_stats(x, out, stats, groups):
    """stats rows: voxels per group, largest component, voxels kept"""
    table = np.zeros(256, np.int64)
    for label, g in groups.items():
        table[label] = g
    gx, go = table[x], table[out]
    for g in set(groups.values()):
        assert stats[0, g] == (gx == g).sum()
        assert stats[2, g] == ((gx == g) & (out == x) & (go == g)).sum()


@gpu
@pytest.mark.parametrize("tag", sorted(C.CALLS))
def test_device_matches_the_reference(tag):
    vol, lr, bg, _ = C.CALLS[tag]
    x = GOLDEN[f"{vol}/input"]
    d = torch.from_numpy(x).to(DEV)
    got = PP.remove_all_but_largest_component_from_segmentation(d, lr, background_label=bg)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == x.shape
    assert np.array_equal(got.cpu().numpy(), GOLDEN[f"{tag}/output"])
    assert np.array_equal(d.cpu().numpy(), x)


@gpu
@pytest.mark.parametrize("tag", sorted(C.VOLUMES))
def test_device_per_class_mode_matches_the_reference_chain(tag):
    x = GOLDEN[f"{tag}/input"]
    groups = {label: label for label in GOLDEN[f"{tag}/per_class_labels"].tolist()}
    got, stats, host = _device_and_host(x, groups)
    assert np.array_equal(got, GOLDEN[f"{tag}/per_class"]) and np.array_equal(got, host)
    _check_stats(x, got, stats, groups)


@gpu
def test_device_accepts_other_integer_dtypes_and_2d():
    x = GOLDEN["multi/input"]
    got = PP.remove_all_but_largest_component_from_segmentation(torch.from_numpy(x.astype(np.int64)).to(DEV), [1, 2, 3, 4])
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), GOLDEN["multi_fg/output"])
    y = torch.from_numpy(GOLDEN["two_d/input"][0]).to(DEV)
    assert np.array_equal(PP.remove_all_but_largest_component_from_segmentation(y, [1, 2]).cpu().numpy(),
                          GOLDEN["two_d_fg/output"][0])


@gpu
def test_synthetic_btcv_volume_matches_the_host_path():
    x = C.btcv_like()
    assert x.shape == (512, 512, 150)
    groups_fg = {label: 1 for label in range(1, 14)}
    got, stats, host = _device_and_host(x, groups_fg)
    assert np.array_equal(got, host)
    _check_stats(x, got, stats, groups_fg)
    groups = {label: label for label in range(1, 15)}
    got, stats, host = _device_and_host(x, groups)
    assert np.array_equal(got, host)
    _check_stats(x, got, stats, groups)
    assert stats[1, 14] == 35 and stats[2, 14] == 70                    # the tie of label 14: both 35-voxel components kept
    assert (got != x).any()


def _serpentine(shape):
    """one path that sweeps every (x, y) row of the volume in turn: z-runs on even (x, y), joined alternately at the two z ends"""
    X, Y, Z = shape
    v = np.zeros(shape, np.uint8)
    k = 0
    prev = None
    for x in range(0, X, 2):
        ys = list(range(0, Y, 2))
        if (x // 2) % 2:
            ys.reverse()
        for y in ys:
            v[x, y, :] = 1
            end = Z - 1 if k % 2 == 0 else 0
            if prev is not None:
                px, py, pend = prev
                v[min(px, x):max(px, x) + 1, min(py, y):max(py, y) + 1, pend] = 1
            prev = (x, y, end)
            k += 1
    return v


@gpu
@pytest.mark.parametrize("shape", [(21, 37, 70), (18, 26, 64)])
def test_serpentine_component_crossing_every_tile(shape):
    v = _serpentine(shape)
    single = PP._keep_largest_host(v, {1: 1}, 0)
    assert np.array_equal(single, v)                                     # one component
    x = v.copy()
    x[1::2, 1::2, 1::2] = np.where(x[1::2, 1::2, 1::2] == 0, 2, x[1::2, 1::2, 1::2])   # a second label woven through it
    for groups in ({1: 1}, {1: 1, 2: 1}, {1: 1, 2: 2}):
        got, stats, host = _device_and_host(x, groups)
        assert np.array_equal(got, host)
    got, _, _ = _device_and_host(v, {1: 1})
    assert np.array_equal(got, v)


@gpu
def test_k23_and_k30_run_one_labelling():
    """both callers of csrc/cc_label.h on the same (10, 17, 70) masks: the largest component's size"""
    from scipy import ndimage as ndi
    from tests import _cascade_cases as K
    for mask in K.component_planes():
        v = mask.astype(np.uint8)
        got, stats, host = _device_and_host(v, {1: 1})
        assert np.array_equal(got, host)
        planes = ops.cascade_pack(torch.from_numpy(v.astype(np.int16)).to(DEV)[None], [1])[0]
        (parent, size, _, _), _ = ops.cascade_cc_stats(planes, v.shape[2], 0.0)
        parent, size = parent[0].cpu().numpy(), size[0].cpu().numpy()
        lab, _ = ndi.label(mask, structure=np.ones((3, 3, 3)))
        largest = np.bincount(lab.ravel())[1:].max()
        assert stats[1, 1] == largest and size[parent == np.arange(parent.size)].max() == largest


@gpu
@pytest.mark.parametrize("shape", [(33, 40, 68), (30, 17, 45)])
def test_lattice_connected_only_through_corners(shape):
    i, j, k = np.indices(shape)
    v = ((i % 2 == j % 2) & (j % 2 == k % 2)).astype(np.uint8)          # all-even or all-odd: only corner contacts
    v[:, :, -8:] = 0
    v[2:6, 2:6, -5:-1] = 1                                                # a 64-voxel block, separated by three empty planes
    got, stats, host = _device_and_host(v, {1: 1})
    assert np.array_equal(got, host)
    assert got[2, 2, -5] == 0 and stats[1, 1] == int(v[:, :, :-8].sum())


@gpu
@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("shape", [(9, 70, 33), (16, 16, 64)])
def test_all_ones_and_all_zeros(fill, shape):
    v = np.full(shape, fill, np.uint8)
    got, stats, host = _device_and_host(v, {1: 1})
    assert np.array_equal(got, v) and np.array_equal(host, v)
    assert stats[0, 1] == v.sum() and stats[1, 1] == v.sum() and stats[2, 1] == v.sum()


@gpu
def test_more_than_2_31_voxels_is_refused_before_any_launch():
    big = (2048, 1024, 1024)
    rc = _lib.lib().mlagg_keep_largest_component(None, *big, None, 0, None, None, None, None, None)
    assert rc == -1                                                       # MLAGG_E_UNSUPPORTED: checked before the pointers
    view = torch.zeros(1, dtype=torch.uint8, device=DEV).expand(*big)
    with pytest.raises(RuntimeError, match="at most"):
        ops.keep_largest_component(view, torch.zeros(256, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="at most"):
        PP.remove_all_but_largest_component_from_segmentation(view, 1)


@gpu
@pytest.mark.parametrize("tag", sorted(C.CV_SETS))
def test_determine_postprocessing_on_the_device_matches_the_reference(tag):
    preds, refs, labels, ignore = cv_inputs(tag)
    dp = [torch.from_numpy(p).to(DEV) for p in preds]
    dr = [torch.from_numpy(r).to(DEV) for r in refs]
    fns, kwargs, summary = PP.determine_postprocessing(dp, dr, labels, ignore_label=ignore)
    assert json.dumps(summary, sort_keys=True) == json.dumps(reference_json(tag), sort_keys=True)
    for i, p in enumerate(dp):
        out = PP.apply_postprocessing(p, fns, kwargs)
        assert out.is_cuda and np.array_equal(out.cpu().numpy(), GOLDEN[f"cv/{tag}/pp_{i}"])
