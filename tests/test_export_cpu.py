"""Prediction export, host side (mlagg_unet_amd.export): the per-axis tap tables against scipy in float64, the separate-z decision
and the host path against the reference's own export_prediction_from_softmax (tests/golden/export.npz, made by
tests/golden/make_golden_export.py), the drop-in's files, and the errors."""
import os
import pickle
import types
import warnings

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import export as E
from tests import _export_cases as C

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "export.npz"))
AXES = ((5, 9), (9, 5), (7, 7), (1, 4), (4, 1), (13, 20), (20, 13), (3, 8), (48, 17), (10, 14), (320, 512))


def _zoom(a, shape):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ndi.zoom(a, np.asarray(shape, float) / np.asarray(a.shape, float), order=1, mode="nearest", grid_mode=True)


def _blend(a, taps):
    idx, w = taps
    return a[idx[:, 0]] * w[:, 0] + a[idx[:, 1]] * w[:, 1]


def _ulps(a, b):
    a, b = torch.as_tensor(a).contiguous(), torch.as_tensor(b).contiguous()
    return int((a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max())


@pytest.mark.parametrize("n_in,n_out", AXES)
def test_axis_tables_match_scipy_in_float64(n_in, n_out):
    a = np.random.default_rng(n_in * 1000 + n_out).standard_normal(n_in)
    assert np.abs(_blend(a, E._axis_taps(n_in, n_out, "linear")) - _zoom(a, (n_out,))).max() <= 1e-12
    c = float(n_in) / n_out * (np.arange(n_out) + 0.5) - 0.5
    assert np.array_equal(_blend(a, E._axis_taps(n_in, n_out, "nearest")), ndi.map_coordinates(a, c[None], order=0, mode="nearest"))
    assert np.abs(_blend(a, E._axis_taps(n_in, n_out, "linear")) - ndi.map_coordinates(a, c[None], order=1, mode="nearest")).max() <= 1e-12


def test_order0_exact_halves():
    # n_in = 2 n_out puts every coordinate on a half: c = 2 o + 0.5 (0.5 -> 1, 2.5 -> 3); 3 -> 6 gives -0.25 (-> 0) at o = 0
    for n_in, n_out in ((3, 6), (2, 8), (8, 4), (6, 3), (5, 2), (6, 4), (1, 3)):
        a = np.arange(n_in, dtype=float) * 10 + 1
        c = float(n_in) / n_out * (np.arange(n_out) + 0.5) - 0.5
        assert np.array_equal(_blend(a, E._axis_taps(n_in, n_out, "nearest")), ndi.map_coordinates(a, c[None], order=0, mode="nearest"))
    idx, w = E._axis_taps(8, 4, "nearest")
    assert idx[:, 0].tolist() == [1, 3, 5, 7] and idx[:, 1].tolist() == [1, 3, 5, 7] and w[:, 1].tolist() == [0.0] * 4
    assert E._axis_taps(3, 6, "nearest")[0][0, 0] == 0


def test_3d_tables_match_scipy_zoom():
    x = np.random.default_rng(3).standard_normal((11, 14, 9))
    for new in ((17, 6, 9), (5, 20, 13), (11, 14, 9)):
        idx, w = E.build_taps(x.shape, new, ("linear",) * 3)
        n0, n1 = new[0], new[0] + new[1]
        t = [(idx[:n0], w[:n0]), (idx[n0:n1], w[n0:n1]), (idx[n1:], w[n1:])]
        got = np.apply_along_axis(_blend, 2, x, t[2])
        got = np.apply_along_axis(_blend, 1, got, t[1])
        got = np.apply_along_axis(_blend, 0, got, t[0])
        assert np.abs(got - _zoom(x, new)).max() <= 1e-12


@pytest.mark.parametrize("tag", sorted(C.CASES))
def test_separate_z_decision_matches_the_reference(tag):
    K, shape, cfg, spacing, _, _, crop, _, _ = C.CASES[tag]
    cur = E.current_spacing_for(cfg, C.properties(tag))
    sep, axis = E.separate_z_decision(cur, spacing)
    assert (int(sep), -1 if axis is None else axis) == tuple(GOLDEN[f"{tag}/separate_z"])


def _scipy_resample(x, new_shape, cur, new, order_z=0):
    """resample_data_or_seg_to_shape(is_seg=False, order=1) restated with scipy in float64 (the fixture checks the reference)."""
    sep, axis = E.separate_z_decision(cur, new)
    x = x.astype(np.float64)
    if tuple(x.shape[1:]) == tuple(new_shape):
        return x.astype(np.float32)
    out = []
    for c in range(x.shape[0]):
        if not sep:
            out.append(_zoom(x[c], new_shape))
            continue
        plane = [s for a, s in enumerate(new_shape) if a != axis]
        r = np.stack([_zoom(np.take(x[c], i, axis), plane) for i in range(x.shape[1 + axis])], axis)
        if r.shape[axis] != new_shape[axis]:
            grid = np.mgrid[tuple(slice(0, s) for s in new_shape)].astype(np.float64)
            grid = [float(r.shape[a]) / new_shape[a] * (grid[a] + 0.5) - 0.5 for a in range(3)]
            r = ndi.map_coordinates(r, np.array(grid), order=order_z, mode="nearest")
        out.append(r)
    return np.stack(out).astype(np.float32)


@pytest.mark.parametrize("tag", sorted(C.CASES))
def test_host_resampling_matches_float64_scipy(tag):
    K, shape, cfg, spacing, _, _, crop, _, _ = C.CASES[tag]
    x = GOLDEN[f"{tag}/logits"]
    cur = E.current_spacing_for(cfg, C.properties(tag))
    got = E.resample_logits_to_shape(torch.from_numpy(x), crop, cur, spacing)
    assert got.dtype == torch.float32 and tuple(got.shape) == (K,) + crop
    assert _ulps(got, torch.from_numpy(_scipy_resample(x, crop, cur, spacing))) <= 1


def test_order_z1_matches_the_reference():
    K, shape, new_shape, cur, new = C.ORDER_Z1
    got = E.resample_logits_to_shape(GOLDEN["order_z1/logits"], new_shape, cur, new, order_z=1)
    assert _ulps(got, torch.from_numpy(GOLDEN["order_z1/resampled"])) <= 1


@pytest.mark.parametrize("tag", sorted(C.CASES))
@pytest.mark.parametrize("as_numpy", [False, True])
def test_host_export_matches_the_reference(tag, as_numpy):
    K, shape, cfg, _, full, lo, crop, tb, _ = C.CASES[tag]
    x = GOLDEN[f"{tag}/logits"]
    seg, probs = E.convert_predicted_logits_to_segmentation_with_correct_shape(
        x if as_numpy else torch.from_numpy(x), C.properties(tag), cfg, tb, return_probabilities=True)
    want_seg, want_p = GOLDEN[f"{tag}/segmentation"], GOLDEN[f"{tag}/probabilities"]
    assert seg.dtype == torch.uint8 and seg.is_contiguous() and tuple(seg.shape) == want_seg.shape
    assert torch.equal(seg, torch.from_numpy(want_seg))
    assert tuple(probs.shape) == want_p.shape and float((probs - torch.from_numpy(want_p)).abs().max()) <= 1e-6
    seg2, none = E.convert_predicted_logits_to_segmentation_with_correct_shape(torch.from_numpy(x), C.properties(tag), cfg, tb)
    assert none is None and torch.equal(seg2, seg)


def test_host_export_accepts_a_non_contiguous_view():
    tag = "b_separate_z"
    K, shape, cfg, _, _, _, _, tb, _ = C.CASES[tag]
    x = torch.from_numpy(GOLDEN[f"{tag}/logits"])
    view = x.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)          # the 2-D sliding window's (K, D, X, Y) view layout
    assert not view.is_contiguous()
    seg, _ = E.convert_predicted_logits_to_segmentation_with_correct_shape(view, C.properties(tag), cfg, tb)
    assert torch.equal(seg, torch.from_numpy(GOLDEN[f"{tag}/segmentation"]))


class _Writer:
    written = {}

    def write_seg(self, seg, output_fname, properties):
        _Writer.written[output_fname] = np.array(seg)


def _managers(tag, regions=False):
    K, _, cfg, _, _, _, _, tb, _ = C.CASES[tag]
    label_manager = types.SimpleNamespace(has_regions=regions)
    plans = types.SimpleNamespace(transpose_backward=list(tb), image_reader_writer_class=_Writer,
                                  get_label_manager=lambda dj: label_manager)
    return types.SimpleNamespace(spacing=list(cfg)), plans


@pytest.mark.parametrize("tag", ["b_separate_z", "g_unchanged"])
@pytest.mark.parametrize("source", ["array", "npy", "npz"])
def test_drop_in_writes_the_reference_files(tag, source, tmp_path):
    K = C.CASES[tag][0]
    x = GOLDEN[f"{tag}/logits"]
    props = C.properties(tag)
    cfg, plans = _managers(tag)
    arg = x
    if source == "npy":
        arg = str(tmp_path / "logits.npy")
        np.save(arg, x)
    elif source == "npz":
        arg = str(tmp_path / "logits.npz")
        np.savez(arg, softmax=x)
    trunc = str(tmp_path / "case")
    E.export_prediction_from_softmax(arg, props, cfg, plans, C.dataset_json(K), trunc, save_probabilities=True)
    if source != "array":
        assert not os.path.exists(arg)                                         # the reference removes the file it loaded
    assert np.array_equal(_Writer.written[trunc + ".nii.gz"], GOLDEN[f"{tag}/segmentation"])
    p = np.load(trunc + ".npz")["probabilities"]
    assert p.dtype == np.float32 and np.abs(p - GOLDEN[f"{tag}/probabilities"]).max() <= 1e-6
    with open(trunc + ".pkl", "rb") as f:
        assert pickle.load(f) == props
    trunc2 = str(tmp_path / "labels_only")
    E.export_prediction_from_softmax(x, props, cfg, plans, C.dataset_json(K), trunc2)
    assert not os.path.exists(trunc2 + ".npz") and not os.path.exists(trunc2 + ".pkl")
    assert np.array_equal(_Writer.written[trunc2 + ".nii.gz"], GOLDEN[f"{tag}/segmentation"])


def test_errors():
    tag = "a_isotropic"
    K, _, cfg, spacing, _, _, crop, tb, _ = C.CASES[tag]
    x = torch.from_numpy(GOLDEN[f"{tag}/logits"])
    props = C.properties(tag)
    convert = E.convert_predicted_logits_to_segmentation_with_correct_shape
    cfgm, plans = _managers(tag, regions=True)
    with pytest.raises(NotImplementedError):
        E.export_prediction_from_softmax(x.numpy(), props, cfgm, plans, C.dataset_json(K), "/nonexistent/never_written")
    with pytest.raises(NotImplementedError):
        E.resample_logits_to_shape(x, crop, cfg, spacing, order=3)
    with pytest.raises(NotImplementedError):
        E.resample_logits_to_shape(x, crop, cfg, spacing, order_z=3)
    with pytest.raises(NotImplementedError):
        convert(x, props, cfg, tb, order=3)
    bad = dict(props, shape_after_cropping_and_before_resampling=(crop[0] + 1,) + crop[1:])
    with pytest.raises(RuntimeError):
        convert(x, bad, cfg, tb)                                              # shape after cropping != bbox extent
    with pytest.raises(RuntimeError):
        convert(x, dict(props, bbox_used_for_cropping=[[30, 60], [3, 15], [1, 17]]), cfg, tb)   # bbox outside the volume
    with pytest.raises(RuntimeError):
        convert(x[0], props, cfg, tb)                                         # not (K, x, y, z)
    for perm in ((0, 1, 1), (0, 1), (1, 2, 3)):
        with pytest.raises(RuntimeError):
            convert(x, props, cfg, perm)
