"""Case preprocessing, host side (mlagg_unet_amd.preprocessing): the host path against the reference's own
DefaultPreprocessor.run_case (tests/golden/preprocess.npz, made by tests/golden/make_golden_preprocess.py), K22's separable cubic
arithmetic restated in numpy against the same fixture, the box of the filled mask, the errors, and predict_case against the
explicit chain of its three public functions."""
import os

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import evaluation, export, inference, predict
from mlagg_unet_amd import preprocessing as P
from tests import _preprocess_cases as C

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "preprocess.npz"))


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("tag", sorted(C.CASES))
def test_host_path_is_bit_identical_to_the_reference(tag):
    plans, name = C.plans(tag)
    image, props_in = C.image(tag), C.properties(tag)
    data, props = P.preprocess_case(image, props_in, plans, name)
    want = GOLDEN[f"{tag}/data"]
    assert isinstance(data, np.ndarray) and data.dtype == np.float32 and data.shape == want.shape
    assert np.array_equal(data.view(np.int32), want.view(np.int32))
    assert props["bbox_used_for_cropping"] == GOLDEN[f"{tag}/bbox"].tolist()
    assert tuple(props["shape_before_cropping"]) == tuple(GOLDEN[f"{tag}/shape_before_cropping"])
    assert tuple(props["shape_after_cropping_and_before_resampling"]) == tuple(GOLDEN[f"{tag}/shape_after_cropping"])
    assert props is not props_in and props_in == C.properties(tag)                  # a new dict; the caller's is untouched
    assert np.array_equal(image, C.image(tag))


def _decision(tag):
    plans, name = C.plans(tag)
    shape, spacing, tf, cfg_spacing = C.CASES[tag][:4]
    crop = tuple(GOLDEN[f"{tag}/shape_after_cropping"])
    cur = [spacing[i] for i in tf]
    target = list(cfg_spacing) if len(cfg_spacing) == 3 else [cur[0], *cfg_spacing]
    new = tuple(P.compute_new_shape(crop, cur, target))
    return crop, new, cur, target


@pytest.mark.parametrize("tag", sorted(C.CASES))
def test_separate_z_decision_matches_the_reference(tag):
    crop, new, cur, target = _decision(tag)
    sep, axis = export.separate_z_decision(cur, target)
    assert (int(sep), -1 if axis is None else axis) == tuple(GOLDEN[f"{tag}/separate_z"])


def _reflect_line(x, n_out):
    """One axis of K22's cubic pass in numpy: the FIR prefilter on the reflect-extended, edge-padded line and the 4-tap evaluation."""
    n = x.shape[-1]
    N = n + 2 * P.SPLINE_PAD
    start, w, P0, M = P._cubic_taps(n, n_out)
    p = np.arange(P0, P0 + M)
    coef = np.zeros(x.shape[:-1] + (M,))
    for q in range(-P.FIR_HALF_WIDTH, P.FIR_HALF_WIDTH + 1):
        u = p + q
        u = np.where(u < 0, -u - 1, np.where(u >= N, 2 * N - 1 - u, u))
        coef = coef + P.FIR[abs(q)] * x[..., np.clip(u - P.SPLINE_PAD, 0, n - 1)]
    return sum(w[:, k] * coef[..., start - P0 + k] for k in range(4))


def _k22_resample_numpy(data, new_shape, sep, axis, order_z):
    def along(y, a, n_out):
        return np.moveaxis(_reflect_line(np.moveaxis(y, a, -1), n_out), -1, a)

    out = []
    for c in range(data.shape[0]):
        x = data[c].astype(np.float64)
        if sep:
            plane = [a for a in range(3) if a != axis]
            y = along(along(x, plane[0], new_shape[plane[0]]), plane[1], new_shape[plane[1]])
            lo = x.min(axis=tuple(plane), keepdims=True)
            hi = x.max(axis=tuple(plane), keepdims=True)
            y = np.clip(y, lo, hi)
            if x.shape[axis] != new_shape[axis]:
                idx, w = export._axis_taps(x.shape[axis], new_shape[axis], "nearest" if order_z == 0 else "linear")
                b = [1, 1, 1]
                b[axis] = -1
                y = np.take(y, idx[:, 0], axis) * w[:, 0].reshape(b) + np.take(y, idx[:, 1], axis) * w[:, 1].reshape(b)
        else:
            y = x
            for a in range(3):
                y = along(y, a, new_shape[a])
            y = np.clip(y, x.min(), x.max())
        out.append(y.astype(np.float32))
    return np.stack(out)


@pytest.mark.parametrize("tag", sorted(t for t in C.CASES if t != "i_unchanged"))
def test_k22_cubic_arithmetic_matches_the_reference(tag):
    """K22's resampling (FIR prefilter with the reflect boundary, separable fp64 passes, clip, separate-z blend), restated in numpy
    on the reference's normalised data: at most 1 fp32 ulp from scipy's 3-D zoom, on at most 1e-4 of the voxels."""
    plans, name = C.plans(tag)
    crop, new, cur, target = _decision(tag)
    assert crop != new
    x = np.array(C.image(tag)).transpose([0, *[t + 1 for t in C.CASES[tag][2]]])
    x, seg, _ = P.crop_to_nonzero(x)
    x = np.array(x)
    cfg = plans["configurations"][name]
    for c in range(x.shape[0]):
        x[c] = P._normalize_channel_host(x[c], seg[0], cfg["normalization_schemes"][c], cfg["use_mask_for_norm"][c],
                                         plans["foreground_intensity_properties_per_channel"][str(c)])
    sep, axis = export.separate_z_decision(cur, target)
    got = _k22_resample_numpy(x, new, sep, axis, C.CASES[tag][8])
    d = _ulps(got, GOLDEN[f"{tag}/data"])
    assert d.max() <= 1 and (d > 0).mean() <= 1e-4


def test_cubic_taps_read_inside_the_padded_line():
    for n_in, n_out in ((1, 1), (1, 7), (7, 1), (2, 3), (512, 492), (148, 500), (300, 30)):
        start, w, P0, M = P._cubic_taps(n_in, n_out)
        assert P0 >= 0 and P0 + M <= n_in + 2 * P.SPLINE_PAD and start.min() == P0 and start.max() + 4 == P0 + M
        assert np.allclose(w.sum(1), 1.0, atol=1e-15)
    assert abs(P.FIR[0] + 2 * P.FIR[1:].sum() - 1.0) < 1e-15            # the prefilter keeps constants


def test_box_of_the_filled_mask_equals_the_box_of_the_non_zero_voxels():
    rng = np.random.default_rng(5)
    for trial in range(30):
        shape = tuple(rng.integers(4, 14, size=3))
        m = np.zeros(shape, dtype=bool)
        lo = [int(rng.integers(0, s - 2)) for s in shape]
        hi = [int(rng.integers(a + 2, s + 1)) for a, s in zip(lo, shape)]
        m[tuple(slice(a, b) for a, b in zip(lo, hi))] = rng.random(tuple(b - a for a, b in zip(lo, hi))) < 0.7
        img = m[None].astype(np.float32) * rng.uniform(1, 5, size=(1,) + shape).astype(np.float32)
        if not m.any():
            continue
        hit = [np.flatnonzero(m.any(tuple(b for b in range(3) if b != a))) for a in range(3)]
        raw = [[int(h[0]), int(h[-1]) + 1] for h in hit]
        assert P.get_bbox_from_mask(ndi.binary_fill_holes(m)) == raw
        _, seg, bbox = P.crop_to_nonzero(img)
        assert bbox == raw and seg.dtype == np.int8 and set(np.unique(seg)) <= {-1, 0}


def test_get_configuration_resolves_inherits_from():
    plans, name = C.plans("c_isotropic_3d")
    plans["configurations"]["3d_child"] = {"inherits_from": name, "spacing": [2.0, 2.0, 2.0]}
    cfg = P.get_configuration(plans, "3d_child")
    assert cfg["spacing"] == [2.0, 2.0, 2.0] and cfg["normalization_schemes"] == ["CTNormalization"]
    plans["configurations"][name]["inherits_from"] = "3d_child"
    with pytest.raises(RuntimeError):
        P.get_configuration(plans, "3d_child")
    with pytest.raises(RuntimeError):
        P.get_configuration(plans, "missing")


def _with(tag, **changes):
    plans, name = C.plans(tag)
    plans["configurations"][name].update(changes)
    return plans, name


def test_errors():
    tag = "c_isotropic_3d"
    plans, name = C.plans(tag)
    with pytest.raises(RuntimeError, match="no non-zero voxel"):
        P.preprocess_case(np.zeros((1, 6, 6, 6), np.float32), C.properties(tag), plans, name)
    with pytest.raises(NotImplementedError):
        P.preprocess_case(C.image(tag), C.properties(tag), *_with(tag, normalization_schemes=["MyScheme"]))
    with pytest.raises(NotImplementedError):
        P.preprocess_case(C.image(tag), C.properties(tag), *_with(tag, resampling_fn_data="resample_torch_fornoseg"))
    for kw in ({"is_seg": False, "order": 1, "order_z": 0, "force_separate_z": None},
               {"is_seg": False, "order": 3, "order_z": 3, "force_separate_z": None},
               {"is_seg": True, "order": 3, "order_z": 0, "force_separate_z": None}):
        with pytest.raises(NotImplementedError):
            P.preprocess_case(C.image(tag), C.properties(tag), *_with(tag, resampling_fn_data_kwargs=kw))
    with pytest.raises(NotImplementedError):
        P.preprocess_case(C.image(tag), C.properties(tag), *_with(tag, previous_stage="3d_lowres"))
    with pytest.raises(NotImplementedError):
        P.preprocess_case(C.image(tag), C.properties(tag), *_with(tag, preprocessor_name="MyPreprocessor"))
    with pytest.raises(NotImplementedError):
        P.resample_data_to_shape(np.ones((1, 4, 4, 4), np.float32), (5, 5, 5), (1, 1, 1), (0.8, 0.8, 0.8), order=1)
    with pytest.raises(RuntimeError):
        P.preprocess_case(np.ones((6, 6, 6), np.float32), C.properties(tag), plans, name)
    rgb = C.image("h_other_schemes")
    rgb[2, 3, 3, 3] = 300.0
    plans_h, name_h = C.plans("h_other_schemes")
    with pytest.raises(RuntimeError, match="RGB"):
        P.preprocess_case(rgb, C.properties("h_other_schemes"), plans_h, name_h)
    net = TinyNet3d(1, 3)
    with pytest.raises(NotImplementedError):
        predict.predict_case(net, C.image(tag), C.properties(tag), plans, name,
                             {"labels": {"background": 0, "organ": [1, 2]}, "regions_class_order": [1, 2]})


def test_resampling_an_unchanged_shape_returns_the_data():
    x = np.random.default_rng(0).standard_normal((2, 5, 6, 7)).astype(np.float32)
    assert P.resample_data_to_shape(x, (5, 6, 7), (1, 1, 1), (1, 1, 1)) is x


class TinyNet3d(torch.nn.Module):
    """A fixed 1x1x1 convolution: deterministic, cheap, and any tile size."""

    def __init__(self, cin, k, seed=0):
        super().__init__()
        self.conv = torch.nn.Conv3d(cin, k, 1)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(self.conv.weight.shape, generator=g))
            self.conv.bias.copy_(torch.randn(self.conv.bias.shape, generator=g))

    def forward(self, x):
        return self.conv(x)


class TinyNet2d(TinyNet3d):
    def __init__(self, cin, k, seed=0):
        torch.nn.Module.__init__(self)
        self.conv = torch.nn.Conv2d(cin, k, 1)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(self.conv.weight.shape, generator=g))
            self.conv.bias.copy_(torch.randn(self.conv.bias.shape, generator=g))


def _explicit_chain(net, tag, K, mirror, folds=None):
    plans, name = C.plans(tag)
    cfg = P.get_configuration(plans, name)
    data, props = P.preprocess_case(C.image(tag), C.properties(tag), plans, name)
    logits = None
    for sd in folds or [None]:
        if sd is not None:
            net.load_state_dict(sd)
        out = inference.predict_sliding_window_return_logits(net, torch.from_numpy(data), K, tuple(cfg["patch_size"]),
                                                             mirror_axes=mirror, device="cpu")
        logits = out if logits is None else logits + out
    if folds and len(folds) > 1:
        logits = logits / len(folds)
    return export.convert_predicted_logits_to_segmentation_with_correct_shape(logits, props, cfg["spacing"],
                                                                              plans["transpose_backward"], return_probabilities=True)


@pytest.mark.parametrize("tag,mirror", [("c_isotropic_3d", (0, 2)), ("e_transpose", None), ("d_2d_config", (0, 1))])
def test_predict_case_equals_the_explicit_chain_on_cpu(tag, mirror):
    K = 3
    cin = C.CASES[tag][0][0]
    net = TinyNet2d(cin, K) if len(C.CASES[tag][3]) == 2 else TinyNet3d(cin, K)
    plans, name = C.plans(tag)
    dj = {"labels": {"background": 0, "liver": 1, "spleen": 2}}
    seg, probs = predict.predict_case(net, C.image(tag), C.properties(tag), plans, name, dj, mirror_axes=mirror,
                                      return_probabilities=True, device="cpu")
    want_seg, want_probs = _explicit_chain(net, tag, K, mirror)
    assert seg.dtype == torch.uint8 and tuple(seg.shape) == C.CASES[tag][0][1:]
    assert torch.equal(seg, want_seg) and torch.equal(probs, want_probs)
    dsc = evaluation.abdomen_case_dsc(seg.numpy(), seg.numpy())
    assert all(v in (1.0, float("nan")) or np.isnan(v) for v in dsc.values())


def test_predict_case_averages_folds():
    tag, K = "c_isotropic_3d", 3
    folds = [{k: v.clone() for k, v in TinyNet3d(1, K, seed=s).state_dict().items()} for s in (1, 2)]
    plans, name = C.plans(tag)
    dj = {"labels": {"background": 0, "a": 1, "b": 2}}
    net = TinyNet3d(1, K)
    seg, probs = predict.predict_case(net, C.image(tag), C.properties(tag), plans, name, dj, parameters=folds,
                                      return_probabilities=True, device="cpu")
    want_seg, want_probs = _explicit_chain(TinyNet3d(1, K), tag, K, None, folds)
    assert torch.equal(seg, want_seg) and torch.equal(probs, want_probs)
