"""Case preprocessing on the device (K22, csrc/preprocess.hip, behind mlagg_unet_amd.preprocessing): against the reference's own
run_case (tests/golden/preprocess.npz), against the host path on permuted inputs, the box kernel against numpy, reproducibility, a
BTCV-sized and a > 2^31-byte separate-z case against scipy on selected slices, and predict_case against the host chain."""
import os

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import export, inference, ops, predict
from mlagg_unet_amd import preprocessing as P
from tests import _preprocess_cases as C
from tests.test_preprocess_cpu import TinyNet2d, _ulps

gpu = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "preprocess.npz"))


def _zscore_bound(want):
    """|device - reference| of a ZScore channel: the device's fp64 mean / std differ from numpy's fp32 pairwise ones by a few fp32
    ulps of each (relative ZSCORE_TOLERANCE), which moves y = (x - mean) / std by that much of |y| + |mean| / std, plus the zoom's
    1 ulp."""
    return P.ZSCORE_TOLERANCE * (np.abs(want) + np.abs(want).max() + 1.0) + 2.0 * np.spacing(np.abs(want).astype(np.float32))


@gpu
@pytest.mark.parametrize("tag", sorted(C.CASES))
def test_device_matches_the_reference(tag):
    plans, name = C.plans(tag)
    data, props = P.preprocess_case(C.image(tag), C.properties(tag), plans, name, device=DEV)
    want = GOLDEN[f"{tag}/data"]
    assert isinstance(data, torch.Tensor) and data.is_cuda and data.dtype == torch.float32 and data.is_contiguous()
    got = data.cpu().numpy()
    assert got.shape == want.shape
    assert props["bbox_used_for_cropping"] == GOLDEN[f"{tag}/bbox"].tolist()
    assert tuple(props["shape_before_cropping"]) == tuple(GOLDEN[f"{tag}/shape_before_cropping"])
    assert tuple(props["shape_after_cropping_and_before_resampling"]) == tuple(GOLDEN[f"{tag}/shape_after_cropping"])
    for c, scheme in enumerate(C.CASES[tag][4]):
        if scheme == "ZScoreNormalization":
            err = np.abs(got[c].astype(np.float64) - want[c])
            assert (err <= _zscore_bound(want[c])).all(), float(err.max())
            print(f"{tag} channel {c}: ZScore max |diff| {err.max():.3g}")
        else:
            d = _ulps(got[c], want[c])
            print(f"{tag} channel {c}: max {d.max()} ulp, {int((d > 0).sum())} of {d.size} voxels differ")
            assert d.max() <= 1 and (d > 0).mean() <= 1e-4


@gpu
@pytest.mark.parametrize("tag", ["e_transpose", "g_masked_zscore", "a_sep_z_changes"])
def test_permuted_and_non_contiguous_inputs(tag):
    plans, name = C.plans(tag)
    img = torch.from_numpy(C.image(tag))
    a, pa = P.preprocess_case(img.to(DEV), C.properties(tag), plans, name)
    view = img.to(DEV).permute(3, 2, 0, 1).contiguous().permute(2, 3, 1, 0)          # same values, other strides
    assert not view.is_contiguous()
    b, pb = P.preprocess_case(view, C.properties(tag), plans, name)
    assert torch.equal(a, b) and pa == pb
    host, ph = P.preprocess_case(C.image(tag), C.properties(tag), plans, name)
    assert ph["bbox_used_for_cropping"] == pa["bbox_used_for_cropping"]
    if "ZScoreNormalization" not in C.CASES[tag][4]:
        d = _ulps(a.cpu().numpy(), host)
        assert d.max() <= 1 and (d > 0).mean() <= 1e-4


def _numpy_box(x):
    """min x, y, z and max x, y, z of the voxels non-zero in any channel"""
    nz = (x != 0).any(0)
    return [int(np.flatnonzero(nz.any(tuple(b for b in range(3) if b != a)))[k]) for k in (0, -1) for a in range(3)]


@gpu
def test_box_kernel_against_numpy():
    shape = (3, 17, 30, 23)
    cases = []
    x = np.zeros(shape, np.float32)
    x[2, 4:9, 3:20, 7:8] = -2.5                                      # non-zero in one channel only
    cases.append(x)
    x = np.zeros(shape, np.float32)
    x[0, 0, 5, 5] = 1.0
    x[1, 16, 29, 22] = 3.0
    x[2, 8, 0, 0] = -1.0                                             # only on the borders
    cases.append(x)
    x = np.zeros(shape, np.float32)
    x[1, 11, 13, 4] = 7.0                                            # a single voxel
    cases.append(x)
    x = np.zeros(shape, np.float32)
    x[0, 9, 0, 22] = -0.0                                            # negative zero counts as zero
    x[0, 3, 4, 5] = 1e-30
    cases.append(x)
    for x in cases:
        got = ops.pp_nonzero_box(torch.from_numpy(x).to(DEV)).cpu().tolist()
        want = _numpy_box(x)
        assert got == want
    perm = torch.from_numpy(cases[1]).to(DEV).permute(0, 2, 3, 1)
    got = ops.pp_nonzero_box(perm).cpu().tolist()
    want = _numpy_box(cases[1].transpose(0, 2, 3, 1))
    assert got == want
    got = ops.pp_nonzero_box(torch.zeros(shape, device=DEV)).cpu().tolist()
    assert got[3:] == [-1, -1, -1]
    plans, name = C.plans("c_isotropic_3d")
    with pytest.raises(RuntimeError, match="no non-zero voxel"):
        P.preprocess_case(torch.zeros((1, 6, 6, 6), device=DEV), C.properties("c_isotropic_3d"), plans, name)


@gpu
@pytest.mark.parametrize("tag", ["g_masked_zscore", "c_isotropic_3d", "j_order_z1"])
def test_two_runs_are_bit_identical(tag):
    plans, name = C.plans(tag)
    a, _ = P.preprocess_case(C.image(tag), C.properties(tag), plans, name, device=DEV)
    b, _ = P.preprocess_case(C.image(tag), C.properties(tag), plans, name, device=DEV)
    assert torch.equal(a, b)


def _ct_plans(cfg_spacing, tf=(0, 1, 2)):
    cfg = {"spacing": list(cfg_spacing), "normalization_schemes": ["CTNormalization"], "use_mask_for_norm": [False],
           "patch_size": [16, 16]}
    return {"transpose_forward": list(tf), "transpose_backward": [int(i) for i in np.argsort(tf)], "configurations": {"2d": cfg},
            "foreground_intensity_properties_per_channel": {"0": dict(C.FG)}}, "2d"


def _blocky_volume(shape, seed, rim):
    """(1, *shape) fp32 on the device: blocky CT levels with noise, a zero rim of `rim` voxels in-plane."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    coarse = torch.rand((1, shape[0], (shape[1] + 7) // 8, (shape[2] + 7) // 8), generator=g, device=DEV) * 4024 - 1024
    v = coarse.repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :, :shape[1], :shape[2]]
    v = torch.round(v + torch.randn(v.shape, generator=g, device=DEV) * 25)
    v[v == 0] = 1
    v[:, :, :rim] = 0
    v[:, :, -rim:] = 0
    v[:, :, :, :rim] = 0
    v[:, :, :, -rim:] = 0
    return v.contiguous()


def _check_slices(image, out, props, plans, name, slices):
    """out[:, o] of a separate-z case along axis 0 with unchanged or order-0 slice axis: the 2-D resize of the input slice the
    order-0 table picks, computed by the host path on that slice alone."""
    cfg = plans["configurations"][name]
    lo = [b[0] for b in props["bbox_used_for_cropping"]]
    hi = [b[1] for b in props["bbox_used_for_cropping"]]
    n_in, n_out = hi[0] - lo[0], out.shape[1]
    idx, _ = export._axis_taps(n_in, n_out, "nearest" if n_in != n_out else "identity")
    for o in slices:
        s = image[0, lo[0] + int(idx[o, 0]), lo[1]:hi[1], lo[2]:hi[2]].cpu().numpy()
        s = P._normalize_channel_host(s, None, "CTNormalization", False, plans["foreground_intensity_properties_per_channel"]["0"])
        want = P._resize_host(s.astype(np.float64), out.shape[2:]).astype(np.float32)
        d = _ulps(out[0, o].cpu().numpy(), want)
        assert d.max() <= 1 and (d > 0).mean() <= 1e-4, (o, int(d.max()), int((d > 0).sum()))
    assert cfg["spacing"]


@gpu
def test_btcv_sized_separate_z_case_against_scipy():
    image = _blocky_volume((148, 512, 512), 148, 6)
    plans, name = _ct_plans((0.79, 0.79))
    out, props = P.preprocess_case(image, {"spacing": [2.5, 0.76, 0.76]}, plans, name)
    assert tuple(out.shape) == (1, 148, 481, 481)
    _check_slices(image, out, props, plans, name, (0, 73, 147))


@gpu
def test_offsets_beyond_2_to_the_31_bytes():
    """300 x 1024 x 1024 -> 300 x 1138 x 1138: the first in-plane pass's fp64 buffer holds 2.8 GB."""
    image = _blocky_volume((300, 1024, 1024), 31, 2)
    plans, name = _ct_plans((0.45, 0.45))
    out, props = P.preprocess_case(image, {"spacing": [2.5, 0.5, 0.5]}, plans, name)
    assert tuple(out.shape) == (1, 300, 1133, 1133)
    assert 8 * 300 * 1020 * 1133 > 2 ** 31
    _check_slices(image, out, props, plans, name, (0, 299))


def _sure(probs, gap=1e-4):
    top2 = torch.as_tensor(probs).topk(2, dim=0).values
    return (top2[0] - top2[1]) > gap


def _host_chain(net, image, props_in, plans, name, K, mirror):
    cfg = P.get_configuration(plans, name)
    data, props = P.preprocess_case(image, props_in, plans, name)
    logits = inference.predict_sliding_window_return_logits(net, torch.from_numpy(data), K, tuple(cfg["patch_size"]),
                                                            mirror_axes=mirror, device=DEV)
    return export.convert_predicted_logits_to_segmentation_with_correct_shape(logits.cpu(), props, cfg["spacing"],
                                                                              plans["transpose_backward"], return_probabilities=True)


@gpu
def test_predict_case_2d_network_device_vs_host_chain():
    tag, K = "d_2d_config", 3
    net = TinyNet2d(1, K).to(DEV)
    plans, name = C.plans(tag)
    dj = {"labels": {"background": 0, "a": 1, "b": 2}}
    seg, probs = predict.predict_case(net, C.image(tag), C.properties(tag), plans, name, dj, mirror_axes=(0, 1),
                                      return_probabilities=True)
    hseg, hprobs = _host_chain(net, C.image(tag), C.properties(tag), plans, name, K, (0, 1))
    assert seg.is_cuda and seg.dtype == torch.uint8
    sure = _sure(hprobs)
    inside = hprobs.sum(0) > 0                                      # zeros outside the crop box: no near-ties there
    assert (sure | ~inside).float().mean() > 0.9
    assert torch.equal(seg.cpu()[~inside], hseg[~inside])
    assert torch.equal(seg.cpu()[sure], hseg[sure])
    assert float((probs.cpu() - hprobs).abs().max()) < 1e-3


@gpu
def test_predict_case_3d_network_device_vs_host_chain():
    from mlagg_unet_amd import model3d
    strides = [[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2], [1, 2, 2], [1, 2, 2]]
    n, K = len(strides), 5
    torch.manual_seed(4)
    net = model3d.build_network_architecture_3d(1, K, [[3, 3, 3]] * n, strides, [2] * n, [2] * (n - 1),
                                                enable_deep_supervision=False).to(DEV).eval()
    shape = (1, 14, 70, 60)
    image = _blocky_volume(shape[1:], 7, 3).cpu().numpy()
    cfg = {"spacing": [2.0, 0.9, 0.9], "normalization_schemes": ["CTNormalization"], "use_mask_for_norm": [False],
           "patch_size": [8, 64, 64]}
    plans = {"transpose_forward": [0, 1, 2], "transpose_backward": [0, 1, 2], "configurations": {"3d_fullres": cfg},
             "foreground_intensity_properties_per_channel": {"0": dict(C.FG)}}
    props = {"spacing": [2.5, 0.8, 0.8]}
    dj = {"labels": {"background": 0, **{f"organ{k}": k for k in range(1, K)}}}
    seg, probs = predict.predict_case(net, image, props, plans, "3d_fullres", dj, mirror_axes=(0, 1, 2), return_probabilities=True)
    hseg, hprobs = _host_chain(net, image, props, plans, "3d_fullres", K, (0, 1, 2))
    assert tuple(seg.shape) == shape[1:]
    sure = _sure(hprobs)
    inside = hprobs.sum(0) > 0                                      # zeros outside the crop box: no near-ties there
    assert (sure | ~inside).float().mean() > 0.9
    assert torch.equal(seg.cpu()[~inside], hseg[~inside])
    assert torch.equal(seg.cpu()[sure], hseg[sure])
