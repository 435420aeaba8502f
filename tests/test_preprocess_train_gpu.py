"""Training-case preprocessing on the device (K26, csrc/preprocess_train.hip, behind mlagg_unet_amd.preprocessing / fingerprint):
against the reference's own run_case(seg_file=...) (tests/golden/preprocess_train.npz), the rank select against numpy, the
segmentation resampler against the host path on large volumes, the fingerprint samples, permuted inputs and reproducibility.

The device sums a voxel's label weights in scipy's order ((wx * wy) * wz, last axis fastest, no contraction), so the labels equal
the host's everywhere, near-tie voxels (some label's fp64 interpolated indicator within preprocessing.NEAR_TIE = 2^-40 of the 0.5
threshold) included: the tests assert equality outright and print the near-tie counts for the record."""
import os

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import export, fingerprint, ops
from mlagg_unet_amd import preprocessing as P
from tests import _preprocess_cases as C
from tests import _preprocess_train_cases as T
from tests.test_preprocess_cpu import _ulps
from tests.test_preprocess_gpu import _zscore_bound
from tests.test_preprocess_train_cpu import GOLDEN, TAGS, check_geometry, check_locations, golden_locations, run

gpu = pytest.mark.gpu
DEV = "cuda:0"


def _collect(tag):
    return P._label_lists(T.dataset_json(tag))[0]


def _near_tie_mask(tag):
    """The host path's near-tie voxels of the case's segmentation resampling (all False when the shape is unchanged)."""
    plans, name = T.plans(tag)
    cfg = plans["configurations"][name]
    tf = plans["transpose_forward"]
    perm = [0, *[i + 1 for i in tf]]
    _, s, _ = P.crop_to_nonzero(T.image(tag).transpose(perm), T.seg(tag).transpose(perm).copy())
    spacing = [T.properties(tag)["spacing"][i] for i in tf]
    target, new_shape = P._target_shape(cfg, s.shape[1:], spacing)
    if tuple(new_shape) == s.shape[1:]:
        return np.zeros(s.shape, dtype=bool)
    sep, axis = export.separate_z_decision(spacing, target, None)
    return P._resample_seg_host(s, new_shape, sep, axis, near_tie=True)[1]


def _check_labels(got, want, near, dyadic, what):
    diff = got != want
    print(f"{what}: {int(diff.sum())} of {diff.size} labels differ, {int(near.sum())} near-tie voxels")
    assert not diff.any()


@gpu
@pytest.mark.parametrize("tag", TAGS)
def test_device_matches_the_reference(tag):
    data, seg, props = run(tag, DEV)
    want_d, want_s = GOLDEN[f"{tag}/data"], GOLDEN[f"{tag}/seg"]
    assert isinstance(data, torch.Tensor) and data.is_cuda and data.dtype == torch.float32 and data.is_contiguous()
    assert isinstance(seg, torch.Tensor) and seg.is_cuda
    got = data.cpu().numpy()
    assert got.shape == want_d.shape
    check_geometry(props, tag)
    for c, scheme in enumerate(T._spec(tag)[4]):
        if scheme == "ZScoreNormalization":
            err = np.abs(got[c].astype(np.float64) - want_d[c])
            print(f"{tag} channel {c}: ZScore max |diff| {err.max():.3g}")
            assert (err <= _zscore_bound(want_d[c])).all(), float(err.max())
        else:
            d = _ulps(got[c], want_d[c])
            print(f"{tag} channel {c}: max {d.max()} ulp, {int((d > 0).sum())} of {d.size} voxels differ")
            assert d.max() <= 1 and (d > 0).mean() <= 1e-4
    s = seg.cpu().numpy()
    assert s.dtype == want_s.dtype and s.shape == want_s.shape
    _check_labels(s, want_s, _near_tie_mask(tag), T.is_dyadic(tag), tag)
    # class locations of the chain's own segmentation: keys and counts by the formula, every coordinate carries its class
    locs = props["class_locations"]
    collect = _collect(tag)
    assert list(locs) == [tuple(c) if isinstance(c, list) else c for c in collect]
    for c in collect:
        k = tuple(c) if isinstance(c, list) else c
        n = int(np.isin(s, c).sum())
        if n == 0:
            assert locs[k] == []
            continue
        v = locs[k]
        assert isinstance(v, np.ndarray) and v.dtype == np.int64 and v.shape == (P._num_to_sample(n), 4) and (v[:, 0] == 0).all()
        assert np.isin(s[0][v[:, 1], v[:, 2], v[:, 3]], c).all()
        assert len(np.unique(v, axis=0)) == len(v)
    if np.array_equal(s, want_s):
        check_locations(locs, golden_locations(tag))


@gpu
@pytest.mark.parametrize("tag", TAGS)
def test_class_locations_of_the_goldens_segmentation_are_identical(tag):
    seg = torch.from_numpy(GOLDEN[f"{tag}/seg"]).to(DEV)
    got = P.sample_foreground_locations(seg, _collect(tag))
    check_locations(got, golden_locations(tag))


def _numpy_select(seg, labels, seed_state):
    locs = np.argwhere(np.isin(seg, labels))
    if len(locs) == 0:
        return []
    return locs[seed_state.choice(len(locs), P._num_to_sample(len(locs)), replace=False)]


@gpu
def test_rank_select_against_numpy_on_a_btcv_sized_volume():
    shape = (1, 150, 400, 400)                                         # 24e6 voxels, 11719 table rows: the last one is partial
    rng = np.random.default_rng(26)
    seg = np.zeros(shape, dtype=np.int16)
    seg[0, 10:120, 30:370, 40:360] = 1                                 # 11.95e6 voxels after the next line: the 1 % branch
    seg[0, 60:70, 100:140, 100:140] = rng.integers(2, 6, size=(10, 40, 40))
    seg[0, 77, 123, 311] = 7                                           # one voxel
    seg[0, 149, 399, 380:] = 8                                         # only in the last, partial row
    seg[0, 0, 0, 0:3] = -1
    classes = [1, 2, 3, 4, 5, 6, 7, 8, [0, 1, 2, 3, 4, 5, 7, 8]]       # 6 is absent
    assert shape[1] * shape[2] * shape[3] % ops.PP_RANK_BLOCK != 0
    assert (seg.reshape(-1)[-(seg.size % ops.PP_RANK_BLOCK):] == 8).sum() == 20
    d = torch.from_numpy(seg).to(DEV)
    a = P.sample_foreground_locations(d, classes)
    b = P.sample_foreground_locations(d, classes)
    rs = np.random.RandomState(1234)
    for c in classes:
        k = tuple(c) if isinstance(c, list) else c
        want = _numpy_select(seg, c, rs)
        if len(want) == 0:
            assert a[k] == [] and b[k] == []
            continue
        assert a[k].dtype == np.int64 and np.array_equal(a[k], want) and np.array_equal(a[k], b[k])
    assert len(a[1]) == 119520 and len(a[7]) == 1 and a[6] == [] and len(a[8]) == 20
    table = ops.pp_group_table([[1], [8]], 8, DEV)
    t1, n1 = ops.pp_rank_counts(d[0], table, 2, 8)
    t2, n2 = ops.pp_rank_counts(d[0], table, 2, 8)
    assert torch.equal(t1, t2) and torch.equal(n1, n2) and n1.tolist() == [int((seg == 1).sum()), 20]
    ranks = torch.tensor([0, 19, 20, -1], device=DEV)
    coords, _ = ops.pp_rank_select(d[0], table, 8, (t1, n1), 1, ranks)
    assert coords.cpu().tolist() == [[0, 149, 399, 380], [0, 149, 399, 399], [-1] * 4, [-1] * 4]


def _label_volume(shape, n_labels, seed, block):
    """(1, *shape) int16 on the device: blocky random labels 0 .. n_labels, most of it background."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    coarse = torch.randint(0, 3 * n_labels, tuple((s + b - 1) // b for s, b in zip(shape, block)), generator=g, device=DEV)
    coarse = torch.where(coarse > n_labels, torch.zeros_like(coarse), coarse)
    for a, b in enumerate(block):
        coarse = coarse.repeat_interleave(b, a)
    return coarse[:shape[0], :shape[1], :shape[2]].to(torch.int16)[None].contiguous()


@gpu
def test_btcv_sized_separate_z_resampling_against_the_host_path_on_slices():
    seg = _label_volume((148, 500, 500), 13, 148, (3, 17, 23))
    seg[0, :, :40] = -1
    out = P.resample_seg_to_shape(seg, (148, 481, 481), (2.5, 0.76, 0.76), (2.5, 0.79, 0.79))
    assert out.is_cuda and out.dtype == torch.int16 and tuple(out.shape) == (1, 148, 481, 481)
    for o in (0, 73, 147):
        s = seg[:, o:o + 1].cpu().numpy()
        want, near = P._resample_seg_host(s, (1, 481, 481), True, 0, near_tie=True)
        _check_labels(out[:, o:o + 1].cpu().numpy(), want, near, False, f"slice {o}")
    # the slice axis changing size: every output slice is the in-plane result of the slice the order-0 table picks
    out2 = P.resample_seg_to_shape(seg, (185, 481, 481), (2.5, 0.76, 0.76), (2.0, 0.79, 0.79))
    idx, _ = export._axis_taps(148, 185, "nearest")
    for o in (0, 92, 184):
        assert torch.equal(out2[0, o], P.resample_seg_to_shape(seg[:, int(idx[o, 0]):int(idx[o, 0]) + 1], (1, 481, 481),
                                                               (2.5, 0.76, 0.76), (2.5, 0.79, 0.79))[0, 0])
    assert torch.equal(out2[0, 92], out[0, int(idx[92, 0])])


@gpu
def test_3d_zoom_with_non_dyadic_factors_against_the_host_path():
    seg = _label_volume((90, 120, 110), 13, 90, (7, 9, 11))
    seg[0, :5] = -1
    new_shape = (113, 97, 110)                                          # one axis up, one down, one unchanged
    out = P.resample_seg_to_shape(seg, new_shape, (1.5, 1.0, 1.0), (1.2, 1.24, 1.0))
    want, near = P._resample_seg_host(seg.cpu().numpy(), new_shape, False, None, near_tie=True)
    _check_labels(out.cpu().numpy(), want, near, False, "3-D zoom")
    again = P.resample_seg_to_shape(seg, new_shape, (1.5, 1.0, 1.0), (1.2, 1.24, 1.0))
    assert torch.equal(out, again)
    as_int8 = P.resample_seg_to_shape(seg.to(torch.int8), new_shape, (1.5, 1.0, 1.0), (1.2, 1.24, 1.0))
    assert as_int8.dtype == torch.int8 and torch.equal(as_int8.to(torch.int16), out)


@gpu
@pytest.mark.parametrize("tag", TAGS)
def test_fingerprint_samples_on_the_device_are_the_references(tag):
    image, seg = torch.from_numpy(T.image(tag)).to(DEV), torch.from_numpy(T.seg(tag)).to(DEV)
    after, spacing, samples, rel = fingerprint.analyze_case(image, seg, T.properties(tag), T.FINGERPRINT_SAMPLES)
    want = GOLDEN[f"{tag}/fp_samples"]
    assert tuple(after) == tuple(GOLDEN[f"{tag}/fp_shape_after_crop"]) and float(rel) == float(GOLDEN[f"{tag}/fp_relative_size"])
    assert len(samples) == want.shape[0]
    for c in range(want.shape[0]):
        assert samples[c].dtype == np.float32 and np.array_equal(samples[c], want[c])
    empty = fingerprint.collect_foreground_intensities(torch.zeros_like(seg), image, num_samples=5)
    assert empty == [[] for _ in range(image.shape[0])]


@gpu
@pytest.mark.parametrize("tag", ["e_transpose", "g_masked_zscore", "f_border_box"])
def test_permuted_inputs_and_two_runs(tag):
    plans, name = T.plans(tag)
    dj = T.dataset_json(tag)
    img, seg = torch.from_numpy(T.image(tag)).to(DEV), torch.from_numpy(T.seg(tag)).to(DEV)
    a, sa, pa = P.preprocess_training_case(img, seg, T.properties(tag), plans, name, dj)
    iv = img.permute(3, 2, 0, 1).contiguous().permute(2, 3, 1, 0)       # same values, other strides
    sv = seg.permute(3, 2, 0, 1).contiguous().permute(2, 3, 1, 0)
    assert not iv.is_contiguous() and not sv.is_contiguous()
    b, sb, pb = P.preprocess_training_case(iv, sv.to(torch.int32), T.properties(tag), plans, name, dj)
    assert a.is_cuda and sa.is_cuda and b.is_cuda and sb.is_cuda
    assert torch.equal(a, b) and torch.equal(sa, sb) and sa.dtype == sb.dtype
    la, lb = pa.pop("class_locations"), pb.pop("class_locations")
    assert pa == pb
    check_locations(la, lb)
    c, sc, pc = P.preprocess_training_case(img, seg, T.properties(tag), plans, name, dj)
    assert torch.equal(a, c) and torch.equal(sa, sc)
    check_locations(pc["class_locations"], la)


@gpu
def test_labels_outside_the_datasets_range_are_refused(tmp_path):
    tag = "c_isotropic_3d"
    plans, name = T.plans(tag)
    seg = T.seg(tag)
    seg[0, 5, 5, 5] = 9
    with pytest.raises(RuntimeError, match="outside -1 .. 4"):
        P.preprocess_training_case(T.image(tag), seg, T.properties(tag), plans, name, T.dataset_json(tag), device=DEV)
    done = P.preprocess_dataset([(tag, T.image(tag), T.seg(tag), T.properties(tag))], str(tmp_path), plans, name,
                                T.dataset_json(tag), device=DEV)
    z = np.load(os.path.join(str(tmp_path), tag + ".npz"))
    assert done == [tag] and z["seg"].dtype == np.int8 and z["data"].shape == GOLDEN[f"{tag}/data"].shape
    assert C.CASES[tag][0][0] == z["data"].shape[0]
