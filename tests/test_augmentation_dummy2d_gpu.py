"""GPU: K31 (csrc/augment3d.hip, ops.aug3d_resample_planar) and the dummy-2-D augmentation chain on HBM-resident batches against the
scipy float64 oracle (tests/_augmentation_dummy2d_cases.py), edge shapes, a batch split over two launches, and the anisotropic 3-D
input path (DataLoader3D + GpuAugmenter3D.for_plan on the PrefetchLoader's side stream)."""
import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import augmentation3d as AUG3
from mlagg_unet_amd import dataloading as DL
from mlagg_unet_amd import ops
from tests import _augmentation_dummy2d_cases as K
from tests import _dataloading_3d_cases as KD

pytestmark = pytest.mark.gpu
TOL = 5e-5                  # fp32 prefilter GEMMs and fp32 tap sums against float64 scipy, volumes of amplitude <= 5
NEAR_CAP = 0.005            # share of label voxels a test may exclude as "within 1e-4 of 0.5"


def _device(p, data, seg, noise, patch=K.OUT):
    aug = AUG3.GpuAugmenter3D(patch, "cuda:0", labels=K.LABELS, dummy_2d=True)
    d, s = aug.apply(torch.from_numpy(data).cuda(), torch.from_numpy(seg).cuda().to(torch.int16), p, torch.from_numpy(noise).cuda())
    assert d.is_cuda and s.is_cuda and d.dtype == torch.float32 and s.dtype == torch.float32
    return d.cpu().numpy(), s.cpu().numpy()


def _check(got_d, got_s, want_d, want_s, near):
    err = np.abs(got_d - want_d).max()
    print(f"max |K31 - oracle| = {err:.3g}; label voxels within 1e-4 of 0.5: {int(near.sum())} of {near.size}")
    assert err < TOL
    assert near.mean() <= NEAR_CAP
    assert np.array_equal(got_s[~near], want_s[~near]), int((got_s != want_s).sum())


def test_k31_resample_matches_the_oracle():
    data, seg = K.volumes()
    p = K.only(K.forced_params(), ["do_rot", "do_scale"])
    got_d, got_s = _device(p, data, seg, np.zeros((K.B, K.C) + K.OUT, np.float32))
    want_d, want_s = K.spatial(data, seg, K.OUT, p)
    _check(got_d, got_s, want_d, want_s, K.near_half(seg, p))
    assert len(np.unique(want_s)) >= 4
    # sample 3 neither rotates nor scales: the centre crop over (Y, Z), bit for bit
    o = [(i - s) // 2 for i, s in zip(K.IN, K.OUT)]
    crop = (slice(None), slice(None), slice(o[1], o[1] + K.OUT[1]), slice(o[2], o[2] + K.OUT[2]))
    assert torch.equal(torch.from_numpy(got_d[3]), torch.from_numpy(data[3][crop]))
    assert torch.equal(torch.from_numpy(got_s[3]), torch.from_numpy(seg[3][crop]))


@pytest.mark.parametrize("shape_in, shape_out", [((3, 21, 13), (3, 17, 9)), ((1, 21, 13), (1, 17, 9))], ids=["mostly-outside", "one-slice"])
def test_k31_edge_shapes(shape_in, shape_out):
    """Planes smaller than a block tile in z and ragged in y, rotation -2.2 with scale 1.37: much of the output leaves the input."""
    data, seg = K.volumes(seed=2, shape=shape_in, batch=2)
    p = K.spatial_params([-2.2, 0.7], [1.37, None])
    assert K.outside_share(p, 0, shape_in[1:], shape_out[1:]) > 0.2
    got_d, got_s = _device(p, data, seg, np.zeros((2, K.C) + shape_out, np.float32), shape_out)
    want_d, want_s = K.spatial(data, seg, shape_out, p)
    _check(got_d, got_s, want_d, want_s, K.near_half(seg, p, shape_out))
    outside = K.coordinates(p, 0, shape_in[1:], shape_out[1:])
    outside = (outside[0] < 0) | (outside[0] > shape_in[1] - 1) | (outside[1] < 0) | (outside[1] > shape_in[2] - 1)
    assert (got_d[0][:, :, outside] == 0).all() and (got_s[0][:, :, outside] == 0).all()


def test_k31_labels_only_over_two_launches():
    """17 samples, one more than a launch holds, labels only (a cascade batch's second seg channel): the host path's result."""
    n, shape_in, shape_out = 17, (3, 21, 13), (3, 17, 9)
    _, seg = K.volumes(seed=4, shape=shape_in, batch=n)
    angles = [None if b % 5 == 4 else 0.41 * (b + 1) for b in range(n)]          # samples 4, 9, 14 are cropped
    scales = [None if b % 5 == 4 or b % 3 == 0 else 0.7 + 0.04 * b for b in range(n)]
    p = K.spatial_params(angles, scales)
    A, do = AUG3.affines(p, shape_in[1:], shape_out[1:])
    assert do.sum() == 14
    out, lab = ops.aug3d_resample_planar(None, torch.from_numpy(seg).cuda().to(torch.int16), A, do, shape_out[1:])
    assert out is None and lab.shape == (n, 1) + shape_out
    data = np.zeros((n, 1) + shape_in, np.float32)
    _, host = AUG3.spatial_transform_dummy_2d(torch.from_numpy(data), torch.from_numpy(seg), shape_out, p)
    near = K.near_half(seg, p, shape_out)
    assert near.mean() <= NEAR_CAP
    assert np.array_equal(lab.cpu().numpy()[~near], host.numpy()[~near])
    assert np.array_equal(lab.cpu().numpy()[16], host.numpy()[16]) and len(np.unique(host.numpy()[16])) >= 2


def test_k31_is_run_to_run_identical_and_refuses_bad_arguments():
    data, seg = K.volumes(seed=3)
    p = K.only(K.forced_params(seed=4), ["do_rot", "do_scale"])
    A, do = AUG3.affines(p, K.IN[1:], K.OUT[1:])
    vol = AUG3._prefiltered(torch.from_numpy(data).cuda(), do, 2)
    lab = torch.from_numpy(seg).cuda().to(torch.int16)
    a = ops.aug3d_resample_planar(vol, lab, A, do, K.OUT[1:])
    b = ops.aug3d_resample_planar(vol, lab, A, do, K.OUT[1:])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(RuntimeError, match="int16"):
        ops.aug3d_resample_planar(vol, lab.float(), A, do, K.OUT[1:])
    with pytest.raises(RuntimeError, match="resample flags"):
        ops.aug3d_resample_planar(vol, lab, A, do[:3], K.OUT[1:])
    with pytest.raises(RuntimeError, match="cropped sample"):
        ops.aug3d_resample_planar(vol, lab, A, do, (K.IN[1] + 1, K.OUT[2]))


@pytest.mark.parametrize("keys", [["do_blur"], ["do_lowres"], None], ids=["blur", "lowres", "chain"])
def test_device_transforms_match_the_oracle(keys):
    shape = K.OUT if keys is not None else K.IN
    data, seg = K.volumes(shape=shape)
    data = K.ramped(data)
    p = K.forced_params() if keys is None else K.only(K.forced_params(), keys)
    noise = np.random.RandomState(5).randn(K.B, K.C, *K.OUT).astype(np.float32)
    got_d, got_s = _device(p, data, seg, noise)
    want_d, want_s = K.apply(data.copy(), seg.copy(), K.OUT, p, noise)
    near = K.near_half(seg, p) if keys is None else np.zeros_like(got_s, dtype=bool)
    _check(got_d, got_s, want_d, want_s, near)
    if keys is not None:
        assert np.abs(got_d - data).max() > 1e-3


def test_cascade_batch_second_seg_channel():
    data, seg = K.volumes()
    seg2 = np.concatenate([seg, K.volumes(seed=7)[1].clip(0, 4)], 1)
    p = K.only(K.forced_params(), ["do_rot", "do_scale"])
    got_d, got_s = AUG3.spatial_transform_dummy_2d(torch.from_numpy(data).cuda(), torch.from_numpy(seg2).cuda().to(torch.int16), K.OUT, p)
    want_d, want_s = K.spatial(data, seg2, K.OUT, p)
    assert got_s.shape == (K.B, 2) + K.OUT
    for c in range(2):
        _check(got_d.cpu().numpy(), got_s.cpu().numpy()[:, c:c + 1], want_d, want_s[:, c:c + 1], K.near_half(seg2, p, channel=c))


def test_plan_driven_prefetch_serves_an_anisotropic_plan(tmp_path):
    KD.write_dataset_3d(str(tmp_path), unpack=True)
    patch = (4, 16, 16)
    aug = AUG3.GpuAugmenter3D.for_plan(patch, "cuda:0", seed=3, labels=KD.LABELS)
    assert aug.dummy_2d and aug.initial_patch_size()[0] == 4
    dl = DL.DataLoader3D(DL.Dataset(str(tmp_path)), 2, aug.initial_patch_size(), patch, KD.LABELS, 0.33)
    scales = [[1, 1, 1], [1, .5, .5], [1, .25, .25]]
    feed = DL.PrefetchLoader(dl, "cuda:0", num_workers=2, depth=2, augmenter=aug, ds_scales=scales)
    try:
        for _ in range(2):
            data, target = feed.next()
            assert data.is_cuda and data.shape == (2, 1) + patch and data.dtype == torch.float32 and torch.isfinite(data).all()
            assert [tuple(t.shape[2:]) for t in target] == [(4, 16, 16), (4, 8, 8), (4, 4, 4)]
            assert all(t.dtype == torch.float32 and set(torch.unique(t).tolist()) <= {0.0, 1.0, 2.0, 3.0} for t in target)
    finally:
        feed.close()
