"""Dummy-2-D augmentation of anisotropic 3-D patches (reference nnUNetTrainer.py:378-404 and 658-690 with do_dummy_2d_data_aug): the
configuration, the parameter draw order, and the host path of mlagg-unet_amd/augmentation3d.py against the scipy float64
restatement (tests/_augmentation_dummy2d_cases.py) with identical parameters.  Data within 5e-5 on amplitude-5 volumes; labels
identical except where the float64 indicator lies within 1e-4 of 0.5, at most 0.5 % of the voxels."""
import math

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import augmentation3d as AUG3
from mlagg_unet_amd import dataloading as DL
from tests import _augmentation_dummy2d_cases as K
from tests import _dataloading_3d_cases as KD

TOL = 5e-5
NEAR_CAP = 0.005            # share of label voxels a test may exclude as "within 1e-4 of 0.5"


def test_configure_3d_both_branches():
    rotation, dummy, initial, mirror = AUG3.configure_3d((20, 256, 224))               # the ACDC 3d_fullres plan
    assert dummy and rotation == ((-math.pi, math.pi), (0, 0), (0, 0)) and initial == (20, 301, 301) and mirror == (0, 1, 2)
    r = 30 / 360 * 2 * math.pi
    rotation, dummy, initial, mirror = AUG3.configure_3d((96, 160, 160))               # BTCV
    assert not dummy and rotation == ((-r, r),) * 3 and initial == (191, 257, 219) and mirror == (0, 1, 2)
    assert AUG3.configure_3d((40, 120, 100))[1] is False                               # exactly 3 is not above the threshold


def test_dummy_2d_augmenter_configuration():
    aug = AUG3.GpuAugmenter3D((16, 160, 160), "cpu", dummy_2d=True)
    assert aug.rotation == ((-math.pi, math.pi), (0, 0), (0, 0)) and aug.initial_patch_size() == (16, 188, 188)
    plan = AUG3.GpuAugmenter3D.for_plan((16, 160, 160), "cpu", seed=1)
    assert plan.dummy_2d and plan.rotation == aug.rotation and plan.initial_patch_size() == (16, 188, 188)
    assert plan.clone(2).dummy_2d and plan.clone(2).initial_patch_size() == (16, 188, 188)
    iso = AUG3.GpuAugmenter3D.for_plan((96, 160, 160), "cpu")
    assert not iso.dummy_2d and not iso.clone(0).dummy_2d and iso.initial_patch_size() == (191, 257, 219)
    with pytest.raises(NotImplementedError, match="dummy-2-D"):                         # the default mode is unchanged
        AUG3.GpuAugmenter3D((16, 160, 160), "cpu")


def test_draw_order_is_batchgenerators_2d_then_3d():
    """draw_params_dummy_2d against a hand-unrolled draw sequence on the same RandomState: one angle per sample, per-channel draws
    over C channels, three mirror flags."""
    B, C = 40, 2
    p = AUG3.draw_params_dummy_2d(np.random.RandomState(9), B, C)
    assert p["angle"].shape == (B,) and p["mirror"].shape == (B, 3)
    r = np.random.RandomState(9)
    for b in range(B):
        rot = r.uniform() < 0.2
        ang = 0.0
        if rot:
            assert r.uniform() <= 1.0
            ang = r.uniform(-math.pi, math.pi)
        assert p["do_rot"][b] == rot and p["angle"][b] == ang
        sc = r.uniform() < 0.2
        if sc:
            v = r.uniform(0.7, 1) if (r.random_sample() < 0.5) else r.uniform(1, 1.4)
            assert p["scale"][b] == v
        assert p["do_scale"][b] == sc
    for b in range(B):
        if r.uniform() < 0.1:
            assert p["noise_std"][b] == r.uniform(0, 0.1)
    for b in range(B):
        if r.uniform() < 0.2:
            for c in range(C):
                if r.uniform() <= 0.5:
                    assert p["blur_sigma"][b, c] == r.uniform(0.5, 1.0)
    for b in range(B):
        if r.uniform() < 0.15:
            assert list(p["bright"][b]) == [r.uniform(0.75, 1.25) for _ in range(C)]
    for b in range(B):
        if r.uniform() < 0.15:
            for c in range(C):
                r.uniform()
                v = r.uniform(0.75, 1) if r.random_sample() < 0.5 else r.uniform(1, 1.25)
                assert p["contrast"][b, c] == v
    for b in range(B):
        if r.uniform() < 0.25:
            for c in range(C):
                if r.uniform() < 0.5:
                    assert p["lowres_zoom"][b, c] == r.uniform(0.5, 1.0)
    for key, prob in (("gamma_inv", 0.1), ("gamma", 0.3)):
        for b in range(B):
            if r.uniform() < prob:
                for c in range(C):
                    v = r.uniform(0.7, 1) if r.random_sample() < 0.5 else r.uniform(1, 1.5)
                    assert p[key][b, c] == v
    for b in range(B):
        assert list(p["mirror"][b]) == [r.uniform() < 0.5 for _ in range(3)]
    assert p["do_rot"].any() and p["do_scale"].any()
    # the parameter stream ends where the hand-unrolled one ends, and the augmenter draws this stream
    q = np.random.RandomState(9)
    AUG3.draw_params_dummy_2d(q, B, C)
    assert q.uniform() == r.uniform()


def test_planar_affine_matches_the_oracle_coordinates():
    p = K.forced_params()
    A, do = AUG3.affines(p, K.IN[1:], K.OUT[1:])
    assert A.shape == (K.B, 2, 3) and A.dtype == np.float64
    grid = np.stack(np.meshgrid(*[np.arange(n) for n in K.OUT[1:]], indexing="ij")).reshape(2, -1).astype(float)
    for b in range(K.B):
        want = K.coordinates(p, b, K.IN[1:], K.OUT[1:])
        assert do[b] == (want is not None)
        if want is not None:
            assert np.abs(A[b, :, :2] @ grid + A[b, :, 2:] - want.reshape(2, -1)).max() < 1e-12
    assert 0.005 < K.outside_share(p, 2, K.IN[1:], K.OUT[1:]) < 0.03          # the rotated and zoomed-out sample leaves the input


def _run(p, data, seg, noise):
    aug = AUG3.GpuAugmenter3D(K.OUT, "cpu", labels=K.LABELS, dummy_2d=True)
    got_d, got_s = aug.apply(torch.from_numpy(data), torch.from_numpy(seg), p, torch.from_numpy(noise))
    want_d, want_s = K.apply(data.copy(), seg.copy(), K.OUT, p, noise)
    return got_d.numpy(), got_s.numpy(), want_d, want_s


def _check_labels(got_s, want_s, near):
    share = near.mean()
    print(f"label voxels within 1e-4 of 0.5: {int(near.sum())} of {near.size}")
    assert share <= NEAR_CAP
    assert np.array_equal(got_s[~near], want_s[~near]), int((got_s != want_s).sum())


@pytest.mark.parametrize("keys", [["do_rot", "do_scale"], ["do_lowres"], None], ids=["spatial", "lowres", "chain"])
def test_host_path_matches_the_oracle(keys):
    spatial = keys is None or keys[0] == "do_rot"
    data, seg = K.volumes(shape=K.IN if spatial else K.OUT)
    data = K.ramped(data)
    p = K.forced_params() if keys is None else K.only(K.forced_params(), keys)
    noise = np.random.RandomState(5).randn(K.B, K.C, *K.OUT).astype(np.float32)
    got_d, got_s, want_d, want_s = _run(p, data, seg, noise)
    err = np.abs(got_d - want_d).max()
    print(f"max |host - oracle| = {err:.3g}")
    assert err < TOL
    if spatial:
        _check_labels(got_s, want_s, K.near_half(seg, p))
        assert set(np.unique(want_s)) <= {-1.0, 0.0, 1.0, 2.0, 3.0, 4.0} and len(np.unique(want_s)) >= 4
    else:
        assert np.array_equal(got_s, want_s)
        assert np.abs(got_d - data).max() > 1e-3                     # the transform did something
        # the case tells the volume clip from a per-slice clip, and the planar mode from the isotropic one
        assert np.abs(K.low_resolution(data, p, per_slice_clip=True) - want_d).max() > 100 * TOL
        do = torch.from_numpy(p["lowres_ch"] & p["do_lowres"][:, None])
        iso = AUG3.simulate_low_resolution_3d(torch.from_numpy(data), do.numpy(), p["lowres_zoom"]).numpy()
        assert np.abs(iso - want_d).max() > 100 * TOL


def test_planar_differs_from_the_3d_transform():
    """The same angle about x through the 3-D chain (prefilter and cubic taps along x too) blurs across slices: not this mode."""
    data, seg = K.volumes()
    p = K.only(K.forced_params(), ["do_rot", "do_scale"])
    got_d, _, want_d, _ = _run(p, data, seg, np.zeros((K.B, K.C) + K.OUT, np.float32))
    q = dict(p, angle=np.stack([p["angle"], np.zeros(K.B), np.zeros(K.B)], 1))
    iso_d, _ = AUG3.spatial_transform_3d(torch.from_numpy(data), torch.from_numpy(seg), K.OUT, q)
    assert np.abs(got_d - want_d).max() < TOL and np.abs(iso_d.numpy()[:3] - want_d[:3]).max() > 100 * TOL


def test_centre_crop_is_bit_exact_and_outside_is_zero():
    data, seg = K.volumes()
    p = K.only(K.forced_params(), ["do_scale"])
    p["do_scale"][:] = [True, True, False, False]
    p["scale"][:2] = [2.5, 1.0]                                         # 2.5: the grid leaves the input; 1.0: a resample at integers
    got_d, got_s, want_d, want_s = _run(p, data, seg, np.zeros((K.B, K.C) + K.OUT, np.float32))
    o = [(i - s) // 2 for i, s in zip(K.IN, K.OUT)]
    crop = (slice(None), slice(o[1], o[1] + K.OUT[1]), slice(o[2], o[2] + K.OUT[2]))
    assert np.array_equal(got_d[2:], data[(slice(2, None), slice(None)) + crop])
    assert np.array_equal(got_s[2:], seg[(slice(2, None), slice(None)) + crop])
    assert (got_d[0, :, :, 0, 0] == 0).all() and (got_s[0, 0, :, 0, 0] == 0).all()      # outside: cval 0, no label assigned
    assert np.abs(got_d - want_d).max() < TOL and np.array_equal(got_s, want_s)


def test_two_channel_seg_of_a_cascade_batch():
    """Both seg channels go through the planar transform with the same map: against the oracle on 2 * X label channels."""
    data, seg = K.volumes()
    prev = K.volumes(seed=7)[1].clip(0, 4)
    seg2 = np.concatenate([seg, prev], 1)
    p = K.only(K.forced_params(), ["do_rot", "do_scale"])
    got_d, got_s = AUG3.spatial_transform_dummy_2d(torch.from_numpy(data), torch.from_numpy(seg2), K.OUT, p)
    want_d, want_s = K.spatial(data, seg2, K.OUT, p)
    assert got_s.shape == (K.B, 2) + K.OUT and np.abs(got_d.numpy() - want_d).max() < TOL
    for c in range(2):
        _check_labels(got_s.numpy()[:, c:c + 1], want_s[:, c:c + 1], K.near_half(seg2, p, channel=c))
    assert not np.array_equal(want_s[:, 0], want_s[:, 1])


def test_cascade_chain_runs_in_dummy_2d_mode():
    data, seg = K.volumes()
    seg2 = np.concatenate([seg, K.volumes(seed=7)[1].clip(0, 4)], 1)
    aug = AUG3.GpuAugmenter3D(K.OUT, "cpu", seed=2, cascade_labels=(1, 2, 3, 4), dummy_2d=True)
    d, s = aug(torch.from_numpy(data), torch.from_numpy(seg2))
    assert d.shape == (K.B, K.C + 4) + K.OUT and s.shape == (K.B, 1) + K.OUT and torch.isfinite(d).all()
    assert set(torch.unique(d[:, K.C:]).tolist()) <= {0.0, 1.0}


def test_loader_with_plan_driven_augmenter_on_cpu(tmp_path):
    KD.write_dataset_3d(str(tmp_path), unpack=True)
    aug = AUG3.GpuAugmenter3D.for_plan((4, 16, 16), "cpu", seed=3, labels=KD.LABELS)
    assert aug.dummy_2d and aug.initial_patch_size()[0] == 4
    dl = DL.DataLoader3D(DL.Dataset(str(tmp_path)), 2, aug.initial_patch_size(), (4, 16, 16), KD.LABELS, 0.33,
                         rng=np.random.RandomState(1), pin_memory=False)
    scales = [[1, 1, 1], [1, .5, .5], [1, .25, .25]]
    feed = DL.PrefetchLoader(dl, "cpu", num_workers=2, depth=2, augmenter=aug, ds_scales=scales)
    try:
        for _ in range(3):
            data, targets = feed.next()
            assert data.shape == (2, 1, 4, 16, 16) and data.dtype == torch.float32 and torch.isfinite(data).all()
            assert [tuple(t.shape[2:]) for t in targets] == [(4, 16, 16), (4, 8, 8), (4, 4, 4)]
            assert all(set(torch.unique(t).tolist()) <= {0.0, 1.0, 2.0, 3.0} for t in targets)
    finally:
        feed.close()
