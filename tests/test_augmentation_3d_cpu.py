"""3-D training augmentation (reference nnUNetTrainer.get_training_transforms B:645-733, 3-D configuration): the parameter
draw order, and the host path of mlagg-unet_amd/augmentation3d.py against the scipy float64 restatement
(tests/_augmentation_3d_oracle.py; batchgenerators is third-party, unpinned) with identical parameters.  Data within 5e-5 on
amplitude-5 volumes; labels identical except where the float64 indicator lies within 1e-4 of 0.5."""
import math

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import augmentation3d as AUG3
from mlagg_unet_amd import dataloading as DL
from tests import _augmentation_3d_cases as K
from tests import _augmentation_3d_oracle as AO3
from tests import _dataloading_3d_cases as KD

TOL = 5e-5


def test_btcv_initial_patch_and_rotation():
    aug = AUG3.GpuAugmenter3D((96, 160, 160), "cpu")
    r = 30 / 360 * 2 * math.pi
    assert aug.rotation == ((-r, r),) * 3 and aug.mirror_axes == (0, 1, 2)
    assert aug.initial_patch_size() == (191, 257, 219)
    with pytest.raises(NotImplementedError, match="dummy-2-D"):
        AUG3.GpuAugmenter3D((16, 160, 160), "cpu")                    # 160 / 16 > 3


def test_draw_order_is_batchgenerators_3d():
    """draw_params_3d against a hand-unrolled draw sequence on the same RandomState."""
    B, C = 40, 2
    p = AUG3.draw_params_3d(np.random.RandomState(9), B, C)
    r = np.random.RandomState(9)
    lo, hi = -30 / 360 * 2 * math.pi, 30 / 360 * 2 * math.pi
    for b in range(B):
        rot = r.uniform() < 0.2
        ang = [0.0, 0.0, 0.0]
        if rot:
            for ax in range(3):
                assert r.uniform() <= 1.0
                ang[ax] = r.uniform(lo, hi)
        assert p["do_rot"][b] == rot and np.array_equal(p["angle"][b], ang)
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
    # the parameter stream ends where the hand-unrolled one ends
    q = np.random.RandomState(9)
    AUG3.draw_params_3d(q, B, C)
    assert q.uniform() == r.uniform()


def test_affine_matches_the_oracle_coordinates():
    p = K.forced_params()
    A, do = AUG3.affines(p, K.IN, K.OUT)
    grid = np.stack(np.meshgrid(*[np.arange(n) for n in K.OUT], indexing="ij")).reshape(3, -1).astype(float)
    for b in range(K.B):
        want = AO3.coordinates(p, b, K.IN, K.OUT)
        assert do[b] == (want is not None)
        if want is not None:
            got = A[b, :, :3] @ grid + A[b, :, 3:]
            assert np.abs(got - want.reshape(3, -1)).max() < 1e-12


def _run(p, data, seg, noise):
    got_d, got_s = AUG3.GpuAugmenter3D(K.OUT, "cpu", labels=K.LABELS).apply(torch.from_numpy(data), torch.from_numpy(seg), p,
                                                                            torch.from_numpy(noise))
    want_d, want_s = AO3.apply(data.copy(), seg.copy(), K.OUT, p, noise)
    return got_d.numpy(), got_s.numpy(), want_d, want_s


@pytest.mark.parametrize("keys", list(K.STAGES) + [None], ids=lambda k: "chain" if k is None else k[0])
def test_host_path_matches_the_oracle(keys):
    shape = K.OUT if keys is not None and keys[0] != "do_rot" else K.IN
    data, seg = K.volumes(shape=shape)
    p = K.forced_params() if keys is None else K.only(K.forced_params(), keys)
    noise = np.random.RandomState(5).randn(K.B, K.C, *K.OUT).astype(np.float32)
    got_d, got_s, want_d, want_s = _run(p, data, seg, noise)
    assert np.abs(got_d - want_d).max() < TOL
    if keys is None or keys[0] == "do_rot":
        near = K.near_half(seg, p)
        assert np.array_equal(got_s[~near], want_s[~near]), int((got_s != want_s).sum())
        assert set(np.unique(want_s)) <= {-1.0, 0.0, 1.0, 2.0, 3.0, 4.0} and len(np.unique(want_s)) >= 4
    else:
        assert np.array_equal(got_s, want_s)
        assert np.abs(got_d - data).max() > 1e-3                     # the transform did something


def test_crop_samples_and_outside_points():
    data, seg = K.volumes()
    p = K.only(K.forced_params(), ["do_scale"])
    p["do_scale"][:] = [True, True, False, False]
    p["scale"][:2] = [2.5, 1.0]                                         # 2.5: the grid leaves the input; 1.0: a resample at integers
    got_d, got_s, want_d, want_s = _run(p, data, seg, np.zeros((K.B, K.C) + K.OUT, np.float32))
    o = [(i - s) // 2 for i, s in zip(K.IN, K.OUT)]
    crop = (slice(o[0], o[0] + K.OUT[0]), slice(o[1], o[1] + K.OUT[1]), slice(o[2], o[2] + K.OUT[2]))
    assert np.array_equal(got_d[2:], data[(slice(2, None), slice(None)) + crop])
    assert np.array_equal(got_s[2:], seg[(slice(2, None), slice(None)) + crop])
    assert (got_d[0, :, 0, 0, 0] == 0).all() and got_s[0, 0, 0, 0, 0] == 0          # outside: cval 0, no label assigned
    assert np.abs(got_d - want_d).max() < TOL and np.array_equal(got_s, want_s)


def test_loader_with_3d_augmenter_on_cpu(tmp_path):
    KD.write_dataset_3d(str(tmp_path), unpack=True)
    aug = AUG3.GpuAugmenter3D((8, 12, 12), "cpu", seed=3, labels=KD.LABELS)
    init = aug.initial_patch_size()
    dl = DL.DataLoader3D(DL.Dataset(str(tmp_path)), 2, init, (8, 12, 12), KD.LABELS, 0.33, rng=np.random.RandomState(1),
                         pin_memory=False)
    scales = [[1, 1, 1], [.5, .5, .5], [.25, .25, .25]]
    feed = DL.PrefetchLoader(dl, "cpu", num_workers=2, depth=2, augmenter=aug, ds_scales=scales)
    try:
        for _ in range(3):
            data, targets = feed.next()
            assert data.shape == (2, 1, 8, 12, 12) and data.dtype == torch.float32 and torch.isfinite(data).all()
            assert [tuple(t.shape[2:]) for t in targets] == [(8, 12, 12), (4, 6, 6), (2, 3, 3)]
            assert all(set(torch.unique(t).tolist()) <= {0.0, 1.0, 2.0, 3.0} for t in targets)
    finally:
        feed.close()
