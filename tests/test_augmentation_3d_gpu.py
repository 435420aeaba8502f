"""GPU: K25 (csrc/augment3d.hip) and the 3-D augmentation chain on HBM-resident batches against the scipy float64 oracle
(tests/_augmentation_3d_oracle.py), a BTCV-sized resample checked on random voxels, and the 3-D input path (DataLoader3D +
GpuAugmenter3D on the PrefetchLoader's side stream) in front of UMambaEnc train steps."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import augmentation3d as AUG3
from mlagg_unet_amd import dataloading as DL
from mlagg_unet_amd import ops
from tests import _augmentation_3d_cases as K
from tests import _augmentation_3d_oracle as AO3
from tests import _dataloading_3d_cases as KD

pytestmark = pytest.mark.gpu
TOL = 5e-5                  # fp32 prefilter GEMMs and fp32 tap sums against float64 scipy, volumes of amplitude ~5


def _device(p, data, seg, noise, seg_dtype=torch.int16):
    aug = AUG3.GpuAugmenter3D(K.OUT, "cuda:0", labels=K.LABELS)
    d, s = aug.apply(torch.from_numpy(data).cuda(), torch.from_numpy(seg).cuda().to(seg_dtype), p, torch.from_numpy(noise).cuda())
    assert d.is_cuda and s.is_cuda and d.dtype == torch.float32 and s.dtype == torch.float32
    return d.cpu().numpy(), s.cpu().numpy()


def test_k25_resample_matches_the_oracle():
    data, seg = K.volumes()
    p = K.only(K.forced_params(), ["do_rot", "do_scale"])
    got_d, got_s = _device(p, data, seg, np.zeros((K.B, K.C) + K.OUT, np.float32))
    want_d, want_s = AO3.spatial(data, seg, K.OUT, p)
    assert np.abs(got_d - want_d).max() < TOL
    near = K.near_half(seg, p)
    print(f"voxels with a float64 indicator within 1e-4 of 0.5: {int(near.sum())}")
    assert np.array_equal(got_s[~near], want_s[~near]), int((got_s != want_s).sum())
    # samples 3 neither rotates nor scales: the centre crop, bit for bit
    o = [(i - s) // 2 for i, s in zip(K.IN, K.OUT)]
    crop = (slice(o[0], o[0] + K.OUT[0]), slice(o[1], o[1] + K.OUT[1]), slice(o[2], o[2] + K.OUT[2]))
    assert torch.equal(torch.from_numpy(got_d[3]), torch.from_numpy(data[3][(slice(None),) + crop]))
    assert torch.equal(torch.from_numpy(got_s[3]), torch.from_numpy(seg[3][(slice(None),) + crop]))


def test_k25_is_run_to_run_identical():
    data, seg = K.volumes(seed=3)
    p = K.only(K.forced_params(seed=4), ["do_rot", "do_scale"])
    A, do = AUG3.affines(p, K.IN, K.OUT)
    vol = AUG3._prefiltered(torch.from_numpy(data).cuda(), do)
    lab = torch.from_numpy(seg).cuda().to(torch.int16)
    a = ops.aug3d_resample(vol, lab, A, do, K.OUT)
    b = ops.aug3d_resample(vol, lab, A, do, K.OUT)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(RuntimeError, match="int16"):
        ops.aug3d_resample(vol, lab.float(), A, do, K.OUT)


@pytest.mark.parametrize("keys", [["do_blur"], ["do_lowres"], None], ids=["blur", "lowres", "chain"])
def test_device_transforms_match_the_oracle(keys):
    shape = K.OUT if keys is not None else K.IN
    data, seg = K.volumes(shape=shape)
    p = K.forced_params() if keys is None else K.only(K.forced_params(), keys)
    noise = np.random.RandomState(5).randn(K.B, K.C, *K.OUT).astype(np.float32)
    got_d, got_s = _device(p, data, seg, noise)
    want_d, want_s = AO3.apply(data.copy(), seg.copy(), K.OUT, p, noise)
    assert np.abs(got_d - want_d).max() < TOL
    near = K.near_half(seg, p) if keys is None else np.zeros_like(got_s, dtype=bool)
    assert np.array_equal(got_s[~near], want_s[~near])
    if keys is not None:
        assert np.abs(got_d - data).max() > 1e-3


def _btcv_case():
    shape, B = (191, 257, 219), 2
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij", sparse=True)
    data = np.stack([5 * np.sin(x / 6.0 + b) * np.cos(y / 9.0) + 2 * np.sin(z / 5.0 + 2 * b) for b in range(B)])[:, None]
    f = (np.sin(x / 13.0) + np.cos(y / 17.0 + 1) + np.sin(z / 11.0) + 3.0) / 6.0
    seg = np.stack([np.floor(np.clip(f + 0.03 * b, 0, 0.999) * 14) for b in range(B)])[:, None].astype(np.int16)
    seg[:, :, :, :6, :] = -1                                           # outside the nonzero region
    return data.astype(np.float32), seg


def test_btcv_sized_resample_on_random_voxels():
    """2 x 191x257x219 -> 96x160x160, rotation and scale on both samples, 14 labels: 10 000 random output voxels against a float64
    host evaluation (scipy) at the same coordinates."""
    data, seg = _btcv_case()
    out_shape = (96, 160, 160)
    p = AUG3.draw_params_3d(np.random.RandomState(0), 2, 1)
    p["do_rot"][:], p["do_scale"][:] = True, True
    p["angle"][:] = [[0.41, -0.27, 0.33], [-0.5, 0.19, -0.44]]
    p["scale"][:] = [0.74, 1.37]
    A, do = AUG3.affines(p, data.shape[2:], out_shape)
    vol = AUG3._prefiltered(torch.from_numpy(data).cuda(), do)
    out, lab = ops.aug3d_resample(vol, torch.from_numpy(seg).cuda(), A, do, out_shape)
    rng = np.random.RandomState(1)
    idx = np.stack([rng.randint(0, n, 10000) for n in out_shape])
    got_d, got_s = out.cpu().numpy(), lab.cpu().numpy()
    n_near = 0
    for b in range(2):
        coords = AO3.coordinates(p, b, data.shape[2:], out_shape)[:, idx[0], idx[1], idx[2]]
        want = ndimage.map_coordinates(data[b, 0].astype(np.float64), coords, order=3, mode="constant", cval=0.0)
        assert np.abs(got_d[b, 0][tuple(idx)] - want).max() < TOL
        labels, r = AO3.segmentation_indicators(seg[b, 0], coords)
        want_s = np.zeros(coords.shape[1])
        for k, c in enumerate(labels):
            want_s[r[k] >= 0.5] = c
        near = (np.abs(r - 0.5) < 1e-4).any(0)
        n_near += int(near.sum())
        assert np.array_equal(got_s[b, 0][tuple(idx)][~near], want_s[~near])
        assert len(np.unique(want_s)) >= 10
    print(f"BTCV case: {n_near} of 20000 checked voxels within 1e-4 of 0.5")


def test_augmented_3d_prefetch_drives_umamba_train_steps(tmp_path):
    from mlagg_unet_amd import model3d, trainer
    KD.write_dataset_3d(str(tmp_path), unpack=True)
    patch, strides = (24, 64, 64), [[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2], [1, 2, 2], [1, 2, 2]]
    aug = AUG3.GpuAugmenter3D(patch, "cuda:0", seed=3, labels=KD.LABELS)
    dl = DL.DataLoader3D(DL.Dataset(str(tmp_path)), 2, aug.initial_patch_size(), patch, KD.LABELS, 0.33)
    scales = model3d.deep_supervision_scales(strides)
    feed = DL.PrefetchLoader(dl, "cuda:0", num_workers=2, depth=2, augmenter=aug, ds_scales=scales)
    try:
        torch.manual_seed(0)
        n = len(strides)
        net = model3d.build_network_architecture_3d(1, 4, [[3, 3, 3]] * n, strides, [2] * n, [2] * (n - 1)).cuda().train()
        opt = torch.optim.SGD(net.parameters(), 1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)
        for _ in range(2):
            data, target = feed.next()
            assert data.shape == (2, 1) + patch
            assert [tuple(t.shape[2:]) for t in target] == [(24, 64, 64), (12, 32, 32), (6, 16, 16), (3, 8, 8), (3, 4, 4)]
            assert all(float(t.min()) >= 0 and float(t.max()) <= 3 for t in target)
            loss = trainer.train_step(net, opt, data, target, batch_dice=False)
        assert torch.isfinite(loss).item()
    finally:
        feed.close()
