"""3-D real-data input path: DataLoader3D against the reference nnUNetDataLoader3D's own batches
(tests/golden/dataloader_3d.npz, numpy seeded), the per-axis deep-supervision target pyramid, PrefetchLoader on 3-D batches."""
import os

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import dataloading as DL
from mlagg_unet_amd import model3d
from oracle import dataloading_oracle as DO
from tests import _dataloading_3d_cases as K

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "dataloader_3d.npz"))


@pytest.mark.parametrize("tag", ["npz", "npy", "ign"])
def test_loader_reproduces_reference_batches(tag, tmp_path):
    unpack, patch, final, bs, fg = K.CASES[tag]
    ign = tag == "ign"
    K.write_dataset_3d(str(tmp_path), unpack=unpack, ignore_label=4 if ign else None)
    dl = DL.DataLoader3D(DL.Dataset(str(tmp_path)), bs, patch, final, K.LABELS, fg, pin_memory=False, has_ignore=ign)
    np.random.seed(11)
    for it in range(3):
        b = dl.generate_train_batch()
        assert [str(k) for k in b["keys"]] == list(GOLD[f"{tag}_keys_{it}"])
        assert b["data"].dtype == torch.float32 and b["seg"].dtype == torch.int16
        assert np.array_equal(b["data"].numpy(), GOLD[f"{tag}_data_{it}"])
        assert np.array_equal(b["seg"].numpy(), GOLD[f"{tag}_seg_{it}"])
    assert any((GOLD[f"{tag}_seg_{it}"] == -1).any() for it in range(3))
    assert any((GOLD[f"{tag}_seg_{it}"] > 0).any() for it in range(3))
    if ign:
        assert any((GOLD[f"ign_seg_{it}"] == 4).any() for it in range(3))


def test_case_smaller_than_the_patch_is_padded(tmp_path):
    K.write_dataset_3d(str(tmp_path), unpack=True)
    ds = DL.Dataset(str(tmp_path), ["case_002"])                      # x extent 5 < patch 8
    dl = DL.DataLoader3D(ds, 2, (8, 12, 12), (8, 12, 12), K.LABELS, 0.0, rng=np.random.RandomState(0), pin_memory=False)
    b = dl.generate_train_batch()
    for j in range(2):
        d, s = b["data"][j, 0].numpy(), b["seg"][j, 0].numpy()
        # 3 planes of padding along x, split -3 // 2 = -2 <= lb <= -1: the case's 5 planes sit at offset 1 or 2
        pad = [x for x in range(8) if (d[x] == 0).all() and (s[x] == -1).all()]
        assert len(pad) == 3
        o = 2 if pad[:2] == [0, 1] else 1
        assert pad == [x for x in range(8) if not o <= x < o + 5]
        assert (s[o:o + 5] != -1).any() and (d[o:o + 5] != 0).any()


def test_case_without_foreground_falls_back_to_a_random_box(tmp_path):
    K.write_dataset_3d(str(tmp_path), unpack=True)
    ds = DL.Dataset(str(tmp_path), ["case_001"])                      # no foreground: class_locations all empty
    dl = DL.DataLoader3D(ds, 3, (8, 12, 12), (8, 12, 12), K.LABELS, 1.0, rng=np.random.RandomState(2), pin_memory=False)
    data, seg = ds.arrays("case_001")
    rng = np.random.RandomState(2)
    rng.choice(ds.keys(), 3, replace=True)
    b = dl.generate_train_batch()
    for j in range(3):
        lb = [rng.randint(0, n - p + 1) for n, p in zip(data.shape[1:], (8, 12, 12))]
        want = data[0, lb[0]:lb[0] + 8, lb[1]:lb[1] + 12, lb[2]:lb[2] + 12]
        assert np.array_equal(b["data"][j, 0].numpy(), want)


def test_oversampled_samples_contain_foreground(tmp_path):
    K.write_dataset_3d(str(tmp_path), unpack=True)
    ds = DL.Dataset(str(tmp_path), ["case_000", "case_003"])
    dl = DL.DataLoader3D(ds, 4, (6, 8, 8), (6, 8, 8), K.LABELS, 1.0, rng=np.random.RandomState(0), pin_memory=False)
    for _ in range(5):
        b = dl.generate_train_batch()
        assert all((b["seg"][j] > 0).any() for j in range(4))


def test_out_of_range_label_is_refused(tmp_path):
    K.write_dataset_3d(str(tmp_path), unpack=True)
    dl = DL.DataLoader3D(DL.Dataset(str(tmp_path)), 4, (8, 12, 12), (8, 12, 12), [0, 1, 2], 1.0,
                         rng=np.random.RandomState(0), pin_memory=False)
    with pytest.raises(RuntimeError, match="segmentation label 3 > 2"):
        for _ in range(20):
            dl.generate_train_batch()


def _nearest_exact(seg, shape):
    """numpy restatement of nearest-exact (half-pixel) down-sampling: source index floor((i + 0.5) * n / m)."""
    idx = [np.minimum(np.floor((np.arange(m) + 0.5) * (n / m)).astype(int), n - 1) for n, m in zip(seg.shape[2:], shape)]
    return seg[:, :, idx[0]][:, :, :, idx[1]][:, :, :, :, idx[2]]


def test_anisotropic_target_pyramid():
    rng = np.random.RandomState(3)
    seg = rng.randint(-1, 5, (2, 1, 12, 20, 18)).astype(np.float32)
    scales = model3d.deep_supervision_scales([[1, 1, 1], [1, 2, 2], [2, 2, 2], [2, 2, 2], [1, 2, 2]])
    assert scales[1] == [1.0, 0.5, 0.5]
    targets = DL.targets_from_seg(torch.from_numpy(seg), ds_scales=scales)
    clean = np.where(seg < 0, 0, seg)
    assert np.array_equal(targets[0].numpy(), clean)
    for sc, t in zip(scales, targets):
        shape = tuple(int(v) for v in np.round(np.array(seg.shape[2:]) * np.array(sc)))
        assert tuple(t.shape[2:]) == shape
        assert np.array_equal(t.numpy(), _nearest_exact(clean, shape))
    # the reference transform chain's own restatement (RemoveLabel + DownsampleSegForDSTransform2, order 0)
    for got, want in zip(targets, DO.downsample_seg_for_ds(seg, scales)):
        assert np.array_equal(got.numpy(), want)
    with pytest.raises(RuntimeError, match="3-D segmentation"):
        DL.targets_from_seg(torch.from_numpy(seg), ds_scales=[[1, 1]])


def test_prefetch_loader_with_a_3d_loader(tmp_path):
    K.write_dataset_3d(str(tmp_path), unpack=True)
    dl = DL.DataLoader3D(DL.Dataset(str(tmp_path)), 2, (8, 12, 12), (8, 12, 12), K.LABELS, 0.5, pin_memory=False)
    scales = [[1, 1, 1], [1, .5, .5], [.5, .25, .25]]
    pf = DL.PrefetchLoader(dl, "cpu", num_workers=2, depth=2, ds_scales=scales)
    try:
        for _ in range(4):
            data, targets = pf.next()
            assert data.shape == (2, 1, 8, 12, 12) and torch.isfinite(data).all()
            assert [tuple(t.shape[2:]) for t in targets] == [(8, 12, 12), (8, 6, 6), (4, 3, 3)]
            assert all(float(t.min()) >= 0 and float(t.max()) <= 3 for t in targets)
    finally:
        pf.close()
    # the workers' loaders are clones: same class, own random state
    twin = dl.clone(np.random.RandomState(5))
    assert type(twin) is DL.DataLoader3D and twin.patch_size == dl.patch_size and twin.rng is not dl.rng
