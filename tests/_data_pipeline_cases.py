"""Shared by tests/test_plugin_data_pipeline_cpu.py and _gpu.py: tiny preprocessed folders (written by the test), the trainer classes
built with data_pipeline="device" on the stand-in base of tests/fake_nnunet_data.py, and the checks, which take the device."""
import os

import numpy as np
import torch

import fake_nnunet as FK
import fake_nnunet_data as FD
from _cascade_cases import write_previous_stage
from _dataloading_3d_cases import write_dataset_3d

REGIONS = [(1, 2, 3), (2, 3), (3,)]
SEED = 11
# kind -> (factory, patch, pool strides (3-D plans), data channels, regions, ignore label, use_mask_for_norm, cascade)
KINDS = {
    "2d": ("mlagg", (32, 48), None, 1, None, None, [False], False),
    "3d_dummy2d": ("umamba", (8, 32, 32), [[1, 1, 1], [1, 2, 2], [2, 2, 2]], 1, None, None, [False], False),
    "3d": ("umamba", (16, 16, 16), [[1, 1, 1], [2, 2, 2], [2, 2, 2]], 1, None, None, [False], False),
    "2d_regions_mask": ("mlagg", (32, 48), None, 2, REGIONS, 4, [True, False], False),
    "3d_cascade": ("umamba", (16, 16, 16), [[1, 1, 1], [2, 2, 2], [2, 2, 2]], 1, None, None, [True], True),
}


def write_folder(root, kind):
    """The case folder of `kind` (and the previous stage's predictions for a cascade); returns the `data` description of
    fake_nnunet_data.with_data."""
    _, _, _, channels, regions, ignore, use_mask, cascade = KINDS[kind]
    folder = os.path.join(root, kind)
    write_dataset_3d(folder, unpack=True, ignore_label=ignore)
    names = sorted(f[:-4] for f in os.listdir(folder) if f.endswith(".npz"))
    if channels > 1:                                           # a second image channel: the first one, negated and shifted
        for name in names:
            case = np.load(os.path.join(folder, name + ".npz"))
            data = np.concatenate([case["data"]] + [-case["data"] + c for c in range(1, channels)], 0)
            np.savez_compressed(os.path.join(folder, name + ".npz"), data=data, seg=case["seg"])
            np.save(os.path.join(folder, name + ".npy"), data)
    desc = dict(folder=folder, split=(names[:3], names[2:]), labels=[0, 1, 2, 3], regions=regions, ignore_label=ignore,
                use_mask_for_norm=use_mask)
    if cascade:
        desc["previous_stage_folder"] = os.path.join(root, kind + "_previous_stage")
        write_previous_stage(desc["previous_stage_folder"], folder, unpack=True)
    return desc


def trainer_class(kind, desc, data_pipeline="device", base=None, **kw):
    from mlagg_unet_amd import nnunet_plugin
    base = FD.with_data(**desc) if base is None else base
    if KINDS[kind][0] == "mlagg":
        return nnunet_plugin.make_trainer_class(base, data_pipeline=data_pipeline, **kw)
    return nnunet_plugin.make_umamba_enc_ss3d_trainer_class(base, data_pipeline=data_pipeline, **kw)


def make_trainer(kind, desc, device, batch_size=2, patch=None, **kw):
    _, plan_patch, strides, channels = KINDS[kind][:4]
    patch = plan_patch if patch is None else patch
    cls = trainer_class(kind, desc, **kw)
    dataset_json = FK.make_dataset_json(4, channels)
    if strides is None:
        tr = cls(FK.make_plans(patch, batch_size), "2d_bs10", 0, dataset_json, device=torch.device(device))
    else:
        tr = cls(FK.make_plans_3d(patch, batch_size, strides, base=8, cap=32), "3d_fullres", 0, dataset_json, device=torch.device(device))
    tr.mlagg_data_seed = SEED
    return tr


class Recording:
    """An augmenter that keeps what it returned (the input of the chain's tail)."""

    def __init__(self, augmenter):
        self.augmenter = augmenter
        self.takes_int16_seg = getattr(augmenter, "takes_int16_seg", False)

    def __call__(self, data, seg):
        data, seg = self.augmenter(data, seg)
        self.seen = (data.clone(), seg.clone())
        return data, seg


def check_pipeline(kind, desc, device, monkeypatch):
    """get_dataloaders() of the device class: two iterators with nnU-Net's protocol; shapes, planes, no -1, the mask; the first
    training and validation batches equal to_device(loader.generate_train_batch(), ...) composed by hand, bit for bit."""
    from mlagg_unet_amd import dataloading as DL
    monkeypatch.setenv("nnUNet_n_proc_DA", "1")
    _, patch, _, channels, regions, ignore, use_mask, cascade = KINDS[kind]
    tr = make_trainer(kind, desc, device)
    assert tr.mlagg_data_pipeline == "device" and tr.inference_allowed_mirroring_axes is None
    scales = tr._get_deep_supervision_scales()
    sizes = DL.level_sizes(patch, ds_scales=scales)
    planes = 1 if regions is None else len(regions) + (ignore is not None)
    fg = tr.label_manager.foreground_labels
    masked = [i for i, m in enumerate(use_mask) if m]
    torch.manual_seed(5)                                       # the augmenter's noise is torch's: the worker draws it first
    train_it, val_it = tr.get_dataloaders()
    try:
        assert isinstance(train_it, DL.DeviceBatchIterator) and isinstance(val_it, DL.DeviceBatchIterator)
        assert tr.inference_allowed_mirroring_axes == tuple(range(len(patch))) and tr.base_calls["get_dataloaders"] == 0
        assert len(train_it.loader.workers) == 1 and len(val_it.loader.workers) == 1
        first = {"train": next(train_it), "val": next(val_it)}
        for it in (train_it, val_it):
            for _ in range(2):                                 # infinite: more batches than a loader's depth would hold at once
                batch = next(it)
                assert set(batch) == {"data", "target"}
                assert batch["data"].shape == (2, channels + (len(fg) if cascade else 0)) + tuple(patch)
                assert batch["data"].device.type == torch.device(device).type and batch["data"].dtype == torch.float32
                assert [tuple(t.shape) for t in batch["target"]] == [(2, planes) + s for s in sizes]
                for t in batch["target"]:
                    assert float(t.min()) >= 0.0 and t.dtype == torch.float32 and t.device == batch["data"].device
                    if regions is not None:
                        assert set(t.unique().tolist()) <= {0.0, 1.0}
    finally:
        train_it._finish()
        val_it._finish()
    assert not any(t.is_alive() for it in (train_it, val_it) for t in it.loader.workers)

    # by hand: worker 0 of a PrefetchLoader owns loader.clone(RandomState(seed)) and augmenter.clone(seed + 7919)
    from mlagg_unet_amd import augmentation, augmentation3d
    labels = tr.label_manager.all_labels
    seg_values = labels + ([ignore] if ignore is not None else [])              # the augmenters resample every value the seg can hold
    tail = dict(ds_scales=scales, mask_channels=masked, regions=regions, ignore_label=ignore)
    loader_class = DL.DataLoader2D if len(patch) == 2 else DL.DataLoader3D
    if len(patch) == 2:
        aug = augmentation.GpuAugmenter(patch, device, seed=SEED + 1 + 7919, labels=seg_values)
    else:
        aug = augmentation3d.GpuAugmenter3D.for_plan(patch, device, seed=SEED + 1 + 7919, labels=seg_values,
                                                     cascade_labels=fg if cascade else None)
    rec = Recording(aug)

    def dataset(keys):
        return DL.Dataset(desc["folder"], keys, folder_with_segs_from_previous_stage=desc.get("previous_stage_folder"))

    tr_loader = loader_class(dataset(desc["split"][0]), 2, aug.initial_patch_size(), patch, labels, tr.oversample_foreground_percent,
                             rng=np.random.RandomState(SEED + 1), has_ignore=ignore is not None)
    torch.manual_seed(5)
    want_data, want_targets = DL.to_device(tr_loader.generate_train_batch(), device, augmenter=rec, **tail)
    assert torch.equal(first["train"]["data"], want_data)
    assert all(torch.equal(g, w) for g, w in zip(first["train"]["target"], want_targets))
    seen_data, seen_seg = rec.seen
    outside = seen_seg[:, 0] < 0
    assert outside.any() and not outside.all()                  # the augmented patch reaches past the case: -1 before the mapping
    for c in range(channels):
        if c in masked:
            assert bool((want_data[:, c][outside] == 0).all()) and torch.equal(want_data[:, c][~outside], seen_data[:, c][~outside])
            assert bool((seen_data[:, c][outside] != 0).any())  # the mask had something to do
        else:
            assert torch.equal(want_data[:, c], seen_data[:, c])
    val_loader = loader_class(dataset(desc["split"][1]), 2, patch, patch, labels, tr.oversample_foreground_percent,
                              rng=np.random.RandomState(SEED + 500009), has_ignore=ignore is not None)
    b = val_loader.generate_train_batch()
    want_data, want_targets = DL.to_device(b, device, cascade_labels=fg if cascade else None, **tail)
    assert torch.equal(first["val"]["data"], want_data)
    assert all(torch.equal(g, w) for g, w in zip(first["val"]["target"], want_targets))
    assert torch.equal(want_data[:, :channels].cpu(), b["data"])       # the validation chain has no MaskTransform
