"""CPU: the host composition behind ops.batch_tail (K36's definition), the one index rule, and the unchanged defaults of the feed.
Everything K36 computes is a copy, a zero or a 0 / 1: every comparison is torch.equal."""
import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import dataloading as DL
from mlagg_unet_amd import ops

import _batch_tail_cases as C
from _dataloading_3d_cases import LABELS, write_dataset_3d


@pytest.mark.parametrize("ignore", [None, 4])
@pytest.mark.parametrize("regions", [None, C.REGIONS_3])
@pytest.mark.parametrize("spatial,scales", [((8, 12), [[1, 1], [.5, .5], [.25, .25]]),
                                            ((4, 8, 12), [[1, 1, 1], [.5, .5, .5], [.25, .25, .25], [.25, .125, .25]])])
def test_host_composition_is_the_four_reference_transforms(spatial, scales, regions, ignore):
    """labels in -1 .. 5, regions [(1, 2, 3), (2, 3), (3,)], with and without an ignore label, against the numpy restatement of
    MaskTransform, RemoveLabelTransform, ConvertSegmentationToRegionsTransform and DownsampleSegForDSTransform2 (shapes whose
    levels are whole fractions: there torch's nearest-exact index and skimage's are the same)."""
    rng = np.random.RandomState(3)
    data = rng.uniform(0.5, 2.0, (2, 3) + spatial).astype(np.float32)
    seg = rng.randint(-1, 6, (2, 1) + spatial).astype(np.int16)
    want_data, want = C.reference_transforms(data, seg, scales, [0, 2], regions, ignore)
    for dtype in (torch.float32, torch.int16):
        d = torch.from_numpy(data.copy())
        got_data, got = ops.batch_tail(d, torch.from_numpy(seg).to(dtype), DL.level_sizes(spatial, ds_scales=scales), [0, 2], regions,
                                       ignore)
        assert got_data is d and torch.equal(got_data, torch.from_numpy(want_data))
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == torch.float32 and g.is_contiguous() and torch.equal(g, torch.from_numpy(w))
    assert not np.array_equal(want_data, data) and np.array_equal(want_data[:, 1], data[:, 1])
    if regions is not None:
        assert want[0].shape[1] == 3 + (ignore is not None) and set(np.unique(want[0])) == {0.0, 1.0}


@pytest.mark.parametrize("name", list(C.GEOMETRIES))
def test_label_mode_is_targets_from_seg(name):
    B, Cn, spatial, levels = C.GEOMETRIES[name]
    data, seg = C.batch(name, torch.float32, 1)
    want = DL.targets_from_seg(seg, levels) if isinstance(levels, int) else DL.targets_from_seg(seg, ds_scales=levels)
    _, got = ops.batch_tail(data, seg, C.level_sizes(name))
    assert [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want]
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def _interpolate_index(n, m):
    ramp = torch.arange(n, dtype=torch.float32).view(1, 1, n)
    return torch.nn.functional.interpolate(ramp, size=m, mode="nearest-exact").view(-1).to(torch.int32)


def test_nearest_index_is_interpolates_choice():
    pairs = set()
    for name in C.GEOMETRIES:
        spatial = C.GEOMETRIES[name][2]
        pairs |= {(n, m) for size in C.level_sizes(name) for n, m in zip(spatial, size)}
    for n in (128, 224, 256, 512, 640, 96, 160):                            # the BASELINE plans' patches, every level of five halvings
        pairs |= {(n, n >> s) for s in range(5)}
    pairs |= {(84, 10), (106, 13), (150, 9)}                                # torch's fp32 index differs from the exact rule here
    for n, m in sorted(pairs):
        idx = DL.nearest_index(n, m)
        assert idx.dtype == torch.int32 and idx.shape == (m,) and torch.equal(idx, _interpolate_index(n, m)), (n, m)
        assert int(idx.min()) >= 0 and int(idx.max()) < n
        if n == m:
            assert torch.equal(idx, torch.arange(n, dtype=torch.int32))
    assert DL.nearest_index(84, 10) is DL.nearest_index(84, 10)             # cached
    exact = [((2 * i + 1) * 84) // 20 for i in range(10)]
    assert DL.nearest_index(84, 10).tolist() != exact                       # the finding recorded in INTEGRATION.md section 5
    with pytest.raises(RuntimeError):
        DL.nearest_index(0, 4)


def test_bad_arguments_raise_on_the_host_too():
    data, seg = C.batch("2d_odd_rows", torch.float32, 1)
    sizes = C.level_sizes("2d_odd_rows")
    for kwargs in (dict(mask_channels=[3]), dict(mask_channels=[-1]), dict(regions=[(i,) for i in range(33)]), dict(regions=[]),
                   dict(ignore_label=-2), dict(tables=[[None, None]])):
        with pytest.raises(RuntimeError):
            ops.batch_tail(data, seg, sizes, **kwargs)
    for bad_sizes in ([], [sizes[0]] * 9, [(23,)], [(0, 37)], [(23, 37, 1)]):
        with pytest.raises(RuntimeError):
            ops.batch_tail(data, seg, bad_sizes)
    short = [[None, None], [DL.nearest_index(23, 11), DL.nearest_index(37, 18)[:-1].contiguous()], [None, None]]
    with pytest.raises(RuntimeError):
        ops.batch_tail(data, seg, sizes, tables=short)
    with pytest.raises(RuntimeError):
        ops.batch_tail(data.transpose(2, 3), seg.transpose(2, 3), [(37, 23)])
    with pytest.raises(RuntimeError):
        ops.batch_tail(data, seg.double(), sizes)
    with pytest.raises(RuntimeError):
        ops.batch_tail(data, seg[:1], sizes)
    with pytest.raises(RuntimeError):                                        # the mask is written by the first level, as the map itself
        ops.batch_tail(data, seg, sizes[1:], mask_channels=[0])


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tail_cases"))
    write_dataset_3d(path, unpack=True)
    return path


def test_feed_defaults_are_unchanged_and_the_keywords_select_the_tail(folder):
    ds = DL.Dataset(folder)
    loader = DL.DataLoader2D(ds, 3, (12, 16), (12, 16), LABELS, 0.33, rng=np.random.RandomState(1), pin_memory=False)
    b = loader.generate_train_batch()
    data, targets = DL.to_device(b, "cpu", n_levels=3)
    want = DL.targets_from_seg(b["seg"].float(), 3)
    assert torch.equal(data, b["data"]) and len(targets) == 3 and all(torch.equal(t, w) for t, w in zip(targets, want))
    assert float(b["seg"].min()) == -1                                       # the loader's padding is in the batch
    # the keywords: no augmenter -> the validation chain, no mask; label mode is the same targets
    data2, targets2 = DL.to_device(b, "cpu", n_levels=3, mask_channels=[0], ignore_label=None)
    assert torch.equal(data2, b["data"]) and all(torch.equal(t, w) for t, w in zip(targets2, want))
    _, planes = DL.to_device(b, "cpu", n_levels=3, regions=C.REGIONS_3)
    assert [tuple(p.shape) for p in planes] == [(3, 3, 12, 16), (3, 3, 6, 8), (3, 3, 3, 4)]
    assert torch.equal(planes[1][:, 2], (want[1][:, 0] == 3).float()) and torch.equal(planes[1][:, 1], ((want[1][:, 0] == 2) | (want[1][:, 0] == 3)).float())

    class Identity:                                                          # an augmenter: the training chain, with the mask
        def __call__(self, data, seg):
            return data, seg

    data3, _ = DL.to_device(b, "cpu", n_levels=3, augmenter=Identity(), mask_channels=[0])
    outside = b["seg"][:, :1] < 0
    assert outside.any() and torch.equal(data3, torch.where(outside, torch.zeros_like(b["data"]), b["data"]))


def test_prefetch_loader_defaults_and_iterator_protocol(folder):
    ds = DL.Dataset(folder)
    loader = DL.DataLoader2D(ds, 2, (12, 16), (12, 16), LABELS, 0.33, pin_memory=False)
    twin = loader.clone(np.random.RandomState(77))
    pf = DL.PrefetchLoader(loader, "cpu", num_workers=1, depth=2, seed=77, n_levels=2)
    try:
        for _ in range(2):
            data, targets = pf.next()
            b = twin.generate_train_batch()
            want = DL.targets_from_seg(b["seg"].float(), 2)
            assert torch.equal(data, b["data"]) and all(torch.equal(t, w) for t, w in zip(targets, want))
        with pf.quiesced():                                                  # no worker assembles a batch inside the block ...
            assert pf._busy == 0 and pf._paused
        data, targets = pf.next()                                            # ... and the stream of batches goes on after it
        b = twin.generate_train_batch()
        assert torch.equal(data, b["data"]) and not pf._paused
    finally:
        pf.close()
    assert not any(t.is_alive() for t in pf.workers)
    scales = [[1, 1], [.5, .5]]
    twin = loader.clone(np.random.RandomState(5))
    it = DL.DeviceBatchIterator(DL.PrefetchLoader(loader, "cpu", num_workers=1, depth=2, seed=5, ds_scales=scales, regions=C.REGIONS_3,
                                                  ignore_label=None))
    try:
        assert iter(it) is it
        batch = next(it)
        b = twin.generate_train_batch()
        _, want = ops.batch_tail(b["data"], b["seg"], [(12, 16), (6, 8)], (), C.REGIONS_3)
        assert set(batch) == {"data", "target"} and isinstance(batch["target"], list)
        assert torch.equal(batch["data"], b["data"]) and all(torch.equal(t, w) for t, w in zip(batch["target"], want))
    finally:
        it._finish()
    assert not any(t.is_alive() for t in it.loader.workers)
    single = DL.DeviceBatchIterator(DL.PrefetchLoader(loader, "cpu", num_workers=1, depth=2, seed=5, n_levels=1))
    try:
        assert torch.is_tensor(next(single)["target"])                       # no deep supervision: one tensor, as NumpyToTensor delivers
    finally:
        single._finish()
