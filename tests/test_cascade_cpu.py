"""CPU: the cascade transforms' definitions, parameter draws and host path (augmentation3d) and the previous-stage channel of the
loaders (dataloading), against the plain numpy + scipy oracle of tests/_cascade_cases.py.  Everything is boolean or integer: equality."""
import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import augmentation3d as AUG3
from mlagg_unet_amd import dataloading as DL
from tests import _cascade_cases as K
from tests import _dataloading_3d_cases as KD

FOOTPRINTS = {"r3": K.random_footprint((3, 3, 3), 1), "r4": K.random_footprint((4, 4, 4), 2), "r2": K.random_footprint((2, 2, 2), 3),
              "r543": K.random_footprint((5, 4, 3), 4), "r6": K.random_footprint((6, 6, 6), 5),
              **{f"ball{r}": AUG3.ball(r) for r in K.RADII}}


@pytest.mark.parametrize("name", list(FOOTPRINTS))
def test_definitions_equal_scipy(name):
    S = FOOTPRINTS[name]
    for seed, density in ((0, 0.3), (1, 0.9)):
        x = np.random.RandomState(seed).rand(9, 11, 13) < density
        for op in range(4):
            want = K.scipy_operation(x, op, S)
            assert np.array_equal(K.operation(x, op, S), want), (name, op)
            assert np.array_equal(AUG3.binary_operation_host(x, op, S), want), (name, op)


def test_ball_shapes():
    for r, n in K.RADII.items():
        S = AUG3.ball(r)
        assert S.shape == (n, n, n) and S.dtype == bool and S[n // 2, n // 2, n // 2]
    assert AUG3.ball(1.0).sum() == 7
    S = AUG3.ball(5.49)
    assert not np.array_equal(S, S[::-1, ::-1, ::-1])             # linspace rounding: not point-symmetric


def test_draws_follow_the_reference_order():
    B, L = 3, 5
    a, b = np.random.RandomState(4), np.random.RandomState(4)
    order_a, order_b = list(range(L)), list(range(L))
    fired = 0
    for _ in range(4):                                            # the shuffled order persists from batch to batch
        got = AUG3.draw_cascade_params(a, B, L, order_a)
        want = K.draw_literal(b, B, L, order_b)
        assert [[(c, op, r) for c, op, r in s] for s in got] == [[(int(c), int(op), float(r)) for c, op, r in s] for s in want]
        assert order_a == order_b
        assert a.uniform() == b.uniform()                          # the same stream position
        fired += sum(len(s) > 0 for s in got)
    assert fired >= 2 and order_a != list(range(L))
    with pytest.raises(RuntimeError, match="permutation"):
        AUG3.draw_cascade_params(a, B, L, [0, 1, 2])


def _removal_seed(fires):
    return next(s for s in range(200) if (np.random.RandomState(s).uniform() < 0.2) == fires)


def _run_host(seg, labels, params, seed, **kw):
    data = torch.zeros((seg.shape[0], 1) + seg.shape[1:])
    rng = np.random.RandomState(seed)
    out = AUG3.cascade_transforms(data, torch.from_numpy(seg)[:, None], labels, params, rng, **kw)
    assert out.shape == (seg.shape[0], 1 + len(labels)) + seg.shape[1:] and out.dtype == torch.float32
    assert torch.equal(out[:, :1], data)
    return out[:, 1:].numpy().astype(bool), rng


def test_was_added_rule_and_empty_plane():
    labels = [1, 2, 3, 4]                                          # label 4 is absent: an empty plane
    seg = np.stack([K.cascade_label_map((9, 12, 14), s) for s in (0, 1)])
    params = [[(0, 0, 1.5), (3, 0, 2.5), (1, 2, K.random_footprint((3, 4, 3), 7))], [(2, 3, 1.0), (1, 1, 1.0), (0, 0, 2.5)]]
    seed = _removal_seed(False)
    got, rng = _run_host(seg, labels, params, seed)
    ref_rng = np.random.RandomState(seed)
    want = K.oracle(seg, labels, params, ref_rng, footprint_of=AUG3.ball)
    assert np.array_equal(got, want)
    assert rng.uniform() == ref_rng.uniform()
    plain = np.stack([seg == lab for lab in labels], 1)
    assert not got[:, 3].any() and (got != plain).any()
    assert (got.sum(1) <= 1).all()                                 # still one-hot: what a dilation adds leaves the other planes
    grown = K.dilation(plain[0, 0], AUG3.ball(1.5))
    assert (grown & plain[0, 1]).any() and not (grown & got[0, 1]).any()


def test_component_removal_draws_and_ranks():
    planes = K.component_planes()
    seg = K.seg_from_planes(planes, [1, 2])[None]
    labels = [1, 2, 3]                                             # plane 2 is empty: no draw beyond its p_per_label
    lab, valid = K.valid_components(planes[0])
    assert len(valid) >= 5
    lab_b, valid_b = K.valid_components(planes[1])
    assert len(valid_b) == 2 and lab_b.max() == 3                  # the 2040-voxel component (>= 15 %) is never a candidate
    seen = set()
    for seed in [s for s in range(400) if np.random.RandomState(s).uniform() < 0.2][:12]:
        got, rng = _run_host(seg, labels, [[]], seed)
        ref_rng = np.random.RandomState(seed)
        want = K.oracle(seg, labels, [[]], ref_rng)
        assert np.array_equal(got, want)
        assert rng.uniform() == ref_rng.uniform()
        removed = planes[0] & ~got[0, 0]
        ids = np.unique(lab[removed])
        assert len(ids) == 1 and ids[0] in valid and np.array_equal(removed, lab == ids[0])
        assert got[0, 1][:, :, 5:17].all()
        seen.add(int(ids[0]))
    assert len(seen) >= 3
    # only a component of >= 15 %: nothing is removed and no choice is drawn
    big = np.zeros((1,) + K.COMPONENT_SHAPE, dtype=np.int16)
    big[0, :, :, 5:17] = 1
    seed = _removal_seed(True)
    got, rng = _run_host(big, [1], [[]], seed)
    assert np.array_equal(got[0, 0], big[0] == 1)
    ref = np.random.RandomState(seed)
    ref.uniform(), ref.uniform()                                   # p_per_sample, p_per_label; nothing more
    assert rng.uniform() == ref.uniform()


def test_fill_with_other_class_on_the_host():
    planes = K.component_planes()
    seg = K.seg_from_planes(planes, [1, 2])[None]
    seed = _removal_seed(True)
    got, rng = _run_host(seg, [1, 2], [[]], seed, fill_with_other_class_p=1.0)
    ref_rng = np.random.RandomState(seed)
    want = K.oracle(seg, [1, 2], [[]], ref_rng, fill_p=1.0)
    assert np.array_equal(got, want) and rng.uniform() == ref_rng.uniform()
    assert (got[0, 1] & planes[0]).any()


def test_move_seg_as_one_hot():
    seg = np.stack([K.cascade_label_map((6, 7, 9), s) for s in (2, 3)])
    both = torch.from_numpy(np.stack([np.zeros_like(seg), seg], 1))
    data = torch.randn(2, 2, 6, 7, 9)
    out, target = AUG3.move_seg_as_one_hot(data, both, [1, 2, 3])
    assert torch.equal(out[:, :2], data) and torch.equal(target, both[:, :1])
    assert np.array_equal(out[:, 2:].numpy(), np.stack([seg == lab for lab in (1, 2, 3)], 1).astype(np.float32))
    with pytest.raises(RuntimeError, match="previous stage"):
        AUG3.move_seg_as_one_hot(data, both[:, :1], [1])


@pytest.mark.parametrize("unpack", [False, True], ids=["npz", "npy"])
def test_loader_reads_the_previous_stage(tmp_path, unpack):
    cases, prev_folder = str(tmp_path / "cases"), str(tmp_path / "prev")
    KD.write_dataset_3d(cases, unpack=unpack)
    K.write_previous_stage(prev_folder, cases, unpack=unpack)
    _, patch, final, bs, oversample = KD.CASES["npz"]
    plain = DL.DataLoader3D(DL.Dataset(cases), bs, patch, final, KD.LABELS, oversample, rng=np.random.RandomState(9), pin_memory=False)
    ds = DL.Dataset(cases, folder_with_segs_from_previous_stage=prev_folder)
    assert ds.keys() == DL.Dataset(cases).keys()
    casc = DL.DataLoader3D(ds, bs, patch, final, KD.LABELS, oversample, rng=np.random.RandomState(9), pin_memory=False)
    boxes, bbox = [], casc._bbox
    casc._bbox = lambda *args: boxes.append(bbox(*args)) or boxes[-1]          # the box of every sample, as the loader drew it
    padded = 0
    for _ in range(3):
        del boxes[:]
        a, b = plain.generate_train_batch(), casc.generate_train_batch()
        assert list(a["keys"]) == list(b["keys"])
        assert torch.equal(a["data"], b["data"]) and b["seg"].shape == (bs, 2) + patch and b["seg"].dtype == torch.int16
        assert torch.equal(a["seg"], b["seg"][:, :1])
        for j, key in enumerate(b["keys"]):
            # both channels: the case's array cropped with that box, -1 where the box leaves the case
            full = np.load(f"{cases}/{key}.npz")["seg"][0]
            prev = np.roll(np.maximum(full, 0), 1, axis=1)                     # what write_previous_stage stored
            assert np.array_equal(np.load(f"{prev_folder}/{key}.npz")["seg"], prev) and (prev != np.maximum(full, 0)).any()
            lb = boxes[j]
            for channel, case in ((0, full), (1, prev)):
                want = np.full(patch, -1, dtype=np.int16)
                src = tuple(slice(max(0, lb[i]), min(case.shape[i], lb[i] + patch[i])) for i in range(3))
                dst = tuple(slice(s.start - lb[i], s.stop - lb[i]) for i, s in enumerate(src))
                want[dst] = case[src]
                assert np.array_equal(b["seg"][j, channel].numpy(), want), (key, channel, lb)
            padded += int((b["seg"][j, 1].numpy() == -1).any())
    assert padded > 0                                                          # a case thinner than the patch: -1 padding
    assert plain.rng.uniform() == casc.rng.uniform()
    # a label above the dataset's in the previous stage's channel is not the target's business
    assert casc.clone(np.random.RandomState(1)).seg_channels == 2


def test_to_device_needs_the_cascade_labels(tmp_path):
    cases, prev = str(tmp_path / "cases"), str(tmp_path / "prev")
    KD.write_dataset_3d(cases)
    K.write_previous_stage(prev, cases)
    _, patch, final, bs, oversample = KD.CASES["npz"]
    dl = DL.DataLoader3D(DL.Dataset(cases, None, prev), bs, patch, final, KD.LABELS, oversample, rng=np.random.RandomState(2),
                         pin_memory=False)
    batch = dl.generate_train_batch()
    data, targets = DL.to_device(batch, "cpu", ds_scales=[[1, 1, 1]], cascade_labels=[1, 2, 3])
    assert data.shape == (bs, 4) + patch and targets[0].shape == (bs, 1) + patch and float(targets[0].min()) >= 0
    prev_seg = batch["seg"][:, 1].numpy()
    assert np.array_equal(data[:, 1:].numpy(), np.stack([prev_seg == lab for lab in (1, 2, 3)], 1).astype(np.float32))
    with pytest.raises(RuntimeError, match="cascade_labels"):
        DL.to_device(batch, "cpu", ds_scales=[[1, 1, 1]])
