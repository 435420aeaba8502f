"""GPU: the cascade's hand-off at prediction time on the device -- K32 (csrc/sliding_window.hip: the tile gather that writes the one-hot
channels of the previous stage's label map), the sliding window with a previous-stage segmentation, resample_logits_to_next_stage
(K21), preprocess_case(seg_from_prev_stage=...) (K22 + K26) and predict_cascade_case -- against torch compositions, the host paths and
the reference's own results (tests/golden/cascade_predict.npz).

The gather copies and compares: equality.  The hand-off's labels follow the rule of the export tests: the device blends in fp64 and
rounds once as the host does, so a label can differ only where the two largest host probabilities are within GAP = 1e-6 of each
other (a few fp32 ulps of a probability); outside that gap no label may differ, and at most GAP_SHARE = 1e-3 of a case's voxels may be
inside it (the golden maker checks both for the host path on the committed seeds)."""
import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import export as E, inference, ops, predict
from mlagg_unet_amd import preprocessing as P
from tests import _cascade_predict_cases as K
from tests import _preprocess_train_cases as T
from tests.test_cascade_predict_cpu import GOLDEN, handoff, run_preprocess, seeded_conv, sliding_window_inputs, toy_case
from tests.test_preprocess_cpu import _ulps
from tests.test_preprocess_gpu import _zscore_bound

gpu = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.int8, torch.uint8, torch.int16]
MIRRORS = {1: None, 2: (0,), 4: (0, 2), 8: (0, 1, 2)}


def label_map(shape, dtype, seed, pool=(0, 1, 2, 3, 4, 5)):
    """Labels of the cascade (1, 2, 5), others (0, 3, 4), -1 for the signed kinds and 200 where the kind holds it."""
    pool = list(pool) + ([-1] if dtype != torch.uint8 else []) + ([200] if dtype != torch.int8 else [])
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(pool, dtype=torch.int64)[torch.randint(0, len(pool), shape, generator=g)].to(dtype)


def check_gather(vol, seg, labels, origins, V, tile):
    flips = inference.mirror_variants(MIRRORS[V])
    got = ops.sliding_window_gather_onehot(vol, seg, labels, origins, flips, tile)
    full = torch.cat((vol, inference.one_hot(seg, labels)))
    C, L = vol.shape[0], len(labels)
    assert got.shape == (V * len(origins), C + L) + tuple(tile) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got, ops.sliding_window_gather(full, origins, flips, tile))
    tx, ty, tz = tile
    tiles = torch.stack([full[:, x:x + tx, y:y + ty, z:z + tz] for x, y, z in origins])
    want = torch.cat([torch.flip(tiles, inference._flip_dims(m, 2)) if m else tiles for m in flips])
    assert torch.equal(got, want)
    assert torch.equal(got[:, :C], ops.sliding_window_gather(vol, origins, flips, tile))
    return got


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_long_odd_rows(dtype):
    """tz = 67 > 64 and odd, Z = 71 odd, odd and even row starts, the far corner (4 + 5, 4 + 6, 4 + 67) touched"""
    vol = torch.randn((3, 9, 10, 71), generator=torch.Generator().manual_seed(1)).to(DEV)
    seg = label_map((9, 10, 71), dtype, 2).to(DEV)
    got = check_gather(vol, seg, [1, 2, 5], [(4, 4, 3), (0, 1, 4), (4, 4, 4), (1, 0, 0)], 8, (5, 6, 67))
    hot = got[:, 3:]
    assert set(hot.unique().tolist()) == {0.0, 1.0} and float(hot.sum(1).max()) == 1.0 and float(hot.sum(1).min()) == 0.0


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1, 2, 4])
def test_gather_splits_chunks_of_more_than_64_tiles(dtype, V):
    vol = torch.randn((1, 4, 5, 9), generator=torch.Generator().manual_seed(3)).to(DEV)
    seg = label_map((4, 5, 9), dtype, 4).to(DEV)
    rng = np.random.default_rng(5)
    origins = [(int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 5))) for _ in range(65)]
    origins[64] = (2, 2, 4)                                                # the tile of the second launch sits in the far corner
    check_gather(vol, seg, [1, 2, 5], origins, V, (2, 3, 5))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("labels", [[3], list(range(1, 65))], ids=["L1", "L64"])
def test_gather_one_and_sixty_four_labels(dtype, labels):
    vol = torch.randn((2, 5, 6, 13), generator=torch.Generator().manual_seed(6)).to(DEV)
    seg = label_map((5, 6, 13), dtype, 7, pool=range(0, 70)).to(DEV)
    check_gather(vol, seg, labels, [(0, 0, 0), (1, 2, 3), (2, 1, 6)], 2, (3, 4, 7))


@gpu
def test_entry_refusals():
    vol = torch.zeros((1, 4, 5, 9), device=DEV)
    seg = torch.zeros((4, 5, 9), dtype=torch.uint8, device=DEV)
    run = ops.sliding_window_gather_onehot
    for labels in ([], list(range(1, 66)), [0], [1, 256]):
        with pytest.raises(RuntimeError):
            run(vol, seg, labels, [(0, 0, 0)], [0], (2, 3, 5))
    for origin in ((3, 0, 0), (0, 0, 5), (-1, 0, 0)):
        with pytest.raises(RuntimeError):
            run(vol, seg, [1], [origin], [0], (2, 3, 5))
    with pytest.raises(RuntimeError):
        run(vol, seg.to(torch.int32), [1], [(0, 0, 0)], [0], (2, 3, 5))
    with pytest.raises(RuntimeError):
        run(vol, seg[:, :, 1:], [1], [(0, 0, 0)], [0], (2, 3, 5))
    with pytest.raises(RuntimeError):
        run(vol, seg.cpu(), [1], [(0, 0, 0)], [0], (2, 3, 5))
    # the entry itself refuses a tile that leaves the volume (the wrapper checks it first)
    from mlagg_unet_amd import _lib
    out = torch.empty((1, 2, 2, 3, 5), device=DEV)
    code = _lib.lib().mlagg_sw_gather_onehot(vol.data_ptr(), 1, seg.data_ptr(), ops.SW_SEG_KINDS[torch.uint8], ops._int_array([1]), 1, 4,
                                             5, 9, ops._int_array([3, 0, 0]), 1, ops._int_array([0]), 1, out.data_ptr(), 2, 3, 5,
                                             ops._stream())
    assert code == _lib.CONSTANTS["MLAGG_E_UNSUPPORTED"]
    code = _lib.lib().mlagg_sw_gather_onehot(vol.data_ptr(), 1, seg.data_ptr(), 3, ops._int_array([1]), 1, 4, 5, 9,
                                             ops._int_array([0, 0, 0]), 1, ops._int_array([0]), 1, out.data_ptr(), 2, 3, 5, ops._stream())
    assert code == _lib.CONSTANTS["MLAGG_E_UNSUPPORTED"]                   # a bad seg_kind


@gpu
@pytest.mark.parametrize("shape", [(11, 13, 20), (6, 13, 20)])
@pytest.mark.parametrize("tile_batch", [1, 3])
def test_sliding_window_equals_the_explicit_stack(shape, tile_batch):
    """c = 2, L = 3, K = 4; the second volume is smaller than the tile along x: the padding path"""
    image, seg, labels = sliding_window_inputs(shape)
    image, seg = image.to(DEV), seg.to(DEV)
    net = seeded_conv(5, 4).to(DEV)
    kw = dict(mirror_axes=(0, 1, 2), tile_batch=tile_batch)
    want = inference.predict_sliding_window_return_logits(net, torch.cat((image, inference.one_hot(seg, labels))), 4, (8, 8, 16), **kw)
    got = inference.predict_sliding_window_return_logits(net, image, 4, (8, 8, 16), previous_stage_seg=seg, cascade_labels=labels, **kw)
    assert got.is_cuda and tuple(got.shape) == (4,) + shape and torch.equal(got, want)
    lab = inference.predict_sliding_window_return_segmentation(net, image, 4, (8, 8, 16), previous_stage_seg=seg[None].cpu().numpy(),
                                                               cascade_labels=labels, **kw)
    assert lab.dtype == torch.int64 and torch.equal(lab, got.argmax(0))


@gpu
def test_no_one_hot_volume_is_allocated():
    """c = 1, L = 13, K = 2 on 64^3: the call's peak stays below the 4 (c + L) 64^3 bytes of the stacked volume alone, a bound from the
    sizes (image copy, accumulators, result and a chunk are 4 (1 + 2 + 1 + 2) 64^3 bytes and a few tiles); the explicit stack
    cannot stay below it."""
    c, L, n = 1, 13, 64
    g = torch.Generator().manual_seed(8)
    image = torch.randn((c, n, n, n), generator=g).to(DEV)
    seg = torch.randint(0, L + 1, (n, n, n), generator=g).to(torch.uint8).to(DEV)
    labels = list(range(1, L + 1))
    net = seeded_conv(c + L, 2, size=1).to(DEV)
    bound = 4 * (c + L) * n ** 3
    kw = dict(mirror_axes=None, tile_batch=4)

    def rise(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - before

    got, used = rise(lambda: inference.predict_sliding_window_return_logits(net, image, 2, (16, 16, 16), previous_stage_seg=seg,
                                                                            cascade_labels=labels, **kw))
    want, explicit = rise(lambda: inference.predict_sliding_window_return_logits(
        net, torch.cat((image, inference.one_hot(seg, labels))), 2, (16, 16, 16), **kw))
    print(f"peak rise: K32 path {used} bytes, explicit stack {explicit} bytes, bound {bound} bytes")
    assert torch.equal(got, want)
    assert used < bound
    assert explicit >= bound


def check_handoff_labels(got, want, ok, what):
    differ = (got != want) & ok
    inside = float((~ok).float().mean())
    print(f"{what}: {int(differ.sum())} of {want.numel()} labels differ outside the gap, {int((got != want).sum())} anywhere, "
          f"share of voxels inside the gap {inside:.3g}")
    assert int(differ.sum()) == 0
    assert inside <= K.GAP_SHARE


@gpu
@pytest.mark.parametrize("tag", list(K.HANDOFF))
def test_handoff_on_the_device_matches_the_reference_and_the_host(tag):
    got = handoff(tag, K.logits(tag), DEV)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == tuple(K.HANDOFF[tag][4]) and got.is_contiguous()
    ok = K.sure(K.host_probabilities(tag))
    check_handoff_labels(got.cpu(), torch.from_numpy(GOLDEN[f"{tag}/seg"]), ok, f"{tag} against the reference")
    check_handoff_labels(got.cpu(), handoff(tag, K.logits(tag)), ok, f"{tag} against the host path")


@gpu
def test_handoff_above_32_classes_takes_the_resampling_kernel():
    logits = (np.random.default_rng(9).standard_normal((40, 6, 12, 11)) * 2.0).astype(np.float32)
    props = {"spacing": [2.2, 0.6, 0.6], "shape_after_cropping_and_before_resampling": (6, 12, 11)}
    args = ((8, 16, 14), (3.0, 0.8, 0.8), props)
    want = E.resample_logits_to_next_stage(logits, *args)
    got = E.resample_logits_to_next_stage(torch.from_numpy(logits).to(DEV), *args)
    cur = [3.0, 0.8, 0.8]
    ok = K.sure(torch.softmax(E.resample_logits_to_shape(torch.from_numpy(logits), (8, 16, 14), cur, cur), 0))
    check_handoff_labels(got.cpu(), want, ok, "40 classes against the host path")


@gpu
@pytest.mark.parametrize("tag", list(K.PREPROCESS))
def test_device_preprocessing_with_previous_stage_matches_the_reference(tag):
    data, seg, props = run_preprocess(tag, DEV)
    assert data.is_cuda and data.dtype == torch.float32 and seg.is_cuda and seg.dtype == torch.int8 and "class_locations" not in props
    labels = K.foreground_labels(tag)
    got = torch.cat((data, inference.one_hot(seg[0], labels))).cpu().numpy()
    want = GOLDEN[f"{tag}/stack"]
    assert got.shape == want.shape
    assert np.array_equal(np.asarray(props["bbox_used_for_cropping"]), GOLDEN[f"{tag}/bbox"])
    for c, scheme in enumerate(T._spec(tag)[4]):
        if scheme == "ZScoreNormalization":
            err = np.abs(got[c].astype(np.float64) - want[c])
            print(f"{tag} channel {c}: ZScore max |diff| {err.max():.3g}")
            assert (err <= _zscore_bound(want[c])).all(), float(err.max())
        else:
            d = _ulps(got[c], want[c])
            print(f"{tag} channel {c}: max {d.max()} ulp, {int((d > 0).sum())} of {d.size} voxels differ")
            assert d.max() <= 1 and (d > 0).mean() <= 1e-4
    C = data.shape[0]
    near = int(GOLDEN[f"{tag}/near_tie"])                                  # the host's near-tie voxels: none on these inputs
    differ = int((got[C:] != want[C:]).sum())
    print(f"{tag}: {differ} one-hot values differ, {near} near-tie voxels")
    assert near == 0 and differ == 0
    assert np.array_equal(seg.cpu().numpy(), GOLDEN[f"{tag}/seg"])


@gpu
def test_device_preprocessing_refuses_labels_outside_the_dataset():
    tag = "c_isotropic_3d"
    plans, name = K.plans(tag)
    prev = K.previous_stage_seg(tag)
    prev[0, 5, 5, 5] = 9
    with pytest.raises(RuntimeError, match="outside"):
        P.preprocess_case(K.image(tag), K.properties(tag), plans, name, device=DEV, seg_from_prev_stage=prev, dataset_json=K.dataset_json(tag))
    with pytest.raises(RuntimeError, match="dataset_json"):
        P.preprocess_case(K.image(tag), K.properties(tag), plans, name, device=DEV, seg_from_prev_stage=K.previous_stage_seg(tag))


@gpu
def test_predict_cascade_case():
    image, props, plans, dj = toy_case()
    nets = (seeded_conv(2, 4, seed=1).to(DEV), seeded_conv(5, 4, seed=2).to(DEV))
    kw = dict(mirror_axes=(0, 1, 2), tile_batch=2)
    seg, probs = predict.predict_cascade_case(nets, image, props, plans, ("3d_lowres", K.STAGE), dj, return_probabilities=True, **kw)
    assert seg.is_cuda and seg.dtype == torch.uint8 and tuple(seg.shape) == tuple(image.shape[1:])
    assert probs.dtype == torch.float32 and tuple(probs.shape) == (4,) + tuple(image.shape[1:])
    low, _ = predict.predict_case(nets[0], image, props, plans, "3d_lowres", dj, **kw)
    assert low.is_cuda and low.dtype == torch.uint8 and tuple(low.shape) == tuple(image.shape[1:])
    want, want_p = predict.predict_case(nets[1], image, props, plans, K.STAGE, dj, previous_stage_seg=low, return_probabilities=True, **kw)
    assert torch.equal(seg, want) and torch.equal(probs, want_p)
    again, again_p = predict.predict_cascade_case(nets, image, props, plans, ("3d_lowres", K.STAGE), dj, return_probabilities=True, **kw)
    assert torch.equal(again, seg) and torch.equal(again_p, probs)
    assert len(seg.unique()) > 1                                           # not a constant map: the comparison says something
    with pytest.raises(RuntimeError, match="reads 5 channels"):
        predict.predict_case(nets[1], image[:1], props, plans, K.STAGE, dj, previous_stage_seg=low)
