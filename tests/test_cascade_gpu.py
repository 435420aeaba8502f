"""GPU: K30 (csrc/cascade_aug.hip) -- bit-plane packing, binary morphology with arbitrary footprints, the "was added" rule and the
random component removal -- against scipy.ndimage and the oracle of tests/_cascade_cases.py, the cascade chain of GpuAugmenter3D
against its CPU-tensor path, and a cascade case folder in front of train steps.  Everything boolean or integer: equality."""
import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import augmentation3d as AUG3
from mlagg_unet_amd import dataloading as DL
from mlagg_unet_amd import ops
from tests import _cascade_cases as K
from tests import _dataloading_3d_cases as KD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5                  # tests/test_augmentation_3d_gpu.py: fp32 prefilter GEMMs and tap sums, volumes of amplitude ~5

# (7, 9, 70): one word border and a 6-bit ragged tail; (5, 6, 130): two word borders; (3, 4, 64): exactly one word
VOLUMES = [(7, 9, 70), (5, 6, 130), (3, 4, 64)]
FOOTPRINTS = {"ball1": AUG3.ball(1.0), "ball1.5": AUG3.ball(1.5), "ball5.49": AUG3.ball(5.49), "ball8": AUG3.ball(8.0),
              "r543": K.multi_run_footprint()}


def _masks(shape):
    corners = np.zeros(shape, dtype=bool)
    corners[::shape[0] - 1, ::shape[1] - 1, ::shape[2] - 1] = True
    return {"random": np.random.RandomState(sum(shape)).rand(*shape) < 0.3, "ones": np.ones(shape, dtype=bool), "corners": corners,
            "empty": np.zeros(shape, dtype=bool)}


def _pack(planes_bool, extra=0):
    """(P, X, Y, Z) bool -> pool (P + extra, X, Y, W) on the device, through cascade_pack of a label map per plane"""
    P, X, Y, Z = planes_bool.shape
    pool = torch.zeros((P + extra, X, Y, ops.cascade_words(Z)), dtype=torch.int64, device=DEV)
    seg = torch.from_numpy(planes_bool.astype(np.int16)).to(DEV)
    ops.cascade_pack(seg, [1], out=pool[:P].view(P, 1, *pool.shape[1:]))
    return pool


def _unpack(planes, Z):
    """(P, X, Y, W) -> (P, X, Y, Z) bool on the host; the padding bits must be 0"""
    P, X, Y, W = planes.shape
    if Z % 64:
        assert int((planes[..., -1] >> (Z % 64)).ne(0).sum()) == 0, "padding bits set"
    out = torch.empty((1, P, X, Y, Z), dtype=torch.float32, device=DEV)
    ops.cascade_unpack(planes.reshape(1, P, X, Y, W), Z, out, 0)
    got = out[0].cpu().numpy()
    assert np.isin(got, (0.0, 1.0)).all()
    return got.astype(bool)


def _runs(S):
    d, e = ops.cascade_footprint_runs(S, ops.CASCADE_DILATION), ops.cascade_footprint_runs(S, ops.CASCADE_EROSION)
    table = torch.tensor(d + e, dtype=torch.int32).to(DEV)
    return table, {0: (0, len(d), 0), 1: (len(d), len(e), 1)}


@pytest.mark.parametrize("fp", list(FOOTPRINTS))
@pytest.mark.parametrize("shape", VOLUMES, ids=lambda s: "x".join(map(str, s)))
def test_morphology_matches_scipy(shape, fp):
    S = FOOTPRINTS[fp]
    masks = _masks(shape)
    names = list(masks)
    stack = np.stack([masks[n] for n in names])
    P, Z = len(names), shape[2]
    table, part = _runs(S)
    for op, parts in enumerate(((0,), (1,), (0, 1), (1, 0))):
        pool = _pack(stack, extra=2 * P)                       # planes, then two scratch planes each
        ops.cascade_morph(pool, Z, [(i, P + i, *part[parts[0]]) for i in range(P)], table)
        res = pool[P:2 * P]
        if len(parts) > 1:
            ops.cascade_morph(pool, Z, [(P + i, 2 * P + i, *part[parts[1]]) for i in range(P)], table)
            res = pool[2 * P:]
        got = _unpack(res, Z)
        assert np.array_equal(_unpack(pool[:P], Z), stack)      # the source planes are untouched
        for i, n in enumerate(names):
            want = K.scipy_operation(masks[n], op, S)
            assert np.array_equal(got[i], want), (K.OPERATIONS[op], n, int((got[i] != want).sum()))


def test_pack_unpack_round_trip():
    labels = [3, 1, 5]                                          # 2 and -1 occur in the map and are in no plane
    for shape in VOLUMES:
        seg = np.random.RandomState(shape[2]).randint(-1, 6, (2,) + shape).astype(np.int16)
        want = np.stack([seg == lab for lab in labels], 1)
        for t in (torch.from_numpy(seg).to(DEV), torch.from_numpy(seg).to(DEV).float()):
            planes = ops.cascade_pack(t, labels)
            assert planes.shape == (2, 3) + shape[:2] + ((shape[2] + 63) // 64,)
            assert np.array_equal(_unpack(planes.view(6, *planes.shape[2:]), shape[2]).reshape(want.shape), want)
        both = torch.from_numpy(np.stack([np.zeros_like(seg), seg], 1)).to(DEV)          # the second channel of a loader batch, in place
        assert torch.equal(ops.cascade_pack(both[:, 1], labels), planes)
        out = torch.full((2, 5) + shape, 7.0, device=DEV)
        ops.cascade_unpack(planes, shape[2], out, 1)
        assert np.array_equal(out[:, 1:4].cpu().numpy(), want.astype(np.float32)) and bool((out[:, 0] == 7).all() & (out[:, 4] == 7).all())
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.cascade_pack(torch.zeros((1, 2, 2, 2), dtype=torch.int16), [1])
    with pytest.raises(RuntimeError, match="words per row"):
        ops.cascade_morph(torch.zeros((3, 2, 2, 2), dtype=torch.int64, device=DEV), 64, [(0, 1, 0, 1, 0)],
                          torch.zeros((1, 4), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="unsupported shape"):        # a job writing its own source
        ops.cascade_morph(torch.zeros((3, 2, 2, 1), dtype=torch.int64, device=DEV), 64, [(1, 1, 0, 1, 0)],
                          torch.zeros((1, 4), dtype=torch.int32, device=DEV))


def test_batched_samples_equal_single_samples():
    labels = [1, 2, 3]
    shape = (7, 9, 70)
    seg = np.stack([K.cascade_label_map(shape, s) for s in (0, 1)])
    far = np.zeros((17, 1, 1), dtype=bool)
    far[0] = True                                               # one offset of 8 along x: it leaves the 7 rows from every voxel
    # sample 1: ball(8) erodes plane 2 empty, so the reference skips the step after it, whose erosion of an empty plane
    # with `far` (no centre, every offset outside: "1 outside") would set every voxel
    params = [[(0, 2, 1.5), (2, 0, 2.5), (1, 1, 1.0)], [(1, 3, 1.0), (0, 0, K.multi_run_footprint()), (2, 1, 8.0), (2, 1, far)]]
    quiet = next(s for s in range(99) if np.random.RandomState(s).rand(2).min() >= 0.2)       # no component removal

    def run(rows):
        data = torch.zeros((len(rows), 1) + shape, device=DEV)
        out = AUG3.cascade_transforms(data, torch.from_numpy(seg[rows]).to(DEV), labels, [params[r] for r in rows],
                                      np.random.RandomState(quiet))
        return out[:, 1:]

    both = run([0, 1])
    assert torch.equal(both, run([0, 1]))                       # bit-identical on a second run
    assert torch.equal(both[:1], run([0])) and torch.equal(both[1:], run([1]))
    want = K.oracle(seg, labels, params, np.random.RandomState(0), p_per_sample=-1.0, footprint_of=AUG3.ball)
    assert np.array_equal(both.cpu().numpy().astype(bool), want)
    plain = np.stack([seg == lab for lab in labels], 1)
    assert (want != plain).any() and plain[1, 2].any() and not want[1, 2].any()
    assert K.erosion(want[1, 2], far).all()                     # what a planning-time emptiness check would have produced


def _check_labelling(planes):
    """cascade_cc_stats of (P, X, Y, Z) non-empty planes against scipy's labelling: the table, parent = each component's first voxel
    in raster order, size at every root = the component's voxel count.  Returns (state, [(label map, valid ids)])."""
    Z = planes.shape[3]
    thresh = float(np.prod(planes.shape[1:], dtype=np.uint64) * 0.15)
    state, table = ops.cascade_cc_stats(_pack(planes), Z, thresh)
    valid = [K.valid_components(p) for p in planes]
    assert table.cpu().tolist() == [[1, len(v)] for _, v in valid]
    parent = state[0].cpu().numpy().reshape(planes.shape)
    size = state[1].cpu().numpy().reshape(planes.shape)
    for p, (lab, _) in enumerate(valid):
        first = np.array([-1] + [np.flatnonzero(lab.ravel() == i)[0] for i in range(1, lab.max() + 1)])
        assert np.array_equal(parent[p], first[lab])
        assert np.array_equal(size[p].ravel()[first[1:]], np.bincount(lab.ravel())[1:])
    return state, valid


@pytest.mark.parametrize("case", list(K.small_component_planes()))
def test_labelling_at_tile_and_word_edges(case):
    planes = K.small_component_planes()[case]
    state, valid = _check_labelling(planes)
    if case == "8x8x32":                                        # one component of 2048 rooted at 0
        assert int(state[0].max()) == 0 and int(state[1][0, 0]) == 2048
    if case == "16x8x128":                                      # the chain is one component, beside the two single voxels
        assert valid[0][0].max() == 3


def test_component_removal_matches_the_oracle():
    planes = K.component_planes()
    Z = K.COMPONENT_SHAPE[2]
    state, valid = _check_labelling(planes)
    thresh = state[3]                                           # the threshold _check_labelling labelled with
    for k in range(len(valid[0][1])):
        for fill in (0, 1):
            pool = _pack(planes)
            ops.cascade_cc_remove(pool, Z, state, [k, -1], [fill, 0])
            got = _unpack(pool, Z)
            comp = valid[0][0] == valid[0][1][k]
            assert np.array_equal(got[0], planes[0] & ~comp), k
            assert np.array_equal(got[1], planes[1] | comp if fill else planes[1]), (k, fill)
    pool = _pack(planes)
    ops.cascade_cc_remove(pool, Z, state, [len(valid[0][1]), 1])       # a rank beyond n_valid removes nothing
    got = _unpack(pool, Z)
    assert np.array_equal(got[0], planes[0]) and np.array_equal(got[1], planes[1] & ~(valid[1][0] == valid[1][1][1]))
    empty = torch.zeros_like(pool)
    assert ops.cascade_cc_stats(empty, Z, thresh)[1].cpu().tolist() == [[0, 0], [0, 0]]


@pytest.mark.parametrize("fill_p", [0.0, 1.0])
def test_cascade_transforms_device_equals_oracle(fill_p):
    planes = K.component_planes()
    seg = np.stack([K.seg_from_planes(planes, [1, 2]), K.cascade_label_map(K.COMPONENT_SHAPE, 4)])
    labels = [1, 2, 3]
    params = [[], [(2, 0, 1.5), (0, 2, 1.0)]]
    seed = next(s for s in range(999) if np.random.RandomState(s).uniform() < 0.2)
    rng, ref = np.random.RandomState(seed), np.random.RandomState(seed)
    data = torch.randn((2, 2) + K.COMPONENT_SHAPE, device=DEV)
    out = AUG3.cascade_transforms(data, torch.from_numpy(seg).to(DEV)[:, None], labels, params, rng, fill_with_other_class_p=fill_p)
    want = K.oracle(seg, labels, params, ref, fill_p=fill_p, footprint_of=AUG3.ball)
    assert torch.equal(out[:, :2], data)
    assert np.array_equal(out[:, 2:].cpu().numpy().astype(bool), want)
    assert rng.uniform() == ref.uniform()
    assert (want[0] != np.stack([seg[0] == lab for lab in labels])).any()


def _cascade_batch():
    """A (2, 1, 24, 28, 72) loader batch with a second seg channel.  Sample 0 is scaled by 0.75 without rotation: every input
    coordinate is a multiple of 1/8, so the trilinear indicator sums are exact in fp32 and float64 alike and the >= 0.5 decisions
    of the device and of the CPU-tensor path cannot differ; sample 1 is the centre crop.  Both are mirrored."""
    shape, patch = (24, 28, 72), (22, 24, 66)        # 66 / 22 = 3: not a dummy-2-D patch
    rng = np.random.RandomState(3)
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij", sparse=True)
    data = np.stack([5 * np.sin(x / 6.0 + b) * np.cos(y / 9.0) + 2 * np.sin(z / 5.0 + 2 * b) for b in range(2)])[:, None].astype(np.float32)
    seg = np.stack([np.stack([K.cascade_label_map(shape, 10 + b), K.cascade_label_map(shape, 20 + b)]) for b in range(2)])
    p = AUG3.draw_params_3d(rng, 2, 1)
    for k in [k for k in p if k.startswith("do_")]:
        p[k][:] = False
    p["do_scale"][0], p["scale"][0] = True, 0.75
    p["do_bright"][:], p["bright"][:] = True, [[1.1], [0.9]]
    p["mirror"][:] = [[True, False, True], [False, True, False]]
    cascade = [[(0, 2, 1.5), (2, 0, 2.5)], [(1, 1, 1.0), (0, 3, 1.0)]]
    return patch, data, seg, p, cascade


def test_cascade_augmenter_equals_its_host_path():
    patch, data, seg, p, cascade = _cascade_batch()
    labels = (1, 2, 3)
    seed = next(s for s in range(999) if np.random.RandomState(s).uniform() < 0.2)
    noise = torch.zeros((2, 1) + patch)
    host = AUG3.GpuAugmenter3D(patch, "cpu", labels=[0, 1, 2, 3, 7], cascade_labels=labels)
    want_d, want_s = host.apply(torch.from_numpy(data), torch.from_numpy(seg), p, noise, cascade, np.random.RandomState(seed))
    dev = AUG3.GpuAugmenter3D(patch, DEV, labels=[0, 1, 2, 3, 7], cascade_labels=labels)
    rng = np.random.RandomState(seed)
    got_d, got_s = dev.apply(torch.from_numpy(data).to(DEV), torch.from_numpy(seg).to(DEV), p, noise.to(DEV), cascade, rng)
    assert got_d.shape == (2, 4) + patch and got_s.shape == (2, 1) + patch and got_d.is_cuda
    print("one-hot mismatches", int((got_d[:, 1:].cpu() != want_d[:, 1:]).sum()), "target mismatches", int((got_s.cpu() != want_s).sum()),
          "image error", float((got_d[:, :1].cpu() - want_d[:, :1]).abs().max()))
    assert torch.equal(got_d[:, 1:].cpu(), want_d[:, 1:]) and torch.equal(got_s.cpu(), want_s)
    assert float((got_d[:, :1].cpu() - want_d[:, :1]).abs().max()) < TOL
    plain_onehot = AUG3.move_seg_as_one_hot(got_d[:, :1], torch.cat([got_s, got_s], 1), labels)[0][:, 1:]
    assert got_d[:, 1:].sum() > 0 and not torch.equal(got_d[:, 1:], plain_onehot)
    # without cascade_labels: the one-channel chain gives, bit for bit, the image and the target of the cascade chain (the
    # one-channel chain itself is pinned by tests/test_augmentation_3d_gpu.py, which this change leaves as it is)
    one = AUG3.GpuAugmenter3D(patch, DEV, labels=[0, 1, 2, 3, 7])
    d1, s1 = one.apply(torch.from_numpy(data).to(DEV), torch.from_numpy(seg[:, :1]).to(DEV), p, noise.to(DEV))
    assert torch.equal(d1, got_d[:, :1]) and torch.equal(s1, got_s)
    with pytest.raises(RuntimeError, match="second seg channel"):
        one.apply(torch.from_numpy(data).to(DEV), torch.from_numpy(seg).to(DEV), p, noise.to(DEV))
    twin = dev.clone(5)
    assert twin.cascade_labels == labels and twin.cascade_order is not dev.cascade_order


def test_cascade_prefetch_drives_train_steps(tmp_path):
    from mlagg_unet_amd import model3d, trainer
    cases, prev = str(tmp_path / "cases"), str(tmp_path / "prev")
    KD.write_dataset_3d(cases, unpack=True)
    K.write_previous_stage(prev, cases, unpack=True)
    labels = (1, 2, 3)
    patch, strides = (16, 32, 32), [[1, 1, 1], [2, 2, 2], [2, 2, 2], [1, 2, 2]]
    aug = AUG3.GpuAugmenter3D(patch, DEV, seed=3, labels=KD.LABELS, cascade_labels=labels)
    dl = DL.DataLoader3D(DL.Dataset(cases, None, prev), 2, aug.initial_patch_size(), patch, KD.LABELS, 0.33)
    scales = model3d.deep_supervision_scales(strides)
    feed = DL.PrefetchLoader(dl, DEV, num_workers=2, depth=2, augmenter=aug, ds_scales=scales)
    try:
        torch.manual_seed(0)
        n = len(strides)
        net = model3d.build_network_architecture_3d(1 + len(labels), 4, [[3, 3, 3]] * n, strides, [2] * n, [2] * (n - 1)).cuda().train()
        opt = torch.optim.SGD(net.parameters(), 1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)
        for _ in range(2):
            data, target = feed.next()
            assert data.shape == (2, 1 + len(labels)) + patch and target[0].shape == (2, 1) + patch
            onehot = data[:, 1:]
            assert bool(((onehot == 0) | (onehot == 1)).all()) and float(onehot.sum(1).max()) <= 1
            loss = trainer.train_step(net, opt, data, target, batch_dice=False)
        assert torch.isfinite(loss).item()
    finally:
        feed.close()
