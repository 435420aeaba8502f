"""Region-based datasets (sigmoid heads) on the host: the eager Dice + BCE loss against the reference's own classes
(tests/golden/regions.npz, made by tests/golden/make_golden_regions.py), both target forms, the plugin's loss and validation step, the
host paths of export, prediction and ensembling, the data-parallel batch dice over gloo, and the ABI of K29 and the region modes."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

import fake_nnunet as FK
import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import _lib, ensembling as EN, evaluation, export as E, nnunet_plugin, predict, trainer
from tests import _region_cases as C
from tests.test_ddp_gloo_cpu import _run
from tests.test_plugin_cpu import StubNet

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "regions.npz"))
N_LEVELS = len(C.LOSS_SHAPES)


def loss_case(ignore, form, device="cpu"):
    """-> (logits per level, targets per level, regions or None) of the fixture, as label maps or as region planes"""
    logits = [torch.from_numpy(GOLDEN[f"loss/logits{i}"]).to(device) for i in range(N_LEVELS)]
    seg = [GOLDEN[f"loss/seg_ign{i}" if ignore else f"loss/seg{i}"] for i in range(N_LEVELS)]
    if form == "labels":
        return logits, [torch.from_numpy(s.astype(np.float32)).to(device) for s in seg], C.REGIONS
    return logits, [torch.from_numpy(C.region_planes(s, ignore)).to(device) for s in seg], None


def test_fixture_holds_its_conditions():
    """What make_golden_regions.py asserts about its inputs, checked on the committed data."""
    for i in range(N_LEVELS):
        z = GOLDEN[f"loss/logits{i}"]
        assert all((z == v).any() for v in C.SPECIAL)
    assert (GOLDEN[f"loss/seg_ign{N_LEVELS - 1}"] == C.IGNORE).all()                    # a fully ignored level
    for tag in C.EXPORT_CASES:
        r = GOLDEN[f"seg/{tag}/resampled"]
        a = np.abs(r)
        assert not ((a > 0) & (a < C.BAND)).any() and (r == 0).any()
        assert np.array_equal(GOLDEN[f"seg/{tag}/logits"], C.export_logits(tag))
    for name in ("fp32", "fp16"):
        d = np.abs(GOLDEN[f"ens/{name}/mean"] - np.float32(0.5))
        assert not ((d > 0) & (d < C.BAND)).any() and (d == 0).any()


@pytest.mark.parametrize("batch_dice,ignore", C.LOSS_CASES)
def test_eager_loss_matches_the_reference_classes(batch_dice, ignore):
    """DeepSupervisionWrapper(DC_and_BCE_loss) of nnUNetTrainer.py:330-352: value and logit gradients of every level."""
    tag = C.loss_tag(batch_dice, ignore)
    logits, targets, _ = loss_case(ignore, "planes")
    zs = [z.requires_grad_(True) for z in logits]
    loss = trainer.region_deep_supervision_loss(zs, targets, None, batch_dice, ignore_label=C.IGNORE if ignore else None)
    assert abs(float(loss.detach()) - float(GOLDEN[f"{tag}/value"])) < 1e-6
    grads = torch.autograd.grad(loss, zs)
    for i, g in enumerate(grads):
        assert float((g - torch.from_numpy(GOLDEN[f"{tag}/grad{i}"])).abs().max()) < 1e-7
    if ignore:
        assert float(grads[-1].abs().max()) == 0.0                                    # the fully ignored level
        masked = torch.from_numpy(GOLDEN["loss/seg_ign0"] == C.IGNORE).expand(-1, 3, -1, -1)
        assert float(grads[0][masked].abs().max()) == 0.0
    # one level alone is dc_and_bce_loss
    one = trainer.dc_and_bce_loss(logits[1].detach(), targets[1], batch_dice, use_ignore_label=ignore)
    alone = trainer.region_deep_supervision_loss([logits[1].detach()], [targets[1]], None, batch_dice,
                                                 ignore_label=C.IGNORE if ignore else None)
    assert torch.equal(one, alone)


@pytest.mark.parametrize("batch_dice,ignore", C.LOSS_CASES)
def test_label_map_form_equals_planes_form(batch_dice, ignore):
    ign = C.IGNORE if ignore else None
    out = []
    for form in ("planes", "labels"):
        logits, targets, regions = loss_case(ignore, form)
        zs = [z.requires_grad_(True) for z in logits]
        loss = trainer.region_deep_supervision_loss(zs, targets, regions, batch_dice, ignore_label=ign)
        out.append((loss.detach(), torch.autograd.grad(loss, zs)))
    assert torch.equal(out[0][0], out[1][0])
    assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))
    seg = torch.from_numpy(GOLDEN["loss/seg_ign0"].astype(np.float32))
    assert torch.equal(trainer.regions_from_label_map(seg, C.REGIONS, C.IGNORE), torch.from_numpy(C.region_planes(GOLDEN["loss/seg_ign0"], True)))


@pytest.fixture
def plugin_class(monkeypatch):
    from mlagg_unet_amd import model

    def build(patch_size, in_ch, n_cls, ds=True, variant="B", precision="fp32"):
        torch.manual_seed(0)
        return StubNet(in_ch, n_cls, ds)

    monkeypatch.setattr(model, "build_network_architecture", build)
    monkeypatch.setenv("MLAGG_MIOPEN_TUNED", "0")
    return nnunet_plugin.make_trainer_class(C.region_trainer_base(FK.nnUNetTrainer), variant="B")


def _region_dataset_json(ignore):
    dj = FK.make_dataset_json(3)                               # the label manager is C.RegionLabelManager (region_trainer_base)
    if ignore:
        dj["ignore_label"] = C.IGNORE
    return dj


@pytest.mark.parametrize("ignore", [False, True])
def test_plugin_builds_the_region_loss_and_may_replay(plugin_class, ignore):
    tr = plugin_class(FK.make_plans((32, 32), 2), "2d_bs10", 0, _region_dataset_json(ignore), device=torch.device("cpu"))
    assert tr.label_manager.has_regions and tr.label_manager.foreground_regions == list(C.REGIONS)
    tr.initialize()
    assert tr.base_calls["_build_loss"] == 0 and callable(tr.loss)                   # not the reference's classes
    logits, targets, _ = loss_case(ignore, "planes")
    assert abs(float(tr.loss(logits, targets)) - float(GOLDEN[f"{C.loss_tag(True, ignore)}/value"])) < 1e-6
    assert abs(float(tr.loss(logits[0], targets[0])) - float(trainer.dc_and_bce_loss(logits[0], targets[0], True, False, ignore))) < 1e-6
    # regions no longer veto the hipGraph replay of the step (constructing on a GPU device needs no GPU)
    on_gpu = plugin_class(FK.make_plans((32, 32), 2), "2d_bs10", 0, _region_dataset_json(ignore), device=torch.device("cuda"))
    assert on_gpu._graph_ok() is bool(nnunet_plugin.PLUGIN_GRAPH)
    # the 3-D trainer class builds the same loss
    cls3d = nnunet_plugin.make_umamba_enc_ss3d_trainer_class(C.region_trainer_base(FK.nnUNetTrainer))
    tr3d = cls3d.__new__(cls3d)
    tr3d.label_manager, tr3d.is_ddp = tr.label_manager, False
    tr3d.configuration_manager = tr.configuration_manager
    assert torch.equal(cls3d._build_loss(tr3d)(logits, targets), tr.loss(logits, targets))


def _reference_region_counts(logits, target, has_ignore):
    """B:906-927 written out: (sigmoid > 0.5).long(), mask = 1 - ignore plane, get_tp_fp_fn_tn over batch and space."""
    pred = (torch.sigmoid(logits) > 0.5).long().float()
    if has_ignore:
        mask = 1 - target[:, -1:]
        target = target[:, :-1]
    else:
        mask = torch.ones_like(target[:, :1])
    axes = (0, 2, 3)
    return (pred * target * mask).sum(axes), (pred * (1 - target) * mask).sum(axes), ((1 - pred) * target * mask).sum(axes)


@pytest.mark.parametrize("ignore", [False, True])
def test_validation_step_counts_every_region_head(plugin_class, ignore):
    tr = plugin_class(FK.make_plans((32, 32), 2), "2d_bs10", 0, _region_dataset_json(ignore), device=torch.device("cpu"))
    tr.initialize()
    rng = np.random.default_rng(5)
    segs = [rng.integers(0, 5 if ignore else 4, (2, 1, 32 >> s, 32 >> s)).astype(np.uint8) for s in range(5)]
    batch = {"data": torch.from_numpy(rng.random((2, 1, 32, 32)).astype(np.float32)),
             "target": [torch.from_numpy(C.region_planes(s, ignore)) for s in segs]}
    out = tr.validation_step(batch)
    assert tr.base_calls.get("validation_step", 0) == 0
    with torch.no_grad():
        logits = tr.network(batch["data"])
    tp, fp, fn = _reference_region_counts(logits[0], batch["target"][0], ignore)
    assert out["tp_hard"].shape == (3,)                                              # no [1:]: every head is a foreground region
    for key, want in (("tp_hard", tp), ("fp_hard", fp), ("fn_hard", fn)):
        assert torch.equal(out[key].float(), want), key
    want = trainer.region_deep_supervision_loss_eager(logits, batch["target"], None, True, ignore_label=C.IGNORE if ignore else None)
    assert abs(float(out["loss"]) - float(want)) < 1e-6
    direct = evaluation.validation_step(tr.network, batch["data"], batch["target"], True, False, C.IGNORE if ignore else None,
                                        regions=True)
    assert torch.equal(direct["tp_hard"], out["tp_hard"]) and abs(float(direct["loss"]) - float(want)) < 1e-6
    res = evaluation.validation_epoch_end([out, out])
    assert len(res["dice_per_class_or_region"]) == 3


class _Writer:
    def __init__(self):
        self.written = {}

    def write_seg(self, seg, fname, properties):
        self.written[fname] = (np.array(seg), properties)


@pytest.mark.parametrize("tag", sorted(C.EXPORT_CASES))
def test_export_host_path_paints_the_regions(tag, tmp_path):
    shape, cfg, spacing, full, lo, crop, tb, order = C.EXPORT_CASES[tag]
    x = GOLDEN[f"seg/{tag}/logits"]
    props = C.export_properties(tag)
    convert = E.convert_predicted_logits_to_segmentation_with_correct_shape
    seg, probs = convert(x, props, cfg, tb, return_probabilities=True, regions_class_order=order)
    want_seg = C.paste(tag, GOLDEN[f"seg/{tag}/segmentation"])
    assert seg.dtype == torch.uint8 and np.array_equal(seg.numpy(), want_seg)
    assert np.array_equal(probs.numpy(), C.paste(tag, GOLDEN[f"seg/{tag}/probabilities"]))      # torch's own fp32 sigmoid on both sides
    cur = E.current_spacing_for(cfg, props)
    assert np.array_equal(E.resample_logits_to_shape(torch.from_numpy(x), crop, cur, spacing).numpy(), GOLDEN[f"seg/{tag}/resampled"])
    # a later region overwrites an earlier one, and the class form of the same logits is something else
    assert not np.array_equal(convert(x, props, cfg, tb)[0].numpy(), want_seg)
    assert np.array_equal(E.paint_regions(torch.from_numpy(GOLDEN[f"seg/{tag}/probabilities"]), order).numpy(),
                          GOLDEN[f"seg/{tag}/segmentation"])
    # the drop-in reads the order from the label manager
    rw = _Writer()
    lm = C.RegionLabelManager(regions_class_order=order)
    plans = types.SimpleNamespace(transpose_backward=list(tb), image_reader_writer_class=lambda: rw, get_label_manager=lambda dj: lm)
    trunc = str(tmp_path / "case")
    E.export_prediction_from_softmax(x, props, types.SimpleNamespace(spacing=list(cfg)), plans, C.dataset_json(), trunc, True)
    assert np.array_equal(rw.written[trunc + ".nii.gz"][0], want_seg)
    assert np.array_equal(np.load(trunc + ".npz")["probabilities"], probs.numpy())
    with pytest.raises(RuntimeError):
        convert(x, props, cfg, tb, regions_class_order=order[:2])


def test_predict_reads_the_regions_of_a_dataset_json():
    from tests import _preprocess_cases as PC
    from tests.test_preprocess_cpu import TinyNet3d
    dj = C.dataset_json()
    assert predict._num_segmentation_heads(dj) == 3 and predict._regions_class_order(dj) == [1, 2, 3]
    assert predict._regions_class_order({"labels": {"background": 0, "a": 1}}) is None
    dj_ign = dict(dj, labels=dict(dj["labels"], ignore=4))
    assert predict._num_segmentation_heads(dj_ign) == 3
    tag = "c_isotropic_3d"
    plans, name = PC.plans(tag)
    net = TinyNet3d(1, 3)
    seg, probs = predict.predict_case(net, PC.image(tag), PC.properties(tag), plans, name, dj, return_probabilities=True, device="cpu")
    assert seg.dtype == torch.uint8 and tuple(seg.shape) == tuple(probs.shape[1:])
    assert torch.equal(seg, E.paint_regions(probs, [1, 2, 3]))
    sums = probs.sum(0)
    assert float(probs.min()) >= 0 and float(probs.max()) <= 1 and float((sums - 1).abs().max()) > 0.1       # sigmoids, not a softmax
    assert len(torch.unique(seg)) > 2
    dj_other = dict(dj, regions_class_order=[3, 1, 2])
    seg2, _ = predict.predict_case(net, PC.image(tag), PC.properties(tag), plans, name, dj_other, device="cpu")
    assert torch.equal(seg2, E.paint_regions(probs, [3, 1, 2])) and not torch.equal(seg2, seg)


@pytest.mark.parametrize("name", ["fp32", "fp16"])
def test_ensembling_host_path_paints_the_regions(name, tmp_path):
    members = [GOLDEN[f"ens/{name}/member{i}"] for i in range(2)]
    want_mean, want = GOLDEN[f"ens/{name}/mean"], GOLDEN[f"ens/{name}/labels"]
    labels, mean = EN.ensemble_probabilities(members, return_probabilities=True, regions_class_order=C.ENSEMBLE_ORDER)
    assert labels.dtype == np.uint8 and np.array_equal(labels, want)
    assert np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32))
    assert np.array_equal(mean, EN.ensemble_probabilities(members, return_probabilities=True)[1])       # the mean of the class form
    assert (labels.reshape(-1)[:5] == 0).all()                                                    # a mean of exactly 0.5 does not fire
    tl, _ = EN.ensemble_probabilities([torch.from_numpy(m) for m in members], regions_class_order=C.ENSEMBLE_ORDER)
    assert isinstance(tl, torch.Tensor) and np.array_equal(tl.numpy(), want)
    one, _ = EN.ensemble_probabilities([m[:1] for m in members], regions_class_order=[7])               # a single region head
    assert set(np.unique(one)) == {0, 7}
    # the drop-in takes the order from the label manager
    files = []
    for i, m in enumerate(members):
        d = tmp_path / f"member{i}"
        d.mkdir()
        np.savez(d / "case.npz", probabilities=m)
        with open(d / "case.pkl", "wb") as f:
            pickle.dump({"member": i}, f)
        files.append(str(d / "case.npz"))
    rw = _Writer()
    lm = C.RegionLabelManager(regions_class_order=C.ENSEMBLE_ORDER)
    EN.merge_files(files, str(tmp_path / "out"), ".seg", rw, lm, True, device="cpu")
    seg, props = rw.written[str(tmp_path / "out.seg")]
    assert np.array_equal(seg, want) and props == {"member": 0}
    assert np.array_equal(np.load(str(tmp_path / "out.npz"))["probabilities"].view(np.uint32), want_mean.view(np.uint32))
    for i in range(2):
        with open(tmp_path / f"member{i}" / "dataset.json", "w") as f:
            f.write('{"file_ending": ".seg"}')
    EN.ensemble_folders([str(tmp_path / "member0"), str(tmp_path / "member1")], str(tmp_path / "ens"), image_reader_writer=rw,
                        label_manager=lm, device="cpu")
    assert np.array_equal(rw.written[str(tmp_path / "ens" / "case.seg")][0], want)


def _region_ddp_case(rank, world):
    """Batch dice of the region loss over two ranks, label-map and planes form: the dice statistics of all levels cross the ranks in
    one exchange, so every rank's dice is the global-batch dice; the BCE mean is local to the rank and the ranks hold equal shares, so
    the mean of the ranks' losses -- and, after DDP's 1 / world, their gradients -- equal the single-process loss on the
    concatenated batch."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import mlagg_unet_amd  # noqa: F401
    from mlagg_unet_amd import trainer as TR
    from tests import _region_cases as RC
    rng = np.random.default_rng(41)
    shapes = ((12, 14), (6, 7))
    logits = [torch.from_numpy((rng.standard_normal((4, 3) + s) * 2).astype(np.float32)) for s in shapes]
    segs = [rng.integers(0, 4, (4, 1) + s).astype(np.uint8) for s in shapes]
    sl = slice(2 * rank, 2 * rank + 2)
    res = []
    for form in ("labels", "planes"):
        if form == "labels":
            tg, regions = [torch.from_numpy(s.astype(np.float32)) for s in segs], RC.REGIONS
        else:
            tg, regions = [torch.from_numpy(RC.region_planes(s)) for s in segs], None
        mine = [z[sl].clone().requires_grad_(True) for z in logits]
        loss = TR.region_deep_supervision_loss(mine, [t[sl] for t in tg], regions, True, True)
        grads = torch.autograd.grad(loss, mine)
        full = [z.clone().requires_grad_(True) for z in logits]
        ref = TR.region_deep_supervision_loss(full, tg, regions, True, False)
        ref_grads = torch.autograd.grad(ref, full)
        local = TR.region_deep_supervision_loss([z[sl] for z in logits], [t[sl] for t in tg], regions, True, False)
        mean_loss = loss.detach().clone()
        torch.distributed.all_reduce(mean_loss)
        res.append((float(mean_loss / world), float(ref.detach()),
                    max(float((a / world - b[sl]).abs().max()) for a, b in zip(grads, ref_grads)),
                    abs(float(loss.detach()) - float(local))))
    return res


def test_ddp_region_batch_dice_equals_the_global_batch():
    for per_rank in _run(_region_ddp_case):
        for loss, ref, gerr, moved in per_rank:
            assert abs(loss - ref) < 1e-6 and gerr < 1e-7
            assert moved > 1e-4                    # ... and the exchange matters: the rank's own batch dice is another number


def test_abi_has_the_region_entries():
    names = ("mlagg_dice_bce_max_regions", "mlagg_dice_bce_stats_workspace_floats", "mlagg_dice_bce_stats", "mlagg_dice_bce_grad",
             "mlagg_export_segmentation_regions", "mlagg_ensemble_mean_regions")
    header = open(_lib.HEADER).read()
    lib = _lib.lib()
    for n in names:
        assert n in _lib.SIGNATURES and n in header and hasattr(lib, n), n
    assert lib.mlagg_dice_bce_max_regions() == 16
    assert lib.mlagg_dice_bce_stats_workspace_floats(2, 3, 2115) == 2 * 3 * (3 * 3 + 2)
    # out-of-range sizes are refused before anything is launched (no device is touched: the size check comes first)
    one = 8
    for R in (0, 17):
        assert lib.mlagg_dice_bce_stats(one, one, None, one, one, one, one, 2, R, 100, -1, None) == _lib.CONSTANTS["MLAGG_E_UNSUPPORTED"]
        assert lib.mlagg_dice_bce_grad(one, one, None, one, one, one, 2, R, 100, -1, None) == _lib.CONSTANTS["MLAGG_E_UNSUPPORTED"]
    names_prof = [lib.mlagg_profile_kernel_name(i).decode() for i in range(lib.mlagg_profile_kernel_count())]
    assert "dice_bce_stats_kernel" in names_prof and "dice_bce_grad_kernel" in names_prof
