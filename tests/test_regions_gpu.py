"""Region-based datasets (sigmoid heads) on the device: K29 (csrc/region_loss.hip) against the reference's own loss classes
(tests/golden/regions.npz) and float64, both target forms, the head-count limits, determinism and extreme logits; the region modes of
K21 (export) and K28 (ensembling) against the reference's LabelManager; and the hipGraph replay of a region train step."""
import copy
import os

import numpy as np
import pytest
import torch

import fake_nnunet as FK
import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import ensembling as EN, export as E, nnunet_plugin, ops, trainer
from tests import _region_cases as C
from tests.test_regions_cpu import GOLDEN, N_LEVELS, loss_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _float64_loss(ignore, batch_dice):
    """dc_and_bce_loss composed level by level on the fixture's inputs in float64: value and gradients"""
    logits, targets, _ = loss_case(ignore, "planes")
    zs = [z.double().requires_grad_(True) for z in logits]
    ws = trainer.deep_supervision_weights(N_LEVELS)
    loss = sum(w * trainer.dc_and_bce_loss(z, t.double(), batch_dice, False, ignore) for w, z, t in zip(ws, zs, targets))
    return float(loss.detach()), torch.autograd.grad(loss, zs)


@pytest.mark.parametrize("form", ["planes", "labels"])
@pytest.mark.parametrize("batch_dice,ignore", C.LOSS_CASES)
def test_fused_region_loss_matches_the_reference_and_float64(batch_dice, ignore, form):
    """K29 + the vectorised level algebra against the reference's DeepSupervisionWrapper(DC_and_BCE_loss) (fixture) and against the
    float64 evaluation of dc_and_bce_loss, value and gradient of every level, in both target forms.  Tolerances: those of the K9
    test against its reference fixture (value 2e-6, gradients 1e-7 absolute).  For scale: on these inputs the reference's own fp32
    classes differ from float64 by at most 2.2e-7 in the value and 5.5e-11 in the gradients (make_golden_regions.py prints both)."""
    tag = C.loss_tag(batch_dice, ignore)
    logits, targets, regions = loss_case(ignore, form, DEV)
    zs = [z.requires_grad_(True) for z in logits]
    loss = trainer.region_deep_supervision_loss(zs, targets, regions, batch_dice, ignore_label=C.IGNORE if ignore else None)
    grads = [g.cpu() for g in torch.autograd.grad(loss, zs)]
    want64, grads64 = _float64_loss(ignore, batch_dice)
    errs = [float((g - torch.from_numpy(GOLDEN[f"{tag}/grad{i}"])).abs().max()) for i, g in enumerate(grads)]
    errs64 = [float((g.double() - w).abs().max()) for g, w in zip(grads, grads64)]
    loss = loss.detach()
    print(f"{tag} {form}: value {float(loss):.9f} fixture {float(GOLDEN[f'{tag}/value']):.9f} float64 {want64:.9f}; "
          f"gradient errors against the fixture {errs}, against float64 {errs64}")
    assert abs(float(loss) - float(GOLDEN[f"{tag}/value"])) < 2e-6 and abs(float(loss) - want64) < 2e-6
    assert abs(float(loss) - float(GOLDEN[f"{tag}/value64"])) < 2e-6               # the reference's own classes on float64 inputs
    assert max(errs) < 1e-7 and max(errs64) < 1e-7
    assert all(torch.isfinite(g).all() for g in grads)
    if ignore:
        assert float(grads[-1].abs().max()) == 0.0                                    # the fully ignored level
        masked = torch.from_numpy(GOLDEN["loss/seg_ign0"] == C.IGNORE).expand(-1, 3, -1, -1)
        assert float(grads[0][masked].abs().max()) == 0.0


def _single_level(R, seed, ignore):
    rng = np.random.default_rng(seed)
    z = torch.from_numpy((rng.standard_normal((2, R, 33, 31)) * 2).astype(np.float32))
    seg = rng.integers(0, R + 1 + int(ignore), (2, 1, 33, 31)).astype(np.float32)          # labels 0 .. R, then the ignore label
    regions = [tuple(range(r + 1, R + 1)) for r in range(R)]                              # nested: region r holds the labels above r
    return z, torch.from_numpy(seg), regions, (R + 1 if ignore else None)


@pytest.mark.parametrize("R", [1, 16, 17])
@pytest.mark.parametrize("ignore", [False, True])
def test_region_loss_head_counts(R, ignore):
    """One and sixteen heads (the kernel's limit) on a single 33 x 31 level, in both target forms, against float64; seventeen heads
    take the eager composition on the device without error.  The value's bound is K9's against its eager form, 2e-6 max(1, |value|):
    with an ignore label the BCE term is a sum over the heads (compound_losses.py:96 divides by the mask sum without a factor R), so
    sixteen heads give a value near 16, where one fp32 step is 1.9e-6 and an absolute 2e-6 would ask for the last bit."""
    z, seg, regions, ign = _single_level(R, 50 + R, ignore)
    planes = trainer.regions_from_label_map(seg, regions, ign)
    z64 = z.double().requires_grad_(True)
    want = trainer.dc_and_bce_loss(z64, planes.double(), False, False, ignore)
    gwant, = torch.autograd.grad(want, z64)
    for tg, rg in ((seg, regions), (planes, None)):
        zd = z.to(DEV).requires_grad_(True)
        loss = trainer.region_deep_supervision_loss([zd], [tg.to(DEV)], rg, False, ignore_label=ign)
        g, = torch.autograd.grad(loss, zd)
        assert abs(float(loss.detach()) - float(want)) < 2e-6 * max(1.0, abs(float(want)))
        assert float((g.cpu().double() - gwant).abs().max()) < 1e-7
    if R == 17:
        with pytest.raises(RuntimeError):
            ops.dice_bce_stats([z.to(DEV)], [planes.to(DEV)], None, ign)


def test_labels_outside_every_region_count_as_background():
    """Label-map form without an ignore label: -1 (the value outside the non-zero mask of a preprocessed case) and a label beyond the
    table are in no region and still count -- np.isin semantics, equal to the eager composition on the planes."""
    rng = np.random.default_rng(12)
    z = torch.from_numpy((rng.standard_normal((2, 3, 33, 31)) * 2).astype(np.float32))
    seg = torch.from_numpy(rng.choice([-1, 0, 1, 2, 3, 200, 300], (2, 1, 33, 31)).astype(np.float32))
    z64 = z.double().requires_grad_(True)
    want = trainer.region_deep_supervision_loss_eager([z64], [seg.double()], C.REGIONS, True)
    gwant, = torch.autograd.grad(want, z64)
    zd = z.to(DEV).requires_grad_(True)
    loss = trainer.region_deep_supervision_loss([zd], [seg.to(DEV)], C.REGIONS, True)
    g, = torch.autograd.grad(loss, zd)
    assert abs(float(loss.detach()) - float(want)) < 2e-6 and float((g.cpu().double() - gwant).abs().max()) < 1e-7


def test_region_loss_is_deterministic():
    logits, targets, regions = loss_case(True, "labels", DEV)
    runs = []
    for _ in range(2):
        zs = [z.clone().requires_grad_(True) for z in logits]
        loss = trainer.region_deep_supervision_loss(zs, targets, regions, True, ignore_label=C.IGNORE)
        runs.append((loss.detach(), torch.autograd.grad(loss, zs)))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_region_loss_extreme_logits_stay_finite():
    z = torch.zeros(2, 3, 20, 20)
    z[:, 0], z[:, 1] = 100.0, -100.0
    z[:, 2, ::2] = 100.0
    z[:, 2, 1::2] = -100.0
    seg = torch.from_numpy(np.random.default_rng(3).integers(0, 4, (2, 1, 20, 20)).astype(np.float32))
    zd = z.to(DEV).requires_grad_(True)
    loss = trainer.region_deep_supervision_loss([zd], [seg.to(DEV)], C.REGIONS, True)
    g, = torch.autograd.grad(loss, zd)
    want = trainer.region_deep_supervision_loss_eager([z.double()], [seg.double()], C.REGIONS, True)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    assert abs(float(loss.detach()) - float(want)) < 1e-4 * abs(float(want))


def _sigmoid_error_bound(tag):
    """Four times the error of torch's fp32 sigmoid against float64 on the fixture's resampled logits (measured: see the test)."""
    r = torch.from_numpy(GOLDEN[f"seg/{tag}/resampled"])
    return 4 * float((torch.sigmoid(r).double() - torch.sigmoid(r.double())).abs().max())


@pytest.mark.parametrize("tag", sorted(C.EXPORT_CASES))
def test_device_export_paints_the_regions(tag):
    """K21's region mode against the reference's LabelManager on the resampled logits: labels exactly; probabilities against the
    float64 sigmoid within four times the error of torch's fp32 sigmoid on the same logits (measured on this fixture: torch's error is
    7.9e-8 for "iso" and 8.3e-8 for "aniso", so the bounds are 3.2e-7 and 3.3e-7)."""
    shape, cfg, spacing, full, lo, crop, tb, order = C.EXPORT_CASES[tag]
    x = torch.from_numpy(GOLDEN[f"seg/{tag}/logits"]).to(DEV)
    props = C.export_properties(tag)
    convert = E.convert_predicted_logits_to_segmentation_with_correct_shape
    seg, probs = convert(x, props, cfg, tb, return_probabilities=True, regions_class_order=order)
    assert seg.is_cuda and seg.dtype == torch.uint8 and seg.is_contiguous() and probs.is_contiguous()
    want_seg = C.paste(tag, GOLDEN[f"seg/{tag}/segmentation"])
    assert np.array_equal(seg.cpu().numpy(), want_seg)
    want64 = C.paste(tag, torch.sigmoid(torch.from_numpy(GOLDEN[f"seg/{tag}/resampled"]).double()).numpy())
    bound = _sigmoid_error_bound(tag)
    err = float(np.abs(probs.cpu().numpy().astype(np.float64) - want64).max())
    print(f"{tag}: sigmoid error {err:.3e}, bound (4 x torch fp32) {bound:.3e}")
    assert err <= bound
    inside = np.zeros(full, bool)
    inside[tuple(slice(a, a + c) for a, c in zip(lo, crop))] = True
    assert float(probs.cpu().numpy()[:, ~inside.transpose(tb)].max()) == 0.0           # zeros outside the box, in every head
    labels_only, none = convert(x, props, cfg, tb, regions_class_order=order)
    assert none is None and torch.equal(labels_only, seg)
    view = x.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)                      # any strides
    assert torch.equal(convert(view, props, cfg, tb, regions_class_order=order)[0], seg)
    # the same logits through the host path
    host = convert(x.cpu(), props, cfg, tb, regions_class_order=order)[0]
    assert torch.equal(host, seg.cpu())


def test_device_export_of_more_than_32_region_heads():
    """More than 32 heads: the resampling kernel, then the torch form of the same steps; equal to the host path."""
    tag = "iso"
    shape, cfg, spacing, full, lo, crop, tb, _ = C.EXPORT_CASES[tag]
    x = torch.from_numpy((np.random.default_rng(8).standard_normal((33,) + shape) * 2).astype(np.float32))
    order = [(7 * k) % 200 + 1 for k in range(33)]
    convert = E.convert_predicted_logits_to_segmentation_with_correct_shape
    seg, _ = convert(x.to(DEV), C.export_properties(tag), cfg, tb, regions_class_order=order)
    assert seg.is_cuda and torch.equal(seg.cpu(), convert(x, C.export_properties(tag), cfg, tb, regions_class_order=order)[0])


@pytest.mark.parametrize("name", ["fp32", "fp16"])
def test_device_ensemble_paints_the_regions(name):
    members = [torch.from_numpy(GOLDEN[f"ens/{name}/member{i}"]).to(DEV) for i in range(2)]
    labels, mean = EN.ensemble_probabilities(members, return_probabilities=True, regions_class_order=C.ENSEMBLE_ORDER)
    assert labels.is_cuda and labels.dtype == torch.uint8
    assert np.array_equal(labels.cpu().numpy(), GOLDEN[f"ens/{name}/labels"])
    assert np.array_equal(mean.cpu().numpy().view(np.uint32), GOLDEN[f"ens/{name}/mean"].view(np.uint32))
    assert torch.equal(mean, ops.ensemble_mean(members, want_mean=True)[1])            # bit-equal to the class form's mean
    only, none = EN.ensemble_probabilities(members, regions_class_order=C.ENSEMBLE_ORDER)
    assert none is None and torch.equal(only, labels)
    one, _ = ops.ensemble_mean([m[:1].contiguous() for m in members], regions_class_order=[9])      # a single region head
    assert torch.equal(one, (mean[0] > 0.5).to(torch.uint8) * 9)


IMG, BATCH = (64, 64), 2


def _region_batches(n, ignore):
    out = []
    for it in range(n):
        rng = np.random.default_rng(900 + it)
        segs = [rng.integers(0, 5 if ignore else 4, (BATCH, 1, IMG[0] >> s, IMG[1] >> s)).astype(np.uint8) for s in range(5)]
        out.append({"data": torch.from_numpy(rng.random((BATCH, 1) + IMG).astype(np.float32)),
                    "target": [torch.from_numpy(C.region_planes(s, ignore)) for s in segs]})
    return out


def test_plugin_replays_a_region_train_step_as_a_hipgraph():
    """A region dataset behind the plugin (three sigmoid heads, ignore plane): GRAPH_AFTER eager steps, then the step is captured and
    replayed twice; losses and parameters equal those of eager ``trainer.train_step`` calls with the same loss on a twin, bit for
    bit (deterministic mode, DropPath off)."""
    from oracle import mlagg_oracle as O
    assert nnunet_plugin.PLUGIN_GRAPH
    trainer.set_deterministic(True)
    try:
        dj = FK.make_dataset_json(3)
        dj["ignore_label"] = C.IGNORE
        cls = nnunet_plugin.make_trainer_class(C.region_trainer_base(FK.nnUNetTrainer), variant="B")
        tr = cls(FK.make_plans(IMG, BATCH), "2d_bs10", 0, dj, device=torch.device("cuda"))
        tr.initialize()
        O.deterministic_fill_(tr.network.state_dict())
        tr.network.eval()
        assert tr._graph_ok() and tr.optimizer.capturable and tr.base_calls["_build_loss"] == 0
        twin = copy.deepcopy(tr.network)
        twin_opt, _ = trainer.configure_optimizers(twin, tr.initial_lr, tr.weight_decay)
        n = nnunet_plugin.GRAPH_AFTER + 2
        for it, b in enumerate(_region_batches(n, True)):
            got = tr.train_step(b)
            want = trainer.train_step(twin, twin_opt, b["data"].cuda(), [t.cuda() for t in b["target"]], loss_fn=tr.loss)
            assert np.isfinite(got["loss"]) and float(got["loss"]) == float(want), it
            assert (tr._graphed is not None) == (it >= nnunet_plugin.GRAPH_AFTER), (it, tr._graph_failed)
        assert tr._graph_failed is None and tr.optimizer.steps_done() == n
        for (k, a), q in zip(tr.network.state_dict().items(), twin.state_dict().values()):
            assert torch.equal(a, q), k
    finally:
        trainer.set_deterministic(False)
