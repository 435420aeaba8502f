"""The loss-variant trainers on the host: the eager compositions of trainer.loss_variant_deep_supervision_loss against the reference's
own TopKLoss, DC_and_topk_loss, MemoryEfficientSoftDiceLoss, RobustCrossEntropyLoss and DC_and_CE_loss(smooth 0)
(tests/golden/loss_variants.npz, made by tests/golden/make_golden_loss_variants.py), the k rule, the refusals, the plugin factories
and the ABI of K33."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fake_nnunet as FK
import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import _lib, nnunet_plugin, ops, trainer
from tests import _loss_variant_cases as C
from tests import _region_cases as RC
from tests.test_plugin_cpu import StubNet

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "loss_variants.npz"))


@pytest.mark.parametrize("variant,batch_dice,ignore", C.cases())
def test_eager_variant_matches_the_reference_classes(variant, batch_dice, ignore):
    """Value and logit gradients of every level; the tolerances of the loss.npz / loss_ignore.npz tests in test_oracle_golden.py."""
    assert int(GOLDEN["seed"]) == C.SEED
    logits, labels = C.inputs(ignore)
    zs = [z.requires_grad_(True) for z in logits]
    loss = trainer.loss_variant_deep_supervision_loss(zs, labels, variant, batch_dice, ignore_label=C.IGNORE if ignore else None)
    tag = C.tag(variant, batch_dice, ignore)
    assert abs(float(loss.detach()) - float(GOLDEN[f"{tag}/value"])) < 1e-6
    for i, g in enumerate(torch.autograd.grad(loss, zs)):
        assert float((g - torch.from_numpy(GOLDEN[f"{tag}/grad{i}"])).abs().max()) < 1e-7, i
    assert set(trainer.LOSS_VARIANTS) == set(C.VARIANTS)


def test_k_rule_and_k_zero():
    """k = int(N * 10 / 100) in Python float arithmetic (robust_ce_loss.py:30-31); k == 0 raises where the reference returns NaN."""
    want = {9: 0, 10: 1, 19: 1, 189: 18, 2146: 214, 655360: 65536}
    for n, k in want.items():
        assert int(np.prod((n,), dtype=np.int64) * 10 / 100) == k          # the reference's own expression
        if k:
            assert ops.topk_count(n, 10) == k
        else:
            with pytest.raises(RuntimeError):
                ops.topk_count(n, 10)
    z, y = torch.randn(1, 3, 3, 3), torch.zeros(1, 1, 3, 3)                # N = 9
    for variant in ("topk10", "topk10_ls01", "dice_topk10"):
        with pytest.raises(RuntimeError):
            trainer.loss_variant_deep_supervision_loss([z], [y], variant)
    with pytest.raises(RuntimeError):
        trainer.loss_variant_deep_supervision_loss([z], [y], "focal")


def test_a_fully_ignored_level_contributes_no_cross_entropy():
    logits, labels = C.inputs(True)
    labels[-1] = torch.full_like(labels[-1], C.IGNORE)
    for variant in ("topk10", "ce", "dice_topk10"):
        zs = [z.detach().requires_grad_(True) for z in logits]
        loss = trainer.loss_variant_deep_supervision_loss(zs, labels, variant, ignore_label=C.IGNORE)
        assert torch.isfinite(loss)
        g = torch.autograd.grad(loss, zs, allow_unused=True)[-1]
        assert g is None or float(g.abs().max()) == 0.0


def _regions_case():
    g = torch.Generator().manual_seed(3)
    logits = [torch.randn(2, 3, 16 >> s, 16 >> s, generator=g) for s in range(3)]
    planes = [(torch.rand(2, 3, 16 >> s, 16 >> s, generator=g) > 0.5).float() for s in range(3)]
    return logits, planes


def test_regions_are_refused_where_the_reference_refuses_them():
    logits, planes = _regions_case()
    for variant in ("topk10", "topk10_ls01", "dice_topk10", "ce"):
        with pytest.raises(RuntimeError, match="regions not supported by this trainer"):
            trainer.loss_variant_deep_supervision_loss(logits, planes, variant, regions=True)
    # the two that the reference builds for regions: MemoryEfficientSoftDiceLoss(sigmoid, do_bg True) alone, DC_and_BCE_loss(smooth 0)
    ws = trainer.deep_supervision_weights(3)
    for variant, smooth, w_ce in (("dice", 1e-5, 0.0), ("dice_ce_nosmooth", 0.0, 1.0)):
        got = trainer.loss_variant_deep_supervision_loss(logits, planes, variant, regions=True)
        want = sum(w * trainer.dc_and_bce_loss(z, t, True, False, False, smooth, w_ce, 1.0) for w, z, t in zip(ws, logits, planes))
        assert abs(float(got) - float(want)) < 1e-6
    z, t = logits[0], planes[0]
    full = trainer.dc_and_bce_loss(z, t)
    dice_only = trainer.dc_and_bce_loss(z, t, weight_ce=0.0)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(z, t)
    assert abs(float(full) - float(dice_only + bce)) < 1e-6 and float(dice_only) < 0
    # the defaults are untouched
    assert torch.equal(trainer.region_deep_supervision_loss(logits, planes), trainer.region_deep_supervision_loss(logits, planes, weight_ce=1.0, weight_dice=1.0))


@pytest.fixture
def stub_model(monkeypatch):
    from mlagg_unet_amd import model

    def build(patch_size, in_ch, n_cls, ds=True, variant="B", precision="fp32"):
        torch.manual_seed(0)
        return StubNet(in_ch, n_cls, ds)

    monkeypatch.setattr(model, "build_network_architecture", build)
    monkeypatch.setenv("MLAGG_MIOPEN_TUNED", "0")


def _cpu_trainer(cls, dataset_json):
    tr = cls(FK.make_plans((32, 32), 2), "2d_bs10", 0, dataset_json, device=torch.device("cpu"))
    tr.initialize()
    return tr


def test_default_factory_classes_are_unchanged(stub_model):
    g = torch.Generator().manual_seed(4)
    outs = [torch.randn(2, 5, 32 >> s, 32 >> s, generator=g) for s in range(5)]
    tg = [torch.round(torch.rand(2, 1, 32 >> s, 32 >> s, generator=g) * 4) for s in range(5)]
    want = trainer.deep_supervision_loss(outs, tg, True, False)
    for cls in (nnunet_plugin.make_trainer_class(FK.nnUNetTrainer), nnunet_plugin.make_trainer_class(FK.nnUNetTrainer, loss="dice_ce")):
        assert cls.__name__ == "nnUNetTrainer_MLAgg_2D_dt_MS"
        tr = _cpu_trainer(cls, FK.make_dataset_json(5))
        assert tr.mlagg_loss_variant == "dice_ce" and torch.equal(tr.loss(outs, tg), want)
    cls3d = nnunet_plugin.make_umamba_enc_ss3d_trainer_class(FK.nnUNetTrainer)
    assert cls3d.__name__ == "nnUNetTrainerUMambaEnc_SS3D"
    tr3d = cls3d.__new__(cls3d)
    tr3d.label_manager, tr3d.is_ddp, tr3d.configuration_manager = tr.label_manager, False, tr.configuration_manager
    assert torch.equal(cls3d._build_loss(tr3d)(outs, tg), want)


@pytest.mark.parametrize("variant", sorted(C.VARIANTS))
def test_factories_build_the_variant(stub_model, variant):
    logits, labels = C.inputs(True)
    want = float(GOLDEN[f"{C.tag(variant, True, True)}/value"])
    dj = FK.make_dataset_json(6)
    dj["ignore_label"] = C.IGNORE
    cls = nnunet_plugin.make_trainer_class(FK.nnUNetTrainer, loss=variant)
    assert cls.__name__ == "nnUNetTrainer_MLAgg_2D_dt_MS"
    tr = _cpu_trainer(cls, dj)
    assert tr.mlagg_loss_variant == variant and tr.base_calls["_build_loss"] == 0
    assert abs(float(tr.loss(logits, labels)) - want) < 1e-6
    one = trainer.loss_variant_deep_supervision_loss([logits[0]], [labels[0]], variant, True, ignore_label=C.IGNORE)
    assert torch.equal(tr.loss(logits[0], labels[0]), one)                         # deep supervision off
    on_gpu = cls(FK.make_plans((32, 32), 2), "2d_bs10", 0, dj, device=torch.device("cuda"))      # constructing needs no GPU
    assert on_gpu._graph_ok() is bool(nnunet_plugin.PLUGIN_GRAPH)
    cls3d = nnunet_plugin.make_umamba_enc_ss3d_trainer_class(FK.nnUNetTrainer, loss=variant)
    tr3d = cls3d.__new__(cls3d)
    tr3d.label_manager, tr3d.is_ddp, tr3d.configuration_manager = tr.label_manager, False, tr.configuration_manager
    assert torch.equal(cls3d._build_loss(tr3d)(logits, labels), tr.loss(logits, labels))
    # validation evaluates self.loss (B:897)
    # 64 x 64: the coarsest of the five levels then holds 32 pixels, k = 3 (at 32 x 32 it would hold 8 and the top-k would raise)
    batch = {"data": torch.rand(2, 1, 64, 64), "target": [torch.randint(0, 6, (2, 1, 64 >> s, 64 >> s)).float() for s in range(5)]}
    out = tr.validation_step(batch)
    with torch.no_grad():
        assert abs(float(out["loss"]) - float(tr.loss(tr.network(batch["data"]), batch["target"]))) < 1e-6


def test_plugin_refuses_regions_and_unknown_losses(stub_model):
    with pytest.raises(RuntimeError):
        nnunet_plugin.make_trainer_class(FK.nnUNetTrainer, loss="focal")
    with pytest.raises(RuntimeError):
        nnunet_plugin.make_umamba_enc_ss3d_trainer_class(FK.nnUNetTrainer, loss="focal")
    base = RC.region_trainer_base(FK.nnUNetTrainer)
    for variant in ("topk10", "ce"):
        cls = nnunet_plugin.make_trainer_class(base, loss=variant)
        tr = cls(FK.make_plans((32, 32), 2), "2d_bs10", 0, FK.make_dataset_json(3), device=torch.device("cpu"))
        with pytest.raises(RuntimeError, match="regions not supported by this trainer"):
            tr.initialize()
    tr = _cpu_trainer(nnunet_plugin.make_trainer_class(base, loss="dice"), FK.make_dataset_json(3))
    logits, planes = _regions_case()
    assert abs(float(tr.loss(logits, planes)) - float(trainer.loss_variant_deep_supervision_loss(logits, planes, "dice", regions=True))) < 1e-6


def test_abi_symbols_exist_and_check_their_arguments():
    """The entry points of K33 reject NULL and unsupported sizes on the host: no kernel is launched, no GPU is needed."""
    lib = _lib.lib()
    U, N = _lib.CONSTANTS["MLAGG_E_UNSUPPORTED"], _lib.CONSTANTS["MLAGG_E_NULLPTR"]
    assert lib.mlagg_topk_ce_record_floats() == ops.TOPK_RECORD_WORDS == 8
    epw = lib.mlagg_topk_ce_select_elements_per_workgroup()
    assert epw > 0 and lib.mlagg_topk_ce_select_workspace_bytes(0) == 0
    assert lib.mlagg_topk_ce_select_workspace_bytes(epw + 1) - lib.mlagg_topk_ce_select_workspace_bytes(epw) == 8   # one partial more
    assert lib.mlagg_topk_ce_select_workspace_bytes(655360) % 8 == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    maxc = lib.mlagg_dice_ce_max_classes()
    assert lib.mlagg_topk_ce_stats(None, p, None, None, None, p, None, 1, 5, 16, -1, 0.0, None) == N
    assert lib.mlagg_topk_ce_stats(p, p, None, None, None, None, None, 1, 5, 16, -1, 0.0, None) == N            # ce_pix is required
    assert lib.mlagg_topk_ce_stats(p, p, p, None, None, p, None, 1, 5, 16, -1, 0.0, None) == N                  # Dice: all four or none
    assert lib.mlagg_topk_ce_stats(p, p, None, None, None, p, None, 1, maxc + 1, 16, -1, 0.0, None) == U
    assert lib.mlagg_topk_ce_stats(p, p, None, None, None, p, None, 1, 1, 16, -1, 0.0, None) == U
    assert lib.mlagg_topk_ce_stats(p, p, None, None, None, p, None, 1, 5, 16, -1, 1.5, None) == U
    assert lib.mlagg_topk_ce_select(None, p, p, 16, 1, None) == N and lib.mlagg_topk_ce_select(p, None, p, 16, 1, None) == N
    assert lib.mlagg_topk_ce_select(p, p, None, 16, 1, None) == N
    assert lib.mlagg_topk_ce_select(p, p, p, 16, 0, None) == U and lib.mlagg_topk_ce_select(p, p, p, 16, 17, None) == U
    assert lib.mlagg_topk_ce_grad(p, p, p, p, None, None, p, 1, 5, 16, 1, -1, 0.0, None) == N                   # g_topk is required
    assert lib.mlagg_topk_ce_grad(p, p, None, p, None, p, p, 1, 5, 16, 1, -1, 0.0, None) == N
    assert lib.mlagg_topk_ce_grad(p, p, p, p, None, p, p, 1, maxc + 1, 16, 1, -1, 0.0, None) == U
    assert lib.mlagg_topk_ce_grad(p, p, p, p, None, p, p, 1, 5, 16, 0, -1, 0.0, None) == U
    names = [lib.mlagg_profile_kernel_name(i).decode() for i in range(lib.mlagg_profile_kernel_count())]
    assert sum("topk_ce" in n for n in names) == 3 and len(set(names)) == len(names)
    with pytest.raises(RuntimeError):
        ops.topk_ce_stats([torch.zeros(1, 3, 8, 8)], [torch.zeros(1, 1, 8, 8)])                                  # no CPU fallback in ops
