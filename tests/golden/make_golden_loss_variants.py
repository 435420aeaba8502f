"""Generate tests/golden/loss_variants.npz from the REFERENCE's own loss classes, as its loss-variant trainers build them
(training/nnUNetTrainer/variants/loss/nnUNetTrainer{TopkLoss,DiceLoss,CELoss}.py).

    MLAGG_REFERENCE=<reference checkout> python tests/golden/make_golden_loss_variants.py

For the seeded inputs of tests/_loss_variant_cases.py -- three levels (2, 5, 24, 20), (2, 5, 12, 10), (2, 5, 6, 5), and once more with
6-channel logits and ignore_label = 5 -- it records value and per-level logit gradients of DeepSupervisionWrapper(loss), weights
1 / 2^i normalised, for
  topk10            TopKLoss(ignore_index, k=10)
  topk10_ls01       TopKLoss(ignore_index, k=10, label_smoothing=0.1)
  dice_topk10       DC_and_topk_loss({batch_dice, smooth 1e-5, do_bg False, ddp False}, {k 10, label_smoothing 0.0}, 1, 1, ignore_label)
  dice              MemoryEfficientSoftDiceLoss(batch_dice, do_bg False, smooth 1e-5, ddp False, apply_nonlin=softmax_helper_dim1)
  ce                RobustCrossEntropyLoss(weight=None, ignore_index)
  dice_ce_nosmooth  DC_and_CE_loss({batch_dice, smooth 0, do_bg False, ddp False}, {}, 1, 1, ignore_label, MemoryEfficientSoftDiceLoss)
with batch_dice True and False for the ones with a Dice term.  The reference's modules are imported unmodified, with the stand-ins of
make_golden_ensemble.py for the absent third-party modules.  Only seeds, values and gradients are stored; only the data is committed."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if "MLAGG_REFERENCE" not in os.environ:
    raise SystemExit("set MLAGG_REFERENCE to a checkout of the reference repository (aticejiang/MLAgg-UNet)")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.environ["MLAGG_REFERENCE"], "mlagg"))

import make_golden_ensemble as MGE  # noqa: E402  (its stand-ins for the third-party modules; importing it runs nothing)
from tests import _loss_variant_cases as C  # noqa: E402


def reference_loss(variant, batch_dice, ignore, n_levels):
    RC = importlib.import_module("nnunetv2.training.loss.robust_ce_loss")
    CL = importlib.import_module("nnunetv2.training.loss.compound_losses")
    DL = importlib.import_module("nnunetv2.training.loss.dice")
    DS = importlib.import_module("nnunetv2.training.loss.deep_supervision")
    H = importlib.import_module("nnunetv2.utilities.helpers")
    index = C.IGNORE if ignore else -100
    label = C.IGNORE if ignore else None
    if variant == "topk10":
        loss = RC.TopKLoss(ignore_index=index, k=10)
    elif variant == "topk10_ls01":
        loss = RC.TopKLoss(ignore_index=index, k=10, label_smoothing=0.1)
    elif variant == "dice_topk10":
        loss = CL.DC_and_topk_loss({'batch_dice': batch_dice, 'smooth': 1e-5, 'do_bg': False, 'ddp': False},
                                   {'k': 10, 'label_smoothing': 0.0}, weight_ce=1, weight_dice=1, ignore_label=label)
    elif variant == "dice":
        loss = DL.MemoryEfficientSoftDiceLoss(**{'batch_dice': batch_dice, 'do_bg': False, 'smooth': 1e-5, 'ddp': False},
                                              apply_nonlin=H.softmax_helper_dim1)
    elif variant == "ce":
        loss = RC.RobustCrossEntropyLoss(weight=None, ignore_index=index)
    else:
        loss = CL.DC_and_CE_loss({'batch_dice': batch_dice, 'smooth': 0, 'do_bg': False, 'ddp': False}, {}, weight_ce=1, weight_dice=1,
                                 ignore_label=label, dice_class=DL.MemoryEfficientSoftDiceLoss)
    weights = np.array([1 / (2 ** i) for i in range(n_levels)])
    return DS.DeepSupervisionWrapper(loss, weights / weights.sum())


def main():
    MGE._stub_third_party()
    out = {"seed": np.int64(C.SEED)}
    for variant, bd, ign in C.cases():
        logits, labels = C.inputs(ign)
        zs = [z.requires_grad_(True) for z in logits]
        value = reference_loss(variant, bd, ign, len(zs))(zs, labels)
        grads = torch.autograd.grad(value, zs)
        assert torch.isfinite(value) and all(torch.isfinite(g).all() for g in grads)
        t = C.tag(variant, bd, ign)
        out[f"{t}/value"] = np.float32(value.item())
        for li, g in enumerate(grads):
            out[f"{t}/grad{li}"] = g.numpy()
        print(t, float(value.detach()))
    path = os.path.join(HERE, "loss_variants.npz")
    np.savez_compressed(path, **out)
    print("loss_variants", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
