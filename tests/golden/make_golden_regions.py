"""Generate tests/golden/regions.npz from the REFERENCE's own loss classes and LabelManager, for region-based datasets (sigmoid heads).

    MLAGG_REFERENCE=<reference checkout> python tests/golden/make_golden_regions.py

For the inputs of tests/_region_cases.py it records:
  - loss: value and per-level logit gradients of DeepSupervisionWrapper(DC_and_BCE_loss({}, {batch_dice, do_bg True, smooth 1e-5, ddp False},
    use_ignore_label, dice_class=MemoryEfficientSoftDiceLoss)), built exactly as nnUNetTrainer.py:330-352 builds it, for batch dice on / off
    and with / without the ignore plane (four cases; the coarsest level is fully ignored in the ignore cases), in fp32, and the value of
    the same classes on float64 inputs.  The targets are ConvertSegmentationToRegionsTransform restated as np.isin on the label maps, so
    the label maps are stored and both target forms of K29 can be fed from them.
  - segmentation: LabelManager.apply_inference_nonlin and convert_logits_to_segmentation (label_handling.py:128-182) of the resampled
    logits of two export cases (the resampling is the package's host path, which tests/golden/export.npz pins to the reference's);
  - ensembling: nnunetv2.ensembling.ensemble.average_probabilities (:17-29) of two members, fp32 and fp16, and
    LabelManager.convert_probabilities_to_segmentation (:146-177) of that mean.
The reference's modules are imported unmodified, with the stand-ins of make_golden_ensemble.py for the absent third-party modules.

A condition on the inputs is asserted here and again by the tests: no value that reaches a `> 0.5` decision lies strictly between the
threshold and BAND = 1e-6 from it -- no resampled logit has 0 < |z| < 1e-6 and no member mean has 0 < |mean - 0.5| < 1e-6.  Inside that
band two correctly working fp32 sigmoids may round to different sides of 0.5; outside it, and exactly on the threshold (which does not
fire), they must agree.
Only the data is committed."""
import importlib
import os
import sys
import tempfile

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
from tests import _region_cases as C  # noqa: E402


def _reference_loss(CL, DS, DL, batch_dice, ignore, n_levels):
    loss = CL.DC_and_BCE_loss({}, {'batch_dice': batch_dice, 'do_bg': True, 'smooth': 1e-5, 'ddp': False},
                              use_ignore_label=ignore, dice_class=DL.MemoryEfficientSoftDiceLoss)
    weights = np.array([1 / (2 ** i) for i in range(n_levels)])
    return DS.DeepSupervisionWrapper(loss, weights / weights.sum())


def main():
    MGE._stub_third_party()
    ENS = importlib.import_module("nnunetv2.ensembling.ensemble")
    L = importlib.import_module("nnunetv2.utilities.label_handling.label_handling")
    CL = importlib.import_module("nnunetv2.training.loss.compound_losses")
    DS = importlib.import_module("nnunetv2.training.loss.deep_supervision")
    DL = importlib.import_module("nnunetv2.training.loss.dice")
    import mlagg_unet_amd  # noqa: F401
    from mlagg_unet_amd import export as E
    out = {}

    # ---- loss ----
    logits, seg, seg_ign = C.loss_inputs()
    for li in range(len(logits)):
        out[f"loss/logits{li}"] = logits[li]
        out[f"loss/seg{li}"] = seg[li]
        out[f"loss/seg_ign{li}"] = seg_ign[li]
        for v in C.SPECIAL:
            assert (logits[li] == v).any(), (li, v)
    assert (seg_ign[-1] == C.IGNORE).all() and 0 < (seg_ign[0] == C.IGNORE).mean() < 0.5
    for bd, ign in C.LOSS_CASES:
        wrap = _reference_loss(CL, DS, DL, bd, ign, len(logits))
        targets = [torch.from_numpy(C.region_planes(s, ign)) for s in (seg_ign if ign else seg)]
        zs = [torch.from_numpy(z).requires_grad_(True) for z in logits]
        value = wrap(zs, targets)
        grads = torch.autograd.grad(value, zs)
        z64 = [torch.from_numpy(z).double().requires_grad_(True) for z in logits]
        value64 = wrap(z64, [t.double() for t in targets])
        grads64 = torch.autograd.grad(value64, z64)
        assert torch.isfinite(value) and all(torch.isfinite(g).all() for g in grads)
        tag = C.loss_tag(bd, ign)
        out[f"{tag}/value"] = np.float32(value.item())
        out[f"{tag}/value64"] = np.float64(value64.item())
        for li, g in enumerate(grads):
            out[f"{tag}/grad{li}"] = g.numpy()
        value, value64 = value.detach(), value64.detach()
        print(tag, float(value), "fp32 classes against float64: value", abs(float(value) - float(value64)), "gradients",
              max(float((a.double() - b).abs().max()) for a, b in zip(grads, grads64)))

    # ---- segmentation ----
    labels = {"background": 0, "whole_tumor": (1, 2, 3), "tumor_core": (2, 3), "enhancing_tumor": (3,)}
    for tag, (shape, cfg, spacing, full, lo, crop, tb, order) in C.EXPORT_CASES.items():
        lm = L.LabelManager(labels, list(order))
        assert lm.has_regions and lm.num_segmentation_heads == 3 and tuple(lm.foreground_regions) == C.REGIONS
        z = C.export_logits(tag)
        cur = E.current_spacing_for(cfg, C.export_properties(tag))
        resampled = E.resample_logits_to_shape(torch.from_numpy(z), crop, cur, spacing).numpy()
        assert resampled.shape == (3,) + tuple(crop)
        a = np.abs(resampled)
        assert not ((a > 0) & (a < C.BAND)).any(), tag
        probs = lm.apply_inference_nonlin(resampled)
        segm = lm.convert_logits_to_segmentation(resampled)
        assert probs.dtype == np.float32 and segm.dtype == np.uint8
        fired = resampled > 0
        assert (resampled == 0).sum() > 0 and np.array_equal(probs > 0.5, fired), tag         # exact zeros do not fire
        assert (~fired.any(0)).sum() > 0 and (segm[~fired.any(0)] == 0).all(), tag             # voxels where no region fires
        assert (fired.sum(0) > 1).sum() > 0, tag                                               # a later region overwrites an earlier one
        assert ((resampled == 0).any(0) & ~fired.any(0)).sum() > 0, tag                        # a zero logit alone: background
        out[f"seg/{tag}/logits"] = z
        out[f"seg/{tag}/resampled"] = resampled
        out[f"seg/{tag}/probabilities"] = probs
        out[f"seg/{tag}/segmentation"] = segm
        print("segmentation", tag, resampled.shape, "zeros", int((resampled == 0).sum()), "labels", np.bincount(segm.ravel()))

    # ---- ensembling ----
    lm = L.LabelManager(labels, list(C.ENSEMBLE_ORDER))
    with tempfile.TemporaryDirectory() as tmp:
        for name, dtype in (("fp32", np.float32), ("fp16", np.float16)):
            members = C.ensemble_members(dtype)
            files = MGE._write_members(os.path.join(tmp, name), name, members)
            mean = ENS.average_probabilities(files)
            assert mean.dtype == np.float32
            d = np.abs(mean - np.float32(0.5))
            assert not ((d > 0) & (d < C.BAND)).any() and (mean == 0.5).sum() >= 15, name
            segm = lm.convert_probabilities_to_segmentation(mean)
            for i, m in enumerate(members):
                out[f"ens/{name}/member{i}"] = m
            out[f"ens/{name}/mean"] = mean
            out[f"ens/{name}/labels"] = segm
            print("ensemble", name, mean.shape, "labels", np.bincount(segm.ravel()))
    np.savez_compressed(os.path.join(HERE, "regions.npz"), **out)
    print("regions", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "regions.npz")), "bytes")


if __name__ == "__main__":
    main()
