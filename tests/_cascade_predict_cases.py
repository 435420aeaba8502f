"""The seeded cases of tests/golden/cascade_predict.npz (made by tests/golden/make_golden_cascade_predict.py with the reference's own
resample_and_save, DefaultPreprocessor.run_case(seg_file=previous stage) and convert_labelmap_to_one_hot): the cascade's hand-off out
of the low-resolution stage, one case per branch of its resampler, and the preprocessing of a cascaded stage's case with the previous
stage's segmentation, on raw volumes and label maps of tests/_preprocess_train_cases.py."""
import copy

import numpy as np

from tests import _preprocess_train_cases as T

GAP = 1e-6                  # two largest probabilities closer than this: the label there is a near-tie (the rule of the export tests)
GAP_SHARE = 1e-3            # at most this share of a case's voxels may be near-ties

# resample_and_save.  tag: (K, logits shape (low-resolution stage), that configuration's spacing, properties spacing, target_shape
# (the next stage's preprocessed shape), seed, what it covers)
HANDOFF = {
    "a_isotropic": (4, (10, 12, 8), (1.5, 1.5, 1.5), (1.0, 2.0, 1.5), (15, 9, 8), 7,
                    "isotropic low-resolution spacing: trilinear, one axis up, one down, one unchanged"),
    "b_separate_z": (14, (6, 12, 11), (3.0, 0.8, 0.8), (2.2, 0.6, 0.6), (8, 16, 14), 7,
                     "anisotropic low-resolution spacing: separate z, the low-resolution axis changes size"),
    "c_two_lowres": (2, (20, 5, 6), (0.24, 1.25, 1.25), (0.3, 0.9, 1.6), (15, 7, 5), 7,
                     "two-axis low-resolution spacing: no separate z"),
    "d_same_shape": (4, (8, 9, 10), (2.0, 2.0, 2.0), (1.0, 1.0, 1.0), (8, 9, 10), 7, "target_shape equal to the input shape"),
}


def logits(tag):
    """The generator of tests/_export_cases.py with the case's seed."""
    K, shape, seed = HANDOFF[tag][0], HANDOFF[tag][1], HANDOFF[tag][5]
    rng = np.random.default_rng(seed + sum(map(ord, tag)))
    return (rng.standard_normal((K,) + shape) * 2.0).astype(np.float32)


def handoff_properties(tag):
    _, shape, _, spacing, _, _, _ = HANDOFF[tag]
    return {"spacing": list(spacing), "shape_after_cropping_and_before_resampling": tuple(shape)}


def handoff_dataset_json(K):
    labels = {"background": 0}
    labels.update({f"class_{k}": k for k in range(1, K)})
    return {"labels": labels, "file_ending": ".nii.gz"}


def host_probabilities(tag):
    """fp32 softmax of the host path's resampled logits of a hand-off case (K, *target_shape): what the near-tie rule reads."""
    import torch
    from mlagg_unet_amd import export
    _, _, spacing, _, target, _, _ = HANDOFF[tag]
    cur = export.current_spacing_for(spacing, handoff_properties(tag))
    return torch.softmax(export.resample_logits_to_shape(torch.from_numpy(logits(tag)), target, cur, cur), 0)


def sure(probs, gap=GAP):
    """voxels whose two largest probabilities differ by more than gap (the label there is not a near-tie)"""
    top2 = probs.topk(2, dim=0).values
    return (top2[0] - top2[1]) > gap


# run_case with the previous stage's segmentation.  tag: the case of tests/_preprocess_train_cases.py whose image, label volume (here:
# the previous stage's exported segmentation in the original geometry) and plans it takes, and what it covers
PREPROCESS = {
    "f_border_box": "off-centre non-zero box, transpose_forward (1, 0, 2); the previous stage labelled voxels outside the non-zero "
                    "mask (label 2 where the filled mask is off, label 3 outside the crop box)",
    "a_sep_z_changes": "anisotropic case: separate z, the low-resolution axis changes size",
    "g_masked_zscore": "two channels, masked ZScore: its mask is seg >= 0 of the previous stage's cropped segmentation",
}
STAGE = "3d_cascade_fullres"


def image(tag):
    return T.image(tag)


def previous_stage_seg(tag):
    """(1, x, y, z) int16 in the original geometry."""
    return T.seg(tag)


def properties(tag):
    return T.properties(tag)


def dataset_json(tag):
    return T.dataset_json(tag)


def foreground_labels(tag):
    return sorted(v for v in T.CASES[tag]["labels"].values() if v != 0)


def plans(tag):
    """The plans of the base case with its configuration renamed to a cascaded stage (previous_stage 3d_lowres)."""
    plans, name = T.plans(tag)
    plans = copy.deepcopy(plans)
    cfg = plans["configurations"].pop(name)
    cfg["previous_stage"] = "3d_lowres"
    plans["configurations"][STAGE] = cfg
    return plans, STAGE


# a two-stage toy plan for predict_cascade_case and next_stage_target_shape: the base case's configuration as the cascaded stage and a
# copy of it at `lowres_spacing` as 3d_lowres
TOY_LABELS = {"background": 0, "a": 1, "b": 2, "c": 3}


def cascade_plans(tag, lowres_spacing):
    plans, name = T.plans(tag)
    plans = copy.deepcopy(plans)
    full = plans["configurations"].pop(name)
    low = copy.deepcopy(full)
    low["spacing"] = [float(s) for s in lowres_spacing]
    full["previous_stage"] = "3d_lowres"
    plans["configurations"] = {"3d_lowres": low, STAGE: full}
    return plans
