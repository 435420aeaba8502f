"""The seeded inputs of tests/golden/regions.npz (made by tests/golden/make_golden_regions.py with the reference's own loss classes and
LabelManager) and the helpers its tests share.  BraTS-style regions: labels 0 .. 3, whole tumour (1, 2, 3), tumour core (2, 3),
enhancing tumour (3,); the ignore label is 4 (the highest label + 1, as label_handling.py:40-44 demands)."""
import numpy as np

REGIONS = ((1, 2, 3), (2, 3), (3,))
IGNORE = 4
LOSS_SHAPES = ((45, 47), (22, 23), (11, 11))            # 2115 pixels: three workgroups of 1024 with a ragged tail; 506; 121
LOSS_CASES = tuple((bd, ign) for bd in (True, False) for ign in (False, True))      # (batch dice, ignore plane)
SPECIAL = (0.0, 20.0, -20.0, 100.0, -100.0)
BAND = 1e-6                                             # no decided value may lie in (0, BAND): see make_golden_regions.py


def loss_tag(batch_dice, ignore):
    return f"loss/bd{int(batch_dice)}_ign{int(ignore)}"


def loss_inputs(seed=29):
    """-> (logits per level (2, 3, h, w) fp32, label maps per level (2, 1, h, w) uint8 without the ignore label, the same with it).
    The logits hold 0, +-20 and +-100 at fixed places of every head; with the ignore label about a quarter of the pixels carry it and
    the coarsest level carries it everywhere (a fully ignored level)."""
    rng = np.random.default_rng(seed)
    logits, seg, seg_ign = [], [], []
    for li, (h, w) in enumerate(LOSS_SHAPES):
        z = (rng.standard_normal((2, 3, h, w)) * 2.0).astype(np.float32)
        flat = z.reshape(2, 3, -1)
        for i, v in enumerate(SPECIAL):
            flat[:, :, 7 * i + 3] = v                   # every special value meets both target values somewhere
            flat[:, :, h * w - 1 - 5 * i] = v
        s = rng.integers(0, 4, (2, 1, h, w)).astype(np.uint8)
        si = s.copy()
        si[rng.random(s.shape) < 0.25] = IGNORE
        if li == len(LOSS_SHAPES) - 1:
            si[:] = IGNORE
        logits.append(z)
        seg.append(s)
        seg_ign.append(si)
    return logits, seg, seg_ign


def region_planes(seg, ignore=False):
    """ConvertSegmentationToRegionsTransform restated: plane r = np.isin(seg, REGIONS[r]); with `ignore` the plane of the ignore
    label follows.  seg (B, 1, ...) -> (B, R (+ 1), ...) float32."""
    planes = [np.isin(seg, r) for r in REGIONS]
    if ignore:
        planes.append(seg == IGNORE)
    return np.concatenate(planes, 1).astype(np.float32)


# tag: (logits shape (preprocessed), configuration spacing, properties spacing, shape_before_cropping, bbox lower corner,
#       shape_after_cropping_and_before_resampling, transpose_backward, regions_class_order)
EXPORT_CASES = {
    "iso": ((10, 12, 9), (2.0, 2.0, 2.0), (1.1, 1.1, 1.1), (20, 24, 18), (1, 1, 1), (18, 22, 16), (2, 0, 1), (1, 2, 3)),
    "aniso": ((6, 11, 8), (3.0, 1.6, 1.6), (2.0, 0.8, 0.8), (10, 24, 18), (1, 2, 1), (9, 22, 16), (1, 2, 0), (1, 3, 2)),
}


def export_logits(tag, seed=31):
    """(3, *shape) fp32 logits; a block of head 0 is exactly 0 where the other two heads are negative (the resampled logits are then
    exactly 0 inside it: sigmoid 0.5, which must not fire), and one corner block is negative in every head (no region fires)."""
    shape = EXPORT_CASES[tag][0]
    z = (np.random.default_rng(seed + len(tag)).standard_normal((3,) + shape) * 2.0).astype(np.float32)
    z[:, :3, :4, :3] = -np.abs(z[:, :3, :4, :3]) - 0.5
    z[0, -3:, -4:, -3:] = 0.0
    z[1:, -3:, -4:, -3:] = -np.abs(z[1:, -3:, -4:, -3:]) - 0.5
    return z


def export_properties(tag):
    _, _, spacing, full, lo, crop, _, _ = EXPORT_CASES[tag]
    return {"spacing": list(spacing), "shape_before_cropping": tuple(full),
            "bbox_used_for_cropping": [[a, a + c] for a, c in zip(lo, crop)],
            "shape_after_cropping_and_before_resampling": tuple(crop)}


def paste(tag, box_values):
    """What export_prediction.py:44-63 does after the label manager: box_values (..., *crop) into zeros of shape_before_cropping at
    the bbox, then transpose_backward."""
    _, _, _, full, lo, crop, tb, _ = EXPORT_CASES[tag]
    lead = box_values.shape[:-3]
    out = np.zeros(lead + tuple(full), dtype=box_values.dtype)
    out[(Ellipsis,) + tuple(slice(a, a + c) for a, c in zip(lo, crop))] = box_values
    n = len(lead)
    return np.ascontiguousarray(out.transpose(tuple(range(n)) + tuple(n + p for p in tb)))


ENSEMBLE_SHAPE = (3, 7, 9, 11)                          # 693 voxels per head: not a multiple of 4
ENSEMBLE_ORDER = (1, 3, 2)


def ensemble_members(dtype, seed=37):
    """Two members of sigmoid probabilities (multiples of 2^-10, exact in fp16 and fp32); the first voxels of every head have the mean
    exactly 0.5 (0.25 and 0.75), which must not fire."""
    rng = np.random.default_rng(seed)
    members = [(rng.integers(0, 1025, ENSEMBLE_SHAPE) / 1024.0).astype(dtype) for _ in range(2)]
    members[0].reshape(3, -1)[:, :5] = 0.25
    members[1].reshape(3, -1)[:, :5] = 0.75
    return members


def dataset_json():
    return {"labels": {"background": 0, "whole_tumor": [1, 2, 3], "tumor_core": [2, 3], "enhancing_tumor": [3]},
            "regions_class_order": [1, 2, 3], "file_ending": ".nii.gz"}


def region_trainer_base(base):
    """`base` (the stand-in nnUNetTrainer of tests/fake_nnunet.py, whose own label manager only carries a has_regions flag) with a
    RegionLabelManager behind the trainer and its plans manager; the ignore label comes from dataset_json["ignore_label"]."""

    class RegionTrainer(base):
        def __init__(self, plans, configuration, fold, dataset_json, unpack_dataset=True, device=None):
            super().__init__(plans, configuration, fold, dataset_json, unpack_dataset, device)
            lm = RegionLabelManager(ignore_label=dataset_json.get("ignore_label"))
            self.label_manager = lm
            self.plans_manager.get_label_manager = lambda dj: lm

    return RegionTrainer


class RegionLabelManager:
    """The members of the reference's LabelManager that this package reads, for a region-based dataset."""

    def __init__(self, regions=REGIONS, regions_class_order=(1, 2, 3), ignore_label=None):
        self.has_regions = True
        self.foreground_regions = list(regions)
        self.regions_class_order = list(regions_class_order)
        self.num_segmentation_heads = len(regions)
        self.ignore_label = ignore_label
        self.has_ignore_label = ignore_label is not None
        self.all_labels = sorted({v for r in regions for v in r} | {0})
