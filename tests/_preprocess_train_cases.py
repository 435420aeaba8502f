"""The seeded training cases of tests/golden/preprocess_train.npz (made by tests/golden/make_golden_preprocess_train.py with the
reference's own DefaultPreprocessor.run_case(seg_file=...) and DatasetFingerprintExtractor): the raw volumes and plans of
tests/_preprocess_cases.py (some with voxels zeroed so that the filled non-zero mask is off inside the crop box) with a blocky
label volume each, and one larger case of its own with dyadic zoom factors and a class of more than 10000 voxels.  The seeds of the
non-dyadic cases were chosen so that no output voxel is a near-tie (preprocessing.NEAR_TIE): label borders stay away from the
planes where a two-tap weight is 0.5."""
import numpy as np

from tests import _preprocess_cases as C

# own raw volumes, in the format of C.CASES
OWN = {
    "k_big_dyadic": ((1, 26, 44, 42), (1.0, 0.5, 1.0), (0, 1, 2), (0.5, 1.0, 1.0), ["CTNormalization"], [False],
                     ((1, 2, 1), (25, 42, 41)), False, 0, "3-D zoom by 2, 1/2 and 1: every tap weight is dyadic"),
}

LABELS4 = {"background": 0, "a": 1, "b": 2, "c": 3, "d": 4}

# tag: base (a tag of C.CASES or OWN), dataset labels, labels drawn as random boxes, seed, regions of the raw image set to zero
# (lo, hi), label boxes written after the random ones (label, lo, hi) in raw axes, what the case adds
CASES = {
    "a_sep_z_changes": dict(base="a_sep_z_changes", labels=LABELS4, present=(1, 2, 3), seed=0,
                            covers="separate z, the slice axis changes; class 4 of the dataset is absent: []"),
    "b_sep_z_same": dict(base="b_sep_z_same", labels=LABELS4, present=(1, 2, 3, 4), seed=0, covers="separate z, the slice axis stays"),
    "c_isotropic_3d": dict(base="c_isotropic_3d", labels=LABELS4, present=(1, 2, 3, 4), seed=1,
                           covers="full 3-D zoom: one axis down, one up, one unchanged"),
    "d_2d_config": dict(base="d_2d_config", labels=LABELS4, present=(1, 2, 3, 4), seed=0, covers="2-D configuration"),
    "e_transpose": dict(base="e_transpose", labels=LABELS4, present=(1, 2, 3, 4), seed=0, covers="transpose_forward (2, 0, 1)"),
    "f_border_box": dict(base="f_border_box", labels=LABELS4, present=(1, 4), seed=8,
                         boxes=((2, (1, 5, 7), (4, 8, 9)), (3, (13, 0, 0), (15, 3, 4))),
                         covers="label 2 inside the crop box where the filled mask is off (it stays), background there (-1), "
                                "label 3 outside the crop box (cropped away, so absent)"),
    "g_masked_zscore": dict(base="g_masked_zscore", labels=LABELS4, present=(1, 3), seed=32, zero=(((1, 6, 4), (4, 10, 8)),),
                            boxes=((2, (1, 6, 4), (4, 8, 8)),),
                            covers="masked ZScore: an open notch of zeros (mask off) partly labelled 2, which counts for the "
                                   "statistics, the rest of it -1, which does not"),
    "i_unchanged": dict(base="i_unchanged", labels={"background": 0, "a": 1, "big": 200}, present=(1,), seed=0,
                        boxes=((200, (2, 3, 4), (5, 6, 8)),), covers="unchanged shape; a label above 127: int16"),
    "l_ignore": dict(base="c_isotropic_3d", labels={"background": 0, "a": 1, "b": 2, "ignore": 3}, present=(1, 2, 3), seed=0,
                     covers="an ignore label: the tuple of all labels is one more class_locations key"),
    "k_big_dyadic": dict(base="k_big_dyadic", labels={"background": 0, "a": 1, "b": 2}, present=(2,), seed=0,
                         boxes=((1, (3, 4, 3), (22, 40, 38)), (2, (8, 10, 9), (13, 21, 20))),
                         covers="dyadic zoom factors (exact ties, exact sums); class 1 has more than 10000 voxels"),
}
FINGERPRINT_SAMPLES = 500


def _spec(tag):
    base = CASES[tag]["base"]
    return OWN[base] if base in OWN else C.CASES[base]


def _slices(lo, hi):
    return tuple(slice(a, b) for a, b in zip(lo, hi))


def image(tag):
    """(c, x, y, z) float32 raw volume of the case."""
    base = CASES[tag]["base"]
    if base in OWN:
        shape, _, _, _, _, _, (lo, hi), _, _, _ = OWN[base]
        rng = np.random.default_rng(26 + sum(map(ord, base)))
        ext = tuple(b - a for a, b in zip(lo, hi))
        coarse = rng.uniform(-1024, 3000, size=tuple((e + 3) // 4 for e in ext))
        v = np.repeat(np.repeat(np.repeat(coarse, 4, 0), 4, 1), 4, 2)[:ext[0], :ext[1], :ext[2]]
        v = np.round(v + rng.normal(0, 25, size=ext))
        v[v == 0] = 1
        img = np.zeros(shape, dtype=np.float32)
        img[0][_slices(lo, hi)] = v
    else:
        img = C.image(base)
    for lo, hi in CASES[tag].get("zero", ()):
        img[(slice(None),) + _slices(lo, hi)] = 0
    return img


def seg(tag):
    """(1, x, y, z) int16 raw label volume: two random boxes per label of `present` inside the image's non-zero box, then the
    case's fixed boxes."""
    case = CASES[tag]
    shape, _, _, _, _, _, (lo, hi), _, _, _ = _spec(tag)
    rng = np.random.default_rng(1000 * case["seed"] + sum(map(ord, tag)))
    out = np.zeros((1,) + tuple(shape[1:]), dtype=np.int16)
    for label in case["present"]:
        for _ in range(2):
            ext = [int(rng.integers(2, max(3, (b - a) // 2 + 1))) for a, b in zip(lo, hi)]
            at = [int(rng.integers(a, b - e + 1)) for a, b, e in zip(lo, hi, ext)]
            out[0][_slices(at, [a + e for a, e in zip(at, ext)])] = label
    for label, blo, bhi in case.get("boxes", ()):
        out[0][_slices(blo, bhi)] = label
    return out


def properties(tag):
    return {"spacing": list(_spec(tag)[1])}


def dataset_json(tag):
    shape = _spec(tag)[0]
    return {"labels": dict(CASES[tag]["labels"]), "channel_names": {str(c): f"ch{c}" for c in range(shape[0])}}


def plans(tag):
    base = CASES[tag]["base"]
    if base not in OWN:
        return C.plans(base)
    shape, _, tf, spacing, schemes, masks, _, _, order_z, _ = OWN[base]
    cfg = {"spacing": list(spacing), "normalization_schemes": list(schemes), "use_mask_for_norm": list(masks),
           "patch_size": [8, 8, 8], "preprocessor_name": "DefaultPreprocessor",
           "resampling_fn_data": "resample_data_or_seg_to_shape",
           "resampling_fn_data_kwargs": {"is_seg": False, "order": 3, "order_z": order_z, "force_separate_z": None},
           "resampling_fn_seg": "resample_data_or_seg_to_shape",
           "resampling_fn_seg_kwargs": {"is_seg": True, "order": 1, "order_z": 0, "force_separate_z": None}}
    return {"transpose_forward": list(tf), "transpose_backward": [int(np.argsort(tf)[i]) for i in range(3)],
            "configurations": {"3d_fullres": cfg},
            "foreground_intensity_properties_per_channel": {str(c): dict(C.FG) for c in range(shape[0])}}, "3d_fullres"


def is_dyadic(tag):
    return CASES[tag]["base"] == "k_big_dyadic"
