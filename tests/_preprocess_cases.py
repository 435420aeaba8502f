"""The seeded cases of tests/golden/preprocess.npz (made by tests/golden/make_golden_preprocess.py with the reference's own
DefaultPreprocessor.run_case): small raw volumes with a CT-like range and sharp edges, one per branch of the preprocessing --
separate z with the low-resolution axis changing size or not, a full 3-D zoom, a 2-D configuration, a non-identity
transpose_forward, off-centre boxes with non-zero voxels on the array border, a masked ZScore channel with an enclosed hole,
NoNormalization / RescaleTo01 / RGBTo01 / ZScore channels, an unchanged shape and order_z = 1."""
import numpy as np

FG = {"mean": 120.7, "std": 410.3, "percentile_00_5": -900.5, "percentile_99_5": 2500.25, "median": 80.0, "min": -1024.0,
      "max": 3000.0}

# tag: (raw shape (c, x, y, z), raw spacing, transpose_forward, configuration spacing, normalization schemes, use_mask_for_norm,
#       non-zero box (lo, hi) in raw axes, border voxels, order_z, what it covers)
CASES = {
    "a_sep_z_changes": ((1, 10, 24, 20), (3.0, 0.8, 0.8), (0, 1, 2), (2.0, 0.7, 0.7), ["CTNormalization"], [False],
                        ((1, 2, 3), (9, 22, 18)), False, 0, "separate z along axis 0, which changes size"),
    "b_sep_z_same": ((1, 21, 6, 17), (0.8, 4.0, 0.8), (0, 1, 2), (0.7, 4.0, 0.9), ["CTNormalization"], [False],
                     ((2, 0, 1), (19, 6, 15)), False, 0, "separate z along axis 1, which keeps its size"),
    "c_isotropic_3d": ((1, 18, 11, 13), (1.0, 2.0, 1.5), (0, 1, 2), (1.5, 1.5, 1.5), ["CTNormalization"], [False],
                       ((1, 1, 1), (17, 10, 12)), False, 0, "full 3-D zoom: one axis down, one up, one unchanged"),
    "d_2d_config": ((1, 7, 26, 23), (2.5, 0.76, 0.76), (0, 1, 2), (0.79, 0.79), ["CTNormalization"], [False],
                    ((1, 3, 2), (6, 24, 22)), False, 0, "2-D configuration: the slice axis keeps its spacing"),
    "e_transpose": ((1, 20, 16, 8), (0.8, 0.8, 3.2), (2, 0, 1), (2.5, 0.9, 0.9), ["CTNormalization"], [False],
                    ((3, 1, 1), (18, 15, 7)), False, 0, "transpose_forward (2, 0, 1): the low-resolution axis moves first"),
    "f_border_box": ((1, 15, 12, 14), (1.2, 1.0, 1.1), (1, 0, 2), (1.0, 1.0, 1.0), ["CTNormalization"], [False],
                     ((5, 4, 6), (12, 10, 11)), True, 0, "off-centre box widened to the array border by single voxels"),
    "g_masked_zscore": ((2, 14, 16, 12), (1.0, 1.0, 1.0), (0, 1, 2), (1.3, 0.8, 1.0),
                        ["CTNormalization", "ZScoreNormalization"], [False, True], ((1, 1, 1), (13, 15, 11)), False, 0,
                        "CT + masked ZScore with a zero-valued enclosed hole that filling puts into the mask"),
    "h_other_schemes": ((3, 12, 13, 10), (1.0, 1.0, 1.0), (0, 1, 2), (0.9, 1.2, 1.0),
                        ["NoNormalization", "RescaleTo01Normalization", "RGBTo01Normalization"], [False, False, False],
                        ((0, 1, 1), (11, 12, 9)), False, 0, "NoNormalization, RescaleTo01, RGBTo01"),
    "i_unchanged": ((1, 9, 10, 11), (1.0, 1.0, 1.0), (0, 1, 2), (1.0, 1.0, 1.0), ["ZScoreNormalization"], [False],
                    ((1, 2, 3), (8, 9, 10)), False, 0, "unchanged shape (no resampling), unmasked ZScore"),
    "j_order_z1": ((1, 10, 24, 20), (3.0, 0.8, 0.8), (0, 1, 2), (2.0, 0.7, 0.7), ["CTNormalization"], [False],
                   ((1, 2, 3), (9, 22, 18)), False, 1, "separate z with order_z = 1"),
}
HOLE = ((5, 6, 4), (8, 10, 7))       # g_masked_zscore: zero in every channel, enclosed by non-zero voxels


def image(tag, seed=22):
    """(c, x, y, z) float32: blocky levels in [-1024, 3000] inside the box (sharp edges, so the clips fire), zeros outside."""
    shape, _, _, _, schemes, _, (lo, hi), border, _, _ = CASES[tag]
    rng = np.random.default_rng(seed + sum(map(ord, tag)))
    img = np.zeros(shape, dtype=np.float32)
    ext = tuple(b - a for a, b in zip(lo, hi))
    for c, s in enumerate(schemes):
        coarse = rng.uniform(-1024, 3000, size=tuple((e + 2) // 3 for e in ext))
        v = np.repeat(np.repeat(np.repeat(coarse, 3, 0), 3, 1), 3, 2)[:ext[0], :ext[1], :ext[2]]
        v = np.round(v + rng.normal(0, 25, size=ext))
        if s == "RGBTo01Normalization":
            v = np.clip(np.round((v + 1024) / 4024 * 255), 1, 255)
        v[v == 0] = 1
        img[c][tuple(slice(a, b) for a, b in zip(lo, hi))] = v
    if border:
        img[0, 0, lo[1] + 1, lo[2] + 2] = 300.0
        img[0, lo[0] + 1, shape[2] - 1, lo[2] + 1] = -500.0
        img[0, lo[0] + 2, lo[1] + 1, shape[3] - 1] = 2800.0
    if tag == "g_masked_zscore":
        img[(slice(None),) + tuple(slice(a, b) for a, b in zip(*HOLE))] = 0
    return img


def properties(tag):
    return {"spacing": list(CASES[tag][1])}


def plans(tag):
    shape, _, tf, spacing, schemes, masks, _, _, order_z, _ = CASES[tag]
    name = "2d" if len(spacing) == 2 else "3d_fullres"
    cfg = {"spacing": list(spacing), "normalization_schemes": list(schemes), "use_mask_for_norm": list(masks),
           "patch_size": [16, 16] if len(spacing) == 2 else [8, 8, 8], "preprocessor_name": "DefaultPreprocessor",
           "resampling_fn_data": "resample_data_or_seg_to_shape",
           "resampling_fn_data_kwargs": {"is_seg": False, "order": 3, "order_z": order_z, "force_separate_z": None},
           "resampling_fn_seg": "resample_data_or_seg_to_shape",
           "resampling_fn_seg_kwargs": {"is_seg": True, "order": 1, "order_z": 0, "force_separate_z": None}}
    tb = [int(np.argsort(tf)[i]) for i in range(3)]
    return {"transpose_forward": list(tf), "transpose_backward": tb, "configurations": {name: cfg},
            "foreground_intensity_properties_per_channel": {str(c): dict(FG) for c in range(shape[0])}}, name
