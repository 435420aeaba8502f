"""The seeded cases of tests/golden/export.npz (made by tests/golden/make_golden_export.py with the reference's own
export_prediction_from_softmax and resample_data_or_seg_to_shape): one per branch of the probability resampler, K in {2, 4, 14},
off-centre boxes and non-identity transpose_backward."""
import numpy as np

# tag: (K, logits shape (preprocessed), configuration spacing, properties spacing, shape_before_cropping, bbox lower corner,
#       shape_after_cropping_and_before_resampling, transpose_backward, what it covers)
CASES = {
    "a_isotropic": (4, (10, 12, 8), (1.5, 1.5, 1.5), (1.0, 2.0, 1.5), (20, 10, 9), (3, 2, 1), (15, 6, 8), (0, 1, 2),
                    "trilinear: one axis up, one down, one unchanged"),
    "b_separate_z": (14, (6, 12, 11), (3.0, 0.8, 0.8), (2.2, 0.6, 0.6), (10, 18, 16), (1, 1, 2), (8, 16, 14), (2, 0, 1),
                     "anisotropic current spacing, separate z, the low-resolution axis changes size"),
    "c_separate_z_same": (2, (12, 6, 15), (0.7, 4.0, 0.7), (0.5, 4.0, 1.0), (17, 6, 11), (0, 0, 0), (17, 6, 11), (0, 1, 2),
                          "separate z along axis 1, which keeps its size"),
    "d_2d_config": (14, (5, 11, 13), (0.8, 0.8), (5.0, 0.7, 0.7), (6, 14, 17), (1, 0, 2), (5, 13, 15), (0, 2, 1),
                    "2-D configuration: current spacing (spacing[0], *configuration spacing)"),
    "e_new_spacing": (4, (11, 13, 18), (1.0, 1.0, 1.0), (1.0, 1.0, 3.5), (15, 13, 6), (2, 0, 1), (12, 13, 5), (0, 1, 2),
                      "anisotropy only in the new spacing (axis 2, order 0)"),
    "f_two_lowres": (2, (20, 5, 6), (0.24, 1.25, 1.25), (0.3, 0.9, 1.6), (15, 7, 5), (0, 0, 0), (15, 7, 5), (0, 1, 2),
                     "two-axis low-resolution spacing: no separate z"),
    "g_unchanged": (4, (8, 9, 10), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (11, 9, 13), (2, 0, 3), (8, 9, 10), (1, 2, 0),
                    "no resampling"),
}
# resample_data_or_seg_to_shape(is_seg=False, order=1, order_z=1) called directly: (K, in shape, new shape, current, new spacing)
ORDER_Z1 = (4, (6, 12, 11), (8, 16, 14), (3.0, 0.8, 0.8), (2.2, 0.6, 0.6))


def logits(tag, seed=7):
    K, shape = CASES[tag][0], CASES[tag][1]
    rng = np.random.default_rng(seed + sum(map(ord, tag)))
    return (rng.standard_normal((K,) + shape) * 2.0).astype(np.float32)


def order_z1_logits(seed=11):
    K, shape = ORDER_Z1[0], ORDER_Z1[1]
    return (np.random.default_rng(seed).standard_normal((K,) + shape) * 2.0).astype(np.float32)


def properties(tag):
    _, _, _, spacing, full, lo, crop, _, _ = CASES[tag]
    return {"spacing": list(spacing), "shape_before_cropping": tuple(full),
            "bbox_used_for_cropping": [[a, a + c] for a, c in zip(lo, crop)],
            "shape_after_cropping_and_before_resampling": tuple(crop)}


def dataset_json(K):
    labels = {"background": 0}
    labels.update({f"class_{k}": k for k in range(1, K)})
    return {"labels": labels, "file_ending": ".nii.gz"}
