"""Generate tests/golden/preprocess_train.npz from the REFERENCE's own training-case preprocessing and fingerprint extraction.

    MLAGG_REFERENCE=<reference checkout> python tests/golden/make_golden_preprocess_train.py

For every case of tests/_preprocess_train_cases.py: nnunetv2's DefaultPreprocessor.run_case (default_preprocessor.py:38-124) with a
seg_file (crop_to_nonzero with a segmentation, the normalization classes, resample_data_or_seg_to_shape for data and
segmentation with the planner's kwargs, _sample_foreground_locations), and DatasetFingerprintExtractor.analyze_case /
collect_foreground_intensities (fingerprint_extractor.py:39-103), with the reference's own LabelManager (it imports under the
stand-ins).  The stand-ins for the third-party modules that are absent offline are those of make_golden_preprocess.py, imported
from it; the plans / configuration managers are duck-typed and the reader returns the in-memory arrays.  The raw inputs are
regenerable from the seeds and not stored.  Stored per case: data, seg, the geometry entries, class_locations (keys, counts and
int16 coordinates), the fingerprint samples, and the number of near-tie voxels of the segmentation resampling (the voxels where
some label's fp64 indicator is within preprocessing.NEAR_TIE of 0.5, evaluated by this package's host path on the segmentation
the reference's resampler received).  Only data is committed."""
import importlib
import os
import sys
import types
from functools import partial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden_preprocess as G  # noqa: E402  (checks MLAGG_REFERENCE, extends sys.path, holds the stand-ins)

from tests import _preprocess_train_cases as T  # noqa: E402


class Reader:
    image = None
    seg = None
    props = None

    def read_images(self, files):
        return Reader.image.copy(), dict(Reader.props)

    def read_seg(self, file):
        return Reader.seg.copy(), dict(Reader.props)


def main():
    G._stub_third_party()
    G._mod("nnunetv2.imageio")
    G._mod("nnunetv2.imageio.base_reader_writer", BaseReaderWriter=object)
    G._mod("nnunetv2.imageio.reader_writer_registry", determine_reader_writer_from_dataset_json=None)
    sys.modules["batchgenerators.utilities.file_and_folder_operations"].__dict__.update(save_json=None, maybe_mkdir_p=None)
    R = importlib.import_module("nnunetv2.preprocessing.resampling.default_resampling")
    P = importlib.import_module("nnunetv2.preprocessing.preprocessors.default_preprocessor")
    F = importlib.import_module("nnunetv2.experiment_planning.dataset_fingerprint.fingerprint_extractor")
    L = importlib.import_module("nnunetv2.utilities.label_handling.label_handling")
    import mlagg_unet_amd  # noqa: F401
    from mlagg_unet_amd import preprocessing as ours
    from mlagg_unet_amd.export import separate_z_decision

    out = {}
    for tag in T.CASES:
        plans, name = T.plans(tag)
        cfg = plans["configurations"][name]
        dj = T.dataset_json(tag)
        seen = {}

        def seg_resampler(seg, new_shape, current_spacing, new_spacing, **kw):
            seen["seg"], seen["new_shape"] = seg.copy(), tuple(int(s) for s in new_shape)
            seen["spacings"] = (list(current_spacing), list(new_spacing))
            return R.resample_data_or_seg_to_shape(seg, new_shape, current_spacing, new_spacing, **kw)

        cm = types.SimpleNamespace(spacing=list(cfg["spacing"]), normalization_schemes=cfg["normalization_schemes"],
                                   use_mask_for_norm=cfg["use_mask_for_norm"],
                                   resampling_fn_data=partial(R.resample_data_or_seg_to_shape, **cfg["resampling_fn_data_kwargs"]),
                                   resampling_fn_seg=partial(seg_resampler, **cfg["resampling_fn_seg_kwargs"]))
        pm = types.SimpleNamespace(image_reader_writer_class=Reader, transpose_forward=plans["transpose_forward"],
                                   foreground_intensity_properties_per_channel=plans["foreground_intensity_properties_per_channel"],
                                   get_label_manager=lambda d: L.LabelManager(d["labels"], d.get("regions_class_order")))
        Reader.image, Reader.seg, Reader.props = T.image(tag), T.seg(tag), T.properties(tag)
        data, seg, props = P.DefaultPreprocessor(verbose=False).run_case(["in-memory"], "in-memory", pm, cm, dj)
        assert data.dtype == np.float32 and seg.dtype in (np.int8, np.int16)
        out[f"{tag}/data"] = data
        out[f"{tag}/seg"] = seg
        out[f"{tag}/bbox"] = np.asarray(props["bbox_used_for_cropping"], dtype=np.int64)
        out[f"{tag}/shape_before_cropping"] = np.asarray(props["shape_before_cropping"], dtype=np.int64)
        out[f"{tag}/shape_after_cropping"] = np.asarray(props["shape_after_cropping_and_before_resampling"], dtype=np.int64)
        keys, counts, coords = [], [], []
        for k, v in props["class_locations"].items():
            key = [int(i) for i in k] if isinstance(k, tuple) else [int(k)]
            keys.append(key + [-2] * (8 - len(key)))                    # a row per key, padded; a tuple key has more than one label
            counts.append(len(v))
            if len(v):
                assert v.dtype == np.int64 and v.shape[1] == 4 and v.max() < 32768
                coords.append(v.astype(np.int16))
        out[f"{tag}/loc_keys"] = np.asarray(keys, dtype=np.int16).reshape(-1, 8)
        out[f"{tag}/loc_is_tuple"] = np.asarray([isinstance(k, tuple) for k in props["class_locations"]], dtype=bool)
        out[f"{tag}/loc_counts"] = np.asarray(counts, dtype=np.int64)
        out[f"{tag}/loc_coords"] = np.concatenate(coords) if coords else np.zeros((0, 4), dtype=np.int16)
        near = 0
        if seen["seg"].shape[1:] != seen["new_shape"]:
            sep, axis = separate_z_decision(*seen["spacings"], cfg["resampling_fn_seg_kwargs"]["force_separate_z"])
            again, mask = ours._resample_seg_host(seen["seg"], seen["new_shape"], sep, axis, near_tie=True)
            assert np.array_equal(again.astype(seg.dtype), seg)
            near = int(mask.sum())
        out[f"{tag}/near_tie"] = np.asarray(near, dtype=np.int64)
        # fingerprint: the reference's analyze_case on the raw arrays
        shape_after, spacing, samples, _, rel = F.DatasetFingerprintExtractor.analyze_case(["in-memory"], "in-memory", Reader,
                                                                                         num_samples=T.FINGERPRINT_SAMPLES)
        out[f"{tag}/fp_shape_after_crop"] = np.asarray(shape_after, dtype=np.int64)
        out[f"{tag}/fp_samples"] = np.stack([np.asarray(s, dtype=np.float32) for s in samples])
        out[f"{tag}/fp_relative_size"] = np.asarray(rel, dtype=np.float64)
        print(tag, data.shape, seg.dtype, "near-tie", near, "of", seg.size, "locations", dict(zip(map(tuple, keys), counts)))
    np.savez_compressed(os.path.join(HERE, "preprocess_train.npz"), **out)
    print("preprocess_train.npz", os.path.getsize(os.path.join(HERE, "preprocess_train.npz")), "bytes")


if __name__ == "__main__":
    main()
