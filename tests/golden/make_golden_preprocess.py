"""Generate tests/golden/preprocess.npz from the REFERENCE's own preprocessing.

    MLAGG_REFERENCE=<reference checkout> python tests/golden/make_golden_preprocess.py

Calls nnunetv2.preprocessing.preprocessors.default_preprocessor.DefaultPreprocessor.run_case (:38-124) with seg_file=None for every
case of tests/_preprocess_cases.py, with the reference's own crop_to_nonzero, normalization classes and resample_data_or_seg_to_shape
(the planner's kwargs, default_experiment_planner.py:123-135), duck-typed plans / configuration managers and a reader that returns
the in-memory array.  It records the (do_separate_z, axis) each case passes to resample_data_or_seg for the data.  Third-party
modules that are absent offline are replaced by restatements: skimage.transform.resize (mode 'edge', no anti-aliasing, clip:
ndi.zoom(mode='nearest', grid_mode=True) clipped to the input's range, what skimage >= 0.19 computes), batchgenerators'
resize_segmentation, acvl_utils' get_bbox_from_mask / bounding_box_to_slice / ptqdm and the batchgenerators file helpers.  Only
the data is committed."""
import importlib
import json
import os
import sys
import types
from functools import partial

import numpy as np
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if "MLAGG_REFERENCE" not in os.environ:
    raise SystemExit("set MLAGG_REFERENCE to a checkout of the reference repository (aticejiang/MLAgg-UNet)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.environ["MLAGG_REFERENCE"], "mlagg"))

from tests import _preprocess_cases as C  # noqa: E402


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def resize(image, output_shape, order, mode="edge", anti_aliasing=False, clip=True):
    assert order in (0, 1, 3) and mode == "edge" and not anti_aliasing
    image = np.asarray(image, dtype=float)
    zoom = np.asarray(output_shape, dtype=float) / np.asarray(image.shape, dtype=float)
    out = ndi.zoom(image, zoom, order=order, mode="nearest", grid_mode=True)
    assert out.shape == tuple(output_shape)
    return np.clip(out, image.min(), image.max()) if clip else out


def resize_segmentation(segmentation, new_shape, order=3):
    tpe = segmentation.dtype
    if order == 0:
        return resize(segmentation.astype(float), new_shape, order).astype(tpe)
    reshaped = np.zeros(new_shape, dtype=tpe)
    for c in np.unique(segmentation):
        reshaped[resize((segmentation == c).astype(float), new_shape, order) >= 0.5] = c
    return reshaped


def get_bbox_from_mask(mask):
    box = []
    for a in range(mask.ndim):
        hit = np.flatnonzero(mask.any(axis=tuple(b for b in range(mask.ndim) if b != a)))
        box.append([int(hit[0]), int(hit[-1]) + 1])
    return box


def bounding_box_to_slice(bbox):
    return tuple(slice(*b) for b in bbox)


def load_json(file):
    with open(file) as f:
        return json.load(f)


def _stub_third_party():
    _mod("skimage")
    _mod("skimage.transform", resize=resize)
    _mod("acvl_utils")
    _mod("acvl_utils.miscellaneous")
    _mod("acvl_utils.miscellaneous.ptqdm", ptqdm=None)
    _mod("acvl_utils.cropping_and_padding")
    _mod("acvl_utils.cropping_and_padding.bounding_boxes", get_bbox_from_mask=get_bbox_from_mask, crop_to_bbox=None,
         bounding_box_to_slice=bounding_box_to_slice)
    _mod("batchgenerators")
    _mod("batchgenerators.augmentations")
    _mod("batchgenerators.augmentations.utils", resize_segmentation=resize_segmentation)
    _mod("batchgenerators.utilities")
    _mod("batchgenerators.utilities.file_and_folder_operations", load_json=load_json, isfile=os.path.isfile, join=os.path.join,
         isdir=os.path.isdir, subfiles=None, maybe_mkdir_p=None, subdirs=None, save_json=None, write_pickle=None, List=list)
    # run_case's module imports these for the dataset-level entry points and type hints only
    _mod("nnunetv2.utilities.plans_handling.plans_handler", PlansManager=object, ConfigurationManager=object)
    _mod("nnunetv2.utilities.dataset_name_id_conversion", maybe_convert_to_dataset_name=None)
    _mod("nnunetv2.utilities.utils", get_identifiers_from_splitted_dataset_folder=None,
         create_lists_from_splitted_dataset_folder=None)


class Reader:
    image = None
    props = None

    def read_images(self, files):
        return Reader.image.copy(), dict(Reader.props)


def main():
    _stub_third_party()
    R = importlib.import_module("nnunetv2.preprocessing.resampling.default_resampling")
    P = importlib.import_module("nnunetv2.preprocessing.preprocessors.default_preprocessor")
    decisions = []
    inner = R.resample_data_or_seg

    def recording(data, new_shape, is_seg=False, axis=None, order=3, do_separate_z=False, order_z=0):
        if not is_seg:
            decisions.append((bool(do_separate_z), -1 if axis is None or not do_separate_z else int(axis[0])))
        return inner(data, new_shape, is_seg, axis, order, do_separate_z, order_z=order_z)

    R.resample_data_or_seg = recording
    out = {}
    for tag in C.CASES:
        plans, name = C.plans(tag)
        cfg = plans["configurations"][name]
        kw = {k: v for k, v in cfg["resampling_fn_data_kwargs"].items()}
        skw = {k: v for k, v in cfg["resampling_fn_seg_kwargs"].items()}
        cm = types.SimpleNamespace(spacing=list(cfg["spacing"]), normalization_schemes=cfg["normalization_schemes"],
                                   use_mask_for_norm=cfg["use_mask_for_norm"],
                                   resampling_fn_data=partial(R.resample_data_or_seg_to_shape, **kw),
                                   resampling_fn_seg=partial(R.resample_data_or_seg_to_shape, **skw))
        pm = types.SimpleNamespace(image_reader_writer_class=Reader, transpose_forward=plans["transpose_forward"],
                                   foreground_intensity_properties_per_channel=plans["foreground_intensity_properties_per_channel"])
        Reader.image, Reader.props = C.image(tag), C.properties(tag)
        decisions.clear()
        data, seg, props = P.DefaultPreprocessor(verbose=False).run_case(["in-memory"], None, pm, cm, {"labels": {"background": 0}})
        assert data.dtype == np.float32
        out[f"{tag}/image"] = C.image(tag)
        out[f"{tag}/data"] = data
        out[f"{tag}/bbox"] = np.asarray(props["bbox_used_for_cropping"], dtype=np.int64)
        out[f"{tag}/shape_before_cropping"] = np.asarray(props["shape_before_cropping"], dtype=np.int64)
        out[f"{tag}/shape_after_cropping"] = np.asarray(props["shape_after_cropping_and_before_resampling"], dtype=np.int64)
        out[f"{tag}/separate_z"] = np.asarray(decisions[0], dtype=np.int64)
    for k, v in out.items():
        if v.dtype == np.float64:
            raise SystemExit(f"{k}: unexpected float64")
    np.savez_compressed(os.path.join(HERE, "preprocess.npz"), **out)
    print("preprocess", {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
