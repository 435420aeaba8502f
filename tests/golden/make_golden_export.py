"""Generate tests/golden/export.npz from the REFERENCE's own prediction export.

    MLAGG_REFERENCE=<reference checkout> python tests/golden/make_golden_export.py

Calls nnunetv2.inference.export_prediction.export_prediction_from_softmax (:10-69) with save_probabilities=True for every case of
tests/_export_cases.py, with the reference's own resample_data_or_seg_to_shape (preprocessing/resampling/default_resampling.py:76-200,
the default kwargs of default_experiment_planner.py:138-154) and LabelManager, duck-typed plans / configuration managers and a writer
that captures the segmentation; the probabilities are read back from the .npz it writes into a temporary folder.  It also records the
(do_separate_z, axis) each case passes to resample_data_or_seg, and one direct call of the resampler with order_z=1.
Third-party modules that are absent offline are replaced by restatements: skimage.transform.resize (order 1, mode 'edge', no
anti-aliasing: ndi.zoom(mode='nearest', grid_mode=True), what skimage >= 0.19 calls), acvl_utils' bounding_box_to_slice and the
batchgenerators helpers the imported modules use.  Only the data is committed."""
import importlib
import json
import os
import pickle
import sys
import tempfile
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

from tests import _export_cases as C  # noqa: E402


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def resize(image, output_shape, order, mode, anti_aliasing):
    assert order == 1 and mode == "edge" and not anti_aliasing
    zoom = np.asarray(output_shape, dtype=float) / np.asarray(image.shape, dtype=float)
    out = ndi.zoom(image, zoom, order=1, mode="nearest", grid_mode=True)
    assert out.shape == tuple(output_shape)
    return out


def bounding_box_to_slice(bbox):
    return tuple(slice(*b) for b in bbox)


def save_pickle(obj, file, mode="wb"):
    with open(file, mode) as f:
        pickle.dump(obj, f)


def load_json(file):
    with open(file) as f:
        return json.load(f)


def _stub_third_party():
    _mod("skimage")
    _mod("skimage.transform", resize=resize)
    _mod("acvl_utils")
    _mod("acvl_utils.cropping_and_padding")
    _mod("acvl_utils.cropping_and_padding.bounding_boxes", bounding_box_to_slice=bounding_box_to_slice)
    _mod("batchgenerators")
    _mod("batchgenerators.augmentations")
    _mod("batchgenerators.augmentations.utils", resize_segmentation=None)
    _mod("batchgenerators.utilities")
    _mod("batchgenerators.utilities.file_and_folder_operations", load_json=load_json, isfile=os.path.isfile,
         save_pickle=save_pickle, join=os.path.join, isdir=os.path.isdir, subfiles=None, maybe_mkdir_p=None, subdirs=None)
    # export_prediction imports these two names for type hints only; the real module pulls in the network and image-io packages
    _mod("nnunetv2.utilities.plans_handling.plans_handler", PlansManager=object, ConfigurationManager=object)


class Writer:
    written = None

    def write_seg(self, seg, output_fname, properties):
        Writer.written = np.array(seg)


def main():
    _stub_third_party()
    R = importlib.import_module("nnunetv2.preprocessing.resampling.default_resampling")
    X = importlib.import_module("nnunetv2.inference.export_prediction")
    L = importlib.import_module("nnunetv2.utilities.label_handling.label_handling")
    decisions = []
    inner = R.resample_data_or_seg

    def recording(data, new_shape, is_seg=False, axis=None, order=3, do_separate_z=False, order_z=0):
        decisions.append((bool(do_separate_z), -1 if axis is None or not do_separate_z else int(axis[0])))
        return inner(data, new_shape, is_seg, axis, order, do_separate_z, order_z=order_z)

    R.resample_data_or_seg = recording
    fn = partial(R.resample_data_or_seg_to_shape, is_seg=False, order=1, order_z=0, force_separate_z=None)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, (K, _, cfg_spacing, _, _, _, _, tb, _) in C.CASES.items():
            logits = C.logits(tag)
            props = C.properties(tag)
            dj = C.dataset_json(K)
            cfg = types.SimpleNamespace(spacing=list(cfg_spacing), resampling_fn_probabilities=fn)
            plans = types.SimpleNamespace(transpose_backward=list(tb), image_reader_writer_class=Writer,
                                          get_label_manager=lambda d: L.LabelManager(d["labels"], regions_class_order=None))
            decisions.clear()
            trunc = os.path.join(tmp, tag)
            X.export_prediction_from_softmax(logits.copy(), props, cfg, plans, dj, trunc, save_probabilities=True)
            out[f"{tag}/logits"] = logits
            out[f"{tag}/segmentation"] = Writer.written
            out[f"{tag}/probabilities"] = np.load(trunc + ".npz")["probabilities"]
            assert len(decisions) == 1                          # labels and probabilities share one resampling
            out[f"{tag}/separate_z"] = np.asarray(decisions[0])
            with open(trunc + ".pkl", "rb") as f:
                assert pickle.load(f) == props
    K, shape, new_shape, cur, new = C.ORDER_Z1
    x = C.order_z1_logits()
    out["order_z1/logits"] = x
    out["order_z1/resampled"] = R.resample_data_or_seg_to_shape(x.copy(), new_shape, cur, new, is_seg=False, order=1, order_z=1,
                                                               force_separate_z=None)
    for k, v in out.items():
        if v.dtype == np.float64:
            raise SystemExit(f"{k}: unexpected float64")
    np.savez_compressed(os.path.join(HERE, "export.npz"), **out)
    print("export", {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
