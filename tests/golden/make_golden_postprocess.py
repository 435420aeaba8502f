"""Generate tests/golden/postprocess.npz from the REFERENCE's own postprocessing by connected components.

    MLAGG_REFERENCE=<reference checkout> python tests/golden/make_golden_postprocess.py

Calls nnunetv2.postprocessing.remove_connected_components' remove_all_but_largest_component_from_segmentation (:22-34) for every call of
tests/_postprocess_cases.py (and, per label in order, for the per-class chains), and determine_postprocessing (:51-246) followed by
apply_postprocessing (:37-40) for every cross-validation set, on .npy files in a temporary folder; the postprocessing.json it writes
is stored as text.  The reference's evaluate_predictions.compute_metrics_on_folder computes every Dice it decides on.
Modules that are absent offline are replaced:
  - acvl_utils' remove_all_but_largest_component is RESTATED, not run: scipy.ndimage.label with the full 3^ndim structure (what
    skimage.measure.label(connectivity=None) uses), np.bincount, every component whose size equals the maximum is kept;
  - batchgenerators' file helpers, an .npy reader-writer behind a duck-typed PlansManager and label manager;
  - a serial stand-in for multiprocessing.get_context("spawn").Pool in both modules, because spawn children would not see the stubs.
Only the data is committed."""
import importlib
import json
import os
import pickle
import shutil
import sys
import tempfile
import types

import numpy as np
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if "MLAGG_REFERENCE" not in os.environ:
    raise SystemExit("set MLAGG_REFERENCE to a checkout of the reference repository (aticejiang/MLAgg-UNet)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.environ["MLAGG_REFERENCE"], "mlagg"))

from tests import _postprocess_cases as C  # noqa: E402


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def remove_all_but_largest_component(binary_image, connectivity=None):
    assert connectivity is None
    labeled, n = ndi.label(binary_image, structure=np.ones((3,) * binary_image.ndim))
    sizes = np.bincount(labeled.ravel())[1:]
    keep = [i + 1 for i, s in enumerate(sizes) if s == max(sizes)]
    return np.isin(labeled, keep)


def subfiles(folder, join=True, prefix=None, suffix=None, sort=True):
    names = [f for f in os.listdir(folder) if os.path.isfile(os.path.join(folder, f))
             and (prefix is None or f.startswith(prefix)) and (suffix is None or f.endswith(suffix))]
    if sort:
        names.sort()
    return [os.path.join(folder, f) for f in names] if join else names


def load_json(file):
    with open(file) as f:
        return json.load(f)


def save_json(obj, file, indent=4, sort_keys=True):
    with open(file, "w") as f:
        json.dump(obj, f, sort_keys=sort_keys, indent=indent)


def save_pickle(obj, file, mode="wb"):
    with open(file, mode) as f:
        pickle.dump(obj, f)


def load_pickle(file, mode="rb"):
    with open(file, mode) as f:
        return pickle.load(f)


class SerialPool:
    def __init__(self, *args, **kwargs):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def starmap(self, fn, iterable):
        return [fn(*args) for args in iterable]


SERIAL = types.SimpleNamespace(get_context=lambda method=None: types.SimpleNamespace(Pool=SerialPool))


class NpyIO:
    """read_seg / write_seg of (1, X, Y, Z) label arrays in .npy files"""

    def read_seg(self, fname):
        return np.load(fname)[None], {}

    def write_seg(self, seg, fname, properties):
        np.save(fname, np.asarray(seg))


class PlansManager:
    label_manager = None

    def __init__(self, plans):
        pass

    def image_reader_writer_class(self):
        return NpyIO()

    def get_label_manager(self, dataset_json):
        return PlansManager.label_manager


def _stub_third_party():
    _mod("acvl_utils")
    _mod("acvl_utils.morphology")
    _mod("acvl_utils.morphology.morphology_helper", remove_all_but_largest_component=remove_all_but_largest_component)
    _mod("batchgenerators")
    _mod("batchgenerators.utilities")
    _mod("batchgenerators.utilities.file_and_folder_operations", load_json=load_json, subfiles=subfiles, join=os.path.join,
         isfile=os.path.isfile, isdir=os.path.isdir, save_pickle=save_pickle, load_pickle=load_pickle, save_json=save_json,
         maybe_mkdir_p=lambda d: os.makedirs(d, exist_ok=True))
    _mod("nnunetv2.configuration", default_num_processes=1)
    _mod("nnunetv2.paths", nnUNet_raw=None, nnUNet_results=None, nnUNet_preprocessed=None)
    _mod("nnunetv2.evaluation.accumulate_cv_results", accumulate_cv_results=None)
    _mod("nnunetv2.imageio.reader_writer_registry", determine_reader_writer_from_dataset_json=None,
         determine_reader_writer_from_file_ending=None)
    _mod("nnunetv2.imageio.simpleitk_reader_writer", SimpleITKIO=object)
    _mod("nnunetv2.utilities.file_path_utilities", folds_tuple_to_string=None)
    _mod("nnunetv2.utilities.plans_handling.plans_handler", PlansManager=PlansManager)


def main():
    _stub_third_party()
    E = importlib.import_module("nnunetv2.evaluation.evaluate_predictions")
    R = importlib.import_module("nnunetv2.postprocessing.remove_connected_components")
    E.multiprocessing = SERIAL
    R.multiprocessing = SERIAL
    out = {}
    for tag, make in C.VOLUMES.items():
        v = make()
        out[f"{tag}/input"] = v
        labels = [int(i) for i in np.unique(v) if i != 0]
        chain = v
        for label in labels:                                       # the per-class mode: one label after the other
            chain = R.remove_all_but_largest_component_from_segmentation(chain, label)
        out[f"{tag}/per_class"] = chain
        out[f"{tag}/per_class_labels"] = np.asarray(labels, np.int64)
    for tag, (vol, lr, bg, _) in C.CALLS.items():
        v = out[f"{vol}/input"]
        got = R.remove_all_but_largest_component_from_segmentation(v, lr, bg)
        assert np.array_equal(v, C.VOLUMES[vol]())                 # the input is untouched
        out[f"{tag}/output"] = got
    with tempfile.TemporaryDirectory() as tmp:
        for tag in C.CV_SETS:
            preds, refs, labels, ignore = C.cv_set(tag)
            pdir, rdir = os.path.join(tmp, tag, "pred"), os.path.join(tmp, tag, "ref")
            os.makedirs(pdir)
            os.makedirs(rdir)
            for i, (p, r) in enumerate(zip(preds, refs)):
                np.save(os.path.join(pdir, f"case_{i:03d}.npy"), p)
                np.save(os.path.join(rdir, f"case_{i:03d}.npy"), r)
                out[f"cv/{tag}/pred_{i}"] = p
                out[f"cv/{tag}/ref_{i}"] = r
            PlansManager.label_manager = types.SimpleNamespace(has_regions=False, foreground_labels=list(labels),
                                                               foreground_regions=None, ignore_label=ignore)
            fns, kwargs = R.determine_postprocessing(pdir, rdir, {}, {"file_ending": ".npy"}, 1, keep_postprocessed_files=False)
            with open(os.path.join(pdir, "postprocessing.json")) as f:
                out[f"cv/{tag}/postprocessing_json"] = np.asarray(f.read())
            for i, p in enumerate(preds):
                out[f"cv/{tag}/pp_{i}"] = R.apply_postprocessing(p, fns, kwargs)
            out[f"cv/{tag}/labels"] = np.asarray(labels, np.int64)
            out[f"cv/{tag}/ignore"] = np.asarray(-1 if ignore is None else ignore, np.int64)
            print(tag, [f.__name__ for f in fns], kwargs)
            shutil.rmtree(os.path.join(tmp, tag))
    np.savez_compressed(os.path.join(HERE, "postprocess.npz"), **out)
    print("postprocess", len(out), "arrays")


if __name__ == "__main__":
    main()
