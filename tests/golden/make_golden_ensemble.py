"""Generate tests/golden/ensemble.npz from the REFERENCE's own ensembling and evaluation code.

    MLAGG_REFERENCE=<reference checkout> python tests/golden/make_golden_ensemble.py

For the cases of tests/_ensemble_cases.py it calls, on files in a temporary folder:
  - nnunetv2.ensembling.ensemble.average_probabilities (:17-29) and merge_files (:32-46) with the reference's real LabelManager
    (utilities/label_handling/label_handling.py) for every set of ensemble members;
  - nnunetv2.evaluation.evaluate_predictions.compute_metrics (:89-120) for every metric case and compute_metrics_on_folder (:123-175)
    for every folder set, whose summary.json is stored as text;
  - merge_files + compute_metrics_on_folder per candidate and per pair of the model-selection constructions, named by
    utilities/file_path_utilities.get_ensemble_name.
Modules that are absent offline are replaced: batchgenerators' file helpers, acvl_utils' bounding_box_to_slice (unused here), the
configuration and paths modules, a duck-typed PlansManager, an .npy reader-writer, and a serial stand-in for
multiprocessing.get_context("spawn").Pool, because spawn children would not see the stubs.

Two conditions on the ensemble inputs are asserted here, for every voxel of every case: the two largest means are exactly equal or at
least 1e-3 apart, and the reference's label, argmax(softmax(mean)), equals argmax(mean).  Under that margin the second softmax cannot
merge two distinct means (a relative gap of exp(1e-3) is four orders above fp32 rounding, and equal inputs give equal outputs), so the
package's rule -- the argmax of the mean -- has the reference's labels as its expected values on every voxel.
Only the data is committed."""
import importlib
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if "MLAGG_REFERENCE" not in os.environ:
    raise SystemExit("set MLAGG_REFERENCE to a checkout of the reference repository (aticejiang/MLAgg-UNet)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.environ["MLAGG_REFERENCE"], "mlagg"))

from tests import _ensemble_cases as C  # noqa: E402


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


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
    """read_seg / write_seg of label arrays in .npy files"""

    def read_seg(self, fname):
        return np.load(fname)[None], {}

    def write_seg(self, seg, fname, properties):
        np.save(fname, np.asarray(seg))


def _stub_third_party():
    _mod("acvl_utils")
    _mod("acvl_utils.cropping_and_padding")
    _mod("acvl_utils.cropping_and_padding.bounding_boxes", bounding_box_to_slice=None)
    _mod("batchgenerators")
    _mod("batchgenerators.utilities")
    import typing
    # the real module is star-imported for its file helpers and, in passing, for os and typing's List / Tuple / Union
    _mod("batchgenerators.utilities.file_and_folder_operations", os=os, List=typing.List, Tuple=typing.Tuple, Union=typing.Union,
         load_json=load_json, subfiles=subfiles, join=os.path.join,
         isfile=os.path.isfile, isdir=os.path.isdir, save_pickle=save_pickle, load_pickle=load_pickle, save_json=save_json,
         maybe_mkdir_p=lambda d: os.makedirs(d, exist_ok=True))
    _mod("nnunetv2.configuration", default_num_processes=1)
    _mod("nnunetv2.paths", nnUNet_raw=None, nnUNet_results=None, nnUNet_preprocessed=None)
    _mod("nnunetv2.imageio.reader_writer_registry", determine_reader_writer_from_dataset_json=None,
         determine_reader_writer_from_file_ending=None)
    _mod("nnunetv2.imageio.simpleitk_reader_writer", SimpleITKIO=object)
    _mod("nnunetv2.utilities.plans_handling.plans_handler", PlansManager=object)


def _label_manager(L, K):
    return L.LabelManager({"background": 0, **{f"class_{i}": i for i in range(1, K)}}, None)


def _jsonable(J, metrics):
    """compute_metrics' 'metrics' dict as the text its JSON export gives (keys through label_or_region_to_key)."""
    m = {k: dict(v) for k, v in metrics.items()}
    J.recursive_fix_for_json_export(m)
    return json.dumps({str(k): v for k, v in m.items()}, sort_keys=True)


def _write_members(folder, name, members):
    files = []
    for i, m in enumerate(members):
        d = os.path.join(folder, f"member_{i}")
        os.makedirs(d, exist_ok=True)
        np.savez(os.path.join(d, name + ".npz"), probabilities=m)
        save_pickle({"case": name}, os.path.join(d, name + ".pkl"))
        files.append(os.path.join(d, name + ".npz"))
    return files


def main():
    _stub_third_party()
    ENS = importlib.import_module("nnunetv2.ensembling.ensemble")
    EV = importlib.import_module("nnunetv2.evaluation.evaluate_predictions")
    L = importlib.import_module("nnunetv2.utilities.label_handling.label_handling")
    P = importlib.import_module("nnunetv2.utilities.file_path_utilities")
    J = importlib.import_module("nnunetv2.utilities.json_export")
    ENS.multiprocessing = SERIAL
    EV.multiprocessing = SERIAL
    rw = NpyIO()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        # ---- ensembles ----
        for name, make in C.ENSEMBLES.items():
            members = make()
            K = members[0].shape[0]
            files = _write_members(os.path.join(tmp, "ens", name), name, members)
            mean = ENS.average_probabilities(files)
            assert mean.dtype == np.float32 and mean.shape == members[0].shape
            trunc = os.path.join(tmp, "ens", name, "merged")
            ENS.merge_files(files, trunc, ".npy", rw, _label_manager(L, K), False)
            labels = np.load(trunc + ".npy")
            flat = np.sort(mean.reshape(K, -1), 0)[-2:]
            assert ((flat[1] == flat[0]) | (flat[1] - flat[0] >= C.MARGIN)).all(), name
            assert np.array_equal(labels, mean.argmax(0)), name
            assert np.array_equal(mean.view(np.uint32), C.mean_fp32(members).view(np.uint32)), name
            out[f"ens/{name}/mean"] = mean
            out[f"ens/{name}/labels"] = labels.astype(np.uint8)
            print("ensemble", name, mean.shape, "ties", int((flat[1] == flat[0]).sum()))
        # ---- compute_metrics ----
        for tag, (vol, lor, ignore) in C.METRIC_CASES.items():
            ref, pred = C.VOLUMES[vol]()
            d = os.path.join(tmp, "metrics", tag)
            os.makedirs(d)
            np.save(os.path.join(d, "ref.npy"), ref)
            np.save(os.path.join(d, "pred.npy"), pred)
            res = EV.compute_metrics(os.path.join(d, "ref.npy"), os.path.join(d, "pred.npy"), rw, lor, ignore)
            out[f"metrics/{tag}"] = np.asarray(_jsonable(J, res["metrics"]))
            # the confusion matrix over the distinct labels in order of appearance, bin L = any other value, from plain mask sums
            values = []
            for r in lor:
                for v in (r if isinstance(r, tuple) else (r,)):
                    if v not in values:
                        values.append(v)
            n = len(values)
            use = np.ones(ref.shape, bool) if ignore is None else ref != ignore
            a = np.full(ref.shape, n, np.int64)
            b = np.full(ref.shape, n, np.int64)
            for i, v in enumerate(values):
                a[ref == v] = i
                b[pred == v] = i
            cm = np.asarray([[np.sum((a == i) & (b == j) & use) for j in range(n + 1)] for i in range(n + 1)], np.int64)
            for r in lor:
                rows = [values.index(v) for v in (r if isinstance(r, tuple) else (r,))]
                tp = cm[np.ix_(rows, rows)].sum()
                m = res["metrics"][r]
                assert (m["TP"], m["FN"], m["FP"]) == (tp, cm[rows].sum() - tp, cm[:, rows].sum() - tp), (tag, r)
                assert m["TN"] == cm.sum() - cm[rows].sum() - cm[:, rows].sum() + tp, (tag, r)
            out[f"cm/{tag}"] = cm
            print("metrics", tag, cm.shape)
        # ---- compute_metrics_on_folder ----
        for tag, (names, lor, ignore) in C.FOLDERS.items():
            rdir, pdir = os.path.join(tmp, "folder", tag, "ref"), os.path.join(tmp, "folder", tag, "pred")
            os.makedirs(rdir)
            os.makedirs(pdir)
            for i, (ref, pred) in enumerate(C.folder_volumes(names)):
                np.save(os.path.join(rdir, f"case_{i:03d}.npy"), ref)
                np.save(os.path.join(pdir, f"case_{i:03d}.npy"), pred)
            summary = os.path.join(pdir, "summary.json")
            EV.compute_metrics_on_folder(rdir, pdir, summary, rw, ".npy", lor, ignore, 1)
            with open(summary) as f:
                out[f"folder/{tag}/summary_json"] = np.asarray(f.read())
            print("folder", tag)
        # ---- model selection ----
        for tag in C.SELECTIONS:
            cands, refs = C.selection(tag)
            base = os.path.join(tmp, "sel", tag)
            rdir = os.path.join(base, "labelsTr")
            os.makedirs(rdir)
            for c, ref in refs.items():
                np.save(os.path.join(rdir, c + ".npy"), ref)
            scores = {}
            for name, cases in cands.items():
                d = os.path.join(base, name)
                os.makedirs(d)
                for c, (seg, probs) in cases.items():
                    np.save(os.path.join(d, c + ".npy"), seg)
                    if probs is not None:
                        np.savez(os.path.join(d, c + ".npz"), probabilities=probs)
                        save_pickle({"case": c}, os.path.join(d, c + ".pkl"))
                scores[name] = EV.compute_metrics_on_folder(rdir, d, None, rw, ".npy", C.SEL_LABELS, None, 1)["foreground_mean"]["Dice"]
            names = list(cands)
            for i in range(len(names)):
                for j in range(i + 1, len(names)):
                    m1, m2 = names[i], names[j]
                    if any(v[1] is None for v in cands[m1].values()) or any(v[1] is None for v in cands[m2].values()):
                        continue
                    name = P.get_ensemble_name(os.path.join(base, m1), os.path.join(base, m2), C.SEL_FOLDS)
                    d = os.path.join(base, name)
                    os.makedirs(d)
                    for c in C.SEL_CASES:
                        files = [os.path.join(base, m, c + ".npz") for m in (m1, m2)]
                        mean = ENS.average_probabilities(files)
                        top = np.sort(mean.reshape(mean.shape[0], -1), 0)[-2:]
                        assert ((top[1] == top[0]) | (top[1] - top[0] >= C.MARGIN)).all(), (tag, name, c)
                        ENS.merge_files(files, os.path.join(d, c), ".npy", rw, _label_manager(L, 3), False)
                        assert np.array_equal(np.load(os.path.join(d, c + ".npy")), mean.argmax(0)), (tag, name, c)
                    scores[name] = EV.compute_metrics_on_folder(rdir, d, None, rw, ".npy", C.SEL_LABELS, None, 1)["foreground_mean"]["Dice"]
            out[f"sel/{tag}/scores"] = np.asarray(json.dumps(scores))
            print("selection", tag, scores)
    np.savez_compressed(os.path.join(HERE, "ensemble.npz"), **out)
    print("ensemble", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "ensemble.npz")), "bytes")


if __name__ == "__main__":
    main()
