"""Ensembling: the reference's mlagg/nnunetv2/ensembling/ensemble.py where the probabilities live.

    average_probabilities        the fp32 mean of M probability volumes (:17-29)
    ensemble_probabilities       the mean's argmax as uint8 labels, and the mean only when asked
    merge_files                  drop-in (:32-46): .npz members -> the segmentation file (and .npz / .pkl)
    ensemble_folders             drop-in (:49-111)
    ensemble_crossvalidations    drop-in (:128-206), with the reference's checks and errors

CUDA tensors run K28 (csrc/ensemble.hip, ops.ensemble_mean): one pass that reads every member value once and writes one byte per
voxel.  CPU tensors and numpy arrays run numpy with the same arithmetic: acc = float32(m_0), acc += m_i in member order, acc /= M.
Both give the same bits.  Cases are processed one after another; there is no process pool (num_processes is accepted and ignored).

Two deliberate deviations from the reference:
  - The label is the argmax of the MEAN, not of softmax(mean).  The reference's merge_files passes the averaged probabilities through
    convert_logits_to_segmentation, which applies softmax a second time before the argmax.  Softmax is monotone, so the label is the
    same wherever the two largest means are equal or clearly apart; it can differ only where fp32 rounding of the second softmax
    merges two distinct means, where the reference falls back to the lower class.  Here the first class whose mean is the maximum
    wins (numpy's argmax; a NaN counts as a maximum).
  - With save_probabilities the .pkl holds the first member's properties, as every other .pkl of the pipeline does; the reference
    pickles the probabilities into it (:46).
Region-based label managers (sigmoid probabilities): the mean is the same and the label is painted from it in regions_class_order
(label_handling.py:166-173: 0, then regions_class_order[k] wherever mean_k > 0.5, the last match winning), which is what the reference
computes with its second nonlinearity left out -- there merge_files applies the sigmoid again to the averaged probabilities, so that
every head fires wherever its mean is positive.
"""
import json
import os
import pickle
import shutil

import numpy as np
import torch

from . import ops
from .export import region_order_of

MAX_CLASSES = ops.ENSEMBLE_MAX_CLASSES


def _load(member):
    """A member as given, a .npz path as its 'probabilities' array (the key the reference reads)."""
    if isinstance(member, (str, os.PathLike)):
        path = os.fspath(member)
        if not path.endswith(".npz"):
            raise RuntimeError(f"ensemble: {path} is not a .npz file")
        with np.load(path) as f:
            return f["probabilities"]
    return member


def _members(members, min_classes=2):
    """The members as a list of arrays / tensors that all live in one place (files join the others: the device if any member is a
    device tensor), checked for a common shape (K, ...) with 2 <= K <= 256 (regions: 1 <= K) and a floating dtype."""
    members = [_load(m) for m in members]
    if not members:
        raise RuntimeError("At least one member must be given")
    device = next((m.device for m in members if isinstance(m, torch.Tensor) and m.is_cuda), None)
    out = []
    for i, m in enumerate(members):
        if not isinstance(m, torch.Tensor):
            m = np.asarray(m)
        if tuple(m.shape) != tuple(members[0].shape):
            raise RuntimeError(f"members[{i}] has shape {tuple(m.shape)}, members[0] {tuple(members[0].shape)}")
        if m.ndim < 2:
            raise RuntimeError(f"members[{i}]: expected probabilities of shape (K, ...), got {tuple(m.shape)}")
        if not min_classes <= m.shape[0] <= MAX_CLASSES:
            raise RuntimeError(f"members[{i}]: {m.shape[0]} classes, {min_classes} to {MAX_CLASSES} are supported (labels are uint8)")
        if device is not None:
            if not isinstance(m, torch.Tensor):
                m = torch.from_numpy(np.ascontiguousarray(m))
            m = m.to(device)
            if m.dtype not in (torch.float32, torch.float16):
                if not m.dtype.is_floating_point:
                    raise RuntimeError(f"members[{i}]: floating-point probabilities expected, got {m.dtype}")
                m = m.float()
            m = m.contiguous()
        else:
            m = m.numpy() if isinstance(m, torch.Tensor) else m
            if m.dtype.kind != "f":
                raise RuntimeError(f"members[{i}]: floating-point probabilities expected, got {m.dtype}")
            if m.dtype not in (np.float32, np.float16):
                m = m.astype(np.float32)                  # as the device path: wider types are rounded to fp32 before the sum
        out.append(m)
    return out, device


def _host_mean(members):
    """The reference's average_probabilities (:17-29) on arrays."""
    avg = members[0].astype(np.float32)                   # a copy: the first member is not modified
    for m in members[1:]:
        avg += m
    avg /= len(members)
    return avg


def _wrap(members_in, x):
    """Host results come back as what went in: tensors if any member was a (CPU) tensor, numpy arrays otherwise."""
    if x is not None and any(isinstance(m, torch.Tensor) for m in members_in):
        return torch.from_numpy(x)
    return x


def _paint_regions(mean, regions_class_order):
    """label_handling.py:166-173 on the mean: 0, then regions_class_order[k] wherever mean[k] > 0.5, in order."""
    order = [int(v) for v in regions_class_order]
    if len(order) != mean.shape[0] or any(not 0 <= v <= 255 for v in order):
        raise RuntimeError(f"regions_class_order {order} for {mean.shape[0]} heads (one uint8 label per head)")
    labels = np.zeros(mean.shape[1:], dtype=np.uint8)
    for k, c in enumerate(order):
        labels[mean[k] > 0.5] = c
    return labels


def ensemble_probabilities(members, return_probabilities=False, regions_class_order=None):
    """members: a list of probability volumes (K, ...) as tensors, numpy arrays or .npz paths -> (uint8 labels (...): the first class
    whose mean is the maximum, the fp32 mean (K, ...) or None).  Without return_probabilities the device path allocates no (K, N)
    buffer.  regions_class_order (one label per head): the members are the sigmoid probabilities of a region-based label manager and
    the labels are painted from the mean in that order."""
    members_in = list(members)
    members, device = _members(members_in, 2 if regions_class_order is None else 1)
    if device is not None:
        return ops.ensemble_mean(members, want_mean=return_probabilities, regions_class_order=regions_class_order)
    mean = _host_mean(members)
    labels = mean.argmax(0).astype(np.uint8) if regions_class_order is None else _paint_regions(mean, regions_class_order)
    return _wrap(members_in, labels), _wrap(members_in, mean if return_probabilities else None)


def average_probabilities(members):
    """The reference's average_probabilities (:17-29): the fp32 mean (K, ...) of tensors, numpy arrays or .npz paths."""
    return ensemble_probabilities(members, return_probabilities=True)[1]


def _to_numpy(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def merge_files(list_of_files, output_filename_truncated, output_file_ending, image_reader_writer, label_manager,
                save_probabilities=False, device=None):
    """Drop-in for the reference's merge_files (:32-46): averages the .npz files, writes the segmentation through
    image_reader_writer.write_seg(seg, file, properties) with the properties of the first file's .pkl, and with save_probabilities
    the mean as .npz and those properties as .pkl.  device: where to ensemble (default: the MI355X when there is one).  A region-based
    label manager has its labels painted from the mean in its regions_class_order."""
    regions_class_order = region_order_of(label_manager)       # a region-based manager without an order is refused here
    if not len(list_of_files):
        raise RuntimeError("At least one file must be given in list_of_files")
    with open(list_of_files[0][:-4] + ".pkl", "rb") as f:
        properties = pickle.load(f)
    members = [_load(f) for f in list_of_files]
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if torch.device(device).type == "cuda":
        members = [torch.from_numpy(np.ascontiguousarray(m)).to(device) for m in members]
    seg, probabilities = ensemble_probabilities(members, return_probabilities=save_probabilities,
                                                regions_class_order=regions_class_order)
    image_reader_writer.write_seg(_to_numpy(seg), output_filename_truncated + output_file_ending, properties)
    if save_probabilities:
        np.savez_compressed(output_filename_truncated + ".npz", probabilities=_to_numpy(probabilities))
        with open(output_filename_truncated + ".pkl", "wb") as f:
            pickle.dump(properties, f)


def _json(file_or_dict):
    if isinstance(file_or_dict, (str, os.PathLike)):
        with open(file_or_dict) as f:
            return json.load(f)
    return file_or_dict


def _npz_files(folder):
    return sorted(f for f in os.listdir(folder) if f.endswith(".npz") and os.path.isfile(os.path.join(folder, f)))


def _io(plans, dataset_json, image_reader_writer, label_manager):
    """The reader/writer object and label manager: as given, else from nnunetv2's PlansManager as in the reference."""
    if image_reader_writer is None or label_manager is None:
        try:
            from nnunetv2.utilities.plans_handling.plans_handler import PlansManager
        except ImportError as e:
            raise RuntimeError("pass image_reader_writer and label_manager, or install nnunetv2 for its PlansManager") from e
        plans_manager = PlansManager(plans)
        image_reader_writer = image_reader_writer or plans_manager.image_reader_writer_class()
        label_manager = label_manager or plans_manager.get_label_manager(dataset_json)
    region_order_of(label_manager)                             # refuses a region-based manager without regions_class_order
    return image_reader_writer, label_manager


def ensemble_folders(list_of_input_folders, output_folder, save_merged_probabilities=False, num_processes=None,
                     dataset_json_file_or_dict=None, plans_json_file_or_dict=None, *, image_reader_writer=None, label_manager=None,
                     device=None):
    """Drop-in for the reference's ensemble_folders (:49-111).  dataset.json and plans.json default to the first folder's; every folder
    must hold the same .npz files; dataset.json is copied to the output folder.  image_reader_writer (an object with write_seg) and
    label_manager replace the ones the reference builds from the plans; num_processes is ignored."""
    dataset_json = _json(dataset_json_file_or_dict if dataset_json_file_or_dict is not None
                         else os.path.join(list_of_input_folders[0], "dataset.json"))
    if image_reader_writer is None or label_manager is None:
        plans = _json(plans_json_file_or_dict if plans_json_file_or_dict is not None
                      else os.path.join(list_of_input_folders[0], "plans.json"))
    else:
        plans = None
    files_per_folder = [set(_npz_files(i)) for i in list_of_input_folders]
    s = set().union(*files_per_folder)
    for f in files_per_folder:
        assert len(s.difference(f)) == 0, "Not all folders contain the same files for ensembling. Please only " \
                                          "provide folders that contain the predictions"
    image_reader_writer, label_manager = _io(plans, dataset_json, image_reader_writer, label_manager)
    os.makedirs(output_folder, exist_ok=True)
    shutil.copy(os.path.join(list_of_input_folders[0], "dataset.json"), output_folder)
    for fi in sorted(s):
        merge_files([os.path.join(fl, fi) for fl in list_of_input_folders], os.path.join(output_folder, fi[:-4]),
                    dataset_json["file_ending"], image_reader_writer, label_manager, save_merged_probabilities, device=device)


def ensemble_crossvalidations(list_of_trained_model_folders, output_folder, folds=(0, 1, 2, 3, 4), num_processes=None, overwrite=True,
                              *, image_reader_writer=None, label_manager=None, device=None):
    """Drop-in for the reference's ensemble_crossvalidations (:128-206): ensembles the fold_X/validation .npz predictions of several
    trained models case by case (different models may have different splits), with its checks and errors: a missing fold or a fold
    without .npz files raises RuntimeError, so does a model that lacks a case, and a case in two folds of one model fails the
    reference's assertion.  overwrite=False skips cases whose output file exists.  plans.json and dataset.json of the first model are
    copied to the output folder."""
    first = list_of_trained_model_folders[0]
    dataset_json = _json(os.path.join(first, "dataset.json"))
    files_per_folder = {}
    unique_filenames = set()
    for tr in list_of_trained_model_folders:
        files_per_folder[tr] = {}
        for f in folds:
            val = os.path.join(tr, f"fold_{f}", "validation")
            if not os.path.isdir(val):
                raise RuntimeError(f"Expected model output directory does not exist. You must train all requested "
                                   f"folds of the speficied model.\nModel: {tr}\nFold: {f}")
            files_here = _npz_files(val)
            if len(files_here) == 0:
                raise RuntimeError(f"No .npz files found in folder {val}. Rerun your "
                                   f"validation with the --npz flag. Use nnUNetv2_train [...] --val --npz.")
            files_per_folder[tr][f] = files_here
            unique_filenames.update(files_here)
    for tr, fi in files_per_folder.items():
        all_files_here = set()
        for f in folds:
            all_files_here.update(fi[f])
        diff = unique_filenames.difference(all_files_here)
        if len(diff) > 0:
            print(f"model {tr} does not seem to contain all predictions. Missing: {diff}")
            raise RuntimeError("There were missing files, see print statements above this one")
    file_mapping = []
    for tr in list_of_trained_model_folders:
        file_mapping.append({})
        for f in folds:
            for fi in files_per_folder[tr][f]:
                assert fi not in file_mapping[-1].keys(), f"Duplicate detected. Case {fi} is present in more than " \
                                                          f"one fold of model {tr}."
                file_mapping[-1][fi] = os.path.join(tr, f"fold_{f}", "validation", fi)
    plans = None if image_reader_writer is not None and label_manager is not None else os.path.join(first, "plans.json")
    image_reader_writer, label_manager = _io(plans, dataset_json, image_reader_writer, label_manager)
    os.makedirs(output_folder, exist_ok=True)
    for fi in sorted(unique_filenames):
        truncated = os.path.join(output_folder, fi[:-4])
        if not overwrite and os.path.isfile(truncated + dataset_json["file_ending"]):
            continue
        merge_files([fm[fi] for fm in file_mapping], truncated, dataset_json["file_ending"], image_reader_writer, label_manager,
                    False, device=device)
    shutil.copy(os.path.join(first, "plans.json"), os.path.join(output_folder, "plans.json"))
    shutil.copy(os.path.join(first, "dataset.json"), os.path.join(output_folder, "dataset.json"))
