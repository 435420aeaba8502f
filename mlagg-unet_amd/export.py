"""Prediction export to the original image geometry: the reference's
mlagg/nnunetv2/inference/export_prediction.py:10-69 with its default probability resampler, resample_data_or_seg_to_shape(is_seg=False,
order=1, order_z=0, force_separate_z=None) of preprocessing/resampling/default_resampling.py:76-200.

From fp32 logits in the preprocessed geometry (cropped to the non-zero box, resampled to the plan's spacing, transposed by
transpose_forward) to a uint8 label volume in the original geometry:
  1. resample the logits to shape_after_cropping_and_before_resampling (order-1 in-plane; order 0 or 1 along a low-resolution axis
     when the spacing is anisotropic);
  2. fp32 softmax over the classes and the first-maximum argmax of the probabilities;
  3. paste the labels (and probabilities) into shape_before_cropping at bbox_used_for_cropping, zeros outside;
  4. transpose by transpose_backward.

Every coordinate comes from one table per output axis (_axis_taps), built in float64 with the reference's expressions: two source
indices and their two weights.  A device tensor takes K21 (csrc/export.hip): one fused kernel for up to 32 classes that never
materialises the resampled logits, or the resampling kernel followed by torch's softmax / argmax for more.  A CPU tensor or numpy
array takes the host path: the same separable blend in torch float64, then the same fp32 softmax, argmax and paste.  Both give the
same fp32 resampled logits bit for bit.

Region-based label managers (sigmoid heads, dataset.json with tuple-valued labels and a regions_class_order) take step 2 in the form of
label_handling.py:46-47, 166-173: the fp32 sigmoid of every head, and a label that starts at 0 and takes regions_class_order[i] wherever
sigmoid_i > 0.5, for i in order -- the last match wins.  K21 has a region mode for it (mlagg_export_segmentation_regions).

The cascade's hand-off out of a low-resolution stage (export_prediction.py:74-106, called per validation case by
nnUNetTrainer.perform_actual_validation :1146-1181) is the same computation with another target: the logits are resampled to the shape
the NEXT stage's preprocessing gives the case and turned into labels there, without paste or transpose.  resample_logits_to_next_stage
does it (K21 with an empty border on the device), resample_and_save is the reference's drop-in that writes the .npz
dataloading.Dataset(folder_with_segs_from_previous_stage=...) reads, and next_stage_target_shape computes that shape from the case's
properties, for a caller that has no preprocessed next-stage file at hand.
"""
import json
import os
import pickle

import numpy as np
import torch

ANISO_THRESHOLD = 3                  # nnunetv2/configuration.py:7


# ------------------------------------------------------------------------------------------------
# the reference's decisions (default_resampling.py:13-20, 76-119)
# ------------------------------------------------------------------------------------------------
def get_do_separate_z(spacing, anisotropy_threshold=ANISO_THRESHOLD):
    return (np.max(spacing) / np.min(spacing)) > anisotropy_threshold


def get_lowres_axis(spacing):
    return np.where(max(spacing) / np.array(spacing) == 1)[0]


def separate_z_decision(current_spacing, new_spacing, force_separate_z=None, separate_z_anisotropy_threshold=ANISO_THRESHOLD):
    """-> (do_separate_z, low-resolution axis or None), as resample_data_or_seg_to_shape decides them (:86-112)."""
    if force_separate_z is not None:
        do_separate_z = bool(force_separate_z)
        axis = get_lowres_axis(current_spacing) if force_separate_z else None
    elif get_do_separate_z(current_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(current_spacing)
    elif get_do_separate_z(new_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(new_spacing)
    else:
        do_separate_z, axis = False, None
    if axis is not None and len(axis) in (2, 3):   # e.g. spacing (0.24, 1.25, 1.25): no separate z
        do_separate_z = False
    if not do_separate_z:
        return False, None
    return True, int(axis[0])


def _axis_taps(n_in, n_out, kind):
    """Table of one output axis: idx (n_out, 2) int32 and w (n_out, 2) float64, out[o] = in[idx[o, 0]] * w[o, 0] + in[idx[o, 1]] * w[o, 1].
    kind 'linear': ndi.zoom(order=1, mode='nearest', grid_mode=True), i.e. skimage resize(order=1, mode='edge', anti_aliasing=False):
    c = (o + 0.5) * n_in / n_out - 0.5 clamped to [0, n_in - 1], taps floor(c) and floor(c) + 1 (clamped), weights 1 - f and f.
    kind 'nearest': map_coordinates(order=0, mode='nearest') along the low-resolution axis (:172-184): floor(c + 0.5), clamped.
    kind 'identity': the axis is unchanged."""
    o = np.arange(n_out, dtype=np.float64)
    if kind == "identity":
        if n_in != n_out:
            raise RuntimeError(f"identity axis of {n_in} -> {n_out}")
        i0 = o.astype(np.int64)
        i1, w1 = i0, np.zeros(n_out)
    else:
        c = float(n_in) / n_out * (o + 0.5) - 0.5
        if kind == "nearest":
            i0 = np.clip(np.floor(c + 0.5), 0, n_in - 1).astype(np.int64)
            i1, w1 = i0, np.zeros(n_out)
        elif kind == "linear":
            c = np.clip(c, 0, n_in - 1)
            fl = np.floor(c)
            i0 = fl.astype(np.int64)
            i1 = np.minimum(i0 + 1, n_in - 1)
            w1 = c - fl
        else:
            raise RuntimeError(f"unknown tap kind {kind!r}")
    idx = np.stack([i0, i1], 1).astype(np.int32)
    w = np.stack([1.0 - w1, w1], 1)
    return idx, w


def _check_orders(order, order_z):
    if order != 1 or order_z not in (0, 1):
        raise NotImplementedError(f"probability resampling of order {order} / order_z {order_z}: only order 1 with order_z 0 or 1 "
                                  "(the export default) is implemented")


def resampling_plan(in_shape, new_shape, current_spacing, new_spacing, order=1, order_z=0, force_separate_z=None,
                    separate_z_anisotropy_threshold=ANISO_THRESHOLD):
    """-> (tap kinds of the three axes, or None when no resampling is needed (the reference returns the data unchanged))."""
    _check_orders(order, order_z)
    in_shape, new_shape = tuple(int(s) for s in in_shape), tuple(int(s) for s in new_shape)
    if len(in_shape) != 3 or len(new_shape) != 3:
        raise RuntimeError(f"resampling needs three spatial axes, got {in_shape} -> {new_shape}")
    if in_shape == new_shape:
        return None
    sep, axis = separate_z_decision(current_spacing, new_spacing, force_separate_z, separate_z_anisotropy_threshold)
    kinds = []
    for a, (n_in, n_out) in enumerate(zip(in_shape, new_shape)):
        if n_in == n_out:
            kinds.append("identity")
        elif sep and a == axis:
            kinds.append("nearest" if order_z == 0 else "linear")
        else:
            kinds.append("linear")
    return tuple(kinds)


def build_taps(in_shape, new_shape, kinds):
    """The three axis tables of a plan, concatenated x, y, z (identity tables when kinds is None)."""
    kinds = kinds or ("identity",) * 3
    parts = [_axis_taps(int(a), int(b), k) for a, b, k in zip(in_shape, new_shape, kinds)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


# ------------------------------------------------------------------------------------------------
# host path: the kernels' arithmetic in torch float64
# ------------------------------------------------------------------------------------------------
def _resample_host(logits, taps, new_shape):
    """(C, X, Y, Z) fp32 CPU -> (C, *new_shape) fp32: blend along z, then y, then x in float64 per channel, rounded once -- the
    products and sums of csrc/export.hip's interp, in the same order."""
    idx, w = (torch.from_numpy(a) for a in taps)
    Xo, Yo, Zo = new_shape
    ix, iy, iz = idx[:Xo].long(), idx[Xo:Xo + Yo].long(), idx[Xo + Yo:].long()
    wx, wy, wz = w[:Xo], w[Xo:Xo + Yo], w[Xo + Yo:]
    out = torch.empty((logits.shape[0],) + tuple(new_shape), dtype=torch.float32)
    for c in range(logits.shape[0]):
        v = logits[c].double()
        v = v[:, :, iz[:, 0]] * wz[:, 0] + v[:, :, iz[:, 1]] * wz[:, 1]
        v = v[:, iy[:, 0], :] * wy[:, 0, None] + v[:, iy[:, 1], :] * wy[:, 1, None]
        v = v[ix[:, 0]] * wx[:, 0, None, None] + v[ix[:, 1]] * wx[:, 1, None, None]
        out[c] = v.float()
    return out


def _as_logits(logits):
    if isinstance(logits, np.ndarray):
        logits = torch.from_numpy(logits)
    if not isinstance(logits, torch.Tensor):
        raise RuntimeError(f"logits: expected a torch tensor or numpy array, got {type(logits)}")
    if not logits.is_floating_point():
        raise RuntimeError(f"logits: expected floating point values, got {logits.dtype}")
    if logits.dim() != 4 or min(logits.shape) < 1:
        raise RuntimeError(f"logits: expected a non-empty (C, x, y, z) array, got shape {tuple(logits.shape)}")
    return logits.float()


def resample_logits_to_shape(logits, new_shape, current_spacing, new_spacing, order=1, order_z=0, force_separate_z=None,
                             separate_z_anisotropy_threshold=ANISO_THRESHOLD):
    """resample_data_or_seg_to_shape(is_seg=False) (default_resampling.py:76-200) for order 1: logits (C, x, y, z) fp32 ->
    (C, *new_shape) fp32 on the input's device (K21's resampling kernel on the GPU, the float64 host blend on the CPU).  As in
    the reference, logits that already have new_shape are returned unchanged."""
    logits = _as_logits(logits)
    new_shape = tuple(int(s) for s in new_shape)
    kinds = resampling_plan(logits.shape[1:], new_shape, current_spacing, new_spacing, order, order_z, force_separate_z,
                            separate_z_anisotropy_threshold)
    if kinds is None:
        return logits
    taps = build_taps(logits.shape[1:], new_shape, kinds)
    if logits.is_cuda:
        from . import ops
        return ops.resample_linear(logits, taps, new_shape)
    return _resample_host(logits, taps, new_shape)


# ------------------------------------------------------------------------------------------------
# export
# ------------------------------------------------------------------------------------------------
def current_spacing_for(configuration_spacing, properties):
    """export_prediction.py:29-32: a 2-D configuration (two spacing values) keeps the original spacing of the first axis."""
    spacing = [float(s) for s in configuration_spacing]
    if len(spacing) == len(properties["shape_after_cropping_and_before_resampling"]):
        return spacing
    return [float(properties["spacing"][0]), *spacing]


def _geometry(logits, properties, transpose_backward):
    crop = tuple(int(s) for s in properties["shape_after_cropping_and_before_resampling"])
    full = tuple(int(s) for s in properties["shape_before_cropping"])
    bbox = [tuple(int(v) for v in b) for b in properties["bbox_used_for_cropping"]]
    perm = tuple(int(p) for p in transpose_backward)
    if len(crop) != 3 or len(full) != 3 or len(bbox) != 3:
        raise RuntimeError(f"export: expected 3-D geometry, got crop {crop}, shape {full}, bbox {bbox}")
    if logits.dim() != 1 + len(crop):
        raise RuntimeError(f"export: logits of shape {tuple(logits.shape)} do not match the preprocessed (c, x, y, z) layout")
    if any(len(b) != 2 or not 0 <= b[0] < b[1] <= s for b, s in zip(bbox, full)):
        raise RuntimeError(f"export: bbox_used_for_cropping {bbox} is not inside shape_before_cropping {full}")
    if tuple(b[1] - b[0] for b in bbox) != crop:
        raise RuntimeError(f"export: shape_after_cropping_and_before_resampling {crop} differs from the extent of the bbox {bbox}")
    if sorted(perm) != [0, 1, 2]:
        raise RuntimeError(f"export: transpose_backward {perm} is not a permutation of (0, 1, 2)")
    if logits.shape[0] > 256:
        raise RuntimeError(f"export: {logits.shape[0]} classes do not fit the uint8 segmentation")
    return crop, full, tuple(b[0] for b in bbox), perm


def paint_regions(probabilities, regions_class_order):
    """convert_probabilities_to_segmentation of a region-based label manager (label_handling.py:166-173): probabilities (K, ...) ->
    uint8 labels (...), 0 and then regions_class_order[i] wherever probabilities[i] > 0.5, in order (the last match wins)."""
    order = [int(v) for v in regions_class_order]
    if len(order) != probabilities.shape[0] or any(not 0 <= v <= 255 for v in order):
        raise RuntimeError(f"regions_class_order {order} for {probabilities.shape[0]} heads (one uint8 label per head)")
    seg = torch.zeros(probabilities.shape[1:], dtype=torch.uint8, device=probabilities.device)
    for i, c in enumerate(order):
        seg[probabilities[i] > 0.5] = c
    return seg


def _finish(resampled, crop, full, lo, perm, return_probabilities, regions_class_order=None):
    """Softmax, argmax, paste and transpose of resampled logits (K, *crop), on their device (host path and K > 32); with
    regions_class_order: sigmoid and the painting of the regions instead of softmax and argmax."""
    sl = tuple(slice(a, a + c) for a, c in zip(lo, crop))
    seg = torch.zeros(full, dtype=torch.uint8, device=resampled.device)
    if regions_class_order is not None:
        probs = torch.sigmoid(resampled)
        seg[sl] = paint_regions(probs, regions_class_order)
    else:
        probs = torch.softmax(resampled, 0)
        seg[sl] = probs.argmax(0).to(torch.uint8)
    seg = seg.permute(perm).contiguous()
    if not return_probabilities:
        return seg, None
    out = torch.zeros((probs.shape[0],) + full, dtype=torch.float32, device=resampled.device)
    out[(slice(None),) + sl] = probs
    return seg, out.permute((0,) + tuple(p + 1 for p in perm)).contiguous()


def convert_predicted_logits_to_segmentation_with_correct_shape(logits, properties, configuration_spacing, transpose_backward=(0, 1, 2),
                                                                 return_probabilities=False, order=1, order_z=0, force_separate_z=None,
                                                                 regions_class_order=None):
    """logits (K, x, y, z) in the preprocessed geometry (any strides) -> (segmentation uint8 in the original geometry, probabilities
    (K, *original) fp32 or None), on the logits' device: export_prediction.py:28-63 with the default probability resampler.
    properties: the preprocessing's dict (spacing, shape_before_cropping, bbox_used_for_cropping,
    shape_after_cropping_and_before_resampling); configuration_spacing: the plan configuration's spacing (2 or 3 values).
    regions_class_order (one label per head): the logits are the sigmoid heads of a region-based label manager; the probabilities are
    their sigmoids and the segmentation is painted in that order (label_handling.py:166-173)."""
    logits = _as_logits(logits)
    crop, full, lo, perm = _geometry(logits, properties, transpose_backward)
    cur = current_spacing_for(configuration_spacing, properties)
    kinds = resampling_plan(logits.shape[1:], crop, cur, [float(s) for s in properties["spacing"]], order, order_z, force_separate_z)
    taps = build_taps(logits.shape[1:], crop, kinds)
    if logits.is_cuda:
        from . import ops
        if logits.shape[0] <= ops.EXPORT_MAX_CLASSES:
            return ops.export_segmentation(logits, taps, crop, lo, full, perm, return_probabilities, regions_class_order)
        resampled = logits if kinds is None else ops.resample_linear(logits, taps, crop)
    else:
        resampled = logits if kinds is None else _resample_host(logits, taps, crop)
    return _finish(resampled, crop, full, lo, perm, return_probabilities, regions_class_order)


def resample_logits_to_next_stage(logits, target_shape, configuration_spacing, properties, regions_class_order=None, order=1,
                                  order_z=0, force_separate_z=None):
    """The computation of the reference's resample_and_save (export_prediction.py:74-106): logits (K, x, y, z) of this (low-resolution)
    configuration -> the uint8 segmentation (*target_shape) in the next stage's preprocessed geometry, on the logits' device.  As in
    the reference, the current AND the new spacing handed to the resampler are this configuration's spacing (with properties['spacing'][0]
    in front of a 2-value spacing), so the separate-z decision depends on it alone.  A device tensor takes K21 (the fused kernel with
    box (0, 0, 0), shape target_shape and the identity transpose; above 32 classes the resampling kernel and torch's softmax / argmax),
    a CPU tensor or numpy array the host path."""
    logits = _as_logits(logits)
    target = tuple(int(s) for s in target_shape)
    if len(target) != 3 or min(target) < 1:
        raise RuntimeError(f"target_shape {tuple(target_shape)}: three positive sizes expected")
    if logits.shape[0] > 256:
        raise RuntimeError(f"{logits.shape[0]} classes do not fit the uint8 segmentation")
    spacing = current_spacing_for(configuration_spacing, properties)
    kinds = resampling_plan(logits.shape[1:], target, spacing, spacing, order, order_z, force_separate_z)
    taps = build_taps(logits.shape[1:], target, kinds)
    origin, identity = (0, 0, 0), (0, 1, 2)
    if logits.is_cuda:
        from . import ops
        if logits.shape[0] <= ops.EXPORT_MAX_CLASSES:
            return ops.export_segmentation(logits, taps, target, origin, target, identity, False, regions_class_order)[0]
        resampled = logits if kinds is None else ops.resample_linear(logits, taps, target)
    else:
        resampled = logits if kinds is None else _resample_host(logits, taps, target)
    return _finish(resampled, target, target, origin, identity, False, regions_class_order)[0]


def next_stage_target_shape(properties, plans, next_configuration):
    """The spatial shape preprocessing.preprocess_case of `next_configuration` gives the case whose (preprocessed) properties these
    are: compute_new_shape of shape_after_cropping_and_before_resampling under the transposed original spacing and the next
    configuration's spacing (default_preprocessor.py:75-81) -- resample_and_save's target_shape, which the reference reads from the
    next stage's preprocessed file (nnUNetTrainer.py:1166-1172)."""
    from . import preprocessing
    tf = [int(t) for t in plans.get("transpose_forward", [0, 1, 2])]
    original_spacing = [float(properties["spacing"][i]) for i in tf]
    cfg = preprocessing.get_configuration(plans, next_configuration)
    shape = tuple(int(s) for s in properties["shape_after_cropping_and_before_resampling"])
    return tuple(int(s) for s in preprocessing._target_shape(cfg, shape, original_spacing)[1])


def region_order_of(label_manager):
    """regions_class_order of a region-based label manager, None for a label-based one."""
    if not getattr(label_manager, "has_regions", False):
        return None
    order = getattr(label_manager, "regions_class_order", None)
    if order is None:
        raise NotImplementedError("a region-based label manager without regions_class_order is not supported: the labels are "
                                  "painted in that order (label_handling.py:158-173)")
    return [int(v) for v in order]


def export_prediction_from_softmax(predicted_array_or_file, properties_dict, configuration_manager, plans_manager,
                                   dataset_json_dict_or_file, output_file_truncated, save_probabilities=False):
    """Drop-in for the reference's export_prediction_from_softmax (export_prediction.py:10-69), same arguments and files.  The logits
    are exported where they live: a device tensor through K21, a CPU tensor or numpy array (or a .npy / .npz file, removed after
    loading) through the host path.  Duck-typed: configuration_manager.spacing, plans_manager.transpose_backward,
    plans_manager.get_label_manager(dataset_json) (a region-based manager gives its regions_class_order) and
    plans_manager.image_reader_writer_class().write_seg(seg, file, properties)."""
    if isinstance(predicted_array_or_file, str):
        path = predicted_array_or_file
        if path.endswith(".npy"):
            predicted_array_or_file = np.load(path)
        elif path.endswith(".npz"):
            predicted_array_or_file = np.load(path)["softmax"]
        else:
            raise RuntimeError(f"export: {path} is neither a .npy nor a .npz file")
        os.remove(path)
    if isinstance(dataset_json_dict_or_file, str):
        with open(dataset_json_dict_or_file) as f:
            dataset_json_dict_or_file = json.load(f)
    label_manager = plans_manager.get_label_manager(dataset_json_dict_or_file)
    regions_class_order = region_order_of(label_manager)
    kwargs = dict(getattr(configuration_manager, "configuration", {}).get("resampling_fn_probabilities_kwargs", {}) or {})
    if kwargs.pop("is_seg", False):
        raise NotImplementedError("the probability resampler must not be a segmentation resampler")
    kwargs = {k: kwargs[k] for k in ("order", "order_z", "force_separate_z") if k in kwargs}
    seg, probs = convert_predicted_logits_to_segmentation_with_correct_shape(
        predicted_array_or_file, properties_dict, configuration_manager.spacing, plans_manager.transpose_backward,
        return_probabilities=save_probabilities, regions_class_order=regions_class_order, **kwargs)
    if save_probabilities:
        np.savez_compressed(output_file_truncated + ".npz", probabilities=probs.cpu().numpy())
        with open(output_file_truncated + ".pkl", "wb") as f:
            pickle.dump(properties_dict, f)
        del probs
    rw = plans_manager.image_reader_writer_class()
    rw.write_seg(seg.cpu().numpy(), output_file_truncated + dataset_json_dict_or_file["file_ending"], properties_dict)


def resample_and_save(predicted, target_shape, output_file, plans_manager, configuration_manager, properties_dict,
                      dataset_json_dict_or_file, next_configuration):
    """Drop-in for the reference's resample_and_save (export_prediction.py:74-106), same arguments: the logits of a low-resolution
    stage (a device tensor, a CPU tensor, a numpy array or a .npy file, removed after loading) -> np.savez_compressed(output_file,
    seg=uint8 (*target_shape)), the file dataloading.Dataset(folder_with_segs_from_previous_stage=...) reads.  Duck-typed as
    export_prediction_from_softmax is; next_configuration is unused, as in the reference."""
    if isinstance(predicted, str):
        path = predicted
        if not path.endswith(".npy") or not os.path.isfile(path):
            raise RuntimeError(f"resample_and_save: {path} is no .npy file")
        predicted = np.load(path)
        os.remove(path)
    if isinstance(dataset_json_dict_or_file, str):
        with open(dataset_json_dict_or_file) as f:
            dataset_json_dict_or_file = json.load(f)
    regions_class_order = region_order_of(plans_manager.get_label_manager(dataset_json_dict_or_file))
    kwargs = dict(getattr(configuration_manager, "configuration", {}).get("resampling_fn_probabilities_kwargs", {}) or {})
    if kwargs.pop("is_seg", False):
        raise NotImplementedError("the probability resampler must not be a segmentation resampler")
    kwargs = {k: kwargs[k] for k in ("order", "order_z", "force_separate_z") if k in kwargs}
    seg = resample_logits_to_next_stage(predicted, target_shape, configuration_manager.spacing, properties_dict,
                                        regions_class_order=regions_class_order, **kwargs)
    np.savez_compressed(output_file, seg=seg.cpu().numpy())
