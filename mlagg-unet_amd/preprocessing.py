"""Case preprocessing (the preprocessing part): the reference's DefaultPreprocessor.run_case
(mlagg/nnunetv2/preprocessing/preprocessors/default_preprocessor.py:38-124) with the default plans: transpose by transpose_forward,
crop to the non-zero box, normalise every channel, resample to the configuration's spacing with
resample_data_or_seg_to_shape(order=3, order_z=0, force_separate_z=None) (default_experiment_planner.py:123-128).  preprocess_case
does it for a test case (no segmentation, or, for a cascaded configuration, the previous stage's segmentation as run_case's seg:
inference/predict_from_raw_data.py:47-67); preprocess_training_case adds the segmentation (cropped with -1 outside the filled
non-zero mask, resampled with resample_data_or_seg_to_shape(is_seg=True, order=1, order_z=0), :129-135) and the sampled
class_locations (_sample_foreground_locations, :134-161); preprocess_dataset writes the case folder dataloading.Dataset reads.

A CUDA device runs K22 (csrc/preprocess.hip): the box of the non-zero voxels (one read-back of 6 ints), crop + normalisation in
fp32, and the cubic zoom one axis at a time in fp64 (prefilter and 4-tap evaluation per line, tap tables from _cubic_taps), clipped
to each resize call's input range and rounded once to fp32; and, for a training case, K26 (csrc/preprocess_train.hip): the
segmentation's crop, its label-wise linear resize without indicator volumes, a label histogram (the case's second read-back) and
the ordered rank select that turns the host's RandomState draws into coordinates.  Anything else runs the reference's arithmetic on
the host with numpy and scipy (binary_fill_holes, ndi.zoom + clip): the CPU path and the A/B side of tools/bench_preprocess*.py.

Parity (tests/test_preprocess_*.py against tests/golden/preprocess.npz and preprocess_train.npz, made by the reference's own
run_case): the host path is bit-identical; on the device, CT / RescaleTo01 / RGBTo01 / unnormalised channels agree to 1 fp32 ulp on
at most 1e-4 of the voxels (the separable fp64 zoom differs from scipy's 3-D one only by its summation order), and ZScore channels
to the rounding of numpy's fp32 mean / std (ZSCORE_TOLERANCE), since the device sums in fp64.  The device's segmentation equals the
host's except possibly where a label's interpolated indicator is within NEAR_TIE of the 0.5 threshold; class locations are
integer work and identical for an identical segmentation.

Not supported (NotImplementedError): training cases of cascaded configurations (previous_stage), region-based labels
(regions_class_order or multi-value labels; with a cascade at prediction time too), preprocessors other than DefaultPreprocessor,
data resamplers other than resample_data_or_seg_to_shape with order 3 and order_z 0 or 1, segmentation resamplers other than
resample_data_or_seg_to_shape with order 1 and order_z 0.  Experiment planning stays the reference's: the plans are an input
(fingerprint.py computes the one entry CT normalisation needs).
File reading is the caller's: the input is the reader's (c, x, y, z) array and its properties (at least 'spacing').
"""
import copy
import os
import pickle

import numpy as np
import scipy.ndimage as ndi
import torch

from .export import ANISO_THRESHOLD, _axis_taps, separate_z_decision

SCHEMES = ("NoNormalization", "CTNormalization", "ZScoreNormalization", "RescaleTo01Normalization", "RGBTo01Normalization")
# |device - host| of a ZScore channel: numpy's fp32 pairwise mean / std against the device's fp64 ones, a few fp32 ulps of the
# statistics relative to the normalised value and to mean / std (tests/test_preprocess_gpu.py)
ZSCORE_TOLERANCE = 2e-6
# a voxel of a resampled segmentation is a near-tie when some label's fp64 interpolated indicator v has |v - 0.5| <= NEAR_TIE: only
# there can another summation order than scipy's flip the label
NEAR_TIE = 2.0 ** -40

SPLINE_POLE = np.sqrt(3.0) - 2.0
SPLINE_PAD = 12                      # scipy's _prepad_for_spline_filter
FIR_HALF_WIDTH = 30                  # |z|^31 < 2e-18: the truncated prefilter is exact in fp64
FIR = np.array([6.0 * SPLINE_POLE / (SPLINE_POLE * SPLINE_POLE - 1.0) * SPLINE_POLE ** k for k in range(FIR_HALF_WIDTH + 1)])


# ------------------------------------------------------------------------------------------------
# plans
# ------------------------------------------------------------------------------------------------
def get_configuration(plans, configuration_name, _visited=()):
    """The configuration dict with inherits_from resolved (PlansManager._internal_resolve_configuration_inheritance)."""
    configurations = plans["configurations"]
    if configuration_name not in configurations:
        raise RuntimeError(f"configuration {configuration_name} not in the plans: {list(configurations)}")
    cfg = copy.deepcopy(configurations[configuration_name])
    if "inherits_from" in cfg:
        parent = cfg["inherits_from"]
        if parent in _visited or parent == configuration_name:
            raise RuntimeError(f"circular inherits_from: {(*_visited, configuration_name, parent)}")
        base = get_configuration(plans, parent, (*_visited, configuration_name))
        base.update(cfg)
        cfg = base
    return cfg


def _data_resampling_kwargs(cfg):
    name = cfg.get("resampling_fn_data", "resample_data_or_seg_to_shape")
    if name != "resample_data_or_seg_to_shape":
        raise NotImplementedError(f"data resampling function {name}: only resample_data_or_seg_to_shape is implemented")
    kw = dict(cfg.get("resampling_fn_data_kwargs") or {"is_seg": False, "order": 3, "order_z": 0, "force_separate_z": None})
    if kw.get("is_seg", False):
        raise NotImplementedError("the data resampler must not be a segmentation resampler")
    order, order_z = kw.get("order", 3), kw.get("order_z", 0)
    _check_orders(order, order_z)
    return order, order_z, kw.get("force_separate_z", None), kw.get("separate_z_anisotropy_threshold", ANISO_THRESHOLD)


def _check_orders(order, order_z):
    if order != 3 or order_z not in (0, 1):
        raise NotImplementedError(f"data resampling of order {order} / order_z {order_z}: only order 3 with order_z 0 or 1 "
                                  "(the planner's default) is implemented")


def _check_configuration(cfg, n_channels):
    if cfg.get("preprocessor_name", "DefaultPreprocessor") != "DefaultPreprocessor":
        raise NotImplementedError(f"preprocessor {cfg['preprocessor_name']}: only DefaultPreprocessor is implemented")
    schemes = list(cfg["normalization_schemes"])
    masks = list(cfg.get("use_mask_for_norm", [False] * len(schemes)))
    if len(schemes) < n_channels or len(masks) < n_channels:
        raise RuntimeError(f"the configuration normalises {len(schemes)} channels, the image has {n_channels}")
    for s in schemes[:n_channels]:
        if s not in SCHEMES:
            raise NotImplementedError(f"normalization scheme {s}: one of {SCHEMES} expected")
    return schemes[:n_channels], [bool(m) if m is not None else None for m in masks[:n_channels]]


# ------------------------------------------------------------------------------------------------
# the reference's helpers, host side
# ------------------------------------------------------------------------------------------------
def compute_new_shape(old_shape, old_spacing, new_spacing):
    """default_resampling.py:22-28."""
    if not len(old_spacing) == len(old_shape) == len(new_spacing):
        raise RuntimeError(f"compute_new_shape: {old_shape}, {old_spacing}, {new_spacing}")
    return np.array([int(round(i / j * k)) for i, j, k in zip(old_spacing, new_spacing, old_shape)])


def create_nonzero_mask(data):
    """cropping.py: OR over the channels of data != 0, holes filled."""
    mask = np.zeros(data.shape[1:], dtype=bool)
    for c in range(data.shape[0]):
        mask |= data[c] != 0
    return ndi.binary_fill_holes(mask)


def get_bbox_from_mask(mask):
    """acvl_utils' get_bbox_from_mask: [[lo, hi + 1], ...] of the True voxels."""
    box = []
    for a in range(mask.ndim):
        hit = np.flatnonzero(mask.any(axis=tuple(b for b in range(mask.ndim) if b != a)))
        if hit.size == 0:
            raise RuntimeError("crop_to_nonzero: the image has no non-zero voxel (the reference fails on it)")
        box.append([int(hit[0]), int(hit[-1]) + 1])
    return box


def crop_to_nonzero(data, seg=None, nonzero_label=-1):
    """cropping.py's crop_to_nonzero: -> (cropped data, seg (1, ...) int8 with nonzero_label outside the filled mask, bbox)."""
    mask = create_nonzero_mask(data)
    bbox = get_bbox_from_mask(mask)
    sl = tuple(slice(*b) for b in bbox)
    data = data[(slice(None),) + sl]
    mask = mask[sl][None]
    if seg is not None:
        seg = seg[(slice(None),) + sl]
        seg[(seg == 0) & (~mask)] = nonzero_label
    else:
        seg = mask.astype(np.int8)
        seg[seg == 0] = nonzero_label
        seg[seg > 0] = 0
    return data, seg, bbox


def _normalize_channel_host(image, seg, scheme, use_mask, props):
    """default_normalization_schemes.py, float32 numpy."""
    image = image.astype(np.float32)
    if scheme == "CTNormalization":
        image = np.clip(image, props["percentile_00_5"], props["percentile_99_5"])
        return (image - props["mean"]) / max(props["std"], 1e-8)
    if scheme == "ZScoreNormalization":
        if use_mask:
            mask = seg >= 0
            mean, std = image[mask].mean(), image[mask].std()
            image[mask] = (image[mask] - mean) / (max(std, 1e-8))
            return image
        return (image - image.mean()) / (max(image.std(), 1e-8))
    if scheme == "RescaleTo01Normalization":
        image = image - image.min()
        return image / np.clip(image.max(), a_min=1e-8, a_max=None)
    if scheme == "RGBTo01Normalization":
        if image.min() < 0 or image.max() > 255:
            raise RuntimeError("RGBTo01Normalization: values outside [0, 255]; the image does not seem to be RGB")
        return image / 255.
    return image


def _resize_host(image, new_shape):
    """skimage resize(order=3, mode='edge', anti_aliasing=False) (>= 0.19): ndi.zoom(grid_mode=True, mode='nearest'), clipped to the
    input's range."""
    out = ndi.zoom(image, np.asarray(new_shape, float) / np.asarray(image.shape, float), order=3, mode="nearest", grid_mode=True)
    return np.clip(out, image.min(), image.max())


def _resample_host(data, new_shape, sep, axis, order_z):
    """resample_data_or_seg (default_resampling.py:120-211) for data of order 3, in float64 -> float32."""
    shape = np.array(data.shape[1:])
    new_shape = np.array(new_shape)
    data = data.astype(float)
    out = []
    if sep:
        plane = [a for a in range(3) if a != axis]
        for c in range(data.shape[0]):
            sl = [_resize_host(np.take(data[c], i, axis), new_shape[plane]) for i in range(shape[axis])]
            r = np.stack(sl, axis)
            if shape[axis] != new_shape[axis]:
                # map_coordinates(order_z, mode='nearest') with the in-plane coordinates on the grid: a blend along the axis alone
                idx, w = _axis_taps(int(shape[axis]), int(new_shape[axis]), "nearest" if order_z == 0 else "linear")
                bshape = [1, 1, 1]
                bshape[axis] = -1
                r = np.take(r, idx[:, 0], axis) * w[:, 0].reshape(bshape) + np.take(r, idx[:, 1], axis) * w[:, 1].reshape(bshape)
            out.append(r[None])
    else:
        for c in range(data.shape[0]):
            out.append(_resize_host(data[c], new_shape)[None])
    return np.vstack(out).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# device side (K22)
# ------------------------------------------------------------------------------------------------
def _cubic_taps(n_in, n_out):
    """One axis of ndi.zoom(order=3, grid_mode=True) on the line edge-padded by SPLINE_PAD: output o reads the prefiltered
    coefficients start[o] .. start[o] + 3 of the padded line with weights w[o] (the cubic B-spline at t = c - floor(c)),
    c = (o + 0.5) * n_in / n_out - 0.5 + SPLINE_PAD.  -> (start int32 (n_out,), w float64 (n_out, 4), P0, M): the coefficients
    start.min() .. start.max() + 3 are the only ones needed."""
    o = np.arange(n_out, dtype=np.float64)
    c = (o + 0.5) * (float(n_in) / n_out) - 0.5 + SPLINE_PAD
    f = np.floor(c)
    t = c - f
    w = np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6], 1)
    start = (f - 1).astype(np.int32)
    P0 = int(start.min())
    return start, w, P0, int(start.max()) + 4 - P0


def _resample_device(x, new_shape, sep, axis, order_z):
    """x (C, X, Y, Z) contiguous fp32 on the device -> (C, *new_shape) fp32: K22's cubic passes, clip and separate-z blend."""
    from . import ops
    shape = tuple(int(s) for s in x.shape[1:])
    new_shape = tuple(int(s) for s in new_shape)
    if sep:
        plane = [a for a in range(3) if a != axis]
        lo, hi = ops.pp_clip_ranges(x, axis)
        clip = (lo, hi, shape[axis], axis)
        last_changes = shape[axis] != new_shape[axis]
        y = ops.pp_cubic_axis(x, plane[0], _cubic_taps(shape[plane[0]], new_shape[plane[0]]), FIR)
        y = ops.pp_cubic_axis(y, plane[1], _cubic_taps(shape[plane[1]], new_shape[plane[1]]), FIR,
                              out_dtype=torch.float64 if last_changes else torch.float32, clip=clip)
        if last_changes:
            y = ops.pp_gather_axis(y, axis, _axis_taps(shape[axis], new_shape[axis], "nearest" if order_z == 0 else "linear"))
        return y
    lo, hi = ops.pp_clip_ranges(x, None)
    y = x
    for a in range(3):
        y = ops.pp_cubic_axis(y, a, _cubic_taps(shape[a], new_shape[a]), FIR, out_dtype=torch.float64 if a < 2 else torch.float32,
                              clip=(lo, hi, 1, None) if a == 2 else None)
    return y


def _resampling_decision(in_shape, new_shape, current_spacing, new_spacing, order, order_z, force_separate_z,
                         threshold=ANISO_THRESHOLD):
    _check_orders(order, order_z)
    in_shape, new_shape = tuple(int(s) for s in in_shape), tuple(int(s) for s in new_shape)
    if len(in_shape) != 3 or len(new_shape) != 3:
        raise RuntimeError(f"resampling needs three spatial axes, got {in_shape} -> {new_shape}")
    if min(new_shape) < 1:
        raise RuntimeError(f"resampling to an empty shape {new_shape}")
    return separate_z_decision(current_spacing, new_spacing, force_separate_z, threshold)


def resample_data_to_shape(data, new_shape, current_spacing, new_spacing, order=3, order_z=0, force_separate_z=None,
                           separate_z_anisotropy_threshold=ANISO_THRESHOLD):
    """resample_data_or_seg_to_shape(is_seg=False) (default_resampling.py:76-200) for order 3: data (c, x, y, z) -> (c, *new_shape)
    float32.  A device tensor runs K22 (contiguous fp32 is expected; other layouts are copied first), anything else the host path.
    As in the reference, data that already has new_shape is returned unchanged."""
    sep, axis = _resampling_decision(data.shape[1:], new_shape, current_spacing, new_spacing, order, order_z, force_separate_z,
                                     separate_z_anisotropy_threshold)
    if tuple(int(s) for s in data.shape[1:]) == tuple(int(s) for s in new_shape):
        return data
    if isinstance(data, torch.Tensor) and data.is_cuda:
        return _resample_device(data.float().contiguous(), new_shape, sep, axis, order_z)
    if isinstance(data, torch.Tensor):
        data = data.numpy()
    return _resample_host(np.asarray(data), new_shape, sep, axis, order_z)


def _filled_mask_device(x, lo, ext):
    """The cropped, hole-filled non-zero mask for the masked ZScore: OR over the channels on the device, binary_fill_holes on the
    host (the one host step of K22's path), uploaded back as uint8.  Filling inside the box equals cropping the filled full mask:
    a background component that reaches the box's border reaches the array's border through voxels outside the box, which are all
    background."""
    sl = tuple(slice(a, a + e) for a, e in zip(lo, ext))
    nz = (x[(slice(None),) + sl] != 0).any(0).cpu().numpy()
    return torch.from_numpy(ndi.binary_fill_holes(nz).astype(np.uint8)).to(x.device)


def _preprocess_device(view, schemes, masks, fg, device, seg=None, max_label=None):
    """K22's crop + normalisation of view (C, X, Y, Z) -> (data, bbox).  With seg (the (X, Y, Z) int16 view of a training case's
    labels): -> (data, bbox, cropped seg, its label histogram), and the masked ZScore takes its mask from the cropped segmentation
    (seg >= 0: labelled voxels where the filled mask is off stay in), as run_case does."""
    from . import ops
    C = view.shape[0]
    box = ops.pp_nonzero_box(view).cpu().tolist()
    if box[3] < 0:
        raise RuntimeError("preprocess_case: the image has no non-zero voxel (the reference fails on it)")
    bbox = [[box[d], box[3 + d] + 1] for d in range(3)]
    lo, ext = [b[0] for b in bbox], [b[1] - b[0] for b in bbox]
    params = np.zeros((C, 4), dtype=np.float32)
    codes = []
    for c, (s, m) in enumerate(zip(schemes, masks)):
        if s == "ZScoreNormalization" and m:
            s = "ZScoreNormalization+mask"
        codes.append(ops.PP_SCHEMES[s])
        if s == "CTNormalization":
            p = fg[str(c)]
            params[c] = [p["percentile_00_5"], p["percentile_99_5"], p["mean"], max(p["std"], 1e-8)]
    d_params = torch.from_numpy(params).to(device)
    stats = torch.zeros((C, 4), dtype=torch.float64, device=device)
    need_mask = ops.PP_SCHEMES["ZScoreNormalization+mask"] in codes
    if seg is not None:
        seg, hist = ops.pp_seg_crop(seg, lo, ext, _filled_mask_device(view, lo, ext), max_label)
        mask = (seg >= 0).to(torch.uint8) if need_mask else None
    else:
        mask = _filled_mask_device(view, lo, ext) if need_mask else None
    for c, code in enumerate(codes):
        if code in (2, 3, 4, 5):
            ops.pp_channel_stats(view, lo, ext, c, code, d_params, stats, mask)
    if 5 in codes:
        mm = stats.cpu().numpy()
        for c, code in enumerate(codes):
            if code == 5 and (mm[c, 2] < 0 or mm[c, 3] > 255):
                raise RuntimeError("RGBTo01Normalization: values outside [0, 255]; the image does not seem to be RGB")
    data = ops.pp_normalize(view, lo, ext, torch.tensor(codes, dtype=torch.int32, device=device), d_params, mask)
    if seg is not None:
        return data, bbox, seg, hist
    return data, bbox


def _case_setup(image, properties, plans, configuration_name, device, what):
    """The checks and plan entries preprocess_case and preprocess_training_case share."""
    cfg = get_configuration(plans, configuration_name)
    if isinstance(image, torch.Tensor):
        on_device = image.is_cuda if device is None else torch.device(device).type == "cuda"
    else:
        on_device = device is not None and torch.device(device).type == "cuda"
    if image.ndim != 4 or min(image.shape) < 1:
        raise RuntimeError(f"{what}: expected a non-empty (c, x, y, z) image, got shape {tuple(image.shape)}")
    schemes, masks = _check_configuration(cfg, int(image.shape[0]))
    tf = [int(t) for t in plans.get("transpose_forward", [0, 1, 2])]
    if sorted(tf) != [0, 1, 2]:
        raise RuntimeError(f"transpose_forward {tf} is not a permutation of (0, 1, 2)")
    fg = plans.get("foreground_intensity_properties_per_channel", {})
    for c, s in enumerate(schemes):
        if s == "CTNormalization" and str(c) not in fg:
            raise RuntimeError(f"CTNormalization of channel {c} needs foreground_intensity_properties_per_channel['{c}']")
    props = dict(properties)
    original_spacing = [float(props["spacing"][i]) for i in tf]
    perm = [0, *[i + 1 for i in tf]]
    dev = None
    if on_device:
        dev = torch.device(device) if device is not None else image.device
    return cfg, dev, schemes, masks, fg, props, original_spacing, perm


def _target_shape(cfg, shape, original_spacing):
    target = [float(s) for s in cfg["spacing"]]
    if len(target) < 3:
        target = [original_spacing[0]] + target
    return target, compute_new_shape(shape, original_spacing, target)


def _check_previous_stage(cfg, seg_from_prev_stage, image):
    """The checks of a cascaded prediction case -> the (1, x, y, z) view of the previous stage's segmentation, or None."""
    if cfg.get("previous_stage") and seg_from_prev_stage is None:
        # a NotImplementedError, which is a RuntimeError: without the segmentation the call asks for what a cascaded stage cannot do
        raise NotImplementedError(f"a cascade configuration (previous_stage {cfg['previous_stage']!r}) needs seg_from_prev_stage: "
                                  "the previous stage's segmentation of this case in the original geometry is missing")
    if seg_from_prev_stage is None:
        return None
    if not cfg.get("previous_stage"):
        raise RuntimeError("seg_from_prev_stage was given, but the configuration has no previous_stage: it is no cascaded stage")
    seg = seg_from_prev_stage
    if seg.ndim == 3:
        seg = seg[None]
    if seg.ndim != 4 or seg.shape[0] != 1 or tuple(seg.shape[1:]) != tuple(image.shape[1:]):
        raise RuntimeError(f"preprocess_case: a (x, y, z) or (1, x, y, z) seg_from_prev_stage matching the image {tuple(image.shape)} "
                           f"expected, got {tuple(seg_from_prev_stage.shape)}")
    return seg


def preprocess_case(image, properties, plans, configuration_name, device=None, seg_from_prev_stage=None, dataset_json=None):
    """DefaultPreprocessor.run_case for a test case: image (c, x, y, z) (numpy or tensor; cast to float32 as the reader delivers
    it), properties (the reader's, with 'spacing'), plans (the plans.json dict) -> (data (c, x', y', z') float32, a new properties
    dict with shape_before_cropping, bbox_used_for_cropping and shape_after_cropping_and_before_resampling).  A CUDA `device` (or a
    device tensor when device is None) runs K22 and returns a device tensor; otherwise the host path returns a numpy array.

    A cascaded configuration (previous_stage) takes seg_from_prev_stage, the previous stage's (x, y, z) or (1, x, y, z) label
    volume in the ORIGINAL geometry (what predict_case of that stage returns), as run_case's seg (predict_from_raw_data.py:47-67):
    transposed, cropped with the image's box (-1 outside the filled non-zero mask) and resampled as preprocess_training_case treats
    a segmentation (K26 on the device); the masked ZScore takes seg >= 0 as its mask.  No class locations are sampled.
    -> (data, seg (1, x', y', z') int8, or int16 with a label above 127, props).  dataset_json (its 'labels'; required on the
    device): region-based labels are refused, and on the device labels outside -1 .. its largest label are."""
    cfg, dev, schemes, masks, fg, props, original_spacing, perm = _case_setup(image, properties, plans, configuration_name, device,
                                                                              "preprocess_case")
    order, order_z, force_separate_z, threshold = _data_resampling_kwargs(cfg)
    max_label = None
    if seg_from_prev_stage is not None or cfg.get("previous_stage"):
        _, _, seg_force_separate_z, seg_threshold = _seg_resampling_kwargs(cfg)
        if dataset_json is not None:
            max_label = _label_lists(dataset_json)[1]              # refuses region-based labels
    s = _check_previous_stage(cfg, seg_from_prev_stage, image)
    if s is not None and dev is not None and max_label is None:
        raise RuntimeError("preprocess_case: seg_from_prev_stage on the device needs dataset_json: its largest label bounds K26's tables")
    if dev is not None:
        x = torch.as_tensor(image).to(device=dev, dtype=torch.float32).permute(perm)
        props["shape_before_cropping"] = tuple(int(v) for v in x.shape[1:])
        if s is None:
            data, bbox = _preprocess_device(x, schemes, masks, fg, dev)
        else:
            s = _as_label_tensor(s, dev).permute(perm)
            data, bbox, s, hist = _preprocess_device(x, schemes, masks, fg, dev, s[0], max_label)
            s = s[None]
    else:
        x = image.cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
        x = np.array(x, dtype=np.float32).transpose(perm)
        props["shape_before_cropping"] = x.shape[1:]
        if s is not None:
            s = s.cpu().numpy() if isinstance(s, torch.Tensor) else np.asarray(s)
            s = np.array(s, dtype=np.int16 if s.dtype.kind in "ub" else s.dtype).transpose(perm)      # -1 needs a signed dtype
        data, seg, bbox = crop_to_nonzero(x, s)                 # seg: the cropped s, or the non-zero mask's stand-in without one
        data = np.array(data)
        for c in range(data.shape[0]):
            data[c] = _normalize_channel_host(data[c], seg[0], schemes[c], masks[c], fg.get(str(c), {}))
        if s is not None:
            s = seg
    props["bbox_used_for_cropping"] = bbox
    props["shape_after_cropping_and_before_resampling"] = tuple(int(v) for v in data.shape[1:])
    target, new_shape = _target_shape(cfg, data.shape[1:], original_spacing)
    old_shape = tuple(int(v) for v in data.shape[1:])
    data = resample_data_to_shape(data, new_shape, original_spacing, target, order, order_z, force_separate_z, threshold)
    if s is None:
        return data, props
    sep, axis = separate_z_decision(original_spacing, target, seg_force_separate_z, seg_threshold)
    s, hist = _resample_case_seg(s, old_shape, new_shape, sep, axis, hist if dev is not None else None, max_label,
                                 "preprocess_case")
    return data, _narrow_seg(s, hist), props


# ------------------------------------------------------------------------------------------------
# training cases: the segmentation, class locations, the case folder (K26 on the device)
# ------------------------------------------------------------------------------------------------
def _seg_resampling_kwargs(cfg):
    name = cfg.get("resampling_fn_seg", "resample_data_or_seg_to_shape")
    if name != "resample_data_or_seg_to_shape":
        raise NotImplementedError(f"segmentation resampling function {name}: only resample_data_or_seg_to_shape is implemented")
    kw = dict(cfg.get("resampling_fn_seg_kwargs") or {"is_seg": True, "order": 1, "order_z": 0, "force_separate_z": None})
    if not kw.get("is_seg", False):
        raise NotImplementedError("the segmentation resampler must be a segmentation resampler (is_seg)")
    order, order_z = kw.get("order", 3), kw.get("order_z", 0)
    _check_seg_orders(order, order_z)
    return order, order_z, kw.get("force_separate_z", None), kw.get("separate_z_anisotropy_threshold", ANISO_THRESHOLD)


def _check_seg_orders(order, order_z):
    if order != 1 or order_z != 0:
        raise NotImplementedError(f"segmentation resampling of order {order} / order_z {order_z}: only order 1 with order_z 0 "
                                  "(the planner's default) is implemented")


def _label_lists(dataset_json):
    """(what run_case collects class locations for, in its order: the foreground labels and, with an ignore label, the list of all
    labels; the largest label value the dataset declares) -- LabelManager.foreground_labels / all_labels for label-based datasets."""
    labels = dataset_json["labels"]
    if "regions_class_order" in dataset_json or any(isinstance(v, (list, tuple)) and len(v) > 1 for v in labels.values()):
        raise NotImplementedError("region-based labels (regions_class_order or multi-value labels) are not supported")
    value = {k: int(v[0] if isinstance(v, (list, tuple)) else v) for k, v in labels.items()}
    if value.get("background") != 0:
        raise RuntimeError("dataset_json['labels'] must declare 'background': 0")
    all_labels = sorted({v for k, v in value.items() if k != "ignore"})
    collect = [v for v in all_labels if v != 0]
    if "ignore" in value:
        collect.append(list(all_labels))
    return collect, max(value.values())


def _resize_segmentation_host(seg, new_shape, near=None):
    """batchgenerators' resize_segmentation(order=1) on skimage's resize(mode='edge', anti_aliasing=False): per label in ascending
    order, the indicator zoomed linearly (ndi.zoom(grid_mode=True, mode='nearest'), clipped to its range) and written where it is
    >= 0.5.  near (bool, new_shape): set where an indicator is within NEAR_TIE of 0.5."""
    out = np.zeros(new_shape, dtype=seg.dtype)
    zoom = np.asarray(new_shape, float) / np.asarray(seg.shape, float)
    for c in np.unique(seg):
        ind = (seg == c).astype(float)
        v = np.clip(ndi.zoom(ind, zoom, order=1, mode="nearest", grid_mode=True), ind.min(), ind.max())
        out[v >= 0.5] = c
        if near is not None:
            near |= np.abs(v - 0.5) <= NEAR_TIE
    return out


def _resample_seg_host(seg, new_shape, sep, axis, near_tie=False):
    """resample_data_or_seg (default_resampling.py:122-212) for a segmentation of order 1 / order_z 0: seg (c, x, y, z) of any
    integer-valued dtype -> (c, *new_shape) of the same dtype; with near_tie also the bool near-tie mask of the same shape."""
    shape = np.array(seg.shape[1:])
    new_shape = np.array([int(s) for s in new_shape])
    data = seg.astype(float)
    out, nears = [], []
    for c in range(data.shape[0]):
        if sep:
            plane = [a for a in range(3) if a != axis]
            near = [np.zeros(tuple(new_shape[plane]), dtype=bool) if near_tie else None for _ in range(shape[axis])]
            r = np.stack([_resize_segmentation_host(np.take(data[c], i, axis), tuple(new_shape[plane]), near[i])
                          for i in range(shape[axis])], axis)
            n = np.stack(near, axis) if near_tie else None
            if shape[axis] != new_shape[axis]:
                # map_coordinates(order=0, mode='nearest') with the in-plane coordinates on the grid: a pick along the axis alone
                idx, _ = _axis_taps(int(shape[axis]), int(new_shape[axis]), "nearest")
                r = np.take(r, idx[:, 0], axis)
                n = np.take(n, idx[:, 0], axis) if near_tie else None
        else:
            n = np.zeros(tuple(new_shape), dtype=bool) if near_tie else None
            r = _resize_segmentation_host(data[c], tuple(new_shape), n)
        out.append(r[None])
        nears.append(n[None] if near_tie else None)
    out = np.vstack(out).astype(seg.dtype)
    return (out, np.vstack(nears)) if near_tie else out


def _seg_taps(shape, new_shape, sep, axis):
    """The stacked export._axis_taps tables of K26's resize: linear on every zoomed axis, the order-0 pick on the low-resolution
    axis of a separate-z case."""
    tabs = []
    for a in range(3):
        kind = "linear"
        if sep and a == axis:
            kind = "nearest" if shape[a] != new_shape[a] else "identity"
        tabs.append(_axis_taps(int(shape[a]), int(new_shape[a]), kind))
    return np.concatenate([t[0] for t in tabs]), np.concatenate([t[1] for t in tabs])


def _as_label_tensor(seg, device=None):
    """Whatever integer-valued dtype the reader delivered -> an int16 tensor (on `device` when given)."""
    t = torch.as_tensor(np.ascontiguousarray(seg) if isinstance(seg, np.ndarray) else seg)
    if device is not None:
        t = t.to(device)
    return t if t.dtype == torch.int16 else t.to(torch.int16)


def _resample_seg_device(seg, new_shape, sep, axis, max_label):
    """seg (c, X, Y, Z) int16 on the device -> ((c, *new_shape) int16, the label histogram of the last channel's result)."""
    from . import ops
    shape = tuple(int(s) for s in seg.shape[1:])
    new_shape = tuple(int(s) for s in new_shape)
    taps = _seg_taps(shape, new_shape, sep, axis)
    outs = [ops.pp_seg_resize(seg[c].contiguous(), taps, new_shape, max_label) for c in range(seg.shape[0])]
    return torch.stack([o for o, _ in outs]), outs[-1][1]


def resample_seg_to_shape(seg, new_shape, current_spacing, new_spacing, order=1, order_z=0, force_separate_z=None,
                          separate_z_anisotropy_threshold=ANISO_THRESHOLD):
    """resample_data_or_seg_to_shape(is_seg=True) (default_resampling.py:76-212) for order 1 / order_z 0: seg (c, x, y, z) of labels
    -> (c, *new_shape) with the input's dtype.  A device tensor runs K26 (int16 arithmetic: labels -32768 .. 32767), anything else the
    host path.  As in the reference, a segmentation that already has new_shape is returned unchanged."""
    _check_seg_orders(order, order_z)
    in_shape, new_shape = tuple(int(s) for s in seg.shape[1:]), tuple(int(s) for s in new_shape)
    if len(in_shape) != 3 or len(new_shape) != 3 or min(new_shape) < 1:
        raise RuntimeError(f"resampling needs three non-empty spatial axes, got {in_shape} -> {new_shape}")
    sep, axis = separate_z_decision(current_spacing, new_spacing, force_separate_z, separate_z_anisotropy_threshold)
    if in_shape == new_shape:
        return seg
    if isinstance(seg, torch.Tensor) and seg.is_cuda:
        lo, hi = (int(v) for v in torch.aminmax(seg))
        if lo < -1 or hi > 32767:
            raise RuntimeError(f"resample_seg_to_shape: labels {lo} .. {hi}; -1 .. 32767 are supported on the device")
        out, _ = _resample_seg_device(_as_label_tensor(seg), new_shape, sep, axis, max(hi, 0))
        return out.to(seg.dtype)
    if isinstance(seg, torch.Tensor):
        seg = seg.numpy()
    return _resample_seg_host(np.asarray(seg), new_shape, sep, axis)


def _resample_case_seg(s, old_shape, new_shape, sep, axis, hist=None, max_label=None, what=None):
    """A case's cropped segmentation (1, x, y, z) -> (the segmentation at new_shape, its label histogram on the host or None).  With
    hist (the device path: K26's histogram of the crop) the labels are checked against -1 .. max_label on the way: the histogram's
    read-back is the case's second and last."""
    resize = tuple(int(v) for v in old_shape) != tuple(int(v) for v in new_shape)
    if hist is None:
        return (_resample_seg_host(s, new_shape, sep, axis) if resize else s), None
    if resize:
        foreign = hist[-1:]                                # a label outside the dataset's range may vanish in the resampling
        s, hist = _resample_seg_device(s, new_shape, sep, axis, max_label)
        hist[-1:] += foreign
    hist = hist.cpu().numpy()
    if hist[-1]:
        raise RuntimeError(f"{what}: {int(hist[-1])} voxels carry a label outside -1 .. {max_label}, the largest label of dataset_json")
    return s, hist


def _narrow_seg(s, hist=None):
    """run_case's last step (:120-123): int16 when a label above 127 is present, else int8; hist: the device path's histogram."""
    if hist is None:
        return s.astype(np.int16 if np.max(s) > 127 else np.int8)
    present = np.flatnonzero(hist[:-1])
    return s.to(torch.int16 if present.size and present[-1] - 1 > 127 else torch.int8)


def _num_to_sample(n):
    """_sample_foreground_locations: at most 10000 voxels of a class, but at least 1 % of them."""
    return max(min(10000, n), int(np.ceil(n * 0.01)))


def _sample_locations_host(seg, classes_or_regions, seed):
    rndst = np.random.RandomState(seed)
    locs = {}
    for c in classes_or_regions:
        k = tuple(c) if isinstance(c, (tuple, list)) else c
        all_locs = np.argwhere(np.isin(seg, list(c)) if isinstance(c, (tuple, list)) else seg == c)
        if len(all_locs) == 0:
            locs[k] = []
            continue
        locs[k] = all_locs[rndst.choice(len(all_locs), _num_to_sample(len(all_locs)), replace=False)]
    return locs


def _sample_locations_device(seg, classes_or_regions, seed, max_label, hist=None):
    """seg (1, X, Y, Z) int16 on the device.  The voxel counts come from hist (the host copy of a K26 label histogram) when given,
    else from the rank table's totals (one read-back); the draws stay on the host, K26 turns the drawn ranks into coordinates."""
    from . import ops
    if seg.dim() != 4 or seg.shape[0] != 1:
        raise RuntimeError(f"sample_foreground_locations: a (1, x, y, z) segmentation expected, got {tuple(seg.shape)}")
    vol = seg[0].contiguous()
    rndst = np.random.RandomState(seed)
    groups = [[int(v) for v in c] if isinstance(c, (tuple, list)) else [int(c)] for c in classes_or_regions]
    keys = [tuple(c) if isinstance(c, (tuple, list)) else c for c in classes_or_regions]
    locs, pending = {}, []
    for g0 in range(0, len(groups), ops.PP_MAX_GROUPS):
        part = groups[g0:g0 + ops.PP_MAX_GROUPS]
        table = ops.pp_group_table(part, max_label, vol.device)
        counts = ops.pp_rank_counts(vol, table, len(part), max_label)
        if hist is not None:
            n_vox = [int(sum(hist[v + 1] for v in set(g) if -1 <= v <= max_label)) for g in part]
        else:
            n_vox = [int(v) for v in counts[1].cpu()]
        for g, n in enumerate(n_vox):
            key = keys[g0 + g]
            if n == 0:
                locs[key] = []
                continue
            ranks = torch.from_numpy(rndst.choice(n, _num_to_sample(n), replace=False).astype(np.int64)).to(vol.device)
            locs[key] = None
            pending.append((key, ops.pp_rank_select(vol, table, max_label, counts, g, ranks)[0]))
    if pending:
        host = torch.cat([c for _, c in pending]).cpu().numpy()
        at = 0
        for key, c in pending:
            locs[key] = host[at:at + c.shape[0]]
            at += c.shape[0]
        if host.min() < 0:
            raise RuntimeError("sample_foreground_locations: the voxel counts do not match the segmentation")
    return locs


def sample_foreground_locations(seg, classes_or_regions, seed=1234):
    """DefaultPreprocessor._sample_foreground_locations (:134-161): per class (an int) or region (a tuple / list of labels), in the
    given order, rndst.choice(n, max(min(10000, n), ceil(0.01 n)), replace=False) of its n voxels in C order -> {class or tuple:
    int64 array (k, 4) of (0, x, y, z) in draw order, or [] for an absent class}.  seg (1, x, y, z): a device tensor (int8 /
    int16 / any integer dtype with labels in -1 .. 32767) runs K26's rank select, a numpy array the reference's arithmetic."""
    if isinstance(seg, torch.Tensor) and seg.is_cuda:
        flat = [int(v) for c in classes_or_regions for v in (c if isinstance(c, (tuple, list)) else (c,))]
        return _sample_locations_device(_as_label_tensor(seg), classes_or_regions, seed, max([0] + flat))
    if isinstance(seg, torch.Tensor):
        seg = seg.numpy()
    return _sample_locations_host(np.asarray(seg), classes_or_regions, seed)


def preprocess_training_case(image, seg, properties, plans, configuration_name, dataset_json, device=None):
    """DefaultPreprocessor.run_case with a segmentation: image (c, x, y, z) and seg (1, x, y, z) (numpy or tensors, as the reader
    delivers them; seg of any integer-valued dtype), properties (the reader's, with 'spacing'), plans, dataset_json (its 'labels')
    -> (data (c, x', y', z') float32, seg (1, x', y', z') int8, or int16 when a label above 127 is present, a new properties dict
    with the three geometry entries of preprocess_case and class_locations: {label: int64 (k, 4) array of (0, x, y, z), or [] for a
    class absent from the case}, with the tuple of all labels as one more key when the dataset has an ignore label).
    A CUDA `device` (or device tensors when device is None) runs K22 + K26 and returns device tensors for data and seg; otherwise
    the host path returns numpy arrays.  class_locations are host arrays either way: the loader indexes them on the host.  On the
    device, labels outside -1 .. the dataset's largest label are refused (RuntimeError)."""
    cfg, dev, schemes, masks, fg, props, original_spacing, perm = _case_setup(image, properties, plans, configuration_name, device,
                                                                              "preprocess_training_case")
    order, order_z, force_separate_z, threshold = _data_resampling_kwargs(cfg)
    _, _, seg_force_separate_z, seg_threshold = _seg_resampling_kwargs(cfg)
    if cfg.get("previous_stage"):
        raise NotImplementedError("training cases of cascade configurations (previous_stage) are not supported")
    collect, max_label = _label_lists(dataset_json)
    if seg.ndim != 4 or seg.shape[0] != 1 or tuple(seg.shape[1:]) != tuple(image.shape[1:]):
        raise RuntimeError(f"preprocess_training_case: a (1, x, y, z) segmentation matching the image {tuple(image.shape)} expected, "
                           f"got {tuple(seg.shape)}")
    if dev is not None:
        x = torch.as_tensor(image).to(device=dev, dtype=torch.float32).permute(perm)
        s = _as_label_tensor(seg, dev).permute(perm)
        props["shape_before_cropping"] = tuple(int(v) for v in x.shape[1:])
        data, bbox, s, hist = _preprocess_device(x, schemes, masks, fg, dev, s[0], max_label)
        s = s[None]
    else:
        x = image.cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
        x = np.array(x, dtype=np.float32).transpose(perm)
        s = seg.cpu().numpy() if isinstance(seg, torch.Tensor) else np.asarray(seg)
        s = np.array(s, dtype=np.int16 if s.dtype.kind in "ub" else s.dtype).transpose(perm)      # -1 needs a signed dtype
        props["shape_before_cropping"] = x.shape[1:]
        data, s, bbox = crop_to_nonzero(x, s)
        data = np.array(data)
        for c in range(data.shape[0]):
            data[c] = _normalize_channel_host(data[c], s[0], schemes[c], masks[c], fg.get(str(c), {}))
    props["bbox_used_for_cropping"] = bbox
    props["shape_after_cropping_and_before_resampling"] = tuple(int(v) for v in data.shape[1:])
    target, new_shape = _target_shape(cfg, data.shape[1:], original_spacing)
    old_shape = tuple(int(v) for v in data.shape[1:])
    data = resample_data_to_shape(data, new_shape, original_spacing, target, order, order_z, force_separate_z, threshold)
    sep, axis = separate_z_decision(original_spacing, target, seg_force_separate_z, seg_threshold)
    if dev is not None:
        s, hist = _resample_case_seg(s, old_shape, new_shape, sep, axis, hist, max_label, "preprocess_training_case")
        props["class_locations"] = _sample_locations_device(s, collect, 1234, max_label, hist)
    else:
        s, hist = _resample_case_seg(s, old_shape, new_shape, sep, axis)
        props["class_locations"] = _sample_locations_host(s, collect, 1234)
    return data, _narrow_seg(s, hist), props


def preprocess_dataset(cases, output_folder, plans, configuration_name, dataset_json, device=None, unpack=False):
    """The per-case work of the reference's preprocessing run (run_case_save, :126-132): cases is an iterable of (identifier,
    image, seg, properties); every case goes through preprocess_training_case and is written as <identifier>.npz ('data', 'seg',
    np.savez_compressed) and <identifier>.pkl (the properties with class_locations) into output_folder, the folder
    dataloading.Dataset reads.  unpack=True also writes <identifier>.npy / <identifier>_seg.npy, which Dataset.arrays memory-maps.
    -> the identifiers written, in order."""
    os.makedirs(output_folder, exist_ok=True)
    done = []
    for identifier, image, seg, properties in cases:
        data, s, props = preprocess_training_case(image, seg, properties, plans, configuration_name, dataset_json, device)
        if isinstance(data, torch.Tensor):
            data, s = data.cpu().numpy(), s.cpu().numpy()
        base = os.path.join(output_folder, identifier)
        np.savez_compressed(base + ".npz", data=data, seg=s)
        with open(base + ".pkl", "wb") as fh:
            pickle.dump(props, fh)
        if unpack:
            np.save(base + ".npy", data)
            np.save(base + "_seg.npy", s)
        done.append(identifier)
    return done
