"""Case preprocessing for prediction (the preprocessing part): the reference's DefaultPreprocessor.run_case
(mlagg/nnunetv2/preprocessing/preprocessors/default_preprocessor.py:38-124) for a test case (no segmentation), with the default
plans: transpose by transpose_forward, crop to the non-zero box, normalise every channel, resample to the configuration's spacing
with resample_data_or_seg_to_shape(order=3, order_z=0, force_separate_z=None) (default_experiment_planner.py:123-128).

A CUDA device runs K22 (csrc/preprocess.hip): the box of the non-zero voxels (one read-back of 6 ints), crop + normalisation in
fp32, and the cubic zoom one axis at a time in fp64 (prefilter and 4-tap evaluation per line, tap tables from _cubic_taps), clipped
to each resize call's input range and rounded once to fp32.  Anything else runs the reference's arithmetic on the host with numpy
and scipy (binary_fill_holes, ndi.zoom + clip): the CPU path and the A/B side of tools/bench_preprocess.py.

Parity (tests/test_preprocess_*.py against tests/golden/preprocess.npz, made by the reference's own run_case): the host path is
bit-identical; on the device, CT / RescaleTo01 / RGB / unnormalised channels agree to 1 fp32 ulp on at most 1e-4 of the voxels
(the separable fp64 zoom differs from scipy's 3-D one only by its summation order), and ZScore channels to the rounding of numpy's
fp32 mean / std (ZSCORE_TOLERANCE), since the device sums in fp64.

Not supported (NotImplementedError): training cases (seg_file, class_locations), cascade stages, region-based labels, preprocessors
other than DefaultPreprocessor, data resamplers other than resample_data_or_seg_to_shape with order 3 and order_z 0 or 1.
File reading is the caller's: the input is the reader's (c, x, y, z) array and its properties (at least 'spacing').
"""
import copy

import numpy as np
import scipy.ndimage as ndi
import torch

from .export import ANISO_THRESHOLD, _axis_taps, separate_z_decision

SCHEMES = ("NoNormalization", "CTNormalization", "ZScoreNormalization", "RescaleTo01Normalization", "RGBTo01Normalization")
# |device - host| of a ZScore channel: numpy's fp32 pairwise mean / std against the device's fp64 ones, a few fp32 ulps of the
# statistics relative to the normalised value and to mean / std (tests/test_preprocess_gpu.py)
ZSCORE_TOLERANCE = 2e-6

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
    if cfg.get("previous_stage"):
        raise NotImplementedError("cascade configurations (previous_stage) are not supported")
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


def _preprocess_device(view, schemes, masks, fg, device):
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
    mask = _filled_mask_device(view, lo, ext) if ops.PP_SCHEMES["ZScoreNormalization+mask"] in codes else None
    for c, code in enumerate(codes):
        if code in (2, 3, 4, 5):
            ops.pp_channel_stats(view, lo, ext, c, code, d_params, stats, mask)
    if 5 in codes:
        mm = stats.cpu().numpy()
        for c, code in enumerate(codes):
            if code == 5 and (mm[c, 2] < 0 or mm[c, 3] > 255):
                raise RuntimeError("RGBTo01Normalization: values outside [0, 255]; the image does not seem to be RGB")
    data = ops.pp_normalize(view, lo, ext, torch.tensor(codes, dtype=torch.int32, device=device), d_params, mask)
    return data, bbox


def preprocess_case(image, properties, plans, configuration_name, device=None):
    """DefaultPreprocessor.run_case for a test case: image (c, x, y, z) (numpy or tensor; cast to float32 as the reader delivers
    it), properties (the reader's, with 'spacing'), plans (the plans.json dict) -> (data (c, x', y', z') float32, a new properties
    dict with shape_before_cropping, bbox_used_for_cropping and shape_after_cropping_and_before_resampling).  A CUDA `device` (or a
    device tensor when device is None) runs K22 and returns a device tensor; otherwise the host path returns a numpy array."""
    cfg = get_configuration(plans, configuration_name)
    if isinstance(image, torch.Tensor):
        on_device = image.is_cuda if device is None else torch.device(device).type == "cuda"
    else:
        on_device = device is not None and torch.device(device).type == "cuda"
    if image.ndim != 4 or min(image.shape) < 1:
        raise RuntimeError(f"preprocess_case: expected a non-empty (c, x, y, z) image, got shape {tuple(image.shape)}")
    schemes, masks = _check_configuration(cfg, int(image.shape[0]))
    order, order_z, force_separate_z, threshold = _data_resampling_kwargs(cfg)
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
    if on_device:
        dev = torch.device(device) if device is not None else image.device
        x = torch.as_tensor(image).to(device=dev, dtype=torch.float32).permute(perm)
        props["shape_before_cropping"] = tuple(int(s) for s in x.shape[1:])
        data, bbox = _preprocess_device(x, schemes, masks, fg, dev)
    else:
        x = image.cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
        x = np.array(x, dtype=np.float32).transpose(perm)
        props["shape_before_cropping"] = x.shape[1:]
        data, seg, bbox = crop_to_nonzero(x)
        data = np.array(data)
        for c in range(data.shape[0]):
            data[c] = _normalize_channel_host(data[c], seg[0], schemes[c], masks[c], fg.get(str(c), {}))
    props["bbox_used_for_cropping"] = bbox
    props["shape_after_cropping_and_before_resampling"] = tuple(int(s) for s in data.shape[1:])
    target = [float(s) for s in cfg["spacing"]]
    if len(target) < 3:
        target = [original_spacing[0]] + target
    new_shape = compute_new_shape(data.shape[1:], original_spacing, target)
    data = resample_data_to_shape(data, new_shape, original_spacing, target, order, order_z, force_separate_z, threshold)
    return data, props
