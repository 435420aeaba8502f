"""Training-time data augmentation of the 3-D path ON the MI355X: the reference's get_training_transforms
(nnUNetTrainer.py:645-733) for a 3-D configuration, without dummy-2-D augmentation (the BTCV plan: 160 / 96 < ANISO_THRESHOLD 3) and
with it (thick-slice plans such as ACDC's 20 x 256 x 224), behind `dataloading.DataLoader3D`.

Parameters are drawn on the host in batchgenerators' 3-D order (`draw_params_3d`); the voxels stay on the device:
  * SpatialTransform (rotation of +-30 degrees about x, y and z, p_rot_per_axis 1; isotropic scale in (0.7, 1.4); p 0.2 each):
    K25 (csrc/augment3d.hip, ops.aug3d_resample) evaluates the cubic B-spline of the prefiltered data (64 taps, mirror-indexed,
    cval 0 outside) and the per-label trilinear indicators of the int16 loader labels (largest label >= 0.5 wins, 0 where none
    does) in one pass; samples that neither rotate nor scale are the exact centre crop.  The prefilter is the 33-tap band matrix
    of augmentation.spline_coefficients applied along each axis (library GEMMs).
  * GaussianBlur: band matrices along the three axes, one sigma per (sample, channel), scipy's "reflect" boundary.
  * SimulateLowResolution: nearest-exact down-sampling, 12-voxel edge padding, prefilter, K25 with a diagonal affine on the
    half-pixel grid, clip to the small image's range.
  * Noise, brightness, contrast, both gammas (reductions over the three spatial axes) and mirroring on (0, 1, 2): torch.
  * The cascade transforms of a 3d_cascade_fullres configuration (B:703-718, `GpuAugmenter3D(cascade_labels=...)`): the previous
    stage's segmentation travels as a second seg channel through the spatial transform and the mirroring, then K30
    (csrc/cascade_aug.hip) packs its one-hot channels into bit planes, applies the drawn binary morphology with skimage's ball
    footprints and the "was added" rule, removes the drawn connected components and writes the planes as fp32 input channels.
  * Dummy-2-D augmentation (`GpuAugmenter3D(dummy_2d=True)`, chosen by `configure_3d` / `GpuAugmenter3D.for_plan` when
    max(patch) / patch[0] > 3, B:380): the 2-D draws (`draw_params_dummy_2d`, one angle in +-180 degrees), the loader patch keeps
    patch[0], the spatial transform resamples every slice in its own plane -- prefilter along Y and Z only, then K31
    (csrc/augment3d.hip, ops.aug3d_resample_planar: 16 cubic taps, 4 bilinear label taps, X never resampled) -- and
    SimulateLowResolution ignores axis 0 (in-plane sizes, padding and prefilter, K31 for the up-sampling, the clip still to the
    small VOLUME's range).  Everything after the spatial transform is 3-D again and shared with the isotropic mode.
CPU tensors take a torch composition of the same arithmetic (augmentation.resample on the float64 coordinates of `affine_coords`;
scipy.ndimage for the cascade transforms), for tests at small sizes.  The sampler, the prefilter, the blur, the parameter table and
the draws are the 2-D module's: they take the number of axes.

Out of scope: the region / mask transforms (B:697-699, B:722-726), as in the 2-D augmenter.
"""
import math

import numpy as np
import torch

from . import augmentation as A2
from .augmentation import contrast_transform, gamma_transform, gaussian_blur, get_patch_size, mirror_transform
from .export import ANISO_THRESHOLD


def rotation_for_3d(patch_size):
    """configure_rotation_dummyDA_mirroring_and_inital_patch_size (B:378-393), 3-D branch without dummy-2-D augmentation:
    +-30 degrees about each axis."""
    if max(patch_size) / patch_size[0] > ANISO_THRESHOLD:
        raise NotImplementedError(f"patch {tuple(patch_size)}: max(patch) / patch[0] > {ANISO_THRESHOLD} selects dummy-2-D "
                                  "augmentation, which the 3-D augmenter does not implement")
    r = 30.0 / 360 * 2.0 * math.pi
    return ((-r, r),) * 3


def draw_params_3d(rng, batch, channels, rotation=None, mirror_axes=(0, 1, 2)):
    """draw_params with batchgenerators' 3-D order: per sample, when rotation fires, a_x, a_y, a_z each behind its own
    uniform() <= p_rot_per_axis (1), then the scale; the intensity transforms and mirroring (three flags) as in 2-D.
    p["angle"] is (B, 3): the angles about x, y, z."""
    p = A2._param_table(batch, channels, 3, 3)
    A2._draw_spatial(rng, p, (rotation_for_3d((1, 1, 1)) if rotation is None else rotation)[:3])
    return A2._draw_intensity_and_mirror(rng, p, batch, channels, mirror_axes)


def configure_3d(patch_size):
    """configure_rotation_dummyDA_mirroring_and_inital_patch_size (B:378-404), 3-D branch, both cases:
    (rotation ranges about x, y, z; do_dummy_2d; the loader's initial patch size; mirror axes)."""
    patch_size = tuple(int(v) for v in patch_size)
    if len(patch_size) != 3:
        raise RuntimeError(f"configure_3d: a 3-D patch, got {patch_size}")
    do_dummy_2d = max(patch_size) / patch_size[0] > ANISO_THRESHOLD
    rotation = ((-math.pi, math.pi), (0, 0), (0, 0)) if do_dummy_2d else rotation_for_3d(patch_size)
    initial = [int(v) for v in get_patch_size(patch_size, *rotation, (0.85, 1.25))]
    if do_dummy_2d:
        initial[0] = patch_size[0]
    return rotation, do_dummy_2d, tuple(initial), (0, 1, 2)


def draw_params_dummy_2d(rng, batch, channels, rotation=(-math.pi, math.pi), mirror_axes=(0, 1, 2)):
    """The draws of the dummy-2-D chain: SpatialTransform sees (B, C * X, Y, Z), so per sample batchgenerators' 2-D order (one
    angle behind its uniform() <= p_rot_per_axis, then the scale: augmentation.draw_params' spatial part); after Convert2DTo3D the
    intensity transforms draw per channel over C (not C * X) and the mirroring draws three flags.  p["angle"] is (B,)."""
    p = A2._param_table(batch, channels, 0, 3)
    A2._draw_spatial(rng, p, (rotation,))
    return A2._draw_intensity_and_mirror(rng, p, batch, channels, mirror_axes)


def rotation_matrix(ax, ay, az):
    """rotate_coords_3d's matrix I . Rx . Ry . Rz (float64); coordinates are rotated as coords^T . M."""
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.identity(3) @ Rx @ Ry @ Rz


def affines(p, in_shape, out_shape):
    """Per sample the (nd, nd + 1) float64 map output index -> input coordinate of augment_spatial over nd = len(out_shape) axes:
    zero-centred mesh, rotated, scaled, moved to the input centre (in / 2 - 0.5); and whether the sample is resampled at all
    (else: centre crop).  p["angle"] (B, 3): `rotation_matrix` about x, y, z.  p["angle"] (B,): the 2-D transform that every
    slice of a dummy-2-D sample goes through, coords^T . [[cos, -sin], [sin, cos]] over (y, z)."""
    B, nd = len(p["do_rot"]), len(out_shape)
    A = np.zeros((B, nd, nd + 1))
    do = np.asarray(p["do_rot"]) | np.asarray(p["do_scale"])
    half = (np.asarray(out_shape, dtype=np.float64) - 1) / 2.0
    three = np.ndim(p["angle"]) == 2
    for b in range(B):
        if three:
            M = rotation_matrix(*p["angle"][b]) if p["do_rot"][b] else np.identity(3)
        else:
            cos, sin = (math.cos(p["angle"][b]), math.sin(p["angle"][b])) if p["do_rot"][b] else (1.0, 0.0)
            M = np.array([[cos, -sin], [sin, cos]])
        L = (M * (p["scale"][b] if p["do_scale"][b] else 1.0)).T               # input_j = sum_i L[j, i] centred_i
        A[b, :, :nd] = L
        A[b, :, nd] = np.asarray(in_shape, dtype=np.float64) / 2.0 - 0.5 - L @ half
    return A, do


def affine_coords(A, out_shape, device):
    """A (B, nd, nd + 1) float64 applied to the output index grid -> the float64 coordinates (B, nd, *out_shape) that
    augmentation.sample takes on the host and K25 / K31 form on the device."""
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64, device=device) for n in out_shape], indexing="ij"))
    At = torch.as_tensor(A, dtype=torch.float64, device=device)
    nd = len(out_shape)
    coords = torch.einsum("bji,ip->bjp", At[:, :, :nd], grid.reshape(nd, -1)) + At[:, :, nd:]     # (B, nd, P)
    return coords.view(len(At), nd, *out_shape)


# ------------------------------------------------------------------------------------------------
# transforms
# ------------------------------------------------------------------------------------------------
def _prefiltered(data, do, nd=3):
    """The resampler's input volume: spline coefficients (along the last nd axes) of the samples in `do`, the data itself for
    the others."""
    idx = np.flatnonzero(do)
    if len(idx) == len(do):
        return A2.spline_coefficients(data, nd).contiguous()
    vol = data.clone()
    if len(idx):
        sel = torch.as_tensor(idx, device=data.device)
        vol[sel] = A2.spline_coefficients(data[sel], nd)
    return vol


def _spatial(data, seg, out_shape, p, labels, nd):
    """The spatial transform over the last nd axes of (B, C, X, Y, Z): K25 (nd 3) or K31 (nd 2) on the device, a further seg
    channel by a call without a volume (the labels only); augmentation.resample on the host."""
    in_nd, out_nd = tuple(data.shape[-nd:]), out_shape[-nd:]
    A, do = affines(p, in_nd, out_nd)
    vol = _prefiltered(data.contiguous(), do, nd)
    if not data.is_cuda:
        keep = None if do.all() else torch.as_tensor(do)
        return A2.resample(vol, data, seg.to(torch.float32), affine_coords(A, out_nd, data.device), keep, labels)
    from . import ops
    kernel = ops.aug3d_resample if nd == 3 else ops.aug3d_resample_planar
    if seg.shape[1] == 1:
        return kernel(vol, seg.to(torch.int16).contiguous(), A, do, out_nd)
    segs = [s.to(torch.int16).contiguous() for s in seg.split(1, 1)]
    out_d, first = kernel(vol, segs[0], A, do, out_nd)
    return out_d, torch.cat([first] + [kernel(None, s, A, do, out_nd)[1] for s in segs[1:]], 1)


def spatial_transform_3d(data, seg, patch_size, p, labels=None):
    """augment_spatial, 3-D, with the nnU-Net arguments: data (B, C, Xi, Yi, Zi) fp32, seg (B, S, Xi, Yi, Zi) (int16 on the
    device path; any integral-valued type on the host) -> (B, C, *patch) fp32 and (B, S, *patch) fp32 labels.  Every seg channel
    is resampled with the same affines and the same indicator rule (`labels` names the values of channel 0 on the host path)."""
    return _spatial(data, seg, tuple(int(v) for v in patch_size), p, labels, 3)


def spatial_transform_dummy_2d(data, seg, patch_size, p, labels=None):
    """Convert3DTo2DTransform, the 2-D augment_spatial with the nnU-Net arguments and Convert2DTo3DTransform (B:658-680): data
    (B, C, X, Yi, Zi) fp32, seg (B, S, X, Yi, Zi) -> (B, C, *patch) fp32 and (B, S, *patch) fp32 labels with patch[0] == X.  Every
    slice of every channel is resampled in its own plane with the sample's one rotation (p["angle"] (B,)) and scale; every seg
    channel with the same map and indicator rule.  The device path is the in-plane prefilter and K31."""
    out_shape = tuple(int(v) for v in patch_size)
    if data.dim() != 5 or len(out_shape) != 3 or out_shape[0] != data.shape[2]:
        raise RuntimeError(f"spatial_transform_dummy_2d: data {tuple(data.shape)} to patch {out_shape}: axis 0 is never resampled, "
                           "the loader delivers patch[0] slices")
    return _spatial(data, seg, out_shape, p, labels, 2)


def simulate_low_resolution_3d(data, do, zoom, ignore_axes=None):
    """SimulateLowResolutionTransform, 3-D: per selected (sample, channel) nearest-exact down-sampling to round(shape * zoom),
    back with a cubic B-spline (12 voxels of edge padding, half-pixel grid), clipped to the small image's range.
    ignore_axes (0,) (the dummy-2-D chain, B:687-690): the small shape keeps axis 0, so both resizes are separable per slice --
    in-plane padding and prefilter, K31 with a diagonal map on the device -- while the clip still uses the range of the small
    VOLUME (skimage's resize clips to the range of its whole input), not of each slice."""
    ignore_axes = tuple(ignore_axes) if ignore_axes else ()
    if ignore_axes not in ((), (0,)):
        raise RuntimeError(f"simulate_low_resolution_3d: ignore_axes {ignore_axes}: None or (0,) expected")
    out = data.clone()
    nd = 2 if ignore_axes else 3
    shape = tuple(data.shape[-nd:])
    for b, c in np.argwhere(np.asarray(do)).tolist():
        small, coef = A2.low_resolution_image(data[b, c], float(zoom[b, c]), nd)     # coef (1, 1 or X, *small + 24)
        A = np.zeros((1, nd, nd + 1))
        for j, (n, m) in enumerate(zip(shape, small.shape[-nd:])):
            A[0, j, j], A[0, j, nd] = m / n, 0.5 * m / n - 0.5 + 12
        if data.is_cuda:
            from . import ops
            kernel = ops.aug3d_resample if nd == 3 else ops.aug3d_resample_planar
            up = kernel(coef.view(1, 1, *coef.shape[-3:]), None, A, [True], shape)[0]
        else:
            up = A2.sample(coef, affine_coords(A, shape, data.device), 3, 0.0)
        out[b, c] = A2.clip_to_range(up.view(data.shape[2:]), small)
    return out


# ------------------------------------------------------------------------------------------------
# the cascade transforms (cascade_transforms.py; B:703-718 and B:744-745)
# ------------------------------------------------------------------------------------------------
CASCADE_OPERATIONS = ("dilation", "erosion", "closing", "opening")      # any_of_these of ApplyRandomBinaryOperatorTransform (:92)


def ball(radius):
    """skimage.morphology.ball(radius) as a boolean array: n = 2 r + 1 points per axis on [-r, r] (mgrid truncates n), set where
    x^2 + y^2 + z^2 <= r^2.  skimage's own when it is importable."""
    try:
        from skimage.morphology import ball as skimage_ball
        return np.asarray(skimage_ball(radius)).astype(bool)
    except ImportError:
        n = 2 * radius + 1
        Z, Y, X = np.mgrid[-radius:radius:n * 1j, -radius:radius:n * 1j, -radius:radius:n * 1j]
        return (X ** 2 + Y ** 2 + Z ** 2) <= radius * radius


def draw_cascade_params(rng, batch, n_labels, order, p_per_sample=0.4, p_per_label=1.0, strel_size=(1, 8)):
    """The draws of ApplyRandomBinaryOperatorTransform.__call__ (cascade_transforms.py:111-119), which do not depend on the data:
    per sample uniform() < p_per_sample, then shuffle(order) IN PLACE (the caller keeps `order`, a list of the n_labels plane
    indices, across batches as the transform keeps self.channel_idx), then per channel in that order uniform() < p_per_label,
    choice(4) over CASCADE_OPERATIONS and uniform(*strel_size).  Returns per sample the list of (plane, operation, radius)."""
    if sorted(order) != list(range(n_labels)):
        raise RuntimeError(f"order {list(order)}: a permutation of the {n_labels} plane indices expected")
    params = []
    for _ in range(batch):
        steps = []
        if rng.uniform() < p_per_sample:
            rng.shuffle(order)
            for c in order:
                if rng.uniform() < p_per_label:
                    operation = int(rng.choice(len(CASCADE_OPERATIONS)))
                    steps.append((int(c), operation, float(rng.uniform(*strel_size))))
        params.append(steps)
    return params


def _footprint(strel):
    """A step's third entry: a radius (skimage's ball) or the footprint itself."""
    return ball(float(strel)) if np.ndim(strel) == 0 else np.asarray(strel).astype(bool)


def binary_operation_host(mask, operation, footprint):
    """skimage.morphology.binary_dilation / erosion / closing / opening as scipy.ndimage calls (closing = erosion of the dilation,
    opening = dilation of the erosion, erosion with border_value True)."""
    from scipy import ndimage as ndi
    dilate = lambda m: ndi.binary_dilation(m, structure=footprint)                             # noqa: E731
    erode = lambda m: ndi.binary_erosion(m, structure=footprint, border_value=True)            # noqa: E731
    return (dilate, erode, lambda m: erode(dilate(m)), lambda m: dilate(erode(m)))[operation](mask)


def _cascade_host(seg_prev, labels, params, rng, p_per_sample, fill_p, frac, p_per_label):
    """(B, X, Y, Z) integral label maps -> (B, L, X, Y, Z) boolean one-hot channels after both transforms, literally."""
    from scipy import ndimage as ndi
    onehot = np.stack([seg_prev == lab for lab in labels], 1)
    B, L = onehot.shape[:2]
    for b in range(B):
        for c, operation, strel in params[b]:
            workon = onehot[b, c].copy()
            if not workon.any():
                continue
            res = binary_operation_host(workon, operation, _footprint(strel))
            onehot[b, c] = res
            added = res & ~workon
            for oc in range(L):
                if oc != c:
                    onehot[b, oc] &= ~added
    num_voxels = np.prod(onehot.shape[2:], dtype=np.uint64)
    for b in range(B):
        if rng.uniform() < p_per_sample:
            for c in range(L):
                if rng.uniform() < p_per_label:
                    workon = onehot[b, c]
                    if not workon.any():
                        continue
                    lab, n = ndi.label(workon, structure=np.ones((3, 3, 3)))
                    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
                    valid = [i + 1 for i in range(n) if sizes[i] < num_voxels * frac]
                    if len(valid) > 0:
                        component = lab == valid[rng.choice(len(valid))]
                        workon[component] = False
                        if rng.uniform() < fill_p:
                            other = [i for i in range(L) if i != c]
                            if len(other) > 0:
                                onehot[b, rng.choice(other)][component] = True
    return onehot


def cascade_plan(params):
    """The host half of the morphology: per sample the steps as (plane, holds its centre, [(kind, first run, runs), ...]) and the
    run table (a list of (dx, dy, lo, len)) of every distinct (footprint, kind) among them."""
    from . import ops
    table, where, todo = [], {}, []
    for steps in params:
        todo.append([])
        for c, operation, strel in steps:
            S = _footprint(strel)
            parts = {"dilation": (0,), "erosion": (1,), "closing": (0, 1), "opening": (1, 0)}[CASCADE_OPERATIONS[operation]]
            sig = (S.shape, S.tobytes())
            for kind in parts:
                if sig + (kind,) not in where:
                    runs = ops.cascade_footprint_runs(S, kind)
                    where[sig + (kind,)] = (len(table), len(runs))
                    table += runs
            todo[-1].append((int(c), bool(S[tuple(n // 2 for n in S.shape)]), [(kind,) + where[sig + (kind,)] for kind in parts]))
    return todo, table


def _cascade_device(seg_prev, labels, params, rng, p_per_sample, fill_p, frac, p_per_label):
    """The same on bit planes (K30): returns (planes (B, L, X, Y, W) int64, Z)."""
    from . import ops
    B, X, Y, Z = (int(v) for v in seg_prev.shape)
    L, dev = len(labels), seg_prev.device
    pool = torch.empty((B * L + 2 * B, X, Y, ops.cascade_words(Z)), dtype=torch.int64, device=dev)     # the planes, two scratch per sample
    planes = pool[:B * L]
    ops.cascade_pack(seg_prev, labels, out=planes.view(B, L, *pool.shape[1:]))
    # morphology: step s of every sample in one launch sequence
    todo, table = cascade_plan(params)
    if table:
        runs = torch.tensor(table, dtype=torch.int32).to(dev)
        for s in range(max(len(t) for t in todo)):
            first, second, commit = [], [], []
            for b in range(B):
                if s < len(todo[b]):
                    c, centre, parts = todo[b][s]
                    target, t0, t1 = b * L + c, B * L + 2 * b, B * L + 2 * b + 1
                    # the reference skips an empty plane.  A footprint holding its centre (every ball) maps an empty plane to an
                    # empty plane; any other is asked now, when its step is due
                    if not centre and not bool(planes[target].any()):
                        continue
                    first.append((target, t0, parts[0][1], parts[0][2], parts[0][0]))
                    if len(parts) > 1:
                        second.append((t0, t1, parts[1][1], parts[1][2], parts[1][0]))
                    commit.append((t1 if len(parts) > 1 else t0, target, b * L))
            if first:
                ops.cascade_morph(pool, Z, first, runs)
                if second:
                    ops.cascade_morph(pool, Z, second, runs)
                ops.cascade_commit(pool, Z, L, commit)
    # component removal: the host draws need (non-empty, n_valid) of a sample's planes once its p_per_sample draw has fired
    thresh = float(np.prod((X, Y, Z), dtype=np.uint64) * frac)
    state = None                                                      # the labelling's workspace, shared by the samples of the batch
    for b in range(B):
        if rng.uniform() < p_per_sample:
            sample = planes[b * L:(b + 1) * L]
            if fill_p == 0:                                           # independent channels: one read-back, one removal launch
                state, stats = ops.cascade_cc_stats(sample, Z, thresh, state)
                stats = stats.cpu().numpy()
                rank = [-1] * L
            for c in range(L):
                if rng.uniform() < p_per_label:
                    if fill_p != 0:                                   # an earlier channel's fill may have changed this plane
                        state, one = ops.cascade_cc_stats(sample[c:c + 1], Z, thresh, state)
                        nonempty, n_valid = (int(v) for v in one.cpu().numpy()[0])
                    else:
                        nonempty, n_valid = (int(v) for v in stats[c])
                    if not nonempty or n_valid == 0:
                        continue
                    k = int(rng.choice(n_valid))
                    fill = 0
                    if rng.uniform() < fill_p:
                        other = [i for i in range(L) if i != c]
                        if len(other) > 0:
                            fill = int(rng.choice(other)) - c
                    if fill_p != 0:
                        ops.cascade_cc_remove(sample[c:c + 1], Z, state, [k], [fill])
                    else:
                        rank[c] = k
            if fill_p == 0 and max(rank) >= 0:
                ops.cascade_cc_remove(sample, Z, state, rank)
    return planes.view(B, L, *pool.shape[1:]), Z


def _label_map(seg_prev):
    """(B, 1, X, Y, Z) or (B, X, Y, Z) -> (B, X, Y, Z)"""
    if seg_prev.ndim == 5:
        if seg_prev.shape[1] != 1:
            raise RuntimeError(f"seg_prev {tuple(seg_prev.shape)}: one channel expected")
        seg_prev = seg_prev[:, 0]
    if seg_prev.ndim != 4:
        raise RuntimeError(f"seg_prev {tuple(seg_prev.shape)}: (B, 1, X, Y, Z) or (B, X, Y, Z) expected")
    return seg_prev


def _append_channels(data, onehot):
    if isinstance(data, torch.Tensor):
        return torch.cat([data, torch.as_tensor(onehot).to(data.dtype)], 1)
    return np.concatenate([data, onehot.astype(data.dtype)], 1)


def cascade_transforms(data, seg_prev, labels, params, rng, p_per_sample=0.2, fill_with_other_class_p=0.0,
                       dont_do_if_covers_more_than_x_percent=0.15, p_per_label=1.0):
    """MoveSegAsOneHotToData(1, labels), ApplyRandomBinaryOperatorTransform with the drawn `params` (draw_cascade_params; a step's
    third entry may be a footprint instead of a radius) and RemoveRandomConnectedComponentFromOneHotEncodingTransform with the
    trainer's arguments (B:705-718), whose draws are taken from `rng` in the reference's order.  data (B, C, X, Y, Z), seg_prev
    (B, 1, X, Y, Z) or (B, X, Y, Z): the previous stage's labels -> data (B, C + L, X, Y, Z).  CUDA tensors run K30; CPU tensors and
    numpy arrays run scipy.ndimage."""
    labels = [int(v) for v in labels]
    seg_prev = _label_map(seg_prev)
    if len(params) != data.shape[0] or tuple(seg_prev.shape) != (data.shape[0], *data.shape[2:]):
        raise RuntimeError(f"cascade_transforms: data {tuple(data.shape)}, seg_prev {tuple(seg_prev.shape)}, {len(params)} parameter lists")
    args = (labels, params, rng, float(p_per_sample), float(fill_with_other_class_p), float(dont_do_if_covers_more_than_x_percent),
            float(p_per_label))
    if isinstance(data, torch.Tensor) and data.is_cuda:
        return _append_planes(data, *_cascade_device(_device_labels(seg_prev), *args))
    host = seg_prev.numpy() if isinstance(seg_prev, torch.Tensor) else np.asarray(seg_prev)
    return _append_channels(data, _cascade_host(host, *args))


def _device_labels(seg_prev):
    return seg_prev if seg_prev.dtype in (torch.int16, torch.float32) else seg_prev.to(torch.float32)


def _append_planes(data, planes, Z):
    """data (B, C, X, Y, Z) and planes (B, L, X, Y, W) -> the fp32 network input (B, C + L, X, Y, Z)"""
    from . import ops
    C = data.shape[1]
    out = torch.empty((data.shape[0], C + planes.shape[1], *data.shape[2:]), dtype=torch.float32, device=data.device)
    out[:, :C] = data
    return ops.cascade_unpack(planes, Z, out, C)


def move_seg_as_one_hot(data, seg, labels):
    """MoveSegAsOneHotToData(1, labels, "seg", "data") of the validation chain (get_validation_transforms, B:744-745): seg (B, 2, ...)
    -> (data (B, C + L, ...), seg (B, 1, ...))."""
    if seg.ndim != 5 or seg.shape[1] != 2:
        raise RuntimeError(f"move_seg_as_one_hot: seg {tuple(seg.shape)}: the target and the previous stage's segmentation expected")
    labels = [int(v) for v in labels]
    prev = seg[:, 1]
    if isinstance(data, torch.Tensor) and data.is_cuda:
        from . import ops
        return _append_planes(data, ops.cascade_pack(_device_labels(prev), labels), prev.shape[-1]), seg[:, :1]
    host = prev.numpy() if isinstance(prev, torch.Tensor) else np.asarray(prev)
    return _append_channels(data, np.stack([host == lab for lab in labels], 1)), seg[:, :1]


class GpuAugmenter3D:
    """(loader batch on the device) -> augmented (data, seg): the reference's 3-D training transform chain behind
    `dataloading.DataLoader3D`.  `patch_size`: the network's; the loader delivers `initial_patch_size()`.
    `dummy_2d`: the chain of an anisotropic plan (do_dummy_2d_data_aug): 2-D draws, every slice resampled in its own plane (K31),
    SimulateLowResolution with ignore_axes (0,).  `for_plan` picks the mode as the reference does."""

    takes_int16_seg = True                      # dataloading.to_device hands over the loader's int16 labels as they are

    def __init__(self, patch_size, device, rotation=None, mirror_axes=(0, 1, 2), seed=None, labels=None, cascade_labels=None,
                 dummy_2d=False):
        self.patch_size = tuple(int(v) for v in patch_size)
        if len(self.patch_size) != 3:
            raise RuntimeError(f"GpuAugmenter3D: a 3-D patch, got {self.patch_size}")
        self.device = torch.device(device)
        self.dummy_2d = bool(dummy_2d)
        if rotation is None:
            rotation = ((-math.pi, math.pi), (0, 0), (0, 0)) if self.dummy_2d else rotation_for_3d(self.patch_size)
        self.rotation = rotation
        self.mirror_axes = tuple(mirror_axes)
        # every value the loader's segmentation can hold (label_manager.all_labels and the -1 padding), ascending (host path)
        self.labels = None if labels is None else torch.tensor(sorted(set(labels) | {-1}), dtype=torch.float32)
        self.rng = np.random.RandomState(seed)
        # 3d_cascade_fullres: the foreground labels of the previous stage's segmentation, the loader's second seg channel
        self.cascade_labels = None if cascade_labels is None else tuple(int(v) for v in cascade_labels)
        self.cascade_order = None if cascade_labels is None else list(range(len(self.cascade_labels)))

    @classmethod
    def for_plan(cls, patch_size, device, **kw):
        """The augmenter of a 3-D plan: rotation ranges, mirror axes and the dummy-2-D switch from `configure_3d`."""
        rotation, dummy_2d, _, mirror_axes = configure_3d(patch_size)
        return cls(patch_size, device, rotation=rotation, mirror_axes=mirror_axes, dummy_2d=dummy_2d, **kw)

    def initial_patch_size(self):
        """get_patch_size with the rotation ranges and the (0.85, 1.25) scale range of B:389-391; dummy-2-D keeps patch[0]
        (B:403-404)."""
        initial = tuple(int(v) for v in get_patch_size(self.patch_size, *self.rotation, (0.85, 1.25)))
        return (self.patch_size[0],) + initial[1:] if self.dummy_2d else initial

    def apply(self, data, seg, p, noise=None, cascade=None, rng=None):
        """The transform chain with given parameters (`draw_params_3d` layout; `draw_params_dummy_2d`'s with dummy_2d, where
        Xi == patch[0]); data (B, C, Xi, Yi, Zi) fp32, seg (B, 1, Xi, Yi, Zi).
        With `cascade_labels`: seg (B, 2, Xi, Yi, Zi), `cascade` the draw_cascade_params lists, `rng` the stream of the component
        removal's draws (the augmenter's own by default); returns data (B, C + L, *patch) and the one-channel target."""
        if (self.cascade_labels is not None) != (seg.shape[1] == 2) or seg.shape[1] > 2:
            raise RuntimeError(f"GpuAugmenter3D: seg {tuple(seg.shape)} with cascade_labels {self.cascade_labels}: the previous "
                               "stage's segmentation is the second seg channel of a cascade batch, and of no other")
        dev = data.device
        T = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a), device=dev).to(dt)      # noqa: E731
        spatial = spatial_transform_dummy_2d if self.dummy_2d else spatial_transform_3d
        data, seg = spatial(data, seg, self.patch_size, p, self.labels)
        if noise is None:
            noise = torch.randn_like(data)
        data = data + noise * T(p["noise_std"] * p["do_noise"]).view(-1, 1, 1, 1, 1)
        blur = p["blur_ch"] & p["do_blur"][:, None]
        radius = int(4.0 * float(p["blur_sigma"][blur].max()) + 0.5) if blur.any() else 0
        data = gaussian_blur(data, T(blur, torch.bool), T(p["blur_sigma"]), radius)
        data = torch.where(T(p["do_bright"], torch.bool).view(-1, 1, 1, 1, 1),
                           data * T(p["bright"]).view(*p["bright"].shape, 1, 1, 1), data)
        data = contrast_transform(data, T(p["do_contrast"], torch.bool), T(p["contrast"]))
        data = simulate_low_resolution_3d(data, p["lowres_ch"] & p["do_lowres"][:, None], p["lowres_zoom"],
                                          (0,) if self.dummy_2d else None)
        data = gamma_transform(data, T(p["do_gamma_inv"], torch.bool), T(p["gamma_inv"]), invert=True)
        data = gamma_transform(data, T(p["do_gamma"], torch.bool), T(p["gamma"]), invert=False)
        data, seg = mirror_transform(data, seg, T(p["mirror"], torch.bool))
        if self.cascade_labels is None:
            return data, seg
        if cascade is None:
            raise RuntimeError("GpuAugmenter3D.apply: a cascade augmenter needs the draw_cascade_params lists")
        # RemoveLabelTransform(-1, 0) (B:701) changes no plane: no listed label is -1 or 0
        data = cascade_transforms(data, seg[:, 1], self.cascade_labels, cascade, self.rng if rng is None else rng)
        return data, seg[:, :1]

    def clone(self, seed):
        """The same chain with its own parameter stream (one per loader worker) and its own channel order."""
        twin = GpuAugmenter3D(self.patch_size, self.device, self.rotation, self.mirror_axes, seed, cascade_labels=self.cascade_labels,
                              dummy_2d=self.dummy_2d)
        twin.labels = self.labels
        return twin

    def __call__(self, data, seg):
        if self.dummy_2d:
            p = draw_params_dummy_2d(self.rng, data.shape[0], data.shape[1], self.rotation[0], self.mirror_axes)
        else:
            p = draw_params_3d(self.rng, data.shape[0], data.shape[1], self.rotation, self.mirror_axes)
        if self.cascade_labels is None:
            return self.apply(data, seg, p)
        cascade = draw_cascade_params(self.rng, data.shape[0], len(self.cascade_labels), self.cascade_order)
        return self.apply(data, seg, p, cascade=cascade)
