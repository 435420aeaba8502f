"""Training-time data augmentation of the 3-D path ON the MI355X: the reference's get_training_transforms
(nnUNetTrainer.py:645-733) for a 3-D configuration without dummy-2-D augmentation (the BTCV plan: 160 / 96 < ANISO_THRESHOLD 3),
behind `dataloading.DataLoader3D`.

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
CPU tensors take a torch composition of the same arithmetic (the sampler as one gather of all taps), for tests at small sizes.

Out of scope: dummy-2-D augmentation of anisotropic patches (NotImplementedError), the cascade / region / mask transforms
(B:697-727), as in the 2-D augmenter.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import augmentation as A2
from .augmentation import band_matrix, contrast_transform, gamma_transform, get_patch_size, mirror_transform

ANISO_THRESHOLD = 3                                  # nnunetv2.configuration.ANISO_THRESHOLD


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
    rotation = rotation_for_3d((1, 1, 1)) if rotation is None else rotation
    B, C = batch, channels
    p = {k: np.zeros(B, dtype=bool) for k in ("do_rot", "do_scale", "do_noise", "do_blur", "do_bright", "do_contrast", "do_lowres",
                                              "do_gamma_inv", "do_gamma")}
    p.update(angle=np.zeros((B, 3)), scale=np.ones(B), noise_std=np.zeros(B), blur_ch=np.zeros((B, C), dtype=bool),
             blur_sigma=np.ones((B, C)), bright=np.ones((B, C)), contrast=np.ones((B, C)), lowres_ch=np.zeros((B, C), dtype=bool),
             lowres_zoom=np.ones((B, C)), gamma_inv=np.ones((B, C)), gamma=np.ones((B, C)), mirror=np.zeros((B, 3), dtype=bool))
    for b in range(B):                                                     # SpatialTransform: p_rot 0.2, p_scale 0.2
        if rng.uniform() < 0.2:
            for ax in range(3):
                if rng.uniform() <= 1.0:                                   # p_rot_per_axis = 1 (B:670): drawn, always taken
                    p["angle"][b, ax] = rng.uniform(rotation[ax][0], rotation[ax][1])
            p["do_rot"][b] = True
        if rng.uniform() < 0.2:
            p["do_scale"][b], p["scale"][b] = True, A2._two_sided(rng, 0.7, 1.4)
    return A2._draw_intensity_and_mirror(rng, p, B, C, mirror_axes)


def rotation_matrix(ax, ay, az):
    """rotate_coords_3d's matrix I . Rx . Ry . Rz (float64); coordinates are rotated as coords^T . M."""
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.identity(3) @ Rx @ Ry @ Rz


def affines(p, in_shape, out_shape):
    """Per sample the (3, 4) float64 map output voxel index -> input coordinate of augment_spatial: zero-centred mesh, rotated,
    scaled, moved to the input centre (in / 2 - 0.5); and whether the sample is resampled at all (else: centre crop)."""
    B = len(p["do_rot"])
    A = np.zeros((B, 3, 4))
    do = np.asarray(p["do_rot"]) | np.asarray(p["do_scale"])
    half = (np.asarray(out_shape, dtype=np.float64) - 1) / 2.0
    for b in range(B):
        M = rotation_matrix(*p["angle"][b]) if p["do_rot"][b] else np.identity(3)
        L = (M * (p["scale"][b] if p["do_scale"][b] else 1.0)).T               # input_j = sum_i L[j, i] centred_i
        A[b, :, :3] = L
        A[b, :, 3] = np.asarray(in_shape, dtype=np.float64) / 2.0 - 0.5 - L @ half
    return A, do


# ------------------------------------------------------------------------------------------------
# host (CPU tensor) sampler; the device runs K25
# ------------------------------------------------------------------------------------------------
def spline_coefficients_3d(x):
    """(.., X, Y, Z) -> cubic B-spline coefficients with scipy's "mirror" boundary: the 33-tap band matrix along each axis."""
    X, Y, Z = x.shape[-3:]
    lead = x.shape[:-3]
    x = (A2._prefilter_matrix(X, x.device) @ x.reshape(-1, X, Y * Z)).reshape(*lead, X, Y, Z)
    x = A2._prefilter_matrix(Y, x.device) @ x
    return x @ A2._prefilter_matrix(Z, x.device).T


def sample_3d(img, A, out_shape, order, cval):
    """map_coordinates(img, coords, order, mode="constant", cval) with coords = A (B, 3, 4) float64 applied to the output voxel
    grid: img (B, C, X, Y, Z) (spline coefficients for order 3) -> (B, C, *out_shape).  The coordinate is float64, its fractions
    fp32 (as K25 forms them); all taps of all channels in one gather."""
    B, C, X, Y, Z = img.shape
    dev = img.device
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64, device=dev) for n in out_shape], indexing="ij"))
    At = torch.as_tensor(A, dtype=torch.float64, device=dev)
    coords = torch.einsum("bji,ip->bjp", At[:, :, :3], grid.reshape(3, -1)) + At[:, :, 3:]       # (B, 3, P)
    inside = torch.ones(coords.shape[::2], dtype=torch.bool, device=dev)
    taps, weights = [], []
    first, n = (-1, 4) if order == 3 else (0, 2)
    for j, size in enumerate((X, Y, Z)):
        c = coords[:, j]
        inside &= (c >= 0) & (c <= size - 1)
        f = torch.floor(c)
        t = (c - f).float()
        w = A2._bspline3_weights(t) if order == 3 else torch.stack([1 - t, t], -2)          # (B, n, P)
        taps.append(A2._mirror_index(f.long().unsqueeze(1) + torch.arange(n, device=dev).view(1, n, 1) + first, size))
        weights.append(w)
    ix, iy, iz = taps
    idx = ((ix[:, :, None, None] * Y + iy[:, None, :, None]) * Z + iz[:, None, None, :]).reshape(B, 1, -1)
    w = (weights[0][:, :, None, None] * weights[1][:, None, :, None] * weights[2][:, None, None, :]).reshape(B, 1, n ** 3, -1)
    vals = img.reshape(B, C, -1).gather(2, idx.expand(-1, C, -1)).view(B, C, n ** 3, -1)
    out = (vals * w).sum(2)
    out = torch.where(inside.unsqueeze(1), out, torch.full_like(out, cval))
    return out.view(B, C, *out_shape)


# ------------------------------------------------------------------------------------------------
# transforms
# ------------------------------------------------------------------------------------------------
def _prefiltered(data, do):
    """The resampler's input volume: spline coefficients of the samples in `do`, the data itself for the others."""
    idx = np.flatnonzero(do)
    if len(idx) == len(do):
        return spline_coefficients_3d(data).contiguous()
    vol = data.clone()
    if len(idx):
        sel = torch.as_tensor(idx, device=data.device)
        vol[sel] = spline_coefficients_3d(data[sel])
    return vol


def spatial_transform_3d(data, seg, patch_size, p, labels=None):
    """augment_spatial, 3-D, with the nnU-Net arguments: data (B, C, Xi, Yi, Zi) fp32, seg (B, 1, Xi, Yi, Zi) (int16 on the
    device path; any integral-valued type on the host) -> (B, C, *patch) fp32 and (B, 1, *patch) fp32 labels."""
    in_shape, out_shape = tuple(data.shape[2:]), tuple(int(v) for v in patch_size)
    A, do = affines(p, in_shape, out_shape)
    vol = _prefiltered(data.contiguous(), do)
    if data.is_cuda:
        from . import ops
        return ops.aug3d_resample(vol, seg.to(torch.int16).contiguous(), A, do, out_shape)
    B = data.shape[0]
    out_d = sample_3d(vol, A, out_shape, 3, 0.0)
    segf = seg.to(torch.float32)
    lab = torch.unique(segf) if labels is None else labels.to(segf.device)
    onehot = (segf == lab.view(1, -1, 1, 1, 1)).to(torch.float32)
    r = sample_3d(onehot, A, out_shape, 1, -1.0)
    rank = ((r >= 0.5) * torch.arange(1, len(lab) + 1).view(1, -1, 1, 1, 1)).amax(1, keepdim=True)
    out_s = torch.where(rank > 0, lab[(rank - 1).clamp_(min=0)], torch.zeros(()))
    o = [(i - s) // 2 for i, s in zip(in_shape, out_shape)]
    crop = (slice(o[0], o[0] + out_shape[0]), slice(o[1], o[1] + out_shape[1]), slice(o[2], o[2] + out_shape[2]))
    m = torch.as_tensor(do).view(B, 1, 1, 1, 1)
    if (~do).any():
        out_d = torch.where(m, out_d, data[(slice(None), slice(None)) + crop])
        out_s = torch.where(m, out_s, segf[(slice(None), slice(None)) + crop])
    return out_d, out_s


def gaussian_blur_3d(data, do, sigma, radius):
    """scipy.ndimage.gaussian_filter(img, sigma) (same sigma on the three axes, truncate 4, "reflect") per (sample, channel)
    where `do`; `radius` = int(4 max(sigma) + 0.5) from the host-side parameters."""
    B, C, X, Y, Z = data.shape
    if radius == 0:
        return data
    t = torch.arange(-radius, radius + 1, device=data.device, dtype=torch.float32).view(1, 1, -1)
    s = sigma.view(B, C, 1)
    w = torch.exp(-0.5 * (t / s) ** 2) * (t.abs() <= torch.floor(4.0 * s + 0.5))
    w = w / w.sum(-1, keepdim=True)
    x = (band_matrix(X, w, "symmetric", data.device) @ data.reshape(B, C, X, Y * Z)).reshape(B, C, X, Y, Z)
    x = band_matrix(Y, w, "symmetric", data.device).unsqueeze(2) @ x
    x = x @ band_matrix(Z, w, "symmetric", data.device).transpose(-1, -2).unsqueeze(2)
    return torch.where(do.view(B, C, 1, 1, 1), x, data)


def simulate_low_resolution_3d(data, do, zoom):
    """SimulateLowResolutionTransform, 3-D: per selected (sample, channel) nearest-exact down-sampling to round(shape * zoom),
    back with a cubic B-spline (12 voxels of edge padding, half-pixel grid), clipped to the small image's range."""
    out = data.clone()
    shape = tuple(data.shape[2:])
    for b, c in np.argwhere(np.asarray(do)).tolist():
        small_shape = tuple(int(v) for v in np.round(np.array(shape, dtype=float) * float(zoom[b, c])))
        f64 = dict(device=data.device, dtype=torch.float64)
        ix, iy, iz = (torch.floor((torch.arange(m, **f64) + 0.5) * (n / m)).long().clamp_(0, n - 1)
                      for n, m in zip(shape, small_shape))
        small = data[b, c][ix][:, iy][:, :, iz]
        coef = spline_coefficients_3d(F.pad(small[None, None], (12,) * 6, mode="replicate")).contiguous()
        A = np.zeros((1, 3, 4))
        for j, (n, m) in enumerate(zip(shape, small_shape)):
            A[0, j, j], A[0, j, 3] = m / n, 0.5 * m / n - 0.5 + 12
        if data.is_cuda:
            from . import ops
            up = ops.aug3d_resample(coef, None, A, [True], shape)[0][0, 0]
        else:
            up = sample_3d(coef, A, shape, 3, 0.0)[0, 0]
        out[b, c] = torch.minimum(torch.maximum(up, small.min()), small.max())
    return out


class GpuAugmenter3D:
    """(loader batch on the device) -> augmented (data, seg): the reference's 3-D training transform chain behind
    `dataloading.DataLoader3D`.  `patch_size`: the network's; the loader delivers `initial_patch_size()`."""

    takes_int16_seg = True                      # dataloading.to_device hands over the loader's int16 labels as they are

    def __init__(self, patch_size, device, rotation=None, mirror_axes=(0, 1, 2), seed=None, labels=None):
        self.patch_size = tuple(int(v) for v in patch_size)
        if len(self.patch_size) != 3:
            raise RuntimeError(f"GpuAugmenter3D: a 3-D patch, got {self.patch_size}")
        self.device = torch.device(device)
        self.rotation = rotation_for_3d(self.patch_size) if rotation is None else rotation
        self.mirror_axes = tuple(mirror_axes)
        # every value the loader's segmentation can hold (label_manager.all_labels and the -1 padding), ascending (host path)
        self.labels = None if labels is None else torch.tensor(sorted(set(labels) | {-1}), dtype=torch.float32)
        self.rng = np.random.RandomState(seed)

    def initial_patch_size(self):
        """get_patch_size with the rotation ranges and the (0.85, 1.25) scale range of B:389-391."""
        return tuple(int(v) for v in get_patch_size(self.patch_size, *self.rotation, (0.85, 1.25)))

    def apply(self, data, seg, p, noise=None):
        """The transform chain with given parameters (`draw_params_3d` layout); data (B, C, Xi, Yi, Zi) fp32, seg (B, 1, Xi, Yi, Zi)."""
        dev = data.device
        T = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a), device=dev).to(dt)      # noqa: E731
        data, seg = spatial_transform_3d(data, seg, self.patch_size, p, self.labels)
        if noise is None:
            noise = torch.randn_like(data)
        data = data + noise * T(p["noise_std"] * p["do_noise"]).view(-1, 1, 1, 1, 1)
        blur = p["blur_ch"] & p["do_blur"][:, None]
        radius = int(4.0 * float(p["blur_sigma"][blur].max()) + 0.5) if blur.any() else 0
        data = gaussian_blur_3d(data, T(blur, torch.bool), T(p["blur_sigma"]), radius)
        data = torch.where(T(p["do_bright"], torch.bool).view(-1, 1, 1, 1, 1),
                           data * T(p["bright"]).view(*p["bright"].shape, 1, 1, 1), data)
        data = contrast_transform(data, T(p["do_contrast"], torch.bool), T(p["contrast"]))
        data = simulate_low_resolution_3d(data, p["lowres_ch"] & p["do_lowres"][:, None], p["lowres_zoom"])
        data = gamma_transform(data, T(p["do_gamma_inv"], torch.bool), T(p["gamma_inv"]), invert=True)
        data = gamma_transform(data, T(p["do_gamma"], torch.bool), T(p["gamma"]), invert=False)
        return mirror_transform(data, seg, T(p["mirror"], torch.bool))

    def clone(self, seed):
        """The same chain with its own parameter stream (one per loader worker)."""
        twin = GpuAugmenter3D(self.patch_size, self.device, self.rotation, self.mirror_axes, seed)
        twin.labels = self.labels
        return twin

    def __call__(self, data, seg):
        p = draw_params_3d(self.rng, data.shape[0], data.shape[1], self.rotation, self.mirror_axes)
        return self.apply(data, seg, p)
