"""Shared inputs and the float64 oracle of the dummy-2-D augmentation tests (host path and K31 against scipy).

The oracle is the reference's own composition: Convert3DTo2DTransform reshapes (B, C, X, Y, Z) to (B, C * X, Y, Z), the 2-D
augment_spatial restated in oracle/augmentation_oracle.py runs on that, Convert2DTo3DTransform reshapes back; the rest of the chain
is the 3-D one of tests/_augmentation_3d_oracle.py except SimulateLowResolution, whose target shape keeps axis 0
(ignore_axes=(0,), nnUNetTrainer.py:687-690)."""
import copy

import numpy as np
from scipy import ndimage

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import augmentation3d as AUG3
from oracle import augmentation_oracle as AO
from tests import _augmentation_3d_oracle as AO3

B, C = 4, 2
IN, OUT = (5, 38, 34), (5, 24, 20)                # loader patch (ragged planes, odd X) -> network patch; 24 / 5 > 3
LABELS = [0, 1, 2, 3, 4]
ANGLES = (2.9, 0.0, -1.65, 0.0)                   # rotation only, scale only, both, neither; no multiple of pi / 2
SCALES = (1.0, 0.74, 1.37, 1.0)


def volumes(seed=0, shape=IN, channels=C, batch=B):
    """Data smooth within each slice only and rescaled to max |data| = 5; labels -1 .. 4 in blobs (-1 as the loader's padding)."""
    rng = np.random.RandomState(seed)
    data = ndimage.gaussian_filter(rng.randn(batch, channels, *shape), (0, 0, 0, 1.5, 1.5))
    data = (data * (5.0 / np.abs(data).max())).astype(np.float32)
    seg = (ndimage.gaussian_filter(rng.randn(batch, 1, *shape), (0, 0, 1, 3, 3)) * 60).round().clip(-1, 4).astype(np.float32)
    return data, seg


def ramped(data):
    """The same volumes with slice x scaled by 0.3 .. 1: every slice has its own range, so a per-slice clip differs from the
    volume's."""
    X = data.shape[2]
    return data * np.linspace(0.3, 1.0, X, dtype=np.float32).reshape(1, 1, X, 1, 1)


def forced_params(seed=1):
    """Every transform active on some sample / channel; rotation only, scale only, both, neither all present."""
    rng = np.random.RandomState(seed)
    p = AUG3.draw_params_dummy_2d(np.random.RandomState(seed), B, C)
    for k in p:
        if k.startswith("do_"):
            p[k][:] = True
    p["do_rot"][:] = [1, 0, 1, 0]
    p["do_scale"][:] = [0, 1, 1, 0]
    p["angle"][:] = ANGLES
    p["scale"][:] = SCALES
    p["noise_std"][:] = rng.uniform(0, 0.1, B)
    p["blur_ch"][:] = rng.rand(B, C) < 0.6
    p["blur_sigma"][:] = rng.uniform(0.5, 1, (B, C))
    p["bright"][:] = rng.uniform(0.75, 1.25, (B, C))
    p["contrast"][:] = rng.uniform(0.75, 1.25, (B, C))
    p["lowres_ch"][:] = rng.rand(B, C) < 0.6
    p["lowres_zoom"][:] = rng.uniform(0.5, 1, (B, C))
    p["gamma"][:] = rng.uniform(0.7, 1.5, (B, C))
    p["gamma_inv"][:] = rng.uniform(0.7, 1.5, (B, C))
    p["mirror"][:] = rng.rand(B, 3) < 0.5
    return p


def spatial_params(angles, scales):
    """Spatial-only parameters for any batch size: sample b rotates by angles[b] where it is not None, scales by scales[b] likewise."""
    n = len(angles)
    p = only(AUG3.draw_params_dummy_2d(np.random.RandomState(0), n, 1), [])
    p["do_rot"][:] = [a is not None for a in angles]
    p["do_scale"][:] = [s is not None for s in scales]
    p["angle"][:] = [0.0 if a is None else a for a in angles]
    p["scale"][:] = [1.0 if s is None else s for s in scales]
    return p


def only(p, keys, mirror=False):
    q = copy.deepcopy(p)
    for k in q:
        if k.startswith("do_") and k not in keys:
            q[k][:] = False
    if not mirror:
        q["mirror"][:] = False
    return q


# ------------------------------------------------------------------------------------------------
# oracle
# ------------------------------------------------------------------------------------------------
def spatial(data, seg, patch_size, p):
    """Convert3DTo2D + the 2-D augment_spatial + Convert2DTo3D; seg may have several channels."""
    Bn, Cn, X = data.shape[:3]
    S = seg.shape[1]
    d, s = AO.spatial(data.reshape(Bn, Cn * X, *data.shape[3:]), seg.reshape(Bn, S * X, *seg.shape[3:]), tuple(patch_size[1:]), p)
    return d.reshape(Bn, Cn, X, *patch_size[1:]), s.reshape(Bn, S, X, *patch_size[1:])


def low_resolution(data, p, per_slice_clip=False):
    """SimulateLowResolutionTransform with ignore_axes=(0,) on (B, C, X, Y, Z).  per_slice_clip: the WRONG variant that clips each
    slice to its own small slice's range (for the test that the case tells the two apart)."""
    data = data.copy()
    shp = np.array(data.shape[2:])
    for b in range(data.shape[0]):
        if p["do_lowres"][b]:
            for c in range(data.shape[1]):
                if p["lowres_ch"][b, c]:
                    target = np.round(shp * p["lowres_zoom"][b, c]).astype(int)
                    target[0] = shp[0]
                    down = AO.resize_edge(data[b, c].astype(float), target, 0)
                    if per_slice_clip:
                        data[b, c] = np.stack([AO.resize_edge(down[x], shp[1:], 3) for x in range(shp[0])])
                    else:
                        data[b, c] = AO.resize_edge(down, shp, 3)
    return data


def apply(data, seg, patch_size, p, noise):
    """The chain B:658-695 with do_dummy_2d_data_aug: the planar spatial transform, then the 3-D chain of
    tests/_augmentation_3d_oracle.apply in its order (on an input that already has the patch's shape its spatial step is the
    identity crop), with the low-resolution step replaced by the ignore_axes one."""
    data, seg = spatial(data.astype(np.float32), seg.astype(np.float32), patch_size, p)
    data, seg = AO3.apply(data, seg, patch_size, only(p, ["do_noise", "do_blur", "do_bright", "do_contrast"]), noise)
    data = low_resolution(data, p)
    return AO3.apply(data, seg, patch_size, only(p, ["do_gamma_inv", "do_gamma"], mirror=True), noise)


def coordinates(p, b, in_yz, out_yz):
    """The 2-D sampling coordinates of sample b (2, Yo, Zo), or None where the sample is centre-cropped."""
    if not (p["do_rot"][b] or p["do_scale"][b]):
        return None
    coords = AO.zero_centered_mesh(out_yz)
    if p["do_rot"][b]:
        coords = AO.rotate_2d(coords, p["angle"][b])
    if p["do_scale"][b]:
        coords = coords * p["scale"][b]
    for d in range(2):
        coords[d] += in_yz[d] / 2.0 - 0.5
    return coords


def near_half(seg, p, patch=OUT, tol=1e-4, channel=0):
    """(B, 1, *patch) mask of the resampled voxels whose float64 bilinear label indicator lies within `tol` of 0.5 (where fp32 and
    float64 may pick different labels), flipped as p["mirror"] flips the output."""
    mask = np.zeros((seg.shape[0], 1) + tuple(patch), dtype=bool)
    for b in range(seg.shape[0]):
        coords = coordinates(p, b, seg.shape[3:], patch[1:])
        if coords is None:
            continue
        m = np.stack([(np.abs(AO3.segmentation_indicators(seg[b, channel, x], coords)[1] - 0.5) < tol).any(0)
                      for x in range(seg.shape[2])])
        for ax in range(3):
            if p["mirror"][b, ax]:
                m = np.flip(m, ax)
        mask[b, 0] = m
    return mask


def outside_share(p, b, in_yz, out_yz):
    """Share of sample b's output pixels whose coordinate leaves the input plane."""
    c = coordinates(p, b, in_yz, out_yz)
    return float(((c[0] < 0) | (c[0] > in_yz[0] - 1) | (c[1] < 0) | (c[1] > in_yz[1] - 1)).mean())
