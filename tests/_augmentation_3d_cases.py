"""Shared inputs of the 3-D augmentation parity tests (host path and K25 against tests/_augmentation_3d_oracle.py)."""
import copy

import numpy as np
from scipy import ndimage

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import augmentation3d as AUG3

B, C = 4, 2
IN, OUT = (30, 38, 34), (16, 24, 20)              # loader patch (ragged) -> network patch
LABELS = [0, 1, 2, 3, 4]


def volumes(seed=0, shape=IN):
    """Amplitude-5 smooth data, and labels -1 .. 4 in blobs (-1 as the loader's padding)."""
    rng = np.random.RandomState(seed)
    data = (ndimage.gaussian_filter(rng.randn(B, C, *shape), (0, 0, 1.5, 1.5, 1.5)) * 12).astype(np.float32)
    seg = (ndimage.gaussian_filter(rng.randn(B, 1, *shape), (0, 0, 3, 3, 3)) * 60).round().clip(-1, 4).astype(np.float32)
    return data, seg


def forced_params(seed=1):
    """Every transform active on some sample / channel; rotation only, scale only, both, neither all present."""
    rng = np.random.RandomState(seed)
    p = AUG3.draw_params_3d(np.random.RandomState(seed), B, C)
    for k in p:
        if k.startswith("do_"):
            p[k][:] = True
    p["do_rot"][:] = [1, 0, 1, 0]
    p["do_scale"][:] = [0, 1, 1, 0]
    r = 30 / 360 * 2 * np.pi
    p["angle"][:] = rng.uniform(-r, r, (B, 3))
    p["scale"][:] = rng.uniform(0.7, 1.4, B)
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


def only(p, keys):
    q = copy.deepcopy(p)
    for k in q:
        if k.startswith("do_") and k not in keys:
            q[k][:] = False
    q["mirror"][:] = False
    return q


STAGES = (["do_rot", "do_scale"], ["do_noise"], ["do_blur"], ["do_bright"], ["do_contrast"], ["do_lowres"], ["do_gamma_inv"],
          ["do_gamma"])


def near_half(seg, p, patch=OUT, tol=1e-4):
    """(B, 1, *patch) mask of the resampled voxels whose float64 label indicator lies within `tol` of 0.5 (where fp32 and float64
    may pick different labels), flipped as p["mirror"] flips the output."""
    from tests import _augmentation_3d_oracle as AO3
    mask = np.zeros((seg.shape[0], 1) + tuple(patch), dtype=bool)
    for b in range(seg.shape[0]):
        coords = AO3.coordinates(p, b, seg.shape[2:], patch)
        if coords is None:
            continue
        _, r = AO3.segmentation_indicators(seg[b, 0], coords)
        m = (np.abs(r - 0.5) < tol).any(0)
        for ax in range(3):
            if p["mirror"][b, ax]:
                m = np.flip(m, ax)
        mask[b, 0] = m
    return mask
