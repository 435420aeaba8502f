"""TEST INFRASTRUCTURE (oracle) -- scipy float64 restatement of the reference's training augmentation chain
(nnUNetTrainer.get_training_transforms, nnUNetTrainer.py:645-733) for a 3-D configuration without dummy-2-D augmentation.

batchgenerators (third-party, absent offline) is restated from its published arithmetic, sample by sample and channel by
channel, as oracle/augmentation_oracle.py does for 2-D (whose zero_centered_mesh / interpolate_img / resize_edge are reused):
rotate_coords_3d is coords^T . (I Rx Ry Rz), then the isotropic scale, then the input centre (shape / 2 - 0.5)."""
import numpy as np
from scipy import ndimage

from oracle.augmentation_oracle import interpolate_img, resize_edge, zero_centered_mesh


def rotate_3d(coords, ax, ay, az):
    """batchgenerators rotate_coords_3d."""
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    M = np.dot(np.dot(np.dot(np.identity(3), Rx), Ry), Rz)
    return np.dot(coords.reshape(3, -1).T, M).T.reshape(coords.shape)


def coordinates(p, b, in_shape, patch_size):
    """augment_spatial's sampling coordinates of sample b (3, *patch), or None where the sample is centre-cropped."""
    coords = zero_centered_mesh(patch_size)
    modified = False
    if p["do_rot"][b]:
        coords, modified = rotate_3d(coords, *p["angle"][b]), True
    if p["do_scale"][b]:
        coords, modified = coords * p["scale"][b], True
    if not modified:
        return None
    for d in range(3):
        coords[d] += in_shape[d] / 2.0 - 0.5
    return coords


def spatial(data, seg, patch_size, p):
    """augment_spatial with the nnU-Net arguments (B:666-677), 3-D: order 3 / 1, cval 0 / -1, centre crop otherwise."""
    B = data.shape[0]
    out_d = np.zeros((B, data.shape[1]) + tuple(patch_size), dtype=np.float32)
    out_s = np.zeros((B, seg.shape[1]) + tuple(patch_size), dtype=np.float32)
    for b in range(B):
        coords = coordinates(p, b, data.shape[2:], patch_size)
        if coords is not None:
            for c in range(data.shape[1]):
                out_d[b, c] = interpolate_img(data[b, c], coords, 3, 0.0)
            for c in range(seg.shape[1]):
                out_s[b, c] = interpolate_img(seg[b, c], coords, 1, -1.0, is_seg=True)
        else:
            lb = [(data.shape[d + 2] - patch_size[d]) // 2 for d in range(3)]
            sl = tuple(slice(lb[d], lb[d] + patch_size[d]) for d in range(3))
            out_d[b], out_s[b] = data[b][(slice(None),) + sl], seg[b][(slice(None),) + sl]
    return out_d, out_s


def segmentation_indicators(seg, coords):
    """float64 trilinear indicator of every label of `seg` at `coords` (K, P): for the 0.5-boundary count of the parity tests."""
    labels = np.unique(seg)
    return labels, np.stack([ndimage.map_coordinates((seg == c).astype(float), coords, order=1, mode="constant", cval=-1.0)
                             for c in labels])


def apply(data, seg, patch_size, p, noise):
    """The chain B:666-695 for 3-D patches with the parameters `p` (augmentation3d.draw_params_3d layout) and the unit-variance
    noise field `noise` (B, C, *patch)."""
    data, seg = spatial(data.astype(np.float32), seg.astype(np.float32), patch_size, p)
    B, C = data.shape[:2]
    for b in range(B):
        if p["do_noise"][b]:
            data[b] += (noise[b] * p["noise_std"][b]).astype(np.float32)
    for b in range(B):
        if p["do_blur"][b]:
            for c in range(C):
                if p["blur_ch"][b, c]:
                    data[b, c] = ndimage.gaussian_filter(data[b, c], p["blur_sigma"][b, c], order=0)
    for b in range(B):
        if p["do_bright"][b]:
            for c in range(C):
                data[b, c] *= p["bright"][b, c]
    for b in range(B):
        if p["do_contrast"][b]:
            for c in range(C):
                mn, lo, hi = data[b, c].mean(), data[b, c].min(), data[b, c].max()
                data[b, c] = np.clip((data[b, c] - mn) * p["contrast"][b, c] + mn, lo, hi)
    for b in range(B):
        if p["do_lowres"][b]:
            shp = np.array(data.shape[2:])
            for c in range(C):
                if p["lowres_ch"][b, c]:
                    target = np.round(shp * p["lowres_zoom"][b, c]).astype(int)
                    down = resize_edge(data[b, c].astype(float), target, 0)
                    data[b, c] = resize_edge(down, shp, 3)
    for key_do, key_g, invert in (("do_gamma_inv", "gamma_inv", True), ("do_gamma", "gamma", False)):
        for b in range(B):
            if p[key_do][b]:
                x = -data[b] if invert else data[b].copy()
                for c in range(C):
                    mn, sd = x[c].mean(), x[c].std()
                    lo = x[c].min()
                    rnge = x[c].max() - lo
                    x[c] = np.power((x[c] - lo) / float(rnge + 1e-7), p[key_g][b, c]) * float(rnge + 1e-7) + lo
                    x[c] = x[c] - x[c].mean()
                    x[c] = x[c] / (x[c].std() + 1e-8) * sd
                    x[c] = x[c] + mn
                data[b] = -x if invert else x
    for b in range(B):
        for ax in range(3):
            if p["mirror"][b, ax]:
                data[b], seg[b] = np.flip(data[b], ax + 1).copy(), np.flip(seg[b], ax + 1).copy()
    return data, seg
