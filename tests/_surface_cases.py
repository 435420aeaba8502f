"""Seeded masks and label volumes for the NSD tests (tests/golden/surface.npz, made by tests/golden/make_golden_surface.py with the
reference's own SurfaceDice.py) and the BTCV-sized synthetic case of the GPU tests and tools/bench_surface.py."""
import numpy as np

F32 = np.float32
AREA_SPACINGS = ((1.0, 1.0, 1.0), (F32(0.78125), F32(0.78125), F32(3.0)), (F32(1.5), F32(0.7), F32(0.7)), (0.3, 2.9, 1.7))
TOLERANCES = (0.0, 1.0, 2.0, 3.0, 5.0)          # of the dict metrics
PERCENTS = (50, 95, 100)                        # of compute_robust_hausdorff


def _ellipsoid(shape, centre, radii):
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return sum(((a - c) / r) ** 2 for a, c, r in zip((x, y, z), centre, radii)) <= 1.0


def _noisy(m, rng, p=0.08):
    """flip a fraction p of the voxels on the mask's boundary layer"""
    from scipy import ndimage as ndi
    edge = m ^ ndi.binary_erosion(m)
    flip = edge & (rng.random(m.shape) < p)
    return m ^ flip


def mask_cases():
    """[(name, mask_gt, mask_pred, spacing)] for compute_surface_distances"""
    rng = np.random.default_rng(2024)
    from scipy import ndimage as ndi
    out = []
    sh = (30, 34, 22)
    a = _ellipsoid(sh, (15, 16, 10), (9, 11, 7))
    out.append(("shifted", a, np.roll(a, (2, -1, 1), (0, 1, 2)), (F32(0.78125), F32(0.78125), F32(3.0))))
    out.append(("eroded", _noisy(a, rng), ndi.binary_erosion(a, iterations=2), (F32(1.5), F32(0.7), F32(0.7))))
    out.append(("isotropic", a, _noisy(np.roll(a, 3, 2), rng), (1.0, 1.0, 1.0)))
    b = np.zeros((9, 11, 7), bool)                       # touches every face of the volume
    b[:, :, :] = _ellipsoid(b.shape, (4, 5, 3), (6, 7, 5))
    c = np.zeros_like(b)
    c[0:5, :, 2:] = True
    c[:, 0, :] = True
    out.append(("faces", b, c, (F32(0.78125), F32(0.78125), F32(3.0))))
    s1, s2 = np.zeros((12, 12, 12), bool), np.zeros((12, 12, 12), bool)
    s1[5, 6, 7] = True
    s2[7, 3, 2] = True
    out.append(("single_voxels", s1, s2, (F32(1.5), F32(0.7), F32(0.7))))
    t1, t2 = np.zeros((16, 14, 18), bool), np.zeros((16, 14, 18), bool)
    t1[3, 4, :] = True                                   # one-voxel tubes along z and along a diagonal
    for k in range(12):
        t2[2 + k, 1 + k, 3 + k // 2] = True
    t2[8, 2:12, 9] = True
    out.append(("tubes", t1, t2, (F32(0.78125), F32(0.78125), F32(3.0))))
    out.append(("empty_gt", np.zeros(sh, bool), a, (F32(1.5), F32(0.7), F32(0.7))))
    out.append(("empty_pred", a, np.zeros(sh, bool), (F32(0.78125), F32(0.78125), F32(3.0))))
    out.append(("both_empty", np.zeros((5, 6, 7), bool), np.zeros((5, 6, 7), bool), (1.0, 1.0, 1.0)))
    e = _ellipsoid((40, 36, 1), (20, 18, 0), (14, 12, 1))           # the endoscopy form mask[..., None]
    out.append(("z1", e, _noisy(np.roll(e, 2, 0), rng, 0.2), (1, 1, 1)))
    # a crop of 260 x 262 x 100 with few surfels: two blobs at opposite corners of each mask
    big_g, big_p = np.zeros((270, 270, 104), bool), np.zeros((270, 270, 104), bool)
    big_g[3:6, 4:8, 2:5] = True
    big_g[258:262, 260:265, 97:101] = True
    big_p[4:7, 4:7, 2:6] = True
    big_p[259:262, 262:266, 98:102] = True
    big_p[130, 131, 50] = True
    out.append(("big_crop", big_g, big_p, (F32(0.78125), F32(0.78125), F32(3.0))))
    return out


def _ellipsoid_box(shape, centre, radii):
    """the ellipsoid's mask inside its bounding box, and the box's slices"""
    lo = [max(0, int(np.floor(c - r))) for c, r in zip(centre, radii)]
    hi = [min(n, int(np.ceil(c + r)) + 1) for n, c, r in zip(shape, centre, radii)]
    sub = _ellipsoid([h - l for l, h in zip(lo, hi)], [c - l for c, l in zip(centre, lo)], radii)
    return sub, tuple(slice(l, h) for l, h in zip(lo, hi))


def _abdomen_like(shape, seed, n_labels=13):
    """gt and a perturbed prediction with n_labels organs (ellipsoids; labels 5, 6, 8, 9, 10 thin tubes along z), the prediction's
    organs shifted by up to two voxels, plus speckles of label 3"""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    gt = np.zeros(shape, np.uint8)
    seg = np.zeros(shape, np.uint8)
    for lab in range(1, n_labels + 1):
        c = rng.uniform((0.2 * X, 0.2 * Y, 0.2 * Z), (0.8 * X, 0.8 * Y, 0.8 * Z))
        r = rng.uniform((0.04 * X, 0.04 * Y, 0.08 * Z), (0.16 * X, 0.16 * Y, 0.3 * Z))
        if lab in (5, 6, 8, 9, 10):
            r[0] = r[1] = max(1.5, 0.03 * X)
            r[2] = 0.45 * Z
        m, box = _ellipsoid_box(shape, c, r)
        gt[box][m] = lab
        shift = rng.integers(-2, 3, 3)
        m, box = _ellipsoid_box(shape, c + shift, r)
        seg[box][m] = lab
    seg[rng.random(shape) < 0.0005] = 3
    return gt, seg


def label_cases():
    """[(name, gt, seg, spacing, tolerances, slab_labels)] for case_nsd"""
    from mlagg_unet_amd import evaluation, surface
    out = []
    gt, seg = _abdomen_like((48, 44, 30), 11)
    seg[seg == 12] = 0                                  # a missed organ
    gt[gt == 7] = 0                                     # an organ only predicted
    seg[seg == 13] = 0
    gt[gt == 13] = 0                                    # an organ in neither
    out.append(("abdomen", gt, seg, (F32(0.78125), F32(0.78125), F32(3.0)), surface.ABDOMEN_NSD_TOLERANCES,
                evaluation.SLAB_LABELS))
    gt, seg = _abdomen_like((40, 46, 26), 12)
    out.append(("btcv", gt, seg, (F32(1.5), F32(0.7), F32(0.7)), surface.BTCV_NSD_TOLERANCES, surface.BTCV_SLAB_LABELS))
    gt, seg = _abdomen_like((36, 40, 10), 13, n_labels=3)
    out.append(("acdc", gt, seg, (F32(1.5625), F32(1.5625), F32(10.0)), surface.ACDC_NSD_TOLERANCES, ()))
    return out


def btcv_sized_case(seed=5):
    """a 512 x 512 x 150 BTCV-like case with 13 organs"""
    return _abdomen_like((512, 512, 150), seed)


def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "surface.npz")

