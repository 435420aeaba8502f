"""Seeded images for the cell-metric tests (tests/golden/cells.npz, made by tests/golden/make_golden_cells.py with the reference's own
evaluation/compute_cell_metric.py) and for tools/bench_cells.py.  Every case is procedural and independent of the reference.

    CASES       name -> (gt instance map, seg class-label image): what the script scores (cells = class 1 of seg)
    PAIRS       name -> (masks_true, masks_pred): instance maps for eval_tp_fp_fn / intersection_over_union directly
    TILED       the CASES also scored through the tiled branch with large_image_pixels = 1 and roi_size = TILED_ROI
    big_case()  one image above the real 25 M-pixel switch with sparse cells (only its CSV row is stored)
"""
import numpy as np

THRESHOLDS = (0.1, 0.3, 0.5, 0.75)
TILED = ("discs", "ring", "split_merge", "gaps")
TILED_ROI = 64
BIG_SHAPE = (5002, 5003)


def _disc(img, cy, cx, r, value):
    H, W = img.shape
    y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
    if y0 >= y1 or x0 >= x1:
        return
    y, x = np.ogrid[y0:y1, x0:x1]
    img[y0:y1, x0:x1][(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = value


def _discs(shape, n, seed, rmin=4, rmax=9, dtype=np.int32, miss=0.15, extra=4, jitter=2):
    """n discs, later ones drawn over earlier ones (overlapping discs, touching predictions merge); the prediction moves and resizes
    each, misses some and invents `extra`; class 2 blobs are another class and count for nothing"""
    rng = np.random.default_rng(seed)
    H, W = shape
    gt, seg = np.zeros(shape, dtype), np.zeros(shape, np.uint8)
    for k in range(n):
        cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(rmin, rmax + 1))
        _disc(gt, cy, cx, r, k + 1)
        dy, dx, dr = (int(v) for v in rng.integers(-jitter, jitter + 1, 3))
        if rng.random() >= miss:
            _disc(seg, cy + dy, cx + dx, max(r + dr, 1), 1)
    for _ in range(extra):
        _disc(seg, int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(rmin, rmax + 1)), 1)
    for _ in range(3):
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        blob = np.zeros(shape, bool)
        _disc(blob, cy, cx, 3, True)
        seg[blob & (seg == 0)] = 2
    return gt, seg


def _split_merge():
    """a gt cell the prediction splits in two, two gt cells it merges into one, and one it finds exactly; 70 x 130"""
    gt, seg = np.zeros((70, 130), np.int32), np.zeros((70, 130), np.uint8)
    gt[10:30, 10:40] = 1                      # split: two halves with a one-pixel gap
    seg[10:30, 10:24] = 1
    seg[10:30, 25:40] = 1
    gt[40:60, 10:30] = 2                      # merged: two touching gt cells, one prediction
    gt[40:60, 30:50] = 3
    seg[40:60, 10:50] = 1
    gt[10:30, 70:100] = 4                     # exact
    seg[10:30, 70:100] = 1
    gt[40:60, 70:90] = 5                      # a diagonal contact joins two predicted squares (8-connectivity)
    seg[40:50, 70:80] = 1
    seg[50:60, 80:90] = 1
    gt[36:64, 100:126] = 6                    # three small predictions in one large cell
    seg[38:46, 102:110] = 1
    seg[38:46, 114:122] = 1
    seg[52:60, 102:122] = 1
    return gt, seg


def _ring():
    """2 x 2 and larger cells on the 2-pixel ring, straddling it, and just inside it, on every side; 41 x 47"""
    H, W = 41, 47
    gt, seg = np.zeros((H, W), np.int32), np.zeros((H, W), np.uint8)
    boxes = [(0, 2, 5, 7), (1, 3, 10, 12), (2, 4, 15, 17), (3, 5, 20, 22),                # top: on, straddling, just inside, inside
             (H - 2, H, 5, 7), (H - 3, H - 1, 10, 12), (H - 4, H - 2, 15, 17),            # bottom
             (10, 12, 0, 2), (14, 16, 1, 3), (18, 20, 2, 4),                              # left
             (10, 12, W - 2, W), (14, 16, W - 3, W - 1), (18, 20, W - 4, W - 2),          # right
             (24, 32, 20, 30)]                                                           # centre
    for k, (r0, r1, c0, c1) in enumerate(boxes):
        gt[r0:r1, c0:c1] = k + 1
        seg[r0:r1, c0:c1] = 1
    seg[2:4, 15:17] = 0                       # the prediction of the cell just inside the top ring instead touches the ring
    seg[1:4, 15:17] = 1
    seg[24:32, 20:30] = 0
    seg[25:32, 20:30] = 1
    return gt, seg


def _gaps():
    """non-sequential gt labels with gaps, in an order that is not the raster order; 90 x 77"""
    gt, seg = _discs((90, 77), 12, 5, rmin=3, rmax=6)
    lut = np.arange(13, dtype=np.int32)
    lut[1:] = [70000, 5, 17, 300, 9, 1000, 12, 65535, 65536, 40, 2, 123456]
    return lut[gt], seg


def _uint16():
    gt, seg = _discs((64, 128), 10, 11, dtype=np.uint16)
    return gt, seg


def _empty_seg():
    gt, seg = _discs((50, 60), 5, 3)
    return gt, np.where(seg == 1, 2, seg).astype(np.uint8)       # other classes only


def _empty_gt():
    gt, seg = _discs((50, 60), 5, 4)
    return np.zeros_like(gt), seg


def _both_empty():
    return np.zeros((33, 35), np.int32), np.zeros((33, 35), np.uint8)


CASES = {
    "discs": lambda: _discs((150, 203), 30, 7),
    "dense": lambda: _discs((97, 131), 60, 9, rmin=3, rmax=7, jitter=3),
    "split_merge": _split_merge,
    "ring": _ring,
    "gaps": _gaps,
    "uint16": _uint16,
    "empty_seg": _empty_seg,
    "empty_gt": _empty_gt,
    "both_empty": _both_empty,
}


def _tie():
    """one gt cell covered exactly half-and-half by two predictions: both IoU are exactly 0.5"""
    t, p = np.zeros((20, 30), np.int32), np.zeros((20, 30), np.int32)
    t[4:14, 6:14] = 1
    p[4:14, 6:10] = 1
    p[4:14, 10:14] = 2
    t[15:19, 20:28] = 2                       # and an ordinary pair
    p[15:19, 21:28] = 3
    return t, p


def _sparse_labels():
    """labels with gaps on both sides: empty rows and columns in the matrices"""
    t, p = np.zeros((24, 24), np.int32), np.zeros((24, 24), np.int32)
    t[2:10, 2:10] = 3
    t[12:20, 12:20] = 7
    p[3:10, 2:10] = 2
    p[12:20, 13:22] = 9
    p[0:2, 20:24] = 4
    return t, p


def _no_background():
    """no background pixel at all"""
    t, p = np.ones((8, 8), np.int32), np.ones((8, 8), np.int32)
    t[:, 4:] = 2
    p[5:, :] = 2
    return t, p


PAIRS = {"tie": _tie, "sparse_labels": _sparse_labels, "no_background": _no_background}


def big_case():
    """5002 x 5003 (above the 25 M-pixel switch, not a multiple of the 2000-pixel tile), 80 sparse cells, some across tile borders"""
    gt, seg = _discs(BIG_SHAPE, 80, 101, rmin=8, rmax=20, extra=6, jitter=3)
    for k, (cy, cx) in enumerate([(2000, 700), (1999, 2400), (3100, 2001), (4000, 3998), (5000, 1200), (2600, 5001)]):
        _disc(gt, cy, cx, 12, 1000 + k)       # on tile borders and on the image border
        _disc(seg, cy + 1, cx - 1, 12, 1)
    return gt, seg


def cells_image(shape, n, seed):
    """(gt, seg) with about n cells for tools/bench_cells.py"""
    r = max(int(0.25 * (shape[0] * shape[1] / n) ** 0.5), 3)
    return _discs(shape, n, seed, rmin=max(r // 2, 2), rmax=r, extra=n // 20, jitter=max(r // 5, 1))
