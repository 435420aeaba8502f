"""Seeded label volumes for the postprocessing tests (tests/golden/postprocess.npz, made by
tests/golden/make_golden_postprocess.py with the reference's own remove_connected_components.py) and the synthetic BTCV-like case
of the GPU tests and tools/bench_postprocess.py."""
import numpy as np


def _box(v, lo, hi, label):
    v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = label


def _ball(v, centre, radii, label):
    X, Y, Z = v.shape
    x, y, z = np.ogrid[:X, :Y, :Z]
    d = sum(((a - c) / r) ** 2 for a, c, r in zip((x, y, z), centre, radii))
    v[d <= 1.0] = label


def _multi():
    """four labels, several components each, in a (20, 22, 26) volume"""
    v = np.zeros((20, 22, 26), np.uint8)
    rng = np.random.default_rng(23)
    _ball(v, (6, 7, 8), (4, 5, 6), 1)
    _ball(v, (14, 15, 18), (4, 4, 5), 2)
    _box(v, (2, 14, 2), (7, 20, 7), 3)
    _box(v, (12, 2, 15), (18, 6, 24), 4)
    for label in (1, 2, 3, 4):                                  # islands of one to eight voxels
        for _ in range(4):
            p = rng.integers(0, (19, 21, 25))
            s = rng.integers(1, 3, 3)
            _box(v, p, np.minimum(p + s, v.shape), label)
    return v


def _ties():
    """label 1: two 3 x 3 x 3 cubes (a tie for the maximum) and a 2 x 2 x 2 cube; label 2: two single voxels"""
    v = np.zeros((12, 12, 12), np.uint8)
    _box(v, (1, 1, 1), (4, 4, 4), 1)
    _box(v, (7, 7, 7), (10, 10, 10), 1)
    _box(v, (1, 8, 1), (3, 10, 3), 1)
    v[10, 1, 10] = 2
    v[1, 10, 10] = 2
    return v


def _contacts():
    """label 1: a 3 x 3 x 3 cube A (27); two 2 x 2 x 4 bars B, C (16 each) joined only through an edge, and a bar D (16) joined to C
    only through a corner -- B + C + D (48) is the largest only with full connectivity.  Label 2: an 18-connected L and a diagonal
    chain of voxels joined by corners only."""
    v = np.zeros((14, 16, 18), np.uint8)
    _box(v, (10, 11, 12), (13, 14, 15), 1)                      # A
    _box(v, (1, 1, 1), (3, 3, 5), 1)                            # B: x 1-2, y 1-2
    _box(v, (3, 3, 1), (5, 5, 5), 1)                            # C: x 3-4, y 3-4 -> touches B along the edge (2, 2, z) / (3, 3, z)
    _box(v, (5, 5, 5), (7, 7, 9), 1)                            # D: touches C only at the corner (4, 4, 4) / (5, 5, 5)
    for i in range(10):
        v[1 + i, 6 + i, 8 + i] = 2                              # corner chain of ten voxels
    _box(v, (8, 1, 12), (10, 3, 14), 2)                         # 8 voxels: the largest unless the chain is one component
    return v


def _two_d():
    v = np.zeros((1, 40, 36), np.uint8)
    _box(v, (0, 3, 3), (1, 20, 15), 1)
    _box(v, (0, 21, 16), (1, 24, 20), 1)                        # corner contact with the first box in the plane
    _box(v, (0, 30, 2), (1, 34, 6), 1)
    _box(v, (0, 5, 25), (1, 12, 33), 2)
    _box(v, (0, 30, 28), (1, 32, 30), 2)
    return v


# tag: (volume, labels_or_regions, background_label, what it covers)
VOLUMES = {
    "multi": _multi,
    "ties": _ties,
    "contacts": _contacts,
    "two_d": _two_d,
}
CALLS = {
    "multi_fg": ("multi", [1, 2, 3, 4], 0, "all foreground labels united"),
    "multi_1": ("multi", 1, 0, "one label"),
    "multi_subset": ("multi", [2, 4], 0, "labels 1 and 3 are outside the requested set"),
    "multi_region": ("multi", (1, 3), 0, "a region tuple"),
    "multi_list_of_regions": ("multi", [(1, 3), 2], 0, "a list of a region and a label"),
    "multi_bg7": ("multi", [1, 2], 7, "background_label 7"),
    "multi_empty": ("multi", 9, 0, "an empty class"),
    "ties_1": ("ties", 1, 0, "two components tie for the maximum"),
    "ties_2": ("ties", 2, 0, "single-voxel ties"),
    "contacts_1": ("contacts", 1, 0, "edge and corner contacts (18- and 26-neighbours)"),
    "contacts_2": ("contacts", 2, 0, "a corner-only chain"),
    "contacts_fg": ("contacts", [1, 2], 0, "labels 1 and 2 united"),
    "two_d_fg": ("two_d", [1, 2], 0, "a (1, H, W) image"),
    "two_d_1": ("two_d", 1, 0, "a (1, H, W) image, one label"),
}


# ------------------------------------------------------------------------------------------------
# cross-validation sets for determine_postprocessing: (predictions, references, foreground labels, ignore label, what it covers)
# ------------------------------------------------------------------------------------------------
SHAPE = (16, 18, 20)


def _islands(v, label, n, rng, avoid=None):
    for _ in range(n):
        while True:
            p = rng.integers(0, np.array(SHAPE) - 2)
            if avoid is None or not avoid[p[0]:p[0] + 2, p[1]:p[1] + 2, p[2]:p[2] + 2].any():
                break
        _box(v, p, p + rng.integers(1, 3, 3), label)


def _set_a(rng):
    """touching organs 1 | 2, islands of both, some touching the other organ: the foreground step is accepted, then both
    per-class steps (the islands that touch the other organ)"""
    preds, refs = [], []
    for c in range(3):
        r = np.zeros(SHAPE, np.uint8)
        _box(r, (3 + c, 3, 3), (9 + c, 10, 10), 1)
        _box(r, (9 + c, 3, 3), (13, 10, 10), 2)
        p = r.copy()
        _islands(p, 1, 3, rng, avoid=r > 0)
        _islands(p, 2, 2, rng, avoid=r > 0)
        preds.append(p)
        refs.append(r)
    return preds, refs, [1, 2], None


def _set_b(rng):
    """separate organs: the foreground mean rises (label 1 loses its islands) but label 2, poorly predicted, falls to 0 -> rejected;
    then the per-class step of label 1 is accepted and that of label 2 (one component) is not"""
    preds, refs = [], []
    for c in range(3):
        r = np.zeros(SHAPE, np.uint8)
        _box(r, (2, 2, 2), (8, 9, 9), 1)
        _box(r, (12, 13, 14), (15, 17, 19), 2)
        p = np.zeros(SHAPE, np.uint8)
        _box(p, (2, 2, 2), (8, 9, 9), 1)
        _box(p, (14, 16, 17), (16, 18, 20), 2)                   # overlaps the reference of label 2 a little
        _islands(p, 1, 20, rng, avoid=np.pad((r > 0) | (p > 0), 1)[:-2, :-2, :-2] | (r > 0) | (p > 0))
        preds.append(p)
        refs.append(r)
    return preds, refs, [1, 2], None


def _set_c(rng):
    """three separate labels: foreground step rejected; label 1 (islands) accepted, label 2 (the reference has two pieces too)
    rejected, label 3 (clean) rejected; label 3 is absent from one case (NaN Dice there)"""
    preds, refs = [], []
    for c in range(3):
        r = np.zeros(SHAPE, np.uint8)
        _box(r, (1, 1, 1), (7, 8, 8), 1)
        _box(r, (9, 1, 1), (14, 6, 6), 2)
        _box(r, (9, 9, 1), (11, 11, 3), 2)
        if c != 1:
            _box(r, (8, 10, 10), (14, 16, 17), 3)
        p = r.copy()
        _islands(p, 1, 3, rng, avoid=r > 0)
        preds.append(p)
        refs.append(r)
    return preds, refs, [1, 2, 3], None


def _set_d(rng):
    """an ignore label (4) in the references: islands of label 1 inside the ignored region do not count"""
    preds, refs = [], []
    for c in range(3):
        r = np.zeros(SHAPE, np.uint8)
        _box(r, (2, 2, 2), (8, 9, 9), 1)
        _box(r, (9, 2, 2), (13, 8, 8), 2)
        _box(r, (0, 12, 12), (16, 18, 20), 4)
        p = np.where(r == 4, 0, r).astype(np.uint8)
        _box(p, (3, 13, 13), (5, 15, 15), 1)                     # inside the ignored region
        _box(p, (10, 14, 3), (12, 16, 5), 2)                     # outside it
        if c == 2:
            _box(p, (9, 10, 10), (10, 11, 11), 1)
        preds.append(p)
        refs.append(r)
    return preds, refs, [1, 2], 4


CV_SETS = {"a_fg_accepted": _set_a, "b_fg_rejected_class_falls": _set_b, "c_some_classes": _set_c, "d_ignore_label": _set_d}


def cv_set(tag):
    return CV_SETS[tag](np.random.default_rng(sorted(CV_SETS).index(tag) + 100))


# ------------------------------------------------------------------------------------------------
# synthetic BTCV-like prediction: 13 organs as ellipsoids in (512, 512, 150), spurious islands, edge / corner contacts and ties
# ------------------------------------------------------------------------------------------------
def btcv_like(shape=(512, 512, 150), seed=0):
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, np.uint8)
    X, Y, Z = shape
    for label in range(1, 14):
        c = (rng.uniform(0.2, 0.8) * X, rng.uniform(0.2, 0.8) * Y, rng.uniform(0.25, 0.75) * Z)
        r = (rng.uniform(0.04, 0.14) * X, rng.uniform(0.04, 0.14) * Y, rng.uniform(0.08, 0.2) * Z)
        lo = [max(0, int(a - b) - 1) for a, b in zip(c, r)]
        hi = [min(s, int(a + b) + 2) for a, b, s in zip(c, r, shape)]
        sub = v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        x, y, z = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        d = ((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2
        sub[d <= 1.0] = label
    for _ in range(600):                                        # islands of 1 to 64 voxels
        p = rng.integers(0, np.array(shape) - 4)
        s = rng.integers(1, 5, 3)
        v[p[0]:p[0] + s[0], p[1]:p[1] + s[1], p[2]:p[2] + s[2]] = rng.integers(1, 14)
    # label 14: two 3 x 3 x 3 cubes, one with a 2 x 2 x 2 cube joined through an edge, the other with one joined through a corner:
    # an exact tie for the maximum (35 voxels each) that only full connectivity produces
    v[0:12, 0:12, 0:12] = 0
    v[0:12, 496:512, 136:150] = 0
    v[4:7, 4:7, 4:7] = 14
    v[7:9, 7:9, 4:6] = 14                                       # edge contact: (6, 6, 4) - (7, 7, 4)
    v[4:7, 500:503, 140:143] = 14
    v[7:9, 503:505, 143:145] = 14                               # corner contact: (6, 502, 142) - (7, 503, 143)
    return v
