"""Cases, references and path predicates for K24 (csrc/surface.hip: sf_stats / sf_codes / sf_zpass / sf_ypass / sf_xpass / sf_sum) at
the sizes where its launchers and loops change path: shared by tests/test_surface_paths_cpu.py and tests/test_surface_paths_gpu.py.

A CASE is a namedtuple and the seed of its own inputs (zlib.crc32(repr(case))):
    MaskCase(group, name, shape, spacing, tols, form)   one gt / prediction mask pair; `form` is how the masks are handed to the device
                                                        ("u8", "bool", "values": uint8 with values other than 1, "view": non-contiguous)
    LabelCase(group, name, shape, spacing, tols, slabs) label volumes for surface._device_run / surface.case_nsd; label k has tols[k - 1]
    StatsCase(group, name, shape, wanted)               label volumes for ops.surface_stats alone
GROUPS maps a group name to its cases.  RAW_CROPS is a hand-written crop list with n = 0 axes (D = 1): surface._device_layout never
makes one (a measured label has n >= 1), ops.surface_prepare accepts it, and it is the only way to a line of length 1.

REFERENCES restate the operation and never call mlagg_unet_amd.surface's host path:
    reference        SurfaceDice.compute_surface_distances: union box + one zero plane, scipy correlate with the 2x2x2 kernel, surfels
                     are the codes other than 0 and 255, scipy distance_transform_edt(~border, sampling) in float64;
    brute_force      min over all surfels of the other set of sqrt(((dx s0)^2 + (dy s1)^2) + (dz s2)^2): the independent check of
                     `reference`, run where the surfel-count product is at most BRUTE_CAP;
    reference_stats  the (256, 10) integers of mlagg_surface_stats;
    reference_case   the per-organ loop of the *_NSD_Eval.py scripts, with the four unrounded sums and the unrounded NSD.
Only the surfel area table comes from surface.surface_area_table, which tests/test_surface_cpu.py pins to the golden.

BOUNDS come from the existing tests and the references, never from the kernel: distances and areas 1e-12 relative (the golden
test's), the in-plane feature distance 1e-12 relative against a per-plane scipy transform, sums and ratios 1e-9 relative (the bound
the golden test gives the NSD made of them), integers and codes exact.  TOLERANCE GAP: no reference distance of a case lies within
1e-9 relative of one of its tolerances unless it equals it (asserted on the host), so the d <= tol decisions of a kernel correct to
1e-12 are determined.  EXCEPTIONS would list a (case, quantity) that needs a wider bound, with the measured figure and the reason.

PATH PREDICATES are pure functions that name the source line they mirror; tests/test_surface_paths_cpu.py asserts that the table
reaches every value of REACH.  UNCOVERED lists what the table cannot reach and why.

MEASURED on an MI355X (profiles/surface_kernel_paths_mi355x.log) -- largest device error per group, relative; the GPU test file takes
2.6 s (47 tests, none above 0.2 s):

    group           distances, areas   in-plane ft distance   pair slices   sums and ratios
    lines           0                  0                      -             4.6e-16
    carries         0                  0                      -             1.8e-16
    degenerate      0                  0                      -             2.6e-16
    maxline         0                  0                      -             6.0e-16
    inclusive_tol   0                  0                      -             5.8e-16
    labels          -                  0                      0             3.6e-16
    stats           every integer equal

Every distance is bit-identical to scipy's, no case needs an exception, and the launch at D = MLAGG_SURFACE_MAX_LINE (61 448 bytes of
dynamic LDS, 2 052 static in the x pass) is accepted on both axes: the documented limit holds.  The sums differ from numpy's
pairwise sums by summation order only.
"""
import collections
import functools
import math
import zlib
from collections import OrderedDict

import numpy as np
import scipy.ndimage as ndi

F32 = np.float32
MaskCase = collections.namedtuple("MaskCase", "group name shape spacing tols form")
LabelCase = collections.namedtuple("LabelCase", "group name shape spacing tols slabs")
StatsCase = collections.namedtuple("StatsCase", "group name shape wanted")

SF_SEG, SF_STATS_BLOCK, SF_STATS_MAX_BLOCKS, SF_WAVE, SF_SUM_BLOCK = 16, 256, 2048, 64, 256      # csrc/surface.hip
MAX_LINE = 2560                                                                                  # MLAGG_SURFACE_MAX_LINE
INT_MAX = 0x7fffffff
BRUTE_CAP = 2e7
REL_DIST, REL_SUM, REL_GAP = 1e-12, 1e-9, 1e-9
EXCEPTIONS = {}

UNCOVERED = (
    ("SF_GRID_CAP", "grid-stride loops of the codes / z / y / x passes start at 2^20 workgroups: over 2.6e8 crop voxels or 2^20 lines, "
                    "minutes of host reference"),
    ("2^31 - 1 voxels per crop", "the refusal is covered by tests/test_surface_gpu.py::test_k24_size_limits_refused; a crop that "
                                 "large cannot be referenced in seconds"),
    ("envelope of one parabola", "a voxel makes surfels at p and p + 1 on every axis, so a line with a site has at least two adjacent "
                                 "ones, and env_build never drops the first of two sites (k > 0 guards the pop): K = 1 cannot come "
                                 "from a mask.  The table reaches K = 2, two adjacent sites at one end of a line of 129, whose last "
                                 "one is queried from 127 positions away"),
)


def seed(case):
    return zlib.crc32(repr(case).encode())


def _cdiv(a, b):
    return (a + b - 1) // b


# =====================================================================================================================
# path predicates
# =====================================================================================================================
def stats_segments(Z):
    """sf_stats_kernel: nseg = (Z + SF_SEG - 1) / SF_SEG threads per (x, y) row."""
    return _cdiv(Z, SF_SEG)


def stats_seam_runs(vol, wanted):
    """sf_stats_kernel: runs of a wanted label that continue across a multiple of SF_SEG along z (flushed at `z1 - 1` by one thread
    and restarted at `sg = z0` by the next): how many (x, y, seam) there are."""
    Z = vol.shape[2]
    n = 0
    for k in range(SF_SEG, Z, SF_SEG):
        a, b = vol[:, :, k - 1], vol[:, :, k]
        n += int(((a == b) & np.isin(a, list(wanted))).sum())
    return n


def stats_grid_stride(shape):
    """mlagg_surface_stats: blocks = min(ceil(work / 256), 2048); the `w += stride` loop of sf_stats_kernel runs twice from there."""
    X, Y, Z = shape
    return X * Y * stats_segments(Z) > SF_STATS_MAX_BLOCKS * SF_STATS_BLOCK


def codes_mixed_waves(crop_voxels):
    """sf_codes_kernel `__all(i == __shfl(i, first))`: the number of 64-voxel waves of the launch that hold more than one crop (they
    take the per-lane atomics); 0: every wave takes the wave-uniform branch."""
    edges = np.cumsum(crop_voxels)[:-1]
    return int(len({int(e) // SF_WAVE for e in edges if e % SF_WAVE}))


def zpass_chunks(D2):
    """sf_zpass_kernel: `for (z0 = 0; z0 < c.D2; z0 += SF_WAVE)`."""
    return _cdiv(D2, SF_WAVE)


def zpass_hops(border):
    """sf_zpass_kernel `v = max(v, carry)` / `v = min(v, carry)`: over all lines and positions, the largest number of chunk ends
    between a position and the last surfel before it (forward) and the first one after it (backward), and whether a line has no
    surfel at all."""
    D2 = border.shape[2]
    z = np.arange(D2)
    prev = np.maximum.accumulate(np.where(border, z, -1), axis=2)
    nxt = np.minimum.accumulate(np.where(border, z, INT_MAX)[:, :, ::-1], axis=2)[:, :, ::-1]
    fwd = np.where(prev >= 0, z // SF_WAVE - prev // SF_WAVE, 0).max()
    bwd = np.where(nxt != INT_MAX, nxt // SF_WAVE - z // SF_WAVE, 0).max()
    return int(fwd), int(bwd), bool((~border.any(axis=2)).any())


def lane_trips(D):
    """sf_ypass_kernel / sf_xpass_kernel: `for (y = lane; y < c.D1; y += SF_WAVE)`."""
    return _cdiv(D, SF_WAVE)


def line_sites(border):
    """The number of sites (finite keys) of the y lines and of the x lines: position y of a y line of plane x is a site when the z
    line (x, y) has a surfel; position x of an x line is one when plane x has a surfel.  ({counts over planes x}, count)."""
    return {int(v) for v in border.any(axis=2).sum(axis=1)}, int(border.any(axis=(1, 2)).sum())


def env_build(f, w):
    """env_build of csrc/surface.hip in the same float64 operations: (sites v, breakpoints zb) of the lower envelope."""
    v, zb = [], []
    for q, fq in enumerate(f):
        if math.isinf(fq):
            continue
        hq = fq + w * float(q) * float(q)
        if not v:
            v, zb = [q], [-math.inf]
            continue
        while True:
            p = v[-1]
            s = (hq - (f[p] + w * float(p) * float(p))) / (2.0 * w * float(q - p))
            if len(v) > 1 and s <= zb[-1]:
                v.pop(), zb.pop()
            else:
                break
        v.append(q), zb.append(s)
    return v, zb


def sum_lines(D):
    """sf_sum_kernel: `for (l = l0 + t; l < l1; l += 256)` over the label's D1 * D2 line partials: "<", "==" or ">" one trip."""
    n = D[1] * D[2]
    return "<" if n < SF_SUM_BLOCK else "==" if n == SF_SUM_BLOCK else ">"


REACH = {
    "stats_segments": {1: 1, 15: 1, 16: 1, 17: 2, 33: 3},                      # Z -> nseg
    "stats_grid_stride": {False, True},
    "codes_all_waves_uniform": {False, True},
    "zpass_D2": {1, 2, 63, 64, 65, 128, 129},
    "zpass_chunks": {1, 2, 3},
    "trips_D": {1, 2, 64, 65, 129},                                            # D1 and D0 each
    "sum_lines": {"<", "==", ">"},
}


# =====================================================================================================================
# references
# =====================================================================================================================
KERNEL = np.array([[[128, 64], [32, 16]], [[8, 4], [2, 1]]])
Ref = collections.namedtuple("Ref", "lo n codes borders dist d_gt a_gt d_pred a_pred")


def area_table(spacing):
    from mlagg_unet_amd import surface
    return surface.surface_area_table(spacing)


def reference(mask_gt, mask_pred, spacing):
    """SurfaceDice.compute_surface_distances restated; None when both masks are empty.  lo / n: the union box's origin and extents
    (the crop is n + 1); codes, borders, dist: [gt, prediction]; d_* / a_*: the unsorted (distance to the other surface, area) of
    every surfel in C order of the crop."""
    g, p = np.asarray(mask_gt) != 0, np.asarray(mask_pred) != 0
    idx = np.nonzero(g | p)
    if len(idx[0]) == 0:
        return None
    lo = tuple(int(i.min()) for i in idx)
    n = tuple(int(i.max()) - l + 1 for i, l in zip(idx, lo))
    box = tuple(slice(l, l + k) for l, k in zip(lo, n))
    sampling = [float(v) for v in spacing]
    codes, borders, dist = [], [], []
    for m in (g, p):
        crop = np.zeros(tuple(k + 1 for k in n), np.uint8)
        crop[:-1, :-1, :-1] = m[box]
        code = ndi.correlate(crop, KERNEL, mode="constant", cval=0)
        b = (code != 0) & (code != 255)
        codes.append(code), borders.append(b)
        dist.append(ndi.distance_transform_edt(~b, sampling=sampling) if b.any() else np.full(b.shape, np.inf))
    table = area_table(spacing)
    return Ref(lo, n, codes, borders, dist, dist[1][borders[0]], table[codes[0][borders[0]]], dist[0][borders[1]],
               table[codes[1][borders[1]]])


def brute_force(border_a, border_b, spacing):
    """For every surfel of a (C order) the distance to the nearest surfel of b, by trying them all; +inf when b has none."""
    s = [float(v) for v in spacing]
    A, B = np.argwhere(border_a).astype(np.float64), np.argwhere(border_b).astype(np.float64)
    if len(B) == 0:
        return np.full(len(A), np.inf)
    out = np.empty(len(A))
    step = max(1, int(4e6 // len(B)))
    for i in range(0, len(A), step):
        a = A[i:i + step, None, :]
        dx, dy, dz = ((a[..., k] - B[None, :, k]) * s[k] for k in range(3))
        out[i:i + step] = np.sqrt(((dx * dx + dy * dy) + dz * dz).min(axis=1))
    return out


def brute_cost(ref):
    return float(ref.borders[0].sum()) * float(ref.borders[1].sum())


def reference_stats(gt, seg, wanted):
    """(256, 10) int64 of mlagg_surface_stats: gt count, prediction count, union box x / y / z min and max, the gt's z min and max;
    INT_MAX / -1 where empty; an unwanted label keeps these initial values."""
    out = np.zeros((256, 10), np.int64)
    out[:, 2::2], out[:, 3::2] = INT_MAX, -1
    gt, seg = np.asarray(gt).astype(np.uint8), np.asarray(seg).astype(np.uint8)          # (a bool mask is label 1)
    for lab in sorted(set(np.unique(gt).tolist()) | set(np.unique(seg).tolist())):
        if lab not in wanted:
            continue
        g, p = gt == lab, seg == lab
        out[lab, 0], out[lab, 1] = int(g.sum()), int(p.sum())
        for ax, idx in enumerate(np.nonzero(g | p)):
            out[lab, 2 + 2 * ax], out[lab, 3 + 2 * ax] = int(idx.min()), int(idx.max())
        if out[lab, 0]:
            z = np.nonzero(g.any(axis=(0, 1)))[0]
            out[lab, 8], out[lab, 9] = int(z.min()), int(z.max())
    return out


Organ = collections.namedtuple("Organ", "label fixed zcut ref sums nsd")


def _sums(ref, tol):
    return (float(np.sum(ref.a_gt)), float(np.sum(ref.a_gt[ref.d_gt <= tol])), float(np.sum(ref.a_pred)),
            float(np.sum(ref.a_pred[ref.d_pred <= tol])))


def reference_case(gt, seg, spacing, tolerances, slab_labels, measure_empty_gt=False):
    """The scripts' per-organ loop: organ k of `tolerances` is label k.  fixed 1 when both masks are empty, 0 when only the gt is
    (measured all the same under measure_empty_gt, as compute_surface_distances does); a slab label is cut to the gt's half-open
    [z_lower, z_upper) first (ValueError when that is empty).  sums: gt area, gt area within tol, prediction area, prediction area
    within tol; nsd unrounded.  The Ref's box is relative to the cut volume: zcut[0] has to be added to its lo[2]."""
    gt, seg = np.asarray(gt), np.asarray(seg)
    out = OrderedDict()
    for lab, (organ, tol) in enumerate(tolerances.items(), 1):
        g, s = gt == lab, seg == lab
        if not g.any() and not s.any():
            out[organ] = Organ(lab, 1, None, None, None, 1.0)
            continue
        if not g.any() and not measure_empty_gt:
            out[organ] = Organ(lab, 0, None, None, None, 0.0)
            continue
        zcut = None
        if lab in slab_labels:
            z = np.nonzero(g.any(axis=(0, 1)))[0]
            zcut = (int(z.min()), int(z.max()))
            if zcut[0] == zcut[1]:
                raise ValueError(f"label {lab}: empty [z_lower, z_upper)")
            g, s = g[:, :, zcut[0]:zcut[1]], s[:, :, zcut[0]:zcut[1]]
        ref = reference(g, s, spacing)
        sums = _sums(ref, float(tol))
        with np.errstate(divide="ignore", invalid="ignore"):
            nsd = float(np.float64(sums[1] + sums[3]) / np.float64(sums[0] + sums[2]))
        out[organ] = Organ(lab, None, zcut, ref, sums, nsd)
    return out


def embed(ref, zcut, lo, n):
    """The reference's code volumes and borders inside the device's crop (origin lo, extents n, dims n + 1), which contains the
    reference's box: zero codes around it (the masks are empty there)."""
    off = [r - l for r, l in zip(ref.lo, lo)]
    if zcut is not None:
        off[2] += zcut[0]
    D = tuple(k + 1 for k in n)
    assert all(o >= 0 and o + k + 1 <= d for o, k, d in zip(off, ref.n, D)), (off, ref.n, D)
    sl = tuple(slice(o, o + k + 1) for o, k in zip(off, ref.n))
    codes = []
    for c in ref.codes:
        full = np.zeros(D, np.uint8)
        full[sl] = c
        codes.append(full)
    return codes, [(c != 0) & (c != 255) for c in codes]


def check_ft(ft, border, spacing):
    """The packed feature transform after the z and y passes against one mask's surfels, plane by plane along x: -1 exactly on the
    planes without a surfel, elsewhere (fy, fz) is a surfel of the plane and its in-plane distance is scipy's.  Returns the largest
    relative error (0 where both distances are 0); raises AssertionError on a structural fault."""
    D0, D1, D2 = border.shape
    ft = np.asarray(ft).reshape(border.shape)
    s1, s2 = float(spacing[1]), float(spacing[2])
    y, z = np.mgrid[:D1, :D2]
    worst = 0.0
    for x in range(D0):
        b, f = border[x], ft[x]
        if not b.any():
            assert (f == -1).all(), f"plane {x}: no surfel, but a feature"
            continue
        assert (f >= 0).all() and (f < D1 * D2).all(), f"plane {x}: a position without a feature"
        fy, fz = f // D2, f % D2
        assert b[fy, fz].all(), f"plane {x}: a feature that is no surfel"
        a, c = (y - fy).astype(np.float64) * s1, (z - fz).astype(np.float64) * s2
        got = np.sqrt(a * a + c * c)
        want = ndi.distance_transform_edt(~b, sampling=[s1, s2])
        assert np.array_equal(got == 0, want == 0), f"plane {x}: zero distances differ"
        nz = want > 0
        if nz.any():
            worst = max(worst, float((np.abs(got[nz] - want[nz]) / want[nz]).max()))
    return worst


def sort_pairs(d, a):
    order = np.lexsort((a, d))
    return d[order], a[order]


def rel_err(got, want):
    """Largest relative error over the finite entries; the infinities must sit in the same places and the lengths agree."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not np.isnan(got).any()
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
    fin = np.isfinite(want)
    zero = fin & (want == 0)
    assert (got[zero] == 0).all()
    nz = fin & ~zero
    return float((np.abs(got[nz] - want[nz]) / np.abs(want[nz])).max()) if nz.any() else 0.0


def check_rounded(got, exact):
    """round(exact, 4), except that within 1e-5 of a rounding boundary either neighbour passes (tests/test_surface_cpu.py)."""
    want = round(exact, 4)
    if abs((exact * 1e4) % 1 - 0.5) < 1e-5:
        assert abs(got - want) <= 1e-4 + 1e-12, (got, exact)
    else:
        assert got == want, (got, exact)


def tolerance_gap_ok(ref, tol, exact=()):
    """No distance within REL_GAP of tol unless it equals it -- or equals one of `exact`: inclusive_tol puts a tolerance one ulp
    below 3.0 = sqrt(9) on an isotropic unit grid, where the squared distance is an exact integer and IEEE sqrt returns 3.0 itself."""
    for d in (ref.d_gt, ref.d_pred):
        d = d[np.isfinite(d) & ~np.isin(d, list(exact))]
        if ((np.abs(d - tol) <= REL_GAP * tol) & (d != tol)).any():
            return False
    return True


# =====================================================================================================================
# inputs
# =====================================================================================================================
def _ellipsoid(shape, centre, radii):
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return sum(((a - c) / r) ** 2 for a, c, r in zip((x, y, z), centre, radii)) <= 1.0


_AXES = {"z": (0, 1, 2), "y": (0, 2, 1), "x": (2, 1, 0)}


def _masks(case):
    rng = np.random.default_rng(seed(case))
    sh, name = case.shape, case.name
    g, p = np.zeros(sh, bool), np.zeros(sh, bool)
    if case.group == "lines":                       # a dense ellipsoid filling the volume, 2 % knocked out; the prediction rolled
        g = _ellipsoid(sh, [(v - 1) / 2 for v in sh], [v / 2 for v in sh]) & (rng.random(sh) >= 0.02)
        p = np.roll(g, (2, -3, 1), (0, 1, 2))
    elif case.group == "carries":
        kind, axis = name.split("_")[0], name.split("_")[1]
        perm = _AXES[axis]
        csh = tuple(sh[i] for i in perm)            # canonical: the long axis last
        a, b = np.zeros(csh, bool), np.zeros(csh, bool)
        if kind == "tie":                           # the gt's surfel at 15 lies midway between the prediction's at 11 and 19
            a[1, 1, 10] = a[1, 1, 19] = True
            b[1, 1, 15] = True
            g, p = b, a
        else:                                       # one cluster at the low end against surfels at the high end only;
            a[0:2, 0:2, 0] = True                   # the lines (3, 3), (3, 4) .. have no surfel of either mask
            b[0:2, 0:2, csh[2] - 1] = True
            b[5, 6, csh[2] - 1] = True
            g, p = (b, a) if kind == "low" else (a, b)          # "low": the prediction is the low cluster
        g, p = np.ascontiguousarray(g.transpose(perm)), np.ascontiguousarray(p.transpose(perm))
    elif case.group == "degenerate":
        if name in ("voxel", "cube3"):
            g[:], p[:] = True, True
        elif name in ("line_y", "line_x"):
            g[:] = True
            p[:] = True
            p.reshape(-1)[[3, 17, 18]] = False
        elif name == "empty_pred":
            g = _ellipsoid(sh, (4, 5, 3), (3, 4, 2.5))
        elif name == "empty_gt":
            p = _ellipsoid(sh, (4, 5, 3), (3, 4, 2.5))
        else:                                       # faces and the dtype forms: both masks touch every face of the volume
            g = _ellipsoid(sh, (4, 5, 3), (6, 7, 5))
            p[0:5, :, 2:] = True
            p[:, 0, :] = True
    elif case.group == "maxline":
        axis = int(np.argmax(sh))
        idx = [slice(None)] * 3
        if name.startswith("sparse"):               # a voxel at either end of the long axis
            for k in (0, sh[axis] - 2):
                idx[axis] = k
                g[tuple(idx)][0, 0] = True
        else:
            idx[axis] = slice(0, sh[axis] - 1)
            g[tuple(idx)] = True
            g &= rng.random(sh) >= 0.02
            idx[axis] = 0
            g[tuple(idx)] = True                    # the union spans the whole axis whatever was knocked out
            idx[axis] = sh[axis] - 2
            g[tuple(idx)] = True
        p = np.roll(g, 1, axis)                     # (the last plane of g is empty: nothing wraps)
    elif case.group == "inclusive_tol":
        g[2:12, 2:12, 2:4] = True
        p[2:12, 2:12, 5:7] = True
    else:
        raise KeyError(case)
    return g, p


@functools.lru_cache(maxsize=None)
def masks(case):
    """(gt, prediction) bool arrays; read-only."""
    g, p = _masks(case)
    g.setflags(write=False), p.setflags(write=False)
    return g, p


def _blob(vol, lab, box, rng=None, p=0.0):
    m = np.ones(tuple(b.stop - b.start for b in box), bool)
    if rng is not None and p:
        m &= rng.random(m.shape) >= p
        m[0, 0, 0] = m[-1, -1, -1] = True           # the box stays the blob's bounding box
    vol[box][m] = lab


def _sl(*abc):
    return tuple(slice(a, b) for a, b in abc)


@functools.lru_cache(maxsize=None)
def volumes(case):
    """(gt, seg) uint8 label volumes of a LabelCase or StatsCase; read-only."""
    rng = np.random.default_rng(seed(case))
    sh = case.shape
    gt, seg = np.zeros(sh, np.uint8), np.zeros(sh, np.uint8)
    if case.group == "labels" and case.name == "eight":
        #  1: a noisy ellipsoid, the prediction shifted: more than 256 x lines
        m = _ellipsoid(sh, (12, 12, 14), (9, 10, 11))
        gt[m & (rng.random(sh) >= 0.03)] = 1
        seg[np.roll(m, (1, -2, 1), (0, 1, 2)) & (rng.random(sh) >= 0.03)] = 1
        #  2: n1 = n2 = 15, so D1 * D2 = 256 lines exactly; the prediction lies inside the gt's box
        _blob(gt, 2, _sl((30, 36), (2, 17), (2, 17)), rng, 0.05)
        _blob(seg, 2, _sl((31, 35), (4, 15), (3, 16)), rng, 0.05)
        #  3: a small one, D1 * D2 = 6 * 8 lines
        _blob(gt, 3, _sl((40, 44), (30, 34), (20, 26)))
        _blob(seg, 3, _sl((41, 46), (31, 35), (21, 27)))
        #  4: missing from the prediction; 5: only predicted; 6: in neither
        _blob(gt, 4, _sl((26, 30), (24, 38), (2, 20)), rng, 0.1)
        _blob(seg, 5, _sl((36, 41), (20, 27), (3, 8)), rng, 0.1)
        #  7: a slab label whose prediction extends beyond the gt's z range on both sides
        _blob(gt, 7, _sl((2, 7), (30, 36), (10, 21)), rng, 0.05)
        _blob(seg, 7, _sl((4, 9), (28, 34), (5, 29)), rng, 0.05)
        #  8: a slab label whose prediction lies wholly outside the gt's z range
        _blob(gt, 8, _sl((14, 18), (32, 37), (4, 9)))
        _blob(seg, 8, _sl((14, 18), (32, 37), (20, 26)))
    elif case.group == "labels":                    # three labels, isotropic
        _blob(gt, 1, _sl((1, 8), (1, 11), (1, 6)), rng, 0.1)
        _blob(seg, 1, _sl((2, 9), (1, 10), (2, 7)), rng, 0.1)
        _blob(gt, 2, _sl((10, 13), (2, 19), (8, 13)), rng, 0.1)
        _blob(seg, 2, _sl((10, 14), (3, 18), (6, 12)), rng, 0.1)
        _blob(gt, 3, _sl((15, 20), (12, 15), (1, 19)), rng, 0.1)
        _blob(seg, 3, _sl((15, 19), (12, 16), (2, 18)), rng, 0.1)
    elif case.name == "second_stride":              # label 1 only where the second grid stride reads, label 2 only in the first rows
        work_first = SF_STATS_MAX_BLOCKS * SF_STATS_BLOCK // stats_segments(sh[2])          # rows of the first stride
        x1 = work_first // sh[1] + 1
        assert x1 < sh[0] - 2
        for vol in (gt, seg):
            vol[x1:, ::7, :] = np.where(rng.random((sh[0] - x1, len(range(0, sh[1], 7)), sh[2])) < 0.3, 1, 0)
            vol[:6, ::5, :] = np.where(rng.random((6, len(range(0, sh[1], 5)), sh[2])) < 0.3, 2, 0)
            vol[500:503, 100:110, :] = 7                                                      # present, not wanted
    else:                                           # runs of the labels 0, 1, 2, 7 (not wanted) and 255 along z
        choices = np.array([0, 1, 2, 7, 255], np.uint8)
        for vol in (gt, seg):
            v = choices[rng.integers(0, 5, sh)]
            keep = rng.random(sh) < 0.7
            for z in range(1, sh[2]):
                v[:, :, z] = np.where(keep[:, :, z], v[:, :, z - 1], v[:, :, z])
            vol[:] = v
        if sh[2] > 20:                              # runs across the seams at 16 (and 32) at several (x, y)
            gt[1, 2, 9] = gt[1, 2, 21] = 0
            gt[1, 2, 10:21] = 1
            gt[3, 0, 12:sh[2]] = 255
            seg[2, 4, 15:17] = 2
            seg[0, 5, 0:sh[2]] = 1
        gt[2, 2, 0] = seg[2, 3, 0] = 7              # present, not wanted
        gt[0, 0, 0] = seg[0, 0, 0] = 2              # the first and the last voxel of the volume
        gt[-1, -1, -1] = seg[-1, -1, -1] = 255
    gt.setflags(write=False), seg.setflags(write=False)
    return gt, seg


def tolerances(case):
    return OrderedDict((f"organ{k}", t) for k, t in enumerate(case.tols, 1))


@functools.lru_cache(maxsize=None)
def mask_reference(case):
    return reference(*masks(case), case.spacing)


@functools.lru_cache(maxsize=None)
def label_reference(case, measure_empty_gt=False):
    return reference_case(*volumes(case), case.spacing, tolerances(case), case.slabs, measure_empty_gt)


# =====================================================================================================================
# the table
# =====================================================================================================================
ANISO = (0.3, 2.9, 1.7)
ACDC = (F32(1.5625), F32(1.5625), F32(10.0))
BTCV = (F32(0.78125), F32(0.78125), F32(3.0))
ISO = (1, 1, 1)


def _m(group, name, shape, spacing, tols, form="u8"):
    return MaskCase(group, name, tuple(shape), tuple(spacing), tuple(tols), form)


GROUPS = OrderedDict()
GROUPS["lines"] = (
    _m("lines", "small_z66", (12, 10, 65), ANISO, (2.0,)),                 # small enough for brute_force
    _m("lines", "x131", (130, 20, 65), ANISO, (2.0,)),
    _m("lines", "y130", (20, 129, 64), ACDC, (3.0,)),
    _m("lines", "z129", (64, 63, 128), BTCV, (2.0,)),
    _m("lines", "all", (66, 70, 131), ISO, (1.0, 2.0)),
    _m("lines", "x129", (128, 19, 63), ACDC, (5.0,)),
    _m("lines", "y129", (21, 128, 62), BTCV, (3.0,)),
    _m("lines", "z128", (63, 64, 127), ANISO, (1.0,)),
)
GROUPS["carries"] = tuple(
    _m("carries", f"{kind}_{axis}_{n}", [(6, 7, n)[i] for i in _AXES[axis]], BTCV, (50.0, 400.0))
    for axis in "zyx" for kind in ("low", "high") for n in (128, 129)
) + tuple(_m("carries", f"tie_{axis}", [(4, 4, 40)[i] for i in _AXES[axis]], ISO, (4.0, 3.5)) for axis in "zyx")
GROUPS["degenerate"] = (
    _m("degenerate", "voxel", (1, 1, 1), ANISO, (1.0,)),
    _m("degenerate", "cube3", (3, 3, 3), ISO, (1.0,)),                     # D = (4, 4, 4): 64 crop voxels, one full wave
    _m("degenerate", "line_y", (1, 40, 1), BTCV, (1.0,)),
    _m("degenerate", "line_x", (40, 1, 1), ACDC, (2.0,)),
    _m("degenerate", "empty_pred", (9, 11, 7), BTCV, (2.0,)),
    _m("degenerate", "empty_gt", (9, 11, 7), BTCV, (2.0,)),
    _m("degenerate", "faces", (9, 11, 7), BTCV, (2.0,)),
    _m("degenerate", "faces_bool", (9, 11, 7), ANISO, (2.0,), "bool"),
    _m("degenerate", "faces_values", (9, 11, 7), ANISO, (2.0,), "values"),
    _m("degenerate", "faces_view", (9, 11, 7), ANISO, (2.0,), "view"),
)
GROUPS["maxline"] = (
    _m("maxline", "y2560", (3, MAX_LINE - 1, 2), ANISO, (2.0,)),
    _m("maxline", "x2560", (MAX_LINE - 1, 3, 2), BTCV, (2.0,)),
    _m("maxline", "sparse_y2560", (3, MAX_LINE - 1, 2), ISO, (1.0,)),
)
GROUPS["inclusive_tol"] = (_m("inclusive_tol", "slab3", (14, 14, 12), ISO, (3.0, float(np.nextafter(3.0, 0.0)))),)
GROUPS["stats"] = tuple(StatsCase("stats", f"z{Z}", (5, 6, Z), (1, 2, 255)) for Z in (1, 15, 16, 17, 33)) + (
    StatsCase("stats", "second_stride", (1024, 520, 16), (1, 2, 255)),)
GROUPS["labels"] = (
    LabelCase("labels", "eight", (48, 40, 32), BTCV, (2.0, 3.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0), (7, 8)),
    LabelCase("labels", "three", (21, 20, 20), ISO, (1.0, 2.0, 1.0), ()),
)
MASK_GROUPS = ("lines", "carries", "degenerate", "maxline", "inclusive_tol")
MASK_CASES = tuple(c for g in MASK_GROUPS for c in GROUPS[g])

# crops with an axis of no mask voxel at all (D = 1): (origin, extents) in an (8, 8, 8) volume of ones
RAW_CROPS = (((1, 1, 1), (0, 3, 3)), ((2, 1, 1), (3, 0, 3)), ((1, 2, 1), (3, 3, 0)), ((4, 4, 4), (0, 0, 0)), ((3, 3, 3), (2, 2, 2)))


def case_id(case):
    return f"{case.group}-{case.name}"


def raw_desc():
    """desc rows of RAW_CROPS (label 1), laid out as surface._device_layout does."""
    rows = []
    vox = zl = yl = xl = 0
    for lo, n in RAW_CROPS:
        D = [k + 1 for k in n]
        rows.append([1, *lo, *n, vox, zl, yl, xl, 0, 0, 0, 0, 0])
        vox += D[0] * D[1] * D[2]
        zl += D[0] * D[1]
        yl += D[0] * D[2]
        xl += D[1] * D[2]
    return rows


def device_form(mask, form):
    """The mask as a numpy array of the form the case hands to the device ("view" is made non-contiguous on the device side)."""
    if form == "bool":
        return mask.copy()
    if form == "values":
        return np.where(mask, np.uint8(200), np.uint8(0)) | (mask & (np.indices(mask.shape).sum(0) % 2 == 0)).astype(np.uint8) * 7
    return mask.astype(np.uint8)
