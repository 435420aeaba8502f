"""Normalized surface Dice (NSD): the second metric of every evaluation script of the reference (evaluation/SurfaceDice.py and the
per-organ loops of evaluation/{abdomen,BTCV,ACDC,endoscopy}_NSD_Eval.py).

  * surface_area_table(spacing) -- the surfel area of every 2x2x2 neighbour code, built here by construction (see _code_triangles);
  * compute_surface_distances -- the reference's dict of sorted distances and surfel areas (SurfaceDice.py:280-425); torch tensors on
    the device run K24 (csrc/surface.hip) and stay there, numpy arrays and CPU tensors take scipy's correlate and
    distance_transform_edt here;
  * compute_surface_dice_at_tolerance / compute_surface_overlap_at_tolerance / compute_average_surface_distance /
    compute_robust_hausdorff -- the reference's metrics on that dict (:428-479);
  * case_nsd -- the scripts' per-organ loop on one case; on the device every organ runs in the same K24 launches, with one small
    read-back of statistics and one of the sums, and no sorted lists are built.
"""
import functools
import itertools
import math
from collections import OrderedDict

import numpy as np
import scipy.ndimage as ndi
import torch

from . import evaluation, ops

ABDOMEN_NSD_TOLERANCES = OrderedDict([("Liver", 5), ("RK", 3), ("Spleen", 3), ("Pancreas", 5), ("Aorta", 2), ("IVC", 2), ("RAG", 2),
                                      ("LAG", 2), ("Gallbladder", 2), ("Esophagus", 3), ("Stomach", 5), ("Duodenum", 7),
                                      ("LK", 3)])          # abdomen_NSD_Eval.py:49-51, labels 1..13; slabs: evaluation.SLAB_LABELS
BTCV_ORGANS = ("Spleen", "RK", "LK", "Gallbladder", "Esophagus", "Liver", "Stomach", "Aorta", "IVC", "PVSV", "Pancreas", "RAG", "LAG")
BTCV_NSD_TOLERANCES = OrderedDict(zip(BTCV_ORGANS, (3, 3, 3, 2, 3, 5, 5, 2, 2, 2, 5, 2, 2)))      # BTCV_NSD_Eval.py:52-54
BTCV_SLAB_LABELS = (5, 8, 9)                                                                      # Esophagus, Aorta, IVC
ACDC_NSD_TOLERANCES = OrderedDict([("RV", 3), ("MLV", 3), ("LVC", 3)])                           # ACDC_NSD_Eval.py:49

mean_nsd = evaluation.abdomen_mean_dsc          # column means over cases, then their mean (pandas skips NaN)

# ------------------------------------------------------------------------------------------------------------------------------------
# surfel areas
# ------------------------------------------------------------------------------------------------------------------------------------
_CORNERS = tuple(itertools.product((0, 1), repeat=3))


def _bit(c):
    """Bit of cube corner (i, j, k) in the neighbour code: the correlation kernel [[[128, 64], [32, 16]], [[8, 4], [2, 1]]]."""
    return 1 << (7 - (4 * c[0] + 2 * c[1] + c[2]))


def _adjacent(a, b):
    return sum(x != y for x, y in zip(a, b)) == 1


def _components(corners):
    """Corners connected along cube edges (corners on a face or body diagonal only are separate)."""
    rest, comps = set(corners), []
    while rest:
        stack = [rest.pop()]
        comp = set(stack)
        while stack:
            c = stack.pop()
            for d in [d for d in rest if _adjacent(c, d)]:
                rest.remove(d)
                comp.add(d)
                stack.append(d)
        comps.append(comp)
    return comps


def _polygon(comp):
    """The marching-cubes polygon around one component: the midpoints of the cube edges that leave it, in cyclic order (two of them
    are neighbours when they lie on one cube face)."""
    edges = [(a, b) for a in _CORNERS for b in _CORNERS if a < b and _adjacent(a, b) and ((a in comp) != (b in comp))]
    faces = [[c for c in _CORNERS if c[ax] == v] for ax in range(3) for v in (0, 1)]
    links = {e: [] for e in edges}
    for f in faces:
        on = [e for e in edges if e[0] in f and e[1] in f]
        if on:                                  # a component of <= 4 corners crosses a face at exactly 0 or 2 edges
            links[on[0]].append(on[1])
            links[on[1]].append(on[0])
    cycle, prev = [edges[0]], None
    while True:
        a, b = links[cycle[-1]]
        nxt = a if a != prev else b
        if nxt == cycle[0]:
            break
        prev = cycle[-1]
        cycle.append(nxt)
    return [tuple((np.array(a, np.float64) + np.array(b, np.float64)) / 2) for a, b in cycle]


def _triangulations(idx):
    """Every triangulation of the polygon over the vertex indices idx (in cyclic order)."""
    if len(idx) < 3:
        return [[]]
    out = []
    for m in range(1, len(idx) - 1):
        for left in _triangulations(idx[:m + 1]):
            for right in _triangulations(idx[m:]):
                out.append(left + right + [(idx[0], idx[m], idx[-1])])
    return out


def _area_vector(p0, p1, p2):
    return np.cross(np.subtract(p1, p0), np.subtract(p2, p0)) / 2


@functools.lru_cache(maxsize=None)
def _code_triangles():
    """(256,) list of (t, 3) float64 arrays: the area vector of every triangle of the surface through one 2x2x2 cell.

    The surface is the marching-cubes one with every vertex at an edge midpoint.  The set corners (the unset ones when more than
    four are set, so that a code and its complement get the same surface) split into edge-connected components, and each component
    is cut off by one polygon.  A planar polygon's triangulation does not matter; a non-planar one (the pentagon of three corners on
    a face, the hexagons of four) is triangulated with the largest total area: the folded triangulation, whose pieces follow the
    cell's faces rather than cutting across it."""
    out = []
    for code in range(256):
        corners = [c for c in _CORNERS if code & _bit(c)]
        if len(corners) > 4:
            corners = [c for c in _CORNERS if not code & _bit(c)]
        tris = []
        for comp in _components(corners):
            P = _polygon(comp)
            best, best_area = None, -1.0
            for T in _triangulations(list(range(len(P)))):
                vecs = [_area_vector(P[a], P[b], P[c]) for a, b, c in T]
                area = sum(float(np.linalg.norm(v)) for v in vecs)
                if area > best_area + 1e-12:
                    best, best_area = vecs, area
            tris += best
        out.append(np.array(tris, np.float64).reshape(-1, 3))
    return out


def surface_area_table(spacing_mm):
    """(256,) float64: the area in mm^2 of the surface through a 2x2x2 cell of every neighbour code at this spacing.  Each triangle's
    area vector n is scaled to (n0 s1 s2, n1 s0 s2, n2 s0 s1) and the norms are summed."""
    s = [float(v) for v in spacing_mm]
    scale = np.array([s[1] * s[2], s[0] * s[2], s[0] * s[1]], np.float64)
    table = np.zeros(256, np.float64)
    for code, tris in enumerate(_code_triangles()):
        for n in tris:
            table[code] += float(np.linalg.norm(n * scale))
    return table


# ------------------------------------------------------------------------------------------------------------------------------------
# compute_surface_distances
# ------------------------------------------------------------------------------------------------------------------------------------
_KERNEL = np.array([[[128, 64], [32, 16]], [[8, 4], [2, 1]]])


def _empty_dict(like=None):
    if isinstance(like, torch.Tensor):
        e = torch.zeros(0, dtype=torch.float64, device=like.device)
        return {"distances_gt_to_pred": e, "distances_pred_to_gt": e.clone(), "surfel_areas_gt": e.clone(),
                "surfel_areas_pred": e.clone()}
    return {"distances_gt_to_pred": np.array([]), "distances_pred_to_gt": np.array([]), "surfel_areas_gt": np.array([]),
            "surfel_areas_pred": np.array([])}


def _sorted_pairs(d, a):
    order = np.lexsort((a, d))
    return d[order], a[order]


def _host_surface_distances(mask_gt, mask_pred, spacing_mm):
    mask_gt, mask_pred = np.asarray(mask_gt, bool), np.asarray(mask_pred, bool)
    sampling = [float(v) for v in spacing_mm]
    both = mask_gt | mask_pred
    if not both.any():
        return _empty_dict()
    box = []
    for ax in range(3):                                 # the union's bounding box, as the reference's max projections give it
        idx = np.nonzero(both.any(axis=tuple(a for a in range(3) if a != ax)))[0]
        box.append(slice(int(idx[0]), int(idx[-1]) + 1))
    box = tuple(box)
    shape = tuple(b.stop - b.start + 1 for b in box)
    out = {}
    borders, codes = [], []
    for m in (mask_gt, mask_pred):
        crop = np.zeros(shape, np.uint8)
        crop[:-1, :-1, :-1] = m[box]
        code = ndi.correlate(crop, _KERNEL, mode="constant", cval=0)      # uint8 output, like the reference's
        codes.append(code)
        borders.append((code != 0) & (code != 255))
    dist = [ndi.distance_transform_edt(~b, sampling=sampling) if b.any() else np.full(b.shape, np.inf) for b in borders]
    table = surface_area_table(spacing_mm)
    d_gt, d_pred = dist[1][borders[0]], dist[0][borders[1]]
    a_gt, a_pred = table[codes[0][borders[0]]], table[codes[1][borders[1]]]
    out["distances_gt_to_pred"], out["surfel_areas_gt"] = _sorted_pairs(d_gt, a_gt)
    out["distances_pred_to_gt"], out["surfel_areas_pred"] = _sorted_pairs(d_pred, a_pred)
    return {k: out[k] for k in ("distances_gt_to_pred", "distances_pred_to_gt", "surfel_areas_gt", "surfel_areas_pred")}


def compute_surface_distances(mask_gt, mask_pred, spacing_mm):
    """SurfaceDice.py:280-425: {"distances_gt_to_pred", "distances_pred_to_gt", "surfel_areas_gt", "surfel_areas_pred"}, each list
    sorted by (distance, area); distances are +inf where the other mask is empty, and all four are empty when both are.  Torch tensors
    on the device run K24 and return float64 device tensors; anything else returns numpy arrays from the host path."""
    if isinstance(mask_gt, torch.Tensor) and mask_gt.is_cuda:
        return _device_surface_distances(mask_gt, mask_pred, spacing_mm)
    if isinstance(mask_gt, torch.Tensor):
        mask_gt = mask_gt.numpy()
    if isinstance(mask_pred, torch.Tensor):
        mask_pred = mask_pred.cpu().numpy()
    return _host_surface_distances(mask_gt, mask_pred, spacing_mm)


# ------------------------------------------------------------------------------------------------------------------------------------
# metrics on the dict (SurfaceDice.py:428-479); torch tensors are reduced where they live
# ------------------------------------------------------------------------------------------------------------------------------------
def _unpack(sd):
    return sd["distances_gt_to_pred"], sd["distances_pred_to_gt"], sd["surfel_areas_gt"], sd["surfel_areas_pred"]


def _total(x):
    return float(x.sum()) if isinstance(x, torch.Tensor) else float(np.sum(x))


def _ratio(num, den):
    """num / den with numpy's float64 semantics: 0 / 0 is nan, x / 0 is +-inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(num) / np.float64(den))


def compute_average_surface_distance(surface_distances):
    d_gt, d_pred, a_gt, a_pred = _unpack(surface_distances)
    return (_ratio(_total(d_gt * a_gt), _total(a_gt)), _ratio(_total(d_pred * a_pred), _total(a_pred)))


def _percentile_distance(d, a, percent):
    if len(d) == 0:
        return math.inf
    if isinstance(d, torch.Tensor):
        cum = torch.cumsum(a, 0) / a.sum()
        idx = int(torch.searchsorted(cum, torch.tensor([percent / 100.0], dtype=cum.dtype, device=cum.device))[0])
    else:
        cum = np.cumsum(a) / np.sum(a)
        idx = int(np.searchsorted(cum, percent / 100.0))
    return float(d[min(idx, len(d) - 1)])


def compute_robust_hausdorff(surface_distances, percent):
    d_gt, d_pred, a_gt, a_pred = _unpack(surface_distances)
    return max(_percentile_distance(d_gt, a_gt, percent), _percentile_distance(d_pred, a_pred, percent))


def compute_surface_overlap_at_tolerance(surface_distances, tolerance_mm):
    d_gt, d_pred, a_gt, a_pred = _unpack(surface_distances)
    return (_ratio(_total(a_gt[d_gt <= tolerance_mm]), _total(a_gt)), _ratio(_total(a_pred[d_pred <= tolerance_mm]), _total(a_pred)))


def compute_surface_dice_at_tolerance(surface_distances, tolerance_mm):
    d_gt, d_pred, a_gt, a_pred = _unpack(surface_distances)
    overlap = _total(a_gt[d_gt <= tolerance_mm]) + _total(a_pred[d_pred <= tolerance_mm])
    return _ratio(overlap, _total(a_gt) + _total(a_pred))


# ------------------------------------------------------------------------------------------------------------------------------------
# per-case loop of the scripts
# ------------------------------------------------------------------------------------------------------------------------------------
_EMPTY_SLAB = ("label {}: a slab organ whose gt lies on one z slice has an empty [z_lower, z_upper); the reference's scripts fail on "
               "it (a reduction over an empty array)")


def _host_case_nsd(gt, seg, spacing, tolerances, slab_labels):
    gt, seg = np.asarray(gt), np.asarray(seg)
    out = OrderedDict()
    for i, (organ, tol) in enumerate(tolerances.items(), 1):
        g, s = gt == i, seg == i
        if not g.any() and not s.any():
            nsd = 1
        elif not g.any():
            nsd = 0
        else:
            if i in slab_labels:
                z = np.nonzero(g.any(axis=(0, 1)))[0]
                lo, hi = int(z.min()), int(z.max())
                if lo == hi:
                    raise ValueError(_EMPTY_SLAB.format(i))
                g, s = g[:, :, lo:hi], s[:, :, lo:hi]          # the scripts' half-open range
            nsd = compute_surface_dice_at_tolerance(_host_surface_distances(g, s, spacing), tol)
        out[organ] = round(nsd, 4)
    return out


def case_nsd(gt, seg, spacing, tolerances, slab_labels=()):
    """Per-organ NSD of one case as the *_NSD_Eval.py scripts compute it (:90-110), rounded to 4 digits: organ k of `tolerances`
    (organ -> tolerance in mm) is label k; 1 when both masks are empty, 0 when only the gt is, organs in `slab_labels` cut to the
    gt's half-open z range [z_lower, z_upper) (ValueError when that range is empty: the scripts fail there).  gt / seg: (X, Y, Z) label volumes
    indexed [x, y, z]; uint8 torch tensors on the device run K24, anything else the host path."""
    tolerances = OrderedDict(tolerances)
    if len(tolerances) > 255:
        raise ValueError("at most 255 labels")
    if isinstance(gt, torch.Tensor) and gt.is_cuda:
        return _device_case_nsd(gt, seg, spacing, tolerances, tuple(slab_labels))
    if isinstance(gt, torch.Tensor):
        gt = gt.numpy()
    if isinstance(seg, torch.Tensor):
        seg = seg.cpu().numpy()
    return _host_case_nsd(gt, seg, spacing, tolerances, tuple(slab_labels))


# ------------------------------------------------------------------------------------------------------------------------------------
# device path (K24)
# ------------------------------------------------------------------------------------------------------------------------------------
def _check_spacing(spacing):
    s = [float(v) for v in spacing]
    if len(s) != 3 or not all(math.isfinite(v) and v > 0 for v in s):
        raise ValueError(f"spacing {tuple(spacing)}: three positive finite values expected")
    return s


def _as_labels(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 3):
        raise RuntimeError(f"{name}: expected a 3-D tensor on the MI355X device")
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise RuntimeError(f"{name}: expected a uint8 label volume or a bool mask, got {t.dtype}")
    return t.contiguous()


def _device_layout(stats, labels, slabs, measure_empty_gt=False):
    """Crops of the measured labels from the statistics (host ints).  Returns (desc rows, per-label outcome: None = measured, else
    the fixed value)."""
    rows, fixed = [], []
    vox = zl = yl = xl = 0
    for lab, slab in zip(labels, slabs):
        s = stats[lab]
        if s[0] == 0 and s[1] == 0:
            fixed.append(1)
            continue
        if s[0] == 0 and not measure_empty_gt:
            fixed.append(0)
            continue
        lo, hi = [s[2], s[4], s[6]], [s[3], s[5], s[7]]
        if slab:
            if s[8] == s[9]:
                raise ValueError(_EMPTY_SLAB.format(lab))
            lo[2], hi[2] = max(lo[2], s[8]), min(hi[2], s[9] - 1)
        fixed.append(None)
        n = [h - l + 1 for l, h in zip(lo, hi)]
        D = [v + 1 for v in n]
        rows.append([lab, *lo, *n, vox, zl, yl, xl, 0, 0, 0, 0, 0])
        vox += D[0] * D[1] * D[2]
        zl += D[0] * D[1]
        yl += D[0] * D[2]
        xl += D[1] * D[2]
    return rows, fixed


def _device_run(gt, seg, spacing, labels, tols, slabs, pairs=False):
    s = _check_spacing(spacing)
    wanted = torch.zeros(256, dtype=torch.uint8)
    wanted[list(labels)] = 1
    stats = ops.surface_stats(gt, seg, wanted.to(gt.device)).cpu().tolist()       # read-back 1
    rows, fixed = _device_layout(stats, labels, slabs, measure_empty_gt=pairs)
    if not rows:
        return fixed, None, None, None
    desc = torch.tensor(rows, dtype=torch.int64)
    state = ops.surface_prepare(gt, seg, desc, s)
    measured = [t for t, f in zip(tols, fixed) if f is None]
    tol = torch.tensor(measured, dtype=torch.float64).to(gt.device)
    area = torch.from_numpy(surface_area_table(s)).to(gt.device)
    pairs_out = counts = None
    if pairs:
        counts = state[2].cpu()                                              # the dict's sizes: one more read-back
        ng, npred = int(counts[:, 0].sum()), int(counts[:, 1].sum())
        off = torch.cumsum(counts.reshape(-1).long(), 0) - counts.reshape(-1).long()
        state[3][:, 11] = off[0::2].to(gt.device)
        state[3][:, 12] = off[1::2].to(gt.device)
        sums, pairs_out = ops.surface_reduce(state, tol, area, s, pairs_total=ng + npred)
    else:
        sums, _ = ops.surface_reduce(state, tol, area, s)
    return fixed, sums, pairs_out, counts


def _device_surface_distances(mask_gt, mask_pred, spacing_mm):
    gt, pred = _as_labels(mask_gt, "mask_gt"), _as_labels(mask_pred, "mask_pred")
    if gt.shape != pred.shape:
        raise RuntimeError(f"mask_gt {tuple(gt.shape)} and mask_pred {tuple(pred.shape)} differ in shape")
    gt, pred = (gt != 0).view(torch.uint8), (pred != 0).view(torch.uint8)
    fixed, sums, pairs, counts = _device_run(gt, pred, spacing_mm, [1], [0.0], [False], pairs=True)
    if sums is None:
        return _empty_dict(gt)
    ng = int(counts[0, 0])
    d_gt, a_gt = _device_sort(pairs[:ng, 0], pairs[:ng, 1])
    d_pred, a_pred = _device_sort(pairs[ng:, 0], pairs[ng:, 1])
    return {"distances_gt_to_pred": d_gt, "distances_pred_to_gt": d_pred, "surfel_areas_gt": a_gt, "surfel_areas_pred": a_pred}


def _device_sort(d, a):
    """Sort (distance, area) pairs lexicographically, as sorted(zip(...)) does."""
    i = torch.sort(a, stable=True).indices
    d, a = d[i], a[i]
    j = torch.sort(d, stable=True).indices
    return d[j].contiguous(), a[j].contiguous()


def _device_case_nsd(gt, seg, spacing, tolerances, slab_labels):
    gt, seg = _as_labels(gt, "gt"), _as_labels(seg, "seg")
    if gt.shape != seg.shape:
        raise RuntimeError(f"gt {tuple(gt.shape)} and seg {tuple(seg.shape)} differ in shape")
    labels = list(range(1, len(tolerances) + 1))
    slabs = [lab in slab_labels for lab in labels]
    fixed, sums, _, _ = _device_run(gt, seg, spacing, labels, [float(t) for t in tolerances.values()], slabs)
    sums = sums.cpu().numpy() if sums is not None else None                 # read-back 2
    out, k = OrderedDict(), 0
    for organ, f in zip(tolerances, fixed):
        if f is None:
            a_gt, w_gt, a_pred, w_pred = sums[k]
            k += 1
            f = _ratio(w_gt + w_pred, a_gt + a_pred)
        out[organ] = round(f, 4)
    return out

