"""Cell-instance F1 score: the microscopy metric of the reference (evaluation/compute_cell_metric.py, adapted there from
stardist's matching.py), on in-memory images.

    label_instances            skimage.measure.label(seg == 1): 8-connected components numbered in raster order of their first pixel
    relabel_sequential         segmentation.relabel_sequential: order-preserving compaction of the positive labels to 1..n
    remove_boundary_cells      drop every label seen in the 2-pixel ring, then relabel_sequential (:124-133)
    intersection_over_union    _intersection_over_union (:21-37), background row and column included
    eval_tp_fp_fn              (:107-122) true / false positives and false negatives at one IoU threshold
    case_cell_metrics          the script's loop body (:170-244) on one image: its CSV columns, one dict per threshold
    summarize_f1               the mean and median F1 it prints

A CUDA tensor runs K27 (csrc/cells.hip through ops.cells_*); CPU tensors and numpy arrays run the reference's numpy / scipy
arithmetic here, which is also the oracle of the GPU tests.  Every count is an integer and every score one float64 division of
integers, so both paths give the same values bit for bit.

The assignment: the reference runs linear_sum_assignment on -(iou >= th) - iou / (2 n_min).  The second term sums to at most 0.5
over an assignment, so the number of assigned pairs with iou >= th is the size of a maximum bipartite matching of the edges
{iou >= th}.  The device path reads back, per threshold, the edge count and the largest row and column degree: when no row and no
column holds more than one edge the edge count is tp; otherwise the edge list is read back and
scipy.sparse.csgraph.maximum_bipartite_matching gives tp.  The host path runs the literal dense assignment.

Where this differs from running the script: maps are int32 throughout.  The script's tiled branch copies the labelled prediction
into an array of the gt's dtype and sums the cell counts in it, which wraps for a narrow gt dtype; nothing wraps here.
"""
import numpy as np
import scipy.ndimage as ndi
import torch
from scipy.optimize import linear_sum_assignment
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching

from . import ops

COLUMNS = ("true_num", "pred_num", "correct_num(TP)", "missed_num(FN)", "wrong_num(FP)", "precision", "recall", "dice", "F1")
LARGE_IMAGE_PIXELS = 25_000_000          # compute_cell_metric.py:176
ROI_SIZE = 2000                          # :187

# which way the device path found tp, for tests and tools: calls answered by the edge count alone / by the matching
PATH_COUNTS = {"edge_count": 0, "matching": 0}


def _is_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _host(x):
    """numpy view of a CPU tensor or array-like"""
    return x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _like(result, x):
    """host results come back as what went in: a CPU tensor for a CPU tensor, numpy otherwise"""
    return torch.from_numpy(result) if isinstance(x, torch.Tensor) else result


def _image(x, name):
    if x.ndim != 2:
        raise RuntimeError(f"{name}: a 2-D image expected, got shape {tuple(x.shape)}")
    return x


# ------------------------------------------------------------------------------------------------------------------------------------
# host path: the reference's arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------
def _label_host(seg, foreground):
    lab, n = ndi.label(seg == foreground, structure=np.ones((3, 3), dtype=bool))
    return lab.astype(np.int32), int(n)


def _relabel_host(mask):
    """skimage's relabel_sequential(offset=1) for its forward map: the positive labels in increasing order become 1..n"""
    mask = np.asarray(mask)
    if mask.size and mask.min() < 0:
        raise RuntimeError("relabel_sequential: negative labels are not supported")          # skimage raises ValueError here
    labels = np.unique(mask)
    labels = labels[labels > 0]
    out = np.searchsorted(labels, mask) + 1
    out[mask <= 0] = 0
    return out.astype(np.int32)


def _remove_boundary_host(mask):
    """remove_boundary_cells (:124-133) on a copy, line by line"""
    mask = np.array(mask, copy=True)
    W, H = mask.shape
    bd = np.ones((W, H))
    bd[2:W - 2, 2:H - 2] = 0
    bd_cells = np.unique(mask * bd)
    mask[np.isin(mask, bd_cells[1:])] = 0             # for i in bd_cells[1:]: mask[mask == i] = 0
    return _relabel_host(mask)


def _overlap_host(x, y):
    """_label_overlap (:40-70): the (x.max() + 1, y.max() + 1) matrix of pixel counts"""
    x, y = np.asarray(x).ravel().astype(np.int64), np.asarray(y).ravel().astype(np.int64)
    if x.size and (x.min() < 0 or y.min() < 0):
        raise RuntimeError("label overlap: negative labels are not supported")
    nx, ny = 1 + int(x.max()), 1 + int(y.max())
    if 8 * nx * ny > 2 * ops.CELLS_MAX_OVERLAP_BYTES:
        raise RuntimeError(f"label overlap: a {nx} x {ny} matrix of 8-byte counts, at most {2 * ops.CELLS_MAX_OVERLAP_BYTES} bytes")
    return np.bincount(x * ny + y, minlength=nx * ny).reshape(nx, ny).astype(np.uint64)


def _iou_host(masks_true, masks_pred):
    overlap = _overlap_host(masks_true, masks_pred)
    n_pixels_pred = np.sum(overlap, axis=0, keepdims=True)
    n_pixels_true = np.sum(overlap, axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = overlap / (n_pixels_pred + n_pixels_true - overlap)
    iou[np.isnan(iou)] = 0.0
    return iou


def _true_positive_host(iou, th):
    """_true_positive (:83-105)"""
    n_min = min(iou.shape[0], iou.shape[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        costs = -(iou >= th).astype(float) - iou / (2 * n_min)
    true_ind, pred_ind = linear_sum_assignment(costs)
    return int((iou[true_ind, pred_ind] >= th).sum())


def matching_true_positive(iou, th):
    """The size of a maximum bipartite matching of {iou >= th}: equal to _true_positive's count (module docstring)."""
    i, j = np.nonzero(np.asarray(iou) >= th)
    return _matching(np.stack([i, j], 1), iou.shape[0], iou.shape[1])


def edge_stats(iou, th):
    """(edge count, largest row degree, largest column degree) of {iou >= th}: what the device path decides on (both degrees at
    most 1: the edge count is tp; otherwise the matching runs).  iou without the background row and column."""
    e = np.asarray(iou) >= th
    if e.size == 0:
        return 0, 0, 0
    return int(e.sum()), int(e.sum(1).max()), int(e.sum(0).max())


def _matching(edges, n_true, n_pred):
    if len(edges) == 0:
        return 0
    order = np.lexsort((edges[:, 1], edges[:, 0]))                   # the device's list comes in the schedule's order
    edges = edges[order]
    graph = csr_matrix((np.ones(len(edges), dtype=np.int8), (edges[:, 0], edges[:, 1])), shape=(n_true, n_pred))
    return int((maximum_bipartite_matching(graph, perm_type="column") >= 0).sum())


def _eval_host(masks_true, masks_pred, threshold):
    num_inst_gt, num_inst_seg = int(np.max(masks_true)), int(np.max(masks_pred))
    if num_inst_seg > 0:
        tp = _true_positive_host(_iou_host(masks_true, masks_pred)[1:, 1:], threshold)
        return tp, num_inst_seg - tp, num_inst_gt - tp
    return 0, 0, 0


def _dice(n_gt, n_seg, n_both):
    """dice (:72-81) from the three counts"""
    if n_gt == 0 and n_seg == 0:
        return 1.0
    if n_gt == 0:
        return 0.0
    return 2 * n_both / (n_gt + n_seg)


def _tiles(H, W, roi_size):
    """origins of the roi_size tiles of the image zero-padded to multiples of roi_size, in the script's order (:189-214)"""
    n_H, n_W = -(-H // roi_size), -(-W // roi_size)
    return [(roi_size * i, roi_size * j) for i in range(n_H) for j in range(n_W)]


def _counts_host(gt, seg, thresholds, count_bd_cells, roi_size, large_image_pixels):
    """(true_num, pred_num, [(tp, fp, fn) per threshold], dice) of one image with numpy / scipy"""
    seg, _ = _label_host(seg, 1)
    dice = _dice(int(np.count_nonzero(gt > 0)), int(np.count_nonzero(seg > 0)), int(np.count_nonzero((gt > 0) & (seg > 0))))
    if int(np.prod(gt.shape)) < large_image_pixels:
        if not count_bd_cells:
            gt, seg = _remove_boundary_host(gt.astype(np.int32)), _remove_boundary_host(seg)
        gt, seg = _relabel_host(gt), _relabel_host(seg)
        return int(np.max(gt)), int(np.max(seg)), [_eval_host(gt, seg, th) for th in thresholds], dice
    _refuse_tiled_bd(count_bd_cells)
    H, W = gt.shape
    new_H, new_W = -(-H // roi_size) * roi_size, -(-W // roi_size) * roi_size
    gt_pad, seg_pad = np.zeros((new_H, new_W), dtype=np.int32), np.zeros((new_H, new_W), dtype=np.int32)
    gt_pad[:H, :W] = gt
    seg_pad[:H, :W] = seg
    true_num = pred_num = 0
    counts = [[0, 0, 0] for _ in thresholds]
    for r0, c0 in _tiles(H, W, roi_size):
        gt_roi = _relabel_host(_remove_boundary_host(gt_pad[r0:r0 + roi_size, c0:c0 + roi_size]))
        seg_roi = _relabel_host(_remove_boundary_host(seg_pad[r0:r0 + roi_size, c0:c0 + roi_size]))
        true_num += int(np.max(gt_roi))
        pred_num += int(np.max(seg_roi))
        for k, th in enumerate(thresholds):
            for m, v in enumerate(_eval_host(gt_roi, seg_roi, th)):
                counts[k][m] += v
    return true_num, pred_num, [tuple(c) for c in counts], dice


def _refuse_tiled_bd(count_bd_cells):
    if count_bd_cells:
        raise RuntimeError("count_bd_cells is not supported on images of large_image_pixels or more: the reference's tiled branch "
                           "raises a NameError there (gt_roi is only assigned when boundary cells are removed) and records the case "
                           "as failed")


# ------------------------------------------------------------------------------------------------------------------------------------
# device path: K27
# ------------------------------------------------------------------------------------------------------------------------------------
def _int_map(x, name):
    """a label image on the device as contiguous int32"""
    _image(x, name)
    if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
        raise RuntimeError(f"{name}: an integer label image expected, got {x.dtype}")
    if x.numel() > ops.CELLS_MAX_PIXELS or x.numel() < 1:
        raise RuntimeError(f"{name}: {x.numel()} pixels, 1 to {ops.CELLS_MAX_PIXELS} are supported")
    return x.to(torch.int32).contiguous()


def _label_range(x, name):
    """(min, max) of a device label map: one read-back; negative labels and labels of 2^31 or more are refused"""
    lo, hi = (int(v) for v in torch.aminmax(x))
    if lo < 0 or hi >= 2 ** 31:
        raise RuntimeError(f"{name}: labels in [{lo}, {hi}]; K27 supports 0 to 2^31 - 1")
    return lo, hi


def _gt_map(gt):
    """(int32 map, label domain = max + 1) of a device gt"""
    _image(gt, "gt")
    if gt.dtype.is_floating_point or gt.dtype.is_complex or gt.dtype == torch.bool:
        raise RuntimeError(f"gt: an integer label image expected, got {gt.dtype}")
    _, hi = _label_range(gt, "gt")
    if hi + 1 > ops.CELLS_MAX_FLAG_BYTES:
        raise RuntimeError(f"gt: labels up to {hi} need {hi + 1} bytes of presence flags, at most {ops.CELLS_MAX_FLAG_BYTES} are "
                           "supported; relabel the map first")
    return _int_map(gt, "gt"), hi + 1


def _seg_map(seg):
    """the class-label image as K27 reads it: uint8 as it is (predict.predict_case's output type), any other integer type as int32"""
    _image(seg, "seg")
    if seg.dtype == torch.uint8:
        if seg.numel() > ops.CELLS_MAX_PIXELS or seg.numel() < 1:
            raise RuntimeError(f"seg: {seg.numel()} pixels, 1 to {ops.CELLS_MAX_PIXELS} are supported")
        return seg.contiguous()
    return _int_map(seg, "seg")


def _tp_device(g, p, n_true, n_pred, thresholds, want_iou=False):
    """[tp per threshold] (and the IoU matrix) of two device maps with labels in [0, n_true] / [0, n_pred]"""
    overlap, area_t, area_p = ops.cells_overlap(g, p, n_true, n_pred)
    tps, iou = [], None
    for k in range(0, max(len(thresholds), 1), ops.CELLS_MAX_THRESHOLDS):
        chunk = list(thresholds[k:k + ops.CELLS_MAX_THRESHOLDS])
        stats, got = ops.cells_match(overlap, area_t, area_p, chunk, want_iou=want_iou and k == 0)
        iou = got if k == 0 else iou
        for th, (count, row_deg, col_deg) in zip(chunk, stats.cpu().tolist()):
            if row_deg <= 1 and col_deg <= 1:
                PATH_COUNTS["edge_count"] += 1
                tps.append(count)
            else:
                PATH_COUNTS["matching"] += 1
                edges = ops.cells_edges(overlap, area_t, area_p, th, count).cpu().numpy().astype(np.int64)
                tps.append(_matching(edges, n_true, n_pred))
    return tps, iou


def _eval_device(g, p, n_true, n_pred, thresholds):
    """[(tp, fp, fn) per threshold] as eval_tp_fp_fn counts them"""
    if n_pred <= 0:
        return [(0, 0, 0) for _ in thresholds]
    if n_true <= 0:
        return [(0, n_pred, n_true) for _ in thresholds]
    return [(tp, n_pred - tp, n_true - tp) for tp in _tp_device(g, p, n_true, n_pred, thresholds)[0]]


def _counts_device(gt, seg, thresholds, count_bd_cells, roi_size, large_image_pixels):
    gt, domain = _gt_map(gt)                                                   # read-back: the largest gt label
    seg = _seg_map(seg)
    if seg.shape != gt.shape or seg.device != gt.device:
        raise RuntimeError(f"gt {tuple(gt.shape)} on {gt.device} and seg {tuple(seg.shape)} on {seg.device} differ")
    H, W = (int(v) for v in gt.shape)
    small = H * W < large_image_pixels
    if not small:
        _refuse_tiled_bd(count_bd_cells)
    parent, dice_counts = ops.cells_label(seg, 1, gt)
    ring = not count_bd_cells
    if small:
        seg_map, n_pred = ops.cells_relabel(parent, H * W + 1, bias=1, ring=ring)
        gt_map, n_true = ops.cells_relabel(gt, domain, ring=ring)
        n_true, n_pred, n_gt, n_seg, n_both = torch.cat([n_true, n_pred, dice_counts]).cpu().tolist()      # read-back: five scalars
        return n_true, n_pred, _eval_device(gt_map, seg_map, n_true, n_pred, thresholds), _dice(n_gt, n_seg, n_both)
    inst, n_inst = ops.cells_relabel(parent, H * W + 1, bias=1)                # the whole image is labelled once, as in the reference
    n_inst, n_gt, n_seg, n_both = torch.cat([n_inst, dice_counts]).cpu().tolist()
    true_num = pred_num = 0
    counts = [[0, 0, 0] for _ in thresholds]
    for r0, c0 in _tiles(H, W, roi_size):
        region = (r0, c0, roi_size, roi_size)
        gt_roi, n_true = ops.cells_relabel(gt, domain, region=region, ring=True)
        seg_roi, n_pred = ops.cells_relabel(inst, n_inst + 1, region=region, ring=True)
        n_true, n_pred = torch.cat([n_true, n_pred]).cpu().tolist()
        true_num += n_true
        pred_num += n_pred
        for k, triple in enumerate(_eval_device(gt_roi, seg_roi, n_true, n_pred, thresholds)):
            for m, v in enumerate(triple):
                counts[k][m] += v
    return true_num, pred_num, [tuple(c) for c in counts], _dice(n_gt, n_seg, n_both)


# ------------------------------------------------------------------------------------------------------------------------------------
# public interface
# ------------------------------------------------------------------------------------------------------------------------------------
def label_instances(seg, foreground=1):
    """skimage.measure.label(seg == foreground) of a 2-D class-label image: (instances (H, W) int32, n).  Full (8-neighbour)
    connectivity; components are numbered in raster order of their first pixel."""
    if _is_device(seg):
        seg = _seg_map(seg)
        parent, _ = ops.cells_label(seg, foreground)
        out, n = ops.cells_relabel(parent, seg.numel() + 1, bias=1)
        return out, int(n)
    lab, n = _label_host(_image(_host(seg), "seg"), foreground)
    return _like(lab, seg), n


def relabel_sequential(mask):
    """segmentation.relabel_sequential's relabelled map: a new int32 map with the positive labels renumbered 1..n in order."""
    if _is_device(mask):
        m, domain = _gt_map(mask)
        return ops.cells_relabel(m, domain)[0]
    return _like(_relabel_host(_image(_host(mask), "mask")), mask)


def remove_boundary_cells(mask):
    """The reference's remove_boundary_cells (:124-133) on a new int32 map: every label present in the 2-pixel ring is zeroed
    everywhere and the rest renumbered 1..n in order.  The reference's np.unique(mask * bd)[1:] drops the smallest value, which is 0
    whenever the image has an interior; the device path needs H, W >= 5 for that reason, the host path follows the line literally."""
    if _is_device(mask):
        m, domain = _gt_map(mask)
        return ops.cells_relabel(m, domain, ring=True)[0]
    return _like(_remove_boundary_host(_image(_host(mask), "mask")), mask)


def intersection_over_union(masks_true, masks_pred):
    """_intersection_over_union: float64 (masks_true.max() + 1, masks_pred.max() + 1), IoU of every label pair, 0 where 0 / 0."""
    if _is_device(masks_true):
        g, p = _int_map(masks_true, "masks_true"), _int_map(masks_pred, "masks_pred")
        if g.shape != p.shape:
            raise RuntimeError(f"masks_true {tuple(g.shape)} and masks_pred {tuple(p.shape)} differ in shape")
        (_, n_true), (_, n_pred) = _label_range(g, "masks_true"), _label_range(p, "masks_pred")
        overlap, area_t, area_p = ops.cells_overlap(g, p, n_true, n_pred)
        return ops.cells_match(overlap, area_t, area_p, (), want_iou=True)[1]
    return _like(_iou_host(_host(masks_true), _host(masks_pred)), masks_true)


def eval_tp_fp_fn(masks_true, masks_pred, threshold=0.5):
    """The reference's eval_tp_fp_fn: (tp, fp, fn) as Python ints; all 0 when masks_pred has no cell."""
    if _is_device(masks_true):
        g, p = _int_map(masks_true, "masks_true"), _int_map(masks_pred, "masks_pred")
        if g.shape != p.shape:
            raise RuntimeError(f"masks_true {tuple(g.shape)} and masks_pred {tuple(p.shape)} differ in shape")
        (_, n_true), (_, n_pred) = _label_range(g, "masks_true"), _label_range(p, "masks_pred")
        return _eval_device(g, p, n_true, n_pred, [threshold])[0]
    return _eval_host(_host(masks_true), _host(masks_pred), threshold)


def case_cell_metrics(gt, seg, thresholds=(0.5,), count_bd_cells=False, roi_size=ROI_SIZE, large_image_pixels=LARGE_IMAGE_PIXELS):
    """The script's loop body on one image.  gt: integer instance map (H, W); seg: class-label image (H, W), cells = class 1.
    Returns one dict per threshold with the script's columns (COLUMNS; precision, recall, dice and F1 rounded to 4 places with
    np.round) and the unrounded values under precision_raw, recall_raw, dice_raw, F1_raw, plus threshold.  Images of
    large_image_pixels pixels or more are scored tile by tile (roi_size), where count_bd_cells raises RuntimeError."""
    thresholds = [float(t) for t in thresholds]
    roi_size = int(roi_size)
    if roi_size < 5:
        raise RuntimeError(f"roi_size {roi_size}: at least 5 (a tile needs an interior inside its 2-pixel ring)")
    if _is_device(gt) != _is_device(seg):
        raise RuntimeError("gt and seg must both be on the device or both on the host")
    if _is_device(gt):
        true_num, pred_num, counts, dice = _counts_device(gt, seg, thresholds, count_bd_cells, roi_size, large_image_pixels)
    else:
        g, s = _image(_host(gt), "gt"), _image(_host(seg), "seg")
        if g.shape != s.shape:
            raise RuntimeError(f"gt {g.shape} and seg {s.shape} differ in shape")
        true_num, pred_num, counts, dice = _counts_host(g, s, thresholds, count_bd_cells, roi_size, large_image_pixels)
    rows = []
    for th, (tp, fp, fn) in zip(thresholds, counts):
        if tp == 0:
            precision = recall = f1 = 0
        else:
            precision = tp / pred_num
            recall = tp / true_num
            f1 = 2 * (precision * recall) / (precision + recall)
        rows.append({"true_num": true_num, "pred_num": pred_num, "correct_num(TP)": tp, "missed_num(FN)": fn, "wrong_num(FP)": fp,
                     "precision": float(np.round(precision, 4)), "recall": float(np.round(recall, 4)),
                     "dice": float(np.round(dice, 4)), "F1": float(np.round(f1, 4)),
                     "precision_raw": float(precision), "recall_raw": float(recall), "dice_raw": float(dice), "F1_raw": float(f1),
                     "threshold": th})
    return rows


def summarize_f1(per_case):
    """(mean, median) of the F1 column over cases, as the script prints them; per_case: dicts of case_cell_metrics or F1 values."""
    f1 = [c["F1"] if isinstance(c, dict) else c for c in per_case]
    return float(np.mean(f1)), float(np.median(f1))
