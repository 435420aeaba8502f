"""Generate tests/golden/cells.npz from the REFERENCE's own cell metric script.

    MLAGG_REFERENCE=<reference checkout> python tests/golden/make_golden_cells.py [--no-big]

evaluation/compute_cell_metric.py is a script: it is run with runpy under a temporary sys.argv on temporary folders that hold the
images of tests/_cell_cases.py, once for CASES at every threshold, once with --count_bd_cells, and once for the image above the
25 M-pixel switch at threshold 0.5.  The CSV rows it writes are recorded.  From the globals the run returns, its own functions
(remove_boundary_cells, _intersection_over_union, eval_tp_fp_fn) give the relabelled maps, IoU matrices and counts of the small
cases and of the instance-map PAIRS.  The tiled branch's constants are fixed in the script, so for the small TILED cases the
recorded value is the script's loop (:186-225) composed here from its own per-tile functions at roi_size = TILED_ROI.
Modules that are absent offline are replaced:
  - numba.jit is an identity decorator, so _label_overlap's own pixel loop runs in plain Python (minutes for the large image);
  - skimage.measure.label and skimage.segmentation.relabel_sequential are RESTATED, not run: scipy.ndimage.label with the full 3 x 3
    structure (components numbered in raster order of their first pixel, as skimage numbers them), and np.unique / np.searchsorted
    over the positive labels;
  - skimage.io.imread and tifffile.imread read .npy data behind the file names the script expects;
  - tqdm is the identity.
Only the data is committed."""
import csv
import json
import os
import runpy
import shutil
import sys
import tempfile
import types

import numpy as np
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if "MLAGG_REFERENCE" not in os.environ:
    raise SystemExit("set MLAGG_REFERENCE to a checkout of the reference repository (aticejiang/MLAgg-UNet)")
SCRIPT = os.path.join(os.environ["MLAGG_REFERENCE"], "evaluation", "compute_cell_metric.py")
sys.path.insert(0, ROOT)

from tests import _cell_cases as C  # noqa: E402


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def label(mask):                                                   # RESTATED skimage.measure.label (2-D, full connectivity)
    return ndi.label(mask, structure=np.ones((3, 3)))[0]


def relabel_sequential(label_field):                               # RESTATED skimage.segmentation.relabel_sequential (offset 1)
    labels = np.unique(label_field)
    labels = labels[labels > 0]
    out = np.searchsorted(labels, label_field) + 1
    out[label_field <= 0] = 0
    forward = np.zeros(int(labels.max()) + 1 if labels.size else 1, dtype=np.int64)
    forward[labels] = np.arange(1, labels.size + 1)
    return out.astype(label_field.dtype if label_field.dtype.itemsize >= 4 else np.int32), forward, np.concatenate([[0], labels])


def jit(*args, **kwargs):
    if len(args) == 1 and callable(args[0]) and not kwargs:
        return args[0]
    return lambda f: f


def install_stubs():
    _mod("numba", jit=jit)
    seg = _mod("skimage.segmentation", relabel_sequential=relabel_sequential)
    io = _mod("skimage.io", imread=np.load)
    measure = _mod("skimage.measure", label=label)
    _mod("skimage", segmentation=seg, io=io, measure=measure)
    _mod("tifffile", imread=np.load)
    _mod("tqdm", tqdm=lambda it, *a, **k: it)


def run_script(cases, thresholds, extra=()):
    """Run the script on {name: (gt, seg)}; returns ({name: {threshold: CSV row}}, the script's globals)"""
    tmp = tempfile.mkdtemp(prefix="golden_cells_")
    try:
        gt_dir, seg_dir, out_dir = (os.path.join(tmp, d) for d in ("gt", "seg", "out"))
        for d in (gt_dir, seg_dir, out_dir):
            os.makedirs(d)
        for name, (gt, seg) in cases.items():
            with open(os.path.join(gt_dir, name + "_label.tiff"), "wb") as f:
                np.save(f, gt)
            with open(os.path.join(seg_dir, name + ".png"), "wb") as f:
                np.save(f, seg)
        argv = sys.argv
        sys.argv = [SCRIPT, "-g", gt_dir, "-s", seg_dir, "-o", out_dir, "-n", "golden", "-thre"] + [str(t) for t in thresholds] + \
            list(extra)
        try:
            G = runpy.run_path(SCRIPT, run_name="__main__")
        finally:
            sys.argv = argv
        rows = {name: {} for name in cases}
        for th in thresholds:
            with open(os.path.join(out_dir, f"golden-{th}.csv")) as f:
                for row in csv.DictReader(f):
                    name = row.pop("names")[:-len(".png")]
                    rows[name][str(th)] = {k: float(v) for k, v in row.items()}
        return rows, G
    finally:
        shutil.rmtree(tmp)


def tiled(G, gt, seg, roi_size, thresholds):
    """the script's tiled branch (:186-225) composed from its own functions, at another roi_size"""
    seg = label(seg == 1)
    H, W = gt.shape
    n_H, n_W = -(-H // roi_size), -(-W // roi_size)
    gt_pad = np.zeros((roi_size * n_H, roi_size * n_W), dtype=np.int32)
    seg_pad = np.zeros_like(gt_pad)
    gt_pad[:H, :W] = gt
    seg_pad[:H, :W] = seg
    out = np.zeros((len(thresholds), 5), np.int64)                 # true_num, pred_num, tp, fp, fn
    for i in range(n_H):
        for j in range(n_W):
            gt_roi = G["remove_boundary_cells"](gt_pad[roi_size * i:roi_size * (i + 1), roi_size * j:roi_size * (j + 1)].copy())
            seg_roi = G["remove_boundary_cells"](seg_pad[roi_size * i:roi_size * (i + 1), roi_size * j:roi_size * (j + 1)].copy())
            gt_roi, seg_roi = relabel_sequential(gt_roi)[0], relabel_sequential(seg_roi)[0]
            for k, th in enumerate(thresholds):
                out[k] += (np.max(gt_roi), np.max(seg_roi)) + tuple(int(v) for v in G["eval_tp_fp_fn"](gt_roi, seg_roi, threshold=th))
    return out


def main():
    install_stubs()
    data = {}
    cases = {name: make() for name, make in C.CASES.items()}
    rows, G = run_script(cases, C.THRESHOLDS)
    data["rows/default"] = np.array(json.dumps(rows))
    data["rows/count_bd_cells"] = np.array(json.dumps(run_script(cases, C.THRESHOLDS, ["--count_bd_cells"])[0]))
    for name, (gt, seg) in cases.items():
        lab = label(seg == 1)
        data[f"{name}/label"] = lab.astype(np.int32)               # restated labelling, recorded for the order of the components
        g = G["remove_boundary_cells"](gt.astype(np.int32))
        s = G["remove_boundary_cells"](lab.astype(np.int32))
        data[f"{name}/rbc_gt"], data[f"{name}/rbc_seg"] = g.astype(np.int32), s.astype(np.int32)
        data[f"{name}/iou"] = G["_intersection_over_union"](g, s)
        data[f"{name}/tpfpfn"] = np.array([[int(v) for v in G["eval_tp_fp_fn"](g, s, threshold=th)] for th in C.THRESHOLDS], np.int64)
    for name in C.TILED:
        data[f"{name}/tiled"] = tiled(G, *cases[name], C.TILED_ROI, C.THRESHOLDS)
    for name, make in C.PAIRS.items():
        t, p = make()
        data[f"pair/{name}/iou"] = G["_intersection_over_union"](t, p)
        data[f"pair/{name}/tpfpfn"] = np.array([[int(v) for v in G["eval_tp_fp_fn"](t, p, threshold=th)] for th in C.THRESHOLDS], np.int64)
    path = os.path.join(HERE, "cells.npz")
    if "--no-big" in sys.argv:
        data["rows/big"] = np.load(path)["rows/big"]               # keep the recorded row of the large image
    else:
        data["rows/big"] = np.array(json.dumps(run_script({"big": C.big_case()}, (0.5,))[0]))
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {len(data)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
