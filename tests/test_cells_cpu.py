"""The cell-instance F1 metric on the host (mlagg_unet_amd.cells on numpy arrays and CPU tensors) against the reference's own
evaluation/compute_cell_metric.py (tests/golden/cells.npz, made by tests/golden/make_golden_cells.py): CSV rows, relabelled maps, IoU
matrices bit for bit, tp / fp / fn, the tiled branch at a small roi_size, the assignment against the matching, and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import cells as CL
from tests import _cell_cases as C

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "cells.npz"))
ROWS = {k: json.loads(str(GOLDEN[f"rows/{k}"])) for k in ("default", "count_bd_cells", "big")}
TH = list(C.THRESHOLDS)


def check_rows(got, want_by_threshold, thresholds):
    """every CSV column of every threshold exactly equal"""
    assert [r["threshold"] for r in got] == [float(t) for t in thresholds]
    for row, th in zip(got, thresholds):
        want = want_by_threshold[str(th)]
        for col in CL.COLUMNS:
            assert row[col] == want[col], (th, col, row[col], want[col])
            assert type(row[col]) in (int, float)
        for col in ("precision", "recall", "dice", "F1"):
            assert float(np.round(row[col + "_raw"], 4)) == row[col]


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_case_rows_equal_the_scripts_csv(name):
    gt, seg = C.CASES[name]()
    gt0, seg0 = gt.copy(), seg.copy()
    check_rows(CL.case_cell_metrics(gt, seg, TH), ROWS["default"][name], TH)
    check_rows(CL.case_cell_metrics(gt, seg, TH, count_bd_cells=True), ROWS["count_bd_cells"][name], TH)
    assert np.array_equal(gt, gt0) and np.array_equal(seg, seg0)
    as_tensor = CL.case_cell_metrics(torch.from_numpy(gt.astype(np.int64)), torch.from_numpy(seg), TH)
    check_rows(as_tensor, ROWS["default"][name], TH)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_maps_iou_and_counts_equal_the_scripts_functions(name):
    gt, seg = C.CASES[name]()
    gt0, seg0 = gt.copy(), seg.copy()
    lab, n = CL.label_instances(seg)
    assert lab.dtype == np.int32 and np.array_equal(lab, GOLDEN[f"{name}/label"]) and n == GOLDEN[f"{name}/label"].max()
    g, s = CL.remove_boundary_cells(gt), CL.remove_boundary_cells(lab)
    assert g.dtype == np.int32 and np.array_equal(g, GOLDEN[f"{name}/rbc_gt"])
    assert np.array_equal(s, GOLDEN[f"{name}/rbc_seg"])
    assert np.array_equal(CL.relabel_sequential(g), g)                           # already sequential
    assert np.array_equal(gt, gt0) and np.array_equal(seg, seg0) and np.array_equal(lab, GOLDEN[f"{name}/label"])
    iou = CL.intersection_over_union(g, s)
    want = GOLDEN[f"{name}/iou"]
    assert iou.dtype == np.float64 and iou.shape == want.shape
    assert np.array_equal(iou.view(np.uint64), want.view(np.uint64))             # bit-equal
    for k, th in enumerate(TH):
        assert CL.eval_tp_fp_fn(g, s, th) == tuple(GOLDEN[f"{name}/tpfpfn"][k])
        if iou.shape[0] > 1 and iou.shape[1] > 1:
            assert CL.matching_true_positive(iou[1:, 1:], th) == CL._true_positive_host(iou[1:, 1:], th)


@pytest.mark.parametrize("name", sorted(C.PAIRS))
def test_instance_pairs(name):
    t, p = C.PAIRS[name]()
    iou = CL.intersection_over_union(t, p)
    want = GOLDEN[f"pair/{name}/iou"]
    assert iou.shape == want.shape and np.array_equal(iou.view(np.uint64), want.view(np.uint64))
    for k, th in enumerate(TH):
        assert CL.eval_tp_fp_fn(t, p, th) == tuple(GOLDEN[f"pair/{name}/tpfpfn"][k])
        assert CL.matching_true_positive(iou[1:, 1:], th) == GOLDEN[f"pair/{name}/tpfpfn"][k][0]
    got = CL.eval_tp_fp_fn(torch.from_numpy(t), torch.from_numpy(p), 0.5)
    assert got == tuple(GOLDEN[f"pair/{name}/tpfpfn"][TH.index(0.5)])


def test_the_tie_is_exactly_one_half_and_needs_the_matching():
    t, p = C.PAIRS["tie"]()
    iou = CL.intersection_over_union(t, p)
    assert iou[1, 1] == 0.5 and iou[1, 2] == 0.5
    assert CL.edge_stats(iou[1:, 1:], 0.5) == (3, 2, 1)                           # a plain edge count would say 3
    assert CL.eval_tp_fp_fn(t, p, 0.5) == (2, 1, 0)


def test_both_device_decisions_occur_among_the_cases():
    """the device path answers from the edge count when no row or column has two edges, else from the matching: both happen"""
    plain = matched = differs = 0
    for name in sorted(C.CASES):
        iou = GOLDEN[f"{name}/iou"][1:, 1:]
        for k, th in enumerate(TH):
            count, row_deg, col_deg = CL.edge_stats(iou, th)
            if count and row_deg <= 1 and col_deg <= 1:
                plain += 1
                assert count == GOLDEN[f"{name}/tpfpfn"][k][0]
            elif count:
                matched += 1
                differs += count != GOLDEN[f"{name}/tpfpfn"][k][0]
    assert plain > 0 and matched > 0 and differs > 0


@pytest.mark.parametrize("name", C.TILED)
def test_tiled_branch_at_a_small_roi(name):
    gt, seg = C.CASES[name]()
    want = GOLDEN[f"{name}/tiled"]
    got = CL.case_cell_metrics(gt, seg, TH, roi_size=C.TILED_ROI, large_image_pixels=1)
    for k, row in enumerate(got):
        assert (row["true_num"], row["pred_num"], row["correct_num(TP)"], row["wrong_num(FP)"], row["missed_num(FN)"]) == \
            tuple(want[k])
    assert got[0]["dice"] == ROWS["default"][name][str(TH[0])]["dice"]          # the dice does not depend on the branch


def test_large_image_row():
    gt, seg = C.big_case()
    assert gt.shape == C.BIG_SHAPE and gt.size >= CL.LARGE_IMAGE_PIXELS
    check_rows(CL.case_cell_metrics(gt, seg, (0.5,)), ROWS["big"]["big"], (0.5,))


def test_summary_and_scores():
    rows = [CL.case_cell_metrics(*C.CASES[name](), (0.5,))[0] for name in sorted(C.CASES)]
    f1 = [ROWS["default"][name]["0.5"]["F1"] for name in sorted(C.CASES)]
    assert CL.summarize_f1(rows) == (float(np.mean(f1)), float(np.median(f1)))
    assert CL.summarize_f1(f1) == CL.summarize_f1(rows)
    empty = CL.case_cell_metrics(*C.CASES["both_empty"](), (0.5,))[0]
    assert empty["dice"] == 1.0 and empty["F1"] == 0.0 and empty["true_num"] == 0
    no_gt = CL.case_cell_metrics(*C.CASES["empty_gt"](), (0.5,))[0]
    assert no_gt["dice"] == 0.0 and no_gt["pred_num"] > 0 and no_gt["wrong_num(FP)"] == no_gt["pred_num"]
    no_seg = CL.case_cell_metrics(*C.CASES["empty_seg"](), (0.5,))[0]
    assert no_seg["true_num"] > 0 and no_seg["missed_num(FN)"] == 0             # the reference counts nothing without a prediction


def test_refusals():
    gt, seg = C.CASES["ring"]()
    with pytest.raises(RuntimeError, match="NameError"):
        CL.case_cell_metrics(gt, seg, (0.5,), count_bd_cells=True, large_image_pixels=1, roi_size=64)
    with pytest.raises(RuntimeError):
        CL.case_cell_metrics(gt, seg[:-1], (0.5,))
    with pytest.raises(RuntimeError):
        CL.case_cell_metrics(gt[None], seg[None], (0.5,))
    with pytest.raises(RuntimeError):
        CL.case_cell_metrics(gt, seg, (0.5,), roi_size=4)
    with pytest.raises(RuntimeError):
        CL.relabel_sequential(-gt)
    with pytest.raises(RuntimeError):
        CL.case_cell_metrics(torch.from_numpy(gt), seg.astype(np.float32)[None], (0.5,))
    huge = np.zeros((4, 4), np.int64)
    huge[0, 0] = huge[1, 1] = 2 ** 20
    with pytest.raises(RuntimeError, match="matrix"):
        CL.intersection_over_union(huge, huge)
