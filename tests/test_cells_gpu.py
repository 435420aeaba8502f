"""Cell-instance F1 evaluation on the device (K27, csrc/cells.hip, behind mlagg_unet_amd.cells): every case of tests/_cell_cases.py
against the reference's recorded results (tests/golden/cells.npz) and against the host path -- instance maps, counts, every dict
value exactly equal, IoU matrices bit for bit -- the tiled branch at a small roi_size and at the real 25 M-pixel switch, both ways of
finding tp, repeatability, input types and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import cells as CL
from mlagg_unet_amd import ops
from tests import _cell_cases as C

gpu = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "cells.npz"))
ROWS = {k: json.loads(str(GOLDEN[f"rows/{k}"])) for k in ("default", "count_bd_cells", "big")}
TH = list(C.THRESHOLDS)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def check_rows(got, want_by_threshold, thresholds):
    for row, th in zip(got, thresholds):
        for col in CL.COLUMNS:
            assert row[col] == want_by_threshold[str(th)][col], (th, col, row[col], want_by_threshold[str(th)][col])


@gpu
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_case_rows_equal_the_script_and_the_host_path(name):
    gt, seg = C.CASES[name]()
    dgt, dseg = dev(gt.astype(np.int32) if gt.dtype == np.uint16 else gt), dev(seg)
    for kwargs, rows in (({}, "default"), ({"count_bd_cells": True}, "count_bd_cells")):
        got = CL.case_cell_metrics(dgt, dseg, TH, **kwargs)
        check_rows(got, ROWS[rows][name], TH)
        assert got == CL.case_cell_metrics(gt, seg, TH, **kwargs)                # every key, raw values included
        assert got == CL.case_cell_metrics(dgt, dseg, TH, **kwargs)              # and again: identical
    assert np.array_equal(dgt.cpu().numpy(), gt) and np.array_equal(dseg.cpu().numpy(), seg)


@gpu
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_maps_iou_and_counts(name):
    gt, seg = C.CASES[name]()
    dgt, dseg = dev(gt.astype(np.int32)), dev(seg)
    lab, n = CL.label_instances(dseg)
    assert lab.is_cuda and lab.dtype == torch.int32 and tuple(lab.shape) == seg.shape
    assert np.array_equal(lab.cpu().numpy(), GOLDEN[f"{name}/label"]) and n == int(GOLDEN[f"{name}/label"].max())
    g, s = CL.remove_boundary_cells(dgt), CL.remove_boundary_cells(lab)
    assert np.array_equal(g.cpu().numpy(), GOLDEN[f"{name}/rbc_gt"]) and np.array_equal(s.cpu().numpy(), GOLDEN[f"{name}/rbc_seg"])
    assert np.array_equal(CL.relabel_sequential(dgt).cpu().numpy(), CL.relabel_sequential(gt))
    assert np.array_equal(dgt.cpu().numpy(), gt) and np.array_equal(lab.cpu().numpy(), GOLDEN[f"{name}/label"])
    iou = CL.intersection_over_union(g, s)
    want = GOLDEN[f"{name}/iou"]
    assert iou.dtype == torch.float64 and tuple(iou.shape) == want.shape
    assert np.array_equal(iou.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert torch.equal(iou, CL.intersection_over_union(g, s))
    for k, th in enumerate(TH):
        assert CL.eval_tp_fp_fn(g, s, th) == tuple(GOLDEN[f"{name}/tpfpfn"][k])


@gpu
@pytest.mark.parametrize("name", sorted(C.PAIRS))
def test_instance_pairs(name):
    t, p = C.PAIRS[name]()
    iou = CL.intersection_over_union(dev(t), dev(p))
    want = GOLDEN[f"pair/{name}/iou"]
    assert tuple(iou.shape) == want.shape and np.array_equal(iou.cpu().numpy().view(np.uint64), want.view(np.uint64))
    for k, th in enumerate(TH):
        assert CL.eval_tp_fp_fn(dev(t), dev(p), th) == tuple(GOLDEN[f"pair/{name}/tpfpfn"][k])
    assert CL.eval_tp_fp_fn(dev(t.astype(np.int64)), dev(p.astype(np.int16)), 0.5) == CL.eval_tp_fp_fn(t, p, 0.5)


@gpu
def test_both_ways_of_finding_tp_are_taken():
    before = dict(CL.PATH_COUNTS)
    t, p = C.PAIRS["tie"]()
    assert CL.eval_tp_fp_fn(dev(t), dev(p), 0.5) == (2, 1, 0)                    # two edges in one row: the matching
    assert CL.PATH_COUNTS["matching"] == before["matching"] + 1
    assert CL.eval_tp_fp_fn(dev(t), dev(p), 0.75) == CL.eval_tp_fp_fn(t, p, 0.75)
    assert CL.PATH_COUNTS["edge_count"] == before["edge_count"] + 1
    before = dict(CL.PATH_COUNTS)
    for name in ("dense", "split_merge"):
        gt, seg = C.CASES[name]()
        CL.case_cell_metrics(dev(gt), dev(seg), TH)
    assert CL.PATH_COUNTS["matching"] > before["matching"] and CL.PATH_COUNTS["edge_count"] > before["edge_count"]


@gpu
@pytest.mark.parametrize("name", C.TILED)
def test_tiled_branch_at_a_small_roi(name):
    gt, seg = C.CASES[name]()
    want = GOLDEN[f"{name}/tiled"]
    got = CL.case_cell_metrics(dev(gt), dev(seg), TH, roi_size=C.TILED_ROI, large_image_pixels=1)
    for k, row in enumerate(got):
        assert (row["true_num"], row["pred_num"], row["correct_num(TP)"], row["wrong_num(FP)"], row["missed_num(FN)"]) == \
            tuple(want[k])
    assert got == CL.case_cell_metrics(gt, seg, TH, roi_size=C.TILED_ROI, large_image_pixels=1)
    assert got == CL.case_cell_metrics(dev(gt), dev(seg), TH, roi_size=C.TILED_ROI, large_image_pixels=1)


@gpu
def test_large_image_above_the_real_switch():
    gt, seg = C.big_case()
    dgt, dseg = dev(gt), dev(seg)
    got = CL.case_cell_metrics(dgt, dseg, (0.5, 0.1))
    check_rows(got[:1], ROWS["big"]["big"], (0.5,))
    assert got == CL.case_cell_metrics(gt, seg, (0.5, 0.1))
    assert got == CL.case_cell_metrics(dgt, dseg, (0.5, 0.1))
    lab, n = CL.label_instances(dseg)                                            # labelling across every tile of a large image
    want, n_want = CL.label_instances(seg)
    assert n == n_want and np.array_equal(lab.cpu().numpy(), want)


@gpu
def test_labelling_shapes_that_cross_tiles():
    """spirals, diagonals and combs over many 32 x 64 tiles, odd sizes, uint8 and int32, unaligned views"""
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (1, 300), (300, 1), (33, 65), (97, 259), (256, 512), (131, 1030)):
        for density in (0.35, 0.6):
            seg = (rng.random((H, W)) < density).astype(np.uint8)
            seg[rng.random((H, W)) < 0.05] = 2
            want, n_want = CL.label_instances(seg)
            odd = dev(np.concatenate([[0], seg.ravel()]).astype(np.uint8))[1:].view(H, W)        # contiguous, base not dword-aligned
            assert odd.is_contiguous() and odd.data_ptr() % 4 == 1
            for d in (dev(seg), dev(seg.astype(np.int32)), odd):
                got, n = CL.label_instances(d)
                assert n == n_want and np.array_equal(got.cpu().numpy(), want), (H, W, density)
    y, x = np.mgrid[:200, :333]
    comb = (((x % 4 == 0) & (y > 2)) | (y == 199) | ((x + y) % 37 == 0)).astype(np.uint8)
    got, n = CL.label_instances(dev(comb))
    want, n_want = CL.label_instances(comb)
    assert n == n_want and np.array_equal(got.cpu().numpy(), want)
    got2, n2 = CL.label_instances(dev(comb * 3), foreground=3)
    assert n2 == n_want and torch.equal(got, got2)


@gpu
def test_uint8_prediction_and_other_input_types():
    """predict.predict_case returns uint8 label maps: accepted as they are; gt of any integer type"""
    gt, seg = C.CASES["discs"]()
    assert seg.dtype == np.uint8
    want = CL.case_cell_metrics(gt, seg, TH)
    for gt_type in (np.int16, np.int32, np.int64, np.uint8):
        if gt.max() <= np.iinfo(gt_type).max:
            assert CL.case_cell_metrics(dev(gt.astype(gt_type)), dev(seg), TH) == want
    assert CL.case_cell_metrics(dev(gt), dev(seg.astype(np.int64)), TH) == want
    assert CL.case_cell_metrics(dev(gt).t().contiguous().t(), dev(seg).t().contiguous().t(), TH) == want     # strided views


@gpu
def test_refusals():
    gt, seg = C.CASES["ring"]()
    dgt, dseg = dev(gt), dev(seg)
    with pytest.raises(RuntimeError, match="NameError"):
        CL.case_cell_metrics(dgt, dseg, (0.5,), count_bd_cells=True, large_image_pixels=1, roi_size=64)
    with pytest.raises(RuntimeError):
        CL.case_cell_metrics(dgt, seg, (0.5,))                                   # one on the device, one on the host
    with pytest.raises(RuntimeError):
        CL.case_cell_metrics(dgt, dseg[:-1], (0.5,))
    with pytest.raises(RuntimeError):
        CL.case_cell_metrics(dgt.float(), dseg, (0.5,))
    with pytest.raises(RuntimeError):
        CL.relabel_sequential(-dgt)
    with pytest.raises(RuntimeError):
        CL.remove_boundary_cells(dgt[:4, :4])                                    # no interior inside the ring
    big = dgt.long().clone()
    big[20, 20] = ops.CELLS_MAX_FLAG_BYTES                                       # a flag array above 1 GiB
    with pytest.raises(RuntimeError, match="flags"):
        CL.case_cell_metrics(big, dseg, (0.5,))
    wide = torch.zeros((8, 8), dtype=torch.int32, device=DEV)
    wide[0, 0] = 2 ** 15
    with pytest.raises(RuntimeError, match="overlap matrix"):
        CL.intersection_over_union(wide, wide)
    with pytest.raises(RuntimeError):
        ops.cells_match(*ops.cells_overlap(dgt, dgt, int(gt.max()), int(gt.max())), [0.5] * (ops.CELLS_MAX_THRESHOLDS + 1))
