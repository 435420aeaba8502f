"""Postprocessing by connected components, host side (mlagg_unet_amd.postprocessing): the host path and determine_postprocessing
against the reference's own remove_connected_components.py (tests/golden/postprocess.npz, made by
tests/golden/make_golden_postprocess.py), the JSON form, the argument forms and predict_case with postprocessing."""
import json
import os

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import predict
from mlagg_unet_amd import postprocessing as PP
from tests import _postprocess_cases as C
from tests import _preprocess_cases as PC

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "postprocess.npz"))


def cv_inputs(tag):
    n = sum(1 for k in GOLDEN.files if k.startswith(f"cv/{tag}/pred_"))
    preds = [GOLDEN[f"cv/{tag}/pred_{i}"] for i in range(n)]
    refs = [GOLDEN[f"cv/{tag}/ref_{i}"] for i in range(n)]
    ignore = int(GOLDEN[f"cv/{tag}/ignore"])
    return preds, refs, GOLDEN[f"cv/{tag}/labels"].tolist(), None if ignore < 0 else ignore


def reference_json(tag):
    return json.loads(str(GOLDEN[f"cv/{tag}/postprocessing_json"]))


def test_fixture_inputs_are_the_seeded_cases():
    for tag, make in C.VOLUMES.items():
        assert np.array_equal(GOLDEN[f"{tag}/input"], make())
    for tag in C.CV_SETS:
        preds, refs, labels, ignore = C.cv_set(tag)
        want = cv_inputs(tag)
        assert all(np.array_equal(a, b) for a, b in zip(preds, want[0]))
        assert all(np.array_equal(a, b) for a, b in zip(refs, want[1]))
        assert (labels, ignore) == (want[2], want[3])


@pytest.mark.parametrize("tag", sorted(C.CALLS))
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_host_path_matches_the_reference(tag, kind):
    vol, lr, bg, _ = C.CALLS[tag]
    x = GOLDEN[f"{vol}/input"].copy()
    seg = torch.from_numpy(x) if kind == "torch" else x
    got = PP.remove_all_but_largest_component_from_segmentation(seg, lr, background_label=bg)
    assert type(got) is type(seg) and got.dtype == seg.dtype and tuple(got.shape) == x.shape
    assert np.array_equal(np.asarray(got), GOLDEN[f"{tag}/output"])
    assert np.array_equal(x, GOLDEN[f"{vol}/input"])                     # the input is never modified


@pytest.mark.parametrize("tag", sorted(C.VOLUMES))
def test_host_per_class_grouping_equals_the_reference_chain(tag):
    labels = GOLDEN[f"{tag}/per_class_labels"].tolist()
    got = PP._keep_largest(GOLDEN[f"{tag}/input"], {label: label for label in labels}, 0)
    assert np.array_equal(got, GOLDEN[f"{tag}/per_class"])


def test_fixture_covers_the_connectivity_cases():
    # full connectivity decides these: with 6- or 18-neighbours the other component would be kept
    out = GOLDEN["contacts_1/output"]
    assert out[11, 12, 13] == 0 and out[1, 1, 1] == 1 and out[6, 6, 8] == 1
    out = GOLDEN["contacts_2/output"]
    assert out[8, 1, 12] == 0 and out[1, 6, 8] == 2
    out = GOLDEN["ties_1/output"]
    assert out[1, 1, 1] == 1 and out[7, 7, 7] == 1 and out[1, 8, 1] == 0
    assert (GOLDEN["multi_bg7/output"] == 7).any()
    assert np.array_equal(GOLDEN["multi_empty/output"], GOLDEN["multi/input"])


@pytest.mark.parametrize("tag", sorted(C.CV_SETS))
def test_determine_postprocessing_matches_the_reference(tag):
    preds, refs, labels, ignore = cv_inputs(tag)
    fns, kwargs, summary = PP.determine_postprocessing(preds, refs, labels, ignore_label=ignore)
    want = reference_json(tag)
    assert [f.__name__ for f in fns] == want["postprocessing_fns"]
    assert kwargs == want["postprocessing_kwargs"]
    # every number, NaN included, through the same JSON encoder
    assert json.dumps(summary, sort_keys=True) == json.dumps(want, sort_keys=True)
    for i, p in enumerate(preds):
        assert np.array_equal(PP.apply_postprocessing(p, fns, kwargs), GOLDEN[f"cv/{tag}/pp_{i}"])


def test_cv_sets_cover_the_decision_branches():
    first = {tag: reference_json(tag)["postprocessing_kwargs"] for tag in C.CV_SETS}
    assert first["a_fg_accepted"][0] == {"labels_or_regions": [1, 2]}
    b = reference_json("b_fg_rejected_class_falls")
    assert b["postprocessing_kwargs"] == [{"labels_or_regions": 1}]
    # rejected although the foreground mean rose: label 2 fell
    preds, refs, labels, ignore = cv_inputs("b_fg_rejected_class_falls")
    fg = [PP.remove_all_but_largest_component_from_segmentation(p, labels) for p in preds]
    after = PP._metrics(PP._counts(fg, refs, labels, ignore), labels)
    assert after["foreground_mean"]["Dice"] > b["input_folder"]["foreground_mean"]["Dice"]
    assert after["mean"][2]["Dice"] < b["input_folder"]["mean"]["2"]["Dice"]
    assert first["c_some_classes"] == [{"labels_or_regions": 1}]
    assert cv_inputs("d_ignore_label")[3] == 4


def test_postprocessing_from_json_round_trips():
    for tag in C.CV_SETS:
        want = reference_json(tag)
        fns, kwargs = PP.postprocessing_from_json(want)
        preds = cv_inputs(tag)[0]
        assert [f.__name__ for f in fns] == want["postprocessing_fns"]
        for i, p in enumerate(preds):
            assert np.array_equal(PP.apply_postprocessing(p, fns, kwargs), GOLDEN[f"cv/{tag}/pp_{i}"])
    fns, kwargs = PP.postprocessing_from_json({"postprocessing_fns": ["remove_all_but_largest_component_from_segmentation"],
                                               "postprocessing_kwargs": [{"labels_or_regions": [[1, 3], 2]}]})
    assert kwargs == [{"labels_or_regions": [(1, 3), 2]}]
    with pytest.raises(ValueError):
        PP.postprocessing_from_json({"postprocessing_fns": ["fill_holes"], "postprocessing_kwargs": [{}]})


def test_two_d_images_need_no_separate_path():
    x = GOLDEN["two_d/input"]
    assert np.array_equal(PP.remove_all_but_largest_component_from_segmentation(x[0], [1, 2]), GOLDEN["two_d_fg/output"][0])


def test_determine_postprocessing_rejects_mismatched_inputs():
    preds, refs, labels, _ = cv_inputs("a_fg_accepted")
    with pytest.raises(RuntimeError):
        PP.determine_postprocessing(preds, refs[:-1], labels)
    with pytest.raises(RuntimeError):
        PP.determine_postprocessing(preds, [r[:-1] for r in refs], labels)


def test_predict_case_applies_postprocessing_on_cpu():
    from tests.test_preprocess_cpu import TinyNet3d
    tag, K = "c_isotropic_3d", 3
    plans, name = PC.plans(tag)
    dj = {"labels": {"background": 0, "liver": 1, "spleen": 2}}
    net = TinyNet3d(1, K)
    pp = ([PP.remove_all_but_largest_component_from_segmentation] * 2, [{"labels_or_regions": [1, 2]}, {"labels_or_regions": 2}])
    seg, _ = predict.predict_case(net, PC.image(tag), PC.properties(tag), plans, name, dj, device="cpu", postprocessing=pp)
    plain, _ = predict.predict_case(net, PC.image(tag), PC.properties(tag), plans, name, dj, device="cpu")
    assert seg.dtype == torch.uint8 and torch.equal(seg, PP.apply_postprocessing(plain, *pp))
