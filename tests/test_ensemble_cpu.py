"""Ensembling, compute_metrics and model selection, host side (mlagg_unet_amd.ensembling / evaluation / model_selection): the numpy
paths against the reference's own average_probabilities, merge_files, compute_metrics and compute_metrics_on_folder
(tests/golden/ensemble.npz, made by tests/golden/make_golden_ensemble.py), dispatch by input type, the folder drop-ins with a stub
writer, and the errors."""
import json
import math
import os
import pickle
import types

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import ensembling as EN
from mlagg_unet_amd import evaluation as EV
from mlagg_unet_amd import model_selection as MS
from mlagg_unet_amd import ops
from mlagg_unet_amd import postprocessing as PP
from tests import _ensemble_cases as C

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "ensemble.npz"))


def same(a, b):
    """equality of nested dicts / lists / numbers in which NaN equals NaN and ints do not pass for floats (key order is not compared)"""
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a.keys()) == set(b.keys()) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def golden_metrics(tag):
    return {EV.key_to_label_or_region(k): v for k, v in json.loads(str(GOLDEN[f"metrics/{tag}"])).items()}


def metrics_of(result, order):
    m = {k: dict(v) for k, v in result["metrics"].items()}
    EV.recursive_fix_for_json_export(m)
    return {k: m[k] for k in order}


# ---- ensembling ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.ENSEMBLES))
def test_host_mean_and_labels_equal_the_reference(name):
    members = C.ENSEMBLES[name]()
    before = [m.copy() for m in members]
    labels, mean = EN.ensemble_probabilities(members, return_probabilities=True)
    assert mean.dtype == np.float32 and labels.dtype == np.uint8 and labels.shape == members[0].shape[1:]
    assert np.array_equal(bits(mean), bits(GOLDEN[f"ens/{name}/mean"]))
    assert np.array_equal(labels, GOLDEN[f"ens/{name}/labels"])
    assert np.array_equal(bits(EN.average_probabilities(members)), bits(mean))
    labels2, none = EN.ensemble_probabilities(members)
    assert none is None and np.array_equal(labels2, labels)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(members, before))


def test_fixture_inputs_keep_the_margin():
    for name in C.ENSEMBLES:
        mean = GOLDEN[f"ens/{name}/mean"]
        top = np.sort(mean.reshape(mean.shape[0], -1), 0)[-2:]
        assert ((top[1] == top[0]) | (top[1] - top[0] >= C.MARGIN)).all(), name
        assert np.array_equal(GOLDEN[f"ens/{name}/labels"], mean.argmax(0)), name
    ties = GOLDEN["ens/j_ties/labels"].reshape(-1)
    assert ties[0] == 1 and ties[1] == 0 and ties[2] == 0 and ties[5] == 2


def test_nan_counts_as_the_maximum():
    members = C.nan_members()
    labels, mean = EN.ensemble_probabilities(members, return_probabilities=True)
    assert np.isnan(mean[2, 1, 3]) and labels[1, 3] == 2 and np.isnan(mean).sum() == 1


def test_dispatch_by_input_type(tmp_path):
    members = C.ENSEMBLES["d_mixed"]()
    want_l, want_m = GOLDEN["ens/d_mixed/labels"], GOLDEN["ens/d_mixed/mean"]
    labels, mean = EN.ensemble_probabilities([torch.from_numpy(m) for m in members], True)
    assert isinstance(labels, torch.Tensor) and isinstance(mean, torch.Tensor) and not labels.is_cuda
    assert labels.dtype == torch.uint8 and np.array_equal(labels.numpy(), want_l) and np.array_equal(bits(mean.numpy()), bits(want_m))
    files = []
    for i, m in enumerate(members):
        files.append(str(tmp_path / f"m{i}.npz"))
        np.savez_compressed(files[-1], probabilities=m)
    labels, mean = EN.ensemble_probabilities(files, True)
    assert isinstance(mean, np.ndarray) and np.array_equal(labels, want_l) and np.array_equal(bits(mean), bits(want_m))
    labels, _ = EN.ensemble_probabilities([files[0], members[1], members[2]])
    assert np.array_equal(labels, want_l)


def test_member_errors(tmp_path):
    a = C.make_members(3, 1, (4, 5), 1)[0]
    with pytest.raises(RuntimeError, match="At least one"):
        EN.ensemble_probabilities([])
    with pytest.raises(RuntimeError, match="shape"):
        EN.ensemble_probabilities([a, a[:, :3]])
    with pytest.raises(RuntimeError, match="shape"):
        EN.ensemble_probabilities([a, np.concatenate([a, a[:1]])])              # K differs
    with pytest.raises(RuntimeError, match="257 classes"):
        EN.ensemble_probabilities([np.zeros((257, 3), np.float32)])
    with pytest.raises(RuntimeError, match="1 classes"):
        EN.ensemble_probabilities([np.zeros((1, 3), np.float32)])
    with pytest.raises(RuntimeError, match="floating-point"):
        EN.ensemble_probabilities([np.zeros((3, 3), np.int32)])
    with pytest.raises(RuntimeError, match=".npz"):
        EN.ensemble_probabilities([str(tmp_path / "x.npy")])
    assert ops.ENSEMBLE_MAX_CLASSES == 256 and ops.CONFUSION_MAX_LABELS == 63


# ---- the folder drop-ins -------------------------------------------------------------------------------------------------------------
class _Writer:
    def __init__(self):
        self.written = {}

    def write_seg(self, seg, output_fname, properties):
        self.written[output_fname] = (np.array(seg), properties)
        with open(output_fname, "wb") as f:
            f.write(b"seg")


LM = types.SimpleNamespace(has_regions=False)


def _prediction_folder(folder, cases, member):
    os.makedirs(folder, exist_ok=True)
    for c in cases:
        m = C.ENSEMBLES[c]()[member]
        np.savez_compressed(os.path.join(folder, c + ".npz"), probabilities=m)
        with open(os.path.join(folder, c + ".pkl"), "wb") as f:
            pickle.dump({"case": c, "member": member}, f)
    for name in ("dataset.json", "plans.json"):
        with open(os.path.join(folder, name), "w") as f:
            json.dump({"file_ending": ".seg", "from": os.path.basename(folder), "name": name}, f)


def test_merge_files_and_ensemble_folders(tmp_path):
    cases = ["a_odd", "c_single"]
    folders = [str(tmp_path / f"in{i}") for i in range(2)]
    _prediction_folder(folders[0], cases, 0)
    _prediction_folder(folders[1], ["a_odd"], 1)
    np.savez_compressed(os.path.join(folders[1], "c_single.npz"), probabilities=C.ENSEMBLES["c_single"]()[0])
    out, rw = str(tmp_path / "out"), _Writer()
    EN.ensemble_folders(folders, out, True, 3, image_reader_writer=rw, label_manager=LM, device="cpu")
    seg, props = rw.written[os.path.join(out, "a_odd.seg")]
    assert np.array_equal(seg, GOLDEN["ens/a_odd/labels"]) and seg.dtype == np.uint8 and props == {"case": "a_odd", "member": 0}
    assert np.array_equal(bits(np.load(os.path.join(out, "a_odd.npz"))["probabilities"]), bits(GOLDEN["ens/a_odd/mean"]))
    with open(os.path.join(out, "a_odd.pkl"), "rb") as f:
        assert pickle.load(f) == {"case": "a_odd", "member": 0}                  # the properties, not the probabilities
    assert np.array_equal(rw.written[os.path.join(out, "c_single.seg")][0], GOLDEN["ens/c_single/labels"])
    with open(os.path.join(out, "dataset.json")) as f:
        assert json.load(f)["from"] == "in0"
    os.remove(os.path.join(folders[1], "c_single.npz"))
    with pytest.raises(AssertionError, match="Not all folders contain the same files"):
        EN.ensemble_folders(folders, out, image_reader_writer=rw, label_manager=LM, device="cpu")
    with pytest.raises(NotImplementedError, match="region-based"):
        EN.ensemble_folders(folders[:1], out, image_reader_writer=rw, label_manager=types.SimpleNamespace(has_regions=True))
    with pytest.raises(NotImplementedError, match="region-based"):
        EN.merge_files([os.path.join(folders[0], "a_odd.npz")], os.path.join(out, "x"), ".seg", rw,
                       types.SimpleNamespace(has_regions=True))


def _trained_model(folder, member, split):
    for fold, cases in enumerate(split):
        _prediction_folder(os.path.join(folder, f"fold_{fold}", "validation"), cases, member)
    for name in ("dataset.json", "plans.json"):
        with open(os.path.join(folder, name), "w") as f:
            json.dump({"file_ending": ".seg", "from": os.path.basename(folder), "name": name}, f)


def test_ensemble_crossvalidations(tmp_path):
    m0, m1, out = str(tmp_path / "model0"), str(tmp_path / "model1"), str(tmp_path / "ens")
    _trained_model(m0, 0, (["a_odd"], ["i_views"]))
    _trained_model(m1, 1, (["i_views"], ["a_odd"]))                              # another split of the same cases
    rw = _Writer()
    kw = dict(image_reader_writer=rw, label_manager=LM, device="cpu")
    EN.ensemble_crossvalidations([m0, m1], out, folds=(0, 1), **kw)
    for c in ("a_odd", "i_views"):
        assert np.array_equal(rw.written[os.path.join(out, c + ".seg")][0], GOLDEN[f"ens/{c}/labels"])
    assert not os.path.exists(os.path.join(out, "a_odd.npz"))
    for name in ("dataset.json", "plans.json"):
        with open(os.path.join(out, name)) as f:
            assert json.load(f) == {"file_ending": ".seg", "from": "model0", "name": name}
    rw2 = _Writer()
    os.remove(os.path.join(out, "i_views.seg"))
    EN.ensemble_crossvalidations([m0, m1], out, folds=(0, 1), overwrite=False, image_reader_writer=rw2, label_manager=LM, device="cpu")
    assert list(rw2.written) == [os.path.join(out, "i_views.seg")]               # the existing output was skipped
    with pytest.raises(RuntimeError, match="Expected model output directory does not exist"):
        EN.ensemble_crossvalidations([m0, m1], out, folds=(0, 1, 2), **kw)
    os.makedirs(os.path.join(m1, "fold_2", "validation"))
    os.makedirs(os.path.join(m0, "fold_2", "validation"))
    with pytest.raises(RuntimeError, match="No .npz files found"):
        EN.ensemble_crossvalidations([m0, m1], out, folds=(0, 1, 2), **kw)
    _prediction_folder(os.path.join(m0, "fold_2", "validation"), ["a_odd"], 0)
    with pytest.raises(AssertionError, match="Duplicate detected"):
        EN.ensemble_crossvalidations([m0], out, folds=(0, 1, 2), **kw)
    _prediction_folder(os.path.join(m1, "fold_2", "validation"), ["c_single"], 0)
    with pytest.raises(RuntimeError, match="There were missing files"):
        EN.ensemble_crossvalidations([m0, m1], out, folds=(1, 2), **kw)
    with pytest.raises(NotImplementedError, match="region-based"):
        EN.ensemble_crossvalidations([m0, m1], out, folds=(0, 1), image_reader_writer=rw,
                                     label_manager=types.SimpleNamespace(has_regions=True))


# ---- compute_metrics -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(C.METRIC_CASES))
def test_host_counts_and_metrics_equal_the_reference(tag):
    vol, lor, ignore = C.METRIC_CASES[tag]
    ref, pred = C.VOLUMES[vol]()
    values = EV._bins(lor)
    cm = EV.label_confusion(ref, pred, values, ignore)
    assert cm.dtype == np.int64 and np.array_equal(cm, GOLDEN[f"cm/{tag}"])
    got = EV.compute_metrics(ref, pred, lor, ignore)
    assert list(got["metrics"]) == lor
    assert all(isinstance(v["TP"], np.int64) for v in got["metrics"].values())
    assert same(metrics_of(got, lor), {k: golden_metrics(tag)[k] for k in lor})
    again = EV.compute_metrics(torch.from_numpy(ref), torch.from_numpy(pred), lor, ignore)
    assert same(metrics_of(again, lor), metrics_of(got, lor))


def test_main_case_holds_what_it_is_for():
    m = golden_metrics("main_ignore")
    assert math.isnan(m[3]["Dice"]) and math.isnan(m[3]["IoU"]) and m[3]["TN"] > 0          # absent from both volumes
    assert m[2]["n_ref"] == 0 and m[2]["n_pred"] > 0 and m[2]["Dice"] == 0.0                # absent from the reference only
    plain = golden_metrics("main_labels")
    assert plain[1]["FP"] > m[1]["FP"]                                                     # foreground predictions under the ignore label
    assert sum(plain[k]["TP"] + plain[k]["FN"] for k in C.LABELS) < 6 * 9 * 5              # the value 9 is in no label's reference


def test_compute_tp_fp_fn_tn_host():
    ref, pred = C.VOLUMES["main"]()
    for ignore in (None, ref == 4):
        use = np.ones(ref.shape, bool) if ignore is None else ~ignore
        tp, fp, fn, tn = EV.compute_tp_fp_fn_tn(ref == 1, pred == 1, ignore)
        assert (tp, fp, fn, tn) == (((ref == 1) & (pred == 1) & use).sum(), ((ref != 1) & (pred == 1) & use).sum(),
                                    ((ref == 1) & (pred != 1) & use).sum(), ((ref != 1) & (pred != 1) & use).sum())
        t = EV.compute_tp_fp_fn_tn(torch.from_numpy(ref == 1), torch.from_numpy(pred == 1), None if ignore is None else torch.from_numpy(ignore))
        assert t == (tp, fp, fn, tn)


@pytest.mark.parametrize("tag", sorted(C.FOLDERS))
def test_cases_summary_and_json_round_trip(tag, tmp_path):
    names, lor, ignore = C.FOLDERS[tag]
    vols = C.folder_volumes(names)
    ref_file = str(tmp_path / "reference_summary.json")
    with open(ref_file, "w") as f:
        f.write(str(GOLDEN[f"folder/{tag}/summary_json"]))
    want = EV.load_summary_json(ref_file)
    out = str(tmp_path / "summary.json")
    got = EV.compute_metrics_on_cases([v[0] for v in vols], [v[1] for v in vols], lor, ignore, output_file=out)
    assert same(got["mean"], want["mean"]) and same(got["foreground_mean"], want["foreground_mean"])
    assert [same(g["metrics"], w["metrics"]) for g, w in zip(got["metric_per_case"], want["metric_per_case"])] == [True] * len(vols)
    loaded = EV.load_summary_json(out)
    assert same(loaded["mean"], want["mean"]) and same(loaded["foreground_mean"], want["foreground_mean"])
    assert all(same(g["metrics"], w["metrics"]) for g, w in zip(loaded["metric_per_case"], want["metric_per_case"]))
    with open(out) as f, open(ref_file) as g:
        a, b = json.load(f), json.load(g)
    assert list(a) == list(b) and list(a["mean"]) == list(b["mean"])                       # the same keys in the same (sorted) order
    by_id = EV.compute_metrics_on_cases({f"c{i}": v[0] for i, v in enumerate(vols)}, {f"c{i}": v[1] for i, v in enumerate(vols)}, lor, ignore)
    assert same(by_id["mean"], got["mean"]) and [c["prediction_file"] for c in by_id["metric_per_case"]] == [f"c{i}" for i in range(len(vols))]


def test_metric_errors(tmp_path):
    ref, pred = C.VOLUMES["main"]()
    with pytest.raises(RuntimeError, match="64 distinct labels, at most 63"):
        EV.compute_metrics(ref, pred, list(range(64)))
    assert len(EV.compute_metrics(ref, pred, list(range(63)))["metrics"]) == 63
    with pytest.raises(RuntimeError, match="differ in shape"):
        EV.compute_metrics(ref, pred[:, :, :4], [1])
    with pytest.raises(RuntimeError, match="predictions for"):
        EV.compute_metrics_on_cases([ref], [pred, pred], [1])
    with pytest.raises(RuntimeError, match="no reference"):
        EV.compute_metrics_on_cases({"a": ref}, {"b": pred}, [1])
    with pytest.raises(RuntimeError, match=".json"):
        EV.compute_metrics_on_cases([ref], [pred], [1], output_file=str(tmp_path / "summary.txt"))
    assert EV.key_to_label_or_region("(1, 3)") == (1, 3) and EV.key_to_label_or_region("2") == 2
    assert EV.label_or_region_to_key((1, 3)) == "(1, 3)"


# ---- model selection -----------------------------------------------------------------------------------------------------------------
def check_selection(tag, to_device=lambda x: x):
    cands, refs = C.selection(tag)
    cands = {n: {c: (to_device(s), None if p is None else to_device(p)) for c, (s, p) in cases.items()} for n, cases in cands.items()}
    refs = {c: to_device(r) for c, r in refs.items()}
    scores = json.loads(str(GOLDEN[f"sel/{tag}/scores"]))
    got = MS.find_best_configuration(cands, refs, C.SEL_LABELS, folds=C.SEL_FOLDS)
    assert same(got["all_results"], scores) and list(got["all_results"]) == list(scores)     # same keys, same order, same floats
    best = max(scores.values())
    want_key = [k for k in scores if scores[k] == best][0]                      # find_best_configuration.py:142-146
    b = got["best_model_or_ensemble"]
    assert b["name"] == want_key and b["result_on_crossval_pre_pp"] == best
    cases = list(C.SEL_CASES)
    if want_key.startswith("ensemble___"):
        _, m1, m2, _ = want_key.split("___")
        preds = [EN.ensemble_probabilities([cands[m1][c][1], cands[m2][c][1]])[0] for c in cases]
        assert b["selected_model_or_models"] == [{"configuration": m.split("__")[2], "trainer": "nnUNetTrainer",
                                                  "plans_identifier": "nnUNetPlans"} for m in (m1, m2)]
    else:
        preds = [cands[want_key][c][0] for c in cases]
        assert b["selected_model_or_models"] == [{"configuration": want_key.split("__")[2], "trainer": "nnUNetTrainer",
                                                  "plans_identifier": "nnUNetPlans"}]
    fns, kwargs, summary = PP.determine_postprocessing(preds, [refs[c] for c in cases], C.SEL_LABELS, None)
    assert b["postprocessing_fns"] == fns and b["postprocessing_kwargs"] == kwargs and same(b["postprocessing_summary"], summary)
    assert b["result_on_crossval_post_pp"] == summary["postprocessed"]["foreground_mean"]["Dice"]
    off = MS.find_best_configuration(cands, refs, C.SEL_LABELS, allow_ensembling=False, folds=C.SEL_FOLDS)
    singles = {k: v for k, v in scores.items() if not k.startswith("ensemble___")}
    assert same(off["all_results"], singles) and off["ensembling_allowed"] is False
    assert off["best_model_or_ensemble"]["name"] == [k for k in singles if singles[k] == max(singles.values())][0]
    return got


def test_an_ensemble_wins():
    got = check_selection("ensemble_wins")
    assert got["best_model_or_ensemble"]["name"] == MS.get_ensemble_name(C.IDS[0], C.IDS[1], C.SEL_FOLDS)
    assert len(got["all_results"]) == 6


def test_a_single_model_wins_a_tie_with_an_ensemble():
    got = check_selection("tie")
    r = got["all_results"]
    assert r[C.IDS[0]] == r[MS.get_ensemble_name(C.IDS[0], C.IDS[1], C.SEL_FOLDS)] == 1.0
    assert got["best_model_or_ensemble"]["name"] == C.IDS[0]


def test_a_candidate_without_probabilities_is_scored_but_never_paired():
    got = check_selection("unpaired")
    assert list(got["all_results"]) == list(C.IDS) + [MS.get_ensemble_name(C.IDS[0], C.IDS[2], C.SEL_FOLDS)]
    assert got["best_model_or_ensemble"]["name"] == C.IDS[1]


def test_ensemble_name():
    assert MS.get_ensemble_name("/x/a__b__c", "/y/d__e__f", (0, 2)) == "ensemble___a__b__c___d__e__f___0_2"
