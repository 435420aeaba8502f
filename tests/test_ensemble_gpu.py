"""Ensembling and model selection on the device (K28, csrc/ensemble.hip, behind mlagg_unet_amd.ensembling / evaluation /
model_selection): every case of tests/_ensemble_cases.py against the reference's recorded results (tests/golden/ensemble.npz) and
against the host path -- means bit for bit, labels, confusion counts, metric dicts and selection results exactly equal --
repeatability, untouched inputs, input forms and the refusals.  Only the fixture is read."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import ensembling as EN
from mlagg_unet_amd import evaluation as EV
from mlagg_unet_amd import ops
from tests import _ensemble_cases as C
from tests.test_ensemble_cpu import GOLDEN, bits, check_selection, golden_metrics, metrics_of, same

gpu = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def device_members(name):
    members = C.ENSEMBLES[name]()
    if name != "i_views":
        return members, [dev(m) for m in members]
    out = []
    for m, off in zip(members, C.VIEW_OFFSETS):                      # the same odd element offsets inside 256-byte aligned device buffers
        buf = torch.zeros(m.size + 8, dtype=torch.float32, device=DEV)
        view = buf[off:off + m.size].view(m.shape)
        view.copy_(torch.from_numpy(m))
        assert view.data_ptr() % 16 == 4 * off
        out.append(view)
    return members, out


@gpu
@pytest.mark.parametrize("name", sorted(C.ENSEMBLES))
def test_mean_and_labels_equal_the_reference_and_the_host_path(name):
    members, dm = device_members(name)
    before = [m.clone() for m in dm]
    labels, mean = EN.ensemble_probabilities(dm, return_probabilities=True)
    assert labels.is_cuda and labels.dtype == torch.uint8 and tuple(labels.shape) == members[0].shape[1:]
    assert mean.dtype == torch.float32 and tuple(mean.shape) == members[0].shape
    host_labels, host_mean = EN.ensemble_probabilities(members, return_probabilities=True)
    got = mean.cpu().numpy()
    assert np.array_equal(bits(got), bits(GOLDEN[f"ens/{name}/mean"])) and np.array_equal(bits(got), bits(host_mean))
    assert np.array_equal(labels.cpu().numpy(), GOLDEN[f"ens/{name}/labels"]) and np.array_equal(labels.cpu().numpy(), host_labels)
    labels2, mean2 = EN.ensemble_probabilities(dm, return_probabilities=True)                  # and again: identical
    assert torch.equal(labels2, labels) and torch.equal(mean2.view(torch.int32), mean.view(torch.int32))
    only_labels, none = EN.ensemble_probabilities(dm)
    assert none is None and torch.equal(only_labels, labels)
    assert torch.equal(EN.average_probabilities(dm).view(torch.int32), mean.view(torch.int32))
    assert all(torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.float16 else torch.int32)) for a, b in zip(dm, before))


@gpu
def test_nan_counts_as_the_maximum_as_on_the_host():
    members = C.nan_members()
    labels, mean = EN.ensemble_probabilities([dev(m) for m in members], return_probabilities=True)
    host_labels, host_mean = EN.ensemble_probabilities(members, return_probabilities=True)
    assert np.array_equal(labels.cpu().numpy(), host_labels) and labels[1, 3] == 2
    assert np.array_equal(bits(mean.cpu().numpy()), bits(host_mean))
    first = [m.copy() for m in members]
    first[0][0, 0, 0] = np.nan                                                                # a NaN in class 0 and a later one: the first wins
    first[1][3, 0, 0] = np.nan
    labels, _ = EN.ensemble_probabilities([dev(m) for m in first])
    assert np.array_equal(labels.cpu().numpy(), EN.ensemble_probabilities(first)[0]) and labels[0, 0] == 0


@gpu
def test_member_forms_agree(tmp_path):
    members = C.ENSEMBLES["d_mixed"]()
    want_l, want_m = GOLDEN["ens/d_mixed/labels"], GOLDEN["ens/d_mixed/mean"]
    files = []
    for i, m in enumerate(members):
        files.append(str(tmp_path / f"m{i}.npz"))
        np.savez_compressed(files[-1], probabilities=m)
    for form in ([dev(m) for m in members], [dev(members[0]), members[1], files[2]], [dev(members[0]), torch.from_numpy(members[1]), members[2]]):
        labels, mean = EN.ensemble_probabilities(form, True)
        assert labels.is_cuda and np.array_equal(labels.cpu().numpy(), want_l) and np.array_equal(bits(mean.cpu().numpy()), bits(want_m))
    rw_written = {}
    rw = type("W", (), {"write_seg": lambda self, seg, f, props: rw_written.__setitem__(f, np.array(seg))})()
    with open(files[0][:-4] + ".pkl", "wb") as f:
        pickle.dump({"p": 1}, f)
    EN.merge_files(files, str(tmp_path / "out"), ".seg", rw, types.SimpleNamespace(has_regions=False), True, device=DEV)
    assert np.array_equal(rw_written[str(tmp_path / "out.seg")], want_l)
    assert np.array_equal(bits(np.load(str(tmp_path / "out.npz"))["probabilities"]), bits(want_m))


@gpu
def test_device_refusals():
    a = dev(C.make_members(3, 1, (4, 5), 1)[0])
    with pytest.raises(RuntimeError, match="shape"):
        EN.ensemble_probabilities([a, a[:, :3].contiguous()])
    with pytest.raises(RuntimeError, match="257 classes"):
        EN.ensemble_probabilities([torch.zeros((257, 3), device=DEV)])
    with pytest.raises(RuntimeError, match="expected a contiguous"):
        ops.ensemble_mean([a.transpose(1, 2)])
    with pytest.raises(RuntimeError, match="at most 63"):
        ops.label_confusion(a.to(torch.uint8), a.to(torch.uint8), torch.zeros(256, dtype=torch.uint8, device=DEV), 64)
    with pytest.raises(RuntimeError, match="both be device tensors"):
        EV.compute_metrics(a.to(torch.uint8), a.to(torch.uint8).cpu(), [1])


@gpu
@pytest.mark.parametrize("tag", sorted(C.METRIC_CASES))
def test_counts_and_metrics_equal_the_reference_and_the_host_path(tag):
    vol, lor, ignore = C.METRIC_CASES[tag]
    ref, pred = C.VOLUMES[vol]()
    dref, dpred = dev(ref), dev(pred)
    values = EV._bins(lor)
    cm = EV.label_confusion(dref, dpred, values, ignore)
    assert cm.dtype == np.int64 and np.array_equal(cm, GOLDEN[f"cm/{tag}"]) and np.array_equal(cm, EV.label_confusion(ref, pred, values, ignore))
    assert np.array_equal(cm, EV.label_confusion(dref, dpred, values, ignore))                # and again: identical
    got = EV.compute_metrics(dref, dpred, lor, ignore)
    assert same(metrics_of(got, lor), {k: golden_metrics(tag)[k] for k in lor})
    assert same(metrics_of(got, lor), metrics_of(EV.compute_metrics(ref, pred, lor, ignore), lor))
    assert np.array_equal(dref.cpu().numpy(), ref) and np.array_equal(dpred.cpu().numpy(), pred)


@gpu
def test_misaligned_and_wider_label_tensors():
    ref, pred = C.VOLUMES["blocks"]()
    values = [0, 1, 2, 3, 4]
    want = EV.label_confusion(ref, pred, values, 4)
    buf_r, buf_p = torch.zeros(ref.size + 16, dtype=torch.uint8, device=DEV), torch.zeros(ref.size + 16, dtype=torch.uint8, device=DEV)
    vr, vp = buf_r[3:3 + ref.size].view(ref.shape), buf_p[16:16 + ref.size].view(ref.shape)  # one base off a 16-byte boundary
    vr.copy_(torch.from_numpy(ref))
    vp.copy_(torch.from_numpy(pred))
    assert np.array_equal(EV.label_confusion(vr, vp, values, 4), want)
    assert np.array_equal(EV.label_confusion(dev(ref).long(), dev(pred).to(torch.int16), values, 4), want)
    tp, fp, fn, tn = EV.compute_tp_fp_fn_tn(dev(ref == 1), dev(pred == 1), dev(ref == 4))
    assert (tp, fp, fn, tn) == EV.compute_tp_fp_fn_tn(ref == 1, pred == 1, ref == 4)
    assert EV.compute_tp_fp_fn_tn(dev(ref == 1), dev(pred == 1)) == EV.compute_tp_fp_fn_tn(ref == 1, pred == 1)


@gpu
@pytest.mark.parametrize("tag", sorted(C.FOLDERS))
def test_cases_summary_equals_the_reference(tag, tmp_path):
    names, lor, ignore = C.FOLDERS[tag]
    vols = C.folder_volumes(names)
    ref_file = str(tmp_path / "reference_summary.json")
    with open(ref_file, "w") as f:
        f.write(str(GOLDEN[f"folder/{tag}/summary_json"]))
    want = EV.load_summary_json(ref_file)
    out = str(tmp_path / "summary.json")
    got = EV.compute_metrics_on_cases([dev(v[0]) for v in vols], [dev(v[1]) for v in vols], lor, ignore, output_file=out)
    host = EV.compute_metrics_on_cases([v[0] for v in vols], [v[1] for v in vols], lor, ignore)
    for r in (got, EV.load_summary_json(out), host):
        assert same(r["mean"], want["mean"]) and same(r["foreground_mean"], want["foreground_mean"])
        assert all(same(g["metrics"], w["metrics"]) for g, w in zip(r["metric_per_case"], want["metric_per_case"]))


@gpu
@pytest.mark.parametrize("tag", C.SELECTIONS)
def test_model_selection_on_the_device(tag):
    got = check_selection(tag, dev)
    host = check_selection(tag)
    assert same(got["all_results"], host["all_results"])
    assert got["best_model_or_ensemble"]["name"] == host["best_model_or_ensemble"]["name"]
    assert got["best_model_or_ensemble"]["postprocessing_kwargs"] == host["best_model_or_ensemble"]["postprocessing_kwargs"]
    assert same(got["best_model_or_ensemble"]["postprocessing_summary"], host["best_model_or_ensemble"]["postprocessing_summary"])
