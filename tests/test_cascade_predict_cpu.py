"""CPU: the cascade's hand-off at prediction time -- export.resample_and_save / resample_logits_to_next_stage / next_stage_target_shape,
preprocessing.preprocess_case(seg_from_prev_stage=...) and the sliding window with a previous-stage segmentation -- against the
reference's own resample_and_save, run_case(seg_file=previous stage) and convert_labelmap_to_one_hot (tests/golden/cascade_predict.npz,
made by tests/golden/make_golden_cascade_predict.py).  The host paths are bit-identical to the reference: equality throughout."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import _lib, dataloading, export as E, inference, predict
from mlagg_unet_amd import preprocessing as P
from tests import _cascade_predict_cases as K
from tests import _preprocess_train_cases as T

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "cascade_predict.npz"))


def managers(tag, regions=False):
    """Duck-typed (plans_manager, configuration_manager) of a hand-off case."""
    label_manager = types.SimpleNamespace(has_regions=regions)
    return (types.SimpleNamespace(get_label_manager=lambda dj: label_manager),
            types.SimpleNamespace(spacing=list(K.HANDOFF[tag][2])))


def handoff(tag, logits, device=None):
    n_classes, _, spacing, _, target, _, _ = K.HANDOFF[tag]
    x = torch.from_numpy(logits) if device is None else torch.from_numpy(logits).to(device)
    return E.resample_logits_to_next_stage(x, target, spacing, K.handoff_properties(tag))


def stacked(data, seg, labels):
    """np.vstack((data, one_hot)) of a preprocessed case, through the package's one_hot."""
    data, seg = torch.as_tensor(data), torch.as_tensor(seg)
    return torch.cat((data, inference.one_hot(seg[0], labels).to(data.device)))


def run_preprocess(tag, device=None):
    plans, name = K.plans(tag)
    return P.preprocess_case(K.image(tag), K.properties(tag), plans, name, device=device, seg_from_prev_stage=K.previous_stage_seg(tag),
                             dataset_json=K.dataset_json(tag))


@pytest.mark.parametrize("tag", list(K.HANDOFF))
@pytest.mark.parametrize("source", ["array", "npy"])
def test_resample_and_save_equals_the_reference(tag, source, tmp_path):
    n_classes, shape, spacing, _, target, _, _ = K.HANDOFF[tag]
    logits = K.logits(tag)
    assert np.array_equal(logits, GOLDEN[f"{tag}/logits"])
    arg = logits
    if source == "npy":
        arg = str(tmp_path / "logits.npy")
        np.save(arg, logits)
    pm, cm = managers(tag)
    out = str(tmp_path / "case.npz")
    E.resample_and_save(arg, list(target), out, pm, cm, K.handoff_properties(tag), K.handoff_dataset_json(n_classes), K.STAGE)
    if source == "npy":
        assert not os.path.exists(arg)                                     # the reference removes the file it loaded
    seg = np.load(out)["seg"]
    assert seg.dtype == np.uint8 and seg.shape == tuple(target)
    assert np.array_equal(seg, GOLDEN[f"{tag}/seg"])
    # both spacings the resampler sees are this configuration's: the decision depends on it alone
    cur = E.current_spacing_for(spacing, K.handoff_properties(tag))
    sep, axis = E.separate_z_decision(cur, cur)
    assert [int(sep), -1 if axis is None else axis] == GOLDEN[f"{tag}/separate_z"].tolist()


def test_handoff_cases_cover_the_branches():
    got = {tag: tuple(GOLDEN[f"{tag}/separate_z"].tolist()) for tag in K.HANDOFF}
    assert got == {"a_isotropic": (0, -1), "b_separate_z": (1, 0), "c_two_lowres": (0, -1), "d_same_shape": (0, -1)}
    assert {K.HANDOFF[t][0] for t in K.HANDOFF} == {2, 4, 14}


def test_handoff_refusals(tmp_path):
    tag = "a_isotropic"
    pm, cm = managers(tag, regions=True)                                  # a region manager without regions_class_order
    with pytest.raises(NotImplementedError):
        E.resample_and_save(K.logits(tag), K.HANDOFF[tag][4], str(tmp_path / "x.npz"), pm, cm, K.handoff_properties(tag),
                            K.handoff_dataset_json(4), K.STAGE)
    with pytest.raises(RuntimeError):
        E.resample_logits_to_next_stage(K.logits(tag), (4, 5), K.HANDOFF[tag][2], K.handoff_properties(tag))
    with pytest.raises(NotImplementedError):
        E.resample_logits_to_next_stage(K.logits(tag), (4, 5, 6), K.HANDOFF[tag][2], K.handoff_properties(tag), order=3)


@pytest.mark.parametrize("tag", list(K.PREPROCESS))
def test_preprocess_with_previous_stage_equals_the_reference(tag):
    data, seg, props = run_preprocess(tag)
    assert isinstance(data, np.ndarray) and data.dtype == np.float32
    assert seg.dtype == GOLDEN[f"{tag}/seg"].dtype and np.array_equal(seg, GOLDEN[f"{tag}/seg"])
    want = GOLDEN[f"{tag}/stack"]
    got = stacked(data, seg, K.foreground_labels(tag)).numpy()
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(np.asarray(props["bbox_used_for_cropping"]), GOLDEN[f"{tag}/bbox"])
    assert tuple(props["shape_before_cropping"]) == tuple(GOLDEN[f"{tag}/shape_before_cropping"])
    assert tuple(props["shape_after_cropping_and_before_resampling"]) == tuple(GOLDEN[f"{tag}/shape_after_cropping"])
    assert "class_locations" not in props
    assert int(GOLDEN[f"{tag}/near_tie"]) == 0
    # a (x, y, z) tensor is the same input
    plans, name = K.plans(tag)
    again = P.preprocess_case(K.image(tag), K.properties(tag), plans, name,
                              seg_from_prev_stage=torch.from_numpy(K.previous_stage_seg(tag)[0]))
    assert np.array_equal(again[0], data) and np.array_equal(again[1], seg)


def test_preprocess_cases_cover_what_they_claim():
    seg = GOLDEN["f_border_box/seg"]
    assert (seg == -1).any() and (seg == 2).any() and not (seg == 3).any()
    assert T.plans("f_border_box")[0]["transpose_forward"] != [0, 1, 2]
    assert GOLDEN["g_masked_zscore/stack"].shape[0] == 2 + 4


@pytest.mark.parametrize("tag,lowres", [("c_isotropic_3d", (3.0, 3.0, 3.0)), ("a_sep_z_changes", (4.0, 1.4, 1.4)),
                                        ("e_transpose", (5.0, 1.8, 1.8))])
def test_next_stage_target_shape_is_the_next_stages_preprocessed_shape(tag, lowres):
    plans = K.cascade_plans(tag, lowres)
    low, props = P.preprocess_case(T.image(tag), T.properties(tag), plans, "3d_lowres")
    data, seg, _ = P.preprocess_case(T.image(tag), T.properties(tag), plans, K.STAGE, seg_from_prev_stage=T.seg(tag))
    assert E.next_stage_target_shape(props, plans, K.STAGE) == tuple(data.shape[1:]) == tuple(seg.shape[1:])
    assert tuple(low.shape[1:]) != tuple(data.shape[1:])


def test_saved_handoff_loads_as_the_second_seg_channel(tmp_path):
    tag = "b_separate_z"
    n_classes, _, _, _, target, _, _ = K.HANDOFF[tag]
    cases, prev = tmp_path / "cases", tmp_path / "predicted_next_stage"
    cases.mkdir()
    prev.mkdir()
    own = np.full((1,) + tuple(target), 1, dtype=np.int8)
    np.savez_compressed(str(cases / "case_0.npz"), data=np.zeros((1,) + tuple(target), np.float32), seg=own)
    with open(cases / "case_0.pkl", "wb") as fh:
        pickle.dump({"class_locations": {}}, fh)
    pm, cm = managers(tag)
    E.resample_and_save(K.logits(tag), target, str(prev / "case_0.npz"), pm, cm, K.handoff_properties(tag),
                        K.handoff_dataset_json(n_classes), K.STAGE)
    ds = dataloading.Dataset(str(cases), folder_with_segs_from_previous_stage=str(prev))
    seg = np.asarray(ds.arrays("case_0")[1])
    assert seg.shape == (2,) + tuple(target)
    assert np.array_equal(seg[0], own[0]) and np.array_equal(seg[1], GOLDEN[f"{tag}/seg"])


def seeded_conv(cin, k, size=3, seed=0):
    torch.manual_seed(seed)
    return torch.nn.Conv3d(cin, k, size, padding=size // 2).eval()


def sliding_window_inputs(shape, c=2, labels=(1, 2, 5), seed=0):
    g = torch.Generator().manual_seed(seed)
    image = torch.randn((c,) + tuple(shape), generator=g)
    seg = torch.randint(-1, 7, tuple(shape), generator=g).to(torch.int8)       # also values that are no cascade label
    return image, seg, list(labels)


@pytest.mark.parametrize("shape", [(11, 13, 20), (6, 13, 20)])
@pytest.mark.parametrize("as_array", [False, True])
def test_sliding_window_with_previous_stage_equals_the_stack(shape, as_array):
    image, seg, labels = sliding_window_inputs(shape)
    net = seeded_conv(2 + 3, 4)
    kw = dict(mirror_axes=(0, 1, 2), tile_batch=3)
    want = inference.predict_sliding_window_return_logits(net, torch.cat((image, inference.one_hot(seg, labels))), 4, (8, 8, 16), **kw)
    given = seg[None].numpy().astype(np.int64) if as_array else seg
    got = inference.predict_sliding_window_return_logits(net, image, 4, (8, 8, 16), previous_stage_seg=given, cascade_labels=labels,
                                                         **kw)
    assert torch.equal(got, want)
    lab = inference.predict_sliding_window_return_segmentation(net, image, 4, (8, 8, 16), previous_stage_seg=given,
                                                               cascade_labels=labels, **kw)
    assert torch.equal(lab, want.argmax(0))


def test_sliding_window_errors():
    image, seg, labels = sliding_window_inputs((8, 9, 16))
    net = seeded_conv(5, 4)
    run = inference.predict_sliding_window_return_logits
    with pytest.raises(RuntimeError, match="3-D"):
        run(torch.nn.Conv2d(5, 4, 1), image, 4, (8, 8), previous_stage_seg=seg, cascade_labels=labels)
    with pytest.raises(RuntimeError, match="go together"):
        run(net, image, 4, (8, 8, 16), previous_stage_seg=seg)
    with pytest.raises(RuntimeError, match="go together"):
        run(net, image, 4, (8, 8, 16), cascade_labels=labels)
    for bad in ([0, 1, 2], [1, 2, 256], []):
        with pytest.raises(RuntimeError, match="cascade_labels"):
            run(net, image, 4, (8, 8, 16), previous_stage_seg=seg, cascade_labels=bad)
    with pytest.raises(RuntimeError, match="does not match the image"):
        run(net, image, 4, (8, 8, 16), previous_stage_seg=seg[:, 1:], cascade_labels=labels)
    with pytest.raises(RuntimeError, match="does not match the image"):
        run(net, image, 4, (8, 8, 16), previous_stage_seg=torch.stack((seg, seg)), cascade_labels=labels)
    with pytest.raises(RuntimeError, match="integer"):
        run(net, image, 4, (8, 8, 16), previous_stage_seg=seg.float() + 0.5, cascade_labels=labels)


def test_preprocess_errors():
    tag = "c_isotropic_3d"
    plans, name = K.plans(tag)
    args = (K.image(tag), K.properties(tag))
    with pytest.raises(RuntimeError, match="seg_from_prev_stage.*missing"):
        P.preprocess_case(*args, plans, name)
    plain, plain_name = T.plans(tag)
    with pytest.raises(RuntimeError, match="no previous_stage"):
        P.preprocess_case(*args, plain, plain_name, seg_from_prev_stage=K.previous_stage_seg(tag))
    with pytest.raises(RuntimeError, match="matching the image"):
        P.preprocess_case(*args, plans, name, seg_from_prev_stage=K.previous_stage_seg(tag)[:, 1:])
    with pytest.raises(NotImplementedError, match="region"):
        P.preprocess_case(*args, plans, name, seg_from_prev_stage=K.previous_stage_seg(tag),
                          dataset_json={"labels": {"background": 0, "whole": [1, 2], "core": 2}, "regions_class_order": [1, 2]})
    # a training case of a cascaded configuration stays refused
    with pytest.raises(NotImplementedError, match="cascade"):
        P.preprocess_training_case(*args[:1], K.previous_stage_seg(tag), args[1], plans, name, K.dataset_json(tag))


def toy_case(tag="g_masked_zscore"):
    """A 2-channel case with a 3-label dataset.json and a two-stage plan."""
    plans = K.cascade_plans(tag, (2.6, 1.6, 2.0))
    dj = {"labels": dict(K.TOY_LABELS), "channel_names": {"0": "a", "1": "b"}}
    return T.image(tag), T.properties(tag), plans, dj


def test_predict_case_errors_and_host_chain():
    image, props, plans, dj = toy_case()
    assert predict.foreground_labels(dj) == [1, 2, 3]
    assert predict.foreground_labels({"labels": {"background": 0, "a": 2, "b": 1, "ignore": 3}}) == [1, 2]
    prev = np.clip(T.seg("g_masked_zscore"), 0, 3)
    with pytest.raises(RuntimeError, match="reads 4 channels.*2 image channels \\+ 3 foreground labels = 5"):
        predict.predict_case(seeded_conv(4, 4), image, props, plans, K.STAGE, dj, previous_stage_seg=prev)
    with pytest.raises(RuntimeError, match="seg_from_prev_stage"):
        predict.predict_case(seeded_conv(5, 4), image, props, plans, K.STAGE, dj)
    with pytest.raises(NotImplementedError):
        predict.predict_case(seeded_conv(5, 4), image, props, plans, K.STAGE,
                             {"labels": {"background": 0, "organ": [1, 2]}, "regions_class_order": [1, 2]}, previous_stage_seg=prev)
    with pytest.raises(RuntimeError, match="previous_stage"):
        predict.predict_cascade_case((seeded_conv(2, 4), seeded_conv(5, 4)), image, props, plans, (K.STAGE, "3d_lowres"), dj)
    nets = (seeded_conv(2, 4, seed=1), seeded_conv(5, 4, seed=2))
    seg, probs = predict.predict_cascade_case(nets, image, props, plans, ("3d_lowres", K.STAGE), dj, mirror_axes={0: None, 1: (0, 1, 2)})
    assert probs is None and seg.dtype == torch.uint8 and tuple(seg.shape) == tuple(image.shape[1:])
    low, _ = predict.predict_case(nets[0], image, props, plans, "3d_lowres", dj)
    want, _ = predict.predict_case(nets[1], image, props, plans, K.STAGE, dj, mirror_axes=(0, 1, 2), previous_stage_seg=low)
    assert torch.equal(seg, want)


def test_abi_exports_the_onehot_gather():
    assert "mlagg_sw_gather_onehot" in _lib.SIGNATURES and hasattr(_lib.lib(), "mlagg_sw_gather_onehot")
    assert len(_lib.SIGNATURES["mlagg_sw_gather_onehot"][1]) == 18
    assert [_lib.CONSTANTS[k] for k in ("MLAGG_SEG_INT8", "MLAGG_SEG_UINT8", "MLAGG_SEG_INT16")] == [0, 1, 2]
