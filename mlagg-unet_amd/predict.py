"""Prediction of one raw case: the reference's nnUNetPredictor per case
(mlagg/nnunetv2/inference/predict_from_raw_data.py:30-67 preprocessing, :263-288 the fold ensemble, then export_prediction.py), as
one chain of this package's functions:

    preprocessing.preprocess_case -> inference.predict_sliding_window_return_logits (2-D or 3-D tiles, from the configuration's
    patch_size) -> export.convert_predicted_logits_to_segmentation_with_correct_shape

On a CUDA device every step runs on the device (K22, the sliding window with K20 for 3-D tiles, K21); the only read-back on the way
is K22's crop box.  The result is a uint8 label volume in the original geometry, which evaluation.abdomen_case_dsc scores directly.
A region-based dataset.json (tuple-valued labels with a regions_class_order) has one sigmoid head per region; its labels are painted in
that order by the export.

A cascaded configuration (previous_stage in the plans, e.g. 3d_cascade_fullres) also takes the previous stage's segmentation of the case
in the original geometry (predict_from_raw_data.py:47-67): it is preprocessed as the case's seg and enters the network one-hot encoded
below the image channels, on the device through the K32 gather without its one-hot volume.  predict_cascade_case runs both stages of
a case; the first stage's labels never leave the device.
"""
import torch

from . import export, inference, postprocessing as pp, preprocessing


def _regions_class_order(dataset_json):
    """regions_class_order of a region-based dataset.json (a label with more than one value, label_handling.py:32-33), else None."""
    if not any(isinstance(v, (list, tuple)) and len(v) > 1 for v in dataset_json["labels"].values()):
        return None
    if dataset_json.get("regions_class_order") is None:
        raise NotImplementedError("a dataset.json with region labels and no regions_class_order is not supported "
                                  "(label_handling.py:81-82)")
    return [int(v) for v in dataset_json["regions_class_order"]]


def _num_segmentation_heads(dataset_json):
    labels = dataset_json["labels"]
    order = _regions_class_order(dataset_json)
    if order is not None:
        # one sigmoid head per foreground region: every entry but 'ignore' and those that are background only (label_handling.py:77-99)
        regions = [v for k, v in labels.items() if k != "ignore"
                   and not (set(v) == {0} if isinstance(v, (list, tuple)) else int(v) == 0)]
        if len(regions) != len(order):
            raise NotImplementedError(f"regions_class_order has {len(order)} entries for {len(regions)} regions: one label per "
                                      "region is supported (label_handling.py:96-98)")
        return len(regions)
    values = sorted({int(v[0] if isinstance(v, (list, tuple)) else v) for v in labels.values()})
    if "ignore" in labels:                               # the ignore label is not a segmentation head (label_handling.py)
        values.remove(int(labels["ignore"]))
    return len(values)


def foreground_labels(dataset_json):
    """LabelManager.foreground_labels of a label-based dataset.json: the sorted label values without 0 and without the ignore label --
    what the previous stage's segmentation is one-hot encoded with."""
    if _regions_class_order(dataset_json) is not None:
        raise NotImplementedError("region-based labels together with a cascade are not supported")
    labels = dataset_json["labels"]
    values = {int(v[0] if isinstance(v, (list, tuple)) else v) for k, v in labels.items() if k != "ignore"}
    return sorted(v for v in values if v != 0)


def _input_channels(network):
    """The input width of a network: in_channels of its first module that has one (its first convolution), else None."""
    for m in network.modules():
        n = getattr(m, "in_channels", None)
        if isinstance(n, int):
            return n
    return None


@torch.no_grad()
def predict_case(network, image, properties, plans, configuration_name, dataset_json, *, parameters=None, mirror_axes=None,
                 tile_step_size=0.5, use_gaussian=True, tile_batch=None, return_probabilities=False, device=None,
                 postprocessing=None, previous_stage_seg=None):
    """image (c, x, y, z) raw intensities and the reader's properties -> (segmentation uint8 in the original geometry, probabilities
    (K, ...) fp32 or None), on `device` (default: the network's).  parameters: optional list of state dicts (folds), each loaded
    with inference.load_inference_weights; their logits are summed in fp32 and divided by their count.  mirror_axes: the
    reference's inference_allowed_mirroring_axes (None: no test-time mirroring).  postprocessing: (pp_fns, pp_fn_kwargs), e.g. from
    postprocessing.determine_postprocessing or postprocessing_from_json, applied to the exported labels (K23 on the device); the
    probabilities are returned as exported.  previous_stage_seg: for a cascaded configuration, the previous stage's (x, y, z) or
    (1, x, y, z) labels of this case in the original geometry (that stage's predict_case result); the network then reads
    c + len(foreground labels) channels."""
    device = torch.device(device) if device is not None else next(network.parameters()).device
    K = _num_segmentation_heads(dataset_json)
    cfg = preprocessing.get_configuration(plans, configuration_name)
    seg, labels = None, None
    if previous_stage_seg is None:
        data, props = preprocessing.preprocess_case(image, properties, plans, configuration_name, device=device)
    else:
        labels = foreground_labels(dataset_json)
        width = _input_channels(network)
        if width is not None and width != int(image.shape[0]) + len(labels):
            raise RuntimeError(f"the network reads {width} channels, a cascaded stage on this case has {int(image.shape[0])} image "
                               f"channels + {len(labels)} foreground labels = {int(image.shape[0]) + len(labels)}")
        data, seg, props = preprocessing.preprocess_case(image, properties, plans, configuration_name, device=device,
                                                         seg_from_prev_stage=previous_stage_seg, dataset_json=dataset_json)
        seg = torch.as_tensor(seg).to(device)
    data = torch.as_tensor(data).to(device)
    tile = tuple(int(s) for s in cfg["patch_size"])
    if len(tile) not in (2, 3):
        raise RuntimeError(f"patch_size {tile}: 2-D or 3-D tiles expected")
    logits = None
    for sd in (parameters if parameters is not None else [None]):
        if sd is not None:
            inference.load_inference_weights(network, sd)
        out = inference.predict_sliding_window_return_logits(network, data, K, tile, mirror_axes=mirror_axes,
                                                             tile_step_size=tile_step_size, use_gaussian=use_gaussian,
                                                             tile_batch=tile_batch, device=device, previous_stage_seg=seg,
                                                             cascade_labels=labels)
        logits = out if logits is None else logits + out
    if parameters is not None and len(parameters) > 1:
        logits = logits / len(parameters)
    seg, probs = export.convert_predicted_logits_to_segmentation_with_correct_shape(
        logits, props, cfg["spacing"], plans.get("transpose_backward", [0, 1, 2]), return_probabilities=return_probabilities,
        regions_class_order=_regions_class_order(dataset_json))
    if postprocessing is not None:
        seg = pp.apply_postprocessing(seg, *postprocessing)
    return seg, probs


def _per_stage(value):
    """A setting given once for both stages or as a (stage 1, stage 2) pair."""
    if isinstance(value, dict) and set(value) == {0, 1}:
        return value[0], value[1]
    return value, value


@torch.no_grad()
def predict_cascade_case(networks, image, properties, plans, configuration_names, dataset_json, *, parameters=None, mirror_axes=None,
                         tile_step_size=0.5, use_gaussian=True, tile_batch=None, return_probabilities=False, device=None,
                         postprocessing=None):
    """Both stages of the cascade on one raw case: networks (lowres_net, fullres_net) and configuration_names, e.g.
    ("3d_lowres", "3d_cascade_fullres").  Stage 1 runs through predict_case; its uint8 labels in the original geometry stay on the
    device and enter stage 2 as previous_stage_seg.  parameters, mirror_axes and tile_batch hold for both stages, or per stage as a
    dict {0: stage 1's, 1: stage 2's}.  postprocessing applies to stage 2's labels.  -> stage 2's (segmentation, probabilities)."""
    if len(networks) != 2 or len(configuration_names) != 2:
        raise RuntimeError("predict_cascade_case: two networks and two configuration names (the low-resolution stage first)")
    second = preprocessing.get_configuration(plans, configuration_names[1])
    if second.get("previous_stage") != configuration_names[0]:
        raise RuntimeError(f"configuration {configuration_names[1]} has previous_stage {second.get('previous_stage')!r}, not "
                           f"{configuration_names[0]!r}")
    params, mirrors, batches = _per_stage(parameters), _per_stage(mirror_axes), _per_stage(tile_batch)
    device = torch.device(device) if device is not None else next(networks[1].parameters()).device
    lowres, _ = predict_case(networks[0], image, properties, plans, configuration_names[0], dataset_json, parameters=params[0],
                             mirror_axes=mirrors[0], tile_step_size=tile_step_size, use_gaussian=use_gaussian, tile_batch=batches[0],
                             device=device)
    return predict_case(networks[1], image, properties, plans, configuration_names[1], dataset_json, parameters=params[1],
                        mirror_axes=mirrors[1], tile_step_size=tile_step_size, use_gaussian=use_gaussian, tile_batch=batches[1],
                        return_probabilities=return_probabilities, device=device, postprocessing=postprocessing,
                        previous_stage_seg=lowres)
