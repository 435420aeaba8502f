"""DSC evaluation: the numbers behind "mean DSC vs reference".

  * validation_step / validation_epoch_end -- the in-loop pseudo-Dice of the reference trainer
    (nnUNetTrainer.py:880-942, 944-978): argmax of the full-resolution head, hard tp/fp/fn per
    foreground class, 2tp / (2tp + fp + fn), nanmean over classes.  Device side: ONE bincount of
    (target * C + prediction) gives the whole confusion matrix (the reference scatters two one-hot
    volumes of B*C*H*W floats and multiplies them three times); DDP sums it with one all_reduce
    (the reference pickles numpy arrays through all_gather_object).
  * compute_dice_coefficient / abdomen_case_dsc / abdomen_mean_dsc -- the offline per-organ DSC of
    evaluation/SurfaceDice.py:481-498 and evaluation/abdomen_DSC_Eval.py:80-113 on label volumes.
  * compute_tp_fp_fn_tn / compute_metrics / compute_metrics_on_cases / save_summary_json / load_summary_json -- the summary.json
    numbers of nnunetv2/evaluation/evaluate_predictions.py on volumes in memory.  Device tensors are counted by K28's
    mlagg_label_confusion (one launch and one read-back of at most 64 x 64 counts per case), numpy arrays and CPU tensors by numpy;
    everything after the integer counts is the reference's numpy arithmetic on either path.
"""
import json
import warnings
from collections import OrderedDict

import numpy as np
import torch
import torch.distributed as dist

from . import ops, trainer

ABDOMEN_ORGANS = ("Liver", "RK", "Spleen", "Pancreas", "Aorta", "IVC", "RAG", "LAG", "Gallbladder", "Esophagus",
                  "Stomach", "Duodenum", "LK")                      # labels 1..13, abdomen_DSC_Eval.py:48-50
SLAB_LABELS = (5, 6, 10)                                            # Aorta, IVC, Esophagus: labelled slices only


def confusion_matrix(pred_labels, target_labels, num_classes):
    """(C, C) int64 counts, row = target label, column = predicted label; stays on the inputs' device."""
    t = target_labels.reshape(-1).long()
    p = pred_labels.reshape(-1).long()
    if t.numel() != p.numel():
        raise RuntimeError("prediction and target differ in size")
    return torch.bincount(t * num_classes + p, minlength=num_classes * num_classes).view(num_classes, num_classes)


def hard_tp_fp_fn(logits, target, ignore_label=None):
    """Foreground tp / fp / fn of argmax(logits) against a label map (reference :899-940, background dropped).  Pixels that
    carry ``ignore_label`` are left out of all three counts (reference B:917-929: ``mask = target != ignore``, the target is
    zeroed there and ``get_tp_fp_fn_tn(..., mask=mask)`` multiplies every count by the mask)."""
    C = logits.shape[1]
    pred, tgt = logits.argmax(1).reshape(-1), target.reshape(-1).long()
    if ignore_label is None:
        cm = confusion_matrix(pred, tgt, C)
    else:
        # no boolean-mask indexing (a nonzero() and a host synchronisation per validation step): ignored pixels are counted into one
        # extra bin that is dropped
        keep = tgt != int(ignore_label)
        idx = torch.where(keep, tgt * C + pred, torch.full_like(tgt, C * C))
        cm = torch.bincount(idx, minlength=C * C + 1)[:C * C].view(C, C)
    tp = cm.diagonal()
    return tp[1:], (cm.sum(0) - tp)[1:], (cm.sum(1) - tp)[1:]


def hard_tp_fp_fn_regions(logits, target, has_ignore_plane=False):
    """tp / fp / fn per sigmoid head of ``sigmoid(logits) > 0.5`` against region planes (reference B:906-927 with
    get_tp_fp_fn_tn(axes=(0, 2, ...), mask=1 - ignore plane)); every head is kept (B:932-939 drops the background of label datasets
    only).  target (B, R, ...) or, with an ignore plane, (B, R + 1, ...).  Torch ops on the inputs' device, no host synchronisation."""
    pred = torch.sigmoid(logits) > 0.5
    if has_ignore_plane:
        keep = target[:, -1:] != 1                          # mask = 1 - target[:, -1:]: the planes are 0 / 1
        target = target[:, :-1]
    else:
        keep = None
    if target.shape != logits.shape:
        raise RuntimeError(f"region planes of shape {tuple(target.shape)} for logits of shape {tuple(logits.shape)}")
    gt = target != 0
    axes = [0] + list(range(2, logits.ndim))
    tp, fp, fn = pred & gt, pred & ~gt, ~pred & gt
    if keep is not None:
        tp, fp, fn = tp & keep, fp & keep, fn & keep
    return tp.sum(axes), fp.sum(axes), fn.sum(axes)


@torch.no_grad()
def validation_step(network, data, target, batch_dice=True, ddp=False, ignore_label=None, loss_fn=None, regions=False):
    """reference validation_step: {'loss', 'tp_hard', 'fp_hard', 'fn_hard'} (device tensors, no host sync).  ``loss_fn``:
    the trainer's own loss (B:897 ``self.loss(output, target)``); default: the fused Dice + CE deep-supervision loss with
    ``ignore_label`` masked inside K9.  ``regions``: the heads are the sigmoid regions of a region-based label manager and the targets
    are region planes (the ignore plane last when ``ignore_label`` is not None): the default loss is the fused Dice + BCE loss (K29)
    and the counts are per head, none dropped (B:906-939)."""
    output = network(data)
    if not isinstance(output, (list, tuple)):
        output, target = [output], target if isinstance(target, (list, tuple)) else [target]
    if loss_fn is not None:
        loss = loss_fn(output, target)
    elif regions:
        loss = trainer.region_deep_supervision_loss(output, target, None, batch_dice=batch_dice, ddp=ddp, ignore_label=ignore_label)
    else:
        loss = trainer.deep_supervision_loss(output, target, batch_dice=batch_dice, ddp=ddp, ignore_label=ignore_label)
    if regions:
        tp, fp, fn = hard_tp_fp_fn_regions(output[0], target[0], ignore_label is not None)
    else:
        tp, fp, fn = hard_tp_fp_fn(output[0], target[0], ignore_label)
    return {"loss": loss.detach(), "tp_hard": tp, "fp_hard": fp, "fn_hard": fn}


def validation_epoch_end(val_outputs, group=None):
    """reference on_validation_epoch_end: {'mean_fg_dice', 'dice_per_class_or_region', 'val_losses'}."""
    tp = torch.stack([o["tp_hard"] for o in val_outputs]).sum(0)
    fp = torch.stack([o["fp_hard"] for o in val_outputs]).sum(0)
    fn = torch.stack([o["fn_hard"] for o in val_outputs]).sum(0)
    loss = torch.stack([o["loss"].reshape(()) for o in val_outputs]).double().mean()
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        packed = torch.cat([tp, fp, fn]).double()
        packed = torch.cat([packed, loss.reshape(1).to(packed.device)])
        dist.all_reduce(packed, group=group)
        n = tp.numel()
        tp, fp, fn = packed[:n], packed[n:2 * n], packed[2 * n:3 * n]
        loss = packed[-1] / dist.get_world_size(group)       # every rank runs the same number of iterations
    tp, fp, fn = (v.double().cpu().numpy() for v in (tp, fp, fn))
    with np.errstate(invalid="ignore", divide="ignore"):
        per_class = 2 * tp / (2 * tp + fp + fn)
    return {"mean_fg_dice": float(np.nanmean(per_class)), "dice_per_class_or_region": [float(v) for v in per_class],
            "val_losses": float(loss)}


def compute_dice_coefficient(mask_gt, mask_pred):
    """SurfaceDice.py:481-498: 2|A & B| / (|A| + |B|); NaN when both masks are empty."""
    volume_sum = int(mask_gt.sum()) + int(mask_pred.sum())
    if volume_sum == 0:
        return float("nan")
    return 2 * int((mask_gt & mask_pred).sum()) / volume_sum


def abdomen_case_dsc(gt, seg, organs=ABDOMEN_ORGANS, slab_labels=SLAB_LABELS):
    """Per-organ DSC of one case (label volumes indexed [x, y, z]), abdomen_DSC_Eval.py:88-106, rounded to 4
    digits as the script stores them.  Runs where the volumes live: torch tensors on the GPU are reduced
    there (one confusion matrix for the whole-volume organs), numpy arrays on the host."""
    if isinstance(gt, np.ndarray):
        gt, seg = torch.from_numpy(gt.astype(np.int64)), torch.from_numpy(np.asarray(seg).astype(np.int64))
    n = len(organs) + 1
    gt, seg = gt.long(), seg.long()
    gt = torch.where((gt > 0) & (gt < n), gt, 0)          # labels outside the organ list count as "not organ i"
    seg = torch.where((seg > 0) & (seg < n), seg, 0)
    cm = confusion_matrix(seg, gt, n).cpu()
    vol_gt, vol_seg = cm.sum(1), cm.sum(0)
    out = OrderedDict()
    for i, organ in enumerate(organs, 1):
        g, s = int(vol_gt[i]), int(vol_seg[i])
        if g == 0 and s == 0:
            d = 1
        elif g == 0 and s > 0:
            d = 0
        elif i in slab_labels:
            z = torch.nonzero((gt == i).flatten(0, 1).any(0)).flatten()
            lo, hi = int(z.min()), int(z.max())
            a, b = gt[:, :, lo:hi] == i, seg[:, :, lo:hi] == i        # the script's half-open z range
            d = compute_dice_coefficient(a, b)
        else:
            d = 2 * int(cm[i, i]) / (g + s)
        out[organ] = round(d, 4)
    return out


def abdomen_mean_dsc(cases):
    """Column means over cases, then their mean (abdomen_DSC_Eval.py:108-114; pandas means skip NaN)."""
    organs = list(cases[0].keys())
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # an organ that is NaN in every case stays NaN
        cols = OrderedDict((o, float(np.nanmean([c[o] for c in cases]))) for o in organs)
    return cols, float(np.nanmean(list(cols.values())))


# ------------------------------------------------------------------------------------------------
# compute_metrics: the reference's evaluate_predictions.py on volumes in memory (K28 counts on the device)
# ------------------------------------------------------------------------------------------------
METRIC_KEYS = ("Dice", "IoU", "FP", "TP", "FN", "TN", "n_pred", "n_ref")      # compute_metrics' keys, in its order


def label_or_region_to_key(label_or_region):
    return str(label_or_region)


def key_to_label_or_region(key):
    try:
        return int(key)
    except ValueError:
        return tuple(int(i) for i in key.replace("(", "").replace(")", "").split(",") if i.strip())


def _region_labels(label_or_region):
    return [int(v) for v in label_or_region] if isinstance(label_or_region, (tuple, list)) else [int(label_or_region)]


def _bins(labels_or_regions):
    """The distinct label values of labels_or_regions in order of appearance: value i of the list is bin i, any other value bin L."""
    values = []
    for r in labels_or_regions:
        for v in _region_labels(r):
            if v not in values:
                values.append(v)
    if len(values) > ops.CONFUSION_MAX_LABELS:
        raise RuntimeError(f"compute_metrics: {len(values)} distinct labels, at most {ops.CONFUSION_MAX_LABELS} are supported")
    return values


def _is_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _device_labels(x, name):
    """x as a contiguous uint8 device tensor (other integer dtypes are converted once their values are known to fit)."""
    if x.dtype == torch.bool:
        return x.contiguous().view(torch.uint8)
    if x.dtype.is_floating_point or x.dtype.is_complex:
        raise RuntimeError(f"{name}: an integer label tensor expected, got {x.dtype}")
    if x.dtype != torch.uint8:
        lo, hi = (int(v) for v in torch.aminmax(x))
        if lo < 0 or hi > 255:
            raise RuntimeError(f"{name}: labels in [{lo}, {hi}]; the device path reads uint8 labels")
        x = x.to(torch.uint8)
    return x.contiguous()


def label_confusion(reference, prediction, values, ignore_label=None):
    """(L + 1, L + 1) int64 numpy array, L = len(values): voxels per (reference bin, prediction bin), bin i = the label values[i], bin L =
    any other value; voxels whose reference value is ignore_label are left out (ignore_mask = seg_ref == ignore_label).  Device
    tensors: one K28 launch and one read-back; numpy arrays and CPU tensors: np.bincount."""
    L = len(values)
    if L > ops.CONFUSION_MAX_LABELS:
        raise RuntimeError(f"label_confusion: {L} labels, at most {ops.CONFUSION_MAX_LABELS} are supported")
    if tuple(reference.shape) != tuple(prediction.shape):
        raise RuntimeError(f"prediction {tuple(prediction.shape)} and reference {tuple(reference.shape)} differ in shape")
    if _is_device(reference) != _is_device(prediction):
        raise RuntimeError("reference and prediction must both be device tensors or both live on the host")
    if _is_device(reference):
        table = torch.full((256,), L, dtype=torch.uint8)
        for i, v in enumerate(values):
            if 0 <= v <= 255:
                table[v] = i
        cm = ops.label_confusion(_device_labels(reference, "reference"), _device_labels(prediction, "prediction"),
                                 table.to(reference.device), L, ignore_label)
        return cm.cpu().numpy()
    ref = reference.numpy() if isinstance(reference, torch.Tensor) else np.asarray(reference)
    pred = prediction.numpy() if isinstance(prediction, torch.Tensor) else np.asarray(prediction)
    a, b = np.full(ref.shape, L, np.int64), np.full(pred.shape, L, np.int64)
    for i, v in enumerate(values):
        a[ref == v] = i
        b[pred == v] = i
    idx = a * (L + 1) + b
    if ignore_label is not None:
        idx = idx[ref != ignore_label]
    return np.bincount(idx.ravel(), minlength=(L + 1) ** 2).astype(np.int64).reshape(L + 1, L + 1)


def _tp_fp_fn_tn(cm, rows):
    """tp, fp, fn, tn (np.int64) of the label set whose bins are `rows` from a confusion matrix."""
    tp = cm[np.ix_(rows, rows)].sum()
    fn = cm[rows, :].sum() - tp
    fp = cm[:, rows].sum() - tp
    return tp, fp, fn, cm.sum() - tp - fp - fn


def compute_tp_fp_fn_tn(mask_ref, mask_pred, ignore_mask=None):
    """The reference's compute_tp_fp_fn_tn (evaluate_predictions.py:77-86) on boolean masks: (tp, fp, fn, tn) as np.int64.  Device
    tensors are counted by K28, numpy arrays and CPU tensors by the reference's numpy expressions."""
    if _is_device(mask_ref):
        ref = mask_ref.to(torch.bool).contiguous().view(torch.uint8)
        if ignore_mask is not None:
            ref = torch.where(ignore_mask.to(torch.bool), torch.full_like(ref, 2), ref)
        cm = label_confusion(ref, mask_pred.to(torch.bool), [0, 1], 2 if ignore_mask is not None else None)
        return cm[1, 1], cm[0, 1], cm[1, 0], cm[0, 0]
    ref, pred = (np.asarray(m.numpy() if isinstance(m, torch.Tensor) else m, dtype=bool) for m in (mask_ref, mask_pred))
    if ignore_mask is None:
        use_mask = np.ones_like(ref, dtype=bool)
    else:
        use_mask = ~np.asarray(ignore_mask.numpy() if isinstance(ignore_mask, torch.Tensor) else ignore_mask, dtype=bool)
    tp = np.sum((ref & pred) & use_mask)
    fp = np.sum(((~ref) & pred) & use_mask)
    fn = np.sum((ref & (~pred)) & use_mask)
    tn = np.sum(((~ref) & (~pred)) & use_mask)
    return tp, fp, fn, tn


def compute_metrics(reference, prediction, labels_or_regions, ignore_label=None):
    """The reference's compute_metrics (evaluate_predictions.py:89-120) on two label volumes in memory: {'metrics': {label or region
    tuple: {'Dice', 'IoU', 'FP', 'TP', 'FN', 'TN', 'n_pred', 'n_ref'}}}, Dice and IoU NaN when tp + fp + fn == 0.  The counts are
    np.int64 and the ratios its numpy expressions, so every value equals the reference's exactly.  At most 63 distinct label
    values; a region is a tuple of labels whose masks are united."""
    values = _bins(labels_or_regions)
    cm = label_confusion(reference, prediction, values, ignore_label)
    results = {"metrics": {}}
    for r in labels_or_regions:
        key = tuple(r) if isinstance(r, list) else r
        tp, fp, fn, tn = _tp_fp_fn_tn(cm, [values.index(v) for v in dict.fromkeys(_region_labels(r))])
        m = {}
        if tp + fp + fn == 0:
            m["Dice"] = np.nan
            m["IoU"] = np.nan
        else:
            m["Dice"] = 2 * tp / (2 * tp + fp + fn)
            m["IoU"] = tp / (tp + fp + fn)
        m["FP"], m["TP"], m["FN"], m["TN"], m["n_pred"], m["n_ref"] = fp, tp, fn, tn, fp + tp, fn + tp
        results["metrics"][key] = m
    return results


def recursive_fix_for_json_export(d):
    """The reference's utilities/json_export.py for the values compute_metrics produces: numpy scalars become Python numbers, in
    place, through nested dicts, lists and tuples."""
    def fix(v):
        if isinstance(v, dict):
            recursive_fix_for_json_export(v)
            return v
        if isinstance(v, (list, tuple)):
            return type(v)(fix(i) for i in v)
        if isinstance(v, np.bool_):
            return bool(v)
        if isinstance(v, np.integer):
            return int(v)
        if isinstance(v, np.floating):
            return float(v)
        return v

    for k in list(d.keys()):
        v = d.pop(k)
        d[int(k) if isinstance(k, np.integer) else k] = fix(v)


def compute_metrics_on_cases(references, predictions, labels_or_regions, ignore_label=None, output_file=None):
    """The reference's compute_metrics_on_folder (evaluate_predictions.py:123-175) on volumes in memory, one case after another where
    they live.  references and predictions: lists in the same case order, or dicts by case id (every predicted case is scored, in the
    predictions' order).  Returns {'metric_per_case', 'mean', 'foreground_mean'}: np.nanmean over the cases in order, then np.mean over
    the keys other than 0 (:151-167), all values Python numbers; 'reference_file' and 'prediction_file' of a case hold its id (its
    index for lists).  output_file (must end with .json): also written with save_summary_json."""
    if output_file is not None and not output_file.endswith(".json"):
        raise RuntimeError("output_file should end with .json")
    if isinstance(predictions, dict):
        missing = [k for k in predictions if k not in references]
        if missing:
            raise RuntimeError(f"no reference for the predicted cases {missing}")
        ids = list(predictions)
    else:
        if len(predictions) != len(references):
            raise RuntimeError(f"{len(predictions)} predictions for {len(references)} references")
        ids = list(range(len(predictions)))
    if not ids:
        raise RuntimeError("compute_metrics_on_cases: no cases")
    labels_or_regions = [tuple(r) if isinstance(r, list) else r for r in labels_or_regions]
    results = []
    for i in ids:
        r = compute_metrics(references[i], predictions[i], labels_or_regions, ignore_label)
        results.append({"reference_file": i, "prediction_file": i, "metrics": r["metrics"]})
    means = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # all-NaN columns and an empty foreground give the reference's NaN
        for r in labels_or_regions:
            means[r] = {m: np.nanmean([i["metrics"][r][m] for i in results]) for m in METRIC_KEYS}
        foreground_mean = {m: np.mean([means[k][m] for k in means if not (k == 0 or k == "0")]) for m in METRIC_KEYS}
    for i in results:
        recursive_fix_for_json_export(i)
    recursive_fix_for_json_export(means)
    recursive_fix_for_json_export(foreground_mean)
    result = {"metric_per_case": results, "mean": means, "foreground_mean": foreground_mean}
    if output_file is not None:
        save_summary_json(result, output_file)
    return result


def save_summary_json(results, output_file):
    """The reference's save_summary_json (:34-48): label and region-tuple keys become strings, keys sorted, indent 4."""
    converted = dict(results)
    converted["mean"] = {label_or_region_to_key(k): v for k, v in results["mean"].items()}
    converted["metric_per_case"] = [dict(c, metrics={label_or_region_to_key(k): v for k, v in c["metrics"].items()})
                                    for c in results["metric_per_case"]]
    with open(output_file, "w") as f:
        json.dump(converted, f, sort_keys=True, indent=4)


def load_summary_json(filename):
    """The reference's load_summary_json (:51-60): the string keys become labels and region tuples again."""
    with open(filename) as f:
        results = json.load(f)
    results["mean"] = {key_to_label_or_region(k): v for k, v in results["mean"].items()}
    for c in results["metric_per_case"]:
        c["metrics"] = {key_to_label_or_region(k): v for k, v in c["metrics"].items()}
    return results
