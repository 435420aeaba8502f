"""Postprocessing by connected components: the reference's
mlagg/nnunetv2/postprocessing/remove_connected_components.py on in-memory label volumes.

    remove_all_but_largest_component_from_segmentation   keep only the largest 26-connected component of the united mask (:22-34)
    apply_postprocessing                                 the chosen steps in order (:37-40)
    determine_postprocessing                             the reference's decision rules (:51-246) on lists of volumes
    postprocessing_from_json                             (pp_fns, pp_fn_kwargs) from a reference postprocessing.json

A CUDA tensor runs K23 (csrc/components.hip, ops.keep_largest_component); CPU tensors and numpy arrays run scipy.ndimage.label with
the full 3 x 3 x 3 structure, which is what acvl_utils' remove_all_but_largest_component gets from skimage.measure.label.  Both keep
every component whose size equals the maximum, and both give the same labels bit for bit.  2-D images arrive as (1, H, W), as
nnU-Net stores them.
"""
import numpy as np
import scipy.ndimage as ndi
import torch

from . import evaluation, ops

METRICS = ("Dice", "IoU", "FP", "TP", "FN", "TN", "n_pred", "n_ref")      # compute_metrics' keys, in its order


def _united_labels(labels_or_regions):
    """The labels whose masks the reference unites (region_or_label_to_mask over a label, a tuple, or a list of them)."""
    items = labels_or_regions if isinstance(labels_or_regions, list) else [labels_or_regions]
    out = []
    for item in items:
        for label in (item if isinstance(item, (tuple, list)) else (item,)):
            if int(label) not in out:
                out.append(int(label))
    return out


def _group_table(groups, device):
    """groups: {label: group}; labels outside 0..255 cannot occur in a uint8 volume and are dropped."""
    table = torch.zeros(256, dtype=torch.uint8)
    for label, g in groups.items():
        if 0 <= label <= 255:
            table[label] = g
    return table.to(device)


def _as_volume(seg):
    """A view of seg as (X, Y, Z): 2-D and 1-D inputs get leading axes of one (their connectivity is unchanged)."""
    if seg.dim() > 3 or seg.dim() < 1:
        raise RuntimeError(f"segmentation: 1-D to 3-D expected, got shape {tuple(seg.shape)}")
    return seg.reshape((1,) * (3 - seg.dim()) + tuple(seg.shape))


def _keep_largest_device(seg, groups, background_label):
    """K23 on a CUDA tensor of any integer dtype; groups {label: group}.  Returns (result with seg's dtype and shape, stats)."""
    if seg.dtype.is_floating_point or seg.dtype.is_complex or seg.dtype == torch.bool:
        raise RuntimeError(f"segmentation: an integer label tensor expected, got {seg.dtype}")
    vol = _as_volume(seg)
    if vol.numel() > ops.CC_MAX_VOXELS:
        raise RuntimeError(f"keep_largest_component: {vol.numel()} voxels, at most {ops.CC_MAX_VOXELS} are supported")
    if seg.dtype != torch.uint8:
        lo, hi = (int(v) for v in torch.aminmax(vol))
        if lo < 0 or hi > 255:
            raise RuntimeError(f"segmentation: labels in [{lo}, {hi}]; K23 reads uint8 labels")
    out, stats = ops.keep_largest_component(vol.to(torch.uint8).contiguous(), _group_table(groups, seg.device), background_label)
    return out.to(seg.dtype).reshape(seg.shape), stats


def _keep_largest_host(seg, groups, background_label):
    """numpy: for every group, scipy.ndimage.label of its mask with full connectivity, np.bincount, keep the maximal components."""
    ret = np.copy(seg)
    by_group = {}
    for label, g in groups.items():
        by_group.setdefault(g, []).append(label)
    structure = np.ones((3,) * seg.ndim, dtype=bool)
    for g in sorted(by_group):
        mask = np.isin(seg, by_group[g])
        components, n = ndi.label(mask, structure=structure)
        if n == 0:
            continue
        sizes = np.bincount(components.ravel())[1:]
        keep = np.flatnonzero(sizes == sizes.max()) + 1
        ret[mask & ~np.isin(components, keep)] = background_label
    return ret


def _keep_largest(segmentation, groups, background_label):
    if isinstance(segmentation, torch.Tensor):
        if segmentation.is_cuda:
            return _keep_largest_device(segmentation, groups, background_label)[0]
        return torch.from_numpy(_keep_largest_host(segmentation.numpy(), groups, background_label))
    return _keep_largest_host(np.asarray(segmentation), groups, background_label)


def remove_all_but_largest_component_from_segmentation(segmentation, labels_or_regions, background_label=0):
    """The reference's function (:22-34): unite the masks of labels_or_regions (an int, a tuple = region, or a list of them), keep the
    largest 26-connected component(s) of that mask and set the rest of it to background_label.  The input is not modified; the
    result has its type, dtype, shape and device."""
    return _keep_largest(segmentation, {label: 1 for label in _united_labels(labels_or_regions)}, int(background_label))


def apply_postprocessing(segmentation, pp_fns, pp_fn_kwargs):
    """The reference's apply_postprocessing (:37-40)."""
    for fn, kwargs in zip(pp_fns, pp_fn_kwargs):
        segmentation = fn(segmentation, **kwargs)
    return segmentation


_FUNCTIONS = {f.__name__: f for f in (remove_all_but_largest_component_from_segmentation,)}


def postprocessing_from_json(d):
    """(pp_fns, pp_fn_kwargs) from the dict of a reference postprocessing.json (its 'postprocessing_fns' names and
    'postprocessing_kwargs').  JSON stores region tuples as lists: a list nested in labels_or_regions becomes a tuple again (a flat
    list of labels unites the same voxels either way).  An unknown function name raises ValueError."""
    fns, kwargs = [], []
    for name, kw in zip(d["postprocessing_fns"], d["postprocessing_kwargs"]):
        if name not in _FUNCTIONS:
            raise ValueError(f"unknown postprocessing function {name!r}; known: {sorted(_FUNCTIONS)}")
        kw = dict(kw)
        lr = kw.get("labels_or_regions")
        if isinstance(lr, list):
            kw["labels_or_regions"] = [tuple(i) if isinstance(i, list) else i for i in lr]
        fns.append(_FUNCTIONS[name])
        kwargs.append(kw)
    if len(fns) != len(d["postprocessing_kwargs"]):
        raise ValueError("postprocessing_fns and postprocessing_kwargs differ in length")
    return fns, kwargs


# ------------------------------------------------------------------------------------------------
# determine_postprocessing
# ------------------------------------------------------------------------------------------------
def _counts(predictions, references, labels, ignore_label):
    """(cases, L, 4) int64 numpy array of tp, fp, fn, tn per case and label (compute_tp_fp_fn_tn with the ignore mask), from one
    evaluation.confusion_matrix per case over the labels (index i), every other value (L) and the ignored voxels (L + 1).  On the
    device the counts stay there until the single read-back of the stacked tensor."""
    L = len(labels)
    rows = []
    for pred, ref in zip(predictions, references):
        pred, ref = torch.as_tensor(pred), torch.as_tensor(ref)
        if pred.shape != ref.shape:
            raise RuntimeError(f"prediction {tuple(pred.shape)} and reference {tuple(ref.shape)} differ in shape")
        ref = ref.to(pred.device)
        lut = torch.full((256,), L, dtype=torch.long)
        for i, label in enumerate(labels):
            if 0 <= label <= 255:
                lut[label] = i
        lut = lut.to(pred.device)

        def index(x):
            x = x.reshape(-1).long()
            return torch.where((x >= 0) & (x <= 255), lut[x.clamp(0, 255)], torch.full_like(x, L))

        p, t = index(pred), index(ref)
        if ignore_label is not None:
            ignored = ref.reshape(-1).long() == int(ignore_label)
            p = torch.where(ignored, torch.full_like(p, L + 1), p)
            t = torch.where(ignored, torch.full_like(t, L + 1), t)
        cm = evaluation.confusion_matrix(p, t, L + 2)[:L + 1, :L + 1]        # rows: reference, columns: prediction
        tp = cm.diagonal()[:L]
        fp = cm.sum(0)[:L] - tp
        fn = cm.sum(1)[:L] - tp
        tn = cm.sum() - tp - fp - fn
        rows.append(torch.stack([tp, fp, fn, tn], 1))
    return torch.stack(rows).cpu().numpy().astype(np.int64)


def _metrics(counts, labels):
    """compute_metrics_on_folder's 'mean' and 'foreground_mean' (evaluation/evaluate_predictions.py:83-168) from the counts, with its
    arithmetic: numpy int64 counts, Dice = 2 tp / (2 tp + fp + fn) (NaN without tp, fp and fn), np.nanmean over the cases in order,
    np.mean over the labels other than 0; values as Python floats (what its JSON round trip gives)."""
    per_case = []
    for c in range(counts.shape[0]):
        m = {}
        for i, label in enumerate(labels):
            tp, fp, fn, tn = (counts[c, i, k] for k in range(4))
            r = {}
            if tp + fp + fn == 0:
                r["Dice"], r["IoU"] = np.nan, np.nan
            else:
                r["Dice"] = 2 * tp / (2 * tp + fp + fn)
                r["IoU"] = tp / (tp + fp + fn)
            r["FP"], r["TP"], r["FN"], r["TN"], r["n_pred"], r["n_ref"] = fp, tp, fn, tn, fp + tp, fn + tp
            m[label] = r
        per_case.append(m)
    with np.errstate(invalid="ignore"), _quiet():
        means = {label: {k: float(np.nanmean([pc[label][k] for pc in per_case])) for k in METRICS} for label in labels}
        fg = {k: float(np.mean([means[label][k] for label in labels if label != 0])) for k in METRICS}
    return {"foreground_mean": fg, "mean": means}


class _quiet:
    """np.nanmean warns on an all-NaN column and np.mean on an empty one; the reference's values are the same NaNs."""

    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore", RuntimeWarning)

    def __exit__(self, *exc):
        return self._w.__exit__(*exc)


def _is_device(predictions):
    return isinstance(predictions[0], torch.Tensor) and predictions[0].is_cuda


def _run(predictions, groups):
    """keep-largest with the group map {label: group} on every case (K23 on the device, scipy on the host)."""
    return [_keep_largest(p, groups, 0) for p in predictions]


def determine_postprocessing(predictions, references, foreground_labels, ignore_label=None):
    """The reference's determine_postprocessing (:51-246) on lists of label volumes (predictions and references in the same case
    order; CUDA tensors run K23 and the counts on the device).  Returns (pp_fns, pp_fn_kwargs, summary) with summary shaped like the
    reference's postprocessing.json.  Its rules:
      - keep the largest foreground component (all foreground labels united) if the foreground-mean Dice rises and no label's mean
        Dice falls;
      - with more than one foreground label, then for each label in order, on the output of the accepted steps: keep its largest
        component if its mean Dice rises.
    The per-label steps are computed in one labelling that maps each label to itself: removing one label's components changes
    neither another label's voxels nor its counts, so each label's step sees exactly what it sees in the reference's sequence."""
    labels = [int(label) for label in foreground_labels]
    if len(predictions) != len(references) or not predictions:
        raise RuntimeError(f"{len(predictions)} predictions for {len(references)} references")
    if not _is_device(predictions):
        predictions = [p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p)) for p in predictions]
    base = _metrics(_counts(predictions, references, labels, ignore_label), labels)
    pp_fns, pp_fn_kwargs = [], []

    fn = remove_all_but_largest_component_from_segmentation
    kwargs = {"labels_or_regions": list(labels)}
    fg_out = _run(predictions, {label: 1 for label in labels})
    pp = _metrics(_counts(fg_out, references, labels, ignore_label), labels)
    do_this = pp["foreground_mean"]["Dice"] > base["foreground_mean"]["Dice"]
    if do_this:
        for label in labels:
            if pp["mean"][label]["Dice"] < base["mean"][label]["Dice"]:
                do_this = False
                break
    if do_this:
        source, source_metrics = fg_out, pp
        pp_fns.append(fn)
        pp_fn_kwargs.append(kwargs)
    else:
        source, source_metrics = predictions, base

    final = {"foreground_mean": dict(source_metrics["foreground_mean"]), "mean": {k: dict(v) for k, v in source_metrics["mean"].items()}}
    if len(labels) > 1:
        per_label = _metrics(_counts(_run(source, {label: label for label in labels}), references, labels, ignore_label), labels)
        for label in labels:
            if per_label["mean"][label]["Dice"] > final["mean"][label]["Dice"]:
                final["mean"][label] = dict(per_label["mean"][label])
                pp_fns.append(fn)
                pp_fn_kwargs.append({"labels_or_regions": label})
        with _quiet():
            final["foreground_mean"] = {k: float(np.mean([final["mean"][label][k] for label in labels if label != 0]))
                                        for k in METRICS}

    def jsonable(r):
        return {"foreground_mean": r["foreground_mean"], "mean": {str(k): v for k, v in r["mean"].items()}}

    summary = {"input_folder": jsonable(base), "postprocessed": jsonable(final),
               "postprocessing_fns": [f.__name__ for f in pp_fns], "postprocessing_kwargs": [dict(k) for k in pp_fn_kwargs]}
    return pp_fns, pp_fn_kwargs, summary
