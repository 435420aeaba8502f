"""Dataset fingerprint: the reference's DatasetFingerprintExtractor
(mlagg/nnunetv2/experiment_planning/dataset_fingerprint/fingerprint_extractor.py:39-163) for in-memory cases.  Its
foreground_intensity_properties_per_channel is the plans entry CTNormalization needs (preprocessing.py, K22); experiment planning
itself (fingerprint -> plans.json) stays the reference's.

Per case: crop to the non-zero box (the image's K22 box kernel and K26's segmentation crop on a CUDA device, numpy otherwise), then
per channel num_samples draws with replacement from the foreground voxels (seg > 0).  The draws are the reference's:
RandomState(seed).choice(foreground_pixels, num_samples, replace=True) is randint(0, n, num_samples) indices into the C-ordered
foreground voxels for the legacy RandomState, so on the device the indices are drawn on the host and K26's ordered rank select
gathers the fp32 intensities; the foreground voxels are never compacted or copied to the host.  The dataset-level statistics run in
numpy on the concatenated float32 samples exactly as run (:146-156) does.  Samples are host numpy arrays on either path."""
import numpy as np
import torch

from . import preprocessing as P


def _on_device(t):
    return isinstance(t, torch.Tensor) and t.is_cuda


def collect_foreground_intensities(segmentation, images, seed=1234, num_samples=10000, max_label=None):
    """collect_foreground_intensities (:39-78): segmentation (1, x, y, z), images (c, x, y, z) -> a list with, per channel, the
    float32 array of num_samples intensities drawn with replacement from the voxels with segmentation > 0 ([] when there are none).
    Device tensors run K26 (max_label: the largest label that can occur, read from the segmentation when None).  The per-case
    statistics dict the reference computes next to the samples is not reproduced: its run() drops it (:139-140)."""
    if segmentation.ndim != 4 or images.ndim != 4 or tuple(segmentation.shape[1:]) != tuple(images.shape[1:]):
        raise RuntimeError(f"collect_foreground_intensities: segmentation {tuple(segmentation.shape)} and images "
                           f"{tuple(images.shape)} must be (1, x, y, z) and (c, x, y, z)")
    num_samples = int(num_samples)
    rs = np.random.RandomState(seed)
    if not (_on_device(segmentation) and _on_device(images)):
        seg = segmentation.cpu().numpy() if isinstance(segmentation, torch.Tensor) else np.asarray(segmentation)
        img = images.cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
        if np.isnan(img).any():
            raise RuntimeError("collect_foreground_intensities: the images contain NaN")
        mask = seg[0] > 0
        out = []
        for c in range(img.shape[0]):
            pixels = img[c][mask]
            out.append(rs.choice(pixels, num_samples, replace=True) if len(pixels) > 0 else [])
        return out
    from . import ops
    seg = P._as_label_tensor(segmentation)[0].contiguous()
    if max_label is None:
        max_label = max(int(seg.max()), 1)
    if bool(torch.isnan(images).any()):
        raise RuntimeError("collect_foreground_intensities: the images contain NaN")
    table = ops.pp_group_table([range(1, int(max_label) + 1)], max_label, seg.device)
    counts = ops.pp_rank_counts(seg, table, 1, max_label)
    n = int(counts[1].cpu()[0])
    if n == 0:
        return [[] for _ in range(images.shape[0])]
    img = images if images.dtype == torch.float32 else images.float()
    picked = []
    for c in range(img.shape[0]):
        ranks = torch.from_numpy(rs.randint(0, n, num_samples).astype(np.int64)).to(seg.device)
        picked.append(ops.pp_rank_select(seg, table, max_label, counts, 0, ranks, image=img[c:c + 1], coords=False)[1][0])
    return list(torch.stack(picked).cpu().numpy())


def analyze_case(image, seg, properties, num_samples=10000, max_label=None):
    """analyze_case (:80-103) on the reader's arrays: image (c, x, y, z), seg (1, x, y, z), properties with 'spacing' -> (shape after
    the non-zero crop, spacing, per-channel foreground samples, relative size after the crop).  Device tensors stay on the device
    (K22's box, K26's segmentation crop and rank select)."""
    shape = tuple(int(s) for s in image.shape[1:])
    if _on_device(image):
        from . import ops
        x = image if image.dtype == torch.float32 else image.float()
        s = P._as_label_tensor(seg, x.device)
        if max_label is None:
            max_label = max(int(s.max()), 1)
        box = ops.pp_nonzero_box(x).cpu().tolist()
        if box[3] < 0:
            raise RuntimeError("analyze_case: the image has no non-zero voxel (the reference fails on it)")
        lo, ext = box[:3], [box[3 + d] - box[d] + 1 for d in range(3)]
        s, _ = ops.pp_seg_crop(s[0], lo, ext, P._filled_mask_device(x, lo, ext), max_label)
        data = x[(slice(None),) + tuple(slice(a, a + e) for a, e in zip(lo, ext))]
        s = s[None]
    else:
        x = image.cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
        s = seg.cpu().numpy() if isinstance(seg, torch.Tensor) else np.asarray(seg)
        data, s, _ = P.crop_to_nonzero(x, np.array(s, dtype=np.int16 if s.dtype.kind in "ub" else s.dtype))
    samples = collect_foreground_intensities(s, data, num_samples=num_samples, max_label=max_label)
    after = tuple(int(v) for v in data.shape[1:])
    return after, properties["spacing"], samples, np.prod(after) / np.prod(shape)


def extract_fingerprint(cases, dataset_json, num_samples=None):
    """DatasetFingerprintExtractor.run (:126-163) without the files: cases is a sequence of (image, seg, properties) ->
    {'spacings', 'shapes_after_crop', 'foreground_intensity_properties_per_channel': {channel: mean, median, std, min, max,
    percentile_99_5, percentile_00_5}, 'median_relative_size_after_cropping'}.  Every case is sampled int(10e7 // n_cases) times per
    channel as in the reference, unless num_samples says otherwise."""
    cases = list(cases)
    if not cases:
        raise RuntimeError("extract_fingerprint: no cases")
    if num_samples is None:
        num_samples = int(10e7 // len(cases))
    flat = [int(v) for lab in dataset_json.get("labels", {}).values() for v in (lab if isinstance(lab, (list, tuple)) else (lab,))]
    max_label = max(flat + [1]) if flat else None
    results = [analyze_case(image, seg, props, num_samples, max_label) for image, seg, props in cases]
    names = dataset_json["channel_names"] if "channel_names" in dataset_json else dataset_json["modality"]
    stats = {}
    for i in range(len(names)):
        v = np.concatenate([r[2][i] for r in results])
        stats[i] = {"mean": float(np.mean(v)), "median": float(np.median(v)), "std": float(np.std(v)), "min": float(np.min(v)),
                    "max": float(np.max(v)), "percentile_99_5": float(np.percentile(v, 99.5)),
                    "percentile_00_5": float(np.percentile(v, 0.5))}
    return {"spacings": [r[1] for r in results], "shapes_after_crop": [r[0] for r in results],
            "foreground_intensity_properties_per_channel": stats,
            "median_relative_size_after_cropping": np.median([r[3] for r in results], 0)}
