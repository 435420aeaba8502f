"""Shared inputs of the K36 tests (tests/test_batch_tail_cpu.py, tests/test_batch_tail_gpu.py): the four geometries, the label draws,
the region sets, and a direct numpy restatement of the four reference transforms K36 replaces."""
import numpy as np
import torch

# name -> (B, C, spatial shape, n_levels of 2-D halvings | per-axis deep-supervision scales)
GEOMETRIES = {
    "2d_five_halvings": (3, 2, (24, 40), 5),                            # down to a 1 x 2 level; every row length a multiple of 4 or below 4
    "2d_odd_rows": (2, 3, (23, 37), 3),                                 # odd rows: scalar tails, rows that start misaligned
    "3d_scales": (2, 2, (8, 16, 24), [[1, 1, 1], [.5, .5, .5], [.25, .25, .25], [.25, .125, .125]]),
    "3d_two_levels": (2, 1, (6, 10, 14), [[1, 1, 1], [.5, .5, .5]]),
}
REGIONS_3 = [(1, 2, 3), (2, 3), (3,)]
REGIONS_8 = [(1,), (2,), (3,), (5,), (255,), (1, 2, 3), (2, 3, 5, 255), (0, 1)]
IGNORE_8 = 4
# mode -> (regions, ignore_label)
MODES = {"labels": (None, None), "regions3": (REGIONS_3, None), "regions8_ignore": (REGIONS_8, IGNORE_8)}
LABEL_VALUES = (-1, 0, 1, 2, 3, 4, 5, 255, 300)                        # the padding, the table's ends, a value above the table


def level_sizes(name):
    from mlagg_unet_amd import dataloading
    _, _, spatial, levels = GEOMETRIES[name]
    return dataloading.level_sizes(spatial, levels) if isinstance(levels, int) else dataloading.level_sizes(spatial, ds_scales=levels)


def mask_choices(C):
    """empty, a strict subset, all channels (fewer when there is one channel)."""
    return sorted({(), tuple(range(C))[1:], tuple(range(C))})


def batch(name, seg_dtype, seg_channels, seed=0):
    """(data (B, C, *S) fp32 without zeros, seg (B, Sc, *S)): every LABEL_VALUES entry occurs; runs of -1 so that whole quads, partial
    quads and single voxels are masked."""
    B, C, spatial, _ = GEOMETRIES[name]
    rng = np.random.RandomState(seed + 17 * len(name))
    data = rng.uniform(0.5, 2.0, (B, C) + spatial).astype(np.float32)
    seg = np.asarray(LABEL_VALUES)[rng.randint(0, len(LABEL_VALUES), (B, seg_channels) + spatial)]
    seg[:, 0, ..., :7] = -1                                                # a run that ends inside a quad
    seg[:, 0, ..., 9] = -1
    seg[0, 0].reshape(-1)[:len(LABEL_VALUES)] = LABEL_VALUES
    return torch.from_numpy(data), torch.from_numpy(seg).to(seg_dtype)


def reference_transforms(data, seg, scales, mask_channels, regions, ignore_label):
    """numpy: MaskTransform (masking.py:18-22), RemoveLabelTransform(-1, 0), ConvertSegmentationToRegionsTransform
    (region_based_training.py:23-38, the ignore label appended as nnUNetTrainer.py:722-726 does) and DownsampleSegForDSTransform2 with
    order 0, i.e. skimage's nearest resize: source index floor((i + 0.5) n / m) per axis, computed in integers.  In the reference's
    order: regions first, then the levels."""
    data, seg = data.copy(), seg.astype(np.float32)
    outside = seg[:, 0] < 0
    for c in mask_channels:
        data[:, c][outside] = 0
    seg[seg == -1] = 0
    target = seg[:, :1]
    if regions is not None:
        todo = list(regions) + ([ignore_label] if ignore_label is not None else [])
        out = np.zeros((seg.shape[0], len(todo)) + seg.shape[2:], dtype=seg.dtype)
        for b in range(seg.shape[0]):
            for r, labels in enumerate(todo):
                for value in (labels if isinstance(labels, (list, tuple)) else (labels,)):
                    out[b, r][seg[b, 0] == value] = 1
        target = out
    levels = []
    for s in scales:
        level = target
        for axis, f in enumerate(s):
            n = target.shape[2 + axis]
            m = int(np.round(n * f))
            level = np.take(level, [((2 * i + 1) * n) // (2 * m) for i in range(m)], axis=2 + axis)
        levels.append(level)
    return data, levels
