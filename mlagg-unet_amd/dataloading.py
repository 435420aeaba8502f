"""Real-data input path of the 2-D train step: the reference's nnUNetDataLoader2D
(training/dataloading/data_loader_2d.py:7-86 on base_data_loader.py:10-139 and nnunet_dataset.py:80-111) re-shaped
for feeding an MI355X, not re-invented: same case folder (<case>.npz or unpacked <case>.npy / <case>_seg.npy, <case>.pkl
with `class_locations`), same sampling decisions in the same order of random draws -- so a seeded run gives the reference's
batches bit for bit -- but

  * only the selected 2-D slice of a case is read (memory-mapped .npy) and the crop is written straight into PINNED host
    batch buffers (the reference loads the case, slices, crops, np.pads into fresh arrays and later collates / converts);
  * `to_device` moves a batch with non-blocking copies on a side HIP stream and builds the five deep-supervision targets
    ON the device (label -1 -> 0 as RemoveLabelTransform, nearest down-sampling as DownsampleSegForDSTransform2), i.e. the
    (data, [target_0..target_4]) pair nnUNetTrainer.train_step consumes (nnUNetTrainer.py:833-845);
  * `PrefetchLoader` overlaps batch assembly (worker threads, one RandomState each) and the H2D copy with the train step.

`DataLoader3D` is the reference's nnUNetDataLoader3D (training/dataloading/data_loader_3d.py:7-52 on get_bbox,
base_data_loader.py:63-139) on the same case folder and pinned buffers; `to_device` / `PrefetchLoader` take the trainer's
per-axis deep-supervision scales for its batches (`ds_scales`).  The augmentation transforms live in augmentation.py (2-D)
and augmentation3d.py (3-D).

A cascade's second stage (3d_cascade_fullres) gives `Dataset` the folder with the previous stage's predictions
(nnunet_dataset.py:48-49, 104-109): every case then has a second seg channel, which the loaders crop with the same box and
pad with -1, and which augmentation3d turns into one-hot input channels on the device.

With `mask_channels` / `regions` / `ignore_label` the feed ends in K36 (ops.batch_tail): MaskTransform, the region planes and every
deep-supervision level in one launch; `DeviceBatchIterator` puts the protocol of nnU-Net's generators on a `PrefetchLoader`
(nnunet_plugin's ``data_pipeline="device"``)."""
import contextlib
import os
import pickle
import queue
import threading

import numpy as np
import torch


class _SegChannels:
    """np.vstack((seg, seg_prev[None])) (nnunet_dataset.py:109) for arrays that are only read through crops: the index is
    applied to both parts, so a memory-mapped case is not copied as a whole."""

    def __init__(self, seg, prev):
        if tuple(prev.shape) != tuple(seg.shape[1:]):
            raise RuntimeError(f"segmentation of the previous stage {tuple(prev.shape)} does not match the case {tuple(seg.shape)}")
        self.parts = (seg, prev[None])
        self.shape, self.dtype, self.ndim = (seg.shape[0] + 1, *seg.shape[1:]), seg.dtype, seg.ndim

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, idx):
        idx = idx if isinstance(idx, tuple) else (idx,)
        return np.concatenate([p[(slice(None),) + idx[1:]] for p in self.parts], 0)[idx[0]]

    def __array__(self, dtype=None, copy=None):
        out = np.concatenate(self.parts, 0)
        return out if dtype is None else out.astype(dtype)


class Dataset:
    """Case folder index (reference nnUNetDataset).  Properties (.pkl) are read once and cached: they hold the sampled
    foreground locations used for every oversampled patch.  `folder_with_segs_from_previous_stage`: the cascade's
    predicted_next_stage/<configuration> folder; its <case>.npz['seg'] (or unpacked <case>.npy) becomes a second seg channel."""

    def __init__(self, folder, case_identifiers=None, folder_with_segs_from_previous_stage=None):
        self.prev_folder = folder_with_segs_from_previous_stage
        ids = case_identifiers if case_identifiers is not None else \
            [i[:-4] for i in os.listdir(folder) if i.endswith("npz") and i.find("segFromPrevStage") == -1]
        self.folder, self.ids = folder, sorted(ids)
        self._props, self._open, self._prev = {}, {}, {}
        if not self.ids:
            raise RuntimeError(f"no <case>.npz in {folder}")

    def keys(self):
        return list(self.ids)

    def __len__(self):
        return len(self.ids)

    def properties(self, key):
        if key not in self._props:
            with open(os.path.join(self.folder, key + ".pkl"), "rb") as fh:
                self._props[key] = pickle.load(fh)
        return self._props[key]

    def arrays(self, key):
        """(data (C, D, H, W), seg (1, D, H, W)): memory maps of the unpacked .npy files when they exist (kept open),
        else the decompressed .npz members.  With a previous-stage folder seg is (2, D, H, W) (nnunet_dataset.py:104-109)."""
        if key not in self._open:
            base = os.path.join(self.folder, key)
            if os.path.isfile(base + ".npy") and os.path.isfile(base + "_seg.npy"):
                self._open[key] = (np.load(base + ".npy", "r"), np.load(base + "_seg.npy", "r"))
            else:
                z = np.load(base + ".npz")
                return z["data"], self._with_previous_stage(key, z["seg"])    # not cached: a decompressed case can be large
        data, seg = self._open[key]
        return data, self._with_previous_stage(key, seg)

    def _with_previous_stage(self, key, seg):
        if self.prev_folder is None:
            return seg
        if key not in self._prev:
            base = os.path.join(self.prev_folder, key)
            if not os.path.isfile(base + ".npy"):
                return _SegChannels(seg, np.load(base + ".npz")["seg"])
            self._prev[key] = np.load(base + ".npy", "r")
        return _SegChannels(seg, self._prev[key])


class DataLoader2D:
    """generate_train_batch() == the reference's, draw for draw.  `rng`: numpy's global state by default (what the
    reference uses); a RandomState for worker threads."""

    def __init__(self, dataset, batch_size, patch_size, final_patch_size, all_labels, oversample_foreground_percent=0.0,
                 rng=None, pin_memory=None, has_ignore=False):
        self.has_ignore = bool(has_ignore)             # label_manager.has_ignore_label (base_data_loader.py:42)
        self.ds, self.batch_size = dataset, int(batch_size)
        self.indices = dataset.keys()
        self.patch_size = tuple(int(v) for v in patch_size)
        self.need_to_pad = (np.array(patch_size) - np.array(final_patch_size)).astype(int)
        self.oversample = float(oversample_foreground_percent)
        self.annotated_classes_key = tuple(all_labels)
        flat = [int(v) for lab in all_labels for v in (lab if isinstance(lab, (tuple, list)) else (lab,))]
        # a larger value in a case file is refused (generate_train_batch); nnU-Net's ignore label is the next integer
        self.max_label = (max(flat) + int(self.has_ignore)) if flat else None
        self.rng = np.random if rng is None else rng
        data, seg = dataset.arrays(self.indices[0])
        self.channels, self.seg_channels = data.shape[0], seg.shape[0]
        self.pin = torch.cuda.is_available() if pin_memory is None else bool(pin_memory)

    def get_do_oversample(self, j):                    # base_data_loader.py:45-49
        return not j < round(self.batch_size * (1 - self.oversample))

    def _bbox(self, shape, force_fg, locs):            # base_data_loader.py:63-139; `locs`: voxels of the chosen class / region
        # on the chosen slice (with an ignore label and no forced foreground: of ALL annotated labels, :91-97)
        need = self.need_to_pad.copy()
        for d in range(2):
            if need[d] + shape[d] < self.patch_size[d]:
                need[d] = self.patch_size[d] - shape[d]
        lbs = [-need[i] // 2 for i in range(2)]
        ubs = [shape[i] + need[i] // 2 + need[i] % 2 - self.patch_size[i] for i in range(2)]
        if (force_fg or self.has_ignore) and locs is not None and len(locs) > 0:
            v = locs[self.rng.choice(len(locs))]
            return [max(lbs[i], int(v[i + 1]) - self.patch_size[i] // 2) for i in range(2)]
        return [self.rng.randint(lbs[i], ubs[i] + 1) for i in range(2)]

    def _buffers(self):
        shp_d = (self.batch_size, self.channels, *self.patch_size)
        shp_s = (self.batch_size, self.seg_channels, *self.patch_size)
        d = torch.zeros(shp_d, dtype=torch.float32, pin_memory=self.pin)
        s = torch.full(shp_s, -1, dtype=torch.int16, pin_memory=self.pin)
        return d, s

    def generate_train_batch(self):
        keys = self.rng.choice(self.indices, self.batch_size, replace=True, p=None)
        data_t, seg_t = self._buffers()
        data_all, seg_all = data_t.numpy(), seg_t.numpy()
        for j, key in enumerate(keys):
            force_fg = self.get_do_oversample(j)
            data, seg = self.ds.arrays(key)
            sel = locs_all = None
            if force_fg:
                cl = self.ds.properties(key)["class_locations"]
                eligible = [i for i in cl.keys() if len(cl[i]) > 0]
                # data_loader_2d.py:29-35: the all-annotated-labels key competes only when nothing else is present
                if len(eligible) > 1 and self.annotated_classes_key in [i for i in eligible if isinstance(i, tuple)]:
                    eligible.remove(self.annotated_classes_key)
                if eligible:
                    sel = eligible[self.rng.choice(len(eligible))]
                    locs_all = cl[sel]
            elif self.has_ignore:                          # data_loader_2d.py:21-23
                sel = self.annotated_classes_key
                locs_all = self.ds.properties(key)["class_locations"][sel]
            sl = self.rng.choice(locs_all[:, 1]) if sel is not None else self.rng.choice(len(data[0]))
            if sel is not None:
                # data_loader_2d.py:55-57: the locations of that class on that slice; get_bbox is told the class
                # (overwrite_class), so it draws a voxel but no class
                locs = locs_all[locs_all[:, 1] == sl][:, (0, 2, 3)]
            else:
                locs = None
            shape = data.shape[2:]
            lb = self._bbox(shape, force_fg if sel is not None else None, locs)
            ub = [lb[i] + self.patch_size[i] for i in range(2)]
            v0 = [max(0, lb[i]) for i in range(2)]
            v1 = [min(shape[i], ub[i]) for i in range(2)]
            o0 = [v0[i] - lb[i] for i in range(2)]
            h, w = v1[0] - v0[0], v1[1] - v0[1]
            data_all[j, :, o0[0]:o0[0] + h, o0[1]:o0[1] + w] = data[:, sl, v0[0]:v1[0], v0[1]:v1[1]]
            seg_all[j, :, o0[0]:o0[0] + h, o0[1]:o0[1] + w] = seg[:, sl, v0[0]:v1[0], v0[1]:v1[1]]
        self._check_labels(seg_all, keys)
        return {"data": data_t, "seg": seg_t, "keys": keys}

    def _check_labels(self, seg_all, keys):
        seg_all = seg_all[:, 0]                           # the target; a cascade's second channel holds the previous stage's labels
        if self.max_label is not None and int(seg_all.max()) > self.max_label:
            # torch's nll_loss (the reference's CE) fails on a label >= C; the fused loss kernel would quietly count such a
            # pixel as "no class hit", so a corrupt case is stopped here, on the host, where the check costs nothing
            raise RuntimeError(f"segmentation label {int(seg_all.max())} > {self.max_label} (largest label of the dataset) "
                               f"in cases {sorted(set(map(str, keys)))}")

    def clone(self, rng):
        """The same loader with its own random state (one per PrefetchLoader worker)."""
        return type(self)(self.ds, self.batch_size, self.patch_size, tuple(np.array(self.patch_size) - self.need_to_pad),
                          self.annotated_classes_key, self.oversample, rng=rng, pin_memory=self.pin, has_ignore=self.has_ignore)


class DataLoader3D(DataLoader2D):
    """nnUNetDataLoader3D.generate_train_batch, draw for draw: the keys, then per sample get_bbox's class choice (no
    overwrite_class, unlike the 2-D loader) and its voxel choice or one randint per axis.  The 3-D crop of each case goes
    straight into the pinned batch buffers (data padded with 0, seg int16 padded with -1)."""

    def _bbox(self, shape, force_fg, class_locations):      # base_data_loader.py:63-139 for dim 3
        dim = len(shape)
        need = self.need_to_pad.copy()
        for d in range(dim):
            if need[d] + shape[d] < self.patch_size[d]:
                need[d] = self.patch_size[d] - shape[d]
        lbs = [-need[i] // 2 for i in range(dim)]
        ubs = [shape[i] + need[i] // 2 + need[i] % 2 - self.patch_size[i] for i in range(dim)]
        if not force_fg and not self.has_ignore:
            return [self.rng.randint(lbs[i], ubs[i] + 1) for i in range(dim)]
        if not force_fg:                                     # ignore label: a patch around an ANNOTATED voxel (:91-97)
            sel = self.annotated_classes_key
            if len(class_locations[sel]) == 0:
                sel = None
        else:
            eligible = [i for i in class_locations.keys() if len(class_locations[i]) > 0]
            # the all-annotated-labels key competes only when nothing else is present (:112-115)
            if len(eligible) > 1 and self.annotated_classes_key in [i for i in eligible if isinstance(i, tuple)]:
                eligible.remove(self.annotated_classes_key)
            sel = eligible[self.rng.choice(len(eligible))] if eligible else None
        vox = class_locations[sel] if sel is not None else None
        if vox is not None and len(vox) > 0:
            v = vox[self.rng.choice(len(vox))]
            return [max(lbs[i], int(v[i + 1]) - self.patch_size[i] // 2) for i in range(dim)]
        return [self.rng.randint(lbs[i], ubs[i] + 1) for i in range(dim)]

    def generate_train_batch(self):
        keys = self.rng.choice(self.indices, self.batch_size, replace=True, p=None)
        data_t, seg_t = self._buffers()
        data_all, seg_all = data_t.numpy(), seg_t.numpy()
        for j, key in enumerate(keys):
            force_fg = self.get_do_oversample(j)
            data, seg = self.ds.arrays(key)
            shape = data.shape[1:]
            cl = self.ds.properties(key)["class_locations"] if (force_fg or self.has_ignore) else None
            lb = self._bbox(shape, force_fg, cl)
            v0 = [max(0, lb[i]) for i in range(3)]
            v1 = [min(shape[i], lb[i] + self.patch_size[i]) for i in range(3)]
            o = [v0[i] - lb[i] for i in range(3)]
            dst = (slice(None),) + tuple(slice(o[i], o[i] + v1[i] - v0[i]) for i in range(3))
            src = (slice(None),) + tuple(slice(v0[i], v1[i]) for i in range(3))
            data_all[j][dst] = data[src]
            seg_all[j][dst] = seg[src]
        self._check_labels(seg_all, keys)
        return {"data": data_t, "seg": seg_t, "keys": keys}


_NEAREST = {}


def nearest_index(n, m):
    """The source index along an axis of n voxels for each of the m voxels that ``F.interpolate(..., size=m, mode="nearest-exact")``
    makes of it, as m int32 (host): THE index rule of the deep-supervision targets.  It is read off torch itself (an arange is
    interpolated once per (n, m)), not restated, so whatever gathers with it (K36, ops.batch_tail) is `targets_from_seg` to the bit."""
    key = (int(n), int(m))
    if key not in _NEAREST:
        if key[0] < 1 or key[1] < 1 or key[0] >= 1 << 24:
            raise RuntimeError(f"nearest_index: an axis of {key[0]} voxels resized to {key[1]}")
        ramp = torch.arange(key[0], dtype=torch.float32).view(1, 1, -1)          # exact in fp32 below 2^24
        _NEAREST[key] = torch.nn.functional.interpolate(ramp, size=key[1], mode="nearest-exact").view(-1).to(torch.int32)
    return _NEAREST[key]


def level_sizes(spatial, n_levels=5, ds_scales=None):
    """The spatial shapes of the deep-supervision targets of a `spatial` map, as `targets_from_seg` makes them: n_levels halvings of
    the two axes of a 2-D map, or round(shape * scale) per level of `ds_scales`."""
    spatial = tuple(int(v) for v in spatial)
    if ds_scales is None:
        if n_levels > 1 and len(spatial) != 2:
            raise RuntimeError(f"level_sizes: {n_levels} halvings are for 2-D maps, got {spatial}: give ds_scales")
        return [spatial] + [tuple(v >> s for v in spatial) for s in range(1, n_levels)]
    sizes = []
    for sc in ds_scales:
        if len(sc) != len(spatial):
            raise RuntimeError(f"deep-supervision scale {list(sc)} for a {len(spatial)}-D segmentation")
        sizes.append(tuple(int(v) for v in np.round(np.array(spatial, dtype=float) * np.array(sc, dtype=float))))
    return sizes


def targets_from_seg(seg, n_levels=5, ds_scales=None):
    """RemoveLabelTransform(-1, 0) (B:701) + DownsampleSegForDSTransform2, order 0 (B:730): the deep-supervision targets.
    2-D: n_levels halvings of both axes.  `ds_scales` (the trainer's _get_deep_supervision_scales(), one per-axis scale
    list per level, e.g. [1, .5, .5]): level shape round(shape * scale), nearest-exact; an all-ones scale is the map itself."""
    seg = torch.where(seg < 0, torch.zeros_like(seg), seg)
    return [seg if size == tuple(seg.shape[2:]) else torch.nn.functional.interpolate(seg, size=size, mode="nearest-exact")
            for size in level_sizes(seg.shape[2:], n_levels, ds_scales)]


def batch_tail_host(data, seg, sizes, mask_channels=(), member=None, n_regions=0, ignore_label=None, tables=None):
    """What K36 computes (ops.batch_tail, which checks the arguments), as a torch composition on whatever device the tensors live on:
    the reference's MaskTransform (masking.py:18-22) as an indexed fill of `data`, then per level of `sizes` the map of
    `targets_from_seg` (the same where + nearest-exact interpolate; with `tables`, a gather by the given per-axis indices) and, with
    the `member` table of ops.region_member_table, the planes of ConvertSegmentationToRegionsTransform
    (region_based_training.py:23-38) by table look-up, the ignore label as one more region (B:722-726)."""
    raw = seg[:, :1]
    if len(mask_channels):
        outside = (raw[:, 0] < 0).unsqueeze(1).expand(-1, len(mask_channels), *raw.shape[2:])
        data[:, list(mask_channels)] = data[:, list(mask_channels)].masked_fill(outside, 0.0)
    labels = raw.float()
    labels = torch.where(labels < 0, torch.zeros_like(labels), labels)
    targets = []
    for lvl, size in enumerate(sizes):
        level = labels
        if tables is not None and any(t is not None for t in tables[lvl]):
            for axis, tab in enumerate(tables[lvl]):
                if tab is not None:
                    level = level.index_select(2 + axis, tab.long().clamp(0, labels.shape[2 + axis] - 1))
        elif tuple(size) != tuple(labels.shape[2:]):
            level = torch.nn.functional.interpolate(labels, size=tuple(size), mode="nearest-exact")
        if member is not None:
            whole = (level >= 0) & (level < 256) & (level == level.floor())        # np.isin: other values are in no region
            bits = torch.where(whole, member.long()[torch.where(whole, level, torch.zeros_like(level)).long()] & 0xFFFFFFFF,
                               torch.zeros_like(level, dtype=torch.int64))
            planes = [(bits >> r) & 1 for r in range(n_regions)]
            if ignore_label is not None:
                planes.append(level == float(ignore_label))
            level = torch.cat(planes, 1).float()
        targets.append(level.contiguous())
    return data, targets


def _tail_wanted(mask_channels, regions, ignore_label):
    return mask_channels is not None or regions is not None or ignore_label is not None


def to_device(batch, device, n_levels=5, stream=None, augmenter=None, ds_scales=None, cascade_labels=None, mask_channels=None,
              regions=None, ignore_label=None):
    """Host batch -> (data (B, C, *spatial) fp32, [target_s (B, 1, *spatial_s) fp32 labels]) on `device`; with an
    `augmenter` (augmentation.GpuAugmenter / augmentation3d.GpuAugmenter3D) the training transforms run on the device in
    between.  2-D: n_levels halvings; `ds_scales`: per-axis scales (targets_from_seg), for 3-D batches.  A cascade batch
    (two seg channels) goes through an augmenter built with `cascade_labels`, or, without an augmenter (validation), through
    augmentation3d.move_seg_as_one_hot with the `cascade_labels` given here: data gains one input channel per label.
    With any of `mask_channels` (indices of the data channels of ``use_mask_for_norm``), `regions` (the label manager's
    ``foreground_regions``) and `ignore_label` given, the rest of the reference's chain (B:697-731) runs as ONE kernel (K36,
    ops.batch_tail) instead of `targets_from_seg`: the mask on `data` (training only: the validation chain has no MaskTransform, so
    without an augmenter no mask is applied), and targets that are region planes (B, R (+ 1 with an ignore label), *spatial_s) when
    there are regions."""
    device = torch.device(device)
    ctx = torch.cuda.stream(stream) if stream is not None else _Null()
    with ctx:
        data = batch["data"].to(device, non_blocking=True)
        seg = batch["seg"].to(device, non_blocking=True)
        # the 3-D augmenter reads the loader's int16 labels as they are (K25); everything else takes fp32 label maps
        seg = seg if getattr(augmenter, "takes_int16_seg", False) else seg.float()
        if augmenter is not None:
            data, seg = augmenter(data, seg)
        elif seg.shape[1] == 2:
            if cascade_labels is None:
                raise RuntimeError("to_device: a cascade batch (two seg channels) needs an augmenter or cascade_labels")
            from .augmentation3d import move_seg_as_one_hot
            data, seg = move_seg_as_one_hot(data, seg, cascade_labels)
        if _tail_wanted(mask_channels, regions, ignore_label):
            from . import ops
            masked = tuple(mask_channels or ()) if augmenter is not None else ()
            if seg.dtype not in (torch.float32, torch.int16):
                seg = seg.float()
            data, targets = ops.batch_tail(data.contiguous(), seg.contiguous(), level_sizes(seg.shape[2:], n_levels, ds_scales),
                                           masked, regions, ignore_label)
        else:
            targets = targets_from_seg(seg.float(), n_levels, ds_scales)
    return data, targets


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


class PrefetchLoader:
    """Background batch assembly + H2D copy.  Each worker thread owns a clone of the loader with its own RandomState
    (numpy's slicing / copies release the GIL); batches arrive on the device through a side stream, and `next()` makes the
    caller's current stream wait for that copy only."""

    def __init__(self, loader, device, num_workers=4, depth=6, seed=1234, n_levels=5, augmenter=None, ds_scales=None,
                 cascade_labels=None, mask_channels=None, regions=None, ignore_label=None):
        self.cascade_labels = cascade_labels
        self.tail = dict(mask_channels=mask_channels, regions=regions, ignore_label=ignore_label)      # K36: see to_device
        self._gate, self._busy, self._paused = threading.Condition(), 0, False                           # see quiesced()
        self.device = torch.device(device)
        self.q = queue.Queue(maxsize=depth)
        self.stop = threading.Event()
        self.n_levels = n_levels
        self.ds_scales = None if ds_scales is None else [list(s) for s in ds_scales]
        self.copy_stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None
        self.workers = []
        for i in range(num_workers):
            clone = loader.clone(np.random.RandomState(seed + i))
            aug = augmenter.clone(seed + 7919 * (i + 1)) if augmenter is not None else None
            t = threading.Thread(target=self._work, args=(clone, aug), daemon=True)
            t.start()
            self.workers.append(t)

    def _work(self, loader, augmenter=None):
        while not self.stop.is_set():
            with self._gate:
                while self._paused and not self.stop.is_set():
                    self._gate.wait(0.2)
                self._busy += 1
            try:
                b = loader.generate_train_batch()
                if self.copy_stream is not None:
                    data, targets = to_device(b, self.device, self.n_levels, self.copy_stream, augmenter, self.ds_scales,
                                              self.cascade_labels, **self.tail)
                    ev = torch.cuda.Event()
                    ev.record(self.copy_stream)
                else:
                    data, targets = to_device(b, self.device, self.n_levels, None, augmenter, self.ds_scales, self.cascade_labels,
                                              **self.tail)
                    ev = None
                item = (data, targets, ev, b)                 # keep the pinned host batch alive until consumed
            except BaseException as e:                        # missing .pkl, bad .npz, out of memory on the copy stream ...
                item = e                                      # handed to the consumer: next() re-raises it
                self.stop.set()
            finally:
                with self._gate:
                    self._busy -= 1
                    self._gate.notify_all()
            while True:
                try:
                    self.q.put(item, timeout=0.2)
                    break
                except queue.Full:
                    if self.stop.is_set() and not isinstance(item, BaseException):
                        break

    @contextlib.contextmanager
    def quiesced(self):
        """Inside the block no worker assembles a batch or talks to the device (batches already queued stay available): for the
        moments in which the consumer captures a hipGraph, when allocations, synchronous copies and event queries of OTHER threads
        are errors in the runtime's default capture mode.  Waits for the batches in assembly to finish."""
        with self._gate:
            self._paused = True
            while self._busy:
                self._gate.wait(0.2)
        try:
            yield self
        finally:
            with self._gate:
                self._paused = False
                self._gate.notify_all()

    def next(self):
        while True:
            try:
                item = self.q.get(timeout=1.0)
                break
            except queue.Empty:
                if not any(t.is_alive() for t in self.workers):
                    raise RuntimeError("PrefetchLoader: every worker thread has exited and no batch is queued")
        if isinstance(item, BaseException):
            self.q.put(item)                                  # the next caller sees it too
            raise RuntimeError(f"PrefetchLoader worker failed: {type(item).__name__}: {item}") from item
        data, targets, ev, _ = item
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
            for t in [data] + targets:
                t.record_stream(torch.cuda.current_stream(self.device))
        return data, targets

    def close(self):
        self.stop.set()
        while not self.q.empty():
            try:
                self.q.get_nowait()
            except queue.Empty:
                break
        for t in self.workers:
            t.join(timeout=2)


class DeviceBatchIterator:
    """A `PrefetchLoader` behind the protocol ``nnUNetTrainer.run_training`` drives its data generators with (the reference's
    NonDetMultiThreadedAugmenter / SingleThreadedAugmenter, nnUNetTrainer.py:600-610): ``next(it)`` is
    ``{"data": tensor, "target": list of tensors}`` -- on the device already, so the trainer's ``.to(device)`` is a no-op -- and
    `target` is a single tensor when the loader has no `ds_scales`, as NumpyToTensor delivers it without deep supervision.  Infinite,
    like the reference's generators: the trainer counts the iterations of an epoch itself.  ``_finish()`` (the name the reference
    calls on its generators when training ends) stops and joins the workers."""

    def __init__(self, prefetch_loader):
        self.loader = prefetch_loader

    def __iter__(self):
        return self

    def __next__(self):
        data, targets = self.loader.next()
        return {"data": data, "target": list(targets) if self.loader.ds_scales is not None else targets[0]}

    def quiesced(self):
        return self.loader.quiesced()

    def _finish(self, timeout=None):
        self.loader.close()
