"""Sliding-window inference for the 2-D MLAgg-UNet and the 3-D UMambaEnc on MI355X, the device side
of the reference's mlagg/nnunetv2/inference/sliding_window_prediction.py:60-210 and the network restore of
predict_from_raw_data.py:96-99.

Same tiling, Gaussian importance map and mirror test-time augmentation as the reference, but
  * tiles are BATCHED through the network (the reference runs one tile, and one flip, per forward: its
    fixed 256x256 patch leaves the GPU idle between ~30 us kernels),
  * the four mirror variants of a tile batch run as one 4x larger batch,
  * logits and weights accumulate in fp32 on the device (the reference accumulates in half),
  * a training checkpoint (which holds the deep-supervision heads out_1..out_4) loads into the inference
    network built with enable_deep_supervision=False (the reference's strict load fails: SURVEY finding 7d).

3-D tiles on a (c, x, y, z) volume (every 3d_fullres model) take the K20 kernels of csrc/sliding_window.hip on the device: one
gather builds a chunk's network input with every mirror variant, one fold per tile sums the variants, scales by the Gaussian and
accumulates in the reference's order, and one finalize divides, crops and (optionally) takes the argmax -- no flipped copy of an
output, no transient, a contiguous result.  On a CPU device the same order runs as a torch composition (_sliding_window_3d_torch).

A cascaded stage (3d_cascade_fullres) also sees the previous stage's segmentation, one-hot encoded below the image channels
(predict_from_raw_data.py:47-67: `np.vstack((data, seg_onehot))`; nnUNetTrainer.py:1099-1101 in validation).  Both public functions
take it as previous_stage_seg / cascade_labels: on the device the K32 gather writes a chunk's one-hot channels from the label map
itself, so the 4 L x y z bytes of the one-hot volume are never allocated; on the host the stack is built and takes the torch path.
"""
import numpy as np
import torch


def compute_gaussian(tile_size, sigma_scale=1.0 / 8):
    """Reference compute_gaussian (:13-28): a unit impulse at the tile centre blurred with sigma = size / 8
    (scipy's truncated kernel), normalised to max 1, zeros replaced by the smallest non-zero value."""
    from scipy.ndimage import gaussian_filter
    tmp = np.zeros(tile_size)
    tmp[tuple(i // 2 for i in tile_size)] = 1
    g = gaussian_filter(tmp, [i * sigma_scale for i in tile_size], 0, mode="constant", cval=0)
    g = (g / g.max()).astype(np.float16)              # the reference builds it in half; keep its rounding
    g[g == 0] = g[g != 0].min()
    return torch.from_numpy(g.astype(np.float32))


def compute_steps_for_sliding_window(image_size, tile_size, tile_step_size):
    """Reference :31-57."""
    if not 0 < tile_step_size <= 1:
        raise RuntimeError("step_size must be larger than 0 and smaller or equal to 1")
    steps = []
    for size, tile in zip(image_size, tile_size):
        if size < tile:
            raise RuntimeError("image size must be as large or larger than patch_size")
        num = int(np.ceil((size - tile) / (tile * tile_step_size))) + 1
        actual = (size - tile) / (num - 1) if num > 1 else 0.0
        steps.append([int(np.round(actual * i)) for i in range(num)])
    return steps


def _pad_to_tile(image, tile_size):
    """acvl_utils.pad_nd_image semantics: symmetric zero padding of the trailing dims up to the tile size."""
    pads, slicer = [], []
    for s, t in zip(image.shape[-len(tile_size):], tile_size):
        diff = max(t - s, 0)
        pads.append((diff // 2, diff // 2 + diff % 2))
        slicer.append(slice(diff // 2, diff // 2 + s))
    flat = []
    for lo, hi in reversed(pads):
        flat += [lo, hi]
    return torch.nn.functional.pad(image, flat), tuple(slicer)


def load_inference_weights(network, state_dict):
    """Load a TRAINING checkpoint's `network_weights` into a network built without deep supervision."""
    own = network.state_dict()
    kept = {k: v for k, v in state_dict.items() if k in own}
    dropped = [k for k in state_dict if k not in own]
    if any(not k.startswith(("out_1.", "out_2.", "out_3.", "out_4.")) for k in dropped):
        raise RuntimeError(f"unexpected keys in checkpoint: {dropped[:5]}")
    network.load_state_dict(kept, strict=True)
    return dropped


def mirror_variants(mirror_axes):
    """Mirror variants of a 3-D tile as bitmasks of flipped axes (bit a = axis a), in maybe_mirror_and_predict's order
    (reference :87-115): none, 0, 1, 2, (0, 1), (0, 2), (1, 2), (0, 1, 2), restricted to the requested axes."""
    if mirror_axes is None:
        return [0]
    axes = set(int(a) for a in mirror_axes)
    if not axes or min(axes) < 0 or max(axes) > 2:
        raise RuntimeError("mirror_axes does not match the dimension of the input")
    order = [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]
    return [sum(1 << a for a in f) for f in order if set(f) <= axes]


def _flip_dims(mask, first):
    return tuple(first + a for a in range(3) if mask >> a & 1)


def _sliding_window_3d_torch(network, data, gaussian, places, flips, tile_size, tile_batch, num_heads):
    """Torch composition of the 3-D sliding window in the reference's order, on data's device: returns the padded accumulators
    (logits sum (K, X, Y, Z), weight sum (X, Y, Z)) in fp32.  The host path of the 3-D branch, and the A/B side of
    tools/bench_inference_3d.py."""
    tx, ty, tz = tile_size
    logits = torch.zeros((num_heads,) + tuple(data.shape[1:]), dtype=torch.float32, device=data.device)
    weight = torch.zeros(tuple(data.shape[1:]), dtype=torch.float32, device=data.device)
    for i in range(0, len(places), tile_batch):
        chunk = places[i:i + tile_batch]
        tiles = torch.stack([data[:, sx:sx + tx, sy:sy + ty, sz:sz + tz] for sx, sy, sz in chunk])   # (n, c, tx, ty, tz)
        batch = torch.cat([torch.flip(tiles, _flip_dims(m, 2)) if m else tiles for m in flips])
        out = network(batch)
        if isinstance(out, (list, tuple)):
            raise RuntimeError("the inference network must be built with enable_deep_supervision=False")
        n = len(chunk)
        for j, (sx, sy, sz) in enumerate(chunk):
            pred = out[j].clone()
            for v, m in enumerate(flips[1:], start=1):
                pred += torch.flip(out[v * n + j], _flip_dims(m, 1))
            pred = pred / len(flips) * gaussian
            logits[:, sx:sx + tx, sy:sy + ty, sz:sz + tz] += pred
            weight[sx:sx + tx, sy:sy + ty, sz:sz + tz] += gaussian
    return logits, weight


def one_hot(seg, labels, dtype=torch.float32):
    """convert_labelmap_to_one_hot's numpy branch (label_handling.py:266-270): seg (x, y, z) -> (L, x, y, z), row i = seg == labels[i]."""
    return torch.stack([seg == int(l) for l in labels]).to(dtype)


_SEG_DTYPES = (torch.int8, torch.uint8, torch.int16)


def _cascade_inputs(input_image, tile_size, previous_stage_seg, cascade_labels):
    """The checks of the two cascade arguments -> (seg (x, y, z) int8 / uint8 / int16 tensor on its device, [labels]) or (None, None)."""
    if previous_stage_seg is None and cascade_labels is None:
        return None, None
    if previous_stage_seg is None or cascade_labels is None:
        raise RuntimeError("previous_stage_seg and cascade_labels go together: the segmentation of the previous stage and the "
                           "foreground labels it is one-hot encoded with")
    if len(tile_size) != 3:
        raise RuntimeError("a previous-stage segmentation needs a 3-D tile_size: the cascade is 3-D only")
    labels = [int(v) for v in cascade_labels]
    if not labels or any(v < 1 or v > 255 for v in labels):
        raise RuntimeError(f"cascade_labels {labels}: at least one foreground label, each in 1 .. 255")
    seg = torch.as_tensor(previous_stage_seg)
    if seg.dim() == 4 and seg.shape[0] == 1:
        seg = seg[0]
    if input_image.dim() != 4 or tuple(seg.shape) != tuple(input_image.shape[1:]):
        raise RuntimeError(f"previous_stage_seg of shape {tuple(torch.as_tensor(previous_stage_seg).shape)} does not match the image "
                           f"{tuple(input_image.shape)}: (x, y, z) or (1, x, y, z) expected")
    if seg.dtype not in _SEG_DTYPES:
        if seg.is_floating_point() and not bool((seg == seg.round()).all()):
            raise RuntimeError("previous_stage_seg must hold integer values")
        lo, hi = (int(v) for v in torch.aminmax(seg))
        if lo < -32768 or hi > 32767:
            raise RuntimeError(f"previous_stage_seg holds labels {lo} .. {hi}: -32768 .. 32767 expected")
        seg = seg.to(torch.int16)
    return seg, labels


def _predict_3d(network, input_image, num_heads, tile_size, mirror_axes, tile_step_size, use_gaussian, tile_batch, device,
                want_labels, seg=None, labels=None):
    """(c, x, y, z) volume, 3-D tile -> (logits (K, x, y, z), labels (x, y, z) int64 or None), contiguous fp32 on `device`.  seg
    (x, y, z) / labels: the previous stage's segmentation of a cascaded stage, one-hot encoded below the image channels."""
    tile_size = tuple(int(t) for t in tile_size)
    flips = mirror_variants(mirror_axes)
    image = torch.as_tensor(input_image, dtype=torch.float32)
    if seg is not None and device.type != "cuda":
        image = torch.cat((image.to(device), one_hot(seg.to(device), labels)))          # the reference's stack
    data, revert = _pad_to_tile(image, tile_size)
    data = data.to(device).contiguous()
    if seg is not None and device.type == "cuda":
        # zero wherever the image is zero-padded: foreground labels are >= 1, so the padded one-hot channels are 0 as in the reference
        seg = _pad_to_tile(seg, tile_size)[0].to(device).contiguous()
    gaussian = compute_gaussian(tile_size).to(device) if use_gaussian else torch.ones(tile_size, device=device)
    steps = compute_steps_for_sliding_window(tuple(data.shape[1:]), tile_size, tile_step_size)
    places = [(sx, sy, sz) for sx in steps[0] for sy in steps[1] for sz in steps[2]]
    if device.type != "cuda":
        logits, weight = _sliding_window_3d_torch(network, data, gaussian, places, flips, tile_size, tile_batch, num_heads)
        logits /= weight
        logits = logits[(slice(None), *revert)].contiguous()
        return logits, (logits.argmax(0) if want_labels else None)
    from . import ops
    X, Y, Z = data.shape[1:]
    acc = torch.zeros((num_heads, X, Y, Z), dtype=torch.float32, device=device)
    weight = torch.zeros((X, Y, Z), dtype=torch.float32, device=device)
    for i in range(0, len(places), tile_batch):
        chunk = places[i:i + tile_batch]
        if seg is None:
            out = network(ops.sliding_window_gather(data, chunk, flips, tile_size))
        else:
            out = network(ops.sliding_window_gather_onehot(data, seg, labels, chunk, flips, tile_size))
        if isinstance(out, (list, tuple)):
            raise RuntimeError("the inference network must be built with enable_deep_supervision=False")
        if tuple(out.shape) != (len(flips) * len(chunk), num_heads) + tile_size:
            raise RuntimeError(f"network output {tuple(out.shape)}: expected {(len(flips) * len(chunk), num_heads) + tile_size}")
        out = out.contiguous()
        for j, origin in enumerate(chunk):
            ops.sliding_window_fold(out, j, len(chunk), flips, gaussian, origin, acc, weight)
    return ops.sliding_window_finalize(acc, weight, revert, return_labels=want_labels)


def _run_3d(network, input_image, num_heads, tile_size, mirror_axes, tile_step_size, use_gaussian, tile_batch, device,
            want_labels, previous_stage_seg=None, cascade_labels=None):
    """Argument handling of the two public functions for a 3-D tile_size."""
    input_image = torch.as_tensor(input_image)
    if input_image.dim() != 4:
        raise RuntimeError("input_image must be (c, x, y, z) for a 3-D tile_size")
    seg, labels = _cascade_inputs(input_image, tile_size, previous_stage_seg, cascade_labels)
    tile_batch = 1 if tile_batch is None else int(tile_batch)
    if tile_batch < 1:
        raise RuntimeError("tile_batch must be at least 1")
    device = torch.device(device) if device is not None else next(network.parameters()).device
    network.eval()
    return _predict_3d(network, input_image, num_heads, tile_size, mirror_axes, tile_step_size, use_gaussian, tile_batch, device,
                       want_labels, seg, labels)


@torch.no_grad()
def predict_sliding_window_return_logits(network, input_image, num_segmentation_heads, tile_size, mirror_axes=None,
                                         tile_step_size=0.5, use_gaussian=True, tile_batch=None, device=None,
                                         previous_stage_seg=None, cascade_labels=None):
    """input_image (c, D, X, Y) with a 2-D tile_size, or (c, x, y, z) with a 3-D tile_size -> fp32 logits
    (num_segmentation_heads, ...) on `device`.  `network(x)` must return a tensor (deep supervision disabled).  tile_batch: tiles per
    network call (the batch is tile_batch * 2^|mirror_axes|); default 8 for 2-D tiles, 1 for 3-D tiles.
    previous_stage_seg (integer-valued (x, y, z) or (1, x, y, z) tensor or array) with cascade_labels (foreground labels in
    1 .. 255): a cascaded stage, 3-D tiles only -- the result equals the call on vstack((input_image, one_hot(seg, cascade_labels)));
    on a CUDA device the K32 gather builds the one-hot channels of every chunk and that volume is never allocated."""
    if len(tile_size) == 3:
        return _run_3d(network, input_image, num_segmentation_heads, tile_size, mirror_axes, tile_step_size, use_gaussian, tile_batch,
                       device, False, previous_stage_seg, cascade_labels)[0]
    _cascade_inputs(torch.as_tensor(input_image), tile_size, previous_stage_seg, cascade_labels)
    if tile_batch is None:
        tile_batch = 8
    if input_image.dim() != 4 or len(tile_size) != 2:
        raise RuntimeError("input_image must be (c, D, X, Y) and tile_size 2-D")
    device = torch.device(device) if device is not None else next(network.parameters()).device
    network.eval()
    data, revert = _pad_to_tile(torch.as_tensor(input_image, dtype=torch.float32), tuple(tile_size))
    data = data.to(device)
    D, X, Y = data.shape[1:]
    gaussian = compute_gaussian(tuple(tile_size)).to(device) if use_gaussian else torch.ones(tuple(tile_size), device=device)
    logits = torch.zeros((num_segmentation_heads, D, X, Y), dtype=torch.float32, device=device)
    weight = torch.zeros((D, X, Y), dtype=torch.float32, device=device)
    steps = compute_steps_for_sliding_window((X, Y), tile_size, tile_step_size)
    places = [(d, sx, sy) for d in range(D) for sx in steps[0] for sy in steps[1]]
    flips = [()]
    if mirror_axes is not None:
        if max(mirror_axes) > 1:
            raise RuntimeError("mirror_axes does not match the dimension of the input")
        if 0 in mirror_axes:
            flips.append((2,))
        if 1 in mirror_axes:
            flips.append((3,))
        if 0 in mirror_axes and 1 in mirror_axes:
            flips.append((2, 3))
    tx, ty = tile_size
    for i in range(0, len(places), tile_batch):
        chunk = places[i:i + tile_batch]
        tiles = torch.stack([data[:, d, sx:sx + tx, sy:sy + ty] for d, sx, sy in chunk])       # (n, c, tx, ty)
        batch = torch.cat([torch.flip(tiles, f) if f else tiles for f in flips])              # (n * nflip, ...)
        out = network(batch)
        if isinstance(out, (list, tuple)):
            raise RuntimeError("the inference network must be built with enable_deep_supervision=False")
        pred = out[:len(chunk)].clone()
        for j, f in enumerate(flips[1:], start=1):
            pred += torch.flip(out[j * len(chunk):(j + 1) * len(chunk)], f)
        pred = pred / len(flips) * gaussian
        for (d, sx, sy), p in zip(chunk, pred):
            logits[:, d, sx:sx + tx, sy:sy + ty] += p
            weight[d, sx:sx + tx, sy:sy + ty] += gaussian
    logits /= weight
    return logits[(slice(None), slice(None), *revert)]


@torch.no_grad()
def predict_sliding_window_return_segmentation(network, input_image, num_segmentation_heads, tile_size, mirror_axes=None,
                                               tile_step_size=0.5, use_gaussian=True, tile_batch=None, device=None,
                                               previous_stage_seg=None, cascade_labels=None):
    """The int64 label map argmax_k(logits) of predict_sliding_window_return_logits (torch.argmax's first-maximum rule).  3-D tiles
    on the device take it from the finalize kernel, which writes it next to the logits without a second pass over them."""
    if len(tile_size) == 3:
        return _run_3d(network, input_image, num_segmentation_heads, tile_size, mirror_axes, tile_step_size, use_gaussian, tile_batch,
                       device, True, previous_stage_seg, cascade_labels)[1]
    return predict_sliding_window_return_logits(network, input_image, num_segmentation_heads, tile_size, mirror_axes,
                                                tile_step_size, use_gaussian, tile_batch, device, previous_stage_seg,
                                                cascade_labels).argmax(0)
