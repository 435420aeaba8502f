#!/usr/bin/env python
"""Time of the tail of the training transform chain on the device: K36 (ops.batch_tail, one launch) against the same steps as a torch
composition on the device (dataloading.batch_tail_host: an indexed fill for the mask, where + nearest-exact interpolate per level,
table look-ups for the region planes) -- what the feed would run without the kernel.

Shapes: the headline 2-D batch (10 x 1 x 256 x 256, five halvings, label targets, no mask) and a BraTS-like region batch (2 x 4 x 128^3,
three regions, five levels, all four channels masked).  The two forms are compared first (torch.equal on every output) and the tool
stops unless they agree.  Both are warmed up, then timed in alternating rounds with device events inside one process; the median round
and the spread over the rounds are printed, and the bytes K36 has to move (labels read once per level, planes written, mask zeros not
counted) over its median time.  Prints one JSON line.  Needs the MI355X: there is no CPU fallback for a time."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import dataloading, ops  # noqa: E402

REGIONS = ((1, 2, 3), (2, 3), (3,))
# name -> (B, C, spatial, n_levels | ds_scales, mask channels, regions, seg dtype)
SHAPES = {
    "headline_2d": (10, 1, (256, 256), 5, (), None, torch.float32),
    "brats_regions_3d": (2, 4, (128, 128, 128), [[1.0 / 2 ** i] * 3 for i in range(5)], (0, 1, 2, 3), REGIONS, torch.int16),
}


def inputs(name, dev):
    B, C, spatial, _, _, _, seg_dtype = SHAPES[name]
    g = torch.Generator().manual_seed(31)
    data = torch.rand((B, C) + spatial, generator=g) + 0.5
    seg = torch.randint(0, 4, (B, 1) + spatial, generator=g)
    seg[..., :spatial[-1] // 8] = -1                               # the padded border of a patch that reaches past its case
    return data.to(dev), seg.to(seg_dtype).to(dev)


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_tail: no GPU; a time is only ever measured on the MI355X")
    dev = torch.device("cuda:0")
    result = {"iters": a.iters, "rounds": a.rounds}
    for name, (B, C, spatial, levels, mask, regions, seg_dtype) in SHAPES.items():
        data, seg = inputs(name, dev)
        sizes = dataloading.level_sizes(spatial, levels) if isinstance(levels, int) else dataloading.level_sizes(spatial, ds_scales=levels)
        member = None if regions is None else ops.region_member_table(regions, dev)
        n_regions = 0 if regions is None else len(regions)
        forms = {"k36": lambda d=data: ops.batch_tail(d, seg, sizes, mask, regions),
                 "composed": lambda d=data: dataloading.batch_tail_host(d, seg, sizes, list(mask), member, n_regions)}
        outs = {form: fn(data.clone()) for form, fn in forms.items()}
        same = torch.equal(outs["k36"][0], outs["composed"][0]) and all(torch.equal(x, y) for x, y in zip(outs["k36"][1], outs["composed"][1]))
        if not same:
            raise SystemExit(f"bench_batch_tail: {name}: the two forms disagree; no time is reported for different results")
        for fn in forms.values():                                  # warm-up of every shape in the timed window
            timed(fn, 5)
        times = {form: [] for form in forms}
        for _ in range(a.rounds):                                  # alternating: both forms see the same machine state
            for form, fn in forms.items():
                times[form].append(timed(fn, a.iters))
        voxels = [B * int(torch.tensor(s).prod()) for s in sizes]
        nbytes = sum(v * (seg.element_size() + 4 * max(n_regions, 1)) for v in voxels)
        med = statistics.median(times["k36"])
        result[name] = {"shape": {"B": B, "C": C, "spatial": list(spatial), "levels": len(sizes), "regions": n_regions, "masked": len(mask),
                                  "seg": str(seg_dtype).replace("torch.", "")},
                        **{f"{form}_ms_median": round(statistics.median(t), 4) for form, t in times.items()},
                        **{f"{form}_ms_min_max": [round(min(t), 4), round(max(t), 4)] for form, t in times.items()},
                        "k36_bytes": nbytes, "k36_gb_per_s": round(nbytes / med / 1e6, 1)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
