#!/usr/bin/env python
"""Time of the deep-supervision Dice + BCE loss of a region-based dataset (forward + backward to the logit maps): the fused loss (K29,
trainer.region_deep_supervision_loss) against trainer.dc_and_bce_loss composed level by level on the device -- the arithmetic that the
reference's DeepSupervisionWrapper(DC_and_BCE_loss) runs for these datasets.

Shape: BraTS-like, batch 2, 3 sigmoid heads, a 128^3 patch with five deep-supervision levels, region planes as targets (what the plugin
receives), without and with an ignore plane.  Both forms are warmed up, then timed in alternating rounds with device events inside one
process; the median round and the spread over the rounds are printed.  The two losses are compared first and the tool stops unless
they agree: the value to 1e-5 relative and the gradients to 1e-7 + 1e-4 of the largest gradient (two fp32 summation orders over
2 x 10^6 pixels per plane; the fused form adds up to 2048 partial rows per sample in sequence, n eps / 2 = 6e-5 at worst), so that the
times are those of the same result.  Prints one JSON line.  Needs the MI355X: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import trainer  # noqa: E402

REGIONS = ((1, 2, 3), (2, 3), (3,))


def inputs(batch, size, levels, ignore, dev):
    g = torch.Generator().manual_seed(29)
    outs, tgs = [], []
    for s in range(levels):
        n = size >> s
        outs.append((torch.randn(batch, len(REGIONS), n, n, n, generator=g) * 2).to(dev).requires_grad_(True))
        seg = torch.randint(0, 5 if ignore else 4, (batch, 1, n, n, n), generator=g).float().to(dev)
        tgs.append(trainer.regions_from_label_map(seg, REGIONS, 4 if ignore else None))
    return outs, tgs


def composed(outs, tgs, ignore):
    ws = trainer.deep_supervision_weights(len(outs))
    return sum(w * trainer.dc_and_bce_loss(o, t, True, False, ignore) for w, o, t in zip(ws, outs, tgs))


def timed(fn, outs, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        for o in outs:
            o.grad = None
        fn().backward()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_region_loss: no GPU; a time is only ever measured on the MI355X")
    dev = torch.device("cuda:0")
    result = {"shape": {"batch": a.batch, "heads": len(REGIONS), "size": a.size, "levels": a.levels}, "iters": a.iters, "rounds": a.rounds}
    for ignore in (False, True):
        outs, tgs = inputs(a.batch, a.size, a.levels, ignore, dev)
        forms = {"fused": lambda: trainer.region_deep_supervision_loss(outs, tgs, None, True, ignore_label=4 if ignore else None),
                 "composed": lambda: composed(outs, tgs, ignore)}
        values, grads = {}, {}
        for name, fn in forms.items():
            for o in outs:
                o.grad = None
            loss = fn()
            loss.backward()
            values[name], grads[name] = float(loss.detach()), [o.grad.clone() for o in outs]
        gerr = max(float((x - y).abs().max()) for x, y in zip(grads["fused"], grads["composed"]))
        gmax = max(float(y.abs().max()) for y in grads["composed"])
        if abs(values["fused"] - values["composed"]) > 1e-5 * abs(values["composed"]) or gerr > 1e-7 + 1e-4 * gmax:
            raise SystemExit(f"bench_region_loss: the two forms disagree (values {values}, gradient difference {gerr} of {gmax}); "
                             "no time is reported for different results")
        for fn in forms.values():                                  # warm-up of every shape in the timed window
            timed(fn, outs, 3)
        times = {name: [] for name in forms}
        for _ in range(a.rounds):                                  # alternating: both forms see the same machine state
            for name, fn in forms.items():
                times[name].append(timed(fn, outs, a.iters))
        result["ignore_plane" if ignore else "no_ignore"] = {
            "value_fused": values["fused"], "value_composed": values["composed"], "max_gradient_difference": gerr,
            **{f"{name}_ms_median": round(statistics.median(t), 4) for name, t in times.items()},
            **{f"{name}_ms_min_max": [round(min(t), 4), round(max(t), 4)] for name, t in times.items()}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
