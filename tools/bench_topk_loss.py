#!/usr/bin/env python
"""Time of the "dice_topk10" deep-supervision loss (forward + backward to the logit maps): the fused loss (K33,
trainer.loss_variant_deep_supervision_loss) against trainer.loss_variant_deep_supervision_loss_eager on the device -- softmax, one-hot,
masked sums, log_softmax + nll, a device-wide torch.topk per level and the backward of all of them, the arithmetic that the reference's
DeepSupervisionWrapper(DC_and_topk_loss) runs.

Shapes: the headline level set (batch 10, 14 classes, 256 x 256 with five levels) and the 3-D plan (batch 2, 14 classes, 96 x 160 x 160
with five levels).  Both forms are warmed up, then timed in alternating rounds with device events inside one process; the median round
and the spread over the rounds are printed.  The two losses are compared first and the tool stops unless they agree: the value to 1e-5
relative and the gradients to 1e-7 + 1e-4 of the largest gradient (random inputs: no ties at the threshold).  Two runs of the fused form
are compared with torch.equal, value and gradients, and the outcome is printed.  Prints one JSON line.  Needs the MI355X: there is no
CPU fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import trainer  # noqa: E402

VARIANT = "dice_topk10"
SHAPES = {"headline_2d": (10, 14, (256, 256)), "plan_3d": (2, 14, (96, 160, 160))}


def inputs(batch, classes, size, levels, dev):
    g = torch.Generator().manual_seed(31)
    outs, tgs = [], []
    for s in range(levels):
        dims = tuple(max(1, n >> s) for n in size)
        outs.append((torch.randn(batch, classes, *dims, generator=g) * 2).to(dev).requires_grad_(True))
        tgs.append(torch.randint(0, classes, (batch, 1) + dims, generator=g).float().to(dev))
    return outs, tgs


def run(fn, outs):
    for o in outs:
        o.grad = None
    loss = fn()
    loss.backward()
    return loss.detach().clone(), [o.grad.clone() for o in outs]


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
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk_loss: no GPU; a time is only ever measured on the MI355X")
    dev = torch.device("cuda:0")
    result = {"variant": VARIANT, "levels": a.levels, "iters": a.iters, "rounds": a.rounds}
    for name, (batch, classes, size) in SHAPES.items():
        outs, tgs = inputs(batch, classes, size, a.levels, dev)
        forms = {"fused": lambda: trainer.loss_variant_deep_supervision_loss(outs, tgs, VARIANT, True, False),
                 "composed": lambda: trainer.loss_variant_deep_supervision_loss_eager(outs, tgs, VARIANT, True, False)}
        first = {k: run(fn, outs) for k, fn in forms.items()}
        again = run(forms["fused"], outs)
        same = bool(torch.equal(first["fused"][0], again[0]) and all(torch.equal(x, y) for x, y in zip(first["fused"][1], again[1])))
        values = {k: float(v[0]) for k, v in first.items()}
        gerr = max(float((x - y).abs().max()) for x, y in zip(first["fused"][1], first["composed"][1]))
        gmax = max(float(y.abs().max()) for y in first["composed"][1])
        if abs(values["fused"] - values["composed"]) > 1e-5 * abs(values["composed"]) or gerr > 1e-7 + 1e-4 * gmax:
            raise SystemExit(f"bench_topk_loss: the two forms disagree at {name} (values {values}, gradient difference {gerr} of {gmax}); "
                             "no time is reported for different results")
        for fn in forms.values():                                  # warm-up of every shape in the timed window
            timed(fn, outs, 2)
        times = {k: [] for k in forms}
        for _ in range(a.rounds):                                  # alternating: both forms see the same machine state
            for k, fn in forms.items():
                times[k].append(timed(fn, outs, a.iters))
        result[name] = {"shape": [batch, classes, *size], "value_fused": values["fused"], "value_composed": values["composed"],
                        "max_gradient_difference": gerr, "two_fused_runs_torch_equal": same,
                        **{f"{k}_ms_median": round(statistics.median(t), 4) for k, t in times.items()},
                        **{f"{k}_ms_min_max": [round(min(t), 4), round(max(t), 4)] for k, t in times.items()}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
