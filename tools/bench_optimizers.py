#!/usr/bin/env python
"""Time of the step TAIL alone -- gradient clipping + the optimizer's update, gradients resident in HBM -- of the fused optimizers of
K34 (trainer.ClipSGD, trainer.ClipAdam in its two recipes; K11's trainer.ClipAdamW for scale) against what the reference's trainers run:
torch.nn.utils.clip_grad_norm_(parameters, 12) + the step of torch.optim.SGD / AdamW(amsgrad=True) / Adam / AdamW (torch's default
multi-tensor path) on a copy of the same parameters.

Parameter lists: the BTCV-shaped 3-D network (bench.py --config 4) and the headline 2-D network (256 x 256, 14 classes, variant B).  Only
the parameter shapes of the networks are used; parameters and gradients are seeded random tensors of those shapes, so that no forward
or backward runs.  Both forms are warmed up, then timed in alternating rounds with device events inside one process; the median round
and the spread over the rounds are printed.  Before any timing the first step of both forms is compared on the same gradients and the
tool stops unless the two updates agree to 1e-4 in relative L2 over all parameters (two fp32 evaluation orders of one step; an
element-wise bound does not fit Adam with L2 decay, whose step lr g / (|g| + 1e-8) is steep where coef g + wd p crosses zero).
Rates are the bytes the fused arithmetic needs -- update 20 (SGD: p, g, buf in; p, buf out) / 36 (amsgrad) / 28 (Adam, AdamW) bytes
per parameter plus 4 for the norm (profiling.algorithmic_bytes_optimizer) -- over the measured time, for both forms: for torch it is
NOT its traffic (it makes five or six sweeps) but the same useful work per second.  Prints one JSON line.  Needs the MI355X: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import model, model3d, profiling, trainer  # noqa: E402

CLIP = 12.0
# name -> (fused optimizer, torch optimizer, the byte count's kind in profiling.OPTIMIZER_VARIANT_BYTES)
RECIPES = {
    "sgd_nesterov": (lambda ps: trainer.ClipSGD(ps, 1e-2, 0.99, 3e-5),
                     lambda ps: torch.optim.SGD(ps, 1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True), "sgd_nesterov"),
    "adamw_amsgrad": (lambda ps: trainer.ClipAdam(ps, 1e-2, weight_decay=3e-5, amsgrad=True, decoupled=True),
                      lambda ps: torch.optim.AdamW(ps, lr=1e-2, weight_decay=3e-5, amsgrad=True), "adamw_amsgrad"),
    "adam_l2": (lambda ps: trainer.ClipAdam(ps, 1e-2, weight_decay=3e-5, amsgrad=False, decoupled=False),
                lambda ps: torch.optim.Adam(ps, lr=1e-2, weight_decay=3e-5), "adam_l2"),
    "adamw_k11": (lambda ps: trainer.ClipAdamW(ps, 5e-4, eps=1e-4, weight_decay=3e-5),
                  lambda ps: torch.optim.AdamW(ps, lr=5e-4, eps=1e-4, weight_decay=3e-5), "adam_l2"),     # the same 28 bytes
}


def parameter_shapes(which):
    """The shapes of the trainable parameters of a network, built on the host (nothing of it runs)."""
    torch.manual_seed(0)
    if which == "btcv_3d":
        n = len(model3d.BTCV_STRIDES)
        net = model3d.build_network_architecture_3d(1, 14, [[3, 3, 3]] * n, model3d.BTCV_STRIDES, [2] * n, [2] * (n - 1))
    else:
        net = model.build_network_architecture((256, 256), 1, 14, True, "B")
    return [tuple(p.shape) for p in net.parameters() if p.requires_grad]


def tensors(shapes, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(dev) for s in shapes]


def timed(step, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)       # a timed window of a quarter of a second and more
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizers: no GPU; a time is only ever measured on the MI355X")
    dev = torch.device("cuda:0")
    result = {"clip": CLIP, "iters": a.iters, "rounds": a.rounds}
    for which in ("btcv_3d", "headline_2d"):
        shapes = parameter_shapes(which)
        n_params = sum(int(torch.Size(s).numel()) for s in shapes)
        init, grads = tensors(shapes, dev, 1), tensors(shapes, dev, 2)
        entry = {"tensors": len(shapes), "parameters": n_params}
        for name, (make_fused, make_torch, kind) in RECIPES.items():
            sides = {}
            for side, make in (("fused", make_fused), ("torch", make_torch)):
                ps = [torch.nn.Parameter(p.clone()) for p in init]
                sides[side] = (ps, make(ps))

            def restore_grads(ps):
                for p, g in zip(ps, grads):                      # clip_grad_norm_ rescales the gradients in memory: start from the same ones
                    if p.grad is None:
                        p.grad = g.clone()
                    else:
                        p.grad.copy_(g)

            def fused_step(ps=sides["fused"][0], opt=sides["fused"][1]):
                opt.step(max_norm=CLIP)

            def torch_step(ps=sides["torch"][0], opt=sides["torch"][1]):
                torch.nn.utils.clip_grad_norm_(ps, CLIP)
                opt.step()

            steps = {"fused": fused_step, "torch": torch_step}
            for side in steps:
                restore_grads(sides[side][0])
                steps[side]()
            torch.cuda.synchronize()
            with torch.no_grad():
                diff = sum(float((p.double() - q.double()).pow(2).sum()) for p, q in zip(sides["fused"][0], sides["torch"][0])) ** 0.5
                moved = sum(float((q.double() - p0.double()).pow(2).sum()) for q, p0 in zip(sides["torch"][0], init)) ** 0.5
            worst = diff / moved
            if not worst <= 1e-4:
                raise SystemExit(f"bench_optimizers: {name} on {which}: the first steps differ by {worst} of the update; no time is "
                                 "reported for different results")
            # the timed window: the gradients stay as the first torch step left them (scaled once, then below the clip norm for torch;
            # unscaled, hence clipped every step, for the fused form): the same kernels and the same bytes every iteration
            for side in steps:
                timed(steps[side], 5)
            times = {side: [] for side in steps}
            for _ in range(a.rounds):                            # alternating: both forms see the same machine state
                for side in steps:
                    times[side].append(timed(steps[side], a.iters))
            useful = profiling.algorithmic_bytes_optimizer(kind, n_params)
            entry[name] = {"bytes_per_parameter": useful // n_params, "first_step_relative_l2_difference": worst,
                           **{f"{s}_ms_median": round(statistics.median(t), 4) for s, t in times.items()},
                           **{f"{s}_ms_min_max": [round(min(t), 4), round(max(t), 4)] for s, t in times.items()},
                           **{f"{s}_useful_GBps": round(useful / statistics.median(t) / 1e6, 1) for s, t in times.items()}}
            del sides, steps
            torch.cuda.empty_cache()
        result[which] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
