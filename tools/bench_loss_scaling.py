#!/usr/bin/env python
"""What fp16 loss scaling costs at the end of the train step, with torch.amp.GradScaler and with K35 (trainer.DeviceGradScaler: the
scaling fused into the clip + update launches of K11 / K34).

1. The step TAIL alone, scaled gradients resident in HBM, on the parameter lists of the BTCV-shaped 3-D network and of the headline
   2-D network (shapes only; seeded random tensors, no forward or backward, as tools/bench_optimizers.py):
     torch   GradScaler.unscale_ + clip_grad_norm_(12) + GradScaler.step(torch optimizer) + GradScaler.update()
     K35     DeviceGradScaler.step(capturable ClipAdamW / ClipSGD, max_norm=12) + update()
   The gradients are scaled by 65536 once.  K35 leaves them as they are, so every iteration repeats the first; torch's unscale_
   rewrites them, so its later iterations see ever smaller (soon zero) gradients: the same kernels and the same bytes, which is
   what is timed.  Before any timing the first step of both forms is compared on the same gradients (1e-4 relative L2 of the update,
   the criterion of tools/bench_optimizers.py) and the tool stops on a difference.
2. The full fp16 train step at the shape of bench.py --config 5 (512 x 640 x 3, 8 classes, variant A, batch 4) in three forms: eager with
   torch's scaler, eager with K35, and K35 captured into a hipGraph (trainer.GraphedTrainStep).  Host wall time per step with a
   synchronisation at the end of each timed window (the eager forms are bound by the host's enqueue rate; device events alone would
   hide that).  Every form starts from scale 65536 on the same fresh network; a step that overflows is skipped and has a cheaper
   tail, so the result says per form how many of the steps taken were applied and the scale it ended on.

All forms are warmed up and timed in alternating rounds inside one process; the median round and the spread are printed, one JSON
line.  Needs the MI355X: there is no CPU fallback."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import model, trainer  # noqa: E402
from tools.bench_optimizers import parameter_shapes, tensors, timed  # noqa: E402

CLIP, SCALE = 12.0, 65536.0
# name -> (capturable fused optimizer, torch optimizer)
RECIPES = {
    "adamw_k11": (lambda ps: trainer.ClipAdamW(ps, 5e-4, eps=1e-4, weight_decay=3e-5, capturable=True),
                  lambda ps: torch.optim.AdamW(ps, lr=5e-4, eps=1e-4, weight_decay=3e-5)),
    "sgd_nesterov": (lambda ps: trainer.ClipSGD(ps, 1e-2, 0.99, 3e-5, capturable=True),
                     lambda ps: torch.optim.SGD(ps, 1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)),
}
FULL = dict(img=(512, 640), in_ch=3, classes=8, batch=4, variant="A")            # bench.py CONFIGS[5]


def tail(which, a, dev):
    shapes = parameter_shapes(which)
    n_params = sum(int(torch.Size(s).numel()) for s in shapes)
    init, grads = tensors(shapes, dev, 1), [g * SCALE for g in tensors(shapes, dev, 2)]
    entry = {"tensors": len(shapes), "parameters": n_params}
    for name, (make_fused, make_torch) in RECIPES.items():
        ps_f = [torch.nn.Parameter(p.clone()) for p in init]
        ps_t = [torch.nn.Parameter(p.clone()) for p in init]
        for ps in (ps_f, ps_t):
            for p, g in zip(ps, grads):
                p.grad = g.clone()
        opt_f, opt_t = make_fused(ps_f), make_torch(ps_t)
        ours, theirs = trainer.DeviceGradScaler(dev, init_scale=SCALE), torch.amp.GradScaler("cuda", init_scale=SCALE)
        theirs.scale(torch.zeros(1, device=dev))                                  # torch creates its scale tensor at the first scale()

        def fused_step():
            ours.step(opt_f, max_norm=CLIP)
            ours.update()

        def torch_step():
            theirs.unscale_(opt_t)
            torch.nn.utils.clip_grad_norm_(ps_t, CLIP)
            theirs.step(opt_t)
            theirs.update()

        steps = {"k35": fused_step, "torch": torch_step}
        for step in steps.values():
            step()
        torch.cuda.synchronize()
        with torch.no_grad():
            diff = sum(float((p.double() - q.double()).pow(2).sum()) for p, q in zip(ps_f, ps_t)) ** 0.5
            moved = sum(float((q.double() - p0.double()).pow(2).sum()) for q, p0 in zip(ps_t, init)) ** 0.5
        worst = diff / moved
        if not worst <= 1e-4 or opt_f.steps_done() != 1:
            raise SystemExit(f"bench_loss_scaling: {name} on {which}: the first steps differ by {worst} of the update; no time is "
                             "reported for different results")
        for step in steps.values():
            timed(step, 5)
        times = {side: [] for side in steps}
        for _ in range(a.rounds):                                                 # alternating: both forms see the same machine state
            for side, step in steps.items():
                times[side].append(timed(step, a.iters))
        entry[name] = {"first_step_relative_l2_difference": worst,
                       **{f"{s}_ms_median": round(statistics.median(t), 4) for s, t in times.items()},
                       **{f"{s}_ms_min_max": [round(min(t), 4), round(max(t), 4)] for s, t in times.items()}}
        del ps_f, ps_t, opt_f, opt_t, steps
        torch.cuda.empty_cache()
    return entry


def wall(step, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def full(a, dev):
    torch.manual_seed(0)
    start = model.build_network_architecture(FULL["img"], FULL["in_ch"], FULL["classes"], True, FULL["variant"], "fp16").to(dev).eval()
    data, target = trainer.synthetic_batch(FULL["batch"], FULL["in_ch"], *FULL["img"], FULL["classes"], device=dev)
    forms, state = {}, {}
    for name, device_scaler, graph in (("eager_torch_scaler", False, False), ("eager_k35", True, False), ("graph_k35", True, True)):
        net = copy.deepcopy(start)
        opt, _ = trainer.configure_optimizers(net, capturable=device_scaler)
        scaler = trainer.DeviceGradScaler(dev) if device_scaler else torch.amp.GradScaler("cuda")
        state[name] = (opt, scaler)
        if graph:
            forms[name] = trainer.GraphedTrainStep(net, opt, data, target, warmup=3, grad_scaler=scaler)
        else:
            forms[name] = lambda net=net, opt=opt, scaler=scaler: trainer.train_step(net, opt, data, target, grad_scaler=scaler)
    for step in forms.values():
        wall(step, 3)
    times = {name: [] for name in forms}
    for _ in range(a.full_rounds):
        for name, step in forms.items():
            times[name].append(wall(step, a.full_iters))
    # a skipped step has a cheaper tail: say per form how many of the steps taken (warm-up and capture warm-up included) were applied,
    # and the scale they ended on.  torch's scaler does not call a skipped step, so ClipAdamW's host counter counts applied steps too
    taken = {name: 3 + a.full_rounds * a.full_iters + (3 if name == "graph_k35" else 0) for name in forms}
    work = {name: {"steps_taken": taken[name], "steps_applied": opt.steps_done(), "final_scale": scaler.get_scale()}
            for name, (opt, scaler) in state.items()}
    return {"shape": FULL, "iters": a.full_iters, "rounds": a.full_rounds, "work": work,
            **{f"{n}_ms_median": round(statistics.median(t), 3) for n, t in times.items()},
            **{f"{n}_ms_min_max": [round(min(t), 3), round(max(t), 3)] for n, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)        # tail: a timed window of a tenth of a second and more
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--full-iters", type=int, default=10)
    ap.add_argument("--full-rounds", type=int, default=5)
    ap.add_argument("--skip-full", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_scaling: no GPU; a time is only ever measured on the MI355X")
    dev = torch.device("cuda:0")
    result = {"clip": CLIP, "scale": SCALE, "iters": a.iters, "rounds": a.rounds}
    for which in ("btcv_3d", "headline_2d"):
        result[which] = tail(which, a, dev)
    if not a.skip_full:
        result["full_fp16_step"] = full(a, dev)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
