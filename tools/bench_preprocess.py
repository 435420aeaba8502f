"""Case preprocessing on one MI355X (K22, csrc/preprocess.hip) against the host path, on two BTCV-like raw cases, and one
predict_case of the config-4 3-D network split into preprocess / network / export.

    python tools/bench_preprocess.py [--repeats 5] [--out profiles/preprocess_k22_btcv_vs_host.log]

  (a) 2-D configuration: raw (1, 148, 512, 512) at (2.5, 0.76, 0.76) with a zero rim, target in-plane 0.79 mm: separate z;
  (b) 3d_fullres-like:   raw (1, 200, 256, 256) at (1.5, 1.0, 1.0) with a zero rim, target 1.2 mm isotropic: full 3-D zoom.
Reports the K22 time from device events around the whole preprocess_case call (upload of the tables and the box read-back
included; the raw volume already on the device) and per kernel (the library's per-kernel event timers); the algorithmic bytes of
the kernels (every read and write once) over 6.29 TB/s of HBM; the host path's time on this machine's CPU (scipy, threads
stated), standing in for the reference's CPU preprocessing; and the agreement of device and host results in fp32 ulps."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import export, inference, model3d, predict, profiling  # noqa: E402
from mlagg_unet_amd import preprocessing as P  # noqa: E402

HBM = 6.29e12
FG = {"mean": 120.7, "std": 410.3, "percentile_00_5": -900.5, "percentile_99_5": 2500.25}
CASES = {
    "a_2d_separate_z": dict(shape=(148, 512, 512), spacing=(2.5, 0.76, 0.76), cfg=(0.79, 0.79), rim=(0, 24, 24), name="2d"),
    "b_3d_zoom": dict(shape=(200, 256, 256), spacing=(1.5, 1.0, 1.0), cfg=(1.2, 1.2, 1.2), rim=(8, 12, 12), name="3d_fullres"),
}
K22 = ("pp_box_kernel", "pp_stats_kernel (+ final)", "pp_normalize_kernel", "pp_minmax_kernel", "pp_cubic_kernel", "pp_gather_kernel")


def plans_for(cfg_spacing, name, patch):
    cfg = {"spacing": list(cfg_spacing), "normalization_schemes": ["CTNormalization"], "use_mask_for_norm": [False],
           "patch_size": list(patch)}
    return {"transpose_forward": [0, 1, 2], "transpose_backward": [0, 1, 2], "configurations": {name: cfg},
            "foreground_intensity_properties_per_channel": {"0": dict(FG)}}


def raw_volume(shape, rim, seed):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand((1,) + tuple((s + 7) // 8 for s in shape), generator=g) * 4024 - 1024
    v = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :shape[0], :shape[1], :shape[2]]
    v = torch.round(v + torch.randn(v.shape, generator=g) * 25)
    v[v == 0] = 1
    out = torch.zeros((1,) + tuple(shape))
    sl = tuple(slice(r, s - r) for r, s in zip(rim, shape))
    out[(slice(None),) + sl] = v[(slice(None),) + sl]
    return out


def device_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def kernels_ms(fn):
    fn()
    torch.cuda.synchronize()
    profiling.select_all()
    profiling.collect()
    fn()
    torch.cuda.synchronize()
    got = profiling.collect()
    profiling.select(None)
    return {k: (round(got[k]["ms"], 3), got[k]["count"]) for k in K22 if k in got}


def algorithmic_bytes(raw, crop, new, sep, axis):
    """every kernel's reads and writes once: box (raw), normalize (crop in and out), clip ranges (crop), the cubic passes (fp32 or
    fp64 in and out), the separate-z blend"""
    n = lambda s: int(np.prod(s))  # noqa: E731
    total = 4 * n(raw) + 8 * n(crop) + 4 * n(crop)
    cur, size = list(crop), 4
    axes = [a for a in range(3) if a != axis] if sep else [0, 1, 2]
    for i, a in enumerate(axes):
        nxt = list(cur)
        nxt[a] = new[a]
        last = i == len(axes) - 1 and (not sep or cur[axis] == new[axis])
        total += size * n(cur) + (4 if last else 8) * n(nxt)
        cur, size = nxt, (4 if last else 8)
    if sep and cur[axis] != new[axis]:
        total += 8 * n(cur) + 4 * n(new)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-predict", action="store_true")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess needs the MI355X")
    dev = torch.device("cuda:0")
    lines = [f"device {torch.cuda.get_device_name(0)}; host path on {torch.get_num_threads()} torch CPU threads "
             f"(scipy's zoom runs on one); device times: median (min-max) of {args.repeats} calls after one warm-up, events around "
             "the whole preprocess_case call, raw volume already on the device"]
    for tag, c in CASES.items():
        plans = plans_for(c["cfg"], c["name"], (16, 16))
        raw = raw_volume(c["shape"], c["rim"], 22)
        rawd = raw.to(dev)
        props = {"spacing": list(c["spacing"])}
        call = lambda: P.preprocess_case(rawd, props, plans, c["name"])  # noqa: E731
        med, lo, hi = device_ms(call, args.repeats)
        kern = kernels_ms(call)
        out, pp = call()
        crop = tuple(pp["shape_after_cropping_and_before_resampling"])
        cur = list(c["spacing"])
        target = list(c["cfg"]) if len(c["cfg"]) == 3 else [cur[0], *c["cfg"]]
        sep, axis = export.separate_z_decision(cur, target)
        nbytes = algorithmic_bytes(c["shape"], crop, tuple(out.shape[1:]), sep, axis)
        ksum = sum(v[0] for v in kern.values())
        t0 = time.perf_counter()
        host, _ = P.preprocess_case(raw.numpy(), props, plans, c["name"])
        host_s = time.perf_counter() - t0
        a = np.ascontiguousarray(out.cpu().numpy()).view(np.int32).astype(np.int64)
        d = np.abs(a - np.ascontiguousarray(host).view(np.int32).astype(np.int64))
        bound = nbytes / HBM * 1e3
        lines.append(f"[{tag}] raw {(1,) + c['shape']} at {c['spacing']} -> crop {crop} -> {tuple(out.shape[1:])}; "
                     f"separate_z={sep} axis={axis}")
        lines.append(f"  K22 whole call {med:.3f} ms ({lo:.3f}-{hi:.3f}); kernels {ksum:.3f} ms: {json.dumps(kern)}")
        lines.append(f"  algorithmic bytes {nbytes / 1e9:.3f} GB -> HBM bound {bound:.3f} ms = {bound / ksum * 100:.1f}% of the "
                     "kernel time")
        lines.append(f"  host path: {host_s:.2f} s")
        lines.append(f"  device vs host: max {int(d.max())} ulp, {int((d > 0).sum())} of {d.size} voxels differ")
        print("\n".join(lines[-5:]), flush=True)
        del rawd, out
        torch.cuda.empty_cache()
    if not args.skip_predict:
        n = len(model3d.BTCV_STRIDES)
        torch.manual_seed(0)
        net = model3d.build_network_architecture_3d(1, 14, [[3, 3, 3]] * n, model3d.BTCV_STRIDES, [2] * n, [2] * (n - 1),
                                                    enable_deep_supervision=False).to(dev).eval()
        plans = plans_for((1.5, 1.5, 1.5), "3d_fullres", (96, 160, 160))
        raw = raw_volume((120, 256, 256), (6, 20, 20), 4)
        props = {"spacing": [2.0, 1.0, 1.0]}
        dj = {"labels": {"background": 0, **{f"organ{k}": k for k in range(1, 14)}}}
        rawd = raw.to(dev)
        with torch.no_grad():
            predict.predict_case(net, rawd, props, plans, "3d_fullres", dj)              # warm-up: kernels, workspaces, MIOpen
            torch.cuda.synchronize()
            t = [time.perf_counter()]
            data, pp = P.preprocess_case(rawd, props, plans, "3d_fullres")
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            logits = inference.predict_sliding_window_return_logits(net, data, 14, (96, 160, 160))
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            seg, _ = export.convert_predicted_logits_to_segmentation_with_correct_shape(logits, pp, (1.5, 1.5, 1.5))
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            whole = time.perf_counter()
            seg2, _ = predict.predict_case(net, rawd, props, plans, "3d_fullres", dj)
            torch.cuda.synchronize()
            whole = time.perf_counter() - whole
        same = bool(torch.equal(seg, seg2))
        lines.append(f"[predict_case] config-4 3-D network (BTCV strides, 14 classes, tile (96, 160, 160), no mirroring): raw "
                     f"{tuple(raw.shape)} at {props['spacing']} -> {tuple(data.shape)} -> labels {tuple(seg.shape)}")
        lines.append(f"  preprocess {1e3 * (t[1] - t[0]):.1f} ms, network (sliding window) {1e3 * (t[2] - t[1]):.1f} ms, export "
                     f"{1e3 * (t[3] - t[2]):.1f} ms; predict_case as one call {1e3 * whole:.1f} ms; same labels: {same}")
        print("\n".join(lines[-2:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
