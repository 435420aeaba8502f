"""Training-case preprocessing on one MI355X (K22 + K26, csrc/preprocess.hip and csrc/preprocess_train.hip) against the host path,
on the two BTCV-like raw cases of tools/bench_preprocess.py with a 14-label segmentation added.

    python tools/bench_preprocess_train.py [--repeats 3] [--out profiles/preprocess_train_k26_vs_host.log]

  (a) 2-D configuration: raw (1, 148, 512, 512) at (2.5, 0.76, 0.76) with a zero rim, target in-plane 0.79 mm: separate z;
  (b) 3d_fullres-like:   raw (1, 200, 256, 256) at (1.5, 1.0, 1.0) with a zero rim, target 1.2 mm isotropic: full 3-D zoom.
Reports, per case: the device path end to end (wall clock around preprocess_training_case from the uploaded raw arrays to
finished data, seg and class_locations, its two read-backs and the host's RandomState draws included) and split into stages
(crop + normalise, data resampling, segmentation resampling, class locations, read-backs), each stage timed on its own with a
synchronize on both sides after a warm-up; the K26 kernels' times (the library's per-kernel event timers) and their algorithmic
bytes (every read and write once) over 6.29 TB/s of HBM; the host path (numpy / scipy, the reference's arithmetic) on this
machine's CPUs, split the same way; and whether the two agree.  Each case runs in a child process of its own under a time limit,
and the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.29e12
FG = {"mean": 120.7, "std": 410.3, "percentile_00_5": -900.5, "percentile_99_5": 2500.25}
CASES = {
    "a_2d_separate_z": dict(shape=(148, 512, 512), spacing=(2.5, 0.76, 0.76), cfg=(0.79, 0.79), rim=(0, 24, 24), name="2d"),
    "b_3d_zoom": dict(shape=(200, 256, 256), spacing=(1.5, 1.0, 1.0), cfg=(1.2, 1.2, 1.2), rim=(8, 12, 12), name="3d_fullres"),
}
K26 = ("pt_seg_crop_kernel", "pt_seg_resize_kernel", "pt_rank_count_kernel (+ scan)", "pt_rank_select_kernel")
N_LABELS = 14
CASE_TIMEOUT = 420


def plans_for(cfg_spacing, name):
    cfg = {"spacing": list(cfg_spacing), "normalization_schemes": ["CTNormalization"], "use_mask_for_norm": [False],
           "patch_size": [16, 16]}
    return {"transpose_forward": [0, 1, 2], "transpose_backward": [0, 1, 2], "configurations": {name: cfg},
            "foreground_intensity_properties_per_channel": {"0": dict(FG)}}


def label_volume(shape, rim, seed):
    """(1, *shape) int16: blocky organs 1 .. 14 over about a third of the non-zero box, background elsewhere."""
    g = torch.Generator().manual_seed(seed)
    block = (6, 24, 24)
    coarse = torch.randint(0, 3 * N_LABELS, tuple((s + b - 1) // b for s, b in zip(shape, block)), generator=g)
    coarse = torch.where(coarse > N_LABELS, torch.zeros_like(coarse), coarse)
    for a, b in enumerate(block):
        coarse = coarse.repeat_interleave(b, a)
    out = torch.zeros((1,) + tuple(shape), dtype=torch.int16)
    sl = tuple(slice(r, s - r) for r, s in zip(rim, shape))
    out[(slice(None),) + sl] = coarse[:shape[0], :shape[1], :shape[2]].to(torch.int16)[sl]
    return out


def timed(fn, repeats, sync):
    """median wall-clock ms of fn after one warm-up call"""
    out = fn()
    sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        sync()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times)), out


def run_case(tag, repeats):
    import mlagg_unet_amd  # noqa: F401
    from mlagg_unet_amd import export, ops, profiling
    from mlagg_unet_amd import preprocessing as P
    from tools.bench_preprocess import raw_volume

    c = CASES[tag]
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    plans = plans_for(c["cfg"], c["name"])
    cfg = plans["configurations"][c["name"]]
    dj = {"labels": {"background": 0, **{f"organ{k}": k for k in range(1, N_LABELS + 1)}}}
    collect, max_label = P._label_lists(dj)
    props = {"spacing": list(c["spacing"])}
    raw, seg = raw_volume(c["shape"], c["rim"], 22), label_volume(c["shape"], c["rim"], 26)
    rawd, segd = raw.to(dev), seg.to(dev)
    lines = []

    whole = lambda: P.preprocess_training_case(rawd, segd, props, plans, c["name"], dj)  # noqa: E731
    dev_ms, (data, s, pp) = timed(whole, repeats, sync)
    crop = tuple(pp["shape_after_cropping_and_before_resampling"])
    new = tuple(data.shape[1:])
    spacing = list(c["spacing"])
    target = list(c["cfg"]) if len(c["cfg"]) == 3 else [spacing[0], *c["cfg"]]
    sep, axis = export.separate_z_decision(spacing, target)

    # stages of the device path, each on its own
    stage = {}
    stage["crop + normalise"], (d0, _, s0, h0) = timed(
        lambda: P._preprocess_device(rawd, ["CTNormalization"], [False], plans["foreground_intensity_properties_per_channel"], dev,
                                     segd[0], max_label), repeats, sync)
    stage["data resampling"], _ = timed(lambda: P.resample_data_to_shape(d0, new, spacing, target), repeats, sync)
    stage["segmentation resampling"], (s1, h1) = timed(lambda: P._resample_seg_device(s0[None], new, sep, axis, max_label), repeats, sync)
    stage["read-back (histogram)"], hist = timed(lambda: h1.cpu().numpy(), repeats, sync)
    stage["class locations"], _ = timed(lambda: P._sample_locations_device(s1, collect, 1234, max_label, hist), repeats, sync)
    t0 = time.perf_counter()
    rs = np.random.RandomState(1234)
    for lab in collect:
        n = int(hist[lab + 1])
        if n:
            rs.choice(n, P._num_to_sample(n), replace=False)
    draws_ms = 1e3 * (time.perf_counter() - t0)

    # K26 kernels
    whole()
    sync()
    profiling.select_all()
    profiling.collect()
    whole()
    sync()
    got = profiling.collect()
    profiling.select(None)
    kern = {k: (round(got[k]["ms"], 3), got[k]["count"]) for k in K26 if k in got}
    n = lambda shp: int(np.prod(shp))  # noqa: E731
    n_sel = sum(len(v) for v in pp["class_locations"].values())
    rows = -(-n(new) // ops.PP_RANK_BLOCK)
    nbytes = {"pt_seg_crop_kernel": 2 * n(crop) + n(crop) + 2 * n(crop),
              "pt_seg_resize_kernel": 2 * n(crop) + 2 * n(new),
              "pt_rank_count_kernel (+ scan)": 2 * n(new) + 3 * 8 * rows * len(collect),
              "pt_rank_select_kernel": n_sel * (2 * ops.PP_RANK_BLOCK // 2 + 8 * 4 + 8)}

    # host path, the same split
    t = [time.perf_counter()]
    x, sh = raw.numpy().copy(), seg.numpy().copy()
    hd, hs, _ = P.crop_to_nonzero(x, sh)
    hd = np.array(hd)
    hd[0] = P._normalize_channel_host(hd[0], hs[0], "CTNormalization", False, FG)
    t.append(time.perf_counter())
    hd = P.resample_data_to_shape(hd, new, spacing, target)
    t.append(time.perf_counter())
    hs = P._resample_seg_host(hs, new, sep, axis)
    t.append(time.perf_counter())
    hl = P._sample_locations_host(hs, collect, 1234)
    t.append(time.perf_counter())
    host = [1e3 * (b - a) for a, b in zip(t[:-1], t[1:])]
    host_ms = 1e3 * (t[-1] - t[0])

    got_s = s.cpu().numpy()
    diff = int((got_s != hs.astype(got_s.dtype)).sum())
    same_locs = diff == 0 and all(np.array_equal(pp["class_locations"][k], hl[k]) for k in hl)
    lines.append(f"[{tag}] raw {(1,) + c['shape']} at {c['spacing']} + {N_LABELS}-label segmentation -> crop {crop} -> {new}; "
                 f"separate_z={sep} axis={axis}; {n_sel} class locations")
    lines.append(f"  device, end to end (raw arrays on the device -> data, seg, class_locations; median of {repeats}): {dev_ms:.1f} ms")
    lines.append("  device stages (ms, each timed alone): " + json.dumps({k: round(v, 2) for k, v in stage.items()}) +
                 f"; of the class locations, the host's RandomState draws: {draws_ms:.1f} ms")
    lines.append(f"  host, end to end: {host_ms:.0f} ms; stages (ms): " + json.dumps(dict(zip(
        ["crop + normalise", "data resampling", "segmentation resampling", "class locations"], [round(v, 1) for v in host]))))
    lines.append(f"  device is {host_ms / dev_ms:.1f}x the host path")
    for k, (ms, cnt) in kern.items():
        bound = nbytes[k] / HBM * 1e3
        lines.append(f"  {k}: {ms:.3f} ms in {cnt} launches; algorithmic bytes {nbytes[k] / 1e6:.1f} MB -> HBM bound {bound:.4f} ms = "
                     f"{100 * bound / ms if ms else 0:.1f}% of its time")
    lines.append(f"  device vs host: {diff} of {got_s.size} labels differ; class locations identical: {same_locs}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)          # the child process of one case
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess_train needs the MI355X")
    if args.case:
        print("\n".join(run_case(args.case, args.repeats)), flush=True)
        return
    lines = [f"device {torch.cuda.get_device_name(0)}; host path on {torch.get_num_threads()} torch CPU threads (numpy / scipy: "
             f"one); wall-clock medians of {args.repeats} calls after one warm-up, synchronized"]
    for tag in CASES:
        cmd = ["timeout", "-k", "10", str(CASE_TIMEOUT), sys.executable, os.path.abspath(__file__), "--case", tag, "--repeats",
               str(args.repeats)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines.append(done.stdout.rstrip())
        print(done.stdout, flush=True)
        if done.returncode != 0:
            lines.append(f"[{tag}] ended with status {done.returncode}; nothing more is run")
            print(lines[-1], flush=True)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if done.returncode != 0:
        raise SystemExit(done.returncode)


if __name__ == "__main__":
    main()
