"""Prediction export on one MI355X (K21, csrc/export.hip) against the host path, on two BTCV-like cases with K = 14.

    python tools/bench_export.py [--repeats 5] [--out profiles/export_k21_btcv_vs_host.log]

  (a) anisotropic: logits (96, 320, 320) at spacing (3.0, 1.0, 1.0) into (148, 512, 512) at (2.5, 0.76, 0.76): separate z;
  (b) isotropic:   logits (160, 192, 192) at 1.5 mm into (240, 360, 360) at 1.0 mm inside (260, 512, 512): trilinear.
Reports the K21 time from device events around the whole call (table build and upload included) and of export_kernel alone (the
library's per-kernel event timers), labels only and with probabilities; the algorithmic bytes (read K * in * 4, write out * 1,
+ K * out * 4 with probabilities) over 6.29 TB/s of HBM; the host path's time on this machine's CPU (labels only, torch threads
stated), standing in for the reference's CPU export; the bytes that leave the device before (logits) and after (labels); and the
agreement of device and host labels."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import export as E  # noqa: E402
from mlagg_unet_amd import profiling  # noqa: E402

HBM = 6.29e12
K = 14
CASES = {
    "a_anisotropic": dict(shape=(96, 320, 320), cfg=(3.0, 1.0, 1.0), spacing=(2.5, 0.76, 0.76), full=(148, 512, 512), lo=(0, 0, 0),
                          crop=(148, 512, 512)),
    "b_isotropic": dict(shape=(160, 192, 192), cfg=(1.5, 1.5, 1.5), spacing=(1.0, 1.0, 1.0), full=(260, 512, 512), lo=(10, 76, 76),
                        crop=(240, 360, 360)),
}


def props(c):
    return {"spacing": list(c["spacing"]), "shape_before_cropping": c["full"],
            "bbox_used_for_cropping": [[a, a + s] for a, s in zip(c["lo"], c["crop"])],
            "shape_after_cropping_and_before_resampling": c["crop"]}


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


def kernel_ms(fn, repeats):
    """export_kernel alone, from the library's own HIP-event timers (mean over `repeats` launches)"""
    fn()
    torch.cuda.synchronize()
    profiling.select("export_kernel")
    profiling.collect()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    got = profiling.collect()["export_kernel"]
    profiling.select(None)
    return got["ms"] / got["count"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_export needs the MI355X")
    lines = [f"device {torch.cuda.get_device_name(0)}; host path on {torch.get_num_threads()} torch CPU threads; K = {K}; "
             f"device times: median (min-max) of {args.repeats} calls after one warm-up, events around the whole call"]
    for tag, c in CASES.items():
        p = props(c)
        x = torch.randn((K,) + c["shape"], generator=torch.Generator().manual_seed(21)) * 3
        xd = x.to("cuda")
        sep, axis = E.separate_z_decision(E.current_spacing_for(c["cfg"], p), c["spacing"])
        n_in = x[0].numel()
        n_out = c["full"][0] * c["full"][1] * c["full"][2]
        res = {}
        for probs in (False, True):
            call = lambda: E.convert_predicted_logits_to_segmentation_with_correct_shape(xd, p, c["cfg"],  # noqa: E731
                                                                                        return_probabilities=probs)
            med, lo, hi = device_ms(call, args.repeats)
            nbytes = K * n_in * 4 + n_out + (K * n_out * 4 if probs else 0)
            res[probs] = (med, lo, hi, kernel_ms(call, args.repeats), nbytes)
        seg, _ = E.convert_predicted_logits_to_segmentation_with_correct_shape(xd, p, c["cfg"])
        t0 = time.perf_counter()
        hseg, _ = E.convert_predicted_logits_to_segmentation_with_correct_shape(x, p, c["cfg"])
        host_s = time.perf_counter() - t0
        diff = int((seg.cpu() != hseg).sum())
        lines.append(f"[{tag}] logits {(K,) + c['shape']} -> {c['crop']} in {c['full']}; separate_z={sep} axis={axis}")
        for probs, (med, lo, hi, kern, nbytes) in res.items():
            bound = nbytes / HBM * 1e3
            lines.append(f"  K21 {'labels+probabilities' if probs else 'labels only'}: whole call {med:.3f} ms ({lo:.3f}-{hi:.3f}), "
                         f"export_kernel {kern:.3f} ms; algorithmic bytes {nbytes / 1e9:.3f} GB -> HBM bound {bound:.3f} ms = "
                         f"{bound / kern * 100:.1f}% of the kernel time ({nbytes / kern / 1e6:.0f} GB/s)")
        lines.append(f"  host path (labels only): {host_s:.2f} s on {torch.get_num_threads()} threads")
        lines.append(f"  to the host: logits {K * n_in * 4 / 1e6:.1f} MB before, labels {n_out / 1e6:.1f} MB after")
        lines.append(f"  device vs host labels: {diff} of {n_out} voxels differ")
        print("\n".join(lines[-6:]), flush=True)
        del xd, seg
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
