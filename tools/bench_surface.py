"""Normalized surface Dice on one MI355X (K24, csrc/surface.hip) against the host path, on the BTCV-sized synthetic case of
tests/_surface_cases.py: (512, 512, 150) uint8 gt and prediction, 13 organs, BTCV tolerances and slab organs, spacing
(0.78125, 0.78125, 3.0) mm.

    python tools/bench_surface.py [--repeats 5] [--out profiles/surface_k24_btcv_vs_host.log]

Reports:
  - the K24 time of one case_nsd call from device events around the whole call (both read-backs and the table upload included), and
    each phase from the library's per-kernel event timers;
  - the algorithmic bytes (both volumes read once; per crop voxel the codes, the int32 feature transform written and read by the
    passes) over 6.29 TB/s of HBM;
  - the host path's time (scipy.ndimage.correlate and distance_transform_edt per organ, single-threaded) with the threads stated;
  - the agreement of device and host NSD per organ."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import profiling  # noqa: E402
from mlagg_unet_amd import surface as SF  # noqa: E402
from tests import _surface_cases as C  # noqa: E402

HBM = 6.29e12
PHASES = ["sf_stats_kernel (+ init)", "sf_codes_kernel", "sf_zpass_kernel", "sf_ypass_kernel", "sf_xpass_kernel", "sf_sum_kernel"]
SPACING = (np.float32(0.78125), np.float32(0.78125), np.float32(3.0))


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


def phase_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    profiling.select_all()
    profiling.collect()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    got = profiling.collect()
    profiling.select(None)
    return {k: got[k]["ms"] / max(got[k]["count"], 1) for k in PHASES}


def crop_voxels(gt, seg):
    """voxels of the crops K24 lays out (union boxes + 1, slab organs cut to the gt's z range)"""
    total = 0
    for lab in range(1, 14):
        m = (gt == lab) | (seg == lab)
        if not (gt == lab).any():
            continue
        idx = [np.nonzero(m.any(axis=tuple(a for a in range(3) if a != ax)))[0] for ax in range(3)]
        lo, hi = [int(i[0]) for i in idx], [int(i[-1]) for i in idx]
        if lab in SF.BTCV_SLAB_LABELS:
            z = np.nonzero((gt == lab).any(axis=(0, 1)))[0]
            lo[2], hi[2] = max(lo[2], int(z[0])), min(hi[2], int(z[-1]) - 1)
        total += int(np.prod([h - l + 2 for l, h in zip(lo, hi)]))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface needs the MI355X")
    threads = os.environ.get("OMP_NUM_THREADS", "unset")
    lines = [f"device {torch.cuda.get_device_name(0)}; host path: scipy.ndimage correlate + distance_transform_edt per organ "
             f"(single-threaded), torch on {torch.get_num_threads()} threads, OMP_NUM_THREADS={threads}; device times: median "
             f"(min-max) of {args.repeats} calls after one warm-up, events around the whole call; phases: mean of the library's "
             f"kernel timers"]
    gt, seg = C.btcv_sized_case()
    dgt, dseg = torch.from_numpy(gt).to("cuda"), torch.from_numpy(seg).to("cuda")
    call = lambda: SF.case_nsd(dgt, dseg, SPACING, SF.BTCV_NSD_TOLERANCES, SF.BTCV_SLAB_LABELS)  # noqa: E731
    med, lo, hi = device_ms(call, args.repeats)
    ph = phase_ms(call, args.repeats)
    kern = sum(ph.values())
    v = crop_voxels(gt, seg)
    nbytes = 2 * gt.size + v * (2 + 2 * 4 + 2 * 4 + 2 * 4 + 2 * 1)     # volumes; per crop voxel: codes, ft z / y passes, x-pass reads
    got = call()
    t0 = time.perf_counter()
    want = SF.case_nsd(gt, seg, SPACING, SF.BTCV_NSD_TOLERANCES, SF.BTCV_SLAB_LABELS)
    host_s = time.perf_counter() - t0
    diff = max(abs(got[o] - want[o]) for o in got)
    lines.append(f"[case_nsd] gt / prediction {gt.shape} uint8, 13 BTCV organs, {v} crop voxels in all")
    lines.append(f"  K24: whole call {med:.3f} ms ({lo:.3f}-{hi:.3f}); phases " +
                 ", ".join(f"{k.split()[0].replace('_kernel', '')} {ph[k]:.3f}" for k in PHASES) + f" ms (sum {kern:.3f})")
    lines.append(f"  algorithmic bytes {nbytes / 1e9:.3f} GB -> HBM bound {nbytes / HBM * 1e3:.3f} ms = "
                 f"{nbytes / HBM * 1e3 / kern * 100:.1f}% of the summed phase time")
    lines.append(f"  host path: {host_s:.2f} s ({host_s * 1e3 / med:.0f}x the device call)")
    lines.append(f"  device vs host NSD (rounded to 4 digits): max |difference| {diff:.1e} over {len(got)} organs")
    lines.append("  NSD: " + ", ".join(f"{o} {got[o]}" for o in got))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
