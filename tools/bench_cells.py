"""Cell-instance F1 evaluation on one MI355X (K27, csrc/cells.hip) against the host path, on synthetic microscopy images of
tests/_cell_cases.py with about 400 cells each: 1024 x 1024, 4000 x 4000, and 5200 x 5200 (above the 25 M-pixel switch: scored tile
by tile), thresholds 0.5 and 0.1 (the second one needs the matching).

    python tools/bench_cells.py [--repeats 5] [--out profiles/cells_k27_vs_host.log]

Reports per image:
  - the K27 time of one case_cell_metrics call from device events around the whole call (every read-back and the host's matching
    included), and each phase from the library's per-kernel event timers;
  - the algorithmic bytes (seg read twice, gt and both int32 maps read and written once per pass) over 6.29 TB/s of HBM;
  - the host path's time (scipy.ndimage.label, numpy, linear_sum_assignment) with the threads stated;
  - that device and host return identical dicts."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import cells as CL  # noqa: E402
from mlagg_unet_amd import profiling  # noqa: E402
from tests import _cell_cases as C  # noqa: E402

HBM = 6.29e12
PHASES = ["cl_local_kernel", "cl_merge_kernel", "cl_compress_kernel", "cl_flag_kernel", "cl_scan (count + offsets + apply)",
          "cl_rewrite_kernel", "cl_overlap_kernel", "cl_match_kernel"]
THRESHOLDS = (0.5, 0.1)
IMAGES = (((1024, 1024), 400, 1), ((4000, 4000), 400, 2), ((5200, 5200), 400, 3))


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
    return {k: got.get(k, {"ms": 0.0})["ms"] / repeats for k in PHASES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cells needs the MI355X")
    threads = os.environ.get("OMP_NUM_THREADS", "unset")
    lines = [f"device {torch.cuda.get_device_name(0)}; host path: scipy.ndimage.label + numpy + linear_sum_assignment "
             f"(single-threaded), OMP_NUM_THREADS={threads}; thresholds {THRESHOLDS}; device times: median (min-max) of "
             f"{args.repeats} calls after one warm-up, events around the whole call; phases: the library's kernel timers, summed over "
             f"the launches of one call"]
    for shape, n, seed in IMAGES:
        gt, seg = C.cells_image(shape, n, seed)
        dgt, dseg = torch.from_numpy(gt).to("cuda"), torch.from_numpy(seg).to("cuda")
        call = lambda: CL.case_cell_metrics(dgt, dseg, THRESHOLDS)  # noqa: E731
        before = dict(CL.PATH_COUNTS)
        got = call()
        took = {k: CL.PATH_COUNTS[k] - before[k] for k in before}
        med, lo, hi = device_ms(call, args.repeats)
        ph = phase_ms(call, args.repeats)
        kern = sum(ph.values())
        px = gt.size
        nbytes = px * (2 * seg.itemsize + 4 + 3 * 4 + 2 * (4 + 4) + 2 * 4)      # label: seg x2, gt, parent w/r/w; relabels; overlap
        t0 = time.perf_counter()
        want = CL.case_cell_metrics(gt, seg, THRESHOLDS)
        host_s = time.perf_counter() - t0
        tiled = px >= CL.LARGE_IMAGE_PIXELS
        lines.append(f"[case_cell_metrics] {shape[0]} x {shape[1]}, gt {gt.dtype}, seg {seg.dtype}, {got[0]['true_num']} gt / "
                     f"{got[0]['pred_num']} predicted cells counted, {'tiled (2000 x 2000)' if tiled else 'whole image'}")
        lines.append(f"  K27: whole call {med:.3f} ms ({lo:.3f}-{hi:.3f}); phases " +
                     ", ".join(f"{k.split()[0].replace('_kernel', '')} {ph[k]:.3f}" for k in PHASES) + f" ms (sum {kern:.3f})")
        lines.append(f"  tp found from the edge count {took['edge_count']} times, from the matching {took['matching']} times per call")
        lines.append(f"  algorithmic bytes {nbytes / 1e9:.3f} GB -> HBM bound {nbytes / HBM * 1e3:.3f} ms = "
                     f"{nbytes / HBM * 1e3 / kern * 100:.1f}% of the summed phase time")
        lines.append(f"  host path: {host_s:.2f} s ({host_s * 1e3 / med:.0f}x the device call)")
        lines.append(f"  device == host: {got == want}; F1 " + ", ".join(f"{r['F1']} at {r['threshold']}" for r in got))
        if got != want:
            raise SystemExit("\n".join(lines) + "\ndevice and host disagree")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
