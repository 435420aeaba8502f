"""Keep-largest-component postprocessing on one MI355X (K23, csrc/components.hip) against the host path, on the synthetic BTCV-like
prediction of tests/_postprocess_cases.py: (512, 512, 150) uint8, 13 organs as ellipsoids, 600 islands, an edge / corner tie.

    python tools/bench_postprocess.py [--repeats 5] [--cases 6] [--out profiles/postprocess_k23_btcv_vs_host.log]

Reports, for the foreground as a whole (labels 1-13 -> group 1) and per class (label -> label):
  - the K23 time from device events around the whole call (group table upload and workspace allocation included), and each phase
    from the library's per-kernel event timers;
  - the algorithmic bytes of the six phases (label reads, the int32 parent / size arrays, the output) over 6.29 TB/s of HBM;
  - the host path's time (scipy.ndimage.label per group) on this machine's CPU, with the torch / scipy threads stated;
  - the agreement of device and host labels;
and determine_postprocessing over --cases such predictions (seed 0, and seeds 1..n-1 laid over it), all scored against the seed-0
volume, device against host."""
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
from mlagg_unet_amd import postprocessing as PP  # noqa: E402
from mlagg_unet_amd import profiling  # noqa: E402
from tests import _postprocess_cases as C  # noqa: E402

HBM = 6.29e12
PHASES = ["cc_local_kernel", "cc_merge_kernel", "cc_compress_kernel", "cc_size_kernel", "cc_max_kernel", "cc_write_kernel"]


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


def algorithmic_bytes(n):
    """local: labels 1 + parent 4 + size 4 written; compress: parent 4 + 4; size: size 4 (+ parent of the tile roots); max: parent 4;
    write: labels 1 + parent 4 + out 1.  The merge reads only tile faces and is left out: a lower bound."""
    return n * (1 + 8 + 8 + 4 + 4 + 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_postprocess needs the MI355X")
    threads = os.environ.get("OMP_NUM_THREADS", "unset")
    lines = [f"device {torch.cuda.get_device_name(0)}; host path: scipy.ndimage.label (single-threaded), torch on "
             f"{torch.get_num_threads()} threads, OMP_NUM_THREADS={threads}; device times: median (min-max) of {args.repeats} calls "
             f"after one warm-up, events around the whole call; phases: mean of the library's kernel timers"]
    x = C.btcv_like()
    n = x.size
    xd = torch.from_numpy(x).to("cuda")
    for mode, groups in (("foreground as a whole", {label: 1 for label in range(1, 14)}),
                         ("per class", {label: label for label in range(1, 15)})):
        call = lambda: PP._keep_largest_device(xd, groups, 0)  # noqa: E731
        med, lo, hi = device_ms(call, args.repeats)
        ph = phase_ms(call, args.repeats)
        kern = sum(ph.values())
        nbytes = algorithmic_bytes(n)
        got = call()[0].cpu().numpy()
        t0 = time.perf_counter()
        host = PP._keep_largest_host(x, groups, 0)
        host_s = time.perf_counter() - t0
        diff = int((got != host).sum())
        lines.append(f"[{mode}] labels {x.shape} uint8, {len(set(groups.values()))} group(s)")
        lines.append(f"  K23: whole call {med:.3f} ms ({lo:.3f}-{hi:.3f}); phases " +
                     ", ".join(f"{k.replace('_kernel', '')} {v:.3f}" for k, v in ph.items()) + f" ms (sum {kern:.3f})")
        lines.append(f"  algorithmic bytes {nbytes / 1e9:.3f} GB -> HBM bound {nbytes / HBM * 1e3:.3f} ms = "
                     f"{nbytes / HBM * 1e3 / kern * 100:.1f}% of the summed phase time")
        lines.append(f"  host path: {host_s:.2f} s")
        lines.append(f"  device vs host labels: {diff} of {n} voxels differ; {int((host != x).sum())} voxels removed")
        print("\n".join(lines[-5:]), flush=True)
    base = C.btcv_like(seed=0)
    ref = base.copy()
    preds = [C.btcv_like(seed=0)] + [np.where(C.btcv_like(seed=s) > 0, C.btcv_like(seed=s), base) for s in range(1, args.cases)]
    refs = [ref] * args.cases
    labels = list(range(1, 14))
    dp = [torch.from_numpy(p).to("cuda") for p in preds]
    dr = [torch.from_numpy(r).to("cuda") for r in refs]
    PP.determine_postprocessing(dp[:1], dr[:1], labels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dres = PP.determine_postprocessing(dp, dr, labels)
    torch.cuda.synchronize()
    dev_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    hres = PP.determine_postprocessing(preds, refs, labels)
    host_s = time.perf_counter() - t0
    same = json.dumps(dres[2], sort_keys=True) == json.dumps(hres[2], sort_keys=True) and dres[1] == hres[1]
    lines.append(f"[determine_postprocessing] {args.cases} cases of {x.shape}, 13 labels: device {dev_s:.2f} s, host {host_s:.2f} s "
                 f"({host_s / dev_s:.1f}x); same decisions and summary: {same}; steps {dres[1]}")
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
