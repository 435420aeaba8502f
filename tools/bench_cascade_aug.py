"""The cascade transforms of a training batch on one MI355X (K30, csrc/cascade_aug.hip, behind augmentation3d.cascade_transforms)
against the host scipy path, at the BTCV plan: 2 samples, 13 labels, patch (96, 160, 160); the previous stage's segmentation is a
synthetic one of 13 ellipsoid organs with a few islands.

    python tools/bench_cascade_aug.py [--repeats 5] [--cases drawn,worst] [--no-host] [--out profiles/cascade_aug_k30_btcv.log]

Two cases:
  drawn  a parameter sequence of draw_cascade_params (the first seed whose two samples both draw the morphology) with the component
         removal fired on both samples;
  worst  every channel of both samples closed with ball(8.0), the removal fired on both samples.
Reports the time of the whole call (events around cascade_transforms: the host's footprints and run tables, packing, every launch,
the read-backs of the removal, unpacking) and, apart, the host's share for the footprints and run tables (cascade_plan), the
host path's time with the samples on a pool of --threads threads (scipy's binary morphology itself is single-threaded and the
"was added" rule orders a sample's channels), and whether both give the same channels."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import augmentation3d as AUG3  # noqa: E402

SHAPE, B, L = (96, 160, 160), 2, 13


def btcv_like_previous_stage(seed):
    rng = np.random.RandomState(seed)
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in SHAPE], indexing="ij", sparse=True)
    seg = np.zeros(SHAPE, dtype=np.int16)
    for lab in range(1, L + 1):
        c = [rng.uniform(0.2, 0.8) * n for n in SHAPE]
        r = [rng.uniform(0.06, 0.16) * n for n in SHAPE]
        seg[((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2 <= 1] = lab
        for _ in range(4):                                                    # islands
            o = [rng.randint(0, n - 4) for n in SHAPE]
            seg[o[0]:o[0] + 3, o[1]:o[1] + 3, o[2]:o[2] + 3] = lab
    return seg


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default="drawn,worst")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true", help="device times only (the host's worst case takes minutes)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cascade_aug needs the MI355X")
    labels = list(range(1, L + 1))
    seg = np.stack([btcv_like_previous_stage(s) for s in range(B)])
    seg_d = torch.from_numpy(seg).cuda()
    data = torch.zeros((B, 1) + SHAPE)
    data_d = data.cuda()
    seed = next(s for s in range(999) if all(AUG3.draw_cascade_params(np.random.RandomState(s), B, L, list(range(L)))))
    cases = {"drawn": AUG3.draw_cascade_params(np.random.RandomState(seed), B, L, list(range(L))),
             "worst": [[(c, 2, 8.0) for c in range(L)] for _ in range(B)]}
    lines = [f"device {torch.cuda.get_device_name(0)}; {B} samples x {L} labels x {SHAPE}; device: median (min-max) of {args.repeats} "
             f"calls after one warm-up; host: scipy.ndimage, the samples on {args.threads} threads, OMP_NUM_THREADS="
             f"{os.environ.get('OMP_NUM_THREADS', 'unset')}"]
    for name in args.cases.split(","):
        params = cases[name]
        kw = dict(p_per_sample=2.0)                                           # uniform() < 2: the removal fires on every sample
        call = lambda: AUG3.cascade_transforms(data_d, seg_d, labels, params, np.random.RandomState(1), **kw)  # noqa: E731
        med, lo, hi = device_ms(call, args.repeats)
        got = call()[:, 1:].cpu().numpy()
        n_ops = sum(len(s) for s in params)
        radii = [r for s in params for _, _, r in s]
        lines.append(f"[{name}] {n_ops} operations, radii {min(radii):.2f}-{max(radii):.2f} (mean {np.mean(radii):.2f}), "
                     f"{sum(op >= 2 for s in params for _, op, _ in s)} of them closings / openings")
        plan = []
        for _ in range(args.repeats + 1):
            t0 = time.perf_counter()
            table = AUG3.cascade_plan(params)[1]
            plan.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"  K30, whole call: {med:.2f} ms ({lo:.2f}-{hi:.2f}); {int(got.sum())} voxels set in the {B * L} channels")
        lines.append(f"  of which on the host, before the first morphology launch: footprints and run tables ({len(table)} runs) "
                     f"{sorted(plan)[len(plan) // 2]:.2f} ms")
        if not args.no_host:
            def one(b):
                rng = np.random.RandomState(1)
                return AUG3.cascade_transforms(data[b:b + 1], torch.from_numpy(seg[b:b + 1]), labels, [params[b]], rng, **kw)
            t0 = time.perf_counter()
            with ThreadPoolExecutor(args.threads) as pool:
                list(pool.map(one, range(B)))
            host_s = time.perf_counter() - t0
            lines.append(f"  host path: {host_s:.2f} s ({host_s * 1e3 / med:.0f}x the device time)")
            if name == "drawn":                                               # one stream over both samples: the same draws as the device
                want = AUG3.cascade_transforms(data, torch.from_numpy(seg), labels, params, np.random.RandomState(1), **kw)
                lines.append(f"  device vs host: {int((want[:, 1:].numpy() != got).sum())} of {got.size} channel voxels differ")
        print("\n".join(lines[-5:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
