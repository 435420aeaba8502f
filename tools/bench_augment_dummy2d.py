"""Spatial transform of the dummy-2-D augmentation at an ACDC-like 3d_fullres plan (batch 4, 1 channel, loader patch 20x301x301 ->
20x256x224, 4 labels and the -1 padding, every sample rotated -- one near pi / 2 -- and scaled): the in-plane prefilter plus K31
(augmentation3d.spatial_transform_dummy_2d) against the same result composed from the 2-D chain's functions on the device
(augmentation.spatial_transform with the slices folded into the batch axis: prefilter, one gather of all taps, per-label
indicators).  Five repeated runs of each, alternating in one process; the spread is max - min of a path's five medians.
    python tools/bench_augment_dummy2d.py [--iters 10] [--repeats 5]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import augmentation as A2  # noqa: E402
from mlagg_unet_amd import augmentation3d as AUG3  # noqa: E402

PATCH, B, N_CLS = (20, 256, 224), 4, 4
ANGLES, SCALES = (1.55, -2.9, 0.6, 2.3), (0.74, 1.37, 1.1, 0.9)


def batch(init, dev, n=B, seed=0):
    rng = np.random.RandomState(seed)
    x, y, z = np.meshgrid(*[np.arange(m, dtype=np.float32) for m in init], indexing="ij", sparse=True)
    data = np.stack([5 * np.sin(y / 6 + b + x) * np.cos(z / 9) + rng.randn(*init).astype(np.float32) * 0.1 for b in range(n)])[:, None]
    f = (np.sin(x / 3) + np.cos(y / 17 + 1) + np.sin(z / 11) + 3) / 6
    seg = np.stack([np.floor(np.clip(f + 0.03 * b, 0, 0.999) * N_CLS) for b in range(n)])[:, None].astype(np.int16)
    seg[:, :, :, :6] = -1
    return torch.from_numpy(data.astype(np.float32)).to(dev), torch.from_numpy(seg).to(dev)


def params(n=B):
    p = AUG3.draw_params_dummy_2d(np.random.RandomState(0), n, 1)
    p["do_rot"][:], p["do_scale"][:] = True, True
    p["angle"][:], p["scale"][:] = ANGLES[:n], SCALES[:n]
    return p


def composition(data, seg, patch, p, labels):
    """The yardstick: augmentation.spatial_transform (the 2-D chain's device path) on the batch with every slice as a sample."""
    Bn, C, X, Yi, Zi = data.shape
    dev = data.device
    T = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a), device=dev).to(dt)      # noqa: E731
    d2 = data.transpose(1, 2).reshape(Bn * X, C, Yi, Zi)
    s2 = seg.to(torch.float32).transpose(1, 2).reshape(Bn * X, 1, Yi, Zi)
    rep = lambda a, dt=torch.float32: T(a, dt).repeat_interleave(X)                       # noqa: E731
    out_d, out_s = A2.spatial_transform(d2, s2, patch[1:], rep(p["do_rot"] | p["do_scale"], torch.bool), rep(p["angle"] * p["do_rot"]),
                                        rep(np.where(p["do_scale"], p["scale"], 1.0)), labels)
    return (out_d.view(Bn, X, C, *patch[1:]).transpose(1, 2).contiguous(), out_s.view(Bn, X, 1, *patch[1:]).transpose(1, 2).contiguous())


def timed(fn, n, sync):
    fn()
    sync()
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms))


def measure(dev, patch, iters, repeats, n=B):
    dev = torch.device(dev)
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    rotation, dummy, init, _ = AUG3.configure_3d(patch)
    assert dummy
    data, seg = batch(init, dev, n)
    p = params(n)
    labels = torch.tensor([-1.0] + [float(v) for v in range(N_CLS)], device=dev)
    k31 = lambda: AUG3.spatial_transform_dummy_2d(data, seg, patch, p, labels.cpu())      # noqa: E731
    comp = lambda: composition(data, seg, patch, p, labels)                              # noqa: E731
    (d1, s1), (d2, s2) = k31(), comp()
    agree = {"data_max_abs_diff": float((d1 - d2).abs().max()), "label_voxels_differing_share": float((s1 != s2).float().mean())}
    del d1, s1, d2, s2
    runs = {"k31_path": [], "composition": []}
    for _ in range(repeats):
        runs["k31_path"].append(timed(k31, iters, sync))
        runs["composition"].append(timed(comp, iters, sync))
    pieces = {}
    if dev.type == "cuda":
        from mlagg_unet_amd import ops
        A, do = AUG3.affines(p, init[1:], patch[1:])
        vol = AUG3._prefiltered(data, do, 2)
        pieces["prefilter_ms"] = round(timed(lambda: A2.spline_coefficients(data), iters, sync), 3)
        pieces["k31_kernel_ms"] = round(timed(lambda: ops.aug3d_resample_planar(vol, seg, A, do, patch[1:]), iters, sync), 3)
        nbytes = n * int(np.prod(init)) * (4 + 2) + n * int(np.prod(patch)) * (4 + 4)
        pieces["k31_bytes_if_input_read_once"] = nbytes
        pieces["k31_GBs_vs_that"] = round(nbytes / (pieces["k31_kernel_ms"] * 1e-3) / 1e9, 1)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    gain = med["composition"] - med["k31_path"]
    return {"workload": f"dummy-2-D spatial transform, batch {n}, {'x'.join(map(str, init))} -> {'x'.join(map(str, patch))}, {N_CLS} labels",
            "angles": list(ANGLES[:n]), "scales": list(SCALES[:n]), "kernel_form": "plain (no LDS staging), 8x8 output tile per wave",
            "k31_path_ms": round(med["k31_path"], 3), "composition_ms": round(med["composition"], 3),
            "k31_path_runs_ms": [round(v, 3) for v in runs["k31_path"]], "composition_runs_ms": [round(v, 3) for v in runs["composition"]],
            "spread_ms": {k: round(v, 3) for k, v in spread.items()}, "speedup": round(med["composition"] / med["k31_path"], 2),
            "faster_by_more_than_the_spread": bool(gain > max(spread.values())), "agreement": agree, **pieces}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment_dummy2d: needs the GPU (K31 has no host timing worth reporting)")
    print(json.dumps(measure("cuda:0", PATCH, a.iters, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
