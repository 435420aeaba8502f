"""Throughput of the 3-D real-data input path at the BTCV plan (batch 2, loader patch 191x257x219 -> 96x160x160, 14 labels):
the pieces of augmentation3d.GpuAugmenter3D (prefilter, K25 resample with both samples rotated and scaled, one low-resolution
channel) and the whole device chain per batch with the H2D copy of the crops.  With --train-steps the 3-D train step
(model3d.UMambaEnc, bench.py --config 4's recipe) fed by PrefetchLoader + DataLoader3D + GpuAugmenter3D against the same step on
a resident synthetic batch, A/B in one process.  The CPU figure is tests/perf/augmentation_3d_cpu_baseline.py.
    python tools/bench_input_path_3d.py [--batches 20] [--train-steps 10]
Prints one JSON line."""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import augmentation as AUG  # noqa: E402
from mlagg_unet_amd import augmentation3d as AUG3  # noqa: E402
from mlagg_unet_amd import dataloading as DL  # noqa: E402
from mlagg_unet_amd import ops  # noqa: E402

PATCH, B, N_CLS = (96, 160, 160), 2, 14
HBM_PEAK_GBS = 8000.0


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def host_batch(init, seed=0):
    rng = np.random.RandomState(seed)
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in init], indexing="ij", sparse=True)
    data = np.stack([5 * np.sin(x / 6 + b) * np.cos(y / 9) + rng.randn(*init).astype(np.float32) * 0.1 for b in range(B)])[:, None]
    f = (np.sin(x / 13) + np.cos(y / 17 + 1) + np.sin(z / 11) + 3) / 6
    seg = np.stack([np.floor(np.clip(f + 0.03 * b, 0, 0.999) * N_CLS) for b in range(B)])[:, None].astype(np.int16)
    seg[:, :, :, :6] = -1
    return torch.from_numpy(data.astype(np.float32)).pin_memory(), torch.from_numpy(seg).pin_memory()


def write_cases(folder, shape=(200, 300, 280), n=3):
    """Raw-sized BTCV-like cases (unpacked .npy + class_locations) for the loader-fed train step."""
    rng = np.random.RandomState(0)
    for i in range(n):
        data = rng.randn(1, *shape).astype(np.float32)
        seg = np.zeros((1, *shape), dtype=np.int16)
        for lab in range(1, N_CLS):
            c = [rng.randint(10, s - 40) for s in shape]
            seg[0, c[0]:c[0] + 30, c[1]:c[1] + 30, c[2]:c[2] + 30] = lab
        locs = {lab: np.argwhere(seg == lab)[rng.choice(int((seg == lab).sum()), 2000, replace=False)] for lab in range(1, N_CLS)}
        np.save(os.path.join(folder, f"case_{i:03d}.npy"), data)
        np.save(os.path.join(folder, f"case_{i:03d}_seg.npy"), seg)
        np.savez(os.path.join(folder, f"case_{i:03d}.npz"), data=data[:, :1, :1, :1], seg=seg[:, :1, :1, :1])
        with open(os.path.join(folder, f"case_{i:03d}.pkl"), "wb") as fh:
            pickle.dump({"class_locations": locs}, fh)


def train_ab(steps, warmup):
    from mlagg_unet_amd import model3d, trainer
    dev = torch.device("cuda:0")
    strides = model3d.BTCV_STRIDES
    n = len(strides)
    torch.manual_seed(0)
    net = model3d.build_network_architecture_3d(1, N_CLS, [[3, 3, 3]] * n, strides, [2] * n, [2] * (n - 1)).to(dev).train()
    opt = torch.optim.SGD(net.parameters(), 1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)
    data, target = model3d.synthetic_batch_3d(B, 1, PATCH, strides, N_CLS, seed=1234, device=dev)
    folder = tempfile.mkdtemp()
    write_cases(folder)
    aug = AUG3.GpuAugmenter3D(PATCH, dev, seed=0, labels=list(range(N_CLS)))
    dl = DL.DataLoader3D(DL.Dataset(folder), B, aug.initial_patch_size(), PATCH, list(range(N_CLS)), 0.33)
    feed = DL.PrefetchLoader(dl, dev, num_workers=4, depth=4, augmenter=aug, ds_scales=model3d.deep_supervision_scales(strides))

    def run(fed):
        for _ in range(warmup):
            d, t = feed.next() if fed else (data, target)
            trainer.train_step(net, opt, d, t, batch_dice=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            d, t = feed.next() if fed else (data, target)
            loss = trainer.train_step(net, opt, d, t, batch_dice=False)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps, float(loss)
    try:
        out = {}
        for tag, fed in (("resident_a", False), ("loader_fed", True), ("resident_b", False)):
            ms, loss = run(fed)
            out[tag] = {"ms_per_step": round(ms, 2), "final_loss": round(loss, 4)}
        return out
    finally:
        feed.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=0)
    ap.add_argument("--train-warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    aug = AUG3.GpuAugmenter3D(PATCH, dev, seed=0, labels=list(range(N_CLS)))
    init = aug.initial_patch_size()
    data_h, seg_h = host_batch(init)
    data, seg = data_h.to(dev), seg_h.to(dev)
    p = AUG3.draw_params_3d(np.random.RandomState(0), B, 1)
    p["do_rot"][:], p["do_scale"][:] = True, True
    p["angle"][:] = [[0.41, -0.27, 0.33], [-0.5, 0.19, -0.44]]
    p["scale"][:] = [0.74, 1.37]
    A, do = AUG3.affines(p, init, PATCH)
    vol = AUG3._prefiltered(data, do)
    prefilter_ms = timed(lambda: AUG.spline_coefficients(data, 3), a.batches)
    k25_ms = timed(lambda: ops.aug3d_resample(vol, seg, A, do, PATCH), a.batches)
    crop = np.zeros(B, dtype=bool)
    k25_crop_ms = timed(lambda: ops.aug3d_resample(data, seg, A, crop, PATCH), a.batches)
    small = torch.randn(1, 1, *PATCH, device=dev)
    lowres_ms = timed(lambda: AUG3.simulate_low_resolution_3d(small, np.ones((1, 1), bool), np.full((1, 1), 0.75)), a.batches)
    batch = {"data": data_h, "seg": seg_h}
    drawn_ms = timed(lambda: DL.to_device(batch, dev, augmenter=aug, ds_scales=[[1, 1, 1], [.5, .5, .5]]), a.batches)
    forced = AUG3.GpuAugmenter3D(PATCH, dev, labels=list(range(N_CLS)))
    q = {k: (v.copy() if k.startswith("do_") else v) for k, v in p.items()}
    for k in q:
        if k.startswith("do_"):
            q[k][:] = True
    q["blur_ch"][:], q["lowres_ch"][:] = True, True
    q["lowres_zoom"][:], q["blur_sigma"][:] = 0.75, 1.0

    def all_on():
        d = batch["data"].to(dev, non_blocking=True)
        s = batch["seg"].to(dev, non_blocking=True)
        return forced.apply(d, s, q)
    forced_ms = timed(all_on, max(3, a.batches // 4))
    Xi, Yi, Zi = init
    nbytes = B * Xi * Yi * Zi * (4 + 2) + B * int(np.prod(PATCH)) * (4 + 4)
    line = {"workload": "3-D augmentation chain B:666-701, batch 2, 191x257x219 -> 96x160x160, 14 labels", "initial_patch": list(init),
            "prefilter_ms": round(prefilter_ms, 3), "prefilter": "33-tap band-matrix GEMM per axis (torch.matmul)",
            "k25_resample_ms": round(k25_ms, 3), "k25_crop_ms": round(k25_crop_ms, 3),
            "k25_bytes_if_input_read_once": nbytes, "k25_GBs_vs_that": round(nbytes / (k25_ms * 1e-3) / 1e9, 1),
            "hbm_peak_GBs": HBM_PEAK_GBS, "lowres_one_channel_zoom_0_75_ms": round(lowres_ms, 3),
            "chain_drawn_params_with_h2d_ms_per_batch": round(drawn_ms, 3),
            "chain_every_transform_on_with_h2d_ms_per_batch": round(forced_ms, 3)}
    if a.train_steps:
        line["train_step_ab"] = train_ab(a.train_steps, a.train_warmup)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
