"""3-D sliding-window inference on one MI355X: the BTCV-shaped UMambaEnc (model3d.BTCV_STRIDES, 14 classes, 96x160x160 tiles) over
a (1, 128, 256, 256) volume, 18 tiles x 8 mirror variants.  Reports total time, network-forward time and the gather + fold +
finalize time of the K20 path (csrc/sliding_window.hip), peak device memory for the K20 path and for the torch composition of the
same order (inference._sliding_window_3d_torch), and how far the two results are apart.
    timeout -k 10 900 python tools/bench_inference_3d.py [--volume 128 256 256] [--mirror 0 1 2] [--tile-batch 1] [--repeats 2]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import inference as PI  # noqa: E402
from mlagg_unet_amd import model3d, profiling  # noqa: E402

TILE = (96, 160, 160)


class TimedNet(torch.nn.Module):
    """Records HIP events around every forward: the network's share of the wall time."""

    def __init__(self, net):
        super().__init__()
        self.net, self.events = net, []

    def forward(self, x):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = self.net(x)
        b.record()
        self.events.append((a, b))
        return y

    def forward_ms(self):
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b in self.events)
        self.events = []
        return ms


def torch_path(net, image, K, mirror, tile_batch, dev):
    """The torch composition of the same order on the device (the A side): pad, chunks, flips, fold by slices, divide, crop."""
    flips = PI.mirror_variants(mirror)
    data, revert = PI._pad_to_tile(image, TILE)
    data = data.to(dev).contiguous()
    g = PI.compute_gaussian(TILE).to(dev)
    steps = PI.compute_steps_for_sliding_window(tuple(data.shape[1:]), TILE, 0.5)
    places = [(sx, sy, sz) for sx in steps[0] for sy in steps[1] for sz in steps[2]]
    acc, w = PI._sliding_window_3d_torch(net, data, g, places, flips, TILE, tile_batch, K)
    acc /= w
    return acc[(slice(None), *revert)].contiguous()


def run(name, fn, tnet, repeats):
    best = None
    for _ in range(repeats):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        fwd = tnet.forward_ms()
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        if best is None or total < best["total_ms"]:
            best = {"path": name, "total_ms": round(total, 1), "forward_ms": round(fwd, 1),
                    "outside_forward_ms": round(total - fwd, 1), "peak_MiB_above_weights": round(peak, 1)}
        del out
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", type=int, nargs=3, default=(128, 256, 256))
    ap.add_argument("--mirror", type=int, nargs="*", default=(0, 1, 2))
    ap.add_argument("--tile-batch", type=int, default=1)
    ap.add_argument("--classes", type=int, default=14)
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = len(model3d.BTCV_STRIDES)
    net = model3d.build_network_architecture_3d(1, a.classes, [[3, 3, 3]] * n, model3d.BTCV_STRIDES, [2] * n, [2] * (n - 1),
                                                enable_deep_supervision=False).to(dev).eval()
    tnet = TimedNet(net).eval()
    image = torch.rand((1,) + tuple(a.volume), generator=torch.Generator().manual_seed(0))
    mirror = tuple(a.mirror) or None
    steps = PI.compute_steps_for_sliding_window(tuple(max(v, t) for v, t in zip(a.volume, TILE)), TILE, 0.5)
    ntiles = len(steps[0]) * len(steps[1]) * len(steps[2])
    V = len(PI.mirror_variants(mirror))
    print(f"volume {tuple(a.volume)}, tile {TILE}, {ntiles} tiles x {V} mirror variants, tile_batch {a.tile_batch} "
          f"(network batch {a.tile_batch * V}), {a.classes} classes", flush=True)
    with torch.no_grad():
        hip = lambda: PI.predict_sliding_window_return_logits(tnet, image, a.classes, TILE, mirror, tile_batch=a.tile_batch)  # noqa: E731
        ref = lambda: torch_path(tnet, image, a.classes, mirror, a.tile_batch, dev)                                          # noqa: E731
        hip()                                                                          # warm-up: kernels, workspaces, MIOpen
        tnet.forward_ms()
        rows = [run("K20 kernels", hip, tnet, a.repeats), run("torch composition", ref, tnet, a.repeats)]
        # the K20 launches' own time, in a separate run with the library's per-kernel event timers on
        profiling.select_all()
        hip()
        torch.cuda.synchronize()
        prof = profiling.collect()
        profiling.select(None)
        tnet.forward_ms()
        rows[0]["gather_fold_finalize_ms"] = round(sum(prof.get(k, {"ms": 0})["ms"] for k in
                                                       ("sw_gather_kernel", "sw_fold_kernel", "sw_finalize_kernel")), 2)
        rows[0]["launches"] = {k: prof[k]["count"] for k in ("sw_gather_kernel", "sw_fold_kernel", "sw_finalize_kernel") if k in prof}
        x, y = hip(), ref()
        tnet.forward_ms()
        diff = float((x - y).abs().max())
        agree = {"max_abs_diff": diff, "bit_identical": bool(torch.equal(x, y)), "contiguous": bool(x.is_contiguous())}
    for r in rows:
        print(json.dumps(r), flush=True)
    print(json.dumps({"agreement": agree}), flush=True)
    if diff > 1e-5:
        raise SystemExit(f"the two paths disagree: max |diff| = {diff}")


if __name__ == "__main__":
    main()
