"""Ensembling and compute_metrics on one MI355X (K28, csrc/ensemble.hip) against the host path and the torch composition, on one
BTCV-sized case: 14 classes, 512 x 512 x 150 voxels, fp32 members.

    python tools/bench_ensemble.py [--members 2] [--repeats 5] [--shape 512 512 150] [--out profiles/ensemble_k28_vs_host.log]

Reports:
  - ensemble_probabilities on the device without and with the mean written: time from device events around the call, the bytes the
    algorithm moves (M K N 4 + N, plus K N 4 with the mean) and GB/s;
  - a device copy of the same number of bytes (torch's copy_ of an fp32 buffer, read + write = the bytes) on the same box, the floor
    the kernel is compared with;
  - the torch composition torch.stack(members).mean(0).argmax(0) on the device;
  - the host path (numpy, the reference's arithmetic), once;
  - compute_metrics of the ensembled labels against a label volume on the device (one K28 launch and the read-back) and on the host;
  - that device and host give the same labels, the same mean bits and the same metrics."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import ensembling as EN  # noqa: E402
from mlagg_unet_amd import evaluation as EV  # noqa: E402

K = 14


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


def make_members(M, shape, seed=0):
    """M softmax volumes (K, *shape) made on the device from seeded logits (the host copy is read back once for the host path)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.softmax(3 * torch.randn((K,) + tuple(shape), generator=g, device="cuda"), 0) for _ in range(M)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", type=int, nargs=3, default=(512, 512, 150))
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble needs the MI355X")
    M, shape = args.members, tuple(args.shape)
    N = int(np.prod(shape))
    members = make_members(M, shape)
    rng = np.random.default_rng(1)
    reference = torch.from_numpy(np.repeat(rng.integers(0, K, size=(N + 63) // 64).astype(np.uint8), 64)[:N].reshape(shape)).cuda()
    lines = [f"device {torch.cuda.get_device_name(0)}; one case of {K} classes x {shape[0]} x {shape[1]} x {shape[2]} = {N} voxels, "
             f"{M} fp32 members; device times: median (min-max) of {args.repeats} calls after one warm-up, events around the whole "
             f"call; OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}"]
    results = {}
    for want_mean in (False, True):
        nbytes = M * K * N * 4 + N + (K * N * 4 if want_mean else 0)
        med, lo, hi = device_ms(lambda: EN.ensemble_probabilities(members, return_probabilities=want_mean), args.repeats)
        results[want_mean] = (nbytes, med)
        lines.append(f"[ensemble_probabilities, mean {'written' if want_mean else 'not written'}] K28: {med:.3f} ms ({lo:.3f}-{hi:.3f}); "
                     f"{nbytes / 1e9:.3f} GB moved -> {nbytes / med / 1e6:.0f} GB/s")
        src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        cmed, clo, chi = device_ms(lambda: dst.copy_(src), args.repeats)
        lines.append(f"  device copy of the same bytes ({src.numel() * 8 / 1e9:.3f} GB read + written): {cmed:.3f} ms ({clo:.3f}-{chi:.3f}) -> "
                     f"{src.numel() * 8 / cmed / 1e6:.0f} GB/s; K28 runs at {cmed / med * 100:.0f}% of the copy's rate")
        del src, dst
    tmed, tlo, thi = device_ms(lambda: torch.stack(members).mean(0).argmax(0), args.repeats)
    lines.append(f"[torch.stack(members).mean(0).argmax(0)] {tmed:.3f} ms ({tlo:.3f}-{thi:.3f}): {tmed / results[False][1]:.1f}x the K28 call "
                 f"without the mean, {tmed / results[True][1]:.1f}x the one with it")
    labels, mean = EN.ensemble_probabilities(members, return_probabilities=True)
    host_members = [m.cpu().numpy() for m in members]
    t0 = time.perf_counter()
    host_labels, host_mean = EN.ensemble_probabilities(host_members, return_probabilities=True)
    host_s = time.perf_counter() - t0
    equal = bool(np.array_equal(labels.cpu().numpy(), host_labels)
                 and np.array_equal(mean.cpu().numpy().view(np.uint32), host_mean.view(np.uint32)))
    lines.append(f"[host path] numpy: {host_s:.2f} s ({host_s * 1e3 / results[True][1]:.0f}x the K28 call with the mean); labels and mean "
                 f"bits equal to the device's: {equal}")
    labs = list(range(K))
    mmed, mlo, mhi = device_ms(lambda: EV.compute_metrics(reference, labels, labs), args.repeats)
    got = EV.compute_metrics(reference, labels, labs)
    ref_host = reference.cpu().numpy()
    t0 = time.perf_counter()
    want = EV.compute_metrics(ref_host, host_labels, labs)
    metrics_s = time.perf_counter() - t0
    same = all(got["metrics"][k][m] == want["metrics"][k][m] or (np.isnan(got["metrics"][k][m]) and np.isnan(want["metrics"][k][m]))
               for k in labs for m in EV.METRIC_KEYS)
    lines.append(f"[compute_metrics, {K} labels] K28: {mmed:.3f} ms ({mlo:.3f}-{mhi:.3f}) with the read-back, {2 * N / 1e9:.3f} GB read -> "
                 f"{2 * N / mmed / 1e6:.0f} GB/s; host path {metrics_s:.2f} s ({metrics_s * 1e3 / mmed:.0f}x); equal: {same}")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not (equal and same):
        raise SystemExit("device and host disagree")


if __name__ == "__main__":
    main()
