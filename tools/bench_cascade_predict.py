"""The cascade's hand-off at prediction time on one MI355X: the input path of a cascaded stage (K32, csrc/sliding_window.hip) against
the explicit one-hot volume through the existing gather, and resample_logits_to_next_stage (K21) against the host path.

    python tools/bench_cascade_predict.py [--repeats 3] [--out profiles/cascade_predict_k32_btcv.log]

BTCV-like case: 1 image channel, 13 foreground labels, a preprocessed volume of 200 x 320 x 320, tile 96 x 160 x 160 at step 0.5 (36
tiles), 8 mirror variants, one tile per network call.  The network is ONE 1 x 1 x 1 convolution (14 -> 14): a stand-in that costs next
to nothing, so that what is timed is the input path, the fold and the finalize.  Both paths run the same sliding window on the same
inputs and must give the same logits:
  K32       predict_sliding_window_return_logits(image, previous_stage_seg=seg (uint8), cascade_labels=1 .. 13);
  explicit  the same call on cat(image, one_hot(seg)): the reference's np.vstack((data, seg_onehot)), 4 * 14 * X * Y * Z bytes.
Reported per path: the time of the whole call (device events, median (min-max) after one warm-up), the rise of
torch.cuda.max_memory_allocated() over the call, and the gather kernel's own time from the library's event timers.  The explicit
path's figures include building the stack, as a caller without K32 has to.
Then the hand-off out of the low-resolution stage: logits (14, 96, 160, 160) -> uint8 labels (200, 320, 320) on the device and on this
machine's CPU (torch threads stated), and the number of labels that differ."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import export as E  # noqa: E402
from mlagg_unet_amd import inference, profiling  # noqa: E402

C, L, HEADS = 1, 13, 14
VOLUME, TILE = (200, 320, 320), (96, 160, 160)
LOWRES, LOWRES_SPACING = (96, 160, 160), (3.0, 1.5, 1.5)


def measure(fn, repeats):
    """-> (result, median / min / max ms of the whole call, peak rise in bytes)"""
    out = fn()
    torch.cuda.synchronize()
    del out
    times, rise = [], 0
    for r in range(repeats):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
        rise = max(rise, torch.cuda.max_memory_allocated() - before)
        if r < repeats - 1:
            del out
    times.sort()
    return out, (times[len(times) // 2], times[0], times[-1]), rise


def kernel_ms(fn, name):
    """total time of kernel `name` over one call, from the library's own HIP-event timers"""
    profiling.select(name)
    profiling.collect()
    fn()
    torch.cuda.synchronize()
    got = profiling.collect()[name]
    profiling.select(None)
    return got["ms"], got["count"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cascade_predict needs the MI355X")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(32)
    image = torch.randn((C,) + VOLUME, generator=g).to(dev)
    seg = torch.randint(0, L + 1, VOLUME, generator=g).to(torch.uint8).to(dev)
    labels = list(range(1, L + 1))
    torch.manual_seed(0)
    net = torch.nn.Conv3d(C + L, HEADS, 1).to(dev).eval()
    kw = dict(mirror_axes=(0, 1, 2), tile_batch=1)
    voxels = VOLUME[0] * VOLUME[1] * VOLUME[2]
    lines = [f"device {torch.cuda.get_device_name(0)}; {C} channel + {L} labels, volume {VOLUME}, tile {TILE}, 8 mirror variants, "
             f"1 tile per call, network: Conv3d({C + L}, {HEADS}, 1); times: median (min-max) of {args.repeats} calls after one warm-up",
             f"one-hot volume: 4 * {L} * {voxels} = {4 * L * voxels / 1e9:.3f} GB; stacked input {4 * (C + L) * voxels / 1e9:.3f} GB; "
             f"label map {voxels / 1e6:.1f} MB"]

    def k32():
        return inference.predict_sliding_window_return_logits(net, image, HEADS, TILE, previous_stage_seg=seg, cascade_labels=labels, **kw)

    def explicit():
        return inference.predict_sliding_window_return_logits(net, torch.cat((image, inference.one_hot(seg, labels))), HEADS, TILE, **kw)

    got, t_k32, m_k32 = measure(k32, args.repeats)
    g_k32 = kernel_ms(k32, "sw_gather_onehot_kernel")
    want, t_exp, m_exp = measure(explicit, args.repeats)
    g_exp = kernel_ms(explicit, "sw_gather_kernel")
    same = bool(torch.equal(got, want))
    del got, want
    torch.cuda.empty_cache()
    for name, t, m, k in (("K32 (label map in, no one-hot volume)", t_k32, m_k32, g_k32), ("explicit one-hot stack", t_exp, m_exp, g_exp)):
        lines.append(f"  {name}: whole call {t[0]:.1f} ms ({t[1]:.1f}-{t[2]:.1f}), peak memory rise {m / 1e9:.3f} GB, gather kernel "
                     f"{k[0]:.2f} ms in {k[1]} launches")
    lines.append(f"  logits of the two paths identical: {same}; peak memory saved {(m_exp - m_k32) / 1e9:.3f} GB")
    print("\n".join(lines), flush=True)

    x = torch.randn((HEADS,) + LOWRES, generator=g) * 3
    props = {"spacing": [2.5, 0.76, 0.76], "shape_after_cropping_and_before_resampling": LOWRES}
    xd = x.to(dev)
    dseg, t_dev, m_dev = measure(lambda: E.resample_logits_to_next_stage(xd, VOLUME, LOWRES_SPACING, props), args.repeats)
    t0 = time.perf_counter()
    hseg = E.resample_logits_to_next_stage(x, VOLUME, LOWRES_SPACING, props)
    host_s = time.perf_counter() - t0
    tail = [f"[hand-off] logits {(HEADS,) + LOWRES} at spacing {LOWRES_SPACING} -> uint8 labels {VOLUME}",
            f"  K21 on the device: whole call {t_dev[0]:.2f} ms ({t_dev[1]:.2f}-{t_dev[2]:.2f}), peak memory rise {m_dev / 1e6:.1f} MB",
            f"  host path: {host_s:.2f} s on {torch.get_num_threads()} torch CPU threads",
            f"  device vs host labels: {int((dseg.cpu() != hseg).sum())} of {voxels} voxels differ"]
    print("\n".join(tail), flush=True)
    lines += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not same:
        raise SystemExit("the two input paths disagree")


if __name__ == "__main__":
    main()
