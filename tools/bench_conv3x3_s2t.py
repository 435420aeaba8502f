#!/usr/bin/env python
"""K19t against MIOpen on the three PatchExpand transposed convolutions (3 x 3, stride 2, padding 1) at batch 10: forward, data
gradient and weight gradient, timed through the C ABI, with the tuned find-db loaded as bench.py loads it.  BENCH_FORM = 3 (fp32:
three bf16 pieces), 1 (bf16) or 2 (fp16); the library side then runs in that 16-bit type."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import _lib, miopen_tuning  # noqa: E402

DEV = torch.device("cuda:0")
FORM = int(os.environ.get("BENCH_FORM", "3"))
LIBT = {1: torch.bfloat16, 2: torch.float16, 3: torch.float32}[FORM]
TOL = 1e-4 if FORM == 3 else 3e-2
SHAPES = [("up_0", 192, 96, 64), ("up_1", 384, 192, 32), ("up_2", 768, 384, 16)]     # (I, O, H = W of the input)


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3


def _rel(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max())


def main():
    # the committed find-db covers the fp32 convolutions of the 256 x 256 step (bench.py loads it for that configuration only)
    miopen_tuning.use_tuned_convolutions(enabled=os.environ.get("MLAGG_BENCH_MIOPEN", "auto") == "auto" and FORM == 3)
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    B = 10
    print(f"form {FORM}, batch {B}")
    print(f"{'layer (I, O, H)':24s} {'fwd':>7s} {'TF/s':>6s} {'MIOpen':>7s} | {'dgrad':>7s} {'TF/s':>6s} {'MIOpen':>7s} | "
          f"{'wgrad':>7s} {'TF/s':>6s} {'MIOpen':>7s}")
    tot = [0.0] * 6
    for name, I, O, H in SHAPES:
        W = H
        x = torch.randn(B, I, H, W, device=DEV)
        w = torch.randn(I, O, 3, 3, device=DEV) * (9 * I) ** -0.5
        gfull = torch.randn(B, O, 2 * H, 2 * W, device=DEV)
        gy = gfull[:, :, 1:, 1:]                            # what PatchExpand's pad hands back
        gyc = gy.contiguous()
        y = torch.empty(B, O, 2 * H - 1, 2 * W - 1, device=DEV)
        dx = torch.empty_like(x)
        dW = torch.empty_like(w)
        ws = torch.empty(lib.mlagg_conv3x3_s2t_workspace_bytes(O, I), device=DEV, dtype=torch.uint8)
        wws = torch.empty(lib.mlagg_conv3x3_s2t_wgrad_workspace_floats(B, O, I, H, W), device=DEV)
        xl, wl, gl = x.to(LIBT), w.to(LIBT), gyc.to(LIBT)
        fl = 2.0 * B * H * W * I * O * 9

        def fwd():
            _lib.check(lib.mlagg_conv3x3_s2t_fwd(x.data_ptr(), x.stride(0), w.data_ptr(), y.data_ptr(), y.stride(0), ws.data_ptr(), B, O, I,
                                                 H, W, FORM, st), "fwd")

        def dgrad():
            _lib.check(lib.mlagg_conv3x3_s2_dgrad(gy.data_ptr(), gy.stride(0), gy.stride(1), gy.stride(2), w.data_ptr(), dx.data_ptr(),
                                                  dx.stride(0), ws.data_ptr(), B, O, I, H, W, FORM, st), "dgrad")

        def wgrad():
            _lib.check(lib.mlagg_conv3x3_s2t_wgrad(x.data_ptr(), x.stride(0), gy.data_ptr(), gy.stride(0), gy.stride(1), gy.stride(2),
                                                   dW.data_ptr(), wws.data_ptr(), B, O, I, H, W, FORM, st), "wgrad")

        def lib_bwd(mask):
            return torch.ops.aten.convolution_backward(gl, xl, wl, None, (2, 2), (1, 1), (1, 1), True, (0, 0), 1, mask)

        f = timeit(fwd)
        fm = timeit(lambda: F.conv_transpose2d(xl, wl, None, 2, 1))
        d = timeit(dgrad)
        dm = timeit(lambda: lib_bwd((True, False, False)))
        g = timeit(wgrad)
        gm = timeit(lambda: lib_bwd((False, True, False)))
        ref = F.conv_transpose2d(xl, wl, None, 2, 1)
        dref, wref = lib_bwd((True, True, False))[:2]
        errs = (_rel(y, ref), _rel(dx, dref), _rel(dW, wref))
        assert max(errs) < TOL, errs
        for i, v in enumerate((f, fm, d, dm, g, gm)):
            tot[i] += v
        print(f"{name + ' ' + str((I, O, H)):24s} {f:7.1f} {fl / f / 1e6:6.1f} {fm:7.1f} | {d:7.1f} {fl / d / 1e6:6.1f} {dm:7.1f} | "
              f"{g:7.1f} {fl / g / 1e6:6.1f} {gm:7.1f}", flush=True)
    print("totals us: fwd %.0f (MIOpen %.0f)  dgrad %.0f (MIOpen %.0f)  wgrad %.0f (MIOpen %.0f)" % tuple(tot))


if __name__ == "__main__":
    main()
