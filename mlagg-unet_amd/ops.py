"""torch.autograd.Function wrappers over the C ABI (include/mlagg_hip.h).

PyTorch is plumbing here: device memory, the current HIP stream and autograd bookkeeping.  Every
op requires CUDA(HIP) fp32 tensors and raises RuntimeError otherwise -- there is no eager path.
"""
import ctypes

import numpy as np
import torch

from . import _lib

_launch = _lib.launch
_stream = _lib.stream           # the raw current stream, for callers that invoke an entry point directly (tests)
_C = _lib.CONSTANTS


# ------------------------------------------------------------------------------------------------
# arithmetic type of the dense products.  The reference's default train step runs the network under autocast
# (nnUNetTrainer.py:848: fp16 + GradScaler; BASELINE configs[2]: bf16): Linear / convolution operands are rounded to 16
# bits, sums are fp32.  Here tensors stay fp32 in HBM in every mode; in "bf16" / "fp16" mode the projections (K5) and
# the library convolutions / small GEMMs round their OPERANDS to that type for the matrix cores.
# ------------------------------------------------------------------------------------------------
PRECISIONS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_LP_CODE = {torch.bfloat16: _C["MLAGG_DTYPE_BF16"], torch.float16: _C["MLAGG_DTYPE_F16"]}
import threading as _threading


class _ComputeStack(_threading.local):
    """Per-thread stack (autograd's backward thread and data-loader threads never see another thread's block)."""

    def __init__(self):
        self.stack = [torch.float32]


_COMPUTE = _ComputeStack()


class compute_precision:
    """with ops.compute_precision("bf16"): ... -- arithmetic type of the dense products inside the block."""

    def __init__(self, precision):
        if precision not in PRECISIONS:
            raise RuntimeError(f"precision {precision!r}: one of {tuple(PRECISIONS)}")
        self.dtype = PRECISIONS[precision]

    def __enter__(self):
        _COMPUTE.stack.append(self.dtype)
        return self

    def __exit__(self, *exc):
        _COMPUTE.stack.pop()
        return False


def compute_dtype():
    return _COMPUTE.stack[-1]


def lp(t, dtype):
    """Operand of a library GEMM / convolution in the arithmetic type of the block (identity in fp32 mode)."""
    return t if (t is None or dtype == torch.float32) else t.to(dtype)


# Library convolutions in 16-bit mode: ON by default -- the literal operand rounding of the reference's autocast step.  The
# maps are fp32 in HBM, so a 16-bit MIOpen convolution costs a cast kernel on its input and another on its output (and again
# in backward), but the 16-bit convolutions themselves are so much faster that the step gains: config 3 (224 x 224, bf16)
# 42.2 -> 34.7 ms, config 5 (512 x 640, fp16) 98.0 -> 82.9 ms.  (Early in round 2, before the fused conv epilogues, the casts
# still outweighed the gain.)  MLAGG_LP_CONV=0 keeps the convolutions in fp32.
import os as _os
LP_CONV = _os.environ.get("MLAGG_LP_CONV", "1") == "1"


def conv_dtype():
    return compute_dtype() if LP_CONV else torch.float32


# 16-bit modes, round 4: the 1 x 1 / 3 x 3 stride-1 convolutions run on K18 / K19 in the ONE-product operand form (csrc/opmode.h: operands
# rounded once to bf16 / fp16 in registers, fp32 sums) straight on the fp32 maps -- the kernels of the fp32 step at a sixth of its matrix
# work, no cast kernels, no NHWC transposes.  Maps below LP_K_MIN_PIXELS pixels, strided and transposed convolutions stay 16-bit library
# calls.
LP_K_MIN_PIXELS = int(_os.environ.get("MLAGG_LP_K_MIN_PIXELS", "1024"))
_DTYPE_BF16X3 = _C["MLAGG_DTYPE_BF16X3"]
_FORM_TORCH = {_LP_CODE[torch.bfloat16]: torch.bfloat16, _LP_CODE[torch.float16]: torch.float16, _DTYPE_BF16X3: torch.float32}


def conv_form():
    """Operand form (MLAGG_DTYPE_* code) of the K18 / K19 products in the current mode: three bf16 pieces (fp32), or one rounded operand."""
    cdt = conv_dtype()
    return _DTYPE_BF16X3 if cdt == torch.float32 else _LP_CODE[cdt]


def _lib_conv(x, w, stride, padding, transposed, form):
    """Library forward of a product that a convolution Function leaves to the library (2-D or 3-D, isotropic stride and padding, no
    bias), in the arithmetic of `form`: fp32 maps in and out."""
    nd, t = x.dim() - 2, _FORM_TORCH[form]
    return torch.convolution(lp(x, t), lp(w, t), None, (stride,) * nd, (padding,) * nd, (1,) * nd, transposed, (0,) * nd, 1).float()


def _lib_conv_bwd(dy, x, w, stride, padding, transposed, mask, form):
    nd, t = x.dim() - 2, _FORM_TORCH[form]
    out = torch.ops.aten.convolution_backward(lp(dy, t).contiguous(), lp(x, t), lp(w, t), None, (stride,) * nd, (padding,) * nd, (1,) * nd,
                                              transposed, (0,) * nd, 1, mask)
    return [None if o is None else o.float() for o in out]


def _ptr(t):
    return None if t is None else t.data_ptr()


# flop of the matrix products this package's own kernels run, per family (bench.py's roofline.mfma): None = not counting
FLOP_COUNT = None


def _flop(family, n):
    if FLOP_COUNT is not None:
        FLOP_COUNT[family] = FLOP_COUNT.get(family, 0) + int(n)


def _require(t, name, shape=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
        raise RuntimeError(f"{name}: expected a float32 tensor on the MI355X device, got "
                           f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '?')}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


class SelectiveScanFn(torch.autograd.Function):
    """K1.  Same contract as mamba-ssm's SelectiveScanFn as used at MambaSkip.py:445-451."""

    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, delta_bias, delta_softplus):
        b, d, L = u.shape
        n, g = A.shape[1], B.shape[1]
        u = _require(u.contiguous(), "u")
        delta = _require(delta.contiguous(), "delta", (b, d, L))
        A = _require(A.contiguous(), "A", (d, n))
        B = _require(B.contiguous(), "B", (b, g, n, L))
        C = _require(C.contiguous(), "C", (b, g, n, L))
        D = None if D is None else _require(D.contiguous(), "D", (d,))
        delta_bias = None if delta_bias is None else _require(delta_bias.contiguous(), "delta_bias", (d,))
        out = torch.empty_like(u)
        state = torch.empty(_lib.lib().mlagg_selscan_state_floats(b, d, L, n), device=u.device, dtype=torch.float32)
        _launch("mlagg_selscan_fwd", _ptr(u), _ptr(delta), _ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(delta_bias), _ptr(out), _ptr(state), b,
                d, L, n, g, int(bool(delta_softplus)))
        ctx.save_for_backward(u, delta, A, B, C, D, delta_bias, state)
        ctx.delta_softplus = bool(delta_softplus)
        return out

    @staticmethod
    def backward(ctx, dout):
        u, delta, A, B, C, D, delta_bias, state = ctx.saved_tensors
        b, d, L = u.shape
        n, g = A.shape[1], B.shape[1]
        dout = _require(dout.contiguous(), "dout", (b, d, L))
        du, ddelta = torch.empty_like(u), torch.empty_like(u)
        dA, dB, dC = torch.empty_like(A), torch.empty_like(B), torch.empty_like(C)
        dD = None if D is None else torch.empty_like(D)
        dbias = None if delta_bias is None else torch.empty_like(delta_bias)
        ws = torch.empty(_lib.lib().mlagg_selscan_bwd_workspace_floats(b, d, L, n), device=u.device, dtype=torch.float32)
        _launch("mlagg_selscan_bwd", _ptr(u), _ptr(delta), _ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(delta_bias), _ptr(dout), _ptr(state),
                _ptr(du), _ptr(ddelta), _ptr(dA), _ptr(dB), _ptr(dC), _ptr(dD), _ptr(dbias), _ptr(ws), b, d, L, n, g,
                int(ctx.delta_softplus))
        return du, ddelta, dA, dB, dC, dD, dbias, None


def selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False,
                      return_last_state=False):
    """Drop-in for ``mamba_ssm.ops.selective_scan_interface.selective_scan_fn`` on the arguments the
    reference passes (MambaSkip.py:445-451: z=None, return_last_state=False).  Anything else raises."""
    if z is not None or return_last_state:
        raise RuntimeError("selective_scan_fn: z gating / return_last_state are not on the MLAgg-UNet path")
    return SelectiveScanFn.apply(u, delta, A, B, C, D, delta_bias, delta_softplus)


class SelectiveScanLowRankFn(torch.autograd.Function):
    """K1 with the rank-R delta projection folded in: delta = softplus(Wdt[d] . dtr[b, g(d), :, l] + delta_bias[d]) is formed
    inside the scan kernels, i.e. SS2D_skip's ``einsum("b k r l, k d r -> b k d l", dts, dt_projs_weight)`` +
    ``selective_scan_fn(..., delta_bias, delta_softplus=True)`` (reference MambaSkip.py:430-451) as one op.  The
    (B, 4*96, L) delta tensor and its gradient (334 MB each at config 2) are never materialised."""

    @staticmethod
    def forward(ctx, u, dtr, Wdt, A, B, C, D, delta_bias, delta_softplus):
        b, d, L = u.shape
        n, g, R = A.shape[1], B.shape[1], dtr.shape[2]
        u = _require(u.contiguous(), "u")
        dtr = _require(dtr.contiguous(), "dtr", (b, g, R, L))
        Wdt = _require(Wdt.contiguous(), "Wdt", (d, R))
        A = _require(A.contiguous(), "A", (d, n))
        B = _require(B.contiguous(), "B", (b, g, n, L))
        C = _require(C.contiguous(), "C", (b, g, n, L))
        D = None if D is None else _require(D.contiguous(), "D", (d,))
        delta_bias = None if delta_bias is None else _require(delta_bias.contiguous(), "delta_bias", (d,))
        out = torch.empty_like(u)
        state = torch.empty(_lib.lib().mlagg_selscan_state_floats(b, d, L, n), device=u.device, dtype=torch.float32)
        _launch("mlagg_selscan_lowrank_fwd", _ptr(u), _ptr(dtr), _ptr(Wdt), R, _ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(delta_bias),
                _ptr(out), _ptr(state), b, d, L, n, g, int(bool(delta_softplus)))
        ctx.save_for_backward(u, dtr, Wdt, A, B, C, D, delta_bias, state)
        ctx.delta_softplus = bool(delta_softplus)
        return out

    @staticmethod
    def backward(ctx, dout):
        u, dtr, Wdt, A, B, C, D, delta_bias, state = ctx.saved_tensors
        b, d, L = u.shape
        n, g, R = A.shape[1], B.shape[1], dtr.shape[2]
        dout = _require(dout.contiguous(), "dout", (b, d, L))
        du, ddtr, dW = torch.empty_like(u), torch.empty_like(dtr), torch.empty_like(Wdt)
        dA, dB, dC = torch.empty_like(A), torch.empty_like(B), torch.empty_like(C)
        dD = None if D is None else torch.empty_like(D)
        dbias = None if delta_bias is None else torch.empty_like(delta_bias)
        ws = torch.empty(_lib.lib().mlagg_selscan_bwd_workspace_floats(b, d, L, n), device=u.device, dtype=torch.float32)
        _launch("mlagg_selscan_lowrank_bwd", _ptr(u), _ptr(dtr), _ptr(Wdt), R, _ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(delta_bias),
                _ptr(dout), _ptr(state), _ptr(du), _ptr(ddtr), _ptr(dW), _ptr(dA), _ptr(dB), _ptr(dC), _ptr(dD), _ptr(dbias), _ptr(ws), b,
                d, L, n, g, int(ctx.delta_softplus))
        return du, ddtr, dW, dA, dB, dC, dD, dbias, None


def selective_scan_lowrank_fn(u, dtr, Wdt, A, B, C, D=None, delta_bias=None, delta_softplus=False):
    return SelectiveScanLowRankFn.apply(u, dtr, Wdt, A, B, C, D, delta_bias, delta_softplus)


# ------------------------------------------------------------------------------------------------
# K1f: the MSMM scan on token-major tensors (csrc/selscan_tok.hip) -- SS2D_skip.forward_corev0 behind x_proj + the four-way sum
# (reference MambaSkip.py:405-473, 534) as ONE op; shapes outside it take the round-3 chain (K1' cross_scan / cross_merge around K1)
# ------------------------------------------------------------------------------------------------
MSMM_XB = 36                      # floats per direction of a padded x_proj row: [dt0 dt1 dt2 0 | B(16) | C(16)]
_SCAN_INDEX = {}


def msmm_scan_index(HW, device):
    """(4, L_cat) int32: the token direction k visits at scan position t -- the orders of reference M:419-422 (k = 0 row-major,
    1 column-major, 2 / 3 their reversals inside every scale; scales concatenated in the same order for every direction)."""
    key = (tuple((int(h), int(w)) for h, w in HW), str(device))
    if key not in _SCAN_INDEX:
        rows, off = [[], [], [], []], 0
        for H, W in key[0]:
            n = H * W
            p = torch.arange(n, dtype=torch.int64)
            col = (p % H) * W + p // H                       # position p of the column-major walk -> token y * W + x
            for k, tok in enumerate((p, col, n - 1 - p, col.flip(0))):
                rows[k].append(tok + off)
            off += n
        table = torch.stack([torch.cat(r) for r in rows]).to(torch.int32)
        if not all(bool((table[k].sort().values == torch.arange(off, dtype=torch.int32)).all()) for k in range(4)):
            raise RuntimeError("msmm_scan_index: a direction is not a permutation of the tokens")
        _SCAN_INDEX[key] = table.to(device)
    return _SCAN_INDEX[key]


class PadXProjFn(torch.autograd.Function):
    """x_proj_weight (4, R + 2N, d) -> (4 * 36, d) with a zero row behind the three dt rows of every direction, so that the B / C
    blocks of a projection row start on 16-byte boundaries; backward drops the pad rows' (exactly zero) gradient."""

    @staticmethod
    def forward(ctx, w):
        K, per, dI = w.shape
        ctx.per = per
        out = w.new_zeros(K, MSMM_XB, dI)
        out[:, :3] = w[:, :3]
        out[:, 4:] = w[:, 3:]
        return out.view(K * MSMM_XB, dI)

    @staticmethod
    def backward(ctx, g):
        g3 = g.view(-1, MSMM_XB, g.shape[-1])
        return torch.cat([g3[:, :3], g3[:, 4:]], dim=1)


def pad_x_proj(w):
    return PadXProjFn.apply(w)


class MsmmScanFn(torch.autograd.Function):
    """K1f.  xc (B, L, 96), xdbl (B, L, 144), idx (4, L) int32, Wdt (384, 3), A (384, 16), D (384), bias (384) -> y (B, L, 96)."""

    @staticmethod
    def forward(ctx, xc, xdbl, idx, Wdt, A, D, bias):
        xc = _require(xc.contiguous(), "xc")
        B, L, dI = xc.shape
        xdbl = _require(xdbl.contiguous(), "x_dbl", (B, L, 4 * MSMM_XB))
        if idx.dtype != torch.int32 or tuple(idx.shape) != (4, L) or not idx.is_cuda or not idx.is_contiguous():
            raise RuntimeError("msmm_scan: idx must be a contiguous int32 (4, L) device table")
        lib = _lib.lib()
        if not lib.mlagg_msmm_scan_supported(dI, int(A.shape[1]), int(Wdt.shape[1]), 4, L):
            raise RuntimeError(f"msmm_scan: shape (d_inner {dI}, d_state {A.shape[1]}, rank {Wdt.shape[1]}, L {L}) is outside K1f")
        Wdt = _require(Wdt.contiguous(), "Wdt", (4 * dI, 3))
        A = _require(A.contiguous(), "A", (4 * dI, 16))
        D = None if D is None else _require(D.contiguous(), "D", (4 * dI,))
        bias = None if bias is None else _require(bias.contiguous(), "delta_bias", (4 * dI,))
        y = torch.empty(B, L, dI, device=xc.device, dtype=torch.float32)
        state = torch.empty(lib.mlagg_msmm_scan_state_floats(B, L), device=xc.device, dtype=torch.float32)
        ws = torch.empty(lib.mlagg_msmm_scan_fwd_workspace_floats(B, L), device=xc.device, dtype=torch.float32)
        _launch("mlagg_msmm_scan_fwd", _ptr(xc), _ptr(xdbl), _ptr(idx), _ptr(Wdt), _ptr(A), _ptr(D), _ptr(bias), _ptr(y), _ptr(state),
                _ptr(ws), B, L)
        ctx.save_for_backward(xc, xdbl, idx, Wdt, A, D, bias, state)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, xdbl, idx, Wdt, A, D, bias, state = ctx.saved_tensors
        B, L, dI = xc.shape
        dy = _require(dy.contiguous(), "dy", (B, L, dI))
        dev = xc.device
        dxc, dxdbl = torch.empty_like(xc), torch.empty_like(xdbl)
        dW, dA = torch.empty_like(Wdt), torch.empty_like(A)
        dD = None if D is None else torch.empty_like(D)
        dbias = None if bias is None else torch.empty_like(bias)
        ws = torch.empty(_lib.lib().mlagg_msmm_scan_bwd_workspace_floats(B, L), device=dev, dtype=torch.float32)
        _launch("mlagg_msmm_scan_bwd", _ptr(xc), _ptr(xdbl), _ptr(idx), _ptr(Wdt), _ptr(A), _ptr(D), _ptr(bias), _ptr(dy), _ptr(state),
                _ptr(dxc), _ptr(dxdbl), _ptr(dW), _ptr(dA), _ptr(dD), _ptr(dbias), _ptr(ws), B, L)
        return dxc, dxdbl, None, dW, dA, dD, dbias


def msmm_scan(xc, xdbl, idx, Wdt, A, D=None, delta_bias=None):
    return MsmmScanFn.apply(xc, xdbl, idx, Wdt, A, D, delta_bias)


def msmm_scan_supported(xc, d_state, dt_rank):
    return bool(xc.is_cuda and xc.dim() == 3 and
                _lib.lib().mlagg_msmm_scan_supported(int(xc.shape[2]), int(d_state), int(dt_rank), 4, int(xc.shape[1])))


def _rows(t, name):
    """(B, N, C) view whose last dim is contiguous and whose batch/token dims collapse to one row
    stride (true for fresh Linear outputs and their channel slices); returns (tensor, row_stride)."""
    _require(t, name)
    if t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1) or t.stride(1) % 4 or \
            t.data_ptr() % 16:
        t = t.contiguous()
    return t, t.stride(1)


class _GradSlot:
    """Column block [col0, col0 + width) of the gradient buffer of one ``split_cols`` call.  The FIRST kernel wrapper that consumes the
    piece claims the slot; its backward kernel then writes d(piece) straight into the shared (B, N, total) buffer (row stride =
    total), so the split's backward hands that buffer on as it is instead of concatenating the pieces
    (``CatArrayBatchedCopy``: 40 launches, 0.79 ms of the 256 x 256 step in profiles/round2_d_kernel_trace_timed_region.md)."""

    __slots__ = ("arena", "col0", "width", "claimed", "dim")

    def __init__(self, arena, col0, width, dim=-1):
        self.arena, self.col0, self.width, self.claimed, self.dim = arena, col0, width, False, dim

    def view(self):
        return self.arena.buffer().narrow(self.dim, self.col0, self.width)


class _GradArena:
    def __init__(self, shape, device):
        self.shape, self.device, self.buf = tuple(shape), device, None

    def buffer(self):
        if self.buf is None:
            self.buf = torch.empty(self.shape, device=self.device, dtype=torch.float32)
        return self.buf


def claim_slot(t):
    """The gradient slot of a ``split_cols`` piece, if it has one nobody claimed yet (a piece feeding two kernels: the second takes
    the ordinary path and autograd's sum of the two gradients is copied into the slot)."""
    slot = getattr(t, "_mlagg_slot", None)
    if slot is None or slot.claimed or not torch.is_grad_enabled():
        return None
    slot.claimed = True
    return slot


def _grad_out(slot, shape, device):
    """(tensor, row stride) a backward kernel writes d(input) into: the claimed arena slot or a fresh contiguous tensor."""
    if slot is not None:
        v = slot.view()
        return v, v.stride(-2)
    t = torch.empty(shape, device=device, dtype=torch.float32)
    return t, shape[-1]


class SplitColsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, arena, *sizes):
        ctx.arena, ctx.sizes = arena, sizes
        return t.split(list(sizes), dim=-1)

    @staticmethod
    def backward(ctx, *grads):
        arena, sizes = ctx.arena, ctx.sizes
        buf = arena.buffer()
        col0 = 0
        for g, w in zip(grads, sizes):
            dst = buf[..., col0:col0 + w]
            if g is None:
                dst.zero_()
            elif g.data_ptr() != dst.data_ptr() or g.stride() != dst.stride():
                dst.copy_(g)
            col0 += w
        arena.buf = None
        return (buf, None) + (None,) * len(sizes)


class SplitPlanesFn(torch.autograd.Function):
    """``t.split(sizes, dim=1)`` of an NCHW map with ONE gradient buffer for the pieces (see split_planes)."""

    @staticmethod
    def forward(ctx, t, arena, *sizes):
        ctx.arena, ctx.sizes = arena, sizes
        return t.split(list(sizes), dim=1)

    @staticmethod
    def backward(ctx, *grads):
        arena, sizes = ctx.arena, ctx.sizes
        buf = arena.buffer()
        c0 = 0
        for g, w in zip(grads, sizes):
            dst = buf.narrow(1, c0, w)
            if g is None:
                dst.zero_()
            elif g.data_ptr() != dst.data_ptr() or g.stride() != dst.stride():
                dst.copy_(g)
            c0 += w
        arena.buf = None
        return (buf, None) + (None,) * len(sizes)


def split_planes(t, sizes):
    """``t.split(sizes, dim=1)`` of an NCHW map whose pieces feed this package's kernels (the (mamba | conv) halves of the MSMM inputs,
    MambaSkip.py:727-733): the same views, and the kernels' backward passes -- the token transpose, K19's data gradient -- write their
    results into ONE (B, C, H, W) gradient buffer, which the split's backward hands on instead of concatenating the pieces
    (``CatArrayBatchedCopy`` behind SplitWithSizesBackward: 163 us of the step).  A piece whose consumer cannot is copied into place."""
    if not (t.is_cuda and t.requires_grad and torch.is_grad_enabled() and t.dim() == 4 and t.is_contiguous()
            and t.dtype == torch.float32 and (t.shape[2] * t.shape[3]) % 4 == 0):
        return t.split(list(sizes), dim=1)
    arena = _GradArena(t.shape, t.device)
    pieces = SplitPlanesFn.apply(t, arena, *sizes)
    c0 = 0
    for p_, w in zip(pieces, sizes):
        p_._mlagg_slot = _GradSlot(arena, c0, w, dim=1)
        c0 += w
    return pieces


def transpose_2d_into(src, dst):
    """(B, R, C) -> dst (B, C, R...) whose samples are dense (C, R) blocks at any sample stride (a channel slice of an NCHW map)."""
    _require(src, "src")
    B, R, C = src.shape
    if not (src.stride(2) == 1 and src.stride(1) == C and src.stride(0) >= R * C and src.data_ptr() % 16 == 0
            and (C % 4 or src.stride(0) % 4 == 0)):
        src = src.contiguous()
    _launch("mlagg_transpose_2d_into", _ptr(src), src.stride(0), _ptr(dst), dst.stride(0), B, R, C)
    return dst


def split_cols(t, sizes):
    """``t.split(sizes, dim=-1)`` of a fresh (B, N, total) projection output whose pieces feed this package's kernels: the pieces are
    the same strided views, and the kernels' backward passes write into ONE gradient buffer (see _GradSlot)."""
    if not (t.is_cuda and t.requires_grad and torch.is_grad_enabled() and t.dim() == 3 and t.is_contiguous()
            and all(w % 4 == 0 for w in sizes)):
        return t.split(list(sizes), dim=-1)
    arena = _GradArena(t.shape, t.device)
    pieces = SplitColsFn.apply(t, arena, *sizes)
    col0 = 0
    for p_, w in zip(pieces, sizes):
        p_._mlagg_slot = _GradSlot(arena, col0, w)
        col0 += w
    return pieces


class DWConv3x3Fn(torch.autograd.Function):
    """K2: depthwise 3x3 (+bias, optional SiLU) on token-major maps."""

    @staticmethod
    def forward(ctx, x, weight, bias, H, W, silu, slot=None, res=None):
        ctx.slot = slot
        x, xs = _rows(x, "x")
        B, N, C = x.shape
        if N != H * W:
            raise RuntimeError(f"dwconv3x3: {N} tokens != {H}x{W}")
        if res is not None:
            if silu or tuple(res.shape) != (B, N, C):
                raise RuntimeError("dwconv3x3: the residual is added to the plain convolution, same shape as the output")
            res = _require(res.contiguous(), "res")
        w = _require(weight.reshape(C, 9).contiguous(), "weight")
        y = torch.empty(B, N, C, device=x.device, dtype=torch.float32)
        pre = torch.empty_like(y) if silu else None      # pre-activation, needed by SiLU's backward
        _launch("mlagg_dwconv3x3_fwd", _ptr(x), xs, _ptr(w), _ptr(bias), _ptr(res), _ptr(y), C, _ptr(pre), B, H, W, C, int(silu))
        ctx.save_for_backward(x, w, pre)
        ctx.geom = (H, W, bool(silu), bias is not None, weight.shape)
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, pre = ctx.saved_tensors
        H, W, silu, has_bias, wshape = ctx.geom
        B, N, C = x.shape
        dy, dys = _rows(dy, "dy")
        dx, dxs = _grad_out(ctx.slot, (B, N, C), x.device)
        dw = torch.empty(C, 9, device=x.device, dtype=torch.float32)
        db = torch.empty(C, device=x.device, dtype=torch.float32) if has_bias else None
        ws = torch.empty(_lib.lib().mlagg_dwconv3x3_bwd_workspace_floats(B, H, W, C), device=x.device, dtype=torch.float32)
        _launch("mlagg_dwconv3x3_bwd", _ptr(x), x.stride(1), _ptr(w), _ptr(dy), dys, _ptr(pre), _ptr(dx), dxs, _ptr(dw), _ptr(db), _ptr(ws),
                B, H, W, C, int(silu))
        return dx, dw.reshape(wshape), db, None, None, None, None, (dy if ctx.has_res else None)


class DWConvGatedFn(torch.autograd.Function):
    """K2, gated form: y = SiLU(dwconv3x3(x) + bias) * gate -- ConvolutionalGLU's ``self.act(self.dwconv(x, H, W)) * v`` (MambaSkip.py:
    559-577) with the product in the convolution's epilogue; backward writes d(gate) from the weight-gradient pass (three ATen
    multiplications per scale and step gone)."""

    @staticmethod
    def forward(ctx, x, gate, weight, bias, H, W, slot=None, gate_slot=None):
        ctx.slots = (slot, gate_slot)
        x, xs = _rows(x, "x")
        gate, gs = _rows(gate, "gate")
        B, N, C = x.shape
        if N != H * W or tuple(gate.shape) != (B, N, C):
            raise RuntimeError(f"dwconv3x3_gated: bad shapes x {tuple(x.shape)} gate {tuple(gate.shape)} map {H}x{W}")
        w = _require(weight.reshape(C, 9).contiguous(), "weight")
        y = torch.empty(B, N, C, device=x.device, dtype=torch.float32)
        pre = torch.empty_like(y)
        _launch("mlagg_dwconv3x3_gated_fwd", _ptr(x), xs, _ptr(w), _ptr(bias), _ptr(gate), gs, _ptr(y), C, _ptr(pre), B, H, W, C)
        ctx.save_for_backward(x, gate, w, pre)
        ctx.geom = (H, W, bias is not None, weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gate, w, pre = ctx.saved_tensors
        H, W, has_bias, wshape = ctx.geom
        B, N, C = x.shape
        dy, dys = _rows(dy, "dy")
        dx, dxs = _grad_out(ctx.slots[0], (B, N, C), x.device)
        dgate, dgs = _grad_out(ctx.slots[1], (B, N, C), x.device)
        dw = torch.empty(C, 9, device=x.device, dtype=torch.float32)
        db = torch.empty(C, device=x.device, dtype=torch.float32) if has_bias else None
        ws = torch.empty(_lib.lib().mlagg_dwconv3x3_bwd_workspace_floats(B, H, W, C), device=x.device, dtype=torch.float32)
        _launch("mlagg_dwconv3x3_gated_bwd", _ptr(x), x.stride(1), _ptr(w), _ptr(dy), dys, _ptr(pre), _ptr(gate), gate.stride(1), _ptr(dx),
                dxs, _ptr(dgate), dgs, _ptr(dw), _ptr(db), _ptr(ws), B, H, W, C)
        return dx, dgate, dw.reshape(wshape), db, None, None, None, None


def dwconv3x3_gated(x, gate, weight, bias, H, W):
    """SiLU(depthwise 3x3(x) + bias) * gate on token-major maps (x, gate: column blocks of one projection output are fine)."""
    return DWConvGatedFn.apply(x, gate, weight, bias, H, W, claim_slot(x), claim_slot(gate))


def dwconv3x3_nlc(x, weight, bias, H, W, silu=False, res=None):
    """Depthwise 3x3 on a token-major map; `res` (same shape as the output) is added in the same pass."""
    return DWConv3x3Fn.apply(x, weight, bias, H, W, silu, claim_slot(x), res)


class DWConv3dFn(torch.autograd.Function):
    """K2v: depthwise 3x3x3 convolution (+ SiLU) on token-major volumes (B, D*H*W, C); weight (C, 1, 3, 3, 3)."""

    @staticmethod
    def forward(ctx, x, weight, bias, dims, silu):
        D, H, W = dims
        x, xs = _rows(x, "x")
        B, L, C = x.shape
        if L != D * H * W or weight.numel() != C * 27:
            raise RuntimeError(f"dwconv3d: bad shapes x {tuple(x.shape)} weight {tuple(weight.shape)} dims {dims}")
        w = _require(weight.reshape(C, 27).contiguous(), "weight")
        bias = None if bias is None else _require(bias.contiguous(), "bias", (C,))
        y = torch.empty(B, L, C, device=x.device, dtype=torch.float32)
        pre = torch.empty_like(y) if silu else None
        _launch("mlagg_dwconv3d_fwd", _ptr(x), xs, _ptr(w), _ptr(bias), _ptr(y), C, _ptr(pre), B, D, H, W, C, int(silu))
        ctx.save_for_backward(x, w, pre)
        ctx.geom = (D, H, W, bool(silu), bias is not None, weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, pre = ctx.saved_tensors
        D, H, W, silu, has_bias, wshape = ctx.geom
        B, L, C = x.shape
        dy, dys = _rows(dy, "dy")
        dx = torch.empty(B, L, C, device=x.device, dtype=torch.float32)
        dw = torch.empty(C, 27, device=x.device, dtype=torch.float32)
        db = torch.empty(C, device=x.device, dtype=torch.float32) if has_bias else None
        ws = torch.empty(_lib.lib().mlagg_dwconv3d_bwd_workspace_floats(B, D, H, W, C), device=x.device, dtype=torch.float32)
        _launch("mlagg_dwconv3d_bwd", _ptr(x), x.stride(1), _ptr(w), _ptr(dy), dys, _ptr(pre), _ptr(dx), C, _ptr(dw), _ptr(db), _ptr(ws), B,
                D, H, W, C, int(silu))
        return dx, dw.reshape(wshape), db, None, None


def dwconv3d_nlc(x, weight, bias, dims, silu=False):
    return DWConv3dFn.apply(x, weight, bias, dims, silu)


class SelectiveScan1Fn(torch.autograd.Function):
    """K1s: the d_state = 1 selective scan of the 3-D network (UMambaEnc_SS3D.py:244-296 + the 12-way sum at :338) on the
    token-major volume: u is gathered and y scattered through the permutation table inside the kernels.
    tok (B, L, C), idx (K, L) int32, dtr (B, K, R, L), Bs / Cs (B, K, L), Wdt (K*C, R), A / D / bias (K*C) -> (B, L, C)."""

    @staticmethod
    def forward(ctx, tok, idx, dtr, Bs, Cs, Wdt, A, D, bias):
        tok, ts = _rows(tok, "tok")
        B, L, C = tok.shape
        K, R = idx.shape[0], dtr.shape[2]
        if idx.dtype != torch.int32 or tuple(idx.shape) != (K, L) or not idx.is_cuda:
            raise RuntimeError("selective_scan1: idx must be an int32 (K, L) device table")
        dtr = _require(dtr.contiguous(), "dtr", (B, K, R, L))
        Bs = _require(Bs.contiguous(), "Bs", (B, K, L))
        Cs = _require(Cs.contiguous(), "Cs", (B, K, L))
        Wdt = _require(Wdt.contiguous(), "Wdt", (K * C, R))
        A, D, bias = (_require(v.reshape(-1).contiguous(), n, (K * C,)) for v, n in ((A, "A"), (D, "D"), (bias, "delta_bias")))
        yk = torch.empty(B, L, K * C, device=tok.device, dtype=torch.float32)
        state = torch.empty(_lib.lib().mlagg_selscan1_state_floats(B, L, C, K), device=tok.device, dtype=torch.float32)
        _launch("mlagg_selscan1_fwd", _ptr(tok), ts, _ptr(idx), _ptr(dtr), _ptr(Bs), _ptr(Cs), _ptr(Wdt), R, _ptr(A), _ptr(D), _ptr(bias),
                _ptr(yk), _ptr(state), B, L, C, K)
        y = torch.empty(B, L, C, device=tok.device, dtype=torch.float32)
        _launch("mlagg_block_sum", _ptr(yk), _ptr(y), B * L, K, C)
        ctx.save_for_backward(tok, idx, dtr, Bs, Cs, Wdt, A, D, bias, state)
        return y

    @staticmethod
    def backward(ctx, dy):
        tok, idx, dtr, Bs, Cs, Wdt, A, D, bias, state = ctx.saved_tensors
        B, L, C = tok.shape
        K, R = idx.shape[0], dtr.shape[2]
        dy, ds = _rows(dy, "dy")
        dev = tok.device
        duk = torch.empty(B, L, K * C, device=dev, dtype=torch.float32)
        ddtr, dBs, dCs = torch.empty_like(dtr), torch.empty_like(Bs), torch.empty_like(Cs)
        dpar = torch.empty(K * C, 3 + R, device=dev, dtype=torch.float32)
        ws = torch.empty(_lib.lib().mlagg_selscan1_bwd_workspace_floats(B, L, C, K, R), device=dev, dtype=torch.float32)
        _launch("mlagg_selscan1_bwd", _ptr(tok), tok.stride(1), _ptr(idx), _ptr(dtr), _ptr(Bs), _ptr(Cs), _ptr(Wdt), R, _ptr(A), _ptr(D),
                _ptr(bias), _ptr(dy), ds, _ptr(state), _ptr(duk), _ptr(ddtr), _ptr(dBs), _ptr(dCs), _ptr(dpar), _ptr(ws), B, L, C, K)
        dtok = torch.empty(B, L, C, device=dev, dtype=torch.float32)
        _launch("mlagg_block_sum", _ptr(duk), _ptr(dtok), B * L, K, C)
        return dtok, None, ddtr, dBs, dCs, dpar[:, 3:], dpar[:, 0], dpar[:, 1], dpar[:, 2]


def selective_scan1(tok, idx, dtr, Bs, Cs, Wdt, A, D, bias):
    return SelectiveScan1Fn.apply(tok, idx, dtr, Bs, Cs, Wdt, A, D, bias)


class LocalDiffAttnFn(torch.autograd.Function):
    """K3: fused 3x3-window differential attention + RMSNorm + LePE (AggregatedAttention local branch)."""

    @staticmethod
    def forward(ctx, q, kv, lam, subln_w, lepe_w, lepe_b, H, W, nh, scale, q_slot=None, kv_slot=None):
        ctx.slots = (q_slot, kv_slot)
        q, qs = _rows(q, "q")
        kv, kvs = _rows(kv, "kv")
        B, N, d = q.shape
        if N != H * W or d != nh * 48 or kv.shape[2] != 2 * d:
            raise RuntimeError(f"local_diff_attn: bad shapes q {tuple(q.shape)} kv {tuple(kv.shape)} H {H} W {W} nh {nh}")
        lam = _require(lam.reshape(1).contiguous(), "lambda")
        subln_w = _require(subln_w.contiguous(), "subln.weight", (48,))
        lw = _require(lepe_w.reshape(d, 9).contiguous(), "lepe.weight")
        lb = _require(lepe_b.contiguous(), "lepe.bias", (d,))
        out = torch.empty(B, N, d, device=q.device, dtype=torch.float32)
        _launch("mlagg_local_attn_fwd", _ptr(q), qs, _ptr(kv), kvs, _ptr(lam), _ptr(subln_w), _ptr(lw), _ptr(lb), _ptr(out), d, B, H, W, nh,
                float(scale))
        ctx.save_for_backward(q, kv, lam, subln_w, lw)
        ctx.geom = (H, W, nh, float(scale), lepe_w.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kv, lam, subln_w, lw = ctx.saved_tensors
        H, W, nh, scale, lwshape = ctx.geom
        B, N, d = q.shape
        dout, dos = _rows(dout, "dout")
        dq, dqs = _grad_out(ctx.slots[0], (B, N, d), q.device)
        dkv, dkvs = _grad_out(ctx.slots[1], (B, N, 2 * d), q.device)
        small = torch.zeros(1 + 48 + d * 9 + d, device=q.device, dtype=torch.float32)
        dlam, dsub, dlw, dlb = small[:1], small[1:49], small[49:49 + d * 9], small[49 + d * 9:]
        ws = torch.empty(_lib.lib().mlagg_local_attn_bwd_workspace_floats(B, H, W, nh), device=q.device, dtype=torch.float32)
        _launch("mlagg_local_attn_bwd", _ptr(q), q.stride(1), _ptr(kv), kv.stride(1), _ptr(lam), _ptr(subln_w), _ptr(lw), _ptr(dout), dos,
                _ptr(dq), dqs, _ptr(dkv), dkvs, _ptr(dlam), _ptr(dsub), _ptr(dlw), _ptr(dlb), _ptr(ws), B, H, W, nh, scale)
        return dq, dkv, dlam.reshape(()), dsub, dlw.reshape(lwshape), dlb, None, None, None, None, None, None


class PooledDiffAttnFn(torch.autograd.Function):
    """K4: fused pooled differential attention + RMSNorm (AggregatedAttention global branch)."""

    @staticmethod
    def forward(ctx, q, kp, vp, lam, subln_w, nh, scale, q_slot=None):
        ctx.slot = q_slot
        q, qs = _rows(q, "q")
        kp, kps = _rows(kp, "k_pool")
        vp, vps = _rows(vp, "v_pool")
        B, N, d = q.shape
        P = kp.shape[1]
        if d != nh * 48 or tuple(kp.shape) != (B, P, d) or tuple(vp.shape) != (B, P, d):
            raise RuntimeError(f"pooled_diff_attn: bad shapes q {tuple(q.shape)} k {tuple(kp.shape)} v {tuple(vp.shape)}")
        lam = _require(lam.reshape(1).contiguous(), "lambda")
        subln_w = _require(subln_w.contiguous(), "subln.weight", (48,))
        out = torch.empty(B, N, d, device=q.device, dtype=torch.float32)
        need = any(ctx.needs_input_grad)      # grad mode is off inside Function.forward
        lse = torch.empty(B, N, nh, 2, device=q.device, dtype=torch.float32) if need else None
        o_pre = torch.empty(B, N, d, device=q.device, dtype=torch.float32) if need else None
        _launch("mlagg_pooled_attn_fwd", _ptr(q), qs, _ptr(kp), kps, _ptr(vp), vps, _ptr(lam), _ptr(subln_w), _ptr(out), d, _ptr(lse),
                _ptr(o_pre), B, N, P, nh, float(scale))
        ctx.save_for_backward(q, kp, vp, lam, subln_w, lse, o_pre)
        ctx.geom = (nh, float(scale))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kp, vp, lam, subln_w, lse, o_pre = ctx.saved_tensors
        nh, scale = ctx.geom
        B, N, d = q.shape
        P = kp.shape[1]
        dout, dos = _rows(dout, "dout")
        dq, dqs = _grad_out(ctx.slot, (B, N, d), q.device)
        dkp = torch.empty(B, P, d, device=q.device, dtype=torch.float32)
        dvp = torch.empty(B, P, d, device=q.device, dtype=torch.float32)
        small = torch.zeros(1 + 48, device=q.device, dtype=torch.float32)
        ws = torch.empty(_lib.lib().mlagg_pooled_attn_bwd_workspace_floats(B, N, P, nh), device=q.device, dtype=torch.float32)
        _launch("mlagg_pooled_attn_bwd", _ptr(q), q.stride(1), _ptr(kp), kp.stride(1), _ptr(vp), vp.stride(1), _ptr(lam), _ptr(subln_w),
                _ptr(dout), dos, _ptr(lse), _ptr(o_pre), _ptr(dq), dqs, _ptr(dkp), d, _ptr(dvp), d, _ptr(small[:1]), _ptr(small[1:]),
                _ptr(ws), B, N, P, nh, scale)
        return dq, dkp, dvp, small[0].reshape(()), small[1:], None, None, None, None


class PooledDiffAttnLpFn(torch.autograd.Function):
    """K4lp: the pooled differential attention on the 16-bit matrix cores (csrc/pooled_attn_lp.hip) -- the 16-bit modes' form of K4:
    q * scale, k, v, the softmax weights and d(o) are bf16 / fp16 MFMA operands (what the reference's four flash_attn_func calls see,
    nnUNetTrainer_MLAgg_2D_dt_MS.py:733-751), sums / softmax / RMSNorm and every tensor in memory fp32."""

    @staticmethod
    def forward(ctx, q, kp, vp, lam, subln_w, nh, scale, cdt, q_slot=None):
        ctx.slot = q_slot
        q, qs = _rows(q, "q")
        kp, kps = _rows(kp, "k_pool")
        vp, vps = _rows(vp, "v_pool")
        B, N, d = q.shape
        P = kp.shape[1]
        if d != nh * 48 or tuple(kp.shape) != (B, P, d) or tuple(vp.shape) != (B, P, d):
            raise RuntimeError(f"pooled_diff_attn: bad shapes q {tuple(q.shape)} k {tuple(kp.shape)} v {tuple(vp.shape)}")
        lam = _require(lam.reshape(1).contiguous(), "lambda")
        subln_w = _require(subln_w.contiguous(), "subln.weight", (48,))
        out = torch.empty(B, N, d, device=q.device, dtype=torch.float32)
        need = any(ctx.needs_input_grad)
        lse = torch.empty(B, N, nh, 2, device=q.device, dtype=torch.float32) if need else None
        o12 = torch.empty(2, B, N, d, device=q.device, dtype=torch.float32) if need else None
        _launch("mlagg_pooled_attn_lp_fwd", _ptr(q), qs, _ptr(kp), kps, _ptr(vp), vps, _ptr(lam), _ptr(subln_w), _ptr(out), d, _ptr(lse),
                _ptr(o12[0]) if need else None, _ptr(o12[1]) if need else None, B, N, P, nh, float(scale), _LP_CODE[cdt])
        ctx.save_for_backward(q, kp, vp, lam, subln_w, lse, o12)
        ctx.geom = (nh, float(scale), cdt)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kp, vp, lam, subln_w, lse, o12 = ctx.saved_tensors
        nh, scale, cdt = ctx.geom
        B, N, d = q.shape
        P = kp.shape[1]
        dout, dos = _rows(dout, "dout")
        dq, dqs = _grad_out(ctx.slot, (B, N, d), q.device)
        dkp = torch.empty(B, P, d, device=q.device, dtype=torch.float32)
        dvp = torch.empty(B, P, d, device=q.device, dtype=torch.float32)
        small = torch.empty(1 + 48, device=q.device, dtype=torch.float32)
        ws = torch.empty(_lib.lib().mlagg_pooled_attn_lp_bwd_workspace_floats(B, N, P, nh), device=q.device, dtype=torch.float32)
        _launch("mlagg_pooled_attn_lp_bwd", _ptr(q), q.stride(1), _ptr(kp), kp.stride(1), _ptr(vp), vp.stride(1), _ptr(lam), _ptr(subln_w),
                _ptr(dout), dos, _ptr(lse), _ptr(o12[0]), _ptr(o12[1]), _ptr(dq), dqs, _ptr(dkp), d, _ptr(dvp), d, _ptr(small[:1]),
                _ptr(small[1:]), _ptr(ws), B, N, P, nh, scale, _LP_CODE[cdt])
        return dq, dkp, dvp, small[0].reshape(()), small[1:], None, None, None, None


class FlashAttnFn(torch.autograd.Function):
    """Boundary #3: softmax(q k^T scale) v on 16-bit (B, N, nh, 24) / (B, P, nh, 24) tensors, fp32 arithmetic."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        if not (q.is_cuda and q.dtype in _LP_CODE and k.dtype == q.dtype and v.dtype == q.dtype):
            raise RuntimeError("flash_attn_func: fp16 / bf16 tensors on the MI355X device expected "
                               f"(got {q.dtype}, {k.dtype}, {v.dtype} on {q.device})")
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, N, nh, e = q.shape
        P = k.shape[1]
        if tuple(k.shape) != (B, P, nh, e) or tuple(v.shape) != (B, P, nh, e):
            raise RuntimeError(f"flash_attn_func: bad shapes q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)}")
        out = torch.empty_like(q)
        need = any(ctx.needs_input_grad[:3])
        lse = torch.empty(B, nh, N, device=q.device, dtype=torch.float32) if need else None
        _launch("mlagg_flash_attn_fwd", _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), B, N, P, nh, e, float(scale), _LP_CODE[q.dtype])
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.scale = float(scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        B, N, nh, e = q.shape
        P = k.shape[1]
        dout = dout.contiguous().to(q.dtype)
        dq = torch.empty_like(q)
        ws = torch.empty(_lib.lib().mlagg_flash_attn_bwd_workspace_floats(B, N, P, nh, e), device=q.device, dtype=torch.float32)
        _launch("mlagg_flash_attn_bwd", _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(dout), _ptr(lse), _ptr(dq), _ptr(ws), B, N, P, nh, e,
                ctx.scale, _LP_CODE[q.dtype])
        dkv = ws[B * nh * N:].view(B, P, nh, 2, e)
        return dq, dkv[:, :, :, 0].to(q.dtype), dkv[:, :, :, 1].to(q.dtype), None


def flash_attn(q, k, v, softmax_scale=None):
    return FlashAttnFn.apply(q, k, v, q.shape[-1] ** -0.5 if softmax_scale is None else softmax_scale)


def local_diff_attn(q, kv, lam, subln_w, lepe_w, lepe_b, H, W, nh, scale):
    return LocalDiffAttnFn.apply(q, kv, lam, subln_w, lepe_w, lepe_b, H, W, nh, scale, claim_slot(q), claim_slot(kv))


def pooled_diff_attn(q, k_pool, v_pool, lam, subln_w, nh, scale):
    cdt = compute_dtype()
    if cdt != torch.float32 and k_pool.shape[1] <= 320:
        return PooledDiffAttnLpFn.apply(q, k_pool, v_pool, lam, subln_w, nh, scale, cdt, claim_slot(q))
    return PooledDiffAttnFn.apply(q, k_pool, v_pool, lam, subln_w, nh, scale, claim_slot(q))


# fp32 projections on the 16-bit matrix instructions (csrc/linear_lp.hip MODE 2: each fp32 operand as three bf16 pieces, six partial
# products, fp32 accumulation -- as accurate against float64 as the fp32 instruction, tools/bench_linear.py).  MLAGG_K5_X3=0: K5 on
# v_mfma_f32_32x32x2_f32.
K5_X3 = _os.environ.get("MLAGG_K5_X3", "1") == "1"
WGRAD_MIN_ROWS = int(_os.environ.get("MLAGG_WGRAD_MIN_ROWS", "0"))      # 0: by the state of the library (below); a number forces it
# K5w against the library's weight-gradient GEMM at short token counts (2 560): with the TUNED table loaded (gemm_tuning: the headline
# configuration) the library ties (35.88 vs 35.89 ms), so K5w starts at 8192 tokens; with the default heuristics (every other configuration)
# K5w wins 0.4 ms of the 224 x 224 bf16 step (profiles/round4_n_lp_k5_min_rows_ab.log) and starts at 2048
GEMM_TABLE_LOADED = [False]


def wgrad_min_rows():
    return WGRAD_MIN_ROWS if WGRAD_MIN_ROWS > 0 else (8192 if GEMM_TABLE_LOADED[0] else 2048)
# 16-bit modes: the one-product K5 from this many tokens on (2048 measured slower than the library's 16-bit GEMM: 28.81 vs 28.62 ms on config 3,
# profiles/round4_n_lp_k5_min_rows_ab.log)
LP_K5_MIN_ROWS = int(_os.environ.get("MLAGG_LP_K5_MIN_ROWS", "8192"))
K5_MIN_ROWS = int(_os.environ.get("MLAGG_K5_MIN_ROWS", "16384"))     # fp32 forward / dx: K5 from this many tokens on (at 10240 tokens the
#                            library's split-K kernels win: 80-320 K5 workgroups do not fill 256 CUs evenly; A/B on the step: +0.9 %)


def _rows2d(t, name):
    """(..., C) tensor -> (M, C) view with unit inner stride and one row stride; copies only if it must."""
    _require(t, name)
    t2 = t.reshape(-1, t.shape[-1])
    if t2.stride(1) != 1:
        t2 = t2.contiguous()
    return t2, t2.stride(0)


def _mfma_rows(t, name):
    """(..., C) -> (M, C) view usable by the MFMA projection kernels (unit inner stride, 16-byte aligned rows)."""
    t2, ts = _rows2d(t, name)
    if ts % 4 or t2.data_ptr() % 16:
        t2 = t2.contiguous()
        ts = t2.shape[1]
    return t2, ts


# ------------------------------------------------------------------------------------------------
# K5, round-4 form (csrc/linear_x3.hip): the weight operand is an IMAGE (its three bf16 pieces, laid out for the kernel; the same for
# W^T for the data gradient), built once per step for every projection of a network in ONE launch (WeightImageSet) or, for a weight
# nobody registered, on the fly.
# ------------------------------------------------------------------------------------------------
# end of round 4: stages 2 / 3 (10 240 / 2 560 tokens) too -- against the TUNED library GEMMs the kernel wins 11 of 16 products there
# (tools/bench_linear_x3.py with BENCH_TUNED_GEMM=1) and the step 0.1-0.3 ms on two boxes (profiles/round4_m_x3_min_rows_ab.log); mid-round,
# before the fused Mlp epilogues and the per-network image set, the same switch had lost 0.2 ms
X3_MIN_ROWS = int(_os.environ.get("MLAGG_X3_MIN_ROWS", "2048"))
_IMAGE_EPOCH = [0]              # bumped by whatever rewrites parameters behind autograd's back (ClipAdamW's raw-pointer update)


def invalidate_weight_images():
    _IMAGE_EPOCH[0] += 1


def image_epoch():
    return _IMAGE_EPOCH[0]


def _image_pair(w):
    """(img, imgT) of a contiguous fp32 (N, K) matrix, built now (one launch)."""
    N, K = w.shape
    lib = _lib.lib()
    img = torch.empty(lib.mlagg_weight_image_bytes(N, K), dtype=torch.uint8, device=w.device)
    imgT = torch.empty(lib.mlagg_weight_image_bytes(K, N), dtype=torch.uint8, device=w.device)
    _launch("mlagg_weight_image", _ptr(w), K, _ptr(img), _ptr(imgT), N, K)
    return img, imgT


class WeightImageSet:
    """The weight images of one network.  The first forward pass under ``with images:`` records which persistent matrices (parameters
    and stacked-weight buffers) the projections ask for; from then on ``begin`` rebuilds all their images with one launch over a
    device table, and lookups are a dictionary hit checked against the matrix's version counter (an in-place change since the build
    -- a stack refreshed again, a loaded checkpoint -- falls back to building that one image on the fly)."""

    active = None

    def __init__(self):
        self.tensors, self.entries, self.table, self.store, self.ptrs, self.max_tiles, self.built = [], {}, None, None, None, 0, None

    def _rebuild_table(self):
        import numpy as np
        lib = _lib.lib()
        dev = self.tensors[0].device
        sizes = [(lib.mlagg_weight_image_bytes(*t.shape), lib.mlagg_weight_image_bytes(t.shape[1], t.shape[0])) for t in self.tensors]
        offs, total = [], 0
        for a, b in sizes:
            offs.append((total, total + ((a + 255) & ~255)))
            total += ((a + 255) & ~255) + ((b + 255) & ~255)
        self.store = torch.empty(total, dtype=torch.uint8, device=dev)
        base = self.store.data_ptr()
        jobs = np.zeros(len(self.tensors), dtype=np.dtype([("w", "<u8"), ("img", "<u8"), ("imgT", "<u8"), ("N", "<i4"), ("K", "<i4"),
                                                           ("ws", "<i4"), ("pad", "<i4")]))
        self.views, self.max_tiles = [], 0
        for i, (t, (oa, ob), (sa, sb)) in enumerate(zip(self.tensors, offs, sizes)):
            N, K = t.shape
            jobs[i] = (t.data_ptr(), base + oa, base + ob, N, K, K, 0)
            self.views.append((self.store[oa:oa + sa], self.store[ob:ob + sb]))
            self.max_tiles = max(self.max_tiles, ((N + 31) // 32) * ((K + 31) // 32))
        self.table = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
        self.ptrs = tuple(t.data_ptr() for t in self.tensors)

    def begin(self):
        WeightImageSet.active = self
        if not self.tensors:
            return
        if self.table is None or self.ptrs != tuple(t.data_ptr() for t in self.tensors):
            self._rebuild_table()
            self.built = None
        ep = _IMAGE_EPOCH[0]
        sig = (ep,) + tuple(t._version for t in self.tensors)
        if sig == self.built and not torch.cuda.is_current_stream_capturing():
            return                                    # nothing changed since the last build (inference loops, a second forward of a step)
        _launch("mlagg_weight_images", _ptr(self.table), len(self.tensors), self.max_tiles)
        self.built = sig
        self.entries = {t.data_ptr(): (t._version, ep, v) for t, v in zip(self.tensors, self.views)}

    def end(self):
        WeightImageSet.active = None

    def __enter__(self):
        self.begin()
        return self

    def __exit__(self, *exc):
        self.end()
        return False

    def lookup(self, w):
        e = self.entries.get(w.data_ptr())
        if e is not None and e[0] == w._version and e[1] == _IMAGE_EPOCH[0]:
            return e[2]
        pair = _image_pair(w)
        # what is worth keeping: a parameter, or the buffer behind a stacked-weight view.  Never the view itself: a tensor with a
        # grad_fn keeps the AccumulateGrad nodes of an earlier iteration alive, and autograd then runs them on the stream they were
        # created on -- inside a hipGraph capture that cross-stream hand-off is a segmentation fault
        keep = getattr(w, "_mlagg_buffer", w if isinstance(w, torch.nn.Parameter) else None)
        if keep is not None and keep.grad_fn is None and keep.dim() == 2 and keep.is_contiguous() and \
                keep.data_ptr() == w.data_ptr() and all(keep.data_ptr() != t.data_ptr() for t in self.tensors):
            self.tensors.append(keep)               # from the next forward on: part of the one-launch build
            self.table = None
        return pair


def weight_images(w):
    """(img, imgT) of the contiguous (N, K) matrix ``w`` that are current NOW."""
    s = WeightImageSet.active
    return _image_pair(w) if s is None else s.lookup(w)


def _x3_ok(M, N, K):
    return M >= X3_MIN_ROWS and bool(_lib.lib().mlagg_linear_x3_supported(M, N, K))


def _x3(x2, xs, img, bias, M, N, K, epilogue=0, pre=None, pre_stride=0, out_shape=None, out=None, out_stride=None):
    """One launch of mlagg_linear_x3; returns y, or (pre-activation, activation) for the GELU epilogue.  ``out`` / ``out_stride``: a
    destination the caller owns (rows of out_stride floats: a column block of a wider buffer)."""
    y = out if out is not None else torch.empty(out_shape if out_shape is not None else (M, N), device=x2.device, dtype=torch.float32)
    ys = N if out_stride is None else out_stride
    act = torch.empty_like(y) if epilogue == 1 else None
    _flop("K5", 2 * M * N * K)
    _launch("mlagg_linear_x3", _ptr(x2), xs, _ptr(img), _ptr(bias), _ptr(y), ys, _ptr(act), _ptr(pre), pre_stride, M, N, K, epilogue)
    return y if epilogue != 1 else (y, act)


def _linear_wgrad(dy2, dys, x, O, I, has_bias, kernel):
    """dW (O, I) and db (O) of a token-major Linear: on K5w (kernel "K5w"), else the library GEMM + K8 column sums."""
    M = dy2.shape[0]
    x2, xs = _rows2d(x, "x")
    if kernel == "K5w":
        # dW | db in one allocation (every entry is written by the reduction)
        buf = torch.empty(O * I + (O if has_bias else 0), device=dy2.device, dtype=torch.float32)
        dW = buf[:O * I].view(O, I)
        db = buf[O * I:] if has_bias else None
        ws = torch.empty(_lib.lib().mlagg_linear_wgrad_workspace_floats(M, O, I), device=dy2.device, dtype=torch.float32)
        _flop("K5w", 2 * M * O * I)
        _launch("mlagg_linear_wgrad_x3" if K5_X3 else "mlagg_linear_wgrad", _ptr(dy2), dys, _ptr(x2), xs, _ptr(dW), _ptr(db), _ptr(ws),
                M, O, I)
        return dW, db
    dW = dy2.t().matmul(x2)
    db = (column_sum(dy2) if dy2.is_cuda else dy2.sum(0)) if has_bias else None
    return dW, db


def linear_plan(M, O, I, cdt, on_device):
    """Where each product of the token-major projection y (M, O) = x (M, I) W^T + b runs in compute dtype `cdt`: (forward, data
    gradient, weight gradient) -- "K5x3" (on weight images), "K5" or None (the library in `cdt`) for the first two, "K5w" or None
    (the library GEMM + K8 column sums) for the third.  Which K5 entry point runs is the mode's (MLAGG_K5_X3, `cdt`), not the plan's.
    A function of shapes, `cdt`, device-ness and the switches and thresholds above only, read at each call."""
    if not on_device:
        return None, None, None
    fp32 = cdt == torch.float32
    k5 = M >= (K5_MIN_ROWS if fp32 else LP_K5_MIN_ROWS) and I % 4 == 0
    fwd = "K5x3" if fp32 and _x3_ok(M, O, I) else ("K5" if k5 else None)
    dgrad = "K5x3" if fwd == "K5x3" and _x3_ok(M, I, O) else ("K5" if k5 and O % 4 == 0 else None)
    return fwd, dgrad, "K5w" if M >= wgrad_min_rows() else None


_X3_PAIR = ("K5x3", "K5x3")


class LinearFn(torch.autograd.Function):
    """y = x W^T + b for token-major activations, each product where the plan says (linear_plan unless one is given): forward and
    dx on K5 (on weight images, or the round-3 kernels) or the library, dW / db on K5w or the library."""

    @staticmethod
    def forward(ctx, x, weight, bias, slot=None, plan=None):
        ctx.save_for_backward(x, weight)
        ctx.slot = slot
        ctx.has_bias = bias is not None
        ctx.cdt = cdt = compute_dtype()
        ctx.imgT = None
        O, I = weight.shape
        M = x.numel() // I
        ctx.plan = plan = plan or linear_plan(M, O, I, cdt, x.is_cuda)
        if plan[0] is None:
            if cdt != torch.float32:
                return torch.nn.functional.linear(x.to(cdt), weight.to(cdt), lp(bias, cdt)).float()
            return torch.nn.functional.linear(x, weight, bias)
        x2, xs = _mfma_rows(x, "x")
        w = _require(weight.contiguous(), "weight")
        if plan[0] == "K5x3":
            img, ctx.imgT = weight_images(w)
            return _x3(x2, xs, img, bias, M, O, I, out_shape=x.shape[:-1] + (O,))
        y = torch.empty(x.shape[:-1] + (O,), device=x.device, dtype=torch.float32)
        _flop("K5", 2 * M * O * I)
        if cdt == torch.float32 and not K5_X3:
            _launch("mlagg_linear_fwd", _ptr(x2), xs, _ptr(w), _ptr(bias), _ptr(y), O, M, O, I)
        else:                           # split-bf16 (fp32) or one-product (16-bit) operands
            _launch("mlagg_linear_lp_fwd", _ptr(x2), xs, _ptr(w), _ptr(bias), _ptr(y), O, M, O, I,
                    _DTYPE_BF16X3 if cdt == torch.float32 else _LP_CODE[cdt])
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dW = db = None
        O, I = weight.shape
        cdt, (_, dgrad, wgrad) = ctx.cdt, ctx.plan
        dy2, dys = _mfma_rows(dy, "dy")
        M = dy2.shape[0]
        if ctx.needs_input_grad[0]:
            if dgrad == "K5x3":
                # dx = dy . W on the image of W^T built with the forward's image (no per-step transpose of the weight); a claimed
                # split_cols slot: written straight into the shared gradient buffer of the pieces
                if ctx.slot is not None:
                    dx, dxs = _grad_out(ctx.slot, x.shape, dy.device)
                    _x3(dy2, dys, ctx.imgT, None, M, I, O, out=dx, out_stride=dxs)
                else:
                    dx = _x3(dy2, dys, ctx.imgT, None, M, I, O, out_shape=x.shape)
            elif dgrad == "K5":
                w = _require(weight.contiguous(), "weight")
                dx = torch.empty(x.shape, device=dy.device, dtype=torch.float32)
                _flop("K5", 2 * M * O * I)
                if cdt == torch.float32 and K5_X3:
                    # dx = dy . W as the forward form of the kernel on W^T (I, O): its weight tile is then read along the
                    # contraction, the fast staging path (the transpose is a (O, I) copy of a few hundred KB)
                    wt = transpose_2d(w.unsqueeze(0))[0]
                    _launch("mlagg_linear_lp_fwd", _ptr(dy2), dys, _ptr(wt), None, _ptr(dx), I, M, I, O, _DTYPE_BF16X3)
                elif cdt == torch.float32:
                    _launch("mlagg_linear_dgrad", _ptr(dy2), dys, _ptr(w), _ptr(dx), I, M, O, I)
                else:
                    _launch("mlagg_linear_lp_dgrad", _ptr(dy2), dys, _ptr(w), _ptr(dx), I, M, O, I, _LP_CODE[cdt])
            elif cdt != torch.float32:
                dx = dy.to(cdt).matmul(weight.to(cdt)).float()
            else:
                dx = dy.matmul(weight)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            # weight / bias gradients stay fp32 in every mode (K5w: the token sum is the long one)
            dW, db = _linear_wgrad(dy2, dys, x, O, I, ctx.has_bias, wgrad)
        return dx, dW, db, None, None


def linear(x, weight, bias=None, plan=None):
    """The token-major projection on linear_plan's kernels (`plan`: that plan, when the caller has it).  A split_cols piece as
    input: its gradient is written in place when forward and data gradient both run on K5x3."""
    if plan is None:
        O, I = weight.shape
        plan = linear_plan(x.numel() // I, O, I, compute_dtype(), x.is_cuda)
    slot = claim_slot(x) if plan[:2] == _X3_PAIR else None
    return LinearFn.apply(x, weight, bias, slot, plan)


class MlpFn(torch.autograd.Function):
    """fc2(GELU(fc1(x))) of reference Mlp (T:176-192) as four K5 launches: fc1 writes the pre-activation AND its GELU, and in backward
    the data gradient of fc2 comes out already multiplied by GELU'(pre) -- the two elementwise GELU passes of the ATen form are gone.
    `wgrads`: the weight-gradient kernels of fc1 and fc2 (linear_plan's third entries)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, wgrads):
        H, I = w1.shape
        O = w2.shape[0]
        M = x.numel() // I
        x2, xs = _mfma_rows(x, "x")
        w1c, w2c = _require(w1.contiguous(), "fc1.weight"), _require(w2.contiguous(), "fc2.weight")
        img1, img1T = weight_images(w1c)
        img2, img2T = weight_images(w2c)
        pre, act = _x3(x2, xs, img1, b1, M, H, I, epilogue=1)
        y = _x3(act, H, img2, b2, M, O, H, out_shape=x.shape[:-1] + (O,))
        ctx.save_for_backward(x, w1, w2, pre, act)
        ctx.images = (img1T, img2T)
        ctx.bias = (b1 is not None, b2 is not None)
        ctx.wgrads = wgrads
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2, pre, act = ctx.saved_tensors
        img1T, img2T = ctx.images
        H, I = w1.shape
        O = w2.shape[0]
        dy2, dys = _mfma_rows(dy, "dy")
        M = dy2.shape[0]
        dW2, db2 = _linear_wgrad(dy2, dys, act, O, H, ctx.bias[1], ctx.wgrads[1])
        dpre = _x3(dy2, dys, img2T, None, M, H, O, epilogue=2, pre=pre, pre_stride=H)          # (dy . W2) * GELU'(pre)
        dW1, db1 = _linear_wgrad(dpre, H, x, H, I, ctx.bias[0], ctx.wgrads[0])
        dx = _x3(dpre, H, img1T, None, M, I, H, out_shape=x.shape) if ctx.needs_input_grad[0] else None
        return dx, dW1, db1, dW2, db2, None


def _mlp_plans(x, w1, w2):
    (H, I), O, cdt = w1.shape, w2.shape[0], compute_dtype()
    M = x.numel() // I
    return linear_plan(M, H, I, cdt, x.is_cuda), linear_plan(M, O, H, cdt, x.is_cuda)


def mlp_supported(x, w1, w2):
    """Does ops.mlp run MlpFn: forward and data gradient of both layers on K5x3?"""
    p1, p2 = _mlp_plans(x, w1, w2)
    return p1[:2] == p2[:2] == _X3_PAIR


def mlp(x, w1, b1, w2, b2):
    """fc2(GELU(fc1(x))): MlpFn where both layers run forward and data gradient on K5x3, else the two projections and GELU."""
    p1, p2 = _mlp_plans(x, w1, w2)
    if p1[:2] == p2[:2] == _X3_PAIR:
        return MlpFn.apply(x, w1, b1, w2, b2, (p1[2], p2[2]))
    return linear(torch.nn.functional.gelu(linear(x, w1, b1, p1)), w2, b2, p2)


class LayerNormFn(torch.autograd.Function):
    """K6: LayerNorm over the last dimension (C in {48, 96, 192, 384, 768})."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        C = x.shape[-1]
        x2, xs = _rows2d(x, "x")
        if xs % 4 or x2.data_ptr() % 16:
            x2 = x2.contiguous()
            xs = C
        rows = x2.shape[0]
        y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        stats = torch.empty(rows, 2, device=x.device, dtype=torch.float32)
        _launch("mlagg_layernorm_fwd", _ptr(x2), xs, _ptr(weight), _ptr(bias), _ptr(y), _ptr(stats), rows, C, float(eps))
        ctx.save_for_backward(x2, weight, stats)
        ctx.has_bias = bias is not None
        ctx.xshape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, weight, stats = ctx.saved_tensors
        rows, C = x2.shape
        dy2, dys = _rows2d(dy, "dy")
        if dys % 4 or dy2.data_ptr() % 16:
            dy2 = dy2.contiguous()
            dys = C
        dx = torch.empty(ctx.xshape, device=dy.device, dtype=torch.float32)
        dg = torch.empty(C, device=dy.device, dtype=torch.float32)
        db = torch.empty(C, device=dy.device, dtype=torch.float32) if ctx.has_bias else None
        ws = torch.empty(_lib.lib().mlagg_layernorm_bwd_workspace_floats(rows, C), device=dy.device, dtype=torch.float32)
        _launch("mlagg_layernorm_bwd", _ptr(x2), x2.stride(0), _ptr(dy2), dys, _ptr(weight), _ptr(stats), _ptr(dx), _ptr(dg), _ptr(db),
                _ptr(ws), rows, C)
        return dx, dg, db, None


def layer_norm(x, weight, bias, eps=1e-5):
    """LayerNorm over the last dimension: K6 for the channel counts of the MLAgg-UNet path, ATen otherwise."""
    if _lib.lib().mlagg_layernorm_supported(int(x.shape[-1])):
        return LayerNormFn.apply(x, weight, bias, eps)
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), weight, bias, eps)


class ResidualLayerNormFn(torch.autograd.Function):
    """K6 with the residual junction in front: (xsum, y) = (skip + branch * scale[sample], LayerNorm(xsum)); backward adds the
    gradient reaching xsum from its other consumers inside the LayerNorm-backward kernel (no separate add / scale kernels)."""

    @staticmethod
    def forward(ctx, skip, branch, scale, weight, bias, eps):
        skip = _require(skip.contiguous(), "skip")
        branch = _require(branch.contiguous(), "branch")
        if skip.shape != branch.shape:
            raise RuntimeError("residual_layer_norm: skip and branch differ in shape")
        C = skip.shape[-1]
        rows = skip.numel() // C
        B = skip.shape[0]
        if scale is not None:
            scale = _require(scale.reshape(-1).contiguous(), "scale", (B,))
        xsum = torch.empty_like(skip)
        y = torch.empty_like(skip)
        stats = torch.empty(rows, 2, device=skip.device, dtype=torch.float32)
        _launch("mlagg_residual_layernorm_fwd", _ptr(skip), _ptr(branch), _ptr(scale), _ptr(weight), _ptr(bias), _ptr(xsum), _ptr(y),
                _ptr(stats), rows, rows // B, C, float(eps))
        ctx.save_for_backward(xsum, weight, stats, scale)
        ctx.has_bias = bias is not None
        return xsum, y

    @staticmethod
    def backward(ctx, dxsum, dy):
        xsum, weight, stats, scale = ctx.saved_tensors
        C = xsum.shape[-1]
        rows = xsum.numel() // C
        B = xsum.shape[0]
        if dy is None:                  # the norm's output went nowhere: a plain residual junction
            dres = _require(dxsum.contiguous(), "dxsum")
            dbranch = dres if scale is None else dres * scale.view((-1,) + (1,) * (dres.dim() - 1))
            return dres, dbranch, None, torch.zeros_like(weight), (torch.zeros_like(weight) if ctx.has_bias else None), None
        dy2, dys = _rows2d(dy, "dy")
        if dys % 4 or dy2.data_ptr() % 16:
            dy2 = dy2.contiguous()
            dys = C
        dres = None if dxsum is None else _require(dxsum.contiguous(), "dxsum")
        dskip = torch.empty_like(xsum)
        dbranch = torch.empty_like(xsum) if scale is not None else None
        dg = torch.empty(C, device=dy.device, dtype=torch.float32)
        db = torch.empty(C, device=dy.device, dtype=torch.float32) if ctx.has_bias else None
        ws = torch.empty(_lib.lib().mlagg_layernorm_bwd_workspace_floats(rows, C), device=dy.device, dtype=torch.float32)
        _launch("mlagg_residual_layernorm_bwd", _ptr(xsum), _ptr(dy2), dys, _ptr(dres), _ptr(scale), _ptr(weight), _ptr(stats), _ptr(dskip),
                _ptr(dbranch), _ptr(dg), _ptr(db), _ptr(ws), rows, rows // B, C)
        return dskip, (dskip if dbranch is None else dbranch), None, dg, db, None


def residual_layer_norm(skip, branch, scale, weight, bias, eps=1e-5):
    """(skip + branch * scale[sample], LayerNorm of that sum) in one pass each way; scale None: plain sum."""
    if not _lib.lib().mlagg_layernorm_supported(int(skip.shape[-1])):
        raise RuntimeError(f"residual_layer_norm: {skip.shape[-1]} channels are outside K6's row shapes")
    return ResidualLayerNormFn.apply(skip, branch, scale, weight, bias, eps)


class DWConv3x3NCHWFn(torch.autograd.Function):
    """K2n: depthwise 3x3 (stride 1 or 2, padding 1) + bias on NCHW maps."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        x = _require(x.contiguous(), "x")
        B, C, H, W = x.shape
        w = _require(weight.reshape(C, 9).contiguous(), "weight")
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty(B, C, Ho, Wo, device=x.device, dtype=torch.float32)
        _launch("mlagg_dwconv3x3_nchw_fwd", _ptr(x), _ptr(w), _ptr(bias), _ptr(y), B, C, H, W, int(stride))
        ctx.save_for_backward(x, w)
        ctx.meta = (int(stride), bias is not None, weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, has_bias, wshape = ctx.meta
        B, C, H, W = x.shape
        dy = _require(dy.contiguous(), "dy")
        dx = torch.empty_like(x)
        dw = torch.empty(C, 9, device=x.device, dtype=torch.float32)
        db = torch.empty(C, device=x.device, dtype=torch.float32) if has_bias else None
        ws = torch.empty(_lib.lib().mlagg_dwconv3x3_nchw_bwd_workspace_floats(B, C, H, W, stride), device=x.device,
                         dtype=torch.float32)
        _launch("mlagg_dwconv3x3_nchw_bwd", _ptr(x), _ptr(w), _ptr(dy), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws), B, C, H, W, stride)
        return dx, dw.reshape(wshape), db, None


def dwconv3x3_nchw(x, weight, bias, stride=1):
    return DWConv3x3NCHWFn.apply(x, weight, bias, stride)


DWC_RES = _os.environ.get("MLAGG_DWC_RES", "1") == "1"


class DWConvResNCHWFn(torch.autograd.Function):
    """(conv1(x), x) of a residual MedNeXtBlock (T:256-300: ``x1 = conv1(x) ... x1 = x + x1``): the block input goes through K2n and, as
    the second output, on to the residual sum.  Backward receives both gradients of x and K2n's data-gradient kernel sums them
    (mlagg_dwconv3x3_nchw_bwd_res) -- autograd's add_ kernel over the map (three per stage, 161 us of the step) is gone."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = _require(x.contiguous(), "x")
        B, C, H, W = x.shape
        w = _require(weight.reshape(C, 9).contiguous(), "weight")
        y = torch.empty(B, C, H, W, device=x.device, dtype=torch.float32)
        _launch("mlagg_dwconv3x3_nchw_fwd", _ptr(x), _ptr(w), _ptr(bias), _ptr(y), B, C, H, W, 1)
        ctx.save_for_backward(x, w)
        ctx.meta = (bias is not None, weight.shape)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dres):
        x, w = ctx.saved_tensors
        has_bias, wshape = ctx.meta
        B, C, H, W = x.shape
        if dy is None:                                            # only the residual path carried a gradient
            return dres, None, None
        dy = _require(dy.contiguous(), "dy")
        if dres is not None:
            dres = _require(dres.contiguous(), "dres")
            if dres.dtype != torch.float32:
                dres = dres.float()
        dx = torch.empty_like(x)
        dw = torch.empty(C, 9, device=x.device, dtype=torch.float32)
        db = torch.empty(C, device=x.device, dtype=torch.float32) if has_bias else None
        ws = torch.empty(_lib.lib().mlagg_dwconv3x3_nchw_bwd_workspace_floats(B, C, H, W, 1), device=x.device, dtype=torch.float32)
        _launch("mlagg_dwconv3x3_nchw_bwd_res", _ptr(x), _ptr(w), _ptr(dy), _ptr(dres), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws), B, C, H, W,
                1)
        return dx, dw.reshape(wshape), db


def dwconv3x3_nchw_res(x, weight, bias):
    """(conv(x), x): the depthwise convolution and the map itself for the block's residual sum; None when the fused backward does not
    apply (the caller keeps the plain form)."""
    if not (DWC_RES and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[3] % 4 == 0 and x.requires_grad
            and torch.is_grad_enabled()):
        return None
    return DWConvResNCHWFn.apply(x, weight, bias)


def _int_array(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _xscan(tok, tok_stride, blk_stride, seq, B, HW, CB, nblk, merge):
    Hs, Ws = _int_array([h for h, _ in HW]), _int_array([w for _, w in HW])
    if merge:
        _launch("mlagg_cross_merge", _ptr(seq), tok, tok_stride, blk_stride, B, len(HW), Hs, Ws, CB, nblk)
    else:
        _launch("mlagg_cross_scan", tok, tok_stride, blk_stride, _ptr(seq), B, len(HW), Hs, Ws, CB, nblk)


class CrossScanFn(torch.autograd.Function):
    """K1' scatter: token-major (B, L_cat, nblk*CB) -> (B, 4*CB, L_cat) scan sequences (nblk = 1: the four
    directions share the source; nblk = 4: direction k reads channel block k)."""

    @staticmethod
    def forward(ctx, tok, HW, CB, nblk):
        tok = _require(tok.contiguous(), "tok")
        B, Lc, width = tok.shape
        if Lc != sum(h * w for h, w in HW) or width != nblk * CB:
            raise RuntimeError(f"cross_scan: bad shape {tuple(tok.shape)} for maps {HW}, CB {CB}, nblk {nblk}")
        seq = torch.empty(B, 4 * CB, Lc, device=tok.device, dtype=torch.float32)
        _xscan(tok.data_ptr(), width, CB, seq, B, HW, CB, nblk, merge=False)
        ctx.meta = (tuple(HW), CB, nblk, width)
        return seq

    @staticmethod
    def backward(ctx, dseq):
        HW, CB, nblk, width = ctx.meta
        dseq = _require(dseq.contiguous(), "dseq")
        B, _, Lc = dseq.shape
        dtok = torch.empty(B, Lc, width, device=dseq.device, dtype=torch.float32)
        _xscan(dtok.data_ptr(), width, CB, dseq, B, HW, CB, nblk, merge=True)
        return dtok, None, None, None


class CrossMergeFn(torch.autograd.Function):
    """K1' gather: (B, 4*CB, L_cat) scan-order outputs -> (B, L_cat, CB) token-major sum of the four directions."""

    @staticmethod
    def forward(ctx, seq, HW, CB):
        seq = _require(seq.contiguous(), "seq")
        B, rows, Lc = seq.shape
        if rows != 4 * CB or Lc != sum(h * w for h, w in HW):
            raise RuntimeError(f"cross_merge: bad shape {tuple(seq.shape)}")
        tok = torch.empty(B, Lc, CB, device=seq.device, dtype=torch.float32)
        _xscan(tok.data_ptr(), CB, CB, seq, B, HW, CB, 1, merge=True)
        ctx.meta = (tuple(HW), CB)
        return tok

    @staticmethod
    def backward(ctx, dtok):
        HW, CB = ctx.meta
        dtok = _require(dtok.contiguous(), "dtok")
        B, Lc, _ = dtok.shape
        dseq = torch.empty(B, 4 * CB, Lc, device=dtok.device, dtype=torch.float32)
        _xscan(dtok.data_ptr(), CB, CB, dseq, B, HW, CB, 1, merge=False)
        return dseq, None, None


class CrossScanBCFn(torch.autograd.Function):
    """The single consumer of the token-major x_proj output (B, L_cat, 4*35), split as at MambaSkip.py:433:
    direction k's dt columns [35k, 35k+3), B columns [35k+3, 35k+19) and C columns [35k+19, 35k+35) all come back as
    scan-order rows -- (B, 4, 3, L_cat), (B, 4, 16, L_cat), (B, 4, 16, L_cat) -- for the low-rank selective scan.
    One backward assembles the whole x_proj gradient (no per-slice zero-fills and accumulations)."""

    @staticmethod
    def forward(ctx, xdbl, HW, dt_rank, d_state):
        xdbl = _require(xdbl.contiguous(), "x_dbl")
        B, Lc, width = xdbl.shape
        per = dt_rank + 2 * d_state
        if width != 4 * per:
            raise RuntimeError("cross_scan_bc: x_dbl must hold 4 directions")
        Bs = torch.empty(B, 4 * d_state, Lc, device=xdbl.device, dtype=torch.float32)
        Cs = torch.empty(B, 4 * d_state, Lc, device=xdbl.device, dtype=torch.float32)
        base = xdbl.data_ptr()
        _xscan(base + 4 * dt_rank, width, per, Bs, B, HW, d_state, 4, merge=False)
        _xscan(base + 4 * (dt_rank + d_state), width, per, Cs, B, HW, d_state, 4, merge=False)
        dtr = torch.empty(B, 4 * dt_rank, Lc, device=xdbl.device, dtype=torch.float32)
        _xscan(base, width, per, dtr, B, HW, dt_rank, 4, merge=False)
        ctx.meta = (tuple(HW), dt_rank, d_state, width)
        return dtr.view(B, 4, dt_rank, Lc), Bs.view(B, 4, d_state, Lc), Cs.view(B, 4, d_state, Lc)

    @staticmethod
    def backward(ctx, ddtr, dBs, dCs):
        HW, dt_rank, d_state, width = ctx.meta
        per = dt_rank + 2 * d_state
        dBs = _require(dBs.contiguous(), "dBs")
        dCs = _require(dCs.contiguous(), "dCs")
        B, Lc = dBs.shape[0], dBs.shape[-1]
        ddtr = _require(ddtr.contiguous(), "ddtr")
        dx = torch.empty(B, Lc, width, device=dBs.device, dtype=torch.float32)
        base = dx.data_ptr()
        _xscan(base, width, per, ddtr, B, HW, dt_rank, 4, merge=True)
        _xscan(base + 4 * dt_rank, width, per, dBs, B, HW, d_state, 4, merge=True)
        _xscan(base + 4 * (dt_rank + d_state), width, per, dCs, B, HW, d_state, 4, merge=True)
        return dx, None, None, None


class IndexScanFn(torch.autograd.Function):
    """K1' for volumes: token-major (B, L, width) -> scan rows (B, K*CB, L) by permutation table idx (K, L) int32; direction k
    reads columns [k*blk, k*blk + CB) of the source (blk = 0: every direction reads the same CB columns)."""

    @staticmethod
    def forward(ctx, tok, idx, CB, blk, col0):
        tok = _require(tok.contiguous(), "tok")
        B, L, width = tok.shape
        K = idx.shape[0]
        if idx.dtype != torch.int32 or tuple(idx.shape) != (K, L) or not idx.is_cuda or col0 + (K - 1) * blk + CB > width:
            raise RuntimeError("index_scan: idx must be an int32 (K, L) device table and the column blocks must fit the rows")
        seq = torch.empty(B, K * CB, L, device=tok.device, dtype=torch.float32)
        _launch("mlagg_index_scan", tok.data_ptr() + 4 * col0, width, blk, _ptr(idx), _ptr(seq), B, L, K, CB)
        ctx.save_for_backward(idx)
        ctx.meta = (CB, blk, col0, width)
        return seq

    @staticmethod
    def backward(ctx, dseq):
        (idx,) = ctx.saved_tensors
        CB, blk, col0, width = ctx.meta
        dseq = _require(dseq.contiguous(), "dseq")
        B, _, L = dseq.shape
        K = idx.shape[0]
        if blk == 0 and width == CB:
            dtok = torch.empty(B, L, width, device=dseq.device, dtype=torch.float32)      # the summed form zero-fills itself
            _launch("mlagg_index_merge", _ptr(dseq), _ptr(idx), _ptr(dtok), width, 0, B, L, K, CB)
            return dtok, None, None, None, None
        if blk == 0:
            raise RuntimeError("index_scan: a shared source must be exactly CB columns wide")
        dtok = torch.zeros(B, L, width, device=dseq.device, dtype=torch.float32)
        _launch("mlagg_index_merge", _ptr(dseq), _ptr(idx), dtok.data_ptr() + 4 * col0, width, blk, B, L, K, CB)
        return dtok, None, None, None, None


class IndexMergeFn(torch.autograd.Function):
    """(B, K*CB, L) scan-order outputs -> (B, L, CB) token-major SUM of the K directions (SS3D.forward's torch.sum(y, dim=1))."""

    @staticmethod
    def forward(ctx, seq, idx, CB):
        seq = _require(seq.contiguous(), "seq")
        B, rows, L = seq.shape
        K = idx.shape[0]
        if rows != K * CB or tuple(idx.shape) != (K, L) or idx.dtype != torch.int32:
            raise RuntimeError(f"index_merge: bad shapes seq {tuple(seq.shape)} idx {tuple(idx.shape)}")
        tok = torch.empty(B, L, CB, device=seq.device, dtype=torch.float32)
        if K > 1 and CB % 4 == 0:
            # every direction into its own column block (plain stores), then the K blocks summed in a fixed order: deterministic,
            # and faster than K float-atomic read-modify-writes per output
            wide = torch.empty(B, L, K * CB, device=seq.device, dtype=torch.float32)
            _launch("mlagg_index_merge", _ptr(seq), _ptr(idx), _ptr(wide), K * CB, CB, B, L, K, CB)
            _launch("mlagg_block_sum", _ptr(wide), _ptr(tok), B * L, K, CB)
        else:
            _launch("mlagg_index_merge", _ptr(seq), _ptr(idx), _ptr(tok), CB, 0, B, L, K, CB)
        ctx.save_for_backward(idx)
        ctx.CB = CB
        return tok

    @staticmethod
    def backward(ctx, dtok):
        (idx,) = ctx.saved_tensors
        dtok = _require(dtok.contiguous(), "dtok")
        B, L, CB = dtok.shape
        K = idx.shape[0]
        dseq = torch.empty(B, K * CB, L, device=dtok.device, dtype=torch.float32)
        _launch("mlagg_index_scan", _ptr(dtok), CB, 0, _ptr(idx), _ptr(dseq), B, L, K, CB)
        return dseq, None, None


class IndexScanBCFn(torch.autograd.Function):
    """The single consumer of the token-major x_proj output of the d_state = 1 blocks, (B, L, K * (R + 2)) split per direction as
    [dt (R) | B | C] (UMambaEnc_SS3D.py:262-263): scan-order rows dtr (B, K, R, L), Bs (B, K, L), Cs (B, K, L).  One backward
    assembles the whole x_proj gradient (every column is written: no zero-fill, no per-slice accumulation)."""

    @staticmethod
    def forward(ctx, xdbl, idx, R):
        xdbl = _require(xdbl.contiguous(), "x_dbl")
        B, L, width = xdbl.shape
        K, per = idx.shape[0], R + 2
        if width != K * per or idx.dtype != torch.int32 or tuple(idx.shape) != (K, L) or not idx.is_cuda:
            raise RuntimeError("index_scan_bc: x_dbl must be (B, L, K * (R + 2)) and idx an int32 (K, L) device table")
        dtr = torch.empty(B, K * R, L, device=xdbl.device, dtype=torch.float32)
        bc = torch.empty(2, B, K, L, device=xdbl.device, dtype=torch.float32)
        base = xdbl.data_ptr()
        _launch("mlagg_index_scan", base, width, per, _ptr(idx), _ptr(dtr), B, L, K, R)
        _launch("mlagg_index_scan", base + 4 * R, width, per, _ptr(idx), _ptr(bc[0]), B, L, K, 1)
        _launch("mlagg_index_scan", base + 4 * (R + 1), width, per, _ptr(idx), _ptr(bc[1]), B, L, K, 1)
        ctx.save_for_backward(idx)
        ctx.meta = (R, width)
        return dtr.view(B, K, R, L), bc[0], bc[1]

    @staticmethod
    def backward(ctx, ddtr, dBs, dCs):
        (idx,) = ctx.saved_tensors
        R, width = ctx.meta
        per = R + 2
        ddtr = _require(ddtr.contiguous(), "ddtr")
        dBs = _require(dBs.contiguous(), "dBs")
        dCs = _require(dCs.contiguous(), "dCs")
        B, K, _, L = ddtr.shape
        dx = torch.empty(B, L, width, device=ddtr.device, dtype=torch.float32)
        base = dx.data_ptr()
        _launch("mlagg_index_merge", _ptr(ddtr), _ptr(idx), base, width, per, B, L, K, R)
        _launch("mlagg_index_merge", _ptr(dBs), _ptr(idx), base + 4 * R, width, per, B, L, K, 1)
        _launch("mlagg_index_merge", _ptr(dCs), _ptr(idx), base + 4 * (R + 1), width, per, B, L, K, 1)
        return dx, None, None


def index_scan_bc(xdbl, idx, R):
    return IndexScanBCFn.apply(xdbl, idx, R)


def index_scan(tok, idx, CB, blk=0, col0=0):
    return IndexScanFn.apply(tok, idx, CB, blk, col0)


def index_merge(seq, idx, CB):
    return IndexMergeFn.apply(seq, idx, CB)


def cross_scan(tok, HW, CB, nblk):
    return CrossScanFn.apply(tok, HW, CB, nblk)


def cross_merge(seq, HW, CB):
    return CrossMergeFn.apply(seq, HW, CB)


def cross_scan_bc(xdbl, HW, dt_rank, d_state):
    return CrossScanBCFn.apply(xdbl, HW, dt_rank, d_state)


class GateFn(torch.autograd.Function):
    """K7: concat(a0, a1) * SiLU(act) (the MLLA block's gate) in one pass each way."""

    @staticmethod
    def forward(ctx, a0, a1, act, slot=None):
        ctx.slot = slot
        a0 = _require(a0.contiguous(), "a0")
        a1 = _require(a1.contiguous(), "a1")
        act2, acts = _rows2d(act, "act")
        h = a0.shape[-1]
        rows = a0.numel() // h
        if a1.shape != a0.shape or act.shape[-1] != 2 * h or act2.shape[0] != rows:
            raise RuntimeError("gate: shape mismatch")
        if acts % 4 or act2.data_ptr() % 16:
            act2 = act2.contiguous()
            acts = 2 * h
        out = torch.empty(a0.shape[:-1] + (2 * h,), device=a0.device, dtype=torch.float32)
        _launch("mlagg_gate_fwd", _ptr(a0), _ptr(a1), _ptr(act2), acts, _ptr(out), rows, h)
        ctx.save_for_backward(a0, a1, act2)
        return out

    @staticmethod
    def backward(ctx, dout):
        a0, a1, act2 = ctx.saved_tensors
        h = a0.shape[-1]
        rows = a0.numel() // h
        d2, ds = _rows2d(dout, "dout")
        if ds % 4 or d2.data_ptr() % 16:
            d2 = d2.contiguous()
            ds = 2 * h
        da0, da1 = torch.empty_like(a0), torch.empty_like(a1)
        dact, dacts = _grad_out(ctx.slot, a0.shape[:-1] + (2 * h,), a0.device)
        _launch("mlagg_gate_bwd", _ptr(d2), ds, _ptr(a0), _ptr(a1), _ptr(act2), act2.stride(0), _ptr(da0), _ptr(da1), _ptr(dact), dacts,
                rows, h)
        return da0, da1, dact, None


def gate(a0, a1, act):
    return GateFn.apply(a0, a1, act, claim_slot(act))


class GeluPoolFn(torch.autograd.Function):
    """K17: r x r window mean of GELU(s) on a token-major map (the pooled branch's key / value reduction, T:722)."""

    @staticmethod
    def forward(ctx, s, H, W, r, slot=None):
        ctx.slot = slot
        s, ss = _rows(s, "s")
        B, N, d = s.shape
        if N != H * W or H % r or W % r:
            raise RuntimeError(f"gelu_pool: {N} tokens, map {H}x{W}, window {r}")
        pooled = torch.empty(B, (H // r) * (W // r), d, device=s.device, dtype=torch.float32)
        _launch("mlagg_gelu_pool_fwd", _ptr(s), ss, _ptr(pooled), B, H, W, d, r)
        ctx.save_for_backward(s)
        ctx.geom = (H, W, r)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        (s,) = ctx.saved_tensors
        H, W, r = ctx.geom
        B, N, d = s.shape
        dp = _require(dpooled.contiguous(), "dpooled")
        ds, dss = _grad_out(ctx.slot, (B, N, d), s.device)
        _launch("mlagg_gelu_pool_bwd", _ptr(s), s.stride(1), _ptr(dp), _ptr(ds), dss, B, H, W, d, r)
        return ds, None, None, None, None


def gelu_pool(s, H, W, r):
    return GeluPoolFn.apply(s, H, W, r, claim_slot(s))


class DiffLambdaFn(torch.autograd.Function):
    """K8: lambda = exp(<q1, k1>) - exp(<q2, k2>) + lambda_init of the differential attention, one launch each way."""

    @staticmethod
    def forward(ctx, q1, k1, q2, k2, lambda_init):
        vs = [_require(v.contiguous(), "lambda vector") for v in (q1, k1, q2, k2)]
        n = vs[0].numel()
        if any(v.numel() != n for v in vs):
            raise RuntimeError("diff_lambda: the four vectors differ in length")
        out = torch.empty(3, device=q1.device, dtype=torch.float32)            # [lambda, exp1, exp2]
        _launch("mlagg_diff_lambda_fwd", *(_ptr(v) for v in vs), float(lambda_init), n, _ptr(out), out.data_ptr() + 4)
        ctx.save_for_backward(*vs, out)
        return out[0]

    @staticmethod
    def backward(ctx, dlam):
        q1, k1, q2, k2, out = ctx.saved_tensors
        n = q1.numel()
        dlam = _require(dlam.reshape(1).contiguous(), "dlambda")
        g = torch.empty(4, n, device=q1.device, dtype=torch.float32)
        _launch("mlagg_diff_lambda_bwd", _ptr(dlam), _ptr(q1), _ptr(k1), _ptr(q2), _ptr(k2), out.data_ptr() + 4, n, _ptr(g[0]), _ptr(g[1]),
                _ptr(g[2]), _ptr(g[3]))
        return g[0].view_as(q1), g[1].view_as(k1), g[2].view_as(q2), g[3].view_as(k2), None


def diff_lambda(q1, k1, q2, k2, lambda_init):
    return DiffLambdaFn.apply(q1, k1, q2, k2, lambda_init)


class ScaledResidualFn(torch.autograd.Function):
    """K8: skip + branch * scale[sample] (residual under stochastic depth), float4 streams both ways."""

    @staticmethod
    def forward(ctx, skip, branch, scale):
        skip = _require(skip.contiguous(), "skip")
        branch = _require(branch.contiguous(), "branch")
        scale = _require(scale.reshape(-1).contiguous(), "scale")
        B = scale.numel()
        if skip.shape != branch.shape or skip.shape[0] != B:
            raise RuntimeError("scaled_residual: shape mismatch")
        per = skip.numel() // B
        out = torch.empty_like(skip)
        _launch("mlagg_scaled_residual", _ptr(skip), _ptr(branch), _ptr(scale), _ptr(out), B, per)
        ctx.save_for_backward(scale)
        return out

    @staticmethod
    def backward(ctx, g):
        (scale,) = ctx.saved_tensors
        g = _require(g.contiguous(), "grad")
        B = scale.numel()
        db = torch.empty_like(g)
        _launch("mlagg_scaled_residual", None, _ptr(g), _ptr(scale), _ptr(db), B, g.numel() // B)
        return g, db, None


def scaled_residual(skip, branch, scale):
    return ScaledResidualFn.apply(skip, branch, scale)


class DiceCEStatsFn(torch.autograd.Function):
    """K9: per-level Dice / cross-entropy statistics of ALL deep-supervision levels (one kernel per level each way).

    ``DiceCEStatsFn.apply(n_levels, ignore_label, *logits, *targets)`` -> (ip (L, B, 2, C): intersect and sum_pred per sample and
    class, gt (L, B, C): label counts, ce (L,): summed -log softmax of the label); gradients flow to the logits from ip and ce.
    ``ignore_label`` (int, -1: none): pixels with that label are left out of every sum and get no gradient."""

    @staticmethod
    def forward(ctx, n, ignore_label, *tensors):
        logits, targets = tensors[:n], tensors[n:]
        ctx.ignore = int(ignore_label)
        B, C = logits[0].shape[:2]
        dev = logits[0].device
        lib = _lib.lib()
        if C > lib.mlagg_dice_ce_max_classes():
            raise RuntimeError(f"dice_ce_stats: at most {lib.mlagg_dice_ce_max_classes()} classes")
        buf = torch.empty(n * B * 3 * C + n, device=dev, dtype=torch.float32)       # every entry is written by the level's reduce
        ip = buf[:n * B * 2 * C].view(n, B, 2, C)
        gt = buf[n * B * 2 * C:n * B * 3 * C].view(n, B, C)
        ce = buf[n * B * 3 * C:]
        saved = []
        for i, (z, t) in enumerate(zip(logits, targets)):
            z = _require(z.contiguous(), "logits")
            t = _require(t.contiguous(), "target")
            if z.shape[:2] != (B, C) or t.numel() * C != z.numel():
                raise RuntimeError("dice_ce_stats: logits / target shapes of a level do not match")
            hw = z.numel() // (B * C)
            ws = torch.empty(lib.mlagg_dice_ce_stats_workspace_floats(B, C, hw), device=dev, dtype=torch.float32)
            _launch("mlagg_dice_ce_stats", _ptr(z), _ptr(t), _ptr(ip[i]), _ptr(gt[i]), ce.data_ptr() + 4 * i, _ptr(ws), B, C, hw,
                    ctx.ignore)
            saved += [z, t]
        ctx.save_for_backward(*saved)
        ctx.n = n
        ctx.mark_non_differentiable(gt)
        return ip, gt, ce

    @staticmethod
    def backward(ctx, g_ip, g_gt, g_ce):
        n = ctx.n
        saved = ctx.saved_tensors
        B, C = saved[0].shape[:2]
        g_ip = torch.zeros(n, B, 2, C, device=saved[0].device) if g_ip is None else _require(g_ip.contiguous(), "g_ip")
        g_ce = torch.zeros(n, device=saved[0].device) if g_ce is None else _require(g_ce.contiguous(), "g_ce")
        grads = []
        for i in range(n):
            z, t = saved[2 * i], saved[2 * i + 1]
            dz = torch.empty_like(z)
            _launch("mlagg_dice_ce_grad", _ptr(z), _ptr(t), _ptr(g_ip[i]), g_ce.data_ptr() + 4 * i, _ptr(dz), B, C, z.numel() // (B * C),
                    ctx.ignore)
            grads.append(dz)
        return (None, None, *grads, *([None] * n))


def dice_ce_stats(logits, targets, ignore_label=None):
    return DiceCEStatsFn.apply(len(logits), -1 if ignore_label is None else int(ignore_label), *logits, *targets)


_TOPK_WORKSPACES = {}
TOPK_RECORD_WORDS = 8              # mlagg_topk_ce_record_floats: t, share, topk_sum, topk_sum / k, int64 n_gt, int64 n_eq


def topk_count(n, kpercent):
    """k of TopKLoss.forward (reference loss/robust_ce_loss.py:30-31): ``int(num_voxels * k / 100)`` in Python float arithmetic, with
    every pixel counted, ignored ones too.  k == 0 is refused: the reference takes the mean of an empty tensor there and returns NaN."""
    k = int(n * kpercent / 100)
    if k <= 0:
        raise RuntimeError(f"top-k loss: {kpercent} % of {n} pixels is less than one pixel (the reference returns NaN here)")
    return k


class TopKCEStatsFn(torch.autograd.Function):
    """K33: per-level top-k cross-entropy of ALL deep-supervision levels, with K9's Dice statistics from the same pass over the logits.

    ``TopKCEStatsFn.apply(n_levels, ignore_label, label_smoothing, kpercent, with_dice, *logits, *targets)`` -> (ip (L, B, 2, C), gt
    (L, B, C): K9's statistics, or None, None without Dice; rec (L, 8): the select's record per level -- [:, 0] the threshold t, [:, 1]
    the share of a pixel that ties with it, [:, 2] the sum of the k largest per-pixel cross-entropies, [:, 3] that sum / k, i.e.
    TopKLoss, and [:, 4:8].view(torch.int64) the counts n_gt, n_eq).  Gradients flow to the logits from ip and rec[:, 3] only.
    Per level: the statistics pass, the select (9 small launches) and, backward, one gradient pass; every launch is on the current
    stream, the select's workspace is cached per size and device, nothing synchronises with the host."""

    @staticmethod
    def forward(ctx, n, ignore_label, label_smoothing, kpercent, with_dice, *tensors):
        logits, targets = tensors[:n], tensors[n:]
        ctx.ignore, ctx.eps, ctx.with_dice = int(ignore_label), float(label_smoothing), bool(with_dice)
        B, C = logits[0].shape[:2]
        dev = logits[0].device
        lib = _lib.lib()
        if not 2 <= C <= lib.mlagg_dice_ce_max_classes():
            raise RuntimeError(f"topk_ce_stats: {C} classes, 2 to {lib.mlagg_dice_ce_max_classes()} are supported")
        W = TOPK_RECORD_WORDS
        npix = [z.numel() // C for z in logits]
        ks = [topk_count(m, kpercent) for m in npix]
        # [records | ip | gt | ce]: the records first, their int64 counts need 8-byte alignment; every entry is written by the kernels
        buf = torch.empty(n * W + (n * B * 3 * C + n if with_dice else 0), device=dev, dtype=torch.float32)
        rec = buf[:n * W].view(n, W)
        ip = gt = ce = None
        if with_dice:
            ip = buf[n * W:n * W + n * B * 2 * C].view(n, B, 2, C)
            gt = buf[n * W + n * B * 2 * C:n * W + n * B * 3 * C].view(n, B, C)
            ce = buf[n * W + n * B * 3 * C:]
        ce_pix = torch.empty(sum(npix), device=dev, dtype=torch.float32)
        saved, at = [], 0
        for i, (z, t) in enumerate(zip(logits, targets)):
            z = _require(z.contiguous(), "logits")
            t = _require(t.contiguous(), "target")
            if z.shape[:2] != (B, C) or t.numel() * C != z.numel():
                raise RuntimeError("topk_ce_stats: logits / target shapes of a level do not match")
            hw, cp = npix[i] // B, ce_pix[at:at + npix[i]]
            at += npix[i]
            key = (npix[i], str(dev))
            ws = _TOPK_WORKSPACES.get(key)
            if ws is None:
                ws = _TOPK_WORKSPACES[key] = torch.empty(lib.mlagg_topk_ce_select_workspace_bytes(npix[i]) // 8, device=dev,
                                                         dtype=torch.int64)
            part = torch.empty(lib.mlagg_dice_ce_stats_workspace_floats(B, C, hw), device=dev, dtype=torch.float32) if with_dice else None
            _launch("mlagg_topk_ce_stats", _ptr(z), _ptr(t), _ptr(ip[i]) if with_dice else None, _ptr(gt[i]) if with_dice else None,
                    ce.data_ptr() + 4 * i if with_dice else None, _ptr(cp), _ptr(part), B, C, hw, ctx.ignore, ctx.eps)
            _launch("mlagg_topk_ce_select", _ptr(cp), _ptr(rec[i]), _ptr(ws), npix[i], ks[i])
            saved += [z, t]
        ctx.save_for_backward(ce_pix, rec, *saved)
        ctx.n, ctx.npix, ctx.ks = n, npix, ks
        if with_dice:
            ctx.mark_non_differentiable(gt)
        return ip, gt, rec

    @staticmethod
    def backward(ctx, g_ip, g_gt, g_rec):
        n, W = ctx.n, TOPK_RECORD_WORDS
        ce_pix, rec, *saved = ctx.saved_tensors
        B, C = saved[0].shape[:2]
        dev = saved[0].device
        if ctx.with_dice:
            g_ip = torch.zeros(n, B, 2, C, device=dev) if g_ip is None else _require(g_ip.contiguous(), "g_ip")
        g_rec = torch.zeros(n, W, device=dev) if g_rec is None else _require(g_rec.contiguous(), "g_rec")
        grads, at = [], 0
        for i in range(n):
            z, t = saved[2 * i], saved[2 * i + 1]
            dz = torch.empty_like(z)
            _launch("mlagg_topk_ce_grad", _ptr(z), _ptr(t), ce_pix.data_ptr() + 4 * at, _ptr(rec[i]),
                    _ptr(g_ip[i]) if ctx.with_dice else None, g_rec.data_ptr() + 4 * (W * i + 3), _ptr(dz), B, C, ctx.npix[i] // B,
                    ctx.ks[i], ctx.ignore, ctx.eps)
            at += ctx.npix[i]
            grads.append(dz)
        return (None, None, None, None, None, *grads, *([None] * n))


def topk_ce_stats(logits, targets, ignore_label=None, label_smoothing=0.0, kpercent=10, with_dice=False):
    """K33 over all levels in one apply: see TopKCEStatsFn."""
    return TopKCEStatsFn.apply(len(logits), -1 if ignore_label is None else int(ignore_label), float(label_smoothing), kpercent,
                               bool(with_dice), *logits, *targets)


_REGION_TABLES = {}
_REGION_WORKSPACES = {}
REGION_LOSS_MAX_REGIONS = 16       # heads held in registers by K29 (mlagg_dice_bce_max_regions)


def region_member_table(regions, device):
    """The K29 membership table of a label manager's ``foreground_regions`` (ints or tuples of ints) as 256 int32 (uint32 bits) on
    `device`: bit r of entry v says that label v belongs to region r -- ``np.isin(seg, regions[r])`` for every r at once.  Uploaded
    once per (regions, device)."""
    key = (tuple(tuple(int(v) for v in r) if isinstance(r, (tuple, list)) else (int(r),) for r in regions), str(device))
    if key not in _REGION_TABLES:
        if not 1 <= len(key[0]) <= 32:
            raise RuntimeError(f"region_member_table: {len(key[0])} regions, 1 to 32 fit the table")
        table = np.zeros(256, dtype=np.uint32)
        for r, labels in enumerate(key[0]):
            for v in labels:
                if 0 <= v < 256:
                    table[v] |= np.uint32(1 << r)
        _REGION_TABLES[key] = torch.from_numpy(table.view(np.int32)).to(device)
    return _REGION_TABLES[key]


class DiceBCEStatsFn(torch.autograd.Function):
    """K29: per-level Dice / binary cross-entropy statistics of ALL deep-supervision levels of a region-based dataset (one kernel per
    level each way).

    ``DiceBCEStatsFn.apply(n_levels, ignore_label, member, *logits, *targets)`` -> (ip (L, B, 2, R): intersect and sum_pred per sample
    and head, gt (L, B, R): masked target sums, sums (L, 2): the summed binary cross-entropy and the mask sum); gradients flow to the
    logits from ip and sums[:, 0].  ``member``: the table of ``region_member_table`` when the targets are label maps (B, 1, ...), None
    when they are region planes (B, R, ...) -- (B, R + 1, ...) with the ignore plane last when ``ignore_label`` >= 0.
    The per-level workspaces are cached per shape and device; nothing here synchronises with the host."""

    @staticmethod
    def forward(ctx, n, ignore_label, member, *tensors):
        logits, targets = tensors[:n], tensors[n:]
        ctx.ignore = int(ignore_label)
        B, R = logits[0].shape[:2]
        dev = logits[0].device
        lib = _lib.lib()
        if not 1 <= R <= REGION_LOSS_MAX_REGIONS:
            raise RuntimeError(f"dice_bce_stats: {R} heads, 1 to {REGION_LOSS_MAX_REGIONS} are supported")
        if member is not None and not (member.is_cuda and member.dtype == torch.int32 and member.numel() == 256
                                       and member.is_contiguous() and member.device == dev):
            raise RuntimeError("dice_bce_stats: the member table is region_member_table(regions, device)")
        planes = 1 if member is not None else R + (1 if ctx.ignore >= 0 else 0)
        buf = torch.empty(n * B * 3 * R + 2 * n, device=dev, dtype=torch.float32)   # every entry is written by the level's reduce
        ip = buf[:n * B * 2 * R].view(n, B, 2, R)
        gt = buf[n * B * 2 * R:n * B * 3 * R].view(n, B, R)
        sums = buf[n * B * 3 * R:].view(n, 2)
        saved = []
        for i, (z, t) in enumerate(zip(logits, targets)):
            z = _require(z.contiguous(), "logits")
            t = _require(t.contiguous(), "target")
            hw = z.numel() // (B * R)
            if z.shape[:2] != (B, R) or t.shape[0] != B or t.numel() != B * planes * hw:
                raise RuntimeError(f"dice_bce_stats: logits {tuple(z.shape)} / target {tuple(t.shape)} of level {i} do not match "
                                   f"({planes} target plane(s) expected)")
            key = (B, R, hw, str(dev))
            ws = _REGION_WORKSPACES.get(key)
            if ws is None:
                ws = _REGION_WORKSPACES[key] = torch.empty(lib.mlagg_dice_bce_stats_workspace_floats(B, R, hw), device=dev,
                                                           dtype=torch.float32)
            _launch("mlagg_dice_bce_stats", _ptr(z), _ptr(t), _ptr(member), _ptr(ip[i]), _ptr(gt[i]), sums.data_ptr() + 8 * i, _ptr(ws),
                    B, R, hw, ctx.ignore)
            saved += [z, t]
        ctx.save_for_backward(*saved)
        ctx.n, ctx.member = n, member
        ctx.mark_non_differentiable(gt)
        return ip, gt, sums

    @staticmethod
    def backward(ctx, g_ip, g_gt, g_sums):
        n = ctx.n
        saved = ctx.saved_tensors
        B, R = saved[0].shape[:2]
        g_ip = torch.zeros(n, B, 2, R, device=saved[0].device) if g_ip is None else _require(g_ip.contiguous(), "g_ip")
        g_sums = torch.zeros(n, 2, device=saved[0].device) if g_sums is None else _require(g_sums.contiguous(), "g_sums")
        grads = []
        for i in range(n):
            z, t = saved[2 * i], saved[2 * i + 1]
            dz = torch.empty_like(z)
            _launch("mlagg_dice_bce_grad", _ptr(z), _ptr(t), _ptr(ctx.member), _ptr(g_ip[i]), g_sums.data_ptr() + 8 * i, _ptr(dz), B, R,
                    z.numel() // (B * R), ctx.ignore)
            grads.append(dz)
        return (None, None, None, *grads, *([None] * n))


def dice_bce_stats(logits, targets, member_table=None, ignore_label=None):
    """K29 over all levels in one apply: see DiceBCEStatsFn.  member_table None: the targets are region planes."""
    return DiceBCEStatsFn.apply(len(logits), -1 if ignore_label is None else int(ignore_label), member_table, *logits, *targets)


def transpose_2d(src):
    """(B, R, C) -> (B, C, R) contiguous on the tiled transpose kernel (K8).  The source matrices must be contiguous;
    their batch stride may be larger than R * C (a channel slice of an NCHW map), anything else is copied first."""
    _require(src, "src")
    B, R, C = src.shape
    if not (src.stride(2) == 1 and src.stride(1) == C and src.stride(0) >= R * C and src.data_ptr() % 16 == 0
            and (C % 4 or src.stride(0) % 4 == 0)):
        src = src.contiguous()
    dst = torch.empty(B, C, R, device=src.device, dtype=torch.float32)
    _launch("mlagg_transpose_2d", _ptr(src), src.stride(0), _ptr(dst), B, R, C)
    return dst


class ChannelBiasFn(torch.autograd.Function):
    """y = x + bias[c] on an NCHW map, in place on the convolution output; backward reduces the bias gradient with the
    library's plane-sum kernel (torch's convolution_backward does it with a generic reduction at 1.3-2 TB/s)."""

    @staticmethod
    def forward(ctx, x, bias):
        ctx.mark_dirty(x)
        x.add_(bias.view(1, -1, *([1] * (x.dim() - 2))))
        return x

    @staticmethod
    def backward(ctx, g):
        g = _require(g.contiguous(), "grad")
        B, C = g.shape[:2]
        db = torch.empty(C, device=g.device, dtype=torch.float32)
        ws = torch.empty(_lib.lib().mlagg_channel_sum_workspace_floats(B, C), device=g.device, dtype=torch.float32)
        _launch("mlagg_channel_sum", _ptr(g), _ptr(db), _ptr(ws), B, C, g.numel() // (B * C))
        return g, db


def channel_bias(x, bias):
    return ChannelBiasFn.apply(x, bias)


EPI_NONE, EPI_GELU = 0, 1


class ChannelEpilogueFn(torch.autograd.Function):
    """K13: y = act(x + bias[c] + res) on the NCHW output `x` of a library convolution, one pass.  `x` is consumed: without an
    activation it is updated in place and returned; with GELU it is overwritten with the pre-activation (kept for backward)
    and the result is a new map."""

    @staticmethod
    def forward(ctx, x, bias, res, act):
        x = _require(x, "x")
        if not x.is_contiguous():
            raise RuntimeError("channel_epilogue: contiguous NCHW map expected")
        res = None if res is None else _require(res.contiguous(), "res", x.shape)
        B, C = x.shape[:2]
        hw = x.numel() // (B * C)
        if act == EPI_GELU and x._version != 0:
            # the GELU form overwrites x with the pre-activation WITHOUT telling autograd: only a map nothing else has
            # written or saved in a modified state (a fresh convolution output) may be handed in
            raise RuntimeError("channel_epilogue(GELU): x must be the fresh output of the producing call")
        y = torch.empty_like(x) if act == EPI_GELU else None
        _launch("mlagg_channel_epilogue_fwd", _ptr(x), _ptr(bias), _ptr(res), _ptr(y), B, C, hw, int(act))
        ctx.meta = (int(act), bias is not None, res is not None)
        if act == EPI_GELU:
            # x now holds the pre-activation.  It is the fresh output of the convolution call in front of this function
            # (nothing else reads it, convolution backward does not need its own output), so it is simply kept.
            ctx.save_for_backward(x)
            return y
        ctx.mark_dirty(x)
        return x

    @staticmethod
    def backward(ctx, dy):
        act, has_bias, has_res = ctx.meta
        dy = _require(dy.contiguous(), "dy")
        B, C = dy.shape[:2]
        hw = dy.numel() // (B * C)
        db = torch.empty(C, device=dy.device, dtype=torch.float32) if has_bias else None
        ws = torch.empty(_lib.lib().mlagg_channel_sum_workspace_floats(B, C), device=dy.device, dtype=torch.float32) if has_bias else None
        if act == EPI_GELU:
            (pre,) = ctx.saved_tensors
            dx = torch.empty_like(dy)
            _launch("mlagg_channel_gelu_bwd", _ptr(pre), _ptr(dy), _ptr(dx), _ptr(db), _ptr(ws), B, C, hw)
        else:
            dx = dy
            if has_bias:
                _launch("mlagg_channel_sum", _ptr(dy), _ptr(db), _ptr(ws), B, C, hw)
        return dx, db, (dx if has_res else None), None


def channel_epilogue(x, bias=None, res=None, act=EPI_NONE):
    return ChannelEpilogueFn.apply(x, bias, res, act)


def column_sum(x2):
    """Sum over the rows of a (rows, cols) matrix with unit inner stride."""
    _require(x2, "x")
    rows, cols = x2.shape
    out = torch.empty(cols, device=x2.device, dtype=torch.float32)
    n = _lib.lib().mlagg_column_sum_workspace_floats(rows, cols)
    ws = torch.empty(n, device=x2.device, dtype=torch.float32) if n else None
    _launch("mlagg_column_sum", _ptr(x2), x2.stride(0), _ptr(out), _ptr(ws), rows, cols)
    return out


ACT_NONE, ACT_LEAKY, ACT_SILU = 0, 1, 2


_DT_CODE = {torch.float32: _C["MLAGG_DTYPE_F32"], **_LP_CODE}


def _require_map(t, name, shape=None):
    """A device map in fp32, bf16 or fp16 (the kernels of the convolutional chains take the element type as an argument)."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in _DT_CODE):
        raise RuntimeError(f"{name}: expected an fp32 / bf16 / fp16 tensor on the MI355X device, got "
                           f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '?')}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _map_slice(t, name):
    """A gradient map as the K10 / shuffle kernels can read it without a copy: (tensor, elements between samples) -- dense, or a channel
    slice of a wider dense map (what ``torch.cat([a, b], 1)``'s backward hands to the producers of a and b); anything else is copied."""
    if t.is_cuda and t.dim() >= 3 and not t.is_contiguous():
        inner, want = 1, []
        for v in reversed(t.shape[1:]):
            want.append(inner)
            inner *= int(v)
        want.reverse()
        plane = inner // int(t.shape[1])
        if tuple(t.stride()[1:]) == tuple(want) and t.stride(0) >= inner and t.stride(0) % plane == 0 and t.stride(0) % 4 == 0 and \
                t.data_ptr() % 16 == 0 and t.dtype in _DT_CODE:
            return t, t.stride(0)
    t = _require_map(t.contiguous(), name)
    return t, 0


class PlaneNormFn(torch.autograd.Function):
    """K10: per-(batch, channel)-plane normalisation of an NCHW map fused with what follows it: y = act(norm(x) + res)
    (GroupNorm(C, C); InstanceNorm2d + LeakyReLU; InstanceNorm2d(affine) + SiLU; the residual sum of the UnetResBlock).
    x, res and y may each be fp32, bf16 or fp16 IN MEMORY (16-bit modes: maps between the 16-bit library convolutions);
    statistics and arithmetic are fp32."""

    @staticmethod
    def forward(ctx, x, gamma, beta, res, eps, act, slope, out_dtype):
        x = _require_map(x.contiguous(), "x")
        res = None if res is None else _require_map(res.contiguous(), "res", x.shape)
        B, C = x.shape[:2]
        hw = x.numel() // (B * C)
        y = torch.empty(x.shape, device=x.device, dtype=out_dtype or x.dtype)
        stats = torch.empty(B * C, 2, device=x.device, dtype=torch.float32)
        nws = _lib.lib().mlagg_plane_norm_fwd_workspace_floats(B, C, hw)          # > 0: planes cut into segments (3-D volumes)
        ws = torch.empty(nws, device=x.device, dtype=torch.float32) if nws else None
        _launch("mlagg_plane_norm_fwd", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(res), _ptr(y), _ptr(stats), _ptr(ws), B, C, hw, float(eps),
                int(act), float(slope), _DT_CODE[x.dtype], 0 if res is None else _DT_CODE[res.dtype], _DT_CODE[y.dtype])
        ctx.save_for_backward(x, gamma, beta, res, stats)
        ctx.meta = (int(act), float(slope))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, res, stats = ctx.saved_tensors
        act, slope = ctx.meta
        dy, dyb = _map_slice(dy, "dy")
        B, C = x.shape[:2]
        hw = x.numel() // (B * C)
        lib = _lib.lib()
        dx = torch.empty_like(x)
        dres = torch.empty_like(res) if (res is not None and ctx.needs_input_grad[3]) else None
        dg = torch.empty_like(gamma) if gamma is not None else None
        db = torch.empty_like(beta) if beta is not None else None
        segmented = lib.mlagg_plane_norm_fwd_workspace_floats(B, C, hw) > 0
        ws = torch.empty(lib.mlagg_plane_norm_bwd_workspace_floats(B, C, hw), device=x.device, dtype=torch.float32) \
            if (dg is not None or db is not None or segmented) else None
        _launch("mlagg_plane_norm_bwd_strided", _ptr(x), _ptr(dy), dyb, _ptr(gamma), _ptr(beta), _ptr(res), _ptr(stats), _ptr(dx),
                _ptr(dres), _ptr(dg), _ptr(db), _ptr(ws), B, C, hw, act, slope, _DT_CODE[x.dtype], _DT_CODE[dy.dtype],
                0 if res is None else _DT_CODE[res.dtype])
        return dx, dg, db, dres, None, None, None, None


def plane_norm(x, gamma, beta, eps=1e-5, act=ACT_NONE, slope=0.0, res=None, out_dtype=None):
    return PlaneNormFn.apply(x, gamma, beta, res, eps, act, slope, out_dtype)


class ChannelEpilogueLpFn(torch.autograd.Function):
    """K13 in the 16-bit modes: y = act(x + bias[c] + res) where x is the bf16 / fp16 output of a library convolution (left
    untouched: backward recomputes the pre-activation from it), y in ``out_dtype``; dx comes back in x's type -- the convolution's
    gradient operand -- with d(bias) from the same pass."""

    @staticmethod
    def forward(ctx, x, bias, res, act, out_dtype):
        x = _require_map(x.contiguous(), "x")
        res = None if res is None else _require_map(res.contiguous(), "res", x.shape)
        B, C = x.shape[:2]
        hw = x.numel() // (B * C)
        y = torch.empty(x.shape, device=x.device, dtype=out_dtype)
        _launch("mlagg_channel_epilogue_lp_fwd", _ptr(x), _DT_CODE[x.dtype], _ptr(bias), _ptr(res),
                0 if res is None else _DT_CODE[res.dtype], _ptr(y), _DT_CODE[y.dtype], B, C, hw, int(act))
        ctx.save_for_backward(x if act == EPI_GELU else None, bias, res if act == EPI_GELU else None)
        ctx.meta = (int(act), x.dtype, None if res is None else res.dtype, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, bias, res = ctx.saved_tensors
        act, xdt, rdt, shape = ctx.meta
        dy = _require_map(dy.contiguous(), "dy", shape)
        B, C = shape[:2]
        hw = dy.numel() // (B * C)
        dx = torch.empty(shape, device=dy.device, dtype=xdt)
        db = torch.empty(C, device=dy.device, dtype=torch.float32) if bias is not None else None
        ws = (torch.empty(_lib.lib().mlagg_channel_sum_workspace_floats(B, C), device=dy.device, dtype=torch.float32)
              if bias is not None else None)
        _launch("mlagg_channel_epilogue_lp_bwd", _ptr(x), _DT_CODE[xdt], _ptr(bias), _ptr(res), 0 if res is None else _DT_CODE[res.dtype],
                _ptr(dy), _DT_CODE[dy.dtype], _ptr(dx), _DT_CODE[xdt], _ptr(db), _ptr(ws), B, C, hw, act)
        dres = None
        if rdt is not None and ctx.needs_input_grad[2]:
            # d(res) = d(pre): dy itself without an activation, else the values of dx -- in res's own element type
            src = dy if act == EPI_NONE else dx
            dres = src if src.dtype == rdt else (dx if dx.dtype == rdt else src.to(rdt))
        return dx, db, dres, None, None


def channel_epilogue_lp(x, bias=None, res=None, act=EPI_NONE, out_dtype=torch.float32):
    return ChannelEpilogueLpFn.apply(x, bias, res, act, out_dtype)


# ------------------------------------------------------------------------------------------------
# K15: full convolutions with the weight gradient on this package's tap-GEMM kernel
# ------------------------------------------------------------------------------------------------
def _planes(t, name):
    """(B, C, *spatial) map whose samples are contiguous (C, P) blocks -- a channel slice of a wider NCHW map qualifies; anything else
    is copied.  Returns (tensor, floats between samples, P)."""
    _require(t, name)
    inner, want = 1, []
    for v in reversed(t.shape[1:]):
        want.append(inner)
        inner *= int(v)
    want.reverse()
    if tuple(t.stride()[1:]) != tuple(want) or t.stride(0) < inner or t.stride(0) % 4 or t.data_ptr() % 16:
        t = t.contiguous()
    return t, t.stride(0), inner // int(t.shape[1])


# K18 against MIOpen's tuned fp32 GEMM kernels on the 1 x 1 shapes of the 256 x 256 step (tools/bench_conv1x1.py,
# profiles/round3_g_conv1x1_*.log): the forward / data-gradient kernel wins where the pixel count is large and the contraction
# short-to-medium (128 x 128 and 256 x 256 maps: 70 vs 110, 64 vs 93, 98 vs 215 us), ties at 64 x 64 and loses on the small maps
# (few, long-K tiles); the weight gradient wins from 64 x 64 up (80 vs 142, 70 vs 88, 150 vs 252 us).  Each of the three products
# of a layer goes to the faster side.
K18 = _os.environ.get("MLAGG_K18", "1") == "1"
# round 4: 64 x 64 maps too (a tie with the library in the step -- 34.61 vs 34.60 ms, profiles/round4_k_k18_thresholds_ab.log -- and no NHWC transposes);
# 32 x 32 maps lose 0.3 ms
K18_FWD_MIN_PIXELS = int(_os.environ.get("MLAGG_K18_FWD_MIN_PIXELS", "4096"))
K18_FWD_MIN_K = int(_os.environ.get("MLAGG_K18_FWD_MIN_K", "96"))
K18_WGRAD_MIN_PIXELS = int(_os.environ.get("MLAGG_K18_WGRAD_MIN_PIXELS", "4096"))


K18_THIN_CH = 32


def _k18_product(O, I, P, form=_DTYPE_BF16X3):
    """forward-form product y (O) = w (O, I) . x (I) on K18?  (the data gradient asks with O and I exchanged.)  A contraction that is
    not a multiple of 16 runs on zero-padded weight columns (mlagg_conv1x1_fwd_ragged)."""
    I16 = -(-I // 16) * 16
    if not bool(_lib.lib().mlagg_conv1x1_supported(O, I16, P)):
        return False
    if form != _DTYPE_BF16X3:                # one product per block: a stream of the maps, ahead of cast + library + cast wherever it runs
        return P >= LP_K_MIN_PIXELS
    if P >= K18_FWD_MIN_PIXELS and min(O, I) <= K18_THIN_CH:
        # a thin side (the 14-class heads and their data gradients): one pass over the wide map, where the library's GEMM kernels
        # took 101 us forward / 261 us backward for 48 -> 14 channels at 256 x 256 (profiles/round4_i_library_convolutions_by_shape.md)
        return True
    return I == I16 and P >= K18_FWD_MIN_PIXELS and I >= K18_FWD_MIN_K


def _conv1x1_k18(x, xb, w, y, B, O, I, P, form, accumulate=False):
    """y (B, O, P) (+)= w (O, I) . x (B, I, P) on K18 (y None: a new map); a contraction that is not a multiple of 16 on zero-padded
    weight columns."""
    if y is None:
        y = torch.empty((B, O) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
    I16 = -(-I // 16) * 16
    if I16 != I:
        wp = torch.zeros(O, I16, device=w.device, dtype=torch.float32)
        wp[:, :I] = w
        w = wp
    _flop("K18", 2 * B * O * I * P)
    _launch("mlagg_conv1x1_fwd_acc", _ptr(x), xb, _ptr(w), None, _ptr(y), O * P, B, O, I16, I, P, form, int(accumulate))
    return y


def _conv1x1_wgrad(dy, dyb, x, B, O, I, P, form):
    """dW (O, I) = dy (B, O, P) . x (B, I, P)^T on K18."""
    dW = torch.empty(O, I, device=x.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().mlagg_conv1x1_wgrad_workspace_floats(B, O, I, P), device=x.device, dtype=torch.float32)
    _flop("K18", 2 * B * O * I * P)
    _launch("mlagg_conv1x1_wgrad_lp", _ptr(dy), dyb, _ptr(x), x.stride(0), _ptr(dW), _ptr(ws), B, O, I, P, form)
    return dW


class Conv1x1Fn(torch.autograd.Function):
    """y = conv2d(x, W) for a 1 x 1 kernel (stride 1, no bias): forward and data gradient (the forward kernel on W^T) on K18 or on the
    library as the plan says (_conv1x1_plan unless one is given), the weight gradient (the pixels as the contraction) on K18."""

    @staticmethod
    def forward(ctx, x, weight, form=_DTYPE_BF16X3, plan=None):
        x, xb, P = _planes(x, "x")
        B, I = x.shape[:2]
        O = weight.shape[0]
        plan = plan or _conv1x1_plan(O, I, P, form)
        w = _require(weight.reshape(O, I).contiguous(), "weight")
        y = _conv1x1_k18(x, xb, w, None, B, O, I, P, form) if plan[0] else _lib_conv(x, weight, 1, 0, False, form)
        ctx.save_for_backward(x, w)
        ctx.wshape, ctx.plan, ctx.form = weight.shape, plan, form
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        B, I = x.shape[:2]
        O = w.shape[0]
        dy, dyb, P = _planes(dy, "dy")
        form = ctx.form
        dx = dW = None
        if ctx.needs_input_grad[0]:
            if ctx.plan[1]:
                wt = transpose_2d(w.unsqueeze(0))[0]                                   # (I, O): the contraction runs along its rows
                dx = _conv1x1_k18(dy, dyb, wt, None, B, I, O, P, form)
            else:
                dx = _lib_conv_bwd(dy, x, w.view(ctx.wshape), 1, 0, False, (True, False, False), form)[0]
        if ctx.needs_input_grad[1]:
            dW = _conv1x1_wgrad(dy, dyb, x, B, O, I, P, form).view(ctx.wshape)
        return dx, dW, None, None


def _conv1x1_plan(O, I, P, form):
    return ("K18" if _k18_product(O, I, P, form) else None, "K18" if _k18_product(I, O, P, form) else None, "K18")


def _pixel_shuffle2(src, B, O, H, W, inverse):
    """(B, 4 O, H, W) -> (B, O, 2 H, 2 W), or back (inverse)."""
    src = _require(src.contiguous(), "src")
    dst = torch.empty((B, 4 * O, H, W) if inverse else (B, O, 2 * H, 2 * W), device=src.device, dtype=torch.float32)
    _launch("mlagg_pixel_shuffle2", _ptr(src), _ptr(dst), B, O, H, W, int(inverse))
    return dst


class ConvT2x2Fn(torch.autograd.Function):
    """y = conv_transpose2d(x, W (I, O, 2, 2), stride 2): the taps do not overlap, so it is the pointwise product with the (4 O, I) matrix
    [tap (a, c)][o][i] = W[i][o][a][c] on K18 followed by a pixel shuffle; backward: the inverse shuffle of dy, then K18's data
    gradient (contraction 4 O) and weight gradient.  (The library ran this layer of the 256 x 256 step in 215 us forward + 350 us
    backward: profiles/round4_i_library_convolutions_by_shape.md.)"""

    @staticmethod
    def forward(ctx, x, weight, form=_DTYPE_BF16X3):
        x, xb, P = _planes(x, "x")
        B, I, H, W = x.shape
        O = weight.shape[1]
        w4 = _require(weight.permute(2, 3, 1, 0).reshape(4 * O, I).contiguous(), "weight")
        z = _conv1x1_k18(x, xb, w4, None, B, 4 * O, I, P, form)
        ctx.save_for_backward(x, w4)
        ctx.form, ctx.O = form, O
        return _pixel_shuffle2(z, B, O, H, W, False)

    @staticmethod
    def backward(ctx, dy):
        x, w4 = ctx.saved_tensors
        B, I, H, W = x.shape
        O, form, P = ctx.O, ctx.form, H * W
        dy, dyb = _map_slice(dy, "dy")                                                # a half of cat([up, skip])'s gradient: read in place
        if dy.dtype != torch.float32:
            dy, dyb = dy.float(), 0
        dyu = torch.empty(B, 4 * O, H, W, device=x.device, dtype=torch.float32)        # (B, 4 O, H, W)
        _launch("mlagg_pixel_unshuffle2_strided", _ptr(dy), dyb, _ptr(dyu), B, O, H, W)
        dx = dW = None
        if ctx.needs_input_grad[0]:
            wt = transpose_2d(w4.unsqueeze(0))[0]                                      # (I, 4 O)
            dx = _conv1x1_k18(dyu, 4 * O * P, wt, None, B, I, 4 * O, P, form)
        if ctx.needs_input_grad[1]:
            dW = _conv1x1_wgrad(dyu, 4 * O * P, x, B, 4 * O, I, P, form).view(2, 2, O, I).permute(3, 2, 0, 1).contiguous()
        return dx, dW, None


K19 = _os.environ.get("MLAGG_K19", "1") == "1"
# K19 against MIOpen's tuned Winograd kernels (tools/bench_conv3x3.py, batch 10): 17-30 % faster from 32 x 32 maps up (48 -> 48 at
# 256 x 256: 302 vs 416 us forward, 272 vs 356 us data gradient; 96 -> 96 at 128 x 128: 202 vs 262), slower on the 16 x 16 maps
# (720 channels: few pixel tiles, long contractions: 315 vs 262 us)
K19_MIN_PIXELS = int(_os.environ.get("MLAGG_K19_MIN_PIXELS", "1024"))


K19_WGRAD = _os.environ.get("MLAGG_K19_WGRAD", "1") == "1"
K19_WGRAD_MIN_PIXELS = int(_os.environ.get("MLAGG_K19_WGRAD_MIN_PIXELS", "1024"))
K19_WGRAD_MIN_CH = int(_os.environ.get("MLAGG_K19_WGRAD_MIN_CH", "48"))      # round 4: the 16-wide tiles fill 48-channel layers (was 96)


def _k19_wgrad(O, I, H, W, form=_DTYPE_BF16X3):
    """3 x 3 weight gradient on K19?  (16-bit operand forms: wherever the kernel runs -- one product per tap and block.)  Measured against MIOpen's implicit-GEMM kernels + their NHWC transposes (tools/bench_conv3x3.py):
    706 vs 816, 280 vs 323, 175 vs 205, 190 vs 212 us where a channel extent reaches 96 (32-channel tiles are then well filled);
    48 x 48 channels fill 56 % of a tile pair and lose or tie (492 vs 493, 179 vs 119 us), 16 x 16 maps tie."""
    if form != _DTYPE_BF16X3:
        return K19_WGRAD and H * W >= LP_K_MIN_PIXELS and bool(_lib.lib().mlagg_conv3x3_wgrad_supported(O, I, H, W))
    return (K19_WGRAD and H * W >= K19_WGRAD_MIN_PIXELS and max(O, I) >= K19_WGRAD_MIN_CH and
            bool(_lib.lib().mlagg_conv3x3_wgrad_supported(O, I, H, W)))


def _k19_product(O, I, H, W, form=_DTYPE_BF16X3):
    """forward-form 3 x 3 product (O output channels, contraction I) on K19?  (the data gradient asks with O and I exchanged)"""
    floor = K19_MIN_PIXELS if form == _DTYPE_BF16X3 else LP_K_MIN_PIXELS
    return K19 and H * W >= floor and bool(_lib.lib().mlagg_conv3x3_supported(O, I, H, W))


def _conv3x3_plan(O, I, H, W, form):
    return tuple("K19" if on else None for on in (_k19_product(O, I, H, W, form), _k19_product(I, O, H, W, form), _k19_wgrad(O, I, H, W, form)))


def _conv3x3_k19(x, xb, w, transposed, O, I, H, W, form, out=None):
    B = x.shape[0]
    y = torch.empty(B, O, H, W, device=x.device, dtype=torch.float32) if out is None else out
    ws = torch.empty(_lib.lib().mlagg_conv3x3_workspace_bytes(O, I), device=x.device, dtype=torch.uint8)
    _flop("K19", 2 * 9 * B * O * I * H * W)
    _launch("mlagg_conv3x3_fwd_lp", _ptr(x), xb, _ptr(w), int(transposed), None, _ptr(y), y.stride(0), _ptr(ws), B, O, I, H, W, form)
    return y


class Conv3x3Fn(torch.autograd.Function):
    """y = conv2d(x, W, padding=1) for a dense 3 x 3 kernel (stride 1, no bias): each product on K19 (nine shifted GEMMs straight on
    the NCHW maps) or on the library as the plan says (_conv3x3_plan unless one is given)."""

    @staticmethod
    def forward(ctx, x, weight, form=_DTYPE_BF16X3, slot=None, plan=None):
        ctx.slot = slot
        x, xb, P = _planes(x, "x")
        B, I, H, W = x.shape
        O = weight.shape[0]
        plan = plan or _conv3x3_plan(O, I, H, W, form)
        w = _require(weight.contiguous(), "weight")
        y = _conv3x3_k19(x, xb, w, False, O, I, H, W, form) if plan[0] else _lib_conv(x, w, 1, 1, False, form)
        ctx.save_for_backward(x, w)
        ctx.plan, ctx.form = plan, form
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        B, I, H, W = x.shape
        O = w.shape[0]
        (_, dgrad, wgrad), form = ctx.plan, ctx.form
        dx = dW = None
        if ctx.needs_input_grad[0]:
            if dgrad:
                dy, dyb, _ = _planes(dy, "dy")
                out = ctx.slot.view() if ctx.slot is not None else None          # a piece of split_planes: written where the map's gradient lives
                dx = _conv3x3_k19(dy, dyb, w, True, I, O, H, W, form, out)
            else:
                dx = _lib_conv_bwd(dy, x, w, 1, 1, False, (True, False, False), form)[0]
        if ctx.needs_input_grad[1]:
            if wgrad:
                lib = _lib.lib()
                dy, dyb, _ = _planes(dy, "dy")
                dW = torch.empty(O, I, 3, 3, device=x.device, dtype=torch.float32)
                ws = torch.empty(lib.mlagg_conv3x3_wgrad_workspace_floats(B, O, I, H, W), device=x.device, dtype=torch.float32)
                _flop("K19", 2 * 9 * B * O * I * H * W)
                _launch("mlagg_conv3x3_wgrad_lp", _ptr(dy), dyb, _ptr(x), x.stride(0), _ptr(dW), _ptr(ws), B, O, I, H, W, form)
            else:
                dW = _lib_conv_bwd(dy.contiguous(), x, w, 1, 1, False, (False, True, False), form)[1]
        return dx, dW, None, None, None


# K19t: the 3 x 3, stride-2, padding-1 transposed convolution of PatchExpand (T:506-513) -- forward, data gradient and weight gradient
# (csrc/conv3x3_s2t.hip).  MLAGG_K19T=0: the library's transposed-convolution solvers, today's dispatch.
K19T = _os.environ.get("MLAGG_K19T", "1") == "1"
# The weight gradient on the kernel: off by default -- the per-lane loads of its 32 channel rows bind it on the texture addresser at 29-34
# TF/s, 2.6x MIOpen's time on the three PatchExpand shapes (profiles/round5_a_conv3x3_s2t_vs_miopen.log); forward and data gradient
# win (fp32: 442 vs 554 and 367 vs 485 us over the three layers at batch 10).  Per-product choice, as Conv3x3Fn makes it.
K19T_WGRAD = _os.environ.get("MLAGG_K19T_WGRAD", "0") == "1"


def _k19t_shape(O, I, H, W, form=_DTYPE_BF16X3):
    floor = K19_MIN_PIXELS if form == _DTYPE_BF16X3 else LP_K_MIN_PIXELS
    return K19T and H * W >= floor and bool(_lib.lib().mlagg_conv3x3_s2t_supported(O, I, H, W))


def _s2t_plan(O, I, H, W, form):
    on = _k19t_shape(O, I, H, W, form)
    return ("K19t" if on else None,) * 2 + ("K19t" if on and K19T_WGRAD else None,)


def _k19t_fwd(x, xb, w, O, I, H, W, form):
    B = x.shape[0]
    y = torch.empty(B, O, 2 * H - 1, 2 * W - 1, device=x.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().mlagg_conv3x3_s2t_workspace_bytes(O, I), device=x.device, dtype=torch.uint8)
    _flop("K19", 2 * 9 * B * O * I * H * W)
    _launch("mlagg_conv3x3_s2t_fwd", _ptr(x), xb, _ptr(w), _ptr(y), y.stride(0), _ptr(ws), B, O, I, H, W, form)
    return y


def _k19t_dgrad(dy, w, O, I, H, W, form):
    B = dy.shape[0]
    dx = torch.empty(B, I, H, W, device=dy.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().mlagg_conv3x3_s2t_workspace_bytes(O, I), device=dy.device, dtype=torch.uint8)
    _flop("K19", 2 * 9 * B * O * I * H * W)
    _launch("mlagg_conv3x3_s2_dgrad", _ptr(dy), dy.stride(0), dy.stride(1), dy.stride(2), _ptr(w), _ptr(dx), dx.stride(0), _ptr(ws), B, O,
            I, H, W, form)
    return dx


def _k19t_wgrad(x, xb, dy, O, I, H, W, form):
    B = x.shape[0]
    dW = torch.empty(I, O, 3, 3, device=x.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().mlagg_conv3x3_s2t_wgrad_workspace_floats(B, O, I, H, W), device=x.device, dtype=torch.float32)
    _flop("K19", 2 * 9 * B * O * I * H * W)
    _launch("mlagg_conv3x3_s2t_wgrad", _ptr(x), xb, _ptr(dy), dy.stride(0), dy.stride(1), dy.stride(2), _ptr(dW), _ptr(ws), B, O, I, H, W,
            form)
    return dW


class ConvT3x3S2Fn(torch.autograd.Function):
    """y = conv_transpose2d(x, W, stride=2, padding=1) for a dense 3 x 3 kernel (no bias), y (B, O, 2H - 1, 2W - 1): each product on
    K19t or on the library as the plan says (_s2t_plan unless one is given)."""

    @staticmethod
    def forward(ctx, x, weight, form=_DTYPE_BF16X3, plan=None):
        x, xb, _ = _planes(x, "x")
        B, I, H, W = x.shape
        O = int(weight.shape[1])
        plan = plan or _s2t_plan(O, I, H, W, form)
        w = _require(weight.contiguous(), "weight")
        y = _k19t_fwd(x, xb, w, O, I, H, W, form) if plan[0] else _lib_conv(x, w, 2, 1, True, form)
        ctx.save_for_backward(x, w)
        ctx.plan, ctx.form = plan, form
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        B, I, H, W = x.shape
        O = int(w.shape[1])
        (_, dgrad, wgrad), form = ctx.plan, ctx.form
        if dgrad and (dy.stride(3) != 1 or dy.data_ptr() % 4):
            dy = dy.contiguous()                                  # any channel / row stride is fine, a strided row is not
        dx = dW = None
        if ctx.needs_input_grad[0]:
            dx = _k19t_dgrad(dy, w, O, I, H, W, form) if dgrad else _lib_conv_bwd(dy, x, w, 2, 1, True, (True, False, False), form)[0]
        if ctx.needs_input_grad[1]:
            dW = _k19t_wgrad(x, x.stride(0), dy, O, I, H, W, form) if wgrad else _lib_conv_bwd(dy, x, w, 2, 1, True, (False, True, False), form)[1]
        return dx, dW, None, None


def _fp32_map(x, nd):
    """An fp32 device map with nd spatial axes?  (Reads attributes only: the plan tests stand a namespace in for a device tensor.)"""
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == nd + 2


def _all(v, n):
    return all(int(a) == n for a in v)


def conv_plan(x, weight, stride, padding, dilation, groups, transposed, output_padding, form):
    """Where each product of the bias-free 2-D convolution (transposed: conv_transpose2d) of `x` with `weight` runs, in operand form
    `form`: (forward, data gradient, weight gradient), each "K18", "K19", "K19t" or None (the library in the arithmetic of `form`) --
    or None where the whole layer is the library's.  A function of shapes, geometry, form and the switches above only."""
    if not (_fp32_map(x, 2) and groups == 1 and _all(dilation, 1) and _all(output_padding, 0)):
        return None
    geom = tuple(tuple(int(v) for v in t) for t in (weight.shape[2:], stride, padding)) + (bool(transposed),)
    I, O = (int(weight.shape[0]), int(weight.shape[1])) if transposed else (int(weight.shape[1]), int(weight.shape[0]))
    H, W = int(x.shape[2]), int(x.shape[3])
    P, one = H * W, form != _DTYPE_BF16X3                # one: a 16-bit mode's one-product form
    if geom[:3] == ((1, 1), (1, 1), (0, 0)):
        # 1 x 1 on K18; a transposed one (the segmentation heads, T:549-561: the same product, weight axes exchanged) only where all
        # three products run on it -- on the small maps the library's transposed-convolution solvers are the faster ones
        if not (K18 and P >= (LP_K_MIN_PIXELS if one else K18_WGRAD_MIN_PIXELS) and P % 16 == 0):
            return None
        plan = _conv1x1_plan(O, I, P, form)
        return None if transposed and None in plan else plan
    if geom == ((2, 2), (2, 2), (0, 0), True):           # K18 on the tap matrix + pixel shuffle (UnetrUpBlock)
        ok = K18 and W % 2 == 0 and P % 16 == 0 and _k18_product(4 * O, I, P, form) and _k18_product(I, 4 * O, P, form)
        return ("K18",) * 3 if ok else None
    if geom == ((3, 3), (1, 1), (1, 1), False):
        # K19 where forward or data gradient take it (16-bit operand forms: or the weight gradient -- the one-channel stem)
        plan = _conv3x3_plan(O, I, H, W, form)
        return plan if K19 and (plan[0] or plan[1] or (one and plan[2])) else None
    if geom == ((3, 3), (2, 2), (1, 1), True):           # K19t (PatchExpand)
        plan = _s2t_plan(O, I, H, W, form)
        return plan if plan[0] else None
    return None


def conv2d(x, weight, stride, padding, dilation, groups, transposed, output_padding, form):
    """The bias-free 2-D convolution (transposed: conv_transpose2d) on this package's kernels as conv_plan decides, or None: the
    caller's library path."""
    plan = conv_plan(x, weight, stride, padding, dilation, groups, transposed, output_padding, form)
    if plan is None:
        return None
    k = int(weight.shape[2])
    if k == 1:
        return Conv1x1Fn.apply(x, weight.permute(1, 0, 2, 3) if transposed else weight, form, plan)
    if k == 2:
        return ConvT2x2Fn.apply(x, weight, form)
    if transposed:
        return ConvT3x3S2Fn.apply(x, weight, form, plan)
    return Conv3x3Fn.apply(x, weight, form, claim_slot(x), plan)


# For a caller that knows the layer kind: conv_plan's layer rule for that kind, and that kind's Function on its own plan (no layer
# rule: every product on the library where its kernel does not take it).
def conv1x1_supported(x, weight, stride, padding, dilation, groups, form=_DTYPE_BF16X3):
    return tuple(weight.shape[2:]) == (1, 1) and conv_plan(x, weight, stride, padding, dilation, groups, False, (0, 0), form) is not None


def conv3x3_supported(x, weight, stride, padding, dilation, groups, form=_DTYPE_BF16X3):
    return tuple(weight.shape[2:]) == (3, 3) and conv_plan(x, weight, stride, padding, dilation, groups, False, (0, 0), form) is not None


def conv_t2x2_supported(x, weight, stride, padding, output_padding, dilation, groups, form=_DTYPE_BF16X3):
    return tuple(weight.shape[2:]) == (2, 2) and conv_plan(x, weight, stride, padding, dilation, groups, True, output_padding, form) is not None


def conv3x3_s2t_supported(x, weight, stride, padding, output_padding, dilation, groups, form=_DTYPE_BF16X3):
    return tuple(weight.shape[2:]) == (3, 3) and conv_plan(x, weight, stride, padding, dilation, groups, True, output_padding, form) is not None


def conv1x1(x, weight, form=_DTYPE_BF16X3):
    return Conv1x1Fn.apply(x, weight, form)


def conv3x3(x, weight, form=_DTYPE_BF16X3):
    return Conv3x3Fn.apply(x, weight, form, claim_slot(x))


def conv_t2x2(x, weight, form=_DTYPE_BF16X3):
    return ConvT2x2Fn.apply(x, weight, form)


def conv3x3_s2t(x, weight, form=_DTYPE_BF16X3):
    return ConvT3x3S2Fn.apply(x, weight, form)


K19_3D = _os.environ.get("MLAGG_K19_3D", "1") == "1"
K19_3D_WGRAD = _os.environ.get("MLAGG_K19_3D_WGRAD", "1") == "1"


# K19 adds every product of an output element into ONE fp32 accumulator chain, and the chain's rounding error grows with
# its length: measured against float64 as a share of the output's maximum, 4.5e-7 at 144 products, 1.0e-6 at 864, 1.3e-6 at 1728 and
# 2.65e-6 at the 2592 of a 96-channel 3 x 3 x 3 contraction (tests/test_conv_kernel_paths_gpu.py, F16) -- past the 2e-6 of an fp32
# convolution that the kernel is held to.  With 27 taps per channel the volumes get there at 3 x fewer channels than the maps, so their
# contraction runs in blocks of at most this many channels (864 products), each a launch of its own on a channel block of x, and the
# partial outputs are added: a blocked sum.
K19_3D_CHAIN_CH = 32


def _k19_3d_blocks(I):
    """[(first channel, end)] of the contraction blocks of a 3 x 3 x 3 product: equal multiples of 16, at most K19_3D_CHAIN_CH each."""
    n = -(-I // K19_3D_CHAIN_CH)
    step = -(-I // (16 * n)) * 16
    return [(c0, min(c0 + step, I)) for c0 in range(0, I, step)]


def _conv3x3x3_k19(x, xb, w, transposed, O, I, dims):
    B = x.shape[0]
    D, H, W = dims
    y = None
    for c0, c1 in _k19_3d_blocks(I):
        # the block's weight: rows of the layer's forward weight (contraction first) for a data gradient, else a copy of its columns
        xc, wc = (x, w) if (c0, c1) == (0, I) else (x[:, c0:c1], w[c0:c1] if transposed else w[:, c0:c1].contiguous())
        part = torch.empty(B, O, D, H, W, device=x.device, dtype=torch.float32)
        ws = torch.empty(_lib.lib().mlagg_conv3x3x3_workspace_bytes(O, c1 - c0), device=x.device, dtype=torch.uint8)
        _launch("mlagg_conv3x3x3_fwd", _ptr(xc), xb, _ptr(wc), int(transposed), None, _ptr(part), O * D * H * W, _ptr(ws), B, O, c1 - c0,
                D, H, W)
        y = part if y is None else y.add_(part)
    return y


def _pad_geometry(D, H, W, stride, wide=False):
    Dq, Hq, Wq, guard = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    _lib.check(_lib.lib().mlagg_conv_pad_geometry(D, H, W, stride, int(wide), ctypes.byref(Dq), ctypes.byref(Hq), ctypes.byref(Wq),
                                                  ctypes.byref(guard)), "mlagg_conv_pad_geometry")
    return Dq.value, Hq.value, Wq.value, guard.value


# The models run K15 on the weight gradients of 3-D convolutions only, where MIOpen has no tuned solver (8.2 s -> 66 ms per step at
# 2 x 96x160x160 voxels).  Not on the 2-D network's dense convolutions: measured on the 21 convolution shapes of the 256 x 256 step
# (profiles/round3_conv_wgrad_2d_shapes_k15_vs_miopen.log), MIOpen's weight-gradient solvers are 1.1-1.9x faster on the 3x3 shapes
# (K15 incl. its two pad copies reaches 28-59 TFLOP/s there) and 4-7x on the 1x1 shapes (plain GEMMs); step 43.5 -> 56.2 ms with it.
# K16 (forward / data gradient of the 3-D stride-1 convolutions on the tap-GEMM kernel) -- MLAGG_K16=0: MIOpen
K16 = _os.environ.get("MLAGG_K16", "1") == "1"


class _Padded:
    """A channel-major map copied into the zero-padded box of the tap-GEMM kernels (csrc/conv_wgrad.hip mlagg_volume_pad)."""

    def __init__(self, t, dims, stride, wide, as_output_of=None):
        t = _require(t.contiguous(), "map")
        self.B, self.C = t.shape[:2]
        self.dims = tuple(dims)                                    # geometry of the convolution INPUT
        self.stride, self.wide = stride, wide
        self.Dq, self.Hq, self.Wq, self.guard = _pad_geometry(*self.dims, stride, wide)
        self.Q = self.Dq * self.Hq * self.Wq
        self.row = 2 * self.guard + self.Q
        self.nph = 1 if (stride == 1 or as_output_of is not None) else 8
        self.buf = torch.empty(self.B, self.nph, self.C, self.row, device=t.device, dtype=torch.float32)
        od = tuple(t.shape[2:]) if t.dim() == 5 else (1,) + tuple(t.shape[2:])
        if as_output_of is None:
            _launch("mlagg_volume_pad", _ptr(t), _ptr(self.buf), self.B, self.C, *self.dims, stride, int(wide), 0, 0, 0, 0)
        else:
            _launch("mlagg_volume_pad", _ptr(t), _ptr(self.buf), self.B, self.C, *self.dims, stride, int(wide), 1, *od)

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.guard


def _tap_offsets(k, nd, stride, Hq, Wq, I=0, row=0):
    taps = []
    kz_range = range(k) if nd == 3 else (k // 2,)
    for kz in kz_range:
        for ky in range(k):
            for kx in range(k):
                if stride == 1:
                    dz = (kz - k // 2) if nd == 3 else 0
                    taps.append(dz * Hq * Wq + (ky - k // 2) * Wq + (kx - k // 2))
                else:
                    # padded input index 2 z + kz (k = 3) or 2 z + 1 (k = 1): parity phase + shift
                    az, ay, ax = (kz, ky, kx) if k == 3 else (1, 1, 1)
                    ph = ((az & 1) << 2) | ((ay & 1) << 1) | (ax & 1)
                    taps.append(ph * I * row + (az >> 1) * Hq * Wq + (ay >> 1) * Wq + (ax >> 1))
    return taps


def _wgrad_from_padded(xp, dyp, k, nd):
    """K15 on the padded copies of the input (xp) and of the output gradient (dyp, same box geometry): dW (O, I, k^nd)."""
    O, I, B = dyp.C, xp.C, xp.B
    taps = _tap_offsets(k, nd, xp.stride, xp.Hq, xp.Wq, I, xp.row)
    ntaps = len(taps)
    Q8 = (xp.Q + 7) & ~7
    off = (ctypes.c_long * ntaps)(*taps)
    dW = torch.empty(O, I, ntaps, device=xp.buf.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().mlagg_conv_wgrad_taps_workspace_floats(B, Q8, O, I, ntaps), device=xp.buf.device, dtype=torch.float32)
    _launch("mlagg_conv_wgrad_taps", dyp.ptr(), O * dyp.row, dyp.row, xp.ptr(), xp.nph * I * xp.row, xp.row, off, ntaps, Q8, O, I, B,
            _ptr(dW), 0, _ptr(ws))
    return dW


def conv_weight_grad(x, dy, k, stride):
    """dW (O, I, k^nd) of a convolution y = conv(x, W, stride, padding k // 2) from x (B, I, *dims) and dy (B, O, *out_dims)."""
    nd = x.dim() - 2
    dims = tuple(x.shape[2:]) if nd == 3 else (1,) + tuple(x.shape[2:])
    xp = _Padded(x, dims, stride, False)
    dyp = _Padded(dy, dims, stride, False, as_output_of=xp)
    return _wgrad_from_padded(xp, dyp, k, nd)


def _conv_taps(src, weight, O, I, k, flip, dims):
    """K16 on a padded copy `src` (wide stride-1 box): y (B, O, *dims) with weight (O', I', k^3) read as [o][i] (forward) or
    transposed with flipped taps (data gradient: O = the convolution's input channels)."""
    ntaps = k ** 3
    taps = _tap_offsets(k, 3, 1, src.Hq, src.Wq)
    off = (ctypes.c_long * ntaps)(*taps)
    y = torch.empty(src.B, O, *dims, device=src.buf.device, dtype=torch.float32)
    w = _require(weight.contiguous(), "weight")
    if flip:      # weight (Cout_conv = I here, Cin_conv = O here, taps): output channel o -> stride ntaps, contraction i -> stride O * ntaps
        w_so, w_si = ntaps, O * ntaps
    else:
        w_so, w_si = I * ntaps, ntaps
    _launch("mlagg_conv_taps", src.ptr(), src.C * src.row, src.row, _ptr(w), w_so, w_si, int(flip), off, ntaps, _ptr(y), src.B, O, I, *dims)
    return y


def conv_wgrad_supported(x, weight, stride, padding):
    """K15's geometry: kernel 3 with padding 1 or kernel 1 with padding 0, isotropic, stride 1 (2-D and 3-D) or 2 (3-D), fp32 device
    maps."""
    nd, k = x.dim() - 2, int(weight.shape[2])
    return (nd in (2, 3) and _fp32_map(x, nd) and k in (1, 3) and _all(weight.shape[2:], k) and _all(padding, k // 2)
            and len(set(int(v) for v in stride)) == 1
            and (int(stride[0]) == 1 or (int(stride[0]) == 2 and nd == 3 and all(int(v) > 1 for v in x.shape[2:]))))


def conv_taps_supported(x, weight, stride, padding):
    """K16: 3-D, stride 1, last extent a multiple of 4, at least 8 input channels (a 1-channel stem would waste 31 / 32 of the MFMAs)."""
    return (K16 and x.dim() == 5 and conv_wgrad_supported(x, weight, stride, padding) and int(stride[0]) == 1 and x.shape[-1] % 4 == 0
            and x.shape[1] >= 8)


def conv3x3x3_supported(x, weight, stride, padding):
    """K19's 3-D forward: 3 x 3 x 3, stride 1, padding 1."""
    return (K19_3D and _fp32_map(x, 3) and tuple(weight.shape[2:]) == (3, 3, 3) and _all(stride, 1) and _all(padding, 1)
            and bool(_lib.lib().mlagg_conv3x3x3_supported(int(weight.shape[0]), int(weight.shape[1]), *(int(v) for v in x.shape[2:]))))


def conv_nd_plan(x, weight, stride, padding):
    """Where each product of the bias-free convolution of `x` (2-D or 3-D) with `weight` runs: (forward, data gradient, weight
    gradient) -- "K19", "K16" (tap GEMMs on a wide padded copy of x, kept for K15) or None (the library) for the first two, "K19" or
    "K15" (tap GEMMs on padded copies) for the third -- or None where the whole layer is the library's.  The layer rules above, in
    this order; a function of shapes, geometry and the switches above only."""
    if conv3x3x3_supported(x, weight, stride, padding):
        O, I, dims, lib = int(weight.shape[0]), int(weight.shape[1]), tuple(int(v) for v in x.shape[2:]), _lib.lib()
        # the data gradient where its contraction (the layer's output channels) is a multiple of 16, the weight gradient where the
        # width is a multiple of 8 (else K15 on non-wide padded copies made in backward)
        return ("K19", "K19" if lib.mlagg_conv3x3x3_supported(I, O, *dims) else None,
                "K19" if K19_3D_WGRAD and lib.mlagg_conv3x3x3_wgrad_supported(O, I, *dims) else "K15")
    if conv_taps_supported(x, weight, stride, padding):
        return "K16", "K16", "K15"
    return (None, None, "K15") if conv_wgrad_supported(x, weight, stride, padding) else None


class ConvNdFn(torch.autograd.Function):
    """y = conv(x, W) (no bias) on channel-major maps, each product where conv_nd_plan says: K19 straight on the NCDHW volumes (27
    shifted split-bf16 GEMMs, no padded copy), K16 / K15 on zero-padded copies, or the library (MIOpen: the north star's "conv stem /
    decoder stages live in PyTorch-ROCm")."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding, plan):
        dims = tuple(int(v) for v in x.shape[2:])
        O, I = int(weight.shape[0]), int(weight.shape[1])
        ctx.xp = None
        if plan[0] == "K19":
            x, xb, _ = _planes(x, "x")
            weight = _require(weight.contiguous(), "weight")
            y = _conv3x3x3_k19(x, xb, weight, False, O, I, dims)
        elif plan[0] == "K16":
            ctx.xp = _Padded(x, dims, 1, True)
            y = _conv_taps(ctx.xp, weight, O, I, int(weight.shape[2]), False, dims)
            x = None                                                    # backward reads the padded copy
        else:
            y = _lib_conv(x, weight, stride, padding, False, _DTYPE_BF16X3)
        ctx.save_for_backward(x, weight)
        ctx.geom, ctx.plan = (stride, padding), plan
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        (stride, padding), (_, dgrad, wgrad), xp = ctx.geom, ctx.plan, ctx.xp
        O, I, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        if xp is not None:
            dims, dyp = xp.dims, _Padded(dy, xp.dims, 1, True, as_output_of=xp)
        else:
            dims, dy = tuple(int(v) for v in x.shape[2:]), dy.contiguous()
        dx = dW = None
        if ctx.needs_input_grad[0]:
            if dgrad == "K19":
                dx = _conv3x3x3_k19(dy, O * dims[0] * dims[1] * dims[2], w, True, I, O, dims)
            elif dgrad == "K16":
                dx = _conv_taps(dyp, w, I, O, k, True, dims)
            else:
                dx = _lib_conv_bwd(dy, x, w, stride, padding, False, (True, False, False), _DTYPE_BF16X3)[0]
        if ctx.needs_input_grad[1]:
            if wgrad == "K19":
                B = x.shape[0]
                dW = torch.empty(O, I, 3, 3, 3, device=x.device, dtype=torch.float32)
                ws = torch.empty(_lib.lib().mlagg_conv3x3x3_wgrad_workspace_floats(B, O, I, *dims), device=x.device, dtype=torch.float32)
                _launch("mlagg_conv3x3x3_wgrad", _ptr(dy), O * dims[0] * dims[1] * dims[2], _ptr(x), x.stride(0), _ptr(dW), _ptr(ws), B, O,
                        I, *dims)
            elif xp is not None:
                dW = _wgrad_from_padded(xp, dyp, k, 3).view(w.shape)
            else:
                dW = conv_weight_grad(x, dy, k, stride).view(w.shape)
        ctx.xp = None
        return dx, dW, None, None, None


def conv_nd(x, weight, stride, padding):
    """Bias-free convolution on conv_nd_plan's kernels; plain torch where the plan is None."""
    plan = conv_nd_plan(x, weight, stride, padding)
    if plan is not None:
        return ConvNdFn.apply(x, weight, int(stride[0]), int(padding[0]), plan)
    return (torch.nn.functional.conv3d if x.dim() == 5 else torch.nn.functional.conv2d)(x, weight, None, stride, padding)


# ------------------------------------------------------------------------------------------------
# K20: 3-D sliding-window inference (csrc/sliding_window.hip).  Mirror variants are bitmasks of flipped tile axes (bit a = axis a),
# in the reference's order (inference.mirror_variants).  No autograd: inference only.
# ------------------------------------------------------------------------------------------------
def _expect(t, name, dtype=torch.float32, dim=None, shape=None, contiguous=True, like=None):
    """The input check of the inference-only entry points (K20-K25): a `dtype` tensor on the MI355X device (`like`'s device when
    given), of rank `dim` / shape `shape` when given, contiguous unless `contiguous` is False."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and (like is None or t.device == like.device)
            and (dim is None or t.dim() == dim) and (shape is None or tuple(t.shape) == tuple(shape))
            and (not contiguous or t.is_contiguous())):
        want = (f"{'contiguous ' if contiguous else ''}{'' if dim is None else f'{dim}-D '}{dtype} tensor"
                f"{'' if shape is None else f' of shape {tuple(shape)}'} on {'the MI355X device' if like is None else like.device}")
        strided = isinstance(t, torch.Tensor) and not t.is_contiguous()
        raise RuntimeError(f"{name}: expected a {want}, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}"
                           f"{' (non-contiguous)' if strided else ''} on {getattr(t, 'device', '?')}")


def _sw_flips(flips):
    flips = [int(m) for m in flips]
    if len(flips) not in (1, 2, 4, 8) or any(m < 0 or m > 7 for m in flips) or len(set(flips)) != len(flips):
        raise RuntimeError(f"mirror variants {flips}: 1, 2, 4 or 8 distinct masks in [0, 7]")
    return flips


def _sw_box(origin, tile, shape, what):
    o = tuple(int(v) for v in origin)
    if len(o) != 3 or any(v < 0 or v + t > s for v, t, s in zip(o, tile, shape)):
        raise RuntimeError(f"{what}: tile at {o} of size {tuple(tile)} is not inside the volume {tuple(shape)}")
    return o


def sliding_window_gather(volume, origins, flips, tile_size):
    """volume (C, X, Y, Z) -> network input (V * n, C, tx, ty, tz): the n tiles at `origins`, variant-major, variant v flipped
    along the axes of mask flips[v]."""
    _expect(volume, "volume", dim=4)
    flips = _sw_flips(flips)
    tile = tuple(int(t) for t in tile_size)
    if len(tile) != 3 or min(tile) < 1:
        raise RuntimeError(f"tile_size {tile_size}: three positive sides")
    C, X, Y, Z = volume.shape
    boxes = [_sw_box(o, tile, (X, Y, Z), "sliding_window_gather") for o in origins]
    if not boxes:
        raise RuntimeError("sliding_window_gather: no tiles")
    out = torch.empty((len(flips) * len(boxes), C) + tile, device=volume.device, dtype=torch.float32)
    _launch("mlagg_sw_gather", _ptr(volume), C, X, Y, Z, _int_array([v for o in boxes for v in o]), len(boxes), _int_array(flips),
            len(flips), _ptr(out), *tile)
    return out


SW_SEG_KINDS = {torch.int8: _C["MLAGG_SEG_INT8"], torch.uint8: _C["MLAGG_SEG_UINT8"], torch.int16: _C["MLAGG_SEG_INT16"]}


def sliding_window_gather_onehot(volume, seg, labels, origins, flips, tile_size):
    """K32: volume (C, X, Y, Z) fp32 and seg (X, Y, Z) int8 / uint8 / int16 labels -> network input (V * n, C + L, tx, ty, tz) of a
    cascaded stage: channels 0 .. C-1 as sliding_window_gather, channel C + i the fp32 indicator seg == labels[i] of the same
    (flipped) voxels.  labels: L values in 1 .. 255, L <= 64.  The one-hot volume is never built."""
    _expect(volume, "volume", dim=4)
    if not isinstance(seg, torch.Tensor) or seg.dtype not in SW_SEG_KINDS:
        raise RuntimeError(f"seg: expected an int8, uint8 or int16 tensor, got {getattr(seg, 'dtype', type(seg))}")
    _expect(seg, "seg", dtype=seg.dtype, shape=volume.shape[1:], like=volume)
    flips = _sw_flips(flips)
    tile = tuple(int(t) for t in tile_size)
    if len(tile) != 3 or min(tile) < 1:
        raise RuntimeError(f"tile_size {tile_size}: three positive sides")
    labels = [int(v) for v in labels]
    C, X, Y, Z = volume.shape
    boxes = [_sw_box(o, tile, (X, Y, Z), "sliding_window_gather_onehot") for o in origins]
    if not boxes:
        raise RuntimeError("sliding_window_gather_onehot: no tiles")
    out = torch.empty((len(flips) * len(boxes), C + len(labels)) + tile, device=volume.device, dtype=torch.float32)
    # the entry refuses an empty or too long label list and labels outside 1 .. 255
    _launch("mlagg_sw_gather_onehot", _ptr(volume), C, _ptr(seg), SW_SEG_KINDS[seg.dtype], _int_array(labels), len(labels), X, Y, Z,
            _int_array([v for o in boxes for v in o]), len(boxes), _int_array(flips), len(flips), _ptr(out), *tile)
    return out


def sliding_window_fold(out, tile, n, flips, gaussian, origin, acc, weight):
    """Fold tile `tile` of the chunk output out (V * n, K, tx, ty, tz) into acc (K, X, Y, Z) and weight (X, Y, Z) at `origin`:
    acc += mean over the variants of the flipped-back outputs * gaussian, weight += gaussian (in place)."""
    _expect(out, "out", dim=5)
    _expect(acc, "acc", dim=4)
    _expect(weight, "weight", dim=3)
    flips = _sw_flips(flips)
    V, n, tile = len(flips), int(n), int(tile)
    K, tx, ty, tz = (int(v) for v in out.shape[1:])
    gaussian = _require(gaussian.contiguous(), "gaussian", (tx, ty, tz))
    if out.shape[0] != V * n or not 0 <= tile < n:
        raise RuntimeError(f"sliding_window_fold: out has {out.shape[0]} rows, expected {V} variants x {n} tiles; tile {tile}")
    if acc.shape[0] != K or acc.shape[1:] != weight.shape:
        raise RuntimeError(f"sliding_window_fold: acc {tuple(acc.shape)} / weight {tuple(weight.shape)} for {K} classes")
    X, Y, Z = weight.shape
    o = _sw_box(origin, (tx, ty, tz), (X, Y, Z), "sliding_window_fold")
    _launch("mlagg_sw_fold", _ptr(out), tile, n, _int_array(flips), V, K, _ptr(gaussian), tx, ty, tz, *o, _ptr(acc), _ptr(weight), X, Y, Z)


def sliding_window_finalize(acc, weight, region, return_labels=False):
    """logits (K, X0, Y0, Z0) = acc / weight on `region` (three slices with explicit bounds), a new contiguous tensor; with
    return_labels also the int64 argmax over K (torch.argmax's first-maximum rule).  Returns (logits, labels or None)."""
    _expect(acc, "acc", dim=4)
    _expect(weight, "weight", dim=3)
    if acc.shape[1:] != weight.shape:
        raise RuntimeError(f"sliding_window_finalize: acc {tuple(acc.shape)} / weight {tuple(weight.shape)}")
    K = int(acc.shape[0])
    shape = tuple(int(s) for s in weight.shape)
    lo, size = [], []
    for sl, s in zip(region, shape):
        a, b = (0 if sl.start is None else int(sl.start)), (s if sl.stop is None else int(sl.stop))
        if sl.step not in (None, 1) or not 0 <= a < b <= s:
            raise RuntimeError(f"sliding_window_finalize: region {region} is not inside {shape}")
        lo.append(a)
        size.append(b - a)
    if len(lo) != 3:
        raise RuntimeError("sliding_window_finalize: region must hold three slices")
    logits = torch.empty((K,) + tuple(size), device=acc.device, dtype=torch.float32)
    labels = torch.empty(tuple(size), device=acc.device, dtype=torch.int64) if return_labels else None
    _launch("mlagg_sw_finalize", _ptr(acc), _ptr(weight), K, *shape, *lo, *size, _ptr(logits), _ptr(labels))
    return logits, labels


# ------------------------------------------------------------------------------------------------
# K21: prediction export (csrc/export.hip).  The per-axis tap tables come from export._axis_taps as host numpy arrays
# (idx (X' + Y' + Z', 2) int32, w (X' + Y' + Z', 2) float64); they are checked against the logits' extent here, on the host, before
# the single upload of the call, so the kernels never read outside the logits.  No autograd: inference only.
# ------------------------------------------------------------------------------------------------
def _strided_volume(t, name):
    """(shape, strides) of a non-empty (C, X, Y, Z) fp32 device tensor that the kernels read through its strides."""
    _expect(t, name, dim=4, contiguous=False)
    if min(t.shape) < 1 or min(t.stride()) < 0:
        raise RuntimeError(f"{name}: expected a non-empty (C, X, Y, Z) tensor with non-negative strides, got shape {tuple(t.shape)}, "
                           f"strides {t.stride()}")
    return tuple(int(s) for s in t.shape), tuple(int(s) for s in t.stride())


def _export_taps(taps, in_shape, out_shape, device):
    idx, w = (np.ascontiguousarray(a) for a in taps)
    n = sum(out_shape)
    if idx.dtype != np.int32 or w.dtype != np.float64 or idx.shape != (n, 2) or w.shape != (n, 2):
        raise RuntimeError(f"tap tables: expected int32 / float64 ({n}, 2) arrays for output shape {tuple(out_shape)}")
    lo = 0
    for n_in, n_out in zip(in_shape, out_shape):
        part = idx[lo:lo + n_out]
        if part.min() < 0 or part.max() >= n_in:
            raise RuntimeError(f"tap tables: an index outside [0, {n_in}) for an axis of {n_in} -> {n_out}")
        lo += n_out
    return torch.from_numpy(idx).to(device), torch.from_numpy(w).to(device)


def resample_linear(logits, taps, out_shape):
    """logits (C, X, Y, Z) fp32, any non-negative strides -> (C, *out_shape) contiguous fp32: out[c, o] = the separable blend of the
    two taps of every axis at o (taps = export._axis_taps tables), in fp64, rounded once."""
    shape, st = _strided_volume(logits, "logits")
    out_shape = tuple(int(s) for s in out_shape)
    if len(out_shape) != 3 or min(out_shape) < 1:
        raise RuntimeError(f"resample_linear: output shape {out_shape}")
    idx, w = _export_taps(taps, shape[1:], out_shape, logits.device)
    out = torch.empty((shape[0],) + out_shape, device=logits.device, dtype=torch.float32)
    _launch("mlagg_resample_linear", _ptr(logits), *shape, *st, _ptr(idx), _ptr(w), _ptr(out), *out_shape)
    return out


EXPORT_MAX_CLASSES = 32        # classes held in registers by the fused export kernel


def export_segmentation(logits, taps, crop_shape, box_lo, shape_before_cropping, transpose_backward, return_probabilities=False,
                        regions_class_order=None):
    """The fused export of K <= 32 classes: resample logits (K, X, Y, Z) to crop_shape with the tap tables, fp32 softmax over K,
    first-maximum argmax, pasted at box_lo into shape_before_cropping (zeros outside) and transposed by transpose_backward.
    regions_class_order (K labels in 0 .. 255): the heads are the sigmoid regions of a region-based label manager -- fp32 sigmoid
    per head, and the label is 0, then regions_class_order[i] wherever sigmoid_i > 0.5, i = 0 .. K-1 in order.
    Returns (labels uint8, probabilities (K, ...) fp32 or None), contiguous."""
    shape, st = _strided_volume(logits, "logits")
    K = shape[0]
    if K > EXPORT_MAX_CLASSES:
        raise RuntimeError(f"export_segmentation: {K} classes, the fused kernel holds at most {EXPORT_MAX_CLASSES}")
    crop = tuple(int(s) for s in crop_shape)
    lo = tuple(int(v) for v in box_lo)
    full = tuple(int(s) for s in shape_before_cropping)
    perm = tuple(int(p) for p in transpose_backward)
    if len(crop) != 3 or len(lo) != 3 or len(full) != 3 or sorted(perm) != [0, 1, 2]:
        raise RuntimeError(f"export_segmentation: crop {crop}, box {lo}, shape {full}, transpose {perm}")
    if any(c < 1 or a < 0 or a + c > s for c, a, s in zip(crop, lo, full)):
        raise RuntimeError(f"export_segmentation: a box of {crop} at {lo} is not inside {full}")
    idx, w = _export_taps(taps, shape[1:], crop, logits.device)
    out_shape = tuple(full[p] for p in perm)
    labels = torch.empty(out_shape, device=logits.device, dtype=torch.uint8)
    probs = torch.empty((K,) + out_shape, device=logits.device, dtype=torch.float32) if return_probabilities else None
    if regions_class_order is not None:
        order = [int(v) for v in regions_class_order]
        if len(order) != K or any(not 0 <= v <= 255 for v in order):
            raise RuntimeError(f"export_segmentation: regions_class_order {order} for {K} heads (one uint8 label per head)")
        _launch("mlagg_export_segmentation_regions", _ptr(logits), *shape, *st, _ptr(idx), _ptr(w), *crop, _int_array(lo),
                _int_array(full), _int_array(perm), _int_array(order), _ptr(labels), _ptr(probs))
        return labels, probs
    _launch("mlagg_export_segmentation", _ptr(logits), *shape, *st, _ptr(idx), _ptr(w), *crop, _int_array(lo), _int_array(full),
            _int_array(perm), _ptr(labels), _ptr(probs))
    return labels, probs


# ------------------------------------------------------------------------------------------------
# K22: case preprocessing (csrc/preprocess.hip).  The cubic tap tables come from preprocessing._cubic_taps and the order-0 / order-1
# tables from export._axis_taps, as host numpy arrays; they are checked here, on the host, before their upload, so the kernels never
# read outside a line.  No autograd: inference only.
# ------------------------------------------------------------------------------------------------
PP_SCHEMES = {"NoNormalization": _C["MLAGG_PP_NONE"], "CTNormalization": _C["MLAGG_PP_CT"], "ZScoreNormalization": _C["MLAGG_PP_ZSCORE"],
              "ZScoreNormalization+mask": _C["MLAGG_PP_ZSCORE_MASKED"], "RescaleTo01Normalization": _C["MLAGG_PP_RESCALE01"],
              "RGBTo01Normalization": _C["MLAGG_PP_RGB01"]}
PP_STATS_PARTIALS = _C["MLAGG_PP_STATS_PARTIALS"]


def _pp_window(shape, lo, ext):
    lo, ext = tuple(int(v) for v in lo), tuple(int(v) for v in ext)
    if len(lo) != 3 or len(ext) != 3 or any(a < 0 or e < 1 or a + e > s for a, e, s in zip(lo, ext, shape[1:])):
        raise RuntimeError(f"crop window of {ext} at {lo} is not inside {tuple(shape[1:])}")
    return lo, ext


def pp_nonzero_box(x):
    """x (C, X, Y, Z) fp32, any non-negative strides -> int32 device tensor (6,): min x, y, z and max x, y, z of the voxels that are
    non-zero in any channel; (2^31 - 1, -1) per axis when there are none."""
    shape, st = _strided_volume(x, "image")
    box = torch.empty(6, dtype=torch.int32, device=x.device)
    _launch("mlagg_pp_nonzero_box", _ptr(x), *shape, *st, _ptr(box))
    return box


def pp_channel_stats(x, lo, ext, c, scheme, params, stats, mask=None):
    """Channel c of x's crop window (under mask, (ext) uint8, for the masked ZScore): fills stats[c] = fp64 (mean, std, min, max) and
    the scheme's fp32 constants in params[c] (see mlagg_pp_channel_stats)."""
    shape, st = _strided_volume(x, "image")
    lo, ext = _pp_window(shape, lo, ext)
    if not 0 <= c < shape[0] or scheme not in PP_SCHEMES.values():
        raise RuntimeError(f"pp_channel_stats: channel {c} of {shape[0]}, scheme {scheme}")
    _expect(params, "params", shape=(shape[0], 4), like=x)
    _expect(stats, "stats", torch.float64, shape=(shape[0], 4), like=x)
    if scheme == PP_SCHEMES["ZScoreNormalization+mask"]:
        _expect(mask, "mask of the masked ZScore", torch.uint8, shape=ext, like=x)
    partials = torch.empty(shape[0] * PP_STATS_PARTIALS * 5, dtype=torch.float64, device=x.device)
    _launch("mlagg_pp_channel_stats", _ptr(x), *shape, *st, _int_array(lo), _int_array(ext), int(c), int(scheme), _ptr(mask),
            _ptr(partials), _ptr(params), _ptr(stats))


def pp_normalize(x, lo, ext, schemes, params, mask=None):
    """Crop x to the window and normalise every channel with its scheme code (PP_SCHEMES) in fp32 -> (C, *ext) contiguous fp32.
    schemes: int32 device tensor (C,); params: fp32 device tensor (C, 4); mask: (ext) uint8 for the masked ZScore."""
    shape, st = _strided_volume(x, "image")
    lo, ext = _pp_window(shape, lo, ext)
    _expect(schemes, "schemes", torch.int32, shape=(shape[0],), like=x)
    _expect(params, "params", shape=(shape[0], 4), like=x)
    if mask is not None:
        _expect(mask, "mask", torch.uint8, shape=ext, like=x)
    elif bool((schemes == PP_SCHEMES["ZScoreNormalization+mask"]).any()):
        raise RuntimeError("pp_normalize: the masked ZScore needs a mask")
    out = torch.empty((shape[0],) + ext, dtype=torch.float32, device=x.device)
    _launch("mlagg_pp_normalize", _ptr(x), *shape, *st, _int_array(lo), _int_array(ext), _ptr(schemes), _ptr(params), _ptr(mask), _ptr(out))
    return out


def pp_clip_ranges(x, axis=None):
    """x (C, X, Y, Z) contiguous fp32 -> (lo, hi) int32 device tensors (C * D,) of ordered-int encoded min / max: per channel
    (axis None, D = 1) or per channel and slice along spatial axis `axis` (D = its extent)."""
    shape, _ = _strided_volume(x, "image")
    if not x.is_contiguous():
        raise RuntimeError("pp_clip_ranges: x must be contiguous")
    D = 1 if axis is None else shape[1 + int(axis)]
    lo = torch.empty(shape[0] * D, dtype=torch.int32, device=x.device)
    hi = torch.empty_like(lo)
    _launch("mlagg_pp_clip_ranges", _ptr(x), *shape, -1 if axis is None else int(axis), _ptr(lo), _ptr(hi))
    return lo, hi


def _line_geometry(x, axis):
    if x.dim() != 4 or not x.is_contiguous() or not x.is_cuda or not 0 <= axis <= 2:
        raise RuntimeError(f"expected a contiguous (C, X, Y, Z) device tensor and a spatial axis, got {tuple(x.shape)}, axis {axis}")
    shape = tuple(int(s) for s in x.shape)
    outer = int(np.prod(shape[:1 + axis]))
    inner = int(np.prod(shape[2 + axis:]))
    return shape, outer, shape[1 + axis], inner


def pp_cubic_axis(x, axis, taps, fir, out_dtype=torch.float64, clip=None):
    """One axis of the cubic zoom: x (C, X, Y, Z) contiguous fp32 | fp64 -> the same with `axis` resampled by taps =
    preprocessing._cubic_taps(n_in, n_out) (start, w, P0, M), fir: the 31 prefilter taps.  clip = (lo, hi, D, domain axis or None):
    pp_clip_ranges output for the output's domains."""
    if x.dtype not in (torch.float32, torch.float64) or out_dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"pp_cubic_axis: fp32 / fp64 only, got {x.dtype} -> {out_dtype}")
    shape, outer, n_in, inner = _line_geometry(x, axis)
    start, w, P0, M = taps
    start, w = np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(w, dtype=np.float64)
    n_out = start.shape[0]
    if n_out < 1 or w.shape != (n_out, 4) or start.min() < P0 or start.max() + 4 > P0 + M or P0 < 0 or P0 + M > n_in + 24:
        raise RuntimeError(f"pp_cubic_axis: tap table does not fit a line of {n_in}")
    if _lib.lib().mlagg_pp_cubic_lines_per_block(n_in, int(M)) < 1:
        raise RuntimeError(f"pp_cubic_axis: a line of {n_in} -> {n_out} samples does not fit the kernel's LDS plan")
    fir = torch.as_tensor(np.ascontiguousarray(fir, dtype=np.float64))
    if fir.shape != (31,):
        raise RuntimeError("pp_cubic_axis: 31 prefilter taps expected")
    out_shape = list(shape)
    out_shape[1 + axis] = n_out
    out = torch.empty(out_shape, dtype=out_dtype, device=x.device)
    d_start, d_w = torch.from_numpy(start).to(x.device), torch.from_numpy(w).to(x.device)
    clo = chi = None
    cstride = dstride = D = 1
    if clip is not None:
        clo, chi, D, dax = clip
        V = int(np.prod(out_shape[1:]))
        cstride = V
        dstride = V if dax is None else int(np.prod(out_shape[2 + dax:]))
        if D != (1 if dax is None else out_shape[1 + dax]) or clo.numel() != shape[0] * D or chi.numel() != shape[0] * D:
            raise RuntimeError("pp_cubic_axis: clip ranges do not match the output's domains")
    _launch("mlagg_pp_cubic_axis", _ptr(x), int(x.dtype == torch.float64), _ptr(out), int(out_dtype == torch.float64), outer, n_in, inner,
            n_out, _ptr(d_start), _ptr(d_w), int(P0), int(M), fir.data_ptr(), _ptr(clo), _ptr(chi), cstride, dstride, int(D))
    return out


def pp_gather_axis(x, axis, taps):
    """x (C, X, Y, Z) contiguous fp64 -> fp32 with `axis` resampled by an export._axis_taps table (order 0 or 1)."""
    if x.dtype != torch.float64:
        raise RuntimeError(f"pp_gather_axis: fp64 input expected, got {x.dtype}")
    shape, outer, n_in, inner = _line_geometry(x, axis)
    idx, w = (np.ascontiguousarray(a) for a in taps)
    n_out = idx.shape[0]
    if idx.dtype != np.int32 or w.dtype != np.float64 or idx.shape != (n_out, 2) or w.shape != (n_out, 2) or n_out < 1:
        raise RuntimeError("pp_gather_axis: int32 / float64 (n_out, 2) tables expected")
    if idx.min() < 0 or idx.max() >= n_in:
        raise RuntimeError(f"pp_gather_axis: an index outside [0, {n_in})")
    out_shape = list(shape)
    out_shape[1 + axis] = n_out
    out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    d_idx, d_w = torch.from_numpy(idx).to(x.device), torch.from_numpy(w).to(x.device)
    _launch("mlagg_pp_gather_axis", _ptr(x), _ptr(out), outer, n_in, inner, n_out, _ptr(d_idx), _ptr(d_w))
    return out


# ------------------------------------------------------------------------------------------------
# K26: the segmentation of a training case and ordered rank selection (csrc/preprocess_train.hip).  Label volumes are int16
# device tensors; `max_label` is the largest label the caller expects, and the histograms returned are int64 device tensors
# (max_label + 3,): labels -1 .. max_label, then the count of any other label.  Inference-style: no autograd.
# ------------------------------------------------------------------------------------------------
PP_RANK_BLOCK = _C["MLAGG_PP_RANK_BLOCK"]
PP_MAX_GROUPS = _C["MLAGG_PP_MAX_GROUPS"]


def _pp_label_volume(seg, name, contiguous=True):
    _expect(seg, name, torch.int16, dim=3, contiguous=contiguous)
    if min(seg.shape) < 1 or min(seg.stride()) < 0:
        raise RuntimeError(f"{name}: expected a non-empty (X, Y, Z) volume with non-negative strides, got {tuple(seg.shape)}, {seg.stride()}")
    return tuple(int(s) for s in seg.shape)


def _pp_max_label(max_label):
    max_label = int(max_label)
    if not 0 <= max_label <= 32767:
        raise RuntimeError(f"max_label {max_label}: 0 .. 32767 expected (int16 labels)")
    return max_label


def pp_seg_crop(seg, lo, ext, mask, max_label):
    """seg (X, Y, Z) int16, any non-negative strides; mask (ext) uint8, the filled non-zero mask of the window -> (the window of seg
    as contiguous int16 with -1 where seg == 0 and the mask is off, the label histogram of the result)."""
    shape = _pp_label_volume(seg, "seg", contiguous=False)
    lo, ext = _pp_window((1,) + shape, lo, ext)
    _expect(mask, "mask", torch.uint8, shape=ext, like=seg)
    max_label = _pp_max_label(max_label)
    out = torch.empty(ext, dtype=torch.int16, device=seg.device)
    hist = torch.empty(max_label + 3, dtype=torch.int64, device=seg.device)
    _launch("mlagg_pp_seg_crop", _ptr(seg), *shape, *(int(s) for s in seg.stride()), _int_array(lo), _int_array(ext), _ptr(mask), _ptr(out),
            max_label, _ptr(hist))
    return out, hist


def pp_seg_resize(seg, taps, out_shape, max_label):
    """seg (X, Y, Z) contiguous int16 -> (resize_segmentation(order=1) of it to out_shape, the label histogram of the result).
    taps: export._axis_taps tables (idx, w) of the three axes stacked, (sum(out_shape), 2) each."""
    shape = _pp_label_volume(seg, "seg")
    out_shape = tuple(int(s) for s in out_shape)
    if len(out_shape) != 3 or min(out_shape) < 1:
        raise RuntimeError(f"pp_seg_resize: output shape {out_shape}")
    max_label = _pp_max_label(max_label)
    d_idx, d_w = _export_taps(taps, shape, out_shape, seg.device)
    out = torch.empty(out_shape, dtype=torch.int16, device=seg.device)
    hist = torch.empty(max_label + 3, dtype=torch.int64, device=seg.device)
    _launch("mlagg_pp_seg_resize", _ptr(seg), *shape, _ptr(d_idx), _ptr(d_w), _ptr(out), *out_shape, max_label, _ptr(hist))
    return out, hist


def pp_group_table(groups, max_label, device):
    """groups: a list of label collections -> the (max_label + 2,) int64 device table of pp_rank_counts: bit g of entry l + 1 is set
    when label l (-1 .. max_label) is in groups[g]."""
    max_label = _pp_max_label(max_label)
    if not 1 <= len(groups) <= PP_MAX_GROUPS:
        raise RuntimeError(f"{len(groups)} label groups: 1 .. {PP_MAX_GROUPS} are supported")
    table = np.zeros(max_label + 2, dtype=np.uint64)
    for g, labels in enumerate(groups):
        for label in labels:
            if -1 <= int(label) <= max_label:
                table[int(label) + 1] |= np.uint64(1 << g)
    return torch.from_numpy(table.view(np.int64)).to(device)


def pp_rank_counts(seg, group_table, n_groups, max_label):
    """seg: contiguous int16 volume of any rank -> (table (rows, n_groups) int64: per group the number of its voxels before each row
    of PP_RANK_BLOCK consecutive voxels, totals (n_groups,) int64), both on the device."""
    _expect(seg, "seg", torch.int16)
    max_label, n_groups = _pp_max_label(max_label), int(n_groups)
    if seg.numel() < 1 or not 1 <= n_groups <= PP_MAX_GROUPS:
        raise RuntimeError(f"pp_rank_counts: {seg.numel()} voxels, {n_groups} groups (1 .. {PP_MAX_GROUPS})")
    _expect(group_table, "group table", torch.int64, shape=(max_label + 2,), like=seg)
    rows = int(_lib.lib().mlagg_pp_rank_rows(seg.numel()))
    table = torch.empty((rows, n_groups), dtype=torch.int64, device=seg.device)
    totals = torch.empty(n_groups, dtype=torch.int64, device=seg.device)
    _launch("mlagg_pp_rank_counts", _ptr(seg), seg.numel(), _ptr(group_table), max_label, n_groups, _ptr(table), _ptr(totals))
    return table, totals


def pp_rank_select(seg, group_table, max_label, counts, group, ranks, image=None, coords=True):
    """The voxels of C-order ranks `ranks` (int64 device tensor (n,)) among the voxels of `group` in seg (X, Y, Z) contiguous int16:
    np.argwhere(mask)[ranks].  counts = pp_rank_counts(seg, ...).  -> (coords (n, 4) int64 = (0, x, y, z) or None, values (C, n)
    fp32 = image[:, x, y, z] for an image (C, X, Y, Z) fp32 of any non-negative strides, or None)."""
    shape = _pp_label_volume(seg, "seg")
    max_label, group = _pp_max_label(max_label), int(group)
    table, totals = counts
    rows = int(_lib.lib().mlagg_pp_rank_rows(seg.numel()))
    _expect(table, "rank table", torch.int64, dim=2, like=seg)
    n_groups = int(table.shape[1])
    if table.shape[0] != rows or not 0 <= group < n_groups <= PP_MAX_GROUPS:
        raise RuntimeError(f"pp_rank_select: table {tuple(table.shape)} for {rows} rows, group {group}")
    _expect(totals, "totals", torch.int64, shape=(n_groups,), like=seg)
    _expect(group_table, "group table", torch.int64, shape=(max_label + 2,), like=seg)
    _expect(ranks, "ranks", torch.int64, dim=1, like=seg)
    n = int(ranks.shape[0])
    if n < 1 or (image is None and not coords):
        raise RuntimeError("pp_rank_select: at least one rank and one output expected")
    st, C = (0, 0, 0, 0), 0
    values = None
    if image is not None:
        ishape, st = _strided_volume(image, "image")
        if ishape[1:] != shape or image.device != seg.device:
            raise RuntimeError(f"pp_rank_select: image {ishape} does not match the segmentation {shape}")
        C = ishape[0]
        values = torch.empty((C, n), dtype=torch.float32, device=seg.device)
    out = torch.empty((n, 4), dtype=torch.int64, device=seg.device) if coords else None
    _launch("mlagg_pp_rank_select", _ptr(seg), seg.numel(), shape[1], shape[2], _ptr(group_table), max_label, n_groups, group,
            _ptr(table), _ptr(totals), _ptr(ranks), n, _ptr(out), _ptr(image), C, *st, _ptr(values))
    return out, values


# ------------------------------------------------------------------------------------------------
# K23: keep the largest connected component (csrc/components.hip).  The group table maps each label to its mask's group (0: not
# in any mask); postprocessing.py builds it.  Inference only.
# ------------------------------------------------------------------------------------------------
CC_MAX_VOXELS = 2 ** 31 - 1


def keep_largest_component(labels, group, background_label=0):
    """labels (X, Y, Z) contiguous uint8 on the device, group (256,) uint8 on the same device -> (out (X, Y, Z) uint8, stats (3, 256)
    int32 device tensor: per group the voxel count, the largest component's size and the voxels kept).  Voxels of a non-zero group
    whose 26-connected same-group component is smaller than the group's largest become background_label; ties are all kept."""
    _expect(labels, "labels", torch.uint8, dim=3, contiguous=False)
    if labels.numel() > CC_MAX_VOXELS:                # before contiguity: a huge expanded view is refused for its size
        raise RuntimeError(f"keep_largest_component: {labels.numel()} voxels, at most {CC_MAX_VOXELS} are supported")
    if min(labels.shape) < 1:
        raise RuntimeError(f"keep_largest_component: empty volume {tuple(labels.shape)}")
    _expect(labels, "labels", torch.uint8, dim=3)
    _expect(group, "group", torch.uint8, shape=(256,), like=labels)
    if not 0 <= int(background_label) <= 255:
        raise RuntimeError(f"background_label {background_label}: a uint8 label expected")
    if labels.data_ptr() % 4:
        labels = labels.clone()                       # the kernels read four labels per dword
    n = labels.numel()
    parent = torch.empty(n, dtype=torch.int32, device=labels.device)
    size = torch.empty(n, dtype=torch.int32, device=labels.device)
    stats = torch.empty((3, 256), dtype=torch.int32, device=labels.device)
    out = torch.empty_like(labels)
    _launch("mlagg_keep_largest_component", _ptr(labels), *labels.shape, _ptr(group), int(background_label), _ptr(parent), _ptr(size),
            _ptr(stats), _ptr(out))
    return out, stats


# ------------------------------------------------------------------------------------------------
# K24: normalized surface Dice (csrc/surface.hip).  surface.py lays out the crops (desc) from the statistics and builds the surfel
# area table.  Inference only.
# ------------------------------------------------------------------------------------------------
SURFACE_MAX_VOXELS = 2 ** 31 - 1
SURFACE_MAX_LINE = _C["MLAGG_SURFACE_MAX_LINE"]          # the longest crop axis (LDS envelope of one line)
SURFACE_DESC_FIELDS = _C["MLAGG_SURFACE_DESC_FIELDS"]


def surface_stats(gt, pred, wanted):
    """gt, pred (X, Y, Z) uint8 label volumes on the device, wanted (256,) uint8 on the same device -> (256, 10) int32 device tensor:
    per label value the gt and prediction voxel counts, the union box (x, y, z min / max) and the gt's z min / max."""
    _expect(gt, "gt", torch.uint8, dim=3)
    _expect(pred, "pred", torch.uint8, shape=gt.shape, like=gt)
    _expect(wanted, "wanted", torch.uint8, shape=(256,), contiguous=False, like=gt)
    stats = torch.empty((256, 10), dtype=torch.int32, device=gt.device)
    _launch("mlagg_surface_stats", _ptr(gt), _ptr(pred), *gt.shape, _ptr(wanted.contiguous()), _ptr(stats))
    return stats


def surface_prepare(gt, pred, desc, spacing):
    """Neighbour codes and the z / y passes of the feature transform for every crop of desc ((L, 16) int64 host tensor, see
    include/mlagg_hip.h).  Returns the state mlagg_surface_reduce needs: (codes, ft, counts, d_desc, layout)."""
    _expect(gt, "gt", torch.uint8, dim=3)
    _expect(pred, "pred", torch.uint8, dim=3)
    L = desc.shape[0]
    n = desc[:, 4:7].long() + 1
    vox = n.prod(1)
    layout = {"total": int(vox.sum()), "max_crop": int(vox.max()), "zlines": int((n[:, 0] * n[:, 1]).sum()),
              "ylines": int((n[:, 0] * n[:, 2]).sum()), "xlines": int((n[:, 1] * n[:, 2]).sum()),
              "nmax_y": int(n[:, 1].max()), "nmax_x": int(n[:, 0].max()), "labels": L}
    if layout["max_crop"] > SURFACE_MAX_VOXELS:
        raise RuntimeError(f"surface: a crop of {layout['max_crop']} voxels, at most {SURFACE_MAX_VOXELS} are supported")
    if int(n.max()) > SURFACE_MAX_LINE:
        raise RuntimeError(f"surface: a crop axis of {int(n.max())} voxels, at most {SURFACE_MAX_LINE} are supported")
    dev = gt.device
    d_desc = desc.to(dev)
    codes = torch.empty(2 * layout["total"], dtype=torch.uint8, device=dev)
    ft = torch.empty(2 * layout["total"], dtype=torch.int32, device=dev)
    counts = torch.empty((L, 2), dtype=torch.int32, device=dev)
    s = [float(v) for v in spacing]
    _launch("mlagg_surface_prepare", _ptr(gt), _ptr(pred), *gt.shape, _ptr(d_desc), L, layout["total"], layout["max_crop"],
            layout["zlines"], layout["ylines"], layout["nmax_y"], s[1], s[2], _ptr(codes), _ptr(ft), _ptr(counts))
    return codes, ft, counts, d_desc, layout


def surface_reduce(state, tol, area, spacing, pairs_total=None):
    """The x pass at the other mask's surfels.  tol (L,) float64 and area (256,) float64 device tensors.  Returns (sums (L, 4)
    float64 device tensor: gt area, gt area within tol, prediction area, prediction area within tol; pairs (pairs_total, 2) float64
    (distance, area) at desc's pair offsets, unsorted, or None)."""
    codes, ft, counts, d_desc, layout = state
    dev = codes.device
    L = layout["labels"]
    partial = torch.empty(4 * layout["xlines"], dtype=torch.float64, device=dev)
    sums = torch.empty((L, 4), dtype=torch.float64, device=dev)
    pairs = pair_count = None
    if pairs_total is not None:
        pairs = torch.empty((max(int(pairs_total), 1), 2), dtype=torch.float64, device=dev)
        pair_count = torch.empty((L, 2), dtype=torch.int32, device=dev)
    s = [float(v) for v in spacing]
    _launch("mlagg_surface_reduce", _ptr(codes), _ptr(ft), _ptr(d_desc), L, layout["total"], layout["xlines"], layout["nmax_x"], _ptr(tol),
            _ptr(area), s[0], s[1], s[2], _ptr(partial), _ptr(sums), _ptr(pairs), _ptr(pair_count))
    return sums, (None if pairs is None else pairs[:int(pairs_total)])


# ------------------------------------------------------------------------------------------------
# K25: 3-D spatial augmentation (augmentation3d.GpuAugmenter3D)
# ------------------------------------------------------------------------------------------------
def aug3d_resample(vol, lab, affine, resample, out_shape):
    """vol (B, C, Xi, Yi, Zi) fp32 (spline coefficients of the resampled samples, raw data of the cropped ones), lab (B, 1, Xi, Yi, Zi)
    int16 or None, affine (B, 3, 4) float64 host array (output voxel index -> input coordinate), resample (B,) host bools ->
    (out (B, C, *out_shape) fp32, out_lab (B, 1, *out_shape) fp32 or None).  vol None with lab: the labels only (a further seg
    channel of a batch whose volume is already resampled), out is None.  See include/mlagg_hip.h, K25."""
    return _aug3d_launch("aug3d_resample", 3, vol, lab, affine, resample, out_shape)


def _aug3d_launch(name, nd, vol, lab, affine, resample, out_nd):
    """K25 (nd 3) and K31 (nd 2: the map covers (Y, Z) only) take the same arguments: the checks, the outputs and the launch."""
    if vol is None:
        _expect(lab, "lab", torch.int16, dim=5)
        B, C, size_in = int(lab.shape[0]), 0, tuple(int(v) for v in lab.shape[2:])
        vol = lab                                         # shape and device of the checks below
    else:
        _expect(vol, "vol", dim=5)
        B, C, *size_in = (int(v) for v in vol.shape)
    if len(out_nd) != nd or min(int(v) for v in out_nd) < 1:
        raise RuntimeError(f"{name}: output shape {tuple(out_nd)}")
    size_out = (*size_in[:3 - nd], *(int(v) for v in out_nd))
    if lab is not None:
        _expect(lab, "lab", torch.int16, shape=(B, 1, *size_in), like=vol)
    A = np.ascontiguousarray(np.asarray(affine, dtype=np.float64).reshape(B, nd * (nd + 1)))
    rs = np.asarray(resample, dtype=bool).reshape(-1)
    if rs.shape[0] != B:
        raise RuntimeError(f"{name}: {rs.shape[0]} resample flags for {B} samples")
    if (~rs).any() and any(o > i for o, i in zip(size_out, size_in)):
        raise RuntimeError(f"{name}: a cropped sample needs an input {tuple(size_in)} at least the output {size_out}")
    out = torch.empty((B, C, *size_out), device=vol.device, dtype=torch.float32) if C else None
    out_lab = torch.empty((B, 1, *size_out), device=vol.device, dtype=torch.float32) if lab is not None else None
    _launch("mlagg_" + name, _ptr(vol) if C else None, _ptr(lab), B, C, *size_in, A.ctypes.data, _int_array(rs.astype(int)), _ptr(out),
            _ptr(out_lab), *size_out[3 - nd:])
    return out, out_lab


# ------------------------------------------------------------------------------------------------
# K31: planar ("dummy 2-D") spatial augmentation of anisotropic 3-D patches (augmentation3d.GpuAugmenter3D(dummy_2d=True))
# ------------------------------------------------------------------------------------------------
def aug3d_resample_planar(vol, lab, affine, resample, out_yz):
    """vol (B, C, X, Yi, Zi) fp32 (spline coefficients along Y and Z of the resampled samples, raw data of the cropped ones), lab
    (B, 1, X, Yi, Zi) int16 or None, affine (B, 2, 3) float64 host array (output pixel (y, z) -> input (y, z), the same for every
    slice and channel of the sample), resample (B,) host bools -> (out (B, C, X, *out_yz) fp32, out_lab (B, 1, X, *out_yz) fp32 or
    None).  vol None with lab: the labels only, out is None.  See include/mlagg_hip.h, K31."""
    return _aug3d_launch("aug3d_resample_planar", 2, vol, lab, affine, resample, out_yz)


# ------------------------------------------------------------------------------------------------
# K27: cell-instance F1 evaluation (csrc/cells.hip).  cells.py composes these per image and per tile and does the assignment on the
# host.  Inference only.
# ------------------------------------------------------------------------------------------------
CELLS_MAX_PIXELS = 2 ** 31 - 1
CELLS_MAX_THRESHOLDS = _C["MLAGG_CELLS_MAX_THRESHOLDS"]
CELLS_MAX_OVERLAP_BYTES = _C["MLAGG_CELLS_MAX_OVERLAP_BYTES"]
CELLS_MAX_FLAG_BYTES = 2 ** 30           # the presence flags of a label domain (one byte per possible label)


def cells_label(seg, foreground=1, gt=None):
    """seg (H, W) contiguous uint8 or int32 on the device, gt None or an int32 map of the same shape -> (parent (H, W) int32: the
    linear index of the first pixel in raster order of the pixel's 8-connected component of {seg == foreground}, -1 elsewhere; counts
    (3,) int32 device tensor: |gt > 0|, |seg == foreground|, |both| (without gt only the middle one))."""
    if not (isinstance(seg, torch.Tensor) and seg.dtype in (torch.uint8, torch.int32)):
        raise RuntimeError(f"seg: expected a uint8 or int32 tensor, got {getattr(seg, 'dtype', type(seg))}")
    _expect(seg, "seg", seg.dtype, dim=2, contiguous=False)
    if seg.numel() > CELLS_MAX_PIXELS:
        raise RuntimeError(f"cells_label: {seg.numel()} pixels, at most {CELLS_MAX_PIXELS} are supported")
    if min(seg.shape) < 1:
        raise RuntimeError(f"cells_label: empty image {tuple(seg.shape)}")
    _expect(seg, "seg", seg.dtype, dim=2)
    if gt is not None:
        _expect(gt, "gt", torch.int32, shape=seg.shape, like=seg)
    parent = torch.empty(seg.shape, dtype=torch.int32, device=seg.device)
    counts = torch.empty(3, dtype=torch.int32, device=seg.device)
    _launch("mlagg_cells_label", _ptr(seg), seg.element_size(), int(foreground), _ptr(gt), *seg.shape, _ptr(parent), _ptr(counts))
    return parent, counts


def cells_relabel(keys, domain, bias=0, region=None, ring=False):
    """Order-preserving compaction of a key map to 1..n.  keys (H, W) contiguous int32 on the device; key = keys + bias in
    [0, domain), 0 = background (bias 1: a parent map of cells_label).  region (r0, c0, Hr, Wr): the Hr x Wr tile at (r0, c0) of the map
    zero-padded as far as needed (default: the whole map).  ring: drop every key seen in the tile's 2-pixel ring.  Returns (out (h, w)
    int32: the part of the tile inside the map, n (1,) int32 device tensor: the number of labels kept)."""
    _expect(keys, "keys", torch.int32, dim=2)
    H, W = (int(v) for v in keys.shape)
    r0, c0, Hr, Wr = (0, 0, H, W) if region is None else (int(v) for v in region)
    h, w = min(Hr, H - r0), min(Wr, W - c0)
    if r0 < 0 or c0 < 0 or h < 1 or w < 1:
        raise RuntimeError(f"cells_relabel: the region {region} lies outside the {H} x {W} map")
    if ring and (Hr < 5 or Wr < 5):
        raise RuntimeError(f"cells_relabel: a {Hr} x {Wr} image has no interior inside its 2-pixel ring; at least 5 x 5 is supported")
    D = int(domain)
    if D < 1 or D > 2 ** 31:
        raise RuntimeError(f"cells_relabel: a label domain of {D}, 1 to 2^31 are supported")
    dev = keys.device
    flags = torch.empty(2 * D, dtype=torch.uint8, device=dev)
    newid = torch.empty(D, dtype=torch.int32, device=dev)
    blocksum = torch.empty(int(_lib.lib().mlagg_cells_scan_blocks(D)), dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    out = torch.empty((h, w), dtype=torch.int32, device=dev)
    _launch("mlagg_cells_relabel", keys.data_ptr() + 4 * (r0 * W + c0), int(bias), W, h, w, Hr, Wr, int(bool(ring)), D, _ptr(flags),
            _ptr(newid), _ptr(blocksum), _ptr(total), _ptr(out))
    return out, total


def cells_overlap(g, p, n_true, n_pred):
    """g, p (h, w) contiguous int32 label maps on the device with labels in [0, n_true] / [0, n_pred] -> (overlap (n_true + 1,
    n_pred + 1) int32 pixel counts of every label pair, area_t (n_true + 1,), area_p (n_pred + 1,): its row and column sums)."""
    _expect(g, "g", torch.int32, dim=2)
    _expect(p, "p", torch.int32, shape=g.shape, like=g)
    n_true, n_pred = int(n_true), int(n_pred)
    nbytes = 4 * (n_true + 1) * (n_pred + 1)
    if n_true < 0 or n_pred < 0 or nbytes > CELLS_MAX_OVERLAP_BYTES:
        raise RuntimeError(f"cells_overlap: a ({n_true} + 1) x ({n_pred} + 1) int32 overlap matrix takes {nbytes} bytes, at most "
                           f"{CELLS_MAX_OVERLAP_BYTES} are supported")
    overlap = torch.empty((n_true + 1, n_pred + 1), dtype=torch.int32, device=g.device)
    area_t = torch.empty(n_true + 1, dtype=torch.int32, device=g.device)
    area_p = torch.empty(n_pred + 1, dtype=torch.int32, device=g.device)
    _launch("mlagg_cells_overlap", _ptr(g), _ptr(p), *g.shape, n_true, n_pred, _ptr(overlap), _ptr(area_t), _ptr(area_p))
    return overlap, area_t, area_p


def cells_match(overlap, area_t, area_p, thresholds, want_iou=False):
    """Per threshold (at most CELLS_MAX_THRESHOLDS) the edges {iou >= th} among the pairs i, j >= 1 of cells_overlap's result.
    Returns (stats (len(thresholds), 3) int32 device tensor: edge count, largest row degree, largest column degree, the degrees 0
    where no row / column has more than one edge; iou (n_true + 1, n_pred + 1) float64 or None)."""
    _expect(overlap, "overlap", torch.int32, dim=2)
    rows, pitch = (int(v) for v in overlap.shape)
    _expect(area_t, "area_t", torch.int32, shape=(rows,), like=overlap)
    _expect(area_p, "area_p", torch.int32, shape=(pitch,), like=overlap)
    th = np.ascontiguousarray(np.asarray(list(thresholds), dtype=np.float64).reshape(-1))
    if th.shape[0] > CELLS_MAX_THRESHOLDS:
        raise RuntimeError(f"cells_match: {th.shape[0]} thresholds, at most {CELLS_MAX_THRESHOLDS} per call")
    dev = overlap.device
    iou = torch.empty((rows, pitch), dtype=torch.float64, device=dev) if want_iou else None
    degrees = torch.empty(CELLS_MAX_THRESHOLDS * (rows + pitch), dtype=torch.int32, device=dev)
    stats = torch.empty((CELLS_MAX_THRESHOLDS, 4), dtype=torch.int32, device=dev)
    _launch("mlagg_cells_match", _ptr(overlap), _ptr(area_t), _ptr(area_p), rows - 1, pitch - 1, th.ctypes.data, th.shape[0], _ptr(iou),
            _ptr(degrees), _ptr(stats), None, 0)
    return stats[:th.shape[0], :3], iou


def cells_edges(overlap, area_t, area_p, threshold, count):
    """The `count` pairs (i - 1, j - 1), i, j >= 1, with iou >= threshold as a (count, 2) int32 device tensor, in no particular order
    (count: the edge count cells_match reported for this threshold)."""
    _expect(overlap, "overlap", torch.int32, dim=2)
    rows, pitch = (int(v) for v in overlap.shape)
    count = int(count)
    if count < 1:
        raise RuntimeError(f"cells_edges: an edge count of {count}")
    th = np.asarray([threshold], dtype=np.float64)
    stats = torch.empty((CELLS_MAX_THRESHOLDS, 4), dtype=torch.int32, device=overlap.device)
    edges = torch.empty((count, 2), dtype=torch.int32, device=overlap.device)
    _launch("mlagg_cells_match", _ptr(overlap), _ptr(area_t), _ptr(area_p), rows - 1, pitch - 1, th.ctypes.data, 1, None, None,
            _ptr(stats), _ptr(edges), count)
    return edges


# ------------------------------------------------------------------------------------------------
# K28: ensembling and model selection (csrc/ensemble.hip).  ensembling.py and evaluation.py compose these.  Inference only.
# ------------------------------------------------------------------------------------------------
ENSEMBLE_MAX_CLASSES = _C["MLAGG_ENSEMBLE_MAX_CLASSES"]
CONFUSION_MAX_LABELS = _C["MLAGG_CONFUSION_MAX_LABELS"]


def ensemble_mean(members, want_mean=False, regions_class_order=None):
    """members: M >= 1 contiguous fp32 or fp16 device tensors of one shape (K, ...), 2 <= K <= ENSEMBLE_MAX_CLASSES (views into larger
    buffers are fine) -> (labels (...) uint8: the first class whose mean is the maximum, a NaN counting as one; mean (K, ...) fp32 or
    None).  The mean is ((m_0 + m_1) + ...) / M in fp32, numpy's arithmetic to the bit.  Without want_mean no (K, N) buffer exists.
    regions_class_order (K labels in 0 .. 255, K >= 1): the members are sigmoid probabilities of a region-based label manager; the
    mean is the same and the label is 0, then regions_class_order[k] wherever mean_k > 0.5, k = 0 .. K-1 in order."""
    members = list(members)
    if not members:
        raise RuntimeError("ensemble_mean: at least one member must be given")
    first = members[0]
    for i, m in enumerate(members):
        if not (isinstance(m, torch.Tensor) and m.dtype in (torch.float32, torch.float16)):
            raise RuntimeError(f"members[{i}]: expected an fp32 or fp16 tensor, got {getattr(m, 'dtype', type(m))}")
        _expect(m, f"members[{i}]", m.dtype, like=first)
        if m.dim() < 2 or tuple(m.shape) != tuple(first.shape):
            raise RuntimeError(f"members[{i}]: shape {tuple(m.shape)}, expected (K, ...) = {tuple(first.shape)} as members[0]")
    K = int(first.shape[0])
    N = first.numel() // max(K, 1)
    order = None
    if regions_class_order is not None:
        order = [int(v) for v in regions_class_order]
        if len(order) != K or any(not 0 <= v <= 255 for v in order):
            raise RuntimeError(f"ensemble_mean: regions_class_order {order} for {K} heads (one uint8 label per head)")
    if K < (2 if order is None else 1) or K > ENSEMBLE_MAX_CLASSES:
        raise RuntimeError(f"ensemble_mean: {K} classes, {2 if order is None else 1} to {ENSEMBLE_MAX_CLASSES} are supported "
                           "(labels are uint8)")
    if N < 1:
        raise RuntimeError(f"ensemble_mean: empty members {tuple(first.shape)}")
    rows = [v for m in members for v in (m.data_ptr(), m.element_size())]
    table = torch.tensor(rows + (order or []), dtype=torch.int64).to(first.device)
    labels = torch.empty(first.shape[1:], dtype=torch.uint8, device=first.device)
    mean = torch.empty(first.shape, dtype=torch.float32, device=first.device) if want_mean else None
    _launch("mlagg_ensemble_mean" if order is None else "mlagg_ensemble_mean_regions", _ptr(table), len(members), K, N, _ptr(labels),
            _ptr(mean))
    return labels, mean


def label_confusion(reference, prediction, table, n_labels, ignore_label=None):
    """reference, prediction: contiguous uint8 device tensors of one shape; table: 256 uint8 on the device, label value -> bin 0 ..
    n_labels (n_labels = "any other value", at most CONFUSION_MAX_LABELS) -> (n_labels + 1, n_labels + 1) int64 device tensor of voxel
    counts, row = reference bin, column = prediction bin.  Voxels whose reference value is ignore_label are left out."""
    _expect(reference, "reference", torch.uint8)
    _expect(prediction, "prediction", torch.uint8, shape=reference.shape, like=reference)
    _expect(table, "table", torch.uint8, shape=(256,), like=reference)
    L = int(n_labels)
    if L < 0 or L > CONFUSION_MAX_LABELS:
        raise RuntimeError(f"label_confusion: {L} labels, at most {CONFUSION_MAX_LABELS} are supported")
    if reference.numel() < 1:
        raise RuntimeError(f"label_confusion: empty volume {tuple(reference.shape)}")
    ignore = -1 if ignore_label is None or not 0 <= int(ignore_label) <= 255 else int(ignore_label)
    counts = torch.empty((L + 1, L + 1), dtype=torch.int64, device=reference.device)
    _launch("mlagg_label_confusion", _ptr(reference), _ptr(prediction), reference.numel(), _ptr(table), L, ignore, _ptr(counts))
    return counts


# ------------------------------------------------------------------------------------------------
# K30: the cascade training transforms on bit planes (csrc/cascade_aug.hip; augmentation3d.cascade_transforms composes them).
# A plane is (X, Y, W) int64 words, W = ceil(Z / 64): bit k of word w is voxel z = 64 w + k; the padding bits are 0.
# ------------------------------------------------------------------------------------------------
CASCADE_MAX_LABELS = _C["MLAGG_CASCADE_MAX_LABELS"]
CASCADE_MAX_REACH = _C["MLAGG_CASCADE_MAX_REACH"]
CASCADE_MAX_VOXELS = 2 ** 31 - 1
CASCADE_DILATION, CASCADE_EROSION = 0, 1


def cascade_words(Z):
    return (int(Z) + 63) // 64


def _cascade_planes(planes, name, Z, dim):
    _expect(planes, name, torch.int64, dim=dim)
    X, Y, W = (int(v) for v in planes.shape[-3:])
    if min(planes.shape) < 1 or W != cascade_words(Z):
        raise RuntimeError(f"{name}: planes {tuple(planes.shape)} for Z = {Z}: {cascade_words(Z)} words per row expected")
    if X * Y * int(Z) > CASCADE_MAX_VOXELS:
        raise RuntimeError(f"{name}: {X * Y * int(Z)} voxels per plane, at most {CASCADE_MAX_VOXELS} are supported")
    return X, Y, int(Z)


def cascade_pack(seg, labels, out=None):
    """seg (B, X, Y, Z) int16 or fp32 label maps on the device, each sample contiguous (the channel slice seg5[:, 1] of a contiguous
    (B, 2, X, Y, Z) batch is accepted as it is); labels: L ints -> planes (B, L, X, Y, W) int64, plane i = (seg == labels[i])
    (written into `out` when given)."""
    if not (isinstance(seg, torch.Tensor) and seg.is_cuda and seg.dtype in (torch.int16, torch.float32) and seg.dim() == 4):
        raise RuntimeError(f"seg: expected a (B, X, Y, Z) int16 or float32 tensor on the MI355X device, got "
                           f"{getattr(seg, 'dtype', type(seg))} {tuple(getattr(seg, 'shape', ()))} on {getattr(seg, 'device', '?')}")
    labels = [int(v) for v in labels]
    B, X, Y, Z = (int(v) for v in seg.shape)
    if min(B, X, Y, Z) < 1 or X * Y * Z > CASCADE_MAX_VOXELS:
        raise RuntimeError(f"cascade_pack: label maps {tuple(seg.shape)}: 1 to {CASCADE_MAX_VOXELS} voxels per sample are supported")
    if not 1 <= len(labels) <= CASCADE_MAX_LABELS:
        raise RuntimeError(f"cascade_pack: {len(labels)} labels, 1 to {CASCADE_MAX_LABELS} are supported")
    if not seg[0].is_contiguous() or (B > 1 and seg.stride(0) < X * Y * Z):
        seg = seg.contiguous()
    shape = (B, len(labels), X, Y, cascade_words(Z))
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=seg.device)
    _expect(out, "out", torch.int64, shape=shape, like=seg)
    _launch("mlagg_cascade_pack", _ptr(seg), seg.element_size(), seg.stride(0) if B > 1 else X * Y * Z, B, X, Y, Z, _int_array(labels),
            len(labels), _ptr(out))
    return out


def cascade_unpack(planes, Z, out, c0):
    """planes (B, L, X, Y, W) -> out[:, c0:c0 + L] of the contiguous fp32 network input out (B, C, X, Y, Z), as 0 / 1."""
    X, Y, Z = _cascade_planes(planes, "planes", Z, 5)
    B, L = int(planes.shape[0]), int(planes.shape[1])
    _expect(out, "out", dim=5, like=planes)
    C, c0 = int(out.shape[1]), int(c0)
    if tuple(out.shape) != (B, C, X, Y, Z) or c0 < 0 or c0 + L > C:
        raise RuntimeError(f"cascade_unpack: out {tuple(out.shape)} does not take {L} planes of ({X}, {Y}, {Z}) at channel {c0}")
    _launch("mlagg_cascade_unpack", _ptr(planes), B, L, X, Y, Z, _ptr(out), C, c0)
    return out


def cascade_footprint_runs(footprint, operation):
    """The run table of one footprint S (boolean, (n0, n1, n2), each n <= 2 MAX_REACH + 1, centre n // 2) for a dilation
    (offsets -(i - c)) or an erosion (offsets i - c): a list of (dx, dy, lo, len), one per run of set offsets along z."""
    S = np.asarray(footprint).astype(bool)
    if S.ndim != 3 or min(S.shape) < 1 or max(S.shape) > 2 * CASCADE_MAX_REACH + 1:
        raise RuntimeError(f"footprint of shape {S.shape}: three axes of 1 to {2 * CASCADE_MAX_REACH + 1} entries are supported")
    if operation not in (CASCADE_DILATION, CASCADE_EROSION):
        raise RuntimeError(f"operation {operation!r}: CASCADE_DILATION or CASCADE_EROSION")
    c = [n // 2 for n in S.shape]
    edge = np.diff(np.pad(S, ((0, 0), (0, 0), (1, 1))).astype(np.int8), axis=2)       # +1 where a run starts, -1 one past its end
    i0, i1, start = np.nonzero(edge == 1)
    end = np.nonzero(edge == -1)[2]                                                   # the same row-major order: run for run
    if operation == CASCADE_EROSION:
        table = np.stack([i0 - c[0], i1 - c[1], start - c[2], end - start], 1)
    else:                                                                             # the reflected footprint
        table = np.stack([c[0] - i0, c[1] - i1, c[2] - (end - 1), end - start], 1)
    return [tuple(row) for row in table.tolist()]


def _cascade_jobs(jobs, width, what):
    rows = [[int(v) for v in j] for j in jobs]
    if not rows or any(len(r) != width for r in rows):
        raise RuntimeError(f"{what}: a non-empty list of {width}-tuples expected")
    return _int_array([v for r in rows for v in r]), len(rows)


def cascade_morph(pool, Z, jobs, runs):
    """pool (P, X, Y, W) planes; runs (R, 4) int32 device table of cascade_footprint_runs rows; jobs: (source plane, destination
    plane, first run, number of runs, operation) each, all run in one launch.  See include/mlagg_hip.h, K30."""
    X, Y, Z = _cascade_planes(pool, "pool", Z, 4)
    _expect(runs, "runs", torch.int32, dim=2, like=pool)
    if runs.shape[1] != 4 or runs.shape[0] < 1:
        raise RuntimeError(f"runs: expected (R, 4) with R >= 1, got {tuple(runs.shape)}")
    arr, n = _cascade_jobs(jobs, 5, "cascade_morph")
    _launch("mlagg_cascade_morph", _ptr(pool), int(pool.shape[0]), X, Y, Z, _ptr(runs), int(runs.shape[0]), arr, n)


def cascade_commit(pool, Z, n_labels, jobs):
    """The "was added" rule: jobs (result plane, target plane, first plane of the target's sample), one per sample: the target takes
    the result, and what the result adds to it is cleared in the sample's other n_labels - 1 planes."""
    X, Y, Z = _cascade_planes(pool, "pool", Z, 4)
    arr, n = _cascade_jobs(jobs, 3, "cascade_commit")
    _launch("mlagg_cascade_commit", _ptr(pool), int(pool.shape[0]), X, Y, Z, int(n_labels), arr, n)


def cascade_cc_stats(planes, Z, thresh, workspace=None):
    """planes (P, X, Y, W) -> (state for cascade_cc_remove, table (P, 2) int32 device tensor: plane non-empty, number of 26-connected
    components with size < thresh).  The state holds two int32 per voxel and plane (parent, size); `workspace`: an earlier call's
    state whose buffers are taken over when they are large enough (that state is then void)."""
    X, Y, Z = _cascade_planes(planes, "planes", Z, 4)
    P, n, dev = int(planes.shape[0]), X * Y * Z, planes.device
    if P > 65535:
        raise RuntimeError(f"cascade_cc_stats: {P} planes, at most 65535 are supported")
    n_blocks = int(_lib.lib().mlagg_cascade_cc_blocks(X, Y, Z))
    if workspace is not None and workspace[0].device == dev and workspace[0].numel() >= P * n and workspace[2].numel() >= P * n_blocks:
        parent, size = workspace[0].view(-1)[:P * n].view(P, n), workspace[1].view(-1)[:P * n].view(P, n)
        blockcnt = workspace[2].view(-1)[:P * n_blocks].view(P, n_blocks)
    else:
        parent = torch.empty((P, n), dtype=torch.int32, device=dev)
        size = torch.empty((P, n), dtype=torch.int32, device=dev)
        blockcnt = torch.empty((P, n_blocks), dtype=torch.int32, device=dev)
    table = torch.empty((P, 2), dtype=torch.int32, device=dev)
    _launch("mlagg_cascade_cc_stats", _ptr(planes), P, X, Y, Z, float(thresh), _ptr(parent), _ptr(size), _ptr(blockcnt), _ptr(table))
    return (parent, size, blockcnt, float(thresh)), table


def cascade_cc_remove(planes, Z, state, rank, fill=None):
    """Clears, in plane p, the rank[p]-th component with size < thresh in root order (rank[p] < 0: nothing); fill[p] != 0 sets the
    same voxels in plane p + fill[p] (which may lie outside `planes`, in the tensor it is a view of).  rank, fill: P ints (host)."""
    X, Y, Z = _cascade_planes(planes, "planes", Z, 4)
    parent, size, blockcnt, thresh = state
    P = int(planes.shape[0])
    rank = [int(v) for v in rank]
    fill = [0] * P if fill is None else [int(v) for v in fill]
    if len(rank) != P or len(fill) != P or tuple(parent.shape) != (P, X * Y * Z):
        raise RuntimeError(f"cascade_cc_remove: {len(rank)} ranks, {len(fill)} fills and a state of {tuple(parent.shape)} for {P} planes")
    words, have = X * Y * cascade_words(Z), planes.untyped_storage().nbytes() // 8
    for p, f in enumerate(fill):                      # the plane to fill lies in the tensor `planes` is a view of
        if f and not 0 <= planes.storage_offset() + (p + f) * words <= have - words:
            raise RuntimeError(f"cascade_cc_remove: fill[{p}] = {f} points outside the planes' tensor")
    args = torch.tensor([rank, fill], dtype=torch.int32).to(planes.device)
    target = torch.empty(P, dtype=torch.int32, device=planes.device)
    _launch("mlagg_cascade_cc_remove", _ptr(planes), P, X, Y, Z, thresh, _ptr(parent), _ptr(size), _ptr(blockcnt), _ptr(args[0]),
            _ptr(args[1]), _ptr(target))


# ------------------------------------------------------------------------------------------------
# K36: the tail of the training transform chain (mask, -1 -> 0, region planes, deep-supervision levels) in one launch
# ------------------------------------------------------------------------------------------------
TAIL_MAX_LEVELS = _C["MLAGG_TAIL_MAX_LEVELS"]
TAIL_MAX_REGIONS = _C["MLAGG_TAIL_MAX_REGIONS"]
_TAIL_SEG_KIND = {torch.float32: _C["MLAGG_TAIL_SEG_F32"], torch.int16: _C["MLAGG_TAIL_SEG_INT16"]}
_TAIL_TABLES = {}


def _tail_table(n, m, device):
    """dataloading.nearest_index(n, m) on `device` (uploaded once per (n, m, device)); None for n == m, where it is the identity."""
    if n == m:
        return None
    key = (n, m, str(device))
    if key not in _TAIL_TABLES:
        from .dataloading import nearest_index
        _TAIL_TABLES[key] = nearest_index(n, m).to(device)
    return _TAIL_TABLES[key]


def batch_tail(data, seg, level_sizes, mask_channels=(), regions=None, ignore_label=None, tables=None):
    """K36: from the augmented batch to what the loss consumes, the reference's MaskTransform, RemoveLabelTransform(-1, 0),
    ConvertSegmentationToRegionsTransform and DownsampleSegForDSTransform2 (nnUNetTrainer.py:697-731) in one launch.
    data (B, C, *S) fp32, contiguous, MODIFIED IN PLACE: zero in the channels `mask_channels` wherever seg[:, 0] < 0.
    seg (B, Sc, *S) fp32 or int16, contiguous; channel 0 is read.  level_sizes: 1 to 8 spatial shapes (dataloading.level_sizes).
    Returns (data, [target_l]): target_l (B, 1, *S_l) fp32 labels with negatives as 0, each voxel that of the source voxel
    ``interpolate(mode="nearest-exact")`` picks (dataloading.nearest_index) -- `dataloading.targets_from_seg` to the bit -- or, with
    `regions` (a label manager's ``foreground_regions``), (B, R (+ 1), *S_l) 0 / 1 planes, the last one `ignore_label`'s when given:
    the layout K29 takes with member=None.  `tables` (tests, other index rules): per level and axis an int32 tensor of source
    indices on the tensors' device, or None for the identity, instead of the nearest-exact ones.
    CPU tensors take the same steps as a torch composition (dataloading.batch_tail_host); device tensors have no other path than K36."""
    from . import dataloading
    if not (isinstance(data, torch.Tensor) and isinstance(seg, torch.Tensor) and data.dtype == torch.float32
            and seg.dtype in _TAIL_SEG_KIND and data.device == seg.device and data.dim() in (4, 5) and seg.dim() == data.dim()):
        raise RuntimeError(f"batch_tail: data (B, C, *S) float32 and seg (B, Sc, *S) float32 or int16 on one device, 2-D or 3-D, got "
                           f"{getattr(data, 'dtype', type(data))} {tuple(getattr(data, 'shape', ()))} on {getattr(data, 'device', '?')}"
                           f" and {getattr(seg, 'dtype', type(seg))} {tuple(getattr(seg, 'shape', ()))} on {getattr(seg, 'device', '?')}")
    if not (data.is_contiguous() and seg.is_contiguous()):
        raise RuntimeError("batch_tail: data and seg must be contiguous (data is written in place)")
    nd, S = data.dim() - 2, tuple(int(v) for v in data.shape[2:])
    B, C, Sc = int(data.shape[0]), int(data.shape[1]), int(seg.shape[1])
    if tuple(seg.shape[2:]) != S or seg.shape[0] != B or min((B, C, Sc) + S) < 1:
        raise RuntimeError(f"batch_tail: data {tuple(data.shape)} and seg {tuple(seg.shape)} do not describe one non-empty batch")
    sizes = [tuple(int(v) for v in s) for s in level_sizes]
    if not 1 <= len(sizes) <= TAIL_MAX_LEVELS or any(len(s) != nd or min(s) < 1 for s in sizes):
        raise RuntimeError(f"batch_tail: level sizes {sizes}: 1 to {TAIL_MAX_LEVELS} non-empty {nd}-D shapes")
    mask = sorted({int(c) for c in mask_channels})
    if mask and not (0 <= mask[0] and mask[-1] < min(C, 64)):
        raise RuntimeError(f"batch_tail: mask_channels {mask} of {C} data channels (indices 0 to {min(C, 64) - 1})")
    if ignore_label is not None and int(ignore_label) < 0:
        raise RuntimeError(f"batch_tail: ignore_label {ignore_label}: None or a label value >= 0")
    member = n_regions = None
    if regions is not None:
        member, n_regions = region_member_table(regions, data.device), len(regions)      # refuses 0 or more than 32 regions
    if tables is None:
        tables = [[_tail_table(n, m, data.device) for n, m in zip(S, s)] for s in sizes]
    else:
        tables = [list(t) for t in tables]
        if len(tables) != len(sizes) or any(len(t) != nd for t in tables):
            raise RuntimeError(f"batch_tail: tables for {len(tables)} levels, {len(sizes)} levels of {nd} axes expected")
    for lvl, (tabs, s) in enumerate(zip(tables, sizes)):
        for axis, (tab, m) in enumerate(zip(tabs, s)):
            if tab is None:
                if m != S[axis]:
                    raise RuntimeError(f"batch_tail: level {lvl} axis {axis}: no table (the identity) for {S[axis]} -> {m} voxels")
            elif not (isinstance(tab, torch.Tensor) and tab.dtype == torch.int32 and tab.dim() == 1 and tab.is_contiguous()
                      and tab.device == data.device and tab.numel() == m):
                raise RuntimeError(f"batch_tail: level {lvl} axis {axis}: the table is {m} contiguous int32 source indices on "
                                   f"{data.device}, got {getattr(tab, 'dtype', type(tab))} {tuple(getattr(tab, 'shape', ()))}")
    if mask and any(t is not None for t in tables[0]):
        raise RuntimeError(f"batch_tail: a mask needs the first level to be the map itself, got {sizes[0]} for {S}")
    if not data.is_cuda:
        return dataloading.batch_tail_host(data, seg, sizes, mask, member, n_regions, ignore_label, tables)
    planes = 1 if member is None else n_regions + (ignore_label is not None)
    out = [torch.empty((B, planes) + s, dtype=torch.float32, device=data.device) for s in sizes]
    pointers = lambda ts: (ctypes.c_void_p * len(ts))(*[_ptr(t) for t in ts])      # noqa: E731
    with torch.cuda.device(data.device):
        _launch("mlagg_batch_tail", _ptr(data), B, C, _ptr(seg), _TAIL_SEG_KIND[seg.dtype], Sc, nd, _int_array(S), _int_array(mask),
                len(mask), len(sizes), _int_array([v for s in sizes for v in s]), pointers([t for tabs in tables for t in tabs]),
                pointers(out), _ptr(member), n_regions or 0, -1 if ignore_label is None else int(ignore_label))
    return data, out
