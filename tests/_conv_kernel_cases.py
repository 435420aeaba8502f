"""Cases, references and path predicates for the matrix-core convolutions -- K18 (csrc/conv1x1.hip) and K19 (csrc/conv3x3.hip) -- at
the sizes where their launchers change tile, form or slab geometry: shared by tests/test_conv_kernel_paths_cpu.py and
tests/test_conv_kernel_paths_gpu.py.

A CASE is a ConvCase (id, family, B, I, O, dims, form, sliced, backward).  `family` names the product the case is about (k19_fwd: the
forward / data-gradient kernel, k19_wgrad: the weight gradient, k18: all three of the 1 x 1 convolution); `form` is the operand form
(3 = fp32 operands as three bf16 pieces, 1 = bf16, 2 = fp16: MLAGG_DTYPE_*); `sliced` is "none", "x" (the input is the channel block
[8, 8 + I) of a wider map) or "dy" (the output gradient is the channel block [8, 8 + O) of a wider gradient); `backward` False: the
forward only.  Inputs come from a generator seeded with the case's shape: unit-variance x and dy, weights scaled by (k k I) ** -0.5.

`reference(case)` is the convolution and its two gradients in float64 on the host -- of the float64 copies in form 3, of the operands
rounded to the 16-bit type in forms 1 and 2 (the exact products of what the kernels multiply; they sum in fp32).  `yardstick(case)`
is the same operation in plain fp32 on the host (on the rounded operands held in fp32 in forms 1 and 2): it shows how well conditioned
a case is, it is not the truth.  `bounds(case)` are the bounds of tests/test_conv_wgrad_gpu.py for these kernels (the error of an fp32
convolution), as max |got - ref| over max |ref|:
    form 3:        y, dx 2e-6; dW 4e-6 (3-D: 1e-5)
    forms 1 and 2: 4e-6 against the exact products of the rounded operands

PATH PREDICATES are pure functions restating a launcher's decision; each names the source function it mirrors, and the CPU test
compares them with the library's host queries (mlagg_conv3x3_fwd_tile, mlagg_conv3x3_wgrad_form, mlagg_conv1x1_fwd_tile,
mlagg_conv1x1_wgrad_tile, the workspace sizes) over the cases and a sweep.  They describe the DEFAULT dispatch: OVERRIDES lists the
environment variables that change it.

Plain-fp32 yardstick errors of the compared quantities, largest over the group's cases, measured on the host (see `yardstick` for
the weight gradient's dependence on the host's thread count):

    cases                       y        dx       dW
    k19_fwd   form 3            5.9e-07  3.3e-07  1.3e-06
    k19_fwd   forms 1, 2        4.7e-07  3.0e-07  8.6e-07
    k19_fwd   3-D               5.2e-07  2.9e-07  3.8e-07
    k19_wgrad form 3            4.7e-07  3.8e-07  1.1e-06
    k19_wgrad forms 1, 2        4.9e-07  4.2e-07  1.2e-06
    k18       form 3            3.6e-07  3.9e-07  7.0e-07
    k18       forms 1, 2        3.8e-07  3.3e-07  6.4e-07
"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

ConvCase = collections.namedtuple("ConvCase", "id family B I O dims form sliced backward")
FORM_TYPE = {3: torch.float32, 1: torch.bfloat16, 2: torch.float16}
FORMS = (3, 1, 2)
OVERRIDES = ("MLAGG_K19_TILE", "MLAGG_K18_TILE", "MLAGG_K19W16", "MLAGG_K19W16_WAVES", "MLAGG_K18_WAVES", "MLAGG_K19_WGRAD_MIN_CH")
SLICE_AT, SLICE_EXTRA = 8, 16                        # a sliced operand: channels [8, 8 + C) of a map 16 channels wider


def pixels(dims):
    n = 1
    for v in dims:
        n *= v
    return n


def kernel_size(case):
    return 1 if case.family == "k18" else 3


# =====================================================================================================================
# path predicates
# =====================================================================================================================
# ---- K19 forward / data gradient (csrc/conv3x3.hip fwd_tile) ---------------------------------------------------------------
K19_TO3_MIN_P, K19_TP2_MIN_P = 16384, 65536


def k19_fwd_tile(O, P, W):
    """(to, tp) of conv3x3_kernel: (32 to) output channels x (32 tp) pixels per wave.  The data gradient asks with the layer's I."""
    to, tp = (1 if O <= 32 else 2), 2
    if O % 96 == 0 and P >= K19_TO3_MIN_P:
        to, tp = 3, (2 if P >= K19_TP2_MIN_P else 1)
    if W % tp:
        tp = 1                                       # a lane's pixel run stays inside one image row
    return to, tp


def k19_fwd_grid(O, P, tile):
    """(workgroups along the pixels, along the channels; pixels of the last workgroup, of the last wave with any; live rows of the
    last channel group): conv3x3.hip launch() -- 4 waves of 32 tp pixels per workgroup."""
    to, tp = tile
    per_wave, per_wg = 32 * tp, 4 * 32 * tp
    return (-(-P // per_wg), -(-O // (32 * to)), P - (-(-P // per_wg) - 1) * per_wg, P - (-(-P // per_wave) - 1) * per_wave,
            O - (-(-O // (32 * to)) - 1) * 32 * to)


# ---- K19 weight gradient (csrc/conv3x3.hip w16_tiles, wgrad_form, make_w16geom) -----------------------------------------------
K19W_WAVES, K19W_MIN_SLAB = 2048, 256
W16Geometry = collections.namedtuple("W16Geometry", "ti slab nslabs nbs last_pixels last_blocks q32 r32 og ig")


def k19_wgrad_form(O, I, D, form):
    """(kernel form, ti): 0 = 32 x 32 tiles with nine taps per wave (volumes), 1 = 16-wide tiles with fragment loads (fp32 operands),
    2 = 16-wide tiles with LDS-staged loads (the 16-bit operand forms); ti = 1 up to 16 input channels, else 3 (0 in form 0)."""
    if D != 1:
        return 0, 0
    return (1 if form == 3 else 2), (1 if I <= 16 else 3)


def k19_wgrad_geometry(B, O, I, H, W):
    """make_w16geom: slabs of at least 256 pixels (a multiple of 32) so that B x slabs x 3 kernel rows x channel tiles reach 2048
    waves; nbs = B * nslabs; the last slab's pixels and 32-pixel blocks; 32 = q32 * W + r32 (the per-block step of a lane's run)."""
    P, ti = H * W, (1 if I <= 16 else 3)
    og, ig = -(-O // 48), -(-I // (16 * ti))
    per_sample = -(-K19W_WAVES // (B * og * ig * 3))
    per_sample = max(1, min(per_sample, (256 << 20) // (4 * 9 * O * I) // B))
    slab = max(K19W_MIN_SLAB, -(-(-(-P // per_sample)) // 32) * 32)
    nslabs = -(-P // slab)
    last = P - (nslabs - 1) * slab
    return W16Geometry(ti, slab, nslabs, B * nslabs, last, -(-last // 32), 32 // W, 32 % W, og, ig)


def k19_wgrad_wraps(W, slab):
    """Does the `x0 >= W` wrap of a lane's run position happen inside a slab?  (r32 = 0: never -- W divides 32.)"""
    return 32 % W != 0 and slab > 32


# ---- K18 (csrc/conv1x1.hip fwd_tile, wgrad_tile, make_wgeom) ---------------------------------------------------------------------
K18_WAVES, K18_MIN_SLAB = 1536, 64
W1Geometry = collections.namedtuple("W1Geometry", "slab nslabs last_pixels")


def k18_fwd_tile(O):
    """(to, tp) of conv1x1_fwd_kernel.  The data gradient asks with the layer's I."""
    return (1, 3) if O <= 32 else ((2, 3) if O <= 64 else (3, 2))


def k18_wgrad_tile(O, I):
    return (3 if O > 64 else -(-O // 32)), (3 if I > 64 else -(-I // 32))


def k18_wgrad_geometry(B, O, I, P):
    """make_wgeom: slabs of at least 64 pixels (a multiple of 16) so that B x slabs x 96-channel groups reach 1536 waves."""
    per_sample = max(1, -(-K18_WAVES // (B * -(-O // 96) * -(-I // 96))))
    slab = max(K18_MIN_SLAB, -(-(-(-P // per_sample)) // 16) * 16)
    nslabs = -(-P // slab)
    return W1Geometry(slab, nslabs, P - (nslabs - 1) * slab)


# ---- which products the kernels take (mlagg_conv3x3_supported, mlagg_conv3x3_wgrad_supported, mlagg_conv1x1_supported) ----------
def on_kernel(case):
    """{"y" | "dx" | "dW": does the kernel family take the product}: the plan the device test passes, and what it compares."""
    P, W = pixels(case.dims), case.dims[-1]
    if case.family == "k18":
        ok = P >= 96 and P % 16 == 0                                   # a ragged contraction runs on zero-padded weight columns
        return dict(y=ok, dx=ok, dW=ok)
    return dict(y=case.I % 16 == 0 and P >= 96, dx=case.O % 16 == 0 and P >= 96, dW=W >= 8 and W % 8 == 0 and P % 16 == 0)


def compared(case):
    """The quantities the device test compares at kernel tolerance."""
    on = on_kernel(case)
    return [q for q in (("y", "dx", "dW") if case.backward else ("y",)) if on[q]]


# =====================================================================================================================
# cases
# =====================================================================================================================
def _case(id, family, B, I, O, dims, form=3, sliced="none", backward=True):
    return ConvCase(id, family, B, I, O, tuple(dims), form, sliced, backward)


K19_FWD_CASES = [
    _case("F1", "k19_fwd", 1, 16, 96, (128, 128)),                     # P = 16384: forward (3,1); data gradient (1,2)
    _case("F2", "k19_fwd", 1, 16, 96, (126, 130)),                     # P = 16380, below the threshold: (2,2)
    _case("F3", "k19_fwd", 1, 16, 96, (127, 129)),                     # P = 16383, odd width: (2,1); data gradient (1,1)
    _case("F4", "k19_fwd", 2, 16, 192, (131, 126)),                    # (3,1), two 96-row groups, partial last workgroup and wave
    _case("F5", "k19_fwd", 1, 16, 96, (256, 256)),                     # P = 65536: (3,2); the one backward at this size
    _case("F6", "k19_fwd", 1, 16, 96, (258, 254), backward=False),     # P = 65532: (3,1), just below
    _case("F7", "k19_fwd", 1, 16, 96, (254, 262), backward=False),     # P = 66548: (3,2), partial last workgroup and wave
    _case("F8", "k19_fwd", 1, 16, 96, (257, 257), backward=False),     # odd width at P >= 65536: (3,1)
    _case("F9-bf16", "k19_fwd", 1, 16, 96, (128, 128), 1, "x"),        # the 96-row tile with one product
    _case("F9-fp16", "k19_fwd", 1, 16, 96, (128, 128), 2, "x"),
    _case("F10-32", "k19_fwd", 2, 16, 32, (10, 12)),                   # (1,2) ...
    _case("F10-33", "k19_fwd", 2, 16, 33, (10, 12)),                   # ... (2,2): the O = 32 / 33 step
    _case("F11", "k19_fwd", 1, 16, 97, (12, 12)),                      # to = 2, a second row group with one live row
    _case("F12", "k19_fwd", 1, 16, 48, (97, 1)),                       # one-pixel rows, no neighbours
    _case("F13", "k19_fwd", 1, 16, 48, (49, 2)),                       # a run is the whole row
    _case("F14", "k19_fwd", 1, 16, 48, (1, 96)),                       # only the middle kernel row is inside
    _case("F15", "k19_fwd", 1, 16, 48, (8, 12)),                       # P = 96, the floor
    _case("F16", "k19_fwd", 1, 16, 96, (16, 32, 32)),                  # 3-D: nine kernel rows with (3,1)
]

K19_WGRAD_SHAPES = [
    ("W1", 2, 48, 48, (32, 56), "none"),        # slab 256, 7 slabs, nbs 14; 256 % 56 = 32: slabs end in mid-row; r32 = 32 wraps
    ("W2", 1, 48, 48, (10, 40), "none"),        # last slab 144 pixels: 5 blocks (odd: peeled), 16-pixel tail
    ("W3", 3, 16, 48, (16, 24), "none"),        # ti = 1, q32 = 1, r32 = 8, nbs 6
    ("W4", 2, 48, 49, (12, 8), "none"),         # W = 8 (q32 = 4), a second output group with one live row, 3 blocks
    ("W5", 1, 20, 33, (34, 8), "none"),         # ragged I and O inside one tile; last slab: one block with 16 live pixels
    ("W6", 2, 96, 192, (140, 88), "none"),      # slab 288 above the floor, 43 slabs, nbs 86; og 4, ig 2; last slab 7 blocks
    ("W7", 1, 48, 48, (6, 24), "none"),         # one slab, 5 blocks, 16-pixel tail
    ("W8", 2, 1, 48, (32, 40), "none"),         # the stem's one input channel, ti = 1, nbs 10
    ("W9", 1, 64, 48, (1, 256), "none"),        # one image row: kernel rows 0 and 2 are exactly 0; ig 2, ragged second group
    ("W10", 1, 48, 48, (2, 136), "none"),       # W > 128; last slab one block
    ("W11-x", 2, 48, 48, (32, 56), "x"),        # W1 with x_batch > I * P ...
    ("W11-dy", 2, 48, 48, (32, 56), "dy"),      # ... and with dy_batch > O * P
    ("W12", 2, 48, 48, (64, 32), "none"),       # nbs 16: two full rounds of the eight XCD slots; W divides 32 (no wrap)
]
K19_WGRAD_CASES = [_case(f"{n}-f{form}", "k19_wgrad", B, I, O, d, form, s) for n, B, I, O, d, s in K19_WGRAD_SHAPES for form in FORMS]

K18_SHAPES = [
    ("C1", 2, 32, 16, (11, 16), "none"),        # weight gradient (1,1); P = 176: slab 64, last slab 48; forward (1,3), clamped last wave
    ("C2", 2, 64, 32, (11, 16), "none"),        # weight gradient (1,2); data gradient (2,3)
    ("C3", 1, 96, 40, (13, 16), "none"),        # weight gradient (2,3); ragged contraction 40 in the data gradient
    ("C4", 2, 16, 80, (9, 16), "none"),         # weight gradient (3,1); forward (3,2)
    ("C5-64", 1, 48, 64, (10, 16), "none"),     # the O = 64 / 65 step, forward and weight gradient: (2,3) and (2,2) ...
    ("C5-65", 1, 48, 65, (10, 16), "none"),     # ... (3,2) and (3,2)
    ("C6", 4, 192, 192, (64, 128), "none"),     # weight gradient (3,3); slab 96 above the floor, 86 slabs per sample, last slab 32
    ("C7", 1, 48, 96, (8, 12), "none"),         # P = 96, the floor
    ("C8", 1, 96, 40, (13, 16), "x"),           # C3 with a channel-slice input
    ("C9", 1, 96, 32, (8, 16), "none"),         # weight gradient (1,3)
    ("C10", 1, 32, 48, (8, 16), "none"),        # weight gradient (2,1)
    ("C11-32", 1, 48, 32, (10, 16), "none"),    # the O = 32 / 33 step, forward and weight gradient: (1,3) and (1,2) ...
    ("C11-33", 1, 48, 33, (10, 16), "none"),    # ... (2,3) and (2,2); ragged contraction 33 in the data gradient
]
K18_CASES = [_case(f"{n}-f{form}", "k18", B, I, O, d, form, s) for n, B, I, O, d, s in K18_SHAPES for form in FORMS]

CASES = {"k19_fwd": K19_FWD_CASES, "k19_wgrad": K19_WGRAD_CASES, "k18": K18_CASES}
ALL_CASES = K19_FWD_CASES + K19_WGRAD_CASES + K18_CASES
SENTINEL_CASES = ("F4", "F11", "C3-f3")              # the forward once more into a channel block of a sentinel-filled buffer


def by_id(cid):
    return next(c for c in ALL_CASES if c.id == cid)


# =====================================================================================================================
# inputs, reference, yardstick
# =====================================================================================================================
def inputs(case):
    """float32 host tensors x (B, I, *dims), w (O, I, k, ..), dy (B, O, *dims); the same for every form and slicing of a shape."""
    k = kernel_size(case)
    g = torch.Generator().manual_seed(zlib.crc32(repr((k, case.B, case.I, case.O, case.dims)).encode()))
    x = torch.randn(case.B, case.I, *case.dims, generator=g)
    w = torch.randn(case.O, case.I, *([k] * len(case.dims)), generator=g) * (k ** len(case.dims) * case.I) ** -0.5
    dy = torch.randn(case.B, case.O, *case.dims, generator=g)
    return dict(x=x, w=w, dy=dy)


def rounded_products(x, w, gy, pad, t):
    """The three products of a stride-1 convolution as the reference's autocast step computes them (nnUNetTrainer.py:848): operands
    rounded to the 16-bit type `t`, exact sums (float64 here; the kernels sum in fp32)."""
    r = lambda v: v.to(t).double()                                                          # noqa: E731
    xr, wr, gr = r(x), r(w), r(gy)
    y = F.conv2d(xr, wr, None, 1, pad)
    dx = torch.nn.grad.conv2d_input(xr.shape, wr, gr, 1, pad)
    dW = torch.nn.grad.conv2d_weight(xr, wr.shape, gr, 1, pad)
    return y, dx, dW


def evaluate(case, dtype):
    """{"y", "dx", "dW"} (the latter two where case.backward) in `dtype` on the host, from the operands as the form holds them."""
    t = inputs(case)
    held = {n: v.to(FORM_TYPE[case.form]).to(dtype) for n, v in t.items()}
    pad = kernel_size(case) // 2
    if len(case.dims) == 2 and case.form != 3 and case.backward and dtype == torch.float64:
        return dict(zip(("y", "dx", "dW"), rounded_products(t["x"], t["w"], t["dy"], pad, FORM_TYPE[case.form])))
    conv = F.conv3d if len(case.dims) == 3 else F.conv2d
    if not case.backward:
        return dict(y=conv(held["x"], held["w"], None, 1, pad))
    x, w = held["x"].requires_grad_(True), held["w"].requires_grad_(True)
    y = conv(x, w, None, 1, pad)
    y.backward(held["dy"])
    return dict(y=y.detach(), dx=x.grad, dW=w.grad)


@functools.lru_cache(maxsize=2)
def reference(case):
    """The float64 reference of a case; computed once, never modified."""
    return evaluate(case, torch.float64)


YARDSTICK_THREADS = 16


def yardstick(case):
    """The plain-fp32 yardstick of a case.  torch's fp32 weight gradient on the host divides the pixel sum among its threads and adds
    each share in plain order, so its error follows the thread count (dW of F5, 65536 pixels: 9.9e-6 of the maximum on one thread,
    3.4e-6 on four, 1.3e-6 from sixteen on -- the device kernels add at most 288 pixels per partial sum); it is taken with
    YARDSTICK_THREADS threads to be the same number on every machine.  y and dx do not depend on it."""
    before = torch.get_num_threads()
    torch.set_num_threads(YARDSTICK_THREADS)
    try:
        return evaluate(case, torch.float32)
    finally:
        torch.set_num_threads(before)


def bounds(case):
    """{quantity: bound on max |got - ref| / max |ref|}: those of tests/test_conv_wgrad_gpu.py (test_conv1x1_matches_float64,
    test_conv3x3_matches_float64, test_conv3x3x3_matches_float64, test_convolutions_in_the_16bit_operand_forms)."""
    if case.form != 3:
        return dict(y=4e-6, dx=4e-6, dW=4e-6)
    return dict(y=2e-6, dx=2e-6, dW=1e-5 if len(case.dims) == 3 else 4e-6)


def error(got, ref):
    """max |got - ref| / max |ref| (a NaN in `got` gives NaN, which no bound admits)."""
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def zero_rows(case):
    """Kernel rows of dW that no pixel pair reaches -- a one-row image has no row above or below: exactly zero."""
    return (0, 2) if len(case.dims) == 2 and case.dims[0] == 1 and kernel_size(case) == 3 else ()
