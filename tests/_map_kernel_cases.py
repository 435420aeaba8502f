"""Cases, references and path predicates for the HBM-bound map kernels -- K2 / K2n / K2v depthwise convolutions, K6 LayerNorm and
K10 plane norm -- at the sizes where their dispatch code changes path: shared by tests/test_map_kernel_paths_cpu.py and
tests/test_map_kernel_paths_gpu.py.

A CASE is a namedtuple (K2Case .. K10Case); its inputs come from a generator seeded with the case itself.  `evaluate(case, dtype)`
runs the op as a plain torch composition on the host -- F.conv2d / F.conv3d(groups=C), F.layer_norm, an explicit mean / variance /
activation formula for K10 -- and returns every output and every gradient by name ("y", "dx", "dw", ...): in float64 it is the
REFERENCE, in float32 the plain-fp32 YARDSTICK (what ordinary fp32 arithmetic makes of the same inputs; it shows how well
conditioned a case is, it is not the truth).  `tolerances(case)` are the bounds of the op's existing parity test; for the summed
parameter gradients of K6 and K10 `bounds` widens them to max(existing, 4 x the yardstick's error on that case): two correct fp32
summation orders err independently at the same scale.

PATH PREDICATES are pure functions naming the path a shape takes; each mirrors the source line in its comment, and the CPU test
compares them with the library's host queries (workspace sizes) wherever one exists.

Plain-fp32 yardstick errors (largest over the group's cases; the metric of each quantity's tolerance: |got - ref| over
max(1, max |ref|) for "close", over max |ref| for "max"), measured on the host:

    cases                                      quantity and error
    K2 plain                                   y 1.3e-07  dx 1.3e-07  dw 2.1e-07  db 3.3e-07
    K2 silu                                    y 1.7e-07  dx 1.7e-07  dw 2.0e-07  db 2.7e-07
    K2 res                                     y 9.5e-08  dx 1.1e-07  dw 1.5e-07  db 1.8e-07  dr 0.0e+00
    K2 gated                                   y 1.9e-07  dx 1.5e-07  dw 2.0e-07  db 2.9e-07  dv 1.3e-07
    K2 packed                                  y 1.4e-07  dx 1.4e-07  dw 2.1e-07  db 2.0e-07  dv 1.6e-07
    K2 silu strided                            y 1.2e-07  dx 1.4e-07  dw 1.4e-07  db 8.1e-08
    K2 plain strided                           y 7.4e-08  dx 8.0e-08  dw 1.3e-07  db 8.8e-08
    K2n plain stride 1                         y 1.2e-07  dx 1.1e-07  dw 1.1e-06  db 2.4e-06
    K2n plain stride 2                         y 1.1e-07  dx 1.2e-07  dw 1.6e-06  db 1.1e-06
    K2n res stride 1                           y 1.4e-07  xres 0.0e+00  dx 1.1e-07  dw 1.7e-06  db 1.2e-06
    K2v                                        y 2.5e-07  dx 2.8e-07  dw 4.4e-07  db 7.3e-07
    K2v strided                                y 2.0e-07  dx 2.8e-07  dw 1.5e-07  db 3.7e-07
    K6 plain <= RPB + 1 rows                   y 1.7e-07  dx 1.7e-07  dw 1.8e-07  db 1.9e-07
    K6 plain looping C=768                     y 1.3e-07  dx 1.6e-07  dw 5.1e-07  db 4.7e-07
    K6 plain looping C=640                     y 1.9e-07  dx 1.6e-07  dw 5.8e-07  db 6.9e-07
    K6 plain looping C=320                     y 1.3e-07  dx 1.5e-07  dw 1.0e-06  db 1.4e-06
    K6 plain looping C=96                      y 1.3e-07  dx 1.5e-07  dw 9.2e-07  db 1.5e-06
    K6 plain looping C=48                      y 1.5e-07  dx 1.4e-07  dw 1.7e-06  db 1.7e-06
    K6 plain looping C=96 strided              y 1.8e-07  dx 1.8e-07  dw 1.6e-06  db 1.2e-06
    K6 res looping C=96 +sum                   xsum 5.7e-08  y 1.4e-07  dskip 2.0e-07  dbranch 1.4e-07  dw 1.7e-06  db 1.3e-06
    K6 res looping C=96                        xsum 5.6e-08  y 1.6e-07  dskip 1.4e-07  dbranch 1.7e-07  dw 1.3e-06  db 1.4e-06
    K10 fp32 none HW <= 8                      y 9.0e-08  dx 9.5e-07  dgamma 7.6e-08  dbeta 9.6e-08
    K10 fp32 none HW 16380..16388              y 1.1e-07  dx 1.3e-07  dgamma 2.0e-06  dbeta 4.8e-07
    K10 fp32 silu HW 16380..16388              y 2.0e-07  dx 2.9e-07  dgamma 1.1e-07  dbeta 5.6e-07
    K10 fp32 none HW 65536..65540              y 1.2e-07  dx 1.3e-07  dgamma 2.1e-07  dbeta 2.6e-07
    K10 fp32 silu HW 65536..65540              y 1.6e-07  dx 3.2e-07  dgamma 4.5e-07  dbeta 6.3e-08
    K10 fp32 none HW 262140..262148            y 1.4e-07  dx 1.6e-07  dgamma 3.8e-07  dbeta 4.1e-07
    K10 fp32 silu HW 262140..262148            y 1.9e-07  dx 3.4e-07  dgamma 3.6e-07  dbeta 4.8e-07
    K10 fp32 silu +res offset 40 HW 65536      y 1.2e-06  dx 3.8e-06  dgamma 2.8e-06  dbeta 1.6e-06  dr 3.8e-06
    K10 fp32 silu +res offset 40 HW 262140     y 1.2e-06  dx 4.7e-06  dgamma 3.5e-06  dbeta 1.2e-06  dr 5.1e-06
    K10 fp32 leaky HW 16380..16388             y 8.4e-08  dx 9.9e-08
    K10 fp32 leaky HW 65536..65540             y 9.3e-08  dx 1.4e-07
    K10 fp32 leaky HW 262140..262148           y 1.4e-07  dx 1.1e-07
    K10 fp32 silu +res HW 16380..16388         y 1.5e-07  dx 2.3e-07  dgamma 2.0e-07  dbeta 1.5e-07  dr 1.9e-07
    K10 fp32 silu +res HW 65536..65540         y 1.4e-07  dx 4.6e-07  dgamma 6.4e-07  dbeta 1.8e-07  dr 4.0e-07
    K10 fp32 silu +res HW 262140..262148       y 1.7e-07  dx 3.2e-07  dgamma 2.8e-07  dbeta 2.4e-07  dr 2.9e-07
    K10 fp32 silu dy slice HW 65536..65540     y 1.3e-07  dx 1.9e-07  dgamma 5.0e-07  dbeta 2.8e-07
    K10 fp32 silu dy slice HW 262140..262148   y 1.5e-07  dx 2.2e-07  dgamma 9.0e-08  dbeta 1.3e-07
    K10 bf16 silu +res HW 65536..65540         y 1.4e-07  dx 1.9e-07  dgamma 1.8e-07  dbeta 3.9e-08  dr 2.0e-07
    K10 fp16 silu +res HW 65536..65540         y 1.3e-07  dx 1.7e-07  dgamma 1.7e-07  dbeta 6.8e-08  dr 1.6e-07
    K10 bf16 silu +res HW 262140..262148       y 1.7e-07  dx 2.4e-07  dgamma 1.2e-07  dbeta 2.0e-07  dr 2.0e-07
    K10 fp16 silu +res HW 262140..262148       y 2.0e-07  dx 2.4e-07  dgamma 2.4e-07  dbeta 2.9e-07  dr 2.2e-07

The widened bounds this gives: 5.2e-6 .. 6.8e-6 on d(gamma) / d(beta) of the looping K6 cases (4 x 1.3e-6 .. 1.7e-6, existing 5e-6);
every K10 case stays on its existing bound.
"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

EPS = 1e-5
LEAKY_SLOPE = 0.01
LEAKY_MIN_PRE = 1e-4             # LeakyReLU gradients are compared where the float64 pre-activation is at least this far from 0 ...
LEAKY_MAX_EXCLUDED = 1e-3        # ... which may leave out this share of a case's elements at the most


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(case)).encode()))


# =====================================================================================================================
# path predicates
# =====================================================================================================================
# ---- K2 (csrc/dwconv.hip) -------------------------------------------------------------------------------------------
K2_TY, K2_TX, K2_CCH = 8, 16, 32                     # dwconv.hip:29  constexpr int TY = 8, TX = 16, CCH = 32


def k2_tile_grid(H, W, C):
    """(tiles along y, tiles along x, 32-channel blocks) of the forward / data-gradient kernel (dwconv.hip:325) and whether the last
    tile of each is ragged."""
    grid = (-(-H // K2_TY), -(-W // K2_TX), -(-C // K2_CCH))
    return grid, (H % K2_TY != 0, W % K2_TX != 0, C % K2_CCH != 0)


def k2_wgrad_wave_shapes(W):
    """(groups of 4 columns, scalar tail columns) that each of the 4 waves of the weight-gradient kernel walks: dwconv.hip:119-120
    seg = (W + 3) / 4, x_begin = ph * seg, x_end = min(x_begin + seg, W); :140 the group loop; :170 the tail."""
    seg = (W + 3) // 4
    out = []
    for ph in range(4):
        n = max(0, min(ph * seg + seg, W) - ph * seg)
        out.append((n // 4, n % 4))
    return out


def k2_wave_kind(shape):
    groups, tail = shape
    if groups == 0:
        return "tail" if tail else "empty"
    return "groups+tail" if tail else "groups"


def k2_wgrad_channel_blocks(C):
    """Channels in each 64-channel block of the weight-gradient grid (dwconv.hip:116, :257)."""
    return [min(64, C - c0) for c0 in range(0, C, 64)]


def k2_partial_rows(B, H):
    """Partial rows the weight-gradient kernel leaves for the reduce kernel: one per (batch, image row) (dwconv.hip:249)."""
    return B * H


def k2_reduce_shapes(rows):
    """{(pairs, tail)} over the 16 row groups of dwconv_wgrad_reduce_kernel (dwconv.hip:216-221: for (; r + 16 < rows; r += 32) a pair,
    then if (r < rows) one more row)."""
    out = set()
    for rg in range(16):
        r, pairs = rg, 0
        while r + 16 < rows:
            pairs, r = pairs + 1, r + 32
        out.add((min(pairs, 2), int(r < rows)))
    return out


# ---- K2n (csrc/dwconv_nchw.hip) -------------------------------------------------------------------------------------
def k2n_path(W, stride):
    """dwconv_nchw.hip:256-261 and :291-305: the 4-pixel strip kernels, the stride-2 kernels, the generic stride-1 kernels."""
    if stride == 1 and W % 4 == 0:
        return "s1_strip"
    return "s2" if stride == 2 else "s1_generic"


def k2n_out(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1          # dwconv_nchw.hip:234-235


def k2n_wgrad_slices(H, W, stride):
    """Work items (strips on the strip path, output pixels otherwise) of every slice of a plane in the weight-gradient kernels:
    dwconv_nchw.hip:239-244 ns = ceil(Ho * Wo / 4096), :130-132 / :182-184 per = ceil(n / ns), [lo, min(lo + per, n))."""
    Ho, Wo = k2n_out(H, W, stride)
    ns = max(1, -(-(Ho * Wo) // 4096))
    n = H * (W // 4) if k2n_path(W, stride) == "s1_strip" else Ho * Wo
    per = -(-n // ns)
    return [max(0, min(s * per + per, n) - s * per) for s in range(ns)]


def k2n_data_blocks(H, W, stride):
    """256-thread workgroups per plane of the forward and of the data-gradient kernel (dwconv_nchw.hip:257-261, :293-298)."""
    Ho, Wo = k2n_out(H, W, stride)
    if k2n_path(W, stride) == "s1_strip":
        n = -(-(H * (W // 4)) // 256)
        return n, n
    return -(-(Ho * Wo) // 256), -(-(H * W) // 256)


# ---- K2v (csrc/dwconv3d.hip) ----------------------------------------------------------------------------------------
K2V_TOK, K2V_WTOK = 64, 256                          # dwconv3d.hip:25, :79


def k2v_blocks(L):
    """((gather workgroups, tokens in the last), (weight-gradient chunks, tokens in the last)): dwconv3d.hip:190, :213."""
    return ((-(-L // K2V_TOK), L - (-(-L // K2V_TOK) - 1) * K2V_TOK), (-(-L // K2V_WTOK), L - (-(-L // K2V_WTOK) - 1) * K2V_WTOK))


def k2v_edge(L, block):
    """Where L sits relative to a multiple of `block`: "under" (one short), "on", "over" (one past) or "between"."""
    return {block - 1: "under", 0: "on", 1: "over"}.get(L % block, "between")


# ---- K6 (csrc/layernorm.hip) ----------------------------------------------------------------------------------------
K6_ROW_SHAPES = {48: (4, 3), 96: (8, 3), 192: (16, 3), 384: (32, 3), 768: (64, 3), 32: (8, 1), 64: (16, 1), 128: (32, 1), 256: (64, 1),
                 512: (64, 2), 320: (16, 5), 640: (32, 5)}          # layernorm.hip:156-173 row_shape: C -> (lanes per row, float4 per lane)
K6_MAX_GRID = 1024                                   # layernorm.hip:180


def k6_rpb(C):
    return 256 // K6_ROW_SHAPES[C][0]                # layernorm.hip:43 RPB = BLOCK / LPR


def k6_grid(rows, C):
    return min(K6_MAX_GRID, -(-rows // k6_rpb(C)))   # layernorm.hip:176-181 grid_blocks


def k6_trips(rows, C):
    """Loop trips of every workgroup (layernorm.hip:51, :103: for (row = blockIdx.x * RPB + rl; row < rows; row += gridDim.x * RPB)):
    a trip counts when at least one of the workgroup's row lanes has a row."""
    rpb, grid = k6_rpb(C), k6_grid(rows, C)
    return [max(0, -(-(rows - wg * rpb) // (grid * rpb))) for wg in range(grid)]


# ---- K10 (csrc/plane_norm.hip) --------------------------------------------------------------------------------------
K10_REG256, K10_REG1024, K10_SEGMENTED = 256 * 4 * 16, 1024 * 4 * 16, 64 * 4096     # plane_norm.hip:476, :477 (mlagg_plane_norm_fwd), :432 (split_segments)
K10_SEG = 4 * 4096                                   # plane_norm.hip:283 SEG4 float4 per segment


def k10_segments(HW):
    """plane_norm.hip:430-434 split_segments (planes of whole float4 only)."""
    if HW % 4 or HW < K10_SEGMENTED:
        return 0
    return -(-HW // K10_SEG)


def k10_fwd_path(HW):
    """plane_norm.hip:465-479, mlagg_plane_norm_fwd (planes of a contiguous map are aligned whenever HW % 4 == 0)."""
    if HW % 4:
        return "stream_scalar"
    if k10_segments(HW):
        return "segmented"
    if HW <= K10_REG256:
        return "reg256"
    return "reg1024" if HW <= K10_REG1024 else "stream_vec"


def k10_bwd_path(HW):
    """plane_norm.hip:503-529, mlagg_plane_norm_bwd_strided: the backward has no register-resident form."""
    if HW % 4:
        return "stream_scalar"
    return "segmented" if k10_segments(HW) else "stream_vec"


# =====================================================================================================================
# cases
# =====================================================================================================================
K2Case = collections.namedtuple("K2Case", "form B H W C pad")                 # form: plain | silu | res | gated | packed; pad: x is a column
K2nCase = collections.namedtuple("K2nCase", "form B C H W stride")            # block of a row C + pad wide.  form: plain | res
K2vCase = collections.namedtuple("K2vCase", "B dims C bias silu pad")
K6Case = collections.namedtuple("K6Case", "form rows C strided_x strided_dy use_sum")      # form: plain | res (3 samples, scale 0 / 1.25 / 1.25)
K10Case = collections.namedtuple("K10Case", "dims act affine res offset dy_slice dtype")   # B = 2, C = 3; act: none | silu | leaky
K10_B, K10_C = 2, 3
K6_RES_SCALE = (0.0, 1.25, 1.25)

K2_ALL_FORMS = ("plain", "silu", "res", "gated", "packed")
K2_GEOMETRIES = [
    # (B, H, W, C), forms                         wave shapes of the weight gradient / what else it reaches
    ((2, 5, 20, 36), K2_ALL_FORMS),              # 4 x (1 group + 1 tail); 36 channels: one quad in a second 32-block
    ((2, 3, 30, 68), K2_ALL_FORMS),              # 3 x 2 groups, last wave 1 group + 2 tail; one quad in a second 64-block
    ((2, 4, 17, 8), K2_ALL_FORMS),               # 3 x (1 group + 1 tail), last wave tail only
    ((2, 9, 2, 4), K2_ALL_FORMS),                # two waves empty
    ((2, 8, 3, 100), K2_ALL_FORMS),              # one wave empty
    ((3, 17, 5, 36), K2_ALL_FORMS),              # seg 2: last wave 1 column, 51 partial rows: two pairs in the reduce kernel
    ((2, 8, 16, 32), ("plain", "silu")),         # exactly one tile, one channel block
    ((2, 9, 33, 64), ("plain", "silu")),         # one row and one column past a tile
    ((3, 11, 7, 12), ("plain", "silu")),         # 33 partial rows
    ((1, 16, 4, 4), ("plain", "silu")),          # 16 partial rows
    ((1, 17, 6, 4), ("plain", "silu")),          # 17
    ((3, 16, 12, 4), ("plain", "silu")),         # 48
]
K2_CASES = [K2Case(f, *g, 0) for g, forms in K2_GEOMETRIES for f in forms] + [K2Case("silu", 2, 5, 20, 36, 8), K2Case("plain", 2, 4, 17, 8, 8)]

K2N_CASES = [K2nCase("plain", 2, *s) for s in [
    (3, 5, 4, 1), (5, 1, 8, 1), (2, 40, 28, 1),  # strips: one strip per row (both neighbours outside), one row, 280 strips = 2 workgroups
    (2, 65, 68, 1),                              # strips, two weight-gradient slices of 553 and 552 strips
    (3, 6, 6, 1), (4, 17, 19, 1),                # generic stride 1
    (2, 65, 65, 1),                              # ... two slices of 2113 and 2112 pixels
    (3, 8, 8, 2), (3, 9, 8, 2), (3, 8, 9, 2), (2, 1, 5, 2), (2, 2, 2, 2), (2, 35, 37, 2),
    (2, 129, 129, 2),                            # stride 2, 65 x 65 outputs: two slices
]] + [K2nCase("res", 2, *s) for s in [(6, 5, 4, 1), (4, 40, 28, 1), (2, 65, 68, 1)]]

K2V_DIMS = [((3, 3, 7), 4), ((4, 4, 4), 68), ((5, 13, 1), 96), ((3, 5, 17), 64), ((4, 8, 8), 4), ((1, 1, 257), 68), ((3, 9, 19), 96)]
K2V_CASES = [K2vCase(2, d, C, bias, silu, 0) for d, C in K2V_DIMS for bias in (True, False) for silu in (True, False)] + \
    [K2vCase(2, (3, 5, 17), 64, True, True, 8)]


def k6_loop_rows(C):
    return K6_MAX_GRID * k6_rpb(C) + k6_rpb(C) + 1


K6_LOOP_WIDTHS = (768, 640, 320, 96, 48)
K6_RES_ROWS = 32802                                  # 3 x 10934 >= k6_loop_rows(96) = 32801; a sample boundary inside a workgroup's rows
K6_CASES = [K6Case("plain", r, C, False, False, False) for C in sorted(K6_ROW_SHAPES)
            for r in sorted({1, k6_rpb(C) - 1, k6_rpb(C), k6_rpb(C) + 1})] + \
    [K6Case("plain", k6_loop_rows(C), C, False, False, False) for C in K6_LOOP_WIDTHS] + \
    [K6Case("plain", k6_loop_rows(96), 96, True, True, False)] + \
    [K6Case("res", K6_RES_ROWS, 96, False, False, s) for s in (True, False)]

K10_SMALL = [(1, 1), (1, 2), (3, 1), (2, 2), (2, 4)]                                                  # HW = 1, 2, 3, 4, 8
K10_LARGE = [(60, 273), (128, 128), (68, 241), (256, 256), (580, 113), (65539, 1), (1020, 257), (64, 64, 64), (4, 65537)]
#        HW = 16380,    16384,      16388,     65536,      65540,      65539,      262140,      262144,       262148
K10_CASES = [K10Case(d, "none", True, False, 0.0, False, "fp32") for d in K10_SMALL] + \
    [K10Case(d, act, True, False, 0.0, False, "fp32") for d in K10_LARGE for act in ("none", "silu")] + \
    [K10Case(d, "silu", True, True, 40.0, False, "fp32") for d in [(256, 256), (1020, 257)]] + \
    [K10Case(d, "leaky", False, False, 0.0, False, "fp32") for d in [(128, 128), (256, 256), (580, 113), (65539, 1), (4, 65537)]] + \
    [K10Case(d, "silu", True, True, 0.0, False, "fp32") for d in [(60, 273), (256, 256), (1020, 257), (65539, 1), (64, 64, 64)]] + \
    [K10Case(d, "silu", True, False, 0.0, True, "fp32") for d in [(256, 256), (64, 64, 64)]] + \
    [K10Case(d, "silu", True, True, 0.0, False, dt) for d in [(256, 256), (64, 64, 64)] for dt in ("bf16", "fp16")]

CASES = {"k2": K2_CASES, "k2n": K2N_CASES, "k2v": K2V_CASES, "k6": K6_CASES, "k10": K10_CASES}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def family(case):
    return type(case).__name__[:-4].lower()


def case_id(case):
    def one(v):
        if isinstance(v, tuple):
            return "x".join(str(i) for i in v)
        if isinstance(v, bool):
            return "T" if v else "F"
        return str(v)
    return "-".join(one(v) for v in case)


def k10_hw(case):
    n = 1
    for v in case.dims:
        n *= v
    return n


# =====================================================================================================================
# inputs: float32 host tensors by name; the cotangent of output "y" is "d_y"
# =====================================================================================================================
def inputs(case):
    g = _gen(case)
    rn = lambda *s: torch.randn(*s, generator=g)                                                      # noqa: E731
    fam = family(case)
    if fam == "k2":
        B, N, C = case.B, case.H * case.W, case.C
        t = dict(x=rn(B, N, C), w=rn(C, 1, 3, 3) * 0.3, b=rn(C) * 0.1, d_y=rn(B, N, C))
        if case.form == "res":
            t["r"] = rn(B, N, C)
        if case.form in ("gated", "packed"):
            t["v"] = rn(B, N, C)
        return t
    if fam == "k2n":
        B, C, H, W = case.B, case.C, case.H, case.W
        Ho, Wo = k2n_out(H, W, case.stride)
        t = dict(x=rn(B, C, H, W), w=rn(C, 1, 3, 3) * 0.3, b=rn(C) * 0.1, d_y=rn(B, C, Ho, Wo))
        if case.form == "res":
            t["d_xres"] = rn(B, C, H, W)
        return t
    if fam == "k2v":
        D, H, W = case.dims
        B, L, C = case.B, D * H * W, case.C
        t = dict(x=rn(B, L, C), w=rn(C, 1, 3, 3, 3) * 0.3, d_y=rn(B, L, C))
        if case.bias:
            t["b"] = rn(C)
        return t
    if fam == "k6":
        C = case.C
        if case.form == "plain":
            return dict(x=rn(case.rows, C) * 2 + 0.5, w=rn(C) * 0.2 + 1, b=rn(C) * 0.1, d_y=rn(case.rows, C))
        n = case.rows // 3
        t = dict(skip=rn(3, n, C), branch=rn(3, n, C), w=rn(C), b=rn(C), d_y=rn(3, n, C))
        if case.use_sum:
            t["d_xsum"] = rn(3, n, C)
        return t
    if fam == "k10":
        shape = (K10_B, K10_C) + tuple(case.dims)
        dt = DTYPES[case.dtype]
        x = rn(*shape) * 0.5 + case.offset if case.offset else rn(*shape) * 2 + 0.5
        t = dict(x=x.to(dt).float(), d_y=rn(*shape).to(dt).float())               # 16-bit maps: the values the device holds, widened
        if case.affine:
            t["gamma"], t["beta"] = rn(K10_C) * 0.5 + 1, rn(K10_C)
        if case.res:
            t["r"] = rn(*shape)                                                   # the residual stays fp32 in the 16-bit modes
        return t
    raise ValueError(fam)


LEAVES = {"k2": ("x", "w", "b", "r", "v"), "k2n": ("x", "w", "b"), "k2v": ("x", "w", "b"), "k6": ("x", "skip", "branch", "w", "b"),
          "k10": ("x", "gamma", "beta", "r")}
GRAD_NAME = {"w": "dw", "b": "db", "x": "dx", "r": "dr", "v": "dv", "skip": "dskip", "branch": "dbranch", "gamma": "dgamma", "beta": "dbeta"}


# =====================================================================================================================
# the ops as plain torch compositions
# =====================================================================================================================
def compose(case, t):
    """{output name: tensor} from the tensors `t` (any floating type); K10 adds "_pre", the pre-activation (not an output)."""
    fam = family(case)
    if fam == "k2":
        B, H, W, C = case.B, case.H, case.W, case.C
        o = F.conv2d(t["x"].reshape(B, H, W, C).permute(0, 3, 1, 2), t["w"], t["b"], padding=1, groups=C)
        if case.form in ("silu", "gated", "packed"):
            o = F.silu(o)
        o = o.permute(0, 2, 3, 1).reshape(B, H * W, C)
        if case.form == "res":
            o = o + t["r"]
        if case.form in ("gated", "packed"):
            o = o * t["v"]
        return dict(y=o)
    if fam == "k2n":
        out = dict(y=F.conv2d(t["x"], t["w"], t["b"], stride=case.stride, padding=1, groups=case.C))
        if case.form == "res":
            out["xres"] = t["x"] * 1.0                                            # the map itself, on its way to the residual sum
        return out
    if fam == "k2v":
        D, H, W = case.dims
        B, C = case.B, case.C
        o = F.conv3d(t["x"].transpose(1, 2).reshape(B, C, D, H, W), t["w"], t.get("b"), padding=1, groups=C)
        return dict(y=(F.silu(o) if case.silu else o).reshape(B, C, D * H * W).transpose(1, 2))
    if fam == "k6":
        if case.form == "plain":
            return dict(y=F.layer_norm(t["x"], (case.C,), t["w"], t["b"], EPS))
        scale = torch.tensor(K6_RES_SCALE, dtype=t["skip"].dtype).view(-1, 1, 1)
        xs = t["skip"] + t["branch"] * scale
        return dict(xsum=xs, y=F.layer_norm(xs, (case.C,), t["w"], t["b"], EPS))
    if fam == "k10":
        x = t["x"].flatten(2)                                                     # (B, C, HW)
        mean = x.mean(2, keepdim=True)
        var = ((x - mean) ** 2).mean(2, keepdim=True)                             # about the mean, biased: what the norm layers use
        pre = (x - mean) / torch.sqrt(var + EPS)
        if case.affine:
            pre = pre * t["gamma"].view(1, -1, 1) + t["beta"].view(1, -1, 1)
        if case.res:
            pre = pre + t["r"].flatten(2)
        y = {"none": pre, "silu": F.silu(pre), "leaky": F.leaky_relu(pre, LEAKY_SLOPE)}[case.act]
        return dict(y=y.reshape(t["x"].shape), _pre=pre.reshape(t["x"].shape))
    raise ValueError(fam)


def evaluate(case, dtype=torch.float64):
    """{quantity: tensor of `dtype`}: every output of `compose` and the gradient of every leaf (GRAD_NAME), on the host."""
    inp = inputs(case)
    t = {k: v.to(dtype) for k, v in inp.items()}
    leaves = [k for k in LEAVES[family(case)] if k in t]
    for k in leaves:
        t[k].requires_grad_(True)
    outs = compose(case, t)
    fed = [k for k in outs if "d_" + k in t]
    torch.autograd.backward([outs[k] for k in fed], [t["d_" + k] for k in fed])
    res = {k: v.detach() for k, v in outs.items()}
    res.update({GRAD_NAME[k]: t[k].grad for k in leaves})
    return res


@functools.lru_cache(maxsize=2)
def reference_and_yardstick(case):
    """(float64 reference, plain-fp32 yardstick) of a case; computed once, never modified."""
    return evaluate(case, torch.float64), evaluate(case, torch.float32)


def compared(case, ref):
    """The quantities the device test compares: all but the underscore ones."""
    return [k for k in ref if not k.startswith("_")]


def mask_for(case, quantity, ref):
    """Elements of `quantity` that are compared (None: all).  Behind LeakyReLU the slope flips within rounding distance of 0: the
    element-wise gradients are compared where the float64 pre-activation is at least LEAKY_MIN_PRE away from it."""
    if family(case) == "k10" and case.act == "leaky" and quantity in ("dx", "dr"):
        return ref["_pre"].abs() >= LEAKY_MIN_PRE
    return None


LEAKY_FLIP_ZONE = 4e-6           # |pre| below which two correct fp32 evaluations may disagree about the sign (their error is ~2e-7)


def leaky_flip_shift(case, ref):
    """The most a LeakyReLU slope evaluated on the other side of 0 can move the COMPARED elements of dx: every element of a plane
    with |pre| < LEAKY_FLIP_ZONE changes the plane's mean gradient by (1 - slope) |dy| / HW, which dx carries times rstd (its share
    of the second mean vanishes with xhat = pre at 0; the cases have no affine and no residual)."""
    assert case.act == "leaky" and not case.affine and not case.res
    t = inputs(case)
    x = t["x"].double().flatten(2)
    rstd = 1.0 / torch.sqrt(x.var(2, unbiased=False) + EPS)
    near = (ref["_pre"].abs() < LEAKY_FLIP_ZONE).flatten(2).sum(2)
    return float((near * rstd).max()) * (1.0 - LEAKY_SLOPE) * float(t["d_y"].abs().max()) / k10_hw(case)


# =====================================================================================================================
# tolerances
# =====================================================================================================================
# ("close", a, r): |got - ref| <= a * max(1, max |ref|) + r * |ref| element-wise (_close of tests/test_blocks_gpu.py);
# ("max", a, c):   max |got - ref| <= a * max |ref| + c.
Tol = collections.namedtuple("Tol", "kind a r widen")


def _tol(kind, a, r, widen=False):
    return Tol(kind, a, r, widen)


def tolerances(case):
    """{quantity: Tol}: the bounds of the op's existing parity test (named in the comments)."""
    fam = family(case)
    c = lambda a, r, widen=False: _tol("close", a, r, widen)                                         # noqa: E731
    if fam == "k2":
        if case.form in ("gated", "packed"):                                      # test_gated_dwconv3x3_matches_conv2d_times_gate
            return dict(y=c(1e-5, 1e-5), dx=c(1e-5, 1e-4), dv=c(1e-5, 1e-4), dw=c(2e-5, 1e-4), db=c(2e-5, 1e-4))
        return dict(y=c(1e-5, 1e-5), dx=c(1e-5, 1e-4), dw=c(1e-5, 1e-4), db=c(1e-5, 1e-4), dr=c(1e-5, 1e-4))     # test_dwconv3x3_matches_conv2d
    if fam == "k2n":                                                              # test_dwconv3x3_nchw_matches_conv2d
        return dict(y=c(1e-5, 1e-5), xres=c(0.0, 0.0), dx=c(1e-5, 1e-4), dw=c(1e-5, 1e-4), db=c(1e-5, 1e-4))
    if fam == "k2v":                                                              # test_dwconv3d_matches_torch_conv3d
        return dict(y=c(2e-5, 0.0), dx=c(2e-5, 0.0), dw=c(1e-4, 0.0), db=c(1e-4, 0.0))
    if fam == "k6":                                                               # test_layernorm_matches_torch, test_residual_layer_norm_matches_torch
        return dict(y=c(2e-6, 1e-5), xsum=c(1e-6, 1e-6), dx=c(5e-6, 1e-4), dskip=c(5e-6, 1e-4), dbranch=c(5e-6, 1e-4),
                    dw=c(5e-6, 1e-4, True), db=c(5e-6, 1e-4, True))
    if fam == "k10":
        m = lambda a, cst, widen=False: _tol("max", a, cst, widen)                                   # noqa: E731
        if case.dtype != "fp32":                                                  # test_plane_norm_16_bit_maps
            e16 = 2.0 ** -8 if case.dtype == "bf16" else 2.0 ** -11
            return dict(y=m(e16 * 1.01, 1e-6), dx=m(2 * e16, 1e-6), dr=m(1e-5, 1e-6), dgamma=m(1e-4, 1e-5, True), dbeta=m(1e-4, 1e-5, True))
        if case.offset:                                                           # test_plane_norm_segmented_planes_match_torch
            return dict(y=m(0.0, 1e-3), dx=m(5e-4, 0.0), dr=m(5e-4, 0.0), dgamma=m(5e-4, 0.0, True), dbeta=m(5e-4, 0.0, True))
        # test_plane_norm_matches_torch; the residual gradient behind SiLU as in test_plane_norm_16_bit_maps (fp32 residual)
        return dict(y=c(2e-5, 0.0), dx=c(5e-5, 0.0), dr=m(1e-5, 1e-6), dgamma=c(1e-4, 0.0, True), dbeta=c(1e-4, 0.0, True))
    raise ValueError(fam)


def error(got, ref, tol, mask=None):
    """(error in the scale of `tol`'s first number, largest excess of |got - ref| over what `tol` allows): passes when excess <= 0."""
    ref = ref.double()
    d = (got.detach().cpu().double() - ref).abs()
    if mask is not None:
        d = d * mask
    top = float(ref.abs().max())
    if tol.kind == "close":
        scale = max(1.0, top)
        return float(d.max()) / scale, float((d - tol.a * scale - tol.r * ref.abs()).max())
    return float(d.max()) / max(top, 1e-30), float(d.max()) - (tol.a * top + tol.r)


def bounds(case, ref, yard):
    """{quantity: Tol} of the device test: `tolerances`, the summed parameter gradients of K6 / K10 widened to 4 x the yardstick's
    error on this case where that is more (from the host yardstick, never from the kernel's output)."""
    out = {}
    for q in compared(case, ref):
        tol = tolerances(case)[q]
        if tol.widen:
            tol = tol._replace(a=max(tol.a, 4.0 * error(yard[q], ref[q], tol, mask_for(case, q, ref))[0]))
        out[q] = tol
    return out
