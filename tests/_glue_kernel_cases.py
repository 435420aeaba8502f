"""Cases, references and path predicates for the glue kernels between the compute families -- K1' 2-D (csrc/cross_scan.hip), K1' 3-D
(csrc/index_scan.hip), K8 (csrc/small_ops.hip), K13 (csrc/channel_epilogue.hip) and K17 (csrc/gelu_pool.hip) -- at the sizes where
their code changes path: shared by tests/test_glue_kernel_paths_cpu.py and tests/test_glue_kernel_paths_gpu.py.

A CASE is a namedtuple (XScanCase .. PoolCase); its inputs come from a generator seeded with the case itself.  `evaluate(case, dtype)`
runs the op as a plain torch composition on the host and returns every output and every gradient by name: in float64 it is the
REFERENCE, in float32 the plain-fp32 YARDSTICK (what ordinary fp32 arithmetic makes of the same inputs; it shows how well conditioned
a case is, it is not the truth).  The references restate the operations, they do not call the package: the 2-D scan sequences are
built per scale from views, transposes and flips the way the reference model does, the merge is the explicit inverse placement, the
3-D forms are `tok[:, idx[k]]` gathers and `index_add`, the pixel shuffle is its index formula.

TOLERANCES (`tolerances`, `bounds`):
  * "equal": pure data movement, compared bit for bit;
  * "sum":   a fixed number of terms, |got - ref| <= (terms - 1) * 2^-24 * sum |terms| element-wise -- holds for any summation order;
  * "resid": 2 * 2^-24 * (|skip| + |branch * scale|) element-wise -- a fused or an unfused multiply-add;
  * "close" / "max": the bound of the op's existing parity test (named in the comments of `tolerances`); the quantities that hang on a
    long fp32 sum (d(bias), the channel and column sums, lambda and what is derived from its exponentials) are widened to
    max(existing, 4 x the yardstick's error on that case): two correct fp32 summation orders err independently at the same scale.
    The widening comes from the host yardstick alone.  For diff_lambda -- one scalar, whose yardstick error can be 0 by luck -- the
    yardstick is evaluated in three summation orders and the largest error counts.

PATH PREDICATES are pure functions naming the path a shape takes; each mirrors the source line in its comment, and the CPU test
compares them with the library's host queries wherever one exists.

Plain-fp32 yardstick errors (largest over the group's cases; in the metric of each quantity's tolerance: |got - ref| over
max(1, max |ref|) for "close", over max |ref| for "max", over max sum |terms| for "sum" / "resid", the largest difference for
"equal"), measured on the host:

    cases                          quantity and error
    K1' 2-D scan                   seq 0.0e+00  dtok 8.1e-08
    K1' 2-D merge                  tok 8.8e-08  dseq 0.0e+00
    K1' 2-D bc                     dtr 0.0e+00  Bs 0.0e+00  Cs 0.0e+00  dxdbl 0.0e+00
    K1' 3-D scan                   seq 0.0e+00  dtok 1.1e-07
    K1' 3-D scanblk                seq 0.0e+00  dtok 0.0e+00
    K1' 3-D merge                  tok 1.2e-07  dseq 0.0e+00
    K1' 3-D bc                     dtr 0.0e+00  Bs 0.0e+00  Cs 0.0e+00  dxdbl 0.0e+00
    K8 transposes, shuffles        y 0.0e+00
    K8 conv_t2x2 (strided inverse) y 2.0e-07  dx 2.4e-07  dw 3.9e-07
    K8 channel_sum (bias)          y 5.4e-08  dx 0.0e+00  dbias 1.8e-06
    K8 channel_sum (epilogue)      y 4.0e-08  dx 0.0e+00  dbias 1.7e-07
    K8 column_sum                  sum 1.6e-07
    K8 scaled_residual             y 6.8e-08  y_zero 0.0e+00  dskip 0.0e+00  dbranch 4.8e-08
    K8 diff_lambda, dot 1          lam 4.1e-07  dq1 1.1e-07  dk1 1.5e-07  dq2 1.5e-07  dk2 1.3e-07   (largest of three orders)
    K8 diff_lambda, dot 8          lam 1.1e-06  dq1 6.3e-07  dk1 6.1e-07  dq2 4.3e-07  dk2 4.1e-07   (largest of three orders)
    K13 fp32                       y 4.6e-07  dx 1.8e-07  dres 1.8e-07  dbias 5.7e-07
    K13 fp32, |x| up to 12         y 7.5e-08  dx 1.2e-07  dres 1.2e-07  dbias 1.4e-07
    K13 16-bit                     y 2.1e-07  dx 1.7e-07  dres 1.7e-07  dbias 5.7e-07   (before the rounding to 16 bits)
    K17                            pooled 2.4e-07  ds 1.5e-07
    K17, inputs x 6                pooled 2.5e-07  ds 8.2e-09

Widened bounds: diff_lambda is the only op whose existing bound (1e-6 absolute, from an n = 24 case with exponentials of order 1)
cannot hold at its new cases: with the dot products at 8 the exponentials reach 3e3, where one fp32 rounding of lambda is 1.2e-4.
Its bound becomes 4 x yardstick x max |ref| + 1e-6: up to 4.3e-6 x max |ref| for lambda and 2.5e-6 x max |ref| for the gradients at
dot 8, 1.7e-6 and 6.0e-7 at dot 1.  The column sums are widened to at most 6.6e-7 x max |ref| on top of their 1e-4 / 2e-3.  Every
other quantity stays on the bound of its existing test (4 x its yardstick error is below it).
"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

U = 2.0 ** -24                   # unit roundoff of fp32


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(case)).encode()))


def _ceil(a, b):
    return -(-a // b)


# =====================================================================================================================
# path predicates
# =====================================================================================================================
# ---- K1' 2-D (csrc/cross_scan.hip) ----------------------------------------------------------------------------------
XS_TS, XS_CH = 16, 32                                # cross_scan.hip:28-29  constexpr int TS = 16; CH = 32


def xscan_offsets(HW):
    """(off[] per scale, L_cat): cross_scan.hip:192-205 make_geom."""
    offs, off = [], 0
    for H, W in HW:
        offs.append(off)
        off += H * W
    return offs, off


def xscan_vec4(HW):
    """Per scale, whether it takes the 16-byte path: cross_scan.hip:65  vec4 = ((H | W | off | g.Lc) & 3) == 0."""
    offs, Lc = xscan_offsets(HW)
    return [((H | W | off | Lc) & 3) == 0 for (H, W), off in zip(HW, offs)]


def xscan_tiles(HW):
    """(tile0[] with the total last, [(ragged in y, ragged in x) per scale]): cross_scan.hip:197, :201 t0 += ceil(H / TS) * ceil(W / TS)."""
    tile0, t0 = [], 0
    for H, W in HW:
        tile0.append(t0)
        t0 += _ceil(H, XS_TS) * _ceil(W, XS_TS)
    return tile0 + [t0], [(H % XS_TS != 0, W % XS_TS != 0) for H, W in HW]


def xscan_channel_blocks(CB):
    """Channels of every 32-channel block of the grid: cross_scan.hip:62 nc = min(CH, CB - c0), :220 (CB + CH - 1) / CH."""
    return [min(XS_CH, CB - c0) for c0 in range(0, CB, XS_CH)]


# ---- K1' 3-D (csrc/index_scan.hip) ----------------------------------------------------------------------------------
IS_TL, IS_UN = 64, 8                                 # index_scan.hip:23-24  constexpr int TL = 64; UN = 8
IS_MAX_CB = 512                                      # index_scan.hip:116  CB > 512 is refused
LDS_OPT_IN = 48 * 1024                               # internal.h:19  bytes > 48 * 1024: hipFuncSetAttribute


def iscan_tile(L):
    """(tiles, steps n of the last): index_scan.hip:33-34 l0 = blockIdx.x * TL, n = min(TL, L - l0); :133 grid (L + TL - 1) / TL."""
    tiles = _ceil(L, IS_TL)
    return tiles, L - (tiles - 1) * IS_TL


def iscan_trips(n, CB):
    """Trips of the gather loop of a tile of n steps: index_scan.hip:42  for (e0 = threadIdx.x; e0 < n * CB; e0 += 256 * UN)."""
    return _ceil(n * CB, 256 * IS_UN)


def iscan_lds_bytes(CB):
    """(dynamic LDS bytes, needs the opt-in, supported): index_scan.hip:130 CB * (TL + 1) * sizeof(float), :116, internal.h:18-20."""
    b = CB * (IS_TL + 1) * 4
    return b, b > LDS_OPT_IN, CB <= IS_MAX_CB


def imerge_form(K, CB):
    """The form ops.index_merge takes: ops.py IndexMergeFn.forward `if K > 1 and CB % 4 == 0` (direction-separated stores +
    block_sum_kernel), else index_scan.hip:148 atomic = blk_stride == 0 && K > 1."""
    if K == 1:
        return "plain"
    return "wide+block_sum" if CB % 4 == 0 else "atomic"


def block_sum_shape(K):
    """(pairs, odd tail) of block_sum_kernel: index_scan.hip:101 for (; k + 1 < K; k += 2), :106 if (k < K)."""
    return K // 2, K % 2


# ---- K8 (csrc/small_ops.hip) ----------------------------------------------------------------------------------------
TR_TT = 64                                           # small_ops.hip:129  constexpr int TT = 64


def transpose_forms(R, C):
    """((v_in, v_out), (tiles along C, tiles along R), (ragged in C, ragged in R)): small_ops.hip:141 v_in = (Cc & 3) == 0,
    v_out = (R & 3) == 0; :203 grid."""
    return (C % 4 == 0, R % 4 == 0), (_ceil(C, TR_TT), _ceil(R, TR_TT)), (C % TR_TT != 0, R % TR_TT != 0)


def plane_sum_shape(HW):
    """(float4 count, trips of the 512-wide loop, second load of the last trip live, scalar tail): small_ops.hip:291 n4 (planes of a
    contiguous map whose HW % 4 == 0 are aligned), :292 for (i = threadIdx.x; i < n4; i += 512), :295 if (i + 256 < n4), :300 the tail."""
    n4 = HW // 4 if HW % 4 == 0 else 0
    trips = _ceil(n4, 512)
    live = trips > 0 and n4 - 512 * (trips - 1) > 256
    return n4, trips, live, HW - 4 * n4


def column_sum_slabs(rows, cols):
    """(slabs, rows per slab): small_ops.hip:329-336 column_sum_slabs, :381 per = (rows + slabs - 1) / slabs."""
    groups = _ceil(cols, 64)
    if rows < 2048 or groups >= 128:
        return 1, rows
    s = min(256 // groups, rows // 512)
    if s < 2:
        return 1, rows
    return s, _ceil(rows, s)


def row_scale_grid(total4):
    """(workgroups, the grid-stride loop repeats): small_ops.hip:74-78 stream_grid, :62 the loop."""
    blocks = min(8192, max(1, _ceil(total4, 256)))
    return blocks, total4 > blocks * 256


def shuffle_threads(O, H, W):
    """(threads, workgroups) of pixel_shuffle2_kernel per sample: small_ops.hip:221 n = O * H * (W >> 1), :254 grid."""
    n = O * H * (W // 2)
    return n, _ceil(n, 256)


# ---- K13 (csrc/channel_epilogue.hip) --------------------------------------------------------------------------------
def epilogue_lp_trips(HW):
    """(trips, per unrolled slot "none" | "some" | "all" of the last trip's active lanes clamped): channel_epilogue.hip:109 n4 = HW >> 2,
    :111 for (i0 = threadIdx.x; i0 < n4; i0 += 256 * UN), :115 i = min(i0 + 256 * u, n4 - 1)."""
    n4 = HW // 4
    trips = _ceil(n4, 1024)
    base = 1024 * (trips - 1)
    active = min(256, n4 - base)
    slots = []
    for u in range(4):
        clamped = sum(1 for t in range(active) if base + t + 256 * u > n4 - 1)
        slots.append("none" if clamped == 0 else "all" if clamped == active else "some")
    return trips, tuple(slots)


def epilogue_fp32_shape(HW):
    """(float4 per plane, scalar tail): channel_epilogue.hip:39 n4 = ((HW & 3) == 0) ? HW >> 2 : 0, :53 the tail loop."""
    n4 = HW // 4 if HW % 4 == 0 else 0
    return n4, HW - 4 * n4


# ---- K17 (csrc/gelu_pool.hip) ---------------------------------------------------------------------------------------
def gelu_pool_geometry(B, H, W, d, r):
    """dict(per, cells, dead, wgs, last_live, supported): gelu_pool.hip:111 per = r * q, :112 per > 256 refused, :113 cells = 256 / per,
    :114-115 ncell = B * PH * PW, grid ceil(ncell / cells); :44 live = cl < cells && cell < ncell."""
    per = r * (d // 4)
    ok = d % 4 == 0 and H % r == 0 and W % r == 0 and 0 < per <= 256
    if not ok:
        return dict(per=per, supported=False)
    cells = 256 // per
    ncell = B * (H // r) * (W // r)
    wgs = _ceil(ncell, cells)
    return dict(per=per, cells=cells, dead=256 - cells * per, wgs=wgs, last_live=ncell - (wgs - 1) * cells, supported=True)


# =====================================================================================================================
# cases
# =====================================================================================================================
XScanCase = collections.namedtuple("XScanCase", "op HW CB")               # op: scan (nblk 1) | merge | bc (dt_rank 3, d_state 16); B = 2
IScanCase = collections.namedtuple("IScanCase", "op L K CB dims")         # op: scan | scanblk | merge | bc (CB is R); dims: scan_orders_3d
MoveCase = collections.namedtuple("MoveCase", "op R C")                   # op: plain | half | into; B = 3
ShufCase = collections.namedtuple("ShufCase", "op O H W I")               # op: fwd | inv | convt (I input channels); B = 2
SumCase = collections.namedtuple("SumCase", "op B C HW")                  # channel_sum through: bias | epi
ColCase = collections.namedtuple("ColCase", "rows cols wide")
ResidCase = collections.namedtuple("ResidCase", "per scales")
LambdaCase = collections.namedtuple("LambdaCase", "n dot")
EpiCase = collections.namedtuple("EpiCase", "HW act bias res scale")      # B = 2, C = 3; act: none | gelu
EpiLpCase = collections.namedtuple("EpiLpCase", "HW xdt rdt ydt bias act")   # rdt: none | fp32 | same; ydt: same | fp32
PoolCase = collections.namedtuple("PoolCase", "B H W d r via scale")      # via: block (a column block of a row 3 d wide) | split (split_cols)

XS_B, XS_R, XS_N = 2, 3, 16
XS_PER = XS_R + 2 * XS_N                             # 35 columns per direction of the x_proj output
XS_GEOMETRIES = [
    # maps                                 CB of scan and merge      what it reaches
    (((16, 16),), (32,)),                                          # one tile, one channel block, vec4
    (((20, 36),), (36, 96)),                                       # vec4, ragged in both axes
    (((17, 33),), (3, 96)),                                        # scalar, one past a tile
    (((6, 8),), (16,)),                                            # scalar through H alone (W and Lc are multiples of 4)
    (((8, 6),), (3,)),                                             # ... through W alone
    (((5, 3),), (16,)),
    (((1, 1),), (96,)),
    (((1, 64),), (3,)),
    (((64, 1),), (36,)),
    (((8, 8), (6, 6), (4, 4)), (96,)),                             # vec4 / scalar / vec4 in one launch, Lc = 116
    (((6, 6), (8, 8)), (16,)),                                     # a vec4 scale at a non-zero 4-aligned offset
    (((5, 5), (8, 8)), (32,)),                                     # an 8 x 8 scale forced scalar by its offset
    (((8, 8), (3, 3)), (36,)),                                     # all scales scalar through Lc % 4
    (((32, 32), (16, 16), (8, 8), (4, 4)), (96, 3)),               # four scales, tile0 lookups
]
XS_BC_GEOMETRIES = [((16, 16),), ((17, 33),), ((8, 8), (6, 6), (4, 4))]
XSCAN_CASES = [XScanCase(op, hw, cb) for hw, cbs in XS_GEOMETRIES for cb in cbs for op in ("scan", "merge")] + \
    [XScanCase("bc", hw, XS_N) for hw in XS_BC_GEOMETRIES]

IS_B = 2
IS_LENGTHS = (1, 63, 64, 65, 129)
IS_FORMS = ((12, 4), (12, 5), (3, 64), (1, 8), (2, 1), (12, 20))
ISCAN_CASES = [IScanCase(op, L, K, CB, None) for op in ("scan", "merge") for L in IS_LENGTHS for K, CB in IS_FORMS] + \
    [IScanCase(op, L, K, 64, None) for op in ("scan", "merge") for L, K in ((33, 3), (32, 3))] + \
    [IScanCase(op, 65, 2, 512, None) for op in ("scan", "merge")] + \
    [IScanCase(op, 60, 12, 4, (3, 4, 5)) for op in ("scan", "merge")] + \
    [IScanCase("scanblk", 65, 12, 4, None), IScanCase("scanblk", 129, 3, 64, None), IScanCase("scanblk", 63, 2, 1, None)] + \
    [IScanCase("bc", L, K, R, None) for L, K, R in ((65, 12, 1), (129, 12, 3), (63, 2, 20), (64, 1, 3))]
IS_BLK_PAD, IS_COL0 = 5, 3                           # scanblk: direction k reads columns [3 + k * (CB + 5), ... + CB): index_scan(wide, idx, 4, 9, 3)

MOVE_B = 3
MOVE_SHAPES = [(64, 64), (63, 65), (65, 63), (1, 1), (1, 130), (130, 1), (4, 4), (3, 8), (8, 3), (128, 48)]
MOVE_PAD, MOVE_C0 = 8, 4                             # into: the channels [4, 4 + C) of a (B, C + 8, R) map
MOVE_CASES = [MoveCase("plain", R, C) for R, C in MOVE_SHAPES] + [MoveCase("half", R, C) for R, C in MOVE_SHAPES if R % 4 == 0] + \
    [MoveCase("into", R, C) for R, C in MOVE_SHAPES]

SHUF_B = 2
SHUF_SHAPES = [(1, 1, 2), (3, 5, 34), (2, 64, 4), (2, 1, 256), (1, 257, 2)]          # O * H * W / 2 = 1, 255, 256, 256, 257
SHUF_CASES = [ShufCase(op, O, H, W, 0) for op in ("fwd", "inv") for O, H, W in SHUF_SHAPES] + \
    [ShufCase("convt", 8, 8, 16, 32), ShufCase("convt", 4, 8, 12, 16)]

SUM_CASES = [SumCase("bias", *s) for s in [(1, 1, 1), (16, 63, 3), (17, 64, 1020), (33, 65, 1023), (1, 65, 1024), (16, 1, 1028),
                                           (17, 63, 2048), (33, 64, 2052)]] + \
    [SumCase("epi", *s) for s in [(17, 65, 1028), (1, 64, 2052), (33, 1, 1023), (16, 63, 1024)]]

COL_CASES = [ColCase(r, c, False) for r, c in [(1, 1), (16, 63), (17, 64), (2047, 65), (2048, 384), (2049, 1), (2561, 63), (2048, 64),
                                               (2049, 65), (2047, 384), (2048, 8128), (2048, 8129)]] + \
    [ColCase(r, c, True) for r, c in [(17, 65), (2049, 64), (2561, 384)]]

RESID_BIG = 4 * (8192 * 128 + 129)                   # two samples of it: 258 float4 past 8192 workgroups x 256
RESID_CASES = [ResidCase(4, (0.0, 1.25, 0.7)), ResidCase(1776, (0.0, 1.25, 1.25, 0.0, 0.3)), ResidCase(RESID_BIG, (0.0, 1.25))]

LAMBDA_INIT, LAMBDA_DY = 0.8, 1.7
LAMBDA_CASES = [LambdaCase(n, dot) for n in (1, 24, 63, 64, 65, 130) for dot in (1.0, 8.0)]

EPI_B, EPI_C = 2, 3
EPI_CASES = [EpiCase(1028, act, b, r, 1.0) for act in ("none", "gelu") for b in (True, False) for r in (True, False)] + \
    [EpiCase(1, "gelu", True, True, 1.0), EpiCase(1, "none", True, False, 1.0), EpiCase(45, "gelu", True, False, 1.0),
     EpiCase(45, "none", False, True, 1.0), EpiCase(1020, "gelu", False, True, 1.0), EpiCase(1020, "none", True, True, 1.0),
     EpiCase(1024, "gelu", True, True, 1.0), EpiCase(1024, "none", True, False, 1.0), EpiCase(1028, "gelu", True, True, 3.0)]

EPILP_SIZES = (4, 1020, 1024, 1028, 4092, 4096, 4100)
EPILP_COMBOS = [(x, r, y, b, a) for x in ("bf16", "fp16") for r in ("none", "fp32", "same") for y in ("same", "fp32") for b in (True, False)
                for a in ("none", "gelu")]
EPILP_CASES = [EpiLpCase(EPILP_SIZES[i % len(EPILP_SIZES)], *c) for i, c in enumerate(EPILP_COMBOS)]

POOL_CASES = [PoolCase(2, 16, 16, 48, 8, "block", 2.0),          # per = 96
              PoolCase(2, 4, 4, 4, 1, "block", 2.0),             # per = 1, 256 cells
              PoolCase(2, 6, 9, 20, 3, "block", 2.0),            # per = 15, cells = 17, one dead lane
              PoolCase(3, 12, 9, 20, 3, "block", 2.0),           # ... three workgroups, the last with 2 of 17 cells
              PoolCase(2, 8, 8, 128, 8, "block", 2.0),           # per = 256
              PoolCase(2, 2, 6, 1024, 1, "block", 2.0),          # per = 256 with r = 1
              PoolCase(2, 8, 12, 96, 4, "block", 2.0),           # non-square
              PoolCase(1, 2, 2, 8, 2, "block", 2.0),             # one cell
              PoolCase(2, 8, 12, 96, 4, "split", 2.0),           # the gradient goes into a split_cols slot: ds_stride > d
              PoolCase(2, 16, 16, 48, 8, "block", 6.0)]          # inputs x 6

# refusals the host code decides before any launch: (op, arguments)
REFUSALS = [("gelu_pool", (8, 8, 192, 8)), ("index_scan", 513), ("scaled_residual", 6), ("pixel_shuffle2", (1, 2, 3))]

CASES = {"xscan": XSCAN_CASES, "iscan": ISCAN_CASES, "move": MOVE_CASES, "shuf": SHUF_CASES, "sum": SUM_CASES, "col": COL_CASES,
         "resid": RESID_CASES, "lambda": LAMBDA_CASES, "epi": EPI_CASES, "epilp": EPILP_CASES, "pool": POOL_CASES}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def family(case):
    return type(case).__name__[:-4].lower()


def case_id(case):
    def one(v):
        if isinstance(v, tuple):
            return "x".join(one(i) for i in v) if v and isinstance(v[0], tuple) else "x".join(str(i) for i in v)
        if isinstance(v, bool):
            return "T" if v else "F"
        return str(v)
    return "-".join(one(v) for v in case)


def xscan_len(case):
    return sum(h * w for h, w in case.HW)


def iscan_orders(case):
    """(K, L) int64 scan orders: a random permutation per direction (the kernels accept any), or the 12 axis orders of a D x H x W volume
    (what ss3d.scan_orders_3d builds: 0 dhw, 1 dwh, 2 hdw, 3 hwd, 4 wdh, 5 whd, 6 .. 11 their reversals)."""
    if case.dims is not None:
        nat = torch.arange(case.L).view(*case.dims)
        fwd = [nat.permute(*p).reshape(-1) for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))]
        return torch.stack(fwd + [t.flip(0) for t in fwd])
    g = torch.Generator().manual_seed(zlib.crc32(repr(tuple(case)).encode()) ^ 0x5EED)
    return torch.stack([torch.randperm(case.L, generator=g) for _ in range(case.K)])


def iscan_layout(case):
    """(row width, column stride between directions, first column) of the token-major source of scan / scanblk / bc."""
    if case.op == "scanblk":
        return case.K * (case.CB + IS_BLK_PAD), case.CB + IS_BLK_PAD, IS_COL0
    if case.op == "bc":
        return case.K * (case.CB + 2), case.CB + 2, 0
    return case.CB, 0, 0


def epilp_types(case):
    """(x, res or None, y) element types."""
    x = DTYPES[case.xdt]
    return x, {"none": None, "fp32": torch.float32, "same": x}[case.rdt], (x if case.ydt == "same" else torch.float32)


# =====================================================================================================================
# inputs: float32 host tensors by name; the cotangent of output "y" is "d_y"
# =====================================================================================================================
def _lambda_pair(g, n, dot):
    q = torch.randn(n, generator=g)
    k = 0.5 * q + 0.1 * torch.randn(n, generator=g)
    s = float((q.double() * k.double()).sum())
    f = (dot / abs(s)) ** 0.5
    return q * f, k * (f if s > 0 else -f)


def inputs(case):
    g = _gen(case)
    rn = lambda *s: torch.randn(*s, generator=g)                                                      # noqa: E731
    fam = family(case)
    if fam == "xscan":
        B, Lc, CB = XS_B, xscan_len(case), case.CB
        if case.op == "scan":
            return dict(tok=rn(B, Lc, CB), d_seq=rn(B, 4 * CB, Lc))
        if case.op == "merge":
            return dict(seq=rn(B, 4 * CB, Lc), d_tok=rn(B, Lc, CB))
        return dict(xdbl=rn(B, Lc, 4 * XS_PER), d_dtr=rn(B, 4, XS_R, Lc), d_Bs=rn(B, 4, XS_N, Lc), d_Cs=rn(B, 4, XS_N, Lc))
    if fam == "iscan":
        B, L, K, CB = IS_B, case.L, case.K, case.CB
        width = iscan_layout(case)[0]
        if case.op in ("scan", "scanblk"):
            return dict(tok=rn(B, L, width), d_seq=rn(B, K * CB, L))
        if case.op == "merge":
            return dict(seq=rn(B, K * CB, L), d_tok=rn(B, L, CB))
        return dict(xdbl=rn(B, L, width), d_dtr=rn(B, K, CB, L), d_Bs=rn(B, K, L), d_Cs=rn(B, K, L))
    if fam == "move":
        return dict(x=rn(MOVE_B, case.R, case.C))
    if fam == "shuf":
        O, H, W = case.O, case.H, case.W
        if case.op == "fwd":
            return dict(x=rn(SHUF_B, 4 * O, H, W))
        if case.op == "inv":
            return dict(x=rn(SHUF_B, O, 2 * H, 2 * W))
        return dict(x=rn(SHUF_B, case.I, H, W), w=rn(case.I, O, 2, 2) * case.I ** -0.5, d_y=rn(SHUF_B, O, 2 * H, 2 * W))
    if fam == "sum":
        shape = (case.B, case.C, case.HW, 1)
        return dict(x=rn(*shape), bias=rn(case.C), d_y=rn(*shape))
    if fam == "col":
        return dict(x=rn(case.rows, case.cols))
    if fam == "resid":
        shape = (len(case.scales), case.per // 4, 4)
        return dict(skip=rn(*shape), branch=rn(*shape), d_y=rn(*shape))
    if fam == "lambda":
        q1, k1 = _lambda_pair(g, case.n, case.dot)
        q2, k2 = _lambda_pair(g, case.n, 0.9 * case.dot)
        return dict(q1=q1, k1=k1, q2=q2, k2=k2)
    if fam == "epi":
        shape = (EPI_B, EPI_C, 1, case.HW)
        t = dict(x=rn(*shape) * case.scale, d_y=rn(*shape))
        if case.bias:
            t["bias"] = rn(EPI_C)
        if case.res:
            t["res"] = rn(*shape)
        return t
    if fam == "epilp":
        xdt, rdt, ydt = epilp_types(case)
        shape = (EPI_B, EPI_C, 1, case.HW)
        t = dict(x=rn(*shape).to(xdt).float(), d_y=rn(*shape).to(ydt).float())   # 16-bit maps: the values the device holds, widened
        if case.bias:
            t["bias"] = rn(EPI_C)
        if rdt is not None:
            t["res"] = rn(*shape).to(rdt).float()
        return t
    if fam == "pool":
        B, N, d = case.B, case.H * case.W, case.d
        return dict(s=rn(B, N, d) * case.scale, d_pooled=rn(B, (case.H // case.r) * (case.W // case.r), d))
    raise ValueError(fam)


LEAVES = {"xscan": ("tok", "seq", "xdbl"), "iscan": ("tok", "seq", "xdbl"), "move": (), "shuf": ("x", "w"), "sum": ("x", "bias"), "col": (),
          "resid": ("skip", "branch"), "lambda": ("q1", "k1", "q2", "k2"), "epi": ("x", "bias", "res"), "epilp": ("x", "bias", "res"),
          "pool": ("s",)}


# =====================================================================================================================
# the ops as plain torch compositions
# =====================================================================================================================
def xscan_sequences(tok, HW):
    """(B, L_cat, C) token-major maps -> (B, 4, C, L_cat): per scale the map row-major, column-major (transpose) and the two flips,
    the scales concatenated in the same order for every direction."""
    B, _, C = tok.shape
    dirs, off = [[], [], [], []], 0
    for H, W in HW:
        x = tok[:, off:off + H * W].transpose(1, 2).reshape(B, C, H, W)
        hw, wh = x.flatten(2), x.transpose(2, 3).flatten(2)
        for k, s in enumerate((hw, wh, hw.flip(-1), wh.flip(-1))):
            dirs[k].append(s)
        off += H * W
    return torch.stack([torch.cat(d, -1) for d in dirs], 1)


def xscan_merge(seq, HW, order=0):
    """(B, 4 * C, L_cat) -> (B, L_cat, C): every direction's rows put back on their tokens -- the inverse placement of
    `xscan_sequences`, written out per direction -- and the four summed (order 0: ((0 + 1) + 2) + 3; order 1: (3 + 2) + (1 + 0))."""
    B, rows, _ = seq.shape
    C = rows // 4
    s4 = seq.reshape(B, 4, C, -1)
    out, off = [], 0
    for H, W in HW:
        p = [s4[:, k, :, off:off + H * W] for k in range(4)]
        d = [p[0].reshape(B, C, H, W), p[1].reshape(B, C, W, H).transpose(2, 3), p[2].flip(-1).reshape(B, C, H, W),
             p[3].flip(-1).reshape(B, C, W, H).transpose(2, 3)]
        m = ((d[0] + d[1]) + d[2]) + d[3] if order == 0 else (d[3] + d[2]) + (d[1] + d[0])
        out.append(m.flatten(2).transpose(1, 2))
        off += H * W
    return torch.cat(out, 1)


def pixel_shuffle2(z):
    """y[b][o][2 i + a][2 j + c] = z[b][(2 a + c) O + o][i][j] (the header comment of the kernel)."""
    B, O4, H, W = z.shape
    O = O4 // 4
    y = z.new_zeros(B, O, 2 * H, 2 * W)
    for a in range(2):
        for c in range(2):
            y[:, :, a::2, c::2] = z[:, (2 * a + c) * O:(2 * a + c + 1) * O]
    return y


def pixel_unshuffle2(y):
    """z[b][(2 a + c) O + o][i][j] = y[b][o][2 i + a][2 j + c]."""
    return torch.cat([y[:, :, a::2, c::2] for a in range(2) for c in range(2)], 1)


def _lambda_dot(q, k, order):
    p = q * k
    if order == 0:
        return p.sum()
    if order == 1:                                                               # one term after the other, from the end
        return p.flip(0).cumsum(0)[-1]
    lanes = torch.zeros(64, dtype=p.dtype)                                       # 64 strided partial sums, then a tree over them
    for i in range(0, p.numel(), 64):
        c = p[i:i + 64]
        lanes = lanes + F.pad(c, (0, 64 - c.numel()))
    while lanes.numel() > 1:
        lanes = lanes[:lanes.numel() // 2] + lanes[lanes.numel() // 2:]
    return lanes[0]


def compose(case, t, order=0):
    """{output name: tensor} from the tensors `t` (any floating type).  `order` picks another, equally valid summation order where
    the op sums (the merges, diff_lambda)."""
    fam = family(case)
    if fam == "xscan":
        if case.op == "scan":
            B = t["tok"].shape[0]
            return dict(seq=xscan_sequences(t["tok"], case.HW).reshape(B, 4 * case.CB, -1))
        if case.op == "merge":
            return dict(tok=xscan_merge(t["seq"], case.HW, order))
        s = xscan_sequences(t["xdbl"], case.HW)                                  # (B, 4, 140, Lc): direction k keeps its own 35 columns
        pick = lambda c0, n: torch.stack([s[:, k, XS_PER * k + c0:XS_PER * k + c0 + n] for k in range(4)], 1)     # noqa: E731
        return dict(dtr=pick(0, XS_R), Bs=pick(XS_R, XS_N), Cs=pick(XS_R + XS_N, XS_N))
    if fam == "iscan":
        idx = iscan_orders(case)
        K, CB = case.K, case.CB
        _, blk, col0 = iscan_layout(case)
        if case.op in ("scan", "scanblk"):
            tok = t["tok"]
            return dict(seq=torch.stack([tok[:, idx[k], col0 + k * blk:col0 + k * blk + CB].transpose(1, 2) for k in range(K)], 1)
                        .reshape(tok.shape[0], K * CB, case.L))
        if case.op == "merge":
            seq = t["seq"]
            out = seq.new_zeros(seq.shape[0], case.L, CB)
            for k in (range(K) if order == 0 else reversed(range(K))):
                out = out.index_add(1, idx[k], seq[:, k * CB:(k + 1) * CB].transpose(1, 2))
            return dict(tok=out)
        x = t["xdbl"]
        rows = lambda c: torch.stack([x[:, idx[k], k * blk + c] for k in range(K)], 1)                 # noqa: E731  (B, K, L)
        return dict(dtr=torch.stack([rows(r) for r in range(CB)], 2), Bs=rows(CB), Cs=rows(CB + 1))
    if fam == "move":
        return dict(y=t["x"].transpose(1, 2).contiguous())
    if fam == "shuf":
        if case.op == "fwd":
            return dict(y=pixel_shuffle2(t["x"]))
        if case.op == "inv":
            return dict(y=pixel_unshuffle2(t["x"]))
        return dict(y=F.conv_transpose2d(t["x"], t["w"], None, 2))
    if fam == "sum":
        return dict(y=t["x"] + t["bias"].view(1, -1, 1, 1))
    if fam == "col":
        return dict(sum=t["x"].sum(0))
    if fam == "resid":
        scale = torch.tensor(case.scales, dtype=t["skip"].dtype).view(-1, *([1] * (t["skip"].dim() - 1)))
        y = t["skip"] + t["branch"] * scale
        zero = [i for i, s in enumerate(case.scales) if s == 0.0]
        return dict(y=y, y_zero=y[zero])
    if fam == "lambda":
        return dict(lam=torch.exp(_lambda_dot(t["q1"], t["k1"], order)) - torch.exp(_lambda_dot(t["q2"], t["k2"], order)) + LAMBDA_INIT)
    if fam in ("epi", "epilp"):
        pre = t["x"]
        if "bias" in t:
            pre = pre + t["bias"].view(1, -1, 1, 1)
        if "res" in t:
            pre = pre + t["res"]
        return dict(y=F.gelu(pre) if case.act == "gelu" else pre * 1.0)
    if fam == "pool":
        B, H, W, d, r = case.B, case.H, case.W, case.d, case.r
        img = F.gelu(t["s"]).reshape(B, H, W, d).permute(0, 3, 1, 2)
        return dict(pooled=F.adaptive_avg_pool2d(img, (H // r, W // r)).flatten(2).transpose(1, 2))
    raise ValueError(fam)


def evaluate(case, dtype=torch.float64, order=0, absolute=False):
    """{quantity: tensor of `dtype`}: every output of `compose` and the gradient of every leaf ("d" + its name), on the host.
    absolute: from the absolute values of all inputs -- for the ops that only move and add, the sum of |terms| behind every element."""
    inp = inputs(case)
    t = {k: (v.abs() if absolute else v).to(dtype) for k, v in inp.items()}
    leaves = [k for k in LEAVES[family(case)] if k in t]
    for k in leaves:
        t[k].requires_grad_(True)
    outs = compose(case, t, order)
    cot = {"lam": torch.tensor(LAMBDA_DY, dtype=dtype)} if family(case) == "lambda" else {k: t["d_" + k] for k in outs if "d_" + k in t}
    if leaves and cot:
        torch.autograd.backward([outs[k] for k in cot], [cot[k] for k in cot])
    res = {k: v.detach() for k, v in outs.items()}
    res.update({"d" + k: t[k].grad for k in leaves if cot})
    return res


@functools.lru_cache(maxsize=2)
def reference_and_yardstick(case):
    """(float64 reference, [plain-fp32 yardsticks]) of a case; computed once, never modified.  diff_lambda has three yardsticks, one per
    summation order; every other op one."""
    orders = (0, 1, 2) if family(case) == "lambda" else (0,)
    return evaluate(case, torch.float64), [evaluate(case, torch.float32, o) for o in orders]


def aux(case, ref):
    """{quantity: tensor} the element-wise bounds are made of: sum |terms| for "sum", |skip| + |branch * scale| for "resid"."""
    fam = family(case)
    if fam in ("xscan", "iscan"):
        return evaluate(case, torch.float64, absolute=True)
    if fam == "resid":
        t = {k: v.double() for k, v in inputs(case).items()}
        scale = torch.tensor(case.scales, dtype=torch.float64).view(-1, *([1] * (t["skip"].dim() - 1)))
        return dict(y=t["skip"].abs() + (t["branch"] * scale).abs(), dbranch=(t["d_y"] * scale).abs())
    return {}


# =====================================================================================================================
# tolerances
# =====================================================================================================================
# ("equal", 0, 0):  got == ref bit for bit;
# ("sum", n, 0):    |got - ref| <= (n - 1) * 2^-24 * aux element-wise, aux = sum |terms|;
# ("resid", 2, 0):  |got - ref| <= 2 * 2^-24 * aux element-wise;
# ("close", a, r):  |got - ref| <= a * max(1, max |ref|) + r * |ref| element-wise (_close of tests/test_blocks_gpu.py);
# ("max", a, c):    max |got - ref| <= a * max |ref| + c.
Tol = collections.namedtuple("Tol", "kind a r widen")
EQUAL = Tol("equal", 0.0, 0.0, False)


def _sum(n):
    return Tol("sum", float(n), 0.0, False)


def tolerances(case):
    """{quantity: Tol}: exact / derived bounds for the data movement and the fixed-count sums, else the bound of the op's existing
    parity test (named in the comments)."""
    fam = family(case)
    c = lambda a, r, widen=False: Tol("close", a, r, widen)                                           # noqa: E731
    m = lambda a, cst, widen=False: Tol("max", a, cst, widen)                                         # noqa: E731
    if fam == "xscan":
        if case.op == "scan":
            return dict(seq=EQUAL, dtok=_sum(4))
        if case.op == "merge":
            return dict(tok=_sum(4), dseq=EQUAL)
        return dict(dtr=EQUAL, Bs=EQUAL, Cs=EQUAL, dxdbl=EQUAL)
    if fam == "iscan":
        if case.op == "scan":
            return dict(seq=EQUAL, dtok=_sum(case.K) if case.K > 1 else EQUAL)
        if case.op == "merge":
            return dict(tok=_sum(case.K) if case.K > 1 else EQUAL, dseq=EQUAL)
        if case.op == "scanblk":
            return dict(seq=EQUAL, dtok=EQUAL)
        return dict(dtr=EQUAL, Bs=EQUAL, Cs=EQUAL, dxdbl=EQUAL)
    if fam == "move":
        return dict(y=EQUAL)
    if fam == "shuf":
        if case.op == "convt":                                                    # test_transposed_2x2_stride2_convolution_on_k18
            return dict(y=m(2e-6, 0.0), dx=m(2e-6, 0.0), dw=m(2e-6, 0.0))
        return dict(y=EQUAL)
    if fam == "sum":
        if case.op == "bias":                                                     # test_channel_bias_and_column_sum
            return dict(y=c(1e-5, 0.0), dx=EQUAL, dbias=c(1e-4, 0.0, True))
        return dict(y=c(1e-5, 1e-5), dx=c(1e-5, 1e-5), dbias=c(2e-4, 1e-4, True))      # test_channel_epilogue_matches_torch
    if fam == "col":                                                              # test_channel_bias_and_column_sum: 1e-4, 2e-3 with slabs
        return dict(sum=m(0.0, 2e-3 if case.rows >= 2048 else 1e-4, True))
    if fam == "resid":
        return dict(y=Tol("resid", 2.0, 0.0, False), y_zero=EQUAL, dskip=EQUAL, dbranch=Tol("resid", 2.0, 0.0, False))
    if fam == "lambda":                                                           # test_diff_lambda_matches_torch: 1e-6 absolute
        return {q: m(0.0, 1e-6, True) for q in ("lam", "dq1", "dk1", "dq2", "dk2")}
    if fam == "epi":                                                              # test_channel_epilogue_matches_torch
        return dict(y=c(1e-5, 1e-5), dx=c(1e-5, 1e-5), dres=c(1e-5, 1e-5), dbias=c(2e-4, 1e-4, True))
    if fam == "epilp":                                                            # test_channel_epilogue_16_bit_maps
        e16 = 2.0 ** -8 if case.xdt == "bf16" else 2.0 ** -11
        two = m(2 * e16, 1e-6)                                                    # two roundings of the 16-bit type
        exact_res = case.act == "none" and case.rdt == "fp32"                     # d(res) = dy itself
        return dict(y=m((e16 if case.ydt == "same" else 1e-6) * 1.01, 1e-6), dx=two, dres=m(0.0, 1e-6) if exact_res else two,
                    dbias=m(1e-4, 1e-4, True))
    if fam == "pool":                                                             # test_gelu_pool_matches_torch
        return dict(pooled=c(2e-6, 1e-5), ds=c(2e-6, 1e-5))
    raise ValueError(fam)


def error(got, ref, tol, bound=None):
    """(error in the scale of `tol`, largest excess of |got - ref| over what `tol` allows): passes when excess <= 0.  `bound`: the
    `aux` tensor of the element-wise kinds."""
    ref = ref.double()
    d = (got.detach().cpu().double() - ref).abs()
    if d.numel() == 0:
        return 0.0, 0.0
    top = float(ref.abs().max())
    if tol.kind == "equal":
        return float(d.max()), float(d.max())
    if tol.kind in ("sum", "resid"):
        allowed = ((tol.a - 1.0) if tol.kind == "sum" else tol.a) * U * bound.double()
        return float(d.max()) / max(float(bound.max()), 1e-30), float((d - allowed).max())
    if tol.kind == "close":
        scale = max(1.0, top)
        return float(d.max()) / scale, float((d - tol.a * scale - tol.r * ref.abs()).max())
    return float(d.max()) / max(top, 1e-30), float(d.max()) - (tol.a * top + tol.r)


def compared(case, ref):
    return [k for k in ref if not k.startswith("_")]


def bounds(case, ref, yards):
    """{quantity: Tol} of the device test: `tolerances`, the quantities behind long fp32 sums widened to 4 x the largest yardstick error
    on this case where that is more (from the host yardsticks, never from the kernel's output)."""
    out = {}
    for q in compared(case, ref):
        tol = tolerances(case)[q]
        if tol.widen:
            tol = tol._replace(a=max(tol.a, 4.0 * max(error(y[q], ref[q], tol)[0] for y in yards)))
        out[q] = tol
    return out
