"""Cases, references and path predicates for the tap-GEMM convolutions -- K15 (csrc/conv_wgrad.hip: the weight gradient and the padded
copies of mlagg_volume_pad), K16 (csrc/conv_taps.hip: forward / data gradient of the 3-D stride-1 layers) and K19t
(csrc/conv3x3_s2t.hip: PatchExpand's transposed convolution and its two gradients) -- at the sizes where their launchers and loops
change slab, tile, tail or guard: shared by tests/test_tap_conv_paths_cpu.py and tests/test_tap_conv_paths_gpu.py.

A CASE is a TapCase (id, family, B, I, O, dims, k, stride, form, sliced).  `family`: "k15" = ops.conv_weight_grad (narrow padded
copies), "k15_nd" = ops.conv_nd where only the weight gradient is this package's (narrow copies made in backward), "k16" = ops.conv_nd
on K16 / K16 / K15 (wide copies shared by the three products), "k19t" = ops.conv3x3_s2t (dims = the INPUT grid; weight (I, O, 3, 3)).
`form` is the operand form of K19t (3 = fp32 as three bf16 pieces, 1 = bf16, 2 = fp16); K15 / K16 multiply fp32 exactly.  `sliced`
("views", K19t): x is a channel block of a wider map and dy the interior view [1:, 1:] of the 2H x 2W padded gradient.  Inputs come
from a generator seeded with the case's shape: unit-variance x and dy, weights scaled by (taps * I) ** -0.5.

`reference(case)` is the convolution and its two gradients in float64 on the host (of the operands rounded to the 16-bit type in forms
1 and 2: the exact products of what the kernel multiplies).  `yardstick(case)` is the same in plain fp32 on the host: it shows how
well conditioned a case is, it is not the truth.  `bounds(case)`, as max |got - ref| over max |ref|, are those an fp32 convolution is
held to in tests/_conv_kernel_cases.py:
    y, dx 2e-6; dW 4e-6 (3-D: 1e-5); the 16-bit forms of K19t 4e-6 against the exact products of the rounded operands
`dw_bound(case, yardstick_error)` widens a summed weight gradient's bound to max(that, 4 x the yardstick's error on the same case) --
two correct fp32 summation orders err independently at the same scale (the rule of tests/_map_kernel_cases.py) -- and never past
the 2e-5 * max + 1e-5 of tests/test_conv_wgrad_gpu.py.  The CPU test holds the yardstick itself inside the UN-widened bound.

PATH PREDICATES are pure functions restating a launcher's or a kernel's decision; each names the source lines it mirrors, and the
CPU test compares them with the library's host queries (mlagg_conv_pad_geometry, mlagg_conv_wgrad_taps_geometry,
mlagg_conv_wgrad_taps_workspace_floats, mlagg_conv_taps_geometry, mlagg_conv3x3_s2t_tile, mlagg_conv3x3_s2t_wgrad_geometry,
mlagg_conv3x3_s2t_wgrad_workspace_floats) over the cases and a sweep.

Plain-fp32 yardstick errors of the compared quantities, largest over the group's cases, measured on the host (16 threads, see
tests/_conv_kernel_cases.py yardstick):

    cases                       y        dx       dW
    k15                         -        -        1.0e-06
    k15_nd                      -        -        7.1e-07
    k16                         7.2e-07  5.7e-07  4.9e-07
    k19t  form 3                1.2e-06  3.7e-07  9.2e-07
    k19t  forms 1, 2            5.7e-07  3.9e-07  5.8e-07
"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

TapCase = collections.namedtuple("TapCase", "id family B I O dims k stride form sliced")
FORM_TYPE = {3: torch.float32, 1: torch.bfloat16, 2: torch.float16}
SLICE_AT, SLICE_EXTRA = 8, 16                        # a sliced x: channels [8, 8 + I) of a map 16 channels wider


def pixels(dims):
    n = 1
    for v in dims:
        n *= v
    return n


def dims3(dims):
    """(D, H, W) of a map: a 2-D one has D = 1 (ops.conv_weight_grad)."""
    return tuple(dims) if len(dims) == 3 else (1,) + tuple(dims)


def out_dims(dims, stride):
    """Output extents of kernel 3 / padding 1 and of kernel 1 / padding 0 alike."""
    return tuple((d - 1) // stride + 1 for d in dims)


# =====================================================================================================================
# path predicates: K15
# =====================================================================================================================
def pad_geometry(D, H, W, stride, wide):
    """(Dq, Hq, Wq, guard) of the padded box, or None where it is refused: mlagg_conv_pad_geometry (conv_wgrad.hip:205-215)."""
    if min(D, H, W) <= 0 or stride not in (1, 2) or (stride == 2 and D == 1) or (wide and (stride != 1 or W % 4)):
        return None
    if stride == 1:
        Dq, Hq, Wq = (1 if D == 1 else D + 2), H + 2, (W + 8 if wide else (W + 2 + 3) & ~3)
    else:
        Dq, Hq, Wq = (D - 1) // 2 + 2, (H - 1) // 2 + 2, ((W - 1) // 2 + 2 + 3) & ~3
    return Dq, Hq, Wq, (Hq * Wq + Wq + 1 + 8 + 7) & ~7


def box_q(D, H, W, stride, wide):
    """(Q, Q8): voxels of the box, and what K15 walks in whole 8-voxel steps (ops._wgrad_from_padded: Q8 = (Q + 7) & ~7; the
    overhang lies in the guard, zero in the copy of dy)."""
    Dq, Hq, Wq, _ = pad_geometry(D, H, W, stride, wide)
    return Dq * Hq * Wq, (Dq * Hq * Wq + 7) & ~7


K15_NT, K15_WAVES, K15_MAX_SLAB, K15_MIN_SLAB = 9, 2048, 8192, 256
K15Geometry = collections.namedtuple("K15Geometry", "slab nslabs ngroups otiles itiles full_steps last_steps last_o last_i rows")


def k15_slab(Q8, waves_per_slab):
    """slab_len (conv_wgrad.hip:248-253): from 8192 halving down to 256 until slabs x (tiles x batch) reach 2048 waves."""
    slab = K15_MAX_SLAB
    while slab > K15_MIN_SLAB and -(-Q8 // slab) * waves_per_slab < K15_WAVES:
        slab >>= 1
    return slab


def k15_tap_groups(ntaps):
    """Live taps `nt` of each tap group (conv_wgrad.hip:56: nt = min(9, ntaps - 9 grp); off[t] clamps to the group's last tap)."""
    return [min(K15_NT, ntaps - t0) for t0 in range(0, ntaps, K15_NT)]


def k15_geometry(batch, Q8, O, I, ntaps):
    """make_tapgeom (conv_wgrad.hip): slab, nslabs, tap groups, channel tiles; the 8-voxel steps of a full slab and of the last one
    (:72 nstep = (q1 - q0) >> 3); live rows of the last channel tile of O and of I (:57 clamps, :110-114 guards); rows = batch *
    nslabs of the reduce kernel."""
    ngroups, otiles, itiles = len(k15_tap_groups(ntaps)), -(-O // 32), -(-I // 32)
    slab = k15_slab(Q8, otiles * itiles * ngroups * batch)
    nslabs = -(-Q8 // slab)
    return K15Geometry(slab, nslabs, ngroups, otiles, itiles, slab // 8, (Q8 - (nslabs - 1) * slab) // 8, O - 32 * (otiles - 1),
                       I - 32 * (itiles - 1), batch * nslabs)


def k15_last_data_voxel(dims, stride):
    """Flat box index of the last voxel of the padded output gradient that is not ring (narrow form; ops._Padded as_output: origin 1,
    0 along z for a map, at stride 1; origin 0 on the phase grid): every A operand of K15 behind it is zero."""
    D, H, W = dims3(dims)
    _, Hq, Wq, _ = pad_geometry(D, H, W, stride, False)
    oD, oH, oW = out_dims((D, H, W), stride)
    if stride == 1:
        return ((oD - 1 + (0 if D == 1 else 1)) * Hq + oH) * Wq + oW
    return ((oD - 1) * Hq + oH - 1) * Wq + oW - 1


def k15_tail(nstep):
    """Which way a slab of `nstep` steps leaves the double-buffered loop (conv_wgrad.hip:88-104): "one" = consume(0) alone, "two" = the
    fetch(1) tail without a loop trip, "odd" = loop trips then consume(0), "even" = loop trips then the fetch(1) tail."""
    return {1: "one", 2: "two"}.get(nstep, "odd" if nstep % 2 else "even")


def k15_reduce_shapes(rows):
    """{(pairs, tail)} over the 16 row groups of conv_wgrad_reduce_kernel (conv_wgrad.hip:130-135): group rg adds the row pairs
    (r, r + 16), r = rg, rg + 32, .. while r + 16 < rows, then one more row if r < rows."""
    shapes = set()
    for rg in range(16):
        r, pairs = rg, 0
        while r + 16 < rows:
            pairs, r = pairs + 1, r + 32
        shapes.add((pairs, int(r < rows)))
    return shapes


def k15_reduce_last_block(ntaps, O, I):
    """Live columns of the reduce kernel's last 64-column block (conv_wgrad.hip:127-129: c < n), 0 = full."""
    return ntaps * O * I % 64


# =====================================================================================================================
# path predicates: K16
# =====================================================================================================================
K16_WG_VOX, K16_CCH = 512, 32
K16Geometry = collections.namedtuple("K16Geometry", "Q nwg past otiles last_o chunks last_chunk odd_clamp lds big_lds")


def k16_geometry(O, I, D, H, W, ntaps):
    """make_cgeom (conv_taps.hip) and what conv_taps_kernel makes of it: the box Q of the wide form; workgroups of 512 voxels and how
    many of the last one's positions lie past Q (:64 clamps their loads); 32-row output tiles and the live rows of the last (:71, :114);
    contraction chunks of 32 with the live channels of the last; whether the kh = 1 lane of the last pair clamps (:80, odd I); bytes
    of the LDS weight image and whether they pass 48 KiB (the hipFuncSetAttribute branch)."""
    Dq, Hq, Wq, _ = pad_geometry(D, H, W, 1, True)
    Q = Dq * Hq * Wq
    nwg, otiles, chunks = -(-Q // K16_WG_VOX), -(-O // 32), -(-I // K16_CCH)
    lds = ntaps * K16_CCH * 32 * 4
    return K16Geometry(Q, nwg, nwg * K16_WG_VOX - Q, otiles, O - 32 * (otiles - 1), chunks, I - K16_CCH * (chunks - 1), I % 2 == 1, lds,
                       lds > 48 * 1024)


def k16_inside(D, H, W):
    """[flat padded index qg of every 4-voxel lane group inside the data box] (conv_taps.hip:104-108), in kernel order."""
    Dq, Hq, Wq, _ = pad_geometry(D, H, W, 1, True)
    orgz, inside = (0 if D == 1 else 1), []
    for qg in range(0, Dq * Hq * Wq, 4):
        xq, r1 = qg % Wq, qg // Wq
        yq, zq = r1 % Hq, r1 // Hq
        if 4 <= xq < W + 4 and 1 <= yq <= H and orgz <= zq < orgz + D:
            inside.append(qg)
    return inside


# =====================================================================================================================
# path predicates: K19t
# =====================================================================================================================
def k19t_tile(R):
    """TO of s2t_gemm_kernel: gemm_tile (conv3x3_s2t.hip): 64-row tiles iff R % 64 == 0; R = O forward, I for the data gradient."""
    return 2 if R % 64 == 0 else 1


K19tGemm = collections.namedtuple("K19tGemm", "to tiles last_rows nblk loop wgs last_wg last_wave split")


def k19t_gemm(mode, O, I, P, form):
    """The forward (mode 0) / data-gradient (mode 1) launch (conv3x3_s2t.hip gemm, launch_gemm, s2t_gemm_kernel): TO; row tiles and the
    live rows of the last (:121 clamps the weight rows of a half-empty tile); nblk = K / 16 and the loop shape (:185-196: "tail" = 1,
    "pair" = 2, "pair+tail" = 3, else by parity); workgroups of 128 pixels, the pixels of the last workgroup and of the last wave with
    any (:78 clamps, :199 returns); whether the five small products have accumulators of their own (:83 SPLIT: six terms and NC * TO
    <= 4 with NC = 4 forward, 1 data gradient)."""
    R, K = (I, O) if mode else (O, I)
    to = k19t_tile(R)
    tiles, nblk = -(-R // (32 * to)), K // 16
    loop = {1: "tail", 2: "pair", 3: "pair+tail"}.get(nblk, "pairs+tail" if nblk % 2 else "pairs")
    wgs, waves = -(-P // 128), -(-P // 32)
    split = form == 3 and (1 if mode else 4) * to <= 4
    return K19tGemm(to, tiles, R - 32 * to * (tiles - 1), nblk, loop, wgs, P - 128 * (wgs - 1), P - 32 * (waves - 1), split)


K19T_WAVES, K19T_MIN_PER_PART, K19T_CAP_BYTES = 2048, 4, 256 << 20
K19tWgrad = collections.namedtuple("K19tWgrad", "cw per_part nparts last_part last_block half1 capped clamped")


def k19t_wgrad_geometry(B, O, I, H, W):
    """make_swgeom (conv3x3_s2t.hip:324-340): cw = ceil(W / 16) blocks per row; per_part blocks per partial sum (about 2048 waves in
    all, partial sums under 256 MB, at least 4) and nparts per sample; the blocks of the last part; the live pixels of a row's last
    block and of its kh = 1 half (:263-268: lanes 32.. own pixels 8..15 of the block); whether the cap, whether the floor of 4 set
    per_part."""
    cw = -(-W // 16)
    nb, tiles = H * cw, -(-O // 32) * -(-I // 32)
    want = -(-K19T_WAVES // (B * tiles))
    cap = K19T_CAP_BYTES // (4 * 9 * O * I) // B
    per_sample = max(1, min(want, cap))
    per = -(-nb // per_sample)
    per_part = max(per, K19T_MIN_PER_PART)
    nparts = -(-nb // per_part)
    last_block = W - 16 * (cw - 1)
    return K19tWgrad(cw, per_part, nparts, nb - per_part * (nparts - 1), last_block, max(0, last_block - 8), cap < want, per < K19T_MIN_PER_PART)


def k19t_padding_rows(H, m):
    """Kernel rows ky whose dy row 2m - 1 + ky is padding for input row m (conv3x3_s2t.hip:274-275, uniform branch)."""
    return tuple(ky for ky in range(3) if not 0 <= 2 * m - 1 + ky < 2 * H - 1)


# =====================================================================================================================
# cases
# =====================================================================================================================
def _case(id, family, B, I, O, dims, k=3, stride=1, form=3, sliced="none"):
    return TapCase(id, family, B, I, O, tuple(dims), k, stride, form, sliced)


# K15 through ops.conv_weight_grad.  (Q, Q8, slab, nslabs, last-slab steps, rows) in the comments are asserted by the CPU test.
K15_CASES = [
    _case("A1", "k15", 1, 3, 5, (4, 9, 2)),                 # the issue's example: Q = Q8 = 264: last slab of ONE step; rows 2
    _case("A2", "k15", 1, 33, 31, (3, 7), 3),               # 2-D 9 taps; Q = 5 * 12 = 60: Q % 8 == 4, Q8 = 64; a single slab; rows 1
    _case("A3", "k15", 1, 31, 33, (2, 3, 3), 3),            # 27 taps = 3 groups; ragged tiles 31 / 33 (a second tile with one row)
    _case("A4", "k15", 2, 32, 1, (5, 6, 7), 1),             # one tap (nt = 1: every off[] clamps to it); O = 1
    _case("A5", "k15", 1, 1, 32, (8, 30), 3),               # 2-D, the stem's one input channel
    _case("A6", "k15", 2, 256, 256, (60, 120), 1),          # slab 512: 64 channel tiles x 2 samples; one tap
    _case("A7", "k15", 1, 5, 7, (14, 31, 12)),              # Q = 8448: rows 33: row group 0 adds a pair AND a tail row
    _case("A8", "k15", 1, 4, 6, (6, 14, 28)),               # Q = 4096: rows 16: every row group a tail row only
    _case("A9", "k15", 1, 4, 6, (6, 15, 28)),               # Q = 4352: rows 17: row group 0 a pair, the others a tail row
    _case("A10", "k15", 2, 4, 6, (6, 14, 28)),              # rows 32: every row group one pair
    _case("A11", "k15", 1, 8, 8, (1, 9, 12)),               # a one-slice 5-D volume, stride 1: kernel planes 0 and 2 are exactly 0
    # The end of every box is zero ring (a volume's whole last plane, a map's last row), so a short last slab of a volume (A1, and
    # the tail row of A7) multiplies zeros only and nothing shows if its steps are dropped.  On a two-pixel-wide map (Wq = 4) the
    # LAST step of the box holds the last data row:
    _case("A12", "k15", 1, 3, 5, (64, 2)),                  # Wq = 4, Q = 264: the ONE step of the last slab holds data row 63
    _case("A13", "k15", 1, 3, 5, (66, 2)),                  # Q = 272: a last slab of two steps, the second holds data row 65
    _case("A14", "k15", 1, 3, 5, (68, 2)),                  # Q = 280: a last slab of three steps (odd), the third holds data row 67
    _case("A15", "k15", 3, 4, 6, (86, 28)),                 # rows 33 = 3 x 11 with data in the tail row (the last slab of the last sample)
    _case("S1", "k15", 2, 4, 6, (6, 5, 8), 3, 2),           # stride 2: even, odd, even extents
    _case("S2", "k15", 1, 33, 8, (7, 6, 3), 3, 2),          # stride 2: odd, even, odd
    _case("S3", "k15", 2, 6, 4, (2, 2, 2), 3, 2),           # stride 2: extent 2, the smallest, k = 3 ...
    _case("S4", "k15", 2, 6, 4, (2, 2, 2), 1, 2),           # ... and k = 1
    _case("S5", "k15", 2, 6, 4, (5, 7, 9), 1, 2),           # 1x1x1 stride 2 (a down-sampling block's residual), odd extents
]
# ... and through ops.conv_nd where the library keeps forward and data gradient (narrow copies made in backward)
K15_ND_CASES = [
    _case("N1", "k15_nd", 2, 4, 6, (6, 5, 8), 3, 2),
    _case("N2", "k15_nd", 1, 40, 70, (4, 9, 10)),           # W % 4 != 0: not K16's; three tap groups x 2 x 3 channel tiles
    _case("N3", "k15_nd", 2, 5, 7, (9, 13)),                # 2-D
    _case("N4", "k15_nd", 2, 6, 4, (5, 7, 9), 1, 2),
]
# K16 / K16 / K15 through ops.conv_nd: wide copies shared by the three products
K16_CASES = [
    _case("T1", "k16", 2, 8, 33, (2, 6, 8), 3),             # Q = 4 * 8 * 16 = 512: exactly one workgroup
    _case("T2", "k16", 1, 9, 31, (2, 3, 4), 3),             # under one workgroup; odd I: the last pair's kh = 1 lane clamps
    _case("T3", "k16", 2, 33, 32, (3, 11, 8), 3),           # Q = 1040 = 2 * 512 + 16: 496 positions of the last workgroup past Q
    _case("T4", "k16", 1, 65, 1, (3, 5, 12), 3),            # three chunks, the last with one channel; O = 1
    _case("T5", "k16", 2, 64, 33, (3, 5, 8), 1),            # 1x1x1: one tap, the 4 KiB weight image; two full chunks
    _case("T6", "k16", 1, 32, 32, (5, 6, 4), 1),            # W = 4
    _case("T7", "k16", 2, 16, 32, (1, 12, 8), 3),           # D == 1 (K19 refuses one slice): no z ring, the kz = 0 / 2 taps read guards
    _case("T8", "k16", 1, 32, 16, (2, 5, 8), 3),            # I % 16 == 0 but under 96 voxels
]
# K19t through ops.conv3x3_s2t, every kernel forced (K19_MIN_PIXELS = LP_K_MIN_PIXELS = 0, K19T_WGRAD)
K19T_SHAPES = [
    ("P1", 2, 16, 16, (1, 1), "none"),        # R = 16 both ways: a half-empty tile; nblk 1; one pixel; H == 1: kernel rows 0 and 2 padding
    ("P2", 1, 32, 48, (2, 15), "none"),       # forward R = 48 (a second tile half empty), nblk 2; data gradient R = 32, nblk 3; P = 30
    ("P3", 2, 48, 32, (3, 11), "none"),       # P = 33: a second wave with one pixel; forward nblk 3
    ("P4", 1, 64, 96, (1, 31), "none"),       # P = 31; forward R = 96 (TO 1, split), data gradient R = 64 (TO 2)
    ("P5", 1, 96, 64, (1, 127), "none"),      # P = 127; forward R = 64: TO 2, accumulators NOT split, ragged pixel count
    ("P6", 2, 64, 64, (3, 43), "none"),       # P = 129: a second workgroup with one pixel; TO 2 both ways
    ("P7", 2, 16, 32, (3, 33), "none"),       # W = 33: cw 3, nb 9: three parts, the last of ONE block; last block one pixel
    ("P8", 1, 32, 16, (2, 17), "views"),      # W = 17; x a channel slice, dy the interior of the padded gradient, ragged map
    ("P9", 2, 48, 16, (3, 16), "views"),      # W = 16: cw 1, full blocks
    ("P10", 1, 16, 48, (2, 8), "none"),       # W = 8: the kh = 1 half of every block is empty
]
K19T_CASES = [_case(f"{n}-f{form}", "k19t", B, I, O, d, 3, 2, form, s) for n, B, I, O, d, s in K19T_SHAPES for form in (3, 1, 2)]
# ... and one shape with enough waves that per_part leaves its floor of 4: nb = 66 blocks in parts of 5, the last of ONE block; two
# 64-row tiles both ways; eight contraction blocks (the pair loop, no tail)
K19T_CASES.append(_case("P11-f3", "k19t", 8, 128, 128, (6, 176), 3, 2, 3, "none"))

CASES = {"k15": K15_CASES, "k15_nd": K15_ND_CASES, "k16": K16_CASES, "k19t": K19T_CASES}
ALL_CASES = K15_CASES + K15_ND_CASES + K16_CASES + K19T_CASES
ACCUMULATE_CASES = ("A12", "A3", "S2")               # mlagg_conv_wgrad_taps with accumulate = 1, twice on the same buffer


def by_id(cid):
    return next(c for c in ALL_CASES if c.id == cid)


def ntaps(case):
    return case.k ** (2 if len(case.dims) == 2 else 3)


def compared(case):
    return ("dW",) if case.family in ("k15", "k15_nd") else ("y", "dx", "dW")


# mlagg_volume_pad, compared exactly: (id, B, C, (D, H, W), stride, wide, as_output's map extents or None)
PAD_CASES = [
    ("narrow", 2, 3, (3, 5, 6), 1, 0, None),
    ("narrow-odd", 1, 2, (2, 3, 7), 1, 0, None),
    ("narrow-out", 2, 3, (3, 5, 6), 1, 0, (3, 5, 6)),
    ("wide", 2, 3, (3, 5, 8), 1, 1, None),
    ("wide-out", 1, 2, (3, 5, 8), 1, 1, (3, 5, 8)),
    ("map", 2, 3, (1, 5, 6), 1, 0, None),
    ("map-out", 2, 3, (1, 5, 6), 1, 0, (1, 5, 6)),
    ("slice-wide", 1, 2, (1, 6, 4), 1, 1, None),
    ("s2-even", 2, 3, (4, 6, 8), 2, 0, None),
    ("s2-odd", 1, 2, (5, 7, 3), 2, 0, None),
    ("s2-mixed", 1, 2, (2, 5, 6), 2, 0, None),
    ("s2-out", 2, 3, (5, 6, 7), 2, 0, (3, 3, 4)),
    ("s2-out-2", 1, 2, (2, 2, 2), 2, 0, (1, 1, 1)),
]
# refused geometries: (D, H, W, stride, wide, as_output extents or None)
PAD_REFUSED = [
    ((3, 5, 6), 1, 1, None),                         # wide with W % 4 != 0
    ((1, 6, 8), 2, 0, None),                         # stride 2 of a 2-D map
    ((3, 5, 8), 2, 1, None),                         # wide at stride 2
    ((3, 5, 6), 1, 0, (5, 5, 6)),                    # an as_output map larger than the box: 5 + 1 > Dq = 5
    ((3, 5, 6), 1, 0, (3, 7, 6)),
    ((3, 5, 6), 1, 0, (3, 5, 8)),
    ((5, 6, 7), 2, 0, (5, 3, 4)),                    # phase grid: Dq = 4
]


def padded_rows(src, dims, stride, wide, as_output):
    """What mlagg_volume_pad must write for `src` (B, C, *map extents): (B, phases, C, 2 guard + Q), the guards included, built here
    from the definition: stride 1 puts voxel (z, y, x) of the map at box position (z + oz, y + 1, x + ox) (oz = 0 for a one-slice
    map, ox = 4 in the wide form, else 1); stride 2 splits the map, padded by one voxel in front, into its 8 parity phases (an
    as_output map lies at the box origin instead); everything else is zero."""
    D, H, W = dims
    Dq, Hq, Wq, guard = pad_geometry(D, H, W, stride, wide)
    B, C = src.shape[:2]
    nph = 8 if (stride == 2 and not as_output) else 1
    box = torch.zeros(B, nph, C, Dq, Hq, Wq, dtype=src.dtype)
    sd, sh, sw = src.shape[2:]
    if stride == 1:
        oz, ox = (0 if D == 1 else 1), (4 if wide else 1)
        box[:, 0, :, oz:oz + sd, 1:1 + sh, ox:ox + sw] = src
    elif as_output:
        box[:, 0, :, :sd, :sh, :sw] = src
    else:
        padded = F.pad(src, (1, 2 * Wq, 1, 2 * Hq, 1, 2 * Dq))                       # one voxel in front, zeros behind
        for ph in range(8):
            pz, py, px = (ph >> 2) & 1, (ph >> 1) & 1, ph & 1
            box[:, ph] = padded[:, :, pz::2, py::2, px::2][:, :, :Dq, :Hq, :Wq]
    rows = torch.zeros(B, nph, C, 2 * guard + Dq * Hq * Wq, dtype=src.dtype)
    rows[..., guard:guard + Dq * Hq * Wq] = box.reshape(B, nph, C, -1)
    return rows


# =====================================================================================================================
# inputs, reference, yardstick
# =====================================================================================================================
def y_dims(case):
    if case.family == "k19t":
        return tuple(2 * d - 1 for d in case.dims)
    return out_dims(case.dims, case.stride)


def inputs(case):
    """float32 host tensors x (B, I, *dims), w (O, I, k, ..) -- K19t: (I, O, 3, 3) --, dy (B, O, *output extents); the same for every
    form and slicing of a shape."""
    nd = len(case.dims)
    g = torch.Generator().manual_seed(zlib.crc32(repr((case.family == "k19t", case.k, case.stride, case.B, case.I, case.O, case.dims)).encode()))
    x = torch.randn(case.B, case.I, *case.dims, generator=g)
    wshape = (case.I, case.O) if case.family == "k19t" else (case.O, case.I)
    w = torch.randn(*wshape, *([case.k] * nd), generator=g) * (case.k ** nd * case.I) ** -0.5
    dy = torch.randn(case.B, case.O, *y_dims(case), generator=g)
    return dict(x=x, w=w, dy=dy)


def evaluate(case, dtype):
    """{"y", "dx", "dW"} in `dtype` on the host, from the operands as the form holds them."""
    t = inputs(case)
    held = {n: v.to(FORM_TYPE[case.form]).to(dtype) for n, v in t.items()}
    x, w = held["x"].requires_grad_(True), held["w"].requires_grad_(True)
    if case.family == "k19t":
        y = F.conv_transpose2d(x, w, None, 2, 1)
    else:
        y = (F.conv3d if len(case.dims) == 3 else F.conv2d)(x, w, None, case.stride, case.k // 2)
    y.backward(held["dy"])
    return dict(y=y.detach(), dx=x.grad, dW=w.grad)


@functools.lru_cache(maxsize=4)
def reference(case):
    """The float64 reference of a case; computed once, never modified."""
    return evaluate(case, torch.float64)


YARDSTICK_THREADS = 16


def yardstick(case):
    """The plain-fp32 yardstick of a case, with YARDSTICK_THREADS threads (tests/_conv_kernel_cases.py yardstick: torch's fp32 weight
    gradient on the host follows the thread count)."""
    before = torch.get_num_threads()
    torch.set_num_threads(YARDSTICK_THREADS)
    try:
        return evaluate(case, torch.float32)
    finally:
        torch.set_num_threads(before)


def bounds(case):
    """{quantity: bound on max |got - ref| / max |ref|}, un-widened: those of tests/_conv_kernel_cases.py bounds()."""
    if case.form != 3:
        return dict(y=4e-6, dx=4e-6, dW=4e-6)
    return dict(y=2e-6, dx=2e-6, dW=1e-5 if len(case.dims) == 3 else 4e-6)


def error(got, ref):
    """max |got - ref| / max |ref| (a NaN in `got` gives NaN, which no bound admits)."""
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def dw_bound(case, ref_dw, yard_dw):
    """The bound a summed weight gradient is held to: max(bounds()["dW"], 4 x the yardstick's error on this case), at most the
    2e-5 * max + 1e-5 of tests/test_conv_wgrad_gpu.py (as a share of the maximum)."""
    b = max(bounds(case)["dW"], 4 * error(yard_dw, ref_dw))
    return min(b, 2e-5 + 1e-5 / float(ref_dw.abs().max()))


def zero_taps(case):
    """Index tuples into dW's kernel axes that no voxel pair reaches: exactly zero.  A one-slice volume has no plane in front or
    behind (kernel planes 0 and 2 of a 3 x 3 x 3 kernel); a one-row K19t input has no dy row above or below."""
    if case.family == "k19t":
        return [(ky,) for ky in (0, 2)] if case.dims[0] == 1 else []
    if len(case.dims) == 3 and case.k == 3 and case.stride == 1:
        return [(kz,) for kz in (0, 2)] if case.dims[0] == 1 else []
    return []
