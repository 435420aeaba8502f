"""Cases, references and path predicates for the selective-scan kernels -- K1 (csrc/selscan.hip), K1f (csrc/selscan_tok.hip) and K1s
(csrc/selscan1.hip) -- at the sizes where their launchers and loops change path: shared by tests/test_selscan_paths_cpu.py and
tests/test_selscan_paths_gpu.py.  The scan algebra (forms, gather / fold-back, the two scans) is tests/_selscan_regime_cases.py's.

A CASE is a namedtuple and the seed of its own inputs (zlib.crc32(repr(case))):
    K1Case(b, G, Hc, L, R, D, bias, softplus, blocked)   R = 0: ops.selective_scan_fn, R > 0: ops.selective_scan_lowrank_fn; D / bias
                                                          False: the operand is None; blocked: under MLAGG_SELSCAN_BWD_BLOCKED=1
    K1fCase(b, HW, D, bias)                               ops.msmm_scan on the maps HW (L = sum of H * W)
    K1sCase(B, L, C, K, R, sliced)                        ops.selective_scan1; sliced "tok" / "dy": that operand is the channel block
                                                          [8, 8 + C) of a tensor 16 channels wider
GROUPS maps a group name to its cases; the GPU test is parametrised per group.

INPUTS HAVE MEMORY ACROSS CHUNKS.  delta is drawn around 0.01 (softplus of -4.6 +- 0.3, or directly where softplus is off) and A
in [-1.4, -0.7], so a step decays the state by 0.975 .. 0.996 and a 64-step chunk by about a half: a chunk's entry state carries as
much as the chunk adds.  `reset_scan` is the same recurrence in float64 with the forward state AND the reverse carry set to zero at
every multiple of the chunk length; `carry_sensitivity` says how far that moves y (after the first chunk) and du (before the last
chunk -- the mirror: the reverse carry enters a chunk from the chunks after it).  The CPU test asserts at least 0.1 of max |ref| for
every case with more than one chunk, so a kernel that lost a chunk carry, a tile-entry state or a prefix could not pass.

`references(case)` is (form, inputs, oracle (y, grads), plain fp32 (y, grads)), computed once per process and never modified.  The
oracle (oracle/selscan_ref.c, double arithmetic) is the truth; the step-by-step float32 loop is the yardstick of the bound:
    bound = min(existing, max(1e-5 max |ref|, 16 x error of the plain fp32 scan on that case))
with `existing` the shape tests' 1e-4 (y), 2e-4 (gradients), 3e-4 (gradients of K1 low-rank and K1f) and no rtol term.  1e-5: every
kernel error measured in tests/test_selscan_regimes_gpu.py is at most 1.4e-6 and at most 12 x the sequential loop's.  EXCEPTIONS
lists the (case, quantity) pairs that get the existing bound instead, each with the measured figure and the reason from the code.
An absent operand enters the scans as zeros (the same y); its gradient is dropped from the reference and must be None on the device.

PATH PREDICATES are pure functions restating a launcher's decision; each names the source line it mirrors, and the CPU test compares
them with the library's host queries over the cases and a sweep.  They describe the DEFAULT dispatch; OVERRIDES lists the environment
variables that change it and whether the cases cover them.

[(2, 3), (2, 5)] (a scale that ends in the middle of a 4-step quad) is part of the K1f list: ops.msmm_scan_index takes any list of
maps, and K1f asks only for L % 4 == 0.

Plain-fp32 yardstick errors (max |plain - oracle| / max |oracle|), largest over the group's cases, measured on the host:

    cases               y        du       ddelta   ddtr     dWdt     dA       dB       dC       dD       dbias
    k1_time_vec         5.9e-07  7.3e-07  4.9e-07  4.1e-07  5.2e-07  1.3e-06  4.9e-07  5.8e-07  1.0e-06  7.0e-07
    k1_time_scalar      3.3e-07  4.0e-07  6.5e-07  4.2e-07  4.0e-07  7.0e-07  4.5e-07  5.7e-07  9.5e-07  5.3e-07
    k1_channels_vec     5.0e-07  4.0e-07  4.5e-07  4.6e-07  3.1e-07  7.8e-07  5.2e-07  4.9e-07  5.8e-07  5.7e-07
    k1_channels_scalar  4.0e-07  4.7e-07  5.2e-07  9.9e-07  8.5e-07  9.6e-07  5.3e-07  6.9e-07  5.8e-07  5.2e-07
    k1_channels_whole   3.2e-07  5.3e-07  3.8e-07  3.2e-07  4.4e-07  8.3e-07  3.9e-07  3.8e-07  3.6e-07  4.8e-07
    k1_ranks            4.7e-07  9.0e-07  -        4.9e-07  4.6e-07  1.2e-06  4.9e-07  5.5e-07  4.0e-07  5.6e-07
    k1_reduce_rows      6.3e-07  6.3e-07  7.3e-07  5.3e-07  4.0e-07  1.7e-06  5.6e-07  6.6e-07  1.1e-06  5.5e-07
    k1_batch            4.0e-07  5.4e-07  4.2e-07  4.4e-07  3.6e-07  6.4e-07  5.1e-07  4.5e-07  4.2e-07  5.1e-07
    k1_optional         4.3e-07  4.8e-07  4.8e-07  4.7e-07  4.6e-07  8.6e-07  5.3e-07  4.2e-07  4.3e-07  5.6e-07
    k1_override         2.9e-07  4.3e-07  3.0e-07  4.4e-07  2.0e-07  3.7e-07  3.7e-07  3.5e-07  1.7e-07  3.8e-07
    cases               y        dxc      dxdbl    dWdt     dA       dD       dbias
    k1f_time            3.7e-07  2.7e-07  4.4e-07  3.5e-07  1.4e-06  8.4e-07  5.7e-07
    k1f_batch_optional  3.0e-07  2.9e-07  3.6e-07  3.7e-07  8.3e-07  7.1e-07  4.0e-07
    cases               y        dtok     ddtr     dBs      dCs      dWdt     dA       dD       dbias
    k1s_time            3.2e-07  3.7e-07  3.2e-07  3.8e-07  8.5e-07  4.6e-07  1.5e-06  7.0e-07  7.1e-07
    k1s_ranks           3.2e-07  3.3e-07  3.4e-07  4.4e-07  3.3e-07  3.7e-07  6.5e-07  5.4e-07  5.2e-07
    k1s_channels        2.8e-07  4.0e-07  6.7e-07  3.8e-07  3.6e-07  4.3e-07  5.2e-07  4.8e-07  5.3e-07
    k1s_chunks          2.8e-07  3.0e-07  4.5e-07  4.2e-07  3.7e-07  4.8e-07  1.0e-06  1.1e-06  5.5e-07
    k1s_sliced          2.1e-07  3.2e-07  3.4e-07  3.8e-07  2.8e-07  3.8e-07  3.8e-07  5.7e-07  3.8e-07

Measured on an MI355X (profiles/selscan_kernel_paths_mi355x.log): every kernel error is at most 8.4e-6, no case needs an exception.
The largest sit at one to nine steps (d(dtr), d(delta), d(bias), dA, dWdt at 5e-6 .. 8e-6, 20 to 60 times the loop's): softplus1
(csrc/activations.h) switches from its series to log(1 + e) at e = exp(-|x|) = 0.01, i.e. at x = -4.6, the middle of these inputs,
and 1 + e rounds at 6e-8 absolute, 3e-6 .. 6e-6 of a delta of 0.01; a sum over a few steps does not average that out.  From a chunk
on, errors are 1e-6 .. 4e-6, 4 to 15 times the loop's.
"""
import collections
import functools
import zlib

import torch

from tests import _selscan_regime_cases as R

K1Case = collections.namedtuple("K1Case", "b G Hc L R D bias softplus blocked")
K1fCase = collections.namedtuple("K1fCase", "b HW D bias")
K1sCase = collections.namedtuple("K1sCase", "B L C K R sliced")

# MLAGG_SELSCAN_BWD_BLOCKED is read on every call (csrc/internal.h getenv_flag: a plain getenv), so the cases with blocked=True run
# it under monkeypatch.setenv.  Nothing else changes the scans' dispatch.
OVERRIDES = (("MLAGG_SELSCAN_BWD_BLOCKED", "covered: group 'k1_override'"),)
SLICE_AT, SLICE_EXTRA = 8, 16

N = R.N
TC, T8, ST = 64, 8, 16                       # csrc/selscan_common.h: steps per chunk, per tile of the group kernel, per LDS sub-tile
SCAN_CB, GROUP_MAX_HC, RMAX, PP, NT8 = 32, 96, 4, 24, 7
E_UNSUPPORTED = -1                           # MLAGG_E_UNSUPPORTED


def _cdiv(a, b):
    return (a + b - 1) // b


# =====================================================================================================================
# path predicates
# =====================================================================================================================
# ---- K1 (csrc/selscan.hip, csrc/selscan_common.h) -------------------------------------------------------------------
def k1_geom(Hc):
    """(nblk, CB, channels of the last block): selscan_common.h make_geom with max_cb = SCAN_CB -- nblk = ceil(Hc / 32) workgroups
    per group, CB = ceil(Hc / nblk) channels each; the last one is ragged when nblk * CB > Hc."""
    nblk = _cdiv(Hc, SCAN_CB)
    CB = _cdiv(Hc, nblk)
    return nblk, CB, Hc - (nblk - 1) * CB


def k1_nchunks(L):
    """selscan_common.h make_geom: gm.nchunks."""
    return _cdiv(L, TC)


def k1_fast(Hc, L):
    """selscan.hip scan_path `fast`: the forward / backward-local instantiation without range checks (block_threads is 128 for every
    CB <= 32, and a low-rank call has R >= 1)."""
    _, CB, _ = k1_geom(Hc)
    return L % 4 == 0 and Hc % CB == 0 and 4 * CB == 128


def k1_bwd_form(Hc, L, R, blocked=False):
    """selscan.hip scan_path `form`: "blocked-atomic" (channel blocks, dB / dC / d(dtr) by atomics: Hc > 96), "blocked" (the same
    kernel with one block per group: only under the override) or (RT, VEC, FULL, WHOLE) of selscan_bwd_group_kernel, RT = 0 (direct
    form), 3 (rank 3 at a VEC and FULL shape) or RMAX (the run-time rank: every other rank, and rank 3 everywhere else)."""
    if Hc > GROUP_MAX_HC or blocked:
        return "blocked-atomic" if k1_geom(Hc)[0] > 1 else "blocked"
    vec, full, whole = L % 4 == 0, Hc % 16 == 0, L % TC == 0
    rgen = RMAX if R else 0
    if R in (0, 3) and vec and full:
        return (R, True, True, whole)
    if vec and full:
        return (rgen, True, True, False)
    if vec:
        return (rgen, True, False, False)
    return (rgen, False, False, False)


def k1_path_code(Hc, L, R, blocked=False):
    """What mlagg_selscan_path returns (include/mlagg_hip.h): form * 2 + fast."""
    f = k1_bwd_form(Hc, L, R, blocked)
    if isinstance(f, str):
        form = 0
    elif f[1] and f[2] and f[0] in (0, 3) and R in (0, 3):
        form = 1 if f[3] else 2
    elif f[1] and f[2]:
        form = 3
    else:
        form = 4 if f[1] else 5
    return form * 2 + int(k1_fast(Hc, L))


def k1_slots(Hc):
    """(J, channels in the last slot): selscan_bwd_group_kernel walks J = ceil(Hc / 16) slots of 16 channels per wave."""
    J = _cdiv(Hc, 16)
    return J, Hc - 16 * (J - 1)


def k1_reduce(b, dim, L):
    """(rows, ragged last column workgroup) of selscan_common.h selscan_reduce_partials: rows = batch * nchunks, 64-column
    workgroups over dim * PP columns."""
    return b * k1_nchunks(L), (dim * PP) % 64 != 0


def k1_state_floats(b, dim, L):
    """selscan.hip mlagg_selscan_state_floats."""
    return b * k1_nchunks(L) * dim * (N + 1 + NT8 * N)


def k1_bwd_workspace_floats(b, dim, L):
    """selscan.hip mlagg_selscan_bwd_workspace_floats."""
    return b * k1_nchunks(L) * dim * (N + PP)


# ---- K1f (csrc/selscan_tok.hip) -------------------------------------------------------------------------------------
MSMM_DIM = R.MSMM_K * R.MSMM_HC


def k1f_len(HW):
    return sum(h * w for h, w in HW)


def k1f_supported(L):
    """selscan_tok.hip mlagg_msmm_scan_supported at the model's d_inner / d_state / rank / directions."""
    return L > 0 and L % 4 == 0 and L * MSMM_DIM < 2 ** 32


def k1f_whole(L):
    """selscan_tok.hip mlagg_msmm_scan_bwd: tok_bwd_group_kernel<WHOLE>, L a multiple of the 64-step chunk."""
    return L % TC == 0


def k1f_state_floats(b, L):
    return b * k1_nchunks(L) * MSMM_DIM * (N + 1 + NT8 * N)


def k1f_workspace_floats(b, L):
    """(forward, backward): selscan_tok.hip mlagg_msmm_scan_fwd_workspace_floats / _bwd_workspace_floats."""
    return b * L * MSMM_DIM, b * k1_nchunks(L) * MSMM_DIM * (N + PP) + b * L * MSMM_DIM


# ---- K1s (csrc/selscan1.hip) ----------------------------------------------------------------------------------------
SEL1_RANKS = (1, 2, 3, 4, 8, 16, 20)         # SEL1_DISPATCH_R
SEL1_TB, SEL1_TS = 16, 64


def k1s_chunk_len(B, K, L):
    """selscan1.hip chunk_len: the longest power of two from 2048 down to 64 that still gives 2048 (sequence, chunk) pairs."""
    ch = 2048
    while ch > 64 and B * K * _cdiv(L, ch) < 2048:
        ch //= 2
    return ch


def k1s_geom(B, L, C, K):
    """(chunk_len, nchunk, nblk): selscan1.hip geom."""
    ch = k1s_chunk_len(B, K, L)
    return ch, _cdiv(L, ch), _cdiv(C, 64)


def k1s_param_pitch(Rk):
    """selscan1.hip param_pitch: floats per staged parameter row [idx, B, C, dt_0 .. dt_{R-1}], padded to 16 bytes."""
    return (3 + Rk + 3) & ~3


def k1s_state_floats(B, L, C, K):
    """selscan1.hip mlagg_selscan1_state_floats."""
    _, nchunk, _ = k1s_geom(B, L, C, K)
    return B * K * C * (2 * nchunk + _cdiv(L, SEL1_TB)) + 128


def k1s_bwd_workspace_floats(B, L, C, K, Rk):
    """selscan1.hip mlagg_selscan1_bwd_workspace_floats."""
    _, nchunk, nblk = k1s_geom(B, L, C, K)
    return B * K * nchunk * C * (4 + Rk) + (B * K * nblk * (2 + Rk) * L if nblk > 1 else 0) + 256


# =====================================================================================================================
# the cases
# =====================================================================================================================
def _k1(b, G, Hc, L, R=0, D=True, bias=True, softplus=True, blocked=False):
    return K1Case(b, G, Hc, L, R, D, bias, softplus, blocked)


def _both(b, G, Hc, L):
    return [_k1(b, G, Hc, L), _k1(b, G, Hc, L, 3)]


VEC_L = (4, 8, 12, 16, 20, 60, 64, 68, 124, 128, 132, 448, 512, 516, 1024, 1028)
SCALAR_L = (1, 2, 3, 5, 7, 9, 15, 17, 63, 65, 66, 127, 129, 513)
CHANNEL_HC = (8, 16, 20, 32, 33, 48, 64, 70, 95, 96, 97, 128, 131)
REDUCE_BL = ((2, 512), (1, 1028), (2, 1024), (3, 704), (3, 1024), (7, 448))          # rows 16, 17, 32, 33, 48, 49
_SUBSETS = [(D, bias, sp) for D in (True, False) for bias in (True, False) for sp in (True, False)]

GROUPS = collections.OrderedDict()
GROUPS["k1_time_vec"] = [c for L in VEC_L for c in _both(1, 2, 32, L)]
GROUPS["k1_time_scalar"] = [c for L in SCALAR_L for c in _both(1, 1, 20, L)]
# every Hc with both G, both forms and both L: the direct form at (G 1, L 132) and (G 3, L 130), rank 3 at the other two
GROUPS["k1_channels_vec"] = [_k1(1, G, Hc, 132, R) for Hc in CHANNEL_HC for G, R in ((1, 0), (3, 3))]
GROUPS["k1_channels_scalar"] = [_k1(1, G, Hc, 130, R) for Hc in CHANNEL_HC for G, R in ((1, 3), (3, 0))]
GROUPS["k1_channels_whole"] = [c for Hc in (32, 96, 128) for c in _both(1, 2, Hc, 128)]
GROUPS["k1_ranks"] = [_k1(1, 2, Hc, L, r) for Hc, L in ((32, 132), (20, 132), (20, 130), (128, 132)) for r in (1, 2, 3, 4)]
# dim = 20: 480 columns, the last 64-column workgroup ragged; dim = 64: 1536 columns, exact
GROUPS["k1_reduce_rows"] = [_k1(b, G, Hc, L, r) for G, Hc in ((1, 20), (2, 32)) for b, L in REDUCE_BL for r in (0, 2)]
# batch 2 on every backward form, block count and last-block kind (the reduction-row cases add the whole-chunk forms)
GROUPS["k1_batch"] = ([_k1(2, 2, Hc, 132, r) for Hc in (20, 32, 33, 64, 70, 96, 128, 131) for r in (0, 2)] +
                      [_k1(2, 2, 32, 132, 3), _k1(2, 2, 32, 128, 3), _k1(2, 2, 20, 130), _k1(2, 2, 20, 130, 2), _k1(2, 2, 33, 130, 3)])
GROUPS["k1_optional"] = [_k1(1, G, Hc, L, r, D, bias, sp) for G, Hc, L, r in ((2, 32, 128, 0), (1, 128, 132, 0), (1, 128, 132, 3),
                                                                            (2, 32, 132, 3), (2, 20, 132, 2))
                         for D, bias, sp in _SUBSETS]
GROUPS["k1_override"] = [_k1(1, 2, 32, 132, blocked=True), _k1(1, 2, 20, 130, 2, blocked=True)]

K1F_MAPS = ([(2, 2)], [(2, 4)], [(2, 6)], [(4, 4), (2, 2)], [(6, 10)], [(8, 8)], [(8, 8), (2, 2)], [(8, 16)], [(8, 16), (2, 2)],
            [(16, 32)], [(16, 32), (2, 2)], [(32, 34)], [(32, 34), (2, 2)])


def _k1f(b, HW, D=True, bias=True):
    return K1fCase(b, tuple(tuple(m) for m in HW), D, bias)


GROUPS["k1f_time"] = [_k1f(1, hw) for hw in K1F_MAPS] + [_k1f(1, [(2, 3), (2, 5)])]
GROUPS["k1f_batch_optional"] = [_k1f(2, [(16, 32)]), _k1f(3, [(8, 16), (2, 2)]), _k1f(1, [(8, 8), (2, 2)], D=False),
                                _k1f(1, [(8, 8), (2, 2)], bias=False), _k1f(1, [(8, 8), (2, 2)], D=False, bias=False)]

SEL1_L = (2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257)
GROUPS["k1s_time"] = [K1sCase(1, L, 64, 3, 3, "none") for L in SEL1_L]
GROUPS["k1s_ranks"] = [K1sCase(2, 150, 128, 2, r, "none") for r in SEL1_RANKS]
GROUPS["k1s_channels"] = [K1sCase(1, 150, C, K, 2, "none") for C in (64, 128, 192) for K in (1, 2, 3)]
# two chunks, the second 6 steps long, at chunk lengths 128 .. 1024; one 2048-step chunk longer than the sequence
GROUPS["k1s_chunks"] = [K1sCase(86, ch + 6, 64, 12, 2, "none") for ch in (128, 256, 512, 1024)] + [K1sCase(171, 70, 64, 12, 2, "none")]
GROUPS["k1s_sliced"] = [K1sCase(2, 150, 128, 2, 3, "tok"), K1sCase(2, 150, 128, 2, 3, "dy"), K1sCase(1, 65, 64, 3, 2, "tok"),
                        K1sCase(1, 65, 64, 3, 2, "dy")]

ALL_CASES = list(dict.fromkeys(c for cases in GROUPS.values() for c in cases))      # a case may serve two groups

# (case, quantity) -> (measured max-scaled kernel error, reason): pairs that take the existing bound instead of the tight one
EXCEPTIONS = {}


def form_of(case):
    if isinstance(case, K1Case):
        return "lowrank" if case.R else "direct"
    return "msmm" if isinstance(case, K1fCase) else "sel1"


def case_id(case):
    if isinstance(case, K1Case):
        flags = "".join(s for s, on in (("-noD", not case.D), ("-nobias", not case.bias), ("-nosp", not case.softplus),
                                        ("-blocked", case.blocked)) if on)
        return f"k1-{case.b}x{case.G}x{case.Hc}x{case.L}r{case.R}{flags}"
    if isinstance(case, K1fCase):
        flags = ("" if case.D else "-noD") + ("" if case.bias else "-nobias")
        return f"k1f-{case.b}x" + "+".join(f"{h}.{w}" for h, w in case.HW) + flags
    return f"k1s-{case.B}x{case.L}x{case.C}x{case.K}r{case.R}" + ("" if case.sliced == "none" else "-" + case.sliced)


def chunk_of(case):
    """Steps per chunk of the case's kernels."""
    return k1s_chunk_len(case.B, case.K, case.L) if isinstance(case, K1sCase) else TC


def seq_len(case):
    return k1f_len(case.HW) if isinstance(case, K1fCase) else case.L


def n_chunks(case):
    return _cdiv(seq_len(case), chunk_of(case))


# =====================================================================================================================
# inputs
# =====================================================================================================================
X0, XS = -4.6, 0.3                           # softplus argument: softplus(-4.6) = 0.01
D_SCALE = 0.1                                # the skip term stays below the scan's part of y
TAIL_MIN = 16                                # a last chunk shorter than this gets a larger dout (see _tail_gain)


def _tail_gain(case):
    """(first step of the last chunk, factor on dout there).  The reverse carry out of a last chunk of r steps is the sum of r terms
    where an ordinary chunk sends about 50: with r < 16 it would move du by less than the condition on the inputs asks, so dout on
    those steps is 4 / sqrt(r) times larger (1 step: 4 x).  y needs no mirror: its carry leaves a full first chunk."""
    L, ch = seq_len(case), chunk_of(case)
    last = (_cdiv(L, ch) - 1) * ch
    r = L - last
    return last, (4.0 * r ** -0.5 if last > 0 and r < TAIL_MIN else 1.0)


def _A(g, *shape):
    return -(0.7 + 0.7 * torch.rand(*shape, generator=g))


def _lowrank_x(g, lead, Rk, L, d, bias, softplus):
    """(dtr (*lead, Rk, L), Wdt (d, Rk), bias (d) or None): the softplus argument Wdt . dtr + bias is X0 +- XS per step with
    softplus, and delta itself (about 0.01, positive) without."""
    rn = lambda *s: torch.randn(*s, generator=g)                                                  # noqa: E731
    if not softplus:
        dtr = torch.rand(*lead, Rk, L, generator=g) + 0.5
        Wdt = (torch.rand(d, Rk, generator=g) + 0.5) * (0.008 / Rk)
        return dtr, Wdt, (0.002 * torch.rand(d, generator=g) if bias else None)
    dtr, Wdt = rn(*lead, Rk, L), rn(d, Rk) * (XS * Rk ** -0.5)
    if bias:
        return dtr, Wdt, X0 + 0.1 * rn(d)
    # no bias: rank row 0 carries the offset, 4 x -1.15 = -4.6
    dtr[..., 0, :] = 4.0 + 0.1 * dtr[..., 0, :]
    Wdt[:, 0] = X0 / 4.0 + 0.03 * rn(d)
    return dtr, Wdt, None


def make_inputs(case):
    """The operands of the case's op as float32 CPU tensors, named like tests/_selscan_regime_cases.py names them (absent: None)."""
    out = _draw_inputs(case)
    last, gain = _tail_gain(case)
    if gain != 1.0:
        if isinstance(case, K1Case):
            out["dout"][..., last:] *= gain
        else:                                    # token-major: the tokens that any direction visits in its last chunk
            out["dout"][:, torch.unique(out["idx"][:, last:])] *= gain
    return out


def _draw_inputs(case):
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    rn = lambda *s: torch.randn(*s, generator=g)                                                  # noqa: E731
    if isinstance(case, K1Case):
        b, G, Hc, L, Rk = case.b, case.G, case.Hc, case.L, case.R
        d = G * Hc
        out = dict(u=rn(b, d, L), A=_A(g, d, N), B=rn(b, G, N, L), C=rn(b, G, N, L), D=D_SCALE * rn(d) if case.D else None,
                   dout=rn(b, d, L))
        if Rk:
            out["dtr"], out["Wdt"], out["bias"] = _lowrank_x(g, (b, G), Rk, L, d, case.bias, case.softplus)
        elif case.softplus:
            out["delta"] = XS * rn(b, d, L) + (0.0 if case.bias else X0)
            out["bias"] = X0 + 0.1 * rn(d) if case.bias else None
        else:
            out["delta"] = 0.006 + 0.008 * torch.rand(b, d, L, generator=g)
            out["bias"] = 0.002 * torch.rand(d, generator=g) if case.bias else None
        return out
    if isinstance(case, K1fCase):
        K, HC, Rk, XB = R.MSMM_K, R.MSMM_HC, R.MSMM_R, R.MSMM_XB
        idx = R.reference_orders(case.HW)
        b, L = case.b, idx.shape[1]
        xdbl = rn(b, L, K, XB)
        dtr, Wdt, bias = _lowrank_x(g, (b, L, K), Rk, 1, K * HC, case.bias, True)                 # token-major rank rows
        xdbl[..., :Rk] = dtr[..., 0]
        xdbl[..., 3] = 0.0                                                                        # the pad column of every direction
        return dict(xc=rn(b, L, HC), xdbl=xdbl.view(b, L, K * XB).contiguous(), Wdt=Wdt, A=_A(g, K * HC, N),
                    D=D_SCALE * rn(K * HC) if case.D else None, bias=bias, dout=rn(b, L, HC), idx=idx)
    B, L, C, K, Rk = case.B, case.L, case.C, case.K, case.R
    dtr, Wdt, bias = _lowrank_x(g, (B, K), Rk, L, K * C, True, True)
    return dict(tok=rn(B, L, C), idx=R.sel1_orders(L, K, g), dtr=dtr, Bs=rn(B, K, L), Cs=rn(B, K, L), Wdt=Wdt, A=_A(g, K * C),
                D=D_SCALE * rn(K * C), bias=bias, dout=rn(B, L, C))


def softplus_of(case):
    return case.softplus if isinstance(case, K1Case) else True


def absent(case):
    """Names of the operands the case passes as None."""
    if isinstance(case, K1sCase):
        return ()
    return tuple(k for k, on in (("D", case.D), ("bias", case.bias)) if not on)


def _filled(form, inputs):
    """The inputs with zeros for the absent operands: what the host scans take."""
    d = inputs["A"].shape[0]
    return {k: (torch.zeros(d) if v is None else v) for k, v in inputs.items()}


def sequences(case):
    """(u, delta, A, B, C, D, bias, dout) of the plain scan, float32."""
    form = form_of(case)
    return R.to_sequences(form, _filled(form, make_inputs(case)))


@functools.lru_cache(maxsize=None)
def references(case):
    """(form, inputs, (y, grads) of the oracle, (y, grads) of the plain fp32 scan); gradients of absent operands left out."""
    form, inputs = form_of(case), make_inputs(case)
    filled = _filled(form, inputs)
    sp = softplus_of(case)
    out = []
    for scan in (R.oracle_scan, R.plain_fp32_scan):
        y, g = R.reference(form, filled, functools.partial(scan, softplus=sp))
        out.append((y, {k: v for k, v in g.items() if k not in absent(case)}))
    return form, inputs, out[0], out[1]


EXISTING = {"direct": 2e-4, "lowrank": 3e-4, "msmm": 3e-4, "sel1": 2e-4}
EXISTING_Y, TIGHT, PLAIN_FACTOR = 1e-4, 1e-5, 16.0


def bound(case, name, ref, plain):
    """The largest allowed max |got - ref| for quantity `name` ("y" or an operand's name) of `case`."""
    s = max(float(ref.abs().max()), 1e-6)
    existing = (EXISTING_Y if name == "y" else EXISTING[form_of(case)]) * s
    if (case, name) in EXCEPTIONS:
        return existing
    return min(existing, max(TIGHT * s, PLAIN_FACTOR * float((plain - ref).abs().max())))


# =====================================================================================================================
# what a lost carry would do to a case
# =====================================================================================================================
def reset_scan(u, delta, A, B, C, D, bias, dout, softplus=True, period=TC):
    """(y, du) of the recurrence in float64 with the forward state h and the reverse carry q set to zero at every multiple of
    `period` steps: h_l = a_l h_{l-1} + delta_l B_l u_l, y_l = C_l . h_l + D u_l; q_l = a_{l+1} q_{l+1} + C_l dout_l,
    du_l = delta_l B_l . q_l + D dout_l, a_l = exp(delta_l A).  period >= L: the scan itself."""
    b, d, L = u.shape
    Hc = d // B.shape[1]
    x = delta.double() + bias.double()[None, :, None]
    dl = torch.nn.functional.softplus(x) if softplus else x
    nper = _cdiv(L, period)
    pad = nper * period - L

    def cut(t):                                              # (..., L) -> (..., nper, period), zero steps behind the end
        t = torch.nn.functional.pad(t.double(), (0, pad))
        return t.reshape(*t.shape[:-1], nper, period)

    dlc, uc, gc = cut(dl), cut(u), cut(dout)
    Bc = cut(B.repeat_interleave(Hc, dim=1)).permute(0, 1, 3, 2, 4)          # (b, d, nper, n, period)
    Cc = cut(C.repeat_interleave(Hc, dim=1)).permute(0, 1, 3, 2, 4)
    Ad = A.double()[None, :, None, :]                                        # (1, d, 1, n)
    h = torch.zeros(b, d, nper, A.shape[1], dtype=torch.float64)
    q = torch.zeros_like(h)
    y, du = torch.zeros_like(uc), torch.zeros_like(uc)
    for t in range(period):
        h = torch.exp(dlc[..., t, None] * Ad) * h + (dlc[..., t] * uc[..., t])[..., None] * Bc[..., t]
        y[..., t] = (Cc[..., t] * h).sum(-1)
    for t in range(period - 1, -1, -1):
        q = q + Cc[..., t] * gc[..., t, None]
        du[..., t] = dlc[..., t] * (Bc[..., t] * q).sum(-1)
        q = torch.exp(dlc[..., t, None] * Ad) * q
    Dd = D.double()[None, :, None]
    y = y.reshape(b, d, -1)[..., :L] + Dd * u.double()
    du = du.reshape(b, d, -1)[..., :L] + Dd * dout.double()
    return y, du


SENS_BATCH = 4


def carry_sensitivity(case):
    """(y, du): how far zeroing the carries at the chunk edges moves them, as max |reset - scan| / max |scan| over the steps a
    carry reaches -- y after the first chunk, du before the last.  Looks at the first SENS_BATCH batch items only (every item is
    drawn alike, and one that moves is enough): the K1s chunk cases have 86 and 171."""
    seq, sp, ch = sequences(case), softplus_of(case), chunk_of(case)
    u, delta, A, B, C, D, bias, dout = seq
    L = u.shape[2]
    last = (_cdiv(L, ch) - 1) * ch
    dy = ddu = sy = sdu = 0.0
    for i in range(min(u.shape[0], SENS_BATCH)):             # one batch item at a time: the float64 pieces stay small
        one = (u[i:i + 1], delta[i:i + 1], A, B[i:i + 1], C[i:i + 1], D, bias, dout[i:i + 1])
        y0, du0 = reset_scan(*one, softplus=sp, period=L)
        y1, du1 = reset_scan(*one, softplus=sp, period=ch)
        dy, ddu = max(dy, float((y1 - y0)[..., ch:].abs().max())), max(ddu, float((du1 - du0)[..., :last].abs().max()))
        sy, sdu = max(sy, float(y0.abs().max())), max(sdu, float(du0.abs().max()))
    return dy / sy, ddu / sdu
