"""GPU parity of the two 16-bit attention kernels -- K4lp (csrc/pooled_attn_lp.hip, ops.pooled_diff_attn under
ops.compute_precision("bf16" | "fp16")) and the flash shim (csrc/flash_attn.hip, shims.flash_attn_func) -- one operation at a time
against the float64 oracles of tests/_attention_lp_cases.py (whose soundness tests/test_attention_lp_regimes_cpu.py checks without a
GPU), at the tile edges of the kernels and outside the O(1)-logit regime of tests/test_pooled_attn_lp_gpu.py and
tests/test_flash_shim_gpu.py.

(a) K4lp parity.  y, dq, dk, dv, dlam, dsubln against ref16 (float64 on the ROUNDED operands); per tensor the bound is
    max(T max|ref16|, 4 max|emul16 - ref16|), T = 4e-3 (fp16) / 3e-2 (bf16), 1 in place of max|ref16| where the oracle is identically
    zero.  The shapes marked strided run with q, dout, k and v as column blocks of wider rows.  Regimes: "peaked" (largest logit
    +100 after rounding, its key at index 0 or at index P - 1 in the ragged last tile; the one-hot rows of the saved o1 / o2 equal the
    V row of their key within T), "flat" (also against the closed form), "cancel" (output within the bound of 0).
(b) The 2 x 3201 x 320 x 8 case takes 128-token chunks in the key-side kernel: the workspace size says so (26 chunks).
(c) Strided operands: bit-identical to the contiguous call, output and all gradients, and nothing outside dq's column block of the
    shared gradient buffer is written.
(d) Two runs of K4lp are bit-identical (fixed-order sums); of the shim, out and dq are (dk and dv come from float atomics).
(e) Loss scale: dout * 2^12 under fp16, dout * 2^-12 under bf16: every gradient within the same relative bound of 2^+-12 times the oracle's.
(f) Flash shim parity against exact float64 attention on the same 16-bit inputs: 3 output ulps + 1e-6, per regime, "flat" also against
    round16(mean(v)); P = 513 is refused.

Every test prints error / bound per tensor (run with -s) and puts it into its assertion message.

Measured on an MI355X: the worst error / bound per kernel, regime and precision, with its tensor and case and, in brackets, the
max-scaled error of the kernel / of the yardstick (emul16; the shim's float64 emulation of its output roundings).
    kernel regime        fp16                                                  bf16
    k4lp   init          0.237  dsubln_w of 1x70x320x4-A (9.47e-04 / 9.46e-04)   0.272  dlam of 2x1x1x1-B (8.15e-03 / 4.86e-03)
    k4lp   peaked-first  0.250  dq of 2x257x33x2-B (1.60e-03 / 1.60e-03)         0.250  dq of 2x257x33x2-B (8.03e-03 / 8.03e-03)
    k4lp   peaked-last   0.250  dq of 2x257x33x2-B (1.60e-03 / 1.60e-03)         0.250  dq of 2x257x33x2-B (8.03e-03 / 8.03e-03)
    k4lp   flat          0.127  dvp of 1x70x320x4-A (5.07e-04 / 5.07e-04)        0.113  dvp of 2x257x33x2-B (3.40e-03 / 3.40e-03)
    k4lp   cancel        0.214  dlam of 1x70x320x4-A (8.57e-04 / 7.79e-04)       0.171  dq of 2x257x33x2-B (5.12e-03 / 5.12e-03)
    k4lp   loss scale    0.142  dkp, dout * 2^12 (5.67e-04 / 5.62e-04)           0.112  dkp, dout * 2^-12 (3.37e-03 / 3.37e-03)
    flash  init          0.138  dq of 1x256x64x1 (4.04e-04 / 4.04e-04)           0.269  dv of 2x257x65x2 (3.15e-03 / 3.15e-03)
    flash  peaked-first  0.376  dk of 1x513x321x1 (1.10e-03 / 1.10e-03)          0.873  dk of 1x513x321x1 (1.02e-02 / 1.02e-02)
    flash  peaked-last   0.376  dk of 1x513x321x1 (1.10e-03 / 1.10e-03)          0.873  dk of 1x513x321x1 (1.02e-02 / 1.02e-02)
    flash  flat          0.112  out of 2x257x65x2 (3.29e-04 / 3.29e-04)          0.264  dv of 2x257x65x2 (3.09e-03 / 3.09e-03)
The kernels' errors are the yardsticks' to two or three digits: the documented roundings account for all of it, and no kernel had
to be changed.  Two entries differ from their yardstick: d(lam) of the single-key shape (zero but for eps, 1.5e-5 of its terms;
kernel 3.8e-3 / yardstick 9.3e-3 of |ref16| in fp16, 8.2e-3 / 4.9e-3 in bf16 -- the fp32 noise of the prologue, and the case whose
second term is the active one: 0.10 and 0.27 of the bound) and d(lam) of "cancel".  The 128-token-chunk case (2x3201x320x8, fp16) is
at 0.118 (dq).  The "peaked" fp16 cases show no sign of flushed subnormal softmax weights: kernel and yardstick (which keeps them)
agree to three digits.  The closed forms: "flat" K4lp within 0.005 and the shim within 0.03 of their bounds; the one-hot rows of
o1 / o2 of "peaked" equal the V row of their key to 1e-3 of the bound.  The shim's bf16 "peaked" dk stands at 0.87 of its three ulps:
backward-1 forms D = dout . out from the ROUNDED out, 2^-9 of a sum whose terms cancel in one-hot rows, times keys 5 times as large
as in "init"; the yardstick reproduces the figure, and with two token chunks the float atomics add in either order to the same sum.

A mutation of the key-side kernel that reads the k rows with d in place of kp_stride fails the parity, strided and loss-scale tests of
the strided shapes here while tests/test_pooled_attn_lp_gpu.py and tests/test_flash_shim_gpu.py still pass."""
import math

import pytest
import torch

from tests import _attention_lp_cases as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4                      # columns either side of the blocks of a wide row
SENTINEL = -12345.0


def _embed(blocks):
    """Tensors (..., w_i) -> (wide (..., 2 GUARD + sum w_i) filled with other numbers, [view of block i])."""
    total = 2 * GUARD + sum(b.shape[-1] for b in blocks)
    wide = torch.randn(*blocks[0].shape[:-1], total, device=DEV, generator=torch.Generator(DEV).manual_seed(total))
    views, c = [], GUARD
    for b in blocks:
        wide[..., c:c + b.shape[-1]] = b
        views.append(wide[..., c:c + b.shape[-1]])
        c += b.shape[-1]
    return wide, views


def _run_k4lp(case, strided=False):
    """The op on the device: (y, {leaf: gradient}) as float64 CPU tensors, the saved (o1, o2), and for a strided run the wide buffers."""
    from mlagg_unet_amd import ops
    lv = {k: t.to(DEV) for k, t in case["leaves"].items()}
    dout = case["dout"].to(DEV)
    extra = {}
    if strided:
        qwide, (lv["q"],) = _embed([lv["q"]])
        kvwide, (lv["kp"], lv["vp"]) = _embed([lv["kp"], lv["vp"]])
        dwide, (dout,) = _embed([dout])
        arena = ops._GradArena(qwide.shape, DEV)
        arena.buf = torch.full(qwide.shape, SENTINEL, device=DEV)
        lv["q"]._mlagg_slot = ops._GradSlot(arena, GUARD, lv["q"].shape[-1])
        wides = (qwide, kvwide, dwide)
        extra = dict(wides=wides, wides0=[w.clone() for w in wides], gbuf=arena.buf)
        for t in (lv["q"], lv["kp"], lv["vp"], dout):
            assert t.stride(-2) > t.shape[-1] and t.stride(-1) == 1
    for t in lv.values():
        t.requires_grad_(True)
    with ops.compute_precision(case["dt"]):
        y = ops.pooled_diff_attn(*lv.values(), case["nh"], case["scale"])
    assert type(y.grad_fn).__name__.startswith("PooledDiffAttnLpFn"), "ops.pooled_diff_attn did not reach K4lp"
    extra["o12"] = y.grad_fn.saved_tensors[6].detach().cpu().double()
    y.backward(dout)
    torch.cuda.synchronize()
    if strided:
        assert lv["q"]._mlagg_slot.claimed
    return y.detach().cpu().double(), {k: t.grad.detach().cpu().double() for k, t in lv.items()}, extra


def _check(cid, rows, bound_of):
    """rows of (name, kernel's, oracle's, yardstick's): error <= bound_of(name, oracle's, yardstick's) for each; the worst error / bound."""
    worst, report = 0.0, []
    for name, got, ref, em in rows:
        err, b = L.max_err(got, ref), bound_of(name, ref, em)
        report.append((name, err, b, bool(torch.isfinite(got).all())))
        worst = max(worst, err / b)
        print(f"parity {cid} {name}: kernel {L.scaled(err, ref):.2e} yardstick {L.scaled(L.max_err(em, ref), ref):.2e} of max|ref|, "
              f"error / bound {err / b:.3f}")
    for name, err, b, finite in report:
        assert finite, f"{cid} {name}: not finite"
        assert err <= b, f"{cid} {name}: error {err:.3e} / bound {b:.3e} = {err / b:.3f}"
    return worst


def _check_k4lp(cid, case, y, g):
    T = L.T_K4LP[case["dt"]]
    return _check(cid, L.k4lp_rows(case, y, g), lambda name, ref, em: L.k4lp_bound(ref, em, T))


def _check_k4lp_regime(cid, regime, case, y, o12):
    T = L.T_K4LP[case["dt"]]
    y_em = case["emul"][0]
    if regime == "flat":
        cf = L.k4lp_flat_closed_form(case)
        err, b = L.max_err(y, cf), L.k4lp_bound(cf, y_em, T)
        print(f"flat {cid}: max |y - closed form| / bound {err / b:.3f}")
        assert err <= b, f"{cid} closed form: error {err:.3e} / bound {b:.3e} = {err / b:.3f}"
    elif regime == "cancel":
        err, b = float(y.abs().max()), L.k4lp_bound(torch.zeros_like(y), y_em, T)
        assert err <= b, f"{cid} output of A == 0: {err:.3e} / bound {b:.3e} = {err / b:.3f}"
    elif regime == "peaked":
        parts, v16 = L.k4lp_parts(case)
        B, N, nh, _, P = parts["s"].shape
        top, idx = parts["s"].max(-1)                                              # (B, N, nh, 2)
        want = v16.reshape(B, P, nh, L.HD2)[torch.arange(B).view(B, 1, 1, 1), idx, torch.arange(nh).view(1, 1, nh, 1)]
        got = o12.reshape(2, B, N, nh, L.HD2).permute(1, 2, 3, 0, 4)
        hot = top >= 1 - 1e-6                                                      # weight 1 to 16 bits, the rest below 1e-6 in all
        lg = L.pooled_logits16(case["leaves"]["q"], case["leaves"]["kp"], nh, case["scale"], case["dt"])
        b_, n_, p_, h_, m_ = (int(i) for i in torch.unravel_index(lg.argmax(), lg.shape))
        assert bool(hot[b_, n_, h_, m_]) and int(idx[b_, n_, h_, m_]) == p_, "the row of the extreme logit is not one-hot at its key"
        err, b = float((got - want).abs().amax(-1)[hot].max()), T * float(v16.abs().max())
        print(f"peaked {cid}: {int(hot.sum())} one-hot rows of {hot.numel()}, max |o_r - v[key]| / bound {err / b:.3f}")
        assert err <= b, f"{cid} one-hot rows: error {err:.3e} / bound {b:.3e} = {err / b:.3f}"


@pytest.mark.parametrize("regime,shape,dt,place", L.K4LP_CASES, ids=L.K4LP_IDS)
def test_k4lp_matches_the_float64_oracle_on_rounded_operands(regime, shape, dt, place):
    case, cid = L.k4lp_case(regime, shape, dt, place), L.k4lp_id(regime, shape, dt, place)
    y, g, ex = _run_k4lp(case, strided=shape[-1])
    _check_k4lp(cid, case, y, g)
    _check_k4lp_regime(cid, regime, case, y, ex["o12"])


def test_k4lp_chunk_case_takes_128_token_chunks():
    """(workspace - 52 units - 49 ceil(units / 256)) / (96 B nh P) is the number of token chunks of the key-side kernel: 26 chunks of 128
    tokens for N = 3201 (51 if a change of the chunk rule made them 64 again)."""
    from mlagg_unet_amd import _lib
    B, N, P, nh = L.K4LP_CHUNK_SHAPE[:4]
    units = B * N * nh
    rest = int(_lib.lib().mlagg_pooled_attn_lp_bwd_workspace_floats(B, N, P, nh)) - 52 * units - 49 * math.ceil(units / 256)
    assert rest % (96 * B * nh * P) == 0 and rest // (96 * B * nh * P) == 26 == math.ceil(N / 128)
    for Bs, Ns, Ps, nhs in (s[:4] for s in L.K4LP_SHAPES[:6]):                     # every other shape: 64-token chunks
        us = Bs * Ns * nhs
        rest = int(_lib.lib().mlagg_pooled_attn_lp_bwd_workspace_floats(Bs, Ns, Ps, nhs)) - 52 * us - 49 * math.ceil(us / 256)
        assert rest == 96 * Bs * nhs * Ps * math.ceil(Ns / 64)


STRIDED = [("init", s, dt, None) for dt in L.DTYPES for s in L.K4LP_SHAPES if s[-1]]


@pytest.mark.parametrize("regime,shape,dt,place", STRIDED, ids=[L.k4lp_id(*c) for c in STRIDED])
def test_k4lp_strided_operands_equal_the_contiguous_call_bit_for_bit(regime, shape, dt, place):
    case = L.k4lp_case(regime, shape, dt, place)
    y, g, _ = _run_k4lp(case)
    ys, gs, ex = _run_k4lp(case, strided=True)
    assert torch.equal(y, ys), "y"
    for k in L.K4LP_LEAVES:
        assert torch.equal(g[k], gs[k]), k
    # the query-side kernel wrote dq into its column block of the shared buffer and nothing else
    gbuf, w = ex["gbuf"].cpu().double(), g["q"].shape[-1]
    assert torch.equal(gbuf[..., GUARD:GUARD + w], g["q"]), "dq in the shared buffer"
    assert bool((gbuf[..., :GUARD] == SENTINEL).all()) and bool((gbuf[..., GUARD + w:] == SENTINEL).all()), "columns outside dq's block were written"
    assert all(torch.equal(a, b) for a, b in zip(ex["wides"], ex["wides0"])), "an input was modified"


@pytest.mark.parametrize("shape,dt", [(L.K4LP_SHAPES[4], "fp16"), (L.K4LP_SHAPES[5], "bf16")], ids=["fp16-2x257x33x2", "bf16-1x70x320x4"])
def test_k4lp_two_runs_are_bit_identical(shape, dt):
    case = L.k4lp_case("init", shape, dt)
    ya, ga, _ = _run_k4lp(case)
    yb, gb, _ = _run_k4lp(case)
    assert torch.equal(ya, yb)
    for k in L.K4LP_LEAVES:
        assert torch.equal(ga[k], gb[k]), k


@pytest.mark.parametrize("dt", list(L.DTYPES))
def test_k4lp_under_a_loss_scale(dt):
    case = L.k4lp_loss_case(dt)
    y, g, _ = _run_k4lp(case, strided=L.LOSS_SHAPE[-1])
    _check_k4lp(f"k4lp-{dt}-loss-scale-2^{int(math.log2(L.LOSS_SCALE[dt]))}", case, y, g)


# ------------------------------------------------------------------------------------------------
# flash shim
# ------------------------------------------------------------------------------------------------
def _run_flash(case):
    import mlagg_unet_amd.shims as shims
    lv = {k: t.to(DEV).requires_grad_(True) for k, t in case["leaves"].items()}
    out = shims.flash_attn_func(*lv.values(), causal=False)                    # default softmax_scale = 24^-0.5, as the reference relies on
    assert out.dtype == L.DTYPES[case["dt"]] and out.shape == lv["q"].shape
    out.backward(case["dout"].to(DEV))
    torch.cuda.synchronize()
    assert all(t.grad.dtype == out.dtype for t in lv.values())
    return out.detach().cpu().double(), {k: t.grad.detach().cpu().double() for k, t in lv.items()}


@pytest.mark.parametrize("regime,shape,dt,place", L.FLASH_CASES, ids=L.FLASH_IDS)
def test_flash_shim_matches_exact_attention(regime, shape, dt, place):
    case, cid = L.flash_case(regime, shape, dt, place), L.flash_id(regime, shape, dt, place)
    out, g = _run_flash(case)
    _check(cid, L.flash_rows(case, out, g), lambda name, ref, em: L.flash_bound(ref, dt))
    if regime == "flat":
        cf = L.flash_flat_closed_form(case)
        err, b = L.max_err(out, cf), L.flash_bound(cf, dt)
        print(f"flat {cid}: max |out - round16(mean(v))| / bound {err / b:.3f}")
        assert err <= b, f"{cid} closed form: error {err:.3e} / bound {b:.3e} = {err / b:.3f}"


def test_flash_shim_out_and_dq_are_bit_identical_between_runs():
    case = L.flash_case("init", L.FLASH_SHAPES[4], "bf16")
    (oa, ga), (ob, gb) = _run_flash(case), _run_flash(case)
    assert torch.equal(oa, ob) and torch.equal(ga["q"], gb["q"])


def test_flash_shim_refuses_more_than_512_keys():
    import mlagg_unet_amd.shims as shims
    q, k = torch.zeros(1, 2, 1, L.E, device=DEV, dtype=torch.float16), torch.zeros(1, 513, 1, L.E, device=DEV, dtype=torch.float16)
    with pytest.raises(RuntimeError):
        shims.flash_attn_func(q, k, k.clone())
    torch.cuda.synchronize()
