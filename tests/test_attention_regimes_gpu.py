"""GPU parity of the three fp32 kernels on the hot path of every MLLA block -- K3 (csrc/local_attn.hip, ops.local_diff_attn), K4
(csrc/pooled_attn.hip, ops.pooled_diff_attn in fp32 mode) and K7 (csrc/gate.hip, ops.gate) -- one operation at a time against the
float64 references of tests/_attention_cases.py (whose soundness tests/test_attention_regimes_cpu.py checks without a GPU), at the
geometry seams of the kernels and outside the O(1)-logit regime of the module tests.

(a) Parity.  Every output and every gradient against the float64 oracle.  Per tensor the absolute bound is
    max(T max|ref|, 4 max|plain_fp32 - ref|), plus the module test's rtol; T is the tolerance of
    test_blocks_gpu.py::test_aggregated_attention_matches_oracle (2e-5 output, 5e-5 dq / dk / dv, 2e-4 parameter gradients), the
    factor 4 the margin the scan tests give a kernel that rounds in another order than the plain loop; the second term comes from
    the two references alone.  Regimes "peaked" (largest logit +100), "flat" (k = 0; also against the closed form
    (1 - lam) mean(v) through the norm) and "cancel" (A == 0: K4's output exactly 0, K3's the LePE term, gradients finite).
(b) K7 sweep over act in [-80, 80], element-wise: relative tolerance 2^-20 (4 + |act|) of the value (y, da) or of the
    condition-aware magnitude |dout a| s (1 + |act| (1 - s)) (dact), floor 1e-37.
(c) Strided operands (q / kv / dout, act / dout as column blocks of wider rows, gradients written into a column block of a wider
    buffer as ops.split_cols arranges it in the model): bit-identical to the contiguous call, nothing outside the block touched.
(d) Two runs of K3 and of K4 are bit-identical (trainer.set_deterministic relies on the fixed-order reductions).
(e) P = 427 keys (K and V past the 160 KiB of LDS) is refused on the host: mlagg_pooled_attn_fwd forms kv_lds_bytes = 2 * 427 * 48 * 4
    = 163 968 > 163 840 and allow_lds returns MLAGG_E_UNSUPPORTED before any launch.

Every parity test prints, per tensor, the max-scaled error of the kernel and of the plain float32 reference, their ratio and
error / bound (run with -s).

Measured on an MI355X: max-scaled error of the kernel / of the plain float32 reference per tensor (0.0e+00 / 0.0e+00: both exactly
equal to the oracle), and the largest error / bound of the case with its tensor.  The kernels are at 1e-7 .. 1e-5 of max|ref|, like the plain float32
reference; T max|ref| is the active term of every bound except for d(lam) of the
single-key shapes and of "flat", a cancelling zero (|ref| ~ 1e-6 of its terms), where 4 max|plain - ref| is.  One entry is within
2x of its bound: d(lam) of k3-init-2x1x1x1 at 0.57 of it, a kernel error of 0.38 |ref| against the plain reference's 0.17 |ref| on
a value of 1e-6 that is zero but for eps; everything else is below 0.4 of its bound, and all but d(lam) and "peaked" below 0.1.
    case                             y                dq              dkv              dlam           dsubln_w         dlepe_w          dlepe_b       worst error / bound
    k3-init-2x1x1x1           7.8e-08/4.1e-08  0.0e+00/0.0e+00  6.7e-08/4.3e-08  3.8e-01/1.7e-01  1.2e-07/5.4e-08  4.7e-08/4.7e-08  3.6e-08/3.6e-08   0.565 (dlam)
    k3-init-2x1x3x1           6.9e-08/9.5e-08  1.5e-06/7.0e-07  1.0e-07/7.8e-08  1.2e-08/1.3e-07  9.6e-08/2.2e-07  9.3e-08/9.3e-08  6.1e-08/1.0e-07   0.029 (dq)
    k3-init-1x3x1x2           7.8e-08/7.8e-08  2.5e-07/3.7e-07  9.4e-08/9.2e-08  2.0e-07/2.0e-07  7.3e-08/8.5e-08  1.1e-07/1.1e-07  5.0e-08/5.0e-08   0.005 (dq)
    k3-init-1x8x8x1           1.2e-07/1.5e-07  1.7e-07/1.9e-07  1.1e-07/1.0e-07  3.0e-07/6.6e-07  1.6e-07/1.5e-07  8.0e-08/1.1e-07  1.2e-07/7.9e-08   0.006 (y)
    k3-init-2x9x8x2           1.0e-07/1.2e-07  1.8e-07/2.0e-07  1.1e-07/9.3e-08  7.4e-07/2.2e-06  1.3e-07/1.4e-07  1.4e-07/1.1e-07  1.5e-07/1.3e-07   0.005 (y)
    k3-init-1x7x17x4          9.0e-08/9.8e-08  7.1e-07/3.3e-07  2.0e-07/1.7e-07  5.8e-08/1.8e-07  1.1e-07/1.4e-07  1.1e-07/1.2e-07  9.0e-08/9.3e-08   0.014 (dq)
    k3-init-1x16x16x1         1.0e-07/1.1e-07  1.5e-07/1.9e-07  1.2e-07/1.2e-07  6.3e-07/1.5e-07  1.8e-07/1.3e-07  1.4e-07/2.2e-07  1.1e-07/1.1e-07   0.005 (y)
    k3-peaked-2x9x8x2         3.0e-07/2.9e-07  3.4e-06/3.7e-06  1.6e-06/1.7e-06  9.4e-07/5.6e-07  3.1e-07/4.2e-07  1.1e-07/9.4e-08  1.2e-07/1.1e-07   0.068 (dq)
    k3-peaked-1x7x17x4        4.2e-07/2.1e-07  1.9e-06/9.8e-07  2.4e-06/1.1e-06  2.3e-06/3.0e-06  3.4e-07/3.9e-07  1.4e-07/1.1e-07  7.7e-08/7.4e-08   0.048 (dkv)
    k3-flat-2x9x8x2           7.3e-08/1.1e-07  0.0e+00/0.0e+00  1.9e-07/2.3e-07  1.3e-04/2.1e-04  1.4e-07/2.0e-07  9.9e-08/1.1e-07  1.2e-07/1.0e-07   0.155 (dlam)
    k3-flat-1x7x17x4          9.1e-08/1.2e-07  0.0e+00/0.0e+00  1.3e-07/1.7e-07  5.6e-05/4.5e-05  1.1e-07/1.6e-07  1.3e-07/1.0e-07  8.7e-08/1.5e-07   0.282 (dlam)
    k3-cancel-2x9x8x2         8.9e-08/1.2e-07  1.1e-07/1.8e-07  2.4e-07/1.9e-07  1.7e-06/1.4e-06  0.0e+00/0.0e+00  1.4e-07/1.5e-07  9.0e-08/9.6e-08   0.008 (dlam)
    k3-cancel-1x7x17x4        8.0e-08/8.1e-08  2.2e-07/2.8e-07  1.5e-07/2.4e-07  3.8e-08/3.8e-08  0.0e+00/0.0e+00  8.0e-08/1.0e-07  8.4e-08/1.1e-07   0.004 (y)
    case                             y                dq              dkp              dvp              dlam           dsubln_w      worst error / bound
    k4-init-2x1x1x1-B         1.2e-07/8.3e-08  0.0e+00/0.0e+00  0.0e+00/0.0e+00  1.0e-07/7.7e-08  6.4e-02/9.6e-02  6.8e-08/7.5e-08   0.167 (dlam)
    k4-init-2x127x49x2-A      1.4e-06/4.3e-07  7.1e-07/2.5e-07  5.8e-07/2.5e-07  8.3e-07/4.2e-07  2.4e-06/4.9e-07  7.3e-07/2.1e-07   0.070 (y)
    k4-init-1x128x64x1-B      2.8e-07/2.3e-07  2.7e-07/3.7e-07  3.3e-07/2.5e-07  2.4e-07/3.1e-07  7.9e-07/2.7e-07  3.9e-07/1.8e-07   0.014 (y)
    k4-init-2x129x65x2-B      5.5e-07/3.7e-07  5.2e-07/3.2e-07  3.6e-07/2.3e-07  3.3e-07/2.5e-07  9.3e-07/1.8e-07  4.4e-07/3.3e-07   0.028 (y)
    k4-init-1x300x128x1-A     7.3e-07/4.9e-07  4.3e-07/2.1e-07  3.0e-07/1.8e-07  3.2e-07/3.6e-07  5.8e-05/1.7e-05  2.8e-07/2.0e-07   0.292 (dlam)
    k4-init-1x300x129x4-B     9.3e-07/4.9e-07  6.9e-07/3.1e-07  5.5e-07/2.6e-07  3.7e-07/3.2e-07  1.2e-06/1.1e-07  3.7e-07/3.0e-07   0.046 (y)
    k4-init-1x257x320x1-A     9.4e-07/4.9e-07  5.8e-07/2.7e-07  3.0e-07/2.0e-07  3.6e-07/3.1e-07  1.2e-05/4.2e-06  3.1e-07/1.7e-07   0.062 (dlam)
    k4-peaked-2x129x65x2-B    2.0e-06/2.3e-06  3.3e-06/3.2e-06  6.4e-06/3.7e-06  6.6e-06/7.3e-07  2.9e-06/1.3e-07  7.0e-07/5.5e-07   0.133 (dvp)
    k4-peaked-1x300x129x4-B   2.0e-06/2.2e-06  3.3e-06/9.0e-06  7.1e-06/9.7e-06  2.8e-06/7.0e-07  1.8e-06/3.2e-07  8.7e-07/7.7e-07   0.142 (dkp)
    k4-flat-2x129x65x2-B      2.4e-07/2.8e-07  0.0e+00/0.0e+00  2.1e-07/1.8e-07  2.3e-07/3.9e-07  6.5e-05/3.2e-05  4.7e-07/3.4e-07   0.323 (dlam)
    k4-flat-1x300x129x4-B     2.9e-07/2.7e-07  0.0e+00/0.0e+00  2.0e-07/2.1e-07  1.3e-07/2.9e-07  4.8e-06/8.1e-06  2.1e-07/2.6e-07   0.024 (dlam)
    k4-cancel-2x129x65x2-B    0.0e+00/0.0e+00  4.8e-07/4.0e-07  4.3e-07/3.5e-07  0.0e+00/0.0e+00  1.1e-07/1.7e-09  0.0e+00/0.0e+00   0.010 (dq)
    k4-cancel-1x300x129x4-B   0.0e+00/0.0e+00  7.0e-07/7.5e-07  4.5e-07/5.1e-07  0.0e+00/0.0e+00  8.5e-09/8.8e-08  0.0e+00/0.0e+00   0.014 (dq)
    case                             y               da0              da1              dact        worst error / bound
    k7-1x4                    1.2e-08/1.2e-08  5.3e-08/4.9e-08  4.1e-08/4.1e-08  1.7e-07/1.7e-07   0.003 (dact)
    k7-257x48                 4.8e-08/4.8e-08  4.8e-08/4.8e-08  4.8e-08/4.8e-08  8.5e-07/8.5e-07   0.017 (dact)
    k7-130x100                4.8e-08/4.8e-08  4.8e-08/4.8e-08  4.7e-08/4.7e-08  6.4e-07/6.4e-07   0.013 (dact)
    k7-5500x384               4.8e-08/4.8e-08  4.8e-08/4.8e-08  4.8e-08/4.8e-08  8.5e-07/8.5e-07   0.017 (dact)
    K7 sweep, worst element-wise error / tolerance, kernel / plain fp32:
    k7-1x4                   y 0.029 / 0.005         da 0.029 / 0.007        dact 0.029 / 0.012      
    k7-257x48                y 0.071 / 0.035         da 0.071 / 0.031        dact 0.068 / 0.056      
    k7-130x100               y 0.068 / 0.033         da 0.068 / 0.031        dact 0.066 / 0.053      
    k7-5500x384              y 0.073 / 0.045         da 0.073 / 0.042        dact 0.069 / 0.066      
    "flat" output against the closed form, max-scaled: k3-flat-2x9x8x2 7.30e-08, k3-flat-1x7x17x4 9.09e-08, k4-flat-2x129x65x2-B 2.38e-07, k4-flat-1x300x129x4-B 2.86e-07

Where a reference gradient is identically zero and the plain float32 reference gives exactly zero too, the bound is zero and the
kernel has to give exactly zero: dq of "flat" (k = 0), and dq and dk of the single-key shapes (a softmax over one key is 1 whatever
the logit is).  k4-init-2x1x1x1-B found K4's backward off there, absolute errors against a reference of 0:
                       dq         dkp
    before the fix   1.7e-13    5.1e-08
    after the fix    0          0
dkp: backward-2 formed s (d(o) . v - D) from a d(o) . v summed in another order than the one backward-1 had summed into D, and fused
-lam d(o) . v with D in one FMA, so the two did not cancel and left the rounding of a 48-term sum of O(1) products times q; dq:
backward-1 fused U - D V into an FMA, which subtracts an exact D V from a rounded U.  csrc/pooled_attn.hip now sums d(o) . v with one
function in both kernels and forms both differences without FMA.
"""
import numpy as np
import pytest
import torch

from tests import _attention_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4                      # columns either side of the blocks of a wide row
SENTINEL = -12345.0

FN = {"k3": "local_diff_attn", "k4": "pooled_diff_attn", "k7": "gate"}
WIDE = {"k3": ("q", "kv"), "k4": ("q",), "k7": ("act",)}       # operands that are column blocks of ONE wide row in the strided runs


def _embed(blocks):
    """Tensors (..., w_i) -> (wide (..., 2 GUARD + sum w_i) filled with other numbers, [view of block i])."""
    lead = blocks[0].shape[:-1]
    total = 2 * GUARD + sum(b.shape[-1] for b in blocks)
    wide = torch.randn(*lead, total, device=DEV, generator=torch.Generator(DEV).manual_seed(total))
    views, c = [], GUARD
    for b in blocks:
        wide[..., c:c + b.shape[-1]] = b
        views.append(wide[..., c:c + b.shape[-1]])
        c += b.shape[-1]
    return wide, views


def _run(kind, case, strided=False):
    """The op on the device: (y, {leaf: gradient}) as float64 CPU tensors, and for a strided run the dict of wide buffers."""
    from mlagg_unet_amd import ops
    assert ops.compute_dtype() == torch.float32, "a 16-bit compute mode is active: ops.pooled_diff_attn would not reach K4"
    lv = {k: t.to(DEV) for k, t in case["leaves"].items()}
    dout = case["dout"].to(DEV)
    extra = None
    if strided:
        wide, views = _embed([lv[k] for k in WIDE[kind]])
        dwide, (dout,) = _embed([dout])
        arena = ops._GradArena(wide.shape, DEV)
        arena.buf = torch.full(wide.shape, SENTINEL, device=DEV)
        extra = dict(wide=wide, wide0=wide.clone(), dwide=dwide, dwide0=dwide.clone(), gbuf=arena.buf, cols={})
        c = GUARD
        for k, v in zip(WIDE[kind], views):
            assert v.stride(-2) == wide.shape[-1] > v.shape[-1]
            lv[k] = v
            v._mlagg_slot = ops._GradSlot(arena, c, v.shape[-1])
            extra["cols"][k] = (c, v.shape[-1])
            c += v.shape[-1]
    for t in lv.values():
        t.requires_grad_(True)
    y = getattr(ops, FN[kind])(*lv.values(), *case.get("geom", ()))
    y.backward(dout)
    torch.cuda.synchronize()
    if strided:
        assert all(lv[k]._mlagg_slot.claimed for k in WIDE[kind])
    return y.detach().cpu().double(), {k: t.grad.detach().cpu().double() for k, t in lv.items()}, extra


def _rows(kind, case, y, g):
    (y_ref, g_ref), (y32, g32) = case["ref"], case["plain"]
    return [("y", y, y_ref, y32)] + [(k, g[k], g_ref[k], g32[k]) for k in C.LEAVES[kind]]


def _check_parity(cid, kind, case, y, g):
    rows = _rows(kind, case, y, g)
    for name, got, ref, plain in rows:
        T, _ = C.tol_of(name)
        ek, ep, b = C.max_err(got, ref), C.max_err(plain, ref), C.bound(ref, plain, T)
        print(f"parity {cid} {'' if name == 'y' else 'd'}{name}: kernel {C.scaled(ek, ref):.2e} plain {C.scaled(ep, ref):.2e} "
              f"ratio {ek / max(ep, 1e-300):.2f} error/bound {ek / b if b else float(ek > 0):.3f}")
    for name, got, ref, plain in rows:
        assert bool(torch.isfinite(got).all()), name
        T, rtol = C.tol_of(name)
        np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=C.bound(ref, plain, T), rtol=rtol, err_msg=f"{cid} {name}")


def _check_regime(cid, kind, regime, case, y):
    T, rtol = C.TOL_Y
    y_ref, y32 = case["ref"][0], case["plain"][0]
    if regime == "flat":
        cf = C.flat_closed_form(kind, case)
        print(f"flat {cid}: max |y - closed form| / max|y| {C.scaled(C.max_err(y, cf), cf):.2e}")
        np.testing.assert_allclose(y.numpy(), cf.numpy(), atol=C.bound(cf, y32, T), rtol=rtol, err_msg=f"{cid} closed form")
    if regime == "cancel":
        if kind == "k4":
            assert float(y.abs().max()) == 0.0, f"{cid}: the output is not exactly zero"
        else:
            lp = C.lepe_only(case)
            np.testing.assert_allclose(y.numpy(), lp.numpy(), atol=C.bound(lp, y32, T), rtol=rtol, err_msg=f"{cid} LePE only")


@pytest.mark.parametrize("regime,shape", C.K3_CASES, ids=C.K3_IDS)
def test_local_attn_matches_float64_reference(regime, shape):
    case = C.local_case(regime, shape)
    y, g, _ = _run("k3", case)
    _check_parity(C.k3_id(regime, shape), "k3", case, y, g)
    _check_regime(C.k3_id(regime, shape), "k3", regime, case, y)


@pytest.mark.parametrize("regime,shape", C.K4_CASES, ids=C.K4_IDS)
def test_pooled_attn_matches_float64_reference(regime, shape):
    case = C.pooled_case(regime, shape)
    y, g, _ = _run("k4", case)
    _check_parity(C.k4_id(regime, shape), "k4", case, y, g)
    _check_regime(C.k4_id(regime, shape), "k4", regime, case, y)


@pytest.mark.parametrize("shape", C.K7_SHAPES, ids=C.K7_IDS)
def test_gate_sweep_matches_float64_reference_elementwise(shape):
    case = C.gate_case(shape)
    y, g, _ = _run("k7", case)
    cid = f"k7-{shape[0]}x{shape[1]}"
    (y_ref, g_ref), (y32, g32) = case["ref"], case["plain"]
    cat = lambda d: torch.cat([d["a0"], d["a1"]], -1)                                               # noqa: E731
    tol = C.gate_tolerances(case)
    rows = [("y", y, y_ref, y32), ("da", cat(g), cat(g_ref), cat(g32)), ("dact", g["act"], g_ref["act"], g32["act"])]
    for name, got, ref, plain in rows:
        rk, rp = float(((got - ref).abs() / tol[name]).max()), float(((plain - ref).abs() / tol[name]).max())
        print(f"sweep {cid} {name}: worst error / tolerance: kernel {rk:.3f} plain {rp:.3f}")
    for name, got, ref, plain in rows:
        assert bool(torch.isfinite(got).all()), name
        bad = (got - ref).abs() > tol[name]
        assert not bool(bad.any()), (f"{cid} {name}: {int(bad.sum())} elements off, the first at act = "
                                     f"{float(case['leaves']['act'].reshape(-1)[bad.reshape(-1).nonzero()[0, 0]])}")
    _check_parity(cid, "k7", case, y, g)


STRIDED = ([("k3", "init", s) for s in C.K3_SHAPES if s[-1]] + [("k4", "init", s) for s in C.K4_SHAPES if s[-1]] +
           [("k7", None, s) for s in C.K7_SHAPES if s[-1]])


def _case_id(kind, regime, shape):
    """The id alone: nothing is computed at collection."""
    return f"k7-{shape[0]}x{shape[1]}" if kind == "k7" else (C.k3_id if kind == "k3" else C.k4_id)(regime, shape)


def _any_case(kind, regime, shape):
    case = C.gate_case(shape) if kind == "k7" else (C.local_case if kind == "k3" else C.pooled_case)(regime, shape)
    return case, _case_id(kind, regime, shape)


@pytest.mark.parametrize("kind,regime,shape", STRIDED, ids=[_case_id(*p) for p in STRIDED])
def test_strided_operands_equal_the_contiguous_call_bit_for_bit(kind, regime, shape):
    case, cid = _any_case(kind, regime, shape)
    y, g, _ = _run(kind, case)
    ys, gs, ex = _run(kind, case, strided=True)
    assert torch.equal(y, ys), "y"
    for k in C.LEAVES[kind]:
        assert torch.equal(g[k], gs[k]), k
    # the kernels wrote the gradients of the wide operands into their column blocks of the shared buffer and nothing else
    gbuf = ex["gbuf"].cpu().double()
    keep = torch.ones(gbuf.shape[-1], dtype=torch.bool)
    for k, (c, w) in ex["cols"].items():
        assert torch.equal(gbuf[..., c:c + w], g[k]), f"d{k} in the shared buffer"
        keep[c:c + w] = False
    assert int(keep.sum()) == 2 * GUARD and bool((gbuf[..., keep] == SENTINEL).all()), "columns outside the blocks were written"
    assert torch.equal(ex["wide"], ex["wide0"]) and torch.equal(ex["dwide"], ex["dwide0"]), "an input was modified"


@pytest.mark.parametrize("kind,shape", [("k3", C.K3_SHAPES[5]), ("k4", C.K4_SHAPES[1])], ids=["k3-1x7x17x4", "k4-2x127x49x2"])
def test_two_runs_are_bit_identical(kind, shape):
    case, _ = _any_case(kind, "init", shape)
    ya, ga, _ = _run(kind, case)
    yb, gb, _ = _run(kind, case)
    assert torch.equal(ya, yb)
    for k in C.LEAVES[kind]:
        assert torch.equal(ga[k], gb[k]), k


def test_pooled_attn_refuses_keys_that_do_not_fit_in_lds():
    from mlagg_unet_amd import ops
    P = 427                                                   # 2 * 427 * 48 * 4 bytes = 163 968 > 160 KiB
    assert 2 * P * C.HD2 * 4 > 160 * 1024 >= 2 * (P - 1) * C.HD2 * 4
    q, k = torch.zeros(1, 1, 48, device=DEV), torch.zeros(1, P, 48, device=DEV)
    with pytest.raises(RuntimeError):
        ops.pooled_diff_attn(q, k, k.clone(), torch.tensor(0.8, device=DEV), torch.ones(48, device=DEV), 1, C.SCALE_B)
    torch.cuda.synchronize()
