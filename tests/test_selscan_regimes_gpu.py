"""GPU parity of the three selective-scan kernel families (K1 csrc/selscan.hip, K1f csrc/selscan_tok.hip, K1s csrc/selscan1.hip)
against the double-precision oracle (oracle/selscan_ref.c) OUTSIDE the regime of their shape tests, on the cases of
tests/_selscan_regime_cases.py (whose soundness tests/test_selscan_regimes_cpu.py checks without a GPU).

(a) Memoryless sweep: A = -1e30 wipes the state at every step, so every step probes softplus and its derivative at one argument
    between -16 and 24 (with the branch points of the implementations).  All operands are positive, so y, du, d(delta) (or row 0
    of d(dtr)), dB, dC, dD and d(bias) are compared ELEMENT-WISE, atol = 0, at the project's rtol (1e-4 forward, 1e-3 backward);
    dA must be exactly 0; dWdt and the unused rank rows are cancelling sums or zero and keep the max-scaled 3e-4.
(b) Regimes with memory ("init": the reference's S4D-real A and dt in [1e-3, 1e-1]; "large_step": delta A down to -160;
    "integrator": A = -1e-4), max-scaled like the shape tests.  Per tensor the absolute bound is the larger of the shape tests'
    (1e-4 max|y|; 2e-4 max|grad|, 3e-4 for K1 low-rank and K1f) and FOUR times the max error of a plain sequential float32 scan on
    the same inputs (tests/_selscan_regime_cases.plain_fp32_scan; the chunked kernels round a state at tile entry, chunk entry
    and in the prefix where the loop rounds once).  The second term comes from the two references alone.
(c) K1f and the group form of K1 are bit-reproducible.

Measured on an MI355X: max-scaled error of the kernel / of the plain fp32 scan (their ratio).  Every kernel error is at most
1.4e-6, two orders under the first term of the bound (1e-4 / 2e-4 / 3e-4), which is therefore the active one everywhere; the
kernels are within 0.1x .. 12x of the sequential fp32 loop, worst in "init" where the loop itself is at 1e-7.
    case                        tensor               init                       large_step                    integrator
    lowrank-1x2x96x1100x3       y         3.2e-07 / 1.1e-07 ( 3.00)    2.9e-07 / 9.6e-08 ( 3.00)    8.1e-07 / 1.0e-06 ( 0.77)
                                du        4.2e-07 / 1.1e-07 ( 3.81)    2.0e-07 / 1.0e-07 ( 2.00)    4.8e-07 / 6.4e-07 ( 0.75)
                                ddtr      9.0e-07 / 1.5e-07 ( 6.04)    3.8e-07 / 1.2e-07 ( 3.16)    7.2e-07 / 6.6e-07 ( 1.08)
                                dWdt      6.7e-07 / 1.3e-07 ( 5.33)    3.0e-07 / 1.1e-07 ( 2.74)    1.0e-06 / 1.3e-06 ( 0.77)
                                dA        7.1e-07 / 5.4e-07 ( 1.31)    1.5e-07 / 6.0e-07 ( 0.25)    7.9e-07 / 1.3e-06 ( 0.60)
                                dB        1.3e-06 / 2.6e-07 ( 4.90)    1.1e-07 / 1.4e-07 ( 0.83)    7.0e-07 / 8.2e-07 ( 0.85)
                                dC        8.4e-07 / 2.2e-07 ( 3.88)    7.8e-08 / 1.1e-07 ( 0.73)    8.8e-07 / 1.0e-06 ( 0.87)
                                dD        1.8e-07 / 7.2e-07 ( 0.25)    1.4e-07 / 6.5e-07 ( 0.22)    1.3e-07 / 7.9e-07 ( 0.17)
                                dbias     7.4e-07 / 1.9e-07 ( 3.95)    3.6e-07 / 1.8e-07 ( 2.00)    1.1e-06 / 9.4e-07 ( 1.12)
    lowrank-1x1x160x200x4       y         1.7e-07 / 7.5e-08 ( 2.25)    1.6e-07 / 1.6e-07 ( 1.00)    7.8e-07 / 4.4e-07 ( 1.75)
                                du        3.3e-07 / 8.2e-08 ( 4.00)    1.6e-07 / 1.6e-07 ( 1.00)    7.8e-07 / 4.7e-07 ( 1.67)
                                ddtr      7.0e-07 / 1.7e-07 ( 4.26)    3.0e-07 / 8.0e-08 ( 3.75)    1.1e-06 / 4.1e-07 ( 2.62)
                                dWdt      4.9e-07 / 9.1e-08 ( 5.44)    2.4e-07 / 1.3e-07 ( 1.88)    5.0e-07 / 2.4e-07 ( 2.06)
                                dA        9.2e-07 / 3.4e-07 ( 2.67)    2.2e-07 / 3.6e-07 ( 0.61)    8.7e-07 / 9.3e-07 ( 0.94)
                                dB        9.2e-07 / 1.7e-07 ( 5.50)    1.0e-07 / 1.2e-07 ( 0.84)    5.9e-07 / 3.3e-07 ( 1.79)
                                dC        9.1e-07 / 2.5e-07 ( 3.57)    1.1e-07 / 1.1e-07 ( 1.00)    8.4e-07 / 5.7e-07 ( 1.47)
                                dD        1.2e-07 / 4.1e-07 ( 0.29)    1.2e-07 / 3.9e-07 ( 0.31)    8.6e-08 / 2.6e-07 ( 0.33)
                                dbias     5.9e-07 / 1.1e-07 ( 5.33)    1.2e-07 / 1.2e-07 ( 1.00)    8.1e-07 / 3.4e-07 ( 2.40)
    direct-1x2x96x1100          y         2.3e-07 / 9.0e-08 ( 2.61)    1.3e-07 / 1.3e-07 ( 1.00)    7.6e-07 / 1.5e-06 ( 0.52)
                                du        3.4e-07 / 8.3e-08 ( 4.12)    1.1e-07 / 1.1e-07 ( 1.06)    5.2e-07 / 8.0e-07 ( 0.66)
                                ddelta    6.3e-07 / 1.1e-07 ( 5.62)    6.0e-07 / 1.0e-07 ( 6.00)    1.4e-06 / 1.1e-06 ( 1.33)
                                dA        7.7e-07 / 4.4e-07 ( 1.74)    1.8e-07 / 8.7e-07 ( 0.20)    1.3e-06 / 1.7e-06 ( 0.77)
                                dB        1.1e-06 / 1.7e-07 ( 6.13)    5.8e-08 / 8.6e-08 ( 0.67)    7.8e-07 / 1.1e-06 ( 0.69)
                                dC        1.1e-06 / 2.2e-07 ( 4.84)    1.1e-07 / 2.1e-07 ( 0.53)    8.7e-07 / 1.1e-06 ( 0.80)
                                dD        9.6e-08 / 1.1e-06 ( 0.09)    1.4e-07 / 1.1e-06 ( 0.12)    1.5e-07 / 1.9e-06 ( 0.08)
                                dbias     5.2e-07 / 1.4e-07 ( 3.77)    1.5e-07 / 1.1e-07 ( 1.33)    9.4e-07 / 7.8e-07 ( 1.21)
    msmm-1x32.32+8.8            y         1.5e-07 / 5.7e-08 ( 2.62)    1.1e-07 / 1.1e-07 ( 1.00)    8.0e-07 / 1.0e-06 ( 0.79)
                                dxc       2.8e-07 / 7.8e-08 ( 3.59)    1.9e-07 / 1.8e-07 ( 1.08)    7.8e-07 / 1.1e-06 ( 0.68)
                                dxdbl     7.6e-07 / 2.3e-07 ( 3.33)    2.7e-07 / 1.4e-07 ( 1.97)    8.5e-07 / 7.5e-07 ( 1.13)
                                dWdt      6.0e-07 / 1.3e-07 ( 4.62)    4.0e-07 / 1.0e-07 ( 4.05)    6.8e-07 / 8.7e-07 ( 0.78)
                                dA        9.7e-07 / 7.4e-07 ( 1.32)    4.0e-07 / 7.9e-07 ( 0.50)    1.3e-06 / 1.3e-06 ( 1.08)
                                dD        1.5e-07 / 9.2e-07 ( 0.17)    1.7e-07 / 1.0e-06 ( 0.17)    1.2e-07 / 1.2e-06 ( 0.10)
                                dbias     7.3e-07 / 2.4e-07 ( 3.06)    2.1e-07 / 1.4e-07 ( 1.50)    5.8e-07 / 6.4e-07 ( 0.90)
    msmm-1x16.16+8.8+4.4+2.2    y         1.7e-07 / 6.8e-08 ( 2.57)    1.6e-07 / 1.0e-07 ( 1.53)    7.1e-07 / 6.2e-07 ( 1.15)
                                dxc       2.0e-07 / 6.3e-08 ( 3.23)    2.1e-07 / 1.7e-07 ( 1.25)    9.5e-07 / 3.5e-07 ( 2.73)
                                dxdbl     1.0e-06 / 2.2e-07 ( 4.75)    1.7e-07 / 1.3e-07 ( 1.25)    7.1e-07 / 3.5e-07 ( 2.02)
                                dWdt      1.4e-06 / 1.2e-07 (11.70)    3.3e-07 / 1.1e-07 ( 2.96)    6.6e-07 / 4.3e-07 ( 1.53)
                                dA        7.4e-07 / 3.7e-07 ( 2.00)    1.7e-07 / 4.1e-07 ( 0.43)    1.4e-06 / 7.5e-07 ( 1.85)
                                dD        1.4e-07 / 5.7e-07 ( 0.25)    8.7e-08 / 8.6e-07 ( 0.10)    9.5e-08 / 4.5e-07 ( 0.21)
                                dbias     1.2e-06 / 2.0e-07 ( 6.08)    1.9e-07 / 1.3e-07 ( 1.50)    9.8e-07 / 4.9e-07 ( 1.98)
    sel1-1x1100x64x2x2          y         1.4e-07 / 9.8e-08 ( 1.44)    1.5e-07 / 9.5e-08 ( 1.59)    7.2e-07 / 1.7e-06 ( 0.43)
                                dtok      1.6e-07 / 9.6e-08 ( 1.65)    1.4e-07 / 6.8e-08 ( 2.03)    6.3e-07 / 1.2e-06 ( 0.52)
                                ddtr      4.2e-07 / 1.3e-07 ( 3.24)    2.0e-07 / 1.2e-07 ( 1.68)    4.4e-07 / 8.7e-07 ( 0.51)
                                dBs       9.8e-07 / 1.7e-07 ( 5.92)    1.2e-07 / 1.2e-07 ( 1.00)    6.7e-07 / 1.1e-06 ( 0.59)
                                dCs       7.7e-07 / 1.9e-07 ( 4.12)    1.5e-07 / 1.3e-07 ( 1.12)    9.2e-07 / 1.2e-06 ( 0.77)
                                dWdt      2.2e-07 / 2.2e-07 ( 1.04)    2.7e-07 / 5.7e-08 ( 4.78)    8.3e-07 / 1.3e-06 ( 0.65)
                                dA        7.3e-07 / 9.6e-07 ( 0.76)    4.4e-07 / 1.4e-06 ( 0.32)    7.4e-07 / 1.3e-06 ( 0.56)
                                dD        1.4e-07 / 1.0e-06 ( 0.14)    2.2e-07 / 1.0e-06 ( 0.22)    1.1e-07 / 4.9e-07 ( 0.21)
                                dbias     5.5e-07 / 3.6e-07 ( 1.55)    3.1e-07 / 1.6e-07 ( 2.00)    5.1e-07 / 1.5e-06 ( 0.33)
"""
import numpy as np
import pytest
import torch

from tests import _selscan_regime_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

Y_TOL = (1e-4, 1e-4)                                                     # (atol / max |ref|, rtol) of the shape tests
GRAD_TOL = {"direct": (2e-4, 1e-3), "lowrank": (3e-4, 1e-3), "msmm": (3e-4, 1e-3), "sel1": (2e-4, 1e-3)}
SWEEP_RTOL_Y, SWEEP_RTOL_GRAD, SWEEP_ATOL_SUMS = 1e-4, 1e-3, 3e-4


def _run(form, case):
    """The op of `form` on the device: (y, {operand: gradient}) as float64 CPU tensors."""
    from mlagg_unet_amd import ops
    lv = {k: case[k].to(DEV).requires_grad_(True) for k in R.LEAVES[form]}
    if form == "direct":
        y = ops.selective_scan_fn(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"], None, lv["bias"], True)
    elif form == "lowrank":
        y = ops.selective_scan_lowrank_fn(lv["u"], lv["dtr"], lv["Wdt"], lv["A"], lv["B"], lv["C"], lv["D"], lv["bias"], True)
    elif form == "msmm":
        idx = case["idx"].to(torch.int32).to(DEV).contiguous()
        y = ops.msmm_scan(lv["xc"], lv["xdbl"], idx, lv["Wdt"], lv["A"], lv["D"], lv["bias"])
    else:
        idx = case["idx"].to(torch.int32).to(DEV).contiguous()
        y = ops.selective_scan1(lv["tok"], idx, lv["dtr"], lv["Bs"], lv["Cs"], lv["Wdt"], lv["A"], lv["D"], lv["bias"])
    y.backward(case["dout"].to(DEV))
    return y.detach().cpu().double(), {k: t.grad.cpu().double() for k, t in lv.items()}


def _split_sweep(form, case, grads):
    """The gradients of a sweep case by the way they are compared: (element-wise, max-scaled sums) as {name: tensor}."""
    g = grads
    if form == "direct":
        return {k: g[k] for k in ("u", "delta", "B", "C", "D", "bias")}, {}
    if form == "lowrank":
        return (dict(u=g["u"], dtr_row0=g["dtr"][:, :, 0], B=g["B"], C=g["C"], D=g["D"], bias=g["bias"]),
                dict(dtr=g["dtr"], Wdt=g["Wdt"]))
    if form == "msmm":
        b, L = case["xc"].shape[:2]
        xd = g["xdbl"].view(b, L, R.MSMM_K, R.MSMM_XB)
        return dict(xc=g["xc"], dtr_row0=xd[..., 0], BC=xd[..., 4:], D=g["D"], bias=g["bias"]), dict(xdbl=g["xdbl"], Wdt=g["Wdt"])
    return (dict(tok=g["tok"], dtr_row0=g["dtr"][:, :, 0], Bs=g["Bs"], Cs=g["Cs"], D=g["D"], bias=g["bias"]),
            dict(dtr=g["dtr"], Wdt=g["Wdt"]))


def _worst_rel(got, ref):
    return float(((got - ref).abs() / ref.abs()).max())


SWEEP_IDS = [R.case_id(*c) for c in R.SWEEP_CASES]


def test_selscan1_sweep_cases_use_two_chunk_lengths():
    from mlagg_unet_amd import _lib
    chunks = [_lib.lib().mlagg_selscan1_chunk(s[0], s[1], s[3]) for f, s in R.SWEEP_CASES if f == "sel1"]
    print("mlagg_selscan1_chunk of the K1s sweep cases:", chunks)
    assert len(chunks) == 2 and chunks[0] != chunks[1]


@pytest.mark.parametrize("form,shape", R.SWEEP_CASES, ids=SWEEP_IDS)
def test_memoryless_sweep_matches_oracle_elementwise(form, shape):
    case, y_ref, g_ref = R.sweep_case(form, shape)
    y, g = _run(form, case)
    assert bool(torch.isfinite(y).all()) and all(bool(torch.isfinite(t).all()) for t in g.values())
    el, sums = _split_sweep(form, case, g)
    el_ref, sums_ref = _split_sweep(form, case, g_ref)
    print(f"sweep {R.case_id(form, shape)} y: worst relative error {_worst_rel(y, y_ref):.2e}")
    for k in el:
        print(f"sweep {R.case_id(form, shape)} d{k}: worst relative error {_worst_rel(el[k], el_ref[k]):.2e}")
    for k in sums:
        print(f"sweep {R.case_id(form, shape)} d{k}: max-scaled error {R.max_scaled_error(sums[k], sums_ref[k]):.2e}")
    print(f"sweep {R.case_id(form, shape)} dA: max |dA| {float(g['A'].abs().max()):.2e}")
    np.testing.assert_allclose(y.numpy(), y_ref.numpy(), rtol=SWEEP_RTOL_Y, atol=0, err_msg="y")
    for k in el:
        np.testing.assert_allclose(el[k].numpy(), el_ref[k].numpy(), rtol=SWEEP_RTOL_GRAD, atol=0, err_msg="d" + k)
    assert bool((g["A"] == 0).all()), "dA"
    for k in sums:
        s = max(float(sums_ref[k].abs().max()), 1e-6)
        np.testing.assert_allclose(sums[k].numpy(), sums_ref[k].numpy(), rtol=SWEEP_RTOL_GRAD, atol=SWEEP_ATOL_SUMS * s, err_msg="d" + k)
    if form == "msmm":
        b, L = case["xc"].shape[:2]
        assert float(g["xdbl"].view(b, L, R.MSMM_K, R.MSMM_XB)[..., 3].abs().max()) == 0.0     # pad columns: written, with zeros


REGIME_PARAMS = [(n, f, s) for f, s in R.REGIME_CASES for n in R.REGIMES]


@pytest.mark.parametrize("name,form,shape", REGIME_PARAMS, ids=[f"{n}-{R.case_id(f, s)}" for n, f, s in REGIME_PARAMS])
def test_regime_matches_oracle(name, form, shape):
    case, (y_ref, g_ref), (y32, g32) = R.regime_case(name, form, shape)
    y, g = _run(form, case)
    rows = [("y", y, y_ref, y32, Y_TOL)] + [("d" + k, g[k], g_ref[k], g32[k], GRAD_TOL[form]) for k in R.LEAVES[form]]
    for nm, got, ref, plain, _ in rows:
        ek, ep = R.max_scaled_error(got, ref), R.max_scaled_error(plain, ref)
        print(f"regime {name} {R.case_id(form, shape)} {nm}: kernel {ek:.2e} plain {ep:.2e} ratio {ek / max(ep, 1e-30):.2f}")
    for nm, got, ref, plain, (atol, rtol) in rows:
        assert bool(torch.isfinite(got).all()), nm
        s = max(float(ref.abs().max()), 1e-6)
        bound = max(atol * s, 4.0 * float((plain - ref).abs().max()))
        np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=bound, rtol=rtol, err_msg=nm)


@pytest.mark.parametrize("form,shape", [("msmm", (1, ((16, 16), (8, 8), (4, 4), (2, 2)))), ("lowrank", (1, 2, 96, 1100, 3))],
                         ids=["msmm", "lowrank-group"])
def test_two_runs_are_bit_identical(form, shape):
    case = R.regime_case("init", form, shape)[0]
    ya, ga = _run(form, case)
    yb, gb = _run(form, case)
    assert torch.equal(ya, yb)
    for k in R.LEAVES[form]:
        assert torch.equal(ga[k], gb[k]), k
