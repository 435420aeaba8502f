"""The cases of tests/_selscan_regime_cases.py are what they claim to be, checked without a GPU.

Memoryless sweep: the oracle (oracle/selscan_ref.c, fed through the same gather / fold-back algebra as on the device) agrees with
an independent float64 closed form, every value the device test compares element-wise is finite and far from the denormal range,
and dA is exactly 0.  Regimes: a plain step-by-step float32 scan meets the parity tests' tolerances against the oracle, i.e. the
inputs are well conditioned and a failure on the device means the kernel."""
import numpy as np
import pytest
import torch

from tests import _selscan_regime_cases as R

# the tolerances of tests/test_selscan_gpu.py, test_msmm_scan_gpu.py and test_selscan1_gpu.py: (atol / max |ref|, rtol)
Y_TOL = (1e-4, 1e-4)
GRAD_TOL = {"direct": (2e-4, 1e-3), "lowrank": (3e-4, 1e-3), "msmm": (3e-4, 1e-3), "sel1": (2e-4, 1e-3)}

SWEEP_IDS = [R.case_id(*c) for c in R.SWEEP_CASES]


def _elementwise(form, case, grads):
    """The oracle outputs of a sweep case that the device test compares element by element: name -> tensor."""
    g = grads
    if form == "direct":
        return {k: g[k] for k in ("u", "delta", "B", "C", "D", "bias")}
    if form == "lowrank":
        return dict(u=g["u"], dtr0=g["dtr"][:, :, 0], B=g["B"], C=g["C"], D=g["D"], bias=g["bias"])
    if form == "msmm":
        b, L = case["xc"].shape[:2]
        xd = g["xdbl"].view(b, L, R.MSMM_K, R.MSMM_XB)
        return dict(xc=g["xc"], dtr0=xd[..., 0], BC=xd[..., 4:], D=g["D"], bias=g["bias"])
    return dict(tok=g["tok"], dtr0=g["dtr"][:, :, 0], Bs=g["Bs"], Cs=g["Cs"], D=g["D"], bias=g["bias"])


@pytest.mark.parametrize("form,shape", R.SWEEP_CASES, ids=SWEEP_IDS)
def test_sweep_oracle_matches_closed_form(form, shape):
    case, _, _ = R.sweep_case(form, shape)
    seq = R.to_sequences(form, case)
    y_seq, grads_seq = R.oracle_scan(*seq)
    y_cf, dd_cf = R.sweep_closed_form(*seq)
    np.testing.assert_allclose(y_seq.numpy(), y_cf.numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(grads_seq[1].numpy(), dd_cf.numpy(), rtol=1e-6, atol=0)


@pytest.mark.parametrize("form,shape", R.SWEEP_CASES, ids=SWEEP_IDS)
def test_sweep_outputs_are_normal_numbers(form, shape):
    case, y, grads = R.sweep_case(form, shape)
    for name, t in dict(y=y, **_elementwise(form, case, grads)).items():
        assert bool(torch.isfinite(t).all()), name
        assert float(t.abs().min()) > 1e-20, name
    assert bool((grads["A"] == 0).all())
    # the rank rows and projection columns that carry no sweep: nothing flows into them
    if form != "direct":
        assert float(grads["Wdt"][:, 1:].abs().max()) == 0.0
    if form in ("lowrank", "sel1"):
        assert float(grads["dtr"][:, :, 1:].abs().max()) == 0.0
    if form == "msmm":
        b, L = case["xc"].shape[:2]
        assert float(grads["xdbl"].view(b, L, R.MSMM_K, R.MSMM_XB)[..., 1:4].abs().max()) == 0.0


REGIME_PARAMS = [(n, f, s) for f, s in R.REGIME_CASES for n in R.REGIMES]


@pytest.mark.parametrize("name,form,shape", REGIME_PARAMS, ids=[f"{n}-{R.case_id(f, s)}" for n, f, s in REGIME_PARAMS])
def test_regime_is_well_conditioned_in_plain_fp32(name, form, shape):
    _, (y, grads), (y32, grads32) = R.regime_case(name, form, shape)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(y32).all())
    print(f"{name} {R.case_id(form, shape)} y: plain fp32 max-scaled error {R.max_scaled_error(y32, y):.2e}")
    np.testing.assert_allclose(y32.numpy(), y.numpy(), atol=Y_TOL[0] * float(y.abs().max()), rtol=Y_TOL[1])
    atol, rtol = GRAD_TOL[form]
    for k in R.LEAVES[form]:
        r = grads[k]
        assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(grads32[k]).all()), k
        print(f"{name} {R.case_id(form, shape)} d{k}: plain fp32 max-scaled error {R.max_scaled_error(grads32[k], r):.2e}")
        s = max(float(r.abs().max()), 1e-6)
        np.testing.assert_allclose(grads32[k].numpy(), r.numpy(), atol=atol * s, rtol=rtol, err_msg=k)
