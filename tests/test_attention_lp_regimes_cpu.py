"""The oracles, yardsticks and cases of tests/_attention_lp_cases.py are what they claim to be, checked without a GPU.

Oracle: ref16 without rounding IS pooled_diff_attn_ref (bit for bit at a power-of-two scale, where scaling q commutes with the sums);
torch.autograd.gradcheck passes on it with the rounding straight-through (the offsets round16(x) - x held fixed, as the gradient
holds them).  Yardstick: emul16 without rounding reproduces ref16's output and every gradient to 1e-12 -- the hand-written backward
is the operation's -- and flash_emul without rounding the shim's oracle.  Regimes: the peak is reached after rounding and sits at
the claimed key, "flat" weights are 1 / P, "cancel" gives A == 0 with non-zero gradients; the fp16 "peaked" operands and the 16-bit
d(o) / dS operands of the fp16 loss-scale case stay below 65504 / 8.

Condition of the cases, from the two references alone: for every "init" case and tensor the documented roundings cost less than
the first term of the bound, max|emul16 - ref16| <= T max|ref16| (T = 4e-3 fp16, 3e-2 bf16; the shim: 3 output ulps + 1e-6), so T
is no slack; and for EVERY case and tensor the bound of the GPU test does not exceed 10 T max|ref16| -- a case that did would be
ill-conditioned for that tensor and would have to be redesigned, not excused.  The shim's GPU bound has no second term, so there
the yardstick has to meet the 3-ulp bound itself on every case.

One first-term check differs from T max|ref16|, and only here, as in tests/test_attention_regimes_cpu.py: d(lam) of the single-key
shape.  With one key both softmaxes are 1, o = (1 - lam) round16(v), and the RMSNorm takes the factor (1 - lam) out again:
d(lam) = -sum_c w_c d(subln_w)_c / (1 - lam) * eps / (mean(o^2) + eps), zero but for eps -- 1.5e-5 of the terms it is the sum of.
The fp32 rounding of d(o) in the workspace alone moves it by 6e-8 of those terms, 9.3e-3 of |ref16| against T = 4e-3 (fp16).  The
check measures this scalar on the scale of its terms, T sum_c |w_c d(subln_w)_c| / |1 - lam|, and asserts that it is the cancelling
zero it is said to be; the 10 T condition and the GPU bound stay as they are for it (the second term is the active one there)."""
import pytest
import torch

from tests import _attention_cases as C
from tests import _attention_lp_cases as L


def _leaves64(leaves, scale=1.0):
    return {k: t.double() * scale for k, t in leaves.items()}


@pytest.mark.parametrize("scale", [0.25, C.SCALE_B, C.SCALE_A])
def test_ref16_without_rounding_is_the_fp32_suites_reference(scale):
    lv, dout = C.pooled_case_inputs("init", 2, 5, 7, 2, scale, 0.8)
    lv = _leaves64(lv)
    with torch.no_grad():
        got, want = L.ref16(*lv.values(), 2, scale, None), C.pooled_diff_attn_ref(*lv.values(), 2, L.scale32(scale))
    if scale == 0.25:
        assert torch.equal(got, want)
    assert C.max_err(got, want) <= 1e-14 * float(want.abs().max())
    y, g = L.run_ref16(lv, dout, 2, scale, None)
    y0, g0 = C.run_reference(C.pooled_diff_attn_ref, lv, dout, torch.float64, 2, L.scale32(scale))
    assert C.max_err(y, y0) <= 1e-14 * float(y0.abs().max())
    for k in L.K4LP_LEAVES:
        assert C.max_err(g[k], g0[k]) <= 1e-13 * float(g0[k].abs().max()), k


def test_chunked_oracle_equals_the_whole_one(monkeypatch):
    lv, dout = C.pooled_case_inputs("init", 2, 5, 7, 2, C.SCALE_B, 0.8)
    y0, g0 = L.run_ref16(lv, dout, 2, C.SCALE_B, "bf16")
    monkeypatch.setattr(L, "CHUNK_ELEMS", 0)
    y, g = L.run_ref16(lv, dout, 2, C.SCALE_B, "bf16")
    assert C.max_err(y, y0) <= 1e-14 * float(y0.abs().max())
    for k in L.K4LP_LEAVES:
        assert C.max_err(g[k], g0[k]) <= 1e-13 * float(g0[k].abs().max()), k


@pytest.mark.parametrize("dt", list(L.DTYPES))
def test_gradcheck_of_ref16_with_straight_through_rounding(dt):
    for shape in ((2, 1, 1, 1, C.SCALE_B, 0.2), (1, 3, 5, 1, C.SCALE_A, 0.8)):
        B, N, P, nh, scale, lam = shape
        lv, _ = L.k4lp_case_inputs("init", B, N, P, nh, scale, lam, dt)
        leaves = [t.double().requires_grad_(True) for t in lv.values()]
        off = L.rounding_offsets(*[t.detach() for t in leaves[:3]], scale, dt)
        assert max(float(o.abs().max()) for o in off) > 0.0                     # the rounding is there
        assert torch.autograd.gradcheck(lambda *a: L.ref16(*a, nh, scale, dt, offsets=off), leaves)
        # and the straight-through gradient of ref16 itself is that of the fixed offsets
        y = L.ref16(*leaves, nh, scale, dt)
        g = torch.autograd.grad(y.sum(), leaves)
        g_off = torch.autograd.grad(L.ref16(*leaves, nh, scale, dt, offsets=off).sum(), leaves)
        assert all(torch.equal(a, b) for a, b in zip(g, g_off))


@pytest.mark.parametrize("regime,shape", [("init", L.K4LP_SHAPES[0]), ("init", L.K4LP_SHAPES[4]), ("peaked", L.K4LP_SHAPES[4]),
                                          ("cancel", L.K4LP_SHAPES[5])], ids=["1x1", "257x33", "peaked", "cancel"])
def test_emul16_without_rounding_is_ref16(regime, shape):
    B, N, P, nh, scale, lam, _ = shape
    lv, dout = L.k4lp_case_inputs(regime, B, N, P, nh, scale, lam, "bf16", "last")
    y, g = L.run_ref16(lv, dout, nh, scale, None)
    ye, ge, _ = L.emul16(lv, dout, nh, scale, None)
    assert C.max_err(ye, y) <= 1e-12 * (float(y.abs().max()) or 1.0)
    for k in L.K4LP_LEAVES:
        err, top = C.max_err(ge[k], g[k]), float(g[k].abs().max())
        print(f"{regime} d{k}: max |emul16 - ref16| {err:.2e}, max |ref16| {top:.2e}")
        # relative to max|ref16|, or to 1 where the gradient is zero (dq, dk of one key) or zero but for eps (dlam of one key)
        assert err <= 1e-12 * max(top, 1.0), k


def test_flash_emul_without_rounding_is_the_oracle():
    lv, dout = L.flash_case_inputs("init", 2, 9, 7, 2, "bf16")
    y, g = L.run_flash_ref(lv, dout, L.FLASH_SCALE)
    ye, ge = L.flash_emul(lv, dout, L.FLASH_SCALE, None)
    assert C.max_err(ye, y) <= 1e-12 * float(y.abs().max())
    for k in L.FLASH_LEAVES:
        assert C.max_err(ge[k], g[k]) <= 1e-12 * float(g[k].abs().max()), k


# ------------------------------------------------------------------------------------------------
# regimes
# ------------------------------------------------------------------------------------------------
K4LP_REGIMES = [c for c in L.K4LP_CASES if c[0] != "init"]
FLASH_REGIMES = [c for c in L.FLASH_CASES if c[0] != "init"]


def _peak_is_there(lg, P, place, dt, fp16_operands):
    """lg (B, N, P, ...) the float64 logits of the rounded operands."""
    top = float(lg.max())
    key = int(lg.amax(tuple(i for i in range(lg.dim()) if i != 2)).argmax())
    print(f"largest logit {top:.4f} at key {key} of {P}, max |logit| {float(lg.abs().max()):.3f}, share within +-80: "
          f"{float((lg.abs() <= 80).double().mean()):.4f}")
    assert abs(top - C.PEAK_LOGIT) <= 2 * L.ULP[dt] * C.PEAK_LOGIT and float(lg.abs().max()) == top
    assert top > 88.73                                                           # ln(FLT_MAX): exp overflows without the max subtraction
    assert key == (0 if place == "first" else P - 1)
    if dt == "fp16":
        assert max(float(t.abs().max()) for t in fp16_operands) < L.FP16_HEADROOM


@pytest.mark.parametrize("regime,shape,dt,place", K4LP_REGIMES, ids=[L.k4lp_id(*c) for c in K4LP_REGIMES])
def test_k4lp_regime_is_what_it_claims(regime, shape, dt, place):
    case = L.k4lp_case(regime, shape, dt, place)
    lv, P = case["leaves"], shape[2]
    (parts, v16), (y, g) = L.k4lp_parts(case), case["ref"]
    assert float(lv["lam"]) == float(torch.tensor(C.REGIME_LAM[regime]))
    if regime == "peaked":
        qs, k16, _ = L.operands16(lv["q"].double(), lv["kp"].double(), lv["vp"].double(), case["scale"], dt)
        _peak_is_there(L.pooled_logits16(lv["q"], lv["kp"], case["nh"], case["scale"], dt), P, place, dt, (qs, k16, v16))
        assert float(parts["s"].max()) > 1 - 1e-6                                # one-hot rows
    elif regime == "flat":
        assert torch.equal(parts["s"], (torch.ones((), dtype=torch.float64) / P).expand_as(parts["s"]))
        cf = L.k4lp_flat_closed_form(case)
        assert C.max_err(y, cf) <= 1e-12 * float(cf.abs().max())
    else:
        assert float(parts["o"].abs().max()) == 0.0 and float(y.abs().max()) == 0.0
        assert float(g["q"].abs().max()) > 0.0 and float(g["kp"].abs().max()) > 0.0


@pytest.mark.parametrize("regime,shape,dt,place", FLASH_REGIMES, ids=[L.flash_id(*c) for c in FLASH_REGIMES])
def test_flash_regime_is_what_it_claims(regime, shape, dt, place):
    case = L.flash_case(regime, shape, dt, place)
    lv, P = case["leaves"], shape[2]
    lg = L.flash_logits(lv["q"], lv["k"], L.FLASH_SCALE)
    if regime == "peaked":
        _peak_is_there(lg, P, place, dt, lv.values())
        assert float(lg.softmax(2).max()) > 1 - 1e-6
    else:
        assert torch.equal(lg.softmax(2), (torch.ones((), dtype=torch.float64) / P).expand_as(lg))
        # the oracle's output is the unrounded mean; the closed form rounds it to the output type
        assert C.max_err(L.round16(case["ref"][0], dt), L.flash_flat_closed_form(case)) <= L.ULP[dt] * float(case["ref"][0].abs().max())


def test_fp16_loss_scale_operands_keep_their_headroom():
    """The 16-bit d(o) and dS operands of the fp16 case under dout * 2^12 stay below 65504 / 8; without the factor they are 2^-12 of that."""
    extra = L.k4lp_loss_case("fp16")["emul"][2]
    print(f"fp16, dout * 2^12: max |d(o)| {extra['dO']:.1f}, max |dS| {extra['dS']:.1f}")
    assert 8.0 < extra["dO"] < L.FP16_HEADROOM and 8.0 < extra["dS"] < L.FP16_HEADROOM


# ------------------------------------------------------------------------------------------------
# condition
# ------------------------------------------------------------------------------------------------
def _k4lp_condition(cid, case, init):
    T = L.T_K4LP[case["dt"]]
    y, g = case["ref"]
    for name, _, ref, em in L.k4lp_rows(case, y, g):
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(em).all()), name
        top = float(ref.abs().max()) or 1.0
        err, b = C.max_err(em, ref), L.k4lp_bound(ref, em, T)
        print(f"{cid} {name}: max|emul16 - ref16| / max|ref16| {err / top:.2e} (T {T:.0e}), bound / (T max|ref16|) {b / (T * top):.2f}")
        if init and name == "lam" and case["leaves"]["kp"].shape[1] == 1:
            terms = float((case["leaves"]["subln_w"].double() * g["subln_w"]).abs().sum()) / abs(1.0 - float(case["leaves"]["lam"]))
            assert top < 1e-4 * terms and err <= T * terms, name
        elif init:
            assert err <= T * top, name
        assert b <= 10 * T * top, name


@pytest.mark.parametrize("regime,shape,dt,place", L.K4LP_CASES, ids=L.K4LP_IDS)
def test_k4lp_case_is_well_conditioned(regime, shape, dt, place):
    _k4lp_condition(L.k4lp_id(regime, shape, dt, place), L.k4lp_case(regime, shape, dt, place), regime == "init")


@pytest.mark.parametrize("dt", list(L.DTYPES))
def test_k4lp_loss_scale_case_is_well_conditioned(dt):
    case = L.k4lp_loss_case(dt)
    f, base = L.LOSS_DOUT_RMS * L.LOSS_SCALE[dt], L.k4lp_case("init", L.LOSS_SHAPE, dt)
    for k in L.K4LP_LEAVES:
        assert torch.equal(case["ref"][1][k], base["ref"][1][k] * f) and float(case["ref"][1][k].abs().max()) > 0.0
    _k4lp_condition(f"k4lp-{dt}-loss-scale", case, True)


@pytest.mark.parametrize("regime,shape,dt,place", L.FLASH_CASES, ids=L.FLASH_IDS)
def test_flash_case_is_well_conditioned(regime, shape, dt, place):
    case = L.flash_case(regime, shape, dt, place)
    y, g = case["ref"]
    for name, _, ref, em in L.flash_rows(case, y, g):
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(em).all()), name
        err, b = C.max_err(em, ref), L.flash_bound(ref, dt)
        print(f"{L.flash_id(regime, shape, dt, place)} {name}: max|emul - ref| {err:.2e}, 3 ulp bound {b:.2e}, ratio {err / b:.3f}")
        assert err <= b, name
