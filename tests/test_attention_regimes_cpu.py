"""The references and cases of tests/_attention_cases.py are what they claim to be, checked without a GPU.

Module agreement: the float64 references, fed the q / k / v that oracle.mlagg_oracle.AggregatedAttention forms itself, reproduce the
module's output to 1e-10 in both branches and both variants -- channel layout, window mask, logit scale, RMSNorm, gain and LePE are
pinned to the project's oracle, not to the kernels.  (The oracle's RMSNorm casts to float32 as the reference trainer does; for the
1e-10 comparison its float64 twin below stands in, and the unchanged float32 module is compared at float32 accuracy as well.)
Gradient check: torch.autograd.gradcheck of the three references.  Regime soundness: "peaked" rows are one-hot, "flat" weights are
1 / count exactly, "cancel" gives o == 0 exactly in both precisions.  Reference health: everything is finite, and the plain float32
reference alone meets the first term of every bound of the GPU test, i.e. the inputs are well conditioned and a failure on the
device means the kernel.

One bound of the health check differs from T max|ref|, and only here: d(lam) of the single-key shapes (k3-init-2x1x1x1 and
k4-init-2x1x1x1-B).  With one key both softmaxes are 1 whatever q and k are, o = (1 - lam) v, and the RMSNorm takes the factor
(1 - lam) out again, so d(lam) = -sum_c w_c d(subln_w)_c / (1 - lam) * eps / (mean(o^2) + eps): zero but for eps, a difference of
O(1) terms that comes to about 1e-6.  From the two references: the float64 value is |ref| ~ 1e-6, the plain float32 reference is
off by 0.17 (K3) and 0.10 (K4) of |ref|, i.e. by about 1e-7 -- one rounding of a single term -- where T max|ref| = 2e-10 is a
thousandth of a rounding, which no float32 evaluation can meet.  The check therefore measures this one scalar on the scale of the
terms it is the sum of, T sum_c |w_c d(subln_w)_c| / |1 - lam| (_single_key_dlam_scale), and asserts that the value is the
cancelling zero it is said to be (|ref| < 1e-4 of that scale).  tests/test_attention_regimes_gpu.py keeps the unmodified bound
max(T max|ref|, 4 max|plain - ref|) for these tensors too; there the second term, from the two references alone, is the active one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mlagg_oracle as O
from tests import _attention_cases as C


class _RMSNorm64(O.RMSNorm):
    """O.RMSNorm without the cast to float32 (T:592-613 computes the statistic in float): the same formula at the input's precision."""

    def forward(self, x):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps) * self.weight


def _module(local, dim, res, nh, sr, variant, dtype):
    torch.manual_seed(3)
    m = O.AggregatedAttention(dim, res, nh, local, sr, variant)
    O.deterministic_fill_(m.state_dict(), seed=11)
    with torch.no_grad():                                   # a gain and a lambda that are not the trivial ones
        m.subln.weight.copy_(1.0 + 0.2 * torch.randn(48, generator=torch.Generator().manual_seed(1)))
        m.lambda_q1.mul_(8.0)
    if dtype == torch.float64:
        norm = _RMSNorm64(48, eps=m.subln.eps)
        norm.weight = m.subln.weight
        m.subln = norm
    return m.to(dtype)


def _reference_in_module(m, x, H, W):
    """The module's own q / k / v through the references of tests/_attention_cases.py."""
    Bsz, N, d = x.shape
    nh = m.num_heads
    q, kv = m.q(x), m.kv(x)
    lam = m.lambda_full(q)
    if m.local:
        return C.local_diff_attn_ref(q, kv, lam, m.subln.weight, m.lepe.weight, m.lepe.bias, H, W, nh, m.scale)
    x_img = x.permute(0, 2, 1).reshape(Bsz, d, H, W)
    pooled = F.adaptive_avg_pool2d(F.gelu(m.sr(x_img)), (m.pool_H, m.pool_W))
    kvp = m.kv(m.norm(pooled.reshape(Bsz, d, -1).permute(0, 2, 1)))
    scale = m.scale if m.variant == "B" else m.scale * m.scale
    o = C.pooled_diff_attn_ref(q, kvp[..., :d], kvp[..., d:], lam, m.subln.weight, nh, scale)
    v_img = kv[..., d:].reshape(Bsz, H, W, d).permute(0, 3, 1, 2)
    return o + m.lepe(v_img).permute(0, 2, 3, 1).reshape(Bsz, N, d)


@pytest.mark.parametrize("variant", ["B", "A"])
@pytest.mark.parametrize("local", [True, False], ids=["local", "pooled"])
@pytest.mark.parametrize("dim,res,nh,sr", [(96, (9, 8), 2, 2), (48, (4, 6), 1, 1)])
def test_references_reproduce_the_oracle_module(local, dim, res, nh, sr, variant):
    x = torch.randn(2, res[0] * res[1], dim, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        m = _module(local, dim, res, nh, sr, variant, torch.float64)
        want = m(x.double(), *res)
        got = _reference_in_module(m, x.double(), *res)
        err = float((got - want).abs().max())
        print(f"float64 {'local' if local else 'pooled'} {variant} {res}: max |reference - module| {err:.2e}, max |module| "
              f"{float(want.abs().max()):.2e}")
        assert float(want.abs().max()) > 0.1
        assert err <= 1e-10
        # the unchanged module (float32 statistic in its RMSNorm) at float32
        m32 = _module(local, dim, res, nh, sr, variant, torch.float32)
        want32, got32 = m32(x, *res), _reference_in_module(m32, x, *res)
        np.testing.assert_allclose(got32.numpy(), want32.numpy(), atol=2e-5 * float(want32.abs().max()), rtol=1e-4)
        np.testing.assert_allclose(want32.double().numpy(), want.numpy(), atol=2e-5 * float(want.abs().max()), rtol=1e-4)


def test_swapped_map_halves_do_not_reproduce_the_module():
    """The agreement test tells the two maps apart: a reference call with the "+" and "-" channel halves of q and k exchanged is far
    from the module."""
    res, nh, dim = (4, 6), 1, 48
    x = torch.randn(2, res[0] * res[1], dim, generator=torch.Generator().manual_seed(5)).double()
    with torch.no_grad():
        m = _module(True, dim, res, nh, 1, "B", torch.float64)
        q, kv = m.q(x), m.kv(x)
        swap = lambda t: t.reshape(*t.shape[:-1], nh, 2, C.HD).flip(-2).reshape(t.shape)                           # noqa: E731
        kv_swapped = torch.cat([swap(kv[..., :dim]), kv[..., dim:]], -1)
        got = C.local_diff_attn_ref(swap(q), kv_swapped, m.lambda_full(q), m.subln.weight, m.lepe.weight, m.lepe.bias, *res, nh, m.scale)
        assert float((got - m(x, *res)).abs().max()) > 1e-3


def _gc_leaves(leaves, scale=1.0):
    return [t.double().mul(scale).requires_grad_(True) for t in leaves.values()]


def test_gradcheck_of_the_references():
    lv, _ = C.local_case_inputs("init", 2, 1, 1, 1, C.SCALE_B, 0.2)
    assert torch.autograd.gradcheck(lambda *a: C.local_diff_attn_ref(*a, 1, 1, 1, C.SCALE_B), _gc_leaves(lv))
    lv, _ = C.local_case_inputs("init", 1, 2, 3, 1, C.SCALE_B, 0.8)               # a window with neighbours and a border
    assert torch.autograd.gradcheck(lambda *a: C.local_diff_attn_ref(*a, 2, 3, 1, C.SCALE_B), _gc_leaves(lv))
    lv, _ = C.pooled_case_inputs("init", 2, 1, 1, 1, C.SCALE_B, 0.2)
    assert torch.autograd.gradcheck(lambda *a: C.pooled_diff_attn_ref(*a, 1, C.SCALE_B), _gc_leaves(lv))
    lv, _ = C.pooled_case_inputs("init", 1, 3, 5, 1, C.SCALE_A, 0.8)
    assert torch.autograd.gradcheck(lambda *a: C.pooled_diff_attn_ref(*a, 1, C.SCALE_A), _gc_leaves(lv))
    lv, _ = C.gate_case_inputs(1, 4)
    lv["act"] = lv["act"] / 16.0                                                  # +-5: silu' is not flat to 1e-6 there
    assert torch.autograd.gradcheck(C.gate_ref, _gc_leaves(lv))


def _parts(kind, case, dtype):
    lv = [t.to(dtype) for t in case["leaves"].values()]
    with torch.no_grad():
        return (C.local_parts if kind == "k3" else C.pooled_parts)(*lv, *case["geom"])


REGIME_PARAMS = ([("k3", r, s) for r, s in C.K3_CASES if r != "init"] + [("k4", r, s) for r, s in C.K4_CASES if r != "init"])
REGIME_IDS = [(C.k3_id if k == "k3" else C.k4_id)(r, s) for k, r, s in REGIME_PARAMS]


def _case(kind, regime, shape):
    return (C.local_case if kind == "k3" else C.pooled_case)(regime, shape)


@pytest.mark.parametrize("kind,regime,shape", REGIME_PARAMS, ids=REGIME_IDS)
def test_regime_is_what_it_claims(kind, regime, shape):
    case = _case(kind, regime, shape)
    lv = case["leaves"]
    if regime == "peaked":
        assert float(lv["lam"]) == 1.5
        for dtype in (torch.float64, torch.float32):
            s = _parts(kind, case, dtype)["s"]
            top = s.max(-1).values
            print(f"{dtype}: largest weight {float(top.max()):.9f}, rows with a weight above 1 - 1e-6: {float((top > 1 - 1e-6).double().mean()):.2f}")
            assert float(top.max()) > 1 - 1e-6
    elif regime == "flat":
        assert float(lv["lam"]) == float(np.float32(0.8))
        for dtype in (torch.float64, torch.float32):
            s = _parts(kind, case, dtype)["s"]
            if kind == "k3":
                H, W = case["geom"][:2]
                valid = C.window_valid(H, W)
                want = (valid.to(dtype) / valid.sum(1, keepdim=True).to(dtype)).view(1, H * W, 1, 1, 9).expand_as(s)
            else:
                want = (torch.ones((), dtype=dtype) / s.shape[-1]).expand_as(s)
            assert torch.equal(s, want)
        np.testing.assert_allclose(case["ref"][0].numpy(), C.flat_closed_form(kind, case).numpy(), rtol=0, atol=1e-12)
    else:
        assert float(lv["lam"]) == 1.0
        for dtype in (torch.float64, torch.float32):
            assert float(_parts(kind, case, dtype)["o"].abs().max()) == 0.0
        y = case["ref"][0]
        if kind == "k3":
            assert torch.equal(y, C.lepe_only(case))
        else:
            assert float(y.abs().max()) == 0.0 and float(case["plain"][0].abs().max()) == 0.0
        # the gradients through rstd = eps^-0.5 are finite and not trivially zero
        assert float(case["ref"][1]["q"].abs().max()) > 0.0


def test_peaked_logits_reach_the_peak():
    for kind, shapes in (("k3", C.K3_REGIME_SHAPES), ("k4", C.K4_REGIME_SHAPES)):
        for shape in shapes:
            case = _case(kind, "peaked", shape)
            lv = {k: t.double() for k, t in case["leaves"].items()}
            if kind == "k3":
                H, W, nh, scale = case["geom"]
                B, N, d = lv["q"].shape
                kw = C.windows(lv["kv"][..., :d], H, W).reshape(B, N, 9, nh, 2, C.HD)
                lg = (lv["q"].reshape(B, N, 1, nh, 2, C.HD) * kw).sum(-1) * scale
            else:
                nh, scale = case["geom"]
                B, N, d = lv["q"].shape
                P = lv["kp"].shape[1]
                lg = torch.einsum("bnhmc,bphmc->bnphm", lv["q"].reshape(B, N, nh, 2, C.HD), lv["kp"].reshape(B, P, nh, 2, C.HD)) * scale
            top, q80 = float(lg.max()), float((lg.abs() <= 80).double().mean())
            print(f"{kind} {shape[:4]}: largest logit {top:.3f}, max |logit| {float(lg.abs().max()):.3f}, share within +-80: {q80:.4f}")
            # float32 exp overflows on the largest (POSITIVE) logit unless the maximum is subtracted first
            assert abs(top - C.PEAK_LOGIT) < 1e-3 and float(lg.abs().max()) <= top + 1e-3 and q80 > 0.95
            assert top > float(np.log(np.finfo(np.float32).max))


ALL_PARAMS = [("k3", r, s) for r, s in C.K3_CASES] + [("k4", r, s) for r, s in C.K4_CASES]
ALL_IDS = C.K3_IDS + C.K4_IDS


def _single_key(kind, case):
    return (case["geom"][:2] == (1, 1)) if kind == "k3" else case["leaves"]["kp"].shape[1] == 1


def _single_key_dlam_scale(case):
    """With ONE key both softmaxes are 1 whatever q and k are, o = (1 - lam) v, and the RMSNorm takes the factor (1 - lam) out again:
    d(lam) = -sum_c w_c d(subln_w)_c / (1 - lam) * eps / (mean(o^2) + eps), zero but for eps (1e-6 here) and a difference of O(1)
    terms.  T max|ref| of that one number is 2e-10, less than one rounding of its terms, which no fp32 evaluation meets; the health
    check therefore measures this scalar, and only it, on the scale of the terms it is the sum of."""
    w, dw = case["leaves"]["subln_w"].double(), case["ref"][1]["subln_w"]
    return float((w * dw).abs().sum()) / abs(1.0 - float(case["leaves"]["lam"]))


@pytest.mark.parametrize("kind,regime,shape", ALL_PARAMS, ids=ALL_IDS)
def test_plain_fp32_reference_meets_the_first_term_of_the_bound(kind, regime, shape):
    case = _case(kind, regime, shape)
    (y, grads), (y32, grads32) = case["ref"], case["plain"]
    for name, ref, plain in [("y", y, y32)] + [(k, grads[k], grads32[k]) for k in C.LEAVES[kind]]:
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(plain).all()), name
        T, rtol = C.tol_of(name)
        err = C.max_err(plain, ref)
        print(f"{(C.k3_id if kind == 'k3' else C.k4_id)(regime, shape)} {name}: plain fp32 max-scaled error {C.scaled(err, ref):.2e}")
        atol = C.bound(ref, plain, T, margin=0)
        if name == "lam" and _single_key(kind, case):
            atol = T * _single_key_dlam_scale(case)
            assert float(ref.abs()) < 1e-4 * _single_key_dlam_scale(case)         # the cancelling zero it is said to be
        np.testing.assert_allclose(plain.numpy(), ref.numpy(), atol=atol, rtol=rtol, err_msg=name)


@pytest.mark.parametrize("shape", C.K7_SHAPES, ids=C.K7_IDS)
def test_gate_sweep_is_sound(shape):
    case = C.gate_case(shape)
    act = case["leaves"]["act"]
    (y, grads), (y32, grads32) = case["ref"], case["plain"]
    assert float(act.abs().max()) <= C.ACT_LIMIT
    for t in (case["leaves"]["a0"], case["leaves"]["a1"], case["dout"]):
        assert 0.5 <= float(t.min()) and float(t.max()) <= 2.0
    if act.numel() >= 1000:
        for v in C.sweep_points().tolist():
            assert bool((act == v).any()), f"sweep point {v} is missing"
        assert float(act.min()) == -C.ACT_LIMIT and float(act.max()) == C.ACT_LIMIT
    nz = act != 0
    assert float(y[nz].abs().min()) > 1e-36
    da = torch.cat([grads["a0"], grads["a1"]], -1)
    assert float(da[nz].abs().min()) > 1e-36
    tol = C.gate_tolerances(case)
    da32 = torch.cat([grads32["a0"], grads32["a1"]], -1)
    for name, got, ref in (("y", y32, y), ("da", da32, da), ("dact", grads32["act"], grads["act"])):
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(got).all()), name
        ratio = float(((got - ref).abs() / tol[name]).max())
        print(f"k7 {shape[:2]} {name}: plain fp32 worst error / tolerance {ratio:.3f}")
        assert ratio <= 1.0, name


def test_root_of_the_silu_derivative():
    x = torch.tensor(-C.SILU_GRAD_ROOT, dtype=torch.float64)
    s = torch.sigmoid(x)
    assert abs(float(s * (1 + x * (1 - s)))) < 1e-15
