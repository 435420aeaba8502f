"""GPU parity of the selective-scan kernels (K1 csrc/selscan.hip, K1f csrc/selscan_tok.hip, K1s csrc/selscan1.hip) against the
double-precision oracle at the sizes where their launchers and loops change path, on inputs whose state crosses every chunk edge:
the cases of tests/_selscan_path_cases.py (whose claims tests/test_selscan_paths_cpu.py checks without a GPU).

Per case: y and every gradient, max-scaled, within min(existing, max(1e-5 max |ref|, 16 x the plain fp32 scan's error)) with no
rtol term (see the cases file); gradients of absent operands are None; K1f's pad columns get exactly 0; the group form of K1 and all
of K1f give the same bits on a second run.  One test per case group; each prints, per case,
    quantity kernel error / plain fp32 error (ratio)
and profiles/selscan_kernel_paths_mi355x.log keeps those lines of a run on an MI355X."""
import pytest
import torch

from tests import _selscan_path_cases as P
from tests import _selscan_regime_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OVERRIDE = "MLAGG_SELSCAN_BWD_BLOCKED"
# where D and bias sit in what the op's backward returns
OPTIONAL_AT = {"direct": (5, 6), "lowrank": (6, 7), "msmm": (5, 6)}


def _wide(t):
    """t (B, L, C) as the channel block [8, 8 + C) of a tensor 16 channels wider (other channels: junk)."""
    w = torch.full((t.shape[0], t.shape[1], t.shape[2] + P.SLICE_EXTRA), 7.0, device=t.device)
    w[..., P.SLICE_AT:P.SLICE_AT + t.shape[2]] = t
    return w[..., P.SLICE_AT:P.SLICE_AT + t.shape[2]]


def _run(case, inputs, monkeypatch):
    """The case's op on the device: (y, {operand: gradient}, what backward returned, row strides _rows handed to the kernels)."""
    from mlagg_unet_amd import ops
    form = P.form_of(case)
    lv = {k: inputs[k].to(DEV).requires_grad_(True) for k in R.LEAVES[form] if inputs[k] is not None}
    opt = lambda k: lv.get(k)                                                                     # noqa: E731
    seen = {"rows": {}}
    fn = {"direct": ops.SelectiveScanFn, "lowrank": ops.SelectiveScanLowRankFn, "msmm": ops.MsmmScanFn, "sel1": ops.SelectiveScan1Fn}[form]
    backward, rows = fn.backward, ops._rows

    def spy_backward(ctx, *grads):
        seen["returned"] = backward(ctx, *grads)
        return seen["returned"]

    def spy_rows(t, name):
        out = rows(t, name)
        seen["rows"][name] = out[1]
        return out

    with monkeypatch.context() as m:
        m.setattr(fn, "backward", staticmethod(spy_backward))
        m.setattr(ops, "_rows", spy_rows)
        if getattr(case, "blocked", False):
            m.setenv(OVERRIDE, "1")
        else:
            m.delenv(OVERRIDE, raising=False)
        dout = inputs["dout"].to(DEV)
        if form == "direct":
            y = ops.selective_scan_fn(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], opt("D"), None, opt("bias"), case.softplus)
        elif form == "lowrank":
            y = ops.selective_scan_lowrank_fn(lv["u"], lv["dtr"], lv["Wdt"], lv["A"], lv["B"], lv["C"], opt("D"), opt("bias"), case.softplus)
        elif form == "msmm":
            idx = ops.msmm_scan_index(case.HW, DEV)
            assert torch.equal(idx.cpu().long(), inputs["idx"])
            y = ops.msmm_scan(lv["xc"], lv["xdbl"], idx, lv["Wdt"], lv["A"], **{k: lv[n] for k, n in (("D", "D"), ("delta_bias", "bias")) if n in lv})
        else:
            idx = inputs["idx"].to(torch.int32).to(DEV).contiguous()
            tok = lv["tok"]
            if case.sliced == "tok":
                tok = _wide(lv["tok"])                                                            # differentiable: d(tok) flows back to the leaf
            if case.sliced == "dy":
                dout = _wide(dout)
            y = ops.selective_scan1(tok, idx, lv["dtr"], lv["Bs"], lv["Cs"], lv["Wdt"], lv["A"], lv["D"], lv["bias"])
        torch.autograd.backward(y, dout)
        torch.cuda.synchronize()
    return y.detach().cpu().double(), {k: t.grad.cpu().double() for k, t in lv.items()}, seen["returned"], seen["rows"]


def _check_case(case, monkeypatch):
    """Runs one case; returns (log line, list of failures)."""
    form, inputs, (y_ref, g_ref), (y32, g32) = P.references(case)
    cid = P.case_id(case)
    y, g, returned, rows = _run(case, inputs, monkeypatch)
    fails, cells = [], []
    assert set(g) == set(g_ref), cid
    for name, got, ref, plain in [("y", y, y_ref, y32)] + [(k, g[k], g_ref[k], g32[k]) for k in g_ref]:
        s = max(float(ref.abs().max()), 1e-6)
        err, perr, lim = float((got - ref).abs().max()), float((plain - ref).abs().max()), P.bound(case, name, ref, plain)
        cells.append(f"{name if name == 'y' else 'd' + name} {err / s:.1e}/{perr / s:.1e}({err / max(perr, 1e-30):5.2f})")
        if not bool(torch.isfinite(got).all()):
            fails.append(f"{cid} {name}: not finite")
        elif not err <= lim:
            fails.append(f"{cid} {name}: max-scaled error {err / s:.2e} above the bound {lim / s:.2e} (plain fp32 {perr / s:.2e})")
    # gradients of absent operands
    for k, at in zip(("D", "bias"), OPTIONAL_AT.get(form, ())):
        if (returned[at] is None) != (k in P.absent(case)):
            fails.append(f"{cid}: backward returned {'a tensor' if returned[at] is not None else 'None'} for d{k}")
    if form == "msmm":
        b, L = inputs["xc"].shape[:2]
        if float(g["xdbl"].view(b, L, R.MSMM_K, R.MSMM_XB)[..., 3].abs().max()) != 0.0:
            fails.append(f"{cid}: pad column gradient is not exactly 0")
    if form == "sel1":
        want = {"tok": case.C + (P.SLICE_EXTRA if case.sliced == "tok" else 0), "dy": case.C + (P.SLICE_EXTRA if case.sliced == "dy" else 0)}
        if rows != want:
            fails.append(f"{cid}: row strides {rows} reached the kernels, the case is about {want}")
    # a second run gives the same bits where nothing is summed by atomics
    if form == "msmm" or (form in ("direct", "lowrank") and not isinstance(P.k1_bwd_form(case.Hc, case.L, case.R, case.blocked), str)):
        y2, g2, _, _ = _run(case, inputs, monkeypatch)
        fails += [f"{cid} {k}: a second run differs" for k, a, b in [("y", y, y2)] + [(k, g[k], g2[k]) for k in g] if not torch.equal(a, b)]
    return f"paths {cid}: " + "  ".join(cells), fails


@pytest.mark.parametrize("group", list(P.GROUPS))
def test_every_case_of_the_group_matches_the_oracle(group, monkeypatch):
    failures = []
    for case in P.GROUPS[group]:
        line, fails = _check_case(case, monkeypatch)
        print(line)
        failures += fails
    assert not failures, "\n".join(failures)
