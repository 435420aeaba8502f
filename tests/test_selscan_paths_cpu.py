"""The cases of tests/_selscan_path_cases.py are what they claim to be, checked without a GPU.

The path predicates agree with the library's host queries (mlagg_selscan_path: the K1 launchers' own decision; the state and
workspace sizes; mlagg_msmm_scan_supported; mlagg_selscan1_chunk) over the cases and a sweep; the case list reaches every backward
form, both forward instantiations, every block count, ragged and exact last blocks -- each with a chunk carry and each at batch > 1
-- and the loop edges of the chunk prefix and the partial reduction (taking a boundary case out of the list fails here); every case
with more than one chunk has inputs a lost carry would move by a tenth of the result; and the references are sound: the plain fp32
scan agrees with the oracle as fp32 should, and the fold-back algebra matches autograd of a float64 composition."""
import os

import pytest
import torch

from tests import _selscan_path_cases as P
from tests import _selscan_regime_cases as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    from mlagg_unet_amd import _lib
    return _lib.lib()


K1 = [c for c in P.ALL_CASES if isinstance(c, P.K1Case)]
K1F = [c for c in P.ALL_CASES if isinstance(c, P.K1fCase)]
K1S = [c for c in P.ALL_CASES if isinstance(c, P.K1sCase)]


def test_no_dispatch_override_is_set():
    on = [v for v, _ in P.OVERRIDES if v in os.environ]
    assert not on, f"{on} set: tests/_selscan_path_cases.py describes the launchers' DEFAULT choices; unset to run them"


# ---------------------------------------------------------------------------------------------------------------------
# predicates against the library
# ---------------------------------------------------------------------------------------------------------------------
def test_k1_path_matches_the_launcher(lib, monkeypatch):
    for c in K1:
        if not c.blocked:
            assert lib.mlagg_selscan_path(c.G * c.Hc, c.L, c.G, c.R) == P.k1_path_code(c.Hc, c.L, c.R), c
    for Hc in range(1, 201):
        G = 1 + Hc % 3
        for L in range(1, 601):
            for Rk in range(5):
                assert lib.mlagg_selscan_path(G * Hc, L, G, Rk) == P.k1_path_code(Hc, L, Rk), (Hc, L, G, Rk)
    # what make_geom refuses, and ranks the low-rank entry points refuse
    for dim, L, G, Rk in ((10, 5, 3, 0), (32, 0, 1, 0), (0, 5, 1, 0), (32, 5, 0, 0), (32, 5, 1, 5), (32, 5, 1, -1), (65536, 4, 65536, 0)):
        assert lib.mlagg_selscan_path(dim, L, G, Rk) == P.E_UNSUPPORTED, (dim, L, G, Rk)
    monkeypatch.setenv("MLAGG_SELSCAN_BWD_BLOCKED", "1")                          # read on every call
    for c in K1:
        assert lib.mlagg_selscan_path(c.G * c.Hc, c.L, c.G, c.R) == P.k1_path_code(c.Hc, c.L, c.R, True) < 2, c


def test_k1_predicates_are_consistent():
    for Hc in range(1, 201):
        nblk, CB, last = P.k1_geom(Hc)
        assert 0 < last <= CB <= P.SCAN_CB and (nblk - 1) * CB + last == Hc
        J, tail = P.k1_slots(Hc)
        assert 0 < tail <= 16 and (J - 1) * 16 + tail == Hc
        for L in (4, 64, 130):
            assert P.k1_fast(Hc, L) == (L % 4 == 0 and Hc % 32 == 0)
            f = P.k1_bwd_form(Hc, L, 3)
            assert (f == "blocked-atomic") == (Hc > 96)
            if Hc <= 96 and (L % 4 or Hc % 16):                                  # rank 3 off the model's shapes: the run-time rank
                assert f[0] == P.RMAX and not f[3]


def test_k1_sizes_match_the_library(lib):
    shapes = [(c.b, c.G * c.Hc, c.L) for c in K1] + [(b, d, L) for b in (1, 3) for d in (1, 33, 384) for L in (1, 63, 64, 65, 5440)]
    for b, d, L in shapes:
        assert lib.mlagg_selscan_state_floats(b, d, L, P.N) == P.k1_state_floats(b, d, L), (b, d, L)
        assert lib.mlagg_selscan_bwd_workspace_floats(b, d, L, P.N) == P.k1_bwd_workspace_floats(b, d, L), (b, d, L)


def test_k1f_predicates_match_the_library(lib):
    lens = [(c.b, P.k1f_len(c.HW)) for c in K1F] + [(2, L) for L in range(1, 200)] + [(1, 21760), (1, 11184808), (1, 11184812)]
    for b, L in lens:
        assert bool(lib.mlagg_msmm_scan_supported(R.MSMM_HC, P.N, R.MSMM_R, R.MSMM_K, L)) == P.k1f_supported(L), L
        assert lib.mlagg_msmm_scan_state_floats(b, L) == P.k1f_state_floats(b, L)
        fwd, bwd = P.k1f_workspace_floats(b, L)
        assert lib.mlagg_msmm_scan_fwd_workspace_floats(b, L) == fwd and lib.mlagg_msmm_scan_bwd_workspace_floats(b, L) == bwd
    assert all(P.k1f_supported(P.k1f_len(c.HW)) for c in K1F)
    for c in K1F:                                                                 # the op's table and the oracle's orders are the same
        from mlagg_unet_amd import ops
        assert torch.equal(ops.msmm_scan_index(c.HW, "cpu").long(), R.reference_orders(c.HW)), c


def test_k1s_predicates_match_the_library(lib):
    shapes = [(c.B, c.L, c.C, c.K, c.R) for c in K1S]
    shapes += [(B, L, 64, K, 2) for B in (1, 2, 19, 86, 171, 300) for K in (1, 3, 12) for L in (1, 63, 64, 65, 300, 1100, 2048, 2049, 5000)]
    for B, L, C, K, Rk in shapes:
        ch, nchunk, nblk = P.k1s_geom(B, L, C, K)
        assert lib.mlagg_selscan1_chunk(B, L, K) == ch, (B, L, K)
        assert lib.mlagg_selscan1_state_floats(B, L, C, K) == P.k1s_state_floats(B, L, C, K)
        assert lib.mlagg_selscan1_bwd_workspace_floats(B, L, C, K, Rk) == P.k1s_bwd_workspace_floats(B, L, C, K, Rk)
    assert [P.k1s_param_pitch(r) for r in P.SEL1_RANKS] == [4, 8, 8, 8, 12, 20, 24]


# ---------------------------------------------------------------------------------------------------------------------
# the case list reaches every path
# ---------------------------------------------------------------------------------------------------------------------
def _k1_properties(c):
    nblk, CB, last = P.k1_geom(c.Hc)
    return {("form", P.k1_bwd_form(c.Hc, c.L, c.R)), ("fast", P.k1_fast(c.Hc, c.L)), ("nblk", nblk),
            ("last block", "ragged" if nblk * CB > c.Hc else "exact")}


K1_WANTED = ({("form", f) for f in ("blocked-atomic", (0, True, True, True), (0, True, True, False), (0, True, False, False),
                                    (0, False, False, False), (3, True, True, True), (3, True, True, False), (4, True, True, False),
                                    (4, True, False, False), (4, False, False, False))} |
             {("fast", v) for v in (True, False)} | {("nblk", n) for n in range(1, 6)} | {("last block", v) for v in ("ragged", "exact")})


def test_k1_cases_reach_every_path_with_a_carry_and_with_a_batch():
    default = [c for c in K1 if not c.blocked]
    seen = set().union(*(_k1_properties(c) for c in default))
    carried = set().union(*(_k1_properties(c) for c in default if P.n_chunks(c) > 1))
    batched = set().union(*(_k1_properties(c) for c in default if c.b > 1))
    assert K1_WANTED <= seen and K1_WANTED <= carried and K1_WANTED <= batched, (K1_WANTED - carried, K1_WANTED - batched)
    # a ragged last block of the blocked backward, with the fast and the checked forward in front of it
    blocked = [c for c in default if c.Hc > 96]
    assert {(P.k1_fast(c.Hc, c.L), c.R > 0) for c in blocked} == {(f, lr) for f in (True, False) for lr in (True, False)}
    assert {P.k1_geom(c.Hc)[2] < P.k1_geom(c.Hc)[1] for c in blocked} == {True, False}
    # the override: the channel-block kernel on groups that take the group form by default
    assert [P.k1_bwd_form(c.Hc, c.L, c.R, c.blocked) for c in K1 if c.blocked] == ["blocked", "blocked"]
    # slots of the group kernel: every count up to 6, full and partial last slots
    slots = {P.k1_slots(c.Hc) for c in default if c.Hc <= 96}
    assert {j for j, _ in slots} == {1, 2, 3, 4, 5, 6} and {t == 16 for _, t in slots} == {True, False}
    # ranks 1..4 at a full, a partial-slot, a scalar and a blocked shape
    for Hc, L in ((32, 132), (20, 132), (20, 130), (128, 132)):
        assert {c.R for c in default if (c.Hc, c.L) == (Hc, L)} >= {1, 2, 3, 4}


def test_k1_cases_sit_on_the_loop_edges():
    default = [c for c in K1 if not c.blocked]
    # selscan_chunk_prefix loads in groups of 8 chunks
    assert {P.n_chunks(c) for c in default} >= {1, 2, 3, 7, 8, 9, 16, 17}
    # selscan_reduce_partials: 16 row groups, two rows per trip and a tail; the last 64-column workgroup ragged or not
    red = {P.k1_reduce(c.b, c.G * c.Hc, c.L) for c in default}
    assert red >= {(rows, ragged) for rows in (16, 17, 32, 33, 48, 49) for ragged in (True, False)}
    # with and without the rank columns of a partial row (dWdt)
    assert {(P.k1_reduce(c.b, c.G * c.Hc, c.L)[0], c.R > 0) for c in default} >= {(r, lr) for r in (16, 17, 32, 33, 48, 49) for lr in (True, False)}
    # time edges of the 4-step quad, the 8-step tile, the 16-step sub-tile and the 64-step chunk, vector and scalar
    assert {c.L for c in default if c.L % 4 == 0} >= set(P.VEC_L) and {c.L for c in default if c.L % 4} >= set(P.SCALAR_L)
    # every subset of the optional operands at a fast whole shape, a blocked shape (both forms) and ranks 3 and 2
    for Hc, L, Rk in ((32, 128, 0), (128, 132, 0), (128, 132, 3), (32, 132, 3), (20, 132, 2)):
        assert {(c.D, c.bias, c.softplus) for c in default if (c.Hc, c.L, c.R) == (Hc, L, Rk)} == set(P._SUBSETS)


def test_k1f_cases_sit_on_the_loop_edges():
    lens = {P.k1f_len(c.HW) for c in K1F}
    assert lens >= {4, 8, 12, 16, 20, 60, 64, 68, 128, 132, 512, 516, 1088, 1092}
    assert {P.k1f_whole(L) for L in lens} == {True, False}
    assert 16 in {c.b * P.n_chunks(c) for c in K1F} and {c.b for c in K1F} >= {1, 2, 3}
    assert {(c.D, c.bias) for c in K1F} == {(a, b) for a in (True, False) for b in (True, False)}
    assert any(h * w % 4 for c in K1F for h, w in c.HW[:-1])                    # a scale that ends inside a quad


def test_k1s_cases_reach_every_rank_chunk_length_and_edge():
    assert {c.R for c in K1S} == set(P.SEL1_RANKS)
    geoms = {c: P.k1s_geom(c.B, c.L, c.C, c.K) for c in K1S}
    assert {g[0] for g in geoms.values()} == {64, 128, 256, 512, 1024, 2048}
    for ch in (128, 256, 512, 1024):                                             # two chunks, the second ragged
        assert any(g[0] == ch and g[1] == 2 and c.L % ch for c, g in geoms.items()), ch
    assert any(g[0] == 2048 and c.L < 2048 for c, g in geoms.items())           # a chunk longer than the sequence
    assert {g[2] for g in geoms.values()} == {1, 2, 3} and {c.K for c in K1S} >= {1, 2, 3}
    assert {c.L for c in K1S} >= set(P.SEL1_L)
    assert any(c.R == 3 and c.L > 1 for c in K1S)
    assert {c.sliced for c in K1S} == {"none", "tok", "dy"}


# ---------------------------------------------------------------------------------------------------------------------
# the inputs have memory across chunks
# ---------------------------------------------------------------------------------------------------------------------
def test_reset_scan_is_the_scan_when_it_never_resets():
    for c in (P.K1Case(2, 2, 5, 70, 0, True, True, True, False), P.K1Case(1, 1, 3, 9, 0, False, False, False, False)):
        seq = P.sequences(c)
        y, g = R.oracle_scan(*seq, softplus=c.softplus)
        y64, du64 = P.reset_scan(*seq, softplus=c.softplus, period=c.L)
        assert R.max_scaled_error(y64, y) < 2e-7 and R.max_scaled_error(du64, g[0]) < 2e-7      # the oracle rounds to float once
        y1, du1 = P.reset_scan(*seq, softplus=c.softplus, period=1)                             # no memory at all
        u, delta, A, B, C, D, bias, dout = (t.double() for t in seq)
        dl = torch.nn.functional.softplus(delta + bias[None, :, None]) if c.softplus else delta + bias[None, :, None]
        bc = (B * C).sum(2).repeat_interleave(c.Hc, dim=1)
        assert torch.allclose(y1, (dl * bc + D[None, :, None]) * u, rtol=1e-12, atol=1e-14)
        assert torch.allclose(du1, (dl * bc + D[None, :, None]) * dout, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("group", list(P.GROUPS))
def test_a_lost_chunk_carry_would_move_every_case(group):
    for c in P.GROUPS[group]:
        if P.n_chunks(c) > 1:
            sy, sdu = P.carry_sensitivity(c)
            assert sy >= 0.1 and sdu >= 0.1, (P.case_id(c), sy, sdu)


# ---------------------------------------------------------------------------------------------------------------------
# the references are sound
# ---------------------------------------------------------------------------------------------------------------------
def _cost(c):
    form = P.form_of(c)
    if form in ("direct", "lowrank"):
        return c.b * c.G * c.Hc * c.L * P.N
    return c.b * P.MSMM_DIM * P.k1f_len(c.HW) * P.N if form == "msmm" else c.B * c.K * c.C * c.L


def _soundness_cases():
    """The cheapest, a middle and the dearest case below 3e6 channel-state-steps of every group."""
    out = []
    for cases in P.GROUPS.values():
        cheap = sorted((c for c in cases if _cost(c) < 3e6), key=_cost)
        out += [cheap[0], cheap[len(cheap) // 2], cheap[-1]] if cheap else []
    return list(dict.fromkeys(out))


SOUNDNESS_CASES = _soundness_cases()


def test_plain_fp32_scan_agrees_with_the_oracle_as_fp32_should():
    """Every quantity is a sum of at most a few hundred products of order one, each rounded at 6e-8: the sequential float32 loop
    stays within 5e-6 of the oracle, max-scaled (half of the tight bound's first term)."""
    for c in SOUNDNESS_CASES:
        form, _, (y, g), (yp, gp) = P.references(c)
        assert set(g) == set(R.LEAVES[form]) - set(P.absent(c))
        for name, ref, plain in [("y", y, yp)] + [(k, g[k], gp[k]) for k in g]:
            live = float(ref.abs().max()) > 0 or (name == "A" and P.seq_len(c) == 1)             # one step: no state to decay
            assert bool(torch.isfinite(ref).all()) and live, (P.case_id(c), name)
            assert R.max_scaled_error(plain, ref) < 5e-6, (P.case_id(c), name)
            scale = max(float(ref.abs().max()), 1e-6)
            assert 0 < P.bound(c, name, ref, plain) <= (P.EXISTING_Y if name == "y" else P.EXISTING[form]) * scale


def _scan64(u, delta, A, B, C, D, bias, softplus):
    """The recurrence on (b, d, L) float64 sequences, differentiable."""
    b, d, L = u.shape
    Hc = d // B.shape[1]
    x = delta + bias[None, :, None]
    dl = torch.nn.functional.softplus(x) if softplus else x
    Bd, Cd = B.repeat_interleave(Hc, dim=1), C.repeat_interleave(Hc, dim=1)
    h, ys = torch.zeros(b, d, A.shape[1], dtype=torch.float64), []
    for dl_l, u_l, B_l, C_l in zip(dl.unbind(-1), u.unbind(-1), Bd.unbind(-1), Cd.unbind(-1)):
        h = torch.exp(dl_l[..., None] * A) * h + (dl_l * u_l)[..., None] * B_l
        ys.append((C_l * h).sum(-1) + D * u_l)
    return torch.stack(ys, -1)


def _compose64(form, lv, idx, softplus):
    """y of the form's op from float64 leaves: gather -> scan -> sum of the directions at their tokens, all by autograd-able torch."""
    if form == "direct":
        return _scan64(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"], lv["bias"], softplus)
    if form == "lowrank":
        b, d, L = lv["u"].shape
        G, Rk = lv["dtr"].shape[1:3]
        delta = (lv["dtr"][:, :, None] * lv["Wdt"].view(1, G, d // G, Rk, 1)).sum(3).reshape(b, d, L)
        return _scan64(lv["u"], delta, lv["A"], lv["B"], lv["C"], lv["D"], lv["bias"], softplus)
    K = idx.shape[0]
    inv = torch.stack([torch.argsort(idx[k]) for k in range(K)])                 # token -> scan position
    if form == "msmm":
        b, L, HC = lv["xc"].shape
        xv = lv["xdbl"].view(b, L, K, R.MSMM_XB)
        y = 0
        for k in range(K):
            xk = xv[:, idx[k], k]                                                 # (b, L, 36) in scan order
            delta = (xk[..., None, :R.MSMM_R] * lv["Wdt"].view(K, HC, R.MSMM_R)[k]).sum(-1).transpose(1, 2)
            sl = slice(k * HC, (k + 1) * HC)
            yk = _scan64(lv["xc"][:, idx[k]].transpose(1, 2), delta, lv["A"][sl], xk[..., 4:4 + P.N].transpose(1, 2)[:, None],
                         xk[..., 4 + P.N:].transpose(1, 2)[:, None], lv["D"][sl], lv["bias"][sl], True)
            y = y + yk.transpose(1, 2)[:, inv[k]]
        return y
    B, L, C = lv["tok"].shape
    Rk = lv["dtr"].shape[2]
    y = 0
    for k in range(K):
        sl = slice(k * C, (k + 1) * C)
        delta = (lv["dtr"][:, k, None] * lv["Wdt"][sl].view(1, C, Rk, 1)).sum(2)
        yk = _scan64(lv["tok"][:, idx[k]].transpose(1, 2), delta, lv["A"][sl, None], lv["Bs"][:, k, None, None], lv["Cs"][:, k, None, None],
                     lv["D"][sl], lv["bias"][sl], True)
        y = y + yk.transpose(1, 2)[:, inv[k]]
    return y


@pytest.mark.parametrize("form", ["direct", "lowrank", "msmm", "sel1"])
def test_fold_back_matches_autograd_of_a_float64_composition(form):
    """The smallest case of the form with a chunk carry (and the smallest without softplus, D and bias where the form has one):
    gather, scan and scatter written a second time as one differentiable float64 expression, its gradients by autograd."""
    mine = [c for c in P.ALL_CASES if P.form_of(c) == form and P.n_chunks(c) > 1]
    picks = [min(mine, key=_cost)]
    bare = [c for c in mine if isinstance(c, P.K1Case) and not (c.D or c.bias or c.softplus)]
    picks += [min(bare, key=_cost)] if bare else []
    for c in picks:
        _, inputs, (y, g), _ = P.references(c)
        filled = P._filled(form, inputs)
        lv = {k: filled[k].double().requires_grad_(True) for k in R.LEAVES[form]}
        y64 = _compose64(form, lv, inputs.get("idx"), P.softplus_of(c))
        y64.backward(inputs["dout"].double())
        # the oracle's one rounding to float; the forms that project delta do it in float32 before the oracle sees it
        tol = 3e-7 if form == "direct" else 2e-6
        assert R.max_scaled_error(y, y64.detach()) < tol, P.case_id(c)
        for k in g:
            assert R.max_scaled_error(g[k], lv[k].grad) < tol, (P.case_id(c), k)
