"""Inputs and references for the selective-scan kernels outside the one numerical regime of their parity tests (decay per step
0.85 .. 0.95): shared by tests/test_selscan_regimes_cpu.py and tests/test_selscan_regimes_gpu.py, and home of the gather / fold-back
algebra that tests/test_msmm_scan_gpu.py and tests/test_selscan1_gpu.py feed the oracle with.

Four operand FORMS of the same recurrence (delta_l = softplus(x_l), h_l = exp(delta_l A) h_{l-1} + delta_l B_l u_l,
y_l = C_l . h_l + D u_l):
    "direct"   K1   ops.selective_scan_fn           shape (b, G, Hc, L)      x = delta + bias
    "lowrank"  K1   ops.selective_scan_lowrank_fn   shape (b, G, Hc, L, R)   x = Wdt[d] . dtr[:, l] + bias
    "msmm"     K1f  ops.msmm_scan                   shape (b, maps)          token-major, four directions through an index table
    "sel1"     K1s  ops.selective_scan1             shape (B, L, C, K, R)    one state, K directions through an index table
A case is a dict of float32 CPU tensors named like the op's parameters, plus "dout" and the int64 table "idx" where the form
has one.  `to_sequences` turns any of them into the (b, d, L) operands of the plain scan, `fold_back` turns the plain scan's
gradients into the gradients of the form's operands (float64 host algebra), and `reference` chains the two around a scan:
`oracle_scan` (oracle/selscan_ref.c, double arithmetic: the truth) or `plain_fp32_scan` (a step-by-step float32 torch loop: what
ordinary fp32 gives on the same inputs, the yardstick for how well conditioned a case is).

`memoryless_sweep` makes every step an independent probe of softplus and its derivative; `regime` makes inputs with memory."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import c_oracle as CO

N = 16                                   # d_state of K1 / K1f
MSMM_K, MSMM_HC, MSMM_R, MSMM_XB = 4, 96, 3, 36
LOG2E = 1.4426950408889634

# operands that receive a gradient, in the order the op takes them
LEAVES = {
    "direct": ("u", "delta", "A", "B", "C", "D", "bias"),
    "lowrank": ("u", "dtr", "Wdt", "A", "B", "C", "D", "bias"),
    "msmm": ("xc", "xdbl", "Wdt", "A", "D", "bias"),
    "sel1": ("tok", "dtr", "Bs", "Cs", "Wdt", "A", "D", "bias"),
}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ------------------------------------------------------------------------------------------------
# scan orders
# ------------------------------------------------------------------------------------------------
def reference_orders(HW):
    """The four scan orders as the reference builds them (M:414-422): per scale x (C, H, W) -> stack([x.flatten(), x.transpose(H, W)
    .flatten()]) and their flips, scales concatenated per direction.  Returned as token indices (4, L)."""
    rows, off = [[], [], [], []], 0
    for H, W in HW:
        tok = torch.arange(H * W).view(H, W)
        hw, wh = tok.flatten(), tok.t().contiguous().flatten()
        for k, t in enumerate((hw, wh, hw.flip(0), wh.flip(0))):
            rows[k].append(t + off)
        off += H * W
    return torch.stack([torch.cat(r) for r in rows])


def sel1_orders(L, K, g):
    """K random permutations of L tokens, the second half the reversals of the first (like directions 6..11 of SS3D)."""
    half = (K + 1) // 2
    perms = [torch.randperm(L, generator=g) for _ in range(half)]
    return torch.stack((perms + [p.flip(0) for p in perms])[:K])


# ------------------------------------------------------------------------------------------------
# the two scans on (b, d, L) sequences
# ------------------------------------------------------------------------------------------------
def oracle_scan(u, delta, A, B, C, D, bias, dout, softplus=True):
    """oracle/selscan_ref.c: y and (du, ddelta, dA, dB, dC, dD, dbias), computed in double and rounded to float once."""
    n = lambda t: None if t is None else t.contiguous().numpy()                                  # noqa: E731
    y = CO.selscan_fwd(n(u), n(delta), n(A), n(B), n(C), n(D), n(bias), softplus)
    grads = CO.selscan_bwd(n(u), n(delta), n(A), n(B), n(C), n(D), n(bias), n(dout), softplus)
    return torch.from_numpy(y), tuple(torch.from_numpy(v) for v in grads)


def plain_fp32_scan(u, delta, A, B, C, D, bias, dout, softplus=True):
    """The same recurrence one step after the other in float32 on the host, gradients by autograd.  Not the truth: the error
    ordinary fp32 arithmetic makes on these inputs."""
    leaves = [t.detach().clone().float().requires_grad_(True) for t in (u, delta, A, B, C, D, bias)]
    u_, x_, A_, B_, C_, D_, b_ = leaves
    b, d, L = u_.shape
    Hc = d // B_.shape[1]
    dl = x_ + b_[None, :, None]
    if softplus:
        dl = F.softplus(dl)                                                                      # threshold 20, as the oracle
    Bd, Cd = B_.repeat_interleave(Hc, dim=1), C_.repeat_interleave(Hc, dim=1)                    # (b, d, n, L)
    h = torch.zeros(b, d, A_.shape[1])
    ys = []
    # one unbind per operand: a select per step would hand autograd a full-size zero tensor per step and operand
    for dl_l, u_l, B_l, C_l in zip(dl.unbind(-1), u_.unbind(-1), Bd.unbind(-1), Cd.unbind(-1)):
        h = torch.exp(dl_l[:, :, None] * A_) * h + (dl_l * u_l)[:, :, None] * B_l
        ys.append((C_l * h).sum(-1) + D_ * u_l)
    y = torch.stack(ys, -1)
    y.backward(dout.float())
    return y.detach(), tuple(t.grad for t in leaves)


# ------------------------------------------------------------------------------------------------
# form -> sequences -> form
# ------------------------------------------------------------------------------------------------
def to_sequences(form, case):
    """(u, delta, A, B, C, D, bias, dout) of the plain scan, float32, as the parity test of the form's kernel feeds the oracle."""
    c = case
    if form == "direct":
        return c["u"], c["delta"], c["A"], c["B"], c["C"], c["D"], c["bias"], c["dout"]
    if form == "lowrank":
        b, d, L = c["u"].shape
        G, R = c["dtr"].shape[1], c["dtr"].shape[2]
        delta = torch.einsum("bgrl,gdr->bgdl", c["dtr"], c["Wdt"].view(G, d // G, R)).reshape(b, d, L).contiguous()
        return c["u"], delta, c["A"], c["B"], c["C"], c["D"], c["bias"], c["dout"]
    if form == "msmm":
        K, HC, R, XB = MSMM_K, MSMM_HC, MSMM_R, MSMM_XB
        xc, idx = c["xc"], c["idx"]
        b, L = xc.shape[:2]
        xv = c["xdbl"].view(b, L, K, XB)
        # scan sequences gathered the way forward_corev0 lays them out
        xs = torch.stack([xc[:, idx[k]] for k in range(K)], 1).permute(0, 1, 3, 2).reshape(b, K * HC, L).contiguous()
        dtr = torch.stack([xv[:, idx[k], k, :R] for k in range(K)], 1).permute(0, 1, 3, 2).contiguous()            # (b, K, R, L)
        Bs = torch.stack([xv[:, idx[k], k, 4:4 + N] for k in range(K)], 1).permute(0, 1, 3, 2).contiguous()        # (b, K, N, L)
        Cs = torch.stack([xv[:, idx[k], k, 4 + N:] for k in range(K)], 1).permute(0, 1, 3, 2).contiguous()
        delta = torch.einsum("bkrl,kdr->bkdl", dtr, c["Wdt"].view(K, HC, R)).reshape(b, K * HC, L).contiguous()
        dout = torch.stack([c["dout"][:, idx[k]] for k in range(K)], 1).permute(0, 1, 3, 2).reshape(b, K * HC, L).contiguous()
        return xs, delta, c["A"], Bs, Cs, c["D"], c["bias"], dout
    if form == "sel1":
        tok, ix, dtr = c["tok"], c["idx"], c["dtr"]
        B, L, C = tok.shape
        K, R = ix.shape[0], dtr.shape[2]
        xs = torch.stack([tok[:, ix[k], :].transpose(1, 2) for k in range(K)], 1).reshape(B, K * C, L)             # (B, K*C, L)
        delta = torch.einsum("bkrl,kcr->bkcl", dtr.double(), c["Wdt"].view(K, C, R).double()).reshape(B, K * C, L).float()
        douts = torch.stack([c["dout"][:, ix[k], :].transpose(1, 2) for k in range(K)], 1).reshape(B, K * C, L)
        return xs, delta, c["A"].view(-1, 1), c["Bs"].view(B, K, 1, L), c["Cs"].view(B, K, 1, L), c["D"], c["bias"], douts
    raise ValueError(form)


def fold_back(form, case, y_seq, grads_seq):
    """y and the gradients of the form's operands (dict by operand name) from the plain scan's; every sum and product that the
    fold adds is formed in float64 (the large sequences are widened piece by piece)."""
    c = case
    du, ddelta, dA, dB, dC, dD, dbias = grads_seq
    if form == "direct":
        return y_seq, dict(u=du, delta=ddelta, A=dA, B=dB, C=dC, D=dD, bias=dbias)
    if form == "lowrank":
        b, d, L = c["u"].shape
        G, R = c["dtr"].shape[1], c["dtr"].shape[2]
        dd = ddelta.double().reshape(b, G, d // G, L)
        ddtr = torch.einsum("bgdl,gdr->bgrl", dd, c["Wdt"].double().view(G, d // G, R))
        dW = torch.einsum("bgdl,bgrl->gdr", dd, c["dtr"].double()).reshape(d, R)
        return y_seq, dict(u=du, dtr=ddtr, Wdt=dW, A=dA, B=dB, C=dC, D=dD, bias=dbias)
    if form == "msmm":
        K, HC, R, XB = MSMM_K, MSMM_HC, MSMM_R, MSMM_XB
        idx = c["idx"]
        b, L = c["xc"].shape[:2]
        xv = c["xdbl"].view(b, L, K, XB)
        dtr = torch.stack([xv[:, idx[k], k, :R] for k in range(K)], 1).permute(0, 1, 3, 2)
        dd = ddelta.double().reshape(b, K, HC, L)
        ddtr = torch.einsum("bkdl,kdr->bkrl", dd, c["Wdt"].double().view(K, HC, R))
        dW = torch.einsum("bkdl,bkrl->kdr", dd, dtr.double()).reshape(K * HC, R)
        y = torch.zeros(b, L, HC, dtype=torch.float64)
        dxc = torch.zeros(b, L, HC, dtype=torch.float64)
        dxd = torch.zeros(b, L, K, XB, dtype=torch.float64)
        y4, du4 = y_seq.reshape(b, K, HC, L), du.reshape(b, K, HC, L)
        for k in range(K):
            ik = idx[k]
            y[:, ik] += y4[:, k].transpose(1, 2).double()
            dxc[:, ik] += du4[:, k].transpose(1, 2).double()
            dxd[:, ik, k, :R] = ddtr[:, k].transpose(1, 2)
            dxd[:, ik, k, 4:4 + N] = dB[:, k].transpose(1, 2).double()
            dxd[:, ik, k, 4 + N:] = dC[:, k].transpose(1, 2).double()
        return y, dict(xc=dxc, xdbl=dxd.reshape(b, L, K * XB), Wdt=dW, A=dA, D=dD, bias=dbias)
    if form == "sel1":
        ix, dtr = c["idx"], c["dtr"]
        B, L, C = c["tok"].shape
        K, R = ix.shape[0], dtr.shape[2]
        out = y_seq.view(B, K, C, L)
        y = torch.zeros(B, L, C, dtype=torch.float64)
        dtok = torch.zeros(B, L, C, dtype=torch.float64)
        du = du.view(B, K, C, L)
        for k in range(K):
            y[:, ix[k], :] += out[:, k].transpose(1, 2).double()
            dtok[:, ix[k], :] += du[:, k].transpose(1, 2).double()
        dd = ddelta.view(B, K, C, L).double()
        ddtr = torch.einsum("bkcl,kcr->bkrl", dd, c["Wdt"].view(K, C, R).double())
        dW = torch.einsum("bkcl,bkrl->kcr", dd, dtr.double()).reshape(K * C, R)
        return y, dict(tok=dtok, dtr=ddtr, Bs=dB.view(B, K, L), Cs=dC.view(B, K, L), Wdt=dW, A=dA.view(-1), D=dD, bias=dbias)
    raise ValueError(form)


def reference(form, case, scan=oracle_scan):
    """(y, {operand: gradient}) of `case` through `scan`, float64."""
    y_seq, grads_seq = scan(*to_sequences(form, case))
    y, grads = fold_back(form, case, y_seq, grads_seq)
    return y.double(), {k: v.double() for k, v in grads.items()}


def msmm_oracle(xc, xdbl, Wdt, A, D, bias, dy, idx):
    """What tests/test_msmm_scan_gpu.py compares K1f with: (y, gradients of xc, xdbl, Wdt, A, D, bias) as float64 arrays."""
    y, g = reference("msmm", dict(xc=xc, xdbl=xdbl, Wdt=Wdt, A=A, D=D, bias=bias, dout=dy, idx=idx))
    return y.numpy(), tuple(g[k].numpy() for k in LEAVES["msmm"])


def selscan1_oracle(tok, idx, dtr, Bs, Cs, Wdt, A, D, bias, dout):
    """What tests/test_selscan1_gpu.py compares K1s with: explicit scan-order tensors -> C oracle -> gradients folded back to the
    kernel's operands (float64 host algebra)."""
    return reference("sel1", dict(tok=tok, idx=idx.long(), dtr=dtr, Bs=Bs, Cs=Cs, Wdt=Wdt, A=A, D=D, bias=bias, dout=dout))


# ------------------------------------------------------------------------------------------------
# memoryless sweep
# ------------------------------------------------------------------------------------------------
SWEEP_A = -1e30                          # exp(delta A) == 0 for every delta of the sweep: no step sees the one before it
SWEEP_LO, SWEEP_HI = -16.0, 24.0         # softplus(-16) = 1.1e-7: every checked value stays a normal float32
BRANCH = 4.60517                         # softplus1 switches between series and logarithm at exp(-|x|) = 0.01


def _with_neighbours(v, k):
    v = np.float32(v)
    out, up, dn = [v], v, v
    for _ in range(k):
        up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
        out += [up, dn]
    return out


def sweep_points(n):
    """n float32 softplus arguments in ascending order: an even grid over [-16, 24] plus the points where an implementation
    changes branch -- 0 and the smallest normal numbers either side, +-4.60517 with three float32 neighbours either side (the
    kernels switch on exp(-|x|) < 0.01, i.e. within rounding of that point), 20 (torch's and the oracle's identity threshold) and
    the float32 after it."""
    tiny = np.finfo(np.float32).tiny
    special = ([np.float32(0.0), tiny, -tiny] + _with_neighbours(BRANCH, 3) + _with_neighbours(-BRANCH, 3) +
               [np.float32(20.0), np.nextafter(np.float32(20.0), np.float32(np.inf))])
    assert n >= len(special) + 8, "sequence too short for the sweep"
    grid = np.linspace(SWEEP_LO, SWEEP_HI, n - len(special), dtype=np.float32)
    return torch.from_numpy(np.sort(np.concatenate([np.asarray(special, np.float32), grid])))


def _sweep_rows(rows, L):
    """(rows, L): the sweep along the sequence, started at a different point in every row."""
    p = sweep_points(L)
    return torch.stack([torch.roll(p, 5 * i) for i in range(rows)])


def _check_sweep(x):
    """The generator's own conditions on the softplus arguments x (any shape, sequence last)."""
    xs = x.double()
    assert float(xs.min()) == SWEEP_LO and float(xs.max()) == SWEEP_HI
    for v in sweep_points(x.shape[-1]).tolist():
        assert bool((xs == v).any()), f"sweep point {v} is missing"
    dl = F.softplus(xs)
    dmin = float(dl.min())
    assert np.exp(np.float32(dmin) * np.float32(SWEEP_A)) == 0.0 and np.exp(dmin * SWEEP_A) == 0.0
    # a chunk's sum of delta is at most the sequence's: the chunk prefix forms exp2(A log2(e) sum) from a finite argument
    assert np.isfinite(np.float32(SWEEP_A) * np.float32(LOG2E) * np.float32(dl.sum(-1).max()))


def _pos(g, *shape):
    return torch.rand(*shape, generator=g) + 0.5


def _rank_rows(x, R):
    """x (..., L) -> (..., R, L) with x in rank row 0 and zeros in the others."""
    out = torch.zeros(*x.shape[:-1], R, x.shape[-1])
    out[..., 0, :] = x
    return out


def _unit_Wdt(d, R):
    W = torch.zeros(d, R)
    W[:, 0] = 1.0
    return W


def memoryless_sweep(form, shape):
    """A case of `form` in which A = -1e30 wipes the state at every step, so that y_l = softplus(x_l) u_l <B_l, C_l> + D u_l and
    d(delta)_l = sigmoid(x_l) u_l <B_l, C_l> dout_l probe softplus and its derivative at x_l alone.  u, B, C, D and dout are
    positive: nothing that is checked element-wise is a cancelling sum."""
    g = torch.Generator().manual_seed(_seed("sweep", form, shape))
    if form == "direct":
        b, G, Hc, L = shape
        d = G * Hc
        x = _sweep_rows(b * d, L).view(b, d, L)
        bias = 0.25 * (torch.arange(d) % 3 - 1).float()                 # -0.25, 0, 0.25: x - bias is exact where bias is 0
        delta = x - bias[None, :, None]
        xe = delta + bias[None, :, None]                                # what the kernel forms in float32
        exact = (torch.arange(d) % 3 == 1)
        assert torch.equal(xe[:, exact], x[:, exact])
        _check_sweep(xe[:, exact])
        assert float(xe.min()) >= SWEEP_LO and float(xe.max()) <= SWEEP_HI
        return dict(u=_pos(g, b, d, L), delta=delta.contiguous(), A=torch.full((d, N), SWEEP_A), B=_pos(g, b, G, N, L),
                    C=_pos(g, b, G, N, L), D=_pos(g, d), bias=bias, dout=_pos(g, b, d, L))
    if form == "lowrank":
        b, G, Hc, L, R = shape
        d = G * Hc
        x = _sweep_rows(b * G, L).view(b, G, L)
        _check_sweep(x)
        return dict(u=_pos(g, b, d, L), dtr=_rank_rows(x, R), Wdt=_unit_Wdt(d, R), A=torch.full((d, N), SWEEP_A),
                    B=_pos(g, b, G, N, L), C=_pos(g, b, G, N, L), D=_pos(g, d), bias=torch.zeros(d), dout=_pos(g, b, d, L))
    if form == "msmm":
        b, HW = shape
        K, HC, R, XB = MSMM_K, MSMM_HC, MSMM_R, MSMM_XB
        idx = reference_orders(HW)
        L = idx.shape[1]
        x = _sweep_rows(b * K, L).view(b, K, L)
        _check_sweep(x)
        xdbl = torch.zeros(b, L, K, XB)
        xdbl[..., 4:] = _pos(g, b, L, K, 2 * N)
        for k in range(K):
            xdbl[:, idx[k], k, 0] = x[:, k]                             # direction k meets the sweep in ITS scan order
        return dict(xc=_pos(g, b, L, HC), xdbl=xdbl.view(b, L, K * XB), Wdt=_unit_Wdt(K * HC, R), A=torch.full((K * HC, N), SWEEP_A),
                    D=_pos(g, K * HC), bias=torch.zeros(K * HC), dout=_pos(g, b, L, HC), idx=idx)
    if form == "sel1":
        B, L, C, K, R = shape
        x = _sweep_rows(B * K, L).view(B, K, L)
        _check_sweep(x)
        return dict(tok=_pos(g, B, L, C), idx=sel1_orders(L, K, g), dtr=_rank_rows(x, R), Bs=_pos(g, B, K, L), Cs=_pos(g, B, K, L),
                    Wdt=_unit_Wdt(K * C, R), A=torch.full((K * C,), SWEEP_A), D=_pos(g, K * C), bias=torch.zeros(K * C),
                    dout=_pos(g, B, L, C))
    raise ValueError(form)


def sweep_closed_form(u, delta, A, B, C, D, bias, dout):
    """y and d(delta) of a memoryless case on its (b, d, L) sequences, float64, without a scan."""
    b, d, L = u.shape
    Hc = d // B.shape[1]
    bc = (B.double() * C.double()).sum(2).repeat_interleave(Hc, dim=1)                          # <B_l, C_l> per channel
    x = delta.double() + bias.double()[None, :, None]
    y = F.softplus(x) * u.double() * bc + D.double()[None, :, None] * u.double()
    sg = torch.where(x > 20.0, torch.ones_like(x), torch.sigmoid(x))
    return y, sg * u.double() * bc * dout.double()


# ------------------------------------------------------------------------------------------------
# regimes with memory
# ------------------------------------------------------------------------------------------------
REGIMES = ("init", "large_step", "integrator")


def _regime_parts(name, d, n_state, g):
    """(A (d, n_state), bias (d), sigma): the softplus argument of channel d is bias[d] + sigma * randn per step."""
    if name == "integrator":
        A = torch.full((d, n_state), -1e-4)
    elif n_state == 1:
        A = -(1.0 + (torch.arange(d) % 16).float()).view(d, 1)
    else:
        A = -(torch.arange(n_state).float() + 1.0).repeat(d, 1)                                   # S4D-real
    if name == "init":
        dt = torch.exp(torch.rand(d, generator=g, dtype=torch.float64) * (np.log(1e-1) - np.log(1e-3)) + np.log(1e-3))
        return A, (dt + torch.log(-torch.expm1(-dt))).float(), 0.3                                # softplus^-1(dt), dt in [1e-3, 1e-1]
    if name == "large_step":
        return A, torch.full((d,), 3.0), 2.0
    if name == "integrator":
        return A, torch.full((d,), -3.0), 0.5
    raise ValueError(name)


def regime(name, form, shape):
    """A case of `form` with memory: "init" (the reference's initialisation of A and dt), "large_step" (delta up to ~10, delta A
    down to -160: underflowing steps among ordinary ones) or "integrator" (A = -1e-4: the state sums the whole sequence)."""
    g = torch.Generator().manual_seed(_seed(name, form, shape))
    rn = lambda *s: torch.randn(*s, generator=g)                                                  # noqa: E731
    if form == "direct":
        b, G, Hc, L = shape
        d = G * Hc
        A, bias, sigma = _regime_parts(name, d, N, g)
        return dict(u=rn(b, d, L), delta=sigma * rn(b, d, L), A=A, B=rn(b, G, N, L), C=rn(b, G, N, L), D=rn(d), bias=bias,
                    dout=rn(b, d, L))
    if form == "lowrank":
        b, G, Hc, L, R = shape
        d = G * Hc
        A, bias, sigma = _regime_parts(name, d, N, g)
        return dict(u=rn(b, d, L), dtr=rn(b, G, R, L), Wdt=rn(d, R) * (sigma * R ** -0.5), A=A, B=rn(b, G, N, L),
                    C=rn(b, G, N, L), D=rn(d), bias=bias, dout=rn(b, d, L))
    if form == "msmm":
        b, HW = shape
        K, HC, R, XB = MSMM_K, MSMM_HC, MSMM_R, MSMM_XB
        idx = reference_orders(HW)
        L = idx.shape[1]
        A, bias, sigma = _regime_parts(name, K * HC, N, g)
        xdbl = rn(b, L, K, XB)
        xdbl[..., 3] = 0.0                                              # the pad column of every direction
        return dict(xc=rn(b, L, HC), xdbl=xdbl.view(b, L, K * XB), Wdt=rn(K * HC, R) * (sigma * R ** -0.5), A=A, D=rn(K * HC),
                    bias=bias, dout=rn(b, L, HC), idx=idx)
    if form == "sel1":
        B, L, C, K, R = shape
        A, bias, sigma = _regime_parts(name, K * C, 1, g)
        return dict(tok=rn(B, L, C), idx=sel1_orders(L, K, g), dtr=rn(B, K, R, L), Bs=rn(B, K, L), Cs=rn(B, K, L),
                    Wdt=rn(K * C, R) * (sigma * R ** -0.5), A=A.view(-1), D=rn(K * C), bias=bias, dout=rn(B, L, C))
    raise ValueError(form)


# ------------------------------------------------------------------------------------------------
# the cases of the two test modules, and their references (computed once per process, never modified)
# ------------------------------------------------------------------------------------------------
SWEEP_CASES = [
    # (form, shape)                                                  what it runs
    ("direct", (2, 2, 96, 1088)),                                   # fast forward, group backward, whole chunks
    ("lowrank", (2, 2, 96, 1088, 3)),                               #   ... with the rank-3 fast form
    ("direct", (1, 2, 96, 1100)),                                   # ragged last chunk
    ("lowrank", (1, 2, 96, 1100, 3)),                               #   ... rank-3 fast form, not whole
    ("lowrank", (1, 2, 96, 1100, 2)),                               # general-rank group backward: vector loads, full slots
    ("lowrank", (1, 2, 20, 132, 2)),                                #   ... vector loads, partial slots
    ("lowrank", (1, 2, 20, 130, 2)),                                #   ... scalar loads
    ("lowrank", (1, 1, 160, 77, 4)),                                # channel-block backward, atomic dB / dC / d(dtr)
    ("msmm", (1, ((32, 32), (8, 8)))),                              # L = 1088: whole chunks
    ("msmm", (1, ((16, 16), (8, 8), (4, 4), (2, 2)))),              # L = 340: ragged last chunk
    ("sel1", (19, 1100, 64, 12, 2)),                                # one channel block; 228 sequences: 128-step chunks
    ("sel1", (1, 300, 128, 3, 4)),                                  # two channel blocks; 64-step chunks
]

REGIME_CASES = [
    ("lowrank", (1, 2, 96, 1100, 3)),
    ("lowrank", (1, 1, 160, 200, 4)),
    ("direct", (1, 2, 96, 1100)),
    ("msmm", (1, ((32, 32), (8, 8)))),
    ("msmm", (1, ((16, 16), (8, 8), (4, 4), (2, 2)))),
    ("sel1", (1, 1100, 64, 2, 2)),
]


def case_id(form, shape):
    return form + "-" + "x".join(str(v) if not isinstance(v, tuple) else "+".join(f"{h}.{w}" for h, w in v) for v in shape)


@functools.lru_cache(maxsize=None)
def sweep_case(form, shape):
    """(case, y, grads): a memoryless case and its oracle reference."""
    case = memoryless_sweep(form, shape)
    return (case,) + reference(form, case)


@functools.lru_cache(maxsize=None)
def regime_case(name, form, shape):
    """(case, (y, grads) of the oracle, (y, grads) of the plain fp32 scan)."""
    case = regime(name, form, shape)
    return case, reference(form, case), reference(form, case, plain_fp32_scan)


def max_scaled_error(got, ref):
    """max |got - ref| / max |ref| (the scale the parity tests use, floored at 1e-6)."""
    ref = torch.as_tensor(ref).double()
    return float((torch.as_tensor(got).double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)
