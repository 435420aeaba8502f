"""Inputs, oracles and yardsticks for the two 16-bit attention kernels, one operation at a time: K4lp (csrc/pooled_attn_lp.hip,
ops.pooled_diff_attn under ops.compute_precision("bf16" | "fp16")) and the flash shim (csrc/flash_attn.hip, shims.flash_attn_func).
Shared by tests/test_attention_lp_regimes_cpu.py (which proves the cases and references sound without a GPU) and
tests/test_attention_lp_regimes_gpu.py (which compares the kernels with them).  Plain torch, no project import; the operation, the
regime builders and the bound are those of tests/_attention_cases.py, imported, not copied.

K4lp.  Rounding the operands is part of the operation ("what flash-attn's 16-bit tensors hold", the kernel's header), so
    ref16    the ORACLE: pooled_diff_attn_ref in float64 on round16(fp32(q * scale)), round16(k), round16(v) with no further scale,
             the rounding straight-through for the gradients (qs = x + (round16(x) - x).detach()); torch's .to(bfloat16 / float16)
             is the round-to-nearest-even of pack2 in csrc/mfma.h
    emul16   the YARDSTICK: the same operation in float64 arithmetic with a rounding at every point at which the kernels hold a value
             in a documented format, forward and a hand-written backward (the formulas of the kernel's header):
                 16 bit   the softmax weights before the product with V; d(o) after the RMSNorm backward; dS; w = P1 - lam P2
                          before the dV product
                 fp32     lse, o1, o2 (saved by the forward), o = o1 - lam o2 as the RMSNorm backward forms it again, and d(o), D1, D2
                          in the workspace ("every tensor in HBM stays fp32"); D1 = d(o) . o1, D2 = -lam d(o) . o2 and
                          d(lam) = -sum d(o) . o2 are formed from the fp32 d(o), dW = d(o) V^T from the 16-bit one
             It plays the role the plain fp32 reference plays for the fp32 kernels: max|emul16 - ref16| is what the documented
             roundings alone produce on a case, and the bound of a tensor is max(T max|ref16|, 4 max|emul16 - ref16|), with 1 in
             place of max|ref16| where the reference is identically zero (the convention of `scaled`).
Flash shim.  Its inputs are 16-bit already: the oracle is exact float64 attention on them, the yardstick rounds what the kernels
round (out, and with it D = dout . out; dq, dk, dv on their way out; lse to fp32), and the bound is the 3 output ulps + 1e-6 of
tests/test_flash_shim_gpu.py.

Regimes (REGIME_LAM of tests/_attention_cases.py):
    init    randn operands, lam 0.2 or 0.8
    peaked  `_peak` applied to the ROUNDED-operand logits until the largest scaled logit is +100 after rounding (within two operand
            ulps of 100: a factor that is not a power of two moves the roundings again); the key of that logit is then moved to
            index 0 ("first") or to index P - 1 ("last": the last, ragged key tile, after large partial sums).  lam = 1.5
    flat    k = 0: weights exactly 1 / P, o = (1 - lam) mean(round16(v)); the shim's out = round16(mean(v))
    cancel  tied maps and lam = 1 (K4lp only): A == 0, rstd = eps^-0.5, finite non-trivial gradients
Loss scale (K4lp only, outputs are fp32): the operands of the "init" case of LOSS_SHAPE under an upstream gradient dout of rms 1 / 4
(LOSS_DOUT_RMS times the case's own), with dout * 2^12 under fp16 (GradScaler territory) and dout * 2^-12 under bf16; the oracle's
gradients are 2^+-12 times those under dout, exactly.  With rms 1 / 4 the 16-bit d(o) and dS operands of the fp16 run keep three
bits of headroom below 65504 (the CPU test asserts it); with rms 1 the largest d(o) is 22 672, a third of the largest fp16 number."""
import functools

import torch

from tests._attention_cases import (HD, HD2, OUT_GAIN, PLAIN_MARGIN, REGIME_LAM, RMS_EPS, SCALE_A, SCALE_B, _peak, _seed,
                                    _subln, _tie_maps, bound, max_err, pooled_diff_attn_ref, pooled_parts, scaled)        # noqa: F401 (max_err, scaled: for the tests)

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
T_K4LP = {"fp16": 4e-3, "bf16": 3e-2}              # tests/test_pooled_attn_lp_gpu.py
ULP = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -8}      # one output ulp relative to the largest value: tests/test_flash_shim_gpu.py
FP16_HEADROOM = 65504.0 / 8
K4LP_LEAVES = ("q", "kp", "vp", "lam", "subln_w")
FLASH_LEAVES = ("q", "k", "v")
E = HD                                             # the shim's head_dim
FLASH_SCALE = E ** -0.5


def round16(x, dt):
    """x rounded to fp32 and then to the 16-bit type `dt` ("fp16", "bf16"; None: x itself), in x's own dtype."""
    return x if dt is None else x.float().to(DTYPES[dt]).to(x.dtype)


def r32(x, dt):
    """x rounded to fp32 (dt None: x itself)."""
    return x if dt is None else x.float().to(x.dtype)


def scale32(scale):
    """The scale as the launcher receives it: a C float."""
    return float(torch.tensor(scale, dtype=torch.float32))


def k4lp_bound(ref, emul, T):
    """max(T max|ref|, PLAIN_MARGIN max|emul16 - ref16|); an identically zero reference counts as max|ref| = 1."""
    if float(ref.abs().max()) == 0.0:
        return max(T, PLAIN_MARGIN * float(emul.double().abs().max()))
    return bound(ref, emul, T, PLAIN_MARGIN)


def flash_bound(ref, dt):
    return 3 * ULP[dt] * float(ref.abs().max()) + 1e-6


# ------------------------------------------------------------------------------------------------
# K4lp: oracle and yardstick
# ------------------------------------------------------------------------------------------------
def rounding_offsets(q, kp, vp, scale, dt):
    """round16(x) - x of x = q * scale, k, v: constants of the straight-through rounding."""
    with torch.no_grad():
        return [round16(x, dt) - x for x in (q * scale32(scale), kp, vp)]


def operands16(q, kp, vp, scale, dt, offsets=None):
    """round16(fp32(q * scale)), round16(k), round16(v), straight-through: x + (round16(x) - x).detach().  For fp32 values held in
    float64 the float64 product with the fp32 scale is exact, so its rounding to fp32 inside round16 is the kernel's fp32 product.
    `offsets`: the rounding offsets of another point (a finite-difference check holds them fixed, as the gradient does)."""
    offsets = rounding_offsets(q, kp, vp, scale, dt) if offsets is None else offsets
    return [x + o for x, o in zip((q * scale32(scale), kp, vp), offsets)]


def ref16(q, kp, vp, lam, subln_w, nh, scale, dt, offsets=None):
    qs, k16, v16 = operands16(q, kp, vp, scale, dt, offsets)
    return pooled_diff_attn_ref(qs, k16, v16, lam, subln_w, nh, 1.0)


CHUNK_ELEMS = 1 << 24                 # pooled_parts forms B N P nh 48 products at once: above this many, one (batch, head, 1024 tokens) at a time


def run_ref16(leaves, dout, nh, scale, dt):
    """ref16 and the gradients of every leaf under dout in float64: (y, {leaf: gradient}).  Every token of every (batch, head) is
    independent of the others, so a large case runs block by block through the same function and autograd adds up the gradients."""
    lv = {k: t.detach().double().requires_grad_(True) for k, t in leaves.items()}
    dout = dout.double()
    B, N, d = lv["q"].shape
    P = lv["kp"].shape[1]
    if B * N * P * d <= CHUNK_ELEMS:
        y = ref16(*lv.values(), nh, scale, dt)
        y.backward(dout)
        return y.detach(), {k: t.grad for k, t in lv.items()}
    y = torch.empty(B, N, d, dtype=torch.float64)
    for b in range(B):
        for h in range(nh):
            c = slice(h * HD2, (h + 1) * HD2)
            for n0 in range(0, N, 1024):
                n = slice(n0, min(N, n0 + 1024))
                yc = ref16(lv["q"][b:b + 1, n, c], lv["kp"][b:b + 1, :, c], lv["vp"][b:b + 1, :, c], lv["lam"], lv["subln_w"], 1, scale, dt)
                yc.backward(dout[b:b + 1, n, c])
                y[b:b + 1, n, c] = yc.detach()
    return y, {k: t.grad for k, t in lv.items()}


def emul16(leaves, dout, nh, scale, dt):
    """The yardstick (see the module's docstring): (y, {leaf: gradient}, {"o12": (2, B, N, d), "dO", "dS": the largest magnitude of
    the 16-bit d(o) and dS operands}), float64, no autograd.  dt None: no rounding anywhere -- ref16's output and gradients."""
    lv = {k: t.detach().double() for k, t in leaves.items()}
    dout = dout.double()
    B, N, d = lv["q"].shape
    P = lv["kp"].shape[1]
    lam, w, sc = lv["lam"], lv["subln_w"], scale32(scale)
    rnd = lambda x: round16(x, dt)                                                                 # noqa: E731
    qs, k16, v16 = (rnd(lv["q"] * sc), rnd(lv["kp"]), rnd(lv["vp"]))
    y, o12 = torch.empty(B, N, d, dtype=torch.float64), torch.empty(2, B, N, d, dtype=torch.float64)
    g = dict(q=torch.empty(B, N, d, dtype=torch.float64), kp=torch.empty(B, P, d, dtype=torch.float64),
             vp=torch.empty(B, P, d, dtype=torch.float64), lam=torch.zeros((), dtype=torch.float64), subln_w=torch.zeros(HD2, dtype=torch.float64))
    top = dict(dO=0.0, dS=0.0)
    sg = torch.stack([torch.ones_like(lam), -lam]).view(2, 1, 1)
    for b in range(B):
        for h in range(nh):
            c = slice(h * HD2, (h + 1) * HD2)
            qh, kh, vh = qs[b, :, c].reshape(N, 2, HD), k16[b, :, c].reshape(P, 2, HD), v16[b, :, c]
            # forward
            S = torch.einsum("nrc,prc->rnp", qh, kh)
            lse = r32(torch.logsumexp(S, -1, keepdim=True), dt)
            Pm = torch.exp(S - lse)                                                                # (2, N, P)
            o = r32(rnd(Pm) @ vh, dt)                                                              # (2, N, 48): o1, o2
            o12[:, b, :, c] = o
            od = r32(o[0] - lam * o[1], dt)
            rstd = torch.rsqrt(od.pow(2).mean(-1, keepdim=True) + RMS_EPS)
            y[b, :, c] = OUT_GAIN * w * od * rstd
            # backward prologue: the gain and the RMSNorm, D1, D2, d(lam), d(subln_w)
            gy = dout[b, :, c]
            kk = (OUT_GAIN * w * gy * od).sum(-1, keepdim=True) * rstd * rstd / HD2
            dO = r32(rstd * (OUT_GAIN * w * gy - od * kk), dt)
            g["subln_w"] += (OUT_GAIN * gy * od * rstd).sum(0)
            D1, D2 = (dO * o[0]).sum(-1), (dO * o[1]).sum(-1)
            g["lam"] -= D2.sum()
            D = r32(torch.stack([D1, -lam * D2]), dt).unsqueeze(-1)                                # (2, N, 1)
            # the three MFMA kernels
            dO16 = rnd(dO)
            dS16 = rnd(Pm * (sg * (dO16 @ vh.t()) - D))                                            # (2, N, P)
            g["q"][b, :, c] = (sc * torch.einsum("rnp,prc->nrc", dS16, kh)).reshape(N, HD2)
            g["kp"][b, :, c] = torch.einsum("rnp,nrc->prc", dS16, qh).reshape(P, HD2)
            g["vp"][b, :, c] = rnd(Pm[0] - lam * Pm[1]).t() @ dO16
            top["dO"], top["dS"] = max(top["dO"], float(dO16.abs().max())), max(top["dS"], float(dS16.abs().max()))
    return y, g, dict(o12=o12, **top)


# ------------------------------------------------------------------------------------------------
# K4lp: cases
# ------------------------------------------------------------------------------------------------
def pooled_logits16(q, k, nh, scale, dt):
    """(B, N, P, nh, 2) float64: the scaled logits of the rounded operands."""
    B, N, d = q.shape
    P = k.shape[1]
    qs, k16 = round16(q.double() * scale32(scale), dt), round16(k.double(), dt)
    return torch.einsum("bnhmc,bphmc->bnphm", qs.reshape(B, N, nh, 2, HD), k16.reshape(B, P, nh, 2, HD))


def _peak16(q, k, logits16):
    """`_peak` until the largest logit of the rounded operands is +PEAK_LOGIT: the factor is no power of two, so it moves the roundings,
    and a few rounds bring the extreme to within rounding noise of the peak."""
    for _ in range(4):
        q, k = _peak(q, k, logits16(q, k))
    return q, k


def _move_key(key, place, P, *tensors):
    """Exchange key `key` and key 0 ("first") or P - 1 ("last") in every (B, P, ...) tensor."""
    to = 0 if place == "first" else P - 1
    out = []
    for t in tensors:
        t = t.clone()
        t[:, [key, to]] = t[:, [to, key]]
        out.append(t)
    return out


def k4lp_case_inputs(regime, B, N, P, nh, scale, lam, dt, place=None):
    g = torch.Generator().manual_seed(_seed("k4lp", regime, B, N, P, nh))
    rn = lambda *s: torch.randn(*s, generator=g)                                                   # noqa: E731
    d = nh * HD2
    q, k, v = rn(B, N, d), rn(B, P, d), rn(B, P, d)
    subln_w, dout = 1.0 + 0.2 * rn(HD2), rn(B, N, d)
    if regime == "peaked":
        q, k = _peak16(q, k, lambda q_, k_: pooled_logits16(q_, k_, nh, scale, dt))
        lg = pooled_logits16(q, k, nh, scale, dt)
        key = int(lg.amax((0, 1, 3, 4)).argmax())
        k, v = _move_key(key, place, P, k, v)
    elif regime == "flat":
        k = torch.zeros_like(k)
    elif regime == "cancel":
        q, k = _tie_maps(q, nh), _tie_maps(k, nh)
    return dict(q=q, kp=k, vp=v, lam=torch.tensor(REGIME_LAM.get(regime, lam)), subln_w=subln_w), dout


# (B, N, P, nh, scale, lam of "init", strided): strided = q, dout, k and v are all column blocks of wider rows
K4LP_SHAPES = [
    (2, 1, 1, 1, SCALE_B, 0.2, False),        # one token, one key: lane half kh = 1 entirely masked
    (1, 33, 16, 2, SCALE_B, 0.8, True),       # half a key tile
    (2, 255, 17, 1, SCALE_A, 0.2, False),     # one key past half a tile; the token block one short
    (1, 256, 32, 1, SCALE_B, 0.8, False),     # exactly one token block, one key tile
    (2, 257, 33, 2, SCALE_B, 0.2, True),      # one token and one key past: the second tile holds one key
    (1, 70, 320, 4, SCALE_A, 0.8, True),      # 10 key tiles: the key-side kernel's 640-thread block
    (2, 3201, 320, 8, SCALE_B, 0.2, False),   # the smallest N at which the key-side kernel takes 128-token chunks; the last holds one token
]
K4LP_REGIME_SHAPES = [K4LP_SHAPES[4], K4LP_SHAPES[5]]
K4LP_CHUNK_SHAPE = K4LP_SHAPES[6]
LOSS_SHAPE = K4LP_SHAPES[4]
LOSS_SCALE = {"fp16": 2.0 ** 12, "bf16": 2.0 ** -12}
LOSS_DOUT_RMS = 0.25
PLACES = ("first", "last")

# (regime, shape, dt, place)
K4LP_CASES = ([("init", s, dt, None) for dt in DTYPES for s in K4LP_SHAPES[:6]] + [("init", K4LP_CHUNK_SHAPE, "fp16", None)] +
              [("peaked", s, dt, pl) for dt in DTYPES for s in K4LP_REGIME_SHAPES for pl in PLACES] +
              [(r, s, dt, None) for r in ("flat", "cancel") for dt in DTYPES for s in K4LP_REGIME_SHAPES])


def k4lp_id(regime, shape, dt, place=None):
    B, N, P, nh, scale = shape[:5]
    return f"k4lp-{dt}-{regime}{'-' + place if place else ''}-{B}x{N}x{P}x{nh}-{'B' if scale == SCALE_B else 'A'}"


K4LP_IDS = [k4lp_id(*c) for c in K4LP_CASES]


@functools.lru_cache(maxsize=None)
def k4lp_case(regime, shape, dt, place=None):
    """dict(leaves, dout, nh, scale, dt, ref=(y, grads) the oracle, emul=(y, grads, extra) the yardstick) -- computed once, never modified."""
    B, N, P, nh, scale, lam, _ = shape
    leaves, dout = k4lp_case_inputs(regime, B, N, P, nh, scale, lam, dt, place)
    return dict(leaves=leaves, dout=dout, nh=nh, scale=scale, dt=dt, ref=run_ref16(leaves, dout, nh, scale, dt),
                emul=emul16(leaves, dout, nh, scale, dt))


@functools.lru_cache(maxsize=None)
def k4lp_loss_case(dt):
    """The "init" case of LOSS_SHAPE under LOSS_DOUT_RMS dout * LOSS_SCALE[dt]: the oracle's gradients are the factor times those of the
    case (a power of two: exact), the yardstick is formed anew (its roundings see the scaled operands)."""
    base = k4lp_case("init", LOSS_SHAPE, dt)
    f = LOSS_DOUT_RMS * LOSS_SCALE[dt]
    dout = base["dout"] * f
    y, grads = base["ref"]
    return dict(base, dout=dout, ref=(y, {k: t * f for k, t in grads.items()}), emul=emul16(base["leaves"], dout, base["nh"], base["scale"], dt))


def k4lp_flat_closed_form(case):
    """The output of a "flat" case without a softmax: o = (1 - lam) mean(round16(v)) through the norm, float64."""
    lv = {k: t.double() for k, t in case["leaves"].items()}
    B, N, d = lv["q"].shape
    o = ((1.0 - lv["lam"]) * round16(lv["vp"], case["dt"]).mean(1, keepdim=True)).expand(B, N, d)
    return _subln(o.reshape(B, N, case["nh"], HD2), lv["subln_w"]).reshape(B, N, d)


def k4lp_parts(case):
    """pooled_parts of the rounded operands, float64: s (B, N, nh, 2, P), o, attn."""
    lv = {k: t.double() for k, t in case["leaves"].items()}
    with torch.no_grad():
        qs, k16, v16 = operands16(lv["q"], lv["kp"], lv["vp"], case["scale"], case["dt"])
        return pooled_parts(qs, k16, v16, lv["lam"], lv["subln_w"], case["nh"], 1.0), v16


def k4lp_rows(case, y, grads):
    """(name, kernel's tensor, oracle's, yardstick's) of the output and every gradient."""
    (y_ref, g_ref), (y_em, g_em, _) = case["ref"], case["emul"]
    return [("y", y, y_ref, y_em)] + [(k, grads[k], g_ref[k], g_em[k]) for k in K4LP_LEAVES]


# ------------------------------------------------------------------------------------------------
# flash shim: oracle, yardstick, cases
# ------------------------------------------------------------------------------------------------
def flash_ref(q, k, v, scale):
    """Exact attention: q (B, N, nh, e), k / v (B, P, nh, e) -> (B, N, nh, e); the scale is the C float the launcher receives."""
    att = torch.einsum("bnhe,bphe->bhnp", q, k) * scale32(scale)
    return torch.einsum("bhnp,bphe->bnhe", att.softmax(-1), v)


def run_flash_ref(leaves, dout, scale):
    lv = {k: t.detach().double().requires_grad_(True) for k, t in leaves.items()}
    y = flash_ref(*lv.values(), scale)
    y.backward(dout.double())
    return y.detach(), {k: t.grad for k, t in lv.items()}


def flash_emul(leaves, dout, scale, dt):
    """Float64 arithmetic with the kernels' roundings: lse to fp32, out to 16 bits and D = dout . out of the rounded out, dq / dk / dv
    to 16 bits on their way out."""
    q, k, v = (leaves[n].double() for n in FLASH_LEAVES)
    dout = dout.double()
    rnd = lambda x: round16(x, dt)                                                                 # noqa: E731
    S = torch.einsum("bnhe,bphe->bhnp", q, k) * scale32(scale)
    Pm = torch.exp(S - r32(torch.logsumexp(S, -1, keepdim=True), dt))
    out = rnd(torch.einsum("bhnp,bphe->bnhe", Pm, v))
    D = (dout * out).sum(-1).permute(0, 2, 1).unsqueeze(-1)                                        # (B, nh, N, 1)
    dS = Pm * (torch.einsum("bnhe,bphe->bhnp", dout, v) - D) * scale32(scale)
    return out, dict(q=rnd(torch.einsum("bhnp,bphe->bnhe", dS, k)), k=rnd(torch.einsum("bhnp,bnhe->bphe", dS, q)),
                     v=rnd(torch.einsum("bhnp,bnhe->bphe", Pm, dout)))


def flash_logits(q, k, scale):
    """(B, N, P, nh) float64."""
    return torch.einsum("bnhe,bphe->bnph", q.double(), k.double()) * scale32(scale)


def flash_case_inputs(regime, B, N, P, nh, dt, place=None):
    g = torch.Generator().manual_seed(_seed("flash", regime, B, N, P, nh))
    rn = lambda *s: torch.randn(*s, generator=g)                                                   # noqa: E731
    q, k, v, dout = rn(B, N, nh, E), rn(B, P, nh, E), rn(B, P, nh, E), rn(B, N, nh, E)
    if regime == "peaked":
        q, k = _peak16(q, k, lambda q_, k_: flash_logits(round16(q_, dt), round16(k_, dt), FLASH_SCALE))
        lg = flash_logits(round16(q, dt), round16(k, dt), FLASH_SCALE)
        k, v = _move_key(int(lg.amax((0, 1, 3)).argmax()), place, P, k, v)
    elif regime == "flat":
        k = torch.zeros_like(k)
    to16 = lambda t: t.to(DTYPES[dt])                                                              # noqa: E731
    return dict(q=to16(q), k=to16(k), v=to16(v)), to16(dout)


# (B, N, P, nh): N around the 256-token workgroup and the 512-token chunk of backward-2, P up to the launcher's limit of 512
FLASH_SHAPES = [(1, 1, 1, 1), (2, 255, 49, 2), (1, 256, 64, 1), (2, 257, 65, 2), (1, 513, 321, 1), (1, 70, 512, 4)]
FLASH_REGIME_SHAPES = [FLASH_SHAPES[3], FLASH_SHAPES[4]]
FLASH_CASES = ([("init", s, dt, None) for dt in DTYPES for s in FLASH_SHAPES] +
               [("peaked", s, dt, pl) for dt in DTYPES for s in FLASH_REGIME_SHAPES for pl in PLACES] +
               [("flat", s, dt, None) for dt in DTYPES for s in FLASH_REGIME_SHAPES])


def flash_id(regime, shape, dt, place=None):
    return f"flash-{dt}-{regime}{'-' + place if place else ''}-" + "x".join(str(n) for n in shape)


FLASH_IDS = [flash_id(*c) for c in FLASH_CASES]


@functools.lru_cache(maxsize=None)
def flash_case(regime, shape, dt, place=None):
    leaves, dout = flash_case_inputs(regime, *shape, dt, place)
    return dict(leaves=leaves, dout=dout, dt=dt, ref=run_flash_ref(leaves, dout, FLASH_SCALE), emul=flash_emul(leaves, dout, FLASH_SCALE, dt))


def flash_flat_closed_form(case):
    """round16(mean(v)) over the keys, for every token: (B, N, nh, e) float64."""
    v = case["leaves"]["v"].double()
    return round16(v.mean(1, keepdim=True), case["dt"]).expand(v.shape[0], case["leaves"]["q"].shape[1], *v.shape[2:])


def flash_rows(case, y, grads):
    (y_ref, g_ref), (y_em, g_em) = case["ref"], case["emul"]
    return [("out", y, y_ref, y_em)] + [("d" + k, grads[k], g_ref[k], g_em[k]) for k in FLASH_LEAVES]
