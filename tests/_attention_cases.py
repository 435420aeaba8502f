"""Inputs and references for the three fp32 kernels on the hot path of every MLLA block, one operation at a time: K3 (csrc/local_attn.hip,
ops.local_diff_attn), K4 (csrc/pooled_attn.hip, ops.pooled_diff_attn in fp32 mode) and K7 (csrc/gate.hip, ops.gate).  Shared by
tests/test_attention_regimes_cpu.py (which proves the references and the cases sound without a GPU) and
tests/test_attention_regimes_gpu.py (which compares the kernels with them).  Plain torch, no project import.

The references are written from the reference trainer's formulas (AggregatedAttention, T:625-784; MLLABlock's gate, T:888-902) and the
kernel headers, dtype-generic: run at float64 they are the oracle, run at float32 they are what ordinary fp32 arithmetic gives on the
same inputs -- the yardstick for how well conditioned a case is, as `plain_fp32_scan` is for the selective scans.

Layout.  A head has 48 channels: map "+" reads q / k channels [0, 24) of the head, map "-" channels [24, 48), v and the output use
all 48.  `kv[..., :d]` is k and `kv[..., d:]` is v.  A = softmax(map +) - lam softmax(map -), o = A V, y = 0.2 subln_w o rsqrt(mean(o^2)
+ 1e-5); K3 takes the softmaxes over the 3x3 window (positions outside the image excluded) and adds the zero-padded depthwise 3x3
LePE of v with bias, K4 takes them over all P pooled keys.

Regimes of K3 / K4 (`REGIMES`):
    init    randn operands, lam 0.2 or 0.8 (the module's initial value)
    peaked  q and k scaled by one factor (k negated where the extreme logit was negative) so that the scaled logit of largest
            magnitude is +PEAK_LOGIT = +100: the bulk of the logits spans about +-80, the largest passes ln(FLT_MAX) = 88.7, so exp
            overflows in fp32 without the max subtraction, rows are one-hot to fp32, and K4's lse = m + log z carries a large m.
            lam = 1.5
    flat    k = 0: every valid logit is equal, s = 1 / count exactly and o = (1 - lam) mean(v) over the valid window / all keys.  lam = 0.8
    cancel  q2 = q1, k2 = k1, lam = 1: A is identically zero in any precision, o = 0, rstd = eps^-0.5; K4's output is 0, K3's the LePE
            term, and the gradients are finite and non-trivial
K7 sweep: act runs over a grid on [-80, 80] with 0, the integers and the root of silu' (+-1.27846); a and dout are uniform in [0.5, 2],
so nothing that is compared element-wise is a cancelling sum; |act| <= 80 keeps every float64 value a normal fp32 number."""
import functools
import zlib

import torch
import torch.nn.functional as F

HD, HD2 = 24, 48                          # head_dim; channels per head in q / k / v / out
RMS_EPS, OUT_GAIN = 1e-5, 0.2             # RMSNorm eps; 1 - lambda_init (T:717)
SCALE_B, SCALE_A = 24 ** -0.5, 1.0 / 24   # variant B (fp32 path) and variant A (the flash path's double scaling)
PEAK_LOGIT = 100.0

REGIMES = ("init", "peaked", "flat", "cancel")
REGIME_LAM = {"peaked": 1.5, "flat": 0.8, "cancel": 1.0}

LEAVES = {
    "k3": ("q", "kv", "lam", "subln_w", "lepe_w", "lepe_b"),
    "k4": ("q", "kp", "vp", "lam", "subln_w"),
    "k7": ("a0", "a1", "act"),
}

# The tolerances of tests/test_blocks_gpu.py::test_aggregated_attention_matches_oracle: (T, rtol) of the output, of the gradients of
# activations (dq, dk, dv; K7: da, dact) and of parameter gradients.
TOL_Y, TOL_ACT, TOL_PARAM = (2e-5, 1e-4), (5e-5, 1e-3), (2e-4, 2e-3)
PARAMS = ("lam", "subln_w", "lepe_w", "lepe_b")
PLAIN_MARGIN = 4.0                        # the margin the scan tests give a kernel that rounds in another order than the plain loop


def tol_of(name):
    """(T, rtol) of the tensor `name` ("y" or a leaf's name)."""
    return TOL_Y if name == "y" else TOL_PARAM if name in PARAMS else TOL_ACT


def bound(ref, plain, T, margin=PLAIN_MARGIN):
    """Absolute error bound of a tensor: max(T max|ref|, margin max|plain_fp32 - ref|); margin 0 leaves the first term alone."""
    ref = ref.double()
    second = margin * float((plain.double() - ref).abs().max()) if margin else 0.0
    return max(T * float(ref.abs().max()), second)


def max_err(got, ref):
    return float((got.double() - ref.double()).abs().max())


def scaled(err, ref):
    """err / max|ref| (1 where the reference is identically zero)."""
    return err / (float(ref.abs().max()) or 1.0)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def window_valid(H, W):
    """(N, 9) bool: window position j = 3 (dy + 1) + (dx + 1) of token (y, x) lies inside the image."""
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    cols = []
    for j in range(9):
        yy, xx = ys + j // 3 - 1, xs + j % 3 - 1
        cols.append(((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).reshape(-1))
    return torch.stack(cols, 1)


def windows(x, H, W):
    """(B, N, C) token-major map -> (B, N, 9, C): the zero-padded 3x3 neighbourhood of every token."""
    B, N, C = x.shape
    p = F.pad(x.reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
    return torch.stack([p[:, j // 3:j // 3 + H, j % 3:j % 3 + W] for j in range(9)], 3).reshape(B, N, 9, C)


def _subln(o, subln_w):
    return o * torch.rsqrt(o.pow(2).mean(-1, keepdim=True) + RMS_EPS) * subln_w * OUT_GAIN


def local_parts(q, kv, lam, subln_w, lepe_w, lepe_b, H, W, nh, scale):
    """The pieces of K3's operation: s (B, N, nh, 2, 9) the two window softmaxes, o (B, N, nh, 48) = A V, attn and lepe (B, N, d)."""
    B, N, d = q.shape
    k, v = kv[..., :d], kv[..., d:]
    qh = q.reshape(B, N, 1, nh, 2, HD)
    kw = windows(k, H, W).reshape(B, N, 9, nh, 2, HD)
    vw = windows(v, H, W)                                                   # (B, N, 9, d)
    logits = (qh * kw).sum(-1).permute(0, 1, 3, 4, 2) * scale               # (B, N, nh, 2, 9)
    valid = window_valid(H, W).view(1, N, 1, 1, 9)
    s = logits.masked_fill(~valid, float("-inf")).softmax(-1)
    A = s[:, :, :, 0] - lam * s[:, :, :, 1]                                 # (B, N, nh, 9)
    o = (A.unsqueeze(-1) * vw.reshape(B, N, 9, nh, HD2).permute(0, 1, 3, 2, 4)).sum(3)       # (B, N, nh, 48)
    attn = _subln(o, subln_w).reshape(B, N, d)
    lepe = (vw * lepe_w.reshape(d, 9).t()).sum(2) + lepe_b
    return dict(s=s, o=o, attn=attn, lepe=lepe)


def local_diff_attn_ref(q, kv, lam, subln_w, lepe_w, lepe_b, H, W, nh, scale):
    p = local_parts(q, kv, lam, subln_w, lepe_w, lepe_b, H, W, nh, scale)
    return p["attn"] + p["lepe"]


def pooled_parts(q, kp, vp, lam, subln_w, nh, scale):
    """s (B, N, nh, 2, P), o (B, N, nh, 48) and attn (B, N, d) of K4's operation."""
    B, N, d = q.shape
    P = kp.shape[1]
    qh = q.reshape(B, N, 1, nh, 2, HD)
    kh = kp.reshape(B, 1, P, nh, 2, HD)
    s = ((qh * kh).sum(-1).permute(0, 1, 3, 4, 2) * scale).softmax(-1)      # (B, N, nh, 2, P)
    A = s[:, :, :, 0] - lam * s[:, :, :, 1]                                 # (B, N, nh, P)
    o = torch.einsum("bnhp,bphc->bnhc", A, vp.reshape(B, P, nh, HD2))
    return dict(s=s, o=o, attn=_subln(o, subln_w).reshape(B, N, d))


def pooled_diff_attn_ref(q, kp, vp, lam, subln_w, nh, scale):
    return pooled_parts(q, kp, vp, lam, subln_w, nh, scale)["attn"]


def gate_ref(a0, a1, act):
    return torch.cat([a0, a1], -1) * F.silu(act)


def run_reference(fn, leaves, dout, dtype, *geom):
    """fn(*leaves, *geom) and the gradients of every leaf under dout, all at `dtype`: (y, {leaf name: gradient}) as float64."""
    lv = {k: t.detach().clone().to(dtype).requires_grad_(True) for k, t in leaves.items()}
    y = fn(*lv.values(), *geom)
    y.backward(dout.to(dtype))
    return y.detach().double(), {k: t.grad.double() for k, t in lv.items()}


# ------------------------------------------------------------------------------------------------
# K3 / K4 cases
# ------------------------------------------------------------------------------------------------
def _tie_maps(t, nh):
    """Channels of map "-" := channels of map "+", head by head."""
    h = t.reshape(*t.shape[:-1], nh, 2, HD).clone()
    h[..., 1, :] = h[..., 0, :]
    return h.reshape(t.shape)


def _peak(q, k, logits):
    """q and k times one factor, k negated if need be, so that the scaled logit of largest magnitude (float64 `logits` of the
    unscaled operands) becomes +PEAK_LOGIT: it is the POSITIVE extreme that overflows exp without the max subtraction."""
    ext = float(logits.flatten()[logits.abs().argmax()])
    f = (PEAK_LOGIT / abs(ext)) ** 0.5
    return (q.double() * f).float(), (k.double() * (f if ext > 0 else -f)).float()


def local_case_inputs(regime, B, H, W, nh, scale, lam):
    g = torch.Generator().manual_seed(_seed("k3", regime, B, H, W, nh))
    rn = lambda *s: torch.randn(*s, generator=g)                                                   # noqa: E731
    N, d = H * W, nh * HD2
    q, k, v = rn(B, N, d), rn(B, N, d), rn(B, N, d)
    lv = dict(subln_w=1.0 + 0.2 * rn(HD2), lepe_w=0.3 * rn(d, 1, 3, 3), lepe_b=0.1 * rn(d))
    dout = rn(B, N, d)
    if regime == "peaked":
        kw = windows(k.double(), H, W).reshape(B, N, 9, nh, 2, HD)
        lg = (q.double().reshape(B, N, 1, nh, 2, HD) * kw).sum(-1) * scale                         # zero outside the image
        q, k = _peak(q, k, lg)
    elif regime == "flat":
        k = torch.zeros_like(k)
    elif regime == "cancel":
        q, k = _tie_maps(q, nh), _tie_maps(k, nh)
    leaves = dict(q=q, kv=torch.cat([k, v], -1), lam=torch.tensor(REGIME_LAM.get(regime, lam)), **lv)
    return leaves, dout


def pooled_case_inputs(regime, B, N, P, nh, scale, lam):
    g = torch.Generator().manual_seed(_seed("k4", regime, B, N, P, nh))
    rn = lambda *s: torch.randn(*s, generator=g)                                                   # noqa: E731
    d = nh * HD2
    q, k, v = rn(B, N, d), rn(B, P, d), rn(B, P, d)
    subln_w, dout = 1.0 + 0.2 * rn(HD2), rn(B, N, d)
    if regime == "peaked":
        lg = torch.einsum("bnhmc,bphmc->bnphm", q.double().reshape(B, N, nh, 2, HD), k.double().reshape(B, P, nh, 2, HD)) * scale
        q, k = _peak(q, k, lg)
    elif regime == "flat":
        k = torch.zeros_like(k)
    elif regime == "cancel":
        q, k = _tie_maps(q, nh), _tie_maps(k, nh)
    return dict(q=q, kp=k, vp=v, lam=torch.tensor(REGIME_LAM.get(regime, lam)), subln_w=subln_w), dout


# (B, H, W, nh, lam of "init", strided)
K3_SHAPES = [
    (2, 1, 1, 1, 0.2, False),             # the only key is the token itself
    (2, 1, 3, 1, 0.8, False),             # every token on the border
    (1, 3, 1, 2, 0.2, False),
    (1, 8, 8, 1, 0.8, False),             # exactly one 8x8 tile
    (2, 9, 8, 2, 0.2, True),              # ragged tile in y; q / kv / dout column blocks of wider rows
    (1, 7, 17, 4, 0.8, True),             # ragged tiles in both axes, 3 tiles in x
    (1, 16, 16, 1, 0.2, False),           # 2 x 2 whole tiles: windows across tile edges
]
# (B, N, P, nh, scale, lam of "init", strided)
K4_SHAPES = [
    (2, 1, 1, 1, SCALE_B, 0.2, False),
    (2, 127, 49, 2, SCALE_A, 0.8, True),       # one ragged token block, one ragged key block; q / dout column blocks of wider rows
    (1, 128, 64, 1, SCALE_B, 0.2, False),      # exactly one token block and one key block
    (2, 129, 65, 2, SCALE_B, 0.8, False),      # one token / one key past the block
    (1, 300, 128, 1, SCALE_A, 0.2, False),     # 48 KiB of K / V in LDS: the last P inside the default limit
    (1, 300, 129, 4, SCALE_B, 0.8, True),      # first P past 48 KiB of LDS
    (1, 257, 320, 1, SCALE_A, 0.2, False),     # the largest P of the model (120 KiB), 5 key blocks
]
K3_REGIME_SHAPES = [K3_SHAPES[4], K3_SHAPES[5]]
K4_REGIME_SHAPES = [K4_SHAPES[3], K4_SHAPES[5]]


def k3_id(regime, shape):
    B, H, W, nh = shape[:4]
    return f"k3-{regime}-{B}x{H}x{W}x{nh}"


def k4_id(regime, shape):
    B, N, P, nh, scale = shape[:5]
    return f"k4-{regime}-{B}x{N}x{P}x{nh}-{'B' if scale == SCALE_B else 'A'}"


K3_CASES = [("init", s) for s in K3_SHAPES] + [(r, s) for r in REGIMES[1:] for s in K3_REGIME_SHAPES]
K4_CASES = [("init", s) for s in K4_SHAPES] + [(r, s) for r in REGIMES[1:] for s in K4_REGIME_SHAPES]
K3_IDS = [k3_id(*c) for c in K3_CASES]
K4_IDS = [k4_id(*c) for c in K4_CASES]


@functools.lru_cache(maxsize=None)
def local_case(regime, shape):
    """dict(leaves, dout, geom=(H, W, nh, scale), ref=(y, grads) float64, plain=(y, grads) float32) -- computed once, never modified."""
    B, H, W, nh, lam, _ = shape
    geom = (H, W, nh, SCALE_B)
    leaves, dout = local_case_inputs(regime, B, H, W, nh, SCALE_B, lam)
    return dict(leaves=leaves, dout=dout, geom=geom, ref=run_reference(local_diff_attn_ref, leaves, dout, torch.float64, *geom),
                plain=run_reference(local_diff_attn_ref, leaves, dout, torch.float32, *geom))


@functools.lru_cache(maxsize=None)
def pooled_case(regime, shape):
    B, N, P, nh, scale, lam, _ = shape
    geom = (nh, scale)
    leaves, dout = pooled_case_inputs(regime, B, N, P, nh, scale, lam)
    return dict(leaves=leaves, dout=dout, geom=geom, ref=run_reference(pooled_diff_attn_ref, leaves, dout, torch.float64, *geom),
                plain=run_reference(pooled_diff_attn_ref, leaves, dout, torch.float32, *geom))


def flat_closed_form(kind, case):
    """The output of a "flat" case without a softmax, float64: o = (1 - lam) mean(v) over the valid window (K3) or all keys (K4)."""
    lv = {k: t.double() for k, t in case["leaves"].items()}
    if kind == "k3":
        H, W, nh, _ = case["geom"]
        B, N, d = lv["q"].shape
        vw = windows(lv["kv"][..., d:], H, W)
        count = window_valid(H, W).sum(1).double().view(1, N, 1)
        o = (1.0 - lv["lam"]) * vw.sum(2) / count
        lepe = (vw * lv["lepe_w"].reshape(d, 9).t()).sum(2) + lv["lepe_b"]
        return _subln(o.reshape(B, N, nh, HD2), lv["subln_w"]).reshape(B, N, d) + lepe
    nh = case["geom"][0]
    B, N, d = lv["q"].shape
    o = ((1.0 - lv["lam"]) * lv["vp"].mean(1, keepdim=True)).expand(B, N, d)
    return _subln(o.reshape(B, N, nh, HD2), lv["subln_w"]).reshape(B, N, d)


def lepe_only(case):
    """The LePE term of a K3 case, float64: what a "cancel" case's output must be."""
    lv = {k: t.double() for k, t in case["leaves"].items()}
    H, W, _, _ = case["geom"]
    d = lv["q"].shape[2]
    return (windows(lv["kv"][..., d:], H, W) * lv["lepe_w"].reshape(d, 9).t()).sum(2) + lv["lepe_b"]


# ------------------------------------------------------------------------------------------------
# K7 sweep
# ------------------------------------------------------------------------------------------------
ACT_LIMIT = 80.0
SILU_GRAD_ROOT = 1.2784645427610738       # silu'(-x) = 0: 1 - x (1 - sigmoid(-x)) = 0
# (rows, h, strided)
K7_SHAPES = [
    (1, 4, False),                        # one float4 per half row
    (257, 48, True),                      # act / dout column blocks of wider rows
    (130, 100, True),                     # h no multiple of 16
    (5500, 384, False),                   # 1 056 000 float4 items: one more trip of the grid-stride loop than 4096 x 256 threads cover
]
K7_IDS = [f"k7-{r}x{h}" for r, h, _ in K7_SHAPES]


def sweep_points():
    """The points every sweep of at least this many elements contains: 0, the integers of [-80, 80], +-1.2785 and the float32
    nearest to the root of silu' either side of 0."""
    root = float(torch.tensor(SILU_GRAD_ROOT, dtype=torch.float32))
    return torch.tensor(sorted(set([float(i) for i in range(-80, 81)] + [1.2785, -1.2785, root, -root])), dtype=torch.float32)


def gate_case_inputs(rows, h):
    g = torch.Generator().manual_seed(_seed("k7", rows, h))
    n = rows * 2 * h
    special = sweep_points()
    if n >= special.numel() + 8:
        pts = torch.cat([special, torch.linspace(-ACT_LIMIT, ACT_LIMIT, n - special.numel())])
    else:                                                                  # too few elements for all of them: an even choice
        pts = special[torch.linspace(0, special.numel() - 1, n).round().long()]
    act = pts[torch.randperm(n, generator=g)].reshape(rows, 2 * h)
    pos = lambda *s: 0.5 + 1.5 * torch.rand(*s, generator=g)                                       # noqa: E731
    return dict(a0=pos(rows, h), a1=pos(rows, h), act=act), pos(rows, 2 * h)


@functools.lru_cache(maxsize=None)
def gate_case(shape):
    rows, h, _ = shape
    leaves, dout = gate_case_inputs(rows, h)
    return dict(leaves=leaves, dout=dout, ref=run_reference(gate_ref, leaves, dout, torch.float64),
                plain=run_reference(gate_ref, leaves, dout, torch.float32))


def gate_tolerances(case):
    """Per-element absolute tolerances (float64) of y, da (a0 | a1 side by side) and dact: 2^-20 (4 + |act|) of the value, for dact of
    the condition-aware magnitude |dout a| s (1 + |act| (1 - s)) (silu' has a root), plus the floor 1e-37.  `__expf` rounds
    act log2(e) in fp32, a relative error of about |act| 2^-24 in the exponential: this is roughly 16 times that."""
    act = case["leaves"]["act"].double()
    a = torch.cat([case["leaves"]["a0"], case["leaves"]["a1"]], -1).double()
    dout = case["dout"].double()
    y, grads = case["ref"]
    rel = 2.0 ** -20 * (4.0 + act.abs())
    s = torch.sigmoid(act)
    one_minus_s = torch.sigmoid(-act)
    mag = (dout * a).abs() * s * (1.0 + act.abs() * one_minus_s)
    da = torch.cat([grads["a0"], grads["a1"]], -1)
    return dict(y=rel * y.abs() + 1e-37, da=rel * da.abs() + 1e-37, dact=rel * mag + 1e-37)
