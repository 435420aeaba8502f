"""Cases, references and path predicates for the kernels that END every train step -- K9 Dice + cross-entropy statistics and gradient
(csrc/loss.hip), K29 Dice + BCE of region datasets (csrc/region_loss.hip) and K11 clip + AdamW (csrc/optimizer.hip) -- at the sizes
where their code changes path: shared by tests/test_step_tail_paths_cpu.py and tests/test_step_tail_paths_gpu.py.

A CASE is a namedtuple (K9Case, K29Case, K11Case, K11AbiCase); its inputs come from a generator seeded with the case itself.
`evaluate(case, dtype)` computes every compared quantity on the host in plain torch and never calls the code under test: explicit
log_softmax / sigmoid / softplus formulas for the statistics, autograd on those formulas for d(logits) under RANDOM upstream cotangents
(so that g_ip differs per sample and per class), clip_grad_norm_ + torch.optim.AdamW on copies of the parameters for K11.  In float64
it is the REFERENCE, in float32 the plain-fp32 YARDSTICK (what ordinary fp32 arithmetic makes of the same inputs; it shows how well
conditioned a case is, it is not the truth).

`tolerances(case)` are the metrics and bounds of each quantity's existing parity test (K9 value 2e-6 max(1, |v|), K9 gradient 1e-5 of
max |ref|, K11 p 2e-6 absolute, exp_avg_sq 1e-4 of max, the norm 1e-5 relative; K29 takes K9's); exp_avg, which no earlier test
compared, gets 1e-5 of max: it is three fp32 multiply-adds of g * coef, each good to 6e-8, and coef itself (a float square root, an
addition and a division) to 2e-7.  `bounds` widens each to max(existing, 4 x the yardstick's error on that case): two correct fp32
summation orders err independently at the same scale.  Label counts and mask sums are integers below 2^24 and are compared EXACTLY.

PATH PREDICATES are pure functions naming the path a shape or an address takes; each mirrors the source line in its comment, and the
CPU test compares them with the library's host queries wherever one exists.

Plain-fp32 yardstick errors (largest over the group's cases, in the metric of each quantity's tolerance), measured on the host:

    cases                                      quantity and error
    K9 unit HW <= 3073                         ip 1.9e-07  ce 9.9e-08  dlogits 3.5e-07  loss 1.4e-07  dloss 2.4e-07
    K9 spread 30                               ip 8.1e-08  ce 2.9e-08  dlogits 3.0e-07  loss 9.9e-09  dloss 2.5e-07
    K9 shifted +80                             ip 8.3e-08  ce 9.1e-08  dlogits 2.0e-07  loss 7.6e-08  dloss 2.2e-07
    K9 near ties                               ip 1.0e-07  ce 1.6e-08  dlogits 2.1e-07  loss 4.1e-08  dloss 1.8e-07
    K9 unit HW 102405 (303 CE partials)        ip 1.0e-07  ce 2.4e-08  dlogits 2.7e-07
    K9 unit HW 2112899 (2064 partial rows)     ip 5.3e-08  ce 4.2e-08  dlogits 2.6e-07
    K29 unit                                   ip 1.8e-07  bce 1.8e-07  dlogits 3.7e-07
    K29 unit HW 102405 (303 BCE partials)      ip 1.1e-07  bce 6.0e-08  dlogits 2.6e-07
    K29 |z| up to 100                          ip 1.2e-07  bce 7.1e-08  dlogits 1.8e-07
    K11 unit / small                           p 8.3e-07  exp_avg 1.6e-06  exp_avg_sq 1.1e-06  norm 5.1e-07
    K11 one tensor dominates                   p 5.2e-07  exp_avg 4.3e-07  exp_avg_sq 8.9e-07  norm 3.8e-07
    K11 zero gradients                         p 2.5e-07  exp_avg 0.0e+00  exp_avg_sq 0.0e+00  norm 0.0e+00
    K11 norm within 1e-3 of max_norm           p 7.2e-07  exp_avg 6.6e-07  exp_avg_sq 1.2e-06  norm 5.7e-07
    K11 resumed at step 999                    p 7.0e-07  exp_avg 1.0e-07  exp_avg_sq 1.7e-07  norm 3.4e-07
    K11 C ABI, one tensor                      p 2.7e-07  exp_avg 5.2e-08  exp_avg_sq 1.0e-07  norm 6.5e-07

The widened bounds this gives: 2.1e-6 .. 3.3e-6 on p of the K11 cases with non-zero gradients (4 x 5.2e-7 .. 8.3e-7, existing 2e-6: torch's
own fp32 AdamW is that far from float64 after three steps on parameters up to |p| = 5); every K9 and K29 case, and every other K11
quantity, stays on its existing bound.  The CPU test holds every widened bound under twice the existing one and shows that the
defects the cases are meant to catch land at least 10 x outside the bounds in use (the closest: 25 x, the last 5 pixels of 102405).
"""
import collections
import functools
import zlib

import torch

# =====================================================================================================================
# path predicates
# =====================================================================================================================
# ---- K9 (csrc/loss.hip) and K29 (csrc/region_loss.hip): same schedule -------------------------------------------------
LOSS_PIX = 256 * 4                                   # loss.hip:29-30, region_loss.hip:38-39  PPT = 4, TPB = 256: pixels per workgroup
K9_MAXC = 16                                         # loss.hip:28  constexpr int MAXC = 16
K29_MAXR = 16                                        # region_loss.hip:37  constexpr int MAXR = 16
REDUCE_TPB = 256                                     # loss.hip:108, region_loss.hip:134  the single reducer workgroup


def loss_workgroups(HW):
    """Workgroups per sample = partial rows per sample: loss.hip:213 nblk = (HW + TPB * PPT - 1) / (TPB * PPT); region_loss.hip:217."""
    return -(-HW // LOSS_PIX)


def loss_last_workgroup_pixels(HW):
    """Pixels of the last workgroup (loss.hip:57, region_loss.hip:91: if (p >= g.HW) break); LOSS_PIX when it is full."""
    return HW - (loss_workgroups(HW) - 1) * LOSS_PIX


def reduce_rows(nblk):
    """The reducer's pair loop, loss.hip:119-120 / region_loss.hip:145-146: for (; r + 1 < nblk; r += 2) two rows, then
    if (r < nblk) one more: "one" (no pair), "even" (pairs only), "odd" (pairs and a last row)."""
    if nblk == 1:
        return "one"
    return "odd" if nblk % 2 else "even"


def ce_trips(B, nblk):
    """Trips of the busiest thread over the scalar partials, loss.hip:127 / region_loss.hip:153: for (i = threadIdx.x; i < B * nblk; i += 256)."""
    return -(-(B * nblk) // REDUCE_TPB)


def k9_workspace_floats(B, C, HW):
    return B * loss_workgroups(HW) * (3 * C + 1)     # loss.hip:203: one row [I(C) | P(C) | G(C) | ce] per workgroup


def k9_ce_writer(C):
    return 3 * C                                     # loss.hip:103: if (threadIdx.x == 3 * C) row[3 * C] = ...


def k29_workspace_floats(B, R, HW):
    return B * loss_workgroups(HW) * (3 * R + 2)     # region_loss.hip:240: one row [I(R) | P(R) | G(R) | bce | m] per workgroup


def k29_rb(R):
    """region_loss.hip:253-255 and :274-276: if (R <= 4) <.., 4>; else if (R <= 8) <.., 8>; else <.., 16>."""
    return 4 if R <= 4 else 8 if R <= 8 else 16


# ---- K11 (csrc/optimizer.hip) ---------------------------------------------------------------------------------------
K11_CHUNK = 65536                                    # optimizer.hip:25  constexpr int CHUNK = 65536


def k11_chunks(n):
    return -(-n // K11_CHUNK)                        # trainer.py ClipAdamW.step: range((n + chunk - 1) // chunk); optimizer.hip:42, :110


def k11_last_chunk(n):
    """(n4, tail) of a tensor's last chunk on the vector path: optimizer.hip:47, :122 n4 = n >> 2; :52, :134 the tail from 4 * n4."""
    last = n - (k11_chunks(n) - 1) * K11_CHUNK
    return last >> 2, last & 3


def k11_sumsq_path(g):
    return "vector" if g % 16 == 0 else "scalar"     # optimizer.hip:46  if ((((uintptr_t)g) & 15) == 0)


def k11_update_path(p, g, m, v):
    return "vector" if (p | g | m | v) % 16 == 0 else "scalar"       # optimizer.hip:121-122  al = ((p | g | m | v) & 15) == 0


def k11_grad_offsets(sizes):
    """Element offset of every gradient in the flat buffer: trainer.py BucketedGradSync._close, flat[off:off + p.numel()]."""
    out, off = [], 0
    for n in sizes:
        out.append(off)
        off += n
    return out


# =====================================================================================================================
# cases
# =====================================================================================================================
# dims: the spatial extent (2-D or 3-D); ignore: the ignore label or None; regime: unit | sat (spread 30) | shift (+80) | ties (spread
# 1e-3); tweak: "" | sample_ignored | class_absent_sample | class_absent_batch | slice (the logits are a slice of a wider tensor);
# loss: also compared through trainer.deep_supervision_loss with both batch_dice values
K9Case = collections.namedtuple("K9Case", "B C dims ignore regime tweak loss")
# labels 0 .. R, head r is the region of the labels above r; ignore: label R + 1 (label map) / a last plane (planes) marks 20 % of the
# pixels; form: labels | planes; regime: unit | big (a quarter of the logits uniform in [-100, 100])
K29Case = collections.namedtuple("K29Case", "B R dims ignore form regime")
# the parameter list is (lead,) + K11_SIZES (lead 0: K11_SIZES alone); regime: unit | small | dominated | zero | near_below | near_above
K11Case = collections.namedtuple("K11Case", "lead regime max_norm resume")
K11AbiCase = collections.namedtuple("K11AbiCase", "n misaligned")              # one tensor, one pointer off by 4 bytes ("none": all aligned)

K9_PIXELS = {1: (1, 1), 63: (7, 9), 255: (3, 5, 17), 256: (16, 16), 257: (257, 1), 1023: (3, 11, 31), 1024: (32, 32), 1025: (25, 41),
             2047: (23, 89), 2049: (3, 683), 3 * 1024 + 1: (7, 439)}
RAGGED = (25, 41)                                    # 1025 pixels: one full workgroup and one pixel
K9_MANY = (5, 20481)                                 # 102405 pixels: 101 partial rows per sample, 303 CE partials at B = 3
K9_LONG = (131, 127, 127)                            # 2112899 pixels, just above 2^21 (a 128^3 patch): 2064 partial rows, the last of 387 pixels
K9_CASES = [K9Case(3, 3, d, None, "unit", "", d == RAGGED or len(d) == 3) for d in K9_PIXELS.values()] + \
    [K9Case(1, 16, d, 16, "unit", "", False) for d in K9_PIXELS.values()] + \
    [K9Case(3, C, RAGGED, None, "unit", "", C != 15) for C in (2, 15, 16)] + \
    [K9Case(3, 3, RAGGED, 3, "unit", "", True), K9Case(3, 16, RAGGED, 16, "unit", "", True),
     K9Case(3, 3, RAGGED, 3, "unit", "sample_ignored", True),
     K9Case(3, 3, RAGGED, None, "unit", "class_absent_sample", False), K9Case(3, 3, RAGGED, None, "unit", "class_absent_batch", True)] + \
    [K9Case(3, 3, RAGGED, None, r, "", True) for r in ("sat", "shift", "ties")] + \
    [K9Case(3, 3, RAGGED, None, "unit", "slice", True)] + \
    [K9Case(3, 3, K9_MANY, None, "unit", "", False), K9Case(1, 2, K9_LONG, None, "unit", "", False)]

K29_HEADS = (1, 4, 5, 8, 9, 16)
K29_PIXELS = {1023: (3, 11, 31), 1024: (32, 32), 4 * 1024 + 3: (4099, 1)}     # 1025 is RAGGED, the size of the head-count cases
K29_FORMS = ("labels", "planes")
K29_CASES = [K29Case(2, R, RAGGED, ign, f, "unit") for R in K29_HEADS for f in K29_FORMS for ign in (False, True)] + \
    [K29Case(2, 5, d, True, f, "unit") for d in K29_PIXELS.values() for f in K29_FORMS] + \
    [K29Case(3, 5, K9_MANY, True, f, "unit") for f in K29_FORMS] + \
    [K29Case(2, R, RAGGED, ign, f, "big") for R, ign in ((5, True), (16, False)) for f in K29_FORMS]

K11_SIZES = (1, 2, 3, 4, 5, 7, 65535, 65536, 65537, 65539, 131072, 131073)
K11_LEADS = (0, 1, 2, 3)                              # between them every size is met aligned and misaligned (the CPU test shows it)
K11_MAX_NORMS = (12.0, 0.05, 0.0)
K11_LR, K11_BETAS, K11_EPS, K11_WD, K11_STEPS = 5e-4, (0.9, 0.999), 1e-4, 3e-5, 3
K11_RESUME_STEP = 999
K11_NEAR = 5e-4                                      # near_below / near_above: the norm is max_norm (1 -/+ this)
K11_CASES = [K11Case(lead, "unit", mn, False) for lead in K11_LEADS for mn in K11_MAX_NORMS] + \
    [K11Case(0, "small", 12.0, False)] + \
    [K11Case(0, "dominated", mn, False) for mn in (12.0, 0.05)] + \
    [K11Case(0, "zero", mn, False) for mn in K11_MAX_NORMS] + \
    [K11Case(2, r, mn, False) for r in ("near_below", "near_above") for mn in (12.0, 0.05)] + \
    [K11Case(3, "unit", mn, True) for mn in (0.05, 0.0)]
K11_ABI_STEP0, K11_ABI_MAX_NORM = 2, 12.0
K11_ABI_CASES = [K11AbiCase(n, w) for n in (5, 65537) for w in ("none", "p", "g", "m", "v")]

CASES = {"k9": K9_CASES, "k29": K29_CASES, "k11": K11_CASES, "k11abi": K11_ABI_CASES}


def family(case):
    return type(case).__name__[:-4].lower()


def case_id(case):
    def one(v):
        if isinstance(v, tuple):
            return "x".join(str(i) for i in v)
        if isinstance(v, bool):
            return "T" if v else "F"
        return str(v) if v != "" else "-"
    return "-".join(one(v) for v in case)


def hw_of(case):
    n = 1
    for v in case.dims:
        n *= v
    return n


def k11_sizes(case):
    if family(case) == "k11abi":
        return (case.n,)
    return ((case.lead,) if case.lead else ()) + K11_SIZES


def group(case):
    """The row of the docstring's table that a case belongs to."""
    fam = family(case)
    if fam == "k9":
        if case.regime != "unit":
            return {"sat": "K9 spread 30", "shift": "K9 shifted +80", "ties": "K9 near ties"}[case.regime]
        hw = hw_of(case)
        if hw <= 3 * 1024 + 1:
            return "K9 unit HW <= 3073"
        return f"K9 unit HW {hw} ({'303 CE partials' if case.dims == K9_MANY else '2064 partial rows'})"
    if fam == "k29":
        if case.regime == "big":
            return "K29 |z| up to 100"
        return "K29 unit HW 102405 (303 BCE partials)" if case.dims == K9_MANY else "K29 unit"
    if fam == "k11abi":
        return "K11 C ABI, one tensor"
    if case.resume:
        return "K11 resumed at step 999"
    return {"unit": "K11 unit / small", "small": "K11 unit / small", "dominated": "K11 one tensor dominates", "zero": "K11 zero gradients",
            "near_below": "K11 norm within 1e-3 of max_norm", "near_above": "K11 norm within 1e-3 of max_norm"}[case.regime]


# =====================================================================================================================
# inputs: float32 host tensors by name
# =====================================================================================================================
def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(case)).encode()))


def k29_regions(R):
    """The label manager's regions of a K29 case: head r holds the labels r + 1 .. R (nested, as whole tumour > core > enhancing)."""
    return [tuple(range(r + 1, R + 1)) for r in range(R)]


def inputs(case):
    g = _gen(case)
    rn = lambda *s: torch.randn(*s, generator=g)                                                      # noqa: E731
    fam = family(case)
    if fam == "k9":
        B, C = case.B, case.C
        z = rn(B, C, *case.dims) * {"unit": 1.0, "sat": 30.0, "shift": 1.0, "ties": 1e-3}[case.regime]
        if case.regime == "shift":
            z = z + 80.0
        y = torch.randint(0, C, (B, 1) + tuple(case.dims), generator=g).float()
        if case.tweak == "class_absent_sample":
            y[0][y[0] == 1] = 0.0
        if case.tweak == "class_absent_batch":
            y[y == C - 1] = 0.0
        if case.ignore is not None:
            y[torch.rand(y.shape, generator=g) < 0.25] = float(case.ignore)
        if case.tweak == "sample_ignored":
            y[B - 1] = float(case.ignore)
        return dict(logits=z, target=y, g_ip=rn(B, 2, C), g_ce=rn(1))
    if fam == "k29":
        B, R = case.B, case.R
        z = rn(B, R, *case.dims) * 2.0
        if case.regime == "big":
            wide = torch.rand(z.shape, generator=g) * 200.0 - 100.0
            z = torch.where(torch.rand(z.shape, generator=g) < 0.25, wide, z)
        seg = torch.randint(0, R + 1, (B, 1) + tuple(case.dims), generator=g).float()
        if case.ignore:
            seg[torch.rand(seg.shape, generator=g) < 0.2] = float(R + 1)
        return dict(logits=z, seg=seg, g_ip=rn(B, 2, R), g_sums=rn(2))
    if fam == "k11":
        sizes = k11_sizes(case)
        params = [rn(n) for n in sizes]
        grads = []
        for _ in range(K11_STEPS):
            gs = [rn(n) for n in sizes]
            if case.regime == "small":
                gs = [a * 0.01 for a in gs]
            elif case.regime == "dominated":
                gs = [a * (1e4 if n == 65537 else 1e-4) for a, n in zip(gs, sizes)]
            elif case.regime == "zero":
                gs = [torch.zeros(n) for n in sizes]
            elif case.regime in ("near_below", "near_above"):
                total = float(torch.sqrt(sum((a.double() ** 2).sum() for a in gs)))
                want = case.max_norm * (1.0 - K11_NEAR if case.regime == "near_below" else 1.0 + K11_NEAR)
                gs = [(a.double() * (want / total)).float() for a in gs]
            grads.append(gs)
        t = dict(params=params, grads=grads)
        if case.resume:
            t["state0"] = [(K11_RESUME_STEP, rn(n) * 0.1, torch.rand(n, generator=g) * 0.01 + 1e-4) for n in sizes]
        return t
    if fam == "k11abi":
        n = case.n
        return dict(params=[rn(n)], grads=[[rn(n)]], state0=[(K11_ABI_STEP0, rn(n) * 0.1, torch.rand(n, generator=g) * 0.01 + 1e-4)])
    raise ValueError(fam)


def k29_targets(case, seg):
    """(t (B, R, HW) bool: plane r is `label in region r`, m (B, HW) bool: the loss mask) of the label map `seg` (B, 1, ...)."""
    s = seg.flatten(1)
    t = torch.stack([(s > r) & (s <= case.R) for r in range(case.R)], 1)
    m = s != case.R + 1 if case.ignore else torch.ones_like(s, dtype=torch.bool)
    return t, m


def k29_planes(case, seg):
    """The float region planes (B, R, ...) -- (B, R + 1, ...) with the ignore plane last -- that the planes form feeds the kernel."""
    t, m = k29_targets(case, seg)
    planes = torch.cat([t, ~m.unsqueeze(1)], 1) if case.ignore else t
    return planes.float().reshape((case.B, planes.shape[1]) + tuple(case.dims))


# =====================================================================================================================
# the operations as plain torch formulas
# =====================================================================================================================
def k9_stats(z, y, C, ignore, keep=None):
    """(ip (B, 2, C), gt (B, C), ce (1,)) of logits z (B, C, HW) and labels y (B, HW) long; keep (B, HW) bool: only these pixels."""
    lsm = torch.log_softmax(z, 1)
    p = lsm.exp()
    valid = torch.ones_like(y, dtype=torch.bool) if ignore is None else y != ignore
    if keep is not None:
        valid = valid & keep
    onehot = ((y.unsqueeze(1) == torch.arange(C).view(1, C, 1)) & valid.unsqueeze(1)).to(z.dtype)
    ip = torch.stack([(p * onehot).sum(2), (p * valid.unsqueeze(1).to(z.dtype)).sum(2)], 1)
    return ip, onehot.sum(2), -(lsm * onehot).sum().reshape(1)


def k9_loss(ip, gt, ce, npix, batch_dice, ignore, smooth=1e-5):
    """DC_and_CE_loss of one level from its statistics: soft Dice without the background class, cross-entropy mean over the valid pixels."""
    inter, pred, gts = ip[:, 0, 1:], ip[:, 1, 1:], gt[:, 1:]
    if batch_dice:
        inter, pred, gts = inter.sum(0), pred.sum(0), gts.sum(0)
    dc = (2 * inter + smooth) / torch.clip(gts + pred + smooth, 1e-8)
    n = npix if ignore is None else gt.sum().clamp(min=1.0)
    return ce[0] / n - dc.mean()


def k9_evaluate(case, dtype, keep=None, g_ip_of_sample_0=False):
    t = inputs(case)
    z = t["logits"].to(dtype).flatten(2).requires_grad_(True)
    y = t["target"].flatten(1).long()
    ip, gt, ce = k9_stats(z, y, case.C, case.ignore, keep)
    g_ip = t["g_ip"].to(dtype)
    if g_ip_of_sample_0:
        g_ip = g_ip[:1].expand_as(g_ip)
    dz, = torch.autograd.grad((ip, ce), z, (g_ip, t["g_ce"].to(dtype)), retain_graph=case.loss)
    res = dict(ip=ip.detach(), gt=gt, ce=ce.detach(), dlogits=dz.reshape(t["logits"].shape))
    if case.loss:
        for bd in (1, 0):
            loss = k9_loss(ip, gt, ce, case.B * hw_of(case), bool(bd), case.ignore)
            dl, = torch.autograd.grad(loss, z, retain_graph=True)
            res[f"loss_bd{bd}"], res[f"dloss_bd{bd}"] = loss.detach().reshape(1), dl.reshape(t["logits"].shape)
    return res


def k29_stats(z, t, m, live=None):
    """(ip (B, 2, R), gt (B, R), bce (1,), mask (1,)) of logits z (B, R, HW), targets t (B, R, HW) and mask m (B, HW), all of z's type;
    live (1, R, 1): only the heads where it is 1 take part."""
    s = torch.sigmoid(z)
    softplus = z.clamp(min=0) + torch.log1p(torch.exp(-z.abs()))
    mm = m.unsqueeze(1) if live is None else m.unsqueeze(1) * live
    ip = torch.stack([(mm * s * t).sum(2), (mm * s).sum(2)], 1)
    return ip, (mm * t).sum(2), (mm * (softplus - z * t)).sum().reshape(1), m.sum().reshape(1)


def k29_evaluate(case, dtype, heads=None):
    """heads: only the first `heads` heads take part (the rest give zero statistics and no gradient)."""
    inp = inputs(case)
    z = inp["logits"].to(dtype).flatten(2).requires_grad_(True)
    t, m = k29_targets(case, inp["seg"])
    live = None if heads is None else (torch.arange(case.R) < heads).to(dtype).view(1, -1, 1)
    ip, gt, bce, mask = k29_stats(z, t.to(dtype), m.to(dtype), live)
    dz, = torch.autograd.grad((ip, bce), z, (inp["g_ip"].to(dtype), inp["g_sums"][:1].to(dtype)))
    return dict(ip=ip.detach(), gt=gt, bce=bce.detach(), mask=mask, dlogits=dz.reshape(inp["logits"].shape))


def k11_run(params, grads, max_norm, dtype, state0=None):
    """clip_grad_norm_(max_norm) + torch.optim.AdamW.step() per entry of `grads`, on copies of `params` in `dtype`."""
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in params]
    opt = torch.optim.AdamW(ps, lr=K11_LR, betas=K11_BETAS, eps=K11_EPS, weight_decay=K11_WD, foreach=False)
    if state0 is not None:
        for p, (step, m, v) in zip(ps, state0):
            opt.state[p] = dict(step=torch.tensor(float(step)), exp_avg=m.to(dtype).clone(), exp_avg_sq=v.to(dtype).clone())
    norms = []
    for gs in grads:
        for p, a in zip(ps, gs):
            p.grad = a.to(dtype).clone()
        if max_norm > 0:
            norms.append(torch.nn.utils.clip_grad_norm_(ps, max_norm).detach().to(dtype).reshape(1))
        opt.step()
    res = dict(p=[p.detach() for p in ps], exp_avg=[opt.state[p]["exp_avg"] for p in ps], exp_avg_sq=[opt.state[p]["exp_avg_sq"] for p in ps])
    if max_norm > 0:
        res["norm"] = norms
    return res


def evaluate(case, dtype=torch.float64):
    """{quantity: tensor (K11: list of tensors) of `dtype`}, on the host."""
    fam = family(case)
    if fam == "k9":
        return k9_evaluate(case, dtype)
    if fam == "k29":
        return k29_evaluate(case, dtype)
    t = inputs(case)
    return k11_run(t["params"], t["grads"], case.max_norm if fam == "k11" else K11_ABI_MAX_NORM, dtype, t.get("state0"))


@functools.lru_cache(maxsize=4)
def reference_and_yardstick(case):
    """(float64 reference, plain-fp32 yardstick) of a case; computed once, never modified."""
    return evaluate(case, torch.float64), evaluate(case, torch.float32)


# =====================================================================================================================
# tolerances
# =====================================================================================================================
# ("value", a): |got - ref| <= a * max(1, |ref|) element-wise;   ("max", a): max |got - ref| <= a * max |ref|;
# ("abs", a):   max |got - ref| <= a;                             ("exact", 0): got == ref.   K11: per tensor, the worst counts.
Tol = collections.namedtuple("Tol", "kind a")
INF = float("inf")


def tolerances(case):
    """{quantity: Tol}: the metric and bound of the quantity's existing parity test (named in the comments)."""
    fam = family(case)
    if fam == "k9":                                   # test_fused_dice_ce_loss_matches_eager: value 2e-6 max(1, |v|), gradient 1e-5 of max
        return dict(ip=Tol("value", 2e-6), gt=Tol("exact", 0.0), ce=Tol("value", 2e-6), dlogits=Tol("max", 1e-5),
                    loss_bd1=Tol("value", 2e-6), loss_bd0=Tol("value", 2e-6), dloss_bd1=Tol("max", 1e-5), dloss_bd0=Tol("max", 1e-5))
    if fam == "k29":                                  # test_region_loss_head_counts for the value; K9's relative metric for the gradient
        return dict(ip=Tol("value", 2e-6), gt=Tol("exact", 0.0), bce=Tol("value", 2e-6), mask=Tol("exact", 0.0), dlogits=Tol("max", 1e-5))
    # test_clip_adamw_matches_torch: p 2e-6 absolute, exp_avg_sq 1e-4 of max, the norm 1e-5 relative; exp_avg: see the docstring
    return dict(p=Tol("abs", 2e-6), exp_avg=Tol("max", 1e-5), exp_avg_sq=Tol("max", 1e-4), norm=Tol("max", 1e-5))


def _error_one(got, ref, kind):
    ref = ref.double()
    d = (got.detach().cpu().double() - ref).abs()
    if d.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(d).all()):
        return INF
    if kind == "value":
        return float((d / ref.abs().clamp(min=1.0)).max())
    if kind == "max":
        top, worst = float(ref.abs().max()), float(d.max())
        return worst / top if top > 0.0 else (0.0 if worst == 0.0 else INF)
    return float(d.max())


def error(got, ref, tol):
    """The error of `got` in the metric of `tol`: it passes when error <= tol.a (a NaN anywhere gives inf)."""
    if isinstance(ref, (list, tuple)):
        assert len(got) == len(ref)
        return max(_error_one(a, b, tol.kind) for a, b in zip(got, ref))
    return _error_one(got, ref, tol.kind)


def bounds(case, ref, yard):
    """{quantity: Tol} of the device test: `tolerances`, each widened to 4 x the yardstick's error on this case where that is more
    (from the host yardstick, never from the kernel's output); exact quantities stay exact."""
    out = {}
    for q in ref:
        tol = tolerances(case)[q]
        if tol.kind != "exact":
            tol = tol._replace(a=max(tol.a, 4.0 * error(yard[q], ref[q], tol)))
        out[q] = tol
    return out
