"""Cases, a float64 reference and a host model for K35 (csrc/optimizer.hip: fp16 loss scaling fused into the clip + update step;
trainer.DeviceGradScaler): shared by tests/test_loss_scaling_cpu.py and tests/test_loss_scaling_gpu.py.

A CASE is an LSCase or an LSAbiCase; its inputs come from a generator seeded with the case itself.  The inputs are UNSCALED gradients
per step; what the code under test receives are the SCALED gradients `scaled_grads(case)`: float32(g * the scale in force at that
step), with the case's poison (an inf, a NaN) written in afterwards.  The scale in force comes from the reference's own decisions.

`evaluate(case, dtype)` is torch's own composition and never calls the code under test: grad * inv_scale with
inv_scale = scale.double().reciprocal().float() (GradScaler.unscale_), found_inf where a scaled gradient element is not finite,
clip_grad_norm_, the torch optimizer of the kind with foreach=False (skipped on found_inf, as GradScaler.step skips it) and
torch._amp_update_scale_.  In float64 it is the REFERENCE, in float32 the plain-fp32 YARDSTICK.  Sizes, leads, the flat gradient
buffer's offsets and the `bounds` metric are K11's (tests/_step_tail_cases.py; floors p 2e-6 absolute, first moments 1e-5 of max,
second moments 1e-4 of max, the norm 1e-5 relative, each widened to 4 x the yardstick's error on the case, computed on the host,
never from the kernel's output).  The DECISIONS -- after every step the scale, the growth tracker and the count of applied steps --
are compared exactly.

Kinds: adamw (K11's AdamW, its hyper-parameters) | sgd | adamw_ams | adam_l2 (K34's, theirs).  Regimes:
  unit         scale 65536, max_norm 12 / 0.05 / 0 over the four leads
  scale1000    a scale that is no power of two: 1 / scale is rounded, g * scale was rounded
  near_below / near_above   the UNSCALED norm is max_norm (1 -/+ 5e-4), the scaled one 65536 x that: a kernel that clips on the scaled
               norm fails here
  inf_tail     four steps; at step 2 the last element of the 131073-element tensor (its chunk's scalar tail) is inf: that step leaves
               parameters and state bit-identical and uncounted, the scale is halved, the tracker 0; step 3 applies with the bias
               correction of step 2
  nan_head     at step 1 element 0 of a large tensor at a 4-byte-misaligned offset of the flat buffer is NaN
  growth       growth_interval 2 over five steps: the scale doubles after steps 2 and 4
  growth_sat   scale 3e38, growth_interval 1, gradients 1e-3: 2 x 3e38 is not finite, the scale stays and the tracker resets
  zero         all-zero gradients: only the weight decay moves anything

`model(case, defect)` restates the kernels' arithmetic in fp32 torch ops on the host; tests/test_loss_scaling_cpu.py shows that it
stays inside the bounds and that each seeded defect lands outside them.
"""
import collections
import functools
import zlib

import torch

from tests import _optimizer_variant_cases as V
from tests import _step_tail_cases as K
from tests._step_tail_cases import Tol, error                                   # noqa: F401  (re-exported for the tests)

KINDS = ("adamw",) + V.KINDS
ABI_KIND = dict(V.ABI_KIND, adamw="MLAGG_OPT_ADAMW")
STATE = dict(V.STATE, adamw=("exp_avg", "exp_avg_sq"))
SIZES, LEADS, MAX_NORMS, NEAR = K.K11_SIZES, K.K11_LEADS, K.K11_MAX_NORMS, K.K11_NEAR
assert SIZES[-1] == 131073 and LEADS == (0, 1, 2, 3) and MAX_NORMS == (12.0, 0.05, 0.0) and NEAR == 5e-4
GROWTH, BACKOFF = 2.0, 0.5
BIG = 131073

LSCase = collections.namedtuple("LSCase", "kind lead regime max_norm")
LSAbiCase = collections.namedtuple("LSAbiCase", "kind n misaligned")            # one tensor, one pointer off by 4 bytes ("none": all aligned)

# regime -> (initial scale, growth interval, steps)
SETUP = {"unit": (65536.0, 2000, 3), "scale1000": (1000.0, 2000, 3), "near_below": (65536.0, 2000, 3), "near_above": (65536.0, 2000, 3),
         "inf_tail": (65536.0, 2000, 4), "nan_head": (65536.0, 2000, 3), "growth": (65536.0, 2, 5), "growth_sat": (3e38, 1, 3),
         "zero": (65536.0, 2000, 3), "abi": (65536.0, 2000, 1)}


def _cases(kind):
    return [LSCase(kind, lead, "unit", mn) for lead, mn in ((0, 12.0), (1, 0.05), (2, 0.0), (3, 12.0), (0, 0.05), (0, 0.0))] + \
        [LSCase(kind, 1, "scale1000", 12.0)] + \
        [LSCase(kind, 2, r, mn) for r in ("near_below", "near_above") for mn in (12.0, 0.05)] + \
        [LSCase(kind, 0, "inf_tail", 12.0), LSCase(kind, 1, "nan_head", 12.0), LSCase(kind, 3, "growth", 12.0),
         LSCase(kind, 0, "growth_sat", 12.0)] + \
        [LSCase(kind, 0, "zero", mn) for mn in (12.0, 0.0)]


CASES = [c for kind in KINDS for c in _cases(kind)]
ABI_STEP0, ABI_MAX_NORM = 2, 12.0
ABI_POINTERS = dict(V.ABI_POINTERS, adamw="pgmv")
ABI_CASES = [LSAbiCase(kind, n, w) for kind in KINDS for n in (5, 65537) for w in ("none",) + tuple(ABI_POINTERS[kind])]


def is_abi(case):
    return isinstance(case, LSAbiCase)


def case_id(case):
    return "-".join(str(v) for v in case)


def regime_of(case):
    return "abi" if is_abi(case) else case.regime


def sizes_of(case):
    if is_abi(case):
        return (case.n,)
    return ((case.lead,) if case.lead else ()) + SIZES


def max_norm_of(case):
    return ABI_MAX_NORM if is_abi(case) else case.max_norm


def hyper(kind):
    """(lr, beta1 or momentum, beta2, eps, weight decay) of a kind: K11's for adamw, K34's for the others."""
    if kind == "adamw":
        return (K.K11_LR,) + tuple(K.K11_BETAS) + (K.K11_EPS, K.K11_WD)
    if kind == "sgd":
        return V.SGD_LR, V.SGD_MOMENTUM, 0.0, 0.0, V.WD
    return (V.ADAM_LR,) + tuple(V.ADAM_BETAS) + (V.ADAM_EPS, V.WD)


def poison(case):
    """None, or (step index, tensor index, element index, value) of the one non-finite scaled gradient element."""
    if is_abi(case):
        return None
    sizes = sizes_of(case)
    if case.regime == "inf_tail":
        return 1, sizes.index(BIG), BIG - 1, float("inf")
    if case.regime == "nan_head":
        offs = K.k11_grad_offsets(sizes)
        i = next(i for i, (n, off) in enumerate(zip(sizes, offs)) if n >= 65535 and off % 4 != 0)
        return 0, i, 0, float("nan")
    return None


# =====================================================================================================================
# inputs: float32 host tensors
# =====================================================================================================================
def inputs(case):
    """dict(params=[...], grads=[[UNSCALED gradients] per step], state0=None | [(step, state tensors in STATE order) per parameter])."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(tuple(case)).encode()))
    rn = lambda *s: torch.randn(*s, generator=g)                                                      # noqa: E731
    sizes, regime = sizes_of(case), regime_of(case)
    params = [rn(n) for n in sizes]
    grads = []
    for _ in range(SETUP[regime][2]):
        gs = [rn(n) for n in sizes]
        if regime == "zero":
            gs = [torch.zeros(n) for n in sizes]
        elif regime == "growth_sat":
            gs = [a * 1e-3 for a in gs]
        elif regime in ("near_below", "near_above"):
            total = float(torch.sqrt(sum((a.double() ** 2).sum() for a in gs)))
            want = case.max_norm * (1.0 - NEAR if regime == "near_below" else 1.0 + NEAR)
            gs = [(a.double() * (want / total)).float() for a in gs]
        grads.append(gs)
    state0 = None
    if regime == "abi":
        state0 = []
        for n in sizes:
            first, second = rn(n) * 0.1, torch.rand(n, generator=g) * 0.01 + 1e-4
            third = second + torch.rand(n, generator=g) * 0.03
            state0.append((ABI_STEP0, (first, second, third)[:len(STATE[case.kind])]))
    return dict(params=params, grads=grads, state0=state0)


def torch_optimizer(kind, ps):
    if kind == "adamw":
        return torch.optim.AdamW(ps, lr=K.K11_LR, betas=K.K11_BETAS, eps=K.K11_EPS, weight_decay=K.K11_WD, foreach=False)
    return V.torch_optimizer(kind, ps)


def _scaled(gs, scale, case, k):
    """The float32 gradients the code under test sees at step k: float32(g * scale), then the case's poison."""
    out = [(a * scale).float() for a in gs]
    bad = poison(case)
    if bad is not None and bad[0] == k:
        out[bad[1]][bad[2]] = bad[3]
    return out


# =====================================================================================================================
# reference / yardstick: torch's own composition
# =====================================================================================================================
def evaluate(case, dtype=torch.float64):
    """dict of the compared quantities -- p, every state tensor by torch's key, norm (per APPLIED step, with clipping) as lists of
    tensors of `dtype` -- plus, under "decisions", per step (scale before, found_inf, scale after, tracker after, applied steps so far)."""
    t = inputs(case)
    kind, max_norm = case.kind, max_norm_of(case)
    init_scale, interval, _ = SETUP[regime_of(case)]
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in t["params"]]
    opt = torch_optimizer(kind, ps)
    if t["state0"] is not None:
        for p, (step, tensors) in zip(ps, t["state0"]):
            st = V.torch_state("adam_l2" if kind == "adamw" else kind, step, tensors, dtype)
            opt.state[p] = st
    scale, tracker = torch.full((1,), init_scale, dtype=torch.float32), torch.zeros(1, dtype=torch.int32)
    norms, decisions, applied = [], [], 0
    for k, gs in enumerate(t["grads"]):
        before = float(scale)
        sg = _scaled(gs, scale, case, k)
        inv = scale.double().reciprocal().float()                                 # GradScaler._unscale_grads_
        found = torch.zeros(1)
        for p, a in zip(ps, sg):
            if not bool(torch.isfinite(a).all()):
                found.fill_(1.0)
            p.grad = a.to(dtype) * inv.to(dtype)
        if not bool(found):
            if max_norm > 0:
                norms.append(torch.nn.utils.clip_grad_norm_(ps, max_norm).detach().to(dtype).reshape(1))
            opt.step()
            applied += 1
        torch._amp_update_scale_(scale, tracker, found, GROWTH, BACKOFF, interval)
        decisions.append((before, bool(found), float(scale), int(tracker), applied))
    res = dict(p=[p.detach() for p in ps])
    for key in STATE[kind]:
        res[key] = [opt.state[p][key] if opt.state[p] else torch.zeros_like(p.detach()) for p in ps]
    if max_norm > 0:
        res["norm"] = norms
    res["decisions"] = decisions
    return res


@functools.lru_cache(maxsize=4)
def reference_and_yardstick(case):
    """(float64 reference, plain-fp32 yardstick) of a case; computed once, never modified."""
    return evaluate(case, torch.float64), evaluate(case, torch.float32)


def scaled_grads(case):
    """[[float32 scaled gradients] per step], scaled by the scale the REFERENCE has in force at that step."""
    ref, _ = reference_and_yardstick(case)
    return [_scaled(gs, torch.tensor(d[0], dtype=torch.float32), case, k) for k, (gs, d) in enumerate(zip(inputs(case)["grads"], ref["decisions"]))]


# =====================================================================================================================
# tolerances
# =====================================================================================================================
FLOORS = V.FLOORS


def quantities(res):
    return [q for q in res if q != "decisions"]


def bounds(case, ref, yard):
    """{quantity: Tol}: K11's floors, each widened to 4 x the yardstick's error on this case where that is more."""
    return {q: FLOORS[q]._replace(a=max(FLOORS[q].a, 4.0 * error(yard[q], ref[q], FLOORS[q]))) for q in quantities(ref)}


# =====================================================================================================================
# the kernels' arithmetic as fp32 torch ops, with seedable defects
# =====================================================================================================================
DEFECTS = ("norm_of_scaled", "count_on_skip", "write_on_skip", "grow_unguarded", "tracker_kept", "mult_from_new_scale")


def model(case, defect=None):
    """What csrc/optimizer.hip computes in the loss-scaled step, restated on the host in float32.  defect: None or one of DEFECTS --
      norm_of_scaled       the unscale is missing from the norm        count_on_skip   the step counter advances on a skipped step
      write_on_skip        the update runs on a skipped step           grow_unguarded  growth without the finiteness guard
      tracker_kept         the tracker is not reset on backoff         mult_from_new_scale  the multiplier uses the updated scale."""
    t = inputs(case)
    kind, max_norm = case.kind, max_norm_of(case)
    init_scale, interval, _ = SETUP[regime_of(case)]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)                                             # noqa: E731
    lr_, b1_, b2_, eps_, wd_ = hyper(kind)
    lr, wd, eps = f32(lr_), f32(wd_), f32(eps_)
    b1, b2 = f32(b1_), f32(b2_)
    # K11 forms bias corrections and 1 - beta from the FLOAT betas, K34 from the doubles
    cb1, cb2 = (float(b1), float(b2)) if kind == "adamw" else (b1_, b2_)
    omb1, omb2 = (f32(1.0) - b1, f32(1.0) - b2) if kind == "adamw" else (f32(1.0 - b1_), f32(1.0 - b2_))
    ps = [p.clone() for p in t["params"]]
    step = 0
    if t["state0"] is None:
        state = [[torch.zeros_like(p) for _ in STATE[kind]] for p in ps]
    else:
        step = t["state0"][0][0]
        state = [[s.clone() for s in tensors] for _, tensors in t["state0"]]
    step0 = step
    scale, tracker = f32(init_scale), 0
    norms, decisions, applied = [], [], 0
    for k, gs in enumerate(t["grads"]):
        before = float(scale)
        sg = _scaled(gs, scale, case, k)
        inv = (1.0 / scale.double()).float()
        total = sum((((a if defect == "norm_of_scaled" else a * inv).double()) ** 2).sum() for a in sg)
        total = torch.as_tensor(total, dtype=torch.float64)
        # squares are formed in fp32 on the device: beyond fp32 they are inf
        bad = not bool(torch.isfinite(total)) or any(float((a * inv).abs().max()) > 1.8e19 for a in sg if a.numel() and bool(torch.isfinite(a).all()))
        old_scale = scale
        if bad:
            scale = (scale.double() * BACKOFF).float()
            tracker = tracker if defect == "tracker_kept" else 0
            if defect == "count_on_skip":
                step += 1
        else:
            step += 1
            applied += 1
            if tracker + 1 == interval:
                grown = (scale.double() * GROWTH).float()
                if bool(torch.isfinite(grown)) or defect == "grow_unguarded":
                    scale = grown
                tracker = 0
            else:
                tracker += 1
        decisions.append((before, bad, float(scale), tracker, (step - step0) if defect == "count_on_skip" else applied))
        if bad and defect != "write_on_skip":
            continue
        coef = f32(1.0)
        if max_norm > 0:
            norm = total.sqrt().float()
            if not bad:
                norms.append(norm.reshape(1))
            coef = torch.minimum(f32(max_norm) / (norm + f32(1e-6)), f32(1.0)) if bool(torch.isfinite(norm)) else f32(float("nan"))
        minv = (1.0 / scale.double()).float() if defect == "mult_from_new_scale" else (1.0 / old_scale.double()).float()
        mult = minv * coef
        n_step = max(step, 1)
        c1 = f32(1.0 - cb1 ** n_step)
        c2 = f32((1.0 - cb2 ** n_step) ** 0.5)
        for p, a, st in zip(ps, sg, state):
            g = a * mult
            if kind == "sgd":
                g = g + wd * p
                st[0].copy_(b1 * st[0] + g)
                p.sub_(lr * (g + b1 * st[0]))
                continue
            if kind == "adam_l2":
                g = g + wd * p
            else:
                p.mul_(1 - lr * wd)
            st[0].copy_(b1 * st[0] + omb1 * g)
            st[1].copy_(b2 * st[1] + omb2 * g * g)
            s = st[1]
            if kind == "adamw_ams":
                st[2].copy_(torch.maximum(st[2], st[1]))
                s = st[2]
            p.sub_((lr / c1) * (st[0] / (s.sqrt() / c2 + eps)))
    res = dict(p=ps)
    for i, key in enumerate(STATE[kind]):
        res[key] = [st[i] for st in state]
    if max_norm > 0:
        res["norm"] = norms
    res["decisions"] = decisions
    return res
