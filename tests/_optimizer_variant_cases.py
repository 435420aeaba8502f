"""Cases, references and a host model for K34 (csrc/optimizer.hip: clip + SGD-Nesterov / AdamW-amsgrad / Adam-L2; trainer.ClipSGD,
trainer.ClipAdam): shared by tests/test_optimizer_variants_cpu.py and tests/test_optimizer_variants_gpu.py.

A CASE is an OptCase or an OptAbiCase; its inputs come from a generator seeded with the case itself.  `evaluate(case, dtype)` is
clip_grad_norm_ + the torch optimizer of the kind (torch.optim.SGD / AdamW(amsgrad=True) / Adam, foreach=False) on copies of the
parameters, three steps, and never calls the code under test: in float64 the REFERENCE, in float32 the plain-fp32 YARDSTICK.  The
sizes, the lead elements, the offsets inside one flat gradient buffer and the path predicates are K11's (tests/_step_tail_cases.py):
K34 keeps K11's 64 Ki-element chunks and its float4 / scalar paths.  Hyper-parameters are the reference's: SGD 1e-2 / momentum 0.99 /
weight decay 3e-5 (nnUNetTrainer.py:146-149, :448-452); Adam 1e-2, torch's betas and eps 1e-8, weight decay 3e-5 (nnUNetTrainerAdam.py).

Regimes: unit | dominated (one tensor 1e8 x the others) | zero (all-zero gradients: only the weight decay moves anything) | near_below /
near_above (the gradient norm is max_norm (1 -/+ 5e-4)) | resumed (a loaded state; the Adam kinds at step 999, amsgrad with
max_exp_avg_sq well above exp_avg_sq) | falling (amsgrad only: the gradients of steps 2 and 3 are 1e-4 x those of step 1, so exp_avg_sq
falls and max_exp_avg_sq keeps the value of step 1 -- a kernel that ignores it passes every other fresh-state case).

`bounds`: every quantity against the float64 reference in the metric of K11's existing floors -- p 2e-6 absolute, first-moment-like
tensors (momentum_buffer, exp_avg) 1e-5 of max, second-moment-like tensors (exp_avg_sq, max_exp_avg_sq) 1e-4 of max, the norm 1e-5
relative -- each widened to 4 x the yardstick's error on that case where that is more (_step_tail_cases.bounds' margin: two correct
fp32 evaluation orders err independently at the same scale), from the host yardstick, never from the kernel's output.

`model(case, defect)` restates the kernel's arithmetic in fp32 torch ops on the host; with a defect seeded it shows what the cases
catch (tests/test_optimizer_variants_cpu.py: each lands at least 10 x outside the bounds on at least one case).

Plain-fp32 yardstick errors (largest over the group's cases, in the metric of each quantity's floor), measured on the host:

    cases                          p        state 0  exp_avg_sq  max_exp_avg_sq  norm
    sgd unit                       5.6e-07  1.6e-06                              5.8e-07
    sgd one tensor dominates       4.9e-07  3.5e-07                              3.5e-07
    sgd zero gradients             3.4e-07  1.3e-07                              0.0e+00
    sgd norm near max_norm         5.7e-07  6.9e-07                              5.9e-07
    sgd resumed                    4.2e-07  1.7e-07                              2.9e-07
    sgd C ABI, one tensor          2.4e-07  2.6e-07                              5.1e-07
    adamw_ams unit                 1.2e-06  2.0e-06  1.1e-06     1.1e-06         4.6e-07
    adamw_ams one tensor dominates 1.0e-06  7.1e-07  1.3e-06     1.3e-06         6.4e-07
    adamw_ams zero gradients       6.9e-07  0.0e+00  0.0e+00     0.0e+00         0.0e+00
    adamw_ams norm near max_norm   1.2e-06  5.5e-07  1.1e-06     1.1e-06         7.4e-07
    adamw_ams resumed at step 999  1.1e-06  1.1e-07  1.8e-07     1.2e-07         4.1e-07
    adamw_ams falling moment       1.1e-06  3.8e-07  8.3e-07     7.8e-07         3.3e-07
    adamw_ams C ABI, one tensor    4.4e-07  6.4e-08  1.0e-07     8.1e-09         6.7e-07
    adam_l2 unit                   3.1e-05  2.8e-06  1.6e-06                     5.8e-07
    adam_l2 one tensor dominates   1.6e-06  2.9e-07  6.6e-07                     4.8e-07
    adam_l2 zero gradients         4.5e-07  1.1e-07  1.4e-07                     0.0e+00
    adam_l2 norm near max_norm     4.3e-05  3.9e-06  3.5e-06                     6.7e-07
    adam_l2 resumed at step 999    5.2e-07  1.2e-07  1.9e-07                     4.4e-07
    adam_l2 C ABI, one tensor      2.1e-07  5.9e-08  1.0e-07                     2.2e-07

The widened bounds this gives on p: 2.0e-6 .. 2.3e-6 for SGD, up to 4.8e-6 for AdamW-amsgrad (torch's own fp32 Adam is 1.2e-6 from float64
after three steps of 1e-2 on parameters up to |p| = 5), and 4e-5 .. 1.7e-4 for the Adam-L2 cases whose gradients are clipped to a norm
of 0.05 (elsewhere 2.1e-6 .. 7.9e-6): there coef g and wd p have the same size, g + wd p crosses zero in some elements, the step
lr m / (sqrt(v) + 1e-8) is steep in them, and clip_grad_norm_'s fp32 norm is 6e-7 off.  Every other quantity stays on its floor.
"""
import collections
import functools
import zlib

import torch

from tests import _step_tail_cases as K
from tests._step_tail_cases import Tol, error                                   # noqa: F401  (re-exported for the tests)

KINDS = ("sgd", "adamw_ams", "adam_l2")
ABI_KIND = {"sgd": "MLAGG_OPT_SGD_NESTEROV", "adamw_ams": "MLAGG_OPT_ADAMW_AMSGRAD", "adam_l2": "MLAGG_OPT_ADAM_L2"}
# the state tensors of a kind by torch's keys, in the order of the kernel's table (columns 2 and 3, then the extra pointer)
STATE = {"sgd": ("momentum_buffer",), "adamw_ams": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"), "adam_l2": ("exp_avg", "exp_avg_sq")}
SIZES, LEADS, MAX_NORMS, STEPS, NEAR = K.K11_SIZES, K.K11_LEADS, K.K11_MAX_NORMS, K.K11_STEPS, K.K11_NEAR
assert SIZES == (1, 2, 3, 4, 5, 7, 65535, 65536, 65537, 65539, 131072, 131073) and LEADS == (0, 1, 2, 3)
assert MAX_NORMS == (12.0, 0.05, 0.0) and STEPS == 3 and NEAR == 5e-4
SGD_LR, SGD_MOMENTUM, WD = 1e-2, 0.99, 3e-5
ADAM_LR, ADAM_BETAS, ADAM_EPS = 1e-2, (0.9, 0.999), 1e-8
RESUME_STEP = 999
FALL = 1e-4                                          # falling: the gradients of steps 2, 3 are this x those of step 1

OptCase = collections.namedtuple("OptCase", "kind lead regime max_norm")
OptAbiCase = collections.namedtuple("OptAbiCase", "kind n misaligned")          # one tensor, one pointer off by 4 bytes ("none": all aligned)


def _cases(kind):
    out = [OptCase(kind, lead, "unit", mn) for lead in LEADS for mn in MAX_NORMS] + \
        [OptCase(kind, 0, "dominated", mn) for mn in (12.0, 0.05)] + \
        [OptCase(kind, 0, "zero", mn) for mn in MAX_NORMS] + \
        [OptCase(kind, 2, r, mn) for r in ("near_below", "near_above") for mn in (12.0, 0.05)] + \
        [OptCase(kind, 3, "resumed", mn) for mn in (0.05, 0.0)]
    if kind == "adamw_ams":
        out += [OptCase(kind, 1, "falling", mn) for mn in (12.0, 0.0)]
    return out


CASES = [c for kind in KINDS for c in _cases(kind)]
ABI_STEP0, ABI_MAX_NORM = 2, 12.0
ABI_POINTERS = {"sgd": "pgm", "adamw_ams": "pgmvx", "adam_l2": "pgmv"}          # m: state 0, v: exp_avg_sq, x: max_exp_avg_sq
ABI_CASES = [OptAbiCase(kind, n, w) for kind in KINDS for n in (5, 65537) for w in ("none",) + tuple(ABI_POINTERS[kind])]


def is_abi(case):
    return isinstance(case, OptAbiCase)


def case_id(case):
    return "-".join(str(v) for v in case)


def sizes_of(case):
    if is_abi(case):
        return (case.n,)
    return ((case.lead,) if case.lead else ()) + SIZES


def max_norm_of(case):
    return ABI_MAX_NORM if is_abi(case) else case.max_norm


def group(case):
    """The row of the docstring's table that a case belongs to."""
    if is_abi(case):
        return f"{case.kind} C ABI, one tensor"
    name = {"unit": "unit", "dominated": "one tensor dominates", "zero": "zero gradients", "near_below": "norm near max_norm",
            "near_above": "norm near max_norm", "falling": "falling moment",
            "resumed": "resumed" if case.kind == "sgd" else "resumed at step 999"}[case.regime]
    return f"{case.kind} {name}"


# =====================================================================================================================
# inputs: float32 host tensors
# =====================================================================================================================
def inputs(case):
    """dict(params=[...], grads=[[...] per step], state0=None | [(step, state tensors in STATE order) per parameter])."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(tuple(case)).encode()))
    rn = lambda *s: torch.randn(*s, generator=g)                                                      # noqa: E731
    sizes = sizes_of(case)
    regime = "resumed" if is_abi(case) else case.regime
    params = [rn(n) for n in sizes]
    grads = []
    for step in range(1 if is_abi(case) else STEPS):
        gs = [rn(n) for n in sizes]
        if regime == "dominated":
            gs = [a * (1e4 if n == 65537 else 1e-4) for a, n in zip(gs, sizes)]
        elif regime == "zero":
            gs = [torch.zeros(n) for n in sizes]
        elif regime in ("near_below", "near_above"):
            total = float(torch.sqrt(sum((a.double() ** 2).sum() for a in gs)))
            want = case.max_norm * (1.0 - NEAR if regime == "near_below" else 1.0 + NEAR)
            gs = [(a.double() * (want / total)).float() for a in gs]
        elif regime == "falling" and step > 0:
            gs = [a * FALL for a in gs]
        grads.append(gs)
    state0 = None
    if regime == "resumed":
        state0 = []
        for n in sizes:
            first = rn(n) * 0.1
            second = torch.rand(n, generator=g) * 0.01 + 1e-4
            third = second + torch.rand(n, generator=g) * 0.03                  # max_exp_avg_sq well above exp_avg_sq
            state0.append((ABI_STEP0 if is_abi(case) else RESUME_STEP, (first, second, third)[:len(STATE[case.kind])]))
    return dict(params=params, grads=grads, state0=state0)


# =====================================================================================================================
# reference / yardstick: the torch optimizers
# =====================================================================================================================
def torch_optimizer(kind, ps):
    if kind == "sgd":
        return torch.optim.SGD(ps, lr=SGD_LR, momentum=SGD_MOMENTUM, weight_decay=WD, nesterov=True, foreach=False)
    if kind == "adamw_ams":
        return torch.optim.AdamW(ps, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=WD, amsgrad=True, foreach=False)
    return torch.optim.Adam(ps, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=WD, foreach=False)


def torch_state(kind, step, tensors, dtype=None, device=None):
    """One parameter's state as the torch optimizer of `kind` keeps it."""
    st = {} if kind == "sgd" else {"step": torch.tensor(float(step))}
    for k, t in zip(STATE[kind], tensors):
        st[k] = t.to(dtype=dtype, device=device).clone()
    return st


def evaluate(case, dtype=torch.float64):
    """{quantity: list of tensors of `dtype`}: p, every state tensor by torch's key, and (with clipping) the norm of every step."""
    t = inputs(case)
    kind, max_norm = case.kind, max_norm_of(case)
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in t["params"]]
    opt = torch_optimizer(kind, ps)
    if t["state0"] is not None:
        for p, (step, tensors) in zip(ps, t["state0"]):
            opt.state[p] = torch_state(kind, step, tensors, dtype)
    norms = []
    for gs in t["grads"]:
        for p, a in zip(ps, gs):
            p.grad = a.to(dtype).clone()
        if max_norm > 0:
            norms.append(torch.nn.utils.clip_grad_norm_(ps, max_norm).detach().to(dtype).reshape(1))
        opt.step()
    res = dict(p=[p.detach() for p in ps])
    for k in STATE[kind]:
        res[k] = [opt.state[p][k] for p in ps]
    if max_norm > 0:
        res["norm"] = norms
    return res


@functools.lru_cache(maxsize=4)
def reference_and_yardstick(case):
    """(float64 reference, plain-fp32 yardstick) of a case; computed once, never modified."""
    return evaluate(case, torch.float64), evaluate(case, torch.float32)


# =====================================================================================================================
# tolerances
# =====================================================================================================================
FLOORS = dict(p=Tol("abs", 2e-6), momentum_buffer=Tol("max", 1e-5), exp_avg=Tol("max", 1e-5), exp_avg_sq=Tol("max", 1e-4),
              max_exp_avg_sq=Tol("max", 1e-4), norm=Tol("max", 1e-5))


def bounds(case, ref, yard):
    """{quantity: Tol}: K11's floors, each widened to 4 x the yardstick's error on this case where that is more."""
    return {q: FLOORS[q]._replace(a=max(FLOORS[q].a, 4.0 * error(yard[q], ref[q], FLOORS[q]))) for q in ref}


# =====================================================================================================================
# the kernel's arithmetic as fp32 torch ops, with seedable defects
# =====================================================================================================================
DEFECTS = {"sgd": ("no_nesterov", "wrong_decay", "no_clip", "skip_tail"),
           "adamw_ams": ("wrong_decay", "v_for_vmax", "no_clip", "skip_tail"),
           "adam_l2": ("wrong_decay", "no_clip", "skip_tail")}


def model(case, defect=None):
    """What csrc/optimizer.hip computes, restated on the host in float32 (the norm from a float64 sum of squares, the coefficient and
    the bias corrections as the kernel forms them).  defect: None, or one of DEFECTS[kind] --
      no_nesterov  p -= lr buf                       wrong_decay  decoupled where the kind has L2, L2 where it has decoupled
      v_for_vmax   max_exp_avg_sq = exp_avg_sq       no_clip      the coefficient is 1
      skip_tail    the last n & 3 elements of every tensor are left as they were."""
    t = inputs(case)
    kind, max_norm = case.kind, max_norm_of(case)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)                                             # noqa: E731
    ps = [p.clone() for p in t["params"]]
    step0 = 0
    if t["state0"] is None:
        state = [[torch.zeros_like(p) for _ in STATE[kind]] for p in ps]
    else:
        step0 = t["state0"][0][0]
        state = [[s.clone() for s in tensors] for _, tensors in t["state0"]]
    lr, wd = f32(SGD_LR if kind == "sgd" else ADAM_LR), f32(WD)
    b1, b2, eps, mu = f32(ADAM_BETAS[0]), f32(ADAM_BETAS[1]), f32(ADAM_EPS), f32(SGD_MOMENTUM)
    l2 = (kind != "adamw_ams") != (defect == "wrong_decay")
    norms = []
    for k, gs in enumerate(t["grads"]):
        coef = f32(1.0)
        if max_norm > 0:
            norm = torch.sqrt(sum((a.double() ** 2).sum() for a in gs)).float()
            norms.append(norm.reshape(1))
            if defect != "no_clip":
                coef = torch.minimum(f32(max_norm) / (norm + f32(1e-6)), f32(1.0))
        step = step0 + k + 1
        c1 = f32(1.0 - ADAM_BETAS[0] ** step)
        c2 = f32((1.0 - ADAM_BETAS[1] ** step) ** 0.5)
        for p, a, st in zip(ps, gs, state):
            live = p.numel() - (p.numel() & 3) if defect == "skip_tail" else p.numel()
            old = [x[live:].clone() for x in [p] + st]
            g = a * coef
            if kind == "sgd":
                if l2:
                    g = g + wd * p
                else:
                    p.mul_(1 - lr * wd)
                st[0].copy_(mu * st[0] + g)
                p.sub_(lr * (st[0] if defect == "no_nesterov" else g + mu * st[0]))
            else:
                if l2:
                    g = g + wd * p
                else:
                    p.mul_(1 - lr * wd)
                st[0].copy_(b1 * st[0] + f32(1.0 - ADAM_BETAS[0]) * g)
                st[1].copy_(b2 * st[1] + f32(1.0 - ADAM_BETAS[1]) * g * g)
                s = st[1]
                if kind == "adamw_ams":
                    st[2].copy_(st[1] if defect == "v_for_vmax" else torch.maximum(st[2], st[1]))
                    s = st[2]
                p.sub_((lr / c1) * (st[0] / (s.sqrt() / c2 + eps)))
            for x, o in zip([p] + st, old):
                x[live:] = o
    res = dict(p=ps)
    for i, key in enumerate(STATE[kind]):
        res[key] = [st[i] for st in state]
    if max_norm > 0:
        res["norm"] = norms
    return res
