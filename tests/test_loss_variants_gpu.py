"""K33 on the device (csrc/loss.hip: top-k cross-entropy statistics, radix select, gradient) against a float64 torch reference written
here: explicit log-softmax, stable descending sort, equal share among the values that tie with the k-th, autograd under random
upstream cotangents.  The plain-fp32 run of the same formulas is the yardstick, as in tests/_step_tail_cases.py.

Bounds: K9's -- value 2e-6 max(1, |v|), gradient 1e-5 of max |ref| -- each widened to 4 x the yardstick's error on the case where that
is more.  Counts (n_gt, n_eq) and sum w_p == k are exact.
Pixels near the threshold: a pixel whose float64 cross-entropy lies within 1e-5 max(1, t) of the threshold t may fall on either side
in fp32 (the fp32 cross-entropy is within 1.4e-6 of float64 on such inputs, so the band is 50 x that).  Those pixels are the set A.
If A holds only the threshold pixel itself nothing is excused; otherwise every pixel of A must equal its "selected" or its
"unselected" reference gradient within the bound, counts and the value are then compared within what |A| pixels can move, and
|A| <= 1e-4 N is asserted from the float64 reference alone before the device result is looked at."""
import copy
import functools
import math

import pytest
import torch

import fake_nnunet as FK
import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import _lib, nnunet_plugin, ops, trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPW = 4096                                            # loss.hip SEL_EPW: elements per workgroup of the select kernels (asserted below)
VALUE_TOL, GRAD_TOL, BAND, CAP = 2e-6, 1e-5, 1e-5, 1e-4


class Case:
    def __init__(self, name, shape, C, scale=2.0, eps=0.0, dice=True, ignore=None, ignored=0.0, zeros=False, plant=False, seed=0):
        self.name, self.shape, self.C, self.scale, self.eps, self.dice = name, tuple(shape), C, scale, eps, dice
        self.ignore, self.ignored, self.zeros, self.plant, self.seed = ignore, ignored, zeros, plant, seed

    def __repr__(self):
        return self.name


CASES = [
    Case("c3_37x29", (2, 37, 29), 3, seed=1),
    Case("c2_7x9", (3, 7, 9), 2, seed=2),
    Case("c14_5d", (2, 8, 12, 10), 14, seed=3),
    Case("c5_ragged", (3, 1, 20481), 5, seed=4),                                 # 15 workgroups of the select and a ragged tail
    Case("c2_epw_minus_1", (1, 1, EPW - 1), 2, seed=5),
    Case("c5_epw", (2, 1, EPW // 2), 5, seed=6),
    Case("c16_epw_plus_1", (1, 1, EPW + 1), 16, seed=7),
    Case("c5_no_dice", (2, 37, 29), 5, dice=False, seed=8),
    Case("c5_all_zero", (2, 37, 29), 5, zeros=True, seed=9),
    # 189 values within 1e-2 of log 5: with this seed the k-th value is 1.3e-4 and 2.1e-4 from its neighbours, above the band of 1.6e-5
    Case("c5_times_1e-3", (3, 7, 9), 5, scale=2e-3, seed=19),
    Case("c5_times_30", (2, 37, 29), 5, scale=60.0, seed=11),
    Case("c5_mostly_ignored", (2, 37, 29), 5, ignore=5, ignored=0.93, seed=12),
    Case("c6_some_ignored", (2, 37, 29), 6, ignore=5, ignored=0.2, seed=13),
    Case("c5_planted_ties", (2, 37, 29), 5, plant=True, seed=14),
    Case("c5_ls01", (2, 37, 29), 5, eps=0.1, seed=15),
    Case("c5_ls01_no_dice_ignored", (2, 37, 29), 5, eps=0.1, dice=False, ignore=5, ignored=0.3, seed=16),
    Case("c14_headline", (10, 256, 256), 14, seed=17),
]


def _ce(z, y, C, eps, ignore):
    """Per-pixel CrossEntropyLoss(reduction='none', ignore_index, label_smoothing) with an explicit log-softmax; (B, HW)."""
    lsm = z - torch.logsumexp(z, 1, keepdim=True)
    valid = torch.ones_like(y, dtype=torch.bool) if ignore is None else y != ignore
    yy = torch.where(valid, y, torch.zeros_like(y))
    nll = -lsm.gather(1, yy.unsqueeze(1)).squeeze(1)
    ce = (1 - eps) * nll + eps * (-lsm.sum(1) / C)
    return torch.where(valid, ce, torch.zeros_like(ce)), valid


@functools.lru_cache(maxsize=None)
def inputs(case):
    """logits (B, C, HW), labels (B, HW) int64, cotangents for ip (B, 2, C) and the top-k mean: fp32 on the host, never modified."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    B, C, hw = case.shape[0], case.C, math.prod(case.shape[1:])
    z = torch.zeros(B, C, hw) if case.zeros else case.scale * torch.randn(B, C, hw, generator=g)
    y = torch.randint(0, C if case.ignore is None or case.ignore >= C else C - 1, (B, hw), generator=g)
    if case.ignore is not None:
        y = torch.where(torch.rand(B, hw, generator=g) < case.ignored, torch.full_like(y, case.ignore), y)
    if case.plant:
        # two pairs of identical pixels at the threshold: the k-th and the (k+1)-th largest pixel (float64 order) are copied over the two
        # smallest, so that ranks k, k + 1 hold the first pair -- the threshold ties, share 1 / 2 -- and the second pair follows it
        ce, _ = _ce(z.double(), y, C, case.eps, case.ignore)
        order = torch.sort(ce.reshape(-1), descending=True, stable=True)[1]
        k = ops.topk_count(B * hw, 10)
        zf, yf = z.permute(0, 2, 1).reshape(B * hw, C), y.reshape(-1)
        for src, dst in ((order[k - 1], order[-1]), (order[k], order[-2])):
            zf[dst], yf[dst] = zf[src], yf[src]
        z, y = zf.reshape(B, hw, C).permute(0, 2, 1).contiguous(), yf.reshape(B, hw)
    g_ip = torch.randn(B, 2, C, generator=g) * 1e-3
    g_topk = torch.rand((), generator=g) + 0.5
    return z, y, g_ip, g_topk


def evaluate(case, dtype):
    """The formulas of K33 in `dtype` on the host -> dict of results (statistics, threshold record, per-pixel cross-entropy, gradient and
    the two alternative gradients of a pixel: as if selected with weight 1, as if unselected)."""
    z0, y, g_ip, g_topk = inputs(case)
    B, C, hw = z0.shape
    z = z0.to(dtype).requires_grad_(True)
    ce, valid = _ce(z, y, C, case.eps, case.ignore)
    n = B * hw
    k = ops.topk_count(n, 10)
    flat = ce.reshape(-1)
    srt = torch.sort(flat.detach(), descending=True, stable=True)[0]
    t = srt[k - 1]
    n_gt, n_eq = int((flat.detach() > t).sum()), int((flat.detach() == t).sum())
    share = (k - n_gt) / n_eq
    w = torch.where(flat.detach() > t, torch.ones_like(flat), torch.where(flat.detach() == t, torch.full_like(flat, share), torch.zeros_like(flat))).detach()
    topk_sum = (w * flat).sum()
    mean = topk_sum / k
    out = dict(t=t.detach(), n_gt=n_gt, n_eq=n_eq, share=share, topk_sum=topk_sum.detach(), mean=mean.detach(), ce=ce.detach(), k=k, w=w)
    obj = mean * g_topk.to(dtype)
    p = torch.softmax(z, 1)
    if case.dice:
        onehot = torch.zeros(B, C, hw, dtype=dtype).scatter_(1, torch.where(valid, y, torch.zeros_like(y)).unsqueeze(1), 1.0) * valid.unsqueeze(1)
        ip = torch.stack([(p * onehot).sum(2), (p * valid.unsqueeze(1)).sum(2)], 1)          # (B, 2, C)
        out["ip"], out["gt"] = ip.detach(), onehot.sum(2)
        obj = obj + (ip * g_ip.to(dtype)).sum()
    (dz,) = torch.autograd.grad(obj, z)
    out["dz"] = dz
    # the cross-entropy part of a pixel's gradient at weight 1: dz = dz_dice + w_p * unit
    pd = p.detach()
    hit = torch.zeros(B, C, hw, dtype=dtype).scatter_(1, torch.where(valid, y, torch.zeros_like(y)).unsqueeze(1), 1.0)
    unit = g_topk.to(dtype) / k * ((1 - case.eps) * (pd - hit) + case.eps * (pd - 1.0 / C)) * valid.unsqueeze(1)
    out["dz_unselected"] = dz - w.reshape(B, 1, hw) * unit
    out["dz_selected"] = out["dz_unselected"] + unit
    return out


@functools.lru_cache(maxsize=4)
def reference_and_yardstick(case):
    return evaluate(case, torch.float64), evaluate(case, torch.float32)


def excused_pixels(ref):
    """A: the pixels whose float64 cross-entropy lies within BAND max(1, t) of the threshold t without being equal to it.  Pixels equal
    to t in float64 are the threshold pixel itself and its exact ties -- ignored pixels (0.0 by contract on both sides), bit-identical
    planted pixels, the all-zero logits -- which the same arithmetic maps to one fp32 value: rounding cannot separate them, so they are
    compared strictly and take no part in the cap."""
    flat, t = ref["ce"].reshape(-1), float(ref["t"])
    return ((flat - t).abs() <= BAND * max(1.0, t)) & (flat != t)


def _value_err(got, ref):
    ref = torch.as_tensor(ref).double()
    return float(((torch.as_tensor(got).detach().cpu().double() - ref).abs() / ref.abs().clamp(min=1.0)).max())


def _grad_err(got, ref):
    top = float(ref.abs().max())
    worst = float((got.detach().cpu().double() - ref.double()).abs().max())
    return worst / top if top > 0 else (0.0 if worst == 0 else float("inf"))


def device_run(case):
    z0, y, g_ip, g_topk = inputs(case)
    B, C, dims = z0.shape[0], z0.shape[1], case.shape[1:]                     # the level in its own rank: 2-D, 3-D (5-D tensors) or flat
    z = z0.reshape(B, C, *dims).to(DEV).requires_grad_(True)
    ip, gt, rec = ops.topk_ce_stats([z], [y.float().reshape(B, 1, *dims).to(DEV)], case.ignore, case.eps, 10, case.dice)
    obj = rec[0, 3] * g_topk.to(DEV)
    if case.dice:
        obj = obj + (ip[0] * g_ip.to(DEV)).sum()
    (dz,) = torch.autograd.grad(obj, z)
    counts = rec[0, 4:8].view(torch.int64).cpu()
    return dict(ip=None if ip is None else ip[0].cpu(), gt=None if gt is None else gt[0].cpu(), rec=rec[0].detach().cpu(),
                dz=dz.reshape(z0.shape).cpu(),
                n_gt=int(counts[0]), n_eq=int(counts[1]))


def test_select_geometry_matches_the_library():
    assert _lib.lib().mlagg_topk_ce_select_elements_per_workgroup() == EPW


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_topk_ce_matches_float64(case):
    ref, yard = reference_and_yardstick(case)
    n, k, t = ref["ce"].numel(), ref["k"], float(ref["t"])
    # ---- the excused set, from the float64 reference alone
    A = excused_pixels(ref)
    nA = int(A.sum())
    assert nA <= CAP * n, (nA, n)
    strict = nA == 0
    vtol = lambda q: max(VALUE_TOL, 4.0 * _value_err(yard[q], ref[q]))        # noqa: E731
    gtol = max(GRAD_TOL, 4.0 * _grad_err(yard["dz"], ref["dz"]))
    got = device_run(case)
    print(case, "N", n, "k", k, "t", t, "|A|", nA, "n_gt", got["n_gt"], ref["n_gt"], "n_eq", got["n_eq"], ref["n_eq"],
          "value err", _value_err(got["rec"][3], ref["mean"]), "bound", vtol("mean"), "grad err", _grad_err(got["dz"], ref["dz"]), "bound", gtol)
    # ---- statistics
    if case.dice:
        assert _value_err(got["ip"], ref["ip"]) <= vtol("ip")
        assert torch.equal(got["gt"].double(), ref["gt"])
    else:
        assert got["ip"] is None and got["gt"] is None
    # ---- the record
    share = float(got["rec"][1])
    if strict:
        assert (got["n_gt"], got["n_eq"]) == (ref["n_gt"], ref["n_eq"])
        assert abs(share - ref["share"]) <= 1e-6
    else:
        assert abs(got["n_gt"] - ref["n_gt"]) <= nA and got["n_gt"] < k <= got["n_gt"] + got["n_eq"]
    assert abs(got["n_gt"] + share * got["n_eq"] - k) <= 1e-6 * k             # sum w_p == k ...
    assert _value_err(got["rec"][0], ref["t"]) <= max(vtol("t"), BAND if not strict else 0.0)
    assert _value_err(got["rec"][2], ref["topk_sum"]) <= vtol("topk_sum") + (0.0 if strict else nA * BAND)
    assert _value_err(got["rec"][3], ref["mean"]) <= vtol("mean") + (0.0 if strict else nA * BAND / k)
    # ---- the gradient: strictly outside A, either alternative inside
    top = float(ref["dz"].abs().max())
    d = (got["dz"].double() - ref["dz"]).abs().amax(1).reshape(-1)
    if strict:
        assert float(d.max()) <= gtol * top
    else:
        assert float(d[~A].max()) <= gtol * top
        alt = torch.minimum((got["dz"].double() - ref["dz_selected"]).abs().amax(1).reshape(-1),
                            (got["dz"].double() - ref["dz_unselected"]).abs().amax(1).reshape(-1))
        assert float(alt[A].max()) <= gtol * top
    if case.ignore is not None:
        ignored = (inputs(case)[1] == case.ignore).unsqueeze(1).expand_as(got["dz"])
        assert float(got["dz"][ignored].abs().max()) == 0.0


def test_sum_of_weights_is_exactly_k():
    """... exactly, in integers: with ties of n_eq pixels sharing k - n_gt, n_gt < k <= n_gt + n_eq; and the special regimes' records."""
    for case in CASES[:16]:
        got = device_run(case)
        k = ops.topk_count(math.prod(case.shape), 10)
        assert got["n_gt"] < k <= got["n_gt"] + got["n_eq"], case
        assert float(got["rec"][1]) == pytest.approx((k - got["n_gt"]) / got["n_eq"], rel=1e-6), case
    zero = device_run(CASES[8])
    n = math.prod(CASES[8].shape)
    assert (zero["n_gt"], zero["n_eq"]) == (0, n) and float(zero["rec"][0]) == pytest.approx(math.log(5), rel=1e-6)
    assert float(zero["rec"][1]) == pytest.approx(ops.topk_count(n, 10) / n, rel=1e-6)
    ign = device_run(CASES[11])                                                # > 90 % ignored: the threshold is 0, the ties are the ignored pixels
    assert float(ign["rec"][0]) == 0.0 and ign["n_eq"] >= int((inputs(CASES[11])[1] == 5).sum()) > 0.9 * n
    planted = device_run(CASES[13])
    assert planted["n_eq"] == 2 and float(planted["rec"][1]) == 0.5          # the k-th pixel and its copy share one place


@pytest.mark.parametrize("case", [CASES[3], CASES[13], CASES[16]], ids=repr)
def test_two_runs_are_bit_identical(case):
    a, b = device_run(case), device_run(case)
    assert torch.equal(a["rec"], b["rec"]) and torch.equal(a["dz"], b["dz"])
    if case.dice:
        assert torch.equal(a["ip"], b["ip"])


def test_k_zero_raises_on_the_device_path():
    with pytest.raises(RuntimeError):
        ops.topk_ce_stats([torch.zeros(1, 3, 3, 3, device=DEV)], [torch.zeros(1, 1, 3, 3, device=DEV)])


def _levels(ignore):
    g = torch.Generator().manual_seed(77)
    C = 6 if ignore else 5                  # the ignore case: 6 channels, label 5 ignored ("dice" takes no mask and counts it as a class)
    shapes = ((2, C, 40, 36), (2, C, 20, 18), (2, C, 10, 9))
    outs = [2 * torch.randn(*s, generator=g) for s in shapes]
    tgs = [torch.randint(0, C, (s[0], 1) + s[2:], generator=g).float() for s in shapes]
    return outs, tgs


@pytest.mark.parametrize("variant", sorted(trainer.LOSS_VARIANTS))
@pytest.mark.parametrize("ignore", [False, True])
def test_three_level_loss_equals_the_eager_composition(variant, ignore):
    """Device against the eager composition (float64 on the host as the reference, fp32 eager as the yardstick), value and gradient.
    Random inputs: no ties, and the gaps at the thresholds (> 1e-3) are far above the band, so the comparison is strict."""
    outs, tgs = _levels(ignore)
    ign = 5 if ignore else None
    res = {}
    for name, dtype, dev in (("ref", torch.float64, "cpu"), ("yard", torch.float32, "cpu"), ("got", torch.float32, DEV)):
        zs = [o.to(dtype).to(dev).requires_grad_(True) for o in outs]
        ts = [t.to(dtype).to(dev) for t in tgs]
        fn = trainer.loss_variant_deep_supervision_loss if dev == DEV else trainer.loss_variant_deep_supervision_loss_eager
        loss = fn(zs, ts, variant, True, False, ign)
        res[name] = (loss.detach().cpu().double(), [g.cpu().double() for g in torch.autograd.grad(loss, zs)])
    assert _value_err(res["got"][0], res["ref"][0]) <= max(VALUE_TOL, 4.0 * _value_err(res["yard"][0], res["ref"][0]))
    for g, y, r in zip(res["got"][1], res["yard"][1], res["ref"][1]):
        assert _grad_err(g, r) <= max(GRAD_TOL, 4.0 * _grad_err(y, r))


class _TinyNet(torch.nn.Module):
    def __init__(self, n_cls=5):
        super().__init__()
        self.body = torch.nn.Conv2d(1, 8, 3, padding=1)
        self.heads = torch.nn.ModuleList([torch.nn.Conv2d(8, n_cls, 1) for _ in range(3)])

    def forward(self, x):
        f = torch.nn.functional.relu(self.body(x))
        return [h(torch.nn.functional.avg_pool2d(f, 2 ** s) if s else f) for s, h in enumerate(self.heads)]


def test_graphed_step_with_the_dice_topk_loss_follows_the_eager_twin():
    """A GraphedTrainStep whose loss_fn is the "dice_topk10" loss against a twin stepped eagerly: after two replays the parameters are
    bit-identical, as test_graph_gpu.py checks for K9."""
    trainer.set_deterministic(True)
    try:
        torch.manual_seed(0)
        net = _TinyNet().to(DEV)
        twin = copy.deepcopy(net)
        opt, _ = trainer.configure_optimizers(net, capturable=True)
        opt_t, _ = trainer.configure_optimizers(twin)
        loss_fn = lambda o, t: trainer.loss_variant_deep_supervision_loss(list(o), list(t[:len(o)]), "dice_topk10", True, False)  # noqa: E731
        g = torch.Generator().manual_seed(5)
        batches = [(torch.rand(2, 1, 32, 32, generator=g).to(DEV),
                    [torch.randint(0, 5, (2, 1, 32 >> s, 32 >> s), generator=g).float().to(DEV) for s in range(3)]) for _ in range(3)]
        graphed = trainer.GraphedTrainStep(net, opt, *batches[0], warmup=1, loss_fn=loss_fn)
        trainer.train_step(twin, opt_t, *batches[0], loss_fn=loss_fn)
        for data, target in batches[1:]:
            got = float(graphed(data, target))
            want = float(trainer.train_step(twin, opt_t, data, target, loss_fn=loss_fn))
            assert got == want
        for (name, a), b in zip(net.state_dict().items(), twin.state_dict().values()):
            assert torch.equal(a, b), name
    finally:
        trainer.set_deterministic(False)


def test_plugin_with_the_topk_loss_steps_and_replays():
    from oracle import mlagg_oracle as O
    cls = nnunet_plugin.make_trainer_class(FK.nnUNetTrainer, variant="B", loss="topk10")
    tr = cls(FK.make_plans((64, 64), 2), "2d_bs10", 0, FK.make_dataset_json(14), device=torch.device("cuda"))
    tr.initialize()
    O.deterministic_fill_(tr.network.state_dict())
    tr.network.eval()
    assert tr.mlagg_loss_variant == "topk10" and tr._graph_ok() is bool(nnunet_plugin.PLUGIN_GRAPH)
    losses = []
    for it in range(nnunet_plugin.GRAPH_AFTER + 2):
        data, target = trainer.synthetic_batch(2, 1, 64, 64, 14, seed=700 + it)
        losses.append(float(tr.train_step({"data": data, "target": target})["loss"]))
        assert (tr._graphed is not None) == (nnunet_plugin.PLUGIN_GRAPH and it >= nnunet_plugin.GRAPH_AFTER), it
    assert tr._graph_failed is None and all(math.isfinite(v) for v in losses) and tr.optimizer.steps_done() == len(losses)
    data, target = trainer.synthetic_batch(2, 1, 64, 64, 14, seed=700)
    with torch.no_grad():
        outs = tr.network(data.cuda())
    want = trainer.loss_variant_deep_supervision_loss_eager([o.cpu() for o in outs], target, "topk10")
    got = trainer.loss_variant_deep_supervision_loss(outs, [t.cuda() for t in target], "topk10")
    assert abs(float(got) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
