"""GPU: K9 (Dice + cross-entropy), K29 (Dice + BCE) and K11 (clip + AdamW) against the float64 references of
tests/_step_tail_cases.py at the sizes, class / head counts, label layouts and gradient addresses where their code changes path
(tests/test_step_tail_paths_cpu.py shows which case enters which path, that the cases are well conditioned and what defects they
catch).  The loss kernels are compared at statistics level and at gradient level under random upstream cotangents, a subset also
through trainer.deep_supervision_loss; K11 through trainer.ClipAdamW in both forms, with the gradients laid out as the bucketed
gradient exchange lays them out, and through the C ABI with one misaligned pointer at a time."""
import pytest
import torch

from tests import _step_tail_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(cases):
    return [K.case_id(c) for c in cases]


def _dev(t):
    return t.to(DEV)


def _check(case, got):
    ref, yard = K.reference_and_yardstick(case)
    tols = K.bounds(case, ref, yard)
    assert set(got) == set(tols), set(got) ^ set(tols)
    failed = []
    for q, tol in tols.items():
        if not isinstance(ref[q], list):
            assert got[q].shape == ref[q].shape, (q, got[q].shape, ref[q].shape)
        err = K.error(got[q], ref[q], tol)
        print(f"{K.family(case)} {K.case_id(case)} {q}: error {err:.2e} ({tol.kind} {tol.a:.2e})")
        if not err <= tol.a:                                                      # (a NaN fails too)
            failed.append((q, err, tol))
    assert not failed, failed


def _sliced(z):
    """`z` as the columns [2, 2 + W) of a tensor four columns wider: not contiguous, the same values."""
    wide = torch.full(z.shape[:-1] + (z.shape[-1] + 4,), 7.0, device=z.device)
    wide[..., 2:-2] = z
    view = wide[..., 2:-2]
    assert not view.is_contiguous()
    return view


class _SliceOf(torch.autograd.Function):
    """z as a NON-CONTIGUOUS slice of a wider tensor holding the same values; the gradient passes through unchanged."""

    @staticmethod
    def forward(ctx, z):
        return _sliced(z)

    @staticmethod
    def backward(ctx, g):
        return g


# ---------------------------------------------------------------------------------------------------------------------
# K9
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.K9_CASES, ids=_ids(K.K9_CASES))
def test_dice_ce_paths_match_float64(case):
    from mlagg_unet_amd import ops, trainer
    t = K.inputs(case)
    assert t["logits"].shape == (case.B, case.C) + tuple(case.dims) and K.hw_of(case) == t["logits"][0, 0].numel()
    target = _dev(t["target"])

    z = _dev(t["logits"]).requires_grad_(True)
    zin = _SliceOf.apply(z) if case.tweak == "slice" else z                       # the wrapper's .contiguous() handles the slice
    assert zin.is_contiguous() == (case.tweak != "slice") and torch.equal(zin, z)
    ip, gt, ce = ops.dice_ce_stats([zin], [target], case.ignore)
    assert ip.shape == (1, case.B, 2, case.C) and gt.shape == (1, case.B, case.C) and ce.shape == (1,)
    dz, = torch.autograd.grad((ip, ce), z, (_dev(t["g_ip"])[None], _dev(t["g_ce"])))
    got = dict(ip=ip[0].detach(), gt=gt[0], ce=ce.detach(), dlogits=dz)
    ignored = None
    if case.ignore is not None:
        ignored = (target == case.ignore).expand(-1, case.C, *[-1] * len(case.dims))
        assert bool(ignored.any()) and float(dz[ignored].abs().max()) == 0.0       # exactly no gradient at an ignored pixel
    if case.loss:
        for bd in (1, 0):
            z2 = _dev(t["logits"]).requires_grad_(True)
            zin2 = _SliceOf.apply(z2) if case.tweak == "slice" else z2
            loss = trainer.deep_supervision_loss([zin2], [target], batch_dice=bool(bd), ignore_label=case.ignore)
            g, = torch.autograd.grad(loss, z2)
            got[f"loss_bd{bd}"], got[f"dloss_bd{bd}"] = loss.detach().reshape(1), g
            if ignored is not None:
                assert float(g[ignored].abs().max()) == 0.0
    _check(case, got)


def test_dice_ce_refuses_more_than_max_classes():
    from mlagg_unet_amd import ops
    z = torch.zeros(1, K.K9_MAXC + 1, 4, 4, device=DEV)
    with pytest.raises(RuntimeError, match="at most 16 classes"):
        ops.dice_ce_stats([z], [torch.zeros(1, 1, 4, 4, device=DEV)], None)


def test_dice_ce_ran_at_max_classes_with_the_ignore_label_equal_to_it():
    """What the parametrised test above ran, said once: C = MAXC = 16 with ignore label 16, thread 48 writing the CE partial."""
    mine = [c for c in K.K9_CASES if c.C == K.K9_MAXC and c.ignore == K.K9_MAXC]
    assert len(mine) >= 12 and K.k9_ce_writer(K.K9_MAXC) == 48 and any(c.loss for c in mine)


# ---------------------------------------------------------------------------------------------------------------------
# K29
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.K29_CASES, ids=_ids(K.K29_CASES))
def test_dice_bce_paths_match_float64(case):
    from mlagg_unet_amd import ops
    t = K.inputs(case)
    R = case.R
    ign = R + 1 if case.ignore else None
    if case.form == "labels":
        target, member = _dev(t["seg"]), ops.region_member_table(K.k29_regions(R), torch.device(DEV))
    else:
        target, member = _dev(K.k29_planes(case, t["seg"])), None
        assert target.shape[1] == R + int(case.ignore)
    z = _dev(t["logits"]).requires_grad_(True)
    ip, gt, sums = ops.dice_bce_stats([z], [target], member, ign)
    assert ip.shape == (1, case.B, 2, R) and gt.shape == (1, case.B, R) and sums.shape == (1, 2)
    dz, = torch.autograd.grad((ip, sums), z, (_dev(t["g_ip"])[None], _dev(t["g_sums"])[None]))       # the mask sum carries no gradient
    if case.ignore:
        ignored = (_dev(t["seg"]) == R + 1).expand(-1, R, *[-1] * len(case.dims))
        assert bool(ignored.any()) and float(dz[ignored].abs().max()) == 0.0
    _check(case, dict(ip=ip[0].detach(), gt=gt[0], bce=sums[0, :1].detach(), mask=sums[0, 1:].detach(), dlogits=dz))


def test_dice_bce_ran_the_eight_head_variant_in_both_target_forms():
    """What the parametrised test above ran, said once: 5 and 8 heads take the RB = 8 kernels, as label map and as planes."""
    for form in K.K29_FORMS:
        assert {c.R for c in K.K29_CASES if c.form == form and K.k29_rb(c.R) == 8} == {5, 8}


# ---------------------------------------------------------------------------------------------------------------------
# K11
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
@pytest.mark.parametrize("case", K.K11_CASES, ids=_ids(K.K11_CASES))
def test_clip_adamw_paths_match_float64(case, capturable):
    from mlagg_unet_amd import trainer
    t = K.inputs(case)
    sizes = K.k11_sizes(case)
    offs = K.k11_grad_offsets(sizes)
    ps = [torch.nn.Parameter(_dev(p)) for p in t["params"]]
    opt = trainer.ClipAdamW(ps, K.K11_LR, betas=K.K11_BETAS, eps=K.K11_EPS, weight_decay=K.K11_WD, capturable=capturable)
    if case.resume:
        sd = opt.state_dict()
        sd["state"] = {i: dict(step=torch.tensor(float(step)), exp_avg=_dev(m), exp_avg_sq=_dev(v)) for i, (step, m, v) in enumerate(t["state0"])}
        opt.load_state_dict(sd)
        assert opt.steps_done() == K.K11_RESUME_STEP
    norms, sumsq_paths, update_paths = [], set(), set()
    for gs in t["grads"]:
        flat = _dev(torch.cat(gs))                                                # one flat buffer, every p.grad a view at a running offset
        assert flat.data_ptr() % 16 == 0
        for p, off in zip(ps, offs):
            p.grad = flat[off:off + p.numel()].view_as(p)
        before = flat.clone()
        opt.step(max_norm=case.max_norm)
        assert torch.equal(flat, before)                                          # the gradients stay as they were, bit for bit
        if case.max_norm > 0:
            norms.append(opt.grad_norm().cpu())
        for p in ps:
            st = opt.state[p]
            sumsq_paths.add(K.k11_sumsq_path(p.grad.data_ptr()))
            update_paths.add(K.k11_update_path(p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()))
    # both kernels took both paths, as the offsets said they would
    assert sumsq_paths == update_paths == {"vector", "scalar"} == {K.k11_sumsq_path(4 * off) for off in offs}
    assert opt.steps_done() == (K.K11_RESUME_STEP if case.resume else 0) + K.K11_STEPS
    got = dict(p=[p.detach() for p in ps], exp_avg=[opt.state[p]["exp_avg"] for p in ps], exp_avg_sq=[opt.state[p]["exp_avg_sq"] for p in ps])
    if case.max_norm > 0:
        got["norm"] = norms
    _check(case, got)


@pytest.mark.parametrize("case", K.K11_ABI_CASES, ids=_ids(K.K11_ABI_CASES))
def test_adamw_c_abi_with_one_misaligned_pointer(case):
    """mlagg_optimizer_clip_step with MLAGG_OPT_ADAMW (no extra table) on a hand-built table and work list: each of p, g, m, v four bytes
    off a 16-byte boundary alone sends the update kernel down its scalar path (g: the norm kernel too); nothing is written beside the
    tensors."""
    from mlagg_unet_amd import _lib
    t = K.inputs(case)
    n = case.n
    step0, m0, v0 = t["state0"][0]
    bufs, views = {}, {}
    for name, values in (("p", t["params"][0]), ("g", t["grads"][0][0]), ("m", m0), ("v", v0)):
        buf = torch.full((n + 8,), 7.0, device=DEV)
        assert buf.data_ptr() % 16 == 0
        lo = 5 if name == case.misaligned else 4
        buf[lo:lo + n] = _dev(values)
        bufs[name], views[name] = (buf, lo), buf[lo:lo + n]
    addr = {k: v.data_ptr() for k, v in views.items()}
    for name in "pgmv":
        assert (addr[name] % 16 != 0) == (name == case.misaligned)
    assert K.k11_update_path(addr["p"], addr["g"], addr["m"], addr["v"]) == ("vector" if case.misaligned == "none" else "scalar")
    assert K.k11_sumsq_path(addr["g"]) == ("scalar" if case.misaligned == "g" else "vector")
    chunks = K.k11_chunks(n)
    table = _dev(torch.tensor([[addr["p"], addr["g"], addr["m"], addr["v"], n]], dtype=torch.int64))
    work = _dev(torch.tensor([(0, c) for c in range(chunks)], dtype=torch.int32))
    sumsq = torch.zeros(1 + chunks, dtype=torch.float64, device=DEV)
    g_before = views["g"].clone()
    _lib.launch("mlagg_optimizer_clip_step", _lib.CONSTANTS["MLAGG_OPT_ADAMW"], table.data_ptr(), None, work.data_ptr(), chunks,
                sumsq.data_ptr(), K.K11_LR, K.K11_BETAS[0], K.K11_BETAS[1], K.K11_EPS, K.K11_WD, K.K11_ABI_MAX_NORM, step0 + 1)
    torch.cuda.synchronize()
    for name, (buf, lo) in bufs.items():
        assert float((buf[:lo] - 7.0).abs().max()) == 0.0 and float((buf[lo + n:] - 7.0).abs().max()) == 0.0, name
    assert torch.equal(views["g"], g_before)
    _check(case, dict(p=[views["p"]], exp_avg=[views["m"]], exp_avg_sq=[views["v"]], norm=[sumsq[:1].sqrt().cpu()]))
