"""K34 on the host: the cases of tests/_optimizer_variant_cases.py are well conditioned (the plain-fp32 torch optimizers stay inside
the bounds, and so does the host model of the kernel's arithmetic) and catch the defects they are meant to catch; PolyLRSchedule is
the reference's formula; ClipSGD / ClipAdam exchange checkpoints with the torch optimizers; configure_optimizers and the plugin
factories deliver the reference's recipes; what the kernels do not implement is refused; the ABI of K34 checks its arguments."""
import copy
import ctypes

import pytest
import torch

import fake_nnunet as FK
import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import _lib, nnunet_plugin, trainer
from tests import _optimizer_variant_cases as V
from tests import _step_tail_cases as K
from tests.test_plugin_cpu import StubNet

ALL = V.CASES + V.ABI_CASES


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def test_case_list_is_the_one_the_kernel_paths_ask_for():
    assert V.SIZES == K.K11_SIZES and V.LEADS == (0, 1, 2, 3) and V.MAX_NORMS == (12.0, 0.05, 0.0)
    # between the four leads every size sits at an aligned and at a misaligned offset of the flat gradient buffer
    seen = {n: set() for n in V.SIZES}
    for lead in V.LEADS:
        sizes = ((lead,) if lead else ()) + V.SIZES
        for n, off in zip(sizes, K.k11_grad_offsets(sizes)):
            if n in seen and not (lead and n == lead and off == 0):
                seen[n].add(K.k11_sumsq_path(4 * off))
    assert all(v == {"vector", "scalar"} for v in seen.values()), seen
    for kind in V.KINDS:
        regimes = {c.regime for c in V.CASES if c.kind == kind}
        assert regimes >= {"unit", "dominated", "zero", "near_below", "near_above", "resumed"}
        assert ("falling" in regimes) == (kind == "adamw_ams")
        assert {c.max_norm for c in V.CASES if c.kind == kind and c.regime == "unit"} == set(V.MAX_NORMS)
        assert {c.misaligned for c in V.ABI_CASES if c.kind == kind} == {"none"} | set(V.ABI_POINTERS[kind])
    assert {c.n for c in V.ABI_CASES} == {5, 65537}


def test_the_falling_regime_separates_max_exp_avg_sq_from_exp_avg_sq():
    for case in V.CASES:
        if case.regime in ("falling", "resumed") and case.kind == "adamw_ams":
            ref, _ = V.reference_and_yardstick(case)
            x, v = torch.cat(ref["max_exp_avg_sq"]), torch.cat(ref["exp_avg_sq"])
            # in most elements the maximum is more than ten times the 1e-4 bound of the second moments above the moment itself
            assert float(((x - v) / x > 1e-3).double().mean()) > 0.75, case


@pytest.mark.parametrize("case", ALL, ids=[V.case_id(c) for c in ALL])
def test_yardstick_and_host_model_stay_inside_the_bounds(case):
    ref, yard = V.reference_and_yardstick(case)
    tols = V.bounds(case, ref, yard)
    assert set(tols) == {"p"} | set(V.STATE[case.kind]) | ({"norm"} if V.max_norm_of(case) > 0 else set())
    got = V.model(case)
    for q, tol in tols.items():
        assert tol.a >= V.FLOORS[q].a
        assert V.error(yard[q], ref[q], tol) <= tol.a, q
        err = V.error(got[q], ref[q], tol)
        assert err <= tol.a, (q, err, tol)


@pytest.mark.parametrize("kind,defect", [(k, d) for k in V.KINDS for d in V.DEFECTS[k]])
def test_seeded_defects_land_ten_times_outside_the_bounds(kind, defect):
    worst = 0.0
    for case in V.CASES:
        if case.kind != kind:
            continue
        if defect == "no_clip" and not (case.max_norm == 0.05 and case.regime in ("unit", "dominated")):
            continue                                                          # where the coefficient is far from 1
        if defect == "v_for_vmax" and case.regime not in ("falling", "resumed"):
            continue
        if defect in ("no_nesterov", "skip_tail") and not (case.regime == "unit" and case.max_norm == 0.0):
            continue
        if defect == "wrong_decay" and case.regime != "zero":
            continue                                                          # only the decay moves anything there
        ref, yard = V.reference_and_yardstick(case)
        tols = V.bounds(case, ref, yard)
        got = V.model(case, defect)
        worst = max(worst, max(V.error(got[q], ref[q], tol) / tol.a for q, tol in tols.items()))
    print(f"{kind} {defect}: {worst:.1f} x the bound")
    assert worst >= 10.0, worst


# ---------------------------------------------------------------------------------------------------------------------
# schedule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epochs", [5, 1000])
def test_poly_lr_is_the_reference_formula(epochs):
    ps = [torch.nn.Parameter(torch.zeros(3))]
    opt = trainer.ClipSGD(ps)
    sched = trainer.PolyLRSchedule(opt, 1e-2, epochs)
    assert opt.param_groups[0]["lr"] == 1e-2 and sched.ctr == 1               # the reference's base class steps once on construction
    for epoch in range(epochs):
        sched.step(epoch)                                                     # nnUNetTrainer.py:825
        lr = opt.param_groups[0]["lr"]
        assert type(lr) is float and lr == 1e-2 * (1 - epoch / epochs) ** 0.9     # polylr.py:18
    assert sched.ctr == 1
    # without an epoch: the internal counter, which the construction left at 1
    for want in range(1, min(epochs, 7)):
        sched.step() if want % 2 else sched.step(-1)
        assert opt.param_groups[0]["lr"] == 1e-2 * (1 - want / epochs) ** 0.9 and sched.ctr == want + 1
    other = trainer.PolyLRSchedule(opt, 3e-4, epochs, exponent=2.0)
    other.step(epochs - 1)
    assert opt.param_groups[0]["lr"] == 3e-4 * (1 - (epochs - 1) / epochs) ** 2.0


# ---------------------------------------------------------------------------------------------------------------------
# state dicts
# ---------------------------------------------------------------------------------------------------------------------
def _ours(kind, ps, **kw):
    if kind == "sgd":
        return trainer.ClipSGD(ps, V.SGD_LR, V.SGD_MOMENTUM, V.WD, **kw)
    return trainer.ClipAdam(ps, V.ADAM_LR, V.ADAM_BETAS, V.ADAM_EPS, V.WD, amsgrad=kind == "adamw_ams", decoupled=kind == "adamw_ams", **kw)


@pytest.mark.parametrize("kind", V.KINDS)
def test_state_dicts_round_trip_with_the_torch_optimizers(kind):
    torch.manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (5, 7)]
    ours, theirs = _ours(kind, ps), V.torch_optimizer(kind, ps)
    assert isinstance(ours, trainer.ClipOptimizer) and not ours.capturable
    assert set(ours.state_dict()["param_groups"][0]) == set(theirs.state_dict()["param_groups"][0])
    for k, v in theirs.state_dict()["param_groups"][0].items():
        assert k == "foreach" or ours.state_dict()["param_groups"][0][k] == v, k      # (the cases pin torch to its single-tensor loop)
    # a torch checkpoint from before the first step
    ours.load_state_dict(theirs.state_dict())
    assert ours.steps_done() == 0 and not ours.state_dict()["state"]
    for p in ps:
        p.grad = torch.randn_like(p)
    theirs.step()
    theirs.step()
    ours.load_state_dict(theirs.state_dict())
    for p in ps:
        assert set(ours.state[p]) == set(theirs.state[p]) == set(V.STATE[kind]) | (set() if kind == "sgd" else {"step"})
        for k in V.STATE[kind]:
            assert torch.equal(ours.state[p][k], theirs.state[p][k])
    assert ours.steps_done() == (0 if kind == "sgd" else 2)
    # and back: torch steps on from our checkpoint exactly as from its own
    twin_ps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    twin = V.torch_optimizer(kind, twin_ps)
    twin.load_state_dict(copy.deepcopy(ours.state_dict()))                    # (an in-memory state dict shares its tensors)
    for p, q in zip(ps, twin_ps):
        q.grad = p.grad.clone()
    theirs.step()
    twin.step()
    for p, q in zip(ps, twin_ps):
        assert torch.equal(p, q)
    with pytest.raises(RuntimeError):
        ours.step(max_norm=12.0)                                              # host tensors: the kernels have no CPU form


def test_sgd_checkpoint_without_a_buffer_loads_as_zeros():
    ps = [torch.nn.Parameter(torch.randn(5))]
    sd = torch.optim.SGD(ps, lr=1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5).state_dict()
    sd["state"] = {0: {"momentum_buffer": None}}                              # what torch.optim.SGD wrote while no buffer existed
    ours = trainer.ClipSGD(ps)
    ours.load_state_dict(sd)
    assert torch.equal(ours.state[ps[0]]["momentum_buffer"], torch.zeros(5))


def test_refusals():
    ps = [torch.nn.Parameter(torch.randn(5))]
    with pytest.raises(RuntimeError, match="nesterov"):
        trainer.ClipSGD(ps, nesterov=False)
    with pytest.raises(RuntimeError, match="dampening"):
        trainer.ClipSGD(ps, dampening=0.1)
    with pytest.raises(RuntimeError, match="one parameter group"):
        trainer.ClipSGD([dict(params=ps), dict(params=[torch.nn.Parameter(torch.randn(2))])])
    with pytest.raises(RuntimeError, match="one parameter group"):
        trainer.ClipAdam([dict(params=ps), dict(params=[torch.nn.Parameter(torch.randn(2))])])
    for amsgrad, decoupled in ((True, False), (False, True)):
        with pytest.raises(RuntimeError, match="has no kernel"):
            trainer.ClipAdam(ps, amsgrad=amsgrad, decoupled=decoupled)
    # a checkpoint of the other recipe, or of plain SGD, is refused before anything is loaded
    ams = trainer.ClipAdam(ps, amsgrad=True, decoupled=True)
    with pytest.raises(RuntimeError, match="other recipe"):
        ams.load_state_dict(torch.optim.Adam(ps, lr=1e-2).state_dict())
    sgd = trainer.ClipSGD(ps)
    with pytest.raises(RuntimeError, match="nesterov"):
        sgd.load_state_dict(torch.optim.SGD(ps, lr=1e-2, momentum=0.9).state_dict())
    assert sgd.param_groups[0]["nesterov"] is True
    with pytest.raises(RuntimeError):
        trainer.configure_optimizers(torch.nn.Linear(2, 2), optimizer="adan")
    for factory in (nnunet_plugin.make_trainer_class, nnunet_plugin.make_umamba_enc_ss3d_trainer_class):
        for bad in ("adan", "adamw"):
            with pytest.raises(RuntimeError):
                factory(FK.nnUNetTrainer, optimizer=bad)


# ---------------------------------------------------------------------------------------------------------------------
# configure_optimizers and the plugin
# ---------------------------------------------------------------------------------------------------------------------
def test_configure_optimizers_on_a_cpu_model_gives_the_reference_recipes():
    net = torch.nn.Linear(4, 3)
    opt, sched = trainer.configure_optimizers(net)                            # the default is untouched
    assert type(opt) is torch.optim.AdamW and type(sched) is trainer.CosineLRSchedule
    g = opt.param_groups[0]
    assert (g["lr"], g["eps"], g["weight_decay"], g["amsgrad"]) == (5e-4, 1e-4, 3e-5, False)
    want = {"sgd": (torch.optim.SGD, dict(lr=1e-2, momentum=0.99, nesterov=True, dampening=0, weight_decay=3e-5)),
            "adam": (torch.optim.AdamW, dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=3e-5, amsgrad=True)),
            "vanilla_adam": (torch.optim.Adam, dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=3e-5, amsgrad=False))}
    for name, (cls, hyper) in want.items():
        opt, sched = trainer.configure_optimizers(net, optimizer=name, num_epochs=50)
        assert type(opt) is cls and type(sched) is trainer.PolyLRSchedule and sched.max_steps == 50 and sched.initial_lr == 1e-2
        for k, v in hyper.items():
            assert opt.param_groups[0][k] == v, (name, k)
        sched.step(10)
        assert opt.param_groups[0]["lr"] == 1e-2 * (1 - 10 / 50) ** 0.9
        opt, sched = trainer.configure_optimizers(net, 3e-4, optimizer=name)
        assert opt.param_groups[0]["lr"] == 3e-4 and sched.max_steps == 1000
    assert trainer.OPTIMIZERS == ("adamw",) + tuple(want)


@pytest.fixture
def stub_model(monkeypatch):
    from mlagg_unet_amd import model, model3d

    def build(patch_size, in_ch, n_cls, ds=True, variant="B", precision="fp32"):
        torch.manual_seed(0)
        return StubNet(in_ch, n_cls, ds)

    def build_3d(in_ch, n_cls, kernels, strides, n_enc, n_dec, base, cap, ds):
        torch.manual_seed(0)
        return StubNet(in_ch, n_cls, ds)

    monkeypatch.setattr(model, "build_network_architecture", build)
    monkeypatch.setattr(model3d, "build_network_architecture_3d", build_3d)
    monkeypatch.setenv("MLAGG_MIOPEN_TUNED", "0")


@pytest.mark.parametrize("name,cls_want", [("sgd", torch.optim.SGD), ("adam", torch.optim.AdamW), ("vanilla_adam", torch.optim.Adam)])
def test_factories_build_the_optimizer_variant(stub_model, name, cls_want):
    dj = FK.make_dataset_json(5)
    cls = nnunet_plugin.make_trainer_class(FK.nnUNetTrainer, optimizer=name)
    assert cls.__name__ == "nnUNetTrainer_MLAgg_2D_dt_MS"
    tr = cls(FK.make_plans((32, 32), 2), "2d_bs10", 0, dj, device=torch.device("cpu"))
    tr.initialize()
    assert tr.mlagg_optimizer == name and tr.mlagg_loss_variant == "dice_ce" and tr.initial_lr == 1e-2
    assert type(tr.optimizer) is cls_want and type(tr.lr_scheduler) is trainer.PolyLRSchedule       # host parameters: torch's optimizer
    assert tr.lr_scheduler.max_steps == tr.num_epochs == 500 and tr.optimizer.param_groups[0]["weight_decay"] == 3e-5
    tr.lr_scheduler.step(100)
    assert tr.optimizer.param_groups[0]["lr"] == 1e-2 * (1 - 100 / 500) ** 0.9
    # the default class keeps AdamW + cosine at 5e-4
    default = nnunet_plugin.make_trainer_class(FK.nnUNetTrainer)(FK.make_plans((32, 32), 2), "2d_bs10", 0, dj, device=torch.device("cpu"))
    default.initialize()
    assert default.mlagg_optimizer is None and default.initial_lr == 5e-4 and type(default.lr_scheduler) is trainer.CosineLRSchedule
    # the 3-D class: None inherits the host trainer's configure_optimizers, a name overrides it
    plain3d = nnunet_plugin.make_umamba_enc_ss3d_trainer_class(FK.nnUNetTrainer)
    assert "configure_optimizers" not in vars(plain3d)
    cls3d = nnunet_plugin.make_umamba_enc_ss3d_trainer_class(FK.nnUNetTrainer, optimizer=name)
    assert cls3d.__name__ == "nnUNetTrainerUMambaEnc_SS3D" and "configure_optimizers" in vars(cls3d)
    strides = [[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2], [2, 2, 2], [1, 2, 2]]
    for c3, opt_want, recorded in ((cls3d, cls_want, name), (plain3d, torch.optim.SGD, None)):
        tr3d = c3(FK.make_plans_3d((96, 160, 160), 2, strides), "3d_fullres", 0, FK.make_dataset_json(14), device=torch.device("cpu"))
        tr3d.initialize()
        assert tr3d.mlagg_optimizer == recorded and tr3d.mlagg_loss_variant == "dice_ce" and tr3d.initial_lr == 1e-2
        assert type(tr3d.optimizer) is opt_want and tr3d.optimizer.param_groups[0]["weight_decay"] == 3e-5
        assert tr3d.optimizer.param_groups[0]["lr"] == 1e-2
        if recorded is not None:
            assert type(tr3d.lr_scheduler) is trainer.PolyLRSchedule and tr3d.lr_scheduler.max_steps == tr3d.num_epochs
            tr3d.lr_scheduler.step(100)
            assert tr3d.optimizer.param_groups[0]["lr"] == 1e-2 * (1 - 100 / tr3d.num_epochs) ** 0.9


# ---------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_exist_and_check_their_arguments():
    """The entry points of the optimizer step reject NULL pointers and unknown kinds on the host: no kernel is launched, no GPU is
    needed."""
    lib = _lib.lib()
    C = _lib.CONSTANTS
    assert (C["MLAGG_OPT_SGD_NESTEROV"], C["MLAGG_OPT_ADAMW_AMSGRAD"], C["MLAGG_OPT_ADAM_L2"], C["MLAGG_OPT_ADAMW"]) == (0, 1, 2, 3)
    assert "mlagg_adamw_clip_step" not in _lib.SIGNATURES and "mlagg_adamw_clip_step_dev" not in _lib.SIGNATURES
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    hyper = (1e-2, 0.9, 0.999, 1e-8, 3e-5, 12.0)
    assert lib.mlagg_optimizer_clip_step(0, None, None, ptr, 1, ptr, *hyper, 1, None) == C["MLAGG_E_NULLPTR"]
    assert lib.mlagg_optimizer_clip_step(0, ptr, None, ptr, 0, ptr, *hyper, 1, None) == C["MLAGG_E_UNSUPPORTED"]
    for kind in (4, -1):
        assert lib.mlagg_optimizer_clip_step(kind, ptr, ptr, ptr, 1, ptr, *hyper, 1, None) == C["MLAGG_E_UNSUPPORTED"]
    assert lib.mlagg_optimizer_clip_step(3, ptr, None, ptr, 1, ptr, *hyper, 0, None) == C["MLAGG_E_UNSUPPORTED"]      # AdamW at step 0
    assert lib.mlagg_optimizer_clip_step(3, None, None, ptr, 1, ptr, *hyper, 1, None) == C["MLAGG_E_NULLPTR"]
    assert lib.mlagg_optimizer_clip_step(1, ptr, None, ptr, 1, ptr, *hyper, 1, None) == C["MLAGG_E_UNSUPPORTED"]      # amsgrad without its table
    assert lib.mlagg_optimizer_clip_step(2, ptr, None, ptr, 1, ptr, *hyper, 0, None) == C["MLAGG_E_UNSUPPORTED"]      # Adam at step 0
    assert lib.mlagg_optimizer_clip_step_dev(0, ptr, None, ptr, 1, ptr, None, ptr, *hyper[1:], None) == C["MLAGG_E_NULLPTR"]
    assert lib.mlagg_optimizer_clip_step_dev(0, ptr, None, ptr, 1, ptr, ptr, None, *hyper[1:], None) == C["MLAGG_E_NULLPTR"]
    assert lib.mlagg_optimizer_clip_step_dev(-1, ptr, None, ptr, 1, ptr, ptr, ptr, *hyper[1:], None) == C["MLAGG_E_UNSUPPORTED"]
    names = [lib.mlagg_profile_kernel_name(i).decode() for i in range(lib.mlagg_profile_kernel_count())]
    assert names[-1].startswith("optimizer variants") and names[-2].startswith("topk_ce grad")      # appended: earlier indices keep their meaning
