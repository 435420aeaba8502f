"""K35 on the host: the cases of tests/_loss_scale_cases.py are well conditioned (the plain-fp32 torch composition and the host model of
the kernels' arithmetic stay inside the bounds and take the reference's decisions) and catch the defects they are meant to catch;
trainer.DeviceGradScaler's host fallback makes the reference's decisions; its state dict is torch.amp.GradScaler's; the plugin
factories take ``loss_scaling``; the ABI of K35 checks its arguments."""
import ctypes

import pytest
import torch

import fake_nnunet as FK
import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import _lib, nnunet_plugin, trainer
from tests import _loss_scale_cases as L
from tests.test_plugin_cpu import StubNet

ALL = L.CASES + L.ABI_CASES


def test_case_list_covers_every_regime_for_every_kind():
    for kind in L.KINDS:
        mine = [c for c in L.CASES if c.kind == kind]
        assert {c.regime for c in mine} == set(L.SETUP) - {"abi"}
        assert {c.max_norm for c in mine if c.regime == "unit"} == set(L.MAX_NORMS) and {c.lead for c in mine if c.regime == "unit"} == set(L.LEADS)
        assert {c.misaligned for c in L.ABI_CASES if c.kind == kind} == {"none"} | set(L.ABI_POINTERS[kind])
    assert {c.n for c in L.ABI_CASES} == {5, 65537}
    # the poisoned elements sit where the issue puts them: the scalar tail of the last chunk of 131073, and element 0 of a tensor whose
    # gradient starts 4-byte-misaligned in the flat buffer
    case = L.LSCase("adamw", 0, "inf_tail", 12.0)
    k, i, e, v = L.poison(case)
    assert (k, L.sizes_of(case)[i], e, v) == (1, 131073, 131072, float("inf")) and L.K.k11_last_chunk(131073) == (0, 1)
    case = L.LSCase("adamw", 1, "nan_head", 12.0)
    k, i, e, v = L.poison(case)
    assert k == 0 and e == 0 and v != v and L.K.k11_sumsq_path(4 * L.K.k11_grad_offsets(L.sizes_of(case))[i]) == "scalar"


def test_reference_decisions_are_the_ones_the_regimes_name():
    for kind in L.KINDS:
        d = L.reference_and_yardstick(L.LSCase(kind, 0, "inf_tail", 12.0))[0]["decisions"]
        assert [x[1:] for x in d] == [(False, 65536.0, 1, 1), (True, 32768.0, 0, 1), (False, 32768.0, 1, 2), (False, 32768.0, 2, 3)]
        d = L.reference_and_yardstick(L.LSCase(kind, 1, "nan_head", 12.0))[0]["decisions"]
        assert [x[1:] for x in d] == [(True, 32768.0, 0, 0), (False, 32768.0, 1, 1), (False, 32768.0, 2, 2)]
        d = L.reference_and_yardstick(L.LSCase(kind, 3, "growth", 12.0))[0]["decisions"]
        assert [x[2:4] for x in d] == [(65536.0, 1), (131072.0, 0), (131072.0, 1), (262144.0, 0), (262144.0, 1)]
        d = L.reference_and_yardstick(L.LSCase(kind, 0, "growth_sat", 12.0))[0]["decisions"]
        big = float(torch.tensor(3e38, dtype=torch.float32))
        assert [x[1:4] for x in d] == [(False, big, 0)] * 3


def test_near_cases_have_a_scaled_norm_far_above_max_norm():
    for case in L.CASES:
        if case.regime in ("near_below", "near_above"):
            ref, _ = L.reference_and_yardstick(case)
            for n, sg in zip(ref["norm"], L.scaled_grads(case)):
                rel = float(n) / case.max_norm - 1.0
                assert 2e-4 < (-rel if case.regime == "near_below" else rel) < 8e-4
                assert float(torch.sqrt(sum((a.double() ** 2).sum() for a in sg))) > 6e4 * case.max_norm


@pytest.mark.parametrize("case", ALL, ids=[L.case_id(c) for c in ALL])
def test_yardstick_and_host_model_stay_inside_the_bounds(case):
    ref, yard = L.reference_and_yardstick(case)
    tols = L.bounds(case, ref, yard)
    assert set(tols) == {"p"} | set(L.STATE[case.kind]) | ({"norm"} if L.max_norm_of(case) > 0 else set())
    got = L.model(case)
    assert yard["decisions"] == ref["decisions"] == got["decisions"]
    for q, tol in tols.items():
        assert tol.a >= L.FLOORS[q].a
        assert L.error(yard[q], ref[q], tol) <= tol.a, q
        err = L.error(got[q], ref[q], tol)
        assert err <= tol.a, (q, err, tol)


# the cases in which a defect can show
DEFECT_REGIMES = {"norm_of_scaled": ("unit", "near_below"), "count_on_skip": ("inf_tail", "nan_head"), "write_on_skip": ("inf_tail", "nan_head"),
                  "grow_unguarded": ("growth_sat",), "tracker_kept": ("inf_tail",), "mult_from_new_scale": ("growth",)}


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("defect", L.DEFECTS)
def test_seeded_defects_land_outside_the_bounds(kind, defect):
    """Each defect either changes a decision (scale, tracker, applied steps: compared exactly) or puts a tensor at least 10 x outside
    its bound on at least one case."""
    worst, decided = 0.0, False
    for case in L.CASES:
        if case.kind != kind or case.regime not in DEFECT_REGIMES[defect] or (defect == "norm_of_scaled" and case.max_norm == 0.0):
            continue
        ref, yard = L.reference_and_yardstick(case)
        tols = L.bounds(case, ref, yard)
        got = L.model(case, defect)
        decided = decided or got["decisions"] != ref["decisions"]
        for q, tol in tols.items():
            if q == "norm" and len(got[q]) != len(ref[q]):
                continue
            worst = max(worst, L.error(got[q], ref[q], tol) / tol.a)
    print(f"{kind} {defect}: decisions differ: {decided}; {worst:.1f} x the bound")
    assert decided or worst >= 10.0, (decided, worst)
    if defect in ("norm_of_scaled", "write_on_skip", "mult_from_new_scale") or (defect == "count_on_skip" and kind != "sgd"):
        assert worst >= 10.0, worst                                           # these show in the tensors themselves


# ---------------------------------------------------------------------------------------------------------------------
# DeviceGradScaler on the host
# ---------------------------------------------------------------------------------------------------------------------
HOST_CASES = [c for c in L.CASES if c.lead in (0, 1) and (c.regime != "unit" or c.lead == 0)]


@pytest.mark.parametrize("case", HOST_CASES, ids=[L.case_id(c) for c in HOST_CASES])
def test_host_fallback_makes_the_reference_decisions(case):
    """Host parameters and the torch optimizer of the kind: DeviceGradScaler.step unscales, tests, clips, steps or skips and updates the
    scale through torch ops."""
    t = L.inputs(case)
    init_scale, interval, _ = L.SETUP[case.regime]
    ps = [torch.nn.Parameter(p.clone()) for p in t["params"]]
    opt = L.torch_optimizer(case.kind, ps)
    scaler = trainer.DeviceGradScaler("cpu", init_scale=init_scale, growth_interval=interval)
    ref, yard = L.reference_and_yardstick(case)
    decisions, applied = [], 0
    for sg in L.scaled_grads(case):
        before = scaler.get_scale()
        for p, a in zip(ps, sg):
            p.grad = a.clone()
        kept = [p.detach().clone() for p in ps]
        scaler.step(opt, max_norm=case.max_norm)
        with pytest.raises(RuntimeError, match="one optimizer per iteration"):
            scaler.step(opt, max_norm=case.max_norm)
        scaler.update()
        found = bool(scaler.found_inf.item())
        applied += 0 if found else 1
        if found:
            assert all(torch.equal(p.detach(), k) for p, k in zip(ps, kept))
        decisions.append((before, found, scaler.get_scale(), scaler.get_growth_tracker(), applied))
    assert decisions == ref["decisions"]
    got = dict(p=[p.detach() for p in ps])
    for key in L.STATE[case.kind]:
        got[key] = [opt.state[p][key] for p in ps]
    tols = L.bounds(case, ref, yard)
    for q in got:
        err = L.error(got[q], ref[q], tols[q])
        assert err <= tols[q].a, (q, err, tols[q])


def test_state_dict_is_the_torch_grad_scalers():
    theirs = torch.amp.GradScaler("cpu", init_scale=4096.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=7)
    sd = theirs.state_dict()
    assert set(sd) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    ours = trainer.DeviceGradScaler("cpu")
    assert ours.state_dict() == torch.amp.GradScaler("cpu").state_dict()          # the same defaults
    scale_at, tracker_at, found_at = ours._scale.data_ptr(), ours._growth_tracker.data_ptr(), ours.found_inf.data_ptr()
    ours.load_state_dict(sd)
    assert ours.state_dict() == sd
    assert (ours._scale.data_ptr(), ours._growth_tracker.data_ptr(), ours.found_inf.data_ptr()) == (scale_at, tracker_at, found_at)
    # and back, with a tracker that is not zero
    ours._growth_tracker.fill_(5)
    back = torch.amp.GradScaler("cpu")
    back.load_state_dict(ours.state_dict())
    assert back.state_dict() == ours.state_dict() and back.state_dict()["_growth_tracker"] == 5
    with pytest.raises(RuntimeError):
        ours.load_state_dict({})
    assert float(ours.scale(torch.tensor(2.0))) == 2.0 * 4096.0 and ours.scale(torch.tensor(2.0)).shape == ()


def test_refusals():
    for kw in (dict(growth_factor=1.0), dict(backoff_factor=1.0), dict(growth_interval=0)):
        with pytest.raises(RuntimeError):
            trainer.DeviceGradScaler("cpu", **kw)
    with pytest.raises(RuntimeError, match="DeviceGradScaler"):
        trainer.GraphedTrainStep(None, None, None, None, grad_scaler=torch.amp.GradScaler("cpu"))
    ps = [torch.nn.Parameter(torch.randn(5))]
    opt = trainer.ClipAdamW(ps)
    ps[0].grad = torch.randn(5)
    with pytest.raises(RuntimeError, match="no host form"):                      # a ClipOptimizer over host parameters: refused up front
        trainer.DeviceGradScaler("cpu").step(opt, max_norm=12.0)
    assert opt.steps_done() == 0
    for factory in (nnunet_plugin.make_trainer_class, nnunet_plugin.make_umamba_enc_ss3d_trainer_class):
        with pytest.raises(RuntimeError, match="loss_scaling"):
            factory(FK.nnUNetTrainer, loss_scaling="host")


# ---------------------------------------------------------------------------------------------------------------------
# the plugin factories
# ---------------------------------------------------------------------------------------------------------------------
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


def test_factories_take_loss_scaling(stub_model):
    dj = FK.make_dataset_json(5)
    for scaling in ("torch", "device"):
        for precision in ("fp32", "fp16"):
            cls = nnunet_plugin.make_trainer_class(FK.nnUNetTrainer, precision=precision, loss_scaling=scaling)
            tr = cls(FK.make_plans((32, 32), 2), "2d_bs10", 0, dj, device=torch.device("cpu"))
            tr.initialize()
            # a host trainer scales no loss (the reference creates its GradScaler for a GPU only, B:152)
            assert tr.mlagg_loss_scaling == scaling and tr.mlagg_precision == precision and tr.grad_scaler is None
            assert type(tr.optimizer) is torch.optim.AdamW
    default = nnunet_plugin.make_trainer_class(FK.nnUNetTrainer, precision="fp16")(FK.make_plans((32, 32), 2), "2d_bs10", 0, dj,
                                                                                   device=torch.device("cpu"))
    assert default.mlagg_loss_scaling == "torch"
    strides = [[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2], [2, 2, 2], [1, 2, 2]]
    cls3d = nnunet_plugin.make_umamba_enc_ss3d_trainer_class(FK.nnUNetTrainer, loss_scaling="device")
    tr3d = cls3d(FK.make_plans_3d((96, 160, 160), 2, strides), "3d_fullres", 0, FK.make_dataset_json(14), device=torch.device("cpu"))
    assert tr3d.mlagg_loss_scaling == "device" and tr3d.grad_scaler is None
    assert nnunet_plugin.LOSS_SCALINGS == ("torch", "device")


# ---------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_symbol_exists_and_checks_its_arguments():
    """mlagg_scaled_clip_step_dev rejects NULL pointers, unknown kinds and a growth interval below 1 on the host: no kernel is
    launched, no GPU is needed."""
    lib = _lib.lib()
    C = _lib.CONSTANTS
    assert C["MLAGG_OPT_ADAMW"] == 3 and "mlagg_scaled_clip_step_dev" in _lib.SIGNATURES
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    tail = (0.9, 0.999, 1e-8, 3e-5, 12.0, 2.0, 0.5, 2000, None)
    good = [3, ptr, None, ptr, 1, ptr, ptr, ptr, ptr, ptr, ptr, ptr]
    for i in (1, 3, 5, 6, 7, 8, 9, 10, 11):
        args = list(good)
        args[i] = None
        assert lib.mlagg_scaled_clip_step_dev(*args, *tail) == C["MLAGG_E_NULLPTR"], i
    for kind in (-1, 4):
        assert lib.mlagg_scaled_clip_step_dev(kind, *good[1:], *tail) == C["MLAGG_E_UNSUPPORTED"]
    assert lib.mlagg_scaled_clip_step_dev(1, *good[1:], *tail) == C["MLAGG_E_UNSUPPORTED"]          # amsgrad without its table
    assert lib.mlagg_scaled_clip_step_dev(*good[:4], 0, *good[5:], *tail) == C["MLAGG_E_UNSUPPORTED"]
    assert lib.mlagg_scaled_clip_step_dev(*good, *tail[:7], 0, None) == C["MLAGG_E_UNSUPPORTED"]
