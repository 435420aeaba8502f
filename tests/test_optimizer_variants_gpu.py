"""GPU: K34 (clip + SGD-Nesterov / AdamW-amsgrad / Adam-L2: csrc/optimizer.hip, trainer.ClipSGD, trainer.ClipAdam) against the float64
references of tests/_optimizer_variant_cases.py (tests/test_optimizer_variants_cpu.py shows that the cases are well conditioned and
what defects they catch): every case through the optimizers in both forms with the gradients laid out as the bucketed gradient
exchange lays them out, the C ABI with one misaligned pointer at a time, non-finite gradients, checkpoints handed to the torch
optimizers, the captured step following a learning rate that changes between replays (GraphedTrainStep; the plugin's train_step),
and the 3-D trainer's step tail."""
import copy

import numpy as np
import pytest
import torch

from tests import _optimizer_variant_cases as V
from tests import _step_tail_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(t):
    return t.to(DEV)


def _ours(kind, ps, capturable=False):
    from mlagg_unet_amd import trainer
    if kind == "sgd":
        return trainer.ClipSGD(ps, V.SGD_LR, V.SGD_MOMENTUM, V.WD, capturable=capturable)
    return trainer.ClipAdam(ps, V.ADAM_LR, V.ADAM_BETAS, V.ADAM_EPS, V.WD, amsgrad=kind == "adamw_ams", decoupled=kind == "adamw_ams",
                            capturable=capturable)


def _check(case, got, tols=None):
    ref, yard = V.reference_and_yardstick(case)
    tols = V.bounds(case, ref, yard) if tols is None else tols
    assert set(got) == set(tols), set(got) ^ set(tols)
    failed = []
    for q, tol in tols.items():
        err = V.error(got[q], ref[q], tol)
        print(f"{V.case_id(case)} {q}: error {err:.2e} ({tol.kind} {tol.a:.2e})")
        if not err <= tol.a:                                                      # (a NaN fails too)
            failed.append((q, err, tol))
    assert not failed, failed


def _update_path(kind, p, st):
    """The path of opt_update_kernel<KIND> (optimizer.hip: al = ((p | g | the state pointers the kind has) & 15) == 0)."""
    bits = p.data_ptr() | p.grad.data_ptr()
    for k in V.STATE[kind]:
        bits |= st[k].data_ptr()
    return "vector" if bits % 16 == 0 else "scalar"


# ---------------------------------------------------------------------------------------------------------------------
# the optimizers, eager and capturable
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
@pytest.mark.parametrize("case", V.CASES, ids=[V.case_id(c) for c in V.CASES])
def test_optimizer_variants_match_float64(case, capturable):
    t = V.inputs(case)
    sizes = V.sizes_of(case)
    offs = K.k11_grad_offsets(sizes)
    ps = [torch.nn.Parameter(_dev(p)) for p in t["params"]]
    opt = _ours(case.kind, ps, capturable)
    steps0 = 0
    if t["state0"] is not None:
        sd = opt.state_dict()
        sd["state"] = {i: V.torch_state(case.kind, step, tensors, device=DEV) for i, (step, tensors) in enumerate(t["state0"])}
        opt.load_state_dict(sd)
        steps0 = 0 if case.kind == "sgd" else V.RESUME_STEP                       # torch's SGD state carries no step count
        assert opt.steps_done() == steps0
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
            sumsq_paths.add(K.k11_sumsq_path(p.grad.data_ptr()))
            update_paths.add(_update_path(case.kind, p, opt.state[p]))
    assert sumsq_paths == update_paths == {"vector", "scalar"} == {K.k11_sumsq_path(4 * off) for off in offs}
    assert opt.steps_done() == steps0 + V.STEPS
    got = dict(p=[p.detach() for p in ps])
    for k in V.STATE[case.kind]:
        got[k] = [opt.state[p][k] for p in ps]
    if case.max_norm > 0:
        got["norm"] = norms
    _check(case, got)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.ABI_CASES, ids=[V.case_id(c) for c in V.ABI_CASES])
def test_c_abi_with_one_misaligned_pointer(case):
    """mlagg_optimizer_clip_step on a hand-built table, extra pointer block and work list: each of p, g and the kind's state tensors
    (max_exp_avg_sq included) four bytes off a 16-byte boundary alone sends the update kernel down its scalar path (g: the norm kernel
    too); nothing is written beside the tensors."""
    from mlagg_unet_amd import _lib
    t = V.inputs(case)
    n, kind = case.n, case.kind
    step0, tensors = t["state0"][0]
    named = [("p", t["params"][0]), ("g", t["grads"][0][0])] + list(zip("mvx", tensors))
    assert "".join(k for k, _ in named) == V.ABI_POINTERS[kind]
    bufs, views = {}, {}
    for name, values in named:
        buf = torch.full((n + 8,), 7.0, device=DEV)
        assert buf.data_ptr() % 16 == 0
        lo = 5 if name == case.misaligned else 4
        buf[lo:lo + n] = _dev(values)
        bufs[name], views[name] = (buf, lo), buf[lo:lo + n]
    addr = {k: v.data_ptr() for k, v in views.items()}
    for name in addr:
        assert (addr[name] % 16 != 0) == (name == case.misaligned)
    chunks = K.k11_chunks(n)
    table = _dev(torch.tensor([[addr["p"], addr["g"], addr["m"], addr.get("v", 0), n]], dtype=torch.int64))
    extra = _dev(torch.tensor([addr["x"]], dtype=torch.int64)) if "x" in addr else None
    work = _dev(torch.tensor([(0, c) for c in range(chunks)], dtype=torch.int32))
    sumsq = torch.zeros(1 + chunks, dtype=torch.float64, device=DEV)
    g_before = views["g"].clone()
    lr, b1, b2, eps = (V.SGD_LR, V.SGD_MOMENTUM, 0.0, 0.0) if kind == "sgd" else (V.ADAM_LR,) + V.ADAM_BETAS + (V.ADAM_EPS,)
    _lib.launch("mlagg_optimizer_clip_step", _lib.CONSTANTS[V.ABI_KIND[kind]], table.data_ptr(), None if extra is None else extra.data_ptr(),
                work.data_ptr(), chunks, sumsq.data_ptr(), lr, b1, b2, eps, V.WD, V.ABI_MAX_NORM, step0 + 1)
    torch.cuda.synchronize()
    for name, (buf, lo) in bufs.items():
        assert float((buf[:lo] - 7.0).abs().max()) == 0.0 and float((buf[lo + n:] - 7.0).abs().max()) == 0.0, name
    assert torch.equal(views["g"], g_before)
    got = dict(p=[views["p"]], norm=[sumsq[:1].sqrt().cpu()])
    for key, name in zip(V.STATE[kind], "mvx"):
        got[key] = [views[name]]
    _check(case, got)


# ---------------------------------------------------------------------------------------------------------------------
# non-finite gradients, checkpoints
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_gradient_poisons_every_parameter(kind, bad, capturable):
    """As clip_grad_norm_'s NaN coefficient does: one bad element in one tensor, and no parameter of any tensor stays finite."""
    torch.manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (7, 65537, 4)]
    opt = _ours(kind, ps, capturable)
    for p in ps:
        p.grad = torch.randn_like(p)
    ps[1].grad[12345] = bad
    opt.step(max_norm=12.0)
    for p in ps:
        assert bool(torch.isnan(p).all())


@pytest.mark.parametrize("kind", ["sgd", "adamw_ams"])
def test_checkpoint_loads_into_the_torch_optimizer_and_both_step_alike(kind):
    """Two fused steps, then the state dict goes to torch.optim.SGD / AdamW(amsgrad=True) on a copy of the parameters; the third step of
    both lands within the bounds of the unit case (the same quantities, the same metric, against each other's float64 image)."""
    case = V.OptCase(kind, 0, "unit", 12.0)
    t = V.inputs(case)
    ps = [torch.nn.Parameter(_dev(p)) for p in t["params"]]
    opt = _ours(kind, ps)
    for gs in t["grads"][:2]:
        for p, a in zip(ps, gs):
            p.grad = _dev(a)
        opt.step(max_norm=case.max_norm)
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    theirs = V.torch_optimizer(kind, qs)
    theirs.load_state_dict(copy.deepcopy(opt.state_dict()))
    for q in qs:
        assert set(theirs.state[q]) == set(V.STATE[kind]) | (set() if kind == "sgd" else {"step"})
        if kind != "sgd":
            assert float(theirs.state[q]["step"]) == 2.0
    for p, q, a in zip(ps, qs, t["grads"][2]):
        p.grad, q.grad = _dev(a), _dev(a)
    opt.step(max_norm=case.max_norm)
    torch.nn.utils.clip_grad_norm_(qs, case.max_norm)
    theirs.step()
    # both sides ran three fp32 steps of the unit case: each is within the case's bounds of the float64 reference
    ref, yard = V.reference_and_yardstick(case)
    tols = {q: tol for q, tol in V.bounds(case, ref, yard).items() if q != "norm"}
    both = {}
    for who, params, o in (("fused", ps, opt), ("torch", qs, theirs)):
        got = dict(p=[p.detach() for p in params])
        for k in V.STATE[kind]:
            got[k] = [o.state[p][k] for p in params]
        print(who)
        _check(case, got, tols)
        both[who] = got
    for q, tol in tols.items():                                                   # and of each other
        err = V.error(both["fused"][q], [x.detach().cpu() for x in both["torch"][q]], tol)
        print(f"fused against torch {q}: {err:.2e} ({tol.kind} {tol.a:.2e})")
        assert err <= tol.a, (q, err, tol)


# ---------------------------------------------------------------------------------------------------------------------
# the captured step follows the schedule
# ---------------------------------------------------------------------------------------------------------------------
def _graph_twins(make):
    from mlagg_unet_amd import model
    torch.manual_seed(0)
    net = model.build_network_architecture((64, 64), 1, 14, True, "B").cuda().eval()      # eval: no DropPath draws to align
    twin = copy.deepcopy(net)
    return net, make(net.parameters(), True), twin, make(twin.parameters(), False)


@pytest.mark.parametrize("kind", ["sgd", "adamw_ams"])
def test_graph_replay_follows_poly_lr_like_the_eager_twin(kind):
    """GraphedTrainStep with the capturable optimizer against a twin driven by eager train_step with the launch-argument form, the
    learning rate stepped by PolyLRSchedule between the replays: parameters and state tensors agree bit for bit in deterministic
    mode.  torch.optim.SGD cannot do this: its learning rate is an argument of the captured launches."""
    from mlagg_unet_amd import trainer
    warmup, epochs = 3, 10
    # SGD at the base trainer's 1e-2; AdamW-amsgrad at the 1e-3 of nnUNetTrainerAdam1en3
    lr0 = 1e-2 if kind == "sgd" else 1e-3
    make = (lambda ps, c: trainer.ClipSGD(ps, lr0, capturable=c)) if kind == "sgd" else \
        (lambda ps, c: trainer.ClipAdam(ps, lr0, amsgrad=True, decoupled=True, capturable=c))
    trainer.set_deterministic(True)
    try:
        net, opt, twin, opt_t = _graph_twins(make)
        sched, sched_t = trainer.PolyLRSchedule(opt, lr0, epochs), trainer.PolyLRSchedule(opt_t, lr0, epochs)
        batches = [trainer.synthetic_batch(2, 1, 64, 64, 14, seed=40 + i, device="cuda") for i in range(3)]
        graphed = trainer.GraphedTrainStep(net, opt, *batches[0], batch_dice=True, warmup=warmup)
        for _ in range(warmup):
            trainer.train_step(twin, opt_t, *batches[0])
        seen = set()
        for epoch, (data, target) in enumerate(batches, start=1):
            sched.step(epoch)
            sched_t.step(epoch)
            lr = opt.param_groups[0]["lr"]
            assert type(lr) is float and lr == lr0 * (1 - epoch / epochs) ** 0.9 == opt_t.param_groups[0]["lr"]
            seen.add(lr)
            got = float(graphed(data, target))
            want = float(trainer.train_step(twin, opt_t, data, target))
            assert np.isfinite(got) and abs(got - want) < 2e-4 * max(1.0, abs(want)), (epoch, got, want)
        assert len(seen) == 3 and lr0 not in seen                                 # three replays, three learning rates, none the captured one
        assert opt.steps_done() == opt_t.steps_done() == warmup + 3
        n = 0
        for (k, p), q in zip(net.named_parameters(), twin.parameters()):
            assert bool(torch.isfinite(p).all()) and torch.equal(p, q), k
            assert bool(opt.state[p]) == bool(opt_t.state[q]), k
            for name in opt._STATE if opt.state[p] else ():
                assert torch.equal(opt.state[p][name], opt_t.state[q][name]), (k, name)
                n += 1
        assert n > 500 * len(opt._STATE)
    finally:
        trainer.set_deterministic(False)


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_plugin_replays_the_optimizer_variant_as_a_hipgraph_under_poly_lr(name):
    """make_trainer_class(optimizer=...) on the device, behind the reference loop (tests/fake_nnunet.py): the class builds the capturable
    fused optimizer + PolyLR, takes three eager steps, then captures the step and replays it.  Deterministic mode, DropPath off: with the
    schedule stepped before every batch, five steps end on the losses, parameters and state tensors of five eager
    ``trainer.train_step`` calls on a twin with the launch-argument form of the same optimizer."""
    import fake_nnunet as FK
    from mlagg_unet_amd import nnunet_plugin, trainer
    from oracle import mlagg_oracle as O
    assert nnunet_plugin.PLUGIN_GRAPH
    want_cls = trainer.ClipSGD if name == "sgd" else trainer.ClipAdam
    trainer.set_deterministic(True)
    try:
        cls = nnunet_plugin.make_trainer_class(FK.nnUNetTrainer, optimizer=name)
        tr = cls(FK.make_plans((64, 64), 2), "2d_bs10", 0, FK.make_dataset_json(14), device=torch.device("cuda"))
        assert tr.initial_lr == 1e-2
        if name == "adam":
            tr.initial_lr = 1e-3                                                  # as nnUNetTrainerAdam1en3 sets it in its constructor
        tr.initialize()
        O.deterministic_fill_(tr.network.state_dict())
        tr.network.eval()
        assert tr.mlagg_optimizer == name and type(tr.optimizer) is want_cls and tr.optimizer.capturable
        assert type(tr.lr_scheduler) is trainer.PolyLRSchedule and tr.lr_scheduler.initial_lr == tr.initial_lr
        twin = copy.deepcopy(tr.network)
        twin_opt, twin_sched = trainer.configure_optimizers(twin, tr.initial_lr, tr.weight_decay, optimizer=name, num_epochs=tr.num_epochs)
        assert type(twin_opt) is want_cls and not twin_opt.capturable
        seen = set()
        for it in range(5):
            data, target = trainer.synthetic_batch(2, 1, 64, 64, 14, seed=700 + it)
            tr.lr_scheduler.step(40 * it)
            twin_sched.step(40 * it)
            seen.add(tr.optimizer.param_groups[0]["lr"])
            got = tr.train_step({"data": data, "target": target})
            want = trainer.train_step(twin, twin_opt, data.cuda(), [t.cuda() for t in target], batch_dice=True)
            assert np.isfinite(got["loss"]) and float(got["loss"]) == float(want), it
            assert (tr._graphed is not None) == (it >= 3), (it, tr._graph_failed)
        assert len(seen) == 5 and tr.optimizer.steps_done() == twin_opt.steps_done() == 5 and tr._graph_failed is None
        for (k, p), q in zip(tr.network.named_parameters(), twin.parameters()):
            assert torch.equal(p, q), k
            for key in tr.optimizer._STATE if tr.optimizer.state[p] else ():
                assert torch.equal(tr.optimizer.state[p][key], twin_opt.state[q][key]), (k, key)
    finally:
        trainer.set_deterministic(False)


# ---------------------------------------------------------------------------------------------------------------------
# the 3-D trainer's step tail
# ---------------------------------------------------------------------------------------------------------------------
def _tail_state(net, opt):
    """(parameter, momentum buffer) of every parameter the optimizer has stepped, in module order."""
    return [(p, opt.state[p]["momentum_buffer"]) for p in net.parameters() if opt.state.get(p)]


def test_3d_train_steps_with_clip_sgd_match_clip_grad_norm_and_torch_sgd():
    """The smallest 3-D network tests/test_umamba3d_gpu.py trains: three train_steps with ClipSGD against the same three with
    clip_grad_norm_ + torch.optim.SGD on a deep copy, in deterministic mode, within 1e-4, that file's loss tolerance.

    Losses: the two networks run free for three steps and every pair of losses is within 1e-4.

    Parameters (and momentum buffers): within 1e-4 after EACH of three steps, every step taken from the same parameters and buffers:
    after the comparison torch's are copied into ClipSGD's network.  That compares three step tails and leaves out how this network
    (stem convolutions in front of an InstanceNorm, |w| <= 0.05) amplifies a rounding difference from one step to the next: running
    free, ClipSGD and torch.optim.SGD were 1.5e-8 apart after the first step on the MI355X (one ulp of a weight between 1/8 and 1/4), 2.6e-5
    after the second and 4.2e-4 after the third, and torch's own step tail evaluated in another fp32 order drifts from torch.optim.SGD
    by as much; a free-running 1e-4 on the parameters measures the network's conditioning, not the optimizer.  The free-running
    figures are printed.

    From identical inputs the two tails differ by rounding alone, and that is asserted too, with eps = 2^-23 and B a bound of every
    intermediate of the tail (|buf'| + 2 |buf|, from torch's buffers before and after the step; g' = buf' - mu buf):
      buffers     g' = coef g + wd p and buf' = mu buf + g' are four roundings at most on either side (the kernel contracts two of
                  them) and a clip coefficient from an fp32 norm on torch's side: 8 eps B
      parameters  the last rounding of p' on either side, eps max|p'|, and the update lr (g' + mu buf'), whose terms are below 2 lr B,
                  with the errors above and three roundings of its own: 16 eps lr B.
    Measured: parameters 1.5e-8 / 7.5e-9 / 1.5e-8 against bounds of 8e-7, buffers 1.5e-8 each against 2e-7 to 6e-7."""
    from mlagg_unet_amd import model3d, ops, trainer
    from tests.test_umamba3d_gpu import CFG, _net
    dev = torch.device(DEV)
    lr, mu, wd, eps = 1e-2, 0.99, 3e-5, 2.0 ** -23
    trainer.set_deterministic(True)
    try:
        start = _net(dev).train()
        data, target = model3d.synthetic_batch_3d(CFG["batch"], CFG["in_ch"], CFG["size"], CFG["strides"], CFG["n_cls"], seed=5, device=dev)

        def pair():
            net, twin = copy.deepcopy(start), copy.deepcopy(start)
            opt = trainer.ClipSGD(net.parameters(), lr, mu, wd)
            opt_t = torch.optim.SGD(twin.parameters(), lr, weight_decay=wd, momentum=mu, nesterov=True)
            assert isinstance(opt, trainer.ClipOptimizer) and not isinstance(opt_t, trainer.ClipOptimizer)
            return net, opt, twin, opt_t

        # running free: the losses
        net, opt, twin, opt_t = pair()
        got, want = [], []
        for k in range(3):
            got.append(float(trainer.train_step(net, opt, data, target, batch_dice=False)))
            want.append(float(trainer.train_step(twin, opt_t, data, target, batch_dice=False)))
            with torch.no_grad():
                drift = max(float((p - q).abs().max()) for p, q in zip(net.parameters(), twin.parameters()))
            print(f"free step {k + 1}: losses {got[-1]:.7f} {want[-1]:.7f}, largest parameter difference {drift:.3e}")
        assert all(np.isfinite(got)) and got[-1] < got[0], got
        for a, b in zip(got, want):
            assert abs(a - b) < 1e-4, (got, want)
        assert opt.steps_done() == 3

        # step by step from the same state: parameters and momentum buffers
        net, opt, twin, opt_t = pair()
        old = None
        for k in range(3):
            a = float(trainer.train_step(net, opt, data, target, batch_dice=False))
            b = float(trainer.train_step(twin, opt_t, data, target, batch_dice=False))
            assert abs(a - b) < 1e-4, (k, a, b)
            ours, theirs = _tail_state(net, opt), _tail_state(twin, opt_t)
            assert len(ours) == len(theirs) > 50
            with torch.no_grad():
                dp = max(float((p - q).abs().max()) for (p, _), (q, _) in zip(ours, theirs))
                db = max(float((x - y).abs().max()) for (_, x), (_, y) in zip(ours, theirs))
                pmax = max(float(q.abs().max()) for q, _ in theirs)
                big = max(float(y.abs().max()) for _, y in theirs) + 2.0 * (0.0 if old is None else max(float(y.abs().max()) for y in old))
                bound_b, bound_p = 8 * eps * big, eps * pmax + 16 * eps * lr * big
                print(f"step {k + 1} from the same state: parameters {dp:.3e} (bound {bound_p:.3e}), buffers {db:.3e} (bound {bound_b:.3e})")
                assert dp <= 1e-4 and db <= 1e-4, (k, dp, db)
                assert dp <= bound_p and db <= bound_b, (k, dp, bound_p, db, bound_b)
                old = [y.clone() for _, y in theirs]
                for (p, x), (q, y) in zip(ours, theirs):
                    p.copy_(q)
                    x.copy_(y)
            ops.invalidate_weight_images()
        assert opt.steps_done() == 3
    finally:
        trainer.set_deterministic(False)
