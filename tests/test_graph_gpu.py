"""GPU: the whole train step captured into one hipGraph (trainer.GraphedTrainStep, `bench.py --graph`) replays the same
optimisation trajectory as eager steps: every C-ABI entry point launches on the capturing stream, takes its workspaces from
torch's graph-private pool and neither allocates nor synchronises (include/mlagg_hip.h).

And the SEAMS between replays and eager work in one process (the trainer plugin trains by replay and validates eagerly): a replay
rewrites parameters, moments, the step counter and reads the learning rate through raw device pointers, changes no version counter
and runs no host code, so every host-side cache (model._Stack buffers, ops.WeightImageSet, ClipAdamW's pointer tables, the device
copy of the learning rate) has to be told.  The reference of every comparison is a twin -- a deepcopy of the network taken before
any step, driven by eager ``trainer.train_step`` with the launch-argument ClipAdamW -- or, for forwards, a freshly built network
with the replayed network's parameters; in deterministic mode both agree with the object under test bit for bit."""
import copy

import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import model, ops, trainer
from _trajectory import assert_same_trajectory

pytestmark = pytest.mark.gpu
WARMUP = 3


def test_graph_replay_follows_the_eager_trajectory():
    torch.manual_seed(0)
    net = model.build_network_architecture((64, 64), 1, 14, True, "B").cuda().eval()      # eval: no DropPath draws to align
    twin = copy.deepcopy(net)
    opt, _ = trainer.configure_optimizers(net, capturable=True)
    opt_t, _ = trainer.configure_optimizers(twin)                                          # the eager, launch-argument form of K11
    batches = [trainer.synthetic_batch(2, 1, 64, 64, 14, seed=40 + i, device="cuda") for i in range(3)]
    # the graph's own warm-up steps (3, on its first batch) are part of the trajectory: mirror them on the twin
    graphed = trainer.GraphedTrainStep(net, opt, *batches[0], batch_dice=True, warmup=3)
    for _ in range(3):
        trainer.train_step(twin, opt_t, *batches[0])
    for data, target in batches:
        got = float(graphed(data, target))
        want = float(trainer.train_step(twin, opt_t, data, target))
        assert abs(got - want) < 2e-4 * max(1.0, abs(want)), (got, want)
    assert_same_trajectory(net, twin, steps=6, lr=5e-4)


# ------------------------------------------------------------------------------------------------
# eager work interleaved with replays
# ------------------------------------------------------------------------------------------------
def _batch(seed, batch=2):
    return trainer.synthetic_batch(batch, 1, 64, 64, 14, seed=seed, device="cuda")


def _captured(first):
    """(net, opt, graphed, twin, twin_opt): the step captured on batch ``first`` after WARMUP eager steps, mirrored on the twin."""
    torch.manual_seed(0)
    net = model.build_network_architecture((64, 64), 1, 14, True, "B").cuda().eval()      # eval: no DropPath draws to align
    twin = copy.deepcopy(net)
    opt, _ = trainer.configure_optimizers(net, capturable=True)
    opt_t, _ = trainer.configure_optimizers(twin)
    graphed = trainer.GraphedTrainStep(net, opt, *first, batch_dice=True, warmup=WARMUP)
    for _ in range(WARMUP):
        trainer.train_step(twin, opt_t, *first)
    return net, opt, graphed, twin, opt_t


def _assert_same_parameters_and_moments(net, opt, twin, opt_t):
    for (k, a), b in zip(net.state_dict().items(), twin.state_dict().values()):
        assert torch.equal(a, b), k
    n = 0
    for (k, p), q in zip(net.named_parameters(), twin.parameters()):
        assert bool(opt.state[p]) == bool(opt_t.state[q]), k
        if opt.state[p]:
            for name in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opt.state[p][name], opt_t.state[q][name]), (k, name)
            n += 1
    assert n > 500                                                 # every trainable parameter of the network has moments


def _fresh_copy(net):
    """A network with the parameters ``net`` has NOW whose stacked-weight buffers and weight images were never built.  Not a
    deepcopy: ``_Stack.sig`` and ``WeightImageSet.built`` are plain attributes and a deepcopy carries them over."""
    fresh = model.build_network_architecture((64, 64), 1, 14, True, "B").cuda().eval()
    fresh.load_state_dict(net.state_dict())
    assert fresh._stacks() and all(st.sig is None and st.buf is None for st in fresh._stacks())
    assert fresh._images.built is None and not fresh._images.tensors
    return fresh


@pytest.mark.parametrize("x3_min_rows", [128, None], ids=["weight_images", "library_gemm"])
def test_eager_forward_after_replays_sees_the_current_parameters(x3_min_rows, monkeypatch):
    """Capture; one eager forward (stacks and images current, their signatures stored); two replays; an eager forward.  Its logits
    are those of a freshly built network with the same parameters.  Tolerance: none -- the run-to-run difference of the reference
    is asserted to be zero HERE (two forwards of the fresh network on one input: the first builds every weight image on the fly,
    the second in the one-launch table build; deterministic mode), so the comparison is ``torch.equal``.
    Teeth: the logits of a copy taken one replay EARLIER differ from the reference's on every head by more than 1e-6 of that
    head's largest logit.  With a tolerance of zero any floor is "100 x the tolerance"; this one is 16 ulp of the largest logit
    (fp32: 6e-8 relative), so rounding cannot clear it, and three orders below what one step does (AdamW moves every weight by
    about lr = 5e-4, the logits by about that much relative to their size), so a forward that is one step behind cannot pass.
    ``weight_images``: K5 on weight images from 128 rows up, so that both caches serve the stage-0 / 1 projections at this size;
    ``library_gemm``: the default threshold, the stacks alone."""
    if x3_min_rows is not None:
        monkeypatch.setattr(ops, "X3_MIN_ROWS", x3_min_rows)
    trainer.set_deterministic(True)
    try:
        net, _, graphed, _, _ = _captured(_batch(40))
        x = _batch(77)[0]
        with torch.no_grad():
            net(x)
        assert all(st.sig is not None for st in net._stacks())
        if x3_min_rows is not None:
            assert len(net._images.tensors) > 0 and net._images.built is not None
        graphed(*_batch(41))
        behind = _fresh_copy(net)                                  # the parameters one replay before the last
        graphed(*_batch(42))
        fresh = _fresh_copy(net)
        with torch.no_grad():
            got, want, again, old = net(x), fresh(x), fresh(x), behind(x)
        assert len(got) == len(want) == 5
        for lvl, (g, w, a, o) in enumerate(zip(got, want, again, old)):
            scale = float(w.abs().max())
            print(f"head {lvl}: max|logit| {scale:.4f}  fresh run-to-run {float((w - a).abs().max()):.3e}  "
                  f"replayed - fresh {float((g - w).abs().max()):.3e}  one step behind - fresh {float((o - w).abs().max()):.3e}")
        for lvl, (g, w, a, o) in enumerate(zip(got, want, again, old)):
            assert torch.equal(w, a), lvl                          # the reference reproduces itself: no tolerance needed
            assert float((o - w).abs().max()) > 1e-6 * float(w.abs().max()), lvl    # teeth: one step behind is visible on this head
            assert torch.equal(g, w), lvl
    finally:
        trainer.set_deterministic(False)


def test_replay_after_an_eager_step_uses_its_own_gradients():
    """Replay, an eager ``train_step`` with the SAME capturable optimizer (a batch of another geometry, as the plugin's fall-back),
    two replays: parameters and both moments equal the twin's.  The eager step uploads a pointer table with its own gradient
    addresses; the captured step must keep reading the addresses its backward writes."""
    trainer.set_deterministic(True)
    try:
        net, opt, graphed, twin, opt_t = _captured(_batch(40))
        graphed(*_batch(41))
        trainer.train_step(twin, opt_t, *_batch(41))
        other = _batch(50, batch=1)
        trainer.train_step(net, opt, *other)
        trainer.train_step(twin, opt_t, *other)
        for seed in (42, 43):
            got = graphed(*_batch(seed))
            want = trainer.train_step(twin, opt_t, *_batch(seed))
            assert float(got) == float(want), seed
        _assert_same_parameters_and_moments(net, opt, twin, opt_t)
        assert opt.steps_done() == opt_t.steps_done() == 4 + WARMUP
    finally:
        trainer.set_deterministic(False)


def test_load_state_dict_between_replays_keeps_the_graph_valid():
    """Capture, two replays, ``load_state_dict`` of the optimizer's own (deep-copied) state, two more replays == four eager steps of
    the twin with the same round trip.  The graph holds the addresses of the moment tensors, of the work list and of the pointer
    table: all of them must survive the load (checked BEFORE the next replay, which would otherwise write through stale ones)."""
    trainer.set_deterministic(True)
    try:
        net, opt, graphed, twin, opt_t = _captured(_batch(40))
        for seed in (41, 42):
            graphed(*_batch(seed))
            trainer.train_step(twin, opt_t, *_batch(seed))

        def addresses():
            out = {(id(p), name): st[name].data_ptr() for p, st in opt.state.items() if st for name in ("exp_avg", "exp_avg_sq")}
            out.update({("work", i): w.data_ptr() for i, (w, _) in enumerate(opt._work.values())})
            out.update({("table", i, j): t.data_ptr() for i, pair in enumerate(opt._tables.values()) for j, t in enumerate(pair)})
            return out
        before = addresses()
        opt.load_state_dict(copy.deepcopy(opt.state_dict()))
        opt_t.load_state_dict(copy.deepcopy(opt_t.state_dict()))
        assert len(before) > 1000 and addresses() == before
        assert opt.steps_done() == opt_t.steps_done() == 2 + WARMUP
        for seed in (43, 44):
            got = graphed(*_batch(seed))
            want = trainer.train_step(twin, opt_t, *_batch(seed))
            assert float(got) == float(want), seed
        _assert_same_parameters_and_moments(net, opt, twin, opt_t)
        assert opt.steps_done() == opt_t.steps_done() == 4 + WARMUP
    finally:
        trainer.set_deterministic(False)


def test_learning_rate_assigned_on_the_host_reaches_the_graph():
    """``param_groups[0]["lr"]`` is a Python float in the capturable form too, and what a training loop or the schedule assigns to it
    between replays governs the next replay: with lr 0 the step and the decay are both zero, so no parameter moves (the moments and
    the step counter still advance, as the twin's do); with the schedule's value restored the parameters land on the twin's."""
    trainer.set_deterministic(True)
    try:
        net, opt, graphed, twin, opt_t = _captured(_batch(40))
        sched, sched_t = (trainer.CosineLRSchedule(o, t_initial=500, lr_min=1e-6, warmup_t=10, warmup_lr_init=1e-4) for o in (opt, opt_t))
        assert type(opt.param_groups[0]["lr"]) is float
        graphed(*_batch(41))
        trainer.train_step(twin, opt_t, *_batch(41))
        before = [p.detach().clone() for p in net.parameters()]
        for o in (opt, opt_t):
            o.param_groups[0]["lr"] = 0.0
        graphed(*_batch(42))
        trainer.train_step(twin, opt_t, *_batch(42))
        for (k, p), b in zip(net.named_parameters(), before):
            assert torch.equal(p, b), k
        sched.step(3)
        sched_t.step(3)
        assert opt.param_groups[0]["lr"] == sched.lr_at(3, 5e-4) == 1e-4 + 3 * (5e-4 - 1e-4) / 10
        graphed(*_batch(43))
        trainer.train_step(twin, opt_t, *_batch(43))
        assert any(not torch.equal(p, b) for p, b in zip(net.parameters(), before))
        _assert_same_parameters_and_moments(net, opt, twin, opt_t)
        assert not any(torch.is_tensor(v) for g in opt.state_dict()["param_groups"] for v in g.values())
    finally:
        trainer.set_deterministic(False)
