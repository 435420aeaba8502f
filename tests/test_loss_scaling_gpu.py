"""GPU: K35 (fp16 loss scaling fused into the clip + update step: csrc/optimizer.hip, trainer.DeviceGradScaler) against the float64
reference of tests/_loss_scale_cases.py (tests/test_loss_scaling_cpu.py shows that the cases are well conditioned and what defects
they catch): every case through DeviceGradScaler.step with the gradients laid out as the bucketed gradient exchange lays them out,
the C ABI with one misaligned pointer at a time, the unscaled entry points against a scaled call with scale 1, the captured step
against the eager one and against torch.amp.GradScaler, the fp16 network, and the plugin."""
import copy
import io

import numpy as np
import pytest
import torch

from tests import _loss_scale_cases as L
from tests import _step_tail_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(t):
    return t.to(DEV)


def _ours(kind, ps, capturable=True):
    from mlagg_unet_amd import trainer
    if kind == "adamw":
        return trainer.ClipAdamW(ps, K.K11_LR, K.K11_BETAS, K.K11_EPS, K.K11_WD, capturable=capturable)
    from tests.test_optimizer_variants_gpu import _ours as variant
    return variant(kind, ps, capturable)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _check(case, got):
    ref, yard = L.reference_and_yardstick(case)
    tols = L.bounds(case, ref, yard)
    assert set(got) == set(tols), set(got) ^ set(tols)
    failed = []
    for q, tol in tols.items():
        err = L.error(got[q], ref[q], tol)
        print(f"{L.case_id(case)} {q}: error {err:.2e} ({tol.kind} {tol.a:.2e})")
        if not err <= tol.a:                                                      # (a NaN fails too)
            failed.append((q, err, tol))
    assert not failed, failed


# ---------------------------------------------------------------------------------------------------------------------
# the cases through DeviceGradScaler.step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.CASES, ids=[L.case_id(c) for c in L.CASES])
def test_cases_match_float64_and_the_reference_decisions(case):
    from mlagg_unet_amd import trainer
    t = L.inputs(case)
    sizes = L.sizes_of(case)
    offs = K.k11_grad_offsets(sizes)
    init_scale, interval, _ = L.SETUP[case.regime]
    ref, _ = L.reference_and_yardstick(case)
    ps = [torch.nn.Parameter(_dev(p)) for p in t["params"]]
    opt = _ours(case.kind, ps)
    scaler = trainer.DeviceGradScaler(DEV, init_scale=init_scale, growth_interval=interval)
    norms, decisions, paths = [], [], set()
    for sg, want in zip(L.scaled_grads(case), ref["decisions"]):
        flat = _dev(torch.cat(sg))                                                # one flat buffer, every p.grad a view at a running offset
        assert flat.data_ptr() % 16 == 0
        for p, off in zip(ps, offs):
            p.grad = flat[off:off + p.numel()].view_as(p)
            paths.add(K.k11_sumsq_path(p.grad.data_ptr()))
        before, scale_before, done_before = _bits(flat).clone(), scaler.get_scale(), opt.steps_done()
        kept = [[p.detach().clone()] + [opt.state[p][k].clone() for k in L.STATE[case.kind] if opt.state[p]] for p in ps]
        scaler.step(opt, max_norm=case.max_norm)
        scaler.update()
        assert torch.equal(_bits(flat), before)                                   # the gradients stay scaled and unclipped, bit for bit
        found = bool(scaler.found_inf.item())
        assert found == want[1]
        if found:                                                                 # a skipped step: nothing written, nothing counted
            assert opt.steps_done() == done_before
            for p, old in zip(ps, kept):
                now = [p.detach()] + [opt.state[p][k] for k in L.STATE[case.kind]][:len(old) - 1]
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(now, old))
                assert all(float(opt.state[p][k].abs().max()) == 0.0 for k in L.STATE[case.kind][len(old) - 1:])
        elif case.max_norm > 0:
            norms.append(opt.grad_norm().cpu())
        decisions.append((scale_before, found, scaler.get_scale(), scaler.get_growth_tracker(), opt.steps_done()))
    assert decisions == ref["decisions"]
    assert paths == {"vector", "scalar"}
    got = dict(p=[p.detach() for p in ps])
    for k in L.STATE[case.kind]:
        got[k] = [opt.state[p][k] for p in ps]
    if case.max_norm > 0:
        got["norm"] = norms
    _check(case, got)


def test_a_clip_optimizer_must_be_capturable():
    from mlagg_unet_amd import trainer
    ps = [torch.nn.Parameter(torch.randn(5, device=DEV))]
    ps[0].grad = torch.randn(5, device=DEV)
    with pytest.raises(RuntimeError, match="capturable=True"):
        trainer.DeviceGradScaler(DEV).step(trainer.ClipSGD(ps), max_norm=12.0)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _abi_buffers(case, scale):
    """The one-tensor buffers of an ABI case -- p, the SCALED g and the kind's state tensors, each inside a guarded buffer, the
    misaligned one four bytes off a 16-byte boundary -- and the table, extra block, work list and scratch of the call."""
    t = L.inputs(case)
    n, kind = case.n, case.kind
    step0, tensors = t["state0"][0]
    named = [("p", t["params"][0]), ("g", (t["grads"][0][0] * scale).float())] + list(zip("mvx", tensors))
    assert "".join(k for k, _ in named) == L.ABI_POINTERS[kind]
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
    return step0, bufs, views, table, extra, work, sumsq


@pytest.mark.parametrize("case", L.ABI_CASES, ids=[L.case_id(c) for c in L.ABI_CASES])
def test_c_abi_with_one_misaligned_pointer(case):
    """mlagg_scaled_clip_step_dev on a hand-built table: each of p, g and the kind's state tensors four bytes off a 16-byte boundary
    alone sends the update kernel down its scalar path (g: the norm kernel too); nothing is written beside the tensors, and the
    device state moves as torch.amp.GradScaler's would."""
    from mlagg_unet_amd import _lib
    n, kind = case.n, case.kind
    scale0 = L.SETUP["abi"][0]
    step0, bufs, views, table, extra, work, sumsq = _abi_buffers(case, scale0)
    lr, b1, b2, eps, wd = L.hyper(kind)
    lr_dev = torch.full((1,), lr, dtype=torch.float32, device=DEV)
    step_dev = torch.full((1,), step0, dtype=torch.int32, device=DEV)
    scale = torch.full((1,), scale0, dtype=torch.float32, device=DEV)
    tracker = torch.zeros(1, dtype=torch.int32, device=DEV)
    found, mult = torch.full((1,), 5.0, device=DEV), torch.zeros(1, device=DEV)
    g_before = views["g"].clone()
    _lib.launch("mlagg_scaled_clip_step_dev", _lib.CONSTANTS[L.ABI_KIND[kind]], table.data_ptr(), None if extra is None else extra.data_ptr(),
                work.data_ptr(), work.shape[0], sumsq.data_ptr(), lr_dev.data_ptr(), step_dev.data_ptr(), scale.data_ptr(),
                tracker.data_ptr(), found.data_ptr(), mult.data_ptr(), b1, b2, eps, wd, L.ABI_MAX_NORM, L.GROWTH, L.BACKOFF, 2000)
    torch.cuda.synchronize()
    for name, (buf, lo) in bufs.items():
        assert float((buf[:lo] - 7.0).abs().max()) == 0.0 and float((buf[lo + n:] - 7.0).abs().max()) == 0.0, name
    assert torch.equal(views["g"], g_before)
    ref, _ = L.reference_and_yardstick(case)
    assert [(scale0, bool(found.item()), float(scale), int(tracker), int(step_dev) - step0)] == ref["decisions"]
    norm = sumsq[:1].sqrt().float()
    want_mult = float(torch.tensor(1.0 / scale0) * torch.clamp(L.ABI_MAX_NORM / (norm + 1e-6), max=1.0))
    assert abs(float(mult) - want_mult) <= 2.0 ** -22 * want_mult                 # (1 / scale) * clip coefficient, two fp32 roundings
    got = dict(p=[views["p"]], norm=[norm.cpu()])
    for key, name in zip(L.STATE[kind], "mvx"):
        got[key] = [views[name]]
    _check(case, got)


# ---------------------------------------------------------------------------------------------------------------------
# the unscaled entry points compute what a scaled call with scale 1 computes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", L.MAX_NORMS)
@pytest.mark.parametrize("kind", L.KINDS)
def test_scale_one_equals_the_unscaled_step_bit_for_bit(kind, max_norm):
    """Multiplication by exactly 1: K11's / K34's own entry points (device form) and the scaled entry point with scale 1.0 leave the same
    parameters, state tensors and squared norm, bit for bit, over three steps on K11's sizes with a misaligning lead element."""
    from mlagg_unet_amd import trainer
    case = L.LSCase(kind, 1, "unit", max_norm)
    t = L.inputs(case)
    sizes = L.sizes_of(case)
    offs = K.k11_grad_offsets(sizes)
    ps = [torch.nn.Parameter(_dev(p)) for p in t["params"]]
    qs = [torch.nn.Parameter(_dev(p)) for p in t["params"]]
    plain, scaled = _ours(kind, ps), _ours(kind, qs)
    scaler = trainer.DeviceGradScaler(DEV, init_scale=1.0)
    for gs in t["grads"]:
        flat = _dev(torch.cat(gs))
        for p, q, off in zip(ps, qs, offs):
            p.grad = flat[off:off + p.numel()].view_as(p)
            q.grad = p.grad
        plain.step(max_norm=max_norm)
        scaler.step(scaled, max_norm=max_norm)
        scaler.update()
        assert not bool(scaler.found_inf.item())
        if max_norm > 0:
            assert torch.equal(plain._sumsq, scaled._sumsq)
        for p, q in zip(ps, qs):
            assert torch.equal(p, q)
            for k in L.STATE[kind]:
                assert torch.equal(plain.state[p][k], scaled.state[q][k]), k
    assert plain.steps_done() == scaled.steps_done() == 3 and scaler.get_scale() == 1.0 and scaler.get_growth_tracker() == 3


# ---------------------------------------------------------------------------------------------------------------------
# replay
# ---------------------------------------------------------------------------------------------------------------------
class TwoLayer(torch.nn.Module):
    """One parameter above 65536 elements (two chunks), the others below."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(300, 300)
        self.b = torch.nn.Linear(300, 10)

    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))


def _two_layer_loss(output, target):
    return ((output - target[0]) ** 2).sum()


def _snapshot(net, opt, scaler):
    tensors = [p.detach().clone() for p in net.parameters()]
    for p in net.parameters():
        tensors += [v.clone() for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v) and v.is_cuda]
    return tensors, scaler.get_scale(), scaler.get_growth_tracker(), opt.steps_done()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_graph_replays_equal_the_eager_sequence_and_torchs_decisions(kind):
    """Eight steps on fixed batches from init_scale 2^126 with growth_interval 2: the first steps overflow (ordinary inf arithmetic in
    the scaled backward) and are skipped, later ones apply and the scale grows again.  (a) GraphedTrainStep with a DeviceGradScaler --
    two warm-up steps, then replays with one eager step in between -- equals the eager train_step sequence of a twin bit for bit in
    parameters, state, scale, tracker and steps_done().  (b) torch.amp.GradScaler("cuda") + clip_grad_norm_ + the torch optimizer on a
    third copy takes the identical skip pattern and scale sequence; its parameters agree within K11's floor for p, 2e-6 absolute:
    forward and backward are the same torch kernels on all copies, the tails differ by the rounding of (g inv) coef against
    g (inv coef) -- one ulp of g, 6e-8 relative -- which lr 1e-3 (SGD, clipped norm 12) / 5e-4 (AdamW) carry into parameters of magnitude
    below 0.1 at 1e-9 per step."""
    from mlagg_unet_amd import trainer
    torch.manual_seed(11)
    start = TwoLayer().to(DEV)
    g = torch.Generator().manual_seed(12)
    batches = [(torch.randn(16, 300, generator=g).to(DEV), [torch.randn(16, 10, generator=g).to(DEV)]) for _ in range(8)]
    kw = dict(init_scale=2.0 ** 126, growth_interval=2)

    def make(net, capturable=True):
        if kind == "sgd":
            return trainer.ClipSGD(net.parameters(), 1e-3, capturable=capturable)
        return trainer.ClipAdamW(net.parameters(), capturable=capturable)

    net, twin, third = copy.deepcopy(start), copy.deepcopy(start), copy.deepcopy(start)
    opt, opt_t = make(net), make(twin)
    scaler, scaler_t = trainer.DeviceGradScaler(DEV, **kw), trainer.DeviceGradScaler(DEV, **kw)
    opt_3 = torch.optim.SGD(third.parameters(), 1e-3, momentum=0.99, weight_decay=3e-5, nesterov=True) if kind == "sgd" else \
        torch.optim.AdamW(third.parameters(), 5e-4, eps=1e-4, weight_decay=3e-5)
    scaler_3 = torch.amp.GradScaler("cuda", **kw)

    graphed = trainer.GraphedTrainStep(net, opt, *batches[0], warmup=2, loss_fn=_two_layer_loss, grad_scaler=scaler)
    pattern, pattern_3 = [], []
    for it in range(8):
        data, target = batches[0] if it < 2 else batches[it]
        if it == 3:                                                               # one eager step between replays
            trainer.train_step(net, opt, data, target, loss_fn=_two_layer_loss, grad_scaler=scaler)
        elif it >= 2:
            graphed(data, target)
        done_before = opt_t.steps_done()
        trainer.train_step(twin, opt_t, data, target, loss_fn=_two_layer_loss, grad_scaler=scaler_t)
        trainer.train_step(third, opt_3, data, target, loss_fn=_two_layer_loss, grad_scaler=scaler_3)
        pattern.append((opt_t.steps_done() - done_before, scaler_t.get_scale(), scaler_t.get_growth_tracker()))
        pattern_3.append((scaler_3.get_scale(), scaler_3._get_growth_tracker()))
        if it >= 1:                                                               # (the warm-up ran both of its steps before the loop)
            a, b = _snapshot(net, opt, scaler), _snapshot(twin, opt_t, scaler_t)
            assert a[1:] == b[1:], (it, a[1:], b[1:])
            assert len(a[0]) == len(b[0]) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[0], b[0])), it
    print(kind, pattern)
    applied = [p[0] for p in pattern]
    assert applied[0] == 0 and sum(applied) >= 3 and applied.count(0) >= 2, pattern
    assert [p[1:] for p in pattern] == pattern_3
    assert any(b[1] > a[1] for a, b in zip(pattern, pattern[1:]))                 # the scale grew at least once
    worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(twin.parameters(), third.parameters()))
    print(f"{kind}: largest parameter difference to the torch-scaler run {worst:.2e}")
    assert all(bool(torch.isfinite(p).all()) for p in twin.parameters()) and worst <= L.FLOORS["p"].a, worst


# ---------------------------------------------------------------------------------------------------------------------
# the fp16 network
# ---------------------------------------------------------------------------------------------------------------------
def _fp16_run(device_scaler):
    from mlagg_unet_amd import model as PM, trainer as TR
    from oracle import mlagg_oracle as O
    torch.manual_seed(0)
    net = PM.build_network_architecture((64, 64), 1, 14, True, "B", "fp16")
    O.deterministic_fill_(net.state_dict())
    net = net.to(DEV).eval()
    opt, _ = TR.configure_optimizers(net, capturable=device_scaler)
    scaler = TR.DeviceGradScaler(DEV, init_scale=1024.0) if device_scaler else torch.amp.GradScaler("cuda", init_scale=1024.0)
    data, target = TR.synthetic_batch(2, 1, 64, 64, 14, seed=99, device=DEV)
    losses = [float(TR.train_step(net, opt, data, target, grad_scaler=scaler)) for _ in range(5)]
    tracker = scaler.get_growth_tracker() if device_scaler else scaler._get_growth_tracker()
    return losses, scaler.get_scale(), tracker, opt.steps_done()


# largest |loss difference| over the five steps between two runs of the torch-scaler path (measured on an MI355X: see the docstring)
FP16_LOSS_SPREAD = 1.6e-4


def test_fp16_network_fits_a_batch_and_decides_like_the_torch_scaler():
    """The 2-D network with precision="fp16" at the shape of tests/test_mixed_precision_gpu.py (64 x 64, 14 classes, variant B, batch 2),
    five steps on one batch with DeviceGradScaler(init_scale=1024) and the capturable ClipAdamW: the criterion of that file's
    test_mixed_precision_train_steps_fit_a_batch (every loss finite, the last below the first); scale, tracker and applied steps equal
    those of the run with torch.amp.GradScaler; the losses of the two runs agree within 4 x the run-to-run spread of the torch-scaler
    path itself (two runs of it, the largest |loss difference| over the five steps: FP16_LOSS_SPREAD).
    Measured on an MI355X: two torch-scaler runs gave losses 4.13806 2.69890 2.08062 1.73956 1.52302 and 4.13790 2.69877 2.08058
    1.73952 1.52296, 1.61e-4 apart at the first step (the library convolutions' weight gradients accumulate with atomics unless
    trainer.set_deterministic is on), so 6.4e-4 is allowed; a DeviceGradScaler run on the same machine was 1.02e-4 from the first of
    them, with scale 1024, tracker 5 and 5 applied steps in all three."""
    ours, scale, tracker, applied = _fp16_run(True)
    theirs, scale_t, tracker_t, applied_t = _fp16_run(False)
    print("device scaler", ours, scale, tracker, applied)
    print("torch scaler ", theirs, scale_t, tracker_t, applied_t)
    assert all(np.isfinite(ours)) and ours[-1] < ours[0], ours
    assert (scale, tracker, applied) == (scale_t, tracker_t, applied_t)
    worst = max(abs(a - b) for a, b in zip(ours, theirs))
    print(f"largest loss difference {worst:.3e}, allowed {4.0 * FP16_LOSS_SPREAD:.3e}")
    assert worst <= 4.0 * FP16_LOSS_SPREAD, (worst, FP16_LOSS_SPREAD)


# ---------------------------------------------------------------------------------------------------------------------
# the plugin
# ---------------------------------------------------------------------------------------------------------------------
def _plugin_trainer(**kw):
    import fake_nnunet as FK
    from mlagg_unet_amd import nnunet_plugin
    from oracle import mlagg_oracle as O
    cls = nnunet_plugin.make_trainer_class(FK.nnUNetTrainer, precision="fp16", **kw)
    tr = cls(FK.make_plans((64, 64), 2), "2d_bs10", 0, FK.make_dataset_json(14), device=torch.device("cuda"))
    tr.initialize()
    O.deterministic_fill_(tr.network.state_dict())
    tr.network.eval()
    return tr


def _through_a_checkpoint(scaler):
    """``grad_scaler_state`` as nnUNetTrainer.save_checkpoint writes it (the scaler's state_dict, through torch.save) and
    load_checkpoint reads it back (``grad_scaler.load_state_dict`` of that entry).  The trainer's OWN save_checkpoint / load_checkpoint
    are NOT exercised: the stand-in base class of the tests (tests/fake_nnunet.py) has neither method, so only the two scaler calls
    those methods make and the serialisation between them are."""
    f = io.BytesIO()
    torch.save({"grad_scaler_state": scaler.state_dict() if scaler is not None else None}, f)
    f.seek(0)
    return torch.load(f, map_location="cpu", weights_only=False)["grad_scaler_state"]


def test_plugin_captures_the_fp16_step_with_device_loss_scaling():
    """make_trainer_class(precision="fp16", loss_scaling="device") behind the reference loop (tests/fake_nnunet.py): a DeviceGradScaler
    and a capturable ClipAdamW, three eager steps, then the step is captured and replayed; every step is either applied or skipped
    and the scaler's state says which.  The default keeps torch's scaler and eager steps.  ``grad_scaler_state`` goes through
    torch.save / torch.load in both directions between the two classes (the trainer's own checkpoint methods are not exercised:
    see ``_through_a_checkpoint``)."""
    from mlagg_unet_amd import nnunet_plugin, trainer
    assert nnunet_plugin.PLUGIN_GRAPH
    tr = _plugin_trainer(loss_scaling="device")
    assert type(tr.grad_scaler) is trainer.DeviceGradScaler and tr.mlagg_loss_scaling == "device"
    assert type(tr.optimizer) is trainer.ClipAdamW and tr.optimizer.capturable and tr._graph_ok()
    assert tr.grad_scaler.state_dict() == torch.amp.GradScaler("cuda").state_dict()
    losses = []
    for it in range(5):
        data, target = trainer.synthetic_batch(2, 1, 64, 64, 14, seed=700 + it)
        losses.append(float(tr.train_step({"data": data, "target": target})["loss"]))
        assert (tr._graphed is not None) == (it >= 3), (it, tr._graph_failed)
    assert all(np.isfinite(losses)) and tr._graph_failed is None
    # scale 65536, interval 2000: a skipped step halves the scale and resets the tracker, an applied one counts up
    sd = tr.grad_scaler.state_dict()
    applied = tr.optimizer.steps_done()
    skipped = 5 - applied
    print("losses", losses, "state", sd, "applied", applied)
    assert sd["scale"] == 65536.0 * 0.5 ** skipped and 0 <= skipped < 5 and sd["_growth_tracker"] <= applied

    default = _plugin_trainer()
    assert type(default.grad_scaler) is torch.amp.GradScaler and default.mlagg_loss_scaling == "torch" and not default._graph_ok()
    assert type(default.optimizer) is trainer.ClipAdamW and not default.optimizer.capturable
    data, target = trainer.synthetic_batch(2, 1, 64, 64, 14, seed=700)
    assert np.isfinite(default.train_step({"data": data, "target": target})["loss"]) and default._graphed is None

    # checkpoints: device -> device (in place: the captured graph holds the addresses), device -> torch, torch -> device
    saved = _through_a_checkpoint(tr.grad_scaler)
    assert saved == sd
    at = tr.grad_scaler._scale.data_ptr()
    tr.grad_scaler.load_state_dict({**saved, "scale": 256.0, "_growth_tracker": 7})
    assert tr.grad_scaler._scale.data_ptr() == at and tr.grad_scaler.get_scale() == 256.0 and tr.grad_scaler.get_growth_tracker() == 7
    data, target = trainer.synthetic_batch(2, 1, 64, 64, 14, seed=705)
    assert np.isfinite(tr.train_step({"data": data, "target": target})["loss"])       # a replay: it reads the loaded state
    skipped = bool(tr.grad_scaler.found_inf.item())                               # the decision the replay took, and its consequences
    assert (tr.grad_scaler.get_scale(), tr.grad_scaler.get_growth_tracker()) == ((128.0, 0) if skipped else (256.0, 8))
    assert tr.optimizer.steps_done() == applied + (0 if skipped else 1)
    default.grad_scaler.load_state_dict(_through_a_checkpoint(tr.grad_scaler))
    assert default.grad_scaler.state_dict() == tr.grad_scaler.state_dict()
    theirs = torch.amp.GradScaler("cuda", init_scale=512.0, growth_interval=3)
    tr.grad_scaler.load_state_dict(_through_a_checkpoint(theirs))
    assert tr.grad_scaler.state_dict() == theirs.state_dict() and tr.grad_scaler.growth_interval == 3


def test_plugin_with_device_loss_scaling_steps_eagerly_when_the_graph_is_off(monkeypatch):
    """MLAGG_PLUGIN_GRAPH=0 (nnunet_plugin.PLUGIN_GRAPH False) keeps every step eager; the DeviceGradScaler still needs -- and the
    class still builds -- a capturable optimizer, for the default recipe and for an ``optimizer=`` variant, and the steps run."""
    from mlagg_unet_amd import nnunet_plugin, trainer
    monkeypatch.setattr(nnunet_plugin, "PLUGIN_GRAPH", False)
    for kw, want in ((dict(), trainer.ClipAdamW), (dict(optimizer="sgd"), trainer.ClipSGD)):
        tr = _plugin_trainer(loss_scaling="device", **kw)
        assert not tr._graph_ok() and type(tr.grad_scaler) is trainer.DeviceGradScaler
        assert type(tr.optimizer) is want and tr.optimizer.capturable
        n = 5
        for it in range(n):
            data, target = trainer.synthetic_batch(2, 1, 64, 64, 14, seed=700 + it)
            assert np.isfinite(tr.train_step({"data": data, "target": target})["loss"])
            assert tr._graphed is None
        applied, sd = tr.optimizer.steps_done(), tr.grad_scaler.state_dict()
        assert 0 < applied <= n and sd["scale"] == 65536.0 * 0.5 ** (n - applied), (applied, sd)
