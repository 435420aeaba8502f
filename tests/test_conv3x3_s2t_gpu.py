"""GPU: K19t -- the 3 x 3, stride-2, padding-1 transposed convolution of PatchExpand (T:506-513) and its two gradients against float64
`conv_transpose2d`, in the three operand forms; run-to-run determinism; the PatchExpand module and the full 2-D network with the kernel
on and off."""
import copy

import pytest
import torch
import torch.nn.functional as F

from mlagg_unet_amd import model, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


def _reference(x, w, dy, rounding=None):
    """float64 y, dx, dW of y = conv_transpose2d(x, w, stride 2, padding 1); operands first rounded to `rounding` if given."""
    cast = (lambda t: t.to(rounding).double()) if rounding else (lambda t: t.double())
    xd = cast(x.detach()).requires_grad_(True)
    wd = cast(w.detach()).requires_grad_(True)
    y = F.conv_transpose2d(xd, wd, None, 2, 1)
    y.backward(cast(dy))
    return y.detach(), xd.grad, wd.grad


def _kernel(x, w, dy, form=ops._DTYPE_BF16X3):
    x = x.detach().requires_grad_(True)
    w = w.detach().requires_grad_(True)
    y = ops.conv3x3_s2t(x, w, form)
    y.backward(dy)
    return y.detach(), x.grad, w.grad


@pytest.fixture
def no_floor(monkeypatch):
    monkeypatch.setattr(ops, "K19_MIN_PIXELS", 0)
    monkeypatch.setattr(ops, "LP_K_MIN_PIXELS", 0)
    monkeypatch.setattr(ops, "K19T_WGRAD", True)            # the kernel's weight gradient too (off in the step by default)


SHAPES = [(2, 192, 96, 64, 64), (2, 384, 192, 32, 32), (2, 768, 384, 16, 16),       # PatchExpand up_0 / up_1 / up_2 at batch 2
          (2, 32, 48, 7, 9), (1, 16, 32, 1, 5), (3, 48, 16, 3, 37), (2, 16, 16, 2, 33)]   # ragged maps


@pytest.mark.parametrize("B,I,O,H,W", SHAPES)
def test_s2t_matches_float64(no_floor, B, I, O, H, W):
    g = torch.Generator(device=DEV).manual_seed(B * 1000 + I + O + H * W)
    x = torch.randn(B, I, H, W, device=DEV, generator=g)
    w = torch.randn(I, O, 3, 3, device=DEV, generator=g) * 0.05
    dy = torch.randn(B, O, 2 * H - 1, 2 * W - 1, device=DEV, generator=g)
    y, dx, dW = _kernel(x, w, dy)
    ry, rdx, rdW = _reference(x, w, dy)
    assert y.shape == ry.shape
    # the fp32 bounds of the stride-1 kernel; on the longest contractions (9 x 384 terms) a single fp32 accumulation chain -- the
    # library's fp32 kernels' too -- is near 2e-6 already, so a product may also stay within twice the library's own error
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yl = F.conv_transpose2d(xl, wl, None, 2, 1)
    yl.backward(dy)
    errs = (_rel(y, ry), _rel(dx, rdx), _rel(dW, rdW))
    libs = (_rel(yl.detach(), ry), _rel(xl.grad, rdx), _rel(wl.grad, rdW))
    for e, le, bound in zip(errs, libs, (2e-6, 2e-6, 4e-6)):
        assert e < max(bound, 2 * le), (errs, libs)


def test_s2t_channel_slice_and_padded_gradient_view(no_floor):
    B, I, O, H, W = 2, 64, 32, 12, 20
    g = torch.Generator(device=DEV).manual_seed(7)
    big = torch.randn(B, I + 48, H, W, device=DEV, generator=g)
    x = big[:, 16:16 + I]                                   # a channel slice: samples are not contiguous
    w = torch.randn(I, O, 3, 3, device=DEV, generator=g) * 0.05
    full = torch.randn(B, O, 2 * H, 2 * W, device=DEV, generator=g)
    dy = full[:, :, 1:, 1:]                                 # the interior of the padded gradient (row stride 2W)
    ry, rdx, rdW = _reference(x, w, dy)
    # through PatchExpand's pad: autograd hands the kernel the view
    xs = x.detach().requires_grad_(True)
    ws = w.detach().requires_grad_(True)
    F.pad(ops.conv3x3_s2t(xs, ws), (1, 0, 1, 0)).backward(full)
    assert _rel(xs.grad, rdx) < 2e-6 and _rel(ws.grad, rdW) < 4e-6
    # and the two gradient products called on the view directly
    xc = x.contiguous()
    assert dy.stride(2) == 2 * W and not dy.is_contiguous()
    dx = ops._k19t_dgrad(dy, w.contiguous(), O, I, H, W, ops._DTYPE_BF16X3)
    dW = ops._k19t_wgrad(x, x.stride(0), dy, O, I, H, W, ops._DTYPE_BF16X3)
    assert _rel(dx, rdx) < 2e-6 and _rel(dW, rdW) < 4e-6
    y = ops._k19t_fwd(x, x.stride(0), w.contiguous(), O, I, H, W, ops._DTYPE_BF16X3)
    assert _rel(y, ry) < 2e-6
    assert torch.equal(y, ops._k19t_fwd(xc, xc.stride(0), w.contiguous(), O, I, H, W, ops._DTYPE_BF16X3))


@pytest.mark.parametrize("form,dt", [(1, torch.bfloat16), (2, torch.float16)])
@pytest.mark.parametrize("B,I,O,H,W", [(2, 192, 96, 64, 64), (2, 32, 48, 7, 9)])
def test_s2t_one_product_forms(no_floor, form, dt, B, I, O, H, W):
    g = torch.Generator(device=DEV).manual_seed(form * 31 + H)
    x = torch.randn(B, I, H, W, device=DEV, generator=g)
    w = torch.randn(I, O, 3, 3, device=DEV, generator=g) * 0.05
    dy = torch.randn(B, O, 2 * H - 1, 2 * W - 1, device=DEV, generator=g)
    y, dx, dW = _kernel(x, w, dy, form)
    ry, rdx, rdW = _reference(x, w, dy, dt)
    assert _rel(y, ry) < 4e-6 and _rel(dx, rdx) < 4e-6 and _rel(dW, rdW) < 4e-6, (_rel(y, ry), _rel(dx, rdx), _rel(dW, rdW))


@pytest.mark.parametrize("form", [1, 2, 3])
def test_s2t_is_deterministic(no_floor, form):
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(2, 384, 32, 32, device=DEV, generator=g)
    w = torch.randn(384, 192, 3, 3, device=DEV, generator=g) * 0.05
    dy = torch.randn(2, 192, 63, 63, device=DEV, generator=g)
    a, b = _kernel(x, w, dy, form), _kernel(x, w, dy, form)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def _count(monkeypatch):
    calls = {"fwd": 0, "dgrad": 0, "wgrad": 0, "shapes": []}
    for name in ("fwd", "dgrad", "wgrad"):
        orig = getattr(ops, "_k19t_" + name)

        def wrap(*a, _orig=orig, _name=name, **k):
            calls[_name] += 1
            if _name == "fwd":
                calls["shapes"].append(tuple(a[0].shape))
            return _orig(*a, **k)
        monkeypatch.setattr(ops, "_k19t_" + name, wrap)
    return calls


def test_patch_expand_kernel_vs_library(monkeypatch):
    torch.manual_seed(3)
    on = model.PatchExpand(192, 96).to(DEV)
    off = copy.deepcopy(on)
    x = torch.randn(2, 192, 64, 64, device=DEV)
    calls = _count(monkeypatch)
    xa = x.clone().requires_grad_(True)
    ya = on(xa)
    ya.square().sum().backward()
    assert calls["fwd"] == 1 and calls["dgrad"] == 1 and calls["wgrad"] == (1 if ops.K19T_WGRAD else 0)
    monkeypatch.setattr(ops, "K19T", False)
    xb = x.clone().requires_grad_(True)
    yb = off(xb)
    yb.square().sum().backward()
    assert calls["fwd"] == 1                                # the library ran
    assert ya.shape == yb.shape == (2, 96, 128, 128)
    assert _rel(ya, yb.double()) < 2e-5
    assert _rel(xa.grad, xb.grad.double()) < 2e-5
    for (n, p), q in zip(on.named_parameters(), off.parameters()):
        assert _rel(p.grad, q.grad.double()) < 5e-5, n


def test_full_model_with_and_without_k19t(monkeypatch):
    from oracle import mlagg_oracle as O
    from mlagg_unet_amd import trainer as TR
    img = (256, 256)
    net = model.build_network_architecture(img, 1, 14, True, "B")
    O.deterministic_fill_(net.state_dict())
    net = net.to(DEV).eval()
    ref = copy.deepcopy(net)
    data, target = O.synthetic_batch(2, 1, *img, 14, seed=5)
    data, target = data.to(DEV), [t.to(DEV) for t in target]
    calls = _count(monkeypatch)
    out = net(data)
    TR.deep_supervision_loss(out, target, batch_dice=True).backward()
    assert (2, 192, 64, 64) in calls["shapes"] and (2, 384, 32, 32) in calls["shapes"]        # up_0, up_1
    assert calls["dgrad"] >= 2
    monkeypatch.setattr(ops, "K19T", False)
    out_ref = ref(data)
    TR.deep_supervision_loss(out_ref, target, batch_dice=True).backward()
    for a, b in zip(out, out_ref):
        assert float((a.detach() - b.detach()).abs().max()) < 1e-4
    for (n, p), q in zip(net.named_parameters(), ref.parameters()):
        if p.grad is None:
            assert q.grad is None, n
            continue
        a, b = p.grad.double().reshape(-1), q.grad.double().reshape(-1)
        if float(b.abs().max()) <= 1e-6:                    # analytically ~0 (a bias in front of a norm): values, not direction
            assert float((a - b).abs().max()) < 1e-6, n
            continue
        na, nb = float(a.norm()), float(b.norm())
        assert float(a @ b) / (na * nb) > 1 - 1e-6, n
