"""CPU: K19t (the 3 x 3, stride-2 transposed convolution of PatchExpand) -- shape rules of the C ABI and the dispatch predicate."""
import types

import torch

from mlagg_unet_amd import _lib, ops


def test_s2t_shape_rules():
    lib = _lib.lib()
    assert lib.mlagg_conv3x3_s2t_supported(192, 384, 32, 32)
    assert lib.mlagg_conv3x3_s2t_supported(96, 192, 64, 64)
    assert lib.mlagg_conv3x3_s2t_supported(384, 768, 16, 16)
    assert not lib.mlagg_conv3x3_s2t_supported(4, 96, 64, 64)          # O % 16
    assert not lib.mlagg_conv3x3_s2t_supported(96, 40, 64, 64)         # I % 16
    assert not lib.mlagg_conv3x3_s2t_supported(0, 96, 64, 64)
    assert not lib.mlagg_conv3x3_s2t_supported(96, 96, 0, 64)
    assert not lib.mlagg_conv3x3_s2t_supported(16, 16, 8192, 8192)     # a sample past the 32-bit buffer offsets
    assert not lib.mlagg_conv3x3_s2t_supported(16, 4096, 512, 512)


def test_s2t_workspace_sizes():
    lib = _lib.lib()
    assert lib.mlagg_conv3x3_s2t_workspace_bytes(96, 192) == 3 * 9 * 96 * 192 * 2
    assert lib.mlagg_conv3x3_s2t_workspace_bytes(0, 192) == 0
    for B, O, I, H, W in [(10, 96, 192, 64, 64), (10, 192, 384, 32, 32), (2, 384, 768, 16, 16), (1, 16, 32, 3, 37)]:
        n = lib.mlagg_conv3x3_s2t_wgrad_workspace_floats(B, O, I, H, W)
        assert n > 0 and n % (9 * O * I) == 0                           # whole partial blocks
        assert n * 4 <= (256 << 20) or n == B * 9 * O * I                # under the cap unless one block per sample
        assert lib.mlagg_conv3x3_s2t_wgrad_workspace_floats(2 * B, O, I, H, W) >= n
    assert lib.mlagg_conv3x3_s2t_wgrad_workspace_floats(2, 4, 96, 64, 64) == 0
    assert lib.mlagg_conv3x3_s2t_wgrad_workspace_floats(0, 96, 192, 64, 64) == 0


def _dev(shape):
    """Something the predicate takes for an fp32 device map of this shape (no GPU on this machine)."""
    return types.SimpleNamespace(is_cuda=True, dtype=torch.float32, shape=torch.Size(shape), dim=lambda: len(shape))


def test_s2t_predicate(monkeypatch):
    w = torch.empty(192, 96, 3, 3)
    ok = dict(stride=(2, 2), padding=(1, 1), output_padding=(0, 0), dilation=(1, 1), groups=1)
    x = _dev((2, 192, 64, 64))
    assert ops.conv3x3_s2t_supported(x, w, **ok)
    assert ops.conv3x3_s2t_supported(x, w, **ok, form=1)
    assert not ops.conv3x3_s2t_supported(torch.empty(2, 192, 64, 64), w, **ok)       # host tensor
    for k, v in [("stride", (1, 1)), ("padding", (0, 0)), ("output_padding", (1, 1)), ("dilation", (2, 2)), ("groups", 2)]:
        assert not ops.conv3x3_s2t_supported(x, w, **dict(ok, **{k: v})), k
    assert not ops.conv3x3_s2t_supported(x, torch.empty(192, 96, 2, 2), **ok)
    assert not ops.conv3x3_s2t_supported(x, torch.empty(192, 96, 1, 1), **ok)
    assert not ops.conv3x3_s2t_supported(_dev((2, 96, 64, 64)), torch.empty(96, 4, 3, 3), **ok)     # O = 4
    # the pixel threshold: a 16 x 16 map stays on the library at the default
    assert ops.conv3x3_s2t_supported(_dev((2, 768, 16, 16)), torch.empty(768, 384, 3, 3), **ok) == (256 >= ops.K19_MIN_PIXELS)
    monkeypatch.setattr(ops, "K19T", False)
    assert not ops.conv3x3_s2t_supported(x, w, **ok)
