"""Prediction export on the device (K21, csrc/export.hip, behind mlagg_unet_amd.export): the resampling kernel against float64 scipy
and the host path, the fused export against the reference's own export (tests/golden/export.npz), the K > 32 path, reproducibility,
64-bit offsets, and the chain from the 3-D sliding window."""
import os

import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import export as E
from mlagg_unet_amd import inference as PI
from mlagg_unet_amd import ops
from tests import _export_cases as C
from tests.test_export_cpu import _scipy_resample, _ulps

gpu = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "export.npz"))
convert = E.convert_predicted_logits_to_segmentation_with_correct_shape


def _sure(probs, gap=1e-6):
    """voxels whose two largest probabilities differ by more than gap (the label there is not a near-tie)"""
    top2 = torch.as_tensor(probs).topk(2, dim=0).values
    return (top2[0] - top2[1]) > gap


@gpu
@pytest.mark.parametrize("tag", sorted(C.CASES))
@pytest.mark.parametrize("contiguous", [True, False])
def test_device_resampling_matches_float64_scipy(tag, contiguous):
    K, shape, cfg, spacing, _, _, crop, _, _ = C.CASES[tag]
    x = GOLDEN[f"{tag}/logits"]
    cur = E.current_spacing_for(cfg, C.properties(tag))
    d = torch.from_numpy(x).to(DEV)
    if not contiguous:
        d = d.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
        assert not d.is_contiguous()
    got = E.resample_logits_to_shape(d, crop, cur, spacing)
    assert got.device.type == "cuda" and got.dtype == torch.float32 and tuple(got.shape) == (K,) + crop
    assert _ulps(got.cpu(), torch.from_numpy(_scipy_resample(x, crop, cur, spacing))) <= 1
    # the host path runs the same float64 products and sums: the same bits
    assert torch.equal(got.cpu(), E.resample_logits_to_shape(torch.from_numpy(x), crop, cur, spacing))


@gpu
def test_device_order_z1_matches_the_reference():
    K, shape, new_shape, cur, new = C.ORDER_Z1
    got = E.resample_logits_to_shape(torch.from_numpy(GOLDEN["order_z1/logits"]).to(DEV), new_shape, cur, new, order_z=1)
    assert _ulps(got.cpu(), torch.from_numpy(GOLDEN["order_z1/resampled"])) <= 1


@gpu
@pytest.mark.parametrize("tag", sorted(C.CASES))
def test_device_export_matches_the_reference(tag):
    K, shape, cfg, _, full, lo, crop, tb, _ = C.CASES[tag]
    x = torch.from_numpy(GOLDEN[f"{tag}/logits"]).to(DEV)
    seg, probs = convert(x, C.properties(tag), cfg, tb, return_probabilities=True)
    want_seg, want_p = torch.from_numpy(GOLDEN[f"{tag}/segmentation"]), torch.from_numpy(GOLDEN[f"{tag}/probabilities"])
    assert seg.device.type == "cuda" and seg.dtype == torch.uint8 and seg.is_contiguous() and probs.is_contiguous()
    seg, probs = seg.cpu(), probs.cpu()
    assert seg.shape == want_seg.shape and probs.shape == want_p.shape
    assert float((probs - want_p).abs().max()) <= 2e-6
    sure = _sure(want_p)
    assert torch.equal(seg[sure], want_seg[sure])
    print(f"{tag}: {int((~sure).sum())} near-tie voxels, {int((seg != want_seg).sum())} labels differ")
    assert int((seg != want_seg).sum()) == 0                             # random logits: no near-ties expected
    # zeros outside the box, in the labels and in every probability channel, and the transposed order
    inside = torch.zeros(full, dtype=torch.bool)
    inside[tuple(slice(a, a + c) for a, c in zip(lo, crop))] = True
    outside = ~inside.permute(tb)
    assert int(seg[outside].abs().sum()) == 0 and float(probs[:, outside].abs().sum()) == 0.0
    assert tuple(seg.shape) == tuple(full[p] for p in tb)
    inv = [tb.index(d) for d in range(3)]
    box = seg.permute(inv)[tuple(slice(a, a + c) for a, c in zip(lo, crop))]
    assert torch.equal(box, want_seg.permute(inv)[tuple(slice(a, a + c) for a, c in zip(lo, crop))])
    labels_only, none = convert(x, C.properties(tag), cfg, tb)
    assert none is None and torch.equal(labels_only.cpu(), seg)


@gpu
def test_device_export_of_a_non_contiguous_view():
    tag = "d_2d_config"
    K, shape, cfg, _, _, _, _, tb, _ = C.CASES[tag]
    x = torch.from_numpy(GOLDEN[f"{tag}/logits"]).to(DEV)
    view = x.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
    a, pa = convert(x, C.properties(tag), cfg, tb, return_probabilities=True)
    b, pb = convert(view, C.properties(tag), cfg, tb, return_probabilities=True)
    assert torch.equal(a, b) and torch.equal(pa, pb)


@gpu
@pytest.mark.parametrize("tag", ["b_separate_z", "a_isotropic"])
def test_more_than_32_classes_take_the_resampling_kernel(tag):
    K, shape, cfg, _, _, _, _, tb, _ = C.CASES[tag]
    x = torch.randn((40,) + shape, generator=torch.Generator().manual_seed(40)) * 2
    seg, probs = convert(x.to(DEV), C.properties(tag), cfg, tb, return_probabilities=True)
    hseg, hprobs = convert(x, C.properties(tag), cfg, tb, return_probabilities=True)
    assert seg.dtype == torch.uint8 and int(seg.max()) > 32
    assert float((probs.cpu() - hprobs).abs().max()) <= 2e-6
    sure = _sure(hprobs)
    assert torch.equal(seg.cpu()[sure], hseg[sure]) and int((seg.cpu() != hseg).sum()) == 0
    with pytest.raises(RuntimeError):
        ops.export_segmentation(x.to(DEV), E.build_taps(shape, shape, None), shape, (0, 0, 0), shape, (0, 1, 2))


@gpu
def test_two_runs_are_bit_identical():
    tag = "b_separate_z"
    K, shape, cfg, _, _, _, crop, tb, _ = C.CASES[tag]
    x = torch.from_numpy(GOLDEN[f"{tag}/logits"]).to(DEV)
    a = convert(x, C.properties(tag), cfg, tb, return_probabilities=True)
    b = convert(x, C.properties(tag), cfg, tb, return_probabilities=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    r1 = E.resample_logits_to_shape(x, crop, E.current_spacing_for(cfg, C.properties(tag)), C.properties(tag)["spacing"])
    r2 = E.resample_logits_to_shape(x, crop, E.current_spacing_for(cfg, C.properties(tag)), C.properties(tag)["spacing"])
    assert torch.equal(r1, r2)


@gpu
def test_probability_offsets_beyond_2_to_the_31():
    """K = 32 classes into 68 M voxels: K x voxels > 2^31, so the last channels' probabilities lie past int32 offsets."""
    K, shape, full = 32, (40, 96, 96), (260, 512, 512)
    assert K * full[0] * full[1] * full[2] > 2 ** 31
    props = {"spacing": [1.0, 0.75, 0.75], "shape_before_cropping": full, "bbox_used_for_cropping": [[0, s] for s in full],
             "shape_after_cropping_and_before_resampling": full}
    cfg, tb = (6.5, 4.0, 4.0), (0, 1, 2)
    x = torch.randn((K,) + shape, generator=torch.Generator().manual_seed(31)) * 2
    seg, probs = convert(x.to(DEV), props, cfg, tb, return_probabilities=True)
    cur = E.current_spacing_for(cfg, props)
    kinds = E.resampling_plan(shape, full, cur, props["spacing"])
    idx, w = E.build_taps(shape, full, kinds)
    for a in (0, 130, 257):                                             # slabs of 3 output x planes, the last one at the end
        taps = (np.concatenate([idx[a:a + 3], idx[full[0]:]]), np.concatenate([w[a:a + 3], w[full[0]:]]))
        host = torch.softmax(E._resample_host(x, taps, (3,) + full[1:]), 0)
        got = probs[:, a:a + 3].cpu()
        assert float((got - host).abs().max()) <= 2e-6
        sure = _sure(host)
        assert torch.equal(seg[a:a + 3].cpu()[sure], host.argmax(0).to(torch.uint8)[sure])


class FakeNet(torch.nn.Module):
    """Returns stored tile outputs R (V, N, K, tile) in tile order (tests/test_sliding_window_3d_gpu.py)."""

    def __init__(self, R):
        super().__init__()
        self.R, self.pos = R, 0

    def forward(self, x):
        V = self.R.shape[0]
        n = x.shape[0] // V
        out = self.R[:, self.pos:self.pos + n].reshape((V * n,) + tuple(self.R.shape[2:])).clone()
        self.pos += n
        return out


@gpu
def test_sliding_window_then_device_export_matches_the_host_chain():
    K, tile, volume, mirror = 5, (12, 20, 36), (2, 10, 50, 70), (0, 2)
    g = torch.Generator().manual_seed(2121)
    vol = torch.randn(volume, generator=g)
    data, _ = PI._pad_to_tile(vol, tile)
    steps = PI.compute_steps_for_sliding_window(tuple(data.shape[1:]), tile, 0.5)
    n = len(steps[0]) * len(steps[1]) * len(steps[2])
    R = (torch.randn((4, n, K) + tile, generator=g) * 3).to(DEV)
    logits = PI.predict_sliding_window_return_logits(FakeNet(R), vol, K, tile, mirror_axes=mirror, device=DEV)
    assert logits.shape == (K,) + volume[1:]
    props = {"spacing": [2.5, 0.8, 0.8], "shape_before_cropping": (16, 66, 90), "bbox_used_for_cropping": [[2, 16], [5, 65], [3, 84]],
             "shape_after_cropping_and_before_resampling": (14, 60, 81)}
    cfg, tb = (3.5, 0.7, 0.7), (2, 0, 1)
    seg, probs = convert(logits, props, cfg, tb, return_probabilities=True)
    hseg, hprobs = convert(logits.cpu(), props, cfg, tb, return_probabilities=True)
    assert float((probs.cpu() - hprobs).abs().max()) <= 2e-6
    sure = _sure(hprobs)
    assert torch.equal(seg.cpu()[sure], hseg[sure]) and int((seg.cpu() != hseg).sum()) == 0
