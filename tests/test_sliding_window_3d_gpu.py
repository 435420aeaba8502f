"""3-D sliding-window inference on the device (K20, csrc/sliding_window.hip, behind inference.predict_sliding_window_return_logits):
kernel level against the torch composition of the same order on the same GPU, and end to end with the product 3-D network against
the reference-order loop driving the oracle network (oracle/umamba3d_oracle.py) on the CPU."""
import numpy as np
import pytest
import torch

import mlagg_unet_amd  # noqa: F401
from mlagg_unet_amd import inference as PI
from mlagg_unet_amd import ops
from oracle import inference_oracle as IO
from oracle import mlagg_oracle as O

gpu = pytest.mark.gpu
DEV = "cuda:0"
TILE = (12, 20, 36)                       # no side a multiple of 64
VOLUME = (2, 10, 50, 70)                  # x padded to 12; 1 x 4 x 3 overlapping tiles
MIRRORS = {1: None, 2: (1,), 4: (0, 2), 8: (0, 1, 2)}


class FakeNet(torch.nn.Module):
    """Stands in for the network: returns the stored outputs R (V, N, K, tile) of the tiles of each call, in tile order, and
    records the inputs it was given."""

    def __init__(self, R):
        super().__init__()
        self.R, self.pos, self.inputs = R, 0, []

    def forward(self, x):
        V = self.R.shape[0]
        n = x.shape[0] // V
        self.inputs.append(x.clone())
        out = self.R[:, self.pos:self.pos + n].reshape((V * n,) + tuple(self.R.shape[2:])).clone()
        self.pos += n
        return out


def _setup(V, K, seed):
    g = torch.Generator().manual_seed(seed)
    vol = torch.randn(VOLUME, generator=g)
    data, revert = PI._pad_to_tile(vol, TILE)
    steps = PI.compute_steps_for_sliding_window(tuple(data.shape[1:]), TILE, 0.5)
    places = [(sx, sy, sz) for sx in steps[0] for sy in steps[1] for sz in steps[2]]
    R = torch.randn((V, len(places), K) + TILE, generator=g).to(DEV)
    return vol, data.to(DEV).contiguous(), revert, places, R


def _ulps(a, b):
    ia, ib = a.view(torch.int32).long(), b.view(torch.int32).long()
    return int((ia - ib).abs().max())


@gpu
@pytest.mark.parametrize("V", [1, 2, 4, 8])
@pytest.mark.parametrize("K", [5, 14])
def test_kernels_match_the_torch_composition(V, K):
    vol, data, revert, places, R = _setup(V, K, seed=V * 100 + K)
    flips = PI.mirror_variants(MIRRORS[V])
    assert len(flips) == V
    gauss = PI.compute_gaussian(TILE).to(DEV)
    N = len(places)
    # torch composition on the same GPU, chunks of 4 tiles (overlapping tiles inside a chunk)
    ref_net = FakeNet(R)
    acc_t, w_t = PI._sliding_window_3d_torch(ref_net, data, gauss, places, flips, TILE, 4, K)
    # the kernels, same chunks
    acc = torch.zeros_like(acc_t)
    w = torch.zeros_like(w_t)
    net = FakeNet(R)
    for c, i in enumerate(range(0, N, 4)):
        chunk = places[i:i + 4]
        x = ops.sliding_window_gather(data, chunk, flips, TILE)
        assert torch.equal(x, ref_net.inputs[c])                          # gather == slice + stack + flip + cat
        out = net(x)
        for j, o in enumerate(chunk):
            ops.sliding_window_fold(out, j, len(chunk), flips, gauss, o, acc, w)
    assert torch.equal(w, w_t)
    assert torch.equal(acc, acc_t)                                        # fold: same bits as the torch composition
    logits, labels = ops.sliding_window_finalize(acc, w, revert, return_labels=True)
    want = (acc_t / w_t)[(slice(None),) + tuple(revert)]
    assert logits.is_contiguous() and logits.shape == (K,) + VOLUME[1:]
    # both divisions are IEEE correctly rounded (hipcc's default for `/`, and torch's true division), so the bits are expected to
    # agree; the bound allows 1 ulp should torch's build take another division sequence
    assert _ulps(logits, want) <= 1
    assert torch.equal(labels, logits.argmax(0))
    # the public function: one chunk of all tiles, chunks of one tile, and a repeat are bit-identical
    runs = [PI.predict_sliding_window_return_logits(FakeNet(R), vol, K, TILE, mirror_axes=MIRRORS[V], tile_batch=tb, device=DEV)
            for tb in (N, 1, 1)]
    assert torch.equal(runs[0], logits) and torch.equal(runs[1], logits) and torch.equal(runs[2], logits)
    seg = PI.predict_sliding_window_return_segmentation(FakeNet(R), vol, K, TILE, mirror_axes=MIRRORS[V], tile_batch=3, device=DEV)
    assert seg.dtype == torch.int64 and torch.equal(seg, labels)


@gpu
def test_ops_reject_boxes_outside_the_volume():
    data = torch.zeros(2, 12, 20, 36, device=DEV)
    with pytest.raises(RuntimeError):
        ops.sliding_window_gather(data, [(1, 0, 0)], [0], TILE)
    acc, w = torch.zeros(3, 12, 20, 36, device=DEV), torch.zeros(12, 20, 36, device=DEV)
    out, g = torch.zeros(2, 3, *TILE, device=DEV), torch.ones(TILE, device=DEV)
    with pytest.raises(RuntimeError):
        ops.sliding_window_fold(out, 0, 1, [0, 1], g, (0, 0, 1), acc, w)
    with pytest.raises(RuntimeError):
        ops.sliding_window_fold(out, 1, 1, [0, 1], g, (0, 0, 0), acc, w)
    with pytest.raises(RuntimeError):
        ops.sliding_window_finalize(acc, w, (slice(0, 13), slice(0, 20), slice(0, 36)))


# the small configuration of tests/test_umamba3d_gpu.py
CFG = dict(size=(8, 64, 64), in_ch=1, n_cls=5,
           strides=[[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2], [1, 2, 2], [1, 2, 2]])


def _reference_order_loop(net, image, num_heads, tile, mirror_axes, step=0.5):
    """sliding_window_prediction.py:118-210 for a 3-D tile, fp32 accumulators, one tile and one flip per forward."""
    with torch.no_grad():
        data, revert = IO.pad_nd_image(image, tile)
        g = torch.from_numpy(IO.compute_gaussian(tile)).float()
        logits = torch.zeros((num_heads,) + tuple(data.shape[1:]))
        weight = torch.zeros(tuple(data.shape[1:]))
        steps = IO.compute_steps(tuple(data.shape[1:]), tile, step)
        ax = set(mirror_axes or ())
        flips = [f for f in ((2,), (3,), (4,), (2, 3), (2, 4), (3, 4), (2, 3, 4)) if mirror_axes and {d - 2 for d in f} <= ax]
        for sx in steps[0]:
            for sy in steps[1]:
                for sz in steps[2]:
                    sl = (slice(sx, sx + tile[0]), slice(sy, sy + tile[1]), slice(sz, sz + tile[2]))
                    x = data[(slice(None),) + sl][None]
                    pred = net(x)
                    for f in flips:
                        pred += torch.flip(net(torch.flip(x, f)), f)
                    pred /= len(flips) + 1
                    logits[(slice(None),) + sl] += pred[0] * g
                    weight[sl] += g
        logits /= weight
        return logits[(slice(None),) + tuple(revert[1:])]


@gpu
@pytest.mark.parametrize("shape,mirror", [((1, 12, 80, 72), (0, 2)), ((1, 6, 50, 70), (1,))])
def test_3d_network_end_to_end_matches_the_reference_order(shape, mirror):
    from mlagg_unet_amd import model3d
    from oracle import umamba3d_oracle as U
    n = len(CFG["strides"])
    net = model3d.build_network_architecture_3d(CFG["in_ch"], CFG["n_cls"], [[3, 3, 3]] * n, CFG["strides"], [2] * n, [2] * (n - 1),
                                                enable_deep_supervision=False)
    O.deterministic_fill_(net.state_dict(), seed=21)
    oracle = U.build_reference_3d_model(CFG["in_ch"], CFG["n_cls"], U.features_for(n), CFG["strides"], deep_supervision=False)
    oracle.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
    net = net.to(DEV).eval()
    oracle.eval()
    image = torch.rand(shape, generator=torch.Generator().manual_seed(sum(shape)))
    got = PI.predict_sliding_window_return_logits(net, image, CFG["n_cls"], CFG["size"], mirror_axes=mirror)
    assert got.device.type == "cuda" and got.dtype == torch.float32 and got.is_contiguous()
    assert got.shape == (CFG["n_cls"],) + shape[1:]
    want = _reference_order_loop(oracle, image, CFG["n_cls"], CFG["size"], mirror)
    err = float((got.cpu() - want).abs().max())
    assert err < 1e-3, err                                                  # north-star tolerance on fp32 logits
    seg = PI.predict_sliding_window_return_segmentation(net, image, CFG["n_cls"], CFG["size"], mirror_axes=mirror).cpu()
    top2 = want.topk(2, dim=0).values
    sure = (top2[0] - top2[1]) > 2e-3
    assert sure.float().mean() > 0.9
    assert torch.equal(seg[sure], want.argmax(0)[sure])
    assert np.isfinite(got.cpu().numpy()).all()
