"""The tiny seeded 3-D case of tests/golden/sliding_window_3d.npz (made by tests/golden/make_golden_sliding_window_3d.py with the
reference's own sliding_window_prediction): Conv3d -> Tanh -> Conv3d, 2 input channels, 3 classes, a tile whose sides differ."""
import torch

TILE = (12, 16, 16)
NUM_CLASSES = 3
# tag, volume (0: full, 1: smaller than the tile along x), mirror axes
CASES = (("mirror_012", 0, (0, 1, 2)), ("plain", 0, None), ("mirror_02", 0, (0, 2)), ("padded", 1, (1,)))
# (image size, tile, step) of the stored compute_steps_for_sliding_window results; the last is the BTCV plan
STEP_SHAPES = (((20, 24, 30), (12, 16, 16), 0.5), ((128, 256, 256), (96, 160, 160), 0.5), ((96, 160, 160), (96, 160, 160), 0.5),
               ((300, 512, 512), (96, 160, 160), 0.5), ((40, 33, 70), (12, 16, 16), 0.25))
GAUSSIAN_SHAPES = ((12, 16, 16), (96, 160, 160))


def case():
    """-> (network, volume (2, 20, 24, 30), volume smaller than the tile along x (2, 9, 24, 20))"""
    g = torch.Generator().manual_seed(2024)
    net = torch.nn.Sequential(torch.nn.Conv3d(2, 4, 3, padding=1), torch.nn.Tanh(), torch.nn.Conv3d(4, NUM_CLASSES, 3, padding=1))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.15)
    img = torch.randn(2, 20, 24, 30, generator=g)
    small = torch.randn(2, 9, 24, 20, generator=g)
    return net.eval(), img, small
