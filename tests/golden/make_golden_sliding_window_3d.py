"""Generate tests/golden/sliding_window_3d.npz from the REFERENCE's own 3-D sliding-window prediction.

    MLAGG_REFERENCE=<reference checkout> python tests/golden/make_golden_sliding_window_3d.py

Runs nnunetv2.inference.sliding_window_prediction.predict_sliding_window_return_logits (:118-210) on its CPU branch for the tiny
seeded network of tests/_sliding_window_3d_case.py, with acvl_utils.pad_nd_image (third-party, absent offline) replaced by the
oracle's restatement exactly as make_golden.golden_sliding_window does, and stores compute_gaussian (:13-28) and
compute_steps_for_sliding_window (:31-57) for a few 3-D shapes.  Only the data is committed."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if "MLAGG_REFERENCE" not in os.environ:
    raise SystemExit("set MLAGG_REFERENCE to a checkout of the reference repository (aticejiang/MLAgg-UNet)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.environ["MLAGG_REFERENCE"], "mlagg"))

from oracle import inference_oracle as IO  # noqa: E402
from tests import _sliding_window_3d_case as C  # noqa: E402


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def pad_nd_image(image, new_shape, mode, kwargs, return_slicer, shape_must_be_divisible_by=None):
    assert mode == "constant" and return_slicer
    return IO.pad_nd_image(image, new_shape, kwargs.get("value", 0))


def main():
    _mod("acvl_utils")
    _mod("acvl_utils.cropping_and_padding")
    _mod("acvl_utils.cropping_and_padding.padding", pad_nd_image=pad_nd_image)
    S = importlib.import_module("nnunetv2.inference.sliding_window_prediction")
    net, img, small = C.case()
    out = {}
    for tag, which, mirror in C.CASES:
        r = S.predict_sliding_window_return_logits(net, (img, small)[which], C.NUM_CLASSES, C.TILE, mirror_axes=mirror,
                                                   tile_step_size=0.5, use_gaussian=True, perform_everything_on_gpu=False,
                                                   verbose=False, device=torch.device("cpu"))
        assert r.dtype == torch.half
        out[tag] = r.float().numpy()
    out["gaussian_12x16x16"] = S.compute_gaussian((12, 16, 16)).astype(np.float32)
    out["gaussian_96x160x160"] = S.compute_gaussian((96, 160, 160)).astype(np.float32)[::8, ::8, ::8]
    steps = [S.compute_steps_for_sliding_window(a, b, c) for a, b, c in C.STEP_SHAPES]
    out["steps"] = np.asarray([v for s_ in steps for ax in s_ for v in ax + [-1]])
    np.savez_compressed(os.path.join(HERE, "sliding_window_3d.npz"), **out)
    print("sliding window 3-D", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
