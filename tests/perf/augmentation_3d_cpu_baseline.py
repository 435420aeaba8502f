"""CPU baseline of the 3-D training augmentation chain: the scipy restatement of the reference's batchgenerators transforms
(tests/_augmentation_3d_oracle.py) on ONE host core at the BTCV plan (batch 2, 191x257x219 -> 96x160x160), the figure quoted
beside tools/bench_input_path_3d.py's device number: how many CPU workers per GPU the reference's chain would need.
    python tests/perf/augmentation_3d_cpu_baseline.py [--batches 2] [--forced]
--forced: rotation and scale on both samples (the expensive case); default: parameters as drawn."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import mlagg_unet_amd  # noqa: E402,F401
from mlagg_unet_amd import augmentation3d as AUG3  # noqa: E402
from tests import _augmentation_3d_oracle as AO3  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--forced", action="store_true")
    a = ap.parse_args()
    patch = (96, 160, 160)
    aug = AUG3.GpuAugmenter3D(patch, "cpu", seed=0)
    init = aug.initial_patch_size()
    rng = np.random.RandomState(0)
    data = rng.randn(2, 1, *init).astype(np.float32)
    seg = rng.randint(-1, 14, (2, 1, *init)).astype(np.float32)
    noise = rng.randn(2, 1, *patch).astype(np.float32)
    t0 = time.perf_counter()
    for i in range(a.batches):
        p = AUG3.draw_params_3d(np.random.RandomState(i), 2, 1, aug.rotation)
        if a.forced:
            p["do_rot"][:], p["do_scale"][:] = True, True
            p["angle"][:], p["scale"][:] = 0.3, 1.2
        AO3.apply(data.copy(), seg.copy(), patch, p, noise)
    cpu = (time.perf_counter() - t0) / a.batches
    print(json.dumps({"workload": "3-D augmentation chain B:666-701 (scipy restatement), batch 2, 191x257x219 -> 96x160x160, "
                                  "14 labels, one core" + (", rotation + scale forced" if a.forced else ""),
                      "cpu_oracle_s_per_batch": round(cpu, 2)}))


if __name__ == "__main__":
    main()
