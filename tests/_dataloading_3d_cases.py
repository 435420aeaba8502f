"""Shared inputs of the 3-D loader tests and of tests/golden/make_golden_dataloader_3d.py: a tiny `3d_fullres`-style case
folder and the three loader settings the fixture pins."""
import os
import pickle

import numpy as np

from oracle import dataloading_oracle as DO

LABELS = [0, 1, 2, 3]
# tag -> (unpacked .npy, loader patch, final patch, batch size, oversample_foreground_percent)
CASES = {"npz": (False, (8, 14, 12), (6, 12, 10), 3, 0.33), "npy": (True, (8, 12, 12), (8, 12, 12), 4, 0.5),
         "ign": (True, (9, 14, 13), (6, 12, 12), 4, 0.33)}     # "ign": partially annotated cases (ignore label 4)


def write_dataset_3d(folder, n_cases=4, seed=5, labels=(1, 2, 3), unpack=False, ignore_label=None):
    """<case>.npz {data (1, X, Y, Z) f32, seg (1, X, Y, Z) i16, -1 outside the 'nonzero' region} + <case>.pkl
    {class_locations (sampled as the preprocessor does)}.  Case 1 has no foreground, case 2 is thinner than every loader
    patch along x.  Data values are multiples of 1/8 so the fixture compresses."""
    os.makedirs(folder, exist_ok=True)
    rng = np.random.RandomState(seed)
    for i in range(n_cases):
        X, Y, Z = (12 + 2 * i, 22 - 2 * i, 16 + 3 * i)
        if i == 2:
            X = 5
        data = (rng.randint(-40, 40, (1, X, Y, Z)) / 8.0).astype(np.float32)
        seg = np.zeros((1, X, Y, Z), dtype=np.int16)
        if i != 1:
            for lab in labels:
                x, y, z = rng.randint(0, X - 2), rng.randint(2, Y - 5), rng.randint(2, Z - 5)
                seg[0, x:x + 2, y:y + 4, z:z + 4] = lab
        seg[0, :, :2, :] = -1
        if ignore_label is not None:
            seg[0, :, Y // 2:Y // 2 + 3, :] = ignore_label
            locs = DO.sample_locations_of(seg, list(labels) + [[0] + list(labels)])
        else:
            locs = DO.sample_foreground_locations(seg, list(labels))
        name = f"case_{i:03d}"
        np.savez_compressed(os.path.join(folder, name + ".npz"), data=data, seg=seg)
        with open(os.path.join(folder, name + ".pkl"), "wb") as fh:
            pickle.dump({"class_locations": locs}, fh)
        if unpack:
            np.save(os.path.join(folder, name + ".npy"), data)
            np.save(os.path.join(folder, name + "_seg.npy"), seg)
