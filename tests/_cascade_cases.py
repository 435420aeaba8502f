"""Shared inputs and the oracle of the cascade tests (K30): the definitions of binary dilation / erosion with an arbitrary footprint,
the "was added" rule and the random component removal, written out in plain numpy + scipy."""
import os

import numpy as np
from scipy import ndimage as ndi

OPERATIONS = ("dilation", "erosion", "closing", "opening")
RADII = {1.0: 3, 1.5: 4, 2.5: 6, 5.49: 11, 8.0: 17}                    # ball radius -> entries per axis


def shifted(x, d, fill):
    """y[p] = x[p + d], `fill` where p + d leaves the volume"""
    y = np.full(x.shape, fill, dtype=bool)
    src = tuple(slice(max(0, k), min(n, n + k)) for k, n in zip(d, x.shape))
    dst = tuple(slice(max(0, -k), min(n, n - k)) for k, n in zip(d, x.shape))
    if all(s.stop > s.start for s in src):
        y[dst] = x[src]
    return y


def dilation(x, S):
    """out[p] = OR over set S[i] of in[p - (i - c)], 0 outside; c = n // 2"""
    c = np.array(S.shape) // 2
    out = np.zeros(x.shape, dtype=bool)
    for i in np.argwhere(S):
        out |= shifted(x, -(i - c), False)
    return out


def erosion(x, S):
    """out[p] = AND over set S[i] of in[p + (i - c)], 1 outside"""
    c = np.array(S.shape) // 2
    out = np.ones(x.shape, dtype=bool)
    for i in np.argwhere(S):
        out &= shifted(x, i - c, True)
    return out


def operation(x, op, S):
    return {"dilation": lambda: dilation(x, S), "erosion": lambda: erosion(x, S), "closing": lambda: erosion(dilation(x, S), S),
            "opening": lambda: dilation(erosion(x, S), S)}[OPERATIONS[op]]()


def scipy_operation(x, op, S):
    d = lambda m: ndi.binary_dilation(m, structure=S)                                   # noqa: E731
    e = lambda m: ndi.binary_erosion(m, structure=S, border_value=True)                 # noqa: E731
    return {"dilation": lambda: d(x), "erosion": lambda: e(x), "closing": lambda: e(d(x)), "opening": lambda: d(e(x))}[OPERATIONS[op]]()


def random_footprint(shape, seed):
    S = np.random.RandomState(seed).rand(*shape) < 0.45
    S[0, 0, 0] = S[-1, -1, -1] = True                       # the full extent, corner to corner
    return S


def multi_run_footprint():
    """5 x 4 x 3, rows with two runs (1 0 1), without its centre"""
    S = random_footprint((5, 4, 3), 11)
    S[:, :, 1] = False
    S[2, 1] = [True, False, True]
    return S


def draw_literal(rng, B, L, order):
    """The reference's draw order of the morphology parameters, as a literal loop"""
    out = []
    for b in range(B):
        steps = []
        if rng.uniform() < 0.4:
            rng.shuffle(order)
            for c in order:
                if rng.uniform() < 1:
                    op = rng.choice(4)
                    steps.append((c, op, rng.uniform(1, 8)))
        out.append(steps)
    return out


def oracle(seg_prev, labels, params, rng, p_per_sample=0.2, fill_p=0.0, frac=0.15, p_per_label=1.0, footprint_of=None):
    """One-hot channels (B, L, X, Y, Z) bool after the morphology steps and the component removal"""
    onehot = np.stack([seg_prev == lab for lab in labels], 1)
    B, L = onehot.shape[:2]
    for b in range(B):
        for c, op, strel in params[b]:
            before = onehot[b, c].copy()
            if not before.any():
                continue
            res = operation(before, op, footprint_of(strel) if np.ndim(strel) == 0 else np.asarray(strel, dtype=bool))
            onehot[b, c] = res
            for oc in range(L):
                if oc != c:
                    onehot[b, oc][res & ~before] = False
    n_vox = np.prod(onehot.shape[2:], dtype=np.uint64)
    for b in range(B):
        if rng.uniform() < p_per_sample:
            for c in range(L):
                if rng.uniform() < p_per_label:
                    if not onehot[b, c].any():
                        continue
                    lab, n = ndi.label(onehot[b, c], structure=np.ones((3, 3, 3)))
                    valid = [i for i in range(1, n + 1) if (lab == i).sum() < n_vox * frac]
                    if valid:
                        comp = lab == valid[rng.choice(len(valid))]
                        onehot[b, c][comp] = False
                        if rng.uniform() < fill_p:
                            other = [i for i in range(L) if i != c]
                            if other:
                                onehot[b, rng.choice(other)][comp] = True
    return onehot


def valid_components(plane, frac=0.15):
    """(label map, ids of the components with size < N * frac in label order)"""
    lab, n = ndi.label(plane, structure=np.ones((3, 3, 3)))
    n_vox = np.prod(plane.shape, dtype=np.uint64)
    return lab, [i for i in range(1, n + 1) if (lab == i).sum() < n_vox * frac]


COMPONENT_SHAPE = (10, 17, 70)            # spans the 8 x 8 x 32 union-find tiles and the word border at z = 64


def component_planes():
    """Two planes: 0 holds a component snaking across tile corners and the word border through 26-only (diagonal) steps, a
    diagonal line and several small components; 1 holds one component of >= 15 % of the volume and two small ones."""
    a = np.zeros(COMPONENT_SHAPE, dtype=bool)
    a[7, 7, 20:32] = True                 # ... (7, 7, 31) -> (8, 8, 32): across the corner of four tiles, diagonally
    a[8, 8, 32:64] = True                 # ... (8, 8, 63) -> (9, 9, 64): across the word border, diagonally
    a[9, 9, 64:69] = True
    a[9, 10:16, 69] = True                # and on along y across the tile face at y = 16
    a[8, 16, 68] = True
    for i in range(6):                    # a diagonal: 26-connectivity only
        a[i, 2 + i, 40 + i] = True
    a[0, 0, 0] = a[9, 16, 0] = a[0, 16, 69] = True       # single voxels in three corners
    a[3:5, 12:14, 62:66] = True           # a block across the word border
    a[0, 4, 31] = a[0, 5, 32] = True      # a diagonal pair across the tile face at z = 32
    b = np.zeros(COMPONENT_SHAPE, dtype=bool)
    b[:, :, 5:17] = True                  # 2040 of 11900 voxels: >= 15 %
    b[2, 3, 30] = True
    b[5:7, 9, 63:65] = True
    return np.stack([a, b])


def small_component_planes():
    """{name: (1, X, Y, Z) planes} at the edges of the labelling's 8 x 8 x 32 tile and of the 64-bit word, next to the ragged
    COMPONENT_SHAPE"""
    chain = np.zeros((16, 8, 128), dtype=bool)       # every extent a multiple of the tile and of the word
    chain[7, 7, 20:32] = True                        # ... (7, 7, 31) -> (8, 6, 32): across the tile corner, diagonally
    chain[8, 6, 32:64] = True                        # ... (8, 6, 63) -> (9, 7, 64): across the word border, diagonally
    chain[9, 7, 64:100] = True
    chain[0, 0, 0] = chain[15, 7, 127] = True        # two single voxels
    return {"1x1x1": np.ones((1, 1, 1, 1), dtype=bool),
            "8x8x32": np.ones((1, 8, 8, 32), dtype=bool),         # exactly one tile, no face and no tail
            "16x8x128": chain[None]}


def seg_from_planes(planes, labels):
    """int16 label map whose listed labels are the (disjoint) planes; elsewhere 0"""
    seg = np.zeros(planes.shape[1:], dtype=np.int16)
    for p, lab in zip(planes, labels):
        seg[p] = lab
    return seg


def cascade_label_map(shape, seed, labels=(1, 2, 3)):
    """A previous-stage-like label map: blobs of each label, -1 outside a margin, and a label that is in no list (7)"""
    rng = np.random.RandomState(seed)
    seg = np.zeros(shape, dtype=np.int16)
    for lab in list(labels) + [7]:
        for _ in range(3):
            lo = [rng.randint(0, max(1, n - 6)) for n in shape]
            ext = [rng.randint(2, 7) for _ in shape]
            seg[tuple(slice(a, a + e) for a, e in zip(lo, ext))] = lab
    seg[:, :1, :] = -1
    return seg


def write_previous_stage(folder, case_folder, unpack=False):
    """<case>.npz {seg (X, Y, Z)} per case of case_folder: the case's labels moved by one voxel along y (a stand-in for the
    lowres prediction)"""
    os.makedirs(folder, exist_ok=True)
    for name in sorted(f[:-4] for f in os.listdir(case_folder) if f.endswith(".npz")):
        seg = np.load(os.path.join(case_folder, name + ".npz"))["seg"][0]
        prev = np.roll(np.maximum(seg, 0), 1, axis=1).astype(np.int16)
        np.savez_compressed(os.path.join(folder, name + ".npz"), seg=prev)
        if unpack:
            np.save(os.path.join(folder, name + ".npy"), prev)
