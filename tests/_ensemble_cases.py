"""Inputs shared by tests/golden/make_golden_ensemble.py, tests/test_ensemble_cpu.py and tests/test_ensemble_gpu.py (K28): ensemble
members, label volumes for the confusion matrix and metrics, and the candidates of the model-selection constructions.

Members are softmaxes of seeded random logits.  The logits are integer multiples of ln 2, so that exp(logit) is an exact power of two
and each probability is one correctly rounded float64 division rounded once to fp32 (or fp16): the inputs are the same bits on every
machine, which the bit-equal comparison with the recorded means needs.  Voxels are redrawn until the two largest fp32 means are exactly
equal or at least MARGIN apart (see make_golden_ensemble.py for why)."""
import numpy as np

MARGIN = 1e-3


def mean_fp32(members):
    """((m_0 + m_1) + ...) / M in fp32: the arithmetic every path has to reproduce."""
    acc = members[0].astype(np.float32)
    for m in members[1:]:
        acc = acc + m.astype(np.float32)
    return acc / np.float32(len(members))


def _softmax_pow2(rng, M, K, n, spread):
    l = rng.integers(-spread, spread + 1, size=(M, K, n))
    e = np.ldexp(1.0, l)
    return e / e.sum(1, keepdims=True)


def _gap_ok(members):
    mean = mean_fp32(members).reshape(members[0].shape[0], -1)
    top = np.sort(mean, 0)[-2:]
    return (top[1] == top[0]) | (top[1] - top[0] >= MARGIN)


def make_members(K, M, shape, seed, dtypes=None, spread=6):
    """M members (K, *shape); dtypes: one numpy dtype per member (default fp32)."""
    dtypes = [np.float32] * M if dtypes is None else list(dtypes)
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    p = _softmax_pow2(rng, M, K, n, spread)
    for _ in range(200):
        members = [p[i].astype(dtypes[i]) for i in range(M)]
        bad = np.flatnonzero(~_gap_ok(members))
        if bad.size == 0:
            return [m.reshape((K,) + tuple(shape)) for m in members]
        p[:, :, bad] = _softmax_pow2(rng, M, K, bad.size, spread)
    raise RuntimeError("no margin found")


def _ties():
    """K = 4, M = 2, 8 voxels: planted exact ties on top of drawn members."""
    m = make_members(4, 2, (2, 4), 10)
    a, b = m[0].reshape(4, 8), m[1].reshape(4, 8)
    a[:, 0], b[:, 0] = (0.1, 0.4, 0.1, 0.4), (0.2, 0.3, 0.2, 0.3)          # classes 1 and 3 tie for the maximum: 1 wins
    a[:, 1], b[:, 1] = (0.25,) * 4, (0.25,) * 4                           # all equal: 0 wins
    a[:, 2], b[:, 2] = (0.0,) * 4, (0.0,) * 4                             # an all-zero voxel: 0 wins
    a[:, 5], b[:, 5] = (0.125, 0.125, 0.375, 0.375), (0.125, 0.125, 0.375, 0.375)      # the last two tie: 2 wins
    return [a.reshape(4, 2, 4), b.reshape(4, 2, 4)]


def _views():
    """Members that are views at an odd element offset into larger buffers (fp32: 4 and 12 bytes past a 16-byte boundary)."""
    out = []
    for i, m in enumerate(make_members(3, 2, (4, 4, 4), 9)):
        off = 1 + 2 * i
        buf = np.zeros(m.size + 8, np.float32)
        buf[off:off + m.size] = m.ravel()
        out.append(buf[off:off + m.size].reshape(m.shape))
    return out


ENSEMBLES = {
    "a_odd": lambda: make_members(2, 2, (5, 7, 3), 1),
    "b_btcv": lambda: make_members(14, 5, (8, 16, 16), 2),
    "c_single": lambda: make_members(3, 1, (6, 5, 4), 3),
    "d_fp16": lambda: make_members(4, 3, (5, 6, 4), 4, [np.float16] * 3),
    "d_mixed": lambda: make_members(4, 3, (5, 6, 4), 5, [np.float16, np.float32, np.float32]),
    "e_many": lambda: make_members(5, 9, (6, 6, 5), 6),
    "f_k33": lambda: make_members(33, 2, (4, 5, 3), 7),
    "g_k256": lambda: make_members(256, 2, (3, 5, 2), 8, spread=8),
    "h_one": lambda: make_members(3, 2, (1,), 11),
    "i_views": _views,
    "j_ties": _ties,
}
VIEW_OFFSETS = (1, 3)                                   # i_views: the element offsets of the two members in their buffers


def nan_members():
    """Case k: one voxel with a NaN in class 2 of one member (host path against device path only)."""
    m = make_members(4, 2, (3, 5), 12)
    m[1][2, 1, 3] = np.nan
    return m


# ---- confusion matrix and metrics ---------------------------------------------------------------------------------------------------
LABELS = [0, 1, 2, 3, 4]
REGIONS = [(1, 3), 2]
CHUNK = 256 * 16                                        # voxels a workgroup of label_confusion_kernel takes per step


def _volume_pair(shape, seed, n_labels=5, agree=0.7):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, n_labels, size=shape).astype(np.uint8)
    # mostly constant along the last axis, as label volumes are
    ref = np.repeat(ref[..., ::3], 3, axis=-1)[..., :shape[-1]] if shape[-1] >= 3 else ref
    noise = rng.integers(0, n_labels, size=shape).astype(np.uint8)
    pred = np.where(rng.random(shape) < agree, ref, noise).astype(np.uint8)
    return ref, pred


def _main_case():
    """(6, 9, 5), labels 0..4: a value 9 outside the label list, ignore label 4 under foreground predictions, class 3 absent from both
    volumes (NaN Dice), class 2 absent from the reference only."""
    ref, pred = _volume_pair((6, 9, 5), 21)
    ref[ref == 3] = 1
    pred[pred == 3] = 0
    ref[ref == 2] = 0
    ref[0, 0, :3] = 9
    pred[5, 8, 2:] = 9
    ref[2, 3:6, :] = 4
    pred[2, 3:6, :] = (1, 2, 1, 0, 2)
    pred[pred == 4] = 1
    return ref, pred


def _flat(n, seed):
    ref, pred = _volume_pair((n,), seed)
    return ref, pred


VOLUMES = {
    "main": _main_case,
    "two_d": lambda: _volume_pair((1, 37, 41), 22),
    "constant": lambda: (np.full((7, 8, 9), 2, np.uint8), np.full((7, 8, 9), 2, np.uint8)),
    "chunk_minus": lambda: _flat(CHUNK - 1, 23),
    "chunk_plus": lambda: _flat(CHUNK + 1, 24),
    "blocks": lambda: _volume_pair((3, 70, 64), 25),       # more than one workgroup
}
# (volume, labels_or_regions, ignore_label)
METRIC_CASES = {
    "main_labels": ("main", LABELS, None),
    "main_ignore": ("main", LABELS, 4),
    "main_regions": ("main", REGIONS, 4),
    "two_d": ("two_d", LABELS, None),
    "constant": ("constant", LABELS, None),
    "chunk_minus": ("chunk_minus", LABELS, 4),
    "chunk_plus": ("chunk_plus", LABELS, None),
    "blocks": ("blocks", [1, 2, (3, 4)], None),
}
# compute_metrics_on_folder over several cases: (volumes, labels_or_regions, ignore_label)
FOLDERS = {
    "labels": (("main", "constant", "blocks"), [1, 2, 3, 4], None),
    "regions": (("main", "blocks"), REGIONS, 4),
}


def folder_volumes(names):
    """The volumes of a folder set as same-rank arrays (the .npy reader of the generator returns them with a leading axis)."""
    return [VOLUMES[n]() for n in names]


# ---- model selection ----------------------------------------------------------------------------------------------------------------
SEL_SHAPE = (8, 12, 12)
SEL_CASES = ("case_0", "case_1", "case_2", "case_3")
SEL_LABELS = [1, 2]
SEL_FOLDS = (0, 1, 2, 3, 4)
IDS = ("nnUNetTrainer__nnUNetPlans__2d", "nnUNetTrainer__nnUNetPlans__3d_fullres", "nnUNetTrainer__nnUNetPlans__3d_lowres")


def _sel_reference(i):
    ref = np.zeros(SEL_SHAPE, np.uint8)
    ref[1:5, 2:8, 2 + i:7 + i] = 1
    ref[5:8, 5:11, 1:6] = 2
    return ref


def _probs_for(ref, wrong, strength):
    """Probabilities (3, ...) built from exact binary fractions: `strength` on the reference class, except on the mask `wrong`, where
    the next class (cyclically) gets it; the rest is shared equally."""
    K = 3
    target = np.where(wrong, (ref.astype(np.int64) + 1) % K, ref.astype(np.int64))
    p = np.full((K,) + ref.shape, (1.0 - strength) / 2, np.float32)
    np.put_along_axis(p, target[None], np.float32(strength), 0)
    return p


def _stripe(axis, lo, hi):
    m = np.zeros(SEL_SHAPE, bool)
    sl = [slice(None)] * 3
    sl[axis] = slice(lo, hi)
    m[tuple(sl)] = True
    return m


def selection(tag):
    """(candidates, references) of one construction.  candidates: {identifier: {case: (labels, probabilities or None)}}.
      ensemble_wins  two candidates are wrong on disjoint stripes with weak confidence and right elsewhere with strong confidence, so
                     their ensemble is right everywhere; the third is wrong on both stripes;
      tie            the first candidate is perfect, and so is the ensemble of the first two: the single model must win;
      unpaired       as ensemble_wins, but the second candidate holds no probabilities: it is scored and never paired."""
    refs = {c: _sel_reference(i) for i, c in enumerate(SEL_CASES)}
    s1, s2 = _stripe(2, 2, 5), _stripe(1, 6, 9)
    cands = {}
    for c, ref in refs.items():
        if tag == "tie":
            layout = ((np.zeros(SEL_SHAPE, bool), 0.75), (s1, 0.5), (s1 | s2, 0.75))
        else:
            layout = ((s1, 0.5), (s2, 0.5), (s1 | s2, 0.75))
        for name, (wrong, weak) in zip(IDS, layout):
            p = np.where(wrong[None], _probs_for(ref, wrong, weak), _probs_for(ref, wrong, 0.75)).astype(np.float32)
            keep = not (tag == "unpaired" and name == IDS[1])
            cands.setdefault(name, {})[c] = (p.argmax(0).astype(np.uint8), p if keep else None)
    return cands, refs


SELECTIONS = ("ensemble_wins", "tie", "unpaired")
