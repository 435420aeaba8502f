"""The cases of tests/_step_tail_cases.py are what they claim to be, checked without a GPU.

The path predicates agree with the library's host queries (workspace sizes, chunk size, class and head limits); the case tables reach
every value a predicate can return and both sides of every threshold (taking a boundary case out of a table fails here); every
reference value is finite and the plain-fp32 yardstick meets the bounds the device test uses, i.e. the inputs are well conditioned and
a failure on the device means the kernel; and the defects the cases are meant to catch -- a dropped ragged workgroup, a dropped odd
partial row, CE partials beyond the first 256 dropped, one sample's g_ip used for all, dropped heads, a chunk tail or a last chunk not
updated, a tensor missing from the norm -- applied to the float64 reference, land at least 10 x outside those bounds."""
import collections

import pytest
import torch

from tests import _step_tail_cases as K


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    from mlagg_unet_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------
# predicates against the library
# ---------------------------------------------------------------------------------------------------------------------
def test_loss_predicates_match_the_workspace_queries(lib):
    assert lib.mlagg_dice_ce_max_classes() == K.K9_MAXC and lib.mlagg_dice_bce_max_regions() == K.K29_MAXR
    sizes = {K.hw_of(c) for c in K.K9_CASES + K.K29_CASES} | {1, 1023, 1024, 1025, 2048, 1 << 21, (1 << 21) + 1, 1 << 31}
    for HW in sorted(sizes):
        nblk = K.loss_workgroups(HW)
        assert (nblk - 1) * K.LOSS_PIX < HW <= nblk * K.LOSS_PIX and 1 <= K.loss_last_workgroup_pixels(HW) <= K.LOSS_PIX
        for B, n in ((1, 2), (3, 16), (2, 5)):
            assert lib.mlagg_dice_ce_stats_workspace_floats(B, n, HW) == K.k9_workspace_floats(B, n, HW), (B, n, HW)
            assert lib.mlagg_dice_bce_stats_workspace_floats(B, n, HW) == K.k29_workspace_floats(B, n, HW), (B, n, HW)
    for c in K.K9_CASES:
        assert lib.mlagg_dice_ce_stats_workspace_floats(c.B, c.C, K.hw_of(c)) == c.B * K.loss_workgroups(K.hw_of(c)) * (3 * c.C + 1)
    for c in K.K29_CASES:
        assert lib.mlagg_dice_bce_stats_workspace_floats(c.B, c.R, K.hw_of(c)) == c.B * K.loss_workgroups(K.hw_of(c)) * (3 * c.R + 2)
    assert [K.reduce_rows(n) for n in (1, 2, 3, 4, 101, 2064)] == ["one", "even", "odd", "even", "odd", "even"]
    assert [K.ce_trips(3, n) for n in (1, 85, 86, 101)] == [1, 1, 2, 2] and K.ce_trips(1, 2064) == 9
    assert [K.k29_rb(R) for R in range(1, 17)] == [4] * 4 + [8] * 4 + [16] * 8


def test_k11_predicates_match_the_library(lib):
    assert lib.mlagg_adamw_chunk_elements() == K.K11_CHUNK
    assert [K.k11_chunks(n) for n in (1, 65535, 65536, 65537, 131072, 131073)] == [1, 1, 1, 2, 2, 3]
    for n in K.K11_SIZES + (70001, 77100):
        n4, tail = K.k11_last_chunk(n)
        assert (K.k11_chunks(n) - 1) * K.K11_CHUNK + 4 * n4 + tail == n and 0 <= tail < 4
    assert K.k11_grad_offsets((1, 48, 7)) == [0, 1, 49]
    base = 0x7F0000000000
    assert K.k11_sumsq_path(base) == "vector" and {K.k11_sumsq_path(base + 4 * k) for k in (1, 2, 3)} == {"scalar"}
    assert K.k11_update_path(base, base + 16, base + 32, base + 48) == "vector"
    for which in range(4):                                                         # every one of the four addresses decides
        for off in (4, 8, 12):
            addrs = [base + 64 * k + (off if k == which else 0) for k in range(4)]
            assert K.k11_update_path(*addrs) == "scalar", (which, off)


# ---------------------------------------------------------------------------------------------------------------------
# coverage: what the tables must reach (each line names the boundary it needs)
# ---------------------------------------------------------------------------------------------------------------------
def _share_ignored(case):
    return float((K.inputs(case)["target"] == case.ignore).float().mean())


def test_k9_cases_cover_the_pixel_counts_classes_and_labels():
    plain = [c for c in K.K9_CASES if c.regime == "unit" and not c.tweak]
    want = {1, 63, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 3 * 1024 + 1}
    small = [c for c in plain if c.B == 3 and c.C == 3 and c.ignore is None and K.hw_of(c) in want]
    top = [c for c in plain if c.B == 1 and c.C == 16 and c.ignore == 16]
    assert {K.hw_of(c) for c in small} == want == {K.hw_of(c) for c in top}
    assert len({c.dims for c in small if len(c.dims) == 3}) >= 2                   # 3-D logits (B, C, D, H, W)
    assert {K.loss_workgroups(hw) for hw in want} == {1, 2, 3, 4}
    assert {K.reduce_rows(K.loss_workgroups(hw)) for hw in want} == {"one", "even", "odd"}
    assert {K.loss_last_workgroup_pixels(hw) for hw in want} == {1, 63, 255, 256, 257, 1023, 1024}
    # many CE partials: more than one trip of the reducer's scalar loop, an odd row count
    many = [c for c in plain if c.B * K.loss_workgroups(K.hw_of(c)) > K.REDUCE_TPB and c.B > 1]
    assert many and all(K.reduce_rows(K.loss_workgroups(K.hw_of(c))) == "odd" and K.ce_trips(c.B, K.loss_workgroups(K.hw_of(c))) == 2 for c in many)
    # the long sum: a 128^3 patch's partial-row count, ragged
    long = [c for c in plain if c.B == 1 and c.C == 2 and K.hw_of(c) > 1 << 21]
    assert long and all(len(c.dims) == 3 and K.hw_of(c) % K.LOSS_PIX and 2048 <= K.loss_workgroups(K.hw_of(c)) < 2100 for c in long)
    assert max(K.hw_of(c) for c in K.K9_CASES) == K.hw_of(long[0])                  # ... and nothing larger (the suite stays quick)
    # class counts, MAXC included: thread 3 * 16 = 48 writes the CE partial
    assert {c.C for c in K.K9_CASES if c.dims == K.RAGGED} >= {2, 3, 15, 16} and K.k9_ce_writer(K.K9_MAXC) == 48
    assert max(c.C for c in K.K9_CASES) == K.K9_MAXC
    # the ignore label is the class count (nnU-Net's convention), at MAXC too, with a share of ignored pixels
    for C in (3, 16):
        mine = [c for c in K.K9_CASES if c.C == C and c.ignore == C and c.dims == K.RAGGED and c.B == 3 and not c.tweak]
        assert mine and all(0.15 < _share_ignored(c) < 0.35 for c in mine), C
    gone = next(c for c in K.K9_CASES if c.tweak == "sample_ignored")
    t = K.inputs(gone)["target"]
    assert bool((t[-1] == gone.ignore).all()) and not bool((t[0] == gone.ignore).all())
    ref = K.evaluate(next(c for c in K.K9_CASES if c.tweak == "class_absent_sample"))
    assert float(ref["gt"][0, 1]) == 0.0 and float(ref["gt"][1, 1]) > 0.0 and float(ref["gt"][0].sum()) == 1025.0
    ref = K.evaluate(next(c for c in K.K9_CASES if c.tweak == "class_absent_batch"))
    assert float(ref["gt"][:, 2].sum()) == 0.0 and float(ref["gt"][:, :2].min()) > 0.0
    # logit regimes at one ragged size; a slice of a wider tensor
    assert {c.regime for c in K.K9_CASES if c.dims == K.RAGGED and c.B == 3 and c.C == 3 and c.ignore is None and not c.tweak} == \
        {"unit", "sat", "shift", "ties"}
    z = {r: K.inputs(next(c for c in K.K9_CASES if c.regime == r))["logits"] for r in ("sat", "shift", "ties")}
    assert float(z["sat"].std()) > 25 and float(z["shift"].min()) > 70 and float(z["ties"].abs().max()) < 1e-2
    assert any(c.tweak == "slice" for c in K.K9_CASES)
    # through the loss, both batch_dice values: every kind of case once
    through = [c for c in K.K9_CASES if c.loss]
    assert {c.regime for c in through} == {"unit", "sat", "shift", "ties"} and {c.C for c in through} >= {2, 3, 16}
    assert {c.tweak for c in through} >= {"", "sample_ignored", "class_absent_batch", "slice"}
    assert {(c.C, c.ignore) for c in through} >= {(3, 3), (16, 16)} and any(len(c.dims) == 3 for c in through)


def test_k29_cases_cover_the_variants_forms_and_pixel_counts():
    heads = [c for c in K.K29_CASES if c.dims == K.RAGGED and c.regime == "unit"]
    for form in K.K29_FORMS:
        for ign in (False, True):
            mine = {c.R for c in heads if c.form == form and c.ignore == ign}
            assert mine == {1, 4, 5, 8, 9, 16}, (form, ign)                         # both sides of each RB threshold
            assert {K.k29_rb(R) for R in mine} == {4, 8, 16}
            assert {R for R in mine if K.k29_rb(R) == 8} == {5, 8}                  # the variant no earlier test ran
    assert max(c.R for c in K.K29_CASES) == K.K29_MAXR
    for form in K.K29_FORMS:
        mine = [c for c in K.K29_CASES if c.form == form and c.regime == "unit"]
        assert {K.hw_of(c) for c in mine} >= {1023, 1024, 1025, 4 * 1024 + 3}
        assert {K.reduce_rows(K.loss_workgroups(K.hw_of(c))) for c in mine} == {"one", "even", "odd"}
        assert any(c.B * K.loss_workgroups(K.hw_of(c)) > K.REDUCE_TPB and c.ignore for c in mine)
        big = [c for c in K.K29_CASES if c.form == form and c.regime == "big"]
        assert {c.ignore for c in big} == {False, True}
        assert all(95.0 < float(K.inputs(c)["logits"].abs().max()) <= 100.0 for c in big)
    c = next(c for c in K.K29_CASES if c.ignore and c.R == 16)                      # the label map: labels 0 .. R and the ignore label
    seg = K.inputs(c)["seg"]
    assert set(seg.unique().tolist()) == set(float(v) for v in range(18)) and 0.15 < float((seg == 17).float().mean()) < 0.25
    assert K.k29_planes(c, seg).shape == (2, 17) + K.RAGGED and K.k29_regions(3) == [(1, 2, 3), (2, 3), (3,)]


def test_k11_cases_cover_both_paths_every_tail_and_every_regime():
    seen = collections.defaultdict(set)
    for lead in K.K11_LEADS:
        case = K.K11Case(lead, "unit", 12.0, False)
        assert case in K.K11_CASES
        sizes = K.k11_sizes(case)
        assert sizes[-len(K.K11_SIZES):] == K.K11_SIZES
        for n, off in list(zip(sizes, K.k11_grad_offsets(sizes)))[-len(K.K11_SIZES):]:
            seen[n].add(off % 4)
        paths = {K.k11_sumsq_path(4 * off) for off in K.k11_grad_offsets(sizes)}
        assert paths == {"vector", "scalar"}, lead                                  # both paths in every case, in both kernels
    for n in K.K11_SIZES:                                                           # every size aligned AND misaligned
        assert 0 in seen[n] and seen[n] - {0}, (n, seen[n])
    assert set().union(*seen.values()) == {0, 1, 2, 3}                              # 4-, 8- and 12-byte misalignment
    assert set(K.K11_SIZES) >= {1, 2, 3, 4, 5, 7, 65535, 65536, 65537, 65539, 131072, 131073}
    assert {K.k11_chunks(n) for n in K.K11_SIZES} == {1, 2, 3}
    last = {n: K.k11_last_chunk(n) for n in K.K11_SIZES}
    assert last[65537] == (0, 1) == last[131073] and last[65539] == (0, 3)          # a chunk of one element, of a tail alone
    assert last[65535] == (16383, 3) and last[65536] == (16384, 0) == last[131072]
    assert {last[n] for n in (1, 2, 3, 4, 5, 7)} == {(0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 3)}
    assert {c.regime for c in K.K11_CASES} == {"unit", "small", "dominated", "zero", "near_below", "near_above"}
    assert {c.max_norm for c in K.K11_CASES if c.regime == "unit" and not c.resume} == {12.0, 0.05, 0.0}
    assert {c.max_norm for c in K.K11_CASES if c.regime == "zero"} == {12.0, 0.05, 0.0}
    for r in ("near_below", "near_above"):
        assert {c.max_norm for c in K.K11_CASES if c.regime == r} == {12.0, 0.05}
    assert {c.max_norm for c in K.K11_CASES if c.resume} == {0.05, 0.0}
    assert {(c.n, c.misaligned) for c in K.K11_ABI_CASES} == {(n, w) for n in (5, 65537) for w in ("none", "p", "g", "m", "v")}


def test_k11_regimes_are_what_they_are_called():
    def norms(case):
        return [float(torch.sqrt(sum((a.double() ** 2).sum() for a in gs))) for gs in K.inputs(case)["grads"]]
    assert all(n > 12.0 for n in norms(K.K11Case(0, "unit", 12.0, False)))          # clipped at both max_norms
    assert all(0.05 < n < 12.0 for n in norms(K.K11Case(0, "small", 12.0, False)))  # not clipped at 12
    assert norms(K.K11Case(0, "zero", 12.0, False)) == [0.0] * K.K11_STEPS
    t = K.inputs(K.K11Case(0, "dominated", 12.0, False))
    for gs in t["grads"]:
        one = float((gs[K.K11_SIZES.index(65537)].double() ** 2).sum())
        assert one / sum(float((a.double() ** 2).sum()) for a in gs) > 1.0 - 1e-12
    for mn in (12.0, 0.05):
        assert all(mn * (1 - 1e-3) < n < mn * (1 - 1e-4) for n in norms(K.K11Case(2, "near_below", mn, False)))
        assert all(mn * (1 + 1e-4) < n < mn * (1 + 1e-3) for n in norms(K.K11Case(2, "near_above", mn, False)))
        ref = K.evaluate(K.K11Case(2, "near_below", mn, False))                      # the clamp at 1 holds on this side ...
        assert all(float(n) + 1e-6 < mn for n in ref["norm"])
    t = K.inputs(K.K11Case(3, "unit", 0.05, True))
    assert all(step == 999 and float(v.min()) > 0.0 for step, m, v in t["state0"])


# ---------------------------------------------------------------------------------------------------------------------
# references and yardstick
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = ("k9", "k29", "k11", "k11abi")
ALL_CASES = [c for fam in FAMILIES for c in K.CASES[fam]]
ALL_IDS = [K.family(c) + "-" + K.case_id(c) for c in ALL_CASES]
_YARDSTICK = {}                                       # case -> {quantity: (yardstick error, bound)}


def test_case_ids_are_unique():
    assert len(set(ALL_IDS)) == len(ALL_IDS) == len(set(ALL_CASES))


def _yardstick(case):
    if case not in _YARDSTICK:
        ref, yard = K.reference_and_yardstick(case)
        tols = K.bounds(case, ref, yard)
        assert set(tols) == set(ref) == set(yard)
        out = {}
        for q, tol in tols.items():
            for side, dt in ((ref[q], torch.float64), (yard[q], torch.float32)):
                for a in (side if isinstance(side, list) else [side]):
                    assert a.dtype == dt and bool(torch.isfinite(a).all()), q
            out[q] = (K.error(yard[q], ref[q], tol), tol.a, K.tolerances(case)[q].a)
        _YARDSTICK[case] = out
    return _YARDSTICK[case]


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_reference_is_finite_and_the_plain_fp32_yardstick_meets_the_bounds(case):
    for q, (err, bound, existing) in _yardstick(case).items():
        print(f"YARDSTICK {K.family(case)} {K.case_id(case)} {q} {err:.2e} bound {bound:.2e}" + (" WIDENED" if bound > existing else ""))
        assert err <= bound, (q, err, bound)
        assert bound <= 2.0 * existing, (q, bound, existing)      # a case that needs more than that is badly conditioned: change its inputs
    fam = K.family(case)
    assert {"k9": {"ip", "gt", "ce", "dlogits"}, "k29": {"ip", "gt", "bce", "mask", "dlogits"}}.get(fam, {"p", "exp_avg", "exp_avg_sq"}) <= \
        set(_yardstick(case))
    if fam == "k9":
        assert ("loss_bd1" in _yardstick(case)) == ("dloss_bd0" in _yardstick(case)) == case.loss
    if fam in ("k11", "k11abi"):
        assert ("norm" in _yardstick(case)) == (fam == "k11abi" or case.max_norm > 0)


def test_print_the_yardstick_table():
    """The table of the case file's docstring: the largest yardstick error per case group and quantity."""
    table = collections.OrderedDict()
    for case in ALL_CASES:
        row = table.setdefault(K.group(case), collections.OrderedDict())
        for q, (err, _, _) in _yardstick(case).items():
            if K.tolerances(case)[q].kind != "exact":
                q = q[:-4] if q.startswith(("loss_bd", "dloss_bd")) else q       # both batch_dice values in one column
                row[q] = max(row.get(q, 0.0), err)
    print()
    print("    cases                                      quantity and error")
    for name, row in table.items():
        print(f"    {name:<43}" + "  ".join(f"{q} {e:.1e}" for q, e in row.items()))
    widened = sorted({(K.group(c), q) for c in ALL_CASES for q, (_, b, e) in _yardstick(c).items() if b > e})
    print("    widened bounds:", widened if widened else "none")
    assert len(table) == 15


def test_the_loss_formula_of_the_case_file_is_the_eager_composition():
    """k9_loss, which turns the reference statistics into the reference loss, against the level-by-level torch composition of
    DC_and_CE_loss (the form pinned to the reference's loss classes by tests/golden/loss.npz), in float64."""
    from mlagg_unet_amd import trainer
    for case in (c for c in K.K9_CASES if c.loss):
        t = K.inputs(case)
        ref = K.reference_and_yardstick(case)[0]
        for bd in (1, 0):
            z = t["logits"].double().requires_grad_(True)
            want = trainer.deep_supervision_loss_eager([z], [t["target"].double()], batch_dice=bool(bd), ignore_label=case.ignore)
            g, = torch.autograd.grad(want, z)
            assert abs(float(want.detach()) - float(ref[f"loss_bd{bd}"])) <= 1e-12 * max(1.0, abs(float(want.detach()))), (case, bd)
            assert float((g - ref[f"dloss_bd{bd}"]).abs().max()) <= 1e-10 * float(g.abs().max()), (case, bd)


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: simulated defects on the float64 reference, 10 x outside the bound of the case meant to catch them
# ---------------------------------------------------------------------------------------------------------------------
MARGIN = 10.0


def _outside(case, defect, quantities):
    """Every quantity of `quantities` of the defective evaluation is at least MARGIN x its bound away from the reference."""
    ref, yard = K.reference_and_yardstick(case)
    tols = K.bounds(case, ref, yard)
    for q in quantities:
        assert K.error(ref[q], ref[q], tols[q]) == 0.0
        err = K.error(defect[q], ref[q], tols[q])
        print(f"DEFECT {K.family(case)} {K.case_id(case)} {q}: {err:.2e} = {err / tols[q].a:.0f} x the bound {tols[q].a:.2e}")
        assert err >= MARGIN * tols[q].a, (q, err, tols[q])


def _keep_pixels(case, drop):
    """(B, HW) bool: False where drop(b, workgroup of the pixel) says so."""
    HW = K.hw_of(case)
    blk = torch.arange(HW) // K.LOSS_PIX
    return torch.stack([~drop(b, blk) for b in range(case.B)])


def test_k9_a_dropped_ragged_workgroup_is_far_outside_the_bounds():
    """The one pixel of 1025 that the second workgroup owns, and the last 387 pixels of the long sum."""
    for case in (K.K9Case(3, 3, K.RAGGED, None, "unit", "", True), K.K9Case(1, 16, K.RAGGED, 16, "unit", "", False),
                 K.K9Case(1, 2, K.K9_LONG, None, "unit", "", False)):
        assert case in K.K9_CASES
        last = K.loss_workgroups(K.hw_of(case)) - 1
        defect = K.k9_evaluate(case, torch.float64, keep=_keep_pixels(case, lambda b, blk: blk == last))
        _outside(case, defect, ("ip", "ce"))


def test_k9_a_dropped_odd_partial_row_is_far_outside_the_bounds():
    for case in (K.K9Case(3, 3, K.K9_PIXELS[2049], None, "unit", "", False), K.K9Case(3, 3, K.K9_MANY, None, "unit", "", False)):
        assert case in K.K9_CASES
        nblk = K.loss_workgroups(K.hw_of(case))
        assert K.reduce_rows(nblk) == "odd"
        defect = K.k9_evaluate(case, torch.float64, keep=_keep_pixels(case, lambda b, blk: blk == nblk - 1))
        _outside(case, defect, ("ip", "ce"))


def test_k9_ce_partials_beyond_the_first_256_dropped_are_far_outside_the_bounds():
    case = K.K9Case(3, 3, K.K9_MANY, None, "unit", "", False)
    assert case in K.K9_CASES
    nblk = K.loss_workgroups(K.hw_of(case))
    defect = K.k9_evaluate(case, torch.float64, keep=_keep_pixels(case, lambda b, blk: b * nblk + blk >= K.REDUCE_TPB))
    _outside(case, defect, ("ce",))


def test_k9_one_samples_g_ip_for_every_sample_is_far_outside_the_bounds():
    for case in (c for c in K.K9_CASES if c.B > 1 and K.hw_of(c) > 1):
        _outside(case, K.k9_evaluate(case, torch.float64, g_ip_of_sample_0=True), ("dlogits",))


def test_k29_dropped_heads_are_far_outside_the_bounds():
    for case in K.K29_CASES:
        for heads in (4, 8):
            if case.R > heads:
                _outside(case, K.k29_evaluate(case, torch.float64, heads=heads), ("ip", "bce", "dlogits"))


def test_k29_dropped_rows_and_partials_are_far_outside_the_bounds():
    """K29's reducer is K9's: the ragged last workgroup, and the scalar partials beyond the first 256, through the mask."""
    for form in K.K29_FORMS:
        case = K.K29Case(2, 5, (4099, 1), True, form, "unit")
        many = K.K29Case(3, 5, K.K9_MANY, True, form, "unit")
        assert case in K.K29_CASES and many in K.K29_CASES
        for c, drop in ((case, lambda b, blk: blk == 4), (many, lambda b, blk: b * 101 + blk >= K.REDUCE_TPB)):
            ref = K.reference_and_yardstick(c)[0]
            inp = K.inputs(c)
            t, m = K.k29_targets(c, inp["seg"])
            keep = _keep_pixels(c, drop)
            ip, gt, bce, mask = K.k29_stats(inp["logits"].double().flatten(2), t.double(), (m & keep).double())
            _outside(c, dict(bce=bce) if c is many else dict(ip=ip, bce=bce), ("bce",) if c is many else ("ip", "bce"))
            assert float(mask) < float(ref["mask"]) and not torch.equal(gt, ref["gt"])         # the exact quantities notice too


K11_CATCHER = K.K11Case(2, "unit", 0.05, False)        # lead 2: 65535 and 65539 aligned (vector path with tails), 65537 and 131073 not


def _k11_defect(case, change):
    """The reference's final p / exp_avg / exp_avg_sq with the elements [lo, hi) of tensor i left as they were before the steps."""
    ref = K.reference_and_yardstick(case)[0]
    t = K.inputs(case)
    out = {q: [a.clone() for a in ref[q]] for q in ("p", "exp_avg", "exp_avg_sq")}
    for i, n in enumerate(K.k11_sizes(case)):
        lo, hi = change(n)
        if hi > lo:
            out["p"][i][lo:hi] = t["params"][i][lo:hi].double()
            out["exp_avg"][i][lo:hi] = 0.0
            out["exp_avg_sq"][i][lo:hi] = 0.0
    return out


def test_k11_a_chunk_tail_not_updated_is_far_outside_the_bounds():
    assert K11_CATCHER in K.K11_CASES

    def tail_of_the_last_chunk(n):
        n4, tail = K.k11_last_chunk(n)
        return (n - tail, n) if n in (65535, 65539) else (0, 0)                      # the aligned tensors of this case with a tail
    _outside(K11_CATCHER, _k11_defect(K11_CATCHER, tail_of_the_last_chunk), ("p", "exp_avg", "exp_avg_sq"))


def test_k11_a_last_chunk_not_updated_is_far_outside_the_bounds():
    def last_chunk(n):
        return ((K.k11_chunks(n) - 1) * K.K11_CHUNK, n) if n == 131073 else (0, 0)   # one element
    _outside(K11_CATCHER, _k11_defect(K11_CATCHER, last_chunk), ("p", "exp_avg", "exp_avg_sq"))


def test_k11_a_misaligned_tensor_missing_from_the_norm_is_far_outside_the_bounds():
    for case in (K11_CATCHER, K.K11Case(2, "near_above", 12.0, False), K.K11Case(0, "dominated", 12.0, False)):
        assert case in K.K11_CASES
        sizes = K.k11_sizes(case)
        offs = K.k11_grad_offsets(sizes)
        # the largest-norm misaligned tensor: 65537 (the dominating one where one dominates)
        miss = sizes.index(65537)
        assert K.k11_sumsq_path(4 * offs[miss]) == "scalar"
        norms = [torch.sqrt(sum((a.double() ** 2).sum() for i, a in enumerate(gs) if i != miss)).reshape(1) for gs in K.inputs(case)["grads"]]
        _outside(case, dict(norm=norms), ("norm",))
