"""The cases of tests/_conv_kernel_cases.py are what they claim to be, checked without a GPU.

The path predicates agree with the library's host queries -- the launchers' own tile and form decisions (mlagg_conv3x3_fwd_tile,
mlagg_conv3x3_wgrad_form, mlagg_conv1x1_fwd_tile, mlagg_conv1x1_wgrad_tile), the workspace sizes, the supported shapes -- over the
cases and a sweep; the case tables reach every tile, form, slab geometry and both sides of every threshold (taking a boundary case
out of a table fails here); every reference value is finite and the plain-fp32 yardstick stays within HALF of the bounds the device
test uses, i.e. the inputs are well conditioned and a failure on the device means the kernel."""
import os

import pytest
import torch

from tests import _conv_kernel_cases as M


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    from mlagg_unet_amd import _lib
    return _lib.lib()


def _find(cid):
    return M.by_id(cid)


def _hw(case):
    return case.dims[-2], case.dims[-1]


# ---------------------------------------------------------------------------------------------------------------------
# the tables describe the default dispatch
# ---------------------------------------------------------------------------------------------------------------------
def test_no_dispatch_override_is_set():
    on = [v for v in M.OVERRIDES if v in os.environ]
    assert not on, f"{on} set: the case tables of tests/_conv_kernel_cases.py describe the launchers' DEFAULT choices; unset to run them"


# ---------------------------------------------------------------------------------------------------------------------
# predicates against the library
# ---------------------------------------------------------------------------------------------------------------------
def test_k19_forward_tile_matches_the_launcher(lib):
    def same(O, D, H, W):
        to, tp = M.k19_fwd_tile(O, D * H * W, W)
        assert lib.mlagg_conv3x3_fwd_tile(O, D, H, W) == to * 4 + tp, (O, D, H, W)
    for c in M.K19_FWD_CASES + M.K19_WGRAD_CASES:
        D = c.dims[0] if len(c.dims) == 3 else 1
        H, W = _hw(c)
        same(c.O, D, H, W)
        same(c.I, D, H, W)                                                        # the data gradient
    maps = [(127, 129), (128, 128), (126, 130), (129, 127), (64, 256), (255, 257), (256, 256), (258, 254), (257, 255), (254, 258),
            (8, 12), (1, 96), (97, 1), (1024, 64), (1, 65536), (65535, 1)]
    assert {H * W >= 16384 for H, W in maps} == {H * W >= 65536 for H, W in maps} == {True, False}
    for O in range(1, 201):
        for H, W in maps:
            same(O, 1, H, W)
        for D, H, W in [(16, 32, 32), (16, 31, 33), (4, 64, 64), (64, 32, 32), (3, 5, 7), (63, 32, 33)]:
            same(O, D, H, W)


def test_k19_weight_gradient_form_and_slabs_match_the_launcher(lib):
    for O in range(1, 201):
        for I in (1, 15, 16, 17, 48, 96, 200):
            for form in M.FORMS:
                kf, ti = M.k19_wgrad_form(O, I, 1, form)
                assert lib.mlagg_conv3x3_wgrad_form(O, I, 1, form) == kf * 4 + ti, (O, I, form)
                assert lib.mlagg_conv3x3_wgrad_form(O, I, 4, form) == 0 == sum(M.k19_wgrad_form(O, I, 4, form))
    assert lib.mlagg_conv3x3_wgrad_form(48, 48, 1, 0) < 0                         # fp32 storage is no operand form
    shapes = [(c.B, c.O, c.I) + _hw(c) for c in M.K19_WGRAD_CASES + M.K19_FWD_CASES if len(c.dims) == 2]
    shapes += [(10, 48, 48, 256, 256), (10, 96, 96, 128, 128), (10, 768, 384, 16, 16), (2, 48, 48, 224, 56), (1, 16, 16, 512, 640), (1, 1, 1, 8, 8)]
    for B, O, I, H, W in shapes:
        if not lib.mlagg_conv3x3_wgrad_supported(O, I, H, W):
            continue
        g = M.k19_wgrad_geometry(B, O, I, H, W)
        assert lib.mlagg_conv3x3_wgrad_workspace_floats(B, O, I, H, W) == g.nbs * 9 * O * I, (B, O, I, H, W)
        assert g.nbs == B * g.nslabs and (g.nslabs - 1) * g.slab + g.last_pixels == H * W and 0 < g.last_pixels <= g.slab
        assert g.slab % 32 == 0 and g.q32 * W + g.r32 == 32


def test_k18_tiles_and_slabs_match_the_launcher(lib):
    for O in range(1, 201):
        to, tp = M.k18_fwd_tile(O)
        assert lib.mlagg_conv1x1_fwd_tile(O) == to * 4 + tp, O
        for I in (1, 16, 31, 32, 33, 63, 64, 65, 96, 97, 200):
            to, ti = M.k18_wgrad_tile(O, I)
            assert lib.mlagg_conv1x1_wgrad_tile(O, I) == to * 4 + ti, (O, I)
    shapes = [(c.B, c.O, c.I, M.pixels(c.dims)) for c in M.K18_CASES] + [(10, 192, 96, 16384), (10, 48, 96, 65536), (1, 768, 384, 256), (3, 14, 48, 65536)]
    for B, O, I, P in shapes:
        g = M.k18_wgrad_geometry(B, O, I, P)
        assert lib.mlagg_conv1x1_wgrad_workspace_floats(B, O, I, P) == B * g.nslabs * O * I, (B, O, I, P)
        assert (g.nslabs - 1) * g.slab + g.last_pixels == P and 0 < g.last_pixels <= g.slab and g.slab % 16 == 0


def test_the_plan_of_every_case_matches_the_supported_queries(lib):
    for c in M.ALL_CASES:
        on, P = M.on_kernel(c), M.pixels(c.dims)
        if c.family == "k18":
            for q, (o, i) in (("y", (c.O, c.I)), ("dx", (c.I, c.O))):
                assert on[q] == bool(lib.mlagg_conv1x1_supported(o, -(-i // 16) * 16, P)), (c.id, q)
            assert on["dW"] and lib.mlagg_conv1x1_wgrad_workspace_floats(c.B, c.O, c.I, P) > 0, c.id
        elif len(c.dims) == 3:
            assert on["y"] == bool(lib.mlagg_conv3x3x3_supported(c.O, c.I, *c.dims)) and on["dx"] == bool(lib.mlagg_conv3x3x3_supported(c.I, c.O, *c.dims))
            assert on["dW"] == bool(lib.mlagg_conv3x3x3_wgrad_supported(c.O, c.I, *c.dims))
        else:
            H, W = c.dims
            assert on["y"] == bool(lib.mlagg_conv3x3_supported(c.O, c.I, H, W)), c.id
            assert on["dx"] == bool(lib.mlagg_conv3x3_supported(c.I, c.O, H, W)), c.id
            assert on["dW"] == bool(lib.mlagg_conv3x3_wgrad_supported(c.O, c.I, H, W)), c.id
        # the product a case is about runs on the kernel
        assert on["y"] if c.family == "k19_fwd" else (on["dW"] if c.family == "k19_wgrad" else all(on.values())), c.id


# ---------------------------------------------------------------------------------------------------------------------
# coverage: what the tables must reach (each line names the boundary case that provides it)
# ---------------------------------------------------------------------------------------------------------------------
def _fwd(cid):
    c = _find(cid)
    return M.k19_fwd_tile(c.O, M.pixels(c.dims), c.dims[-1])


def _dgrad(cid):
    c = _find(cid)
    return M.k19_fwd_tile(c.I, M.pixels(c.dims), c.dims[-1])


def test_k19_forward_cases_cover_every_tile_and_both_sides_of_each_threshold():
    ids = {c.id for c in M.K19_FWD_CASES}
    assert len(ids) == len(M.K19_FWD_CASES)
    P = {cid: M.pixels(_find(cid).dims) for cid in ids}
    # the 16384-pixel threshold of the 96-row tile: on it, below it with an even and with an odd width
    assert P["F1"] == 16384 and _fwd("F1") == (3, 1) and _dgrad("F1") == (1, 2)
    assert P["F2"] == 16380 and _fwd("F2") == (2, 2)
    assert P["F3"] == 16383 and _fwd("F3") == (2, 1) and _dgrad("F3") == (1, 1)
    # (3,1) with two 96-row groups, B = 2, a partial last workgroup and a partial last wave
    c = _find("F4")
    wgs, groups, last_wg, last_wave, live = M.k19_fwd_grid(c.O, P["F4"], _fwd("F4"))
    assert _fwd("F4") == (3, 1) and c.B == 2 and groups == 2 and live == 96 and 0 < last_wg < 128 and last_wave == P["F4"] % 32 == 26
    # the 65536-pixel threshold of the two-pixel runs: on it, just below, above with ragged ends, above with an odd width
    assert P["F5"] == 65536 and _fwd("F5") == (3, 2) and _find("F5").backward
    assert P["F6"] == 65532 and _fwd("F6") == (3, 1)
    wgs, groups, last_wg, last_wave, live = M.k19_fwd_grid(96, P["F7"], _fwd("F7"))
    assert P["F7"] == 66548 and _fwd("F7") == (3, 2) and 0 < last_wg < 256 and 0 < last_wave < 64
    assert P["F8"] == 66049 and _find("F8").dims[1] % 2 == 1 and _fwd("F8") == (3, 1)
    # the 96-row tile in the one-product forms, on a channel-slice input
    for cid, form in (("F9-bf16", 1), ("F9-fp16", 2)):
        assert _find(cid).form == form and _find(cid).sliced == "x" and _fwd(cid) == (3, 1)
    # the O = 32 / 33 step, a second row group with one live row
    assert (_find("F10-32").O, _find("F10-33").O) == (32, 33) and _fwd("F10-32") == (1, 2) and _fwd("F10-33") == (2, 2)
    assert _fwd("F11") == (2, 2) and M.k19_fwd_grid(97, P["F11"], (2, 2))[1:] == (2, 144, 16, 33) and 33 % 32 == 1      # ... in its second 32-row tile
    # image edges: one-pixel rows, a run that is the whole row, one image row, the floor of 96 pixels
    assert _find("F12").dims == (97, 1) and _fwd("F12") == (2, 1)
    assert _find("F13").dims == (49, 2) and _fwd("F13") == (2, 2)
    assert _find("F14").dims == (1, 96) and P["F15"] == 96 == P["F14"]
    # nine kernel rows with the 96-row tile
    assert len(_find("F16").dims) == 3 and _fwd("F16") == (3, 1) and _dgrad("F16") == (1, 2)
    # all six tiles, counting the data gradients that run
    tiles = {_fwd(cid) for cid in ids} | {_dgrad(cid) for cid in ids if _find(cid).backward and M.on_kernel(_find(cid))["dx"]}
    assert tiles == {(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2)}


def test_k19_weight_gradient_cases_cover_the_slab_geometry():
    geo = {}
    for n, B, I, O, d, s in M.K19_WGRAD_SHAPES:
        geo[n] = M.k19_wgrad_geometry(B, O, I, *d)
        forms = {c.form: c for c in M.K19_WGRAD_CASES if c.id.startswith(n + "-f")}
        assert set(forms) == {3, 1, 2}, n                                          # both kernels and every operand form
        assert {M.k19_wgrad_form(O, I, 1, f)[0] for f in forms} == {1, 2}
    W = {n: d[1] for n, B, I, O, d, s in M.K19_WGRAD_SHAPES}
    g = geo["W1"]
    assert (g.slab, g.nslabs, g.nbs, g.r32, g.q32, g.ti) == (256, 7, 14, 32, 0, 3) and g.slab % W["W1"] == 32 and M.k19_wgrad_wraps(W["W1"], g.slab)
    g = geo["W2"]
    assert (g.last_pixels, g.last_blocks, g.last_pixels % 32) == (144, 5, 16) and W["W2"] == 40
    g = geo["W3"]
    assert (g.ti, g.q32, g.r32, g.nbs) == (1, 1, 8, 6)
    g = geo["W4"]
    assert (W["W4"], g.q32, g.r32, g.og, g.last_blocks) == (8, 4, 0, 2, 3) and 49 - 48 == 1
    g = geo["W5"]
    assert (g.og, g.ig, g.nslabs, g.last_pixels, g.last_blocks) == (1, 1, 2, 16, 1)
    g = geo["W6"]
    assert (g.slab, g.nslabs, g.nbs, g.nbs % 8, g.slab % W["W6"], g.og, g.ig, g.last_blocks) == (288, 43, 86, 6, 24, 4, 2, 7)
    g = geo["W7"]
    assert (g.nslabs, g.last_blocks, g.last_pixels % 32) == (1, 5, 16)
    g = geo["W8"]
    assert (g.ti, g.nbs) == (1, 10)
    g = geo["W9"]
    assert (g.ig, 64 - 48, g.nslabs) == (2, 16, 1) and M.zero_rows(_find("W9-f3")) == (0, 2)
    g = geo["W10"]
    assert W["W10"] > 128 and g.last_blocks == 1 and g.nslabs == 2
    assert geo["W11-x"] == geo["W11-dy"] == geo["W1"]
    assert {c.sliced for c in M.K19_WGRAD_CASES if c.id.startswith("W11")} == {"x", "dy"}
    g = geo["W12"]
    assert g.nbs % 8 == 0 and g.nbs > 8 and g.r32 == 0
    # the properties, each on both sides
    all_g = list(geo.items())
    assert {W[n] % 16 for n, _ in all_g} == {0, 8}
    assert {56, 40} <= set(W.values())                                             # the widths of the 224 x 224 / 512 x 640 configurations
    assert {g.ti for _, g in all_g} == {1, 3}
    assert {g.slab == M.K19W_MIN_SLAB for _, g in all_g} == {True, False}
    assert {g.last_blocks % 2 for _, g in all_g} == {0, 1} and {g.last_pixels % 32 for _, g in all_g} == {0, 16}
    assert {g.nbs % 8 == 0 for _, g in all_g} == {True, False}
    assert {M.k19_wgrad_wraps(W[n], g.slab) for n, g in all_g} == {True, False}
    assert any(g.nslabs > 1 and g.slab % W[n] for n, g in all_g)                     # a slab that ends in mid-row


def test_k18_cases_cover_every_tile_and_the_slab_geometry():
    shape = {n: (B, I, O, M.pixels(d)) for n, B, I, O, d, s in M.K18_SHAPES}
    for n in shape:
        assert {c.form for c in M.K18_CASES if c.id.startswith(n + "-f")} == {3, 1, 2}, n

    def wg(n):
        return M.k18_wgrad_tile(shape[n][2], shape[n][1])

    def geom(n):
        B, I, O, P = shape[n]
        return M.k18_wgrad_geometry(B, O, I, P)

    assert wg("C1") == (1, 1) and geom("C1") == (64, 3, 48) and M.k18_fwd_tile(shape["C1"][2]) == (1, 3) and shape["C1"][3] % 96 == 80
    assert wg("C2") == (1, 2) and M.k18_fwd_tile(shape["C2"][1]) == (2, 3)
    assert wg("C3") == (2, 3) and shape["C3"][2] % 16 == 8
    assert wg("C4") == (3, 1) and M.k18_fwd_tile(shape["C4"][2]) == (3, 2)
    assert (shape["C5-64"][2], shape["C5-65"][2]) == (64, 65) and wg("C5-64") == (2, 2) and wg("C5-65") == (3, 2)
    assert M.k18_fwd_tile(64) == (2, 3) and M.k18_fwd_tile(65) == (3, 2)
    assert wg("C6") == (3, 3) and geom("C6") == (96, 86, 32)
    assert shape["C7"][3] == 96
    assert shape["C8"] == shape["C3"] and {c.sliced for c in M.K18_CASES if c.id.startswith("C8")} == {"x"}
    assert wg("C9") == (1, 3) and wg("C10") == (2, 1)
    assert {wg(n) for n in shape} == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)}
    fwd = {M.k18_fwd_tile(s[2]) for s in shape.values()} | {M.k18_fwd_tile(s[1]) for s in shape.values()}
    assert fwd == {(1, 3), (2, 3), (3, 2)}
    assert (shape["C11-32"][2], shape["C11-33"][2]) == (32, 33) and wg("C11-32") == (1, 2) and wg("C11-33") == (2, 2)
    assert M.k18_fwd_tile(32) == (1, 3) and M.k18_fwd_tile(33) == (2, 3)
    assert {geom(n).slab == M.K18_MIN_SLAB for n in shape} == {True, False}
    assert any(geom(n).nslabs > 1 and geom(n).last_pixels < geom(n).slab for n in shape)
    assert {(geom(n).slab // 16) % 2 for n in shape} == {0} and {(geom(n).last_pixels // 16) % 2 for n in shape} == {0, 1}       # blocks per slab: pairs, and a peeled last one


def test_case_ids_are_unique_and_the_sentinel_cases_exist():
    ids = [c.id for c in M.ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert [M.by_id(cid).family for cid in M.SENTINEL_CASES] == ["k19_fwd", "k19_fwd", "k18"]
    assert all(c.form in M.FORM_TYPE and c.sliced in ("none", "x", "dy") for c in M.ALL_CASES)


# ---------------------------------------------------------------------------------------------------------------------
# references and yardstick
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.ALL_CASES, ids=[c.id for c in M.ALL_CASES])
def test_reference_is_finite_and_the_plain_fp32_yardstick_is_within_half_the_bounds(case):
    ref, yard = M.reference(case), M.yardstick(case)
    tols = M.bounds(case)
    assert set(ref) == set(yard) == ({"y", "dx", "dW"} if case.backward else {"y"})
    assert set(M.compared(case)) <= set(ref) and M.compared(case)
    for q in ref:
        assert ref[q].dtype == torch.float64 and yard[q].dtype == torch.float32
        assert bool(torch.isfinite(ref[q]).all()) and bool(torch.isfinite(yard[q]).all()), q
        err = M.error(yard[q], ref[q])
        used = q in M.compared(case)                   # a product left to the library is not held to the kernel's bound
        print(f"YARDSTICK {case.id} {q} {err:.2e} bound {tols[q]:.1e}{'' if used else ' (not compared on the device)'}")
        assert not used or err <= 0.5 * tols[q], (q, err, tols[q])
    for ky in M.zero_rows(case):                       # a one-row image: the kernel rows above and below see padding only
        if "dW" in ref:
            assert float(ref["dW"][:, :, ky].abs().max()) == 0.0 and float(ref["dW"][:, :, 1].abs().max()) > 0.0
