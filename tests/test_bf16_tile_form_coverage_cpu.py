"""The bf16 host planners restated in tests/bf16_tile_cases.py equal the library's, the case tables of
tests/test_gpu_bf16_tile_forms_fp64.py reach every kernel instantiation and tile the planners can return and every decode / tail
edge of the large-tile kernels, and the exact pass of that module is exact -- on the CPU: the queries read no device memory.

A planner change that moves a case to another tile (and so silently un-covers a form) fails here, naming the form.
"""
import itertools

import pytest
import torch

import bf16_tile_cases as B
import bf16_tile_ops as O
import fp64_ref as R
from gelslim_depth_amd import _lib as L

lib = L.lib
NS = (1, 2, 3, 8)
KNOBS = ("GSD_BF16_TW", "GSD_BF16_XCD", "GSD_BF16_CONV_BUF", "GSD_BF16_CTGEMM", "GSD_BF16_CT_BM", "GSD_BF16_WGRAD_BLOCKS",
         "GSD_BF16_WGRAD_BIG")
BIG = ((3, 150, 150), (8, 64, 128), (2, 130, 130), (16, 320, 427), (32, 160, 213), (7, 80, 106), (1, 4096, 4095))   # items past the grid


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _grid(env=None):
    """N in {1, 2, 3, 8}, H <= 48, W <= 80 (with a knob set, every fourth shape of it), plus large pixel counts."""
    full = itertools.product(NS, range(1, 49), range(1, 81))
    return itertools.chain(full if not env else (s for s in full if (s[1] * 5 + s[2]) % 4 == 0), BIG)


def _ids(e):
    return "-".join(f"{k[4:]}={v}" for k, v in e.items()) or "default"


@pytest.mark.parametrize("env", [{}, {"GSD_BF16_TW": "16"}, {"GSD_BF16_TW": "32"}, {"GSD_BF16_TW": "64"}], ids=_ids)
def test_conv_partial_rows_restatement_equals_the_library(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bad = [(n, h, w, m) for n, h, w in _grid(env) for m in (48, 64, 128, 256, 384)
           if B.conv_partial_rows(n, h, w, m, env) != lib.gsd_bf16_conv_partial_rows(n, h, w, m)]
    assert not bad, bad[:8]


@pytest.mark.parametrize("env", [{}, {"GSD_BF16_CTGEMM": "0"}, {"GSD_BF16_CT_BM": "128"}, {"GSD_BF16_CT_BM": "256"},
                                 {"GSD_BF16_TW": "16", "GSD_BF16_CT_BM": "256"}], ids=_ids)
def test_dense_partial_rows_restatement_equals_the_library(monkeypatch, env):
    """The 1-tap and the 4-tap stride-2 forms at (K, M) pairs on and off the large-tile conditions (K % 64 zero and not, M in
    {64, 128, 256, 384, 512}), W on both sides of 16 (the grid)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bad = []
    for n, h, w in _grid(env):
        for k in (32, 64, 96, 128):
            for m in (64, 128, 256, 384, 512):
                for taps, stride in ((1, 1), (4, 2)):
                    got = B.conv_dense_partial_rows(n, h, w, k, m, taps, stride, env)
                    if got != lib.gsd_bf16_conv_dense_partial_rows(n, h, w, k, m, taps, stride):
                        bad.append((n, h, w, k, m, taps, got))
    assert not bad, bad[:8]


@pytest.mark.parametrize("env", [{}, {"GSD_BF16_WGRAD_BLOCKS": "3"}, {"GSD_BF16_WGRAD_BLOCKS": "64"}, {"GSD_BF16_WGRAD_BIG": "0"},
                                 {"GSD_BF16_WGRAD_BIG": "0", "GSD_BF16_WGRAD_BLOCKS": "5"}], ids=_ids)
def test_wgrad_workspace_restatement_equals_the_library(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bad = []
    for n, h, w in _grid(env):
        for taps in (1, 4, 9):
            for m, nc in ((64, 32), (48, 64), (128, 64), (80, 48), (256, 128), (384, 64), (512, 256)):
                got = B.wgrad_workspace(taps, n, h, w, m, nc, env)
                if got != lib.gsd_bf16_wgrad_workspace(taps, n, h, w, m, nc):
                    bad.append((taps, n, h, w, m, nc, got))
    assert not bad, bad[:8]


# ------------------------------------------------------------------------------------------------- what the tables reach
ALL = B.CONV3_CASES + B.DENSE_CASES + B.CT_CASES + B.WG_CASES + B.WGBIG_CASES


def test_every_case_reaches_the_form_its_row_names():
    wrong = [(c, B.form_of(c)) for c in ALL if B.form_of(c) != c.form]
    assert not wrong, "; ".join(f"{c} runs {f}, its row names {c.form}" for c, f in wrong[:4])


def _missing(want, cases):
    return sorted(map(str, set(want) - {B.form_of(c) for c in cases}))


def test_cases_reach_every_conv3x3_form():
    want = {("conv3x3", wide, tw, buf, ep) for wide in (False, True) for tw in (16, 32, 64) for buf in (0, 1) for ep in ("stats",)}
    want |= {("conv3x3", wide, tw, buf, "bnbwd") for wide, tw in ((False, 32), (True, 64)) for buf in (0, 1)}
    want |= {("conv3x3", False, 32, 1, "bnrelu"), ("conv3x3", True, 32, 1, "bnrelu")}
    assert not _missing(want, B.CONV3_CASES), f"conv3x3 forms not reached: {_missing(want, B.CONV3_CASES)}"


def test_cases_reach_every_dense_form():
    want = {("dense", wide, tw, 1, 1, "plain") for wide, tw in ((True, 64), (False, 32), (False, 16), (True, 16), (False, 64))}
    want |= {("dense", True, 32, 1, 1, "bnrelu"), ("dense", False, 64, 1, 1, "bnrelu")}
    want |= {("dense", True, 32, 1, 1, "scatter"), ("dense", False, 16, 1, 1, "scatter")}
    want |= {("dense", wide, tw, 4, 2, ep) for wide, tw in ((True, 32), (False, 16)) for ep in ("plain", "bnbwd")}
    want |= {("dense", False, 32, 4, 2, "plain"), ("dense", False, 32, 4, 2, "bnbwd"), ("refused",)}
    assert not _missing(want, B.DENSE_CASES), f"dense forms not reached: {_missing(want, B.DENSE_CASES)}"
    # host fallbacks at a shape the large-tile kernel takes: a cropped gradient buffer, an output buffer larger than the grid
    big = [c for c in B.DENSE_CASES if c.kind == "ctdx" and B.ctgemm_shape(c.n, c.h, c.w, c.k, c.m, 4, 2, 0, B.env_of(c))]
    assert any(c.crop and not c.fused and B.form_of(c)[0] == "dense" for c in big), "cropped, plain: the general kernel"
    assert any(c.crop and c.fused and B.form_of(c) == ("refused",) and c.want == -2 for c in big), "cropped, fused: refused"
    assert any(c.opad and B.form_of(c)[0] == "dense" for c in big), "output buffer larger than the grid: the general kernel"
    # every tile width and both blocks over the table, every scatter offset at both Cs
    assert {(f[1], f[2]) for f in map(B.form_of, B.DENSE_CASES) if f[0] == "dense"} >= {(wd, tw) for wd in (False, True) for tw in (16, 32, 64)}
    assert {(c.cs, c.oy, c.ox) for c in B.DENSE_CASES if c.kind == "ctfwd"} == {(cs, oy, ox) for cs in (16, 32) for oy in (0, 1) for ox in (0, 1)}


def test_cases_reach_every_large_tile_convT_kernel():
    want = {("ct", 0, 256, False)} | {("ct", 1, bm, f) for bm in (128, 256) for f in (False, True)}
    assert not _missing(want, B.CT_CASES), f"large-tile ConvT forms not reached: {_missing(want, B.CT_CASES)}"
    fwd = [c for c in B.CT_CASES if not c.dx]
    assert {c.m for c in fwd} == {256, 512} and {c.k for c in fwd} == {64, 128}
    dx = [(c.m, B.form_of(c)[2], dict(c.env).get("GSD_BF16_CT_BM")) for c in B.CT_CASES if c.dx]
    assert {(256, 256, "256"), (128, 128, None), (384, 128, None), (256, 128, "128"), (256, 128, None)} <= set(dx), sorted(set(dx), key=str)
    assert {c.k for c in B.CT_CASES if c.dx} == {64, 128}


def test_cases_reach_every_wgrad_form():
    want = {("wgrad", halo, t, wide, tw) for halo, t in ((1, 9), (0, 4), (0, 1)) for wide in (False, True) for tw in (32, 64)}
    assert not _missing(want, B.WG_CASES), f"dW forms not reached: {_missing(want, B.WG_CASES)}"
    want = {("wgrad_big", 128), ("wgrad_big", 256), ("wgrad", 0, 4, False, 32)}
    assert not _missing(want, B.WGBIG_CASES), f"large-tile dW forms not reached: {_missing(want, B.WGBIG_CASES)}"


# --------------------------------------------------------------------------------------------------- what edges they reach
def _need(cases, pred, what):
    hit = [c for c in cases if pred(c)]
    assert hit, f"no case with {what}"
    return hit


def _images_in_a_tile(c, npx=256):
    hw = c.h * c.w
    p = c.n * hw
    return max((min(p, t + npx) - 1) // hw - t // hw + 1 for t in range(0, p, npx))


@pytest.mark.parametrize("dx", (0, 1), ids=("forward", "dX"))
def test_large_tile_convT_cases_reach_every_decode_and_tail_edge(dx):
    cases = [c for c in B.CT_CASES if c.dx == dx and B.form_of(c)[0] == "ct"]
    px = lambda c: c.n * c.h * c.w                                                                  # noqa: E731
    plan = lambda c: B.ct_plan(px(c), c.m, bool(c.dx), B.env_of(c))                                 # noqa: E731
    _need(cases, lambda c: px(c) < 256, "P < 256")
    _need(cases, lambda c: px(c) == 256, "P == 256")
    _need(cases, lambda c: px(c) % 256 != 0 and plan(c).ntile >= 3, "P % 256 != 0 over at least three tiles")
    _need(cases, lambda c: _images_in_a_tile(c) >= 3, "a tile holding pixels of three images")
    _need(cases, lambda c: c.h == 1, "H == 1")
    _need(cases, lambda c: c.w == 16, "W == 16")
    _need(cases, lambda c: c.w == 17, "W == 17")
    _need(cases, lambda c: plan(c).mblocks == 2, "two m-blocks")
    for on in (True, False):     # a persistent block then walks at least two tiles
        _need(cases, lambda c: plan(c).ntile * plan(c).mblocks > plan(c).grid and B.xcd_on(plan(c).grid, plan(c).mblocks, B.env_of(c)) == on,
              f"more items than blocks with the XCD order {'on' if on else 'off'}")
    assert {(c.oy, c.ox) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c.spare > 0 for c in cases} == {True, False}, "a buffer of exactly the block's extent, and one with spare"
    assert all(c.n >= 2 for c in cases)


def test_large_tile_wgrad_cases_reach_every_stage_edge():
    cases = [c for c in B.WGBIG_CASES if B.form_of(c)[0] == "wgrad_big"]
    px = lambda c: c.n * c.h * c.w                                                                  # noqa: E731
    plan = lambda c: B.make_bigplan(4, c.n, c.h, c.w, c.m, c.ncols, B.env_of(c))                    # noqa: E731
    _need(cases, lambda c: px(c) < 64, "P < 64")
    _need(cases, lambda c: px(c) % 64 != 0 and px(c) > 64, "P % 64 != 0")
    _need(cases, lambda c: plan(c).stages_total > plan(c).splits and plan(c).stages_total % plan(c).splits != 0,
          "stages_total > splits with a remainder")
    assert {B.form_of(c)[1] for c in cases} == {128, 256}
    assert {c.m for c in cases} >= {128, 256, 384, 512} and {c.ncols for c in cases} >= {64, 128}
    assert {(c.oy, c.ox) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    _need(B.WGBIG_CASES, lambda c: c.crop and B.form_of(c)[0] == "wgrad", "a cropped b that falls back to the general kernel")


def test_general_conv_cases_reach_every_tile_edge():
    for cases, name in ((B.CONV3_CASES, "conv3x3"), ([c for c in B.DENSE_CASES if B.form_of(c)[0] == "dense"], "dense")):
        plans = [(c, B.make_plan(c.h, c.w, c.m, B.env_of(c))) for c in cases]
        for tw in (16, 32, 64):
            mine = [(c, p) for c, p in plans if p.TW == tw]
            assert any(p.tiles_y >= 2 for _, p in mine) or tw == 64, f"{name} TW {tw}: no case with two tile rows"
            assert any(c.h % p.TH or c.w % p.TW for c, p in mine), f"{name} TW {tw}: no partly filled last tile"
        assert any(p.TW == 64 and p.tiles_x >= 2 for _, p in plans), f"{name}: no case with two tile columns"
        assert any(p.tiles_x >= 2 and p.tiles_y >= 2 for _, p in plans) or name == "dense", f"{name}: no 2 x 2 tiling"
        assert {48, 80} <= {c.m for c in cases}, f"{name}: M off the block size (48, 80)"
        assert any(B.conv_items(c.n, c.h, c.w, c.m, B.env_of(c)) > B.launch_grid(10 ** 9, p.mblocks) for c, p in plans), f"{name}: items > grid"
        assert all(c.n >= 2 for c in cases)
    for wide in (False, True):      # conv3x3: every (block, TW) tiles in both directions in some case
        for tw in (16, 32, 64):
            assert any(p.wide == wide and p.TW == tw and p.tiles_x >= 2 and p.tiles_y >= 2
                       for p in (B.make_plan(c.h, c.w, c.m, B.env_of(c)) for c in B.CONV3_CASES)), f"conv3x3 wide={wide} TW {tw}: no 2 x 2 tiling"
    assert any(c.in_tot > c.k for c in B.CONV3_CASES) and any(c.out_tot > c.m for c in B.CONV3_CASES), "channel slices"
    assert any(p.mblocks == 2 for p in (B.make_plan(c.h, c.w, c.m, {}) for c in B.CONV3_CASES))


def test_general_wgrad_cases_reach_every_edge():
    cases = B.WG_CASES
    plan = lambda c: B.make_wplan(c.taps == 9, c.taps, c.n, c.h, c.w, c.m, c.ncols, B.env_of(c))    # noqa: E731
    assert any(c.m % plan(c).BM for c in cases), "ragged M"
    assert any(c.ncols % plan(c).BNC for c in cases), "ragged Ncols"
    assert any(c.m == 48 for c in cases)
    assert any(c.b_off > 0 for c in cases), "b as a channel slice at an offset"
    kernels = {(f[1], f[2], f[3]) for f in map(B.form_of, cases)}
    deep = {(B.form_of(c)[1], B.form_of(c)[2], B.form_of(c)[3]) for c in cases if plan(c).stages_total > plan(c).splits}
    assert deep == kernels, f"kernels without a case of stages_total > splits: {sorted(kernels - deep)}"
    assert any(c.taps == 1 and c.ncols == 32 and c.ncols_out == 27 for c in cases)
    assert {(c.m, c.ncols) for c in cases if c.taps == 4} >= {(64, 32), (64, 48), (128, 32), (128, 48)}


# ----------------------------------------------------------------------------------------------- the exact pass is exact
def _stat_limits(c, stored, o, fused, what):
    if fused:
        _, _, b1, _ = R.bn_bwd_sums(stored, o["y"], o["mean"], o["invstd"])
        m = R.bnrelu_mask(o["y"], o["sc"], o["sh"])
        arg = o["y"] * o["sc"].double().view(1, -1, 1, 1) + o["sh"].double().view(1, -1, 1, 1)
        assert float(arg.abs().min()) >= 0.5 and bool(m.any()) and not bool(m.all()), f"{what}: the mask argument must stay off zero"
    else:
        _, _, b1, _ = R.stored_sums(stored)
    assert float(b1.max()) < O.LIM_F32, f"{what}: first moments must be exact (sum |.| = {float(b1.max())})"


@pytest.mark.parametrize("c", B.CONV3_CASES, ids=B.conv3_id)
def test_exact_pass_of_conv3x3_cases_is_exact(c):
    o = O.conv3_ops(c, "exact")
    ref, cond = O.conv3_ref(c, o)
    assert float(cond.max()) <= O.LIM_BF16 and torch.equal(ref, ref.round()) and float(ref.abs().max()) > 8
    if c.ep != "bnrelu":
        _stat_limits(c, ref, o, c.ep == "bnbwd", B.conv3_id(c))


DENSE_AND_CT = [(B.dense_id(c), c) for c in B.DENSE_CASES] + [(B.ct_id(c), B.ct_as_dense(c)) for c in B.CT_CASES]


@pytest.mark.parametrize("cid,c", DENSE_AND_CT, ids=[i for i, _ in DENSE_AND_CT])
def test_exact_pass_of_dense_and_convT_cases_is_exact(cid, c):
    o = O.dense_ops(c, "exact", cid)
    ref, cond = O.dense_ref(c, o)
    assert float(cond.max()) <= O.LIM_BF16 and torch.equal(ref, ref.round()) and float(ref.abs().max()) > 8
    if c.kind == "1x1" or c.fused:
        _stat_limits(c, ref, o, bool(c.fused), cid)


@pytest.mark.parametrize("c", B.WG_CASES + B.WGBIG_CASES, ids=B.wg_id)
def test_exact_pass_of_wgrad_cases_is_exact(c):
    ref, cond, db = O.wg_ref(c, O.wg_ops(c, "exact"))
    assert float(cond.max()) < O.LIM_F32 and torch.equal(ref, ref.round()) and float(cond.max()) > 8
    if db is not None:
        assert float(db[1].max()) < O.LIM_F32
