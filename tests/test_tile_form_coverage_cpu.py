"""The tile planners restated in tests/tile_cases.py equal the library's, and the case tables of
tests/test_gpu_tile_forms_fp64.py reach every tile form the planners can return -- on the CPU: the queries read no device memory.

A planner change that moves a case to another tile (and so silently un-covers a form) fails here, naming the form.
"""
import itertools

import pytest

import tile_cases as T
from gelslim_depth_amd import _lib as L

lib = L.lib
NS, COUTS = (1, 2, 3, 8), (20, 64, 130)
KNOBS = ("GSD_W2D_TW", "GSD_W2D_TW8_PCT", "GSD_W43_TW", "GSD_W43_FOLD", "GSD_WG43_TW", "GSD_WG2D_KX", "GSD_WGRAD_BLOCKS",
         "GSD_WG2D_BLOCKS", "GSD_WGRAD_W2D", "GSD_WGRAD_ALGO")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _grid(env=None):
    """N in {1, 2, 3, 8}, H <= 48, W <= 80; with a knob set, every eighth shape of it (the library's folded planner searches an
    LDS pitch per candidate: the full grid under GSD_W43_FOLD=1 alone takes most of a minute)."""
    full = itertools.product(NS, range(1, 49), range(1, 81))
    return full if not env else (s for s in full if (s[1] * 5 + s[2]) % 8 == 0)


def _check_conv(fam, rows_fn, count_fn, env):
    bad = []
    for n, h, w in _grid(env):
        for co in COUTS:
            want = rows_fn(n, h, w, co)
            got = T.conv_partial_rows(fam, n, h, w, co, env)
            if got != want:
                bad.append((n, h, w, co, got, want))
        if count_fn is not None:
            for ci, co in ((5, 20), (64, 130)):
                if T.conv_mfma_count(fam, n, h, w, ci, co, env) != count_fn(n, h, w, ci, co):
                    bad.append(("mfma", n, h, w, ci, co))
    assert not bad, bad[:8]


def test_direct_restatement_equals_the_library():
    _check_conv("direct", lib.gsd_conv3x3_partial_rows, None, {})


@pytest.mark.parametrize("env", [{}, {"GSD_W43_FOLD": "0"}, {"GSD_W43_FOLD": "1"}, {"GSD_W43_TW": "56", "GSD_W43_FOLD": "1"},
                                 {"GSD_W43_TW": "4"}], ids=lambda e: "-".join(f"{k[4:]}={v}" for k, v in e.items()) or "default")
def test_w43_restatement_equals_the_library(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check_conv("w43", lib.gsd_conv3x3_w43_partial_rows, lib.gsd_conv3x3_w43_mfma_count, env)


@pytest.mark.parametrize("env", [{}, {"GSD_W2D_TW": "8"}, {"GSD_W2D_TW": "64"}, {"GSD_W2D_TW8_PCT": "0"}],
                         ids=lambda e: "-".join(f"{k[4:]}={v}" for k, v in e.items()) or "default")
def test_w2d_restatement_equals_the_library(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check_conv("w2d", lib.gsd_conv3x3_w2d_partial_rows, lib.gsd_conv3x3_w2d_mfma_count, env)


@pytest.mark.parametrize("env", [{}, {"GSD_WG43_TW": "64"}, {"GSD_WG2D_KX": "1"}, {"GSD_WG2D_KX": "4", "GSD_WG43_TW": "4"}],
                         ids=lambda e: "-".join(f"{k[4:]}={v}" for k, v in e.items()) or "default")
def test_dw_restatements_equal_the_library(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bad = []
    for n, h, w in _grid(env):
        for ci, co in ((64, 64), (32, 128), (48, 64), (64, 130), (20, 20), (128, 256)):
            for form in (1, 2):
                if T.wgrad_mfma_count(form, n, h, w, ci, co, env) != lib.gsd_conv3x3_wgrad_mfma_count(form, n, h, w, ci, co):
                    bad.append(("mfma", form, n, h, w, ci, co))
            if T.wgrad_workspace(n, h, w, ci, co, env) != lib.gsd_conv3x3_wgrad_workspace(n, h, w, ci, co):
                bad.append(("workspace", n, h, w, ci, co))
    assert not bad, bad[:8]


# ------------------------------------------------------------------------------------------------- what the tables reach
def _conv_plans(fam):
    cases = [c for c in T.CONV_CASES + T.SPLIT_CASES if c.fam == fam]
    return [(c, T.conv_plan(fam, c.n, c.h, c.w, c.co, T.env_of(c))) for c in cases]


def _shape_properties(fam):
    """H odd, W = 0..3 (mod 4), more than one tile row / column: each must occur in the family's cases."""
    plans = _conv_plans(fam)
    assert any(c.h % 2 == 1 for c, _ in plans), f"{fam}: no case with odd H"
    for r in range(4):
        assert any(c.w % 4 == r for c, _ in plans), f"{fam}: no case with W = {r} (mod 4)"
    assert any(p.tiles_y > 1 for _, p in plans), f"{fam}: no case with more than one tile row"
    assert any(p.tiles_x > 1 for _, p in plans), f"{fam}: no case with more than one tile column"
    assert all(c.n >= 2 for c, _ in plans), f"{fam}: a case with one image cannot show a read of the wrong image"


def test_cases_reach_every_w2d_tile():
    got = {p.TW for _, p in _conv_plans("w2d")}
    assert got == set(T.W2D_TWS), f"w2d tile widths reached: {sorted(got)}"
    _shape_properties("w2d")


def test_cases_reach_every_w43_tile_and_fold():
    got = {(p.TW, p.fold) for _, p in _conv_plans("w43")}
    want = {(tw, 0) for tw in T.W43_TWS[:5]} | {(tw, 1) for tw in T.W43_TWS}
    assert got == want, f"w43 (TW, fold) missing: {sorted(want - got)}"
    _shape_properties("w43")
    fast = {c.c0 % 4 == 0 and (c.c0 + c.c1) % 4 == 0 for c, _ in _conv_plans("w43")}
    assert fast == {True, False}, "w43: both the straight fills (FAST) and channel counts off a multiple of 4"


def test_cases_reach_both_direct_blocks():
    got = {(p.WM, p.WN) for _, p in _conv_plans("direct")}
    assert got == {(1, 4), (2, 2)}
    _shape_properties("direct")


def test_fused_cases_reach_every_family_and_tile():
    by = {}
    for c in T.FUSED_CASES:
        p = T.conv_plan(c.fam, c.n, c.h, c.w, c.ci, T.env_of(c))
        by.setdefault(c.fam, set()).add(p.TW if c.fam != "direct" else (p.WM, p.WN))
    assert by["w2d"] == set(T.W2D_TWS)
    assert by["direct"] == {(1, 4), (2, 2)}
    assert len(by["w43"]) >= 4


def test_dw_cases_reach_every_stage_and_kstep_shape():
    stages, ksteps, blocks43, blocks2d = set(), set(), set(), set()
    for c in T.WG_CASES:
        ci = c.c0 + c.c1
        if c.form == 1:
            p = T.plan_wg43(c.n, c.h, c.w, c.co, ci, T.env_of(c))
            stages.add((p.TH, p.TW))
            blocks43.add((p.BM, p.BN))
        else:
            p = T.plan_wg2d(c.n, c.h, c.w, c.co, ci, T.env_of(c))
            assert p.ok, c
            ksteps.add((p.KY, p.KX))
            blocks2d.add((p.BM, p.BN))
    assert stages == set(T.WG43_STAGES), f"dW row form stage shapes missing: {sorted(set(T.WG43_STAGES) - stages)}"
    assert ksteps == set(T.WG2D_KSTEPS), f"dW 2-D form k-step shapes missing: {sorted(set(T.WG2D_KSTEPS) - ksteps)}"
    assert blocks43 == {(64, 32), (64, 64), (128, 32)} and blocks2d == {(64, 64), (128, 32)}


def test_the_issue_table_of_shapes():
    """The shapes the case tables were built from, as checked against the built library when the tables were written."""
    w2d = {(2, 4, 64): (4, 64), (2, 12, 45): (4, 64), (2, 3, 37): (4, 64), (3, 30, 7): (30, 8), (2, 23, 5): (24, 8),
           (2, 33, 3): (18, 8)}
    for (n, h, w), (th, tw) in w2d.items():
        p = T.plan_w2d(n, h, w, 64, {})
        assert (p.TH, p.TW) == (th, tw), (n, h, w, p)
    folded = {(3, 18, 20): 4, (3, 9, 50): 8, (3, 9, 11): 16, (2, 6, 70): 16, (2, 4, 17): 24, (3, 5, 53): 28, (3, 13, 28): 28,
              (2, 2, 4): 32, (3, 7, 48): 48, (2, 5, 61): 64}
    for (n, h, w), tw in folded.items():
        p = T.plan_w43(n, h, w, 64, {})
        assert (p.TW, p.fold) == (tw, 1), (n, h, w, p)
    for n in (2, 3):
        for h in range(1, 41):
            for w in range(1, 71):
                assert T.plan_w43(n, h, w, 64, {}).TW != 56, "a small shape picks folded TW 56: use it instead of the knob"
