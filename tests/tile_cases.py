"""Tile planners of the fp32 convolution family restated in plain Python, and the case tables of the smallest shapes that
reach every tile form.  A helper module (imported by tests/test_tile_form_coverage_cpu.py and tests/test_gpu_tile_forms_fp64.py),
not collected; it imports neither torch nor the library.

The restatements follow the host code line by line -- plan_w2d (gsd_conv3x3_w2d.hip), plan_w43 (gsd_conv3x3_w43.hip), choose_tile /
plan_conv3x3 (gsd_conv3x3.hip), plan_wg43 (gsd_wgrad_w43.hip), plan_wg2d (gsd_wgrad_w2d.hip), choose_wgrad_tile / plan_wgrad
(gsd_wgrad.hip: the direct dW form), wgrad_pick_splits (gsd_wgrad_host.h: _splits here) -- including their force knobs, read from `env` (default: the process environment, as the library reads it on
every call).  tests/test_tile_form_coverage_cpu.py holds them to the library over a grid of shapes through the ABI's queries, and
proves through them that the tables below reach every form.

A convolution case is (family, N, H, W, channel layout (C0, C1, Cout), operand form, knobs): see CONV_CASES.  Every shape has
N >= 2 (a read of the wrong image shows), and wherever the form admits it more than one tile in some direction and a partly
filled last tile.
"""
from __future__ import annotations

import os
from collections import namedtuple
from typing import Mapping, Optional


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def round_up(a: int, b: int) -> int:
    return ceil_div(a, b) * b


def env_int(env: Optional[Mapping[str, str]], name: str, dflt: int) -> int:
    """gsd_env_int: atoi of the variable when it is set."""
    v = (os.environ if env is None else env).get(name)
    if v is None:
        return dflt
    v = v.strip()
    k = 1 if v[:1] in "+-" else 0
    while k < len(v) and v[k].isdigit():
        k += 1
    try:
        return int(v[:k])
    except ValueError:
        return 0


# ----------------------------------------------------------------------------------------------- forward / dX planners
Tile = namedtuple("Tile", "TH TW tiles_y tiles_x mblocks fold")
NWP = 2          # gsd_conv3x3_w2d.hip: pixel groups of 16 tiles per block
W2D_TWS = (32, 64, 16, 8)
W43_TWS = (32, 64, 16, 8, 4, 28, 56, 24, 48)        # the last four only folded


def plan_w2d(n: int, h: int, w: int, m: int, env=None) -> Optional[Tile]:
    best_cost, best = -1, None
    force_tw = env_int(env, "GSD_W2D_TW", 0)
    maxpos = 256 * NWP
    for tw in W2D_TWS:
        if force_tw and tw != force_tw:
            continue
        twq = tw // 4
        th = 2 * (16 * NWP // twq)
        if (th + 2) * round_up(tw + 2, 4) > maxpos:
            continue
        ty = ceil_div(h, th)
        th = round_up(ceil_div(h, ty), 2)
        blocks = ty * ceil_div(w, tw) * n
        pref = 0 if tw == 32 else 1 if tw == 64 else 2 if tw == 16 else 3
        cost = (blocks * 8 + pref) * (100 + env_int(env, "GSD_W2D_TW8_PCT", 8) if tw == 8 else 100)
        if best_cost < 0 or cost < best_cost:
            best_cost = cost
            best = Tile(th, tw, ty, ceil_div(w, tw), ceil_div(m, 64), 0)
    return best


def plan_w43(n: int, h: int, w: int, m: int, env=None) -> Optional[Tile]:
    best_cost, best = -1, None
    force_tw = env_int(env, "GSD_W43_TW", 0)
    fold_mode = env_int(env, "GSD_W43_FOLD", -1)
    plain_blocks = -1
    for fold in (0, 1):
        if fold and (fold_mode == 0 or n <= 1 or h * w > 8192):
            continue
        for tw in W43_TWS[:9 if fold else 5]:
            if force_tw and tw != force_tw:
                continue
            twq = tw // 4
            th = 64 // twq
            wcp = round_up(tw + 2, 4)
            while th > 1 and (th + 2) * wcp > 512:
                th -= 1
            if (th + 2) * wcp > 512:
                continue
            rows = n * (h + 1) if fold else h
            th = min(th, rows)
            ty = ceil_div(rows, th)
            if not fold:
                th = ceil_div(h, ty)
            blocks = ty * ceil_div(w, tw) * (1 if fold else n)
            if not fold and (plain_blocks < 0 or blocks < plain_blocks):
                plain_blocks = blocks
            if fold and fold_mode < 0 and blocks * 104 > plain_blocks * 100:
                continue
            cost = blocks * 8 + (0 if tw == 32 else 1 if tw == 64 else 2 if tw == 16 else 3)
            if best_cost < 0 or cost < best_cost:
                best_cost = cost
                best = Tile(th, tw, ty, ceil_div(w, tw), ceil_div(m, 64), fold)
    return best


def choose_tile(h: int, w: int, bn: int):
    """(TH, TW) of the direct form."""
    min_tiles, out = -1, None
    for pas in (0, 1):
        best_score = -1
        for tw in range(1, min(w + 15, bn) + 1):
            th = min(bn // tw, h)
            while th > 1 and (th + 2) * (tw + 2) > 512:
                th -= 1
            if (th + 2) * (tw + 2) > 512:
                continue
            ty = ceil_div(h, th)
            th = ceil_div(h, ty)
            tiles = ty * ceil_div(w, tw)
            if pas == 0:
                if min_tiles < 0 or tiles < min_tiles:
                    min_tiles = tiles
            elif tiles * 100 <= min_tiles * 105:
                score = (1000000 if tw % 16 == 0 else 0) + min(tw, w) * 1000 - tiles
                if score > best_score:
                    best_score = score
                    out = (th, tw)
    return out


Direct = namedtuple("Direct", "TH TW tiles_y tiles_x mblocks WM WN")


def plan_conv3x3(h: int, w: int, m: int) -> Direct:
    """The direct form: block <1,4> (64 x 256) for Cout <= 64, <2,2> (128 x 128) above."""
    wide = m <= 64
    th, tw = choose_tile(h, w, 256 if wide else 128)
    return Direct(th, tw, ceil_div(h, th), ceil_div(w, tw), ceil_div(m, 64 if wide else 128), 1 if wide else 2, 4 if wide else 2)


def conv_plan(fam: str, n: int, h: int, w: int, m: int, env=None):
    return plan_conv3x3(h, w, m) if fam == "direct" else plan_w43(n, h, w, m, env) if fam == "w43" else plan_w2d(n, h, w, m, env)


def conv_partial_rows(fam: str, n: int, h: int, w: int, m: int, env=None) -> int:
    p = conv_plan(fam, n, h, w, m, env)
    if p is None:
        return 0
    if fam == "direct":
        return n * p.tiles_y * p.tiles_x * p.WN
    if fam == "w43":
        return (1 if p.fold else n) * p.tiles_y * p.tiles_x * 4
    return n * p.tiles_y * p.tiles_x * NWP


def conv_mfma_count(fam: str, n: int, h: int, w: int, cin: int, cout: int, env=None) -> int:
    p = conv_plan(fam, n, h, w, cout, env)
    if p is None:
        return 0
    if fam == "w43":
        return (1 if p.fold else n) * p.tiles_y * p.tiles_x * p.mblocks * ceil_div(cin, 4) * (4 * 72)
    return n * p.tiles_y * p.tiles_x * p.mblocks * ceil_div(cin, 4) * (2 * NWP * 48)


# ----------------------------------------------------------------------------------------------------------- dW planners
Wg43 = namedtuple("Wg43", "TH TW BM BN mblocks nblocks stages_total splits slab_elems")
Wg2d = namedtuple("Wg2d", "KY KX BM BN ok mblocks nblocks ksteps_total splits slab_elems")
WG43_STAGES = ((16, 4), (8, 8), (4, 16), (2, 32), (1, 64))
WG2D_KSTEPS = ((1, 4), (2, 2), (4, 1))


def _splits(target: int, blocks: int, total: int) -> int:
    return max(1, min(ceil_div(target, blocks), total, 2048))


def plan_wg43(n: int, h: int, w: int, m: int, ncols: int, env=None) -> Wg43:
    """The row form of dW: 16 Winograd tiles a stage, TH rows of TW / 4."""
    best, th_, tw_ = -1, 0, 0
    force_tw = env_int(env, "GSD_WG43_TW", 0)
    for tw in (4, 8, 16, 32, 64):
        if force_tw and tw != force_tw:
            continue
        th = 64 // tw
        cost = ceil_div(h, th) * ceil_div(w, tw) * (100 if tw == 16 else 107 if tw in (8, 32) else 160)
        if best < 0 or cost < best:
            best, th_, tw_ = cost, th, tw
    bm = 128 if m >= 128 else 64
    bn = 64 if (bm == 64 and ncols >= 64 and tw_ != 64) else 32       # (1 x 64 stages: 64 window columns do not fit the LDS)
    mb, nb = ceil_div(m, bm), ceil_div(ncols, bn)
    total = n * ceil_div(h, th_) * ceil_div(w, tw_)
    target = env_int(env, "GSD_WGRAD_BLOCKS", 512)
    splits = _splits(target // 2 if bm * bn > 64 * 32 else target, mb * nb, total)
    return Wg43(th_, tw_, bm, bn, mb, nb, total, splits, splits * 9 * m * ncols)


def plan_wg2d(n: int, h: int, w: int, m: int, ncols: int, env=None) -> Wg2d:
    """The two-dimensional form of dW: a k-step of KY x KX tiles of 2 x 4 pixels."""
    ty, tx = ceil_div(h, 2), ceil_div(w, 4)
    best, ky_, kx_ = -1, 0, 0
    force_kx = env_int(env, "GSD_WG2D_KX", 0)
    for kx in (4, 2, 1):
        if force_kx and kx != force_kx:
            continue
        ky = 4 // kx
        steps = ceil_div(ty, ky) * ceil_div(tx, kx) * (100 if kx == 4 else 99 if kx == 2 else 112)
        if best < 0 or steps < best:
            best, ky_, kx_ = steps, ky, kx
    bm = 128 if m >= 128 else 64
    bn = 32 if bm == 128 else 64
    ok = m % bm == 0 and ncols % bn == 0
    mb, nb = ceil_div(m, bm), ceil_div(ncols, bn)
    total = n * ceil_div(ty, ky_) * ceil_div(tx, kx_)
    splits = _splits(env_int(env, "GSD_WG2D_BLOCKS", 256), mb * nb, total)
    return Wg2d(ky_, kx_, bm, bn, ok, mb, nb, total, splits, splits * 9 * m * ncols)


def choose_wgrad_tile(h: int, w: int):
    min_work, out = -1, None
    for pas in (0, 1):
        best = -1
        for tw in range(4, 65, 4):
            th = min(64 // tw, h)
            while th > 1 and (th + 2) * (tw + 2) > 256:
                th -= 1
            if (th + 2) * (tw + 2) > 256:
                continue
            ty = ceil_div(h, th)
            th = ceil_div(h, ty)
            stages = ty * ceil_div(w, tw)
            work = stages * th * tw
            if pas == 0:
                if min_work < 0 or work < min_work:
                    min_work = work
                continue
            if work * 100 > min_work * 103:
                continue
            cost = work * 1000 + stages * 10 - tw
            if best < 0 or cost < best:
                best, out = cost, (th, tw)
    return out


def wgrad_direct_slab_elems(n: int, h: int, w: int, m: int, ncols: int, env=None) -> int:
    """plan_wgrad(...).slab_elems: the direct-tap dW form."""
    wide = m <= 64
    ksplit = wide and ncols <= 16
    bnw = 16 if ksplit else (64 if wide else 32)
    th, tw = choose_wgrad_tile(h, w)
    total = n * ceil_div(h, th) * ceil_div(w, tw)
    splits = _splits(env_int(env, "GSD_WGRAD_BLOCKS", 512), ceil_div(m, 64 if wide else 128) * ceil_div(ncols, bnw), total)
    return splits * (36 if ksplit else 9) * m * ncols


def wgrad_workspace(n: int, h: int, w: int, cin: int, cout: int, env=None) -> int:
    """gsd_conv3x3_wgrad_workspace: whichever form may serve the call."""
    g2 = plan_wg2d(n, h, w, cout, cin, env)
    return max(wgrad_direct_slab_elems(n, h, w, cout, cin, env), plan_wg43(n, h, w, cout, cin, env).slab_elems,
               g2.slab_elems if g2.ok else 0)


def wgrad_mfma_count(form: int, n: int, h: int, w: int, cin: int, cout: int, env=None) -> int:
    if form == 1:
        p = plan_wg43(n, h, w, cout, cin, env)
        return p.stages_total * 72 * (p.mblocks * p.BM // 16) * (p.nblocks * p.BN // 16)
    p = plan_wg2d(n, h, w, cout, cin, env)
    return p.ksteps_total * 24 * (cout // 16) * (cin // 16) if p.ok else 0


# ----------------------------------------------------------------------------------------------------------- case tables
# Operand forms of a forward / dX case (how tests/test_gpu_tile_forms_fp64.py lays the source out; dX mirrors it):
#   x4        one plain source, rows pitched to 4 floats and 16-byte aligned, zero pad columns (the aligned 16-byte fills)
#   slack     one plain contiguous source with 4 readable floats either side (the unaligned 16-byte pieces of w2d)
#   slack_bn  the same with deferred BatchNorm + ReLU
#   dword     one contiguous source, no slack, 4 bytes off 16-byte alignment (the dword gathers)
#   two11     two slack segments, the second smaller and at off = (1, 1); dX into two cropped destinations with the same offsets
#   two04     ... the second at off = (0, 4) (off_w % 4 == 0), the first with deferred BatchNorm + ReLU
#   slice     x4 with source and destination given as channels [3, 3 + C) of wider tensors (c_off / c_len)
ConvCase = namedtuple("ConvCase", "fam n h w c0 c1 co form env")


def _cc(fam, n, h, w, c0, c1, co, form, **env):
    return ConvCase(fam, n, h, w, c0, c1, co, form, tuple(sorted(env.items())))


def case_id(c) -> str:
    s = f"{c.fam}-{c.n}x{c.h}x{c.w}-c{c.c0}+{c.c1}-m{c.co}-{c.form}"
    return s + "".join(f"-{k[4:]}={v}" for k, v in c.env)


CONV_CASES = [
    # ---- w2d TW 64
    _cc("w2d", 2, 4, 64, 64, 0, 64, "x4"),
    _cc("w2d", 2, 12, 45, 8, 0, 70, "slack_bn"),            # three tile rows, a partly filled second m-block
    _cc("w2d", 2, 3, 37, 8, 4, 7, "two11"),                 # odd H
    _cc("w2d", 2, 12, 45, 8, 0, 130, "dword"),
    # ---- w2d TW 8: always the dword gathers (4 NI > 8)
    _cc("w2d", 3, 30, 7, 8, 0, 64, "x4"),
    _cc("w2d", 2, 23, 5, 4, 4, 7, "two11"),
    _cc("w2d", 2, 33, 3, 8, 0, 70, "slack_bn"),             # two tile rows
    # ---- w2d TW 16 / 32 off the pyramid
    _cc("w2d", 2, 15, 13, 8, 0, 7, "slack"),
    _cc("w2d", 3, 9, 11, 8, 8, 64, "two11"),                # the 6 x 8 up-sample in a 9 x 11 grid
    _cc("w2d", 2, 7, 29, 12, 0, 130, "x4"),
    _cc("w2d", 2, 21, 29, 8, 8, 70, "two04"),
    _cc("w2d", 2, 6, 70, 8, 0, 64, "dword"),                # three tile columns
    _cc("w2d", 2, 21, 29, 8, 0, 8, "slice"),
    _cc("w2d", 2, 16, 32, 8, 0, 64, "slack"),               # W = 0 (mod 4), full tiles
    # ---- w43 unfolded TW 64 / 4 / 8 / 16 / 32
    _cc("w43", 2, 12, 45, 8, 0, 70, "x4", GSD_W43_FOLD=0),
    _cc("w43", 2, 33, 3, 5, 0, 7, "slack", GSD_W43_FOLD=0),           # FAST = false
    _cc("w43", 3, 30, 7, 6, 5, 64, "two11", GSD_W43_FOLD=0),          # FAST = false, two segments
    _cc("w43", 2, 15, 13, 8, 0, 130, "slack_bn", GSD_W43_FOLD=0),
    _cc("w43", 2, 21, 29, 8, 8, 64, "two04", GSD_W43_FOLD=0),
    _cc("w43", 2, 6, 70, 8, 0, 7, "dword", GSD_W43_FOLD=0),
    # ---- w43 folded TW 4 / 8 / 16 / 24 / 28 / 32 / 48 / 64 (56: no shape with N <= 3, H <= 40, W <= 70 picks it)
    _cc("w43", 3, 18, 20, 8, 0, 64, "x4"),
    _cc("w43", 3, 9, 50, 8, 0, 70, "slack_bn"),
    _cc("w43", 3, 9, 11, 8, 8, 7, "two11"),
    _cc("w43", 2, 6, 70, 6, 5, 64, "two04"),                # FAST = false
    _cc("w43", 2, 4, 17, 5, 0, 130, "dword"),               # FAST = false
    _cc("w43", 3, 5, 53, 8, 0, 64, "slack"),
    _cc("w43", 3, 13, 28, 8, 0, 70, "x4"),
    _cc("w43", 2, 2, 4, 8, 0, 7, "x4"),
    _cc("w43", 3, 7, 48, 8, 4, 64, "two04"),
    _cc("w43", 2, 5, 61, 8, 0, 130, "slack_bn"),
    _cc("w43", 3, 5, 53, 8, 0, 64, "x4", GSD_W43_TW=56, GSD_W43_FOLD=1),
    _cc("w43", 3, 13, 28, 8, 0, 8, "slice"),
    # ---- direct: block <1,4> (Cout <= 64) and <2,2> (Cout > 64)
    _cc("direct", 2, 9, 11, 3, 0, 64, "slack"),
    _cc("direct", 2, 21, 29, 5, 0, 130, "dword"),
    _cc("direct", 2, 6, 70, 4, 3, 70, "two11"),
    _cc("direct", 3, 15, 13, 8, 0, 7, "slack_bn"),
    _cc("direct", 2, 7, 32, 4, 4, 130, "two04"),
]

# forced K-slab split (GSD_W43_SPLIT / GSD_W2D_SPLIT) on one TW-64 and one TW-8 shape, two-destination epilogue; Cout = Cin, so
# that the dX launch (which contracts over Cout) admits the same slab count
SPLIT_CASES = [_cc(fam, n, h, w, ci // 2, ci // 2, ci, "two11", **{f"GSD_{fam.upper()}_SPLIT": s, **env})
               for fam, env in (("w43", {"GSD_W43_FOLD": 0}), ("w2d", {}))
               for n, h, w in ((2, 12, 45), (3, 30, 7)) for ci, s in ((64, 2), (96, 3))]

# fused dX epilogue (gsd_conv3x3[_w43|_w2d]_dgrad_bnrelu[_ws]): one shape per tile form; (family, N, H, W, Cout of the
# forward = channels of dy, Cin = channels of dz, knobs)
FusedCase = namedtuple("FusedCase", "fam n h w co ci env")
FUSED_CASES = [FusedCase(*a, tuple(sorted(e.items()))) for a, e in [
    (("w2d", 2, 12, 45, 8, 70), {}), (("w2d", 3, 30, 7, 8, 64), {}), (("w2d", 2, 15, 13, 12, 7), {}), (("w2d", 2, 21, 29, 8, 130), {}),
    (("w2d", 2, 12, 45, 64, 64), {"GSD_W2D_SPLIT": 2}),
    (("w43", 2, 12, 45, 8, 70), {"GSD_W43_FOLD": 0}), (("w43", 2, 33, 3, 5, 7), {"GSD_W43_FOLD": 0}),
    (("w43", 3, 30, 7, 8, 64), {"GSD_W43_FOLD": 0}), (("w43", 3, 9, 11, 8, 130), {}), (("w43", 3, 5, 53, 8, 64), {}),
    (("w43", 3, 7, 48, 64, 64), {"GSD_W43_SPLIT": 2}),
    (("direct", 2, 9, 11, 8, 64), {}), (("direct", 2, 21, 29, 5, 130), {}),
]]

# dW (gsd_conv3x3_wgrad): (N, H, W, C0, C1, Cout, dy pitched to 4 floats and aligned, activation slack, deferred BatchNorm on the
# first segment, the form gsd_conv3x3_wgrad_form must report, knobs)
WgCase = namedtuple("WgCase", "n h w c0 c1 co pitched slack bn form env")
WG_CASES = [WgCase(*a, tuple(sorted(e.items()))) for a, e in [
    # row form (1): stage shapes (2,32) / (8,8) / (16,4) / (1,64) / (4,16), blocks (64,32) / (64,64) / (128,32)
    ((2, 21, 29, 48, 0, 64, True, 4, False, 1), {}),          # Cin off the 64-column block grid
    ((2, 6, 70, 64, 0, 70, True, 4, True, 1), {}),            # a partly filled m-block
    ((2, 33, 3, 32, 32, 128, False, 0, False, 1), {}),        # unpitched dy, no slack; a[0].C on the block size
    ((2, 1, 40, 20, 44, 64, True, 4, False, 1), {}),          # a[0].C off the block size (a launch the library refused: LDS)
    ((2, 15, 13, 64, 0, 64, False, 0, True, 1), {}),
    ((2, 15, 13, 64, 0, 128, True, 4, False, 1), {"GSD_WGRAD_W2D": 0}),     # the row-reuse stage 4 x 16
    ((2, 6, 70, 64, 0, 64, True, 4, False, 1), {"GSD_WGRAD_W2D": 0}),       # the row-reuse stage 8 x 8
    # two-dimensional form (2): k-steps (1,4) / (4,1) / (2,2), blocks (64,64) / (128,32)
    ((2, 21, 29, 64, 0, 64, True, 4, False, 2), {}),
    ((2, 21, 29, 32, 0, 128, True, 4, True, 2), {}),
    ((2, 33, 3, 64, 0, 64, True, 4, True, 2), {}),
    ((2, 33, 3, 32, 0, 128, True, 4, False, 2), {}),
    ((2, 15, 13, 64, 64, 64, True, 4, True, 2), {}),             # two segments, a[0].C on the block size
]]

WGRAD_BN_SHAPES = [(2, 9, 37), (1, 5, 16), (3, 7, 50)]

# ConvTranspose2d 2x2/s2: (N, H, W, Cin, Cout)
CONVT_CASES = [(2, 4, 5, 8, 32), (3, 5, 53, 36, 40), (2, 7, 9, 264, 32), (1, 3, 2, 36, 40)]


def second_segment(form, h, w):
    """(off_h, off_w, H, W) of the second source segment: smaller than the grid, as F.pad of an up-sampled tensor leaves it."""
    if form == "two11":
        oh, ow = (1 if h >= 3 else 0), (1 if w >= 3 else 0)
        return oh, ow, h - oh - (1 if h >= 4 else 0), w - ow - (1 if w >= 4 else 0)
    ow = 4 if w >= 6 else 0
    return 0, ow, (h - 1 if h > 1 else h), (w - ow - 1 if w - ow > 1 else w - ow)


def env_of(case) -> dict:
    return {k: str(v) for k, v in case.env}
