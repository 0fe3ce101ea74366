"""Host planners of the bf16 convolution family restated in plain Python, and the case tables of the smallest shapes that reach
every kernel instantiation and tile they can pick.  A helper module (imported by tests/test_bf16_tile_form_coverage_cpu.py and
tests/test_gpu_bf16_tile_forms_fp64.py), not collected; it imports neither torch nor the library.

The restatements follow the host code line by line, force knobs included (read from `env`; default: the process environment, as
the library reads it on every call); `cus` is the CU count the planners size their grids by (256: what the library assumes
without a device, and what the MI355X reports):
  gsd_bf16_host.h      bf16_pick_tile (the loop of make_plan and of make_wplan, with either tie rule), bf16_mblock_grid (launch_grid
                       here, and the grid of ct_plan), bf16_xcd_order (xcd_on here)                               (GSD_BF16_XCD)
  gsd_bf16_conv.hip    make_plan, gsd_bf16_conv_partial_rows, the BUF rule of conv3x3_impl, gsd_bf16_conv_dense_partial_rows
                                                                    (GSD_BF16_TW, GSD_BF16_CONV_BUF)
  gsd_bf16_ctgemm.hip  ct_plan, gsd_ctgemm_shape, gsd_ctgemm_operands, gsd_ctgemm_partial_rows      (GSD_BF16_CTGEMM, GSD_BF16_CT_BM)
  gsd_bf16_wgrad.hip   make_wplan, make_bigplan, gsd_bf16_wgrad_workspace and the dispatch of gsd_bf16_wgrad
                                                                    (GSD_BF16_WGRAD_BLOCKS, GSD_BF16_WGRAD_BIG)

form_of(case) names the kernel instantiation and tile a case runs:
  ("conv3x3", wide, TW, BUF, epilogue)          gconv_bf16_kernel<0, wide ? 1,4 : 2,2, BUF>; epilogue "stats" | "bnbwd" | "bnrelu"
  ("dense", wide, TW, ntaps, stride, epilogue)  gconv_bf16_kernel<1, ..>; epilogue "plain" | "bnrelu" | "scatter" | "bnbwd"
  ("ct", DX, BM, fused)                         ctgemm_bf16_kernel<0,4,2,8> / <1,4,2,8> (BM 256) / <1,2,4,4> (BM 128)
  ("wgrad", HALO, T, wide, TW)                  gwgrad_bf16_kernel<HALO, T, wide ? 1,4 : 2,2>
  ("wgrad_big", BM)                             gwgrad_big_bf16_kernel<4,2> (BM 256) / <2,4> (BM 128)

What restating ct_plan showed: a dX launch takes the 256-row tile only under GSD_BF16_CT_BM=256 -- by default every dX shape
(M % 128 == 0) runs <1,2,4,4>, M = 256 with two m-blocks.  The dX rows of CT_CASES that name BM 256 therefore set the knob.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

from tile_cases import ceil_div, env_int, round_up

CUS = 256


# ------------------------------------------------------------------------------------------------------ gsd_bf16_conv.hip
Plan = namedtuple("Plan", "wide BM NPX TH TW tiles_y tiles_x mblocks Mpad HC HP")


def make_plan(h: int, w: int, m: int, env=None) -> Plan:
    wide = m <= 64
    bm = 64 if wide else 128
    npx = 512 if wide else 256
    best, tw_, th_ = -1, 0, 0
    force_tw = env_int(env, "GSD_BF16_TW", 0)
    for tw in (16, 32, 64):
        if force_tw and tw != force_tw:
            continue
        th = npx // tw
        cost = ceil_div(h, th) * ceil_div(w, tw)
        if best < 0 or cost <= best:        # ties -> wider rows
            best, tw_, th_ = cost, tw, th
    return Plan(wide, bm, npx, th_, tw_, ceil_div(h, th_), ceil_div(w, tw_), ceil_div(m, bm), round_up(m, 128), tw_ + 2,
                (th_ + 2) * (tw_ + 2))


def launch_grid(items: int, mblocks: int, cus: int = CUS) -> int:
    grid = cus // mblocks * mblocks
    if grid < mblocks:
        grid = mblocks
    return items if grid > items else grid


def xcd_on(grid: int, mblocks: int, env=None) -> bool:
    return env_int(env, "GSD_BF16_XCD", 1) != 0 and grid % 8 == 0 and (grid // 8) % mblocks == 0


def conv_items(n: int, h: int, w: int, m: int, env=None) -> int:
    p = make_plan(h, w, m, env)
    return n * p.tiles_y * p.tiles_x * p.mblocks


def conv_partial_rows(n: int, h: int, w: int, m: int, env=None, cus: int = CUS) -> int:
    if n <= 0 or h <= 0 or w <= 0 or m <= 0:
        return 0
    p = make_plan(h, w, m, env)
    return launch_grid(n * p.tiles_y * p.tiles_x * p.mblocks, p.mblocks, cus) // p.mblocks * (4 if p.wide else 2)


def conv_buf(h: int, w: int, in_pitch: int, m: int, k: int, env=None) -> int:
    """conv3x3_impl: fills through buffer descriptors when one image and the weight image stay below 2 GiB."""
    ib = h * w * in_pitch * 2
    wb = 9 * round_up(m, 128) * k * 2
    return 1 if ib < (1 << 31) and wb < (1 << 31) and env_int(env, "GSD_BF16_CONV_BUF", 1) != 0 else 0


# ---------------------------------------------------------------------------------------------------- gsd_bf16_ctgemm.hip
CtPlan = namedtuple("CtPlan", "ok BM NPX WN mblocks ntile grid")
CT_NO = CtPlan(False, 0, 0, 0, 0, 0, 0)


def ct_plan(ppix: int, m: int, dx: bool, env=None, cus: int = CUS) -> CtPlan:
    if ppix <= 0 or ppix >= (1 << 24):
        return CT_NO
    force = env_int(env, "GSD_BF16_CT_BM", 0)
    if m % 256 == 0 and force != 128 and not (dx and force != 256):
        bm, wn = 256, 2
    elif m % 128 == 0 and dx:
        bm, wn = 128, 4
    else:
        return CT_NO
    npx = 256
    mblocks = m // bm
    ntile = (ppix + npx - 1) // npx
    grid = cus // mblocks * mblocks
    if grid < mblocks:
        return CT_NO
    items = ntile * mblocks
    if grid > items:
        grid = items
    return CtPlan(True, bm, npx, wn, mblocks, ntile, grid)


def ctgemm_shape(n, h, w, k, m, ntaps, stride, scatter_cs, env=None, cus: int = CUS) -> bool:
    if env_int(env, "GSD_BF16_CTGEMM", 1) == 0:
        return False
    if k <= 0 or k % 64 != 0 or w < 16 or n <= 0 or h <= 0:
        return False
    fwd = ntaps == 1 and stride == 1 and scatter_cs > 0 and scatter_cs % 64 == 0
    dx = ntaps == 4 and stride == 2 and scatter_cs == 0
    return (fwd or dx) and ct_plan(n * h * w, m, dx, env, cus).ok


Buf = namedtuple("Buf", "N H W pitch")      # the extent and pixel pitch of a gsd_nhwc


def ctgemm_operands(in_: Buf, out: Buf, bw_y: Optional[Buf], ntaps: int, ty, tx, h: int, w: int) -> bool:
    def fits(t):
        return (t.N * t.H * t.W + 512) * t.pitch < 2147483647
    if not fits(in_) or not fits(out):
        return False
    if bw_y is not None and not fits(bw_y):
        return False
    if ntaps == 1:
        return ty[0] == 0 and tx[0] == 0 and in_.H == h and in_.W == w
    if out.H != h or out.W != w:
        return False
    oy, ox = ty[0], tx[0]
    if oy < 0 or ox < 0 or ty[1] != oy or tx[1] != ox + 1 or ty[2] != oy + 1 or tx[2] != ox or ty[3] != oy + 1 or tx[3] != ox + 1:
        return False
    return 2 * (h - 1) + oy + 1 < in_.H and 2 * (w - 1) + ox + 1 < in_.W


def ctgemm_partial_rows(n, h, w, m, env=None, cus: int = CUS) -> int:
    pl = ct_plan(n * h * w, m, True, env, cus)
    return pl.grid // pl.mblocks * pl.WN if pl.ok else 0


def conv_dense_partial_rows(n, h, w, k, m, ntaps, stride, env=None, cus: int = CUS) -> int:
    if ctgemm_shape(n, h, w, k, m, ntaps, stride, 0, env, cus):
        return ctgemm_partial_rows(n, h, w, m, env, cus)
    return conv_partial_rows(n, h, w, m, env, cus)


# ----------------------------------------------------------------------------------------------------- gsd_bf16_wgrad.hip
WPlan = namedtuple("WPlan", "wide BM BNC NPIX TH TW tiles_y tiles_x mblocks nblocks stages_total splits slab_elems")


def make_wplan(halo: bool, t: int, n, h, w, m, ncols, env=None) -> WPlan:
    wide = m <= 64
    bm = 64 if wide else 128
    bnc = 64 if wide else 32
    npix = 128 if halo else 64
    best, tw_, th_ = -1, 0, 0
    for tw in (32, 64):
        th = npix // tw
        cost = ceil_div(h, th) * ceil_div(w, tw)
        if best < 0 or cost < best:         # ties -> the narrower tile
            best, tw_, th_ = cost, tw, th
    tiles_y, tiles_x = ceil_div(h, th_), ceil_div(w, tw_)
    mblocks, nblocks = ceil_div(m, bm), ceil_div(ncols, bnc)
    stages_total = n * tiles_y * tiles_x
    target = env_int(env, "GSD_BF16_WGRAD_BLOCKS", 512)
    splits = ceil_div(target, mblocks * nblocks)
    if splits > stages_total:
        splits = stages_total
    if splits < 1:
        splits = 1
    return WPlan(wide, bm, bnc, npix, th_, tw_, tiles_y, tiles_x, mblocks, nblocks, stages_total, splits, splits * t * m * ncols)


BigPlan = namedtuple("BigPlan", "ok BM mblocks nblocks stages_total splits slab_elems")
BIG_NO = BigPlan(False, 0, 0, 0, 0, 0, 0)


def make_bigplan(ntaps, n, h, w, m, ncols, env=None, cus: int = CUS) -> BigPlan:
    p = n * h * w
    if ntaps != 4 or m % 128 != 0 or ncols % 64 != 0 or p >= (1 << 24) or env_int(env, "GSD_BF16_WGRAD_BIG", 1) == 0:
        return BIG_NO
    bm = 256 if m % 256 == 0 else 128
    mblocks, nblocks = m // bm, ncols // 64
    stages_total = (p + 63) // 64
    splits = cus // (mblocks * nblocks)
    if splits < 1:
        splits = 1
    if splits > stages_total:
        splits = stages_total
    return BigPlan(True, bm, mblocks, nblocks, stages_total, splits, splits * 4 * m * ncols)


def wgrad_workspace(ntaps, n, h, w, m, ncols, env=None, cus: int = CUS) -> int:
    if ntaps < 1 or ntaps > 9 or n <= 0 or h <= 0 or w <= 0 or m <= 0 or ncols <= 0:
        return 0
    return max(make_wplan(ntaps == 9, ntaps, n, h, w, m, ncols, env).slab_elems, make_bigplan(ntaps, n, h, w, m, ncols, env, cus).slab_elems)


def wgrad_big(a: Buf, b: Buf, m, ncols, ntaps, stride, ty, tx, env=None, cus: int = CUS) -> bool:
    """The dispatch of gsd_bf16_wgrad: the large tile only at stride 2 with all four taps of every pixel inside b."""
    bp = make_bigplan(ntaps, a.N, a.H, a.W, m, ncols, env, cus)
    if not (bp.ok and stride == 2 and a.N * a.H * a.W * a.pitch < 2147483647 and b.N * b.H * b.W * b.pitch < 2147483647):
        return False
    return all(ty[t] >= 0 and tx[t] >= 0 and 2 * (a.H - 1) + ty[t] < b.H and 2 * (a.W - 1) + tx[t] < b.W for t in range(4))


# ------------------------------------------------------------------------------------------------------------ case tables
def env_of(c) -> dict:
    return dict(c.env)


def _id(prefix, c, *extra):
    e = "-".join(f"{k[4:]}={v}" for k, v in c.env)
    return "-".join(str(x) for x in (prefix, f"{c.n}x{c.h}x{c.w}") + extra + ((e,) if e else ()))


# conv3x3 (gsd_bf16_conv3x3 / _bnrelu).  ep: "stats" (plain, with the statistics of the stored values), "bnbwd" (a dX launch with
# the fused BatchNorm-backward pass 1: K = Cout, M = Cin of the unit, dgrad weight image) or "bnrelu" (eval epilogue).
# in_tot/in_off, out_tot/out_off: the operand is channels [off, off + C) of a buffer of tot channels.
Conv3 = namedtuple("Conv3", "n h w k m ep in_tot in_off out_tot out_off env form")


def _c3(n, h, w, k, m, wide, tw, buf=1, ep="stats", in_=None, out=None):
    env = (("GSD_BF16_CONV_BUF", "0"),) if not buf else ()
    it, io = in_ or (k, 0)
    ot, oo = out or (m, 0)
    return Conv3(n, h, w, k, m, ep, it, io, ot, oo, env, ("conv3x3", wide, tw, buf, ep))


CONV3_CASES = []
for _buf in (1, 0):
    CONV3_CASES += [
        _c3(2, 20, 10, 32, 80, False, 16, _buf),       # narrow TW 16: two tile rows, the second a quarter full; M off the block
        _c3(2, 13, 27, 96, 128, False, 32, _buf),      # narrow TW 32: two tile rows, last column partly filled
        _c3(2, 4, 70, 32, 256, False, 64, _buf),       # narrow TW 64: two tile columns, two m-blocks
        _c3(2, 7, 100, 96, 80, False, 64, _buf),       # narrow TW 64: 2 x 2 tiles, both last tiles partly filled
        _c3(2, 40, 10, 96, 48, True, 16, _buf),        # wide TW 16: two tile rows, M = 48 off the block
        _c3(2, 20, 27, 32, 64, True, 32, _buf),        # wide TW 32: two tile rows
        _c3(2, 8, 70, 96, 64, True, 64, _buf),         # wide TW 64: two tile columns
        _c3(2, 11, 100, 32, 48, True, 64, _buf),       # wide TW 64: 2 x 2 tiles
        _c3(2, 13, 27, 128, 96, False, 32, _buf, "bnbwd"),     # dX of a 96 -> 128 unit with the fused pass 1, ragged M
        _c3(2, 8, 70, 64, 64, True, 64, _buf, "bnbwd"),        # dX of a 64 -> 64 unit with the fused pass 1
    ]
CONV3_CASES += [
    _c3(2, 13, 27, 32, 128, False, 32, ep="bnrelu"),
    _c3(2, 20, 27, 96, 48, True, 32, ep="bnrelu"),
    _c3(2, 7, 100, 32, 80, False, 64, in_=(96, 32)),           # the input is channels [32, 64) of 96
    _c3(2, 20, 27, 32, 48, True, 32, out=(80, 16)),            # the output is channels [16, 64) of 80
    _c3(8, 64, 128, 32, 256, False, 64),                       # 512 items on 256 persistent blocks (XCD order)
    _c3(2, 29, 40, 32, 128, False, 16),                        # narrow TW 16 tiling in both directions: 2 x 3 tiles
    _c3(2, 13, 90, 32, 80, False, 32),                         # narrow TW 32: 2 x 3 tiles
    _c3(2, 58, 40, 32, 64, True, 16),                          # wide TW 16: 2 x 3 tiles
    _c3(2, 29, 90, 32, 48, True, 32),                          # wide TW 32: 2 x 3 tiles
]

# gsd_bf16_conv_dense on the general kernel.  kind:
#   "1x1"      one tap, plain output                         "1x1bnrelu" gsd_bf16_conv1x1_bnrelu
#   "ctfwd"    ConvT forward: one tap, scatter (cs, oy, ox) + bias into a buffer `spare` rows / columns larger than the block
#   "ctdx"     ConvT dX: 4 taps at stride 2 from the gradient slice at (oy, ox); fused: with the BatchNorm-backward pass 1;
#              crop = 1: the gradient buffer has 2H - 1 rows and 2W - 1 columns (the last taps leave it and read zeros);
#              opad: the output buffer is opad rows and columns larger than the pixel grid (the large-tile kernel addresses its
#              output by the flattened pixel index, so such a launch belongs to the general kernel)
# want: the return code the launch must give (0, or -2 = GSD_ERR_UNSUPPORTED for the refused fallback).
Dense = namedtuple("Dense", "kind n h w k m cs oy ox spare fused crop opad env want form")


def _dn(kind, n, h, w, k, m, wide, tw, cs=0, oy=0, ox=0, spare=0, fused=0, crop=0, opad=0, env=(), want=0):
    taps, stride = (4, 2) if kind == "ctdx" else (1, 1)
    ep = {"1x1": "plain", "1x1bnrelu": "bnrelu", "ctfwd": "scatter", "ctdx": "bnbwd" if fused else "plain"}[kind]
    form = ("dense", wide, tw, taps, stride, ep) if want == 0 else ("refused",)
    return Dense(kind, n, h, w, k, m, cs, oy, ox, spare, fused, crop, opad, tuple(env), want, form)


_NOCT = (("GSD_BF16_CTGEMM", "0"),)
DENSE_CASES = [
    _dn("1x1", 2, 21, 37, 32, 64, True, 64),                   # wide: K 32 -> M 64, 3 x 1 tiles per image
    _dn("1x1", 2, 13, 27, 64, 128, False, 32),                 # narrow: K 64 -> M 128 (two k sub-chunks per barrier)
    _dn("1x1", 2, 20, 10, 64, 80, False, 16),                  # narrow TW 16, M off the block
    _dn("1x1", 2, 40, 10, 32, 48, True, 16),                   # wide TW 16, M = 48
    _dn("1x1", 8, 64, 128, 64, 256, False, 64),                # 512 items on 256 blocks
    _dn("1x1bnrelu", 2, 20, 27, 32, 64, True, 32),
    _dn("1x1bnrelu", 2, 7, 100, 64, 128, False, 64),
] + [
    _dn("ctfwd", 2, 10, 13, 64, 4 * cs, cs == 16, 16 if cs == 32 else 32, cs=cs, oy=oy, ox=ox, spare=sp)
    for cs in (16, 32) for (oy, ox, sp) in ((0, 0, 0), (0, 1, 1), (1, 0, 2), (1, 1, 0))
] + [
    _dn("ctdx", 2, 10, 13, 32, 64, True, 32, oy=0, ox=1),                        # wide, K % 64 != 0
    _dn("ctdx", 2, 10, 13, 32, 64, True, 32, oy=1, ox=0, fused=1),
    _dn("ctdx", 2, 10, 13, 64, 128, False, 16, oy=1, ox=1),                      # narrow: W < 16 keeps it off the large tile
    _dn("ctdx", 2, 10, 13, 64, 128, False, 16, oy=0, ox=0, fused=1),
    _dn("ctdx", 2, 9, 29, 64, 256, False, 32, oy=0, ox=1, fused=1, env=_NOCT),    # a large-tile shape held on the general kernel
    _dn("ctdx", 2, 10, 13, 32, 64, True, 32, crop=1),                            # cropped gradient buffer: zeros outside
    _dn("ctdx", 2, 9, 29, 64, 256, False, 32, crop=1),                           # ... at a large-tile shape: falls back, plain
    _dn("ctdx", 2, 9, 29, 64, 256, False, 32, crop=1, fused=1, want=-2),         # ... fused with statistics: refused
    _dn("ctdx", 2, 9, 29, 64, 256, False, 32, oy=1, ox=0, opad=1),               # a large-tile shape whose output buffer is larger than the grid
]

# The large-tile kernel (gsd_bf16_ctgemm.hip).  dx = 0: forward, K -> M = 4 Cs scattered at (oy, ox) with bias into a buffer
# `spare` larger; dx = 1: dX, K per tap (= Cout) -> M (= Cin) from the second half of a concat gradient buffer of extent
# (2H + oy + spare, 2W + ox + spare), plain or fused.
Ct = namedtuple("Ct", "dx n h w k m oy ox spare fused env form")


def _ct(dx, n, h, w, k, m, oy, ox, spare=0, fused=0, bm=None, env=()):
    env = tuple(env)
    if dx and bm == 256:
        env += (("GSD_BF16_CT_BM", "256"),)
    return Ct(dx, n, h, w, k, m, oy, ox, spare, fused, env, ("ct", dx, bm or (256 if not dx else 128), bool(fused)))


_XCD0 = (("GSD_BF16_XCD", "0"),)
CT_CASES = [
    # forward: Cs = 64 -> M = 256, Cs = 128 -> M = 512 (two m-blocks)
    _ct(0, 2, 3, 16, 64, 256, 0, 0),               # P = 96 < 256, W = 16: every 16-pixel step wraps a row
    _ct(0, 3, 5, 17, 128, 512, 0, 1, spare=1),     # P = 255, W = 17, one tile holds three images, two m-blocks
    _ct(0, 2, 8, 16, 128, 256, 1, 0),              # P = 256 exactly
    _ct(0, 2, 9, 29, 64, 512, 1, 1, spare=2),      # P = 522: three tiles, the last 10 pixels
    _ct(0, 5, 1, 53, 64, 256, 1, 1),               # H = 1: every row wrap is an image wrap; tile 0 holds five images
    _ct(0, 3, 2, 40, 128, 256, 0, 1, spare=1),     # P = 240: three images in one tile
    _ct(0, 3, 150, 150, 64, 256, 0, 1),            # 264 tiles on 256 blocks, XCD order
    _ct(0, 3, 150, 150, 64, 256, 1, 0, env=_XCD0),  # ... and plain order
]
for _f in (0, 1):
    CT_CASES += [
        # dX: <1,2,4,4> (BM 128) by default, <1,4,2,8> (BM 256) under GSD_BF16_CT_BM=256
        _ct(1, 2, 3, 16, 64, 256, 0, 0, fused=_f, bm=256),
        _ct(1, 3, 5, 17, 128, 256, 0, 1, spare=1, fused=_f, bm=256),
        _ct(1, 2, 8, 16, 64, 128, 1, 0, fused=_f),
        _ct(1, 2, 9, 29, 128, 384, 1, 1, spare=2, fused=_f),
        _ct(1, 5, 1, 53, 64, 256, 1, 1, fused=_f, env=(("GSD_BF16_CT_BM", "128"),)),
        _ct(1, 3, 2, 40, 128, 128, 0, 1, spare=1, fused=_f),
        _ct(1, 2, 9, 29, 64, 256, 0, 0, fused=_f, bm=256),
        _ct(1, 5, 1, 53, 128, 384, 1, 0, spare=1, fused=_f),
    ]
CT_CASES += [
    _ct(1, 2, 130, 130, 64, 256, 0, 1, fused=1),                 # 133 tiles x 2 m-blocks on 256 blocks, XCD order
    _ct(1, 2, 130, 130, 64, 256, 1, 0, fused=1, env=_XCD0),
]

# gsd_bf16_wgrad on the general kernel.  taps 9: a = dy (m channels), b = the layer input (ncols channels), same extent;
# taps 4: ConvT dW at stride 2, b the gradient slice at (oy, ox) of a buffer of extent (2H + oy, 2W + ox); taps 1: b has
# ncols channels of which ncols_out leave.  b_tot / b_off: b is channels [off, off + ncols) of b_tot.
Wg = namedtuple("Wg", "taps n h w m ncols ncols_out oy ox b_tot b_off crop env form")


def _wg(taps, n, h, w, m, ncols, tw, ncols_out=None, oy=0, ox=0, b=None, crop=0, env=(), big=None):
    bt, bo = b or (ncols, 0)
    form = ("wgrad_big", big) if big else ("wgrad", 1 if taps == 9 else 0, taps, m <= 64, tw)
    return Wg(taps, n, h, w, m, ncols, ncols_out or ncols, oy, ox, bt, bo, crop, tuple(env), form)


def _blocks(k):
    return (("GSD_BF16_WGRAD_BLOCKS", str(k)),)


_NOBIG = (("GSD_BF16_WGRAD_BIG", "0"),)
WG_CASES = [
    # (HALO 1, T 9)
    _wg(9, 2, 5, 27, 128, 64, 32),                             # narrow TW 32: two tile rows, two n-blocks
    _wg(9, 3, 9, 70, 80, 48, 32, b=(96, 32)),                  # narrow TW 32: 3 x 3 tiles, ragged M and Ncols, b a channel slice
    _wg(9, 2, 5, 50, 128, 32, 64),                             # narrow TW 64: three tile rows
    _wg(9, 2, 2, 100, 256, 40, 64, env=_blocks(6)),            # narrow TW 64: two tile columns, stages_total 4 > splits 2
    _wg(9, 2, 5, 27, 64, 96, 32),                              # wide TW 32, ragged n-block
    _wg(9, 3, 9, 70, 48, 64, 32, env=_blocks(4)),              # wide TW 32: M = 48, 27 stages in 4 splits
    _wg(9, 2, 5, 50, 64, 64, 64),                              # wide TW 64
    _wg(9, 2, 2, 100, 48, 32, 64, b=(64, 16)),                 # wide TW 64: two tile columns, b a slice at an offset
    # (HALO 0, T 4) at stride 2
    _wg(4, 2, 4, 20, 128, 32, 32, oy=0, ox=1, b=(64, 32)),     # narrow TW 32
    _wg(4, 2, 3, 40, 128, 48, 64, oy=1, ox=0, b=(96, 48)),     # narrow TW 64, ragged Ncols
    _wg(4, 2, 4, 20, 64, 48, 32, oy=1, ox=1, b=(96, 48)),      # wide TW 32, ragged Ncols
    _wg(4, 2, 3, 40, 64, 32, 64, oy=0, ox=0, b=(64, 32)),      # wide TW 64
    _wg(4, 3, 7, 19, 128, 64, 32, oy=0, ox=1, b=(128, 64), env=_NOBIG + _blocks(5)),    # a large-tile shape held back; 12 stages in 3 splits
    _wg(4, 3, 7, 19, 48, 32, 32, oy=1, ox=0, b=(64, 32), env=_blocks(2)),               # wide, M = 48; 12 stages in 2 splits
    # (HALO 0, T 1): the first layer's im2col'd input, 32 channels of which 27 leave
    _wg(1, 2, 19, 33, 64, 32, 64, ncols_out=27),               # wide TW 64
    _wg(1, 2, 19, 27, 64, 32, 32, ncols_out=27, env=_blocks(3)),    # wide TW 32; 20 stages in 3 splits
    _wg(1, 2, 19, 33, 128, 32, 64, ncols_out=27),              # narrow TW 64
    _wg(1, 2, 19, 27, 80, 32, 32, ncols_out=27, env=_blocks(3)),    # narrow TW 32, ragged M
]

# gsd_bf16_wgrad on the large tile (4 taps at stride 2, M % 128 == 0, Ncols % 64 == 0) and its fallback.
WGBIG_CASES = [
    _wg(4, 1, 3, 16, 256, 64, 0, oy=0, ox=0, b=(128, 64), big=256),         # P = 48 < 64: one stage, partly filled
    _wg(4, 2, 5, 13, 128, 128, 0, oy=0, ox=1, b=(256, 128), big=128),       # P = 130: the third stage holds 2 pixels
    _wg(4, 3, 7, 19, 384, 64, 0, oy=1, ox=0, b=(128, 64), big=128),         # P = 399, three m-blocks
    _wg(4, 2, 5, 13, 512, 256, 0, oy=1, ox=1, b=(512, 256), big=256),       # two m-blocks x four n-blocks
    _wg(4, 2, 30, 37, 512, 256, 0, oy=0, ox=1, b=(512, 256), big=256),      # 35 stages in 32 splits: one or two stages each
    _wg(4, 3, 7, 19, 128, 64, 0, oy=1, ox=1, b=(128, 64), big=128),
    _wg(4, 2, 5, 13, 128, 128, 32, oy=0, ox=0, b=(256, 128), crop=1),       # b cropped to (2H - 1, 2W - 1): the general kernel
]


def conv3_id(c):
    return _id("c3", c, f"k{c.k}-m{c.m}", c.ep, *(("in",) if c.in_tot > c.k else ()), *(("out",) if c.out_tot > c.m else ()))


def dense_id(c):
    return _id(c.kind, c, f"k{c.k}-m{c.m}", f"o{c.oy}{c.ox}", *(("fused",) if c.fused else ()), *(("crop",) if c.crop else ()),
               *(("opad",) if c.opad else ()))


def ct_id(c):
    return _id("dx" if c.dx else "fwd", c, f"k{c.k}-m{c.m}", f"o{c.oy}{c.ox}s{c.spare}", *(("fused",) if c.fused else ()))


def wg_id(c):
    return _id(f"t{c.taps}", c, f"m{c.m}-n{c.ncols}", f"o{c.oy}{c.ox}", *(("crop",) if c.crop else ()))


# ------------------------------------------------------------------------------------------------------- geometry of a case
def dense_geometry(c: Dense):
    """(in Buf, out Buf, ty, tx) of a dense / large-tile ConvT case as the GPU module builds its buffers."""
    if c.kind == "ctdx":
        gh, gw = (2 * c.h - 1, 2 * c.w - 1) if c.crop else (2 * c.h + c.oy + c.spare, 2 * c.w + c.ox + c.spare)
        return (Buf(c.n, gh, gw, 2 * c.k), Buf(c.n, c.h + c.opad, c.w + c.opad, c.m), [c.oy, c.oy, c.oy + 1, c.oy + 1], [c.ox, c.ox + 1, c.ox, c.ox + 1])
    if c.kind == "ctfwd":
        return (Buf(c.n, c.h, c.w, c.k), Buf(c.n, 2 * c.h + c.oy + c.spare, 2 * c.w + c.ox + c.spare, 2 * c.cs), [0], [0])
    return Buf(c.n, c.h, c.w, c.k), Buf(c.n, c.h, c.w, c.m), [0], [0]


def ct_as_dense(c: Ct) -> Dense:
    if c.dx:
        return Dense("ctdx", c.n, c.h, c.w, c.k, c.m, 0, c.oy, c.ox, c.spare, c.fused, 0, 0, c.env, 0, c.form)
    return Dense("ctfwd", c.n, c.h, c.w, c.k, c.m, c.m // 4, c.oy, c.ox, c.spare, 0, 0, 0, c.env, 0, c.form)


def wg_geometry(c: Wg):
    """(a Buf, b Buf, stride, ty, tx)."""
    a = Buf(c.n, c.h, c.w, c.m)
    if c.taps == 9:
        return a, Buf(c.n, c.h, c.w, c.b_tot), 1, [t // 3 - 1 for t in range(9)], [t % 3 - 1 for t in range(9)]
    if c.taps == 1:
        return a, Buf(c.n, c.h, c.w, c.b_tot), 1, [0], [0]
    bh, bw = (2 * c.h - 1, 2 * c.w - 1) if c.crop else (2 * c.h + c.oy, 2 * c.w + c.ox)
    return a, Buf(c.n, bh, bw, c.b_tot), 2, [c.oy, c.oy, c.oy + 1, c.oy + 1], [c.ox, c.ox + 1, c.ox, c.ox + 1]


# ------------------------------------------------------------------------------------------------------------------ form_of
def dense_runs_ct(c: Dense, cus: int = CUS):
    """What conv_dense_impl does with a dense case: "ct" (the large-tile kernel), "general" or "refused"."""
    env = env_of(c)
    taps, stride = (4, 2) if c.kind == "ctdx" else (1, 1)
    if c.kind != "1x1bnrelu" and ctgemm_shape(c.n, c.h, c.w, c.k, c.m, taps, stride, c.cs, env, cus):
        in_, out, ty, tx = dense_geometry(c)
        if ctgemm_operands(in_, out, Buf(c.n, c.h, c.w, c.m) if c.fused else None, taps, ty, tx, c.h, c.w):
            return "ct"
        if c.fused:
            return "refused"
    return "general"


def form_of(c, cus: int = CUS):
    """The kernel instantiation and tile a case runs, from the restated planners alone."""
    env = env_of(c)
    if isinstance(c, Conv3):
        p = make_plan(c.h, c.w, c.m, env)
        return ("conv3x3", p.wide, p.TW, conv_buf(c.h, c.w, c.in_tot, c.m, c.k, env), c.ep)
    if isinstance(c, Ct):
        d = ct_as_dense(c)
        if dense_runs_ct(d, cus) != "ct":
            return form_of(d, cus)
        return ("ct", c.dx, ct_plan(c.n * c.h * c.w, c.m, bool(c.dx), env, cus).BM, bool(c.fused))
    if isinstance(c, Dense):
        how = dense_runs_ct(c, cus)
        if how == "refused":
            return ("refused",)
        if how == "ct":
            return ("ct", int(c.kind == "ctdx"), ct_plan(c.n * c.h * c.w, c.m, c.kind == "ctdx", env, cus).BM, bool(c.fused))
        p = make_plan(c.h, c.w, c.m, env)
        taps, stride = (4, 2) if c.kind == "ctdx" else (1, 1)
        ep = {"1x1": "plain", "1x1bnrelu": "bnrelu", "ctfwd": "scatter", "ctdx": "bnbwd" if c.fused else "plain"}[c.kind]
        return ("dense", p.wide, p.TW, taps, stride, ep)
    if isinstance(c, Wg):
        a, b, stride, ty, tx = wg_geometry(c)
        if wgrad_big(a, b, c.m, c.ncols, c.taps, stride, ty, tx, env, cus):
            return ("wgrad_big", make_bigplan(c.taps, c.n, c.h, c.w, c.m, c.ncols, env, cus).BM)
        p = make_wplan(c.taps == 9, c.taps, c.n, c.h, c.w, c.m, c.ncols, env)
        return ("wgrad", 1 if c.taps == 9 else 0, c.taps, p.wide, p.TW)
    raise TypeError(c)
