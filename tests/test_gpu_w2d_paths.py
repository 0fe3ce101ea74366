"""The two epilogue paths and the scalar-base fill addressing of gsd_conv3x3_w2d, at the smallest shapes that reach them.

The kernel's epilogue has an unmasked path for interior waves (every lane's 2 x 4 tile inside the image and inside the crop of the
one destination that holds the wave's 32 channels: unconditional 16-byte stores at a scalar plane base) and a masked path for
everything else; its fills address a wave-uniform base 16 bytes in front of the channel plane plus an unsigned 32-bit lane offset.
Shapes (plan_w2d picks 8 x 32 tiles, TH shrunk to 6 at H = 9 / 10, for all of them):

  * forward at W = 32 and W = 30 on the same data (the wide run's two extra columns activate to 0): at W = 32 the first pixel group
    of every block is interior, at W = 30 no wave is -- every pixel both launches store must be BIT-equal; H = 9 puts a half-valid
    tile row under the second pixel group; Cout = 72 adds a second m-block with a channel tail (masked) beside a full one;
  * dX with the decoder's two destinations (the second offset by one row and column and smaller, both pitched wider than W) from
    the row-pitched plain gradient (16-byte aligned pieces) at 24 x 96: the middle block of the 3 x 3 is interior for both;
  * the fused BatchNorm-backward epilogue with its two sums, with and without a channel tail;
  * one K-slab launch and its reducer (GSD_W2D_SPLIT=2), which shares the epilogue;
  * a concat source whose second segment starts at column 1 and is 29 wide: its 16-byte pieces straddle both edges, the first of
    row 0 starts one float in front of the plane.

Every case: each stored element within TAU_WINO * sum |a||b| of the fp64 tap reference, the statistics rows against fp64 sums of
what was stored, and every float outside the H x W x C regions (guard bands, pad columns between rows, neighbouring channels)
still the sentinel -- what the unmasked stores must not touch.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import fp64_ref as R
from test_gpu_fp64_bounds import sums
from test_gpu_layer_shapes import gsd, layout  # noqa: F401  (gsd: the module fixture)
from test_gpu_tile_forms_fp64 import (NAN, Out, Scratch, _r4, _r64, check_stats, field, gen, launch_conv, randn, source, trace_line,
                                      uniform, vec)

pytestmark = pytest.mark.gpu

N = 2
KEY = "w2d-paths"


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a fault in an earlier launch: the context is gone, launch nothing more
        pytest.exit(f"the GPU context is in error ({e}); stopping", returncode=3)
    for k in ("GSD_W2D_TW", "GSD_W2D_SPLIT", "GSD_W2D_X4", "GSD_W2D_U4", "GSD_CONV_W2D"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GSD_W2D_TRACE", "1")


def _forward(gsd, capfd, raw, sc, sh, wd, co, h, w, tag, dead_column=False):
    """One forward launch from a deferred BatchNorm + ReLU source with slack; returns (output, statistics rows).

    dead_column: the source's last two columns activate to 0, so every product of the LAST output column is 0 and so is its
    sum |a||b|.  No Winograd kernel meets a bound of 0 there: the F(2x4,3x3) tile that holds the column (output columns w-4 ..
    w-1, input columns w-5 .. w) forms all four of its output columns from the same 6 x 4 transformed products, in which the
    live input columns cancel only up to rounding.  That residue scales with the tile's products, so the column is held to tau
    times the sum of cond over the four output columns of its tile in the same row -- a bound from the tile's own taps, a little
    over twice an interior pixel's, that a read of anything but zeros from the dead columns or the padding overshoots.  Every other
    column keeps its own sum |a||b|."""
    ci = raw.shape[1]
    src = gsd.src_array([gsd.make_src(raw, sc, sh, relu=True, slack=gsd.SLACK)])
    rows = gsd.lib.gsd_conv3x3_w2d_partial_rows(N, h, w, co)
    y = Out((N, co, h, w), w + 1)
    part = Scratch(rows * 2 * _r64(co))
    capfd.readouterr()
    launch_conv(gsd, "w2d", src, 1, layout(gsd, 8, wd, co, ci), ci, co, [y.dst(gsd)], part.ptr(), N, h, w, False)
    torch.cuda.synchronize()
    line, _ = trace_line(capfd, "w2d")
    assert field(line, "tile") == "6x32" and int(field(line, "u4")) == 1 and int(field(line, "plain")) == 0, line
    ref, cond = R.conv3x3_fwd(R.deferred_act(raw, sc, sh), wd.double())
    bound = cond
    if dead_column:
        assert w % 4 == 0 and not bool(cond[..., w - 1].any()) and bool((cond[..., :w - 1] > 0).all())
        bound = cond.clone()
        bound[..., w - 1] = cond[..., w - 4:].sum(-1)
    R.check_bound(y.t, ref, bound, R.TAU_WINO, f"{tag} forward", image=N - 1, key=f"{KEY}:{tag}")
    y.check(f"{tag} forward")
    part.check(f"{tag} partials")
    check_stats(gsd, part, rows, co, [(0, y.t)], [(0, cond)], f"{tag} forward", f"{KEY}:stats:{tag}")
    return y, rows


@pytest.mark.parametrize("h,co", [(10, 64), (9, 64), (10, 72)], ids=["h10-m64", "h9-m64", "h10-m72"])
def test_forward_interior_and_masked_paths_agree_bit_for_bit(gsd, capfd, h, co):
    ci, w = 8, 32
    g = gen(h, co, 1)
    sc, sh = uniform(g, 0.5, 1.5, ci), randn(g, ci, scale=0.3)
    wd = randn(g, co, ci, 3, 3, scale=1.0 / (9 * ci) ** 0.5)
    wide = source(g, (N, ci, h, w))
    wide[..., w - 2:] = ((-1.0 - sh) / sc).view(1, ci, 1, 1)           # fmaf(raw, scale, shift) ~ -1: activates to 0
    assert bool((R.deferred_act(wide, sc, sh)[..., w - 2:] == 0).all())
    narrow = source(g, (N, ci, h, w - 2))
    narrow.copy_(wide[..., :w - 2])
    y_wide, rows_wide = _forward(gsd, capfd, wide, sc, sh, wd, co, h, w, f"h{h}-m{co}-w{w}", dead_column=True)
    y_narrow, rows_narrow = _forward(gsd, capfd, narrow, sc, sh, wd, co, h, w - 2, f"h{h}-m{co}-w{w - 2}")
    assert rows_wide == rows_narrow, "both widths must run the same tile grid"
    a, b = y_wide.t[..., :w - 2].contiguous().view(torch.int32), y_narrow.t.contiguous().view(torch.int32)
    bad = a != b
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} pixels differ in their bits between the interior and the masked " \
                                f"epilogue, first at {tuple(int(i) for i in bad.nonzero()[0])}"


def test_dx_two_cropped_destinations_from_the_pitched_gradient(gsd, capfd):
    """The decoder's dX: destination 0 takes C0 channels of the whole grid, destination 1 the rest, cropped by one row and column
    at the top left and two at the bottom right; the statistics are those of what each stored."""
    h, w, kd, c0, c1 = 24, 96, 8, 64, 64
    ci = c0 + c1
    g = gen(h, w, kd, ci, 2)
    wd = randn(g, kd, ci, 3, 3, scale=1.0 / (9 * kd) ** 0.5)
    dy = source(g, (N, kd, h, w), pitch=_r4(w))
    geom = [(0, 0, h, w), (1, 1, h - 2, w - 2)]
    outs = [Out((N, ch, uh, uw), uw + 1) for (_, _, uh, uw), ch in zip(geom, (c0, c1))]
    rows = gsd.lib.gsd_conv3x3_w2d_partial_rows(N, h, w, ci)
    part = Scratch(rows * 2 * _r64(ci))
    dsts = [o.dst(gsd, off=(oh, ow)) for o, (oh, ow, _, _) in zip(outs, geom)]
    capfd.readouterr()
    launch_conv(gsd, "w2d", gsd.src_array([gsd.make_src(dy)]), 1, layout(gsd, 9, wd, kd, ci), kd, ci, dsts, part.ptr(), N, h, w, False)
    torch.cuda.synchronize()
    line, _ = trace_line(capfd, "w2d")
    assert field(line, "tile") == "8x32" and int(field(line, "x4")) == 1 and int(field(line, "ndst")) == 2, line
    ref, cond = R.conv3x3_dx(dy.double(), wd.double())
    stored, conds, lo = [], [], 0
    for o, (oh, ow, uh, uw) in zip(outs, geom):
        ch = o.t.shape[1]
        r_, c_ = ref[:, lo:lo + ch, oh:oh + uh, ow:ow + uw], cond[:, lo:lo + ch, oh:oh + uh, ow:ow + uw]
        R.check_bound(o.t, r_, c_, R.TAU_WINO, f"dX destination at ({oh},{ow})", image=N - 1, key=f"{KEY}:dx2")
        o.check(f"dX destination at ({oh},{ow})")
        stored.append((lo, o.t))
        conds.append((lo, c_))
        lo += ch
    part.check("dX partials")
    check_stats(gsd, part, rows, ci, stored, conds, "dX two destinations", f"{KEY}:stats:dx2")


@pytest.mark.parametrize("ci", [64, 72])
def test_fused_bn_backward_epilogue_with_partial_sums(gsd, ci):
    """gsd_conv3x3_w2d_dgrad_bnrelu at 10 x 32: the first pixel group of each block stores unmasked (all of it at ci = 64, the
    first m-block at ci = 72), the second and the channel tail masked."""
    h, w, co = 10, 32, 8
    L, st = gsd.lib, gsd.stream_ptr()
    g = gen(h, w, ci, co, 3)
    tag = f"fused-m{ci}"
    dy = source(g, (N, co, h, w), pitch=_r4(w))
    raw = source(g, (N, ci, h, w), pitch=w + 1)          # raw shares dz's strides: both rows pitched, one pad column between them
    sc, sh = uniform(g, 0.5, 1.5, ci), randn(g, ci, scale=0.3)
    mean, invstd = randn(g, ci, scale=0.3), uniform(g, 0.5, 2.0, ci)
    wd = randn(g, co, ci, 3, 3, scale=1.0 / (9 * co) ** 0.5)
    rows = L.gsd_conv3x3_w2d_partial_rows(N, h, w, ci)
    part = Scratch(rows * 2 * _r64(ci))
    dz = Out((N, ci, h, w), w + 1)
    s, d = gsd.make_src(dy), dz.dst(gsd)
    gsd.check(L.gsd_conv3x3_w2d_dgrad_bnrelu(C.byref(s), layout(gsd, 9, wd, co, ci).data_ptr(), co, ci, C.byref(d), raw.data_ptr(),
                                             sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(), part.ptr(), N, h, w, st),
              "gsd_conv3x3_w2d_dgrad_bnrelu")
    torch.cuda.synchronize()
    ref, cond = R.conv3x3_dx(dy.double(), wd.double())
    m = R.bnrelu_mask(raw, sc, sh)
    ref, cond = ref * m, cond * m
    R.check_bound(dz.t, ref, cond, R.TAU_WINO, f"{tag} dz", image=N - 1, key=f"{KEY}:{tag}")
    assert bool((dz.t[~m] == 0).all()), "dz is exactly 0 where the mask is off"
    dz.check(f"{tag} dz")
    part.check(f"{tag} partials")
    q1, q2 = sums(gsd, part.flat, rows, _r64(ci), ci)
    xhat = (raw.double() - vec(mean)) * vec(invstd)
    z64 = dz.t.double()
    R.check_sums(q1, z64.sum((0, 2, 3)), cond.sum((0, 2, 3)), R.TAU_STATS, f"{tag} sum dz", key=f"{KEY}:stats:{tag}")
    R.check_sums(q2, (z64 * xhat).sum((0, 2, 3)), (cond * xhat.abs()).sum((0, 2, 3)), R.TAU_STATS, f"{tag} sum dz*xhat",
                 key=f"{KEY}:stats:{tag}")


def test_k_slab_launch_and_reducer(gsd, monkeypatch, capfd):
    """Two K slabs of 8 chunks each and the reducer that adds them and runs the shared epilogue (interior and masked waves)."""
    monkeypatch.setenv("GSD_W2D_SPLIT", "2")
    h, w, ci, co = 10, 32, 64, 64
    g = gen(h, w, ci, co, 4)
    x = source(g, (N, ci, h, w))
    wd = randn(g, co, ci, 3, 3, scale=1.0 / (9 * ci) ** 0.5)
    rows = gsd.lib.gsd_conv3x3_w2d_partial_rows(N, h, w, co)
    y = Out((N, co, h, w), w + 1)
    part = Scratch(rows * 2 * _r64(co))
    capfd.readouterr()
    ws = launch_conv(gsd, "w2d", gsd.src_array([gsd.make_src(x, slack=gsd.SLACK)]), 1, layout(gsd, 8, wd, co, ci), ci, co, [y.dst(gsd)],
                     part.ptr(), N, h, w, True)
    torch.cuda.synchronize()
    line, _ = trace_line(capfd, "w2d")
    assert int(field(line, "slabs")) == 2 and int(field(line, "x4")) == 1, line      # (a plain source with 16-byte rows: the X4 form)
    ref, cond = R.conv3x3_fwd(x.double(), wd.double())
    R.check_bound(y.t, ref, cond, R.TAU_WINO, "K-slab forward", image=N - 1, key=f"{KEY}:slabs")
    y.check("K-slab forward")
    part.check("K-slab partials")
    ws.check("K-slab scratch")
    check_stats(gsd, part, rows, co, [(0, y.t)], [(0, cond)], "K-slab forward", f"{KEY}:stats:slabs")


def test_concat_source_whose_pieces_straddle_both_edges(gsd, capfd):
    """Two source segments: a deferred BatchNorm + ReLU one on the grid and a plain one at column offset 1, 29 wide.  On the
    16-byte piece grid (image columns 4k - 4) the second segment's first piece of a row covers its columns -1 .. 2 -- in row 0 it
    starts one float in FRONT of the channel plane -- and its last one runs past the right edge."""
    h, w, c0, c1, co = 10, 32, 8, 8, 64
    oh, ow, uh, uw = 0, 1, h - 1, w - 3
    g = gen(h, w, c0, c1, 5)
    sc, sh = uniform(g, 0.5, 1.5, c0), randn(g, c0, scale=0.3)
    raw0 = source(g, (N, c0, h, w))
    up = source(g, (N, c1, uh, uw))
    segs = [gsd.make_src(raw0, sc, sh, relu=True, slack=gsd.SLACK), gsd.make_src(up, off=(oh, ow), slack=gsd.SLACK)]
    act = torch.cat([R.deferred_act(raw0, sc, sh), F.pad(up.double(), [ow, w - uw - ow, oh, h - uh - oh])], 1)
    ci = c0 + c1
    wd = randn(g, co, ci, 3, 3, scale=1.0 / (9 * ci) ** 0.5)
    rows = gsd.lib.gsd_conv3x3_w2d_partial_rows(N, h, w, co)
    y = Out((N, co, h, w), w + 1)
    part = Scratch(rows * 2 * _r64(co))
    capfd.readouterr()
    launch_conv(gsd, "w2d", gsd.src_array(segs), 2, layout(gsd, 8, wd, co, ci), ci, co, [y.dst(gsd)], part.ptr(), N, h, w, False)
    torch.cuda.synchronize()
    line, _ = trace_line(capfd, "w2d")
    assert int(field(line, "u4")) == 1 and int(field(line, "nsrc")) == 2, line
    ref, cond = R.conv3x3_fwd(act, wd.double())
    R.check_bound(y.t, ref, cond, R.TAU_WINO, "concat forward", image=N - 1, key=f"{KEY}:concat")
    y.check("concat forward")
    part.check("concat partials")
    check_stats(gsd, part, rows, co, [(0, y.t)], [(0, cond)], "concat forward", f"{KEY}:stats:concat")
    assert not bool(torch.isnan(y.t).any()), "a NaN from the slack around a segment reached an output"
