"""conv3x3_w2d_strips_kernel (the band-major flat tile list of the deep levels, gsd_conv3x3_w2d_strips.hip) against the rectangular
form it replaces and against fp64, at the smallest shapes that take every path of the listing.

GSD_W2D_STRIPS = 1 (wherever the list is admitted) is compared with GSD_W2D_STRIPS = 0 (never) on the same operands; which kernel ran
is read from the launch line (GSD_W2D_TRACE).  A tile keeps its anchor, its window and its products, so

  * the outputs are torch.equal to the rectangular form's, and within the project's 1e-5 relative L1 of tests/fp64_ref.py;
  * the partial rows are the rectangular form's, bit for bit (the strips form leaves per-tile sums in the lent workspace and a second
    kernel adds them in the rectangles' rows and lane order; the rows start as NaN here), so batch statistics and a train step do not
    depend on which form ran; reduced, they meet the tolerances tests/test_gpu_ops.py holds sums and sums of squares to;
  * a second run gives the same bits, partial rows included;
  * without workspace a launch with partial rows keeps the rectangles, one without them takes the list.

Input channels 8 (two chunks: the shortest unrolled loop) and 12 (an odd chunk count); output channels 64 and 72 (a channel tail).

  (5, 20, 26)   forward with statistics: 14 tiles a band, groups span two bands and two images, the last block is part empty
  (3, 40, 53)   dX of 128 channels into two destinations of 64, the second cropped to 52 columns as a decoder's up-sampled half is
                at an odd width; statistics of what each stored
  (5, 20, 26)   dX with the fused BatchNorm-backward epilogue: dz and both partial sums
  (3, 40, 53)   the same through the unmasked (interior) epilogue
  (2, 7, 13)    partial tiles at the right and bottom edges, one block
  (33, 4, 8)    four tiles a band: refused, the rectangles run and the result is still right
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fp64_ref as R
from conftest import rel_l1
from test_gpu_fp64_bounds import sums
from test_gpu_layer_shapes import gsd, layout  # noqa: F401  (gsd: the module fixture)
from test_gpu_tile_forms_fp64 import NAN, Out, Scratch, _r4, _r64, gen, launch_conv, randn, source, uniform, vec

pytestmark = pytest.mark.gpu

CHANNELS = [(8, 64), (12, 72), (8, 72), (12, 64)]
IDS = [f"k{k}-m{m}" for k, m in CHANNELS]


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a fault in an earlier launch: the context is gone, launch nothing more
        pytest.exit(f"the GPU context is in error ({e}); stopping", returncode=3)
    for k in ("GSD_W2D_TW", "GSD_W2D_SPLIT", "GSD_W2D_X4", "GSD_W2D_U4", "GSD_CONV_W2D", "GSD_W2D_STRIPS", "GSD_W2D_MGROUP", "GSD_W2D_PGROUP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GSD_W2D_TRACE", "1")
    monkeypatch.setenv("GSD_W2D_SPLIT", "0")          # the workspace these launches get is for the strip statistics, not K slabs


def lent(gsd, n, h, w, k, m):
    """The workspace the strips form asks for as the switch stands (none with the switch at 0), with sentinels behind it."""
    return Scratch(gsd.lib.gsd_conv3x3_w2d_strips_scratch(n, h, w, k, m), fill=NAN)


def ran_strips(capfd):
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("w2d ")]
    assert lines, "no w2d launch line on stderr"
    return lines[-1].startswith("w2d strips "), lines[-1]


def both_paths(monkeypatch, capfd, launch, expect_strips=True):
    """launch() -> list of tensors the launch wrote.  Runs it with the switch at 0, at 1 and at 1 again."""
    got = {}
    for tag, sw in (("rect", "0"), ("strips", "1"), ("again", "1")):
        monkeypatch.setenv("GSD_W2D_STRIPS", sw)
        capfd.readouterr()
        got[tag] = launch()
        torch.cuda.synchronize()
        strips, line = ran_strips(capfd)
        assert strips == (sw == "1" and expect_strips), line
    for a, b in zip(got["strips"], got["again"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs of the strips form differ in their bits"
    return got


def conv_case(gsd, monkeypatch, capfd, n, h, w, k, m, mode, geom=None, split=None, expect_strips=True):
    """mode 8: forward k -> m; 9: dX k -> m (weights laid out for the transposed operator)."""
    g = gen(n, h, w, k, m, mode)
    x = source(g, (n, k, h, w), pitch=_r4(w))
    wd = randn(g, m, k, 3, 3, scale=1.0 / (9 * k) ** 0.5) if mode == 8 else randn(g, k, m, 3, 3, scale=1.0 / (9 * k) ** 0.5)
    wl = layout(gsd, mode, wd, m, k) if mode == 8 else layout(gsd, 9, wd, k, m)
    geom = geom or [(0, 0, h, w)]
    split = split or [m]
    rows = gsd.lib.gsd_conv3x3_w2d_partial_rows(n, h, w, m)
    ref, _ = R.conv3x3_fwd(x.double(), wd.double()) if mode == 8 else R.conv3x3_dx(x.double(), wd.double())
    keep = []

    def launch():
        outs = [Out((n, ch, uh, uw), _r4(uw) + 4) for (_, _, uh, uw), ch in zip(geom, split)]
        part = Scratch(rows * 2 * _r64(m), fill=NAN)
        dsts = [o.dst(gsd, off=(oh, ow)) for o, (oh, ow, _, _) in zip(outs, geom)]
        ws = lent(gsd, n, h, w, k, m)
        gsd.check(gsd.lib.gsd_conv3x3_w2d_ws(gsd.src_array([gsd.make_src(x)]), 1, wl.data_ptr(), k, m, gsd.dst_array(dsts), len(dsts),
                                             part.ptr(), ws.ptr(), ws.need, n, h, w, gsd.stream_ptr()), "gsd_conv3x3_w2d_ws")
        torch.cuda.synchronize()
        for o in outs:
            o.check("destination")
        part.check("partials")
        ws.check("workspace")
        s1, s2 = sums(gsd, part.flat, rows, _r64(m), m)
        keep.append(part)
        return [o.t for o in outs] + [s1, s2, part.flat[:part.need]]

    got = both_paths(monkeypatch, capfd, launch, expect_strips)
    nd = len(geom)
    assert torch.equal(got["rect"][nd + 2].view(torch.int32), got["strips"][nd + 2].view(torch.int32)), "partial rows differ from the rectangular form's"
    lo = 0
    for i, ((oh, ow, uh, uw), ch) in enumerate(zip(geom, split)):
        a, b = got["rect"][i], got["strips"][i]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
            f"destination {i}: {int((a.view(torch.int32) != b.view(torch.int32)).sum())} of {a.numel()} outputs differ from the rectangular form's"
        r_ = ref[:, lo:lo + ch, oh:oh + uh, ow:ow + uw]
        err = rel_l1(b.cpu().numpy(), r_.cpu().numpy())
        print(f"destination {i}: relative L1 against fp64 {err:.3g}")
        assert err < 1e-5, err
        for tag in ("rect", "strips"):
            s1, s2 = got[tag][nd], got[tag][nd + 1]
            y64 = got[tag][i].double()
            np.testing.assert_allclose(s1[lo:lo + ch].cpu().numpy(), y64.sum((0, 2, 3)).cpu().numpy(), rtol=1e-4, atol=1e-3, err_msg=tag)
            np.testing.assert_allclose(s2[lo:lo + ch].cpu().numpy(), (y64 * y64).sum((0, 2, 3)).cpu().numpy(), rtol=1e-4, atol=1e-3,
                                       err_msg=tag)
        lo += ch


@pytest.mark.parametrize("k,m", CHANNELS, ids=IDS)
def test_forward_with_statistics_two_bands_two_images(gsd, monkeypatch, capfd, k, m):
    conv_case(gsd, monkeypatch, capfd, 5, 20, 26, k, m, 8)


@pytest.mark.parametrize("k", [8, 12])
def test_dx_into_two_destinations_the_second_cropped(gsd, monkeypatch, capfd, k):
    conv_case(gsd, monkeypatch, capfd, 3, 40, 53, k, 128, 9, geom=[(0, 0, 40, 53), (0, 0, 40, 52)], split=[64, 64])


@pytest.mark.parametrize("k,m", CHANNELS, ids=IDS)
def test_partial_tiles_on_both_edges(gsd, monkeypatch, capfd, k, m):
    conv_case(gsd, monkeypatch, capfd, 2, 7, 13, k, m, 8)


@pytest.mark.parametrize("k,m", CHANNELS, ids=IDS)
def test_four_tiles_a_band_falls_back(gsd, monkeypatch, capfd, k, m):
    conv_case(gsd, monkeypatch, capfd, 33, 4, 8, k, m, 8, expect_strips=False)


@pytest.mark.parametrize("n,h,w,k,m", [(5, 20, 26, k, m) for k, m in CHANNELS] + [(3, 40, 53, 8, 64), (3, 40, 53, 12, 72)],
                         ids=[f"20x26-{i}" for i in IDS] + ["40x53-k8-m64", "40x53-k12-m72"])
def test_fused_bn_backward_epilogue(gsd, monkeypatch, capfd, n, h, w, k, m):
    """gsd_conv3x3_w2d_dgrad_bnrelu: dX of k channels into dz of m, masked by relu'(bn(raw)), with sum dz and sum dz * xhat.
    At 20 x 26 every group holds a column that is cut by the right edge (the masked epilogue); at 40 x 53 the groups of columns
    0 .. 7 are interior and store through the unmasked path, whose lane offsets carry the image."""
    L, st = gsd.lib, gsd.stream_ptr()
    g = gen(n, h, w, k, m, 11)
    dy = source(g, (n, k, h, w), pitch=_r4(w))
    p = _r4(w) + 4
    raw = source(g, (n, m, h, w), pitch=p)               # raw shares dz's strides
    sc, sh = uniform(g, 0.5, 1.5, m), randn(g, m, scale=0.3)
    mean, invstd = randn(g, m, scale=0.3), uniform(g, 0.5, 2.0, m)
    wd = randn(g, k, m, 3, 3, scale=1.0 / (9 * k) ** 0.5)
    wl = layout(gsd, 9, wd, k, m)
    rows = L.gsd_conv3x3_w2d_partial_rows(n, h, w, m)
    keep = []

    def launch():
        dz = Out((n, m, h, w), p)
        part = Scratch(rows * 2 * _r64(m), fill=NAN)
        s, d = gsd.make_src(dy), dz.dst(gsd)
        ws = lent(gsd, n, h, w, k, m)
        gsd.check(L.gsd_conv3x3_w2d_dgrad_bnrelu_ws(C.byref(s), wl.data_ptr(), k, m, C.byref(d), raw.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                                    mean.data_ptr(), invstd.data_ptr(), part.ptr(), ws.ptr(), ws.need, n, h, w, st),
                  "gsd_conv3x3_w2d_dgrad_bnrelu_ws")
        torch.cuda.synchronize()
        dz.check("dz")
        part.check("partials")
        ws.check("workspace")
        q1, q2 = sums(gsd, part.flat, rows, _r64(m), m)
        keep.append(part)
        return [dz.t, q1, q2, part.flat[:part.need]]

    got = both_paths(monkeypatch, capfd, launch)
    a, b = got["rect"][0], got["strips"][0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "dz differs from the rectangular form's"
    assert torch.equal(got["rect"][3].view(torch.int32), got["strips"][3].view(torch.int32)), "partial rows differ from the rectangular form's"
    ref, _ = R.conv3x3_dx(dy.double(), wd.double())
    mask = R.bnrelu_mask(raw, sc, sh)
    ref = ref * mask
    err = rel_l1(b.cpu().numpy(), ref.cpu().numpy())
    print(f"dz: relative L1 against fp64 {err:.3g}")
    assert err < 1e-5, err
    assert bool((b[~mask] == 0).all()), "dz is exactly 0 where the mask is off"
    xhat = (raw.double() - vec(mean)) * vec(invstd)
    z64 = b.double()
    for tag in ("rect", "strips"):
        np.testing.assert_allclose(got[tag][1].cpu().numpy(), z64.sum((0, 2, 3)).cpu().numpy(), rtol=2e-4, atol=2e-3, err_msg=tag)
        np.testing.assert_allclose(got[tag][2].cpu().numpy(), (z64 * xhat).sum((0, 2, 3)).cpu().numpy(), rtol=2e-4, atol=2e-3, err_msg=tag)


def test_without_workspace_only_launches_without_partial_rows_take_the_list(gsd, monkeypatch, capfd):
    n, h, w, k, m = 5, 20, 26, 8, 64
    g = gen(n, h, w, k, m, 12)
    x = source(g, (n, k, h, w), pitch=_r4(w))
    wd = randn(g, m, k, 3, 3, scale=1.0 / (9 * k) ** 0.5)
    wl = layout(gsd, 8, wd, m, k)
    rows = gsd.lib.gsd_conv3x3_w2d_partial_rows(n, h, w, m)
    monkeypatch.setenv("GSD_W2D_STRIPS", "1")
    ys = []
    for with_rows, want in ((True, False), (False, True)):
        y = Out((n, m, h, w), _r4(w) + 4)
        part = Scratch(rows * 2 * _r64(m), fill=NAN)
        capfd.readouterr()
        launch_conv(gsd, "w2d", gsd.src_array([gsd.make_src(x)]), 1, wl, k, m, [y.dst(gsd)], part.ptr() if with_rows else None, n, h, w, False)
        torch.cuda.synchronize()
        strips, line = ran_strips(capfd)
        assert strips == want, line
        y.check("destination")
        part.check("partials")
        ys.append(y.t)
    assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32))
