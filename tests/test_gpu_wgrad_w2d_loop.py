"""The k-step loop of the two-dimensional Winograd dW kernel (gelslim_depth_amd/csrc/gsd_wgrad_w2d.hip) at the smallest shapes at
which its bookkeeping can go wrong, through gsd_conv3x3_wgrad as the engine calls it.

What the cases reach: a block that runs 1, 2, 3 or 4 k-steps (the walk that stops at the block's last k-step, at odd and even
counts, and a block whose only k-step is a border one: GSD_WG2D_BLOCKS sets the split), every border class of a k-step in both
directions (first, last, first and last at once, last but one where a cropped second segment ends inside its window, none),
partial tiles, both block forms (Cout 64 and 128), plain and deferred sources, every k-step shape (GSD_WG2D_KX), two segments.

Reference: the direct dW in float64 on the CPU of the same activated inputs; bound 5e-5 relative L1 (the bound of
test_gpu_wgrad_w2d.py: fp32 products of O(1) values summed over at most a few thousand terms in a Winograd form whose transforms
amplify rounding by a small constant).  Two runs must agree bitwise (ordered slab reduction).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_l1

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gsd():
    from gelslim_depth_amd import _lib
    return _lib


def ceil_div(a, b):
    return -(-a // b)


def slack_dev(gsd, a):
    t = gsd.slack_empty(tuple(a.shape), "cuda")
    t.copy_(a)
    return t


def reference_dw(a, dy):
    """fp64 direct dW[co][ci][r][s] = sum_{n,h,w} dy[n,co,h,w] a[n,ci,h+r-1,w+s-1]"""
    a, dy = a.double(), dy.double()
    h, w = dy.shape[2:]
    ap = torch.nn.functional.pad(a, (1, 1, 1, 1))
    out = torch.empty(dy.shape[1], a.shape[1], 3, 3, dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            out[:, :, r, s] = torch.einsum("nohw,nihw->oi", dy, ap[:, :, r:r + h, s:s + w])
    return out.numpy()


# (n, h, w, c0, c1, co, deferred BatchNorm + ReLU on segment 0, (up_h, up_w), GSD_WG2D_KX, k-steps per block or 0: the planner's split)
CASES = [
    (1, 4, 8, 32, 0, 128, True, None, 2, 1),       # ONE 2x2 k-step in all: first and last in both directions, the block's only one
    (3, 4, 8, 64, 0, 64, False, None, 2, 3),       # one block walks three images of one k-step each (odd count)
    (3, 4, 8, 64, 0, 64, True, None, 2, 2),        # blocks of 1 and 2 k-steps
    (1, 3, 5, 32, 0, 128, False, None, 0, 0),      # partial tiles only
    (3, 3, 5, 64, 0, 64, True, None, 1, 4),        # 4x1 tiles, partial, six k-steps in blocks of three
    (1, 2, 16, 32, 0, 128, True, None, 4, 1),      # one 1x4 k-step: first and last in both directions
    (3, 2, 16, 64, 0, 64, False, None, 2, 2),      # first and last in the rows only
    (1, 8, 4, 64, 0, 64, True, None, 1, 1),        # one 4x1 k-step
    (3, 8, 4, 32, 0, 128, False, None, 2, 3),      # first and last in the columns only
    (1, 9, 21, 32, 0, 128, True, None, 2, 3),      # odd sizes with an interior k-step, three blocks of three
    (3, 9, 21, 64, 0, 64, True, None, 0, 0),
    (1, 9, 21, 64, 0, 128, False, None, 1, 4),     # twelve 4x1 k-steps in blocks of four
    (1, 9, 21, 64, 0, 64, False, None, 4, 2),
    (1, 20, 26, 32, 0, 128, True, None, 2, 4),     # twenty k-steps in blocks of four
    (1, 20, 26, 64, 0, 64, True, None, 4, 2),
    (3, 20, 26, 64, 0, 128, False, None, 0, 0),
    (1, 20, 26, 64, 0, 64, False, None, 1, 1),     # every block one k-step, interior ones among them
    (1, 20, 26, 32, 32, 128, True, (18, 25), 2, 3),   # two segments, the second cropped (pad offset (1, 0))
    (3, 9, 21, 64, 64, 64, True, (8, 20), 0, 0),      # 64 x 64 form with two segments
    (1, 9, 25, 32, 32, 128, True, (8, 24), 1, 2),     # the cropped segment ends inside the window of the last-but-one k-step column
    (1, 9, 25, 64, 64, 64, True, (8, 24), 4, 3),      # ... and of the last-but-one k-step row
]


def case_id(c):
    return f"N{c[0]}-{c[1]}x{c[2]}-C{c[3]}+{c[4]}-M{c[5]}-{'bn' if c[6] else 'plain'}-kx{c[8]}-q{c[9]}"


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_wgrad_w2d_loop_vs_fp64(gsd, monkeypatch, case):
    n, h, w, c0, c1, co, bn, up_hw, kx, per_block = case
    ci = c0 + c1
    L = gsd.lib
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + kx + per_block)
    raw0 = torch.randn((n, c0, h, w), generator=g)
    keep = [slack_dev(gsd, raw0)]
    if bn:
        sc, sh = torch.rand(c0, generator=g) + 0.5, torch.randn(c0, generator=g) * 0.3
        a = torch.relu(raw0 * sc[None, :, None, None] + sh[None, :, None, None])
        keep += [sc.cuda(), sh.cuda()]
        segs = [gsd.make_src(keep[0], keep[1], keep[2], relu=True, slack=gsd.SLACK)]
    else:
        a = raw0
        segs = [gsd.make_src(keep[0], slack=gsd.SLACK)]
    if c1:
        uh, uw = up_hw
        up = torch.randn((n, c1, uh, uw), generator=g)
        top, left = (h - uh) // 2, (w - uw) // 2
        a = torch.cat([a, torch.nn.functional.pad(up, (left, w - uw - left, top, h - uh - top))], 1)
        keep.append(slack_dev(gsd, up))
        segs.append(gsd.make_src(keep[-1], off=(top, left), slack=gsd.SLACK))
    dy = torch.randn((n, co, h, w), generator=g)
    dyb = torch.zeros((n, co, h, (w + 3) // 4 * 4), device="cuda")
    dyb[..., :w] = dy.cuda()
    dyp = dyb[..., :w]

    if kx:
        monkeypatch.setenv("GSD_WG2D_KX", str(kx))
    if per_block:
        ksteps = n * ceil_div(ceil_div(h, 2), 4 // kx) * ceil_div(ceil_div(w, 4), kx)
        bm = 128 if co >= 128 else 64
        monkeypatch.setenv("GSD_WG2D_BLOCKS", str(ceil_div(ksteps, per_block) * (co // bm) * (ci // (32 if bm == 128 else 64))))

    src, dy_src = gsd.src_array(segs), gsd.make_src(dyp)
    assert L.gsd_conv3x3_wgrad_form(src, len(segs), C.byref(dy_src), ci, co, n, h, w) == 2, "the two-dimensional form serves this call"
    need = L.gsd_conv3x3_wgrad_workspace(n, h, w, ci, co)
    got = []
    for _ in range(2):
        ws = torch.zeros(max(need, 64), device="cuda")
        dw = torch.full((co, ci, 3, 3), float("nan"), device="cuda")
        gsd.check(L.gsd_conv3x3_wgrad(src, len(segs), C.byref(dy_src), ci, co, dw.data_ptr(), ws.data_ptr(), ws.numel(), n, h, w,
                                      gsd.stream_ptr()), "wgrad")
        torch.cuda.synchronize()
        got.append(dw.cpu().numpy())
    ref = reference_dw(a, dy)
    err = rel_l1(got[0], ref)
    print(case_id(case), "rel L1 %.3g" % err)
    assert np.isfinite(got[0]).all()
    assert err < 5e-5
    if c1:
        assert rel_l1(got[0][:, c0:], ref[:, c0:]) < 5e-5
    assert np.array_equal(got[0], got[1]), "two runs are bitwise equal"
