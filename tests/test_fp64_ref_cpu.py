"""tests/fp64_ref.py on the CPU at small shapes: its tap-matmul references equal torch's own float64 convolutions and autograd,
cond bounds |ref| (and equals it for non-negative operands), and check_bound at the module's taus accepts an fp32 rounding of
the exact result while rejecting the small, local mistakes the GPU kernel tests exist to catch: one product missing at a corner,
one 2x4 Winograd tile off by 1e-4, two images swapped, one column's halo read one column too far, one image row missing from
dW, one element never written."""
import pytest
import torch
import torch.nn.functional as F

import fp64_ref as R

G = torch.Generator().manual_seed(7)


def rn(*shape):
    return torch.randn(shape, generator=G, dtype=torch.float64)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def f32(t):
    return t.float().double()


@pytest.mark.parametrize("segs,crop", [(1, False), (2, True)])
def test_conv3x3_refs_equal_torch(segs, crop):
    """Forward, dX and dW against F.conv2d and its autograd, one source segment or the decoder's two (skip | F.pad(up) at an
    odd offset) with dX cropped back to the up-sampled tensor."""
    n, h, w, c0, co = 3, 9, 11, 5, 6
    a0 = rn(n, c0, h, w)
    up = rn(n, 4, 6, 8) if segs == 2 else None
    if up is not None:
        a, (top, left) = R.decoder_src(a0, up, h, w)
        assert (top, left) == (1, 1)
        assert torch.equal(a[:, c0:, top:top + 6, left:left + 8], up) and float(a[:, c0:, 0].abs().sum()) == 0
    else:
        a = a0
    wt = rn(co, a.shape[1], 3, 3)
    dy = rn(n, co, h, w)
    x = a.clone().requires_grad_(True)
    wv = wt.clone().requires_grad_(True)
    y = F.conv2d(x, wv, padding=1)
    y.backward(dy)
    ref, cond = R.conv3x3_fwd(a, wt)
    assert rel(ref, y.detach()) < 1e-12
    dx, _ = R.conv3x3_dx(dy, wt)
    assert rel(dx, x.grad) < 1e-12
    if crop:
        assert rel(dx[:, c0:, 1:7, 1:9], x.grad[:, c0:, 1:7, 1:9]) < 1e-12
    dw, _ = R.conv3x3_dw(a, dy)
    assert rel(dw, wv.grad) < 1e-12
    rows = R.conv3x3_dw_rows(a[1:2], dy[1:2])
    assert rel(rows.sum(0), R.conv3x3_dw(a[1:2], dy[1:2])[0]) < 1e-12


def test_convT_and_1x1_refs_equal_torch():
    n, ci, co, h, w = 2, 6, 3, 5, 7
    x, wt, b = rn(n, ci, h, w), rn(ci, co, 2, 2), rn(co)
    dy = rn(n, co, 2 * h, 2 * w)
    xv, wv, bv = (t.clone().requires_grad_(True) for t in (x, wt, b))
    y = F.conv_transpose2d(xv, wv, bv, stride=2)
    y.backward(dy)
    assert rel(R.convT_fwd(x, wt, b)[0], y.detach()) < 1e-12
    assert rel(R.convT_dx(dy, wt)[0], xv.grad) < 1e-12
    dw, _, db, _ = R.convT_dw(x, dy)
    assert rel(dw, wv.grad) < 1e-12 and rel(db, bv.grad) < 1e-12
    # output conv + MSE loss
    a, w1, b1, t = rn(n, 4, h, w).clamp_min(0), rn(1, 4), rn(1), rn(n, 1, h, w)
    av, wv1, bv1 = (v.clone().requires_grad_(True) for v in (a, w1, b1))
    o = F.conv2d(av, wv1.view(1, 4, 1, 1), bv1)
    o.retain_grad()
    F.mse_loss(o, t).backward()
    assert rel(R.conv1x1_fwd(a, w1, b1)[0], o.detach()) < 1e-12
    g, _ = R.mse_grad(o.detach(), t, o.numel())
    assert rel(g, o.grad) < 1e-12
    assert rel(R.conv1x1_dx(g, w1)[0], av.grad) < 1e-12
    dw1, _, db1, _ = R.conv1x1_dw(a, g)
    assert rel(dw1, wv1.grad) < 1e-12 and rel(db1, bv1.grad) < 1e-12


def test_cond_bounds_ref():
    a, wt, dy = rn(2, 4, 6, 9), rn(5, 4, 3, 3), rn(2, 5, 6, 9)
    for ref, cond in (R.conv3x3_fwd(a, wt), R.conv3x3_dx(dy, wt), R.conv3x3_dw(a, dy), R.convT_fwd(a, rn(4, 3, 2, 2), rn(3)),
                      R.convT_dx(rn(2, 3, 12, 18), rn(4, 3, 2, 2))):
        assert bool((cond >= ref.abs()).all())
    ap, wp, dp = a.abs(), wt.abs(), dy.abs()
    for ref, cond in (R.conv3x3_fwd(ap, wp), R.conv3x3_dx(dp, wp), R.conv3x3_dw(ap, dp)):
        assert torch.allclose(ref, cond, rtol=1e-14, atol=0)


def test_deferred_operands_are_the_kernels_fp32_values():
    raw, sc, sh = torch.randn(2, 3, 4, 5, generator=G), torch.rand(3, generator=G) + 0.5, torch.randn(3, generator=G)
    a = R.deferred_act(raw, sc, sh)
    assert a.dtype == torch.float64 and torch.equal(a, a.float().double()) and bool((a >= 0).all())
    m = R.bnrelu_mask(raw, sc, sh)
    assert torch.equal(m, a > 0)


# ---- sensitivity of check_bound at the module's taus: a fp32-rounded exact result passes, each local mistake fails
N, CI, CO, H, W = 3, 16, 8, 8, 12


@pytest.fixture(scope="module")
def conv():
    g = torch.Generator().manual_seed(11)
    a = torch.randn((N, CI, H, W), generator=g, dtype=torch.float64)
    wt = torch.randn((CO, CI, 3, 3), generator=g, dtype=torch.float64) / (3 * CI ** 0.5)
    dy = torch.randn((N, CO, H, W), generator=g, dtype=torch.float64)
    return a, wt, dy, R.conv3x3_fwd(a, wt), R.conv3x3_dw(a, dy)


def test_fp32_rounding_is_accepted(conv):
    _, _, _, (ref, cond), (dw, cw) = conv
    assert R.TAU_WINO <= R.ceiling(1024) and R.TAU_DIRECT <= R.ceiling(1024)
    for tau in (R.TAU_WINO, R.TAU_DIRECT, R.TAU_CONVT, R.TAU_1X1):
        R.check_bound(f32(ref), ref, cond, tau, "fp32 rounding")
    R.check_bound(f32(dw), dw, cw, R.TAU_DW, "fp32 rounding (dW)")


def _rejects(got, ref, cond, tau, match):
    with pytest.raises(AssertionError, match=match):
        R.check_bound(got, ref, cond, tau, "mutated")


@pytest.mark.parametrize("tau", [R.TAU_WINO, R.TAU_DIRECT])
def test_mutations_are_rejected(conv, tau):
    a, wt, dy, (ref, cond), _ = conv
    # one product removed at a corner pixel (the smallest of the ci products there: any one of them must show)
    got = ref.clone()
    prods = (wt[2, :, 1, 1] * a[1, :, 0, 0]).abs()
    ci = int(prods.argmin())
    got[1, 2, 0, 0] -= wt[2, ci, 1, 1] * a[1, ci, 0, 0]
    _rejects(f32(got), ref, cond, tau, "worst ratio")
    # one 2x4 tile of one channel scaled by (1 + 1e-4)
    got = ref.clone()
    got[2, 5, 2:4, 4:8] *= 1 + 1e-4
    _rejects(f32(got), ref, cond, tau, r"at \(2, 5, [23], [4-7]\)")
    # two images swapped
    got = ref.clone()
    got[[0, 1]] = got[[1, 0]]
    _rejects(f32(got), ref, cond, tau, "images")
    # one column's left halo read one column too far: output column 4 takes its kw=0 taps from column 2 instead of 3
    got = ref.clone()
    ap = F.pad(a, [1, 1, 1, 1])
    for kh in range(3):
        wrong = torch.einsum("oc,nch->noh", wt[:, :, kh, 0], ap[:, :, kh:kh + H, 3] - ap[:, :, kh:kh + H, 4])
        got[:, :, :, 4] += wrong
    _rejects(f32(got), ref, cond, tau, "tile column edge")
    # one element left unwritten
    got = f32(ref)
    got[0, 7, H - 1, W - 1] = float("nan")
    _rejects(got, ref, cond, tau, r"not finite .* first at \(0, 7, 7, 11\)")


def test_dw_row_removed_is_rejected(conv):
    a, _, dy, _, (dw, cw) = conv
    rows = R.conv3x3_dw_rows(a[2:3], dy[2:3])
    for r in (0, H // 2, H - 1):
        _rejects(f32(dw - rows[r]), dw, cw, R.TAU_DW, "worst ratio")


def test_unwritten_and_cond_zero():
    ref = torch.zeros(1, 1, 2, 4, dtype=torch.float64)
    cond = torch.zeros_like(ref)
    assert R.check_bound(ref.clone(), ref, cond, 1e-6, "zeros") == 0.0
    got = ref.clone()
    got[0, 0, 1, 3] = 1e-30          # a masked (cond == 0) element must be exactly 0
    _rejects(got, ref, cond, 1e-6, "worst ratio inf")
