"""tests/fp64_ref.py on the CPU at small shapes: its tap-matmul references equal torch's own float64 convolutions and autograd,
cond bounds |ref| (and equals it for non-negative operands), and check_bound at the module's taus accepts an fp32 rounding of
the exact result while rejecting the small, local mistakes the GPU kernel tests exist to catch: one product missing at a corner,
one 2x4 Winograd tile off by 1e-4, two images swapped, one column's halo read one column too far, one image row missing from
dW, one element never written."""
import math

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


# ---- the bf16 bound and the references of the bf16-only operations
def _bf16_grid():
    """fp64 values across binades: exact powers of two, ties half-way between two bf16 neighbours, values just off a tie."""
    e = torch.arange(-20, 21, dtype=torch.float64)
    p2 = torch.pow(2.0, e)
    m = torch.arange(128, 256, dtype=torch.float64) / 128          # the 128 bf16 mantissas of [1, 2)
    tie = (m + 0.5 / 128)[None, :] * p2[:, None]                   # half-way between neighbours (RNE: to the even one)
    off = (m + 0.37 / 128)[None, :] * p2[:, None]
    vals = torch.cat([p2, tie.reshape(-1), off.reshape(-1), rn(4096) * 3])
    return torch.cat([vals, -vals]).view(1, 1, 1, -1)


def test_check_bound_bf16_accepts_rne_across_binades():
    ref = _bf16_grid()
    cond = torch.zeros_like(ref)         # no accumulation at all: the rounding allowance alone must carry RNE
    got = ref.float().to(torch.bfloat16).float()
    assert R.check_bound_bf16(got, ref, cond, 0.0, "RNE") == 0.0
    assert bool((got.double() != ref).any())       # (the grid does round)
    # ties go to the even mantissa, and an exact power of two is kept exactly
    assert float(torch.tensor(1.0 + 1.5 / 128).to(torch.bfloat16)) == 1.0 + 2.0 / 128
    assert float(torch.tensor(2.0 ** -20).to(torch.bfloat16)) == 2.0 ** -20


def test_check_bound_bf16_rejects_truncation_one_ulp_and_nan():
    ref = rn(1, 8, 16, 16) * 10
    cond = ref.abs() * 4
    ok = ref.float().to(torch.bfloat16).float()
    R.check_bound_bf16(ok, ref, cond, R.TAU_BF16_CONV, "RNE")
    # round toward zero: the 16 low bits of the fp32 pattern cut off
    rtz = (ref.float().view(torch.int32) & ~0xffff).view(torch.float32)
    with pytest.raises(AssertionError, match="2\\^-8"):
        R.check_bound_bf16(rtz, ref, cond, R.TAU_BF16_CONV, "RTZ")
    # one element one bf16 ulp off the RNE result, away from the exact value: 1.3 rounds down to 1.296875 (ulp 2^-7 in [1, 2)),
    # the wrong result is 1.2890625 (the ulp toward 1.3 would still lie within 2^-8 |ref| -- that is what the bound admits)
    ref[0, 3, 5, 7] = 1.3
    cond[0, 3, 5, 7] = 4 * 1.3
    ok[0, 3, 5, 7] = 1.296875
    R.check_bound_bf16(ok, ref, cond, R.TAU_BF16_CONV, "RNE")
    one = ok.clone()
    one[0, 3, 5, 7] = 1.296875 - 2.0 ** -7
    with pytest.raises(AssertionError, match=r"at 1 of .* \(0, 3, 5, 7\)"):
        R.check_bound_bf16(one, ref, cond, R.TAU_BF16_CONV, "one ulp")
    nan = ok.clone()
    nan[0, 1, 2, 3] = float("nan")
    with pytest.raises(AssertionError, match=r"not finite .* \(0, 1, 2, 3\)"):
        R.check_bound_bf16(nan, ref, cond, R.TAU_BF16_CONV, "NaN")


def test_bf16_first_layer_and_batchnorm_refs_equal_torch():
    """first_fwd == F.conv2d on bf16(x), bf16(w); pass 1 + pass 2 of the BatchNorm backward (bn_bwd_dz, bn_bwd_sums,
    bn_bwd_apply with c1 = sum dz / count, c2 = sum dz*xhat / count) == torch's train-mode BatchNorm2d + ReLU autograd; the
    apply is relu(fmaf(y, scale, shift)) rounded through fp32 to bf16."""
    n, c, h, w = 2, 6, 7, 9
    x = rn(n, 3, h, w).float()
    wt = rn(c, 3, 3, 3).float()
    ref, cond = R.first_fwd(x, wt)
    t = F.conv2d(x.to(torch.bfloat16).double(), wt.to(torch.bfloat16).double(), padding=1)
    assert rel(ref, t) < 1e-12 and bool((cond >= ref.abs()).all())
    # BatchNorm2d(train) + ReLU forward and backward in float64
    y = R.bf16(rn(n, c, h, w) * 2 + 0.3)
    gamma, beta = rn(c).abs() + 0.5, rn(c) * 0.3
    bn = torch.nn.BatchNorm2d(c, eps=1e-5).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    yv = y.clone().requires_grad_(True)
    a = torch.relu(bn(yv))
    da = rn(n, c, h, w)
    a.backward(da)
    mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    stored, aref, acond = R.bn_relu_bf16(y, scale, shift)
    assert rel(aref, a.detach()) < 1e-12
    assert torch.equal(stored, a.detach().float().to(torch.bfloat16).double()) or \
        float((stored - a.detach()).abs().max()) <= 2.0 ** -8 * float(a.abs().max())
    R.check_bound_bf16(stored.float(), aref, acond, R.TAU_BF16_PW, "apply")
    dz, dzc = R.bn_bwd_dz(y, scale, shift, da)
    assert torch.equal(dz, da * (a.detach() > 0)) and torch.equal(dzc, dz.abs())
    s1, s2, b1, b2 = R.bn_bwd_sums(dz, y, mean, invstd)
    cnt = n * h * w
    dx, dxc = R.bn_bwd_apply(dz, y, scale, mean, invstd, s1 / cnt, s2 / cnt)
    assert rel(dx, yv.grad) < 1e-10 and bool((dxc >= dx.abs() * (1 - 1e-12)).all())
    assert bool((b1 >= s1.abs()).all()) and bool((b2 >= s2.abs()).all())
    # the statistics epilogue's sums
    q1, q2, c1_, c2_ = R.stored_sums(y)
    assert rel(q1 / cnt, mean) < 1e-12 and rel(q2 / cnt - (q1 / cnt) ** 2, var) < 1e-10 and bool((c1_ >= q1.abs()).all())


@pytest.mark.parametrize("h,w", [(6, 8), (7, 9)])
def test_maxpool_route_equals_torch_including_ties(h, w):
    """maxpool_route / pool_grad == F.max_pool2d(return_indices) and its gradient, on coarse values with many ties (torch, like
    the kernels, keeps the first maximum in window order) and with the odd last row / column dropped."""
    n, c = 2, 5
    a = (torch.randint(0, 3, (n, c, h, w), generator=G).double() - 1).clamp_min(0)     # ReLU'd, mostly 0 / 1: ties everywhere
    a[0, 0, :2, :2] = torch.tensor([[1.0, 1.0], [1.0, 1.0]])                           # a 4-way tie: position 0
    a[0, 1, :2, :2] = torch.tensor([[0.0, 2.0], [2.0, 2.0]])                           # a 3-way tie: position 1
    pooled, code = R.maxpool_route(a)
    tp, ti = F.max_pool2d(a, 2, return_indices=True)
    assert torch.equal(pooled, tp)
    hp, wp = h // 2, w // 2
    rr = torch.arange(hp).view(1, 1, hp, 1) * 2
    cc = torch.arange(wp).view(1, 1, 1, wp) * 2
    flat = (rr + code // 2) * w + (cc + code % 2)
    assert torch.equal(flat, ti)
    assert int(code[0, 0, 0, 0]) == 0 and int(code[0, 1, 0, 0]) == 1
    dp = rn(n, c, hp, wp)
    av = a.clone().requires_grad_(True)
    F.max_pool2d(av, 2).backward(dp)
    assert torch.equal(R.pool_grad(dp, code, h, w), av.grad)


# --------------------------------------------------------------------------- fp32 engine: fmaf, finalize, Adam + EMA
def _round_f32(x):
    """An exact rational rounded to fp32, nearest, ties to even (the reference for fmaf32)."""
    from fractions import Fraction
    c = torch.tensor(float(x), dtype=torch.float64).float()
    cands = [c, torch.nextafter(c, torch.tensor(math.inf)), torch.nextafter(c, torch.tensor(-math.inf))]
    return float(min(cands, key=lambda t: (abs(Fraction(float(t)) - x), int(t.view(torch.int32)) & 1)))


def test_fmaf32_is_fmaf_bit_for_bit():
    """fmaf32 against exact rational arithmetic: random operands, and constructed cases whose fp64 sum lands exactly on an fp32
    midpoint while the exact sum lies just below it -- there the plain fp64-then-fp32 rounding (deferred_act) is one ulp off."""
    from fractions import Fraction
    g = torch.Generator().manual_seed(11)
    x, s, b = (torch.randn(400, generator=g) * 3 for _ in range(3))
    got = R.fmaf32(x, s, b)
    for i in range(400):
        ex = Fraction(float(x[i])) * Fraction(float(s[i])) + Fraction(float(b[i]))
        assert float(got[i]) == _round_f32(ex), i
    # b with an odd last mantissa bit, x * s = ulp(b)/2 * (1 - 2^-46): t = b + ulp/2 (a midpoint) in fp64, the exact sum is
    # just below it, so fmaf gives b while ties-to-even of t gives the even neighbour b + ulp
    r = (torch.rand(64, generator=g) + 1.0).float()
    r = torch.where((r.view(torch.int32) & 1) == 1, r, torch.nextafter(r, torch.full_like(r, 3.0)))
    r = r * torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0) * 2.0 ** torch.randint(-20, 20, (64,), generator=g).float()
    ulp = (torch.nextafter(r.abs(), torch.full_like(r, math.inf)) - r.abs()).double()
    xs = torch.full_like(r, 1.0 + 2.0 ** -23)
    ss = (torch.sign(r).double() * ulp / 2 * (1 - 2.0 ** -23)).float()
    got = R.fmaf32(xs, ss, r)
    plain = (xs.double() * ss.double() + r.double()).float().double()
    for i in range(64):
        ex = Fraction(float(xs[i])) * Fraction(float(ss[i])) + Fraction(float(r[i]))
        assert float(got[i]) == _round_f32(ex) == float(r[i]), i
    assert bool((plain != got).all()), "the constructed cases are double-rounding cases"


def _bn_toy(offset=0.0):
    g = torch.Generator().manual_seed(5)
    n, c, h, w = 4, 6, 5, 7
    x = torch.randn((n, c, h, w), generator=g, dtype=torch.float64) * torch.linspace(0.2, 3.0, c).view(1, c, 1, 1)
    x = x + offset * torch.linspace(-1, 1, c).view(1, c, 1, 1)
    gamma, beta = torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(c, generator=g, dtype=torch.float64) * 0.1, torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    return x, gamma, beta, rm, rv


@pytest.mark.parametrize("offset", [0.0, 30.0])
def test_bn_finalize_ref_equals_batch_norm(offset):
    """bn_finalize_ref from exact sums == F.batch_norm(training=True) in fp64 (normalised output through scale / shift, running
    mean / unbiased running variance), also for channels whose |mean| / std is about 30; its cond of var is the carried sums
    bound (b2 + 2 |mean| b1) / count."""
    x, gamma, beta, rm, rv = _bn_toy(offset)
    cnt = x.numel() / x.shape[1]
    s = lambda t: t.sum((0, 2, 3))  # noqa: E731
    r = R.bn_finalize_ref(s(x), s(x * x), s(x.abs()), s(x * x), cnt, gamma, beta, running_mean=rm, running_var=rv)
    rm_t, rv_t = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm_t, rv_t, gamma, beta, training=True, momentum=R.f32c(0.1), eps=R.f32c(1e-5))
    v = (1, -1, 1, 1)
    assert rel(x * r["scale"][0].view(v) + r["shift"][0].view(v), y) < 1e-10
    assert rel(r["running_mean"][0], rm_t) < 1e-12 and rel(r["running_var"][0], rv_t) < 1e-10
    mu = x.mean((0, 2, 3))
    assert torch.allclose(r["var"][1], (s(x * x) + 2 * mu.abs() * s(x.abs())) / cnt, rtol=1e-14)
    if offset:
        assert float((mu.abs() / x.std((0, 2, 3))).max()) > 25


def test_bn_finalize_bound_rejects_mutations():
    """At toy size the carried bound rejects normalising with the unbiased variance, and a running variance updated with the
    biased one, while it accepts an fp32 rounding of each output."""
    x, gamma, beta, rm, rv = _bn_toy()
    cnt = x.numel() / x.shape[1]
    s = lambda t: t.sum((0, 2, 3))  # noqa: E731
    r = R.bn_finalize_ref(s(x), s(x * x), s(x.abs()), s(x * x), cnt, gamma, beta, running_mean=rm, running_var=rv)
    for k in ("mean", "invstd", "scale", "shift", "running_mean", "running_var"):
        R.check_bound_rounded(r[k][0].float(), r[k][0], r[k][1], R.TAU_STATS, k)
    var = r["var"][0]
    unb = 1.0 / torch.sqrt(var * cnt / (cnt - 1) + R.f32c(1e-5))
    with pytest.raises(AssertionError):
        R.check_bound_rounded(unb.float(), *r["invstd"], R.TAU_STATS, "invstd from the unbiased variance")
    biased = (1 - R.f32c(0.1)) * rv + R.f32c(0.1) * var
    with pytest.raises(AssertionError):
        R.check_bound_rounded(biased.float(), *r["running_var"], R.TAU_STATS, "running_var from the biased variance")


def _adam_f32(p, g, m, v, ema, step, lr, b1, b2, eps, wd, d, gs):
    """gsd_adam_ema's arithmetic in fp32, operation by operation (fmaf exactly, through fmaf32)."""
    f = lambda t: t.float().double()  # noqa: E731
    c = lambda a: torch.full_like(p, R.f32c(a))  # noqa: E731
    b1, b2 = R.f32c(b1), R.f32c(b2)
    lr_bc1, sbc2 = R.f32c(R.f32c(lr) / (1 - b1 ** step)), R.f32c(math.sqrt(1 - b2 ** step))
    gv = R.fmaf32(c(wd), p, f(g * R.f32c(gs)))
    mv = f(m + f(f(gv - m) * (1 - b1)))
    vv = R.fmaf32(c(1 - b2), f(gv * gv), f(v * b2))
    den = f(f(f(torch.sqrt(vv)) / sbc2) + R.f32c(eps))
    pv = f(p - f(lr_bc1 * f(mv / den)))
    out = {"p": pv, "m": mv, "v": vv}
    if ema is not None:
        omd = R.f32c(1 - R.f32c(d))
        out["ema"] = f(ema - f(omd * f(ema - pv)))
    return out


def _opt_state(n=4000, seed=3):
    g = torch.Generator().manual_seed(seed)
    f = lambda t: t.float().double()  # noqa: E731
    p = f(torch.randn(n, generator=g, dtype=torch.float64) * 0.05)
    gr = f(torch.randn(n, generator=g, dtype=torch.float64) * 1e-3 * torch.rand(n, generator=g, dtype=torch.float64))
    m = f(torch.randn(n, generator=g, dtype=torch.float64) * 1e-4)
    v = f(torch.rand(n, generator=g, dtype=torch.float64) * 1e-7)
    ema = f(p + torch.randn(n, generator=g, dtype=torch.float64) * 1e-3)
    return p, gr, m, v, ema


def test_adam_ema_ref_equals_torch_adam_and_ema():
    """adam_ema_ref with plain fp64 constants over four steps == torch.optim.Adam(weight_decay=0.1) in float64, and its EMA ==
    torch_ema's update with the warm-up decay min(d, (1 + n) / (10 + n))."""
    p, gr, _, _, _ = _opt_state()
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
    m, v, ema, pr = torch.zeros_like(p), torch.zeros_like(p), p.clone(), p.clone()
    for step in range(1, 5):
        gs = gr * (1.0 + 0.3 * step)
        pt.grad = gs.clone()
        opt.step()
        d = min(0.995, (1.0 + step) / (10.0 + step))
        r = R.adam_ema_ref(pr, gs, m, v, ema, step, 1e-3, weight_decay=0.1, ema_decay=d, kernel_constants=False)
        shadow = ema - (1.0 - d) * (ema - pt.detach())
        pr, m, v, ema = r["p"][0], r["m"][0], r["v"][0], r["ema"][0]
        st = opt.state[pt]
        assert rel(pr, pt.detach()) < 1e-13 and rel(m, st["exp_avg"]) < 1e-13 and rel(v, st["exp_avg_sq"]) < 1e-13
        assert rel(ema, shadow) < 1e-13


@pytest.mark.parametrize("step,wd,gs", [(1, 0.0, 1.0), (2, 1e-6, 1.0), (1000, 0.1, 0.5)])
def test_adam_ema_bound_accepts_fp32_and_rejects_mutations(step, wd, gs):
    """The kernel's fp32 arithmetic lands within TAU_ADAM * cond of adam_ema_ref; the bias correction of step - 1 used at step,
    and the EMA decay of the other warm-up step, are rejected (as is dropping the weight decay where it is 0.1)."""
    p, gr, m, v, ema = _opt_state(seed=step)
    d = min(0.995, (1.0 + step) / (10.0 + step))
    r = R.adam_ema_ref(p, gr, m, v, ema, step, 1e-3, weight_decay=wd, ema_decay=d, grad_scale=gs)
    got = _adam_f32(p, gr, m, v, ema, step, 1e-3, 0.9, 0.999, 1e-8, wd, d, gs)
    for k in ("p", "m", "v", "ema"):
        R.check_bound(got[k], r[k][0], r[k][1], R.TAU_ADAM, f"adam {k}")
    if step > 1:
        bad = _adam_f32(p, gr, m, v, ema, 1 if step == 2 else step - 1, 1e-3, 0.9, 0.999, 1e-8, wd, d, gs)
        with pytest.raises(AssertionError):
            R.check_bound(bad["p"], *r["p"], R.TAU_ADAM, "bias correction of the previous step")
    other = min(0.995, (1.0 + step + 1) / (10.0 + step + 1))
    bad = _adam_f32(p, gr, m, v, ema, step, 1e-3, 0.9, 0.999, 1e-8, wd, other, gs)
    with pytest.raises(AssertionError):
        R.check_bound(bad["ema"], *r["ema"], R.TAU_ADAM, "EMA decay of the next step")
    if wd >= 0.1:
        bad = _adam_f32(p, gr, m, v, ema, step, 1e-3, 0.9, 0.999, 1e-8, 0.0, d, gs)
        with pytest.raises(AssertionError):
            R.check_bound(bad["p"], *r["p"], R.TAU_ADAM, "weight decay dropped")


def test_pool_routing_and_c2_mutations_are_rejected():
    """A pooled gradient routed to the second-largest element of its window, and c2 dropped for one channel of d_raw, fail the
    bounds the engine step holds dz and d_raw to."""
    g = torch.Generator().manual_seed(9)
    n, c, h, w = 2, 3, 6, 7
    raw = torch.randn((n, c, h, w), generator=g).double()
    sc, sh = torch.rand(c, generator=g).double() + 0.5, torch.randn(c, generator=g).double() * 0.1
    a = R.bnrelu_act(raw, sc, sh)
    best, code = R.maxpool_route(a)
    dp = torch.randn((n, c, h // 2, w // 2), generator=g).double() * 1e-3
    da = torch.randn((n, c, h, w), generator=g).double() * 1e-3
    routed = R.pool_grad(dp, code, h, w)
    ref, cond = R.bn_bwd_dz(raw, sc, sh, da + routed, da.abs() + routed.abs())
    R.check_bound(ref.float(), ref, cond, R.TAU_WINO, "dz")
    # the window of (0, 0, 0, 0) with the largest two positive entries: route to the second one instead
    win = a[:, :, :2 * (h // 2), :2 * (w // 2)].reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    srt = win.sort(-1, descending=True)
    ok = (srt.values[..., 1] > 0).nonzero()
    assert len(ok) > 0
    i0, c0, y0, x0 = ok[0].tolist()
    second = int(srt.indices[i0, c0, y0, x0, 1])
    code2 = code.clone()
    code2[i0, c0, y0, x0] = second
    bad, _ = R.bn_bwd_dz(raw, sc, sh, da + R.pool_grad(dp, code2, h, w))
    with pytest.raises(AssertionError):
        R.check_bound(bad.float(), ref, cond, R.TAU_WINO, "routed to the second-largest element")
    mean, invstd = raw.mean((0, 2, 3)), 1.0 / raw.std((0, 2, 3))
    c1, c2 = torch.randn(c, generator=g).double() * 1e-4, torch.randn(c, generator=g).double() * 1e-4
    d, dc = R.bn_bwd_apply(ref, raw, sc, mean, invstd, c1, c2)
    R.check_bound(d.float(), d, dc, R.TAU_PW, "d_raw")
    bad = d.clone()
    k = int(c2.abs().argmax())
    bad[:, k] += sc[k] * (raw[:, k] - mean[k]) * invstd[k] * c2[k]
    with pytest.raises(AssertionError):
        R.check_bound(bad.float(), d, dc, R.TAU_PW, "c2 dropped")
