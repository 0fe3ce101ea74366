"""Element-wise fp64 bounds for the fp32 engine's non-contraction kernels (gelslim_depth_amd/csrc/gsd_bn.hip, gsd_head.hip, gsd_optim.hip) in the
cases one default train step cannot reach: both forms of every launch, K > 1 output classes, odd H, windows built to tie, the
SyncBN finalize, channels with a large |mean| / std, eval coefficients, and the optimiser at step 1, 2 and 1000 with a visible
coupled L2 term, grad_scale 1/2, without EMA and under a guard that marks the step bad.

Shapes are the network's (N = 32 at the five level sizes of 3x320x427) unless a case needs another.  Outputs start as NaN, and
whatever a launch must not touch -- partial rows past gsd_bn_bwd_partial_rows, the pitched pad columns' neighbours, the rest of
a buffer -- holds a sentinel that is checked afterwards.  Where a result is a selection or one fp32 rounding of a known value
(dz of the reduce kernels, pooled values and pool routing, eval-mode mean, the backward finalize) it must be bit-equal
(torch.equal); everything else is held to |got - ref| <= tau * cond (+ one fp32 rounding where the kernel rounds an fp64 value).

GSD_FP64_REPORT_POINTWISE=<path>: write the worst ratio per key, the module's wall time and peak device memory there as JSON.
"""
import ctypes as C
import json
import os
import time

import pytest
import torch
import torch.nn.functional as F

import fp64_ref as R

pytestmark = pytest.mark.gpu

DIMS = [64, 128, 256, 512, 1024]
HS = [320, 160, 80, 40, 20]
WS = [427, 213, 106, 53, 26]
N = 32
TAIL = 4096
SENT = 12345.0
T0 = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    torch.cuda.reset_peak_memory_stats()
    T0["t"] = time.time()
    yield
    path = os.environ.get("GSD_FP64_REPORT_POINTWISE")
    if path:
        with open(path, "w") as f:
            json.dump({"wall_s": time.time() - T0["t"], "max_memory_allocated": torch.cuda.max_memory_allocated(),
                       "ratios": dict(sorted((k, v) for k, v in R.RATIOS.items() if k.startswith("pw")))}, f, indent=1)


@pytest.fixture(scope="module")
def L():
    from gelslim_depth_amd import _lib
    return _lib


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def uniform(g, lo, hi, *shape):
    return torch.rand(shape, generator=g, device="cuda") * (hi - lo) + lo


def randn(g, *shape, scale=1.0):
    return torch.randn(shape, generator=g, device="cuda") * scale


def buffer(shape, fill=float("nan"), offset=0):
    """A tensor of `shape` at float `offset` of a buffer with a sentinel tail: offset 1 breaks 16-byte alignment (the scalar
    forms), the tail shows a write past the end."""
    numel = 1
    for s in shape:
        numel *= s
    b = torch.full((offset + numel + TAIL,), SENT, device="cuda")
    t = b[offset:offset + numel].view(shape)
    t.fill_(fill)
    return b, t


def tail_ok(b, numel, offset, what):
    torch.cuda.synchronize()
    assert bool((b[offset + numel:] == SENT).all()) and (offset == 0 or bool((b[:offset] == SENT).all())), \
        f"{what}: written outside the tensor"


def bn_params(g, c):
    return (uniform(g, 0.3, 1.5, c), randn(g, c, scale=0.3), randn(g, c, scale=0.3), uniform(g, 0.5, 2.0, c))


def bwd_sums(L, part, rows, c):
    s = torch.zeros(65 * 3 * c, dtype=torch.float64, device="cuda")
    L.check(L.lib.gsd_bn_bwd_reduce_partials(part.data_ptr(), rows, c, s.data_ptr(), L.stream_ptr()), "bwd sums")
    return s[:c], s[c:2 * c], s[2 * c:3 * c]


def check_dz_sums(L, part, rows, dz, raw, mean, invstd, what, key):
    """The reduce kernel's per-channel sums (of what it stored) against fp64 sums of the stored dz."""
    s1, s2, s3 = bwd_sums(L, part, rows, dz.shape[1])
    q1, q2, a1, a2 = R.bn_bwd_sums(dz, raw, mean, invstd)
    R.check_sums(s1, q1, a1, R.TAU_STATS, f"{what} sum dz", key=key)
    R.check_sums(s2, q2, a2, R.TAU_STATS, f"{what} sum dz*xhat", key=key)
    return s3


def rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


# ------------------------------------------------------------------------------------------------ BatchNorm backward pass 1
RED = [(lvl, mode, form) for lvl in range(5) for mode in (0, 2) for form in ("vec", "scalar")]


@pytest.mark.parametrize("lvl,mode,form", RED, ids=[f"L{l}-mode{m}-{f}" for l, m, f in RED])
def test_bn_bwd_reduce_elementwise(L, lvl, mode, form):
    """gsd_bn_bwd_reduce modes 0 (dz = where(mask, da, 0)) and 2 with K = 1 (dz = where(mask, fl32(dout * w), 0), third sum
    dW_out) on the 16-byte kernel and, with every operand one float off 16-byte alignment, the scalar one: dz bit-equal, the
    partial sums against fp64, nothing written past the partial rows or the tensors."""
    c, h, w = DIMS[lvl], HS[lvl], WS[lvl]
    g = gen(100 * lvl + 10 * mode + (form == "scalar"))
    off = 1 if form == "scalar" else 0
    sc, sh, mean, invstd = bn_params(g, c)
    braw, raw = buffer((N, c, h, w), offset=off)
    raw.normal_(generator=g)
    bdz, dz = buffer((N, c, h, w), offset=off)
    rows = L.lib.gsd_bn_bwd_partial_rows(N, c, h, w)
    part = torch.full((rows * 3 * c + TAIL,), SENT, device="cuda")
    part[:rows * 3 * c] = float("nan")
    tag = f"L{lvl}-mode{mode}-{form}"
    if mode == 0:
        bda, da = buffer((N, c, h, w), offset=off)
        da.normal_(generator=g)
        src = L.make_src(da)
        L.check(L.lib.gsd_bn_bwd_reduce(0, raw.data_ptr(), sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                        C.byref(src), None, None, None, 1, dz.data_ptr(), part.data_ptr(), N, c, h, w,
                                        L.stream_ptr()), "bn_bwd_reduce(0)")
        gref = da.double()
    else:
        bdo, dout = buffer((N, 1, h, w), offset=off)
        dout.normal_(generator=g)
        wo = randn(g, 1, c, scale=0.125)
        L.check(L.lib.gsd_bn_bwd_reduce(2, raw.data_ptr(), sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                        None, None, dout.data_ptr(), wo.data_ptr(), 1, dz.data_ptr(), part.data_ptr(), N, c, h,
                                        w, L.stream_ptr()), "bn_bwd_reduce(2)")
        gref = (dout.double() * wo.double().view(1, c, 1, 1)).float().double()
    tail_ok(bdz, dz.numel(), off, f"{tag} dz")
    assert bool((part[rows * 3 * c:] == SENT).all()), f"{tag}: partial rows written past the {rows} reported"
    m = R.bnrelu_mask(raw, sc, sh)
    ref = torch.where(m, gref, torch.zeros((), dtype=torch.float64, device="cuda"))
    assert torch.equal(dz.double(), ref), f"{tag}: dz is not where(mask, g, 0) bit for bit"
    s3 = check_dz_sums(L, part, rows, dz, raw, mean, invstd, tag, f"pw-stats:{tag}")
    if mode == 2:
        a = R.bnrelu_act(raw, sc, sh)
        r_ = R.conv1x1_dw(a, dout.double())
        R.check_bound(s3.view(1, c), r_[0], r_[1], R.TAU_1X1, f"{tag} dW_out (third sum)", key=f"pw-1x1:{tag}", weights=True)


@pytest.mark.parametrize("k", (2, 8))
def test_bn_bwd_reduce_outc_k_classes(L, k):
    """Mode 2 with K > 1 output classes (the scalar kernel): dz = where(mask, fmaf(d_K-1, w_K-1, ... fmaf(d_0, w_0, 0))) bit for
    bit, and gsd_conv1x1_out_wgrad for all K rows of dW_out against fp64."""
    c, h, w = DIMS[0], HS[0], WS[0]
    g = gen(700 + k)
    sc, sh, mean, invstd = bn_params(g, c)
    raw = randn(g, N, c, h, w)
    dout = randn(g, N, k, h, w)
    wo = randn(g, k, c, scale=0.125)
    bdz, dz = buffer((N, c, h, w))
    rows = L.lib.gsd_bn_bwd_partial_rows(N, c, h, w)
    part = torch.full((rows * 3 * c + TAIL,), SENT, device="cuda")
    L.check(L.lib.gsd_bn_bwd_reduce(2, raw.data_ptr(), sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(), None,
                                    None, dout.data_ptr(), wo.data_ptr(), k, dz.data_ptr(), part.data_ptr(), N, c, h, w,
                                    L.stream_ptr()), "bn_bwd_reduce(2, K)")
    tail_ok(bdz, dz.numel(), 0, f"K{k} dz")
    assert bool((part[rows * 3 * c:] == SENT).all())
    for i in range(0, N, 8):
        gk = torch.zeros((8, c, h, w), dtype=torch.float64, device="cuda")
        for q in range(k):
            gk = R.fmaf32(dout[i:i + 8, q:q + 1].expand(-1, c, -1, -1), wo[q].view(1, c, 1, 1).expand(8, c, h, w), gk)
        ref = torch.where(R.bnrelu_mask(raw[i:i + 8], sc, sh), gk, torch.zeros((), dtype=torch.float64, device="cuda"))
        assert torch.equal(dz[i:i + 8].double(), ref), f"K{k}: dz (images {i}..{i + 8})"
        del gk, ref
    check_dz_sums(L, part, rows, dz, raw, mean, invstd, f"K{k}", f"pw-stats:K{k}")
    dw = torch.full((k, c), float("nan"), device="cuda")
    wrows = L.lib.gsd_conv1x1_out_wgrad_rows(N, h, w)
    wpart = torch.full((wrows * k * c,), float("nan"), device="cuda")
    wsums = torch.zeros(65 * k * c, dtype=torch.float64, device="cuda")
    L.check(L.lib.gsd_conv1x1_out_wgrad(raw.data_ptr(), sc.data_ptr(), sh.data_ptr(), dout.data_ptr(), c, k, dw.data_ptr(),
                                        wpart.data_ptr(), wsums.data_ptr(), N, h, w, L.stream_ptr()), "conv1x1_out_wgrad")
    ref = torch.zeros((k, c), dtype=torch.float64, device="cuda")
    cond = torch.zeros_like(ref)
    for i in range(0, N, 8):
        r_ = R.conv1x1_dw(R.bnrelu_act(raw[i:i + 8], sc, sh), dout[i:i + 8].double())
        ref += r_[0]
        cond += r_[1]
    R.check_bound(dw, ref, cond, R.TAU_1X1, f"K{k} conv1x1_out_wgrad", key=f"pw-1x1:K{k}", weights=True)


POOL = [("L0", 32, 64, 320, 427), ("L1", 32, 128, 160, 213), ("L2", 32, 256, 80, 106), ("L3", 32, 512, 40, 53),
        ("oddHW", 5, 24, 21, 27)]


def tie_windows(raw, g):
    """A quarter of the windows with two equal maxima, an eighth with four equal values, an eighth all far below zero (after
    BatchNorm + ReLU every element 0): the first-maximum rule decides them all."""
    hp, wp = raw.shape[2] // 2, raw.shape[3] // 2
    v = raw[:, :, :2 * hp, :2 * wp]
    v[:, :, 0::2, 1::2][..., 0::4, :] = v[:, :, 0::2, 0::2][..., 0::4, :]           # (0,0) == (0,1)
    v[:, :, 1::2, 1::2][..., 1::4, :] = v[:, :, 0::2, 1::2][..., 1::4, :]           # (0,1) == (1,1)
    for q in ((0, 1), (1, 0), (1, 1)):
        v[:, :, q[0]::2, q[1]::2][..., 2::8, :] = v[:, :, 0::2, 0::2][..., 2::8, :]  # all four equal
    for q in ((0, 0), (0, 1), (1, 0), (1, 1)):
        v[:, :, q[0]::2, q[1]::2][..., 6::8, :] = -50.0 - torch.rand(v[:, :, q[0]::2, q[1]::2][..., 6::8, :].shape,
                                                                     generator=g, device="cuda")


@pytest.mark.parametrize("case", POOL, ids=[p[0] for p in POOL])
def test_bn_bwd_reduce_pool_and_maxpool(L, case):
    """gsd_maxpool2 (bit-equal to the 2x2 max of max(fmaf(raw, scale, shift), 0), the odd last row / column dropped) and mode 1
    of gsd_bn_bwd_reduce with da present: dz = where(mask, fl32(da + routed dpool), 0) bit for bit, routed like
    F.max_pool2d(return_indices=True) on the fp32 activation, ties included; the partial sums against fp64.  The network's
    levels have even heights, so the odd-H shape is the one that runs the window form's `row1 == false` path."""
    name, n, c, h, w = case
    g = gen(900 + c)
    sc, sh, mean, invstd = bn_params(g, c)
    sc = sc.abs()
    sh = sh.clamp(-0.3, 0.3)
    raw = L.slack_empty((n, c, h, w), "cuda")
    raw.normal_(generator=g)
    tie_windows(raw, g)
    hp, wp = h // 2, w // 2
    bp, pooled = buffer((n, c, hp, wp))
    s = L.make_src(raw, sc, sh, relu=True, slack=L.SLACK)
    L.check(L.lib.gsd_maxpool2(C.byref(s), pooled.data_ptr(), n, c, h, w, L.stream_ptr()), "maxpool2")
    tail_ok(bp, pooled.numel(), 0, f"{name} maxpool2")
    da = randn(g, n, c, h, w)
    dpool = randn(g, n, c, hp, wp)
    bdz, dz = buffer((n, c, h, w))
    rows = L.lib.gsd_bn_bwd_partial_rows(n, c, h, w)
    part = torch.full((rows * 3 * c + TAIL,), SENT, device="cuda")
    src = L.make_src(da)
    L.check(L.lib.gsd_bn_bwd_reduce(1, raw.data_ptr(), sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                    C.byref(src), dpool.data_ptr(), None, None, 1, dz.data_ptr(), part.data_ptr(), n, c, h, w,
                                    L.stream_ptr()), "bn_bwd_reduce(1)")
    tail_ok(bdz, dz.numel(), 0, f"{name} dz")
    assert bool((part[rows * 3 * c:] == SENT).all()), f"{name}: partial rows written past the {rows} reported"
    step = max(1, (1 << 25) // (c * h * w))
    ties = 0
    for i in range(0, n, step):
        j = min(n, i + step)
        a = R.bnrelu_act(raw[i:j], sc, sh)
        best, code = R.maxpool_route(a)
        assert torch.equal(pooled[i:j].double(), best), f"{name}: pooled (images {i}..{j})"
        _, ti = F.max_pool2d(a.float(), 2, return_indices=True)
        rr = torch.arange(hp, device="cuda").view(1, 1, hp, 1) * 2
        cc = torch.arange(wp, device="cuda").view(1, 1, 1, wp) * 2
        assert torch.equal((rr + code // 2) * w + (cc + code % 2), ti), f"{name}: routing differs from F.max_pool2d"
        win = torch.stack([a[:, :, 0:2 * hp:2, 0:2 * wp:2], a[:, :, 0:2 * hp:2, 1:2 * wp:2], a[:, :, 1:2 * hp:2, 0:2 * wp:2],
                           a[:, :, 1:2 * hp:2, 1:2 * wp:2]], -1)
        ties += int(((win == best.unsqueeze(-1)).sum(-1) > 1).sum())
        routed = R.pool_grad(dpool[i:j], code, h, w)
        gsum = R.fmaf32(da[i:j], torch.ones_like(da[i:j]), routed)        # fl32(da + routed), one rounding
        ref = torch.where(R.bnrelu_mask(raw[i:j], sc, sh), gsum, torch.zeros((), dtype=torch.float64, device="cuda"))
        assert torch.equal(dz[i:j].double(), ref), f"{name}: dz (images {i}..{j})"
        del a, best, code, routed, gsum, ref, win
    assert ties > 0
    check_dz_sums(L, part, rows, dz, raw, mean, invstd, name, f"pw-stats:{name}")


# ------------------------------------------------------------------------------------------------ BatchNorm backward pass 2
APPLY = [(lvl, form) for lvl in range(5) for form in ("vec", "scalar", "pitched")]


@pytest.mark.parametrize("lvl,form", APPLY, ids=[f"L{l}-{f}" for l, f in APPLY])
def test_bn_bwd_apply(L, lvl, form):
    """gsd_bn_bwd_apply d_raw = scale * (dz - c1 - (raw - mean) * invstd * c2): in place on the 16-byte and (one float off
    alignment) the scalar kernel, and out of place into a pitched buffer whose pad columns W .. pitch-1 must be exactly 0."""
    c, h, w = DIMS[lvl], HS[lvl], WS[lvl]
    g = gen(1100 + 10 * lvl + len(form))
    sc, _, mean, invstd = bn_params(g, c)
    c1, c2 = randn(g, c, scale=0.1), randn(g, c, scale=0.1)
    off = 1 if form == "scalar" else 0
    braw, raw = buffer((N, c, h, w), offset=off)
    raw.normal_(generator=g)
    bdz, dz = buffer((N, c, h, w), offset=off)
    dz.normal_(generator=g)
    dz0 = dz.clone()
    tag = f"L{lvl}-{form}"
    if form == "pitched":
        p = (w + 3) // 4 * 4
        bout, outp = buffer((N, c, h, p))
        L.check(L.lib.gsd_bn_bwd_apply(dz.data_ptr(), raw.data_ptr(), sc.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                       c1.data_ptr(), c2.data_ptr(), N, c, h, w, outp.data_ptr(), p, L.stream_ptr()), "apply pitched")
        tail_ok(bout, outp.numel(), 0, tag)
        assert torch.equal(dz, dz0), f"{tag}: the pitched form wrote its input"
        assert bool((outp[..., w:] == 0).all()), f"{tag}: pad columns W..pitch-1 are not 0"
        got = outp[..., :w]
    else:
        L.check(L.lib.gsd_bn_bwd_apply(dz.data_ptr(), raw.data_ptr(), sc.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                       c1.data_ptr(), c2.data_ptr(), N, c, h, w, None, 0, L.stream_ptr()), "apply")
        tail_ok(bdz, dz.numel(), off, tag)
        got = dz
    step = max(1, (1 << 25) // (c * h * w))
    for i in range(0, N, step):
        ref, cond = R.bn_bwd_apply(dz0[i:i + step], raw[i:i + step], sc, mean, invstd, c1, c2)
        R.check_bound(got[i:i + step], ref, cond, R.TAU_PW, f"{tag} d_raw", n0=i, key=f"pw-apply:{tag}")
        del ref, cond


# ------------------------------------------------------------------------------------------------ BatchNorm finalize paths
def _fwd_rows(lvl, c):
    from gelslim_depth_amd.engine import _ConvForm
    cin = DIMS[lvl - 1] if lvl else c
    return _ConvForm.choose(N, HS[lvl], WS[lvl], cin, cin, c, True).partial_rows(N, HS[lvl], WS[lvl], c)


def conv_partials(g, rows, c, mpad, mu_over_std):
    """Partial rows as a statistics epilogue leaves them ([sum | sum of squares] of each row's pixels, fp32, mpad apart) for
    channels whose mean / std runs up to mu_over_std, and their exact fp64 sums and bounds."""
    per = 128
    mu = torch.linspace(-mu_over_std, mu_over_std, c, device="cuda", dtype=torch.float64)
    sd = torch.linspace(0.5, 2.0, c, device="cuda", dtype=torch.float64)
    s = (mu * per + torch.randn((rows, c), generator=g, device="cuda", dtype=torch.float64) * per ** 0.5) * sd
    # a row's sum of squares is at least its sum squared over its pixels (so the variance of the whole is >= 0), plus its spread
    q = s * s / per + (torch.rand((rows, c), generator=g, device="cuda", dtype=torch.float64) * 0.2 + 0.9) * per * sd * sd
    part = torch.full((rows, 2 * mpad), float("nan"), device="cuda")
    part[:, :c], part[:, mpad:mpad + c] = s.float(), q.float()
    s32, q32 = part[:, :c].double(), part[:, mpad:mpad + c].double()
    return part, s32.sum(0), q32.sum(0), s32.abs().sum(0), q32.sum(0), float(rows * per)


FIN = [(lvl, mos) for lvl in range(5) for mos in (1.0, 30.0)]


@pytest.mark.parametrize("lvl,mos", FIN, ids=[f"L{l}-mos{int(m)}" for l, m in FIN])
def test_bn_forward_finalize_paths(L, lvl, mos):
    """gsd_bn_reduce_finalize and gsd_bn_reduce_partials + gsd_bn_finalize on the same partials at the level's real row count
    (N = 32), and the SyncBN form (two ranks' sums added, count x 2): sums, mean, invstd, scale, shift and the running
    statistics against fp64 with the sums' bound carried through the one-pass variance; channels up to |mean| / std = 30."""
    c = DIMS[lvl]
    rows = _fwd_rows(lvl, c)
    mpad = (c + 63) // 64 * 64
    g = gen(1300 + 10 * lvl + int(mos))
    part, s1, s2, b1, b2, count = conv_partials(g, rows, c, mpad, mos)
    gamma, beta = uniform(g, 0.5, 1.5, c), randn(g, c, scale=0.3)
    rm0, rv0 = randn(g, c, scale=0.5), uniform(g, 0.5, 3.0, c)
    tag = f"L{lvl}-mos{int(mos)}"
    eps, mom = 1e-5, 0.1

    def outs():
        return [torch.full((c,), float("nan"), device="cuda") for _ in range(4)] + [rm0.clone(), rv0.clone()]

    def check(o, sums, ref_s, what):
        fin = R.bn_finalize_ref(*ref_s, gamma, beta, running_mean=rm0, running_var=rv0)
        if sums is not None:
            R.check_sums(sums[:c], ref_s[0], ref_s[2], R.TAU_STATS, f"{what} sum", key=f"pw-stats:{tag}")
            R.check_sums(sums[c:2 * c], ref_s[1], ref_s[3], R.TAU_STATS, f"{what} sum of squares", key=f"pw-stats:{tag}")
        for k, got in zip(("mean", "invstd", "scale", "shift", "running_mean", "running_var"), o):
            R.check_bound_rounded(got, *fin[k], R.TAU_STATS, f"{what} {k}", key=f"pw-bn:{tag}")
        return fin

    o = outs()
    sums = torch.full((65 * 2 * c,), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib.gsd_bn_reduce_finalize(part.data_ptr(), rows, mpad, c, sums.data_ptr(), count, gamma.data_ptr(), beta.data_ptr(),
                                         eps, mom, o[4].data_ptr(), o[5].data_ptr(), o[0].data_ptr(), o[1].data_ptr(),
                                         o[2].data_ptr(), o[3].data_ptr(), None, L.stream_ptr()), "bn_reduce_finalize")
    fin = check(o, sums, (s1, s2, b1, b2, count), f"{tag} one launch")
    if mos > 1:
        assert float((fin["mean"][0].abs() / fin["var"][0].sqrt()).max()) > 25
    o2 = outs()
    sums2 = torch.full((65 * 2 * c,), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib.gsd_bn_reduce_partials(part.data_ptr(), rows, mpad, c, sums2.data_ptr(), L.stream_ptr()), "bn_reduce_partials")
    L.check(L.lib.gsd_bn_finalize(sums2.data_ptr(), c, count, gamma.data_ptr(), beta.data_ptr(), eps, mom, o2[4].data_ptr(),
                                  o2[5].data_ptr(), o2[0].data_ptr(), o2[1].data_ptr(), o2[2].data_ptr(), o2[3].data_ptr(), None,
                                  L.stream_ptr()), "bn_finalize")
    check(o2, sums2, (s1, s2, b1, b2, count), f"{tag} three launches")
    # SyncBN: the second rank's partials, sums added (the all-reduce), count x world
    part_b, t1, t2, d1, d2, _ = conv_partials(gen(1400 + 10 * lvl + int(mos)), rows, c, mpad, mos)
    sums_b = torch.zeros((65 * 2 * c,), dtype=torch.float64, device="cuda")
    L.check(L.lib.gsd_bn_reduce_partials(part_b.data_ptr(), rows, mpad, c, sums_b.data_ptr(), L.stream_ptr()), "rank 1 sums")
    glob = sums2.clone()
    glob[:2 * c] += sums_b[:2 * c]
    o3 = outs()
    L.check(L.lib.gsd_bn_finalize(glob.data_ptr(), c, 2 * count, gamma.data_ptr(), beta.data_ptr(), eps, mom, o3[4].data_ptr(),
                                  o3[5].data_ptr(), o3[0].data_ptr(), o3[1].data_ptr(), o3[2].data_ptr(), o3[3].data_ptr(), None,
                                  L.stream_ptr()), "bn_finalize (SyncBN)")
    check(o3, None, (s1 + t1, s2 + t2, b1 + d1, b2 + d2, 2 * count), f"{tag} SyncBN")


@pytest.mark.parametrize("lvl", range(5))
def test_bn_backward_finalize_paths(L, lvl):
    """gsd_bn_bwd_finalize with sums_global != sums_local (c1, c2 from the global sums, dgamma, dbeta, dW_out from the local
    ones; each one fp32 rounding of an fp64 value: bit-equal), and gsd_bn_bwd_reduce_finalize in both layouts (the reduce
    kernels' 3C rows and a dX epilogue's 2 x mpad rows) at the level's real row counts against fp64."""
    c, h, w = DIMS[lvl], HS[lvl], WS[lvl]
    g = gen(1500 + lvl)
    count = float(N * h * w)
    sl = torch.randn(65 * 3 * c, generator=g, device="cuda", dtype=torch.float64)
    sg = torch.randn(65 * 3 * c, generator=g, device="cuda", dtype=torch.float64) * 3
    o = [torch.full((c,), float("nan"), device="cuda") for _ in range(5)]
    L.check(L.lib.gsd_bn_bwd_finalize(sl.data_ptr(), sg.data_ptr(), c, count, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                      o[3].data_ptr(), o[4].data_ptr(), L.stream_ptr()), "bn_bwd_finalize")
    exp = [sl[c:2 * c], sl[:c], sl[2 * c:3 * c], sg[:c] / count, sg[c:2 * c] / count]
    for name, got, e in zip(("dgamma", "dbeta", "dwout", "c1", "c2"), o, exp):
        assert torch.equal(got, e.float()), f"L{lvl} bn_bwd_finalize {name}"
    for layout in ("reduce", "epilogue"):
        if layout == "reduce":
            rows, mpad, ld = L.lib.gsd_bn_bwd_partial_rows(N, c, h, w), 0, 3 * c
        else:
            from gelslim_depth_amd.engine import _ConvForm
            co = DIMS[min(lvl + 1, 4)]
            rows = _ConvForm.choose(N, h, w, co, co, c, True).partial_rows(N, h, w, c)
            mpad = (c + 63) // 64 * 64
            ld = 2 * mpad
        part = torch.randn((rows, ld), generator=g, device="cuda") * 1e-3
        cols = [part[:, :c].double(), part[:, (mpad or c):(mpad or c) + c].double()]
        if layout == "reduce":
            cols.append(part[:, 2 * c:3 * c].double())
        sums = torch.full((65 * 3 * c,), float("nan"), dtype=torch.float64, device="cuda")
        o = [torch.full((c,), float("nan"), device="cuda") for _ in range(5)]
        L.check(L.lib.gsd_bn_bwd_reduce_finalize(part.data_ptr(), rows, mpad, c, sums.data_ptr(), count, o[0].data_ptr(),
                                                 o[1].data_ptr(), o[2].data_ptr() if layout == "reduce" else None,
                                                 o[3].data_ptr(), o[4].data_ptr(), L.stream_ptr()), "bn_bwd_reduce_finalize")
        what = f"L{lvl} bn_bwd_reduce_finalize ({layout})"
        ref = [x.sum(0) for x in cols]
        bnd = [x.abs().sum(0) for x in cols]
        for k in range(len(cols)):
            R.check_sums(sums[k * c:(k + 1) * c], ref[k], bnd[k], R.TAU_STATS, f"{what} sums[{k}]", key=f"pw-stats:L{lvl}")
        R.check_bound_rounded(o[1], ref[0], bnd[0], R.TAU_STATS, f"{what} dbeta", key=f"pw-bn:L{lvl}")
        R.check_bound_rounded(o[0], ref[1], bnd[1], R.TAU_STATS, f"{what} dgamma", key=f"pw-bn:L{lvl}")
        R.check_bound_rounded(o[3], ref[0] / count, bnd[0] / count, R.TAU_STATS, f"{what} c1", key=f"pw-bn:L{lvl}")
        R.check_bound_rounded(o[4], ref[1] / count, bnd[1] / count, R.TAU_STATS, f"{what} c2", key=f"pw-bn:L{lvl}")
        if layout == "reduce":
            R.check_bound_rounded(o[2], ref[2], bnd[2], R.TAU_STATS, f"{what} dW_out", key=f"pw-bn:L{lvl}")
        else:
            assert bool(o[2].isnan().all()), f"{what}: dW_out written without a third column block"


def test_bn_eval_coeffs(L):
    """gsd_bn_eval_coeffs and gsd_bn_eval_coeffs_bwd for every channel count of the network: scale = gamma / sqrt(rv + eps),
    shift = beta - rm * scale and invstd against fp64 (three fp32 roundings each); the backward form's mean IS the running
    mean, bit for bit, and its scale / shift are the forward form's bits."""
    for c in DIMS:
        g = gen(1600 + c)
        gamma, beta, rm, rv = uniform(g, 0.5, 1.5, c), randn(g, c, scale=0.3), randn(g, c, scale=2.0), uniform(g, 1e-4, 5.0, c)
        o = [torch.full((c,), float("nan"), device="cuda") for _ in range(6)]
        L.check(L.lib.gsd_bn_eval_coeffs(gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5, c, o[0].data_ptr(),
                                         o[1].data_ptr(), L.stream_ptr()), "bn_eval_coeffs")
        L.check(L.lib.gsd_bn_eval_coeffs_bwd(gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5, c,
                                             o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), o[5].data_ptr(), L.stream_ptr()),
                "bn_eval_coeffs_bwd")
        istd = 1.0 / torch.sqrt(rv.double() + R.f32c(1e-5))
        sc = gamma.double() * istd
        sh = beta.double() - rm.double() * sc
        R.check_bound(o[0], sc, sc.abs(), R.TAU_PW, f"C{c} eval scale", key="pw-eval", weights=True)
        R.check_bound(o[1], sh, beta.double().abs() + (rm.double() * sc).abs(), R.TAU_PW, f"C{c} eval shift", key="pw-eval",
                      weights=True)
        R.check_bound(o[5], istd, istd, R.TAU_PW, f"C{c} eval invstd", key="pw-eval", weights=True)
        assert torch.equal(o[4], rm), f"C{c}: eval mean is not the running mean"
        assert torch.equal(o[2], o[0]) and torch.equal(o[3], o[1]), f"C{c}: eval_coeffs_bwd scale / shift differ"


# ------------------------------------------------------------------------------------------------------------- Adam + EMA
def _arena_numel():
    from gelslim_depth_amd.models.unet import UNet
    return sum(p.numel() for p in UNet(n_channels=3, n_classes=1, layer_dimensions=DIMS).parameters())


ADAM = [(1, True), (2, False), (1000, True)]


@pytest.mark.parametrize("step,with_ema", ADAM, ids=[f"step{s}-{'ema' if e else 'noema'}" for s, e in ADAM])
def test_adam_ema_arena(L, step, with_ema):
    """gsd_adam_ema over the real arena size (TrainStep.numel: the grid-stride loop runs past 4096 x 256 elements) with coupled
    L2 at weight_decay 0.1 and grad_scale 1/2, against adam_ema_ref element by element; dropping the weight decay must be
    rejected, and nothing may be written past the arena."""
    numel = _arena_numel()
    assert numel > 4096 * 256
    g = gen(1700 + step)
    wd, gs, d = 0.1, 0.5, min(0.995, (1.0 + step) / (10.0 + step))
    bufs = {}
    init = {"p": randn(g, numel, scale=0.05), "g": randn(g, numel, scale=1e-3) * torch.rand(numel, generator=g, device="cuda"),
            "m": randn(g, numel, scale=1e-4), "v": torch.rand(numel, generator=g, device="cuda") * 1e-7}
    init["ema"] = init["p"] + randn(g, numel, scale=1e-3)
    t = {}
    for k, v in init.items():
        bufs[k], t[k] = buffer((numel,), 0.0)
        t[k].copy_(v)
    L.check(L.lib.gsd_adam_ema(t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(),
                               t["ema"].data_ptr() if with_ema else None, numel, step, 1e-3, 0.9, 0.999, 1e-8, wd, d, gs, None,
                               L.stream_ptr()), "adam_ema")
    for k in t:
        tail_ok(bufs[k], numel, 0, f"adam {k}")
    ref = R.adam_ema_ref(init["p"], init["g"], init["m"], init["v"], init["ema"] if with_ema else None, step, 1e-3,
                         weight_decay=wd, ema_decay=d, grad_scale=gs)
    tag = f"step{step}"
    for k in ("p", "m", "v") + (("ema",) if with_ema else ()):
        R.check_bound(t[k], *ref[k], R.TAU_ADAM, f"{tag} adam {k}", key=f"pw-adam:{tag}", weights=True)
    if not with_ema:
        assert torch.equal(t["ema"], init["ema"])
    assert torch.equal(t["g"], init["g"])
    bad = R.adam_ema_ref(init["p"], init["g"], init["m"], init["v"], None, step, 1e-3, weight_decay=0.0, grad_scale=gs)
    rejects(R.check_bound, bad["p"][0].float(), *ref["p"], R.TAU_ADAM, f"{tag} p without weight decay", weights=True)


def test_adam_ema_guard_skips_a_bad_step(L):
    """A guard whose tick marks the step bad: nothing changes (p, m, v, ema bit-identical) and the skip counter goes up by one."""
    numel = _arena_numel()
    g = gen(1800)
    t = {k: randn(g, numel, scale=1e-2) for k in ("p", "g", "m", "ema")}
    t["v"] = torch.rand(numel, generator=g, device="cuda") * 1e-6
    before = {k: v.clone() for k, v in t.items()}
    words = torch.tensor([7, 3], dtype=torch.int32, device="cuda")
    guard = L.make_guard(words, 7)
    L.check(L.lib.gsd_adam_ema(t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["ema"].data_ptr(),
                               numel, 3, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.995, 1.0, guard, L.stream_ptr()), "adam_ema (guarded)")
    torch.cuda.synchronize()
    for k in t:
        assert torch.equal(t[k], before[k]), f"guarded step changed {k}"
    assert words.tolist() == [7, 4]
    # a guard whose tick is not the marked one lets the step through
    words2 = torch.tensor([6, 0], dtype=torch.int32, device="cuda")
    L.check(L.lib.gsd_adam_ema(t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["ema"].data_ptr(),
                               numel, 3, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.995, 1.0, L.make_guard(words2, 7), L.stream_ptr()),
            "adam_ema (guard clear)")
    torch.cuda.synchronize()
    assert not torch.equal(t["p"], before["p"]) and words2.tolist() == [6, 0]
