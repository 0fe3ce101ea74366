"""Element-wise fp64 bounds for the fp32 engine's kernels at the batches the product runs.

Every conv3x3 unit of BASELINE.json's network ([64,128,256,512,1024] @ 3x320x427), the first layer, the four transposed
convolutions and the output conv + MSE loss, launched exactly as gelslim_depth_amd/engine.py launches them at N = 8, 32 (and 64
at the 40x53 / 20x26 levels): the form _ConvForm.choose picks for the shape, its K-slab scratch where the form asks for one, the
deferred BatchNorm+ReLU sources with slack, the two-segment decoder source with its F.pad offset, the pitched d_raw, the fused
BatchNorm-backward dX epilogue, the two cropped dX destinations and the statistics epilogues.  Every output element of every
image is held to |got - ref| <= tau * cond against tests/fp64_ref.py (fp64 on the GPU, same fp32 operands).  At N = 32 the
other Winograd form is checked too (forced), and the eval-mode forward at N = 16 (BASELINE configs[1]).

A global relative-L1 metric cannot see one wrong 2x4 tile, one garbage halo row or one wrong image of a 32-image batch; a
per-element bound can, and each conv3x3 case proves it at its real shape: after the real check passes, the largest single
product is removed from an edge pixel of the last image of the forward output (a copy), and one image row's fp64 contribution
from dW, and check_bound must reject both.

GSD_FP64_REPORT=<path>: write the worst ratio per case, the module's wall time and peak device memory there as JSON.
"""
import ctypes as C
import json
import os
import time
import zlib

import pytest
import torch

import fp64_ref as R
from test_gpu_layer_shapes import HS, UNITS, WS, gsd, layout  # noqa: F401  (gsd: the module fixture)

pytestmark = pytest.mark.gpu

BUDGET = 1 << 26       # fp64 elements per image chunk of a reference tensor (512 MiB)
T0 = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    torch.cuda.reset_peak_memory_stats()
    T0["t"] = time.time()
    yield
    path = os.environ.get("GSD_FP64_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"wall_s": time.time() - T0["t"], "max_memory_allocated": torch.cuda.max_memory_allocated(),
                       "ratios": dict(sorted(R.RATIOS.items()))}, f, indent=1)


def _r64(c):
    return (c + 63) // 64 * 64


def chunks(n, per_image):
    step = max(1, BUDGET // per_image)
    for i in range(0, n, step):
        yield i, min(n, i + step)


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def slack_randn(gsd, shape, g):
    t = gsd.slack_empty(shape, "cuda")
    t.normal_(generator=g)
    return t


def randn(g, *shape, scale=1.0):
    return torch.randn(shape, generator=g, device="cuda") * scale


def uniform(g, lo, hi, *shape):
    return torch.rand(shape, generator=g, device="cuda") * (hi - lo) + lo


def vec(t):
    return t.double().view(1, -1, 1, 1)


def rejects(got, ref, cond, tau, what, weights=False):
    with pytest.raises(AssertionError):
        R.check_bound(got, ref, cond, tau, what, weights=weights)


def sums(gsd, part, rows, mpad, c):
    s = torch.zeros(65 * 2 * c, device="cuda", dtype=torch.float64)
    gsd.check(gsd.lib.gsd_bn_reduce_partials(part.data_ptr(), rows, mpad, c, s.data_ptr(), gsd.stream_ptr()))
    return s[:c], s[c:2 * c]


def forward_mutation_rejected(a_last, w64, y_last, ref, cond, tau, what):
    """Subtract the largest single product from the bottom-right corner pixel of channel 0 of the last image (a copy of the
    kernel's output) and require check_bound to reject it."""
    h, w = a_last.shape[2], a_last.shape[3]
    win = torch.nn.functional.pad(a_last, [1, 1, 1, 1])[0, :, h - 1:h + 2, w - 1:w + 2]
    prods = w64[0] * win
    k = int(prods.abs().reshape(-1).argmax())
    p = prods.reshape(-1)[k]
    assert float(p.abs()) > 0
    got = y_last.double().clone()
    got[0, 0, h - 1, w - 1] -= p
    rejects(got.float(), ref, cond, tau, f"{what}: largest product removed")


def dw_mutation_rejected(a_last, dy_last, dw, ref, cond, tau, what):
    """Subtract the fp64 contribution of one image row of the last image (the row whose removal shows most) from a copy of dW."""
    rows = R.conv3x3_dw_rows(a_last, dy_last)
    r = int((rows.abs() / cond.clamp_min(1e-300)).reshape(rows.shape[0], -1).amax(1).argmax())
    rejects((dw.double() - rows[r]).float(), ref, cond, tau, f"{what}: row {r} of the last image removed", weights=True)


# ------------------------------------------------------------------------------------------------------------ conv3x3
TRAIN = [(u, n) for n in (8, 32) for u in UNITS] + [(u, 64) for u in UNITS if u[1] >= 3]
CASES = [(u, n, "train") for u, n in TRAIN] + [(u, 32, "other") for u in UNITS] + [(u, 16, "eval") for u in UNITS]


def _form(n, h, w, cin, c0, cout, mode):
    from gelslim_depth_amd.engine import _ConvForm
    f = _ConvForm.choose(n, h, w, cin, c0, cout, mode != "eval")
    if mode == "other":
        assert f.algo in (1, 2), "every unit at N = 32 runs a Winograd form"
        f = _ConvForm(3 - f.algo)
    return f


@pytest.mark.parametrize("unit,n,mode", CASES, ids=[f"{u[0]}-N{n}-{m}" for u, n, m in CASES])
def test_conv3x3_unit_fp64_bound(gsd, unit, n, mode):
    """mode: train (the engine's forms; forward + statistics, dX, dW), other (the other Winograd form forced, forward + dX),
    eval (the eval-mode forward form, no statistics, no K slabs)."""
    name, lvl, c0, c1, co, pooled = unit
    h, w = HS[lvl], WS[lvl]
    ci = c0 + c1
    L = gsd.lib
    st = gsd.stream_ptr()
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(name.encode()) % 10000 + n)
    tag = f"{name}-N{n}-{mode}"

    # ---- operands as the engine holds them
    raw0 = slack_randn(gsd, (n, c0, h, w), g)
    if pooled:
        sc = sh = None
        segs = [gsd.make_src(raw0, slack=gsd.SLACK)]
    else:
        sc, sh = uniform(g, 0.5, 1.5, c0), randn(g, c0, scale=0.3)
        segs = [gsd.make_src(raw0, sc, sh, relu=True, slack=gsd.SLACK)]
    up = top = left = None
    if c1:
        uh, uw = 2 * HS[lvl + 1], 2 * WS[lvl + 1]
        up = slack_randn(gsd, (n, c1, uh, uw), g)
        top, left = (h - uh) // 2, (w - uw) // 2
        segs.append(gsd.make_src(up, off=(top, left), slack=gsd.SLACK))
    wd = randn(g, co, ci, 3, 3, scale=1.0 / (9 * ci) ** 0.5)
    w64 = wd.double()
    src = gsd.src_array(segs)

    def act(i, j):
        a0 = raw0[i:j].double() if pooled else R.deferred_act(raw0[i:j], sc, sh)
        return R.decoder_src(a0, up[i:j].double(), h, w)[0] if c1 else a0

    # ---- forward (+ BatchNorm partial sums in train mode)
    form = _form(n, h, w, ci, c0, co, mode)
    tau = R.TAU_WINO if form.algo else R.TAU_DIRECT
    assert tau <= R.ceiling(ci)
    fam = ("direct", "w43", "w2d")[form.algo]
    wsz = form.workspace(n, h, w, ci, co) if mode != "eval" else 0
    ws = torch.empty(wsz, device="cuda") if wsz > 0 else None
    y = nan(n, co, h, w)
    rows = form.partial_rows(n, h, w, co)
    part = torch.zeros(rows * 2 * _r64(co), device="cuda") if mode != "eval" else None
    gsd.check(form.run(ws, src, len(segs), layout(gsd, form.mode_f, wd, co, ci).data_ptr(), ci, co,
                       gsd.dst_array([gsd.make_dst(y)]), 1, gsd.ptr(part), n, h, w, st), "conv3x3")
    s1 = torch.zeros(co, dtype=torch.float64, device="cuda")
    s2, b1, b2 = s1.clone(), s1.clone(), s1.clone()
    for i, j in chunks(n, max(ci, co) * h * w):
        a = act(i, j)
        ref, cond = R.conv3x3_fwd(a, w64)
        R.check_bound(y[i:j], ref, cond, tau, f"{tag} forward ({fam})", n0=i, image=n - 1, key=f"fwd-{fam}:{tag}")
        s1 += ref.sum((0, 2, 3))
        s2 += (ref * ref).sum((0, 2, 3))
        b1 += cond.sum((0, 2, 3))
        b2 += (cond * cond).sum((0, 2, 3))
        if j == n:
            forward_mutation_rejected(a[-1:], w64, y[n - 1:n], ref[-1:], cond[-1:], tau, f"{tag} forward")
        del a, ref, cond
    if part is not None:
        g1, g2 = sums(gsd, part, rows, _r64(co), co)
        R.check_sums(g1, s1, b1, R.TAU_STATS, f"{tag} forward sum", key=f"stats:{tag}")
        R.check_sums(g2, s2, b2, R.TAU_STATS, f"{tag} forward sum of squares", key=f"stats:{tag}")
    del y, part, ws
    if mode == "eval":
        return

    # ---- dX, in the form the engine launches for this unit, from d_raw as the engine holds it (pitched for Winograd dX + dW)
    form_d = _form(n, h, w, co, co, ci, mode)
    tau_d = R.TAU_WINO if form_d.algo else R.TAU_DIRECT
    assert tau_d <= R.ceiling(co)
    fam_d = ("direct", "w43", "w2d")[form_d.algo]
    pitched = bool(L.gsd_conv3x3_wgrad_takes_pitched_dy(n, h, w, ci, co)) and form_d.algo >= 1
    dy = torch.zeros((n, co, h, (w + 3) // 4 * 4), device="cuda")[..., :w] if pitched else torch.empty((n, co, h, w), device="cuda")
    dy.copy_(randn(g, n, co, h, w))
    wl_d = layout(gsd, form_d.mode_d, wd, co, ci)
    wsz = form_d.workspace(n, h, w, co, ci)
    ws = torch.empty(wsz, device="cuda") if wsz > 0 else None
    rows_d = form_d.partial_rows(n, h, w, ci)
    mp = _r64(ci)
    key_d = f"dx-{fam_d}:{tag}"
    if c1:        # decoder c0: skip gradient | cropped gradient of the up-sampled tensor, + ConvT bias grad from its statistics
        g_skip = nan(n, c0, h, w)
        g_up = gsd.slack_empty((n, c1, uh, uw), "cuda").fill_(float("nan"))     # as the engine allocates up.dout
        stats = form_d.algo >= 1
        part_d = torch.zeros(rows_d * 2 * mp, device="cuda") if stats else None
        gsd.check(form_d.run(ws, gsd.src_array([gsd.make_src(dy)]), 1, wl_d.data_ptr(), co, ci,
                             gsd.dst_array([gsd.make_dst(g_skip), gsd.make_dst(g_up, off=(top, left))]), 2, gsd.ptr(part_d),
                             n, h, w, st), "dX")
        db_ref = torch.zeros(c1, dtype=torch.float64, device="cuda")
        db_b = db_ref.clone()
        for i, j in chunks(n, max(ci, co) * h * w):
            ref, cond = R.conv3x3_dx(dy[i:j].double(), w64)
            R.check_bound(g_skip[i:j], ref[:, :c0], cond[:, :c0], tau_d, f"{tag} dX skip ({fam_d})", n0=i, key=key_d)
            ru, cu = ref[:, c0:, top:top + uh, left:left + uw], cond[:, c0:, top:top + uh, left:left + uw]
            R.check_bound(g_up[i:j], ru, cu, tau_d, f"{tag} dX up, cropped ({fam_d})", n0=i, key=key_d)
            db_ref += ru.sum((0, 2, 3))
            db_b += cu.sum((0, 2, 3))
            del ref, cond, ru, cu
        if stats:
            db = nan(c1)
            sc_ = torch.zeros(65 * 2 * ci, device="cuda", dtype=torch.float64)
            gsd.check(L.gsd_partials_channel_sums(part_d.data_ptr(), rows_d, mp, ci, c0, c1, db.data_ptr(), sc_.data_ptr(), st))
            R.check_sums(db, db_ref, db_b, R.TAU_STATS, f"{tag} ConvT bias grad from dX statistics", key=f"stats:{tag}")
        del g_skip, g_up, part_d
    elif pooled:  # encoder c0 below level 0: plain dX into the pooled tensor's gradient
        gx = nan(n, ci, h, w)
        gsd.check(form_d.run(ws, gsd.src_array([gsd.make_src(dy)]), 1, wl_d.data_ptr(), co, ci, gsd.dst_array([gsd.make_dst(gx)]),
                             1, None, n, h, w, st), "dX")
        for i, j in chunks(n, max(ci, co) * h * w):
            ref, cond = R.conv3x3_dx(dy[i:j].double(), w64)
            R.check_bound(gx[i:j], ref, cond, tau_d, f"{tag} dX ({fam_d})", n0=i, key=key_d)
            del ref, cond
        del gx
    else:         # c1 of a DoubleConv: dX fused with the backward of the producer's ReLU + BatchNorm pass-1 sums
        mean, invstd = randn(g, c0, scale=0.3), uniform(g, 0.5, 2.0, c0)
        dz = nan(n, ci, h, w)
        part_d = torch.zeros(rows_d * 2 * mp, device="cuda")
        s, d = gsd.make_src(dy), gsd.make_dst(dz)
        gsd.check(form_d.run_bnrelu(ws, C.byref(s), wl_d.data_ptr(), co, ci, C.byref(d), raw0.data_ptr(), sc.data_ptr(),
                                    sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(), part_d.data_ptr(), n, h, w, st), "fused dX")
        t1 = torch.zeros(ci, dtype=torch.float64, device="cuda")
        t2, u1, u2 = t1.clone(), t1.clone(), t1.clone()
        for i, j in chunks(n, max(ci, co) * h * w):
            ref, cond = R.conv3x3_dx(dy[i:j].double(), w64)
            m = R.bnrelu_mask(raw0[i:j], sc, sh)
            ref, cond = ref * m, cond * m
            R.check_bound(dz[i:j], ref, cond, tau_d, f"{tag} dX fused ({fam_d})", n0=i, key=key_d)
            xhat = (raw0[i:j].double() - vec(mean)) * vec(invstd)
            t1 += ref.sum((0, 2, 3))
            t2 += (ref * xhat).sum((0, 2, 3))
            u1 += cond.sum((0, 2, 3))
            u2 += (cond * xhat.abs()).sum((0, 2, 3))
            del ref, cond, m, xhat
        q1, q2 = sums(gsd, part_d, rows_d, mp, ci)
        R.check_sums(q1, t1, u1, R.TAU_STATS, f"{tag} fused dX sum dz", key=f"stats:{tag}")
        R.check_sums(q2, t2, u2, R.TAU_STATS, f"{tag} fused dX sum dz*xhat", key=f"stats:{tag}")
        del dz, part_d
    del ws
    if mode != "train":
        return

    # ---- dW: activation segments as in the forward, dy as the engine holds it
    need = L.gsd_conv3x3_wgrad_workspace(n, h, w, ci, co)
    wws = torch.zeros(need, device="cuda")
    dw = nan(co, ci, 3, 3)
    dy_src = gsd.make_src(dy)
    gsd.check(L.gsd_conv3x3_wgrad(src, len(segs), C.byref(dy_src), ci, co, dw.data_ptr(), wws.data_ptr(), need, n, h, w, st))
    ref = torch.zeros((co, ci, 3, 3), dtype=torch.float64, device="cuda")
    cond = torch.zeros_like(ref)
    for i, j in chunks(n, max(ci, co) * h * w):
        r_, c_ = R.conv3x3_dw(act(i, j), dy[i:j].double())
        ref += r_
        cond += c_
        del r_, c_
    R.check_bound(dw, ref, cond, R.TAU_DW, f"{tag} dW", key=f"dw:{tag}", weights=True)
    dw_mutation_rejected(act(n - 1, n), dy[n - 1:n].double(), dw, ref, cond, R.TAU_DW, f"{tag} dW")


FIRST = [(8, "train"), (32, "train"), (16, "eval")]


@pytest.mark.parametrize("n,mode", FIRST, ids=[f"N{n}-{m}" for n, m in FIRST])
def test_first_layer_fp64_bound(gsd, n, mode):
    """inc.c0 (3 -> 64 @320x427): the forward in the engine's form (+ statistics), and in train mode the dW kernel that forms
    d_raw = scale * (dz - c1 - (raw - mean) * invstd * c2) itself (gsd_conv3x3_wgrad_bn; no dX: the input is the image)."""
    L = gsd.lib
    st = gsd.stream_ptr()
    ci, co, h, w = 3, 64, HS[0], WS[0]
    g = torch.Generator(device="cuda").manual_seed(1000 + n)
    tag = f"inc.c0-N{n}-{mode}"
    x = torch.rand((n, ci, h, w), generator=g, device="cuda")
    wd = randn(g, co, ci, 3, 3, scale=0.2)
    w64 = wd.double()
    form = _form(n, h, w, ci, ci, co, mode)
    tau = R.TAU_WINO if form.algo else R.TAU_DIRECT
    fam = ("direct", "w43", "w2d")[form.algo]
    wsz = form.workspace(n, h, w, ci, co) if mode != "eval" else 0
    ws = torch.empty(wsz, device="cuda") if wsz > 0 else None
    src = gsd.src_array([gsd.make_src(x)])
    y = nan(n, co, h, w)
    rows = form.partial_rows(n, h, w, co)
    part = torch.zeros(rows * 2 * 64, device="cuda") if mode != "eval" else None
    gsd.check(form.run(ws, src, 1, layout(gsd, form.mode_f, wd, co, ci).data_ptr(), ci, co, gsd.dst_array([gsd.make_dst(y)]), 1,
                       gsd.ptr(part), n, h, w, st), "conv3x3")
    s1 = torch.zeros(co, dtype=torch.float64, device="cuda")
    s2, b1, b2 = s1.clone(), s1.clone(), s1.clone()
    for i, j in chunks(n, co * h * w):
        ref, cond = R.conv3x3_fwd(x[i:j].double(), w64)
        R.check_bound(y[i:j], ref, cond, tau, f"{tag} forward ({fam})", n0=i, image=n - 1, key=f"fwd-{fam}:{tag}")
        s1 += ref.sum((0, 2, 3))
        s2 += (ref * ref).sum((0, 2, 3))
        b1 += cond.sum((0, 2, 3))
        b2 += (cond * cond).sum((0, 2, 3))
        if j == n:
            forward_mutation_rejected(x[n - 1:n].double(), w64, y[n - 1:n], ref[-1:], cond[-1:], tau, f"{tag} forward")
        del ref, cond
    if mode == "eval":
        return
    g1, g2 = sums(gsd, part, rows, 64, co)
    R.check_sums(g1, s1, b1, R.TAU_STATS, f"{tag} forward sum", key=f"stats:{tag}")
    R.check_sums(g2, s2, b2, R.TAU_STATS, f"{tag} forward sum of squares", key=f"stats:{tag}")

    assert L.gsd_conv3x3_wgrad_bn_supported(n, h, w, ci, co) == 1
    dz = randn(g, n, co, h, w)
    sc, mu = uniform(g, 0.5, 1.5, co), randn(g, co, scale=0.3)
    istd, k1, k2 = uniform(g, 0.5, 2.0, co), randn(g, co, scale=0.1), randn(g, co, scale=0.1)
    need = L.gsd_conv3x3_wgrad_bn_workspace(n, h, w, ci, co)
    wws = torch.zeros(need, device="cuda")
    dw = nan(co, ci, 3, 3)
    a_src = gsd.make_src(x)
    gsd.check(L.gsd_conv3x3_wgrad_bn(C.byref(a_src), dz.data_ptr(), y.data_ptr(), sc.data_ptr(), mu.data_ptr(), istd.data_ptr(),
                                     k1.data_ptr(), k2.data_ptr(), ci, co, dw.data_ptr(), wws.data_ptr(), need, n, h, w, st))

    def d_raw(i, j):
        """d_raw in fp64 and the magnitude bound of its fp32 evaluation in the kernel: scale * (|dz| + |c1| + |xhat c2|)."""
        t = (y[i:j].double() - vec(mu)) * vec(istd) * vec(k2)
        return (vec(sc) * (dz[i:j].double() - vec(k1) - t),
                vec(sc) * (dz[i:j].double().abs() + vec(k1).abs() + t.abs()))
    ref = torch.zeros((co, ci, 3, 3), dtype=torch.float64, device="cuda")
    cond = torch.zeros_like(ref)
    for i, j in chunks(n, co * h * w):
        d, da = d_raw(i, j)
        r_, c_ = R.conv3x3_dw(x[i:j].double(), d, da)
        ref += r_
        cond += c_
        del d, da, r_, c_
    R.check_bound(dw, ref, cond, R.TAU_DW, f"{tag} dW (BatchNorm backward on the fly)", key=f"dw:{tag}", weights=True)
    dw_mutation_rejected(x[n - 1:n].double(), d_raw(n - 1, n)[0], dw, ref, cond, R.TAU_DW, f"{tag} dW")


# ---------------------------------------------------------------------------------------------------------------- ConvT
CONVT = [("up0.up", 4, 1024), ("up1.up", 3, 512), ("up2.up", 2, 256), ("up3.up", 1, 128)]
CONVT_CASES = [(c, n) for n in (8, 32) for c in CONVT]


@pytest.mark.parametrize("case,n", CONVT_CASES, ids=[f"{c[0]}-N{n}" for c, n in CONVT_CASES])
def test_convT_fp64_bound(gsd, case, n):
    """ConvTranspose2d(Cin, Cin/2, 2, 2) of the four decoder levels: forward (+bias) from a deferred BatchNorm+ReLU source, dX
    (fused with the producer's ReLU + BatchNorm pass-1 sums where the engine fuses it), dW and the bias gradient."""
    name, lvl, ci = case
    L = gsd.lib
    st = gsd.stream_ptr()
    co, h, w = ci // 2, HS[lvl], WS[lvl]
    g = torch.Generator(device="cuda").manual_seed(ci + n)
    tag = f"{name}-N{n}"
    raw = slack_randn(gsd, (n, ci, h, w), g)
    sc, sh = uniform(g, 0.5, 1.5, ci), randn(g, ci, scale=0.3)
    wd, bd = randn(g, ci, co, 2, 2, scale=1.0 / ci ** 0.5), randn(g, co)
    w64, b64 = wd.double(), bd.double()
    s = gsd.make_src(raw, sc, sh, relu=True, slack=gsd.SLACK)
    y = gsd.slack_empty((n, co, 2 * h, 2 * w), "cuda").fill_(float("nan"))
    d = gsd.make_dst(y)
    gsd.check(L.gsd_convT2x2(C.byref(s), layout(gsd, 6, wd, co, ci).data_ptr(), bd.data_ptr(), ci, co, C.byref(d), n, h, w, st))
    per = max(ci * h * w, co * 4 * h * w)
    for i, j in chunks(n, per):
        ref, cond = R.convT_fwd(R.deferred_act(raw[i:j], sc, sh), w64, b64)
        R.check_bound(y[i:j], ref, cond, R.TAU_CONVT, f"{tag} forward", n0=i, key=f"convT:{tag}")
        del ref, cond
    del y

    dy = slack_randn(gsd, (n, co, 2 * h, 2 * w), g)       # as the engine allocates up.dout
    sdy = gsd.make_src(dy, slack=gsd.SLACK)
    mode = L.gsd_convT2x2_dgrad_layout(C.byref(sdy), ci, co, n, h, w)
    bn_rows = L.gsd_convT2x2_dgrad_bnrelu_partial_rows(C.byref(sdy), ci, co, n, h, w) if mode == 7 else 0
    wl_d = layout(gsd, mode, wd, co, ci)
    dx = nan(n, ci, h, w)
    ddx = gsd.make_dst(dx)
    mean, invstd = randn(g, ci, scale=0.3), uniform(g, 0.5, 2.0, ci)
    if bn_rows:
        part = torch.zeros(bn_rows * 2 * _r64(ci), device="cuda")
        gsd.check(L.gsd_convT2x2_dgrad_bnrelu(C.byref(sdy), wl_d.data_ptr(), ci, co, C.byref(ddx), raw.data_ptr(), sc.data_ptr(),
                                              sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(), part.data_ptr(), n, h, w, st))
    else:
        gsd.check(L.gsd_convT2x2_dgrad_as(mode, C.byref(sdy), wl_d.data_ptr(), ci, co, C.byref(ddx), n, h, w, st))
    t1 = torch.zeros(ci, dtype=torch.float64, device="cuda")
    t2, u1, u2 = t1.clone(), t1.clone(), t1.clone()
    for i, j in chunks(n, per):
        ref, cond = R.convT_dx(dy[i:j].double(), w64)
        if bn_rows:
            m = R.bnrelu_mask(raw[i:j], sc, sh)
            ref, cond = ref * m, cond * m
            xhat = (raw[i:j].double() - vec(mean)) * vec(invstd)
            t1 += ref.sum((0, 2, 3))
            t2 += (ref * xhat).sum((0, 2, 3))
            u1 += cond.sum((0, 2, 3))
            u2 += (cond * xhat.abs()).sum((0, 2, 3))
            del m, xhat
        R.check_bound(dx[i:j], ref, cond, R.TAU_CONVT, f"{tag} dX{' fused' if bn_rows else ''}", n0=i, key=f"convT:{tag}")
        del ref, cond
    if bn_rows:
        q1, q2 = sums(gsd, part, bn_rows, _r64(ci), ci)
        R.check_sums(q1, t1, u1, R.TAU_STATS, f"{tag} fused dX sum dz", key=f"stats:{tag}")
        R.check_sums(q2, t2, u2, R.TAU_STATS, f"{tag} fused dX sum dz*xhat", key=f"stats:{tag}")
    del dx

    need = L.gsd_convT2x2_wgrad_workspace(n, h, w, ci, co)
    ws = torch.zeros(need, device="cuda")
    dw, db = nan(ci, co, 2, 2), nan(co)
    gsd.check(L.gsd_convT2x2_wgrad(C.byref(s), C.byref(sdy), ci, co, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need, n, h, w, st))
    acc = [torch.zeros((ci, co, 2, 2), dtype=torch.float64, device="cuda")] * 2 + \
          [torch.zeros(co, dtype=torch.float64, device="cuda")] * 2
    for i, j in chunks(n, per):
        part_ = R.convT_dw(R.deferred_act(raw[i:j], sc, sh), dy[i:j].double())
        acc = [a_ + p_ for a_, p_ in zip(acc, part_)]
        del part_
    R.check_bound(dw, acc[0], acc[1], R.TAU_CONVT, f"{tag} dW", key=f"convT:{tag}", weights=True)
    R.check_bound(db, acc[2], acc[3], R.TAU_CONVT, f"{tag} db", key=f"convT:{tag}")


# ------------------------------------------------------------------------------------------------------- output conv
def test_output_conv_and_loss_fp64_bound(gsd):
    """outc (64 -> 1, 1x1 @320x427, N = 32) from the last unit's deferred BatchNorm+ReLU, the MSE loss and its gradient, dX (the
    engine's gsd_bn_bwd_reduce mode OUTC: masked, with the dW_out third sum), dW (gsd_conv1x1_out_wgrad) and db."""
    L = gsd.lib
    st = gsd.stream_ptr()
    n, c, k, h, w = 32, 64, 1, HS[0], WS[0]
    g = torch.Generator(device="cuda").manual_seed(77)
    raw = slack_randn(gsd, (n, c, h, w), g)
    sc, sh = uniform(g, 0.5, 1.5, c), randn(g, c, scale=0.3)
    wd, bd = randn(g, k, c, scale=0.125), randn(g, k)
    w64, b64 = wd.double(), bd.double()
    s = gsd.make_src(raw, sc, sh, relu=True, slack=gsd.SLACK)
    out = nan(n, k, h, w)
    gsd.check(L.gsd_conv1x1_out(C.byref(s), wd.data_ptr(), bd.data_ptr(), c, k, out.data_ptr(), n, h, w, st))
    per = c * h * w
    for i, j in chunks(n, per):
        ref, cond = R.conv1x1_fwd(R.deferred_act(raw[i:j], sc, sh), w64, b64)
        R.check_bound(out[i:j], ref, cond, R.TAU_1X1, "outc forward", n0=i, key="1x1:forward")
        del ref, cond
    tgt = randn(g, n, k, h, w)
    loss, grad = torch.zeros(1, device="cuda"), nan(n, k, h, w)
    lws = torch.zeros(2048, dtype=torch.float64, device="cuda")
    gsd.check(L.gsd_loss_fwd_bwd(0, out.data_ptr(), tgt.data_ptr(), out.numel(), 1.0, loss.data_ptr(), grad.data_ptr(),
                                 lws.data_ptr(), None, st))
    gref, gcond = R.mse_grad(out, tgt, out.numel())
    R.check_bound(grad, gref, gcond, R.TAU_1X1, "MSE gradient", key="1x1:loss")
    lref = ((out.double() - tgt.double()) ** 2).mean().view(1)
    R.check_bound(loss, lref, lref, R.TAU_1X1, "MSE loss", key="1x1:loss")
    g64 = grad.double()

    # dX through the engine's launch: gsd_bn_bwd_reduce(mode 2) leaves dz = (w^T g) * [raw*scale+shift > 0] and sum g*a
    mean, invstd = randn(g, c, scale=0.3), uniform(g, 0.5, 2.0, c)
    dz = nan(n, c, h, w)
    rows = L.gsd_bn_bwd_partial_rows(n, c, h, w)
    part = torch.zeros(rows * 3 * c, device="cuda")
    da = gsd.make_src(dz)
    gsd.check(L.gsd_bn_bwd_reduce(2, raw.data_ptr(), sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(), C.byref(da),
                                  None, grad.data_ptr(), wd.data_ptr(), k, dz.data_ptr(), part.data_ptr(), n, c, h, w, st))
    bsum = torch.zeros(65 * 3 * c, device="cuda", dtype=torch.float64)
    gsd.check(L.gsd_bn_bwd_reduce_partials(part.data_ptr(), rows, c, bsum.data_ptr(), st))
    dw_ref = torch.zeros((k, c), dtype=torch.float64, device="cuda")
    dw_cond, db_ref, db_cond = dw_ref.clone(), torch.zeros(k, dtype=torch.float64, device="cuda"), \
        torch.zeros(k, dtype=torch.float64, device="cuda")
    for i, j in chunks(n, per):
        ref, cond = R.conv1x1_dx(g64[i:j], w64)
        m = R.bnrelu_mask(raw[i:j], sc, sh)
        R.check_bound(dz[i:j], ref * m, cond * m, R.TAU_1X1, "outc dX (masked)", n0=i, key="1x1:dx")
        r_ = R.conv1x1_dw(R.deferred_act(raw[i:j], sc, sh), g64[i:j])
        dw_ref += r_[0]
        dw_cond += r_[1]
        db_ref += r_[2]
        db_cond += r_[3]
        del ref, cond, m, r_
    R.check_bound(bsum[2 * c:3 * c].view(k, c), dw_ref, dw_cond, R.TAU_1X1, "outc dW (gsd_bn_bwd_reduce third sum)", key="1x1:dw")

    dw = nan(k, c)
    wrows = L.gsd_conv1x1_out_wgrad_rows(n, h, w)
    wpart = torch.zeros(wrows * k * c, device="cuda")
    wsums = torch.zeros(65 * k * c, device="cuda", dtype=torch.float64)
    gsd.check(L.gsd_conv1x1_out_wgrad(raw.data_ptr(), sc.data_ptr(), sh.data_ptr(), grad.data_ptr(), c, k, dw.data_ptr(),
                                      wpart.data_ptr(), wsums.data_ptr(), n, h, w, st))
    R.check_bound(dw, dw_ref, dw_cond, R.TAU_1X1, "outc dW (gsd_conv1x1_out_wgrad)", key="1x1:dw")
    db = nan(k)
    pws = torch.zeros(64 * k, device="cuda")
    gsd.check(L.gsd_sum_planes(grad.data_ptr(), n, k, h * w, db.data_ptr(), pws.data_ptr(), st))
    R.check_bound(db, db_ref, db_cond, R.TAU_1X1, "outc db", key="1x1:db")
