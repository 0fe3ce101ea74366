"""Element-wise fp64 bounds for the bf16 engine (gelslim_depth_amd/engine_bf16.py, UNet(precision="bf16"), BASELINE configs[4])
at 320x427 with BASELINE's dims [64, 128, 256, 512, 1024], at the batches the product runs: train N = 16 (configs[4]'s per-GPU
share) and 32 (the bf16 twin of the metric), N = 7 (item counts that are no multiple of the grid or of the 8 XCDs), eval N = 16
and 1.  Which kernel serves a launch is not re-decided here: a real engine's _ensure says (first_direct, fused_inc, _use_c64,
apply_pool, fused_out), and the default fast path must be the one it takes.

Every stored bf16 result is held to |got - ref| <= 2^-8 |ref| + tau * cond (tests/fp64_ref.py: check_bound_bf16), every fp32
result (dW, the output conv) to |got - ref| <= tau * cond, against fp64 on the GPU from the same bf16 operands, at every element
of every image; statistics epilogues against the sums of the values as stored.  Destinations start as NaN; what a launch must
not touch (the other channels of a concat buffer, the F.pad border of an up-slice, the rows past a partials buffer's
*_partial_rows) holds a sentinel and is checked afterwards.  Each conv3x3 / c64 / inc case proves its bound can see a small,
local mistake at its real shape: the largest product removed from an edge pixel of the last image's forward output, one image
row removed from dW -- check_bound(_bf16) must reject both.

The short-XCD-range branch of gconv_bf16_kernel (`an XCD's range can be shorter than its blocks`) is not reachable on a 256-CU
chip by any launch of this network: the grid is min(256, items) with mblocks in {1, 2, 4, 8}; with items >= 256 every XCD's
range holds >= floor(ntile / 8) >= 32 / mblocks tiles = its blocks' lane count, and with items < 256 the XCD order needs
ntile % 8 == 0, which splits the tiles evenly.  N = 7 still puts uneven tile counts on the XCDs (ntile % 8 != 0 at every level).

The last test runs one full-size teacher-forced TrainStep (N = 16, default mode, weight gradients on the side stream) and holds
the engine's own surviving tensors to the same bounds.

GSD_FP64_REPORT_BF16=<path>: write the worst ratio per case, the module's wall time and peak device memory there as JSON.
"""
import ctypes as C
import json
import os
import time
import zlib

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu

DIMS = [64, 128, 256, 512, 1024]
HS = [320, 160, 80, 40, 20]
WS = [427, 213, 106, 53, 26]
T3Y = [t // 3 - 1 for t in range(9)]
T3X = [t % 3 - 1 for t in range(9)]
BUDGET = 1 << 26       # fp64 elements per image chunk of a reference tensor (512 MiB)
TAIL = 4096            # sentinel floats past the partial rows a launch reports
SENT = 12345.0
T0 = {}

# (name, level, Cin, Cout, dX fused with the producer's BatchNorm-backward pass 1, dX writes a concat gradient with statistics)
UNITS = [
    ("inc.c1|up3.c1", 0, 64, 64, True, False),
    ("down0.c0", 1, 64, 128, False, False),
    ("down0.c1|up2.c1", 1, 128, 128, True, False),
    ("down1.c0", 2, 128, 256, False, False),
    ("down1.c1|up1.c1", 2, 256, 256, True, False),
    ("down2.c0", 3, 256, 512, False, False),
    ("down2.c1|up0.c1", 3, 512, 512, True, False),
    ("down3.c0", 4, 512, 1024, False, False),
    ("down3.c1", 4, 1024, 1024, True, False),
    ("up0.c0", 3, 1024, 512, False, True),
    ("up1.c0", 2, 512, 256, False, True),
    ("up2.c0", 1, 256, 128, False, True),
    ("up3.c0", 0, 128, 64, False, True),
]
TRAIN_N = (16, 32, 7)
EVAL_N = (16, 1)


@pytest.fixture(scope="module", autouse=True)
def report():
    torch.cuda.reset_peak_memory_stats()
    T0["t"] = time.time()
    yield
    path = os.environ.get("GSD_FP64_REPORT_BF16")
    if path:
        with open(path, "w") as f:
            json.dump({"wall_s": time.time() - T0["t"], "max_memory_allocated": torch.cuda.max_memory_allocated(),
                       "ratios": dict(sorted((k, v) for k, v in R.RATIOS.items() if k.startswith("bf16")))}, f, indent=1)


@pytest.fixture(scope="module")
def L():
    from gelslim_depth_amd import _lib
    return _lib


_FLAGS = {}


def flags(n, train):
    """What a real bf16 engine at (n, 320, 427) decides in _ensure, and that it is the default fast path."""
    key = (n, train)
    if key not in _FLAGS:
        from gelslim_depth_amd.engine_bf16 import UNetEngineBF16
        eng = UNetEngineBF16(3, 1, DIMS)
        eng._ensure(n, HS[0], WS[0], torch.device("cuda"), train)
        f = dict(first_direct=eng.first_direct, fused_inc=eng.fused_inc, c64=eng._use_c64(64, 64), c64_128=eng._use_c64(128, 64),
                 apply_pool=eng.apply_pool, fused_out=eng.fused_out, side_dw=eng.side_dw)
        del eng
        torch.cuda.empty_cache()
        assert f["first_direct"] and f["c64"] and not f["c64_128"] and f["apply_pool"] and f["fused_out"], f
        assert f["fused_inc"] and f["side_dw"] == train, f
        _FLAGS[key] = f
    return _FLAGS[key]


def chunks(n, per_image):
    step = max(1, BUDGET // per_image)
    for i in range(0, n, step):
        yield i, min(n, i + step)


def nan_bf16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device="cuda")


def rand_bf16(g, *shape, scale=1.0, relu=False):
    t = torch.randn(shape, generator=g, device="cuda") * scale
    return (t.clamp_min(0) if relu else t).to(torch.bfloat16)


def uniform(g, lo, hi, *shape):
    return torch.rand(shape, generator=g, device="cuda") * (hi - lo) + lo


def partials(rows, width):
    """A partials buffer of `rows` rows and a sentinel tail: a launch that writes more rows than it reports shows there."""
    t = torch.full((rows * width + TAIL,), float("nan"), device="cuda")
    t[rows * width:] = SENT
    return t


def tail_ok(part, rows, width, what):
    torch.cuda.synchronize()
    assert bool((part[rows * width:] == SENT).all()), f"{what}: partial rows written past the {rows} reported"


def image(L, mode, w, co, ci):
    img = torch.empty((L.lib.gsd_bf16_weight_image_size(mode, co, ci),), dtype=torch.bfloat16, device="cuda")
    L.check(L.lib.gsd_bf16_weight_image(mode, w.data_ptr(), co, ci, img.data_ptr(), L.stream_ptr()), "weight image")
    return img


def conv_sums(L, part, rows, c):
    s = torch.zeros(65 * 3 * c, dtype=torch.float64, device="cuda")
    L.check(L.lib.gsd_bn_reduce_partials(part.data_ptr(), rows, L.lib.gsd_bf16_conv_mpad(c), c, s.data_ptr(), L.stream_ptr()), "sums")
    return s[:c], s[c:2 * c]


def bwd_sums(L, part, rows, c):
    s = torch.zeros(65 * 3 * c, dtype=torch.float64, device="cuda")
    L.check(L.lib.gsd_bn_bwd_reduce_partials(part.data_ptr(), rows, c, s.data_ptr(), L.stream_ptr()), "bwd sums")
    return s[:c], s[c:2 * c], s[2 * c:3 * c]


def check_stored_sums(got1, got2, y_nhwc, c_off, c, tag, key):
    """A statistics epilogue's (sum, sum of squares) against the sums of the values it stored."""
    acc = [torch.zeros(c, dtype=torch.float64, device="cuda") for _ in range(4)]
    n, h, w = y_nhwc.shape[:3]
    for i, j in chunks(n, c * h * w):
        acc = [a + b for a, b in zip(acc, R.stored_sums(R.nchw(y_nhwc[i:j], c_off, c)))]
    R.check_sums(got1, acc[0], acc[2], R.TAU_BF16_STATS, f"{tag} sum", key=key)
    R.check_sums(got2, acc[1], acc[3], R.TAU_BF16_STATS, f"{tag} sum of squares", key=key)


def check_bwd_sums(q1, q2, dz_nhwc, y_nhwc, mean, invstd, tag, key):
    c = dz_nhwc.shape[3]
    acc = [torch.zeros(c, dtype=torch.float64, device="cuda") for _ in range(4)]
    n, h, w = dz_nhwc.shape[:3]
    for i, j in chunks(n, c * h * w):
        acc = [a + b for a, b in zip(acc, R.bn_bwd_sums(R.nchw(dz_nhwc[i:j]), R.nchw(y_nhwc[i:j]), mean, invstd))]
    R.check_sums(q1, acc[0], acc[2], R.TAU_BF16_STATS, f"{tag} sum dz", key=key)
    R.check_sums(q2, acc[1], acc[3], R.TAU_BF16_STATS, f"{tag} sum dz*xhat", key=key)


def rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def forward_mutation_rejected(a_last, w64, y_last, ref, cond, tau, what):
    """Subtract the largest single product from the bottom-right corner pixel of channel 0 of the last image (a copy of the
    kernel's output, NCHW) and require check_bound_bf16 to reject it."""
    h, w = a_last.shape[2], a_last.shape[3]
    win = torch.nn.functional.pad(a_last, [1, 1, 1, 1])[0, :, h - 1:h + 2, w - 1:w + 2]
    prods = w64[0] * win
    k = int(prods.abs().reshape(-1).argmax())
    p = prods.reshape(-1)[k]
    assert float(p.abs()) > 0
    got = y_last.double().clone()
    got[0, 0, h - 1, w - 1] -= p
    rejects(R.check_bound_bf16, got.float(), ref, cond, tau, f"{what}: largest product removed")


def dw_mutation_rejected(a_last, dy_last, dw, ref, cond, tau, what):
    rows = R.conv3x3_dw_rows(a_last, dy_last)
    r = int((rows.abs() / cond.clamp_min(1e-300)).reshape(rows.shape[0], -1).amax(1).argmax())
    rejects(R.check_bound, (dw.double() - rows[r]).float(), ref, cond, tau, f"{what}: row {r} of the last image removed", weights=True)


def wgrad(L, dy, a, ci, co, n, h, w):
    """gsd_bf16_wgrad as the engine launches it for a conv3x3 unit: (co, ci, 3, 3) fp32."""
    need = L.lib.gsd_bf16_wgrad_workspace(9, n, h, w, co, ci)
    ws = torch.empty((max(need, 64),), device="cuda")
    dw = torch.full((co, ci, 3, 3), float("nan"), device="cuda")
    L.check(L.lib.gsd_bf16_wgrad(C.byref(L.make_nhwc(dy)), C.byref(L.make_nhwc(a)), 9, 1, L.int_array(T3Y), L.int_array(T3X),
                                 dw.data_ptr(), ci, ws.data_ptr(), ws.numel(), L.stream_ptr()), "wgrad")
    return dw


def dw_check(a, dy, dw, tag, key, dy_abs_fn=None):
    """dW of a conv3x3 unit against fp64 over all images, and the row-removal mutation."""
    n = a.shape[0]
    ci, co = a.shape[3], dy.shape[3]
    ref = torch.zeros((co, ci, 3, 3), dtype=torch.float64, device="cuda")
    cond = torch.zeros_like(ref)
    for i, j in chunks(n, max(ci, co) * a.shape[1] * a.shape[2]):
        r_, c_ = R.conv3x3_dw(R.nchw(a[i:j]), R.nchw(dy[i:j]))
        ref += r_
        cond += c_
        del r_, c_
    R.check_bound(dw, ref, cond, R.TAU_BF16_DW, f"{tag} dW", key=key, weights=True)
    dw_mutation_rejected(R.nchw(a[n - 1:n]), R.nchw(dy[n - 1:n]), dw, ref, cond, R.TAU_BF16_DW, f"{tag} dW")


# ------------------------------------------------------------------------------------------------------------ conv3x3 / c64
CASES = [(u, n, "train") for n in TRAIN_N for u in UNITS] + [(u, n, "eval") for n in EVAL_N for u in UNITS]


@pytest.mark.parametrize("unit,n,mode", CASES, ids=[f"{u[0]}-N{n}-{m}" for u, n, m in CASES])
def test_conv3x3_unit_bf16_fp64_bound(L, unit, n, mode):
    """Forward (+ statistics of the stored values), dX (plain, with the fused BatchNorm-backward pass 1 and its sums, or into a
    concat gradient with the statistics the ConvT bias gradient is built from) and dW of one conv3x3 unit, on the kernel the
    engine picks (the weights-resident 64 -> 64 kernel at level 0, the DMA-filled one elsewhere); eval: conv + BatchNorm + ReLU
    in one launch."""
    name, lvl, ci, co, fused, cat_stats = unit
    train = mode == "train"
    fl = flags(n, train)
    h, w = HS[lvl], WS[lvl]
    st = L.stream_ptr()
    lib = L.lib
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(name.encode()) % 10000 + n + (0 if train else 500))
    tag = f"{name}-N{n}-{mode}"
    a = rand_bf16(g, n, h, w, ci, relu=True)
    wt = torch.randn((co, ci, 3, 3), generator=g, device="cuda") * (2.0 / (9 * ci)) ** 0.5
    w64 = R.bf16(wt)
    assert R.TAU_BF16_CONV <= R.ceiling(ci) and R.TAU_BF16_CONV <= R.ceiling(co)
    use_c64 = ci == 64 and co == 64 and fl["c64"]
    fam = "c64" if use_c64 else "conv3x3"
    per = max(ci, co) * h * w

    if not train:
        sc, sh = uniform(g, 0.3, 1.5, co), torch.randn(co, generator=g, device="cuda") * 0.3
        out = nan_bf16(n, h, w, co)
        L.check(lib.gsd_bf16_conv3x3_bnrelu(C.byref(L.make_nhwc(a)), image(L, 0, wt, co, ci).data_ptr(), C.byref(L.make_nhwc(out)), ci, co,
                                            sc.data_ptr(), sh.data_ptr(), st), "conv3x3_bnrelu")
        cv = (1, -1, 1, 1)
        for i, j in chunks(n, per):
            ref, cond = R.conv3x3_fwd(R.nchw(a[i:j]), w64)
            t = ref * sc.double().view(cv) + sh.double().view(cv)
            cond = cond * sc.double().abs().view(cv) + sh.double().abs().view(cv)
            R.check_bound_bf16(R.nchw(out[i:j]), t.clamp_min(0.0), cond, R.TAU_BF16_CONV, f"{tag} conv+BN+ReLU", n0=i,
                               key=f"bf16-fwd:{tag}")
            if j == n:
                forward_mutation_rejected(R.nchw(a[n - 1:n]) * sc.double()[0], w64, R.nchw(out[n - 1:n]), t[-1:].clamp_min(0.0),
                                          cond[-1:], R.TAU_BF16_CONV, f"{tag} forward")
            del ref, cond, t
        return

    # ---- forward + statistics of the stored values
    y = nan_bf16(n, h, w, co)
    mp = lib.gsd_bf16_conv_mpad(co)
    if use_c64:
        rows = lib.gsd_bf16_conv3x3_c64_partial_rows(n, h, w)
        part = partials(rows, 2 * mp)
        L.check(lib.gsd_bf16_conv3x3_c64(C.byref(L.make_nhwc(a)), image(L, 0, wt, co, ci).data_ptr(), C.byref(L.make_nhwc(y)),
                                         part.data_ptr(), None, st), "conv3x3_c64")
    else:
        rows = lib.gsd_bf16_conv_partial_rows(n, h, w, co)
        part = partials(rows, 2 * mp)
        L.check(lib.gsd_bf16_conv3x3(C.byref(L.make_nhwc(a)), image(L, 0, wt, co, ci).data_ptr(), C.byref(L.make_nhwc(y)), ci, co,
                                     part.data_ptr(), None, st), "conv3x3")
    for i, j in chunks(n, per):
        ref, cond = R.conv3x3_fwd(R.nchw(a[i:j]), w64)
        R.check_bound_bf16(R.nchw(y[i:j]), ref, cond, R.TAU_BF16_CONV, f"{tag} forward ({fam})", n0=i, image=n - 1,
                           key=f"bf16-fwd:{tag}")
        if j == n:
            forward_mutation_rejected(R.nchw(a[n - 1:n]), w64, R.nchw(y[n - 1:n]), ref[-1:], cond[-1:], R.TAU_BF16_CONV, f"{tag} forward")
        del ref, cond
    tail_ok(part, rows, 2 * mp, f"{tag} forward")
    g1, g2 = conv_sums(L, part, rows, co)
    check_stored_sums(g1, g2, y, 0, co, f"{tag} forward", f"bf16-stats:{tag}")
    del y, part

    # ---- dX through the dX weight image
    dy = rand_bf16(g, n, h, w, co, scale=1e-3)
    img_d = image(L, 1, wt, co, ci)
    dz = nan_bf16(n, h, w, ci)
    mpi = lib.gsd_bf16_conv_mpad(ci)
    if use_c64:
        rows_d = lib.gsd_bf16_conv3x3_c64_partial_rows(n, h, w)
    else:
        rows_d = lib.gsd_bf16_conv_partial_rows(n, h, w, ci)
    if fused:
        yp = rand_bf16(g, n, h, w, ci)
        sc, sh = uniform(g, 0.3, 1.5, ci), torch.randn(ci, generator=g, device="cuda") * 0.3
        mean, invstd = torch.randn(ci, generator=g, device="cuda") * 0.2, uniform(g, 0.5, 2.0, ci)
        ypv = L.make_nhwc(yp)
        bw = L.gsd_bf16_bnbwd()
        bw.y = C.pointer(ypv)
        bw.scale, bw.shift, bw.mean, bw.invstd = sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr()
        bwp = C.byref(bw)
    else:
        bwp = None
    part_d = partials(rows_d, 2 * mpi) if (fused or cat_stats) else None
    if use_c64:
        L.check(lib.gsd_bf16_conv3x3_c64(C.byref(L.make_nhwc(dy)), img_d.data_ptr(), C.byref(L.make_nhwc(dz)), L.ptr(part_d), bwp, st),
                "conv3x3_c64 dX")
    else:
        L.check(lib.gsd_bf16_conv3x3(C.byref(L.make_nhwc(dy)), img_d.data_ptr(), C.byref(L.make_nhwc(dz)), co, ci, L.ptr(part_d), bwp,
                                     st), "conv3x3 dX")
    what = f"{tag} dX{' fused' if fused else ''} ({fam})"
    for i, j in chunks(n, per):
        ref, cond = R.conv3x3_dx(R.nchw(dy[i:j]), w64)
        if fused:
            m = R.bnrelu_mask(R.nchw(yp[i:j]), sc, sh)
            ref, cond = ref * m, cond * m
            del m
        R.check_bound_bf16(R.nchw(dz[i:j]), ref, cond, R.TAU_BF16_CONV, what, n0=i, key=f"bf16-dx:{tag}")
        del ref, cond
    if part_d is not None:
        tail_ok(part_d, rows_d, 2 * mpi, what)
        q1, q2 = conv_sums(L, part_d, rows_d, ci)
        if fused:
            check_bwd_sums(q1, q2, dz, yp, mean, invstd, what, f"bf16-stats:{tag}")
        else:
            check_stored_sums(q1, q2, dz, 0, ci, what, f"bf16-stats:{tag}")
    del dz, part_d

    # ---- dW: dy against the unit's input over all N*H*W pixels
    dw_check(a, dy, wgrad(L, dy, a, ci, co, n, h, w), tag, f"bf16-dw:{tag}")


# ------------------------------------------------------------------------------------------------------------------- inc
INC_CASES = [(n, "train") for n in TRAIN_N] + [(n, "eval") for n in EVAL_N]


@pytest.mark.parametrize("n,mode", INC_CASES, ids=[f"N{n}-{m}" for n, m in INC_CASES])
def test_inc_bf16_fp64_bound(L, n, mode):
    """`inc` (3 -> 64 -> 64 at 320x427) as the engine runs it.  Train (fused_inc): conv3x3_first's statistics-only pass against
    its storing form's stored y0 (which is checked too: y0 exists only inside the fused kernels), inc_conv (a0 written once into a
    channel slice of a wider buffer, y1, y1's sums), first_bn_bwd_reduce and wgrad_first_recompute.  Eval: conv3x3_first with
    BatchNorm + ReLU in the epilogue."""
    train = mode == "train"
    fl = flags(n, train)
    assert fl["first_direct"] and fl["fused_inc"]
    lib = L.lib
    st = L.stream_ptr()
    c, m, h, w = 3, 64, HS[0], WS[0]
    g = torch.Generator(device="cuda").manual_seed(2000 + n + (0 if train else 500))
    tag = f"inc-N{n}-{mode}"
    x = torch.rand((n, c, h, w), generator=g, device="cuda")
    w0 = torch.randn((m, c, 3, 3), generator=g, device="cuda") * 0.3
    w1 = torch.randn((m, m, 3, 3), generator=g, device="cuda") * (2.0 / (9 * m)) ** 0.5
    w064, w164 = R.bf16(w0), R.bf16(w1)
    img0 = image(L, 2, w0, m, c)
    mp = lib.gsd_bf16_conv_mpad(m)
    per = m * h * w
    if not train:
        sc, sh = uniform(g, 0.3, 1.5, m), torch.randn(m, generator=g, device="cuda") * 0.3
        out = nan_bf16(n, h, w, m)
        L.check(lib.gsd_bf16_conv3x3_first(x.data_ptr(), n, c, h, w, img0.data_ptr(), C.byref(L.make_nhwc(out)), m, None, sc.data_ptr(),
                                           sh.data_ptr(), st), "conv3x3_first bnrelu")
        cv = (1, -1, 1, 1)
        for i, j in chunks(n, per):
            ref, cond = R.first_fwd(x[i:j], w0)
            t = ref * sc.double().view(cv) + sh.double().view(cv)
            cond = cond * sc.double().abs().view(cv) + sh.double().abs().view(cv)
            R.check_bound_bf16(R.nchw(out[i:j]), t.clamp_min(0.0), cond, R.TAU_BF16_FIRST, f"{tag} first conv+BN+ReLU", n0=i,
                               key=f"bf16-first:{tag}")
            if j == n:
                forward_mutation_rejected(R.bf16(x[n - 1:n]) * sc.double()[0], w064, R.nchw(out[n - 1:n]), t[-1:].clamp_min(0.0),
                                          cond[-1:], R.TAU_BF16_FIRST, f"{tag} forward")
            del ref, cond, t
        return

    # ---- the storing form (what the fused launches never write) and the statistics-only pass the engine runs
    rows0 = lib.gsd_bf16_conv3x3_first_partial_rows(n, h, w, m)
    y0 = nan_bf16(n, h, w, m)
    p_store, p_stat = partials(rows0, 2 * mp), partials(rows0, 2 * mp)
    L.check(lib.gsd_bf16_conv3x3_first(x.data_ptr(), n, c, h, w, img0.data_ptr(), C.byref(L.make_nhwc(y0)), m, p_store.data_ptr(),
                                       None, None, st), "conv3x3_first")
    L.check(lib.gsd_bf16_conv3x3_first(x.data_ptr(), n, c, h, w, img0.data_ptr(), None, m, p_stat.data_ptr(), None, None, st),
            "conv3x3_first (statistics)")
    for i, j in chunks(n, per):
        ref, cond = R.first_fwd(x[i:j], w0)
        R.check_bound_bf16(R.nchw(y0[i:j]), ref, cond, R.TAU_BF16_FIRST, f"{tag} y0 (storing form)", n0=i, image=n - 1,
                           key=f"bf16-first:{tag}")
        if j == n:
            forward_mutation_rejected(R.bf16(x[n - 1:n]), w064, R.nchw(y0[n - 1:n]), ref[-1:], cond[-1:], R.TAU_BF16_FIRST,
                                      f"{tag} y0")
        del ref, cond
    for p_ in (p_store, p_stat):
        tail_ok(p_, rows0, 2 * mp, f"{tag} conv3x3_first")
        g1, g2 = conv_sums(L, p_, rows0, m)
        check_stored_sums(g1, g2, y0, 0, m, f"{tag} conv3x3_first statistics", f"bf16-stats:{tag}")
    del p_store
    g1, g2 = conv_sums(L, p_stat, rows0, m)
    cnt = float(n * h * w)
    mean = g1 / cnt
    invstd = 1.0 / torch.sqrt((g2 / cnt - mean * mean).clamp_min(0) + 1e-5)
    gamma, beta = uniform(g, 0.5, 1.5, m).double(), torch.randn(m, generator=g, device="cuda").double() * 0.3
    sc, sh = (gamma * invstd).float(), (beta - mean * gamma * invstd).float()
    mean, invstd = mean.float(), invstd.float()

    # ---- inc_conv: a0 into channels [16, 80) of a 96-channel buffer (sentinel elsewhere), y1 and its sums
    cat = torch.full((n, h, w, m + 32), 7.0, dtype=torch.bfloat16, device="cuda")
    cat[..., 16:16 + m] = float("nan")
    y1 = nan_bf16(n, h, w, m)
    rows1 = lib.gsd_bf16_inc_conv_partial_rows(n, h, w)
    p1 = partials(rows1, 2 * mp)
    L.check(lib.gsd_bf16_inc_conv(x.data_ptr(), n, c, h, w, img0.data_ptr(), sc.data_ptr(), sh.data_ptr(), image(L, 0, w1, m, m).data_ptr(),
                                  C.byref(L.make_nhwc(cat, 16, m)), C.byref(L.make_nhwc(y1)), p1.data_ptr(), st), "inc_conv")
    torch.cuda.synchronize()
    assert bool((cat[..., :16] == 7.0).all()) and bool((cat[..., 16 + m:] == 7.0).all()), f"{tag}: inc_conv wrote outside a0's slice"
    for i, j in chunks(n, per):
        _, aref, acond = R.bn_relu_bf16(R.nchw(y0[i:j]), sc, sh)
        R.check_bound_bf16(R.nchw(cat[i:j], 16, m), aref, acond, R.TAU_BF16_PW, f"{tag} a0", n0=i, key=f"bf16-pw:{tag}")
        del aref, acond
        a_ = R.nchw(cat[i:j], 16, m)
        ref, cond = R.conv3x3_fwd(a_, w164)
        R.check_bound_bf16(R.nchw(y1[i:j]), ref, cond, R.TAU_BF16_CONV, f"{tag} y1 (inc_conv)", n0=i, image=n - 1,
                           key=f"bf16-fwd:{tag}")
        if j == n:
            forward_mutation_rejected(a_[-1:], w164, R.nchw(y1[n - 1:n]), ref[-1:], cond[-1:], R.TAU_BF16_CONV, f"{tag} y1")
        del ref, cond, a_
    tail_ok(p1, rows1, 2 * mp, f"{tag} inc_conv")
    q1, q2 = conv_sums(L, p1, rows1, m)
    check_stored_sums(q1, q2, y1, 0, m, f"{tag} inc_conv", f"bf16-stats:{tag}")
    del cat, y1, p1

    # ---- backward of the first unit without y0: pass 1 from da, dW recomputing y0
    da = rand_bf16(g, n, h, w, m, scale=1e-3)
    pb = partials(rows0, 2 * mp)
    L.check(lib.gsd_bf16_first_bn_bwd_reduce(x.data_ptr(), n, c, h, w, img0.data_ptr(), C.byref(L.make_nhwc(da)), sc.data_ptr(),
                                             sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(), pb.data_ptr(), st), "first_bn_bwd_reduce")
    tail_ok(pb, rows0, 2 * mp, f"{tag} first_bn_bwd_reduce")
    s1, s2 = conv_sums(L, pb, rows0, m)
    acc = [torch.zeros(m, dtype=torch.float64, device="cuda") for _ in range(4)]
    for i, j in chunks(n, per):
        dz, _ = R.bn_bwd_dz(R.nchw(y0[i:j]), sc, sh, R.nchw(da[i:j]))
        acc = [a_ + b_ for a_, b_ in zip(acc, R.bn_bwd_sums(dz, R.nchw(y0[i:j]), mean, invstd))]
        del dz
    R.check_sums(s1, acc[0], acc[2], R.TAU_BF16_STATS, f"{tag} first_bn_bwd_reduce sum dz", key=f"bf16-stats:{tag}")
    R.check_sums(s2, acc[1], acc[3], R.TAU_BF16_STATS, f"{tag} first_bn_bwd_reduce sum dz*xhat", key=f"bf16-stats:{tag}")
    c1, c2 = (s1 / cnt).float(), (s2 / cnt).float()
    need = lib.gsd_bf16_wgrad_first_workspace(n, h, w, m)
    ws = torch.zeros(need, device="cuda")
    dw = torch.full((m, c, 3, 3), float("nan"), device="cuda")
    L.check(lib.gsd_bf16_wgrad_first_recompute(x.data_ptr(), n, c, h, w, img0.data_ptr(), C.byref(L.make_nhwc(da)), sc.data_ptr(),
                                               sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(), c1.data_ptr(), c2.data_ptr(),
                                               dw.data_ptr(), ws.data_ptr(), need, st), "wgrad_first_recompute")

    def d_raw(i, j):
        """d_raw as the kernel forms it (fp32, then bf16) and the magnitude its fp32 evaluation scales with."""
        y_ = R.nchw(y0[i:j])
        dz, _ = R.bn_bwd_dz(y_, sc, sh, R.nchw(da[i:j]))
        ref, cond = R.bn_bwd_apply(dz, y_, sc, mean, invstd, c1, c2)
        return R.bf16(ref), cond
    ref = torch.zeros((m, c, 3, 3), dtype=torch.float64, device="cuda")
    cond = torch.zeros_like(ref)
    for i, j in chunks(n, per):
        d, dabs = d_raw(i, j)
        r_, c_ = R.conv3x3_dw(R.bf16(x[i:j]), d, torch.maximum(d.abs(), dabs))
        ref += r_
        cond += c_
        del d, dabs, r_, c_
    R.check_bound(dw, ref, cond, R.TAU_BF16_DW, f"{tag} dW (wgrad_first_recompute)", key=f"bf16-dw:{tag}", weights=True)
    dw_mutation_rejected(R.bf16(x[n - 1:n]), d_raw(n - 1, n)[0], dw, ref, cond, R.TAU_BF16_DW, f"{tag} dW")


# ------------------------------------------------------------------------------------------- encoder skips: apply + pool
SKIP_CASES = [(lvl, n) for n in (16, 32, 7) for lvl in range(4)]


@pytest.mark.parametrize("lvl,n", SKIP_CASES, ids=[f"enc{l}-N{n}" for l, n in SKIP_CASES])
def test_skip_apply_pool_and_backward_bf16_fp64_bound(L, lvl, n):
    """An encoder skip unit: gsd_bf16_bn_apply_pool_idx (activation into channels [0, C) of the level's concat buffer, pooled
    output, 2-bit arg-max codes), then gsd_bf16_bn_bwd_reduce_pool_idx (skip gradient from the concat gradient + the pooled
    gradient routed by the codes; dz and its sums) and gsd_bf16_bn_bwd_apply."""
    fl = flags(n, True)
    assert fl["apply_pool"]
    lib = L.lib
    st = L.stream_ptr()
    c, h, w = DIMS[lvl], HS[lvl], WS[lvl]
    cup = DIMS[lvl + 1] // 2
    hp, wp = h // 2, w // 2
    g = torch.Generator(device="cuda").manual_seed(3000 + 10 * lvl + n)
    tag = f"enc{lvl}-N{n}"
    y = rand_bf16(g, n, h, w, c)
    # a quarter of the windows hold exact ties (so the first-maximum rule is exercised at the real shape)
    y[:, 0:2 * hp:2, 1:2 * wp:2][:, ::2] = y[:, 0:2 * hp:2, 0:2 * wp:2][:, ::2]
    sc, sh = uniform(g, 0.3, 1.5, c), torch.randn(c, generator=g, device="cuda") * 0.3
    cat = torch.full((n, h, w, c + cup), 7.0, dtype=torch.bfloat16, device="cuda")
    cat[..., :c] = float("nan")
    pooled = nan_bf16(n, hp, wp, c)
    idx = torch.full((n, hp, wp, c // 8), -1, dtype=torch.int16, device="cuda")
    L.check(lib.gsd_bf16_bn_apply_pool_idx(C.byref(L.make_nhwc(y)), sc.data_ptr(), sh.data_ptr(), C.byref(L.make_nhwc(cat, 0, c)),
                                           C.byref(L.make_nhwc(pooled)), idx.data_ptr(), st), "bn_apply_pool_idx")
    torch.cuda.synchronize()
    assert bool((cat[..., c:] == 7.0).all()), f"{tag}: apply wrote into the up slice"
    per = c * h * w
    codes = idx.to(torch.int32) & 0xffff
    got_code = torch.stack([(codes >> (2 * i)) & 3 for i in range(8)], dim=-1).reshape(n, hp, wp, c).permute(0, 3, 1, 2)
    for i, j in chunks(n, per):
        _, aref, acond = R.bn_relu_bf16(R.nchw(y[i:j]), sc, sh)
        R.check_bound_bf16(R.nchw(cat[i:j], 0, c), aref, acond, R.TAU_BF16_PW, f"{tag} activation", n0=i, key=f"bf16-pw:{tag}")
        del aref, acond
        pref, cref = R.maxpool_route(R.nchw(cat[i:j], 0, c))
        assert torch.equal(R.nchw(pooled[i:j]), pref), f"{tag}: pooled output (images {i}..{j})"
        assert torch.equal(got_code[i:j].long(), cref), f"{tag}: arg-max codes (images {i}..{j})"
        del pref, cref

    # ---- backward: dz = mask * (skip gradient + routed pooled gradient), its sums, then pass 2
    gcat = rand_bf16(g, n, h, w, c + cup, scale=1e-3)
    dpool = rand_bf16(g, n, hp, wp, c, scale=1e-3)
    mean, invstd = torch.randn(c, generator=g, device="cuda") * 0.2, uniform(g, 0.5, 2.0, c)
    dz = nan_bf16(n, h, w, c)
    rows = lib.gsd_bf16_bn_bwd_partial_rows(n, h, w)
    part = partials(rows, 3 * c)
    L.check(lib.gsd_bf16_bn_bwd_reduce_pool_idx(C.byref(L.make_nhwc(y)), sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                                C.byref(L.make_nhwc(gcat, 0, c)), idx.data_ptr(), C.byref(L.make_nhwc(dpool)),
                                                C.byref(L.make_nhwc(dz)), part.data_ptr(), st), "bn_bwd_reduce_pool_idx")
    for i, j in chunks(n, per):
        routed = R.pool_grad(R.nchw(dpool[i:j]), got_code[i:j].long(), h, w)
        gs = R.nchw(gcat[i:j], 0, c)
        ref, cond = R.bn_bwd_dz(R.nchw(y[i:j]), sc, sh, gs + routed, gs.abs() + routed.abs())
        R.check_bound_bf16(R.nchw(dz[i:j]), ref, cond, R.TAU_BF16_PW, f"{tag} dz (pool-routed)", n0=i, key=f"bf16-pw:{tag}")
        del routed, gs, ref, cond
    tail_ok(part, rows, 3 * c, f"{tag} bn_bwd_reduce_pool_idx")
    s1, s2, _ = bwd_sums(L, part, rows, c)
    check_bwd_sums(s1, s2, dz, y, mean, invstd, f"{tag} bn_bwd_reduce_pool_idx", f"bf16-stats:{tag}")
    cnt = float(n * h * w)
    c1, c2 = (s1 / cnt).float(), (s2 / cnt).float()
    dz0 = dz.clone()
    L.check(lib.gsd_bf16_bn_bwd_apply(C.byref(L.make_nhwc(dz)), C.byref(L.make_nhwc(y)), sc.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                      c1.data_ptr(), c2.data_ptr(), st), "bn_bwd_apply")
    for i, j in chunks(n, per):
        ref, cond = R.bn_bwd_apply(R.nchw(dz0[i:j]), R.nchw(y[i:j]), sc, mean, invstd, c1, c2)
        R.check_bound_bf16(R.nchw(dz[i:j]), ref, cond, R.TAU_BF16_PW, f"{tag} bn_bwd_apply", n0=i, key=f"bf16-pw:{tag}")
        del ref, cond


# ---------------------------------------------------------------------------------------------------------------- ConvT
CONVT = [("up0.up", 4, 1024), ("up1.up", 3, 512), ("up2.up", 2, 256), ("up3.up", 1, 128)]
CONVT_CASES = [(cse, n) for n in (16, 32, 7) for cse in CONVT]


def pad_off(lvl_in):
    return (HS[lvl_in - 1] - 2 * HS[lvl_in]) // 2, (WS[lvl_in - 1] - 2 * WS[lvl_in]) // 2


@pytest.mark.parametrize("case,n", CONVT_CASES, ids=[f"{c[0]}-N{n}" for c, n in CONVT_CASES])
def test_convT_bf16_fp64_bound(L, case, n):
    """ConvTranspose2d(Cin, Cin/2, 2, 2) as the engine runs it: forward (+bias) scattered into the up slice of the level's concat
    buffer at its F.pad offset (gsd_bf16_conv_dense picks its large-tile kernel itself at these shapes; the skip channels and the
    pad border must keep their sentinels), dX from the gradient slice with the fused BatchNorm-backward pass 1 of the unit below
    (+ its sums), and the 4-tap dW."""
    name, li, ci = case
    lib = L.lib
    st = L.stream_ptr()
    co, h, w = ci // 2, HS[li], WS[li]
    H2, W2 = HS[li - 1], WS[li - 1]
    cs = DIMS[li - 1]
    oy, ox = pad_off(li)
    g = torch.Generator(device="cuda").manual_seed(4000 + ci + n)
    tag = f"{name}-N{n}"
    a = rand_bf16(g, n, h, w, ci, relu=True)
    wt = torch.randn((ci, co, 2, 2), generator=g, device="cuda") / ci ** 0.5
    b = torch.randn(co, generator=g, device="cuda")
    w64, b64 = R.bf16(wt), b.double()
    cat = torch.full((n, H2, W2, cs + co), 7.0, dtype=torch.bfloat16, device="cuda")
    cat[:, oy:oy + 2 * h, ox:ox + 2 * w, cs:] = float("nan")
    z = L.int_array([0])
    L.check(lib.gsd_bf16_conv_dense(C.byref(L.make_nhwc(a)), image(L, 3, wt, co, ci).data_ptr(), C.byref(L.make_nhwc(cat, cs, co)), ci,
                                    4 * co, 1, 1, z, z, h, w, co, oy, ox, b.data_ptr(), None, None, st), "convT")
    torch.cuda.synchronize()
    assert bool((cat[..., :cs] == 7.0).all()), f"{tag}: forward wrote into the skip channels"
    border = cat[..., cs:].clone()
    border[:, oy:oy + 2 * h, ox:ox + 2 * w] = 7.0
    assert bool((border == 7.0).all()), f"{tag}: forward wrote into the F.pad border of the up slice"
    del border
    per = max(ci * h * w, co * H2 * W2)
    for i, j in chunks(n, per):
        ref, cond = R.convT_fwd(R.nchw(a[i:j]), w64, b64)
        R.check_bound_bf16(R.nchw(cat[i:j, oy:oy + 2 * h, ox:ox + 2 * w], cs, co), ref, cond, R.TAU_BF16_CONVT, f"{tag} forward",
                           n0=i, key=f"bf16-convT:{tag}")
        del ref, cond
    del cat

    # ---- dX with the fused pass 1 of the unit below (whose raw output y has the low-res geometry)
    gcat = torch.zeros((n, H2, W2, cs + co), dtype=torch.bfloat16, device="cuda")
    gcat[:, oy:oy + 2 * h, ox:ox + 2 * w, cs:] = rand_bf16(g, n, 2 * h, 2 * w, co, scale=1e-3)
    yb = rand_bf16(g, n, h, w, ci)
    sc, sh = uniform(g, 0.3, 1.5, ci), torch.randn(ci, generator=g, device="cuda") * 0.3
    mean, invstd = torch.randn(ci, generator=g, device="cuda") * 0.2, uniform(g, 0.5, 2.0, ci)
    ybv = L.make_nhwc(yb)
    bw = L.gsd_bf16_bnbwd()
    bw.y = C.pointer(ybv)
    bw.scale, bw.shift, bw.mean, bw.invstd = sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr()
    rows = lib.gsd_bf16_conv_dense_partial_rows(n, h, w, co, ci, 4, 2)
    mpi = lib.gsd_bf16_conv_mpad(ci)
    part = partials(rows, 2 * mpi)
    dz = nan_bf16(n, h, w, ci)
    ty, tx = L.int_array([oy, oy, oy + 1, oy + 1]), L.int_array([ox, ox + 1, ox, ox + 1])
    gup = L.make_nhwc(gcat, cs, co)
    L.check(lib.gsd_bf16_conv_dense(C.byref(gup), image(L, 4, wt, co, ci).data_ptr(), C.byref(L.make_nhwc(dz)), co, ci, 4, 2, ty, tx, h, w,
                                    0, 0, 0, None, part.data_ptr(), C.byref(bw), st), "convT dX")
    for i, j in chunks(n, per):
        ref, cond = R.convT_dx(R.nchw(gcat[i:j, oy:oy + 2 * h, ox:ox + 2 * w], cs, co), w64)
        m = R.bnrelu_mask(R.nchw(yb[i:j]), sc, sh)
        R.check_bound_bf16(R.nchw(dz[i:j]), ref * m, cond * m, R.TAU_BF16_CONVT, f"{tag} dX fused", n0=i, key=f"bf16-convT:{tag}")
        del ref, cond, m
    tail_ok(part, rows, 2 * mpi, f"{tag} dX fused")
    q1, q2 = conv_sums(L, part, rows, ci)
    check_bwd_sums(q1, q2, dz, yb, mean, invstd, f"{tag} dX fused", f"bf16-stats:{tag}")
    del dz, part

    # ---- dW: a against the gradient slice, 4 taps at stride 2 from the pad offset
    need = lib.gsd_bf16_wgrad_workspace(4, n, h, w, ci, co)
    ws = torch.empty((max(need, 64),), device="cuda")
    dw = torch.full((ci, co, 2, 2), float("nan"), device="cuda")
    L.check(lib.gsd_bf16_wgrad(C.byref(L.make_nhwc(a)), C.byref(gup), 4, 2, ty, tx, dw.data_ptr(), co, ws.data_ptr(), ws.numel(), st),
            "convT wgrad")
    acc = [torch.zeros((ci, co, 2, 2), dtype=torch.float64, device="cuda")] * 2
    for i, j in chunks(n, per):
        p_ = R.convT_dw(R.nchw(a[i:j]), R.nchw(gcat[i:j, oy:oy + 2 * h, ox:ox + 2 * w], cs, co))
        acc = [acc[0] + p_[0], acc[1] + p_[1]]
        del p_
    R.check_bound(dw, acc[0], acc[1], R.TAU_BF16_DW, f"{tag} dW", key=f"bf16-dw:{tag}", weights=True)


# ------------------------------------------------------------------------------------------------------------ output conv
@pytest.mark.parametrize("n", (16, 32, 7))
def test_output_conv_bf16_fp64_bound(L, n):
    """outc (64 -> 1, 1x1) as the engine runs it: train, the last unit's BatchNorm + ReLU folded into the output conv
    (gsd_bf16_bn_relu_conv1x1_out, fused_out); eval, gsd_bf16_conv1x1_out from the stored activation; backward,
    gsd_bf16_bn_bwd_reduce mode 2 (dz = mask * w * dout, its sums and the dW_out third sum), then gsd_bf16_bn_bwd_apply."""
    assert flags(n, True)["fused_out"]
    lib = L.lib
    st = L.stream_ptr()
    c, h, w = DIMS[0], HS[0], WS[0]
    g = torch.Generator(device="cuda").manual_seed(5000 + n)
    tag = f"outc-N{n}"
    y = rand_bf16(g, n, h, w, c)
    sc, sh = uniform(g, 0.3, 1.5, c), torch.randn(c, generator=g, device="cuda") * 0.3
    wo, bo = torch.randn((1, c), generator=g, device="cuda") / c ** 0.5, torch.randn(1, generator=g, device="cuda")
    out = torch.full((n, 1, h, w), float("nan"), device="cuda")
    L.check(lib.gsd_bf16_bn_relu_conv1x1_out(C.byref(L.make_nhwc(y)), sc.data_ptr(), sh.data_ptr(), wo.data_ptr(), bo.data_ptr(), 1,
                                             out.data_ptr(), st), "bn_relu_conv1x1_out")
    a = torch.empty((n, h, w, c), dtype=torch.bfloat16, device="cuda")
    per = c * h * w
    for i, j in chunks(n, per):
        stored, _, _ = R.bn_relu_bf16(R.nchw(y[i:j]), sc, sh)
        a[i:j] = stored.permute(0, 2, 3, 1).to(torch.bfloat16)
        ref, cond = R.conv1x1_fwd(stored, wo.double(), bo.double())
        R.check_bound(out[i:j], ref, cond, R.TAU_BF16_PW, f"{tag} bn_relu_conv1x1_out", n0=i, key=f"bf16-pw:{tag}")
        del stored, ref, cond
    out2 = torch.full((n, 1, h, w), float("nan"), device="cuda")
    L.check(lib.gsd_bf16_conv1x1_out(C.byref(L.make_nhwc(a)), wo.data_ptr(), bo.data_ptr(), 1, out2.data_ptr(), st), "conv1x1_out")
    for i, j in chunks(n, per):
        ref, cond = R.conv1x1_fwd(R.nchw(a[i:j]), wo.double(), bo.double())
        R.check_bound(out2[i:j], ref, cond, R.TAU_BF16_PW, f"{tag} conv1x1_out (eval)", n0=i, key=f"bf16-pw:{tag}")
        del ref, cond

    dout = torch.randn((n, 1, h, w), generator=g, device="cuda") * 1e-6
    mean, invstd = torch.randn(c, generator=g, device="cuda") * 0.2, uniform(g, 0.5, 2.0, c)
    dz = nan_bf16(n, h, w, c)
    rows = lib.gsd_bf16_bn_bwd_partial_rows(n, h, w)
    part = partials(rows, 3 * c)
    dzv = L.make_nhwc(dz)
    L.check(lib.gsd_bf16_bn_bwd_reduce(2, C.byref(L.make_nhwc(y)), sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                       C.byref(dzv), C.byref(L.make_nhwc(a)), C.byref(dzv), dout.data_ptr(), wo.data_ptr(), C.byref(dzv),
                                       part.data_ptr(), st), "bn_bwd_reduce(2)")
    dw_ref = torch.zeros(c, dtype=torch.float64, device="cuda")
    dw_cond = torch.zeros_like(dw_ref)
    cv = (1, -1, 1, 1)
    for i, j in chunks(n, per):
        gd = dout[i:j].double() * wo.double().view(cv)
        ref, cond = R.bn_bwd_dz(R.nchw(y[i:j]), sc, sh, gd)
        R.check_bound_bf16(R.nchw(dz[i:j]), ref, cond, R.TAU_BF16_PW, f"{tag} dz (mode 2)", n0=i, key=f"bf16-pw:{tag}")
        r_ = R.conv1x1_dw(R.nchw(a[i:j]), dout[i:j].double())
        dw_ref += r_[0][0]
        dw_cond += r_[1][0]
        del gd, ref, cond, r_
    tail_ok(part, rows, 3 * c, f"{tag} bn_bwd_reduce(2)")
    s1, s2, s3 = bwd_sums(L, part, rows, c)
    check_bwd_sums(s1, s2, dz, y, mean, invstd, f"{tag} bn_bwd_reduce(2)", f"bf16-stats:{tag}")
    R.check_bound(s3, dw_ref, dw_cond, R.TAU_BF16_PW, f"{tag} dW_out (third sum)", key=f"bf16-pw:{tag}", weights=True)


# ------------------------------------------------------------------------------------------- one full-size engine step
def test_full_size_teacher_forced_bf16_step():
    """TrainStep on UNet(precision="bf16") at 16x3x320x427, dims [64, 128, 256, 512, 1024], default mode (fused inc, c64, apply +
    pool, fused output conv, weight gradients on the side stream); then every surviving tensor of the engine against fp64 on
    the GPU from the engine's own stored inputs: every unit's y, a, mean / invstd; pooled and the concat up slices with their
    zero borders; every unit's dW from its stored g and src; the ConvT weight and bias gradients; the output conv and its
    gradients.  Catches a launch argument the unit tests copied right and the engine gets wrong, or an ordering fault of the
    real two-stream schedule."""
    from gelslim_depth_amd import synth
    from gelslim_depth_amd.models.unet import UNet
    from gelslim_depth_amd.train import TrainStep
    from gelslim_depth_amd import _lib as L
    n, h, w = 16, HS[0], WS[0]
    st_ = synth.make_state(3, 1, DIMS, 11, "conditioned")
    x, t = synth.make_batch(n, h, w, 3)
    xt, tt = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=DIMS, precision="bf16")
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st_.items()}, strict=True)
    m = m.to("cuda").train()
    step = TrainStep(m, lr=1e-3, weight_decay=1e-6, ema_decay=0.995, loss="mse")
    p0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    step(xt, tt)
    torch.cuda.synchronize()
    out = step._out
    eng = m._engine
    assert eng.first_direct and eng.fused_inc and eng._use_c64(64, 64) and eng.apply_pool and eng.fused_out and eng.side_dw
    G = {k: v for k, v in m._grad_views.items()}
    tag = "step-N16"
    cv = (1, -1, 1, 1)
    Lv = eng.L

    def dw_rows(u, ref_fn):
        ref = torch.zeros(G[u.wname].shape, dtype=torch.float64, device="cuda")
        cond = torch.zeros_like(ref)
        for i, j in chunks(n, max(u.cin, u.cout) * eng.hs[u.level] * eng.ws[u.level]):
            r_, c_ = ref_fn(i, j)
            ref += r_
            cond += c_
            del r_, c_
        R.check_bound(G[u.wname], ref, cond, R.TAU_BF16_DW, f"{tag} {u.wname} dW", key=f"bf16-dw:{tag}", weights=True)

    for u in eng.units:
        lh, lw = eng.hs[u.level], eng.ws[u.level]
        wq = R.bf16(p0[u.wname])
        per = max(u.cin, u.cout) * lh * lw
        fused0 = u is eng.enc[0][0]
        if fused0:      # y0 never stored: the storing form of the same kernel on the same x and weight image
            y = torch.empty_like(u.y)
            L.check(L.lib.gsd_bf16_conv3x3_first(eng._x.data_ptr(), n, u.cin, lh, lw, u.wt_f.data_ptr(), C.byref(L.make_nhwc(y)), u.cout,
                                                 None, None, None, L.stream_ptr()), "first")
        else:
            y = u.y
        last = u is eng._last_unit()
        if last:        # never stored under fused_out: the apply kernel it replaces
            L.check(L.lib.gsd_bf16_bn_apply(C.byref(L.make_nhwc(u.y)), u.scale.data_ptr(), u.shift.data_ptr(), C.byref(u.a), 1,
                                            L.stream_ptr()), "bn_apply")
        acc = [torch.zeros(u.cout, dtype=torch.float64, device="cuda") for _ in range(4)]
        for i, j in chunks(n, per):
            if u.first:
                ref, cond = R.first_fwd(xt[i:j], p0[u.wname])
            else:
                tsr, off, c_ = u.src
                ref, cond = R.conv3x3_fwd(R.nchw(tsr[i:j], off, c_), wq)
            R.check_bound_bf16(R.nchw(y[i:j]), ref, cond, R.TAU_BF16_FIRST if u.first else R.TAU_BF16_CONV, f"{tag} {u.wname} y",
                               n0=i, key=f"bf16-{'first' if u.first else 'fwd'}:{tag}")
            del ref, cond
            acc = [a_ + b_ for a_, b_ in zip(acc, R.stored_sums(R.nchw(y[i:j])))]
            _, aref, acond = R.bn_relu_bf16(R.nchw(y[i:j]), u.scale, u.shift)
            R.check_bound_bf16(R.nchw(u.a_t[i:j], u.a_off, u.cout), aref, acond, R.TAU_BF16_PW, f"{tag} {u.gname} a", n0=i,
                               key=f"bf16-pw:{tag}")
            del aref, acond
        cnt = float(n * lh * lw)
        mean = acc[0] / cnt
        var = acc[1] / cnt - mean * mean
        # mean / invstd from the stored values' sums: the sums' own bound, carried through the finalize
        R.check_sums(u.mean.double() * cnt, acc[0], acc[2], R.TAU_BF16_STATS + 2.0 ** -23, f"{tag} {u.gname} mean",
                     key=f"bf16-stats:{tag}")
        istd = 1.0 / torch.sqrt(var + 1e-5)
        assert float(((u.invstd.double() - istd).abs() / istd).max()) <= 1e-4, f"{tag} {u.gname} invstd"
        # dW from the stored gradient and input
        if fused0:      # g holds da: d_raw = bf16(scale * (mask * da - c1 - xhat * c2)), formed inside the kernel
            def ref_fn(i, j, u=u, y=y):
                y_ = R.nchw(y[i:j])
                dz, _ = R.bn_bwd_dz(y_, u.scale, u.shift, R.nchw(u.g[i:j]))
                d, dabs = R.bn_bwd_apply(dz, y_, u.scale, u.mean, u.invstd, u.c1, u.c2)
                d = R.bf16(d)
                return R.conv3x3_dw(R.bf16(xt[i:j]), d, torch.maximum(d.abs(), dabs))
        else:
            def ref_fn(i, j, u=u):
                tsr, off, c_ = u.src
                return R.conv3x3_dw(R.nchw(tsr[i:j], off, c_), R.nchw(u.g[i:j]))
        dw_rows(u, ref_fn)
        del y
    for lvl in range(1, Lv + 1):
        prev = eng.enc[lvl - 1][1]
        for i, j in chunks(n, prev.cout * eng.hs[lvl - 1] * eng.ws[lvl - 1]):
            pref, _ = R.maxpool_route(R.nchw(prev.a_t[i:j], prev.a_off, prev.cout))
            assert torch.equal(R.nchw(eng.pooled[lvl][i:j]), pref), f"{tag} pooled[{lvl}]"
    for jj, up in enumerate(eng.ups):
        lvl = Lv - 1 - jj
        prev = eng.dec[jj - 1][1] if jj > 0 else eng.enc[Lv][1]
        hi, wi = eng.hs[lvl + 1], eng.ws[lvl + 1]
        oy, ox = eng._pad_off(lvl)
        cs = DIMS[lvl]
        sl = eng.cat[lvl][..., cs:]
        border = sl.clone()
        border[:, oy:oy + 2 * hi, ox:ox + 2 * wi] = 0
        assert float(border.float().abs().max()) == 0.0, f"{tag} {up.wname}: pad border of the up slice"
        del border
        wq = R.bf16(p0[up.wname])
        accw = [torch.zeros(p0[up.wname].shape, dtype=torch.float64, device="cuda")] * 2 + \
               [torch.zeros(up.cout, dtype=torch.float64, device="cuda")] * 2
        for i, j in chunks(n, max(up.cin * hi * wi, up.cout * 4 * hi * wi)):
            a_in = R.nchw(prev.a_t[i:j], prev.a_off, prev.cout)
            ref, cond = R.convT_fwd(a_in, wq, p0[up.bname].double())
            R.check_bound_bf16(R.nchw(eng.cat[lvl][i:j, oy:oy + 2 * hi, ox:ox + 2 * wi], cs, up.cout), ref, cond, R.TAU_BF16_CONVT,
                               f"{tag} {up.wname} forward", n0=i, key=f"bf16-convT:{tag}")
            del ref, cond
            p_ = R.convT_dw(a_in, R.nchw(eng.gcat[lvl][i:j, oy:oy + 2 * hi, ox:ox + 2 * wi], cs, up.cout))
            accw = [x_ + y_ for x_, y_ in zip(accw, p_)]
            del p_, a_in
        R.check_bound(G[up.wname], accw[0], accw[1], R.TAU_BF16_DW, f"{tag} {up.wname} dW", key=f"bf16-dw:{tag}", weights=True)
        R.check_bound(G[up.bname], accw[2], accw[3], R.TAU_BF16_CONVT, f"{tag} {up.bname}", key=f"bf16-convT:{tag}", weights=True)
    last = eng._last_unit()
    wo, bo = p0["outc.conv.weight"].double().view(1, -1), p0["outc.conv.bias"].double()
    dout, dcond = R.mse_grad(out, tt, out.numel())
    dwo = torch.zeros_like(wo)
    dwc = torch.zeros_like(wo)
    for i, j in chunks(n, last.cout * h * w):
        a_last = R.nchw(last.a_t[i:j], last.a_off, last.cout)
        ref, cond = R.conv1x1_fwd(a_last, wo, bo)
        R.check_bound(out[i:j], ref, cond, R.TAU_BF16_PW, f"{tag} output", n0=i, key=f"bf16-pw:{tag}")
        r_ = R.conv1x1_dw(a_last, dout[i:j])
        dwo += r_[0]
        dwc += r_[1]
        del a_last, ref, cond, r_
    R.check_bound(G["outc.conv.weight"].view(1, -1), dwo, dwc, R.TAU_BF16_PW, f"{tag} outc dW", key=f"bf16-pw:{tag}", weights=True)
    R.check_bound(G["outc.conv.bias"], dout.sum((0, 2, 3)), dcond.sum((0, 2, 3)), R.TAU_BF16_PW, f"{tag} outc db",
                  key=f"bf16-pw:{tag}", weights=True)
