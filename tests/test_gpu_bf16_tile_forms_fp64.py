"""Element-wise fp64 checks of every kernel instantiation and tile of the bf16 convolution family -- gconv_bf16_kernel<0|1, ..>
(gsd_bf16_conv3x3[_bnrelu], gsd_bf16_conv_dense, gsd_bf16_conv1x1_bnrelu), the large-tile ConvT kernels ctgemm_bf16_kernel
<0,4,2,8>, <1,4,2,8>, <1,2,4,4>, gwgrad_bf16_kernel<HALO,T,..> and gwgrad_big_bf16_kernel<4,2>, <2,4> (gsd_bf16_wgrad) -- at the
smallest shapes that reach them and the decode / tail edges of the large-tile kernels (W = 16 and 17, H = 1, P < 256, P = 256,
tiles that straddle three images, more tiles than blocks in both item orders).  The case tables are tests/bf16_tile_cases.py;
tests/test_bf16_tile_form_coverage_cpu.py proves on the CPU that they reach every form and every listed edge, and that the exact
pass below is exact.  Operands and references: tests/bf16_tile_ops.py and tests/fp64_ref.py (fp64 on the GPU, same bf16 operands).

Every case runs two passes.
  random  stored bf16 results to check_bound_bf16 at TAU_BF16_CONV (conv3x3, 1x1) / TAU_BF16_CONVT (ConvT forward, dX), fp32 dW to
          check_bound at TAU_BF16_DW, statistics epilogues to check_sums at TAU_BF16_STATS against the sums of the values as
          stored, the ConvT bias gradient (gsd_bf16_channel_sums) at TAU_BF16_CONVT.  The worst ratio of a case is recorded under
          RATIOS["bf16tile/<case id>"].
  exact   small-integer operands (bf16_tile_ops: cond <= 256 at every stored element, < 2^24 at every dW element): every
          partial sum in any order is exact, so the output must EQUAL the reference (torch.equal) -- one wrong, missing or doubled
          product anywhere fails.  Statistics equal the fp64 sums wherever the reference's absolute sum is below 2^24.

Common to every case: N >= 2 wherever the edge under test allows it; destinations start as NaN; the other channels of a concat
buffer, the F.pad border around a scattered block, the rows past the reported *_partial_rows and the workspace past
*_workspace hold sentinels that must survive; sources that are channel slices or padded blocks lie between 7.0s.

GSD_FP64_REPORT_BF16_TILES=<path>: write the worst ratio per case and the module's wall time there as JSON
(profiles/fp64_bf16_tile_forms.json is one such report from the MI355X).
"""
import ctypes as C
import json
import os
import time

import pytest
import torch

import bf16_tile_cases as B
import bf16_tile_ops as O
import fp64_ref as R
from test_gpu_bf16_fp64_bounds import SENT, TAIL, conv_sums, image, nan_bf16, partials, tail_ok

pytestmark = pytest.mark.gpu

KNOBS = ("GSD_BF16_TW", "GSD_BF16_XCD", "GSD_BF16_CONV_BUF", "GSD_BF16_CTGEMM", "GSD_BF16_CT_BM", "GSD_BF16_WGRAD_BLOCKS",
         "GSD_BF16_WGRAD_BIG")
FILL = 7.0          # what surrounds a source slice and what a launch must leave alone around its destination
T0 = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    T0["t"] = time.time()
    yield
    path = os.environ.get("GSD_FP64_REPORT_BF16_TILES")
    if path:
        with open(path, "w") as f:
            json.dump({"wall_s": time.time() - T0["t"],
                       "ratios": dict(sorted((k, v) for k, v in R.RATIOS.items() if k.startswith("bf16tile/")))}, f, indent=1)


@pytest.fixture(scope="module")
def L():
    from gelslim_depth_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a fault in an earlier launch: the context is gone, launch nothing more
        pytest.exit(f"the GPU context is in error ({e}); stopping", returncode=3)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def set_env(monkeypatch, c):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env:
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------------------------ buffers
def nhwc_src(x, tot=None, off=0, hw=None, at=(0, 0)):
    """An (n, c, h, w) fp64 operand as channels [off, off + c) of a bf16 NHWC buffer of `tot` channels and extent `hw`, placed at
    pixel `at`; everything else holds FILL (a read of a neighbouring slice or of the border shows)."""
    n, c, h, w = x.shape
    bh, bw = hw or (h, w)
    buf = torch.full((n, bh, bw, tot or c), FILL, dtype=torch.bfloat16, device="cuda")
    hh, ww = min(h, bh - at[0]), min(w, bw - at[1])
    buf[:, at[0]:at[0] + hh, at[1]:at[1] + ww, off:off + c] = x[:, :, :hh, :ww].permute(0, 2, 3, 1).to(torch.bfloat16)
    return buf


def nhwc_dst(n, h, w, c, tot=None, off=0, hw=None, at=(0, 0)):
    """A destination: NaN where the launch must write, FILL everywhere else."""
    bh, bw = hw or (h, w)
    buf = torch.full((n, bh, bw, tot or c), FILL, dtype=torch.bfloat16, device="cuda")
    buf[:, at[0]:at[0] + h, at[1]:at[1] + w, off:off + c] = float("nan")
    return buf


def untouched(buf, h, w, c, off, at, what):
    """Everything of `buf` outside the block (at, h, w) x channels [off, off + c) still holds FILL."""
    torch.cuda.synchronize()
    rest = buf.clone()
    rest[:, at[0]:at[0] + h, at[1]:at[1] + w, off:off + c] = FILL
    assert bool((rest == FILL).all()), f"{what}: wrote outside its block (other channels or the border)"


def hand_image(L, w_mk):
    """(M, K) fp32 -> the one-tap weight image [1][mpad(M)][K] bf16, zero-padded rows."""
    m, k = w_mk.shape
    img = torch.zeros((1, L.lib.gsd_bf16_conv_mpad(m), k), dtype=torch.bfloat16, device="cuda")
    img[0, :m] = w_mk.to(torch.bfloat16)
    return img


def bnbwd(L, o, ybuf):
    bw = L.gsd_bf16_bnbwd()
    yv = L.make_nhwc(ybuf)
    bw.y = C.pointer(yv)
    bw.scale, bw.shift, bw.mean, bw.invstd = o["sc"].data_ptr(), o["sh"].data_ptr(), o["mean"].data_ptr(), o["invstd"].data_ptr()
    return bw, yv       # (yv must outlive the launch)


# ------------------------------------------------------------------------------------------------------------------- checks
def stored(mode, got, ref, cond, tau, what, key):
    """A stored bf16 result (NCHW fp64 view of the output) against its reference."""
    if mode == "exact":
        assert float(cond.max()) <= O.LIM_BF16, f"{what}: the exact pass is not exact (cond {float(cond.max())})"
        assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written"
        if not torch.equal(got, ref):
            bad = (got != ref).nonzero()
            p = tuple(bad[0].tolist())
            raise AssertionError(f"{what} (exact pass): {len(bad)} of {got.numel()} elements differ, first at (n, c, h, w) = {p}: "
                                 f"got {float(got[p])}, want {float(ref[p])}")
    else:
        R.check_bound_bf16(got, ref, cond, tau, what, key=key)


def sums(mode, got, ref, bound, what, key):
    """Per-channel sums of a statistics epilogue: the tolerance in the random pass, equality in the exact pass wherever the
    reference's absolute sum is an fp32 integer range."""
    if mode != "exact":
        R.check_sums(got, ref, bound, R.TAU_BF16_STATS, what, key=key)
        return
    ex = bound < O.LIM_F32
    assert torch.equal(got[ex], ref[ex]), f"{what} (exact pass): sums differ, worst by {float((got[ex] - ref[ex]).abs().max())}"
    if not bool(ex.all()):
        R.check_sums(got[~ex], ref[~ex], bound[~ex], R.TAU_BF16_STATS, what)


def stat_sums(L, mode, part, rows, c, y_stored, bw_o, what, key):
    """The partial rows of a launch against the sums of what it stored: (sum y, sum y^2), or with bw_o (sum dz, sum dz * xhat)."""
    mp = L.lib.gsd_bf16_conv_mpad(c)
    tail_ok(part, rows, 2 * mp, what)
    g1, g2 = conv_sums(L, part, rows, c)
    if bw_o is None:
        s1, s2, b1, b2 = R.stored_sums(y_stored)
    else:
        s1, s2, b1, b2 = R.bn_bwd_sums(y_stored, bw_o["y"], bw_o["mean"], bw_o["invstd"])
    if mode == "exact":
        assert bool((b1 < O.LIM_F32).all()), f"{what}: first moments must be exact"
    sums(mode, g1, s1, b1, f"{what} first moment", key)
    sums(mode, g2, s2, b2, f"{what} second moment", key)


# ------------------------------------------------------------------------------------------------------------------ conv3x3
@pytest.mark.parametrize("c", B.CONV3_CASES, ids=B.conv3_id)
def test_conv3x3_bf16_tile_forms(L, monkeypatch, c):
    """gsd_bf16_conv3x3 (plain with statistics, or a dX launch with the fused BatchNorm-backward pass 1) and
    gsd_bf16_conv3x3_bnrelu on every (block, TW, BUF) of gconv_bf16_kernel<0, ..>."""
    set_env(monkeypatch, c)
    lib, st = L.lib, L.stream_ptr()
    cid = B.conv3_id(c)
    for mode in O.PASSES:
        what = f"{cid} [{mode}]"
        o = O.to(O.conv3_ops(c, mode), "cuda")
        ref, cond = O.conv3_ref(c, o)
        xin = nhwc_src(o["a"], c.in_tot, c.in_off)
        out = nhwc_dst(c.n, c.h, c.w, c.m, c.out_tot, c.out_off)
        din, dout = L.make_nhwc(xin, c.in_off, c.k), L.make_nhwc(out, c.out_off, c.m)
        part, rows = None, 0
        if c.ep == "bnrelu":
            img = image(L, 0, o["wt"], c.m, c.k)
            L.check(lib.gsd_bf16_conv3x3_bnrelu(C.byref(din), img.data_ptr(), C.byref(dout), c.k, c.m, o["sc"].data_ptr(),
                                                o["sh"].data_ptr(), st), what)
        else:
            rows = lib.gsd_bf16_conv_partial_rows(c.n, c.h, c.w, c.m)
            assert rows == B.conv_partial_rows(c.n, c.h, c.w, c.m, B.env_of(c), torch.cuda.get_device_properties(0).multi_processor_count)
            part = partials(rows, 2 * lib.gsd_bf16_conv_mpad(c.m))
            if c.ep == "bnbwd":
                img = image(L, 1, o["wt"], c.k, c.m)
                ybuf = nhwc_src(o["y"])
                bw, _keep = bnbwd(L, o, ybuf)
                L.check(lib.gsd_bf16_conv3x3(C.byref(din), img.data_ptr(), C.byref(dout), c.k, c.m, part.data_ptr(), C.byref(bw), st), what)
            else:
                img = image(L, 0, o["wt"], c.m, c.k)
                L.check(lib.gsd_bf16_conv3x3(C.byref(din), img.data_ptr(), C.byref(dout), c.k, c.m, part.data_ptr(), None, st), what)
        untouched(out, c.h, c.w, c.m, c.out_off, (0, 0), what)
        got = R.nchw(out, c.out_off, c.m)
        stored(mode, got, ref, cond, R.TAU_BF16_CONV, what, f"bf16tile/{cid}")
        if part is not None:
            stat_sums(L, mode, part, rows, c.m, got, o if c.ep == "bnbwd" else None, what, f"bf16tile/{cid}")


# --------------------------------------------------------------------------------------------- dense and large-tile ConvT
def run_dense(L, c, cid, mode):
    """One pass of a dense / ConvT case through gsd_bf16_conv_dense (or gsd_bf16_conv1x1_bnrelu)."""
    lib, st = L.lib, L.stream_ptr()
    what = f"{cid} [{mode}]"
    key = f"bf16tile/{cid}"
    o = O.to(O.dense_ops(c, mode, cid), "cuda")
    z = L.int_array([0])
    if c.kind in ("1x1", "1x1bnrelu"):
        ref, cond = O.dense_ref(c, o)
        xin, out = nhwc_src(o["a"]), nan_bf16(c.n, c.h, c.w, c.m)
        img = hand_image(L, o["wt"])
        if c.kind == "1x1bnrelu":
            L.check(lib.gsd_bf16_conv1x1_bnrelu(C.byref(L.make_nhwc(xin)), img.data_ptr(), C.byref(L.make_nhwc(out)), c.k, c.m,
                                                o["sc"].data_ptr(), o["sh"].data_ptr(), st), what)
            stored(mode, R.nchw(out), ref, cond, R.TAU_BF16_CONV, what, key)
            return
        rows = lib.gsd_bf16_conv_dense_partial_rows(c.n, c.h, c.w, c.k, c.m, 1, 1)
        part = partials(rows, 2 * lib.gsd_bf16_conv_mpad(c.m))
        L.check(lib.gsd_bf16_conv_dense(C.byref(L.make_nhwc(xin)), img.data_ptr(), C.byref(L.make_nhwc(out)), c.k, c.m, 1, 1, z, z, c.h,
                                        c.w, 0, 0, 0, o["b"].data_ptr(), part.data_ptr(), None, st), what)
        stored(mode, R.nchw(out), ref, cond, R.TAU_BF16_CONV, what, key)
        stat_sums(L, mode, part, rows, c.m, R.nchw(out), None, what, key)
        return
    if c.kind == "ctfwd":
        ref, cond = O.dense_ref(c, o)
        cs = c.cs
        hw = (2 * c.h + c.oy + c.spare, 2 * c.w + c.ox + c.spare)
        xin = nhwc_src(o["a"])
        cat = nhwc_dst(c.n, 2 * c.h, 2 * c.w, cs, 2 * cs, cs, hw, (c.oy, c.ox))
        L.check(lib.gsd_bf16_conv_dense(C.byref(L.make_nhwc(xin)), image(L, 3, o["wt"], cs, c.k).data_ptr(), C.byref(L.make_nhwc(cat, cs, cs)),
                                        c.k, c.m, 1, 1, z, z, c.h, c.w, cs, c.oy, c.ox, o["b"].data_ptr(), None, None, st), what)
        untouched(cat, 2 * c.h, 2 * c.w, cs, cs, (c.oy, c.ox), what)
        stored(mode, R.nchw(cat[:, c.oy:c.oy + 2 * c.h, c.ox:c.ox + 2 * c.w], cs, cs), ref, cond, R.TAU_BF16_CONVT, what, key)
        return
    # ctdx
    in_, _, ty, tx = B.dense_geometry(c)
    gcat = nhwc_src(o["a"], 2 * c.k, c.k, (in_.H, in_.W), (c.oy, c.ox))
    dz = nhwc_dst(c.n, c.h, c.w, c.m, hw=(c.h + c.opad, c.w + c.opad))
    part, rows, bwp = None, 0, None
    if c.fused:
        rows = lib.gsd_bf16_conv_dense_partial_rows(c.n, c.h, c.w, c.k, c.m, 4, 2)
        part = partials(rows, 2 * lib.gsd_bf16_conv_mpad(c.m))
        ybuf = nhwc_src(o["y"])
        bw, _keep = bnbwd(L, o, ybuf)
        bwp = C.byref(bw)
    rc = lib.gsd_bf16_conv_dense(C.byref(L.make_nhwc(gcat, c.k, c.k)), image(L, 4, o["wt"], c.k, c.m).data_ptr(), C.byref(L.make_nhwc(dz)),
                                 c.k, c.m, 4, 2, L.int_array(ty), L.int_array(tx), c.h, c.w, 0, 0, 0, None, L.ptr(part), bwp, st)
    if c.want != 0:
        torch.cuda.synchronize()
        assert rc == c.want, f"{what}: returned {rc}, want {c.want} ({lib.gsd_last_error().decode()})"
        assert bool(torch.isnan(dz.float()).all()), f"{what}: a refused launch wrote its output"
        return
    L.check(rc, what)
    ref, cond = O.dense_ref(c, o)
    untouched(dz, c.h, c.w, c.m, 0, (0, 0), what)
    got = R.nchw(dz[:, :c.h, :c.w])
    stored(mode, got, ref, cond, R.TAU_BF16_CONVT, what, key)
    if c.fused:
        stat_sums(L, mode, part, rows, c.m, got, o, what, key)


@pytest.mark.parametrize("c", B.DENSE_CASES, ids=B.dense_id)
def test_dense_bf16_tile_forms(L, monkeypatch, c):
    """gsd_bf16_conv_dense on gconv_bf16_kernel<1, ..>: one tap plain / with the eval epilogue, the ConvT forward scatter at
    Cs 16 and 32, the 4-tap stride-2 dX plain and fused, a cropped gradient buffer (taps that leave it read zeros), and what
    the host does at a large-tile shape with operands that kernel cannot serve: a cropped gradient buffer or an output buffer
    larger than the pixel grid go to the general kernel when plain, the cropped one is GSD_ERR_UNSUPPORTED when fused."""
    set_env(monkeypatch, c)
    for mode in O.PASSES:
        run_dense(L, c, B.dense_id(c), mode)


@pytest.mark.parametrize("c", B.CT_CASES, ids=B.ct_id)
def test_large_tile_convT_bf16(L, monkeypatch, c):
    """ctgemm_bf16_kernel<0,4,2,8> (forward, scatter + bias), <1,4,2,8> and <1,2,4,4> (dX, plain and fused) at the decode and
    tail edges of the flattened pixel run."""
    set_env(monkeypatch, c)
    assert B.form_of(c, torch.cuda.get_device_properties(0).multi_processor_count) == c.form
    for mode in O.PASSES:
        run_dense(L, B.ct_as_dense(c), B.ct_id(c), mode)


# ----------------------------------------------------------------------------------------------------------------------- dW
def run_wgrad(L, c, mode):
    lib, st = L.lib, L.stream_ptr()
    cid = B.wg_id(c)
    what = f"{cid} [{mode}]"
    key = f"bf16tile/{cid}"
    o = O.to(O.wg_ops(c, mode), "cuda")
    ref, cond, db = O.wg_ref(c, o)
    _, bg, stride, ty, tx = B.wg_geometry(c)
    abuf = nhwc_src(o["a"])
    bbuf = nhwc_src(o["b"], c.b_tot, c.b_off, (bg.H, bg.W), (c.oy, c.ox) if c.taps == 4 else (0, 0))
    need = lib.gsd_bf16_wgrad_workspace(c.taps, c.n, c.h, c.w, c.m, c.ncols)
    ws = torch.full((need + TAIL,), float("nan"), device="cuda")
    ws[need:] = SENT
    dw = torch.full((c.m, c.ncols_out, c.taps), float("nan"), device="cuda")
    bview = L.make_nhwc(bbuf, c.b_off, c.ncols)
    L.check(lib.gsd_bf16_wgrad(C.byref(L.make_nhwc(abuf)), C.byref(bview), c.taps, stride, L.int_array(ty), L.int_array(tx),
                               dw.data_ptr(), c.ncols_out, ws.data_ptr(), need, st), what)
    torch.cuda.synchronize()
    assert bool((ws[need:] == SENT).all()), f"{what}: workspace written past the {need} floats of gsd_bf16_wgrad_workspace"
    if mode == "exact":
        assert float(cond.max()) < O.LIM_F32
        assert bool(torch.isfinite(dw).all()), f"{what}: dW elements not written"
        if not torch.equal(dw.double(), ref):
            bad = (dw.double() != ref).nonzero()
            p = tuple(bad[0].tolist())
            raise AssertionError(f"{what} (exact pass): {len(bad)} of {dw.numel()} dW elements differ, first at (m, n, tap) = {p}: "
                                 f"got {float(dw[p])}, want {float(ref[p])}")
    else:
        R.check_bound(dw, ref, cond, R.TAU_BF16_DW, f"{what} dW", key=key, weights=True)
    if db is None:
        return
    # the ConvT bias gradient over the same window of the gradient slice
    hh, ww = min(2 * c.h, bg.H - c.oy), min(2 * c.w, bg.W - c.ox)
    nws = lib.gsd_bf16_channel_sums_workspace(c.n, hh, ww, c.ncols)
    cws = torch.full((nws + TAIL,), float("nan"), device="cuda")
    cws[nws:] = SENT
    got = torch.full((c.ncols,), float("nan"), device="cuda")
    L.check(lib.gsd_bf16_channel_sums(C.byref(bview), c.oy, c.ox, hh, ww, got.data_ptr(), cws.data_ptr(), nws, st), f"{what} channel sums")
    torch.cuda.synchronize()
    assert bool((cws[nws:] == SENT).all()), f"{what}: channel sums wrote past their workspace"
    if mode == "exact":
        assert torch.equal(got.double(), db[0]), f"{what} (exact pass): bias gradient differs"
    else:
        R.check_bound(got, db[0], db[1], R.TAU_BF16_CONVT, f"{what} db", key=key, weights=True)


@pytest.mark.parametrize("c", B.WG_CASES, ids=B.wg_id)
def test_wgrad_bf16_tile_forms(L, monkeypatch, c):
    """gsd_bf16_wgrad on gwgrad_bf16_kernel<HALO, T, ..>: both tile widths of every (HALO, T, block), ragged M and Ncols, b as a
    channel slice, more stages than splits."""
    set_env(monkeypatch, c)
    for mode in O.PASSES:
        run_wgrad(L, c, mode)


@pytest.mark.parametrize("c", B.WGBIG_CASES, ids=B.wg_id)
def test_large_tile_wgrad_bf16(L, monkeypatch, c):
    """gsd_bf16_wgrad on gwgrad_big_bf16_kernel<4,2> / <2,4> (P < 64, P % 64 != 0, several stages per split, every tap offset),
    its fallback to the general kernel when b is cropped, and the bias gradient beside it."""
    set_env(monkeypatch, c)
    assert B.form_of(c, torch.cuda.get_device_properties(0).multi_processor_count) == c.form
    for mode in O.PASSES:
        run_wgrad(L, c, mode)
