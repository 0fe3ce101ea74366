"""The strided fp32 kernels held to their fp64 bounds with operands whose images and planes lie gigabytes apart: every address a
kernel forms from n_stride / c_stride crosses 2^31 bytes, 2^32 bytes, 2^31 elements or 2^32 elements (tests/far_layouts.py; the
arithmetic of the placements is proved in tests/test_far_layouts_cpu.py), while the tensors stay a few kilobytes.

Launches, references and every check are those of tests/test_gpu_tile_forms_fp64.py (conv_case, fused_case, wgrad_case,
wgrad_bn_case, convT_case), called twice per case: once with compact operands and once with every strided operand, the
statistics partials and the K-slab scratch carved from one 24-GiB arena of a NaN bit pattern.  Per case:

  bound        every output element within the family's tau * cond of fp64_ref (the constants of fp64_ref.py, unchanged);
  same bits    the far launch stores the bits of the compact one, wherever the host layer picks the same kernel and block order
               for both (SAME below says where it does not, and which host line decides);
  containment  after the outputs are copied out and the operands' words put back, the WHOLE arena holds the fill pattern again
               (a full scan per case: 24 GiB in 12 ms on the MI355X, 16 ms at most, so no case needs the windowed form) -- and
               during the case the pad columns, the neighbouring channels of a channel slice and the floats behind the partials
               and the scratch do; the arena is scanned once more, without repair, when the module ends;
  operands     the placement handed out exactly the operand list the CPU proof was made for;
  refusals     a folded gsd_conv3x3_w43 plan under n33 / c29 is GSD_ERR_UNSUPPORTED "batch too large for row folding" with
               nothing written -- asserted, not skipped.

SAME (far == compact bit for bit) is asserted for every case except
  w2d under c29       gsd_conv3x3_w2d.hip w2d_impl: P.dfast is off once 12 * c_stride * 4 + plane >= 2^32 (the launch line's
                      `dfast` field is asserted 0 there and all ones under n31 / n33) -- another store path;
  dW under c25        gsd_wgrad_w2d.hip gsd_wgrad_w2d_use (BM * dy.c_stride * 4 >= 2^31: the 2-D cases run the row form, asserted
                      from gsd_conv3x3_wgrad_form and the wg43 line) and gsd_wgrad_w43.hip gsd_wgrad_w43_run (BN * c_stride >= 2^31:
                      bx4 0, asserted) -- other kernels.

What no layout admits, and why: K-slab launches under c29 (a slab needs 8 chunks of 4 channels, c29 holds 16 channels); the
folded w43 form under n33 / c29 (refused, above; n31 folds: 3 * (2^29 + 64) < 2^31 -- so no folding shape exists under c29, whose
N * n_stride is 2^32 + 2048 at N = 2); dW under c29 (a dW block takes 64 channels: 32 GiB an image at that plane distance --
c25 is the same idea at a quarter of it and trips the same two guards); gsd_conv1x1_out under c29 (dense planes by contract:
refused, asserted).  Dense by contract, with no stride to place: dz / raw of gsd_conv3x3_wgrad_bn, every operand of
gsd_conv3x3_dgrad_bn, gsd_bn_bwd_reduce mode 2, gsd_bn_bwd_apply and gsd_conv1x1_out_wgrad, dW / db and the dW workspaces, and dy
of gsd_convT2x2_wgrad when it is asked for the bias gradient (a strided dy is refused there before anything is launched -- it
used to be refused after dW had been written, which this module found; dW alone takes any strides).

Worst |got - ref| / cond over this module on the MI355X (profiles/fp64_far_strides.json) against the family's tau, no constant
widened and none of the module's own (the gathers use tests/test_gpu_augment.py's TAU_AUG, the pool, the activations, dz and
gsd_gather_affine are bit-exact):
    w43    1.45e-06  against TAU_WINO = 6.0e-06     (n31 / n33 w43-3x9x50-c8+0-m70-slack_bn)
    w2d    1.19e-06  against TAU_WINO = 6.0e-06     (w2d-3x12x45-c8+0-m70-slack_bn)
    direct 3.17e-07  against TAU_DIRECT = 1.6e-06   (direct-3x21x29-c5+0-m130-dword)
    dw     4.87e-07  against TAU_DW = 4.0e-06       (2x1x40-c20+44-m64-pitched-slack4-form1 under c25)
    convT  2.83e-07  against TAU_CONVT = 1.9e-06    (convT-3x5x53-k36-m40)
    stats  3.05e-08  against TAU_STATS = 3.4e-08    (pointwise-c29-16x8x12: gsd_bn_bwd_reduce's sums over 2 x 96 elements, where the
                                                     one fp32 rounding of a stored sum is already 2^-25 = 2.98e-08 of it; the compact
                                                     launch gives the same bits; the conv epilogues stay below 9.7e-09)
    1x1    1.20e-07  against TAU_1X1 = 8.0e-07      (pointwise-n31-13x9x11)
    gather 6.09e-08  against TAU_AUG = 4.5e-07      (gsd_gather_augment image, 3x9x11)
The module takes 7 s, 26.5 GB of device memory at its peak (the arena is allocated once and freed when the module ends).

GSD_FP64_REPORT_FAR=<path>: worst ratio per family and case, the kernel line of each launch, wall time, scan times and peak
memory as JSON (profiles/fp64_far_strides.json is the MI355X run).
"""
import json
import os
import time

import pytest
import torch

import far_layouts as FL
import fp64_ref as R
import test_gpu_tile_forms_fp64 as TF
import tile_cases as T
from test_gpu_fp64_bounds import rejects
from test_gpu_layer_shapes import gsd  # noqa: F401  (the module fixture)
from test_gpu_tile_forms_fp64 import clean_env  # noqa: F401  (autouse: a context in error ends the module; knobs cleared)

pytestmark = pytest.mark.gpu

TABLES = FL._tables()
LINES = {}          # case id -> launch lines
WALL = {}


@pytest.fixture(scope="module")
def arena():
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    a = FL.Arena()
    yield a
    bad = a.scan(repair=False)
    path = os.environ.get("GSD_FP64_REPORT_FAR")
    if path:
        mine = {k[4:]: v for k, v in R.RATIOS.items() if k.startswith("far:")}
        worst = {}
        for k, v in mine.items():
            fam = k.split(":")[1]
            if fam not in worst or v > worst[fam]["ratio"]:
                worst[fam] = {"ratio": v, "tau": {**TF.TAUS, "1x1": R.TAU_1X1, "gather": 4.5e-7}[fam], "case": k.split(":", 2)[2]}
        with open(path, "w") as f:
            json.dump({"wall_s": time.time() - t0, "arena_bytes": 4 * a.elems, "scans": len(a.scan_s),
                       "scan_s_mean": sum(a.scan_s) / len(a.scan_s), "scan_s_max": max(a.scan_s),
                       "peak_memory_bytes": torch.cuda.max_memory_allocated(), "worst": dict(sorted(worst.items())),
                       "ratios": dict(sorted(mine.items())), "kernels": dict(sorted(LINES.items())),
                       "case_wall_s": dict(sorted(WALL.items()))}, f, indent=1)
    a.free()
    assert not bad, f"words of the arena changed and were never put back: {bad[:8]}"


def same_bits(far, compact, what):
    for k, v in compact.items():
        if torch.is_tensor(v) and k in far:          # (ConvT: db comes from the compact launch only, see convT_case)
            assert far[k].shape == v.shape and torch.equal(far[k].contiguous().view(torch.int32), v.contiguous().view(torch.int32)), \
                f"{what}: `{k}` of the far launch differs from the compact launch's " \
                f"({int((far[k] != v).sum())} of {v.numel()} elements, worst |diff| {float((far[k] - v).abs().max()):.3g})"


def far_run(arena, lay, tag, fn, expect_ops, same):
    """fn(place, ns) compact and far; operands, containment, bits."""
    t0 = time.time()
    compact = fn(None, "farc")
    place = arena.placement(lay)
    err = None
    far = None
    try:
        far = fn(place, f"far:{lay}")
    except BaseException as e:       # put the arena back whatever happened, then say both
        err = e
    got_ops = list(place.recs)
    place.restore()
    bad = arena.scan()
    WALL[f"{lay}:{tag}"] = time.time() - t0
    where = "; ".join(f"word {i} ({i - FL.FRONT:+d} from the operands' band)" for i in bad[:6])
    if err is not None:
        if bad:
            raise AssertionError(f"{tag} under {lay}: {err}; and outside the operands the arena changed at {where}") from err
        raise err
    assert not bad, f"{tag} under {lay}: the launch wrote outside its operands: {where}"
    assert got_ops == FL.dry(lay, expect_ops()).recs, "the launch's operands are not the list the CPU proof is about"
    LINES[f"{lay}:{tag}"] = {k: v for k, v in far.items() if isinstance(v, str)}
    if same:
        same_bits(far, compact, f"{tag} under {lay}")
    return far


def refused(arena, gsd, lay, tag, fn, dst_index):
    """The far launch must be refused as the folded w43 plan is, with nothing written."""
    place = arena.placement(lay)
    with pytest.raises(gsd.GsdError, match=r"code -2\).*batch too large for row folding"):
        fn(place, f"far:{lay}")
    torch.cuda.synchronize()
    d = place.recs[dst_index]
    words = place.int_view(d)
    nan = torch.full((1,), float("nan"), device="cuda").view(torch.int32)
    untouched = bool(((words == FL.FILL_I32) | (words == nan)).all())
    place.restore()
    bad = arena.scan()
    assert untouched and not bad, f"{tag} under {lay}: a refused launch wrote something"
    LINES[f"{lay}:{tag}"] = {"refused": "batch too large for row folding"}


# -------------------------------------------------------------------------------------------------------- conv3x3 forward / dX
CONV = [(lay, c) for lay in ("n31", "n33", "c29") for c in TABLES["conv"][lay]]


@pytest.mark.parametrize("lay,case", CONV, ids=[f"{lay}-{T.case_id(c)}" for lay, c in CONV])
def test_conv3x3_far(gsd, arena, monkeypatch, capfd, lay, case):
    c = case
    tag = T.case_id(c)
    ci = c.c0 + c.c1

    def fn(place, ns):
        return TF.conv_case(gsd, monkeypatch, capfd, c, place=place, ns=ns)

    if FL.fold_refused(lay, c.fam, c.n, c.h, c.w, c.co, T.env_of(c)):
        return refused(arena, gsd, lay, tag, fn, 1 + (1 if c.c1 else 0))

    def ops():
        ws = (0, 0)
        if any(k.endswith("_SPLIT") for k, _ in c.env):
            q = getattr(gsd.lib, f"gsd_conv3x3_{c.fam}_workspace")
            ws = (q(c.n, c.h, c.w, ci, c.co), q(c.n, c.h, c.w, FL._r4(c.co) if c.fam == "w2d" else c.co, ci))
        return FL.conv_operands(c, ws)

    far = far_run(arena, lay, tag, fn, ops, same=not (c.fam == "w2d" and lay == "c29"))
    if c.fam == "w2d":
        ndst_dx = 2 if c.c1 else 1
        want = (0, 0) if lay == "c29" else (1, (1 << ndst_dx) - 1)
        assert (int(TF.field(far["line"], "dfast")), int(TF.field(far["line_dx"], "dfast"))) == want, (far["line"], far["line_dx"])


# ----------------------------------------------------------------------------------------------------------- fused dX epilogue
FUSED = [(lay, c) for lay in ("n31", "n33", "c29") for c in TABLES["fused"][lay]]


def _fused_id(c):
    return f"{c.fam}-{c.n}x{c.h}x{c.w}-k{c.co}-m{c.ci}" + "".join(f"-{k[4:]}={v}" for k, v in c.env)


@pytest.mark.parametrize("lay,case", FUSED, ids=[f"{lay}-{_fused_id(c)}" for lay, c in FUSED])
def test_fused_dx_far(gsd, arena, monkeypatch, lay, case):
    c = case
    tag = "fused-" + _fused_id(c)

    def fn(place, ns):
        return TF.fused_case(gsd, monkeypatch, c, place=place, ns=ns)

    if FL.fold_refused(lay, c.fam, c.n, c.h, c.w, c.ci, T.env_of(c)):
        return refused(arena, gsd, lay, tag, fn, 3)

    def ops():
        split = any(k.endswith("_SPLIT") for k, _ in c.env)
        return FL.fused_operands(c, getattr(gsd.lib, f"gsd_conv3x3_{c.fam}_workspace")(c.n, c.h, c.w, c.co, c.ci) if split else 0)

    far_run(arena, lay, tag, fn, ops, same=not (c.fam == "w2d" and lay == "c29"))


# --------------------------------------------------------------------------------------------------------------------------- dW
WG = [(lay, c, form) for lay in ("n31", "n33", "c25") for c, form in TABLES["wgrad"][lay]]


@pytest.mark.parametrize("lay,case,form", WG, ids=[f"{lay}-{TF._wg_id(c)}" for lay, c, _ in WG])
def test_conv3x3_wgrad_far(gsd, arena, monkeypatch, capfd, lay, case, form):
    c = case
    tag = "dw-" + TF._wg_id(c)

    def fn(place, ns):
        return TF.wgrad_case(gsd, monkeypatch, capfd, c, place=place, ns=ns, form=None if place is None else form)

    far = far_run(arena, lay, tag, fn, lambda: FL.wgrad_operands(c), same=lay != "c25")
    if lay == "c25" and form == 1:
        p = T.plan_wg43(c.n, c.h, c.w, c.co, c.c0 + c.c1, T.env_of(c))
        if p.BN * FL.LAYOUTS["c25"].c_stride >= 1 << 31:
            assert int(TF.field(far["line"], "bx4")) == 0, far["line"]
        assert far["line"].startswith("wg43 "), far["line"]          # (the 2-D cases: the documented fall-back to the row form)


WGBN = [(lay, s) for lay in ("n31", "n33") for s in TABLES["wgrad_bn"][lay]]


@pytest.mark.parametrize("lay,shape", WGBN, ids=[f"{lay}-{n}x{h}x{w}" for lay, (n, h, w) in WGBN])
def test_first_layer_wgrad_bn_far(gsd, arena, lay, shape):
    n, h, w = shape
    far_run(arena, lay, f"wgrad_bn-{n}x{h}x{w}", lambda place, ns: TF.wgrad_bn_case(gsd, n, h, w, place=place, ns=ns),
            lambda: FL.wgrad_bn_operands(n, h, w), same=True)


# ------------------------------------------------------------------------------------------------------------------------ ConvT
CONVT = [(lay, s) for lay in ("n31", "n33", "c29") for s in TABLES["convT"][lay]]


@pytest.mark.parametrize("lay,shape", CONVT, ids=[f"{lay}-{n}x{h}x{w}-k{ci}-m{co}" for lay, (n, h, w, ci, co) in CONVT])
def test_convT_far(gsd, arena, lay, shape):
    n, h, w, ci, co = shape
    far_run(arena, lay, f"convT-{n}x{h}x{w}-k{ci}-m{co}", lambda place, ns: TF.convT_case(gsd, n, h, w, ci, co, place=place, ns=ns),
            lambda: FL.convT_operands(n, h, w, ci, co), same=True)


# ------------------------------------------------------------------------------------------------- pooling, activation, head
# The pointwise entry points that take a strided descriptor: gsd_maxpool2 (src), gsd_maxpool2_pitched (src, pooled, act),
# gsd_bnrelu_pitched (src, dst), gsd_bn_bwd_reduce mode 0 (da) and gsd_conv1x1_out (src; planes must be dense, so c29 is refused).
# gsd_bn_bwd_reduce mode 2, gsd_bn_bwd_apply and gsd_conv1x1_out_wgrad take dense pointers only.  Results are bit-exact against the
# single-rounded fp64_ref expressions, as in tests/test_gpu_fp32_pointwise_fp64.py; the 1x1 conv against TAU_1X1.
PW_SHAPES = [(13, 9, 11), (16, 8, 12)]          # odd sizes (the scalar forms, a dropped last row / column); H * W % 4 == 0


def _carve(place, n, c, h, w, pitch=None):
    return place.view(n, c, h, pitch or w)[..., :w]


def _pad_columns_zero(t_full, w, what):
    assert bool((t_full[..., w:] == 0).all()), f"{what}: pad columns must be written 0"


@pytest.mark.parametrize("lay", ["n31", "n33", "c29"])
@pytest.mark.parametrize("shape", PW_SHAPES, ids=[f"{c}x{h}x{w}" for c, h, w in PW_SHAPES])
def test_pointwise_far(gsd, arena, lay, shape):
    import ctypes as C
    import test_gpu_fp32_pointwise_fp64 as TP
    L, st = gsd.lib, gsd.stream_ptr()
    c, h, w = shape
    n = FL.LAYOUTS[lay].max_n
    hp, wp = h // 2, w // 2
    g = TF.gen(n, c, h, w, 31)
    sc, sh = TF.uniform(g, 0.5, 1.5, c), TF.randn(g, c, scale=0.3)
    mean, invstd = TF.randn(g, c, scale=0.3), TF.uniform(g, 0.5, 2.0, c)
    vals, dav = TF.randn(g, n, c, h, w), TF.randn(g, n, c, h, w)
    k = 3
    wo, bo = TF.randn(g, k, c, scale=0.25), TF.randn(g, k)
    place = arena.placement(lay)
    tag = f"pointwise-{lay}-{c}x{h}x{w}"
    out = {}
    try:
        for far in (False, True):
            if far:
                raw = _carve(place, n, c, h, w)
                pooled_full, act_full, once_full = place.view(n, c, hp, FL._r4(wp)), place.view(n, c, h, FL._r4(w)), place.view(n, c, h, FL._r4(w))
                da = _carve(place, n, c, h, w)
            else:
                raw = torch.empty((n, c, h, w), device="cuda")
                pooled_full, act_full, once_full = (torch.empty((n, c, hp, FL._r4(wp)), device="cuda"),
                                                    torch.empty((n, c, h, FL._r4(w)), device="cuda"), torch.empty((n, c, h, FL._r4(w)), device="cuda"))
                da = torch.empty((n, c, h, w), device="cuda")
            raw.copy_(vals)
            da.copy_(dav)
            for t in (pooled_full, act_full, once_full):
                t.fill_(float("nan"))
            src = gsd.make_src(raw, sc, sh, relu=True)
            y = torch.full((n, c, hp, wp), float("nan"), device="cuda")
            gsd.check(L.gsd_maxpool2(C.byref(src), y.data_ptr(), n, c, h, w, st), "maxpool2")
            dp, da_ = gsd.make_dst(pooled_full[..., :wp]), gsd.make_dst(act_full[..., :w])
            gsd.check(L.gsd_maxpool2_pitched(C.byref(src), C.byref(dp), C.byref(da_), n, st), "maxpool2_pitched")
            do = gsd.make_dst(once_full[..., :w])
            gsd.check(L.gsd_bnrelu_pitched(C.byref(src), C.byref(do), n, st), "bnrelu_pitched")
            rows = L.gsd_bn_bwd_partial_rows(n, c, h, w)
            part = torch.full((rows * 3 * c + 64,), TF.SENT, device="cuda")
            dz = torch.full((n, c, h, w), float("nan"), device="cuda")
            rawd = vals.clone()
            sda = gsd.make_src(da)
            gsd.check(L.gsd_bn_bwd_reduce(0, rawd.data_ptr(), sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(), C.byref(sda),
                                          None, None, None, 1, dz.data_ptr(), part.data_ptr(), n, c, h, w, st), "bn_bwd_reduce(0)")
            o = torch.full((n, k, h, w), float("nan"), device="cuda")
            rc = L.gsd_conv1x1_out(C.byref(src), wo.data_ptr(), bo.data_ptr(), c, k, o.data_ptr(), n, h, w, st)
            torch.cuda.synchronize()
            if far and lay == "c29":           # planes that are not dense: the documented refusal, nothing written
                assert rc == gsd.GSD_ERR_BAD_ARG and b"full contiguous (C,H,W) tensor" in L.gsd_last_error()
                assert bool(torch.isnan(o).all())
            else:
                gsd.check(rc, "conv1x1_out")
            a = R.bnrelu_act(vals, sc, sh)
            best, _ = R.maxpool_route(a)
            w_ = f"{tag} ({'far' if far else 'compact'})"
            assert torch.equal(y.double(), best), f"{w_}: gsd_maxpool2"
            assert torch.equal(pooled_full[..., :wp].double(), best), f"{w_}: gsd_maxpool2_pitched pooled"
            assert torch.equal(act_full[..., :w].double(), a), f"{w_}: gsd_maxpool2_pitched act"
            assert torch.equal(once_full[..., :w].double(), a), f"{w_}: gsd_bnrelu_pitched"
            for t, ww in ((pooled_full, wp), (act_full, w), (once_full, w)):
                _pad_columns_zero(t, ww, w_)
            ref = torch.where(R.bnrelu_mask(vals, sc, sh), dav.double(), torch.zeros((), dtype=torch.float64, device="cuda"))
            assert torch.equal(dz.double(), ref), f"{w_}: gsd_bn_bwd_reduce mode 0 dz"
            assert bool((part[rows * 3 * c:] == TF.SENT).all())
            TP.check_dz_sums(gsd, part, rows, dz, vals, mean, invstd, w_, f"far:{lay}:stats:{tag}" if far else "farc:stats")
            if not (far and lay == "c29"):
                r1, c1 = R.conv1x1_fwd(a, wo.double(), bo.double())
                R.check_bound(o, r1, c1, R.TAU_1X1, f"{w_}: gsd_conv1x1_out", image=n - 1, key=f"far:{lay}:1x1:{tag}" if far else None)
                out.setdefault("o", o.clone())
                assert torch.equal(out["o"], o), f"{w_}: gsd_conv1x1_out differs from the compact launch"
    finally:
        place.restore()
    bad = arena.scan()
    assert not bad, f"{tag}: the launches wrote outside their operands: {bad[:6]}"


# -------------------------------------------------------------------------------------------------------------------- data path
# The dataset arena of the gathers is one dense (M, C, H, W) array: here it IS the arena behind FRONT, M in the millions, and the
# batch names row 0 and the first row behind each of the four lines; only those rows hold data (the rest is fill: a slipped row
# offset reads NaN).  The sources of gsd_ingest_images[_interp] are uint8 / fp32 frames whose image and channel strides cross
# 2^31 and 2^32 BYTES (uint8: the arena's bytes) and elements (fp32).  References, bounds and bit-exactness as in
# tests/test_gpu_data_path_fp64.py and tests/test_gpu_augment.py.
def _far_rows(r, extra=0):
    """Row 0 and, for each line, the first row of r floats that starts behind it (+ extra)."""
    return [0] + [-(-line // r) + extra for line in FL.LINES.values()]


@pytest.mark.parametrize("chw", [(3, 9, 11), (2, 8, 12)], ids=["3x9x11", "2x8x12"])
def test_gathers_far(arena, chw):
    import numpy as np
    import augment_ref as AR
    import data_path_ref as D
    from gelslim_depth_amd import dataset as DS
    from test_gpu_augment import MEAN_STD, DEPTH, TAU_AUG, _dev
    c, h, w = chw
    r = c * h * w
    flat = arena.words.view(torch.float32)
    shift = 5                                        # the depth array starts 5 rows further: its named rows are img rows + 5, unnamed there
    m = (arena.elems - FL.FRONT - shift * r) // r
    img = flat[FL.FRONT:FL.FRONT + m * r].view(m, c, h, w)
    dep = flat[FL.FRONT + shift * r:FL.FRONT + (shift + m) * r].view(m, c, h, w)
    rows = _far_rows(r)
    assert max(rows) < m and all(abs(a - b) != shift for a in rows for b in rows)
    assert [i * r >= line for i, line in zip(rows[1:], FL.LINES.values())] == [True] * 4
    g = torch.Generator().manual_seed(r)
    vi = (torch.rand((len(rows), c, h, w), generator=g) * 255.0)
    vd = (torch.rand((len(rows), c, h, w), generator=g) * -2.0)
    idx = torch.tensor(rows, dtype=torch.int64, device="cuda")
    try:
        img[idx] = vi.cuda()
        dep[idx] = vd.cuda()
        ab_i, ab_d = _dev(MEAN_STD, c), _dev(DEPTH)
        got = DS.gather_affine(img, idx, *ab_i)
        ref, _ = D.gather_affine_ref(vi, list(range(len(rows))), MEAN_STD[0][:c], MEAN_STD[1][:c])
        assert torch.equal(got.cpu().double(), ref.view(got.shape)), "gsd_gather_affine: rows behind the lines are not one fmaf of the source"
        p = AR.params(seed=7, p_hflip=0.5, p_vflip=0.5, max_dy=2, max_dx=3, gain=0.2, offset=12.0, noise_std=0.0, pivot=127.5)
        oi, od = DS.gather_augment(img, dep, idx, *ab_i, *ab_d, AR.lib_struct(p, 3))
        torch.cuda.synchronize()
        compact = list(range(len(rows)))
        for name, out, v, ab, photo in (("image", oi, vi, (MEAN_STD[0][:c], MEAN_STD[1][:c]), True), ("depth", od, vd, DEPTH, False)):
            draws = AR.sample(p, 3, np.asarray(rows), c if photo else 1)        # keyed by the TRUE dataset rows
            rf, cd = AR.gather_augment_ref(v.numpy(), compact, ab[0], ab[1], p, 3, photometry=photo, draws=draws)
            R.check_bound(out, torch.from_numpy(rf).cuda(), torch.from_numpy(cd).cuda(), TAU_AUG, f"gsd_gather_augment {name}",
                          key=f"far:rows:gather:{name}-{c}x{h}x{w}")
    finally:
        for t in (img, dep):
            t.view(torch.int32)[idx] = FL.FILL_I32
    bad = arena.scan()
    assert not bad, f"the gathers wrote into the dataset arena: {bad[:6]}"


INGEST = [("u8", 1, 3 * (1 << 30) + 256, (1 << 30) + 64), ("f32", 4, (1 << 29) + 64, (1 << 27) + 64), ("f32e", 4, (1 << 31) + 64, (1 << 20) + 64)]


@pytest.mark.parametrize("name,esize,ns,cs", INGEST, ids=[i[0] for i in INGEST])
@pytest.mark.parametrize("mode", ["area", "bilinear"])
def test_ingest_images_far(gsd, arena, mode, name, esize, ns, cs):
    """u8: channel 2 of image 0 and image 1 start behind 2^31 bytes, channel 1 of image 1 and image 2 behind 2^32 bytes.  f32: the
    same lines in bytes (n31's image stride).  f32e: image 1 / 2 behind 2^31 / 2^32 ELEMENTS.  The base frames share the strides,
    4096 elements on."""
    import data_path_ref as D
    from gelslim_depth_amd.dataset import INTERP_MODES
    from test_gpu_data_path_fp64 import held
    n, c, h, w, size = 3, 3, 13, 17, (5, 7)
    dt = torch.uint8 if esize == 1 else torch.float32
    raw, base = D.frames(21, n, c, h, w, dt), D.frames(22, n, c, h, w, dt)
    store = arena.words.view(dt)
    first = FL.FRONT * 4 // esize
    assert ns >= c * cs and cs >= h * w + 4096 + h * w
    assert first + 4096 + 2 * ns + 2 * cs + h * w <= store.numel()
    views = [store.as_strided((n, c, h, w), (ns, cs, w, 1), first + k * 4096) for k in (0, 1)]
    out = torch.full((n * c * size[0] * size[1] + 64,), float("nan"), device="cuda")
    try:
        views[0].copy_(raw.cuda())
        views[1].copy_(base.cuda())
        args = (views[0].data_ptr(), views[1].data_ptr(), 1 if esize == 1 else 0, n, c, h, w, ns, cs, ns, cs, out.data_ptr(), size[0], size[1],
                255.0, 0.5, gsd.stream_ptr())
        if mode == "area":
            gsd.check(gsd.lib.gsd_ingest_images(*args), "ingest_images")
        else:
            gsd.check(gsd.lib.gsd_ingest_images_interp(INTERP_MODES[mode], *args), "ingest_images_interp")
        torch.cuda.synchronize()
    finally:
        for k in (0, 1):             # (every plane starts on a word: first, 4096, ns and cs are multiples of 4 elements)
            arena.words.as_strided((n, c, -(-h * w * esize // 4)), (ns * esize // 4, cs * esize // 4, 1),
                                   (first + k * 4096) * esize // 4).fill_(FL.FILL_I32)
    assert bool(torch.isnan(out[-64:]).all())
    got = out[:-64].view(n, c, *size).cpu().numpy()
    if mode == "area":
        ref, cond, n_e = D.area_ref(raw, base, size, [1.0], [0.0])
        held(got, ref, cond, D.area_bound(cond, n_e), f"far ingest_images {name}")
    else:       # the compact launch is the reference of the other modes: the same kernel, so the same bits
        o2 = torch.full_like(out, float("nan"))
        rd, bd = raw.cuda().contiguous(), base.cuda().contiguous()
        gsd.check(gsd.lib.gsd_ingest_images_interp(INTERP_MODES[mode], rd.data_ptr(), bd.data_ptr(), 1 if esize == 1 else 0, n, c, h, w,
                                                   c * h * w, h * w, c * h * w, h * w, o2.data_ptr(), size[0], size[1], 255.0, 0.5,
                                                   gsd.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(out[:-64], o2[:-64]) and bool(torch.isfinite(out[:-64]).all()), \
            f"far ingest_images_interp {name}: differs from the compact launch"          # (which tests/test_gpu_interp.py holds to ATen)
    bad = arena.scan()
    assert not bad, f"ingest wrote into its source: {bad[:6]}"


# ------------------------------------------------------------------------------------- the harness sees the bug it is for
@pytest.mark.parametrize("lay", ["n31", "n33", "c29", "c25"])
def test_truncated_strides_are_rejected_and_stray_stores_found(arena, lay):
    """No library launch.  A tensor gathered through plane offsets cut to 32 bits -- each of the four ways -- is rejected by the
    bound check; one float stored at an alias of each kind that lies in fill is found by the scan, at that word."""
    L = FL.LAYOUTS[lay]
    n, c, h, w = L.max_n, L.max_c or 16, 9, 11
    place = arena.placement(lay)
    t = place.view(n, c, h, w)
    rec = place.recs[-1]
    t.copy_(torch.randn((n, c, h, w), generator=TF.gen(n, c, h, w), device="cuda"))
    ref = t.double()
    cond = ref.abs() + 1.0
    R.check_bound(t, ref, cond, R.TAU_DIRECT, "the tensor itself")
    flat = arena.words.view(torch.float32)
    pix = (torch.arange(h, device="cuda")[:, None] * rec.p + torch.arange(w, device="cuda")[None, :]).view(1, 1, h, w)
    kinds = {}
    for i in range(n):
        for j in range(c):
            for kind, a in FL.aliases(i * rec.n_stride + j * rec.c_stride):
                kinds.setdefault(kind, {})[(i, j)] = a
    assert kinds, "the layout crosses no line"
    for kind, moved in kinds.items():
        base = torch.tensor([[moved.get((i, j), i * rec.n_stride + j * rec.c_stride) for j in range(c)] for i in range(n)],
                            device="cuda", dtype=torch.int64).view(n, c, 1, 1)
        got = flat[rec.off + base + pix]
        try:
            rejects(got, ref, cond, R.TAU_DIRECT, f"{lay}: planes gathered through the {kind}")
        except BaseException:
            place.restore()
            raise
    stray = {}                   # one address in fill per alias kind (two kinds may share one)
    for k, i, j, kind, where, cls in place.alias_report():
        if cls == "fill":
            stray.setdefault(kind, where)
    place.restore()
    assert set(stray) == set(kinds), f"{lay}: an alias kind without a representative in fill: {set(kinds) - set(stray)}"
    assert arena.scan() == []
    for where in set(stray.values()):
        flat[where] = 1.0
    bad = arena.scan()
    assert sorted(bad) == sorted(set(stray.values())), (bad, stray)
    assert arena.scan() == [], "the scan puts back what it reports"
