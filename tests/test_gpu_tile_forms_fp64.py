"""Element-wise fp64 bounds for every tile form and operand form of the fp32 convolution family, at the smallest shapes that
reach them (tests/tile_cases.py; tests/test_tile_form_coverage_cpu.py proves on the CPU that the tables reach every form).

The full-size modules (test_gpu_fp64_bounds.py, test_gpu_fp32_step_fp64.py) hold the kernels to |got - ref| <= tau * cond at the
five level sizes of 3x320x427 only; the small odd shapes of test_gpu_ops.py / test_gpu_kslabs.py only to a whole-tensor relative
L1.  Here every output element of gsd_conv3x3, gsd_conv3x3_w43[_ws], gsd_conv3x3_w2d[_ws], their fused *_dgrad_bnrelu[_ws]
epilogues, gsd_conv3x3_wgrad, gsd_conv3x3_wgrad_bn and the ConvT kernels is checked with fp64_ref.check_bound at shapes that pick:
w2d tiles 64 / 8 wide and 16 / 32 off the pyramid; w43 unfolded 64 / 4 / 8 / 16 / 32 and folded 4 / 8 / 16 / 24 / 28 / 32 / 48 / 64
(56 through GSD_W43_TW=56 GSD_W43_FOLD=1: no small shape picks it), channel counts off a multiple of 4 (FAST = false); both
direct blocks; the dW row form's five stage shapes and the 2-D form's three k-step shapes with every (BM, BN) block; ConvT
forward with and without 16-byte pieces, dX in weight layout modes 7 and 3, the fused dX and dW.

Common to every case: outputs are NaN-filled; every destination, partials buffer and workspace lies inside a larger buffer of
sentinels that must survive (pad columns of a pitched destination, channels next to a channel slice, the floats in front and
behind); every source lies between NaN floats -- the slack a segment vouches for is readable, not zero -- and the pad columns of
a pitched source hold 0 (include/gsd.h).  Which instantiation ran is read from the launch lines GSD_W2D_TRACE / GSD_W43_TRACE /
GSD_WG43_TRACE print.

Worst |got - ref| / cond measured on the MI355X over this module (profiles/fp64_tile_forms.json), against the family's tau --
no family constant had to be widened and the module has no constant of its own:
    w43    1.93e-06  against TAU_WINO = 6.0e-06   (w43-2x5x61-c8+0-m130-slack_bn)
    w2d    1.10e-06  against TAU_WINO = 6.0e-06   (w2d-2x12x45-c8+0-m70-slack_bn)
    direct 3.45e-07  against TAU_DIRECT = 1.6e-06   (direct-2x7x32-c4+4-m130-two04)
    dw     4.89e-07  against TAU_DW = 4.0e-06   (2x15x13-c64+64-m64-pitched-slack4-bn-form2)
    convT  2.83e-07  against TAU_CONVT = 1.9e-06   (convT-3x5x53-k36-m40)
    stats  1.87e-08  against TAU_STATS = 3.4e-08   (w43-2x15x13-c8+0-m130-slack_bn-W43_FOLD=0)

What the module found when it was written: gsd_conv3x3_wgrad refused (GSD_ERR_UNSUPPORTED, "LDS image 165888 B too large") the
1 x 64 stage of the row form with 64 x 64 blocks whenever the activation windows could not move as 16-byte pieces (two segments
with a[0].C off the block size, or no slack) -- e.g. H = 1, W = 40, Cin = 64, Cout = 64; plan_wg43 now takes
32-column blocks for that stage (the case 2x1x40-c20+44-m64 of tile_cases.WG_CASES keeps it covered).  The direct form's
statistics rows sum the whole raw output whether a destination crops it or not (include/gsd.h), unlike the Winograd forms', whose
second (cropped) destination's sums are the ConvT bias gradient: the direct dX cases pass no partials, as the engine does.

GSD_FP64_REPORT_TILES=<path>: write the worst ratio per family and per case there as JSON.

The bodies of the tests are functions (conv_case, fused_case, wgrad_case, wgrad_bn_case, convT_case) and the allocators (source,
Out, Scratch) take a placement: tests/test_gpu_far_strides_fp64.py runs the same launches and checks with every strided operand
carved from an arena in which images and planes lie gigabytes apart (tests/far_layouts.py).
"""
import ctypes as C
import json
import math
import os
import time

import pytest
import torch
import torch.nn.functional as F

import far_layouts as FL
import fp64_ref as R
import tile_cases as T
from conftest import rel_l1
from test_gpu_fp64_bounds import dw_mutation_rejected, forward_mutation_rejected, rejects, sums
from test_gpu_layer_shapes import gsd, layout  # noqa: F401  (gsd: the module fixture)

pytestmark = pytest.mark.gpu

GUARD = 8                   # floats in front of and behind every tensor (32 bytes: the tensor starts 16-byte aligned)
SENT = -12345.0             # what no kernel may overwrite
NAN = float("nan")
KNOBS = ("GSD_W2D_TW", "GSD_W43_TW", "GSD_W43_FOLD", "GSD_W43_SPLIT", "GSD_W2D_SPLIT", "GSD_WGRAD_W2D", "GSD_WG43_TW", "GSD_WG2D_KX")
TAUS = {"w43": R.TAU_WINO, "w2d": R.TAU_WINO, "direct": R.TAU_DIRECT, "dw": R.TAU_DW, "convT": R.TAU_CONVT, "stats": R.TAU_STATS}
T0 = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    T0["t"] = time.time()
    yield
    path = os.environ.get("GSD_FP64_REPORT_TILES")
    if path:
        mine = {k[6:]: v for k, v in R.RATIOS.items() if k.startswith("tiles:")}
        worst = {}
        for k, v in mine.items():
            fam = k.split(":")[0]
            if fam not in worst or v > worst[fam]["ratio"]:
                worst[fam] = {"ratio": v, "tau": TAUS[fam], "case": k.split(":", 1)[1]}
        with open(path, "w") as f:
            json.dump({"wall_s": time.time() - T0["t"], "worst": dict(sorted(worst.items())), "ratios": dict(sorted(mine.items()))},
                      f, indent=1)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a fault in an earlier launch: the context is gone, launch nothing more
        pytest.exit(f"the GPU context is in error ({e}); stopping", returncode=3)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k in ("GSD_W2D_TRACE", "GSD_W43_TRACE", "GSD_WG43_TRACE"):
        monkeypatch.setenv(k, "1")


def _r64(c):
    return (c + 63) // 64 * 64


def _r4(c):
    return (c + 3) // 4 * 4


def gen(*key):
    return torch.Generator(device="cuda").manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def randn(g, *shape, scale=1.0):
    return torch.randn(shape, generator=g, device="cuda") * scale


def uniform(g, lo, hi, *shape):
    return torch.rand(shape, generator=g, device="cuda") * (hi - lo) + lo


def vec(t):
    return t.double().view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------ buffers
def source(g, shape, pitch=None, front=GUARD, positive=False, place=None):
    """A random (n, c, h, w) source tensor with row pitch `pitch` (pad columns 0) between NaN floats: `front` in front (8: the
    tensor starts 16-byte aligned, 5: 4 bytes off) and GUARD behind.  Whatever a kernel reads outside the tensor and its pad
    columns and lets into a result shows as a NaN.
    place: a far_layouts.Placement -- the tensor is carved from its arena instead (the same values, the same alignment class,
    the layout's strides; the arena's fill is the NaN around it)."""
    n, c, h, w = shape
    p = pitch or w
    if place is not None:
        body = place.view(n, c, h, p, misalign=front % 4)
    else:
        flat = torch.full((front + n * c * h * p + GUARD,), NAN, device="cuda")
        body = flat[front:front + n * c * h * p].view(n, c, h, p)
    body.zero_()
    t = body[..., :w]
    t.copy_(torch.rand(shape, generator=g, device="cuda") if positive else torch.randn(shape, generator=g, device="cuda"))
    return t


class Out:
    """An (n, ct, h, w) destination with row pitch `pitch` inside a buffer of sentinels; the launch owns columns < w of channels
    [c_off, c_off + c_len), NaN-filled before the launch.  check(): everything else still holds the sentinel."""

    def __init__(self, shape, pitch=None, c_off=0, c_len=None, fill=NAN, place=None):
        n, ct, h, w = shape
        p = pitch or w
        self.c_off, self.c_len = c_off, ct - c_off if c_len is None else c_len
        self.place, self.w = place, w
        if place is not None:       # carved from a far_layouts arena: its fill pattern is the sentinel
            self.full = place.view(n, ct, h, p)[..., :w]
            self.rec = place.recs[-1]
            self.t = self.full[:, c_off:c_off + self.c_len]
            self.t.fill_(fill)
            return
        self.flat = torch.full((GUARD + n * ct * h * p + GUARD,), SENT, device="cuda")
        self.full = self.flat[GUARD:GUARD + n * ct * h * p].view(n, ct, h, p)[..., :w]
        self.t = self.full[:, c_off:c_off + self.c_len]
        self.t.fill_(fill)
        self.owned = torch.zeros_like(self.flat, dtype=torch.bool)
        self.owned[GUARD:GUARD + n * ct * h * p].view(n, ct, h, p)[:, c_off:c_off + self.c_len, :, :w] = True

    def dst(self, gsd, off=(0, 0)):
        return gsd.make_dst(self.full, c_off=self.c_off, c_len=self.c_len, off=off)

    def check(self, what):
        if self.place is not None:  # pad columns and neighbouring channels here; everything else by the arena's scan
            bad = self.place.int_view(self.rec) != FL.FILL_I32
            bad[:, self.c_off:self.c_off + self.c_len, :, :self.w] = False
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} words of the destination's pad columns / other channels were written"
            return
        bad = (self.flat != SENT) & ~self.owned
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} floats outside the destination were written, first at flat index " \
                                    f"{int(bad.nonzero()[0, 0])} of {self.flat.numel()} (guard {GUARD})"


class Scratch:
    """`need` floats the launch may use (filled with `fill`) and 64 sentinels behind them."""

    def __init__(self, need, fill=0.0, place=None):
        self.need = int(need)
        self.place = place
        if place is not None:
            self.flat = place.view(1, 1, 1, max(self.need, 1) + 64).view(-1)
            self.rec = place.recs[-1]
        else:
            self.flat = torch.full((max(self.need, 1) + 64,), SENT, device="cuda")
        self.flat[:self.need] = fill

    def ptr(self):
        return self.flat.data_ptr()

    def check(self, what):
        if self.place is not None:
            behind = self.place.int_view(self.rec).view(-1)[self.need:]
            assert bool((behind == FL.FILL_I32).all()), f"{what}: written behind its {self.need} floats"
            return
        assert bool((self.flat[self.need:] == SENT).all()), f"{what}: written behind its {self.need} floats"


# ------------------------------------------------------------------------------------------------------- conv3x3 operands
MODES = {"direct": (0, 1), "w43": (4, 5), "w2d": (8, 9)}


second_segment = T.second_segment


class ConvOperands:
    """Sources of a forward case in its operand form (tile_cases.py), the fp64 activation they stand for, and the dX operands
    that mirror them: dy in the same alignment class, one destination per source segment with the segment's offsets."""

    def __init__(self, gsd, c, g, place=None):
        n, h, w, c0, c1 = c.n, c.h, c.w, c.c0, c.c1
        self.c, self.gsd, self.place = c, gsd, place
        form = c.form
        self.bn = form in ("slack_bn", "two04")
        self.sc = uniform(g, 0.5, 1.5, c0) if self.bn else None
        self.sh = randn(g, c0, scale=0.3) if self.bn else None
        self.aligned = form in ("x4", "slice")
        self.slack = 0 if form in ("x4", "slice", "dword") else gsd.SLACK
        ct, self.c_off = (c0 + 5, 3) if form == "slice" else (c0, 0)
        self.raw0 = source(g, (n, ct, h, w), pitch=_r4(w) if self.aligned else None, front=5 if form == "dword" else GUARD, place=place)
        self.segs = [gsd.make_src(self.raw0, self.sc, self.sh, relu=self.bn, c_off=self.c_off, c_len=c0, slack=self.slack)]
        r0 = self.raw0[:, self.c_off:self.c_off + c0]
        a = R.deferred_act(r0, self.sc, self.sh) if self.bn else r0.double()
        self.geom = [(0, 0, h, w)]
        if c1:
            oh, ow, uh, uw = second_segment(form, h, w)
            self.up = source(g, (n, c1, uh, uw), place=place)
            self.segs.append(gsd.make_src(self.up, off=(oh, ow), slack=self.slack))
            a = torch.cat([a, F.pad(self.up.double(), [ow, w - uw - ow, oh, h - uh - oh])], 1)
            self.geom.append((oh, ow, uh, uw))
        self.act = a
        self.src = gsd.src_array(self.segs)

    def dy(self, g, co):
        c = self.c
        t = source(g, (c.n, co, c.h, c.w), pitch=_r4(c.w) if self.aligned else None, front=5 if c.form == "dword" else GUARD,
                   place=self.place)
        return t, self.gsd.make_src(t, slack=self.slack)

    def dx_outs(self):
        c = self.c
        outs = []
        for (oh, ow, uh, uw), ch in zip(self.geom, (c.c0, c.c1)):
            pitch = _r4(uw) if self.aligned else uw + 1
            outs.append(Out((c.n, ch + 5, uh, uw), pitch, 3, ch, place=self.place) if c.form == "slice"
                        else Out((c.n, ch, uh, uw), pitch, place=self.place))
        return outs


def trace_line(capfd, prefix):
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith(prefix + " ")]
    assert lines, f"no {prefix} launch line on stderr"
    return lines[-1], len(lines)


def field(line, name):
    tok = line.replace("|", " ").split()
    return tok[tok.index(name) + 1]


def expected_halo_form(fam, plan, segs, plain):
    """The (x4, u4 / fast) fields the launchers derive from the operands (w2d_impl / w43_impl), from the descriptors."""
    def al(s):
        return s.ptr % 16 == 0 and s.w_stride % 4 == 0 and s.c_stride % 4 == 0 and s.n_stride % 4 == 0
    np_ = plan.TW // 4 + 2
    wr = plan.TH + 2
    if fam == "w2d":
        ni = -(-wr * np_ // 64)
        s = segs[0]
        x4 = plain and len(segs) == 1 and 4 * ni <= 8 and al(s) and s.off_h == 0 and s.off_w == 0 and s.w_stride >= _r4(s.W)
        u4 = (not x4) and 4 * ni <= 8 and all(s.slack >= 4 for s in segs)
        return int(x4), int(u4)
    ni = -(-wr // (64 // np_))
    x4 = ni <= 2 and all(al(s) and s.off_w % 4 == 0 for s in segs)
    cin = sum(s.C for s in segs)
    fast = cin % 4 == 0 and (len(segs) == 1 or segs[0].C % 4 == 0)
    return int(x4), int(fast)


def launch_conv(gsd, fam, srcs, nsrc, wl, cin, cout, dsts, part, n, h, w, split, place=None):
    """One forward / dX launch: the K-slab entry point with the scratch the library asks for when the case forces a split.
    Returns the scratch (or None)."""
    L, st = gsd.lib, gsd.stream_ptr()
    darr = gsd.dst_array(dsts)
    if fam == "direct":
        gsd.check(L.gsd_conv3x3(srcs, nsrc, wl.data_ptr(), cin, cout, darr, len(dsts), part, n, h, w, st), "gsd_conv3x3")
        return None
    fn = getattr(L, f"gsd_conv3x3_{fam}")
    if not split:
        gsd.check(fn(srcs, nsrc, wl.data_ptr(), cin, cout, darr, len(dsts), part, n, h, w, st), f"gsd_conv3x3_{fam}")
        return None
    need = getattr(L, f"gsd_conv3x3_{fam}_workspace")(n, h, w, cin, cout)
    assert need > 0, "a forced slab count applies wherever the shape admits it"
    ws = Scratch(need, NAN, place=place)
    gsd.check(getattr(L, f"gsd_conv3x3_{fam}_ws")(srcs, nsrc, wl.data_ptr(), cin, cout, darr, len(dsts), part, ws.ptr(), need,
                                                   n, h, w, st), f"gsd_conv3x3_{fam}_ws")
    return ws


def check_stats(gsd, part, rows, c_total, stored, conds, what, key):
    """Statistics rows of a launch through gsd_bn_reduce_partials against fp64 sums of the values it stored: `stored` / `conds`
    list (first channel, stored tensor, cond tensor) per destination."""
    g1, g2 = sums(gsd, part.flat, rows, _r64(c_total), c_total)
    for (c_lo, y), (_, cond) in zip(stored, conds):
        y64 = y.double()
        ch = slice(c_lo, c_lo + y.shape[1])
        R.check_sums(g1[ch], y64.sum((0, 2, 3)), cond.sum((0, 2, 3)), R.TAU_STATS, f"{what} sum", key=key)
        R.check_sums(g2[ch], (y64 * y64).sum((0, 2, 3)), (cond * cond).sum((0, 2, 3)), R.TAU_STATS, f"{what} sum of squares", key=key)


ALL_CONV = T.CONV_CASES + T.SPLIT_CASES


@pytest.mark.parametrize("case", ALL_CONV, ids=[T.case_id(c) for c in ALL_CONV])
def test_conv3x3_forward_and_dx_tile_form(gsd, monkeypatch, capfd, case):
    conv_case(gsd, monkeypatch, capfd, case)


def conv_case(gsd, monkeypatch, capfd, case, place=None, ns="tiles"):
    """One forward + statistics and one dX launch of `case`, every check of this module on them.  place: carve every strided
    operand, the partials and the K-slab scratch from a far_layouts arena; ns: the prefix of the keys in fp64_ref.RATIOS.
    Returns what the launches stored (compact copies) and the launch line, for a caller that compares two placements."""
    c = case
    res = {}
    fam, n, h, w, co = c.fam, c.n, c.h, c.w, c.co
    ci = c.c0 + c.c1
    for k, v in T.env_of(c).items():
        monkeypatch.setenv(k, v)
    split = any(k.endswith("_SPLIT") for k, _ in c.env)
    L = gsd.lib
    g = gen(n, h, w, ci, co, len(c.form), len(fam))
    tag = T.case_id(c)
    tau = TAUS[fam]
    assert tau <= R.ceiling(max(ci, co))
    op = ConvOperands(gsd, c, g, place)
    wd = randn(g, co, ci, 3, 3, scale=1.0 / (9 * ci) ** 0.5)
    w64 = wd.double()
    plan = T.conv_plan(fam, n, h, w, co, T.env_of(c))
    rows_fn = {"direct": L.gsd_conv3x3_partial_rows, "w43": L.gsd_conv3x3_w43_partial_rows, "w2d": L.gsd_conv3x3_w2d_partial_rows}[fam]

    if fam == "w2d" and (ci % 4 or c.c0 % 4):
        pytest.fail("table error: w2d cases must have channel counts on a multiple of 4")

    # ---- forward + statistics
    rows = rows_fn(n, h, w, co)
    assert rows == T.conv_partial_rows(fam, n, h, w, co, T.env_of(c))
    y = Out((n, co + 5, h, w), _r4(w), 3, co, place=place) if c.form == "slice" \
        else Out((n, co, h, w), _r4(w) if op.aligned else w + 1, place=place)
    part = Scratch(rows * 2 * _r64(co), place=place)
    capfd.readouterr()
    ws = launch_conv(gsd, fam, op.src, len(op.segs), layout(gsd, MODES[fam][0], wd, co, ci), ci, co, [y.dst(gsd)], part.ptr(),
                     n, h, w, split, place)
    torch.cuda.synchronize()
    if fam != "direct":
        line, _ = trace_line(capfd, fam)
        res["line"] = line
        assert field(line, "tile") == f"{plan.TH}x{plan.TW}", line
        assert int(field(line, "plain")) == int(not op.bn), line
        assert int(field(line, "slabs")) == (int(dict(c.env)[f"GSD_{fam.upper()}_SPLIT"]) if split else 1), line
        x4, other = expected_halo_form(fam, plan, op.segs, not op.bn)
        assert int(field(line, "x4")) == x4, line
        assert int(field(line, "u4" if fam == "w2d" else "fast")) == other, line
        if fam == "w43":
            assert int(field(line, "fold")) == plan.fold, line
    ref, cond = R.conv3x3_fwd(op.act, w64)
    R.check_bound(y.t, ref, cond, tau, f"{tag} forward", image=n - 1, key=f"{ns}:{fam}:{tag}")
    res["y"], res["part"] = y.t.clone(), part.flat[:part.need].clone()
    y.check(f"{tag} forward")
    part.check(f"{tag} forward partials")
    if ws is not None:
        ws.check(f"{tag} forward K-slab scratch")
    check_stats(gsd, part, rows, co, [(0, y.t)], [(0, cond)], f"{tag} forward", f"{ns}:stats:{tag}")
    forward_mutation_rejected(op.act[-1:], w64, y.t[n - 1:n], ref[-1:], cond[-1:], tau, f"{tag} forward")

    # ---- dX: dy in the same alignment class, one (cropped) destination per source segment
    # (the two-dimensional form contracts over whole 4-channel chunks: its dX takes a gradient of round_up(Cout, 4) channels)
    kd = _r4(co) if fam == "w2d" else co
    if kd != co:
        wd = randn(g, kd, ci, 3, 3, scale=1.0 / (9 * ci) ** 0.5)
        w64 = wd.double()
    dy, sdy = op.dy(g, kd)
    outs = op.dx_outs()
    rows_d = rows_fn(n, h, w, ci)
    # statistics of the two (cropped) destinations, as the engine takes the ConvT bias gradient from them -- of the Winograd forms
    # only: the direct form sums the whole raw output, cropped or not (include/gsd.h), and the engine never asks it
    part_d = Scratch(rows_d * 2 * _r64(ci), place=place) if len(outs) == 2 and fam != "direct" else None
    dsts = [o.dst(gsd, off=(oh, ow)) for o, (oh, ow, _, _) in zip(outs, op.geom)]
    ws = launch_conv(gsd, fam, gsd.src_array([sdy]), 1, layout(gsd, MODES[fam][1], wd, kd, ci), kd, ci, dsts,
                     part_d.ptr() if part_d else None, n, h, w, split, place)
    torch.cuda.synchronize()
    if fam != "direct":
        res["line_dx"] = trace_line(capfd, fam)[0]
    ref, cond = R.conv3x3_dx(dy.double(), w64)
    stored, conds, lo = [], [], 0
    for o, (oh, ow, uh, uw) in zip(outs, op.geom):
        ch = o.t.shape[1]
        r_, c_ = ref[:, lo:lo + ch, oh:oh + uh, ow:ow + uw], cond[:, lo:lo + ch, oh:oh + uh, ow:ow + uw]
        R.check_bound(o.t, r_, c_, tau, f"{tag} dX segment at ({oh},{ow})", image=n - 1, key=f"{ns}:{fam}:{tag}")
        res[f"dx{len(stored)}"] = o.t.clone()
        o.check(f"{tag} dX segment at ({oh},{ow})")
        stored.append((lo, o.t))
        conds.append((lo, c_))
        lo += ch
    if part_d is not None:
        part_d.check(f"{tag} dX partials")
        check_stats(gsd, part_d, rows_d, ci, stored, conds, f"{tag} dX", f"{ns}:stats:{tag}")
        res["part_d"] = part_d.flat[:part_d.need].clone()
    if ws is not None:
        ws.check(f"{tag} dX K-slab scratch")
    return res


@pytest.mark.parametrize("c0,c1", [(5, 0), (6, 5), (8, 6)])
def test_w2d_refuses_channel_counts_off_a_multiple_of_4(gsd, c0, c1):
    """Channels off a multiple of 4 belong to gsd_conv3x3_w43 (FAST = false): the two-dimensional form must refuse them."""
    n, h, w, co = 2, 9, 11, 8
    g = gen(c0, c1)
    segs = [gsd.make_src(source(g, (n, c0, h, w)), slack=gsd.SLACK)]
    if c1:
        segs.append(gsd.make_src(source(g, (n, c1, h, w)), slack=gsd.SLACK))
    ci = c0 + c1
    y = Out((n, co, h, w))
    wl = torch.zeros(gsd.lib.gsd_weight_layout_size(8, co, _r4(ci)) + 64, device="cuda")
    rc = gsd.lib.gsd_conv3x3_w2d(gsd.src_array(segs), len(segs), wl.data_ptr(), ci, co, gsd.dst_array([y.dst(gsd)]), 1, None, n, h, w,
                                 gsd.stream_ptr())
    torch.cuda.synchronize()
    assert rc == gsd.GSD_ERR_UNSUPPORTED
    assert bool(torch.isnan(y.t).all()), "a refused launch writes nothing"
    y.check("refused w2d launch")


# ------------------------------------------------------------------------------------------------------- fused dX epilogue
@pytest.mark.parametrize("case", T.FUSED_CASES, ids=[f"{c.fam}-{c.n}x{c.h}x{c.w}-k{c.co}-m{c.ci}" + "".join(f"-{k[4:]}={v}" for k, v in c.env)
                                                     for c in T.FUSED_CASES])
def test_fused_dx_epilogue_tile_form(gsd, monkeypatch, case):
    """gsd_conv3x3[_w43|_w2d]_dgrad_bnrelu[_ws]: dz = dX * [fmaf(raw, scale, shift) > 0] against the exact mask, and both sums
    (sum dz, sum dz * xhat) of the values stored."""
    fused_case(gsd, monkeypatch, case)


def fused_case(gsd, monkeypatch, case, place=None, ns="tiles"):
    """The launch and checks of test_fused_dx_epilogue_tile_form; place / ns / the return value as conv_case (raw shares dz's
    strides, so it shares its placement)."""
    c = case
    fam, n, h, w, co, ci = c.fam, c.n, c.h, c.w, c.co, c.ci
    for k, v in T.env_of(c).items():
        monkeypatch.setenv(k, v)
    split = any(k.endswith("_SPLIT") for k, _ in c.env)
    L, st = gsd.lib, gsd.stream_ptr()
    g = gen(n, h, w, ci, co, 17, len(fam))
    tag = f"fused-{fam}-{n}x{h}x{w}-k{co}-m{ci}" + ("-split" if split else "")
    tau = TAUS[fam]
    pitched = fam != "direct"          # the direct form takes row-contiguous sources only
    dy = source(g, (n, co, h, w), pitch=_r4(w) if pitched else None, place=place)
    raw = source(g, (n, ci, h, w), place=place)
    sc, sh = uniform(g, 0.5, 1.5, ci), randn(g, ci, scale=0.3)
    mean, invstd = randn(g, ci, scale=0.3), uniform(g, 0.5, 2.0, ci)
    wd = randn(g, co, ci, 3, 3, scale=1.0 / (9 * co) ** 0.5)
    rows_fn = {"direct": L.gsd_conv3x3_partial_rows, "w43": L.gsd_conv3x3_w43_partial_rows, "w2d": L.gsd_conv3x3_w2d_partial_rows}[fam]
    rows = rows_fn(n, h, w, ci)
    part = Scratch(rows * 2 * _r64(ci), place=place)
    dz = Out((n, ci, h, w), place=place)
    s, d = gsd.make_src(dy), dz.dst(gsd)
    wl = layout(gsd, MODES[fam][1], wd, co, ci)
    name = "gsd_conv3x3_dgrad_bnrelu" if fam == "direct" else f"gsd_conv3x3_{fam}_dgrad_bnrelu"
    args = (C.byref(s), wl.data_ptr(), co, ci, C.byref(d), raw.data_ptr(), sc.data_ptr(), sh.data_ptr(), mean.data_ptr(),
            invstd.data_ptr(), part.ptr())
    ws = None
    if split:
        need = getattr(L, f"gsd_conv3x3_{fam}_workspace")(n, h, w, co, ci)
        assert need > 0
        ws = Scratch(need, NAN, place=place)
        gsd.check(getattr(L, name + "_ws")(*args, ws.ptr(), need, n, h, w, st), name + "_ws")
    else:
        gsd.check(getattr(L, name)(*args, n, h, w, st), name)
    torch.cuda.synchronize()
    ref, cond = R.conv3x3_dx(dy.double(), wd.double())
    m = R.bnrelu_mask(raw, sc, sh)
    ref, cond = ref * m, cond * m
    R.check_bound(dz.t, ref, cond, tau, f"{tag} dz", image=n - 1, key=f"{ns}:{fam}:{tag}")
    res = {"dz": dz.t.clone(), "part": part.flat[:part.need].clone()}
    assert bool((dz.t[~m] == 0).all()), "dz is exactly 0 where the mask is off"
    dz.check(f"{tag} dz")
    part.check(f"{tag} partials")
    if ws is not None:
        ws.check(f"{tag} K-slab scratch")
    q1, q2 = sums(gsd, part.flat, rows, _r64(ci), ci)
    xhat = (raw.double() - vec(mean)) * vec(invstd)
    z64 = dz.t.double()
    R.check_sums(q1, z64.sum((0, 2, 3)), cond.sum((0, 2, 3)), R.TAU_STATS, f"{tag} sum dz", key=f"{ns}:stats:{tag}")
    R.check_sums(q2, (z64 * xhat).sum((0, 2, 3)), (cond * xhat.abs()).sum((0, 2, 3)), R.TAU_STATS, f"{tag} sum dz*xhat",
                 key=f"{ns}:stats:{tag}")
    # one product removed from the corner pixel of the last image (where the mask lets it through)
    if bool(m[n - 1, 0, h - 1, w - 1]):
        win = F.pad(dy[n - 1:n].double(), [1, 1, 1, 1])[0, :, h - 1:h + 2, w - 1:w + 2]
        prods = wd.double()[:, 0].flip(1, 2) * win
        p = prods.reshape(-1)[int(prods.abs().reshape(-1).argmax())]
        got = dz.t[n - 1:n].double().clone()
        got[0, 0, h - 1, w - 1] -= p
        rejects(got.float(), ref[-1:], cond[-1:], tau, f"{tag}: largest product removed")
    return res


# --------------------------------------------------------------------------------------------------------------------- dW
def _wg_id(c):
    return f"{c.n}x{c.h}x{c.w}-c{c.c0}+{c.c1}-m{c.co}-{'pitched' if c.pitched else 'flat'}-slack{c.slack}{'-bn' if c.bn else ''}" \
           f"-form{c.form}" + "".join(f"-{k[4:]}={v}" for k, v in c.env)


@pytest.mark.parametrize("case", T.WG_CASES, ids=[_wg_id(c) for c in T.WG_CASES])
def test_conv3x3_wgrad_stage_shapes(gsd, monkeypatch, capfd, case):
    wgrad_case(gsd, monkeypatch, capfd, case)


def wgrad_case(gsd, monkeypatch, capfd, case, place=None, ns="tiles", form=None):
    """The launch and checks of test_conv3x3_wgrad_stage_shapes; place / ns / the return value as conv_case (dW itself and the
    workspace are dense and stay outside the arena).  form: the form the library must report under this placement when it is
    not the case's own (a documented fall-back)."""
    c = case
    form = c.form if form is None else form
    n, h, w, c0, c1, co = c.n, c.h, c.w, c.c0, c.c1, c.co
    ci = c0 + c1
    for k, v in T.env_of(c).items():
        monkeypatch.setenv(k, v)
    L, st = gsd.lib, gsd.stream_ptr()
    g = gen(n, h, w, ci, co, c.form, c.slack)
    tag = _wg_id(c)
    sc, sh = (uniform(g, 0.5, 1.5, c0), randn(g, c0, scale=0.3)) if c.bn else (None, None)
    raw0 = source(g, (n, c0, h, w), place=place)
    segs = [gsd.make_src(raw0, sc, sh, relu=c.bn, slack=c.slack)]
    act = R.deferred_act(raw0, sc, sh) if c.bn else raw0.double()
    if c1:
        oh, ow, uh, uw = second_segment("two11", h, w)
        up = source(g, (n, c1, uh, uw), place=place)
        segs.append(gsd.make_src(up, off=(oh, ow), slack=c.slack))
        act = torch.cat([act, F.pad(up.double(), [ow, w - uw - ow, oh, h - uh - oh])], 1)
    dy = source(g, (n, co, h, w), pitch=_r4(w) if c.pitched else None, place=place)
    sdy = gsd.make_src(dy)
    src = gsd.src_array(segs)
    assert L.gsd_conv3x3_wgrad_form(src, len(segs), C.byref(sdy), ci, co, n, h, w) == form
    need = L.gsd_conv3x3_wgrad_workspace(n, h, w, ci, co)
    assert need == T.wgrad_workspace(n, h, w, ci, co, T.env_of(c))
    ws = Scratch(need, NAN)
    dw = Out((co, ci, 3, 3))
    capfd.readouterr()
    gsd.check(L.gsd_conv3x3_wgrad(src, len(segs), C.byref(sdy), ci, co, dw.t.data_ptr(), ws.ptr(), need, n, h, w, st), "gsd_conv3x3_wgrad")
    torch.cuda.synchronize()
    if form == 0:                    # the direct-tap form prints no launch line
        line = "direct"
    elif form == 1:
        p = T.plan_wg43(n, h, w, co, ci, T.env_of(c))
        line, _ = trace_line(capfd, "wg43")
        assert field(line, "tile") == f"{p.TH}x{p.TW}" and int(field(line, "BM")) == p.BM and int(field(line, "BN")) == p.BN, line
        aligned = sdy.w_stride % 4 == 0 and sdy.c_stride % 4 == 0 and sdy.n_stride % 4 == 0 and sdy.ptr % 16 == 0
        assert int(field(line, "ax4")) == int(aligned), line
        if not aligned or c.slack < 4 or (c1 and c0 % p.BN):
            assert int(field(line, "bx4")) == 0, line
        if dict(c.env).get("GSD_WGRAD_W2D") == 0:
            assert int(field(line, "bx4")) == 1 and int(field(line, "rr")) == (1 if p.TW == 16 else 2), line
    else:
        p = T.plan_wg2d(n, h, w, co, ci, T.env_of(c))
        line, _ = trace_line(capfd, "wg2d")
        assert field(line, "kstep") == f"{p.KY}x{p.KX}" and int(field(line, "BM")) == p.BM and int(field(line, "BN")) == p.BN, line
    assert form == 0 or int(field(line, "plain")) == int(not c.bn), line
    ref, cond = R.conv3x3_dw(act, dy.double())
    R.check_bound(dw.t, ref, cond, R.TAU_DW, f"{tag} dW", key=f"{ns}:dw:{tag}", weights=True)
    dw.check(f"{tag} dW")
    ws.check(f"{tag} dW workspace")
    dw_mutation_rejected(act[n - 1:n], dy[n - 1:n].double(), dw.t, ref, cond, R.TAU_DW, f"{tag} dW")
    return {"dw": dw.t.clone(), "line": line}


@pytest.mark.parametrize("n,h,w", T.WGRAD_BN_SHAPES, ids=[f"{n}x{h}x{w}" for n, h, w in T.WGRAD_BN_SHAPES])
def test_first_layer_wgrad_bn_small_shapes(gsd, n, h, w):
    """gsd_conv3x3_wgrad_bn (3 -> 64): forms d_raw = scale * (dz - c1 - (raw - mean) * invstd * c2) itself."""
    wgrad_bn_case(gsd, n, h, w)


def wgrad_bn_case(gsd, n, h, w, place=None, ns="tiles"):
    """The launch and checks of test_first_layer_wgrad_bn_small_shapes; place: the input image `a`, the entry point's only strided
    operand (dz and raw are dense by contract)."""
    L, st = gsd.lib, gsd.stream_ptr()
    ci, co = 3, 64
    g = gen(n, h, w, 3)
    tag = f"wgrad_bn-{n}x{h}x{w}"
    assert L.gsd_conv3x3_wgrad_bn_supported(n, h, w, ci, co) == 1
    x = source(g, (n, ci, h, w), positive=True, place=place)
    y, dz = source(g, (n, co, h, w)), source(g, (n, co, h, w))
    sc, mu = uniform(g, 0.5, 1.5, co), randn(g, co, scale=0.3)
    istd, k1, k2 = uniform(g, 0.5, 2.0, co), randn(g, co, scale=0.1), randn(g, co, scale=0.1)
    need = L.gsd_conv3x3_wgrad_bn_workspace(n, h, w, ci, co)
    ws = Scratch(need, NAN)
    dw = Out((co, ci, 3, 3))
    a_src = gsd.make_src(x)
    gsd.check(L.gsd_conv3x3_wgrad_bn(C.byref(a_src), dz.data_ptr(), y.data_ptr(), sc.data_ptr(), mu.data_ptr(), istd.data_ptr(),
                                     k1.data_ptr(), k2.data_ptr(), ci, co, dw.t.data_ptr(), ws.ptr(), need, n, h, w, st))
    torch.cuda.synchronize()
    t = (y.double() - vec(mu)) * vec(istd) * vec(k2)
    d = vec(sc) * (dz.double() - vec(k1) - t)
    da = vec(sc) * (dz.double().abs() + vec(k1).abs() + t.abs())
    ref, cond = R.conv3x3_dw(x.double(), d, da)
    R.check_bound(dw.t, ref, cond, R.TAU_DW, f"{tag} dW", key=f"{ns}:dw:{tag}", weights=True)
    dw.check(f"{tag} dW")
    ws.check(f"{tag} workspace")
    dw_mutation_rejected(x[n - 1:n].double(), d[n - 1:n], dw.t, ref, cond, R.TAU_DW, f"{tag} dW")
    return {"dw": dw.t.clone()}


# ------------------------------------------------------------------------------------------------------------------ ConvT
@pytest.mark.parametrize("n,h,w,ci,co", T.CONVT_CASES, ids=[f"{n}x{h}x{w}-k{ci}-m{co}" for n, h, w, ci, co in T.CONVT_CASES])
def test_convT_small_shapes(gsd, n, h, w, ci, co):
    """gsd_convT2x2 (H*W on and off a multiple of 4: with and without 16-byte pieces; 1 and 2 m-blocks), gsd_convT2x2_dgrad_as in
    weight layout mode 7 (odd W with the 2 floats of slack it asks for) and mode 3 (block <1,4> for Cin <= 64, <2,2> above),
    gsd_convT2x2_dgrad_bnrelu and gsd_convT2x2_wgrad."""
    convT_case(gsd, n, h, w, ci, co)


def convT_case(gsd, n, h, w, ci, co, place=None, ns="tiles"):
    """The launches and checks of test_convT_small_shapes; place / ns / the return value as conv_case (dW, db and the workspace are
    dense and stay outside the arena)."""
    L, st = gsd.lib, gsd.stream_ptr()
    g = gen(n, h, w, ci, co)
    tag = f"convT-{n}x{h}x{w}-k{ci}-m{co}"
    key = f"{ns}:convT:{tag}"
    res = {}
    bn = ci != 36          # two cases from a deferred BatchNorm + ReLU source, two from a plain one
    raw = source(g, (n, ci, h, w), place=place)
    sc, sh = (uniform(g, 0.5, 1.5, ci), randn(g, ci, scale=0.3)) if bn else (None, None)
    x64 = R.deferred_act(raw, sc, sh) if bn else raw.double()
    wd, bd = randn(g, ci, co, 2, 2, scale=1.0 / ci ** 0.5), randn(g, co)
    w64 = wd.double()
    s = gsd.make_src(raw, sc, sh, relu=bn)
    y = Out((n, co, 2 * h, 2 * w), place=place)
    d = y.dst(gsd)
    gsd.check(L.gsd_convT2x2(C.byref(s), layout(gsd, 6, wd, co, ci).data_ptr(), bd.data_ptr(), ci, co, C.byref(d), n, h, w, st))
    torch.cuda.synchronize()
    ref, cond = R.convT_fwd(x64, w64, bd.double())
    R.check_bound(y.t, ref, cond, R.TAU_CONVT, f"{tag} forward", image=n - 1, key=key)
    res["y"] = y.t.clone()
    y.check(f"{tag} forward")
    prods = w64[:, 0, 1, 1] * x64[n - 1, :, h - 1, w - 1]        # one product removed from the last pixel of the last image
    got = y.t[n - 1:n].double().clone()
    got[0, 0, 2 * h - 1, 2 * w - 1] -= prods[int(prods.abs().argmax())]
    rejects(got.float(), ref[-1:], cond[-1:], R.TAU_CONVT, f"{tag} forward: largest product removed")

    dy = source(g, (n, co, 2 * h, 2 * w), place=place)
    slack = 2 if w % 2 else 0
    sdy = gsd.make_src(dy, slack=slack)
    assert L.gsd_convT2x2_dgrad_layout(C.byref(sdy), ci, co, n, h, w) == 7
    bare = gsd.make_src(dy)
    assert L.gsd_convT2x2_dgrad_layout(C.byref(bare), ci, co, n, h, w) == (3 if w % 2 else 7)
    ref, cond = R.convT_dx(dy.double(), w64)
    for mode, sd in ((7, sdy), (3, bare)):
        dx = Out((n, ci, h, w), place=place)
        dd = dx.dst(gsd)
        gsd.check(L.gsd_convT2x2_dgrad_as(mode, C.byref(sd), layout(gsd, mode, wd, co, ci).data_ptr(), ci, co, C.byref(dd), n, h, w, st),
                  f"dgrad mode {mode}")
        torch.cuda.synchronize()
        R.check_bound(dx.t, ref, cond, R.TAU_CONVT, f"{tag} dX (mode {mode})", image=n - 1, key=key)
        res[f"dx{mode}"] = dx.t.clone()
        dx.check(f"{tag} dX (mode {mode})")

    rows = L.gsd_convT2x2_dgrad_bnrelu_partial_rows(C.byref(sdy), ci, co, n, h, w)
    assert rows == -(-n * h * (w + w % 2) // 128) * 2
    rs, rh = uniform(g, 0.5, 1.5, ci), randn(g, ci, scale=0.3)
    mean, invstd = randn(g, ci, scale=0.3), uniform(g, 0.5, 2.0, ci)
    part = Scratch(rows * 2 * _r64(ci), place=place)
    dz = Out((n, ci, h, w), place=place)
    dd = dz.dst(gsd)
    gsd.check(L.gsd_convT2x2_dgrad_bnrelu(C.byref(sdy), layout(gsd, 7, wd, co, ci).data_ptr(), ci, co, C.byref(dd), raw.data_ptr(),
                                          rs.data_ptr(), rh.data_ptr(), mean.data_ptr(), invstd.data_ptr(), part.ptr(), n, h, w, st))
    torch.cuda.synchronize()
    m = R.bnrelu_mask(raw, rs, rh)
    rm, cm = ref * m, cond * m
    R.check_bound(dz.t, rm, cm, R.TAU_CONVT, f"{tag} dX fused", image=n - 1, key=key)
    res["dz"], res["part"] = dz.t.clone(), part.flat[:part.need].clone()
    dz.check(f"{tag} dX fused")
    part.check(f"{tag} dX fused partials")
    q1, q2 = sums(gsd, part.flat, rows, _r64(ci), ci)
    xhat = (raw.double() - vec(mean)) * vec(invstd)
    z64 = dz.t.double()
    R.check_sums(q1, z64.sum((0, 2, 3)), cm.sum((0, 2, 3)), R.TAU_STATS, f"{tag} fused dX sum dz", key=f"{ns}:stats:{tag}")
    R.check_sums(q2, (z64 * xhat).sum((0, 2, 3)), (cm * xhat.abs()).sum((0, 2, 3)), R.TAU_STATS, f"{tag} fused dX sum dz*xhat",
                 key=f"{ns}:stats:{tag}")

    need = L.gsd_convT2x2_wgrad_workspace(n, h, w, ci, co)
    ws = Scratch(need, NAN)
    dw, db = Out((ci, co, 2, 2)), Out((1, 1, 1, co))
    if place is not None:
        # the bias gradient sums dy as one dense array: a strided dy is refused before anything is launched; dW alone takes it
        rc = L.gsd_convT2x2_wgrad(C.byref(s), C.byref(bare), ci, co, dw.t.data_ptr(), db.t.data_ptr(), ws.ptr(), need, n, h, w, st)
        torch.cuda.synchronize()
        assert rc == gsd.GSD_ERR_UNSUPPORTED and b"bias gradient needs a contiguous dy" in L.gsd_last_error()
        assert bool(torch.isnan(dw.t).all()) and bool(torch.isnan(db.t).all()) and bool(torch.isnan(ws.flat[:need]).all()), \
            "a refused launch writes nothing"
        gsd.check(L.gsd_convT2x2_wgrad(C.byref(s), C.byref(bare), ci, co, dw.t.data_ptr(), None, ws.ptr(), need, n, h, w, st))
        db.t.copy_(dy.sum((0, 2, 3)).view(1, 1, 1, co))      # (torch's sum: not what is under test here)
    else:
        gsd.check(L.gsd_convT2x2_wgrad(C.byref(s), C.byref(bare), ci, co, dw.t.data_ptr(), db.t.data_ptr(), ws.ptr(), need, n, h, w, st))
    torch.cuda.synchronize()
    rw, cw, rb, cb = R.convT_dw(x64, dy.double())
    R.check_bound(dw.t, rw, cw, R.TAU_CONVT, f"{tag} dW", key=key, weights=True)
    R.check_bound(db.t.view(co), rb, cb, R.TAU_CONVT, f"{tag} db", key=key, weights=True)
    res["dw"] = dw.t.clone()
    if place is None:
        res["db"] = db.t.clone()
    dw.check(f"{tag} dW")
    db.check(f"{tag} db")
    ws.check(f"{tag} dW workspace")
    rows_ = torch.einsum("ip,op->io", x64[n - 1].reshape(ci, h * w)[:, :w], dy[n - 1].double()[:, 0, 0:2 * w:2])   # image row 0, tap (0,0)
    got = dw.t.double().clone()
    got[:, :, 0, 0] -= rows_
    rejects(got.float(), rw, cw, R.TAU_CONVT, f"{tag} dW: one image row removed", weights=True)
    return res


# ------------------------------------------------------------------------------------------------------ the metric's blind spot
def test_relative_l1_passes_what_the_bound_rejects(gsd):
    """At (1, 64, 64, 40, 53) -- the shape tests/test_gpu_ops.py holds to a whole-tensor relative L1 < 2e-5 -- one interior
    output element replaced by 0 still passes that metric; the per-element bound rejects it."""
    n, ci, co, h, w = 1, 64, 64, 40, 53
    g = gen(n, ci, co, h, w)
    x = source(g, (n, ci, h, w))
    wd = randn(g, co, ci, 3, 3, scale=1.0 / (9 * ci) ** 0.5)
    y = Out((n, co, h, w))
    gsd.check(gsd.lib.gsd_conv3x3_w43(gsd.src_array([gsd.make_src(x)]), 1, layout(gsd, 4, wd, co, ci).data_ptr(), ci, co,
                                      gsd.dst_array([y.dst(gsd)]), 1, None, n, h, w, gsd.stream_ptr()))
    torch.cuda.synchronize()
    ref, cond = R.conv3x3_fwd(x.double(), wd.double())
    R.check_bound(y.t, ref, cond, R.TAU_WINO, "40x53 forward", key="tiles:w43:blind-spot-1x64x64x40x53")
    y.check("40x53 forward")
    bad = y.t.clone()
    i = int((ref[0, 17, 5:35, 5:48].abs() - 1.0).abs().reshape(-1).argmin())          # an interior element of ordinary size
    r, col = 5 + i // 43, 5 + i % 43
    assert 0.5 < abs(float(ref[0, 17, r, col])) < 1.5
    bad[0, 17, r, col] = 0.0
    assert rel_l1(bad.cpu().numpy(), ref.cpu().numpy()) < 2e-5, "the whole-tensor metric does not see a 100 % wrong element"
    rejects(bad, ref, cond, R.TAU_WINO, "one interior element zeroed")
    assert not math.isnan(float(bad.sum()))
