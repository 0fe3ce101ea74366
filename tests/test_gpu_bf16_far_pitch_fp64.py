"""The bf16 NHWC kernels held to their fp64 bounds with operands whose pixels lie megabytes apart: every address a kernel forms
from `pixel * pitch` or from an image base crosses 2^30, 2^31 or 2^32 elements (2, 4, 8 GiB) while the tensors stay a few
kilobytes (tests/bf16_far_layouts.py; tests/test_bf16_far_layouts_cpu.py proves the placements' arithmetic and which side of
every host size condition each case is on).

Launches, references and checks are those of tests/test_gpu_bf16_tile_forms_fp64.py (its conv3x3 test, run_dense, run_wgrad, over
the operands of tests/bf16_tile_ops.py) and of tests/test_gpu_bf16_fp64_bounds.py / test_gpu_bf16_pointwise_forms.py (the c64,
first-layer / inc, BatchNorm, pooling and head runners below follow them at small shapes), called twice per case: once with
compact buffers and once with every gsd_nhwc operand carved from one 15.8-GiB arena of a NaN bit pattern.  Per case:

  bound        every stored element, dW element and statistics sum within the family's TAU_BF16_* of fp64_ref.py against the same
               fp64 references; no constant widened, none added;
  exact        the small-integer pass of bf16_tile_ops equals the reference (torch.equal), far as well as compact (conv3x3, c64,
               dense / ConvT, dW); the pooled outputs, arg-max codes and the im2col tensor are exact in both;
  same bits    everything the far launch stores -- outputs, dW, statistics sums -- has the bits of the compact launch's, wherever the
               host layer runs the same kernel and block order for both (exceptions below);
  containment  after the case, with the operands' words put back, the WHOLE arena holds the fill again (a full scan per case); and
               during the case the other channels of every buffer (7.0 around each slice), the F.pad border of a scattered block, the
               rows past *_partial_rows and the floats past *_workspace keep their sentinels;
  buffers      the placement handed out exactly the buffer list the CPU proof was made for;
  refusals     where the table says a call is refused it is, with the documented code and message, and nothing is written.

Where far and compact do NOT run the same kernel (the far launch is then compared, bit for bit, with a compact launch that a knob
holds on the far launch's kernel -- which shows that the other kernel ran, since the two kernels' bits differ or their partial rows do):
  conv3x3 under `big`      gsd_bf16_conv.hip conv3x3_impl: P.buf = ib < 2^31 && wb < 2^31 -- one image of 2^30 elements or more is
                           filled through per-lane 64-bit addresses and the zero line; compact twin: GSD_BF16_CONV_BUF=0
  ConvT fwd / dX past fits gsd_bf16_ctgemm.hip gsd_ctgemm_operands: (N*H*W + 512) * pitch < 2^31 - 1 for in, out, bw.y -- the general
                           kernel stands in for the large-tile one (plain launches); compact twin: GSD_BF16_CTGEMM=0.  With fused
                           statistics the launch is refused instead (gsd_bf16_conv.hip conv_dense_impl), asserted
  dW past 2^31 elements    gsd_bf16_wgrad.hip gsd_bf16_wgrad: N*H*W*pitch < 2^31 - 1 for a and b -- the general kernel stands in for
                           the large-tile one; compact twin: GSD_BF16_WGRAD_BIG=0
Refused under `big`, before anything is launched: gsd_bf16_conv3x3_c64 ("one input image exceeds 2 GiB") and the general
gsd_bf16_wgrad ("one image of an operand exceeds 2 GiB").

Which case sits on which side of each size condition (the table of tests/test_bf16_far_layouts_cpu.py asserts it):
  gsd_check_nhwc, image < 2^31 elements       every launched case below it (few 0.94e9, many 0.73e9 / 0.96e9, big 1.26e9 .. 1.76e9);
                                              above it nothing can launch: tests/test_bf16_addressing_limits_cpu.py
  conv3x3 P.buf, image < 2^31 bytes           few, many below (buffer descriptors); big above (64-bit fills)
  conv.hip:196 int offsets inside an image    few / many: byte offsets below 2^31; big: element offsets 2^30 .. 2^31 on the 64-bit path
  c64 / general dW, image < 2^30 elements     few, many below (launched); big above (refused)
  wgrad large tile, N*H*W*pitch < 2^31        many: b of 4095 pixels below (large tile), 4158 above (general kernel)
  ctgemm fits, (N*H*W + 512) * pitch < 2^31   many: 3528 pixels below (large tile), 3654 above (general kernel / refused when fused)
  pointwise `pixel * pitch` in 64 bits        few: pixels 128.., 256.., 512.. of 560 past 2^30, 2^31, 2^32 elements; many: 4096.. of 4158

Dense by contract, and compact in both runs: the BatchNorm / statistics partials, the weight images, the pool index, the fp32
outputs (dW, db, the 1x1 output conv's planes, channel sums), every workspace, and the fp32 input x of the first-layer kernels
(no stride to place).  What no layout can place: an image of 2^31 elements or more (refused by gsd_check_nhwc; its messages are
held on the CPU), and pick_pixb's larger blocks by size alone (more than 16384 pixels: the arena ends at 8000 under `many`;
GSD_BF16_BN_BLOCKS=64 makes the blocks 96 pixels at 4158).

Measured on the MI355X (profiles/fp64_bf16_far_pitch.json): worst (|got - ref| - 2^-8 |ref| for stored bf16)+ / cond of the far
launches against the family's tau, no constant widened and none of the module's own:
    conv   1.63e-08  against TAU_BF16_CONV  = 2.1e-07   (c64 3x22x63 under many)
    first  0.00e+00  against TAU_BF16_FIRST = 6.4e-08   (27 products: every stored value within its rounding allowance)
    convT  4.27e-08  against TAU_BF16_CONVT = 1.7e-07   (gsd_bf16_convT_bias_grad, pw 5x7x16 c64 under few)
    dw     5.99e-08  against TAU_BF16_DW    = 1.1e-06   (t4-5x3x8-m128-n32 under few)
    pw     7.16e-08  against TAU_BF16_PW    = 5.6e-07   (pw 3x21x65 c128 under many)
    stats  7.00e-08  against TAU_BF16_STATS = 4.2e-06   (c64 3x5x21 under few)
Every far launch stored the bits of its compact launch (or of its knob-held twin).  The module's 54 tests take 4.7 s; the 55 full
scans of the 16.9-GB arena take 8.0 ms each (8.2 ms at most); peak device memory 17.7 GB (the arena is allocated once and freed
when the module ends).  No addressing error was found in a kernel.  Two host errors were: gsd_bf16_conv_dense with statistics but
without bw at a large-tile shape ran on the general kernel, whose row count is not the one gsd_bf16_conv_dense_partial_rows gives
(now refused; tests/test_bf16_addressing_limits_cpu.py), and UNetEngineBF16 met the fits refusal inside backward()
(UNetEngineBF16.preflight; tests/test_engine_bf16_preflight_cpu.py).

The first-layer dW (gsd_bf16_wgrad_first, _recompute) is held to fp64 from the d_raw that gsd_bf16_bn_bwd_apply stores -- the
header's contract for what both forms multiply, itself held to fp64 at TAU_BF16_PW -- because at 4158 pixels ONE d_raw that fp32
rounds to the other bf16 neighbour than fp64 does moves 27 dW elements by 2^-8 / 4158 of cond, past TAU_BF16_DW (seen: 51 of 1728
elements, worst ratio 2.2e-05, with the compact launch); tests/test_gpu_bf16_fp64_bounds.py has 2.2 million pixels under the same tau.

Mutation check (done once on a scratch copy of the library, not committed): each of these one-line slips fails far cases while
every compact case still passes --
    gsd_bf16_conv.hip dma_slot: the image base `(long long)n * P.Hin * P.Win * P.in_pitch` narrowed to int (both fill paths)
        18 far cases fail (conv3x3 under few and big, conv_dense under few and big: the images past 2^31 elements are not finite)
    gsd_bf16_conv.hip conv3x3_impl: the `ib < 2^31` term of P.buf dropped
        the 5 conv3x3 cases under big fail (the zero offset 0x80000000 lies inside such an image: pad pieces read the fill)
    gsd_bf16_ctgemm.hip gsd_ctgemm_misfit: `if (!fits(in)) return 1;` dropped
        test_dense_far[many-ctdx-2x14x31-k64-m128-o11-fused] fails (the launch runs instead of being refused)

GSD_FP64_REPORT_BF16_FAR=<path>: worst ratio per family and case, the kernel each launch ran (as the restated host conditions
say), scan times, wall time and peak memory as JSON.
"""
import ctypes as C
import json
import os
import time

import pytest
import torch

import bf16_far_layouts as FL
import bf16_tile_cases as B
import bf16_tile_ops as O
import fp64_ref as R
import test_gpu_bf16_tile_forms_fp64 as TF
from test_gpu_bf16_fp64_bounds import SENT, TAIL, bwd_sums, conv_sums, image, partials, tail_ok
from test_gpu_bf16_tile_forms_fp64 import clean_env  # noqa: F401  (autouse: a context in error ends the module; knobs cleared)

pytestmark = pytest.mark.gpu

TABLES = FL._tables()
TAU_FAMILY = {R.TAU_BF16_CONV: "conv", R.TAU_BF16_FIRST: "first", R.TAU_BF16_DW: "dw", R.TAU_BF16_CONVT: "convT",
              R.TAU_BF16_PW: "pw", R.TAU_BF16_STATS: "stats"}
RATIOS = {}         # "<family>:<layout>:<case>" -> worst ratio of the far run
KERNELS = {}        # "<layout>:<case>" -> what ran
WALL = {}


@pytest.fixture(scope="module")
def L():
    from gelslim_depth_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def arena():
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    a = FL.Arena()
    yield a
    bad = a.scan(repair=False)
    path = os.environ.get("GSD_FP64_REPORT_BF16_FAR")
    if path:
        worst = {}
        for k, v in RATIOS.items():
            fam = k.split(":")[0]
            if fam not in worst or v > worst[fam]["ratio"]:
                worst[fam] = {"ratio": v, "tau": {f: t for t, f in TAU_FAMILY.items()}[fam], "case": k.split(":", 1)[1]}
        with open(path, "w") as f:
            json.dump({"wall_s": time.time() - t0, "arena_bytes": 2 * a.elems, "scans": len(a.scan_s),
                       "scan_s_mean": sum(a.scan_s) / len(a.scan_s), "scan_s_max": max(a.scan_s),
                       "peak_memory_bytes": torch.cuda.max_memory_allocated(), "worst": dict(sorted(worst.items())),
                       "ratios": dict(sorted(RATIOS.items())), "kernels": dict(sorted(KERNELS.items())),
                       "case_wall_s": dict(sorted(WALL.items()))}, f, indent=1)
    a.free()
    assert not bad, f"elements of the arena changed and were never put back: {bad[:8]}"


# ------------------------------------------------------------------------------------------------------------ far machinery
class FarLib:
    """gelslim_depth_amd._lib with make_nhwc taking a buffer of a placement: the contiguous (N, H, W, PITCH) view of the arena that
    holds it goes to the real make_nhwc unchanged, with the buffer's channel offset."""

    def __init__(self, real, place):
        self._real, self._place = real, place

    def __getattr__(self, k):
        return getattr(self._real, k)

    def make_nhwc(self, t, c_off=0, c_len=None):
        if t.untyped_storage().data_ptr() != self._place.arena.words.untyped_storage().data_ptr():
            return self._real.make_nhwc(t, c_off, c_len)
        wide, off = self._place.wide(t)
        return self._real.make_nhwc(wide, off + c_off, t.shape[3] - c_off if c_len is None else c_len)


def far_makers(place):
    """nhwc_src / nhwc_dst / nan_bf16 of the tile-forms module over a placement: the same contents, pixels a pitch apart."""
    def src(x, tot=None, off=0, hw=None, at=(0, 0)):
        n, c, h, w = x.shape
        bh, bw = hw or (h, w)
        buf = place.view(n, bh, bw, tot or c)
        buf.fill_(TF.FILL)
        hh, ww = min(h, bh - at[0]), min(w, bw - at[1])
        buf[:, at[0]:at[0] + hh, at[1]:at[1] + ww, off:off + c] = x[:, :, :hh, :ww].permute(0, 2, 3, 1).to(torch.bfloat16)
        return buf

    def dst(n, h, w, c, tot=None, off=0, hw=None, at=(0, 0)):
        bh, bw = hw or (h, w)
        buf = place.view(n, bh, bw, tot or c)
        buf.fill_(TF.FILL)
        buf[:, at[0]:at[0] + h, at[1]:at[1] + w, off:off + c] = float("nan")
        return buf

    def nan(*shape):
        return place.view(*shape).fill_(float("nan"))
    return src, dst, nan


def recorded(monkeypatch, fn, lib, makers=None):
    """Run fn(lib) with every tensor that reaches a check recorded: [(what, bits)], the worst ratio per tau, and the partials made."""
    got, ratios, parts = [], {}, []
    with monkeypatch.context() as m:
        orig_bound, orig_stored, orig_partials = R.check_bound, TF.stored, TF.partials

        def bound(g, ref, cond, tau, what, *a, **kw):
            got.append((what, g.detach().clone()))
            worst = orig_bound(g, ref, cond, tau, what, *a, **kw)
            ratios[tau] = max(ratios.get(tau, 0.0), worst)
            return worst

        def stored(mode, g, *a, **kw):
            if mode == "exact":
                got.append((f"exact {a[3]}", g.detach().clone()))
            return orig_stored(mode, g, *a, **kw)

        def parts_(rows, width):
            p = orig_partials(rows, width)
            parts.append((p, rows * width))
            return p
        m.setattr(R, "check_bound", bound)
        m.setattr(TF, "stored", stored)
        m.setattr(TF, "partials", parts_)
        if makers is not None:
            m.setattr(TF, "nhwc_src", makers[0])
            m.setattr(TF, "nhwc_dst", makers[1])
            m.setattr(TF, "nan_bf16", makers[2])
        fn(lib)
    torch.cuda.synchronize()
    return got, ratios, parts


def same_bits(far, other, what, versus):
    assert [k for k, _ in far] == [k for k, _ in other], f"{what}: the far run checked other tensors than {versus}"
    for (k, a), (_, b) in zip(far, other):
        a, b = a.contiguous(), b.contiguous()
        bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        assert a.shape == b.shape and torch.equal(a.view(bits), b.view(bits)), \
            f"{what}: `{k}` of the far launch differs from {versus} ({int((a != b).sum())} of {a.numel()} elements)"


def far_run(L, arena, monkeypatch, lay, tag, fn, buffers, twin_env=None, far_fn=None):
    """fn(lib) compact and far: bound and exact passes in both (inside fn), buffers, containment, bits.  twin_env: the far launch runs
    another kernel than the compact one -- its bits are held to a compact run under these knobs instead."""
    t0 = time.time()
    compact, _, _ = recorded(monkeypatch, fn, L)
    if twin_env:
        with monkeypatch.context() as m:
            for k, v in twin_env:
                m.setenv(k, v)
            twin, _, _ = recorded(monkeypatch, lambda lib: fn(lib, keep_env=True), L)
    place = arena.placement(lay)
    err, far, ratios, parts = None, None, {}, []
    try:
        far, ratios, parts = recorded(monkeypatch, far_fn or fn, FarLib(L, place), far_makers(place))
    except BaseException as e:       # put the arena back whatever happened, then say both
        err = e
    got = [tuple(r[1:]) for r in place.recs]
    place.restore()
    bad = arena.scan()
    WALL[f"{lay}:{tag}"] = time.time() - t0
    where = "; ".join(f"element {i} ({i - FL.FRONT:+d} from the operands' first pixel)" for i in bad[:6])
    if err is not None:
        if bad:
            raise AssertionError(f"{tag} under {lay}: {err}; and outside the operands the arena changed at {where}") from err
        raise err
    assert not bad, f"{tag} under {lay}: the launch wrote outside its operands: {where}"
    assert got == list(buffers), f"{tag}: the launch's buffers are not the list the CPU proof is about: {got}"
    for tau, v in ratios.items():
        if tau in TAU_FAMILY:        # (tau 0: a bit-exact result recorded for the same-bits check)
            RATIOS[f"{TAU_FAMILY[tau]}:{lay}:{tag}"] = v
    if twin_env:
        same_bits(far, twin, f"{tag} under {lay}", "the compact launch under " + " ".join(f"{k}={v}" for k, v in twin_env))
    elif far_fn is None:
        same_bits(far, compact, f"{tag} under {lay}", "the compact launch")
    return far, compact, parts


# ------------------------------------------------------------------------------------------------- conv3x3 / dense / ConvT / dW
def _cases(fam):
    return [(lay, c, kind) for lay in ("few", "big", "many") for c, kind in TABLES[fam].get(lay, [])]


def _with_env(monkeypatch, c, keep_env):
    """set_env of the tile-forms module clears the knobs first; a twin run keeps the one that holds it on the far launch's kernel."""
    if keep_env:
        for k, v in c.env:
            monkeypatch.setenv(k, v)
    else:
        TF.set_env(monkeypatch, c)


CONV3 = _cases("conv3")


@pytest.mark.parametrize("lay,c,kind", CONV3, ids=[f"{lay}-{B.conv3_id(c)}" for lay, c, _ in CONV3])
def test_conv3x3_far(L, arena, monkeypatch, lay, c, kind):
    """gsd_bf16_conv3x3 (statistics; dX with the fused gsd_bf16_bnbwd) and gsd_bf16_conv3x3_bnrelu."""
    assert FL.far_kind(c, lay) == kind and FL.far_kind(c, None) == "buf"
    tag = B.conv3_id(c)

    def fn(lib, keep_env=False):
        with monkeypatch.context() as m:
            if keep_env:        # the test function below clears the knobs itself: make that a no-op for the twin
                m.setattr(TF, "set_env", lambda mp, c_: None)
            TF.test_conv3x3_bf16_tile_forms(lib, monkeypatch, c)

    far_run(L, arena, monkeypatch, lay, tag, fn, FL.conv3_buffers(c), twin_env=(("GSD_BF16_CONV_BUF", "0"),) if kind == "fill64" else None)
    KERNELS[f"{lay}:{tag}"] = f"gconv_bf16_kernel<0> {c.form[1:3]} " + ("buffer-descriptor fills" if kind == "buf" else "64-bit fills")


DENSE = _cases("dense")
MSG_FUSED = "counted the large-tile kernel's rows"


@pytest.mark.parametrize("lay,c,kind", DENSE, ids=[f"{lay}-{B.dense_id(c)}" for lay, c, _ in DENSE])
def test_dense_far(L, arena, monkeypatch, lay, c, kind):
    """gsd_bf16_conv_dense: one tap (+ gsd_bf16_conv1x1_bnrelu), the ConvT forward with scatter and bias and the ConvT dX, plain
    and with fused statistics, on the general and on the large-tile kernel, on both sides of gsd_ctgemm_operands' fits."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert FL.far_kind(c, lay) == kind and FL.far_kind(c, None) == ("ct" if c.form[0] == "ct" else "general") and B.form_of(c, cus) == c.form
    tag = B.dense_id(c)

    def fn(lib, keep_env=False, case=c):
        _with_env(monkeypatch, case, keep_env)
        for mode in O.PASSES:
            TF.run_dense(lib, case, tag, mode)

    if kind == "refused":
        far, _, parts = far_run(L, arena, monkeypatch, lay, tag, fn, FL.dense_buffers(c), far_fn=lambda lib: fn(lib, case=c._replace(want=-2)))
        assert MSG_FUSED in L.lib.gsd_last_error().decode() and not far
        for p, live in parts:
            assert bool(torch.isnan(p[:live]).all()) and bool((p[live:] == SENT).all()), f"{tag}: a refused launch wrote its partials"
        KERNELS[f"{lay}:{tag}"] = "refused: " + MSG_FUSED
        return
    twin = (("GSD_BF16_CTGEMM", "0"),) if kind == "general" and c.form[0] == "ct" else None
    far_run(L, arena, monkeypatch, lay, tag, fn, FL.dense_buffers(c), twin_env=twin)
    KERNELS[f"{lay}:{tag}"] = f"ctgemm_bf16_kernel {c.form[1:]}" if kind == "ct" else "gconv_bf16_kernel<1>" + (" (in place of the large tile)" if twin else "")


WGRAD = _cases("wgrad")


@pytest.mark.parametrize("lay,c,kind", WGRAD, ids=[f"{lay}-{B.wg_id(c)}" for lay, c, _ in WGRAD])
def test_wgrad_far(L, arena, monkeypatch, lay, c, kind):
    """gsd_bf16_wgrad: 9 taps, 4 taps at stride 2 through the large-tile and the general kernel, 1 tap; gsd_bf16_channel_sums beside
    the 4-tap cases."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert FL.far_kind(c, lay) == kind and FL.far_kind(c, None) == ("big" if c.form[0] == "wgrad_big" else "general") and B.form_of(c, cus) == c.form
    tag = B.wg_id(c)

    def fn(lib, keep_env=False):
        _with_env(monkeypatch, c, keep_env)
        for mode in O.PASSES:
            TF.run_wgrad(lib, c, mode)

    twin = (("GSD_BF16_WGRAD_BIG", "0"),) if kind == "general" and c.form[0] == "wgrad_big" else None
    far_run(L, arena, monkeypatch, lay, tag, fn, FL.wgrad_buffers(c), twin_env=twin)
    KERNELS[f"{lay}:{tag}"] = f"gwgrad_big_bf16_kernel {c.form[1]}" if kind == "big" else "gwgrad_bf16_kernel" + (" (in place of the large tile)" if twin else "")


# -------------------------------------------------------------------------------------------------------------------- c64
def run_c64(L, n, h, w):
    """gsd_bf16_conv3x3_c64, plain with statistics and as a dX launch with the fused BatchNorm backward; operands are channels
    [8, 72) of 80-channel buffers.  Both passes of bf16_tile_ops."""
    lib, st = L.lib, L.stream_ptr()
    mp = lib.gsd_bf16_conv_mpad(64)
    for ep in ("stats", "bnbwd"):
        c = B.Conv3(n, h, w, 64, 64, ep, 80, 8, 80, 8, (), None)
        cid = "c64-" + B.conv3_id(c)
        for mode in O.PASSES:
            what = f"{cid} [{mode}]"
            o = O.to(O.conv3_ops(c, mode), "cuda")
            ref, cond = O.conv3_ref(c, o)
            xin = TF.nhwc_src(o["a"], 80, 8)
            out = TF.nhwc_dst(n, h, w, 64, 80, 8)
            rows = lib.gsd_bf16_conv3x3_c64_partial_rows(n, h, w)
            part = TF.partials(rows, 2 * mp)
            bwp = None
            if ep == "bnbwd":
                img = image(L, 1, o["wt"], 64, 64)
                bw, _keep = TF.bnbwd(L, o, TF.nhwc_src(o["y"]))
                bwp = C.byref(bw)
            else:
                img = image(L, 0, o["wt"], 64, 64)
            L.check(lib.gsd_bf16_conv3x3_c64(C.byref(L.make_nhwc(xin, 8, 64)), img.data_ptr(), C.byref(L.make_nhwc(out, 8, 64)), part.data_ptr(),
                                             bwp, st), what)
            TF.untouched(out, h, w, 64, 8, (0, 0), what)
            got = R.nchw(out, 8, 64)
            TF.stored(mode, got, ref, cond, R.TAU_BF16_CONV, what, None)
            TF.stat_sums(L, mode, part, rows, 64, got, o if ep == "bnbwd" else None, what, None)


C64 = [(lay, s) for lay in ("few", "many") for s in TABLES["c64"][lay]]


@pytest.mark.parametrize("lay,shape", C64, ids=[f"{lay}-{'x'.join(map(str, s))}" for lay, s in C64])
def test_c64_far(L, arena, monkeypatch, lay, shape):
    tag = "c64-" + "x".join(map(str, shape))
    far_run(L, arena, monkeypatch, lay, tag, lambda lib: run_c64(lib, *shape), FL.c64_buffers(*shape))
    KERNELS[f"{lay}:{tag}"] = "conv64_bf16_kernel<EP_STATS, 8>, <EP_BNBWD, 8>"


# ------------------------------------------------------------------------------------------------------- first layer, inc
def run_first(L, n, h, w):
    """gsd_bf16_conv3x3_first (storing, statistics only, eval epilogue), gsd_bf16_inc_conv, gsd_bf16_first_bn_bwd_reduce,
    gsd_bf16_wgrad_first (with y) and _recompute, gsd_bf16_im2col3x3, as tests/test_gpu_bf16_fp64_bounds.py checks `inc`; x is fp32
    NCHW and compact."""
    lib, st = L.lib, L.stream_ptr()
    c, m = 3, 64
    tag = f"first-{n}x{h}x{w}"
    g = torch.Generator(device="cuda").manual_seed(2000 + n * h * w)
    x = torch.rand((n, c, h, w), generator=g, device="cuda")
    w0 = torch.randn((m, c, 3, 3), generator=g, device="cuda") * 0.3
    w1 = torch.randn((m, m, 3, 3), generator=g, device="cuda") * (2.0 / (9 * m)) ** 0.5
    img0 = image(L, 2, w0, m, c)
    mp = lib.gsd_bf16_conv_mpad(m)
    cv = (1, -1, 1, 1)
    rows0 = lib.gsd_bf16_conv3x3_first_partial_rows(n, h, w, m)
    y0 = TF.nhwc_dst(n, h, w, m)
    p_store, p_stat = partials(rows0, 2 * mp), partials(rows0, 2 * mp)
    L.check(lib.gsd_bf16_conv3x3_first(x.data_ptr(), n, c, h, w, img0.data_ptr(), C.byref(L.make_nhwc(y0)), m, p_store.data_ptr(), None, None,
                                       st), "conv3x3_first")
    L.check(lib.gsd_bf16_conv3x3_first(x.data_ptr(), n, c, h, w, img0.data_ptr(), None, m, p_stat.data_ptr(), None, None, st),
            "conv3x3_first (statistics)")
    ref, cond = R.first_fwd(x, w0)
    R.check_bound_bf16(R.nchw(y0), ref, cond, R.TAU_BF16_FIRST, f"{tag} y0")
    s = R.stored_sums(R.nchw(y0))
    for p_ in (p_store, p_stat):
        tail_ok(p_, rows0, 2 * mp, f"{tag} conv3x3_first")
        g1, g2 = conv_sums(L, p_, rows0, m)
        R.check_sums(g1, s[0], s[2], R.TAU_BF16_STATS, f"{tag} first sum")
        R.check_sums(g2, s[1], s[3], R.TAU_BF16_STATS, f"{tag} first sum of squares")
    cnt = float(n * h * w)
    mean = g1 / cnt
    invstd = 1.0 / torch.sqrt((g2 / cnt - mean * mean).clamp_min(0) + 1e-5)
    gamma = (torch.rand(m, generator=g, device="cuda") + 0.5).double()
    beta = torch.randn(m, generator=g, device="cuda").double() * 0.3
    sc, sh = (gamma * invstd).float(), (beta - mean * gamma * invstd).float()
    mean, invstd = mean.float(), invstd.float()
    # eval epilogue
    oe = TF.nhwc_dst(n, h, w, m)
    L.check(lib.gsd_bf16_conv3x3_first(x.data_ptr(), n, c, h, w, img0.data_ptr(), C.byref(L.make_nhwc(oe)), m, None, sc.data_ptr(), sh.data_ptr(),
                                       st), "conv3x3_first bnrelu")
    t = ref * sc.double().view(cv) + sh.double().view(cv)
    R.check_bound_bf16(R.nchw(oe), t.clamp_min(0.0), cond * sc.double().abs().view(cv) + sh.double().abs().view(cv), R.TAU_BF16_FIRST,
                       f"{tag} first conv+BN+ReLU")
    # inc_conv: a0 into channels [16, 80) of a 96-channel buffer, y1 and its sums
    cat = TF.nhwc_dst(n, h, w, m, 96, 16)
    y1 = TF.nhwc_dst(n, h, w, m)
    rows1 = lib.gsd_bf16_inc_conv_partial_rows(n, h, w)
    p1 = partials(rows1, 2 * mp)
    L.check(lib.gsd_bf16_inc_conv(x.data_ptr(), n, c, h, w, img0.data_ptr(), sc.data_ptr(), sh.data_ptr(), image(L, 0, w1, m, m).data_ptr(),
                                  C.byref(L.make_nhwc(cat, 16, m)), C.byref(L.make_nhwc(y1)), p1.data_ptr(), st), "inc_conv")
    TF.untouched(cat, h, w, m, 16, (0, 0), f"{tag} inc_conv a0")
    _, aref, acond = R.bn_relu_bf16(R.nchw(y0), sc, sh)
    R.check_bound_bf16(R.nchw(cat, 16, m), aref, acond, R.TAU_BF16_PW, f"{tag} a0")
    ref1, cond1 = R.conv3x3_fwd(R.nchw(cat, 16, m), R.bf16(w1))
    R.check_bound_bf16(R.nchw(y1), ref1, cond1, R.TAU_BF16_CONV, f"{tag} y1 (inc_conv)")
    tail_ok(p1, rows1, 2 * mp, f"{tag} inc_conv")
    q1, q2 = conv_sums(L, p1, rows1, m)
    s = R.stored_sums(R.nchw(y1))
    R.check_sums(q1, s[0], s[2], R.TAU_BF16_STATS, f"{tag} inc_conv sum")
    R.check_sums(q2, s[1], s[3], R.TAU_BF16_STATS, f"{tag} inc_conv sum of squares")
    # backward of the first unit: pass 1 from da with y0 recomputed, dW recomputing y0, dW from the stored y0
    da64 = R.bf16(torch.randn((n, m, h, w), generator=g, device="cuda") * 1e-3)
    da = TF.nhwc_src(da64)
    pb = partials(rows0, 2 * mp)
    L.check(lib.gsd_bf16_first_bn_bwd_reduce(x.data_ptr(), n, c, h, w, img0.data_ptr(), C.byref(L.make_nhwc(da)), sc.data_ptr(), sh.data_ptr(),
                                             mean.data_ptr(), invstd.data_ptr(), pb.data_ptr(), st), "first_bn_bwd_reduce")
    tail_ok(pb, rows0, 2 * mp, f"{tag} first_bn_bwd_reduce")
    s1, s2 = conv_sums(L, pb, rows0, m)
    dz64, _ = R.bn_bwd_dz(R.nchw(y0), sc, sh, da64)
    b = R.bn_bwd_sums(dz64, R.nchw(y0), mean, invstd)
    R.check_sums(s1, b[0], b[2], R.TAU_BF16_STATS, f"{tag} first_bn_bwd_reduce sum dz")
    R.check_sums(s2, b[1], b[3], R.TAU_BF16_STATS, f"{tag} first_bn_bwd_reduce sum dz*xhat")
    c1, c2 = (s1 / cnt).float(), (s2 / cnt).float()
    need = lib.gsd_bf16_wgrad_first_workspace(n, h, w, m)
    dws = []
    dz = TF.nhwc_src(dz64)
    # d_raw as gsd_bf16_bn_bwd_apply stores it -- the header's contract for both dW forms -- held to fp64 itself; dW is then held to
    # fp64 from that operand.  (From the fp64 d_raw rounded to bf16 instead, ONE value that the fp32 evaluation rounds the other way
    # moves 27 dW elements by 2^-8 / (N*H*W) of cond: more than TAU_BF16_DW below about 3500 pixels.)
    dr = TF.nhwc_src(dz64)
    L.check(lib.gsd_bf16_bn_bwd_apply(C.byref(L.make_nhwc(dr)), C.byref(L.make_nhwc(y0)), sc.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                      c1.data_ptr(), c2.data_ptr(), st), "bn_bwd_apply")
    dref, dabs = R.bn_bwd_apply(dz64, R.nchw(y0), sc, mean, invstd, c1, c2)
    R.check_bound_bf16(R.nchw(dr), dref, dabs, R.TAU_BF16_PW, f"{tag} d_raw (bn_bwd_apply)")
    d = R.nchw(dr)
    rw, cw = R.conv3x3_dw(R.bf16(x), d, torch.maximum(d.abs(), dabs))
    for how in ("recompute", "stored y"):
        ws = torch.full((need + TAIL,), float("nan"), device="cuda")
        ws[need:] = SENT
        dw = torch.full((m, c, 3, 3), float("nan"), device="cuda")
        if how == "recompute":
            rc = lib.gsd_bf16_wgrad_first_recompute(x.data_ptr(), n, c, h, w, img0.data_ptr(), C.byref(L.make_nhwc(da)), sc.data_ptr(), sh.data_ptr(),
                                                    mean.data_ptr(), invstd.data_ptr(), c1.data_ptr(), c2.data_ptr(), dw.data_ptr(), ws.data_ptr(),
                                                    need, st)
        else:
            rc = lib.gsd_bf16_wgrad_first(x.data_ptr(), n, c, h, w, C.byref(L.make_nhwc(dz)), C.byref(L.make_nhwc(y0)), sc.data_ptr(), mean.data_ptr(),
                                          invstd.data_ptr(), c1.data_ptr(), c2.data_ptr(), dw.data_ptr(), ws.data_ptr(), need, st)
        L.check(rc, f"wgrad_first ({how})")
        torch.cuda.synchronize()
        assert bool((ws[need:] == SENT).all()), f"{tag}: wgrad_first ({how}) wrote past its workspace"
        R.check_bound(dw, rw, cw, R.TAU_BF16_DW, f"{tag} dW ({how})", weights=True)
        dws.append(dw)
    assert torch.equal(dws[0], dws[1]), f"{tag}: wgrad_first_recompute and wgrad_first from the stored y0 differ"
    # the im2col tensor: exact
    col = TF.nhwc_dst(n, h, w, 32)
    L.check(lib.gsd_bf16_im2col3x3(x.data_ptr(), n, c, h, w, C.byref(L.make_nhwc(col)), st), "im2col3x3")
    torch.cuda.synchronize()
    want = R.bf16(torch.nn.functional.unfold(x, 3, padding=1).view(n, 27, h, w))
    gotc = R.nchw(col)
    assert torch.equal(gotc[:, :27], want) and bool((gotc[:, 27:] == 0).all()), f"{tag}: im2col3x3"
    R.check_bound(gotc, torch.cat([want, torch.zeros_like(gotc[:, 27:])], 1), torch.ones_like(gotc), 0.0, f"{tag} im2col (bits)", weights=True)


FIRST = [(lay, s) for lay in ("few", "many") for s in TABLES["first"][lay]]


@pytest.mark.parametrize("lay,shape", FIRST, ids=[f"{lay}-{'x'.join(map(str, s))}" for lay, s in FIRST])
def test_first_layer_and_inc_far(L, arena, monkeypatch, lay, shape):
    tag = "first-" + "x".join(map(str, shape))
    far_run(L, arena, monkeypatch, lay, tag, lambda lib: run_first(lib, *shape), FL.first_buffers(*shape))
    KERNELS[f"{lay}:{tag}"] = "first_bf16_kernel (store, statistics, eval), inc_conv, first_bn_bwd_reduce, wgrad_first (both), im2col3x3"


# --------------------------------------------------------------------------------------------- BatchNorm, pooling, the head
def run_pw(L, n, h, w, c):
    """gsd_bf16_bn_apply (relu 0 / 1), _pool_idx, _pool, gsd_bf16_maxpool2, gsd_bf16_bn_bwd_reduce modes 0, 1, 2 and _pool_idx,
    gsd_bf16_bn_bwd_apply, gsd_bf16_conv1x1_out, gsd_bf16_bn_relu_conv1x1_out and gsd_bf16_convT_bias_grad; every bf16 tensor is
    channels [8, 8 + c) of a buffer of c + 16 (pooled: [0, c) of c + 8).  C > 256 (the multi-pixel apply forms at few pixels): the
    two apply kernels only."""
    lib, st = L.lib, L.stream_ptr()
    tag = f"pw-{n}x{h}x{w}-c{c}"
    g = torch.Generator(device="cuda").manual_seed(900 + c + n * h * w)
    tot, off = c + 16, 8
    hp, wp = h // 2, w // 2
    y64 = R.bf16(torch.round(torch.randn((n, c, h, w), generator=g, device="cuda") * 4) / 4)      # coarse: ties in the pooling windows
    k = {"scale": torch.rand((c,), generator=g, device="cuda") + 0.5, "shift": torch.randn((c,), generator=g, device="cuda") * 0.3,
         "mean": 0.3 * torch.randn((c,), generator=g, device="cuda"), "invstd": torch.rand((c,), generator=g, device="cuda") * 1.5 + 0.5}
    ptr = {q: v.data_ptr() for q, v in k.items()}
    y = TF.nhwc_src(y64, tot, off)
    yv = L.make_nhwc(y, off, c)
    form = FL.pw_form(n, h, w, c)

    def apply(relu):
        a = TF.nhwc_dst(n, h, w, c, tot, off)
        L.check(lib.gsd_bf16_bn_apply(C.byref(yv), ptr["scale"], ptr["shift"], C.byref(L.make_nhwc(a, off, c)), relu, st), "bn_apply")
        TF.untouched(a, h, w, c, off, (0, 0), f"{tag} bn_apply")
        _, ref, cond = R.bn_relu_bf16(y64, k["scale"], k["shift"])
        if not relu:    # y*scale + shift = relu(t) - relu(-t); the magnitudes of the two halves add up to |y*scale| + |shift|
            _, nref, ncond = R.bn_relu_bf16(-y64, k["scale"], -k["shift"])
            ref, cond = ref - nref, cond + ncond
        R.check_bound_bf16(R.nchw(a, off, c), ref, cond, R.TAU_BF16_PW, f"{tag} bn_apply relu {relu} ({form})")
        return a

    def bwd_apply(dz, dz0, c1, c2):
        L.check(lib.gsd_bf16_bn_bwd_apply(C.byref(L.make_nhwc(dz, off, c)), C.byref(yv), ptr["scale"], ptr["mean"], ptr["invstd"], c1.data_ptr(),
                                          c2.data_ptr(), st), "bn_bwd_apply")
        TF.untouched(dz, h, w, c, off, (0, 0), f"{tag} bn_bwd_apply")
        ref, cond = R.bn_bwd_apply(dz0, y64, k["scale"], k["mean"], k["invstd"], c1, c2)
        R.check_bound_bf16(R.nchw(dz, off, c), ref, cond, R.TAU_BF16_PW, f"{tag} bn_bwd_apply ({form})")

    if c > 256:
        apply(1)
        dz64 = R.bf16(torch.randn((n, c, h, w), generator=g, device="cuda") * 1e-3)
        bwd_apply(TF.nhwc_src(dz64, tot, off), dz64, 1e-4 * torch.randn((c,), generator=g, device="cuda"),
                  1e-4 * torch.randn((c,), generator=g, device="cuda"))
        return
    apply(0)
    a1 = apply(1)
    a64 = R.nchw(a1, off, c)
    # apply + pool (+ index), apply + pool, the stand-alone pool: the same activation, pooled values and codes, exactly
    a2 = TF.nhwc_dst(n, h, w, c, tot, off)
    pooled = [TF.nhwc_dst(n, hp, wp, c, c + 8, 0) for _ in range(3)]
    idx = torch.full((n, hp, wp, c // 8), -1, dtype=torch.int16, device="cuda")
    pv = [L.make_nhwc(p_, 0, c) for p_ in pooled]
    L.check(lib.gsd_bf16_bn_apply_pool_idx(C.byref(yv), ptr["scale"], ptr["shift"], C.byref(L.make_nhwc(a2, off, c)), C.byref(pv[0]), idx.data_ptr(),
                                           st), "bn_apply_pool_idx")
    TF.untouched(a2, h, w, c, off, (0, 0), f"{tag} bn_apply_pool_idx")
    assert torch.equal(R.nchw(a2, off, c), a64), f"{tag}: bn_apply_pool_idx's activation differs from bn_apply's"
    L.check(lib.gsd_bf16_bn_apply_pool(C.byref(yv), ptr["scale"], ptr["shift"], C.byref(L.make_nhwc(a2, off, c)), C.byref(pv[1]), st), "bn_apply_pool")
    L.check(lib.gsd_bf16_maxpool2(C.byref(L.make_nhwc(a1, off, c)), C.byref(pv[2]), st), "maxpool2")
    pref, cref = R.maxpool_route(a64)
    for i, p_ in enumerate(pooled):
        TF.untouched(p_, hp, wp, c, 0, (0, 0), f"{tag} pooled {i}")
        assert torch.equal(R.nchw(p_, 0, c), pref), f"{tag}: pooled output {i}"
    codes = idx.to(torch.int32) & 0xffff
    got_code = torch.stack([(codes >> (2 * i)) & 3 for i in range(8)], dim=-1).reshape(n, hp, wp, c).permute(0, 3, 1, 2)
    assert torch.equal(got_code.long(), cref), f"{tag}: arg-max codes"
    R.check_bound(R.nchw(pooled[0], 0, c), pref, torch.ones_like(pref), 0.0, f"{tag} pooled (bits)", weights=True)
    # backward, pass 1
    g64 = R.bf16(torch.randn((n, c, h, w), generator=g, device="cuda") * 1e-3)
    dp64 = R.bf16(torch.randn((n, c, hp, wp), generator=g, device="cuda") * 1e-3)
    gsk, dpool = TF.nhwc_src(g64, tot, off), TF.nhwc_src(dp64, c + 8, 0)
    gv, dpv = L.make_nhwc(gsk, off, c), L.make_nhwc(dpool, 0, c)
    rows = lib.gsd_bf16_bn_bwd_partial_rows(n, h, w)
    assert rows == n * -(-h * w // FL.pick_pixb(n, h * w, int(os.environ.get("GSD_BF16_BN_BLOCKS", "0"))))
    routed = R.pool_grad(dp64, cref, h, w)
    dout = torch.randn((n, 1, h, w), generator=g, device="cuda") * 1e-3
    wo, bo = torch.randn((1, c), generator=g, device="cuda") / c ** 0.5, torch.randn(1, generator=g, device="cuda")
    coef = (ptr["scale"], ptr["shift"], ptr["mean"], ptr["invstd"])
    kept = {}
    for how in ("mode 0", "mode 1", "pool_idx", "mode 2"):
        dz = TF.nhwc_dst(n, h, w, c, tot, off)
        dzv = L.make_nhwc(dz, off, c)
        part = partials(rows, 3 * c)
        if how == "mode 0":
            rc = lib.gsd_bf16_bn_bwd_reduce(0, C.byref(yv), *coef, C.byref(gv), None, None, None, None, C.byref(dzv), part.data_ptr(), st)
            ref, cond = R.bn_bwd_dz(y64, k["scale"], k["shift"], g64)
        elif how == "mode 1":
            rc = lib.gsd_bf16_bn_bwd_reduce(1, C.byref(yv), *coef, C.byref(gv), C.byref(L.make_nhwc(a1, off, c)), C.byref(dpv), None, None,
                                            C.byref(dzv), part.data_ptr(), st)
            ref, cond = R.bn_bwd_dz(y64, k["scale"], k["shift"], g64 + routed, g64.abs() + routed.abs())
        elif how == "pool_idx":
            rc = lib.gsd_bf16_bn_bwd_reduce_pool_idx(C.byref(yv), *coef, C.byref(gv), idx.data_ptr(), C.byref(dpv), C.byref(dzv), part.data_ptr(), st)
        else:
            rc = lib.gsd_bf16_bn_bwd_reduce(2, C.byref(yv), *coef, C.byref(dzv), C.byref(L.make_nhwc(a1, off, c)), C.byref(dzv), dout.data_ptr(),
                                            wo.data_ptr(), C.byref(dzv), part.data_ptr(), st)
            ref, cond = R.bn_bwd_dz(y64, k["scale"], k["shift"], dout.double() * wo.double().view(1, -1, 1, 1))
        L.check(rc, f"bn_bwd_reduce {how}")
        TF.untouched(dz, h, w, c, off, (0, 0), f"{tag} dz ({how})")
        tail_ok(part, rows, 3 * c, f"{tag} bn_bwd_reduce {how}")
        got = R.nchw(dz, off, c)
        R.check_bound_bf16(got, ref, cond, R.TAU_BF16_PW, f"{tag} dz ({how})")
        s1, s2, s3 = bwd_sums(L, part, rows, c)
        b = R.bn_bwd_sums(got, y64, k["mean"], k["invstd"])
        R.check_sums(s1, b[0], b[2], R.TAU_BF16_STATS, f"{tag} sum dz ({how})")
        R.check_sums(s2, b[1], b[3], R.TAU_BF16_STATS, f"{tag} sum dz*xhat ({how})")
        if how == "mode 2":
            r_ = R.conv1x1_dw(a64, dout.double())
            R.check_bound(s3, r_[0][0], r_[1][0], R.TAU_BF16_PW, f"{tag} dW_out (third sum)", weights=True)
        kept[how] = (dz, got, part, s1, s2)
    assert torch.equal(kept["mode 1"][1], kept["pool_idx"][1]) and \
        torch.equal(kept["mode 1"][2].view(torch.int32), kept["pool_idx"][2].view(torch.int32)), f"{tag}: the two pooling routes differ"
    dz, dz0, _, s1, s2 = kept["mode 0"]
    cnt = float(n * h * w)
    bwd_apply(dz, dz0, (s1 / cnt).float(), (s2 / cnt).float())
    # the head: the 1x1 output conv from the stored activation and with BatchNorm + ReLU folded in
    stored_a, _, _ = R.bn_relu_bf16(y64, k["scale"], k["shift"])
    ref, cond = R.conv1x1_fwd(stored_a, wo.double(), bo.double())
    for how in ("bn_relu_conv1x1_out", "conv1x1_out"):
        out = torch.full((n, 1, h, w), float("nan"), device="cuda")
        if how == "conv1x1_out":
            rc = lib.gsd_bf16_conv1x1_out(C.byref(L.make_nhwc(a1, off, c)), wo.data_ptr(), bo.data_ptr(), 1, out.data_ptr(), st)
        else:
            rc = lib.gsd_bf16_bn_relu_conv1x1_out(C.byref(yv), ptr["scale"], ptr["shift"], wo.data_ptr(), bo.data_ptr(), 1, out.data_ptr(), st)
        L.check(rc, how)
        R.check_bound(out, ref, cond, R.TAU_BF16_PW, f"{tag} {how}")
    # the ConvT bias gradient from statistics rows and the strips of g outside a window
    oy, ox, hh, ww = 1, 1, 2 * ((h - 1) // 2), 2 * ((w - 1) // 2)
    prow, ld, col0 = 5, 2 * lib.gsd_bf16_conv_mpad(c + 32), 32
    pr = torch.randn((prow, ld), generator=g, device="cuda")
    need = lib.gsd_bf16_convT_bias_grad_workspace(n, h, w, oy, ox, hh, ww, c)
    ws = torch.full((need + TAIL,), float("nan"), device="cuda")
    ws[need:] = SENT
    db = torch.full((c,), float("nan"), device="cuda")
    L.check(lib.gsd_bf16_convT_bias_grad(pr.data_ptr(), prow, ld, col0, C.byref(gv), oy, ox, hh, ww, db.data_ptr(), ws.data_ptr(), need, st),
            "convT_bias_grad")
    torch.cuda.synchronize()
    assert bool((ws[need:] == SENT).all()), f"{tag}: convT_bias_grad wrote past its workspace"
    outside = g64.clone()
    outside[:, :, oy:oy + hh, ox:ox + ww] = 0
    pcol = pr[:, col0:col0 + c].double()
    R.check_bound(db, pcol.sum(0) - outside.sum((0, 2, 3)), pcol.abs().sum(0) + outside.abs().sum((0, 2, 3)), R.TAU_BF16_CONVT,
                  f"{tag} convT_bias_grad", weights=True)


PW = [(lay, s) for lay in ("few", "many") for s in TABLES["pw"][lay]]


@pytest.mark.parametrize("lay,case", PW, ids=[f"{lay}-{'x'.join(map(str, s[:3]))}-c{s[3]}" + (f"-BN_BLOCKS={s[4]}" if s[4] else "") for lay, s in PW])
def test_pointwise_far(L, arena, monkeypatch, lay, case):
    n, h, w, c, blocks = case
    tag = f"pw-{n}x{h}x{w}-c{c}" + (f"-b{blocks}" if blocks else "")
    if blocks:
        monkeypatch.setenv("GSD_BF16_BN_BLOCKS", str(blocks))
    far_run(L, arena, monkeypatch, lay, tag, lambda lib: run_pw(lib, n, h, w, c), FL.pw_buffers(n, h, w, c))
    KERNELS[f"{lay}:{tag}"] = f"bn_apply / bn_bwd_apply: {FL.pw_form(n, h, w, c)} form; reduce blocks of {FL.pick_pixb(n, h * w, blocks)} pixels"


# --------------------------------------------------------------------------------------------------------------- refusals
REFUSED = TABLES["refused"]["big"]


@pytest.mark.parametrize("which,shape", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_under_big(L, arena, which, shape):
    """One image of 2^30 elements or more: gsd_bf16_conv3x3_c64 and the general gsd_bf16_wgrad refuse before anything is launched."""
    n, h, w, m, ncols = shape
    lib, st = L.lib, L.stream_ptr()
    place = arena.placement("big")
    far = FarLib(L, place)
    a = place.view(n, h, w, m).fill_(1.0)
    b = place.view(n, h, w, ncols).fill_(float("nan"))
    out = torch.full((m * ncols * 9 + 64,), float("nan"), device="cuda")
    ws = torch.full((1 << 20,), float("nan"), device="cuda")
    if which == "c64":
        img = torch.zeros((lib.gsd_bf16_weight_image_size(0, 64, 64),), dtype=torch.bfloat16, device="cuda")
        rc = lib.gsd_bf16_conv3x3_c64(C.byref(far.make_nhwc(a)), img.data_ptr(), C.byref(far.make_nhwc(b)), out.data_ptr(), None, st)
        text = "gsd_bf16_conv3x3_c64: one input image exceeds 2 GiB"
    else:
        taps = 9 if which == "wgrad9" else 1
        ty = [t // 3 - 1 for t in range(9)] if taps == 9 else [0]
        tx = [t % 3 - 1 for t in range(9)] if taps == 9 else [0]
        b.fill_(1.0)
        rc = lib.gsd_bf16_wgrad(C.byref(far.make_nhwc(a)), C.byref(far.make_nhwc(b)), taps, 1, L.int_array(ty), L.int_array(tx), out.data_ptr(),
                                ncols, ws.data_ptr(), ws.numel(), st)
        text = "gsd_bf16_wgrad: one image of an operand exceeds 2 GiB"
    torch.cuda.synchronize()
    msg = lib.gsd_last_error().decode()
    untouched = bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all()) and (which != "c64" or bool(torch.isnan(b.float()).all()))
    place.restore()
    bad = arena.scan()
    assert rc == L.GSD_ERR_UNSUPPORTED and text in msg, (rc, msg)
    assert untouched and not bad, f"{which}: a refused launch wrote something"
    KERNELS[f"big:refused-{which}"] = "refused: " + text
