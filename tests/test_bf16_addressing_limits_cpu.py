"""Every host-side addressing limit of the bf16 entry points, crossed where nothing can launch: the library must refuse with the
documented code and message BEFORE it reaches a kernel launch -- and one step below each limit the call must get past its checks,
which without a GPU shows as GSD_ERR_HIP naming the kernel it was about to launch (that is how the two sides of
gsd_ctgemm_operands' fits and of gsd_bf16_wgrad's large-tile condition are told apart here).  Runs only without a GPU: with one,
the calls below the limits would run on pointers nobody owns.  Pointers are fake, aligned and non-null.  include/gsd_bf16.h states
each limit next to its entry point; DESIGN.md lists them with the host line and the case of tests/test_gpu_bf16_far_pitch_fp64.py
that crosses the corresponding kernel arithmetic.

Not reachable, and so not here: "grid out of range" of gsd_bf16_conv.hip's launch (the grid is at most the CU count).
"""
import ctypes as C

import pytest
import torch

import bf16_far_layouts as FL
import bf16_tile_cases as B
from test_bf16_host_cpu import BLOCK2, STENCIL, ZERO, bnbwd, clean_env, ints, nhwc  # noqa: F401  (clean_env: autouse, knobs cleared)
from test_bf16_host_cpu import COEF, DW, OUT, PART, WSP, WT, WT1, X, Y

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: runs only where nothing can launch")

FEW, MANY = FL.LAYOUTS["few"].pitch, FL.LAYOUTS["many"].pitch
MSG_FUSED = "counted the large-tile kernel's rows"


@pytest.fixture(scope="module")
def L():
    from gelslim_depth_amd import _lib
    return _lib


def refused(L, rc, code, text):
    msg = L.lib.gsd_last_error().decode()
    assert rc != L.GSD_ERR_HIP, f"the call reached a launch: {msg}"
    assert rc == code and text in msg, (rc, msg)


def launched(L, rc, kernel):
    """The call got past every check: without a GPU the launch itself fails, and its message names the kernel's entry."""
    msg = L.lib.gsd_last_error().decode()
    assert rc == L.GSD_ERR_HIP and msg.startswith(kernel + ":"), (rc, msg)


# ------------------------------------------------------------------------------------------------------------ gsd_check_nhwc
def _calls(L):
    """name -> f(t): an entry point with t as one of its gsd_nhwc operands (the others small and sound, of t's extents)."""
    lib = L.lib

    def like(t, c=None, ptr=OUT):
        return nhwc(t.N, t.H, t.W, c or t.C, ptr=ptr)
    z = ZERO
    return {
        "gsd_bf16_conv3x3 in": lambda t: lib.gsd_bf16_conv3x3(C.byref(t), WT, C.byref(like(t)), t.C, t.C, PART, None, None),
        "gsd_bf16_conv3x3 out": lambda t: lib.gsd_bf16_conv3x3(C.byref(like(t, ptr=X)), WT, C.byref(t), t.C, t.C, PART, None, None),
        "gsd_bf16_conv3x3_c64": lambda t: lib.gsd_bf16_conv3x3_c64(C.byref(t), WT, C.byref(like(t)), PART, None, None),
        "gsd_bf16_conv_dense in": lambda t: lib.gsd_bf16_conv_dense(C.byref(t), WT, C.byref(like(t)), t.C, t.C, 1, 1, z[0], z[1], t.H, t.W, 0, 0, 0,
                                                                    None, None, None, None),
        "gsd_bf16_wgrad a": lambda t: lib.gsd_bf16_wgrad(C.byref(t), C.byref(like(t, ptr=Y)), 1, 1, z[0], z[1], DW, t.C, WSP, 1 << 40, None),
        "gsd_bf16_wgrad b": lambda t: lib.gsd_bf16_wgrad(C.byref(like(t, ptr=X)), C.byref(t), 1, 1, z[0], z[1], DW, t.C, WSP, 1 << 40, None),
        "gsd_bf16_bn_apply y": lambda t: lib.gsd_bf16_bn_apply(C.byref(t), COEF, COEF, C.byref(like(t)), 1, None),
        "gsd_bf16_bn_bwd_apply dz": lambda t: lib.gsd_bf16_bn_bwd_apply(C.byref(t), C.byref(like(t, ptr=Y)), COEF, COEF, COEF, COEF, COEF, None),
        "gsd_bf16_bn_bwd_reduce y": lambda t: lib.gsd_bf16_bn_bwd_reduce(0, C.byref(t), COEF, COEF, COEF, COEF, C.byref(like(t, ptr=X)), None, None, None,
                                                                        None, C.byref(like(t)), PART, None),
        "gsd_bf16_maxpool2 a": lambda t: lib.gsd_bf16_maxpool2(C.byref(t), C.byref(nhwc(t.N, t.H // 2, t.W // 2, t.C)), None),
        "gsd_bf16_channel_sums t": lambda t: lib.gsd_bf16_channel_sums(C.byref(t), 0, 0, t.H, t.W, DW, WSP, 1 << 40, None),
        "gsd_bf16_conv1x1_out a": lambda t: lib.gsd_bf16_conv1x1_out(C.byref(t), WT, None, 1, DW, None),
        "gsd_bf16_im2col3x3 col": lambda t: lib.gsd_bf16_im2col3x3(X, t.N, 3, t.H, t.W, C.byref(nhwc(t.N, t.H, t.W, 32, pitch=t.pitch, ptr=t.ptr)), None),
        "gsd_bf16_inc_conv a0": lambda t: lib.gsd_bf16_inc_conv(X, t.N, 3, t.H, t.W, WT, COEF, COEF, WT1, C.byref(t), C.byref(like(t, ptr=Y)), PART, None),
        "gsd_bf16_wgrad_first dz": lambda t: lib.gsd_bf16_wgrad_first(X, t.N, 3, t.H, t.W, C.byref(t), None, None, None, None, None, None, DW, WSP, 1 << 40,
                                                                      None),
    }


NAMES = ["gsd_bf16_conv3x3 in", "gsd_bf16_conv3x3 out", "gsd_bf16_conv3x3_c64", "gsd_bf16_conv_dense in", "gsd_bf16_wgrad a", "gsd_bf16_wgrad b",
         "gsd_bf16_bn_apply y", "gsd_bf16_bn_bwd_apply dz", "gsd_bf16_bn_bwd_reduce y", "gsd_bf16_maxpool2 a", "gsd_bf16_channel_sums t",
         "gsd_bf16_conv1x1_out a", "gsd_bf16_im2col3x3 col", "gsd_bf16_inc_conv a0", "gsd_bf16_wgrad_first dz"]


@pytest.mark.parametrize("name", NAMES)
def test_check_nhwc_limits_of_every_entry_point(L, name):
    """gsd_check_nhwc: one image of 2^31 - 1 elements or more, a pitch that is no multiple of 8, a base off 16 bytes, pitch < C."""
    call = _calls(L)[name]
    n, h, w, c = 2, 16, 16, 32
    assert 256 * FEW >= 2 ** 31 - 1 > 255 * FEW
    refused(L, call(nhwc(n, h, w, c, pitch=FEW)), L.GSD_ERR_UNSUPPORTED, "one image exceeds 2^31 elements")
    refused(L, call(nhwc(n, h, w, c, pitch=36)), L.GSD_ERR_UNSUPPORTED, "base must be 16-byte aligned and pitch a multiple of 8 elements")
    refused(L, call(nhwc(n, h, w, c, ptr=OUT + 8)), L.GSD_ERR_UNSUPPORTED, "base must be 16-byte aligned and pitch a multiple of 8 elements")
    refused(L, call(nhwc(n, h, w, c, pitch=24)), L.GSD_ERR_BAD_ARG, "pitch 24 < C")
    assert name.rsplit(" ", 1)[0].split("_first")[0] in L.lib.gsd_last_error().decode()


def test_an_image_just_below_2_31_elements_is_served_by_conv3x3_on_its_64_bit_fills(L):
    n, h, w, c = 2, 15, 17, 64
    assert 2 ** 30 <= h * w * FEW < 2 ** 31 - 1
    rc = L.lib.gsd_bf16_conv3x3(C.byref(nhwc(n, h, w, c, pitch=FEW, ptr=X)), WT, C.byref(nhwc(n, h, w, c)), c, c, PART, None, None)
    launched(L, rc, "gsd_bf16_conv3x3")
    assert B.conv_buf(h, w, FEW, c, c) == 0 and B.conv_buf(7, 16, FEW, c, c) == 1


# ------------------------------------------------------------------------------------------------------ 2^30 elements an image
def test_c64_input_image_of_2_30_elements(L):
    n, c = 2, 64
    call = lambda h, w: L.lib.gsd_bf16_conv3x3_c64(C.byref(nhwc(n, h, w, c, pitch=FEW, ptr=X)), WT, C.byref(nhwc(n, h, w, c)), PART, None, None)      # noqa: E731
    assert 127 * FEW < 2 ** 30 <= 128 * FEW
    refused(L, call(8, 16), L.GSD_ERR_UNSUPPORTED, "gsd_bf16_conv3x3_c64: one input image exceeds 2 GiB")
    launched(L, call(1, 127), "gsd_bf16_conv3x3_c64")
    # (the output is addressed in 64 bits: only gsd_check_nhwc's line holds for it)
    rc = L.lib.gsd_bf16_conv3x3_c64(C.byref(nhwc(n, 8, 16, c, ptr=X)), WT, C.byref(nhwc(n, 8, 16, c, pitch=FEW)), PART, None, None)
    launched(L, rc, "gsd_bf16_conv3x3_c64")


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("taps", [9, 1, 4])
def test_general_wgrad_image_of_2_30_elements(L, which, taps):
    n, c = 2, 64
    ty, tx = {9: STENCIL, 1: ZERO, 4: BLOCK2}[taps]

    def call(h, w):
        a = nhwc(n, h, w, c, pitch=FEW if which == "a" else None, ptr=X)
        bh, bw = (2 * h, 2 * w) if taps == 4 else (h, w)
        b = nhwc(n, bh, bw, c, pitch=FEW if which == "b" else None, ptr=Y)
        return L.lib.gsd_bf16_wgrad(C.byref(a), C.byref(b), taps, 2 if taps == 4 else 1, ty, tx, DW, c, WSP, 1 << 40, None)
    assert not B.make_bigplan(taps, n, 8, 16, c, c).ok      # M = 64: the large tile never takes it
    big, small = ((8, 16), (1, 127)) if not (taps == 4 and which == "b") else ((4, 8), (1, 31))
    refused(L, call(*big), L.GSD_ERR_UNSUPPORTED, "gsd_bf16_wgrad: one image of an operand exceeds 2 GiB")
    launched(L, call(*small), "gsd_bf16_wgrad")


def test_wgrad_extent(L):
    n, c = 2, 64
    call = lambda h, w: L.lib.gsd_bf16_wgrad(C.byref(nhwc(n, h, w, c, ptr=X)), C.byref(nhwc(n, h, w, c, ptr=Y)), 1, 1, ZERO[0], ZERO[1], DW, c, WSP,      # noqa: E731
                                             1 << 40, None)
    refused(L, call(256 * 128, 1), L.GSD_ERR_UNSUPPORTED, "gsd_bf16_wgrad: extent too large")
    refused(L, call(1, 4096), L.GSD_ERR_UNSUPPORTED, "gsd_bf16_wgrad: extent too large")
    launched(L, call(256 * 128 - 1, 1), "gsd_bf16_wgrad")
    launched(L, call(1, 4095), "gsd_bf16_wgrad")


def test_wgrad_large_tile_runs_only_below_2_31_elements(L):
    """gsd_bf16_wgrad.hip:603, on both sides, with the shapes of the far module's `many` pair: b of 3 x 21 x 65 = 4095 pixels and of
    3 x 22 x 63 = 4158."""
    n, h, w, m, ncols = 3, 10, 31, 128, 64
    assert B.make_bigplan(4, n, h, w, m, ncols).ok and 4095 * MANY < 2 ** 31 - 1 <= 4158 * MANY

    def call(oy, ox, a_pitch=None):
        a = nhwc(n, h, w, m, pitch=a_pitch, ptr=X)
        b = nhwc(n, 2 * h + oy, 2 * w + ox, ncols, pitch=MANY, ptr=Y)
        return L.lib.gsd_bf16_wgrad(C.byref(a), C.byref(b), 4, 2, ints(oy, oy, oy + 1, oy + 1), ints(ox, ox + 1, ox, ox + 1), DW, ncols, WSP, 1 << 40,
                                    None)
    launched(L, call(1, 3), "gsd_bf16_wgrad (large tile)")
    launched(L, call(2, 1), "gsd_bf16_wgrad")
    launched(L, call(1, 3, a_pitch=MANY), "gsd_bf16_wgrad (large tile)")        # a: 930 pixels
    wide = 3 * 2 ** 20 + 64             # a past the line, one image of it still below 2^30 elements
    assert n * h * w * wide >= 2 ** 31 - 1 and h * w * wide < 2 ** 30
    launched(L, call(1, 3, a_pitch=wide), "gsd_bf16_wgrad")


# ------------------------------------------------------------------------------------------------------------ gsd_bf16_conv_dense
def test_conv_dense_grid_extent(L):
    n, k, m = 1, 32, 64
    call = lambda h, w: L.lib.gsd_bf16_conv_dense(C.byref(nhwc(n, h, w, k, ptr=X)), WT, C.byref(nhwc(n, h, w, m)), k, m, 1, 1, ZERO[0], ZERO[1], h, w,      # noqa: E731
                                                  0, 0, 0, None, None, None, None)
    refused(L, call(65536, 1), L.GSD_ERR_BAD_ARG, "gsd_bf16_conv_dense: bad grid")
    refused(L, call(1, 4096), L.GSD_ERR_BAD_ARG, "gsd_bf16_conv_dense: bad grid")
    launched(L, call(65535, 1), "gsd_bf16_conv_dense")
    launched(L, call(1, 4095), "gsd_bf16_conv_dense")


def _ctdx(L, oy, ox, fused, partials=True, out_pitch=None, y_pitch=None, n=2, h=14, w=31, k=64, m=128):
    gin = nhwc(n, 2 * h + oy, 2 * w + ox, k, pitch=MANY, ptr=X)
    out = nhwc(n, h, w, m, pitch=out_pitch)
    y = nhwc(n, h, w, m, pitch=y_pitch, ptr=Y)
    ty, tx = ints(oy, oy, oy + 1, oy + 1), ints(ox, ox + 1, ox, ox + 1)
    bw = bnbwd(y) if fused else None
    rc = L.lib.gsd_bf16_conv_dense(C.byref(gin), WT, C.byref(out), k, m, 4, 2, ty, tx, h, w, 0, 0, 0, None, PART if (fused or partials) else None,
                                   C.byref(bw) if fused else None, None)
    ask = L.lib.gsd_bf16_conv_dense_fused_misfit(C.byref(gin), C.byref(out), C.byref(y) if fused else None, k, m, 4, 2, ty, tx, h, w)
    return rc, ask


def test_convT_dx_with_fused_statistics_on_both_sides_of_fits(L):
    """gsd_ctgemm_operands' fits and what conv_dense_impl does past it; gsd_bf16_conv_dense_partial_rows and the launch agree on whose
    rows are counted: the large-tile kernel's at this shape -- which is why a launch with statistics that cannot run there is refused
    and never handed to the general kernel -- and the pre-flight query gives the launch's answer without a pointer."""
    n, h, w, k, m = 2, 14, 31, 64, 128
    assert (2 * 28 * 63 + 512) * MANY < 2 ** 31 - 1 <= (2 * 29 * 63 + 512) * MANY
    rows = L.lib.gsd_bf16_conv_dense_partial_rows(n, h, w, k, m, 4, 2)
    assert rows == B.ctgemm_partial_rows(n, h, w, m) != B.conv_partial_rows(n, h, w, m)
    rc, ask = _ctdx(L, 0, 1, fused=True)
    launched(L, rc, "gsd_bf16_conv_dense (large tile)")
    assert ask == 0
    rc, ask = _ctdx(L, 1, 1, fused=True)
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, MSG_FUSED)
    assert ask == 1
    # statistics without bw: the large-tile kernel has no such form, and the general kernel would write ITS row count into a buffer
    # sized by the query -- refused on both sides of fits (it used to run on the general kernel); without statistics: served
    for oy in (0, 1):
        rc, ask = _ctdx(L, oy, 1, fused=False)
        refused(L, rc, L.GSD_ERR_UNSUPPORTED, MSG_FUSED)
        assert ask == 5
    rc, _ = _ctdx(L, 1, 1, fused=False, partials=False)
    launched(L, rc, "gsd_bf16_conv_dense")
    rc, _ = _ctdx(L, 0, 1, fused=False, partials=False)
    launched(L, rc, "gsd_bf16_conv_dense (large tile)")
    # out and bw.y: (2 * 14 * 31 + 512) pixels at a pitch that keeps one image below 2^31 elements
    wide = 3 * 2 ** 20 + 64
    assert (n * h * w + 512) * wide >= 2 ** 31 - 1 > (n * h * w + 512) * MANY and h * w * wide < 2 ** 31 - 1
    rc, ask = _ctdx(L, 0, 1, fused=True, out_pitch=wide)
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, MSG_FUSED)
    assert ask == 2
    rc, ask = _ctdx(L, 0, 1, fused=True, y_pitch=wide)
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, MSG_FUSED)
    assert ask == 3
    rc, ask = _ctdx(L, 0, 1, fused=True, out_pitch=MANY, y_pitch=MANY)
    launched(L, rc, "gsd_bf16_conv_dense (large tile)")
    assert ask == 0
    # a shape the large tile never takes (W < 16): the general kernel's rows are counted and any operand size is served
    rc, ask = _ctdx(L, 1, 1, fused=True, h=60, w=15)
    launched(L, rc, "gsd_bf16_conv_dense")
    assert ask == 0 and L.lib.gsd_bf16_conv_dense_partial_rows(n, 60, 15, k, m, 4, 2) == B.conv_partial_rows(n, 60, 15, m)


def test_convT_forward_on_both_sides_of_fits(L):
    n, h, w, k, cs = 2, 14, 31, 64, 64

    def call(oy, ox):
        out = nhwc(n, 2 * h + oy, 2 * w + ox, cs, pitch=MANY)
        return L.lib.gsd_bf16_conv_dense(C.byref(nhwc(n, h, w, k, ptr=X)), WT, C.byref(out), k, 4 * cs, 1, 1, ZERO[0], ZERO[1], h, w, cs, oy, ox, COEF,
                                         None, None, None)
    launched(L, call(0, 1), "gsd_bf16_conv_dense (large tile)")
    launched(L, call(1, 1), "gsd_bf16_conv_dense")


# ------------------------------------------------------------------------------------------------------ work items, tiles, images
def test_work_items_and_tiles_of_2_31(L):
    lib = L.lib
    n = 1 << 30
    rc = lib.gsd_bf16_conv3x3(C.byref(nhwc(n, 8, 8, 32, ptr=X)), WT, C.byref(nhwc(n, 8, 8, 256)), 32, 256, PART, None, None)      # two m-blocks
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, "gsd_bf16_conv3x3: 2147483648 work items out of range")
    rc = lib.gsd_bf16_conv_dense(C.byref(nhwc(n, 8, 8, 64, ptr=X)), WT, C.byref(nhwc(n, 8, 8, 256)), 64, 256, 1, 1, ZERO[0], ZERO[1], 8, 8, 0, 0, 0, None,
                                 None, None, None)
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, "gsd_bf16_conv_dense: 2147483648 work items out of range")
    rc = lib.gsd_bf16_conv3x3_c64(C.byref(nhwc(n, 16, 8, 64, ptr=X)), WT, C.byref(nhwc(n, 16, 8, 64)), PART, None, None)                # two tile rows
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, "gsd_bf16_conv3x3_c64: too many tiles")
    rc = lib.gsd_bf16_conv3x3_first(X, n, 3, 8, 8, WT, C.byref(nhwc(n, 8, 8, 64)), 64, PART, None, None, None)
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, "gsd_bf16_conv3x3_first: too many tiles")
    rc = lib.gsd_bf16_first_bn_bwd_reduce(X, n, 3, 8, 8, WT, C.byref(nhwc(n, 8, 8, 64)), COEF, COEF, COEF, COEF, PART, None)
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, "too many tiles")
    rc = lib.gsd_bf16_wgrad_first(X, n, 3, 8, 8, C.byref(nhwc(n, 8, 8, 64)), None, None, None, None, None, None, DW, WSP, 1 << 40, None)
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, "gsd_bf16_wgrad_first: too many tiles")
    rc = lib.gsd_bf16_inc_conv(X, n, 3, 16, 8, WT, COEF, COEF, WT1, C.byref(nhwc(n, 16, 8, 64)), C.byref(nhwc(n, 16, 8, 64, ptr=Y)), PART, None)
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, "too many tiles")
    assert lib.gsd_bf16_conv3x3_c64_partial_rows(n, 16, 8) == 256       # (the query saturates instead of wrapping)


def test_weight_images_too_large(L):
    job = (L.gsd_bf16_wimg_job * 2)()
    for j, (co, ci) in zip(job, ((64, 64), (65536, 32768))):
        j.w, j.out, j.mode, j.Cout, j.Cin = X, OUT, 0, co, ci
    assert 65536 * 32768 >= 2 ** 31 - 1
    refused(L, L.lib.gsd_bf16_weight_images(job, 2, None), L.GSD_ERR_UNSUPPORTED, "gsd_bf16_weight_images: image 1 too large")
