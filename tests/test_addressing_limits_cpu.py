"""Every host-side addressing limit of the fp32 entry points, crossed where nothing can launch: the library must refuse with
the documented code and message BEFORE it reaches a kernel launch.  Runs only without a GPU (a call that got past its checks would
then come back GSD_ERR_HIP, which is the failure this module is about; with a GPU it would run on pointers nobody owns).
Pointers are fake, aligned and non-null.  include/gsd.h states each limit next to its entry point; DESIGN.md lists them with the
host line and the GPU case that crosses the corresponding kernel arithmetic (tests/test_gpu_far_strides_fp64.py).
"""
import ctypes as C

import pytest
import torch

import far_layouts as FL
import tile_cases as T

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: runs only where nothing can launch")

P0 = 0x7000_0000_0000          # fake device addresses, 16-byte aligned, far from anything mapped


@pytest.fixture(scope="module")
def L():
    from gelslim_depth_amd import _lib
    return _lib


def src(L, c, h, w, ws=None, ns=None, cs=None, slack=0, k=0, scale=False, off=(0, 0)):
    s = L.gsd_src()
    ws = ws or w
    cs = cs or h * ws
    s.ptr = P0 + (k << 36)
    if scale:
        s.scale, s.shift, s.relu = P0 + (40 << 36), P0 + (41 << 36), 1
    s.C, s.H, s.W, s.off_h, s.off_w, s.w_stride, s.slack = c, h, w, off[0], off[1], ws, slack
    s.n_stride, s.c_stride = ns or c * cs, cs
    return s


def dst(L, c, h, w, ws=None, ns=None, cs=None, k=8):
    d = L.gsd_dst()
    ws = ws or w
    cs = cs or h * ws
    d.ptr = P0 + (k << 36)
    d.C, d.H, d.W, d.off_h, d.off_w, d.w_stride = c, h, w, 0, 0, ws
    d.n_stride, d.c_stride = ns or c * cs, cs
    return d


def refused(L, rc, code, text):
    msg = L.lib.gsd_last_error().decode()
    assert rc != L.GSD_ERR_HIP, f"the call reached a launch: {msg}"
    assert rc == code and text in msg, (rc, msg)


WT, PART, WS = P0 + (16 << 36), P0 + (17 << 36), P0 + (18 << 36)


def conv(L, fam, s, d, ci, co, n, h, w):
    fn = L.lib.gsd_conv3x3 if fam == "direct" else getattr(L.lib, f"gsd_conv3x3_{fam}")
    return fn(L.src_array([s]), 1, WT, ci, co, L.dst_array([d]), 1, None, n, h, w, None)


@pytest.mark.parametrize("fam", ["w43", "w2d"])
def test_conv3x3_source_plane_of_2_31_floats(L, fam):
    """conv3_check_operands: lane offsets inside a source plane are 32-bit."""
    h, w, ws = 32767, 8, 65540
    assert h * ws >= 2 ** 31
    refused(L, conv(L, fam, src(L, 8, h, w, ws), dst(L, 8, h, w), 8, 8, 1, h, w), L.GSD_ERR_UNSUPPORTED, "plane too large")


def test_w2d_destination_plane_of_2_31_floats(L):
    h, w, ws = 32767, 8, 65540
    refused(L, conv(L, "w2d", src(L, 8, h, w), dst(L, 8, h, w, ws), 8, 8, 1, h, w), L.GSD_ERR_UNSUPPORTED, "plane too large")


def test_w2d_source_plane_of_2_30_floats(L):
    """gsd_conv3x3_w2d: halo fills address a plane by an unsigned 32-bit BYTE offset from 16 bytes in front of it."""
    h, w, ws = 16384, 8, 65536
    assert h * ws + 4 >= 2 ** 30 and h * ws < 2 ** 31
    refused(L, conv(L, "w2d", src(L, 8, h, w, ws), dst(L, 8, h, w), 8, 8, 1, h, w), L.GSD_ERR_UNSUPPORTED,
            "a source plane must stay below 2^30 floats")


@pytest.mark.parametrize("which", ["src", "dst"])
@pytest.mark.parametrize("ns", [FL.LAYOUTS["n33"].n_stride, FL.LAYOUTS["c29"].n_stride, -(-2 ** 31 // 3)], ids=["n33", "c29", "2^31/3"])
def test_w43_folded_plan_with_a_batch_offset_past_32_bits(L, which, ns):
    """Folded tile rows carry n * n_stride in 32-bit lane offsets: N * n_stride >= 2^31 is refused, and stays refused -- running the
    unfolded plan instead would need other partial rows than the shape-only gsd_conv3x3_w43_partial_rows told the caller."""
    n, h, w, c = 3, 18, 20, 8
    assert T.plan_w43(n, h, w, 64).fold == 1 and n * ns >= 2 ** 31
    s = src(L, c, h, w, ns=ns if which == "src" else None)
    d = dst(L, 64, h, w, ns=ns if which == "dst" else None)
    refused(L, conv(L, "w43", s, d, c, 64, n, h, w), L.GSD_ERR_UNSUPPORTED, "batch too large for row folding")
    assert L.lib.gsd_conv3x3_w43_partial_rows(n, h, w, 64) == T.conv_partial_rows("w43", n, h, w, 64)      # (the folded count)


def test_wgrad_forms_under_far_channel_strides(L):
    """gsd_conv3x3_wgrad_form: the 2-D form needs 32-bit byte offsets inside a block's 64 planes (dy and every segment); past that the
    row form serves the call (a fall-back, not a refusal)."""
    n, h, w, ci, co = 2, 21, 29, 64, 64
    a, dy = src(L, ci, h, w, slack=4), src(L, co, h, w, ws=32, k=1)
    form = lambda a_, dy_: L.lib.gsd_conv3x3_wgrad_form(L.src_array([a_]), 1, C.byref(dy_), ci, co, n, h, w)      # noqa: E731
    assert form(a, dy) == 2
    cs = FL.LAYOUTS["c25"].c_stride
    assert form(a, src(L, co, h, w, ws=32, cs=cs, k=1)) == 1
    assert form(src(L, ci, h, w, cs=cs, slack=4), dy) == 1
    assert form(a, src(L, co, h, w, ws=32, cs=2 ** 23 - 64, k=1)) == 2          # 64 * c_stride * 4 just below 2^31


GRID_YZ = [
    ("gsd_maxpool2 N", lambda L: L.lib.gsd_maxpool2(C.byref(src(L, 4, 8, 8)), WS, 65536, 4, 8, 8, None), "gsd_maxpool2: N, C must be <= 65535"),
    ("gsd_maxpool2 C", lambda L: L.lib.gsd_maxpool2(C.byref(src(L, 65536, 8, 8)), WS, 2, 65536, 8, 8, None), "gsd_maxpool2: N, C must be <= 65535"),
    ("gsd_maxpool2_pitched N", lambda L: L.lib.gsd_maxpool2_pitched(C.byref(src(L, 4, 8, 8)), C.byref(dst(L, 4, 4, 4)), None, 65536, None),
     "gsd_maxpool2_pitched: N, C must be <= 65535"),
    ("gsd_bnrelu_pitched N", lambda L: L.lib.gsd_bnrelu_pitched(C.byref(src(L, 4, 8, 8, scale=True)), C.byref(dst(L, 4, 8, 8)), 65536, None),
     "gsd_bnrelu_pitched: N, C must be <= 65535"),
    ("gsd_bn_bwd_reduce C", lambda L: L.lib.gsd_bn_bwd_reduce(0, WS, WS, WS, WS, WS, C.byref(src(L, 65536, 8, 8)), None, None, None, 1, WT, PART,
                                                             2, 65536, 8, 8, None), "gsd_bn_bwd_reduce: N, C must be <= 65535"),
    ("gsd_bn_bwd_apply N", lambda L: L.lib.gsd_bn_bwd_apply(WT, WS, WS, WS, WS, WS, WS, 65536, 4, 8, 8, None, 0, None),
     "gsd_bn_bwd_apply: N, C must be <= 65535"),
    ("gsd_conv1x1_out N", lambda L: L.lib.gsd_conv1x1_out(C.byref(src(L, 4, 8, 8)), WT, None, 4, 1, WS, 65536, 8, 8, None),
     "gsd_conv1x1_out: N must be <= 65535"),
    ("gsd_gather_affine B", lambda L: L.lib.gsd_gather_affine(WS, PART, 100, 65536, 3, 64, WT, WT, 1, P0, None),
     "gsd_gather_affine: B, C must be <= 65535"),
    ("gsd_ingest_images N", lambda L: L.lib.gsd_ingest_images(WS, None, 0, 65536, 3, 8, 8, 192, 64, 0, 0, P0, 4, 4, 255.0, 0.5, None),
     "gsd_ingest_images: N, C must be <= 65535 per call"),
    ("gsd_ingest_images_interp N", lambda L: L.lib.gsd_ingest_images_interp(3, WS, None, 0, 65536, 3, 8, 8, 192, 64, 0, 0, P0, 4, 4, 255.0, 0.5, None),
     "gsd_ingest_images_interp: N, C must be <= 65535 per call"),
]


@pytest.mark.parametrize("name,call,text", GRID_YZ, ids=[g[0] for g in GRID_YZ])
def test_grid_dimension_limits(L, name, call, text):
    """Kernels that put the image and the channel on grid.z / grid.y (16 bits each)."""
    refused(L, call(L), L.GSD_ERR_UNSUPPORTED, text)


def test_gather_augment_limits(L):
    aug = L.make_augment()
    call = lambda b, h, w: L.lib.gsd_gather_augment(WS, WS, PART, 100, b, 3, 1, h, w, WT, WT, 1, WT, WT, 1, C.byref(aug), P0, P0, None)      # noqa: E731
    refused(L, call(65536, 8, 8), L.GSD_ERR_UNSUPPORTED, "B, Ci + Cd must be <= 65535 and H*W < 2^30")
    refused(L, call(2, 32768, 32768), L.GSD_ERR_UNSUPPORTED, "B, Ci + Cd must be <= 65535 and H*W < 2^30")


def test_first_layer_dx_channel_limit(L):
    assert L.lib.gsd_conv3x3_dgrad_bn_supported(2, 8, 8, 3, 65536) == 0 and L.lib.gsd_conv3x3_dgrad_bn_supported(2, 8, 8, 3, 65535) == 1
    rc = L.lib.gsd_conv3x3_dgrad_bn(WS, None, None, None, None, None, None, WT, 3, 65536, P0, 2, 8, 8, None)
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, "serves Cin * 9 <= 32 and Cout <= 65535 only")


def test_conv1x1_out_wants_dense_planes(L):
    cs = FL.LAYOUTS["c29"].c_stride
    rc = L.lib.gsd_conv1x1_out(C.byref(src(L, 4, 8, 8, cs=cs)), WT, None, 4, 1, WS, 2, 8, 8, None)
    refused(L, rc, L.GSD_ERR_BAD_ARG, "src must be the full contiguous (C,H,W) tensor")


def test_convT_bias_gradient_wants_a_dense_dy_before_anything_is_launched(L):
    n, h, w, ci, co = 2, 4, 5, 8, 16
    need = L.lib.gsd_convT2x2_wgrad_workspace(n, h, w, ci, co)
    x = src(L, ci, h, w)
    dy = src(L, co, 2 * h, 2 * w, ns=FL.LAYOUTS["n31"].n_stride, k=1)
    rc = L.lib.gsd_convT2x2_wgrad(C.byref(x), C.byref(dy), ci, co, WT, PART, WS, need, n, h, w, None)
    refused(L, rc, L.GSD_ERR_UNSUPPORTED, "bias gradient needs a contiguous dy")
