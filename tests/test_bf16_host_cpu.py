"""Host logic of the six bf16 MFMA convolution units (gsd_bf16_conv / _ctgemm / _wgrad / _c64 / _inc / _first .hip over
gsd_bf16_host.h), on the CPU: the queries read no device memory and every other call here is refused by validation before any
launch, so descriptors with made-up (aligned) addresses are enough.  What the engine relies on: how many BatchNorm partial rows and
how many workspace elements each launch asks for -- four of the seven queries have no restatement in tests/bf16_tile_cases.py -- and
that a call with one faulty operand comes back with the documented code, naming its entry point, instead of reaching a kernel."""
import ctypes as C

import pytest

import bf16_tile_cases as B
from gelslim_depth_amd import _lib as L

lib = L.lib
BAD_ARG, UNSUPPORTED, WORKSPACE = L.GSD_ERR_BAD_ARG, L.GSD_ERR_UNSUPPORTED, L.GSD_ERR_WORKSPACE
BASE = 0x7F0000000000
X, WT, WT1, OUT, Y, COEF, PART, DW, WSP = (BASE + (i << 36) for i in range(9))
KNOBS = ("GSD_BF16_TW", "GSD_BF16_XCD", "GSD_BF16_CONV_BUF", "GSD_BF16_CTGEMM", "GSD_BF16_CT_BM", "GSD_BF16_WGRAD_BLOCKS",
         "GSD_BF16_WGRAD_BIG")
# the (n, h, w) of the conv3x3 tile-form cases, the five U-Net levels at batch 16 and 32, a shape with fewer tiles than CUs under
# every tiling and one with more than 2048 tiles under every tiling
LEVELS = [(n, h, w) for n in (16, 32) for h, w in ((320, 427), (160, 213), (80, 106), (40, 53), (20, 26))]
SHAPES = sorted({(c.n, c.h, c.w) for c in B.CONV3_CASES}) + LEVELS + [(1, 24, 100), (8, 512, 512)]
IDS = [f"{n}x{h}x{w}" for n, h, w in SHAPES]


def queries(n, h, w):
    """(conv rows at M = 48 / 64 / 128 / 512, c64 rows, inc rows, first rows at M = 64, first-dW workspace at M = 64, dW workspace of
    4 taps at M = 512 and 256 columns, dense rows at K = 512, M = 256, 4 taps, stride 2)"""
    return (tuple(lib.gsd_bf16_conv_partial_rows(n, h, w, m) for m in (48, 64, 128, 512)),
            lib.gsd_bf16_conv3x3_c64_partial_rows(n, h, w),
            lib.gsd_bf16_inc_conv_partial_rows(n, h, w),
            lib.gsd_bf16_conv3x3_first_partial_rows(n, h, w, 64),
            lib.gsd_bf16_wgrad_first_workspace(n, h, w, 64),
            lib.gsd_bf16_wgrad_workspace(4, n, h, w, 512, 256),
            lib.gsd_bf16_conv_dense_partial_rows(n, h, w, 512, 256, 4, 2))


# queries(n, h, w) as the library of the commit before the bf16 host layer (gsd_bf16_host.h) returned them on a machine without a GPU
# (256 CUs assumed, every knob unset)
PARENT = {
    (2, 4, 70): ((16, 16, 8, 8), 4, 4, 4, 8192, 6291456, 12),
    (2, 7, 100): ((16, 16, 16, 16), 4, 4, 8, 16384, 11534336, 24),
    (2, 8, 70): ((16, 16, 12, 12), 4, 4, 8, 16384, 9437184, 20),
    (2, 11, 100): ((32, 32, 24, 24), 8, 8, 12, 24576, 16777216, 36),
    (2, 13, 27): ((8, 8, 8, 8), 4, 4, 8, 16384, 7340032, 12),
    (2, 13, 90): ((24, 24, 24, 24), 8, 8, 16, 32768, 16777216, 40),
    (2, 20, 10): ((8, 8, 8, 8), 6, 6, 10, 20480, 8388608, 8),
    (2, 20, 27): ((16, 16, 12, 12), 6, 6, 10, 20480, 8912896, 20),
    (2, 29, 40): ((24, 24, 24, 24), 8, 8, 16, 32768, 16777216, 40),
    (2, 29, 90): ((48, 48, 48, 48), 16, 16, 32, 65536, 16777216, 84),
    (2, 40, 10): ((16, 16, 12, 12), 10, 10, 20, 40960, 8388608, 12),
    (2, 58, 40): ((48, 48, 48, 48), 16, 16, 30, 61440, 16777216, 76),
    (8, 64, 128): ((512, 512, 512, 128), 128, 128, 256, 524288, 16777216, 512),
    (16, 320, 427): ((1024, 1024, 512, 128), 256, 256, 2048, 1572864, 16777216, 512),
    (16, 160, 213): ((1024, 1024, 512, 128), 256, 256, 2048, 1572864, 16777216, 512),
    (16, 80, 106): ((1024, 1024, 512, 128), 256, 256, 640, 1310720, 16777216, 512),
    (16, 40, 53): ((320, 320, 320, 128), 80, 80, 160, 327680, 16777216, 512),
    (16, 20, 26): ((128, 128, 96, 96), 48, 48, 80, 163840, 16777216, 132),
    (32, 320, 427): ((1024, 1024, 512, 128), 256, 256, 2048, 1572864, 16777216, 512),
    (32, 160, 213): ((1024, 1024, 512, 128), 256, 256, 2048, 1572864, 16777216, 512),
    (32, 80, 106): ((1024, 1024, 512, 128), 256, 256, 1280, 1572864, 16777216, 512),
    (32, 40, 53): ((640, 640, 512, 128), 160, 160, 320, 655360, 16777216, 512),
    (32, 20, 26): ((256, 256, 192, 128), 96, 96, 160, 327680, 16777216, 260),
    (1, 24, 100): ((24, 24, 24, 24), 6, 6, 12, 24576, 16777216, 40),
    (8, 512, 512): ((1024, 1024, 512, 128), 256, 256, 2048, 1572864, 16777216, 512),
}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def nhwc(n, h, w, c, *, pitch=None, ptr=OUT):
    t = L.gsd_nhwc()
    t.ptr, t.pitch, t.N, t.H, t.W, t.C = ptr, pitch or c, n, h, w, c
    return t


def bnbwd(y, *, scale=COEF, shift=COEF + 0x1000, mean=COEF + 0x2000, invstd=COEF + 0x3000):
    b = L.gsd_bf16_bnbwd()
    b.y, b.scale, b.shift, b.mean, b.invstd = C.pointer(y), scale, shift, mean, invstd
    return b


def ints(*v):
    return (C.c_int * len(v))(*v)


STENCIL = (ints(*(t // 3 - 1 for t in range(9))), ints(*(t % 3 - 1 for t in range(9))))
BLOCK2 = (ints(0, 0, 1, 1), ints(0, 1, 0, 1))     # the 2 x 2 taps of a ConvT k2s2 at offset (0, 0)
ZERO = (ints(0), ints(0))


def refused(rc, code, name):
    assert rc == code, (rc, lib.gsd_last_error().decode())
    assert name in lib.gsd_last_error().decode()


@pytest.mark.parametrize("n,h,w", SHAPES, ids=IDS)
def test_partial_rows_and_workspaces_are_the_parents(n, h, w):
    assert queries(n, h, w) == PARENT[(n, h, w)]


def test_queries_of_an_empty_shape_are_zero():
    for n, h, w in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        assert queries(n, h, w) == ((0, 0, 0, 0), 0, 0, 0, 0, 0, 0)


def test_parent_table_agrees_with_the_restatement_where_there_is_one():
    for (n, h, w), (conv, _, _, _, _, wgw, dense) in PARENT.items():
        assert conv == tuple(B.conv_partial_rows(n, h, w, m) for m in (48, 64, 128, 512))
        assert wgw == B.wgrad_workspace(4, n, h, w, 512, 256)
        assert dense == B.conv_dense_partial_rows(n, h, w, 512, 256, 4, 2)


def test_conv3x3_refusals():
    n, h, w = 2, 13, 27

    def call(k=32, m=64, in_=None, out=None, wt=WT, partials=PART, bw=None):
        in_ = in_ or nhwc(n, h, w, k, ptr=X)
        out = out or nhwc(n, h, w, m)
        return lib.gsd_bf16_conv3x3(C.byref(in_), wt, C.byref(out), k, m, partials, C.byref(bw) if bw else None, None)

    name = "gsd_bf16_conv3x3"
    refused(call(k=40), UNSUPPORTED, name)                                  # K not a multiple of 32
    refused(call(m=24), UNSUPPORTED, name)                                  # M not a multiple of 16
    refused(call(in_=nhwc(n, h, w, 64, ptr=X)), UNSUPPORTED, name)          # in->C != K
    refused(call(out=nhwc(n, h + 1, w, 64)), BAD_ARG, name)                 # extents differ
    refused(call(out=nhwc(n, h, w + 1, 64)), BAD_ARG, name)
    refused(call(out=nhwc(n + 1, h, w, 64)), BAD_ARG, name)
    refused(call(out=nhwc(n, h, w, 64, pitch=68)), UNSUPPORTED, name)       # out pitch: a multiple of 4 that the tensor check (8) refuses
    refused(call(out=nhwc(n, h, w, 64, pitch=66)), UNSUPPORTED, name)       # ... and no multiple of 4
    refused(call(wt=None), BAD_ARG, name)
    y = nhwc(n, h, w, 64, ptr=Y)
    for coef in ("scale", "shift", "mean", "invstd"):
        refused(call(bw=bnbwd(y, **{coef: None})), BAD_ARG, name)
    refused(call(bw=bnbwd(y), partials=None), BAD_ARG, name)
    refused(call(bw=bnbwd(nhwc(n, h + 1, w, 64, ptr=Y))), BAD_ARG, name)    # y of another extent
    refused(call(bw=bnbwd(nhwc(n + 1, h, w, 64, ptr=Y))), BAD_ARG, name)
    refused(call(bw=bnbwd(nhwc(n, h, w, 48, ptr=Y, pitch=64))), BAD_ARG, name)   # y->C != M


def test_conv_dense_refusals():
    n, h, w = 2, 7, 9
    name = "gsd_bf16_conv_dense"

    def call(k=64, m=256, taps=ZERO, ntaps=1, stride=1, in_=None, out=None, cs=0, oy=0, ox=0, bias=None, partials=None, bw=None):
        in_ = in_ or nhwc(n, stride * h, stride * w, k, ptr=X)
        out = out or (nhwc(n, 2 * h, 2 * w, cs) if cs else nhwc(n, h, w, m))
        return lib.gsd_bf16_conv_dense(C.byref(in_), WT, C.byref(out), k, m, ntaps, stride, taps[0], taps[1], h, w, cs, oy, ox, bias,
                                       partials, C.byref(bw) if bw else None, None)

    refused(call(ntaps=10, taps=STENCIL), BAD_ARG, name)
    refused(call(stride=3), BAD_ARG, name)
    refused(call(cs=32), BAD_ARG, name)                                     # scatter: M = 256 != 4 * 32
    refused(call(m=128, cs=32, oy=1), BAD_ARG, name)                        # the scattered block leaves the buffer
    refused(call(m=128, cs=32, ox=1), BAD_ARG, name)
    refused(call(m=128, cs=32, partials=PART), UNSUPPORTED, name)           # no statistics in scatter mode
    y = nhwc(n, h, w, 256, ptr=Y)
    dx = dict(ntaps=4, stride=2, taps=BLOCK2, partials=PART)
    refused(call(bw=bnbwd(y), bias=COEF, **dx), BAD_ARG, name)              # fused BatchNorm backward together with a bias
    refused(call(bw=bnbwd(y, mean=None), **dx), BAD_ARG, name)
    refused(call(bw=bnbwd(nhwc(n, h, w + 1, 256, ptr=Y)), **dx), BAD_ARG, name)
    refused(call(k=96, m=128), UNSUPPORTED, name)                           # K a multiple of 64 when M > 64
    assert "multiple of 64" in lib.gsd_last_error().decode()


def test_c64_refusals():
    n, h, w = 2, 8, 70
    name = "gsd_bf16_conv3x3_c64"

    def call(in_=None, out=None, wt=WT, partials=PART, bw=None):
        in_ = in_ or nhwc(n, h, w, 64, ptr=X)
        out = out or nhwc(n, h, w, 64)
        return lib.gsd_bf16_conv3x3_c64(C.byref(in_), wt, C.byref(out), partials, C.byref(bw) if bw else None, None)

    refused(call(in_=nhwc(n, h, w, 32, ptr=X)), UNSUPPORTED, name)          # 32 -> 64 channels
    refused(call(wt=WT + 8), BAD_ARG, name)
    refused(call(out=nhwc(n, h, w + 2, 64)), BAD_ARG, name)                 # extents differ
    y = nhwc(n, h, w, 64, ptr=Y)
    refused(call(bw=bnbwd(y), partials=None), BAD_ARG, name)
    refused(call(bw=bnbwd(y, invstd=None)), BAD_ARG, name)
    refused(call(bw=bnbwd(nhwc(n, h + 1, w, 64, ptr=Y))), BAD_ARG, name)


def test_inc_refusals():
    n, h, w = 2, 13, 27
    name = "gsd_bf16_inc_conv"

    def call(c=3, wt1=WT1, a0=None, y1=None):
        a0 = a0 or nhwc(n, h, w, 64)
        y1 = y1 or nhwc(n, h, w, 64, ptr=Y)
        return lib.gsd_bf16_inc_conv(X, n, c, h, w, WT, COEF, COEF + 0x1000, wt1, C.byref(a0), C.byref(y1), PART, None)

    refused(call(c=4), UNSUPPORTED, name)
    refused(call(wt1=WT1 + 8), BAD_ARG, name)
    refused(call(y1=nhwc(n, h + 1, w, 64, ptr=Y)), BAD_ARG, name)


def test_first_refusals():
    n, h, w = 2, 13, 27
    name = "gsd_bf16_conv3x3_first"

    def call(m=64, out=True, partials=PART, ep=None):
        o = nhwc(n, h, w, m)
        return lib.gsd_bf16_conv3x3_first(X, n, 3, h, w, WT, C.byref(o) if out else None, m, partials, ep, ep + 0x1000 if ep else None,
                                          None)

    refused(call(m=48), UNSUPPORTED, name)
    refused(call(ep=COEF), BAD_ARG, name)                                   # eval coefficients together with partials
    refused(call(out=False, partials=None), BAD_ARG, name)


def test_wgrad_refusals():
    n, h, w = 2, 13, 27
    name = "gsd_bf16_wgrad"

    def call(a, b, taps, ntaps, stride, elems, ncols_out=None):
        return lib.gsd_bf16_wgrad(C.byref(a), C.byref(b), ntaps, stride, taps[0], taps[1], DW, ncols_out or b.C, WSP, elems, None)

    a, b = nhwc(n, h, w, 128, ptr=X), nhwc(n, h, w, 64, ptr=Y)
    need = lib.gsd_bf16_wgrad_workspace(9, n, h, w, 128, 64)
    refused(call(a, nhwc(n + 1, h, w, 64, ptr=Y), STENCIL, 9, 1, need), BAD_ARG, name)
    refused(call(a, b, STENCIL, 9, 2, need), UNSUPPORTED, name)
    refused(call(a, b, (STENCIL[1], STENCIL[0]), 9, 1, need), UNSUPPORTED, name)        # nine taps, not the 3 x 3 stencil
    refused(call(a, b, STENCIL, 9, 1, need, ncols_out=65), BAD_ARG, name)
    # one element short of the form that runs: the small tile (3 x 3; 4 taps that the large tile does not take) ...
    assert need == B.make_wplan(True, 9, n, h, w, 128, 64).slab_elems
    refused(call(a, b, STENCIL, 9, 1, need - 1), WORKSPACE, name)
    b2 = nhwc(n, 2 * h, 2 * w, 64, ptr=Y)
    small = B.make_wplan(False, 4, n, h, w, 128, 64).slab_elems
    refused(call(a, b2, BLOCK2, 4, 1, small - 1), WORKSPACE, name)
    # ... and the large tile (4 taps at stride 2, every tap inside b): its own slab count, not the query's maximum
    big = B.make_bigplan(4, n, h, w, 128, 64)
    assert big.ok and B.wgrad_big(B.Buf(n, h, w, 128), B.Buf(n, 2 * h, 2 * w, 64), 128, 64, 4, 2, (0, 0, 1, 1), (0, 1, 0, 1))
    assert big.slab_elems != small and lib.gsd_bf16_wgrad_workspace(4, n, h, w, 128, 64) == max(big.slab_elems, small)
    refused(call(a, b2, BLOCK2, 4, 2, big.slab_elems - 1), WORKSPACE, name)


def test_wgrad_first_refusals():
    n, h, w = 2, 13, 27
    dz = nhwc(n, h, w, 64, ptr=Y)
    need = lib.gsd_bf16_wgrad_first_workspace(n, h, w, 64)

    def call(elems):
        return lib.gsd_bf16_wgrad_first(X, n, 3, h, w, C.byref(dz), None, None, None, None, None, None, DW, WSP, elems, None)

    refused(call(need - 1), WORKSPACE, "gsd_bf16_wgrad_first")
    refused(call(1), WORKSPACE, "gsd_bf16_wgrad_first")
