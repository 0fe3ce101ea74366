"""Host logic of the fp32 ConvTranspose2d(k2,s2) entry points (gsd_convT.hip, gsd_convT_wgrad.hip over gsd_convT_host.h), on the CPU:
the queries read no device memory and every other call here is refused by validation before any launch, so descriptors with made-up
(aligned) addresses are enough.  What the engine relies on: which weight image a dX call wants, how many partial rows the fused dX
leaves, how much workspace dW asks for, and that faulty operands come back with the documented code instead of reaching a kernel."""
import ctypes as C

import pytest

import tile_cases as T
from gelslim_depth_amd import _lib as L

lib = L.lib
BAD_ARG, UNSUPPORTED, WORKSPACE = L.GSD_ERR_BAD_ARG, L.GSD_ERR_UNSUPPORTED, L.GSD_ERR_WORKSPACE
BASE = 0x7F0000000000
WT, RAW, COEF, PART, DW, WSP = (BASE + (i << 36) for i in range(1, 7))
# (n, h, w, ci, co): the small tile-form cases and the four decoder levels at batch 32
LEVELS = [(32, h, w, ci, ci // 2) for ci, h, w in ((1024, 20, 26), (512, 40, 53), (256, 80, 106), (128, 160, 213))]
SHAPES = T.CONVT_CASES + LEVELS
IDS = [f"{n}x{h}x{w}-k{ci}-m{co}" for n, h, w, ci, co in SHAPES]
# gsd_convT2x2_wgrad_workspace and gsd_weight_layout_size(3 / 6 / 7, co, ci) per shape, as the library of the commit before the
# ConvT host layer (gsd_convT_host.h) returned them on a machine without a GPU (GSD_WGRAD_BLOCKS unset)
PARENT = {
    (2, 4, 5, 8, 32): (4096, 8192, 4096, 16384),
    (3, 5, 53, 36, 40): (88960, 10240, 16384, 20480),
    (2, 7, 9, 264, 32): (69632, 40960, 36864, 49152),
    (1, 3, 2, 36, 40): (8320, 10240, 16384, 20480),
    (32, 20, 26, 1024, 512): (8421376, 2097152, 2097152, 2097152),
    (32, 40, 53, 512, 256): (8404992, 524288, 524288, 524288),
    (32, 80, 106, 256, 128): (8396800, 131072, 131072, 131072),
    (32, 160, 213, 128, 64): (8392704, 32768, 32768, 32768),
}


def src(c, h, w, *, slack=0, ptr=BASE, affine=False, n_stride=None, c_stride=None):
    s = L.gsd_src()
    s.ptr = ptr
    s.scale = COEF if affine else None
    s.shift = COEF + 0x10000 if affine else None
    s.C, s.H, s.W = c, h, w
    s.off_h = s.off_w = 0
    s.relu = 1 if affine else 0
    s.w_stride = w
    s.slack = slack
    s.c_stride = c_stride or h * w
    s.n_stride = n_stride or c * s.c_stride
    return s


def dst(c, h, w, *, pitch=None, ptr=BASE + (7 << 36)):
    d = L.gsd_dst()
    d.ptr = ptr
    d.C, d.H, d.W = c, h, w
    d.off_h = d.off_w = 0
    d.w_stride = pitch or w
    d.c_stride = h * d.w_stride
    d.n_stride = c * d.c_stride
    return d


def grad(n, h, w, co, **kw):
    """dy of a ConvT whose input is (h, w): the plain (co, 2h, 2w) gradient."""
    return src(co, 2 * h, 2 * w, **kw)


def layout(dy, n, h, w, ci, co):
    return lib.gsd_convT2x2_dgrad_layout(C.byref(dy), ci, co, n, h, w)


def rows(dy, n, h, w, ci, co):
    return lib.gsd_convT2x2_dgrad_bnrelu_partial_rows(C.byref(dy), ci, co, n, h, w)


def dgrad_as(mode, dy, d, n, h, w, ci, co, wt=WT):
    return lib.gsd_convT2x2_dgrad_as(mode, C.byref(dy), wt, ci, co, C.byref(d), n, h, w, None)


def dgrad_bnrelu(dy, d, n, h, w, ci, co, partials=PART):
    return lib.gsd_convT2x2_dgrad_bnrelu(C.byref(dy), WT, ci, co, C.byref(d), RAW, COEF, COEF, COEF, COEF, partials, n, h, w, None)


def last_error():
    return lib.gsd_last_error().decode()


@pytest.mark.parametrize("n,h,w,ci,co", SHAPES, ids=IDS)
def test_dgrad_layout_and_partial_rows(monkeypatch, n, h, w, ci, co):
    monkeypatch.delenv("GSD_CONVT_DG_DMA", raising=False)
    want_rows = 2 * -(-(n * h * (w + (w & 1))) // 128)
    for slack in (0, 1, 2, 4):
        dy = grad(n, h, w, co, slack=slack)
        admitted = w % 2 == 0 or slack >= 2
        assert layout(dy, n, h, w, ci, co) == (7 if admitted else 3), slack
        assert rows(dy, n, h, w, ci, co) == (want_rows if admitted else 0), slack
    # the batch's dy offsets must stay below 2^40 elements
    for n_stride, admitted in ((((1 << 40) - 1) // n, True), (-(-(1 << 40) // n), False)):
        dy = grad(n, h, w, co, slack=4, n_stride=n_stride)
        assert (n * n_stride < 1 << 40) == admitted
        assert layout(dy, n, h, w, ci, co) == (7 if admitted else 3), n_stride
        assert rows(dy, n, h, w, ci, co) == (want_rows if admitted else 0), n_stride
    # the tuning switch moves the layout query only
    monkeypatch.setenv("GSD_CONVT_DG_DMA", "0")
    dy = grad(n, h, w, co, slack=4)
    assert layout(dy, n, h, w, ci, co) == 3
    assert rows(dy, n, h, w, ci, co) == want_rows
    assert rows(grad(n, h, w, co), n, h, w, ci, co) == (want_rows if w % 2 == 0 else 0)
    # no operand, no sizes: the register-staged layout, no rows
    assert lib.gsd_convT2x2_dgrad_layout(None, ci, co, n, h, w) == 3 and layout(dy, 0, h, w, ci, co) == 3
    assert lib.gsd_convT2x2_dgrad_bnrelu_partial_rows(None, ci, co, n, h, w) == 0 and rows(dy, n, h, 0, ci, co) == 0


@pytest.mark.parametrize("n,h,w,ci,co", SHAPES, ids=IDS)
def test_wgrad_workspace_and_layout_sizes_are_the_parents(monkeypatch, n, h, w, ci, co):
    monkeypatch.delenv("GSD_WGRAD_BLOCKS", raising=False)
    ws, m3, m6, m7 = PARENT[(n, h, w, ci, co)]
    assert lib.gsd_convT2x2_wgrad_workspace(n, h, w, ci, co) == ws
    assert [lib.gsd_weight_layout_size(m, co, ci) for m in (3, 6, 7)] == [m3, m6, m7]
    assert lib.gsd_convT2x2_wgrad_workspace(n, h, 0, ci, co) == 0


def test_weight_layout_mode_2_is_retired():
    for co, ci in ((32, 8), (40, 36), (512, 1024)):
        assert lib.gsd_weight_layout_size(2, co, ci) == 0
        assert lib.gsd_weight_layout(2, BASE, co, ci, WT, None) == BAD_ARG
        assert "mode 6" in last_error()
    job = (L.gsd_wl_job * 1)()
    job[0].w, job[0].wt, job[0].mode, job[0].Co, job[0].Ci, job[0].reserved = BASE, WT, 2, 32, 8, 0
    assert lib.gsd_weight_layout_batch(job, 1, None) == BAD_ARG
    assert "mode 6" in last_error()


@pytest.mark.parametrize("n,h,w,ci,co", SHAPES, ids=IDS)
def test_dgrad_refusals(n, h, w, ci, co):
    good, d = grad(n, h, w, co, slack=4), dst(ci, h, w)
    for mode in (0, 2, 6, 8, -1):
        assert dgrad_as(mode, good, d, n, h, w, ci, co) == BAD_ARG
        assert "neither 3 nor 7" in last_error()
    if w % 2:          # a stated mode-7 image for arguments the LDS-DMA kernel does not admit
        assert dgrad_as(7, grad(n, h, w, co, slack=1), d, n, h, w, ci, co) == BAD_ARG
        assert "mode-7" in last_error()
        assert dgrad_bnrelu(grad(n, h, w, co, slack=1), d, n, h, w, ci, co) == UNSUPPORTED
    big = grad(n, h, w, co, slack=4, n_stride=(-(-(1 << 40) // n) + 1) & ~1)
    assert dgrad_as(7, big, d, n, h, w, ci, co) == BAD_ARG and "mode-7" in last_error()
    assert dgrad_bnrelu(big, d, n, h, w, ci, co) == UNSUPPORTED
    assert dgrad_as(7, good, d, n, h, w, ci, co, wt=WT + 8) == BAD_ARG          # (mode 3 reads its image as dwords)
    assert "16-byte aligned" in last_error()
    for mode in (7, 3):
        call = lambda s_, d_: dgrad_as(mode, s_, d_, n, h, w, ci, co)
        assert call(grad(n, h, w, co + 1, slack=4), d) == BAD_ARG                # dy: wrong extent
        assert call(src(co, 2 * h, 2 * w + 2, slack=4), d) == BAD_ARG
        assert call(grad(n, h, w, co, slack=4, affine=True), d) == BAD_ARG       # dy: not plain
        assert "plain" in last_error()
        assert call(grad(n, h, w, co, slack=4, c_stride=4 * h * w + 1), d) == UNSUPPORTED     # dy: odd strides, odd address
        assert call(grad(n, h, w, co, slack=4, n_stride=4 * h * w * co + 1), d) == UNSUPPORTED
        assert call(grad(n, h, w, co, slack=4, ptr=BASE + 4), d) == UNSUPPORTED
        assert "8-byte aligned" in last_error()
        assert call(good, dst(ci + 1, h, w)) == BAD_ARG                          # dst: wrong extent
        assert call(good, dst(ci, h + 1, w)) == BAD_ARG
        assert call(good, dst(ci, h, w, pitch=w + 2)) == UNSUPPORTED             # ... and dX writes contiguous rows
        assert lib.gsd_convT2x2_dgrad_as(mode, C.byref(good), None, ci, co, C.byref(d), n, h, w, None) == BAD_ARG
        assert dgrad_as(mode, good, d, n, h, w, 0, co) == BAD_ARG
    # the fused form: the same operand checks, and its own
    assert dgrad_bnrelu(good, d, n, h, w, ci, co, partials=None) == BAD_ARG
    assert dgrad_bnrelu(grad(n, h, w, co + 1, slack=4), d, n, h, w, ci, co) == BAD_ARG
    assert dgrad_bnrelu(grad(n, h, w, co, slack=4, affine=True), d, n, h, w, ci, co) == BAD_ARG
    assert dgrad_bnrelu(grad(n, h, w, co, slack=4, ptr=BASE + 4), d, n, h, w, ci, co) == UNSUPPORTED
    assert dgrad_bnrelu(good, dst(ci + 1, h, w), n, h, w, ci, co) == BAD_ARG


@pytest.mark.parametrize("n,h,w,ci,co", SHAPES, ids=IDS)
def test_forward_and_wgrad_refusals(n, h, w, ci, co):
    x = src(ci, h, w, affine=True)
    fwd = lambda s_, d_, wt=WT: lib.gsd_convT2x2(C.byref(s_), wt, None, ci, co, C.byref(d_), n, h, w, None)
    assert fwd(x, dst(co, 2 * h, 2 * w, pitch=2 * w + 1)) == UNSUPPORTED         # a pitched destination needs an even pitch
    assert "even row pitch" in last_error()
    assert fwd(x, dst(co + 1, 2 * h, 2 * w)) == BAD_ARG
    assert fwd(x, dst(co, 2 * h, 2 * w, ptr=BASE + 4)) == UNSUPPORTED
    assert fwd(src(ci + 1, h, w), dst(co, 2 * h, 2 * w)) == BAD_ARG
    assert fwd(x, dst(co, 2 * h, 2 * w, pitch=2 * w + 2), wt=WT + 4) == BAD_ARG
    dy = grad(n, h, w, co)
    need = lib.gsd_convT2x2_wgrad_workspace(n, h, w, ci, co)
    wgrad = lambda x_, dy_, elems=need: lib.gsd_convT2x2_wgrad(C.byref(x_), C.byref(dy_), ci, co, DW, None, WSP, elems, n, h, w, None)
    assert wgrad(x, dy, need - 1) == WORKSPACE
    assert wgrad(x, grad(n, h, w, co + 1)) == BAD_ARG
    assert wgrad(x, grad(n, h, w, co, affine=True)) == BAD_ARG
    assert wgrad(x, grad(n, h, w, co, c_stride=4 * h * w + 1)) == UNSUPPORTED
    assert wgrad(x, grad(n, h, w, co, ptr=BASE + 4)) == UNSUPPORTED
    assert "8-byte aligned" in last_error()
    assert wgrad(src(ci + 1, h, w), dy) == BAD_ARG
