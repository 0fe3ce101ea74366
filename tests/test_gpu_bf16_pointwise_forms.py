"""The two kernel forms of gsd_bf16_bn_apply and gsd_bf16_bn_bwd_apply at the smallest shapes that reach each, and the pooling
backward reduce with C / 8 dividing 256.

groups = C / 8.  The multi-pixel form is taken when groups divides 256 and N*H*W*groups >= 65536; one of its blocks covers
(256 / groups) * 4 pixels.  Every tensor is a channel slice of a wider buffer (pitch > C) filled with a sentinel bit pattern, with
one more pixel row allocated behind it: the channels outside the slice and that row must keep the sentinel.  Outputs are held to
fp64 with the helpers and constants of fp64_ref.py."""
import ctypes as C

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fa5          # a bf16 NaN that no kernel produces
#         C, (N, H, W), form reached, pieces of the second run of bn_apply: (first pixel, (N, H, W)), each under the threshold
CASES = {
    "a": (64, (1, 1, 8191), "one-pixel", None),                                              # total 65528, just under
    "b": (64, (1, 1, 8193), "multi", [(0, (1, 1, 4096)), (4096, (1, 1, 4097))]),             # last block holds one live pixel
    "c": (64, (1, 91, 91), "multi", [(0, (1, 45, 91)), (45 * 91, (1, 46, 91))]),             # ragged tail, 89 of 128
    "d": (128, (1, 1, 4097), "multi", [(0, (1, 1, 2048)), (2048, (1, 1, 2049))]),            # groups 16, tail of one
    "e": (40, (1, 1, 13108), "one-pixel", None),                                             # total >= 65536 but 5 does not divide 256
    "f": (64, (2, 64, 64), "multi", [(0, (1, 64, 64)), (4096, (1, 32, 64)), (6144, (1, 32, 64))]),   # exact threshold, no tail
}


def _lib():
    from gelslim_depth_amd import _lib as L
    return L


def _form(c, shape):
    groups, npix = c // 8, shape[0] * shape[1] * shape[2]
    return "multi" if 256 % groups == 0 and npix * groups >= 65536 else "one-pixel"


@pytest.mark.parametrize("case", sorted(CASES))
def test_cases_reach_the_form_they_name(case):
    c, shape, form, pieces = CASES[case]
    assert _form(c, shape) == form
    for _, pshape in pieces or []:
        assert _form(c, pshape) == "one-pixel"
    if pieces:
        assert sum(s[0] * s[1] * s[2] for _, s in pieces) == shape[0] * shape[1] * shape[2]


class Buf:
    """npix + 1 pixel rows of `pitch` bf16 channels, all sentinel; the tensor is channels [off, off + c) of the first npix rows."""

    def __init__(self, shape, pitch, off, c, values=None):
        self.shape, self.pitch, self.off, self.c = shape, pitch, off, c
        self.npix = shape[0] * shape[1] * shape[2]
        self.flat = torch.full((self.npix + 1, pitch), SENTINEL, dtype=torch.int16).view(torch.bfloat16)
        if values is not None:      # (n, c, h, w) float, bf16-representable
            self.flat[:self.npix, off:off + c] = values.permute(0, 2, 3, 1).reshape(self.npix, c).to(torch.bfloat16)
        self.flat = self.flat.cuda()

    def view(self, first=0, shape=None):
        n, h, w = shape or self.shape
        t = self.flat[first:first + n * h * w].view(n, h, w, self.pitch)
        return _lib().make_nhwc(t, self.off, self.c)

    def nchw(self):
        return R.nchw(self.flat[:self.npix].view(*self.shape, self.pitch), self.off, self.c)

    def assert_rest_untouched(self, what):
        bits = self.flat.view(torch.int16)
        assert bool((bits[:, :self.off] == SENTINEL).all()) and bool((bits[:, self.off + self.c:] == SENTINEL).all()), \
            f"{what}: channels outside the slice were written"
        assert bool((bits[self.npix] == SENTINEL).all()), f"{what}: the pixel row behind the tensor was written"


_INPUTS = {}


def _inputs(case):
    """y (bf16-representable), dz and the per-channel coefficients of a case: made once, shared by its tests, left unchanged."""
    if case not in _INPUTS:
        c, (n, h, w), _, _ = CASES[case]
        g = torch.Generator().manual_seed(900 + ord(case))
        y = R.bf16(torch.randn((n, c, h, w), generator=g)).float()
        dz = R.bf16(torch.randn((n, c, h, w), generator=g)).float()
        coef = {"scale": torch.rand((c,), generator=g) + 0.5, "shift": torch.randn((c,), generator=g),
                "mean": 0.3 * torch.randn((c,), generator=g), "invstd": torch.rand((c,), generator=g) * 1.5 + 0.5,
                "c1": 0.1 * torch.randn((c,), generator=g), "c2": 0.1 * torch.randn((c,), generator=g)}
        _INPUTS[case] = (y, dz, {k: v.cuda() for k, v in coef.items()})
    return _INPUTS[case]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_bn_apply_forms_bf16(case, relu):
    L = _lib()
    c, shape, _, pieces = CASES[case]
    y, _, k = _inputs(case)
    ybuf = Buf(shape, c + 16, 8, c, y)
    y_bits = ybuf.flat.view(torch.int16).clone()

    def run(parts):
        out = Buf(shape, c + 24, 0, c)
        for first, pshape in parts:
            yv, av = ybuf.view(first, pshape), out.view(first, pshape)
            L.check(L.lib.gsd_bf16_bn_apply(C.byref(yv), k["scale"].data_ptr(), k["shift"].data_ptr(), C.byref(av), relu,
                                            L.stream_ptr()), "bn_apply")
        torch.cuda.synchronize()
        return out

    out = run([(0, shape)])
    out.assert_rest_untouched(f"bn_apply {case}")
    assert torch.equal(ybuf.flat.view(torch.int16), y_bits)
    yd = ybuf.nchw()
    _, ref, cond = R.bn_relu_bf16(yd, k["scale"], k["shift"])
    if not relu:    # y*scale + shift = relu(t) - relu(-t), and the magnitudes of the two halves add up to |y*scale| + |shift| everywhere
        _, nref, ncond = R.bn_relu_bf16(-yd, k["scale"], -k["shift"])
        ref, cond = ref - nref, cond + ncond
    worst = R.check_bound_bf16(out.nchw(), ref, cond, R.TAU_BF16_PW, f"bn_apply case {case} relu {relu}")
    print(f"bn_apply case {case} relu {relu}: worst ratio {worst:.3e} (tau {R.TAU_BF16_PW:.1e})")
    if pieces:      # fmaf then fmaxf in both forms: the multi-pixel form against one-pixel launches over the same pixels, bit for bit
        again = run(pieces)
        assert torch.equal(out.flat.view(torch.int16), again.flat.view(torch.int16)), f"bn_apply {case}: the forms differ"


@pytest.mark.parametrize("case", sorted(CASES))
def test_bn_bwd_apply_forms_bf16(case):
    L = _lib()
    c, shape, _, _ = CASES[case]
    y, dz, k = _inputs(case)
    ybuf, dzbuf = Buf(shape, c + 16, 8, c, y), Buf(shape, c + 24, 0, c, dz)
    y_bits = ybuf.flat.view(torch.int16).clone()
    dz0 = dzbuf.nchw()
    dzv, yv = dzbuf.view(), ybuf.view()
    L.check(L.lib.gsd_bf16_bn_bwd_apply(C.byref(dzv), C.byref(yv), k["scale"].data_ptr(), k["mean"].data_ptr(), k["invstd"].data_ptr(),
                                        k["c1"].data_ptr(), k["c2"].data_ptr(), L.stream_ptr()), "bn_bwd_apply")
    torch.cuda.synchronize()
    dzbuf.assert_rest_untouched(f"bn_bwd_apply {case}")
    assert torch.equal(ybuf.flat.view(torch.int16), y_bits)
    ref, cond = R.bn_bwd_apply(dz0, ybuf.nchw(), k["scale"], k["mean"], k["invstd"], k["c1"], k["c2"])
    worst = R.check_bound_bf16(dzbuf.nchw(), ref, cond, R.TAU_BF16_PW, f"bn_bwd_apply case {case}")
    print(f"bn_bwd_apply case {case}: worst ratio {worst:.3e} (tau {R.TAU_BF16_PW:.1e})")


@pytest.mark.parametrize("h,w", [(13, 18), (12, 17)])
def test_bn_bwd_reduce_pool_routes_agree_when_groups_divide_256_bf16(h, w):
    """C = 64: all 256 threads of a reduce block carry pixels (test_bn_bwd_bf16 has C = 72: 28 pixel lanes and 4 idle threads).  The
    index route (gsd_bf16_bn_bwd_reduce_pool_idx) and the `a`-tensor route (gsd_bf16_bn_bwd_reduce mode 1) leave the same dz and the
    same partial rows, bit for bit, and the third column block of the rows is written as zero."""
    L = _lib()
    n, c = 2, 64
    g = torch.Generator().manual_seed(300 + h)
    y = R.bf16(torch.round(torch.randn((n, h, w, c), generator=g) * 4) / 4).to(torch.bfloat16).cuda()      # coarse: ties in windows
    k = [t.cuda() for t in (torch.rand((c,), generator=g) + 0.5, 0.3 * torch.randn((c,), generator=g),
                            0.3 * torch.randn((c,), generator=g), torch.rand((c,), generator=g) * 1.5 + 0.5)]
    gsk = R.bf16(torch.randn((n, h, w, c), generator=g)).to(torch.bfloat16).cuda()
    dpool = R.bf16(torch.randn((n, h // 2, w // 2, c), generator=g)).to(torch.bfloat16).cuda()
    a = torch.full((n, h, w, c), float("nan"), dtype=torch.bfloat16, device="cuda")
    pooled = torch.full((n, h // 2, w // 2, c), float("nan"), dtype=torch.bfloat16, device="cuda")
    idx = torch.full((n, h // 2, w // 2, c // 8), -1, dtype=torch.int16, device="cuda")
    yv = L.make_nhwc(y)
    L.check(L.lib.gsd_bf16_bn_apply_pool_idx(C.byref(yv), k[0].data_ptr(), k[1].data_ptr(), C.byref(L.make_nhwc(a)),
                                             C.byref(L.make_nhwc(pooled)), idx.data_ptr(), L.stream_ptr()), "apply_pool_idx")
    rows = L.lib.gsd_bf16_bn_bwd_partial_rows(n, h, w)
    res = []
    for use_idx in (False, True):
        dz = torch.full((n, h, w, c), float("nan"), dtype=torch.bfloat16, device="cuda")
        part = torch.full((rows, 3 * c), float("nan"), device="cuda")
        args = (C.byref(yv), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(), k[3].data_ptr(), C.byref(L.make_nhwc(gsk)))
        if use_idx:
            L.check(L.lib.gsd_bf16_bn_bwd_reduce_pool_idx(*args, idx.data_ptr(), C.byref(L.make_nhwc(dpool)), C.byref(L.make_nhwc(dz)),
                                                          part.data_ptr(), L.stream_ptr()), "reduce_pool_idx")
        else:
            L.check(L.lib.gsd_bf16_bn_bwd_reduce(1, *args, C.byref(L.make_nhwc(a)), C.byref(L.make_nhwc(dpool)), None, None,
                                                 C.byref(L.make_nhwc(dz)), part.data_ptr(), L.stream_ptr()), "reduce_pool")
        torch.cuda.synchronize()
        res.append((dz, part))
    assert not bool(torch.isnan(res[0][0].float()).any())
    assert torch.equal(res[0][0].view(torch.int16), res[1][0].view(torch.int16))
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
    assert bool((res[0][1][:, 2 * c:].view(torch.int32) == 0).all())
    assert bool((res[0][1][:, :c].abs().sum(dim=0) > 0).all())
