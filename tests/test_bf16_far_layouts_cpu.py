"""The arithmetic of tests/bf16_far_layouts.py, proved without a GPU and without the library: which pixel of which buffer crosses
which line, that the buffers of a launch are disjoint, that every true and every slipped (32-bit) address lies inside the arena and
every slipped one in fill, and which side of each host size condition every case of the tables is on -- restated in plain Python
from the host lines named below, so that a moved threshold fails here instead of silently changing what the GPU module
(tests/test_gpu_bf16_far_pitch_fp64.py) covers.

    gsd_bf16_common.h  gsd_check_nhwc       H*W*pitch < 2^31 - 1 elements, else refused
    gsd_bf16_conv.hip  conv3x3_impl         P.buf: H*W*pitch*2 < 2^31 bytes (and the weight image), else 64-bit fills
    gsd_bf16_c64.hip   c64_common           H*W*pitch < 2^30 elements, else refused
    gsd_bf16_wgrad.hip gsd_bf16_wgrad       large tile: N*H*W*pitch < 2^31 - 1 for a and b; general kernel: H*W*pitch < 2^30 each
    gsd_bf16_ctgemm.hip gsd_ctgemm_operands (N*H*W + 512) * pitch < 2^31 - 1 for in, out, bw.y
    gsd_bf16_bn.hip    multi_ppb            C/8 divides 256 and N*H*W * C/8 >= 65536: the multi-pixel apply kernels
    gsd_bf16_pointwise.h pick_pixb          ceil(N*H*W / blocks) rounded up to 32, at least 32
"""
import pytest

import bf16_far_layouts as FL
import bf16_tile_cases as B

TABLES = FL._tables()
I31 = (1 << 31) - 1
FEW, MANY = FL.LAYOUTS["few"].pitch, FL.LAYOUTS["many"].pitch


def every_case():
    """(family, layout, id, buffer list) of every launched case."""
    out = []
    for fam, ops, ident in (("conv3", FL.conv3_buffers, B.conv3_id), ("dense", FL.dense_buffers, B.dense_id), ("wgrad", FL.wgrad_buffers, B.wg_id)):
        for lay, cases in TABLES[fam].items():
            out += [(fam, lay, ident(c), ops(c)) for c, _ in cases]
    for lay, shapes in TABLES["c64"].items():
        out += [("c64", lay, str(s), FL.c64_buffers(*s)) for s in shapes]
    for lay, shapes in TABLES["first"].items():
        out += [("first", lay, str(s), FL.first_buffers(*s)) for s in shapes]
    for lay, shapes in TABLES["pw"].items():
        out += [("pw", lay, str(s), FL.pw_buffers(*s[:4])) for s in shapes]
    return out


CASES = every_case()
IDS = [f"{f}-{lay}-{i}" for f, lay, i, _ in CASES]


def test_the_arena_is_15_77_gib_and_holds_every_view():
    assert FL.ARENA_ELEMS * 2 == 16_928_307_328 and FL.ARENA_ELEMS * 2 <= 16 << 30
    for L in FL.LAYOUTS.values():
        assert L.pitch % 8 == 0 and L.pitch % 64 == 0 and (L.pitch - 64) & (L.pitch - 65) == 0     # 2^k + 64
        assert FL.FRONT + L.max_pixels * L.pitch + FL.BAND <= FL.ARENA_ELEMS
    assert FL.FRONT == 1 << 31 and FL.FILL32 < 1 << 31 and FL.FILL16 & 0x7F80 == 0x7F80 and FL.FILL16 & 0x40 == 0     # a signalling NaN


def test_which_pixel_crosses_which_line():
    """few, 5 images of 7 x 16: image 1 holds the first pixel past 2^30 elements, image 2 past 2^31, image 4 past 2^32.
    many, 3 images of 22 x 63: image 1 holds the first pixel past 2^30, image 2 past 2^31; 4095 pixels stay below 2^31."""
    pl = FL.dry("few", [(5, 7, 16, 64)])
    assert pl.lines_crossed() == {"2^30 el": (0, 1, 128), "2^31 el": (0, 2, 256), "2^32 el": (0, 4, 512)}
    for name, (_, _, p) in pl.lines_crossed().items():
        assert (p - 1) * FEW < FL.LINES[name] <= p * FEW
    assert 111 * FEW + 64 < 1 << 30 and 112 * FEW < 1 << 30 < 224 * FEW            # image 0 wholly below, image 1 straddles
    assert 224 * FEW < 1 << 31 < 336 * FEW and 448 * FEW < 1 << 32 < 560 * FEW      # images 2 and 4 straddle
    pl = FL.dry("many", [(3, 22, 63, 64)])
    assert pl.lines_crossed() == {"2^30 el": (0, 1, 2048), "2^31 el": (0, 2, 4096)}
    assert 4095 * MANY < I31 < 4096 * MANY
    pl = FL.dry("big", [(3, 10, 15, 64)])
    assert pl.lines_crossed() == {"2^30 el": (0, 0, 128), "2^31 el": (0, 1, 256)}      # inside image 0: offsets within an image pass 2^30
    assert 1 << 30 <= pl.largest_image() < I31


@pytest.mark.parametrize("fam,lay,ident,ops", CASES, ids=IDS)
def test_buffers_are_disjoint_and_every_alias_lands_in_fill_inside_the_arena(fam, lay, ident, ops):
    pl = FL.dry(lay, ops)
    L = pl.layout
    assert pl.disjoint()
    assert all(r.off % 8 == 0 for r in pl.recs), "16-byte aligned bases"
    assert L.image_lo <= pl.largest_image() < L.image_hi and pl.largest_image() < I31
    # every true address
    for r in pl.recs:
        last = FL.FRONT + r.off + (r.n * r.h * r.w - 1) * L.pitch + r.tot
        assert FL.FRONT < FL.FRONT + r.off and last <= FL.ARENA_ELEMS
        assert pl.classify(FL.FRONT + r.off, FL.FRONT + r.off + r.tot) == "data"
    # every slipped address: inside the arena, and in fill -- a read there is a NaN in a result, a write a changed word
    rep = pl.alias_report()
    assert not [x for x in rep if x[4] != "fill"], [x for x in rep if x[4] != "fill"][:4]
    crossed = pl.lines_crossed()
    assert ("2^31 el" in crossed) == any(kind == "byte offset mod 2^32" for _, _, kind, _, _ in rep)
    if lay != "big" and fam != "dense" and (lay, max(n * h * w for n, h, w, _ in ops)) != ("many", 4095):
        assert "2^31 el" in crossed, "the case's pixels do not reach 4 GiB"
    assert "2^30 el" in crossed and rep, "no address of the case can slip"
    if lay == "few" and ops[0][0] == 5:
        assert "2^32 el" in crossed


def test_every_alias_of_a_displaced_pixel_keeps_clear_of_the_band():
    """Why the aliases land in fill: a pixel p slipped by k * 2^31 elements is pixel p - k * 2^31 / (pitch - 64) displaced by
    64 * that many channels -- 16384 (few) or 262144 (many), past BAND and below the pitch."""
    for L, per in ((FL.LAYOUTS["few"], 256), (FL.LAYOUTS["many"], 4096)):
        assert per * (L.pitch - 64) == 1 << 31
        for k in (1, 2):
            if k * per < L.max_pixels:
                p = L.max_pixels - 1
                assert (p * L.pitch) - k * (1 << 31) == (p - k * per) * L.pitch + 64 * k * per
                assert FL.BAND <= 64 * k * per and 64 * k * per + FL.BAND < L.pitch
        assert -(1 << 31) <= FL._sext32(L.max_pixels * L.pitch) and L.max_pixels * L.pitch < 3 << 31


# ---------------------------------------------------------------------------------------------------- sides of the host conditions
def img(lay, h, w):
    return h * w * FL.LAYOUTS[lay].pitch


def test_conv3x3_cases_and_the_buffer_descriptor_line():
    for lay, cases in TABLES["conv3"].items():
        for c, kind in cases:
            ib = img(lay, c.h, c.w) * 2
            wb = 9 * B.round_up(c.m, 128) * c.k * 2
            assert img(lay, c.h, c.w) < I31, "gsd_check_nhwc would refuse it"
            assert kind == ("buf" if ib < 1 << 31 and wb < 1 << 31 else "fill64") == FL.far_kind(c, lay)
            assert FL.far_kind(c, None) == "buf" and c.form == B.form_of(c) and c.n >= 3
            assert (lay == "big") == (kind == "fill64")
            # conv.hip:196-197: an int element offset inside the image, doubled to bytes on the descriptor path
            assert img(lay, c.h, c.w) * (2 if kind == "buf" else 1) < 1 << 31
    eps = {(lay, c.ep) for lay, cases in TABLES["conv3"].items() for c, _ in cases}
    assert {(lay, ep) for lay in ("few", "big") for ep in ("stats", "bnbwd", "bnrelu")} <= eps
    wide = {(lay, c.form[1]) for lay, cases in TABLES["conv3"].items() for c, _ in cases}
    assert {("few", True), ("few", False), ("big", True), ("big", False)} <= wide           # both blocks of gconv_bf16_kernel<0>


def test_dense_cases_and_fits():
    """gsd_ctgemm_operands: (N*H*W + 512) * pitch < 2^31 - 1.  The gradient / concat buffer of the `many` pairs is 3528 pixels at
    offset (0, 1) and 3654 at (1, 1); two more cases put 4158 pixels (more than 2^32 bytes) behind the general kernel."""
    assert (3528 + 512) * MANY < I31 <= (3654 + 512) * MANY and (3583 + 512) * MANY < I31 <= (3584 + 512) * MANY
    seen = set()
    for lay, cases in TABLES["dense"].items():
        for c, kind in cases:
            in_, out, ty, tx = B.dense_geometry(c)
            assert max(in_.H * in_.W, out.H * out.W) * FL.LAYOUTS[lay].pitch < I31
            assert FL.far_kind(c, lay) == kind and c.form == B.form_of(c)
            assert FL.far_kind(c, None) == ("ct" if c.form[0] == "ct" else "general")
            if c.form[0] == "ct":
                big = in_ if c.kind == "ctdx" else out
                pix = big.N * big.H * big.W
                assert pix in (3528, 3654, 4158) and (kind == "ct") == ((pix + 512) * MANY < I31)
                assert pix == 4158 or pix * MANY < I31, "the pair's switch is the + 512 of fits, not N*H*W*pitch"
                assert (kind == "refused") == (bool(c.fused) and pix == 3654)
            seen.add((c.kind, bool(c.fused), kind))
    assert {("ctfwd", False, "ct"), ("ctfwd", False, "general"), ("ctdx", False, "ct"), ("ctdx", False, "general"), ("ctdx", True, "ct"),
            ("ctdx", True, "refused"), ("ctdx", True, "general"), ("1x1", False, "general"), ("1x1bnrelu", False, "general")} <= seen
    assert {c.form[2] for c, k in TABLES["dense"]["many"] if k == "ct" and c.kind == "ctdx"} == {128, 256}      # both dX instantiations


def test_wgrad_cases_and_the_large_tile_line():
    """gsd_bf16_wgrad.hip:603: large tile while N*H*W*pitch < 2^31 - 1 for a and b; b of the `many` pairs is 4095 pixels at (1, 3)
    and 4158 at (2, 1).  :639: the general kernel needs one image below 2^30 elements."""
    assert 4095 * MANY < I31 <= 4158 * MANY
    seen = set()
    for lay, cases in TABLES["wgrad"].items():
        for c, kind in cases:
            a, b, stride, ty, tx = B.wg_geometry(c)
            assert FL.far_kind(c, lay) == kind and c.form == B.form_of(c)
            assert FL.far_kind(c, None) == ("big" if c.form[0] == "wgrad_big" else "general")
            if c.form[0] == "wgrad_big":
                pix = b.N * b.H * b.W
                assert pix in (4095, 4158) and (kind == "big") == (pix * MANY < I31) and a.N * a.H * a.W * MANY < I31
            if kind == "general":
                assert img(lay, a.H, a.W) < 1 << 30 and img(lay, b.H, b.W) < 1 << 30, "the general kernel would refuse it"
            seen.add((c.taps, kind))
    assert {(9, "general"), (4, "general"), (4, "big"), (1, "general")} <= seen
    assert {c.form[1] for c, k in TABLES["wgrad"]["many"] if k == "big"} == {128, 256}


def test_c64_first_and_refused_cases_and_the_2_30_line():
    for lay in ("few", "many"):
        for n, h, w in TABLES["c64"][lay] + TABLES["first"][lay]:
            assert img(lay, h, w) < 1 << 30 and n >= 3 and n * h * w * FL.LAYOUTS[lay].pitch > 1 << 31
    for which, (n, h, w, m, ncols) in TABLES["refused"]["big"]:
        assert 1 << 30 <= img("big", h, w) < I31, "refused by the 2^30 line, not by gsd_check_nhwc"
        if which != "c64":      # the large tile does not take it (9 taps / 1 tap), so the general kernel's line decides
            assert not B.make_bigplan(9 if which == "wgrad9" else 1, n, h, w, m, ncols).ok


def test_pointwise_cases_reach_both_apply_forms_and_two_block_sizes():
    want = {("few", (5, 7, 16, 64, 0)): ("one-pixel", 32), ("few", (5, 7, 16, 2048, 0)): ("multi", 32), ("few", (5, 7, 15, 72, 0)): ("one-pixel", 32),
            ("many", (3, 22, 63, 128, 0)): ("multi", 32), ("many", (3, 22, 63, 64, 64)): ("one-pixel", 96),
            ("many", (3, 21, 65, 128, 0)): ("one-pixel", 32)}
    got = {(lay, s): (FL.pw_form(*s[:4]), FL.pick_pixb(s[0], s[1] * s[2], s[4])) for lay, shapes in TABLES["pw"].items() for s in shapes}
    assert got == want
    # the threshold of multi_ppb between two neighbouring cases: 4095 and 4158 pixels of 16 channel groups
    assert 4095 * 16 < 65536 <= 4158 * 16 and 560 * 256 >= 65536 > 560 * 8
    for lay, shapes in TABLES["pw"].items():
        for n, h, w, c, _ in shapes:
            assert img(lay, h, w) < 1 << 30 and c % 8 == 0
            assert n * h * w * FL.LAYOUTS[lay].pitch > (1 << 31 if (lay, n * h * w) != ("many", 4095) else 1 << 30)
