"""The arithmetic of tests/far_layouts.py, proved without a GPU for every layout and operand set that
tests/test_gpu_far_strides_fp64.py launches (the GPU module holds each launch to the same operand lists):

  * the operands of a launch do not overlap and lie inside the arena, FRONT = 2^31 floats behind its start;
  * the start of some plane the launch touches lies behind each of the lines 2^31 B, 2^32 B, 2^31 elements, 2^32 elements that the
    layout is there to cross;
  * every alias of every plane offset -- the byte offset modulo 2^32 or sign-extended from 32 bits, the element offset modulo 2^32
    or sign-extended -- lies inside the arena, and either in fill or on other data of the same launch at a displacement that is
    no plane start of any operand.  The strides of the layouts end in + 64 floats, so the aliases that fall behind an operand's
    own base (offsets 64, 128, 256 ... floats) cannot lie in fill once an image is larger than that: which kind each alias is
    is stated below, per layout, and at least one alias of every kind that exists for a layout lies in fill.
"""
import pytest

import far_layouts as FL
import tile_cases as T

TABLES = FL._tables()

# the lines each layout must cross (the smallest offsets a launch forms, counted from an operand's base)
MUST_CROSS = {"n31": ("2^31 B", "2^32 B"), "n33": ("2^31 B", "2^32 B", "2^31 el", "2^32 el"),
              "c29": ("2^31 B", "2^32 B", "2^31 el"), "c25": ("2^31 B", "2^32 B", "2^31 el")}


def _ws(c, fused=False):
    """K-slab scratch of a forced split: the library's own figure when it is built, else a stand-in of the same order (the proof
    does not depend on the figure, only on the band holding it)."""
    fam = c.fam
    key = f"GSD_{fam.upper()}_SPLIT"
    if key not in dict(c.env):
        return (0, 0) if not fused else 0
    n, h, w = c.n, c.h, c.w
    tiles = n * -(-h // 2) * -(-w // 4) * 4
    est = tiles * 64 * 256 // 16
    return est if fused else (est, est)


def launches():
    out = []
    for lay, cases in TABLES["conv"].items():
        out += [(f"conv-{lay}-{T.case_id(c)}", lay, FL.conv_operands(c, _ws(c))) for c in cases]
    for lay, cases in TABLES["fused"].items():
        out += [(f"fused-{lay}-{c.fam}-{c.n}x{c.h}x{c.w}-k{c.co}-m{c.ci}", lay, FL.fused_operands(c, _ws(c, True))) for c in cases]
    for lay, cases in TABLES["wgrad"].items():
        out += [(f"wgrad-{lay}-{c.n}x{c.h}x{c.w}-c{c.c0}+{c.c1}-m{c.co}-f{c.form}", lay, FL.wgrad_operands(c)) for c, _ in cases]
    for lay, cases in TABLES["wgrad_bn"].items():
        out += [(f"wgrad_bn-{lay}-{n}x{h}x{w}", lay, FL.wgrad_bn_operands(n, h, w)) for n, h, w in cases]
    for lay, cases in TABLES["convT"].items():
        out += [(f"convT-{lay}-{n}x{h}x{w}-k{ci}-m{co}", lay, FL.convT_operands(n, h, w, ci, co)) for n, h, w, ci, co in cases]
    return out


LAUNCHES = launches()


def test_layout_constants():
    L = FL.LAYOUTS
    assert L["n31"].n_stride == 2 ** 29 + 64 and L["n33"].n_stride == 2 ** 31 + 64
    assert L["c29"].c_stride == 2 ** 27 + 64 and L["c29"].n_stride == 16 * L["c29"].c_stride
    assert L["c25"].c_stride == 2 ** 25 + 64 and L["c25"].n_stride == 64 * L["c25"].c_stride
    for lay in L.values():
        assert lay.n_stride % 4 == 0 and (lay.c_stride or 4) % 4 == 0, "the 16-byte forms need strides on a multiple of 4 floats"
    assert FL.FRONT == 2 ** 31 and FL.ARENA_ELEMS * 4 <= 25 * 2 ** 30
    # c29: channel 4 / channel 8 / image 1 behind 2^31 B / 2^32 B / 2^31 elements; dfast off; both dW guards trip under c25
    cs = L["c29"].c_stride
    assert 4 * cs * 4 > 2 ** 31 and 8 * cs * 4 > 2 ** 32 and L["c29"].n_stride > 2 ** 31
    assert 4 * 12 * cs >= 2 ** 32                                     # gsd_conv3x3_w2d.hip: P.dfast stays 0
    cs = L["c25"].c_stride
    assert 64 * cs * 4 >= 2 ** 31 and 64 * cs >= 2 ** 31              # gsd_wgrad_w2d_use; the row form's bx4
    assert 32 * cs < 2 ** 31                                          # (BN = 32 keeps its 16-byte activation pieces)


def test_aliases_of_an_offset():
    assert FL.aliases(100) == []                                      # below every line: nothing to slip
    d = 2 ** 29 + 64                                                  # 2^31 + 256 bytes
    assert dict(FL.aliases(d)) == {"byte offset sign-extended": -(2 ** 29) + 64}
    d = 2 ** 31 + 64
    assert dict(FL.aliases(d)) == {"byte offset mod 2^32": 64, "byte offset sign-extended": 64, "element offset sign-extended": -(2 ** 31) + 64}
    d = 2 ** 32 + 128
    assert dict(FL.aliases(d)) == {"byte offset mod 2^32": 128, "byte offset sign-extended": 128, "element offset mod 2^32": 128,
                                   "element offset sign-extended": 128}


@pytest.mark.parametrize("name,lay,ops", LAUNCHES, ids=[x[0] for x in LAUNCHES])
def test_placement_of_a_launch(name, lay, ops):
    pl = FL.dry(lay, ops)
    iv = pl.intervals()                                               # raises when two planes overlap
    assert iv[0][0] >= FL.FRONT + 64 and iv[-1][1] + 64 <= FL.ARENA_ELEMS
    for a, b in zip(iv, iv[1:]):
        assert a[1] <= b[0]
    # operands of one launch: at least 64 floats of fill between any two
    for i, r in enumerate(pl.recs):
        for s in pl.recs[i + 1:]:
            assert s.off - r.off >= 64
    crossed = pl.lines_crossed()
    big = max(r.n for r in pl.recs) == pl.layout.max_n and (pl.layout.max_c is None or max(r.c for r in pl.recs) >= 13)
    if big:
        for line in MUST_CROSS[lay]:
            assert line in crossed, f"{name}: no plane starts behind {line}"
    starts = {s for r in pl.recs for _, _, s, _ in pl.planes(r)}
    kinds = {}
    for k, i, j, kind, where, cls in pl.alias_report():
        assert cls != "outside", f"{name}: the {kind} alias of operand {k} plane ({i},{j}) leaves the arena"
        assert where not in starts, f"{name}: the {kind} alias of operand {k} plane ({i},{j}) is another plane's start"
        kinds.setdefault(kind, set()).add(cls)
    # what sign extension sends backwards lands in the front headroom: fill, always
    for k, i, j, kind, where, cls in pl.alias_report():
        if where < FL.FRONT:
            assert cls == "fill" and kind.endswith("sign-extended")


def test_every_layout_has_launches_that_cross_its_lines():
    for lay, lines in MUST_CROSS.items():
        got = set()
        for name, l2, ops in LAUNCHES:
            if l2 == lay:
                got |= set(FL.dry(lay, ops).lines_crossed())
        assert set(lines) <= got, (lay, got)


def test_alias_kinds_per_layout():
    """Which aliases lie in fill (a read there is a NaN, a write a changed word) and which on other data of the launch."""
    fill = {}
    for name, lay, ops in LAUNCHES:
        for k, i, j, kind, where, cls in FL.dry(lay, ops).alias_report():
            fill.setdefault((lay, kind), set()).add(cls)
    # the sign-extended aliases of the first line a layout crosses go backwards, into the headroom
    assert "fill" in fill[("n31", "byte offset sign-extended")]
    assert "fill" in fill[("n33", "element offset sign-extended")]
    assert "fill" in fill[("c29", "byte offset sign-extended")] and "fill" in fill[("c29", "element offset sign-extended")]
    assert "fill" in fill[("c25", "byte offset sign-extended")] and "fill" in fill[("c25", "element offset sign-extended")]
    # n31 never forms an element offset of 2^31 or more
    assert ("n31", "element offset mod 2^32") not in fill and ("n31", "element offset sign-extended") not in fill


def test_folded_w43_is_refused_where_the_batch_offset_leaves_32_bits():
    ran = [c for c in TABLES["conv"]["n31"] if c.fam == "w43" and T.plan_w43(c.n, c.h, c.w, c.co, T.env_of(c)).fold]
    assert ran and not any(FL.fold_refused("n31", c.fam, c.n, c.h, c.w, c.co, T.env_of(c)) for c in ran)
    for lay in ("n33", "c29"):
        ref = [c for c in TABLES["conv"][lay] if FL.fold_refused(lay, c.fam, c.n, c.h, c.w, c.co, T.env_of(c))]
        assert ref, f"{lay}: no folded case to refuse"
        # no folded plan is admitted there: N * n_stride >= 2^31 already at N = 1 (n33) and N = 2 (c29)
        assert FL.LAYOUTS[lay].n_stride * 2 >= 2 ** 31
