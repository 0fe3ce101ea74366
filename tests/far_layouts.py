"""Far placements: small NCHW operands whose images or planes lie gigabytes apart inside one fp32 arena, so that every address
a strided kernel forms crosses the 2^31-byte, 2^32-byte, 2^31-element and 2^32-element lines while the tensors stay a few
kilobytes.  A helper module (tests/test_far_layouts_cpu.py proves its arithmetic; tests/test_gpu_far_strides_fp64.py launches
through it), not collected.  The arithmetic half imports nothing; torch is imported only when an Arena is allocated.

Layouts (strides in floats, all multiples of 4 so the 16-byte forms stay eligible):
    n31   n_stride = 2^29 + 64, compact planes, up to 3 images: image bases at 0, just past 2^31 B, just past 2^32 B
    n33   n_stride = 2^31 + 64, compact planes, up to 3 images: image bases at 0, just past 2^31 and 2^32 ELEMENTS (8 / 16 GiB)
    c29   c_stride = 2^27 + 64, n_stride = 16 * c_stride, up to 16 channels and 2 images: channel 4 starts past 2^31 B,
          channel 8 past 2^32 B, image 1 past 2^31 elements (and its last planes end just past 2^32 elements)
    c25   c_stride = 2^25 + 64, n_stride = 64 * c_stride, up to 64 channels and 2 images: c29 for the dW kernels, whose blocks
          take 64 channels (channel 16 past 2^31 B, channel 32 past 2^32 B, image 1 past 2^31 elements)

Every operand starts FRONT = 2^31 floats (8 GiB) into the arena: an offset that was cut to 32 bits and sign-extended -- at most
2^31 elements backwards -- still lands inside the allocation.  The operands of one launch share the strides of the layout and lie
at distinct small offsets (a `band` of at most BAND floats) behind FRONT.

The arena holds one NaN bit pattern (FILL) everywhere and is compared as int32: a read outside an operand shows as a NaN in a
result, a write outside as a changed word.

A 32-bit slip in the offset D = n * n_stride + c * c_stride of a plane can land on four other addresses (aliases): the byte
offset 4 D modulo 2^32 or sign-extended from 32 bits, and the element offset D modulo 2^32 or sign-extended.  aliases(D) lists
those that differ from D.  Most lie in fill.  Some cannot: with n_stride = 2^29 + 64 the byte offset of image 2 is
2^32 + 512, and its low word, 128 floats, lies inside image 0 of the same operand whenever an image is larger than 128 floats
(and so for image 2 of n33 and the planes of c29 modulo 2^32).  Such an alias lands on OTHER DATA of the launch, displaced by
a multiple of 64 floats that is no multiple of the plane: a read there takes different random values and a write lands on
elements the bound check or the sentinel check of that operand sees.  classify() tells the two kinds apart and the CPU test
states which alias of which plane is of which kind.
"""
from __future__ import annotations

from collections import namedtuple
from typing import List, Optional, Tuple

FILL = 0x7FC12345                   # a quiet NaN with a payload no kernel produces
FILL_I32 = FILL                     # (below 2^31: the same number as an int32)
FRONT = 1 << 31                     # floats in front of every operand
BAND = 1 << 22                      # floats a launch's operands may take up behind each plane / image base
LINES = {"2^31 B": 1 << 29, "2^32 B": 1 << 30, "2^31 el": 1 << 31, "2^32 el": 1 << 32}      # in floats

Layout = namedtuple("Layout", "name n_stride c_stride max_n max_c")
LAYOUTS = {
    "n31": Layout("n31", (1 << 29) + 64, None, 3, None),
    "n33": Layout("n33", (1 << 31) + 64, None, 3, None),
    "c29": Layout("c29", 16 * ((1 << 27) + 64), (1 << 27) + 64, 2, 16),
    # dW needs 64 channels a block (BM = BN = 64): 64 planes 2^27 floats apart would be 32 GiB an image.  The same idea at a quarter
    # of the plane distance: channel 16 starts past 2^31 B, channel 32 past 2^32 B, image 1 past 2^31 elements, and both dW guards
    # trip -- 64 * c_stride * 4 >= 2^31 (gsd_wgrad_w2d_use) and 64 * c_stride >= 2^31 (the row form's 16-byte activation pieces)
    "c25": Layout("c25", 64 * ((1 << 25) + 64), (1 << 25) + 64, 2, 64),
}
SPAN = max((L.max_n - 1) * L.n_stride + ((L.max_c or 1) - 1) * (L.c_stride or 0) for L in LAYOUTS.values())       # the farthest plane base of any layout
ARENA_ELEMS = FRONT + SPAN + 2 * BAND               # 24 GiB + 32 MiB: FRONT, every true and every aliased offset, the bands
assert SPAN >= 1 << 32
assert ARENA_ELEMS * 4 <= 25 << 30

Rec = namedtuple("Rec", "off n c h p n_stride c_stride")       # one operand: off = floats from the arena's start to (0,0,0,0)


def _sext32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def aliases(d: int) -> List[Tuple[str, int]]:
    """Where the element offset d lands after a 32-bit slip, as element offsets; only those that differ from d."""
    out = [("byte offset mod 2^32", ((4 * d) & 0xFFFFFFFF) // 4), ("byte offset sign-extended", _sext32(4 * d) // 4),
           ("element offset mod 2^32", d & 0xFFFFFFFF), ("element offset sign-extended", _sext32(d))]
    return [(k, v) for k, v in out if v != d]


def strides_of(layout: Layout, c: int, h: int, p: int) -> Tuple[int, int]:
    """(n_stride, c_stride) of a (c, h, p) operand under `layout`."""
    if layout.c_stride is None:
        return layout.n_stride, h * p
    return layout.n_stride, layout.c_stride


class Placement:
    """Hands out operand positions of one launch under one layout.  Pure arithmetic unless made by an Arena (then view()
    returns tensors)."""

    def __init__(self, layout: str, arena: Optional["Arena"] = None):
        self.layout = LAYOUTS[layout]
        self.arena = arena
        self.cursor = 64
        self.recs: List[Rec] = []

    def reserve(self, n: int, c: int, h: int, p: int, misalign: int = 0) -> Rec:
        """An (n, c, h, p) operand (p: the row pitch) starting `misalign` floats off 16-byte alignment."""
        L = self.layout
        if n > L.max_n or (L.max_c is not None and c > L.max_c):
            raise ValueError(f"layout {L.name} holds at most {L.max_n} images of {L.max_c} channels, asked for {n} x {c}")
        ns, cs = strides_of(L, c, h, p)
        extent = h * p if L.c_stride is not None else c * h * p           # what the operand takes up behind each base
        # the k-th operand starts 4 k floats off a multiple of 64: the aliases of a plane are displaced by multiples of 64 floats
        # (the + 64 of the strides), so none of them is the start of a plane of another operand
        stagger = 4 * (len(self.recs) % 16)
        rec = Rec(FRONT + self.cursor + stagger + misalign, n, c, h, p, ns, cs)
        self.cursor += (extent + stagger + misalign + 63) // 64 * 64 + 64   # 64 floats of fill at least between two operands
        if self.cursor > BAND:
            raise ValueError("the operands of one launch outgrow the band")
        self.recs.append(rec)
        return rec

    # ---- arithmetic the CPU test proves
    def planes(self, rec: Rec):
        """(n, c, first float, one past the last float) of every plane of an operand, in floats from the arena's start."""
        for i in range(rec.n):
            for j in range(rec.c):
                s = rec.off + i * rec.n_stride + j * rec.c_stride
                yield i, j, s, s + rec.h * rec.p

    def intervals(self) -> List[Tuple[int, int]]:
        """Sorted, merged [lo, hi) of everything the launch owns."""
        iv = sorted((s, e) for r in self.recs for _, _, s, e in self.planes(r))
        out: List[Tuple[int, int]] = []
        for s, e in iv:
            if out and s < out[-1][1]:
                raise AssertionError(f"planes overlap: {out[-1]} and {(s, e)}")
            if out and s == out[-1][1]:          # the next plane of a compact operand
                out[-1] = (out[-1][0], e)
            else:
                out.append((s, e))
        return out

    def classify(self, lo: int, hi: int, iv=None) -> str:
        """'fill' when [lo, hi) touches nothing the launch owns, 'outside' when it leaves the arena, else 'data'."""
        if lo < 0 or hi > ARENA_ELEMS:
            return "outside"
        for s, e in (self.intervals() if iv is None else iv):
            if lo < e and s < hi:
                return "data"
        return "fill"

    def alias_report(self):
        """For every plane of every operand and each alias of its offset: (operand index, n, c, kind, where it lands, class)."""
        out, iv = [], self.intervals()
        for k, r in enumerate(self.recs):
            for i, j, s, e in self.planes(r):
                d = s - r.off
                for kind, a in aliases(d):
                    out.append((k, i, j, kind, r.off + a, self.classify(r.off + a, r.off + a + r.h * r.p, iv)))
        return out

    def lines_crossed(self):
        """Which of the four lines some plane of the launch starts behind (offsets are counted from the operand's own base, as a
        kernel forms them) -- and, for each, the smallest such offset."""
        got = {}
        for r in self.recs:
            for i, j, s, e in self.planes(r):
                d = s - r.off
                for name, line in LINES.items():
                    if d >= line and (name not in got or d < got[name]):
                        got[name] = d
        return got

    # ---- tensors (an Arena's placement only)
    def view(self, n: int, c: int, h: int, p: int, misalign: int = 0):
        rec = self.reserve(n, c, h, p, misalign)
        return self.arena.words.view(self.arena.torch.float32).as_strided((n, c, h, p), (rec.n_stride, rec.c_stride, p, 1), rec.off)

    def int_view(self, rec: Rec):
        return self.arena.words.as_strided((rec.n, rec.c, rec.h, rec.p), (rec.n_stride, rec.c_stride, rec.p, 1), rec.off)

    def restore(self):
        """Put the fill pattern back over every operand handed out."""
        for r in self.recs:
            self.int_view(r).fill_(FILL_I32)


class Arena:
    """ARENA_ELEMS words of FILL on the GPU.  scan(): every word that no longer holds FILL, chunk by chunk."""
    CHUNK = 1 << 28

    def __init__(self, elems: int = ARENA_ELEMS, device: str = "cuda"):
        import torch
        self.torch = torch
        self.elems = elems
        self.words = torch.full((elems,), FILL_I32, dtype=torch.int32, device=device)
        self.scan_s = []

    def placement(self, layout: str) -> Placement:
        return Placement(layout, self)

    def scan(self, repair: bool = True) -> List[int]:
        """Word indices (the first few) that do not hold FILL; with `repair` they are put back so that one case's damage is not
        reported by the next."""
        import time
        torch = self.torch
        torch.cuda.synchronize()
        t0 = time.time()
        bad: List[int] = []
        fill = FILL_I32
        for lo in range(0, self.elems, self.CHUNK):
            ch = self.words[lo:lo + self.CHUNK]
            ne = ch != fill
            if bool(ne.any()):
                idx = ne.nonzero()[:16, 0]
                bad.extend(int(i) + lo for i in idx.tolist())
                if repair:
                    ch.fill_(fill)
        torch.cuda.synchronize()
        self.scan_s.append(time.time() - t0)
        return bad

    def free(self):
        self.words = None
        self.torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- operand sets of the launches
# What tests/test_gpu_tile_forms_fp64.py carves from a placement for one case, in the order it asks: (n, c, h, pitch, misalign).
# The GPU module holds each far case to these lists (Placement.recs must equal the dry placement's), so what the CPU test
# proves about them holds for the launches.  `ws`: floats of K-slab scratch the library asks for (forward, dX), where a case
# forces a split.
def _r4(v: int) -> int:
    return (v + 3) // 4 * 4


def _r64(v: int) -> int:
    return (v + 63) // 64 * 64


def _flat(k: int):
    return (1, 1, 1, max(int(k), 1) + 64, 0)


def conv_operands(c, ws=(0, 0)):
    import tile_cases as T
    n, h, w, c0, c1, co, fam = c.n, c.h, c.w, c.c0, c.c1, c.co, c.fam
    ci = c0 + c1
    env = T.env_of(c)
    aligned, mis = c.form in ("x4", "slice"), 1 if c.form == "dword" else 0
    p0 = _r4(w) if aligned else w
    ops = [(n, c0 + 5 if c.form == "slice" else c0, h, p0, mis)]
    geom = [(h, w)]
    if c1:
        _, _, uh, uw = T.second_segment(c.form, h, w)
        ops.append((n, c1, uh, uw, 0))
        geom.append((uh, uw))
    ops.append((n, co + 5, h, _r4(w), 0) if c.form == "slice" else (n, co, h, _r4(w) if aligned else w + 1, 0))
    ops.append(_flat(T.conv_partial_rows(fam, n, h, w, co, env) * 2 * _r64(co)))
    if ws[0]:
        ops.append(_flat(ws[0]))
    kd = _r4(co) if fam == "w2d" else co
    ops.append((n, kd, h, p0, mis))
    for (uh, uw), ch in zip(geom, (c0, c1)):
        ops.append((n, ch + 5 if c.form == "slice" else ch, uh, _r4(uw) if aligned else uw + 1, 0))
    if len(geom) == 2 and fam != "direct":
        ops.append(_flat(T.conv_partial_rows(fam, n, h, w, ci, env) * 2 * _r64(ci)))
    if ws[1]:
        ops.append(_flat(ws[1]))
    return ops


def fused_operands(c, ws=0):
    import tile_cases as T
    n, h, w, co, ci = c.n, c.h, c.w, c.co, c.ci
    ops = [(n, co, h, _r4(w) if c.fam != "direct" else w, 0), (n, ci, h, w, 0),
           _flat(T.conv_partial_rows(c.fam, n, h, w, ci, T.env_of(c)) * 2 * _r64(ci)), (n, ci, h, w, 0)]
    if ws:
        ops.append(_flat(ws))
    return ops


def wgrad_operands(c):
    import tile_cases as T
    ops = [(c.n, c.c0, c.h, c.w, 0)]
    if c.c1:
        _, _, uh, uw = T.second_segment("two11", c.h, c.w)
        ops.append((c.n, c.c1, uh, uw, 0))
    ops.append((c.n, c.co, c.h, _r4(c.w) if c.pitched else c.w, 0))
    return ops


def wgrad_bn_operands(n, h, w):
    return [(n, 3, h, w, 0)]


def convT_operands(n, h, w, ci, co):
    rows = -(-n * h * (w + w % 2) // 128) * 2
    return [(n, ci, h, w, 0), (n, co, 2 * h, 2 * w, 0), (n, co, 2 * h, 2 * w, 0), (n, ci, h, w, 0), (n, ci, h, w, 0),
            _flat(rows * 2 * _r64(ci)), (n, ci, h, w, 0)]


def dry(layout: str, ops) -> Placement:
    pl = Placement(layout)
    for n, c, h, p, mis in ops:
        pl.reserve(n, c, h, p, mis)
    return pl


# ------------------------------------------------------------------------------------------------------------- case tables
# One small shape per kernel path and layout.  Under n31 / n33 every case has 3 images (image 2 is the one behind the 2^32-byte /
# 2^32-element line); under c29 / c25 2 images of at most 16 / 64 channels.  Built from the entries of tile_cases.py (the same
# shapes, N raised to 3) so that the planners restated there say which tile form each one reaches.
def _tables():
    import tile_cases as T
    cc, FC, WG = T._cc, T.FusedCase, T.WgCase
    nfar = [c._replace(n=3) for c in T.CONV_CASES if (c.fam, c.h, c.w, c.form) in {
        ("w2d", 4, 64, "x4"), ("w2d", 12, 45, "slack_bn"), ("w2d", 9, 11, "two11"), ("w2d", 21, 29, "two04"), ("w2d", 6, 70, "dword"),
        ("w2d", 21, 29, "slice"), ("w2d", 30, 7, "x4"), ("w2d", 15, 13, "slack"),
        ("w43", 12, 45, "x4"), ("w43", 30, 7, "two11"), ("w43", 15, 13, "slack_bn"), ("w43", 21, 29, "two04"), ("w43", 33, 3, "slack"),
        ("w43", 18, 20, "x4"), ("w43", 9, 11, "two11"), ("w43", 9, 50, "slack_bn"), ("w43", 13, 28, "slice"),
        ("direct", 9, 11, "slack"), ("direct", 6, 70, "two11"), ("direct", 15, 13, "slack_bn"), ("direct", 21, 29, "dword")}]
    nfar += [c for c in T.SPLIT_CASES if (c.n, c.c0) == (3, 32)]                 # the _ws launches: 3 x 30 x 7, 64 channels, 2 slabs
    f0 = {"GSD_W43_FOLD": 0}
    cfar = [cc("w2d", 2, 12, 45, 8, 0, 8, "slack_bn"), cc("w2d", 2, 9, 11, 8, 8, 16, "two11"), cc("w2d", 2, 7, 29, 12, 0, 16, "x4"),
            cc("w2d", 2, 6, 70, 8, 0, 16, "dword"), cc("w2d", 2, 21, 29, 8, 0, 8, "slice"), cc("w2d", 2, 21, 29, 8, 8, 12, "two04"),
            cc("w2d", 2, 33, 3, 8, 0, 16, "slack_bn"),
            cc("w43", 2, 12, 45, 8, 0, 7, "x4", **f0), cc("w43", 2, 30, 7, 6, 5, 16, "two11", **f0),
            cc("w43", 2, 15, 13, 8, 0, 16, "slack_bn", **f0), cc("w43", 2, 6, 70, 6, 5, 16, "two04"), cc("w43", 2, 2, 4, 8, 0, 7, "x4"),
            cc("direct", 2, 9, 11, 3, 0, 16, "slack"), cc("direct", 2, 6, 70, 4, 3, 13, "two11"), cc("direct", 2, 15, 13, 8, 0, 7, "slack_bn")]
    fused_n = [c._replace(n=3) for c in T.FUSED_CASES if (c.fam, c.h, c.w) in {
        ("w2d", 12, 45), ("w2d", 30, 7), ("w43", 12, 45), ("w43", 9, 11), ("w43", 7, 48), ("direct", 9, 11), ("direct", 21, 29)}]
    fused_c = [FC("w2d", 2, 12, 45, 8, 16, ()), FC("w43", 2, 12, 45, 8, 12, (("GSD_W43_FOLD", 0),)), FC("w43", 2, 9, 11, 8, 16, ()),
               FC("direct", 2, 9, 11, 8, 16, ())]
    direct_dw = [WG(3, 9, 11, 8, 0, 8, False, 0, False, 0, ()), WG(3, 12, 45, 40, 0, 8, False, 4, True, 0, ())]
    wg_n = [c._replace(n=3) for c in T.WG_CASES] + direct_dw
    # c25: (case, the form the library must report).  The two-dimensional cases fall back to the row form (gsd_wgrad_w2d_use: 64 planes
    # of dy span 2^31 bytes or more), and the row form drops its 16-byte activation pieces where BN = 64 (gsd_wgrad_w43_run)
    wg_c = [(c, 1 if c.form == 2 else c.form) for c in T.WG_CASES if max(c.c0, c.c1, c.co) <= 64 and not c.env]
    wg_c += [(direct_dw[0]._replace(n=2), 0)]
    convT_n = [(3, 5, 53, 36, 40), (3, 4, 5, 8, 32), (3, 3, 2, 36, 40)]
    convT_c = [(2, 4, 5, 8, 16), (2, 5, 7, 16, 12)]
    return {"conv": {"n31": nfar, "n33": nfar, "c29": cfar}, "fused": {"n31": fused_n, "n33": fused_n, "c29": fused_c},
            "wgrad": {"n31": [(c, c.form) for c in wg_n], "n33": [(c, c.form) for c in wg_n], "c25": wg_c},
            "wgrad_bn": {"n31": [(3, 9, 37)], "n33": [(3, 7, 50)]},
            "convT": {"n31": convT_n, "n33": convT_n, "c29": convT_c}}


def fold_refused(layout: str, fam: str, n: int, h: int, w: int, m: int, env) -> bool:
    """gsd_conv3x3_w43 folds images into tile rows whose lane offsets carry n * n_stride in 32 bits: a plan that folds is refused
    (GSD_ERR_UNSUPPORTED, "batch too large for row folding") where N * n_stride >= 2^31 -- n33, c29; n31 (3 * (2^29 + 64)) folds."""
    import tile_cases as T
    if fam != "w43":
        return False
    p = T.plan_w43(n, h, w, m, env)
    return bool(p.fold) and n * LAYOUTS[layout].n_stride >= 1 << 31
