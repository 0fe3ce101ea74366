"""Far placements for the bf16 NHWC family: kilobyte-sized gsd_nhwc operands whose PIXELS lie megabytes apart inside one bf16 arena, so
that every address a kernel forms from `pixel * pitch` or from an image base `n * H * W * pitch` crosses the 2^30-, 2^31- and
2^32-element lines (2, 4 and 8 GiB) while the tensors stay small.  A helper module (tests/test_bf16_far_layouts_cpu.py proves its
arithmetic; tests/test_gpu_bf16_far_pitch_fp64.py launches through it), not collected.  The arithmetic half imports nothing; torch
is imported only when an Arena is allocated.

gsd_nhwc has no image stride, only `pitch`: distance comes from a giant pitch.  An operand is channels [off, off + C) of a contiguous
(N, H, W, PITCH) bf16 view of the arena that starts FRONT elements into it; _lib.make_nhwc takes that view unchanged.  The operands of
one launch are disjoint channel ranges at small offsets (below BAND channels) of the same pixels; operands with other extents (the
ConvT's 2h x 2w side, a pooled tensor) are other views over the same elements.

Layouts (pitch in elements, a multiple of 8; the + 64 keeps every alias of a pixel off the start of another operand's pixel):
    few    pitch 2^23 + 64, at most 752 pixels, one image below 2^30 elements (H*W <= 127): with 5 images of 7 x 16, image 1 straddles
           2^30 elements, image 2 straddles 2^31 (4 GiB), image 4 straddles 2^32 (8 GiB); the buffer-descriptor fills of
           gsd_bf16_conv3x3, gsd_bf16_conv3x3_c64 and the general gsd_bf16_wgrad stay on
    big    the same pitch with images of 128 .. 255 pixels: one image lies between 2^30 and 2^31 elements -- gsd_bf16_conv3x3 runs
           its 64-bit fill path, gsd_bf16_conv3x3_c64 and the general gsd_bf16_wgrad refuse
    many   pitch 2^19 + 64, at most 8000 pixels (4096 pixels are 2^31 elements): for what needs thousands of pixels to pick its form
           (the multi-pixel apply kernels, the large-tile ConvT and dW plans), and for pairs of shapes just below and just above
           N*H*W*pitch = 2^31 and (N*H*W + 512) * pitch = 2^31, where gsd_bf16_wgrad and gsd_ctgemm_operands switch kernels

Every operand starts FRONT = 2^31 elements (4 GiB) into the arena.  The possible slips are a byte or element offset taken modulo 2^32
or sign-extended from 32 bits, and an `int` pixel * pitch or image base; each moves an address by a multiple of 2^31 elements at most
2^32 back, so with that FRONT the slipped address still lies inside the allocation: a slip shows as wrong data (a NaN of the fill) or
as a changed word, never as a fault.  aliases() lists them, Placement.alias_report() classifies where each lands; the CPU test
asserts that none leaves the arena and that every one lands in fill (a displaced pixel keeps its channel offset plus a multiple of
64 * 256 or 64 * 4096 channels, far above BAND).

The arena is ARENA_ELEMS bf16 elements = 15.77 GiB (at most 16 GiB), all of one NaN bit pattern that no kernel produces (a
signalling bf16 NaN: arithmetic quiets it), compared as int32 words.
"""
from __future__ import annotations

from collections import namedtuple
from typing import List, Optional, Tuple

FILL16 = 0x7FA5                     # a signalling bf16 NaN with a payload
FILL32 = (FILL16 << 16) | FILL16    # two of them: the arena is scanned as int32 words (below 2^31: the same number as an int32)
FRONT = 1 << 31                     # elements in front of every operand
BAND = 8192                         # channels the operands of one launch may take up behind FRONT
LINES = {"2^30 el": 1 << 30, "2^31 el": 1 << 31, "2^32 el": 1 << 32}

Layout = namedtuple("Layout", "name pitch max_pixels image_lo image_hi")       # image_lo <= H*W*pitch < image_hi for the largest view
LAYOUTS = {
    "few": Layout("few", (1 << 23) + 64, 752, 0, 1 << 30),
    "big": Layout("big", (1 << 23) + 64, 752, 1 << 30, (1 << 31) - 1),
    "many": Layout("many", (1 << 19) + 64, 8000, 0, 1 << 30),
}
SPAN = max(L.max_pixels * L.pitch for L in LAYOUTS.values())
ARENA_ELEMS = FRONT + SPAN + max(L.pitch for L in LAYOUTS.values())         # FRONT, every pixel of the largest view, its last pitch
assert ARENA_ELEMS % 2 == 0 and ARENA_ELEMS * 2 <= 16 << 30

Rec = namedtuple("Rec", "off n h w tot")        # one buffer: channels [off, off + tot) of the (n, h, w, pitch) view


def _sext32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def aliases(d: int) -> List[Tuple[str, int]]:
    """Where the element offset d lands after a 32-bit slip, as element offsets; only those that differ from d."""
    out = [("byte offset mod 2^32", ((2 * d) & 0xFFFFFFFF) // 2), ("byte offset sign-extended", _sext32(2 * d) // 2),
           ("element offset mod 2^32", d & 0xFFFFFFFF), ("element offset sign-extended / int", _sext32(d))]
    return [(k, v) for k, v in out if v != d]


class Placement:
    """Hands out the buffers of one launch under one layout.  Pure arithmetic unless made by an Arena (then view() returns tensors)."""

    def __init__(self, layout: str, arena: Optional["Arena"] = None):
        self.layout = LAYOUTS[layout]
        self.arena = arena
        self.cursor = 64
        self.recs: List[Rec] = []

    def reserve(self, n: int, h: int, w: int, tot: int) -> Rec:
        L = self.layout
        if n * h * w > L.max_pixels:
            raise ValueError(f"layout {L.name} holds at most {L.max_pixels} pixels, asked for {n} x {h} x {w}")
        if h * w * L.pitch >= L.image_hi:
            raise ValueError(f"layout {L.name}: an image of {h} x {w} pixels is {h * w * L.pitch} elements, not below {L.image_hi}")
        # the k-th buffer starts 8 (k mod 8) channels off a multiple of 64: aliases are displaced by multiples of 64 channels (the + 64
        # of the pitch times a pixel count), so none of them is the start of a pixel of another buffer
        stagger = 8 * (len(self.recs) % 8)
        rec = Rec(self.cursor + stagger, n, h, w, tot)
        self.cursor += (tot + stagger + 63) // 64 * 64 + 64       # 64 channels of fill at least between two buffers
        if self.cursor > BAND:
            raise ValueError("the operands of one launch outgrow the band")
        self.recs.append(rec)
        return rec

    # ---- arithmetic the CPU test proves
    def largest_image(self) -> int:
        return max(r.h * r.w for r in self.recs) * self.layout.pitch

    def pixel_offset(self, rec: Rec, p: int) -> int:
        """Element offset of pixel p (flattened over n, h, w) from the buffer's own base, as a kernel forms it."""
        return p * self.layout.pitch

    def spans(self, rec: Rec):
        """(pixel, first element, one past the last) of every pixel of a buffer, in elements from the arena's start."""
        for p in range(rec.n * rec.h * rec.w):
            s = FRONT + rec.off + p * self.layout.pitch
            yield p, s, s + rec.tot

    def disjoint(self) -> bool:
        """Buffers share pixels (the same view, or views of other extents over the same elements): they are disjoint exactly when
        their channel ranges are, and every range ends inside one pitch."""
        iv = sorted((r.off, r.off + r.tot) for r in self.recs)
        return all(a[1] <= b[0] for a, b in zip(iv, iv[1:])) and iv[-1][1] <= BAND < self.layout.pitch

    def classify(self, lo: int, hi: int) -> str:
        """'fill' when [lo, hi) touches no buffer of the launch, 'outside' when it leaves the arena, else 'data'."""
        if lo < 0 or hi > ARENA_ELEMS:
            return "outside"
        P = self.layout.pitch
        for r in self.recs:
            b0 = FRONT + r.off
            if hi <= b0:
                continue
            # pixels whose channel range [b0 + p P, b0 + p P + tot) can meet [lo, hi)
            p_lo = max(0, (lo - b0 - r.tot) // P + 1) if lo > b0 + r.tot - 1 else 0
            p_hi = min(r.n * r.h * r.w - 1, (hi - 1 - b0) // P)
            for p in range(p_lo, p_hi + 1):
                s = b0 + p * P
                if lo < s + r.tot and s < hi:
                    return "data"
        return "fill"

    def alias_report(self):
        """For every pixel of every buffer, each alias of its offset and each alias of its image base carried into the pixel:
        (buffer index, pixel, kind, where it lands, class)."""
        out = []
        P = self.layout.pitch
        for k, r in enumerate(self.recs):
            b0 = FRONT + r.off
            for p in range(r.n * r.h * r.w):
                d = p * P
                base = (p // (r.h * r.w)) * r.h * r.w * P
                cand = aliases(d) + [("image base: " + kind, a + d - base) for kind, a in aliases(base)]
                for kind, a in cand:
                    if a != d:
                        out.append((k, p, kind, b0 + a, self.classify(b0 + a, b0 + a + r.tot)))
        return out

    def lines_crossed(self):
        """For each line, the first (buffer index, image, pixel) whose offset from its buffer's base lies at or past it."""
        got = {}
        P = self.layout.pitch
        for k, r in enumerate(self.recs):
            for name, line in LINES.items():
                p = -(-line // P)
                if p < r.n * r.h * r.w and (name not in got or p < got[name][2]):
                    got[name] = (k, p // (r.h * r.w), p)
        return got

    # ---- tensors (an Arena's placement only)
    def view(self, n: int, h: int, w: int, tot: int):
        """The buffer as an (n, h, w, tot) bf16 tensor over the arena: pixel stride = the layout's pitch."""
        rec = self.reserve(n, h, w, tot)
        P = self.layout.pitch
        return self.arena.bf16.as_strided((n, h, w, tot), (h * w * P, w * P, P, 1), FRONT + rec.off)

    def wide(self, t):
        """(the contiguous (n, h, w, PITCH) view that holds a buffer handed out by view(), the buffer's channel offset in it)."""
        n, h, w, _ = t.shape
        P = self.layout.pitch
        assert t.stride() == (h * w * P, w * P, P, 1), "not a buffer of this placement"
        off = t.storage_offset() - FRONT
        assert any(r.off == off and (r.n, r.h, r.w) == (n, h, w) for r in self.recs), "not a buffer of this placement"
        return self.arena.bf16[FRONT:FRONT + n * h * w * P].view(n, h, w, P), off

    def restore(self):
        """Put the fill pattern back over every buffer handed out."""
        P = self.layout.pitch
        for r in self.recs:
            self.arena.i16.as_strided((r.n * r.h * r.w, r.tot), (P, 1), FRONT + r.off).fill_(FILL16)


class Arena:
    """ARENA_ELEMS bf16 elements of FILL16 on the GPU.  scan(): every int32 word that no longer holds FILL32, chunk by chunk."""
    CHUNK = 1 << 28

    def __init__(self, elems: int = ARENA_ELEMS, device: str = "cuda"):
        import torch
        self.torch = torch
        self.elems = elems
        self.words = torch.full((elems // 2,), FILL32, dtype=torch.int32, device=device)
        self.bf16 = self.words.view(torch.bfloat16)
        self.i16 = self.words.view(torch.int16)
        self.scan_s: List[float] = []

    def placement(self, layout: str) -> Placement:
        return Placement(layout, self)

    def scan(self, repair: bool = True) -> List[int]:
        """Element indices (the first few, even) of the words that do not hold the fill; with `repair` they are put back so that one
        case's damage is not reported by the next."""
        import time
        torch = self.torch
        torch.cuda.synchronize()
        t0 = time.time()
        bad: List[int] = []
        for lo in range(0, self.words.numel(), self.CHUNK):
            ch = self.words[lo:lo + self.CHUNK]
            ne = ch != FILL32
            if bool(ne.any()):
                bad.extend(2 * (int(i) + lo) for i in ne.nonzero()[:16, 0].tolist())
                if repair:
                    ch.fill_(FILL32)
        torch.cuda.synchronize()
        self.scan_s.append(time.time() - t0)
        return bad

    def free(self):
        self.words = self.bf16 = self.i16 = None
        self.torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- case tables
# Built from the namedtuples and planners of bf16_tile_cases.py, at the smallest shapes that reach the form under test.  Per layout:
#   few   N = 5 images of 7 x 16 (N = 3 where three images already cross 2^31 elements and the shape needs more pixels an image)
#   big   N = 3 images of 128 .. 255 pixels
#   many  N = 3 images of 22 x 63 (4158 pixels; 4095 are the last below 2^31 elements), and pairs of ConvT shapes around 4096 pixels
#         (N*H*W*pitch = 2^31) and 3583 pixels ((N*H*W + 512) * pitch = 2^31)
# An entry of the conv3 / dense / wgrad tables is (case, kind): what far_kind() -- the host's size conditions restated with the
# layout's pitch -- must say of the far launch.  The compact launch of every case is "buf" / "ct" or "general" by its shape / "big" or
# "general" by its shape (the CPU test holds each table to both).
def far_kind(c, layout: Optional[str]):
    """Which side of the host's size conditions a case is on when its buffers have the layout's pitch (None: compact).
    conv3: "buf" | "fill64" (conv3x3_impl's P.buf);  dense: "ct" | "general" | "refused" (conv_dense_impl with gsd_ctgemm_operands'
    fits);  wgrad: "big" | "general" (gsd_bf16_wgrad's N*H*W*pitch < 2^31 - 1 for a and b)."""
    import bf16_tile_cases as B
    env = B.env_of(c)
    pitch = (lambda compact: compact) if layout is None else (lambda compact: LAYOUTS[layout].pitch)
    if isinstance(c, B.Conv3):
        return "buf" if B.conv_buf(c.h, c.w, pitch(c.in_tot), c.m, c.k, env) else "fill64"
    if isinstance(c, B.Dense):
        taps, stride = (4, 2) if c.kind == "ctdx" else (1, 1)
        if c.kind != "1x1bnrelu" and B.ctgemm_shape(c.n, c.h, c.w, c.k, c.m, taps, stride, c.cs, env):
            in_, out, ty, tx = B.dense_geometry(c)
            in_, out = in_._replace(pitch=pitch(in_.pitch)), out._replace(pitch=pitch(out.pitch))
            y = B.Buf(c.n, c.h, c.w, pitch(c.m)) if c.fused else None
            if B.ctgemm_operands(in_, out, y, taps, ty, tx, c.h, c.w):
                return "ct"
            if c.fused:
                return "refused"
        return "general"
    a, b, stride, ty, tx = B.wg_geometry(c)
    a, b = a._replace(pitch=pitch(a.pitch)), b._replace(pitch=pitch(b.pitch))
    return "big" if B.wgrad_big(a, b, c.m, c.ncols, c.taps, stride, ty, tx, env) else "general"


def _tables():
    import bf16_tile_cases as B

    def f(c):
        return c._replace(form=B.form_of(c))

    def c3(n, h, w, k, m, ep="stats", in_=None, out=None, env=()):
        it, io = in_ or (k, 0)
        ot, oo = out or (m, 0)
        return f(B.Conv3(n, h, w, k, m, ep, it, io, ot, oo, tuple(env), None))

    def dn(kind, n, h, w, k, m, cs=0, oy=0, ox=0, spare=0, fused=0, env=()):
        return f(B.Dense(kind, n, h, w, k, m, cs, oy, ox, spare, fused, 0, 0, tuple(env), 0, None))

    def wg(taps, n, h, w, m, ncols, ncols_out=None, oy=0, ox=0, b=None, env=()):
        bt, bo = b or (ncols, 0)
        return f(B.Wg(taps, n, h, w, m, ncols, ncols_out or ncols, oy, ox, bt, bo, 0, tuple(env), None))

    def each(kind, cases):
        return [(c, kind) for c in cases]

    conv3 = {
        "few": each("buf", [c3(5, 7, 16, 32, 128), c3(5, 7, 16, 96, 64), c3(5, 7, 16, 128, 96, "bnbwd"), c3(5, 7, 16, 64, 64, "bnbwd"),
                            c3(5, 7, 16, 32, 128, "bnrelu"), c3(5, 7, 16, 32, 80, in_=(96, 32)), c3(5, 7, 16, 32, 48, out=(80, 16)),
                            c3(3, 3, 40, 32, 256)]),
        # one image of 1.17 .. 1.64 * 2^30 elements: the 64-bit fill path (conv3x3_impl: ib >= 2^31 bytes)
        "big": each("fill64", [c3(3, 10, 15, 32, 128), c3(3, 7, 30, 96, 64), c3(3, 10, 15, 128, 96, "bnbwd"),
                               c3(3, 7, 30, 64, 64, "bnbwd"), c3(3, 10, 15, 32, 128, "bnrelu")]),
        "many": each("buf", [c3(3, 22, 63, 32, 128), c3(3, 22, 63, 64, 64, "bnbwd")]),
    }
    _bm256 = (("GSD_BF16_CT_BM", "256"),)
    dense = {
        # the ConvT forward (scatter + bias) and dX at a large-tile shape, on both sides of gsd_ctgemm_operands' `fits`: the gradient /
        # concat buffer of 2 x (28 + oy) x (62 + ox) pixels is 3528 pixels at (0, 1) and 3654 at (1, 1); 3583 fit
        "many": [(dn("ctfwd", 2, 14, 31, 64, 256, cs=64, oy=0, ox=1), "ct"), (dn("ctfwd", 2, 14, 31, 64, 256, cs=64, oy=1, ox=1), "general"),
                 (dn("ctdx", 2, 14, 31, 64, 128, oy=0, ox=1), "ct"), (dn("ctdx", 2, 14, 31, 64, 128, oy=1, ox=1), "general"),
                 (dn("ctdx", 2, 14, 31, 64, 128, oy=0, ox=1, fused=1), "ct"), (dn("ctdx", 2, 14, 31, 64, 128, oy=1, ox=1, fused=1), "refused"),
                 (dn("ctdx", 2, 14, 31, 64, 256, oy=0, ox=1, fused=1, env=_bm256), "ct"),
                 # ... and with the big operand of 3 x 22 x 63 = 4158 pixels, past 2^32 BYTES: what a 32-bit byte offset cannot reach
                 (dn("ctfwd", 3, 11, 31, 64, 256, cs=64, oy=0, ox=1), "general"), (dn("ctdx", 3, 11, 31, 64, 128, oy=0, ox=1), "general")],
        # the general kernel: scatter at Cs 32 (no large-tile shape), dX plain and fused below W = 16, one tap
        "few": each("general", [dn("ctfwd", 5, 3, 6, 64, 128, cs=32, oy=1, ox=1, spare=1), dn("ctdx", 5, 3, 7, 64, 128, oy=1, ox=1),
                                dn("ctdx", 5, 3, 7, 64, 128, oy=0, ox=1, spare=1, fused=1), dn("1x1", 5, 7, 16, 64, 128),
                                dn("1x1bnrelu", 5, 7, 16, 32, 64)]),
        "big": each("general", [dn("1x1", 3, 10, 15, 64, 128), dn("1x1bnrelu", 3, 10, 15, 32, 64),
                                dn("ctfwd", 3, 4, 8, 64, 128, cs=32, oy=0, ox=1)]),
    }
    wgrad = {
        "few": each("general", [wg(9, 5, 7, 16, 128, 64), wg(9, 5, 7, 16, 48, 32, b=(64, 16)), wg(4, 5, 3, 8, 128, 32, oy=1, ox=0, b=(64, 32)),
                                wg(1, 5, 7, 16, 64, 32, ncols_out=27)]),
        # 4 taps at stride 2 at a large-tile shape: b is 3 x (20 + oy) x (62 + ox) pixels, 4095 at (1, 3) and 4158 at (2, 1); 4095 fit
        # (and one image of b stays below 2^30 elements, or the general kernel would refuse what the large tile hands over)
        "many": [(wg(4, 3, 10, 31, 128, 64, oy=1, ox=3, b=(128, 64)), "big"), (wg(4, 3, 10, 31, 128, 64, oy=2, ox=1, b=(128, 64)), "general"),
                 (wg(4, 3, 10, 31, 256, 64, oy=1, ox=3, b=(128, 64)), "big"), (wg(9, 3, 22, 63, 64, 64), "general")],
    }
    # (n, h, w): 64 -> 64 on the weights-resident kernel, and the first layer / `inc` kernels (x stays compact fp32)
    c64 = {"few": [(5, 7, 16), (3, 5, 21)], "many": [(3, 22, 63)]}
    first = {"few": [(5, 7, 16)], "many": [(3, 22, 63)]}
    # gsd_bf16_conv3x3_c64 and the general gsd_bf16_wgrad (9 taps, 1 tap) under `big`: refused.  (n, h, w, M, Ncols)
    refused = {"big": [("c64", (3, 10, 15, 64, 64)), ("wgrad9", (3, 10, 15, 64, 64)), ("wgrad1", (3, 10, 15, 64, 32))]}
    # (n, h, w, C, GSD_BF16_BN_BLOCKS or 0): bn_apply / bn_bwd_apply pick the multi-pixel form where C / 8 divides 256 and
    # N*H*W * C / 8 >= 65536; pick_pixb gives 32 pixels a block below 16385 pixels, the knob makes it 96 at 4158
    pw = {"few": [(5, 7, 16, 64, 0), (5, 7, 16, 2048, 0), (5, 7, 15, 72, 0)],
          "many": [(3, 22, 63, 128, 0), (3, 22, 63, 64, 64), (3, 21, 65, 128, 0)]}
    return {"conv3": conv3, "dense": dense, "wgrad": wgrad, "c64": c64, "first": first, "refused": refused, "pw": pw}


def pw_form(n: int, h: int, w: int, c: int) -> str:
    """multi_ppb of gsd_bf16_bn.hip."""
    groups = c // 8
    return "multi" if groups <= 256 and 256 % groups == 0 and n * h * w * groups >= 65536 else "one-pixel"


def pick_pixb(n: int, hw: int, blocks: int = 0) -> int:
    """pick_pixb of gsd_bf16_pointwise.h."""
    pixb = (n * hw + (blocks or 512) - 1) // (blocks or 512)
    return max(32, (pixb + 31) // 32 * 32)


# ----------------------------------------------------------------------------------------------- buffers of the launches
# What the GPU module carves from a placement for one case, in the order it asks: (n, h, w, channels of the buffer).  The GPU module
# holds each far case to these lists (Placement.recs must equal the dry placement's), so what the CPU test proves about them holds
# for the launches.  The tile-form cases run two passes (random, exact): their buffers come twice.
def conv3_buffers(c):
    ops = [(c.n, c.h, c.w, c.in_tot), (c.n, c.h, c.w, c.out_tot)]
    if c.ep == "bnbwd":
        ops.append((c.n, c.h, c.w, c.m))
    return ops * 2


def dense_buffers(c):
    import bf16_tile_cases as B
    in_, out, _, _ = B.dense_geometry(c)
    ops = [(in_.N, in_.H, in_.W, in_.pitch), (out.N, out.H, out.W, out.pitch)]
    if c.kind == "ctdx" and c.fused:
        ops.append((c.n, c.h, c.w, c.m))
    return ops * 2


def wgrad_buffers(c):
    import bf16_tile_cases as B
    a, b, _, _, _ = B.wg_geometry(c)
    return [(a.N, a.H, a.W, a.pitch), (b.N, b.H, b.W, b.pitch)] * 2


def c64_buffers(n, h, w):
    io = (n, h, w, 80)          # in and out are channels [8, 72) of 80; bw.y is its own 64 channels
    return [io, io] * 2 + [io, io, (n, h, w, 64)] * 2


def first_buffers(n, h, w):
    # y0 (storing form), the eval output, a0 in a 96-channel buffer, y1, da, dz of gsd_bf16_wgrad_first, d_raw, the im2col tensor
    return [(n, h, w, 64), (n, h, w, 64), (n, h, w, 96), (n, h, w, 64), (n, h, w, 64), (n, h, w, 64), (n, h, w, 64), (n, h, w, 32)]


def pw_buffers(n, h, w, c):
    full, pool = (n, h, w, c + 16), (n, h // 2, w // 2, c + 8)
    if c > 256:                 # y, a, dz: the two apply kernels only
        return [full] * 3
    # y, a (relu 0), a (relu 1), a (pool) | pooled x 3 | g, dpool | dz (mode 0, mode 1, pool_idx, mode 2)
    return [full] * 4 + [pool] * 3 + [full, pool] + [full] * 4


def dry(layout: str, ops) -> Placement:
    pl = Placement(layout)
    for n, h, w, tot in ops:
        pl.reserve(n, h, w, tot)
    return pl
