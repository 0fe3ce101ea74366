"""CPU: the band-major flat tile list of conv3x3_w2d_strips_kernel, through the host mirrors of the map the kernel runs
(w2d_group_strips / w2d_tile_of in gsd_conv3x3_w2d_kernel.h, exported as gsd_conv3x3_w2d_strips_plan / _strips_tile).  No device.

A band is two Winograd tile rows of one image across its width (a last band may hold one); tiles are listed image by image, band by
band, column by column, upper tile then lower; pixel group g owns tiles [16 g, 16 g + 16), block b groups 2 b and 2 b + 1.  Inside a
group the tiles of one band are a strip of c whole tile columns whose window is six rows of c + 2 16-byte pieces; the strips lie side
by side.  For each shape:

  * every (image, tile row, tile column) appears in exactly one (group, lane), lanes past the end of the list are marked empty;
  * the block count is ceil(N tiles / 32): 280 at (32, 40, 53) and 70 at (32, 20, 26), against 320 and 96 rectangles;
  * no group has more than three strips, no window row more than 14 pieces: at most 672 pieces per block and chunk;
  * a tile's window -- pieces [piece, piece + 3) of rows 2 (ty & 1) .. + 3 -- lies inside its strip's pieces, tiles of one strip keep
    piece - column constant (they share the columns they share), and strips of one group do not overlap;
  * the listing order is the specified one.

(33, 4, 8) has four tiles per band, so a group would be four strips: refused, and the launcher keeps the rectangles.
"""
import ctypes

import pytest

SHAPES = [(32, 40, 53), (32, 20, 26), (8, 20, 26), (5, 20, 26), (3, 40, 53), (2, 7, 13)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gelslim_depth_amd import _lib
    return _lib.lib


def plan(lib, n, h, w, cin=512, cout=512):
    out = (ctypes.c_int * 7)()
    assert lib.gsd_conv3x3_w2d_strips_plan(n, h, w, cin, cout, out) == 0
    return dict(zip(("blocks", "strips", "pieces", "chunk_pieces", "rect_blocks", "admitted", "taken"), out))


def tile(lib, n, h, w, t):
    out = (ctypes.c_int * 5)()
    assert lib.gsd_conv3x3_w2d_strips_tile(n, h, w, t, out) == 0
    return tuple(out)          # image, tile row, tile column, strip, first piece


@pytest.mark.parametrize("n,h,w", SHAPES, ids=lambda v: str(v))
def test_every_tile_once_in_at_most_three_strips(lib, monkeypatch, n, h, w):
    monkeypatch.setenv("GSD_W2D_STRIPS", "1")
    ty, tx = -(-h // 2), -(-w // 4)
    p = plan(lib, n, h, w)
    assert p["blocks"] == -(-n * ty * tx // 32)
    if (n, h, w) == (32, 40, 53):
        assert (p["blocks"], p["rect_blocks"]) == (280, 320)
    if (n, h, w) == (32, 20, 26):
        assert (p["blocks"], p["rect_blocks"]) == (70, 96)
    assert 1 <= p["strips"] <= 3 and p["pieces"] <= 14 and p["chunk_pieces"] <= 672, p
    assert p["admitted"] == 1 and p["taken"] == 1, p
    seen = {}
    expect = [(i, 2 * b + r, c) for i in range(n) for b in range(-(-ty // 2)) for c in range(tx) for r in range(min(2, ty - 2 * b))]
    for t in range(32 * p["blocks"]):
        img, r, c, k, piece = tile(lib, n, h, w, t)
        if t >= n * ty * tx:
            assert img == -1, (t, img)                       # an empty lane
            continue
        assert (img, r, c) == expect[t], (t, (img, r, c), expect[t])
        assert (img, r, c) not in seen
        seen[(img, r, c)] = (t >> 4, k, piece)
        assert 0 <= k < p["strips"] and 0 <= piece and piece + 3 <= p["pieces"], (t, k, piece)
    assert len(seen) == n * ty * tx
    # per group: a strip is one (image, band); its tiles share piece - column; strips occupy disjoint piece ranges
    groups = {}
    for (img, r, c), (g, k, piece) in seen.items():
        groups.setdefault(g, {}).setdefault(k, []).append((img, r // 2, c, piece))
    for g, strips in groups.items():
        spans = []
        for k, tiles in sorted(strips.items()):
            assert len({(i, b) for i, b, _, _ in tiles}) == 1, (g, k, tiles)
            assert len({piece - c for _, _, c, piece in tiles}) == 1, (g, k, tiles)
            cols = sorted({c for _, _, c, _ in tiles})
            assert cols == list(range(cols[0], cols[-1] + 1))                       # a run of whole columns
            lo = min(piece for *_, piece in tiles)
            spans.append((lo, lo + len(cols) + 2))
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a1 <= b0, (g, spans)
        assert spans[0][0] == 0 and spans[-1][1] <= 14, (g, spans)


def test_four_tiles_per_band_is_refused(lib, monkeypatch):
    monkeypatch.setenv("GSD_W2D_STRIPS", "1")
    p = plan(lib, 33, 4, 8)
    assert p["strips"] > 3 and p["admitted"] == 0 and p["taken"] == 0, p


def test_switch_and_default_rule(lib, monkeypatch):
    """0: never; 1: wherever admitted; unset: at the deep levels, where the run-time model (whole blocks per CU, two resident) has
    the shorter list finish sooner at 3 % more per chunk.  At batch 32 that is every deep launch but 40 x 53 512 -> 256 (1120
    blocks against 1280: five per CU either way; measured 2 % slower) and 20 x 26 1024 -> 512 (560 against 768: three either way);
    at 80 x 106 and above the rectangles stay."""
    monkeypatch.setenv("GSD_W2D_STRIPS", "0")
    assert plan(lib, 32, 40, 53)["taken"] == 0
    monkeypatch.delenv("GSD_W2D_STRIPS")
    for h, w, cin, cout, want in ((40, 53, 256, 512, 1), (40, 53, 512, 512, 1), (40, 53, 1024, 512, 1), (40, 53, 512, 1024, 1),
                                  (40, 53, 512, 256, 0), (20, 26, 512, 1024, 1), (20, 26, 1024, 1024, 1), (20, 26, 1024, 512, 0)):
        assert plan(lib, 32, h, w, cin, cout)["taken"] == want, (h, w, cin, cout)
    assert plan(lib, 8, 40, 53, 256, 512)["taken"] == 0 and plan(lib, 8, 40, 53, 512, 1024)["taken"] == 0
    for h, w, c in ((160, 213, 128), (80, 106, 256)):
        p = plan(lib, 32, h, w, c, c)
        assert p["admitted"] == 1 and p["blocks"] < p["rect_blocks"] and p["taken"] == 0, p
    monkeypatch.setenv("GSD_W2D_STRIPS", "1")
    assert plan(lib, 32, 160, 213, 128, 128)["taken"] == 1 and plan(lib, 32, 40, 53, 512, 256)["taken"] == 1


def test_host_counts_price_the_path_that_runs(lib, monkeypatch):
    """The executed-MFMA count of a class-1 launch follows the block count of the path taken; every other class keeps the rectangles'."""
    monkeypatch.delenv("GSD_W2D_STRIPS", raising=False)
    monkeypatch.setenv("GSD_W2D_SPLIT", "0")
    rect = lib.gsd_conv3x3_w2d_mfma_count(32, 40, 53, 512, 512)
    assert lib.gsd_conv3x3_w2d_mfma_count_class(32, 40, 53, 512, 512, 0, 1) == rect
    assert lib.gsd_conv3x3_w2d_mfma_count_class(32, 40, 53, 512, 512, 1, 1) * 320 == rect * 280
    assert lib.gsd_conv3x3_w2d_mfma_count_class(32, 20, 26, 1024, 1024, 1, 1) * 96 == lib.gsd_conv3x3_w2d_mfma_count(32, 20, 26, 1024, 1024) * 70
    monkeypatch.setenv("GSD_W2D_STRIPS", "0")
    assert lib.gsd_conv3x3_w2d_mfma_count_class(32, 40, 53, 512, 512, 1, 1) == rect


def test_scratch_query_follows_the_rule(lib, monkeypatch):
    """Per-tile statistics scratch: 32 tiles a block, two sums, the padded channel count -- where a launch takes the list, else 0."""
    monkeypatch.delenv("GSD_W2D_STRIPS", raising=False)
    assert lib.gsd_conv3x3_w2d_strips_scratch(32, 40, 53, 512, 512) == 280 * 32 * 2 * 512
    assert lib.gsd_conv3x3_w2d_strips_scratch(32, 20, 26, 512, 1024) == 70 * 32 * 2 * 1024
    assert lib.gsd_conv3x3_w2d_strips_scratch(32, 40, 53, 512, 256) == 0 and lib.gsd_conv3x3_w2d_strips_scratch(32, 160, 213, 128, 128) == 0
    monkeypatch.setenv("GSD_W2D_STRIPS", "0")
    assert lib.gsd_conv3x3_w2d_strips_scratch(32, 40, 53, 512, 512) == 0
