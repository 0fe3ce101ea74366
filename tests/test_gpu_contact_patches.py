"""GPU: gsd_contact_patches_* (gelslim_depth_amd.contact_patches) against the CPU twin of DESIGN.md section 22
(tests/contact_patches_ref.py).

labels, counts, stats and filtered_depth are integers or bit copies: they must be EQUAL to the twin's.  Every derived property
must lie within 4 fp64 ulps of the same formula in numpy on the twin's integers (a handful of correctly rounded operations; atan2
and sqrt may differ in the last bit between torch and numpy).  Masks are built on the host; depth is -1.0 where the mask is set
and +0.0 elsewhere unless a test says otherwise.  The kernel cuts rows into segments of 64 columns (GSD_CONTACT_PATCHES_SEG):
sizes of 63, 64 and 65 stand on either side of that edge."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import contact_patches_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEG = 64
HEIGHT_MM = 12.0
FLOAT_PROPS = ("area_mm2", "centroid_mm", "axis_angle", "axis_lengths_mm", "volume_mm3", "mean_depth")


def depth_of(*masks):
    """(B, 2, H, W) fp32 from 2 B masks: -1.0 where set, +0.0 elsewhere."""
    planes = [np.where(np.asarray(m, dtype=bool), np.float32(-1.0), np.float32(0.0)).astype(np.float32) for m in masks]
    return np.stack(planes).reshape(len(planes) // 2, 2, *planes[0].shape)


def assert_ulps(got, want, what, ulps=4.0):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
    worst = float((err / np.spacing(np.abs(want[ok])).astype(np.float64)).max())
    print(f"{what}: worst {worst:.2f} ulp")
    assert worst <= ulps, (what, worst)
    return worst


def check(depth, contact_depth=0.0, connectivity=8, min_area=1, max_patches=64, keep=(None,)):
    """contact_patches on the device against the twin: labels, counts, stats equal, the properties within 4 ulps, filtered_depth
    equal bit for bit for every keep_largest in `keep`.  Returns (ContactPatches, the twin's (labels, counts, stats))."""
    from gelslim_depth_amd.contact_patches import contact_patches
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    on = torch.from_numpy(depth).to(DEV)
    got = contact_patches(on, contact_depth, connectivity, min_area, max_patches, HEIGHT_MM)
    labels, counts, stats = P.contact_patches(depth, contact_depth, connectivity, min_area, max_patches)
    assert got.labels.dtype == torch.int32 and got.counts.dtype == torch.int32 and got.stats.dtype == torch.int64
    assert got.stats.shape == stats.shape
    g_labels, g_counts, g_stats = got.labels.cpu().numpy(), got.counts.cpu().numpy(), got.stats.cpu().numpy()
    assert np.array_equal(g_counts, counts), (g_counts.tolist(), counts.tolist())
    assert np.array_equal(g_labels, labels), ("labels differ at", np.argwhere(g_labels != labels)[:8].tolist())
    assert np.array_equal(g_stats, stats), ("stats differ at", np.argwhere(g_stats != stats)[:8].tolist())
    want = P.derived(stats, depth.shape[2:], HEIGHT_MM)
    for name in FLOAT_PROPS:
        assert_ulps(getattr(got, name).cpu().numpy(), want[name], name)
    peak = got.peak_depth.cpu().numpy()
    assert peak.dtype == np.float32 and np.array_equal(peak.view(np.uint32)[stats[..., 0] > 0], want["peak_depth"].view(np.uint32)[stats[..., 0] > 0])
    assert np.array_equal(np.isnan(peak), stats[..., 0] == 0)
    assert np.array_equal(got.peak_rc.cpu().numpy(), want["peak_rc"]) and np.array_equal(got.bbox.cpu().numpy(), want["bbox"])
    for n in keep:
        out = got.filtered_depth(on, keep_largest=n).cpu().numpy()
        ref = P.filtered_depth(depth, labels, stats, contact_depth, n)
        assert np.array_equal(out.view(np.int32), ref.view(np.int32)), ("filtered_depth", n)
    return got, (labels, counts, stats)


# ---- degenerate sizes and planes ------------------------------------------------------------------------------------------
def test_degenerate_sizes():
    for conn in (4, 8):
        _, (_, counts, _) = check(depth_of([[1]], [[0]], [[0]], [[1]]), connectivity=conn)
        assert counts.tolist() == [[1, 0], [0, 1]]
        rng = np.random.default_rng(3)
        line = rng.random(37) < 0.5
        check(depth_of(line[None], np.ones((1, 37)), np.zeros((1, 37)), ~line[None]), connectivity=conn)
        _, (_, counts, _) = check(depth_of(line[:, None], np.ones((37, 1)), np.zeros((37, 1)), ~line[:, None]), connectivity=conn)
        assert counts[0, 1] == 1 and counts[1, 0] == 0


def test_empty_full_and_corner_planes():
    corners = np.zeros((24, 31), dtype=bool)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = True
    for conn in (4, 8):
        got, (labels, counts, stats) = check(depth_of(np.zeros((24, 31)), np.ones((24, 31)), corners, corners[::-1]), connectivity=conn)
        assert counts.tolist() == [[0, 1], [4, 4]] and stats[0, 1, 0, 0] == 744 and not stats[0, 0].any()
        assert labels[1, 0, 0, 0] == 1 and labels[1, 0, 0, -1] == 2 and labels[1, 0, -1, 0] == 3 and labels[1, 0, -1, -1] == 4


def test_checkerboard():
    r, k = np.mgrid[0:24, 0:31]
    board = (r + k) % 2 == 0
    _, (_, counts, stats) = check(depth_of(board, ~board), connectivity=8)
    assert counts.tolist() == [[1, 1]] and stats[0, 0, 0, 0] == 372 and stats[0, 1, 0, 0] == 372
    got, (labels, counts, stats) = check(depth_of(board, ~board), connectivity=4, max_patches=64)
    assert counts.tolist() == [[372, 372]] and labels.max() == 372 and (stats[..., 0] == 1).all() and stats.shape[2] == 64
    _, (labels, counts, stats) = check(depth_of(board, ~board), connectivity=4, min_area=2)
    assert counts.tolist() == [[0, 0]] and not labels.any() and not stats.any()


def test_diagonals():
    main = np.eye(70, 130, dtype=bool)
    anti = main[:, ::-1]
    _, (_, counts, _) = check(depth_of(main, anti, main[::-1], np.eye(70, 130, 60, dtype=bool)), connectivity=8)
    assert counts.tolist() == [[1, 1], [1, 1]]
    _, (_, counts, _) = check(depth_of(main, anti), connectivity=4, max_patches=8)
    assert counts.tolist() == [[70, 70]]


# ---- long paths -----------------------------------------------------------------------------------------------------------
def serpentine(h, w):
    m = np.zeros((h, w), dtype=bool)
    m[0::2] = True
    for r in range(1, h, 2):
        m[r, w - 1 if (r // 2) % 2 == 0 else 0] = True
    return m


def spiral(n):
    m = np.zeros((n, n), dtype=bool)
    r = k = 0
    dr, dk = 0, 1
    m[0, 0] = True

    def free(r, k, dr, dk):
        nr, nk, ar, ak = r + dr, k + dk, r + 2 * dr, k + 2 * dk
        return 0 <= nr < n and 0 <= nk < n and not m[nr, nk] and not (0 <= ar < n and 0 <= ak < n and m[ar, ak])
    for _ in range(n * n):
        if not free(r, k, dr, dk):
            dr, dk = dk, -dr
            if not free(r, k, dr, dk):
                break
        r, k = r + dr, k + dk
        m[r, k] = True
    return m


def comb(h, w):
    m = np.zeros((h, w), dtype=bool)
    m[:, 0::2] = True
    m[-1] = True
    return m


def rings(h, w):
    r, k = np.mgrid[0:h, 0:w]
    return np.minimum(np.minimum(r, k), np.minimum(h - 1 - r, w - 1 - k)) % 2 == 0


@pytest.mark.parametrize("conn", (4, 8))
def test_serpentine_full_size(conn):
    """One patch whose only path is 68,480 pixels long: no fixed number of propagation sweeps reaches its end."""
    m = serpentine(320, 427)
    assert m.sum() == 68480
    _, (_, counts, stats) = check(depth_of(m, m[::-1, ::-1]), connectivity=conn, max_patches=2)
    assert counts.tolist() == [[1, 1]] and stats[0, :, 0, 0].tolist() == [68480, 68480]


@pytest.mark.parametrize("conn", (4, 8))
def test_serpentine_spiral_comb_and_rings(conn):
    _, (_, counts, _) = check(depth_of(serpentine(40, 53), serpentine(40, 53)[::-1], comb(40, 53), comb(40, 53)[:, ::-1]), connectivity=conn)
    assert counts.tolist() == [[1, 1], [1, 1]]
    s = spiral(70)
    assert s.sum() > 70 * 70 // 2 - 70
    _, (_, counts, _) = check(depth_of(s, s.T, s[::-1], s[:, ::-1]), connectivity=conn)
    assert counts.tolist() == [[1, 1], [1, 1]]
    _, (_, counts, _) = check(depth_of(rings(40, 53), rings(65, 130)[:40, :53], comb(40, 53)[::-1], ~rings(40, 53)), connectivity=conn)
    assert counts[0, 0] == 10


# ---- random masks ---------------------------------------------------------------------------------------------------------
SIZES = [(24, 31), (40, 53), (33, 65), (64, 64), (65, 129), (70, 130), (SEG - 1, SEG + 1), (SEG, SEG - 1), (SEG + 1, SEG), (5, 2 * SEG - 1),
         (5, 2 * SEG), (5, 2 * SEG + 1)]


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_masks(size, conn):
    """B = 3, the four densities over the planes; image 2's right channel is image 0's left one: planes never connect."""
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    m = [rng.random(size) < p for p in (0.2, 0.45, 0.6, 0.8, 0.45)]
    _, (labels, counts, _) = check(depth_of(m[0], m[1], m[2], m[3], m[4], m[0]), connectivity=conn, max_patches=48)
    assert np.array_equal(labels[2, 1], labels[0, 0]) and counts[2, 1] == counts[0, 0]


# ---- threshold, NaN, infinity, equal minima -----------------------------------------------------------------------------
def test_threshold_nan_infinity_and_equal_minima():
    c = np.float32(0.25)
    below, above = np.nextafter(-c, np.float32(-1)), np.nextafter(-c, np.float32(0))
    d = np.zeros((2, 2, 9, 11), dtype=np.float32)
    d[0, 0, 1:5, 1:6] = -1.0
    d[0, 0, 2, 2] = -c            # not contact: a hole
    d[0, 0, 2, 4] = above         # not contact
    d[0, 0, 3, 3] = np.nan        # not contact, inside the patch
    d[0, 0, 1, 6] = np.nan        # beside it
    d[0, 0, 5, 1] = below         # contact, joins from below
    d[0, 0, 7, 8:11] = (below, -c, below)      # two single pixels
    d[0, 1, 2:6, 3:9] = -0.5
    d[0, 1, 3, 5] = -np.inf       # contact: clamps in dq, wins the peak
    d[0, 1, 4, 4] = -3.0e38
    d[1, 0, 1:4, 1:8] = -1.0
    d[1, 0, 2, 5] = d[1, 0, 1, 6] = d[1, 0, 3, 2] = -2.0      # equal minima: the first in raster order is (1, 6)
    d[1, 1] = np.nan
    d[1, 1, 4, 4:7] = (-0.2500001, -0.25, -0.26)
    for conn in (4, 8):
        got, (labels, counts, stats) = check(d, contact_depth=0.25, connectivity=conn, max_patches=4)
        assert counts.tolist() == [[3, 1], [1, 2]]
        assert labels[0, 0, 2, 2] == 0 and labels[0, 0, 2, 4] == 0 and labels[0, 0, 3, 3] == 0 and labels[0, 0, 5, 1] == 1
        assert stats[0, 1, 0, 0] == 24 and stats[0, 1, 0, 10] == -((22 << 19) + (2 << 30))
        assert got.peak_depth[0, 1, 0].item() == -np.inf and got.peak_rc[0, 1, 0].tolist() == [3, 5]
        assert got.peak_depth[1, 0, 0].item() == -2.0 and got.peak_rc[1, 0, 0].tolist() == [1, 6]


# ---- min_area and numbering -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", (4, 8))
def test_min_area_drops_patches_and_the_numbering_closes_up(conn):
    rng = np.random.default_rng(50)
    a, b = rng.random((64, 64)) < 0.45, rng.random((64, 64)) < 0.6
    seen = []
    for min_area in (1, 2, 50):
        _, (labels, counts, stats) = check(depth_of(a, b), connectivity=conn, min_area=min_area, max_patches=16)
        for ch in range(2):
            assert sorted(set(labels[0, ch].ravel().tolist()) - {0}) == list(range(1, counts[0, ch] + 1))
        assert (stats[..., 0][stats[..., 0] > 0] >= min_area).all()
        seen.append(counts.copy())
    assert (seen[0] > seen[1]).all() and (seen[1] > seen[2]).all() and (seen[2] >= 1).all()


# ---- buffers and batches --------------------------------------------------------------------------------------------------
def random_depth(rng, b, h, w, density=0.5):
    """contact pixels with random depths in (-2, 0), a background of +0.0, -0.0, small positives and NaNs with payloads"""
    d = np.where(rng.random((b, 2, h, w)) < density, -rng.random((b, 2, h, w)) * 2 - 1e-3, 0.0).astype(np.float32)
    back = d == 0
    pick = rng.random(d.shape)
    d[back & (pick < 0.1)] = -0.0
    d[back & (pick > 0.9)] = 0.125
    bits = d.view(np.uint32)
    bits[back & (pick > 0.45) & (pick < 0.5)] = 0x7FC12345
    bits[back & (pick > 0.5) & (pick < 0.55)] = 0xFFC00001
    return d


def raw_call(depth, conn, min_area, k, fill):
    """The C entry points on buffers pre-filled with the byte `fill`: labels, counts, stats, and what the workspace was left as."""
    from gelslim_depth_amd import _lib as L
    b, _, h, w = depth.shape
    view = L.gsd_contact_patches_view()
    view.contact_depth, view.connectivity, view.min_area = 0.0, conn, min_area
    words = int(L.lib.gsd_contact_patches_workspace(b, h, w))
    word = int.from_bytes(bytes([fill]) * 4, "little", signed=True)
    ws = torch.full((words + 8,), word, device=DEV, dtype=torch.int32)
    labels = torch.full((b, 2, h, w), word, device=DEV, dtype=torch.int32)
    counts = torch.full((b, 2), word, device=DEV, dtype=torch.int32)
    stats = torch.full((b, 2, k, 12), int.from_bytes(bytes([fill]) * 8, "little", signed=True), device=DEV, dtype=torch.int64)
    L.check(L.lib.gsd_contact_patches_label(C.byref(view), depth.data_ptr(), b, h, w, labels.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                            words, L.stream_ptr()), "label")
    L.check(L.lib.gsd_contact_patches_stats(C.byref(view), depth.data_ptr(), labels.data_ptr(), b, h, w, k, stats.data_ptr(),
                                            L.stream_ptr()), "stats")
    torch.cuda.synchronize()
    assert (ws[words:] == word).all(), "the label call wrote past its workspace"
    return labels.cpu().numpy(), counts.cpu().numpy(), stats.cpu().numpy()


def test_recycled_buffers_and_repeated_runs_give_the_same_bits():
    rng = np.random.default_rng(7)
    depth = random_depth(rng, 2, 40, 53)
    on = torch.from_numpy(depth).to(DEV)
    want = P.contact_patches(depth, 0.0, 8, 2, 8)
    first = raw_call(on, 8, 2, 8, 0x7F)
    for other in (raw_call(on, 8, 2, 8, 0x7F), raw_call(on, 8, 2, 8, 0x00), raw_call(on, 8, 2, 8, 0xFF)):
        for a, b in zip(first, other):
            assert np.array_equal(a, b)
    for a, b in zip(first, want):
        assert np.array_equal(a, b)


def test_an_image_does_not_depend_on_its_batch():
    from gelslim_depth_amd.contact_patches import contact_patches
    rng = np.random.default_rng(11)
    depth = random_depth(rng, 5, 40, 53, 0.55)
    got, _ = check(depth, connectivity=8, min_area=3, max_patches=12, keep=(None, 2))
    for b in (0, 3, 4):
        alone = contact_patches(torch.from_numpy(depth[b:b + 1]).to(DEV), 0.0, 8, 3, 12, HEIGHT_MM)
        assert torch.equal(alone.labels[0], got.labels[b]) and torch.equal(alone.counts[0], got.counts[b])
        assert torch.equal(alone.stats[0], got.stats[b])


# ---- filtering ------------------------------------------------------------------------------------------------------------
def test_filtered_depth_keeps_every_other_bit_and_ranks_equal_areas_by_number():
    rng = np.random.default_rng(13)
    depth = random_depth(rng, 2, 33, 65, 0.4)
    for conn in (4, 8):
        check(depth, connectivity=conn, min_area=4, max_patches=6, keep=(None, 1, 2, 6, 100))
    # equal areas: four 2 x 3 blocks and a larger one; keep_largest = 1 keeps the large one, 2 adds the FIRST small one
    m = np.zeros((24, 31), dtype=bool)
    for r, k in ((1, 1), (1, 20), (10, 5), (18, 24)):
        m[r:r + 2, k:k + 3] = True
    m[12:16, 14:19] = True
    d = depth_of(m, m[::-1])
    got, (labels, _, stats) = check(d, keep=(None, 1, 2, 3), max_patches=8)
    assert stats[0, 0, :5, 0].tolist() == [6, 6, 6, 20, 6]
    out = got.filtered_depth(torch.from_numpy(d).to(DEV), keep_largest=2).cpu().numpy()
    assert sorted(set(labels[0, 0][out[0, 0] < 0].tolist())) == [1, 4]


def test_no_host_read_anywhere():
    """contact_patches, filtered_depth and the properties under torch's sync debug mode: a host read would raise."""
    from gelslim_depth_amd.contact_patches import contact_patches
    rng = np.random.default_rng(17)
    on = torch.from_numpy(random_depth(rng, 2, 24, 31)).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = contact_patches(on, 0.0, 8, 2, 8, HEIGHT_MM)
        kept = got.filtered_depth(on), got.filtered_depth(on, keep_largest=2)
        props = [getattr(got, n) for n in FLOAT_PROPS + ("peak_depth", "peak_rc", "bbox")]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(kept) == 2 and len(props) == 9 and got.labels.shape == on.shape


# ---- end to end -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rendered(size):
    """A clean render of mesh_depth_ref's ellipsoid, two poses, as test_gpu_depth_points makes it."""
    import mesh_depth_ref as R
    from gelslim_depth_amd.mesh_depth import MeshGrid, render_depth
    tri = R.ellipsoid(2, (3.0, 2.5, 3.5), 0.12, (1.5, 0.75, -0.5))
    _, _, q, _ = R.prepare(tri, 1.0, "+y+z")
    poses = torch.tensor([(1.1e-3, -0.7e-3, 0.4), (-0.6e-3, 0.9e-3, -1.3)], dtype=torch.float32, device=DEV)
    widths = torch.tensor([2 * (float(q.max()) - 0.8), 2 * (float(q.max()) - 0.5)], dtype=torch.float32, device=DEV)
    return render_depth(MeshGrid(tri, 1.0, "+y+z", DEV), poses, widths, size, HEIGHT_MM)


def speckled(clean, rng, tries=40):
    """`clean` with seeded speckles of 1-3 pixels at -0.05 mm: each at least two pixels away from every contact pixel and from
    every other speckle, and only on pixels that are +0.0 in the clean image."""
    noisy = clean.copy()
    shapes = ([(0, 0)], [(0, 0), (0, 1)], [(0, 0), (1, 0), (1, 1)])
    b, _, h, w = clean.shape
    placed = 0
    for i in range(b):
        for ch in range(2):
            busy = clean[i, ch] < 0
            for t in range(tries):
                r, k = int(rng.integers(0, h - 1)), int(rng.integers(0, w - 1))
                cells = [(r + dr, k + dk) for dr, dk in shapes[t % 3]]
                near = busy[max(r - 2, 0):r + 4, max(k - 2, 0):k + 4]
                if near.any() or any(clean[i, ch, pr, pk].view(np.uint32) != 0 for pr, pk in cells):
                    continue
                for pr, pk in cells:
                    noisy[i, ch, pr, pk] = -0.05
                    busy[pr, pk] = True
                placed += 1
    return noisy, placed


@pytest.mark.parametrize("size", ((40, 53), (24, 31)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_despeckled_render_feeds_depth_points_as_the_clean_one_does(size):
    from gelslim_depth_amd.contact_patches import contact_patches
    from gelslim_depth_amd.contact_points import depth_points
    clean_on = rendered(size)
    clean = clean_on.cpu().numpy()
    _, _, clean_stats = P.contact_patches(clean, 0.0, 8, 1, 16)
    areas = clean_stats[..., 0]
    assert (areas[areas > 0] >= 4).all() and (areas.sum(axis=(1, 2)) > 0).all(), "every rendered patch outlives min_area = 4"
    noisy, placed = speckled(clean, np.random.default_rng(size[0]))
    assert placed >= 8 and not np.array_equal(noisy, clean)
    noisy_on = torch.from_numpy(noisy).to(DEV)
    out = contact_patches(noisy_on, min_area=4, image_height_mm=HEIGHT_MM).filtered_depth(noisy_on)
    assert torch.equal(out.view(torch.int32), clean_on.view(torch.int32))
    a, b = depth_points(out, frame="sensor", image_height_mm=HEIGHT_MM), depth_points(clean_on, frame="sensor", image_height_mm=HEIGHT_MM)
    assert torch.equal(a.points, b.points) and torch.equal(a.normals, b.normals) and torch.equal(a.pixel, b.pixel)
    assert torch.equal(a.counts, b.counts) and int(a.counts.sum()) > 0
    worse = depth_points(noisy_on, frame="sensor", image_height_mm=HEIGHT_MM)
    assert int(worse.counts.sum()) > int(b.counts.sum())
