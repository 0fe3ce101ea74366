"""CPU: the twin of gsd_contact_patches_* (tests/contact_patches_ref.py) against cases typed out by hand and, where it imports,
against scipy.ndimage.label; the fixed-point and key encodings; the argument refusals of `contact_patches` that need no device."""
import numpy as np
import pytest

import contact_patches_ref as P

ONE = 1 << 20
MASK = np.array([[1, 1, 0, 0, 1],
                 [0, 0, 0, 1, 0],
                 [1, 0, 0, 0, 0],
                 [0, 1, 0, 0, 1]], dtype=bool)
KEY_M1 = 0x407FFFFF << 32      # ord(-1.0f) = ~0xBF800000
KEY_M2 = 0x3FFFFFFF << 32      # ord(-2.0f) = ~0xC0000000


def depth_of(mask):
    return np.where(mask, np.float32(-1.0), np.float32(0.0)).astype(np.float32)


def test_labels_of_a_small_mask_are_the_ones_typed_out():
    l8, n8 = P.label_plane(MASK, 8)
    assert n8 == 4 and l8.dtype == np.int32
    assert l8.tolist() == [[1, 1, 0, 0, 2], [0, 0, 0, 2, 0], [3, 0, 0, 0, 0], [0, 3, 0, 0, 4]]
    l4, n4 = P.label_plane(MASK, 4)
    assert n4 == 6
    assert l4.tolist() == [[1, 1, 0, 0, 2], [0, 0, 0, 3, 0], [4, 0, 0, 0, 0], [0, 5, 0, 0, 6]]
    # min_area = 2: single pixels are dropped, the numbers close up
    l8, n8 = P.label_plane(MASK, 8, 2)
    assert n8 == 3 and l8.tolist() == [[1, 1, 0, 0, 2], [0, 0, 0, 2, 0], [3, 0, 0, 0, 0], [0, 3, 0, 0, 0]]
    l4, n4 = P.label_plane(MASK, 4, 2)
    assert n4 == 1 and l4.tolist() == [[1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]


def test_statistics_of_a_small_mask_are_the_ones_typed_out():
    depth = depth_of(MASK)
    depth[1, 3] = -2.0
    both = np.stack((depth, np.zeros_like(depth)))[None]
    labels, counts, stats = P.contact_patches(both, 0.0, 8, 1, 5)
    assert counts.tolist() == [[4, 0]] and stats.shape == (1, 2, 5, 12) and stats.dtype == np.int64
    assert stats[0, 0].tolist() == [
        # area r_min r_max k_min k_max  sum r  sum k  sum rr  sum kk  sum rk  sum dq      peak key
        [2, 0, 0, 0, 1, 0, 1, 0, 1, 0, -2 * ONE, KEY_M1 | 0],
        [2, 0, 1, 3, 4, 1, 7, 1, 25, 3, -3 * ONE, KEY_M2 | 8],
        [2, 2, 3, 0, 1, 5, 1, 13, 1, 3, -2 * ONE, KEY_M1 | 10],
        [1, 3, 3, 4, 4, 3, 4, 9, 16, 12, -1 * ONE, KEY_M1 | 19],
        [0] * 12]
    assert not stats[0, 1].any() and not labels[0, 1].any()
    # K = 2: the third and fourth patch keep their labels and are counted, but have no row
    labels2, counts2, stats2 = P.contact_patches(both, 0.0, 8, 1, 2)
    assert np.array_equal(labels2, labels) and counts2.tolist() == [[4, 0]] and np.array_equal(stats2[0, 0], stats[0, 0, :2])


def test_filter_of_a_small_mask_is_the_one_typed_out():
    depth = depth_of(MASK)
    depth[2, 2] = -0.0
    depth[3, 3] = np.nan
    both = np.stack((depth, depth))[None]
    labels, _, stats = P.contact_patches(both, 0.0, 8, 2, 4)
    out = P.filtered_depth(both, labels, stats)
    want = depth.copy()
    want[3, 4] = 0.0
    assert np.array_equal(out.view(np.uint32)[0, 0], want.view(np.uint32)) and np.array_equal(out.view(np.uint32)[0, 1], want.view(np.uint32))
    # three patches of two pixels: the largest is the first, the two largest the first two
    for n, gone in ((1, [(0, 4), (1, 3), (2, 0), (3, 1), (3, 4)]), (2, [(2, 0), (3, 1), (3, 4)])):
        out = P.filtered_depth(both, labels, stats, keep_largest=n)
        want = depth.copy()
        for r, k in gone:
            want[r, k] = 0.0
        assert np.array_equal(out.view(np.uint32)[0, 0], want.view(np.uint32)), n
    # K = 1 under keep_largest: patches numbered above K are never kept
    labels, _, stats = P.contact_patches(both, 0.0, 8, 2, 1)
    out = P.filtered_depth(both, labels, stats, keep_largest=3)
    want = depth.copy()
    for r, k in [(0, 4), (1, 3), (2, 0), (3, 1), (3, 4)]:
        want[r, k] = 0.0
    assert np.array_equal(out.view(np.uint32)[0, 0], want.view(np.uint32))


def test_threshold_nan_and_infinity():
    c = np.float32(0.25)
    row = np.array([-0.25, np.nextafter(np.float32(-0.25), np.float32(-1)), np.nextafter(np.float32(-0.25), np.float32(0)),
                    np.nan, -np.inf, 0.0, -0.0, 1.0], dtype=np.float32)
    assert P.contact_mask(row, c).tolist() == [False, True, False, False, True, False, False, False]
    assert P.contact_mask(np.array([-0.0, 0.0, -1e-45], dtype=np.float32), 0.0).tolist() == [False, False, True]


def test_twin_numbers_patches_as_scipy_does():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(20)
    for trial in range(60):
        h, w = int(rng.integers(1, 20)), int(rng.integers(1, 24))
        mask = rng.random((h, w)) < (0.2, 0.45, 0.6, 0.8)[trial % 4]
        for conn, structure in ((4, None), (8, np.ones((3, 3)))):
            want, n = ndi.label(mask, structure=structure)
            got, m = P.label_plane(mask, conn, 1)
            assert m == n and np.array_equal(got, want), (trial, conn)


def test_ord_is_monotone_and_round_trips():
    tiny = np.float32(1e-45)
    vals = np.array([-np.inf, -3.0e38, -1024.0, -1.0, -1.0, -1.1754944e-38, -tiny, -tiny, -0.0, 0.0, tiny, 1.1754944e-38, 1.0, 1.0, 3.0e38,
                     np.inf], dtype=np.float32)
    assert np.all(np.diff(vals) >= 0)
    o = [P.ord32(v) for v in vals]
    for a, b, x, y in zip(o, o[1:], vals, vals[1:]):
        assert 0 <= a < 1 << 32
        if x.tobytes() == y.tobytes():
            assert a == b
        else:
            assert a < b, (x, y)       # -0.0 sorts below +0.0: the bits differ, the order of the values is kept
    for v, a in zip(vals, o):
        assert P.ord32_inverse(a).tobytes() == v.tobytes()
    # the key: depth first, then the raster index; a contact pixel's key fits an int64
    assert P.peak_key(np.float32(-2.0), 100) < P.peak_key(np.float32(-1.0), 0) < P.peak_key(np.float32(-1.0), 1)
    assert P.peak_key(-np.inf, (1 << 31) - 1) < P.peak_key(np.float32(-3.0e38), 0)
    assert P.peak_key(np.float32(-1e-45), (1 << 31) - 1) < 1 << 63
    key = P.peak_key(np.float32(-0.75), 4711)
    assert P.ord32_inverse(key >> 32) == np.float32(-0.75) and key & 0xFFFFFFFF == 4711


def test_dq_is_exact_rounds_half_to_even_and_clamps():
    assert P.dq(-1.0) == -ONE and P.dq(0.0) == 0 and P.dq(-0.5) == -ONE // 2
    assert P.dq(-np.inf) == -1024 * ONE and P.dq(-2000.0) == -1024 * ONE and P.dq(-1024.0) == -1024 * ONE
    assert P.dq(np.nextafter(np.float32(-1024.0), np.float32(0))) == -1024 * ONE + 64      # one fp32 ulp at 1024 is 2^-14
    # ties: d 2^20 = n + 1/2 exactly
    for n, want in ((0, 0), (1, 2), (2, 2), (3, 4)):
        d = np.float32(-(n + 0.5) / ONE)
        assert float(d) * ONE == -(n + 0.5)
        assert P.dq(d) == -want, n
    # every fp32 below 2^-20 in magnitude times 2^20 is exact in fp64: dq of a denormal is 0
    assert P.dq(np.float32(-1e-45)) == 0
    # the sum over a full-size call fits an int64
    assert 1024 * ONE * ((1 << 31) - 1) < 1 << 63


def test_derived_properties_of_a_rectangle():
    mask = np.zeros((12, 20), dtype=bool)
    mask[2:6, 3:13] = True                       # 4 rows x 10 columns
    depth = depth_of(mask) * np.float32(0.5)
    _, _, stats = P.contact_patches(np.stack((depth, depth))[None], 0.0, 8, 1, 2)
    d = P.derived(stats, (12, 20), 12.0)         # 1 mm per pixel
    assert d["area_mm2"][0, 0].tolist()[0] == 40.0 and np.isnan(d["area_mm2"][0, 0, 1])
    assert d["centroid_mm"][0, 0, 0].tolist() == [3.5 - 6.0, 7.5 - 10.0]
    assert d["axis_angle"][0, 0, 0] == np.pi / 2          # the long side runs along the columns
    np.testing.assert_allclose(d["axis_lengths_mm"][0, 0, 0], [np.sqrt(99 / 12), np.sqrt(15 / 12)], rtol=1e-14)
    assert d["volume_mm3"][0, 0, 0] == 20.0 and d["mean_depth"][0, 0, 0] == -0.5 and d["peak_depth"][0, 0, 0] == np.float32(-0.5)
    assert d["peak_rc"][0, 0].tolist() == [[2, 3], [-1, -1]] and d["bbox"][0, 0].tolist() == [[2, 5, 3, 12], [-1, -1, -1, -1]]


def test_contact_patches_refuses_bad_arguments_without_a_device():
    import torch
    from gelslim_depth_amd.contact_patches import contact_patches
    from gelslim_depth_amd.mesh_depth import MeshDepthError
    host = torch.zeros(1, 2, 4, 5)
    for bad in (dict(connectivity=6), dict(connectivity=True), dict(connectivity="8"), dict(min_area=0), dict(min_area=1.5),
                dict(max_patches=0), dict(max_patches=True), dict(max_patches=1 << 31), dict(contact_depth=-0.1),
                dict(contact_depth=float("nan")), dict(contact_depth=float("inf"))):
        with pytest.raises(MeshDepthError, match="contact_patches: " + next(iter(bad)).split("_")[0]):
            contact_patches(host, **bad)
    with pytest.raises(MeshDepthError, match="must be a float32 .* tensor on the GPU"):
        contact_patches(host)
    with pytest.raises(MeshDepthError, match="must be a float32 .* tensor on the GPU"):
        contact_patches(host.numpy())
    with pytest.raises(MeshDepthError, match="must be a float32 .* tensor on the GPU"):
        contact_patches(host.double())


def test_library_refuses_before_any_launch():
    """The C entry points on null device pointers (no GPU is touched): every refusal comes before a launch."""
    import ctypes as C
    from gelslim_depth_amd import _lib as L
    lib = L.lib
    assert lib.gsd_contact_patches_workspace(1, 4, 5) == 2 * 4 * 5 + 2 and lib.gsd_contact_patches_workspace(64, 320, 427) > 0
    assert lib.gsd_contact_patches_workspace(0, 4, 5) == 0 and lib.gsd_contact_patches_workspace(1, 0, 5) == 0
    assert lib.gsd_contact_patches_workspace(1 << 10, 1 << 10, 1 << 10) == 0       # 2 B H W = 2^31
    assert lib.gsd_contact_patches_workspace(1, 1, (1 << 30) - 1) > 0
    view = L.gsd_contact_patches_view()
    view.contact_depth, view.connectivity, view.min_area = 0.0, 8, 1
    fake = 1 << 12      # a non-null address that is never dereferenced: each call is refused first
    assert lib.gsd_contact_patches_label(C.byref(view), fake, 1, 4, 5, fake, fake, fake, 41, None) == L.GSD_ERR_WORKSPACE
    assert lib.gsd_contact_patches_label(C.byref(view), None, 1, 4, 5, fake, fake, fake, 42, None) == L.GSD_ERR_BAD_ARG
    assert lib.gsd_contact_patches_label(C.byref(view), fake, 1 << 10, 1 << 10, 1 << 10, fake, fake, fake, 1 << 40, None) == L.GSD_ERR_BAD_ARG
    assert lib.gsd_contact_patches_stats(C.byref(view), fake, fake, 1, 4, 5, 0, fake, None) == L.GSD_ERR_BAD_ARG
    assert lib.gsd_contact_patches_filter(C.byref(view), fake, fake, None, 1, 4, 5, 0, fake, None) == L.GSD_ERR_BAD_ARG
    for field, value in (("connectivity", 6), ("min_area", 0), ("contact_depth", -1.0), ("contact_depth", float("nan"))):
        v = L.gsd_contact_patches_view()
        v.contact_depth, v.connectivity, v.min_area = 0.0, 4, 1
        setattr(v, field, value)
        assert lib.gsd_contact_patches_label(C.byref(v), fake, 1, 4, 5, fake, fake, fake, 42, None) == L.GSD_ERR_BAD_ARG, field
        assert lib.gsd_contact_patches_stats(C.byref(v), fake, fake, 1, 4, 5, 4, fake, None) == L.GSD_ERR_BAD_ARG, field
        assert lib.gsd_contact_patches_filter(C.byref(v), fake, fake, None, 1, 4, 5, 4, fake, None) == L.GSD_ERR_BAD_ARG, field
    assert C.sizeof(L.gsd_contact_patches_view) == 16 and L.gsd_contact_patches_view.connectivity.offset == 8
    assert L.GSD_CONTACT_PATCHES_SEG == 64 and L.GSD_CONTACT_PATCHES_COLS == P.COLS == 12      # include/gsd.h's


def test_contact_patches_kernels_use_no_scratch():
    """gsd_contact_patches.hip at build.py's flags: eleven kernels, none with scratch (device-only compile, a few seconds)."""
    import os
    import re
    import shutil
    import subprocess
    from gelslim_depth_amd import build as b
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this machine")
    r = subprocess.run([hipcc] + b.CFLAGS + [f"-I{b.INCLUDE}", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(b.CSRC, "gsd_contact_patches.hip"), "-o", os.devnull], capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    kernels = {n: s for n, s in zip(names, scratch) if "patches_" in n}
    assert len(kernels) == 11 and len(names) == len(scratch), r.stderr[-2000:]
    assert all(v == 0 for v in kernels.values()), kernels
