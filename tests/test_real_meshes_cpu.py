"""CPU: the real object meshes of tests/golden/meshes/ (tests/real_mesh_cases.py) through the package's STL reader, and the
preconditions of the fp64 yardsticks that tests/test_gpu_real_meshes.py holds the kernels to on them -- checked here, without a
GPU, so that a pose whose interval says too little, or whose Jacobian twin is too unsure, is named before a kernel runs.  Nothing
here launches a kernel.  The last test holds the exact definition to the restated reference on two real objects, as
test_mesh_depth_cpu does on the ellipsoid."""
import functools
import os

import numpy as np
import pytest

import mesh_depth_ref as R
import mesh_pose_refine_ref as PR
import real_mesh_cases as M

RECORD = np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")])


def raw_file(name):
    with open(os.path.join(M.MESH_DIR, name + ".stl"), "rb") as fh:
        return fh.read()


# ---- 1. the reader ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.NAMES)
def test_read_stl_on_the_fixture(name, tmp_path):
    from gelslim_depth_amd.mesh_depth import read_stl
    raw = raw_file(name)
    count = int(np.frombuffer(raw, "<u4", 1, 80)[0])
    tri = M.mesh(name)
    assert count == M.MESHES[name]["triangles"] and len(raw) == 84 + 50 * count
    assert tri.dtype == np.float32 and tri.shape == (count, 3, 3) and np.isfinite(tri).all()
    rec = np.frombuffer(raw, RECORD, count, 84)          # an independent parse of the same bytes
    assert np.array_equal(tri.view(np.uint32), np.ascontiguousarray(rec["v"]).view(np.uint32))
    # two of the forms of file the objects come in: an all-zero header, or 'STLB ...' with an attribute word in every record.  That
    # is what these six files hold, not a property of the format: the 80 bytes are free text (a third form among the objects, one
    # that begins 'Creat', is in no fixture), and read_stl looks at them only to tell a text file by its 'solid'.  The third form is
    # made here from the fixture's own records
    if name == "peg1":
        assert raw[:5] == b"STLB " and (rec["a"] != 0).all()
    else:
        assert not any(raw[:80]) and not rec["a"].any()
    third = str(tmp_path / "created.stl")
    with open(third, "wb") as fh:
        fh.write(b"Created by a CAD program".ljust(80, b" ") + raw[80:])
    assert np.array_equal(read_stl(third).view(np.uint32), tri.view(np.uint32))
    v = tri.reshape(-1, 3).astype(np.float64) * M.pc_scale(name)
    lo, hi = M.MESHES[name]["bbox"]
    assert np.abs(v.min(axis=0) - lo).max() <= 6e-4 and np.abs(v.max(axis=0) - hi).max() <= 6e-4, (v.min(axis=0), v.max(axis=0))
    assert np.allclose(M.centre_of(name), M.MESHES[name]["centre"], atol=1e-3)
    # through ASCII and back.  A writer of decimal text is free to round (a '%e' with nine digits does not always return the
    # float it was given), so the round trip is held to one fp32 ulp, not to the bits
    path = str(tmp_path / "ascii.stl")
    R.write_stl_ascii(path, tri)
    back = read_stl(path)
    assert back.dtype == np.float32 and back.shape == tri.shape
    assert np.all(np.abs(back.astype(np.float64) - tri) <= np.spacing(np.abs(tri))), name


# ---- 2. the yardsticks' preconditions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.NAMES)
def test_every_rendered_case_has_a_tight_interval_and_the_contact_it_is_there_for(name):
    """At most WIDE_CAP of an image's pixels may have hi - lo > WIDE_MM: an interval that wide admits nearly anything.  (a)..(d)
    have pixels that are in contact whatever the rounding (hi < 0), (d) also pixels that are not (lo = 0), (e) and the wide grasp
    are 0 everywhere."""
    worst = (-1.0, ())
    for plane, size, flip, invert, batch in M.launches(name):
        for label, pose, g in batch:
            lo, hi = M.interval(name, plane, pose, g, size, invert)
            share = M.wide_share(lo, hi)
            worst = max(worst, (share, (plane, size, label, invert)))
            assert share <= M.WIDE_CAP, (name, plane, size, label, invert, pose, share)
            assert np.all(lo <= hi) and np.all(hi <= 0)
            if label in "abcd":
                assert (hi < 0).any(), (name, plane, size, label, invert, pose)
            # (d) on the four plates is rendered with g = 0, a covered edge; the contact boundary at the working indentation is in
            # (a), (b), (c) of every mesh but the flat plate: the raised feature, or the peg, ends inside the image
            if label == "d" or (label in "abc" and plane == M.PLANE and name != "pattern_18_hex_1"):
                assert (lo == 0).any(), (name, plane, size, label, pose)
            if label in ("e", "wide"):
                assert not lo.any() and not hi.any(), (name, plane, size, label, pose)
    print(f"{name}: {len(M.launches(name))} launches, widest-interval share {worst[0]:.4f} at {worst[1]}")
    if name == "pattern_05_3_lines_angle_2":          # the same mesh reflected by pc_scale = -1000
        for size in M.SIZES:
            for label, pose, g in M.reflected_cases(name):
                lo, hi = M.interval(name, M.PLANE, pose, g, size, False, -1000.0)
                assert M.wide_share(lo, hi) <= M.WIDE_CAP and (hi < 0).any(), (name, size, label, pose)


def test_the_jacobian_twin_is_certain_about_nearly_every_active_point():
    """And every axis of J is alive in every image (largest |J| > J_MIN), but for the one exemption that real_mesh_cases.J_DEAD
    names: peg1 at (a), whose aligned axis is dead -- asserted too, so that the exemption cannot outlive its reason."""
    for entry in M.JACOBIANS:
        pose, g, t = M.twin_image(*entry)
        active = int(t["active"].sum())
        unsure = int((t["uncertain"] & t["active"]).sum())
        big = [float(np.abs(t["J"][:, k]).max()) for k in range(3)]
        print(f"{entry}: {active} active points, {unsure} of them uncertain ({100.0 * unsure / max(active, 1):.2f} %), largest |J| per axis {big}")
        assert active >= M.ACTIVE_MIN and unsure <= PR.UNCERTAIN_CAP * active, (entry, pose, active, unsure)
        assert M.live_axes(entry[0], entry[2], big), (entry, big)
        dead = M.J_DEAD.get((entry[0], entry[2]))
        assert dead is None or big[dead] <= M.J_MIN, (entry, big)
    assert {(e[0], e[2]) for e in M.JACOBIANS} >= set(M.J_DEAD)


def test_the_flat_plate_has_no_slope_under_any_pixel():
    G = M.twin_records("pattern_18_hex_1")
    _, pose, g = M.case("pattern_18_hex_1", "a")
    t = PR.point_terms(G, pose, np.float32(g), (24, 31))
    assert t["active"].all() and not t["J"].any()


# ---- 3. which triangles are skipped -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.NAMES)
def test_the_fp32_and_the_fp64_rule_skip_the_same_triangles(name):
    """The record skips a triangle whose fp32 doubled area (two rounded products of fp32 differences) is exactly 0, raster_ref one
    whose fp64 area is below 1e-12 of the product of two edge lengths.  They agree on four of the six files.  On the two others the
    fp32 rule skips a few walls more -- the table's `skip_differs`, walls that lean by 7e-8 .. 8e-7 mm --, and never one fewer.
    Each of those is thinner than delta (area < delta * longest edge, delta raster_ref's position uncertainty of 6e-5 mm): a
    triangle that thin has no interior once it is shrunk by delta, so raster_ref's lo never relies on it, and its hi only gains."""
    tri = M.mesh(name)
    skipped32 = M.twin_records(name)["rec"][:, 9] == 0
    a, b, _, _ = R.prepare(tri, M.pc_scale(name), M.PLANE)
    e1a, e1b, e2a, e2b = a[:, 1] - a[:, 0], b[:, 1] - b[:, 0], a[:, 2] - a[:, 0], b[:, 2] - b[:, 0]
    doubled = e1a * e2b - e1b * e2a
    skipped64 = ~(np.abs(doubled) > 1e-12 * np.hypot(e1a, e1b) * np.hypot(e2a, e2b))          # raster_ref's `keep`, restated
    differ = np.nonzero(skipped32 != skipped64)[0]
    kept = np.abs(doubled[~skipped64]) / 2
    print(f"{name}: {tri.shape[0]} triangles, the fp32 rule skips {int(skipped32.sum())}, the fp64 rule {int(skipped64.sum())}, they differ on "
          f"{differ.tolist()}; smallest kept area {kept.min():.3e} mm^2")
    delta = 16 * 2.0 ** -23 * max(np.abs(a).max(), np.abs(b).max())
    longest = np.maximum.reduce([np.hypot(e1a, e1b), np.hypot(e2a, e2b), np.hypot(e2a - e1a, e2b - e1b)])
    assert np.all(np.abs(doubled[differ]) / 2 < delta * longest[differ]), (name, differ)
    assert differ.tolist() == list(M.MESHES[name].get("skip_differs", ())), (name, differ)
    assert not (skipped64 & ~skipped32).any()
    assert skipped32.sum() >= 8          # the walls are there: 8 of 12 triangles even on the hexagonal plate


# ---- 4. the definition against the restated reference on real objects ---------------------------------------------------------------
# measured on the four cases below: worst mean |difference| (the marble's; the peg's is 0.000715) and worst
# max |difference| 2 px inside both patches (the marble's; the peg's is 0.016323)
REAL_WORST_MEAN_MM, REAL_WORST_INNER_MM = 0.001581, 0.022268
FACTOR = 3.0                 # another numpy build may draw another cloud
BAND_CAP = 0.25
# (mesh, image size, whether the 2 px band can remove at most BAND_CAP of the contact).  The marble at 24 x 31 cannot: 0.8 mm into
# its cap touches 91 pixels per finger, a disc of 5.4 px radius, and taking 2 px off the rim of any disc that small leaves at most
# (3.4 / 5.4)^2 = 40 % of it.  Its mean over the whole image does not depend on the band and is held as it stands, its inner
# maximum over the pixels that are left (there must be some); the peg at 40 x 53, a ridge 32 px wide, meets all four conditions
DEFINITION_CASES = (("marble", (24, 31), False), ("peg1", (40, 53), True))


@functools.lru_cache(maxsize=None)
def _real_pair(name, size, invert):
    """(raster_ref at delta = 0, the restated reference on 2e5 surface points) of pose (a), as test_mesh_depth_cpu._pair."""
    _, pose, g = M.case(name, "a")
    pose = M.inverted(pose) if invert else pose
    lo, hi = R.raster_ref(M.mesh(name), M.pc_scale(name), M.PLANE, pose, g, size, 12.0, False, invert, delta=0.0)
    assert np.array_equal(lo, hi)
    cloud = R.sample_surface(M.mesh(name).astype(np.float64) * M.pc_scale(name), 2e5, seed=0)
    return lo, R.reference_depth_image(cloud, M.PLANE, pose, g, size, 12.0, False, invert)


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("name,size,band_holds", DEFINITION_CASES, ids=[c[0] for c in DEFINITION_CASES])
def test_exact_definition_means_what_the_reference_computes_on_a_real_object(name, size, band_holds, invert):
    pytest.importorskip("scipy")
    ours, ref = _real_pair(name, size, invert)
    peak = float(-ref.min())
    assert 0.8 * M.INDENT_MM < peak < 1.1 * M.INDENT_MM and abs(-ours.min() - M.INDENT_MM) < 0.05
    diff = np.abs(ours - ref)
    mean = float(diff.mean())
    worst = kept = total = 0
    for ch in (0, 1):
        contact = (ours[ch] < 0) & (ref[ch] < 0)
        inner = R.erode(contact, 2)
        assert inner.any(), (name, ch)
        total += int(contact.sum())
        kept += int(inner.sum())
        worst = max(worst, float(diff[ch][inner].max()))
    print(f"{name} {size} invert={invert}: mean {mean:.6f} mm, inner max {worst:.6f} mm, band removes {1 - kept / total:.3f}, peak {peak:.4f} mm")
    # the two conditions under which the bounds mean anything
    assert FACTOR * REAL_WORST_MEAN_MM < 0.1 * peak and FACTOR * REAL_WORST_INNER_MM < 0.1 * peak
    assert (1 - kept / total <= BAND_CAP) == band_holds, (name, kept, total)
    assert mean <= FACTOR * REAL_WORST_MEAN_MM and worst <= FACTOR * REAL_WORST_INNER_MM
