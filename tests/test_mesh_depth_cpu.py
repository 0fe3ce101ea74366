"""CPU: the host side of gelslim_depth_amd.mesh_depth (STL reader, plane conventions, file and width rules), and the MEANING of
the exact definition pinned to the reference's sampled one: tests/mesh_depth_ref.py's raster_ref against its restatement of
depth_from_mesh.py on a point cloud.  Nothing here launches a kernel.  The 48 pinned cases share 24 reference runs of about
five seconds each, nearly all of it scipy's Delaunay triangulation of the 2e5-point cloud."""
import functools
import itertools
import math

import numpy as np
import pytest

import mesh_depth_ref as R


def test_read_stl_round_trips_both_flavours_and_refuses_malformed_files(tmp_path):
    from gelslim_depth_amd.mesh_depth import MeshDepthError, read_stl
    from gelslim_depth_amd._lib import GsdError
    tri = R.torus(nu=7, nv=5, centre=(1.25, -3.5, 0.1))
    b, a = str(tmp_path / "b.stl"), str(tmp_path / "a.stl")
    R.write_stl_binary(b, tri)
    R.write_stl_ascii(a, tri)
    for path in (b, a):
        got = read_stl(path)
        assert got.dtype == np.float32 and got.shape == tri.shape and np.array_equal(got, tri), path
    # a binary file whose header starts with "solid" is still binary
    s = str(tmp_path / "s.stl")
    R.write_stl_binary(s, tri, header=b"solid but binary")
    assert np.array_equal(read_stl(s), tri)
    raw = open(b, "rb").read()
    bad = {"short": raw[:60], "cut": raw[:-7], "count": raw[:80] + np.uint32(tri.shape[0] + 1).tobytes() + raw[84:],
           "ascii_cut": open(a, "rb").read()[:-400], "empty": b""}
    assert issubclass(MeshDepthError, GsdError) and issubclass(MeshDepthError, ValueError)
    for name, data in bad.items():
        p = str(tmp_path / (name + ".stl"))
        open(p, "wb").write(data)
        with pytest.raises(MeshDepthError, match="truncated|announces"):
            read_stl(p)


def test_plane_convention_equals_the_restated_table():
    from gelslim_depth_amd.mesh_depth import plane_convention
    seen = set()
    for first, second in itertools.permutations("xyz", 2):
        for s1, s2 in itertools.product("+-", repeat=2):
            plane = s1 + first + s2 + second
            assert plane_convention(plane) == R.plane_table(plane), plane
            seen.add(R.plane_table(plane))
    assert len(seen) == 12 and len(R.PLANES) == 12 and len({R.plane_table(p) for p in R.PLANES}) == 12
    for bad in ("+x+x", "", "+a+b", "+x", "xy", "+q+x+y", None):
        with pytest.raises(ValueError, match="Invalid gelslim_plane"):
            plane_convention(bad)


def test_width_file_parser_and_name_rule_match_the_reference():
    from gelslim_depth_amd.mesh_depth import dataset_key, parse_grasp_widths, select_dataset_files
    # depth_from_mesh.py:38-46: "object: distance" lines, ' None' with or without the newline
    w = parse_grasp_widths(["peg: 12.5\n", "gear_1: None\n", "bolt:3\n", "last: None"])
    assert w == {"peg": 12.5, "gear_1": None, "bolt": 3.0, "last": None}
    with pytest.raises(ValueError):
        parse_grasp_widths(["peg: none\n"])          # only the literal ' None' means "per sample": float('none') raises there too
    # :51-54 / :62-65: the field before the last underscore for split files, the stem otherwise
    assert dataset_key("peg_train.pt") == "peg" and dataset_key("set3_gear_val.pt") == "gear"
    assert dataset_key("a_b_test.pt") == "b" and dataset_key("peg.pt") == "peg" and dataset_key("peg.v2.pt") == "peg"
    # :26-33: only .pt files; with an object list the rule is chosen by the FIRST file
    names = ["peg_train.pt", "peg_val.pt", "gear_train.pt", "notes.txt", "bolt.pt"]
    assert select_dataset_files(names, None) == ["peg_train.pt", "peg_val.pt", "gear_train.pt", "bolt.pt"]
    assert select_dataset_files(names[:4], ["peg"]) == ["peg_train.pt", "peg_val.pt"]
    with pytest.raises(IndexError):
        select_dataset_files(names, ["peg"])         # 'bolt.pt' has no field before a last underscore: the reference fails alike
    assert select_dataset_files(["bolt.pt", "peg.pt", "x.stl"], ["peg"]) == ["peg.pt"]
    assert select_dataset_files(["notes.txt"], ["peg"]) == []


# ---- meaning pinned to the reference ----------------------------------------------------------------------------------
IMAGE, HEIGHT_MM = (80, 106), 12.0
POSE = (0.8e-3, -0.5e-3, 0.4)
INDENT = 1.0                 # mm of peak indentation on each finger
# measured on the 48 cases: worst mean |difference| and worst max |difference| 2 px inside both patches
WORST_MEAN_MM, WORST_INNER_MM = 0.000137, 0.003236
FACTOR = 3.0                 # another numpy build may draw another cloud


def _ellipsoid_for(plane):
    """Semi-axes 6 mm along the perpendicular axis, 5 along the unaligned (image rows) and 7 along the aligned one."""
    perp, aligned, unaligned, _ = R.plane_table(plane)
    axes = [0.0, 0.0, 0.0]
    axes[perp], axes[unaligned], axes[aligned] = 6.0, 5.0, 7.0
    centre = [0.0, 0.0, 0.0]
    centre[perp], centre[unaligned], centre[aligned] = 3.0, 0.4, -0.6
    return R.ellipsoid(4, axes, 0.12, centre)


@functools.lru_cache(maxsize=None)
def _pair(plane, invert):
    """(raster_ref midpoint, reference) as (left, right) stacks, and the peak depth: computed once per (plane, invert); LR_flip
    swaps the channels of both, as depth_from_mesh.py:73-76 and the definition do."""
    tri = _ellipsoid_for(plane)
    _, _, q, _ = R.prepare(tri, 1.0, plane)
    g = 2 * (float(q.max()) - INDENT)
    pose = R.inverted_pose(POSE) if invert else POSE
    # delta = 0: the interval collapses onto the definition itself.  With the GPU test's delta about one pixel per image lies
    # within delta of a triangle edge, where [lo, hi] = [depth, 0] and the midpoint says nothing (measured: 0.25 .. 0.48 mm there)
    lo, hi = R.raster_ref(tri, 1.0, plane, pose, g, IMAGE, HEIGHT_MM, False, invert, delta=0.0)
    assert np.array_equal(lo, hi)
    ref = R.reference_depth_image(R.sample_surface(tri, 2e5, seed=0), plane, pose, g, IMAGE, HEIGHT_MM, False, invert)
    return (lo + hi) / 2, ref


CASES = [(p, f, i) for p in R.PLANES for f in (False, True) for i in (False, True)]


@pytest.mark.parametrize("plane,flip,invert", CASES, ids=[f"{p}-flip{int(f)}-inv{int(i)}" for p, f, i in CASES])
def test_exact_definition_means_what_the_reference_computes(plane, flip, invert):
    pytest.importorskip("scipy")
    ours, ref = _pair(plane, invert)
    if flip:
        ours, ref = ours[::-1], ref[::-1]
    peak = float(-ref.min())
    assert 0.8 * INDENT < peak < 1.1 * INDENT and abs(-ours.min() - INDENT) < 0.05
    diff = np.abs(ours - ref)
    mean = float(diff.mean())
    worst = kept = total = 0
    for ch in (0, 1):
        contact = (ours[ch] < 0) & (ref[ch] < 0)
        inner = R.erode(contact, 2)
        total += int(contact.sum())
        kept += int(inner.sum())
        worst = max(worst, float(diff[ch][inner].max()))
    print(f"{plane} flip={flip} invert={invert}: mean {mean:.6f} mm, inner max {worst:.6f} mm, band removes {1 - kept / total:.3f}")
    # the two conditions under which the bounds mean anything
    assert FACTOR * WORST_MEAN_MM < 0.1 * peak and FACTOR * WORST_INNER_MM < 0.1 * peak
    assert total > 0 and 1 - kept / total <= 0.25
    assert mean <= FACTOR * WORST_MEAN_MM and worst <= FACTOR * WORST_INNER_MM


def test_inverted_pose_with_invert_affine_is_the_same_picture():
    lo, hi = R.raster_ref(R.box(), 1.0, "+y+z", POSE, 4.0, (24, 31), 12.0, False, False)
    lo2, hi2 = R.raster_ref(R.box(), 1.0, "+y+z", R.inverted_pose(POSE), 4.0, (24, 31), 12.0, False, True)
    assert np.all(lo <= hi2 + 1e-9) and np.all(lo2 <= hi + 1e-9) and lo.min() < -0.4
    assert math.isclose(float(np.abs((lo + hi) / 2 - (lo2 + hi2) / 2).max()), 0.0, abs_tol=1e-6)
