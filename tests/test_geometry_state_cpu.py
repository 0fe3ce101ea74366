"""CPU: the instruments of tests/geometry_state.py can see (nothing here needs a GPU).

The list-order tests on the GPU permute every cell's triangle list and ask for the same bits.  That proves something only if (a)
the permutation moves entries and keeps each cell's set, (b) inputs exist on which a tie rule decides the result, and (c) a wrong
tie rule gives another result on them.  Here all three are shown with the numpy twins: the roof has 31 pixels (the whole of image
row 12) at which a left-slope and a right-slope triangle give bit-equal values and opposite Jacobians, 30 after a shift by one
pixel; the box lattice has 326 points with bit-equal distances to two triangles; and a "first in list order" rule under the
descending order names other winners on every one of them.
"""
import numpy as np
import pytest

import geometry_state as S
import mesh_closest_ref as MC
import mesh_depth_ref as R
import mesh_pose_refine_ref as PR

F = np.float32
ROOF_TIES = {S.ROOF_POSE: 31, S.ROOF_SHIFTED: 30}      # tie pixels of the right channel: the columns of row 12 that lie over the roof


def roof_lists(nx, ny):
    """The roof's cell lists on an nx x ny grid over its box, padded as gsd_mesh_depth_plan pads it."""
    G = PR.records(S.roof(), S.ROOF_PLANE)
    cell = 8.0 / min(nx, ny) if max(nx, ny) > 1 else 1e6
    pad = 1e-3 * cell
    lo, hi = R.grid_cell_ranges(G["rec"], F(-4.0 - pad), F(-4.0 - pad), F(1.0 / cell), nx, ny)
    listed = np.nonzero(G["rec"][:, 9] != 0)[0]
    return S.lists_from_ranges(lo, hi, (nx, ny), listed)


def box_lists():
    tri = R.box()
    lo, hi = MC.volume_cell_ranges(tri, S.BOX_ORIGIN, 1.0 / S.BOX_CELL_MM, S.BOX_DIMS)
    return S.lists_from_ranges(lo, hi, S.BOX_DIMS, np.nonzero(~MC.skipped(MC.vertices(tri)))[0])


LISTS = {"roof-one-cell": lambda: roof_lists(1, 1), "roof-4x4": lambda: roof_lists(4, 4), "roof-9x9": lambda: roof_lists(9, 9), "box": box_lists}


@pytest.mark.parametrize("how", S.HOWS, ids=S.how_id)
@pytest.mark.parametrize("name", list(LISTS))
def test_permute_segments_keeps_every_cells_set_and_moves_entries(name, how):
    start, entries = LISTS[name]()
    assert entries.size == start[-1] and (np.diff(start) >= 3).any(), "some cell must hold three ids or more"
    before = entries.copy()
    got = S.permute_segments(start, entries, how)
    assert np.array_equal(entries, before), "the input is not changed"
    assert got.dtype == entries.dtype and got.shape == entries.shape
    moved = 0
    for c in range(start.size - 1):
        a, b = entries[start[c]:start[c + 1]], got[start[c]:start[c + 1]]
        assert np.array_equal(np.sort(a), np.sort(b)), f"cell {c}: the set of ids changed"
        moved += int((a != b).sum())
    print(f"{name} {S.how_id(how)}: {moved} of {entries.size} entries moved")
    assert moved >= 1
    if how in ("sorted", "sorted_desc"):
        step = np.diff(got.astype(np.int64))
        inner = np.ones(step.size, bool)
        inner[start[1:-1][(start[1:-1] > 0) & (start[1:-1] < got.size)] - 1] = False      # steps across a cell boundary
        assert ((step > 0) if how == "sorted" else (step < 0))[inner].all()
    if how == "reversed":
        assert np.array_equal(S.permute_segments(start, got, how), entries)
    assert np.array_equal(S.permute_segments(start, got, "sorted"), S.permute_segments(start, entries, "sorted"))
    with pytest.raises(ValueError):
        S.permute_segments(start, entries, "rotated")


def test_the_one_cell_roof_list_holds_all_eight_and_the_box_skips_none():
    start, entries = roof_lists(1, 1)
    assert start.tolist() == [0, 8] and sorted(entries.tolist()) == list(range(8)) and entries.tolist() != list(range(8))
    start, entries = box_lists()
    assert start.size == 7 * 5 * 6 + 1 and set(entries.tolist()) == set(range(12))


def exact32(a):
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(a.astype(F).astype(np.float64), a))


@pytest.mark.parametrize("pose", list(ROOF_TIES), ids=["centred", "one-pixel"])
def test_the_roof_is_exact_and_its_ridge_is_a_row_of_ties(pose):
    tri = S.roof()
    assert tri.shape == (8, 3, 3) and tri.dtype == F
    G = PR.records(tri, S.ROOF_PLANE)
    assert float(G["cx"]) == 0.0 and float(G["cy"]) == 0.0 and not G["swap_axes"]
    rec = G["rec"].astype(np.float64)
    assert (np.abs(rec[:, 9]) == 0.0625).all(), "every doubled area is 16: its reciprocal is exact"
    assert np.array_equal(rec * 16, np.round(rec * 16)), "the records are dyadic"
    assert float(F(1000) * F(pose[1])) == pose[1] * 1000 and F(1000) * F(S.ROOF_SHIFTED[1]) == F(S.ROOF_HEIGHT_MM / S.SIZE[0])
    fr = PR.frame(G, pose, S.SIZE, S.ROOF_HEIGHT_MM, True, False)
    exact = PR.frame(G, (1000 * pose[0], 1000 * pose[1], pose[2]), S.SIZE, S.ROOF_HEIGHT_MM, True, False, exact=True)
    for k in ("cs", "sn", "pa", "pb", "da", "db", "x", "y"):
        assert exact32(fr[k]) and np.array_equal(np.asarray(fr[k], np.float64), np.asarray(exact[k], np.float64)), k
    assert (fr["x"][S.ROOF_ROW] == 0.0).all(), "row 12 lies on the ridge"
    t = PR.finger_terms(G, pose, F(S.ROOF_G), S.SIZE, S.ROOF_HEIGHT_MM, True, False)
    assert exact32(t["R"]) and exact32(t["J"])
    # the covering triangles of every pixel and their values, by the twin's own expressions
    x0, y0, x1, y1, x2, y2, q0, q1, q2, inv = (rec[:, k][:, None, None] for k in range(10))
    x, y = fr["x"][None], fr["y"][None]
    l2 = ((x1 - x0) * (y - y0) - (y1 - y0) * (x - x0)) * inv
    l1 = -(((x2 - x0) * (y - y0) - (y2 - y0) * (x - x0)) * inv)
    l0 = ((x2 - x1) * (y - y1) - (y2 - y1) * (x - x1)) * inv
    cover = (l0 >= 0) & (l1 >= 0) & (l2 >= 0)
    val = np.where(cover, q0 + l1 * (q1 - q0) + l2 * (q2 - q0), -np.inf)
    slope = (((q1 - q0) * (y2 - y0) - (q2 - q0) * (y1 - y0)) * inv)[:, 0, 0]      # dq/dx of each triangle
    assert np.array_equal(slope[list(S.ROOF_LEFT)], [0.5] * 4) and np.array_equal(slope[list(S.ROOF_RIGHT)], [-0.5] * 4)
    best = val.max(axis=0)
    at_best = cover & (val == best[None])
    both = at_best[list(S.ROOF_LEFT)].any(axis=0) & at_best[list(S.ROOF_RIGHT)].any(axis=0)      # bit-equal values, different J
    ties = both & t["active"]
    print(f"pose {pose}: {int(ties.sum())} active tie pixels of {int(t['active'].sum())} active, rows {sorted(set(np.nonzero(ties)[0].tolist()))}")
    assert int(ties.sum()) == ROOF_TIES[pose] >= 20
    assert set(np.nonzero(ties)[0].tolist()) == {S.ROOF_ROW} and (ties[S.ROOF_ROW] == t["active"][S.ROOF_ROW]).all()
    assert (t["uncertain"] & t["active"])[ties].all(), "a tie pixel is uncertain: the older Jacobian comparisons drop every one"
    winners = set(t["win"][ties].tolist())
    assert winners == {0, 5} and 0 in S.ROOF_LEFT and 5 in S.ROOF_RIGHT
    assert set(t["J"][0][ties].tolist()) == {0.5, -0.5} and (t["R"][ties] == -0.75).all()
    # the mutation: first in list order
    same = S.first_in_list_terms(G, np.arange(8), pose, F(S.ROOF_G), S.SIZE, S.ROOF_HEIGHT_MM, True)
    for k in ("R", "J", "win", "active"):
        assert np.array_equal(same[k], t[k]), f"ascending order is the lowest-id rule: {k}"
    wrong = S.first_in_list_terms(G, np.arange(8)[::-1], pose, F(S.ROOF_G), S.SIZE, S.ROOF_HEIGHT_MM, True)
    assert np.array_equal(wrong["R"], t["R"]), "the depth is a max: no order changes it"
    differs = (wrong["J"] != t["J"]).any(axis=0)
    assert np.array_equal(differs, ties), "the Jacobian differs on the tie pixels and nowhere else"
    assert set(wrong["win"][ties].tolist()) == {3, 6} and np.array_equal(wrong["J"][0][ties], -t["J"][0][ties])
    # the sums of a normal row are sums of exact dyadics: the order of addition cannot matter
    lo, _ = R.raster_ref(tri, 1.0, S.ROOF_PLANE, pose, S.ROOF_G, S.SIZE, S.ROOF_HEIGHT_MM, delta=0.0)
    full = PR.point_terms(G, pose, F(S.ROOF_G), S.SIZE, S.ROOF_HEIGHT_MM)
    assert np.array_equal(full["R"], lo), "the twin's image is the definition's"
    terms = PR.normal_terms(full["R"], full["J"], np.zeros((2,) + S.SIZE))
    assert np.array_equal(terms.sum(axis=1), terms[:, ::-1].sum(axis=1))


def test_the_box_lattice_has_exact_ties_and_a_first_in_list_rule_names_other_triangles():
    tri, pts = R.box(), S.tie_box_points()
    assert pts.shape == (4 * 8 * 6 * 7, 3) and pts.dtype == F
    tid, x, d2, second = MC.closest_brute(tri, pts)
    ties = second == d2
    print(f"{int(ties.sum())} of {len(pts)} box points have two triangles at bit-equal distances")
    assert int(ties.sum()) == 326 and (tid >= 0).all()
    same = S.first_in_list_closest(tri, np.arange(12), pts)
    assert np.array_equal(same[0], tid) and np.array_equal(same[2], d2)
    wrong = S.first_in_list_closest(tri, np.arange(12)[::-1], pts)
    assert np.array_equal(wrong[2], d2), "the distance is a min: no order changes it"
    assert np.array_equal(wrong[0] != tid, ties), "the winner differs on the tie points and nowhere else"


def test_workloads_are_named_as_the_gpu_modules_expect():
    assert list(S.WORKLOADS) == ["mesh_grid", "contact", "mesh_volume", "touch_fusion", "metrics_data"]
    assert all(callable(w) and callable(w.stage) for w in S.WORKLOADS.values())
    depth, widths, poses, _ = S.contact_batch()
    assert depth.shape == (4, 2) + S.SIZE and not depth[2].any() and np.isnan(depth[3]).sum() == 6 and np.isinf(depth[3]).sum() == 2
    assert (depth[:2].min(axis=(1, 2, 3)) < -0.2).all() and not (depth == 0)[np.signbit(depth)].any(), "contact in both renders, no -0.0"
