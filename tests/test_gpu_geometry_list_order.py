"""GPU: no result of MeshGrid's or MeshVolume's consumers depends on the order inside a cell's triangle list.

mesh_fill and the volume's fill place ids with atomicAdd on a cursor, so the order inside a list changes from build to build; the
consumers claim to be order-free (the render and the score take a max, md_walk<true> and the closest-point walk take the lowest id
among equal values).  Building a grid twice and hoping that the order differs tests that by luck.  Here the order is varied on
purpose -- geometry_state.permute_lists rewrites `owner.list` in place: reversed, ascending, descending, two seeded shuffles -- and
every output must keep its bits.

That alone would pass a kernel that breaks ties by list position on inputs without ties, so the inputs have them: the roof of
geometry_state.roof() puts the whole of image row 12 exactly on a ridge where a left-slope and a right-slope triangle give bit-equal
surface values and opposite Jacobians (test_geometry_state_cpu.py counts 31 such pixels, 30 after a one-pixel shift, and shows that
a first-in-list rule changes J on every one of them under the descending order), and the box lattice of tie_box_points() has 326
points at bit-equal distances from two triangles.  On the roof every number is dyadic, so the device's fp32 / fp64 mix and the
twin's fp64 agree exactly: R, the Jacobian images and the normal rows are compared with == on EVERY pixel, the tie pixels included,
which the older Jacobian comparisons drop as `uncertain`.  Nothing here has a tolerance.

Measured on an MI355X: the 60 tests of the module take 2.9 s together; the first one 0.7 s (it loads the library and builds the
first grid), every other one 0.01 s or less.  With md_walk<true>'s `t < best` flipped to `t > best` in a scratch build the 18
twin comparisons fail (the Jacobian differs on the 31 pixels of row 12); with the clause removed (first maximum in list order) 13
of the permutation tests fail on the roof as well.
"""
import functools

import numpy as np
import pytest
import torch

import engine_state as E
import geometry_state as S
import mesh_closest_ref as MC
import mesh_depth_ref as R
import mesh_pose_ref as P
import mesh_pose_refine_ref as PR

pytestmark = pytest.mark.gpu

F = np.float32
DEV = S.DEV
UNPERMUTED = "as built"
ORDERS = (UNPERMUTED,) + S.HOWS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------------------- MeshGrid
GRIDS = {"roof-one-cell": ("roof", 1e6), "roof-default": ("roof", None), "roof-fine": ("roof", "fine"), "lprism": ("lprism", None),
         "torus": ("torus", None)}
MESHES = {"roof": S.roof, "lprism": P.MESHES["lprism"], "torus": R.torus}


@functools.lru_cache(maxsize=None)
def grid(name):
    from gelslim_depth_amd.mesh_depth import MeshGrid
    mesh, cell = GRIDS[name]
    if cell == "fine":
        cell = grid(name.replace("fine", "default")).cell_mm / 4
    return MeshGrid(MESHES[mesh](), 1.0, P.PLANE, DEV, cell_mm=cell)


@functools.lru_cache(maxsize=None)
def grid_inputs(mesh):
    """(height, poses (3, 3), widths (3,), candidates (3, 4, 3), many (3, 3)) on the device."""
    if mesh == "roof":
        height, gw = S.ROOF_HEIGHT_MM, S.ROOF_G
        poses = np.asarray([S.ROOF_POSE, S.ROOF_SHIFTED, (0.3e-3, -0.2e-3, 0.4)], F)
    else:
        height, gw = 12.0, P.contact_width(MESHES[mesh]())
        poses = np.asarray([(0.6e-3, -0.45e-3, 0.45), (-0.4e-3, 0.35e-3, -1.1), (0.0, 0.0, 0.0)], F)
    widths = np.asarray([gw, gw, gw - 0.25], F)
    rng = np.random.Generator(np.random.PCG64(11))
    cand = poses[:, None, :] + ((rng.random((3, 4, 3)) * 2 - 1) * np.asarray([0.5e-3, 0.5e-3, 0.2])).astype(F)
    cand[:, 0] = poses          # the observation's own pose: on the roof, candidates that sit on the ties
    cand[0, 1] = S.ROOF_SHIFTED if mesh == "roof" else cand[0, 1]
    many = np.stack([widths, widths - F(0.125), widths + F(0.25)], axis=1)
    return height, dev(poses), dev(widths), dev(cand.astype(F)), dev(many.astype(F))


def grid_results(name):
    from gelslim_depth_amd import mesh_depth as M
    g = grid(name)
    height, poses, widths, cand, many = grid_inputs(GRIDS[name][0])
    observed = M.render_depth(g, poses, widths, S.SIZE, height)
    res = {"render": observed, "jacobian": M.render_depth_jacobian(g, poses, widths, S.SIZE, height),
           "score": M.score_poses(g, observed, cand, widths, height), "score_widths": M.score_poses_widths(g, observed, cand, many, height),
           "normal_rows": M.pose_normal_rows(g, observed, cand, widths, height),
           "normal_rows_stride2": M.pose_normal_rows(g, observed, cand, widths, height, stride=2)}
    for fit in (False, True):
        r = M.refine_pose(g, observed, widths, cand[:, 1:3].contiguous(), iterations=3, fit_width=fit, image_height_mm=height)
        res.update({f"refine{int(fit)}.{k}": getattr(r, k) for k in S.REFINEMENT})
    torch.cuda.synchronize()
    return {k: E.snap(v) for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def grid_baseline(name):
    return grid_results(name)


@pytest.mark.parametrize("how", S.HOWS, ids=S.how_id)
@pytest.mark.parametrize("name", list(GRIDS))
def test_mesh_grid_results_do_not_depend_on_the_list_order(name, how):
    g = grid(name)
    want = grid_baseline(name)
    # (the L prism's caps are flat: its depth does not change with the pose where it is active, its Jacobian is all zero)
    assert int((want["render"] < 0).sum()) > 100 and (name == "lprism" or int((want["jacobian"] != 0).sum()) > 100)
    old = S.permute_lists(g, how)
    try:
        moved = int((g.list != old).sum())
        got = grid_results(name)
    finally:
        g.list.copy_(old)
    print(f"{name} {S.how_id(how)}: {moved} of {g.pairs} list entries moved, {g.grid.nx} x {g.grid.ny} cells")
    start = S.list_start(g)
    assert np.array_equal(S.permute_segments(start, g.list.cpu().numpy(), "sorted"), S.permute_segments(start, old.cpu().numpy(), "sorted"))
    E.same_results(want, got, f"{name}: as built against {S.how_id(how)}")


@pytest.mark.parametrize("name", list(GRIDS))
def test_the_orders_differ_from_one_another(name):
    """The stimulus is not vacuous: ascending and descending differ wherever a cell holds two ids, and the list as built and its
    five permutations are at least four different lists (as built may itself be ascending or descending: two of the six then
    coincide with two others)."""
    g = grid(name)
    start, built = S.list_start(g), g.list.cpu().numpy()
    assert (np.diff(start) >= 2).any()
    lists = {how: S.permute_segments(start, built, how).tobytes() for how in S.HOWS}
    assert lists["sorted"] != lists["sorted_desc"] and len(set(lists.values()) | {built.tobytes()}) >= 4


# ---- the roof against the twin, on every pixel
@functools.lru_cache(maxsize=None)
def roof_twin(pose):
    G = PR.records(S.roof(), S.ROOF_PLANE)
    return PR.point_terms(G, pose, F(S.ROOF_G), S.SIZE, S.ROOF_HEIGHT_MM)


@pytest.mark.parametrize("order", ORDERS, ids=[S.how_id(o) for o in ORDERS])
@pytest.mark.parametrize("name", ["roof-one-cell", "roof-default", "roof-fine"])
def test_roof_images_and_normal_rows_equal_the_twin_on_every_pixel(name, order):
    from gelslim_depth_amd import mesh_depth as M
    g = grid(name)
    poses = dev(np.asarray([S.ROOF_POSE, S.ROOF_SHIFTED], F))
    widths = dev(np.asarray([S.ROOF_G, S.ROOF_G], F))
    twins = [roof_twin(S.ROOF_POSE), roof_twin(S.ROOF_SHIFTED)]
    # both are scored against the image of the roof one pixel further along a1 (the roof does not change along a2): e = R - D is a
    # difference of exact dyadics, +-0.125 on the slopes
    seen = roof_twin(S.ROOF_SEEN)["R"]
    observed = dev(np.stack([seen, seen]).astype(F))
    cand = dev(np.asarray([[S.ROOF_POSE, S.ROOF_SHIFTED], [S.ROOF_SHIFTED, S.ROOF_POSE]], F))
    old = S.permute_lists(g, order) if order != UNPERMUTED else None
    try:
        image = M.render_depth(g, poses, widths, S.SIZE, S.ROOF_HEIGHT_MM).cpu().numpy()
        jac = M.render_depth_jacobian(g, poses, widths, S.SIZE, S.ROOF_HEIGHT_MM).cpu().numpy()
        rows = {s: M.pose_normal_rows(g, observed, cand, widths, S.ROOF_HEIGHT_MM, stride=s).cpu().numpy() for s in (1, 2)}
    finally:
        if old is not None:
            g.list.copy_(old)
    for n, t in enumerate(twins):
        ties = int((t["uncertain"] & t["active"]).sum())
        assert ties >= 30 and image.dtype == F and jac.dtype == np.float64
        assert np.array_equal(image[n].astype(np.float64), t["R"]), f"pose {n}: R differs from the twin on {int((image[n] != t['R']).sum())} pixels"
        bad = (jac[n] != t["J"]).any(axis=1)
        assert not bad.any(), (f"pose {n}: the Jacobian differs from the twin on {int(bad.sum())} pixels, {int((bad & t['uncertain']).sum())} of "
                               f"them among the {int(t['uncertain'].sum())} that the twin marks uncertain; rows {sorted(set(np.nonzero(bad)[1].tolist()))}")
    for s, got in rows.items():
        for b in range(2):
            for p in range(2):
                t = twins[b] if p == 0 else twins[1 - b]          # cand[b, p]
                terms = PR.normal_terms(t["R"], t["J"], seen, s)
                want = terms.sum(axis=1)
                assert np.array_equal(want, terms[:, ::-1].sum(axis=1)) and np.array_equal(want, np.array([float(np.sum(r[np.argsort(np.abs(r))])) for r in terms]))
                # == on every entry: bit equality wherever the value is not zero (a zero's sign is not part of the contract)
                assert np.array_equal(got[b, p], want), (s, b, p, got[b, p].tolist(), want.tolist())
                assert want[1] > 50 and want[0] > 0 and want[2] != 0 and want[4] != 0          # (J_a2 is 0: the roof does not change along a2)


# ------------------------------------------------------------------------------------------------------------------- MeshVolume
VOLUMES = {"box": (R.box, S.BOX_CELL_MM), "l_prism": (R.l_prism, None)}
CLOSEST = ("triangle", "closest", "distance", "sq_distance")


@functools.lru_cache(maxsize=None)
def volume(name):
    from gelslim_depth_amd.mesh_register import MeshVolume
    make, cell = VOLUMES[name]
    return MeshVolume(make(), 1.0, DEV, cell)


@functools.lru_cache(maxsize=None)
def volume_points(name):
    if name == "box":
        return S.tie_box_points()
    rng = np.random.Generator(np.random.PCG64(7))
    return ((rng.random((1000, 3)) - 0.5) * 9.0).astype(F)


def volume_results(name):
    from gelslim_depth_amd import mesh_register as G
    vol, pts = volume(name), dev(volume_points(name))
    starts = dev(np.stack((np.eye(4), MC.rigid((0.3, -0.2, 0.1), (0, 1, 1), 0.1), MC.rigid((-0.2, 0.1, 0.3), (1, 0.5, 0), -0.15))))
    res = {}
    for label, d in (("all", None), ("near", 1.0)):
        c = G.closest_points(vol, pts, d)
        res.update({f"closest.{label}.{k}": getattr(c, k) for k in CLOSEST})
    for kind in ("plane", "point"):
        res[f"icp_rows.{kind}"] = G.icp_rows(vol, pts, starts, 2.0, kind)
    torch.cuda.synchronize()
    return {k: E.snap(v) for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def volume_baseline(name):
    return volume_results(name)


NOT_FINITE = tuple(f"closest.near.{k}" for k in ("closest", "distance", "sq_distance"))      # a miss is NaN, +inf, +inf by contract


@pytest.mark.parametrize("order", ORDERS, ids=[S.how_id(o) for o in ORDERS])
@pytest.mark.parametrize("name", list(VOLUMES))
def test_mesh_volume_results_do_not_depend_on_the_list_order(name, order):
    vol = volume(name)
    want = volume_baseline(name)
    old = S.permute_lists(vol, order) if order != UNPERMUTED else None
    try:
        got = volume_results(name)
    finally:
        if old is not None:
            vol.list.copy_(old)
    E.same_results(want, got, f"{name}: as built against {S.how_id(order)}", not_finite=NOT_FINITE)
    assert int((got["closest.near.triangle"] < 0).sum()) > 0 and int((got["closest.near.triangle"] >= 0).sum()) > 0
    if name == "box":
        g = vol.volume
        assert (g.nx, g.ny, g.nz) == S.BOX_DIMS and (g.x0, g.y0, g.z0) == S.BOX_ORIGIN and g.cell == S.BOX_CELL_MM
        for label, d in (("all", None), ("near", 1.0)):
            tid, x, d2, second = MC.closest_brute(R.box(), volume_points(name), d)
            if d is None:
                assert int((second == d2).sum()) == 326, "the points with two triangles at bit-equal distances"
            assert np.array_equal(got[f"closest.{label}.triangle"].numpy(), tid), f"{label}: the winner"
            assert np.array_equal(got[f"closest.{label}.sq_distance"].numpy().view(np.int64), d2.view(np.int64)), f"{label}: sq_distance"
            assert np.array_equal(got[f"closest.{label}.closest"].numpy(), x.astype(F), equal_nan=True), f"{label}: closest"
