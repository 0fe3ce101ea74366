"""GPU: register_cloud (gelslim_depth_amd.mesh_register, gsd_mesh_icp_rows + gsd_mesh_icp_lm_update) against the numpy twin's
whole loop (tests/mesh_closest_ref.py `register`) and against the known motion, and end to end from rendered depth images.

The bounds on the recovered motion come from mesh_closest_ref.TWIN, what the twin itself reaches on the same clouds
(test_mesh_closest_cpu measures those figures again): 10 x for the plane fit of (a), as the reduction order differs; the recorded
figure itself for the point kind (1 % for the four digits it is recorded to); 2 x with outliers, where one differing accept decision
changes which outliers stay within the limit."""
import functools

import numpy as np
import pytest
import torch

import mesh_closest_ref as M
import mesh_depth_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLACK_MM = 1e-4          # test_gpu_mesh_depth's: the fp32 interpolation of q in render_depth
AGREE_MM = 1e-6          # device against twin over the bounding box's corners: sin / cos and the order of the sums, over 20 steps


@functools.lru_cache(maxsize=None)
def volume(name):
    from gelslim_depth_amd.mesh_register import MeshVolume
    return MeshVolume(M.case_mesh(name), 1.0, DEV)


@functools.lru_cache(maxsize=None)
def cloud(name, outliers=0.0):
    tri, p = M.case_cloud(name, outliers)
    return tri, p, torch.from_numpy(p).to(DEV)


@functools.lru_cache(maxsize=None)
def twin(name):
    tri, p, _ = cloud(name)
    return M.register(tri, p, None, 20, None, "plane")


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", ("ellipsoid", "l_prism"))
def test_a_displaced_cloud_is_brought_back_as_the_twin_does(name):
    from gelslim_depth_amd.mesh_register import register_cloud
    tri, p, pts = cloud(name)
    res = register_cloud(volume(name), pts, kind="plane", iterations=20)
    trace = host(res.trace)
    assert trace.shape == (21, 1) and (np.diff(trace[:, 0]) <= 0).all() and trace[-1, 0] < 1e-9 * trace[0, 0]
    ref = twin(name)
    gap = M.corner_gap(host(res.matrix), ref["matrix"], tri)
    err = M.corner_gap(host(res.matrix) @ M.T0, np.eye(4), tri)
    want_err, want_rms = M.TWIN[(name, "plane", None, 0.0)]
    print(f"{name}: device - twin {gap:.3e} mm, error {err:.3e} mm (twin {want_err:.3e}), rms {float(res.rms[0]):.3e} mm, "
          f"{int(res.accepted[0])} accepted (twin {ref['accepted']}), cost {trace[0, 0]:.3e} -> {trace[-1, 0]:.3e}")
    assert gap <= AGREE_MM
    assert err <= 10 * want_err
    assert int(res.active[0]) == len(p) and float(res.rms[0]) <= 10 * want_rms and float(res.cost[0]) == trace[-1, 0]
    assert host(res.matrices).shape == (1, 4, 4) and np.array_equal(host(res.matrices[0]), host(res.matrix)) and int(res.best) == 0
    assert np.array_equal(host(res.matrix)[3], (0, 0, 0, 1)) and abs(np.linalg.det(host(res.matrix)[:3, :3]) - 1) < 1e-12
    moved = host(res.apply(pts)).astype(np.float64)
    assert moved.dtype == np.float64 and np.abs(moved - (p.astype(np.float64) @ host(res.matrix)[:3, :3].T + host(res.matrix)[:3, 3])).max() < 1e-5
    again = register_cloud(volume(name), pts, kind="plane", iterations=20)
    assert torch.equal(again.trace.view(torch.int64), res.trace.view(torch.int64)) and torch.equal(again.matrix, res.matrix)


def unit_sag(subdivisions):
    """1 - the smallest distance from the centre to a facet's plane on the unit icosphere: how far a facet sags below the sphere."""
    v = R.icosphere(subdivisions, 1.0)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    return 1.0 - float(np.abs(np.einsum("tk,tk->t", n / np.linalg.norm(n, axis=1, keepdims=True), v[:, 0])).min())


def test_end_to_end_from_rendered_depth_images():
    """render_depth at two poses -> depth_points(frame='object') with each render's own pose and width -> one cloud.  It lies on
    the mesh: within the mesh's sag (the linear map of the ellipsoid stretches the unit icosphere's by at most its norm) plus the
    render's SLACK_MM, as in section 21.  Displaced by T0, register_cloud brings its rms back under the same bound."""
    from gelslim_depth_amd.contact_points import depth_points
    from gelslim_depth_amd.mesh_depth import MeshGrid, render_depth
    from gelslim_depth_amd.mesh_register import cloud_mesh_error, register_cloud
    tri, plane, size = M.case_mesh("ellipsoid"), "+y+z", (40, 53)
    grid = MeshGrid(tri, 1.0, plane, DEV)
    _, _, q, _ = R.prepare(tri, 1.0, plane)
    clouds = []
    for pose, indent in (((1.1e-3, -0.7e-3, 0.4), 0.8), ((-0.6e-3, 0.9e-3, -1.3), 0.5)):
        poses = torch.tensor([pose], dtype=torch.float32, device=DEV)
        widths = torch.tensor([2 * (float(q.max()) - indent)], dtype=torch.float32, device=DEV)
        depth = render_depth(grid, poses, widths, size, 12.0)
        clouds.append(depth_points(depth, widths, 12.0, frame="object", grid=grid, poses=poses).points)
    pts = torch.cat(clouds)
    m = np.eye(3)
    m[0, 1], m[0, 2], m[1, 2] = 0.12, -0.06, 0.09
    bound = float(np.linalg.norm(m @ np.diag((6.0, 5.0, 7.0)), 2)) * unit_sag(3) + SLACK_MM
    vol = volume("ellipsoid")
    err = cloud_mesh_error(vol, pts)
    print(f"{len(pts)} points: mean {float(err['mean']):.3e}, rms {float(err['rms']):.3e}, max {float(err['max']):.3e} mm; bound {bound:.3e}")
    assert len(pts) > 300 and int(err["within"]) == len(pts)
    assert float(err["max"]) < bound and float(err["mean"]) <= float(err["rms"]) <= float(err["max"])
    moved = (pts.double() @ torch.from_numpy(M.T0[:3, :3].T).to(DEV) + torch.from_numpy(M.T0[:3, 3]).to(DEV)).float()
    before = cloud_mesh_error(vol, moved)
    res = register_cloud(vol, moved, kind="plane", iterations=20)
    print(f"displaced: rms {float(before['rms']):.3e} mm -> {float(res.rms[0]):.3e} mm, {int(res.accepted[0])} accepted")
    assert float(before["rms"]) > 3 * bound and float(res.rms[0]) < bound and (np.diff(host(res.trace)[:, 0]) <= 0).all()
    assert abs(float(cloud_mesh_error(vol, res.apply(moved))["rms"]) - float(res.rms[0])) < 1e-5


@pytest.mark.parametrize("name", ("ellipsoid", "l_prism"))
def test_the_point_kind_and_the_truncated_cost(name):
    from gelslim_depth_amd.mesh_register import register_cloud
    tri, p, pts = cloud(name)
    res = register_cloud(volume(name), pts, kind="point", iterations=20)
    err = M.corner_gap(host(res.matrix) @ M.T0, np.eye(4), tri)
    want_err, want_rms = M.TWIN[(name, "point", None, 0.0)]
    print(f"{name} point: error {err:.3e} mm (twin {want_err:.3e}), rms {float(res.rms[0]):.3e} (twin {want_rms:.3e}), {int(res.accepted[0])} accepted")
    assert (np.diff(host(res.trace)[:, 0]) <= 0).all() and err <= 1.01 * want_err and float(res.rms[0]) <= 1.01 * want_rms
    # 10 % gross outliers and a limit: the cost counts a lost point as D^2, so the fit cannot win by shedding points
    tri, p, pts = cloud(name, 0.1)
    res = register_cloud(volume(name), pts, kind="plane", iterations=20, max_distance_mm=M.OUTLIER_D)
    err = M.corner_gap(host(res.matrix) @ M.T0, np.eye(4), tri)
    want_err, want_rms = M.TWIN[(name, "plane", M.OUTLIER_D, 0.1)]
    print(f"{name} outliers: error {err:.3e} mm (twin {want_err:.3e}), rms {float(res.rms[0]):.3e} (twin {want_rms:.3e}), "
          f"{int(res.active[0])} of {len(p)} active")
    assert (np.diff(host(res.trace)[:, 0]) <= 0).all() and err <= 2 * want_err and float(res.rms[0]) <= 2 * want_rms
    assert 0.9 * len(p) <= int(res.active[0]) < len(p)
    free = register_cloud(volume(name), pts, kind="plane", iterations=20)          # without the limit the outliers drag the fit away
    assert M.corner_gap(host(free.matrix) @ M.T0, np.eye(4), tri) > 2 * want_err


def test_several_starts_no_iterations_and_refusals():
    from gelslim_depth_amd.mesh_depth import MeshDepthError
    from gelslim_depth_amd.mesh_register import icp_rows, register_cloud
    name = "l_prism"
    tri, p, pts = cloud(name)
    vol = volume(name)
    starts = np.stack((np.eye(4), M.rigid((3.0, -2.0, 1.0), (0, 1, 1), 1.0), np.linalg.inv(M.T0)))
    res = register_cloud(vol, pts, init=starts, iterations=3)
    cost = host(res.cost)
    best = int(res.best)
    assert cost.shape == (3,) and best == int(np.argmin(cost)) and np.array_equal(host(res.matrix), host(res.matrices[best]))
    assert (np.diff(host(res.trace), axis=0) <= 0).all() and host(res.trace).shape == (4, 3) and host(res.last_step).shape == (3, 6)
    assert best == 2 and cost[1] > 1e3 * cost[0] > 1e6 * cost[2]          # after three steps the nearer start is the better one
    alone = register_cloud(vol, pts, init=starts[0], iterations=3)          # every start is refined on its own
    assert torch.equal(alone.trace[:, 0].view(torch.int64), res.trace[:, 0].view(torch.int64))
    assert torch.equal(alone.matrix, res.matrices[0])
    flat = register_cloud(vol, pts, init=torch.from_numpy(starts[:, :3, :].reshape(3, 12).copy()), iterations=3)
    assert torch.equal(flat.matrices, res.matrices)
    # no iterations: the start and its row
    zero = register_cloud(vol, pts, init=starts, iterations=0)
    assert np.array_equal(host(zero.matrices), starts) and host(zero.trace).shape == (1, 3) and not host(zero.accepted).any()
    rows = icp_rows(vol, pts, torch.from_numpy(starts))
    assert torch.equal(zero.rows.view(torch.int64), rows.view(torch.int64)) and torch.equal(zero.cost, rows[:, 0])
    assert int(zero.best) == 2 and torch.equal(zero.trace[0], rows[:, 0])
    for kw in (dict(iterations=-1), dict(iterations=2.5), dict(kind="line"), dict(max_distance_mm=-1.0), dict(damping=0.0),
               dict(damping_up=0.5), dict(damping_down=0.0), dict(damping_down=1.5), dict(max_step=(1.0,) * 5),
               dict(max_step=(1.0, 1.0, 1.0, 0.1, 0.1, -0.1)), dict(init=np.eye(3)), dict(init=np.zeros((0, 4, 4))),
               dict(weights=torch.ones(3, device=DEV))):
        with pytest.raises(MeshDepthError):
            register_cloud(vol, pts, **kw)
    with pytest.raises(MeshDepthError):
        register_cloud(vol, pts.cpu())
    with pytest.raises(MeshDepthError):
        register_cloud("volume", pts)
    # weights: zero weight on a displaced half leaves the other half's fit
    w = torch.ones(len(p), device=DEV)
    w[::2] = 0.0
    half = register_cloud(vol, pts, weights=w, iterations=20)
    only = register_cloud(vol, pts[1::2].contiguous(), iterations=20)
    assert M.corner_gap(host(half.matrix), host(only.matrix), tri) < 1e-6 and int(half.active[0]) == len(p)


def test_register_cloud_and_cloud_mesh_error_read_nothing_back():
    """Under torch's sync debug mode a host read would raise: one start and several, with and without a limit and weights."""
    from gelslim_depth_amd.mesh_register import closest_points, cloud_mesh_error, icp_rows, register_cloud
    tri, p, pts = cloud("l_prism")
    vol = volume("l_prism")
    starts = torch.from_numpy(np.stack((np.eye(4), np.linalg.inv(M.T0)))).to(DEV)
    w = torch.ones(len(p), device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one = register_cloud(vol, pts, iterations=3)
        two = register_cloud(vol, pts, init=starts, iterations=3, max_distance_mm=1.5, weights=w, kind="point")
        moved = two.apply(pts)
        err = cloud_mesh_error(vol, moved, 2.0)
        rows = icp_rows(vol, pts, starts)
        hits = closest_points(vol, moved)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(two.best) == 1 and torch.equal(two.matrix, two.matrices[1]) and torch.equal(one.matrix, one.matrices[0])
    assert int(err["within"]) == len(p) and rows.shape == (2, 30) and hits.triangle.shape == (len(p),)
