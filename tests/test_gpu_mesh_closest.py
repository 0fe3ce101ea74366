"""GPU: gsd_mesh_closest_points and gsd_mesh_icp_rows (gelslim_depth_amd.mesh_register) against the numpy fp64 twins of DESIGN.md
section 23 (tests/mesh_closest_ref.py).

The kernel computes a triangle's closest point in the twin's order of operations, in fp64 with + - * / alone, so the comparison is
BIT FOR BIT: the winning triangle, sq_distance, closest = fp32(x); distance = fp32(sqrt(d^2)) within one fp32 ulp for the square
root.  The rows are sums: every entry within n * 2^-52 * sum |terms| of the twin's math.fsum, the count equal."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_closest_ref as M
import mesh_depth_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def volume(name, cell=None):
    from gelslim_depth_amd.mesh_register import MeshVolume
    tri, scale = M.query_mesh(name)
    return MeshVolume(tri, scale, DEV, cell)


@functools.lru_cache(maxsize=None)
def twin(name):
    """label -> (points fp32, closest_brute of them), computed once per mesh."""
    tri, scale = M.query_mesh(name)
    return {k: (p, M.closest_brute(tri, p, pc_scale=scale)) for k, p in M.query_points(name).items()}


def query(vol, pts, D=None):
    from gelslim_depth_amd.mesh_register import closest_points
    res = closest_points(vol, torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(DEV), D)
    assert res.triangle.dtype == torch.int32 and res.sq_distance.dtype == torch.float64 and res.closest.dtype == torch.float32
    return [t.cpu().numpy() for t in (res.triangle, res.closest, res.distance, res.sq_distance)]


def bits(arrays):
    return [a.view(np.int32 if a.dtype.itemsize == 4 else np.int64) for a in arrays]


def hold(got, want, what):
    """Device against twin, bit for bit (the root within one fp32 ulp)."""
    tid, closest, dist, sq = got
    wid, wx, wd2 = want[:3]
    assert np.array_equal(tid, wid), (what, "triangle", int((tid != wid).sum()), len(tid))
    assert np.array_equal(sq.view(np.int64), wd2.view(np.int64)), (what, "sq_distance", float(M.ulp_gap(sq, wd2).max()))
    assert np.array_equal(closest, wx.astype(np.float32), equal_nan=True), (what, "closest")
    root = np.sqrt(wd2).astype(np.float32)
    hit = wid >= 0
    assert np.isinf(dist[~hit]).all() and (dist[~hit] > 0).all() and np.isnan(closest[~hit]).all(), what
    assert (np.abs(dist[hit].astype(np.float64) - root[hit]) <= np.spacing(root[hit])).all(), (what, "distance")


@pytest.mark.parametrize("name", M.QUERY_MESHES)
def test_closest_points_equal_the_brute_force_twin_bit_for_bit(name):
    vol = volume(name)
    tri, scale = M.query_mesh(name)
    assert vol.skipped == int(M.skipped(M.vertices(tri, scale)).sum()) and vol.triangles == len(tri) and vol.pairs > 0
    print(vol)
    cases = twin(name)
    pts = np.concatenate([p for p, _ in cases.values()])
    want = [np.concatenate([w[k] for _, w in cases.values()]) for k in range(3)]
    assert (want[0] >= 0).all() and (want[2][:700] > 0).all() and (want[2][700:1200] < 1e-8).all()
    hold(query(vol, pts), want, name)
    p, w = cases["random"]
    for n in (1, 63, 64, 65, 257):      # one lane, around a wave, past a block
        hold(query(vol, p[:n]), [a[:n] for a in w[:3]], f"{name} N={n}")
    # a limit: the winner needs d^2 <= D^2 -- the median distance splits the random points
    D = float(np.sqrt(np.median(w[2])))
    hold(query(vol, p, D), M.closest_brute(tri, p, D, scale), f"{name} D={D}")


def test_points_on_the_cell_planes_of_a_box():
    """cell_mm = 1 divides the box's extent (6, 4, 5): query the lattice of cell corners and the points beside them."""
    vol = volume("box", 1.0)
    g = vol.volume
    assert (g.nx, g.ny, g.nz) == (7, 5, 6)
    lattice = np.array([(g.x0 + i * g.cell, g.y0 + j * g.cell, g.z0 + k * g.cell) for i in range(g.nx + 1) for j in range(g.ny + 1)
                        for k in range(g.nz + 1)])
    pts = np.concatenate([np.float32(lattice), np.nextafter(np.float32(lattice), np.float32(np.inf)),
                          np.nextafter(np.float32(lattice), np.float32(-np.inf)), np.float32(lattice + (0.5, 0.0, 0.0))])
    hold(query(vol, pts), M.closest_brute(R.box(), pts), "box cell planes")


def test_the_result_does_not_depend_on_the_grid_the_batch_or_the_call():
    from gelslim_depth_amd.mesh_register import MeshVolume
    for name in ("torus", "pattern_32"):
        tri, scale = M.query_mesh(name)
        default = volume(name)
        ext = float(max(default.bbox[1] - default.bbox[0]))
        one, fine = MeshVolume(tri, scale, DEV, 4 * ext), MeshVolume(tri, scale, DEV, default.cell_mm / 4)
        assert one.shape == (1, 1, 1) and fine.cell_mm < default.cell_mm < one.cell_mm and fine.pairs > default.pairs > one.pairs
        pts = np.concatenate([p for p, _ in twin(name).values()])[::3]
        ref = bits(query(default, pts))
        for vol in (one, fine, default):      # `default` again: a second call repeats the bits
            assert all(np.array_equal(a, b) for a, b in zip(bits(query(vol, pts)), ref)), (name, vol)
        for i in (0, 5, 400, len(pts) - 1):      # a point alone equals itself in the batch
            assert all(np.array_equal(a, b[i:i + 1]) for a, b in zip(bits(query(default, pts[i:i + 1])), ref)), (name, i)


def test_edge_batches():
    from gelslim_depth_amd.mesh_register import MeshVolume
    tri = R.box()
    vol = volume("box")
    nan, inf = np.nan, np.inf
    pts = np.array([(nan, 0, 0), (0, inf, 0), (0, 0, -inf), (nan, nan, nan), (3, 0, 0), (4, 0, 0), (0, 0, 0), (3, 2, 2.5)], np.float32)
    tid, closest, dist, sq = query(vol, pts)
    assert np.array_equal(tid[:4], [-1] * 4) and np.isnan(closest[:4]).all() and np.isinf(dist[:4]).all() and np.isinf(sq[:4]).all()
    hold((tid, closest, dist, sq), M.closest_brute(tri, pts), "non-finite")
    # D = 0 keeps the points on the surface, d^2 == 0, alone
    got = query(vol, pts, 0.0)
    assert np.array_equal(got[0] >= 0, [False] * 4 + [True, False, False, True]) and not got[3][[4, 7]].any()
    hold(got, M.closest_brute(tri, pts, 0.0), "D = 0")
    # a D below every distance: nothing
    off = np.array([(4, 0, 0), (0, 0, 0), (0, 9, 0)], np.float32)
    got = query(vol, off, 0.5)
    assert np.array_equal(got[0], [-1] * 3) and np.isnan(got[1]).all() and np.isinf(got[3]).all()
    # a mesh of one triangle, and one of degenerate triangles alone
    rng = np.random.Generator(np.random.PCG64(3))
    q = np.float32((rng.random((300, 3)) - 0.5) * 12)
    single = MeshVolume(tri[:1], 1.0, DEV)
    hold(query(single, q), M.closest_brute(tri[:1], q), "one triangle")
    flat = np.repeat(R.l_prism()[20:21], 3, axis=0)
    none = MeshVolume(flat, 1.0, DEV)
    assert none.skipped == 3 and none.pairs == 0
    got = query(none, q)
    assert np.array_equal(got[0], [-1] * 300) and np.isnan(got[1]).all() and np.isinf(got[2]).all() and np.isinf(got[3]).all()
    # a mesh far from the origin: the walk's bound is formed relative to the grid, not from absolute coordinates
    centre = (4096.0, -2048.0, 8192.0)
    away = R.box(centre=centre)
    hold(query(MeshVolume(away, 1.0, DEV, 0.5), q + np.float32(centre)), M.closest_brute(away, q + np.float32(centre)), "far from the origin")
    # l_prism: its degenerate triangle is skipped, a point on it finds another
    lp = volume("l_prism")
    far = np.float32(M.vertices(R.l_prism())[20].mean(axis=0))[None]
    hold(query(lp, far), M.closest_brute(R.l_prism(), far), "on a skipped triangle")


def test_python_refusals():
    from gelslim_depth_amd.mesh_depth import MeshDepthError
    from gelslim_depth_amd.mesh_register import ClosestPoints, MeshVolume, closest_points, cloud_mesh_error, icp_rows
    tri = R.box()
    for bad in (np.zeros((0, 3, 3)), np.zeros((4, 3)), np.full((2, 3, 3), np.nan), np.full((1, 3, 3), 1e39)):
        with pytest.raises(MeshDepthError):
            MeshVolume(bad, 1.0, DEV)
    for kw in (dict(pc_scale=0.0), dict(pc_scale=float("inf")), dict(cell_mm=0.0), dict(cell_mm=float("nan")), dict(device="cpu")):
        with pytest.raises(MeshDepthError):
            MeshVolume(tri, **{"pc_scale": 1.0, "device": DEV, **kw})
    vol = volume("box")
    p = torch.zeros((5, 3), device=DEV)
    for bad in (p.cpu(), p.double(), p[:0], p[:, :2], p.reshape(-1), "points"):
        with pytest.raises(MeshDepthError):
            closest_points(vol, bad)
    for D in (-1.0, float("nan"), "far"):
        with pytest.raises(MeshDepthError):
            closest_points(vol, p, D)
    with pytest.raises(MeshDepthError):
        closest_points("volume", p)
    with pytest.raises(MeshDepthError):
        closest_points(vol, p, out=ClosestPoints(torch.empty(4, device=DEV, dtype=torch.int32), None, None, None))
    out = closest_points(vol, p)
    again = closest_points(vol, p + 1, out=out)
    assert again.triangle is out.triangle and float(again.sq_distance[0]) == 1.0          # (1, 1, 1) is 1 mm below the face y = 2
    eye = torch.eye(4, dtype=torch.float64)
    for kw in (dict(kind="line"), dict(weights=torch.ones(4, device=DEV)), dict(weights=torch.ones(5)), dict(max_distance_mm=-2.0),
               dict(out=torch.empty((2, 30), device=DEV, dtype=torch.float64))):
        with pytest.raises(MeshDepthError):
            icp_rows(vol, p, eye, **kw)
    for bad in (torch.eye(3), torch.zeros((2, 11)), torch.zeros((0, 12))):
        with pytest.raises(MeshDepthError):
            icp_rows(vol, p, bad)
    # a padded ContactCloud's NaN rows are ignored by rule
    from gelslim_depth_amd.contact_points import ContactCloud
    pad = torch.full((2, 4, 3), float("nan"), device=DEV)
    pad[0, :2] = torch.tensor([(4.0, 0, 0), (0, 3.0, 0)], device=DEV)
    err = cloud_mesh_error(vol, ContactCloud(pad, None, None, torch.zeros((2, 2), dtype=torch.int32, device=DEV), "object", 4))
    assert int(err["within"]) == 2 and float(err["max"]) == 1.0 and float(err["mean"]) == 1.0 and float(err["rms"]) == 1.0
    assert int(cloud_mesh_error(vol, pad.reshape(-1, 3), 0.5)["within"]) == 0


def test_abi_refusals():
    from gelslim_depth_amd import _lib as L
    lib = L.lib
    vol = volume("box")
    n = 8
    p = torch.zeros((n, 3), device=DEV)
    tid = torch.empty(n, device=DEV, dtype=torch.int32)
    x, d, sq = torch.empty((n, 3), device=DEV), torch.empty(n, device=DEV), torch.empty(n, device=DEV, dtype=torch.float64)
    mesh = list(vol._mesh_args())
    ok = mesh + [p.data_ptr(), n, float("inf"), tid.data_ptr(), x.data_ptr(), d.data_ptr(), sq.data_ptr(), None]
    assert lib.gsd_mesh_closest_points(*ok) == L.GSD_OK
    for i, bad in ((0, None), (1, None), (2, 0), (3, None), (4, None), (5, 0), (6, None), (7, 0), (7, -3), (8, -1.0), (8, float("nan")),
                   (9, None), (10, None), (11, None), (12, None), (12, sq.data_ptr() + 4)):
        args = list(ok)
        args[i] = bad
        assert lib.gsd_mesh_closest_points(*args) == L.GSD_ERR_BAD_ARG, (i, bad)
    broken = L.gsd_mesh_volume.from_buffer_copy(vol.volume)
    broken.reserved = 1
    assert lib.gsd_mesh_closest_points(C.byref(broken), *ok[1:]) == L.GSD_ERR_BAD_ARG
    broken.reserved, broken.nx = 0, 4096
    assert lib.gsd_mesh_closest_points(C.byref(broken), *ok[1:]) == L.GSD_ERR_BAD_ARG
    t = torch.eye(4, dtype=torch.float64, device=DEV)[:3].reshape(1, 12).contiguous()
    rows = torch.empty((1, 30), device=DEV, dtype=torch.float64)
    ws = torch.empty(30, device=DEV, dtype=torch.float64)
    ok = mesh + [p.data_ptr(), None, n, t.data_ptr(), 1, float("inf"), 0, rows.data_ptr(), ws.data_ptr(), 30, None]
    assert lib.gsd_mesh_icp_rows(*ok) == L.GSD_OK
    for i, bad in ((6, None), (8, 0), (9, None), (10, 0), (11, -1.0), (11, float("nan")), (12, 2), (12, -1), (13, None), (14, None)):
        args = list(ok)
        args[i] = bad
        assert lib.gsd_mesh_icp_rows(*args) == L.GSD_ERR_BAD_ARG, (i, bad)
    args = list(ok)
    args[15] = 29
    assert lib.gsd_mesh_icp_rows(*args) == L.GSD_ERR_WORKSPACE
    lm = L.gsd_icp_lm()
    lm.down, lm.up, lm.lambda_min, lm.lambda_max, lm.first = 0.1, 10.0, 1e-12, 1e12, 1
    lm.max_step[:] = (1.0,) * 6
    state, lam, row = torch.empty_like(t), torch.ones(1, device=DEV, dtype=torch.float64), torch.empty_like(rows)
    trace, acc, step = torch.empty(1, device=DEV, dtype=torch.float64), torch.empty(1, device=DEV, dtype=torch.int32), torch.empty(6, device=DEV, dtype=torch.float64)
    ok = [C.byref(lm), 1, state.data_ptr(), lam.data_ptr(), row.data_ptr(), t.data_ptr(), rows.data_ptr(), trace.data_ptr(), acc.data_ptr(),
          step.data_ptr(), None]
    assert lib.gsd_mesh_icp_lm_update(*ok) == L.GSD_OK
    for i, bad in ((0, None), (1, 0), (2, None), (5, None), (9, None)):
        args = list(ok)
        args[i] = bad
        assert lib.gsd_mesh_icp_lm_update(*args) == L.GSD_ERR_BAD_ARG, (i, bad)
    for field, bad in (("down", 0.0), ("down", 2.0), ("up", 0.5), ("lambda_min", -1.0), ("lambda_max", 1e-13), ("reserved", 1)):
        keep = getattr(lm, field)
        setattr(lm, field, bad)
        assert lib.gsd_mesh_icp_lm_update(*ok) == L.GSD_ERR_BAD_ARG, (field, bad)
        setattr(lm, field, keep)
    lm.max_step[3] = -0.1
    assert lib.gsd_mesh_icp_lm_update(*ok) == L.GSD_ERR_BAD_ARG
    torch.cuda.synchronize()


# ---- normal-equation rows -----------------------------------------------------------------------------------------------------
# identity; 0.01 rad about (1, 2, -2) and (0.05, -0.03, 0.02) mm; 0.7 rad about (2, -1, 1) and (1.5, -2, 1) mm: written out, so that
# no sine or cosine stands between the two sides
TRANSFORMS = (
    (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0),
    (0.9999555559259247, 0.00667766657462994, 0.00665544453759228, 0.05, -0.00665544453759228, 0.9999722224537029,
     -0.0033554998150932156, -0.03, -0.00667766657462994, 0.003311055741017894, 0.9999722224537029, 0.02),
    (0.9216140624281628, -0.3413867070732082, -0.18461483192953376, 1.5, 0.18461483192953376, 0.804035156070407, -0.5651945077886605,
     -2.0, 0.3413867070732082, 0.48680857021682333, 0.804035156070407, 1.0),
)
ICP_D = 0.5


@functools.lru_cache(maxsize=None)
def icp_case():
    """(tri, cloud fp32 (5000, 3), weights fp32, closest_brute per transform): surface samples of ellipsoid(3) with 0.3 mm of
    noise, one NaN row; every smaller cloud is a prefix."""
    tri = R.ellipsoid(3)
    rng = np.random.Generator(np.random.PCG64(21))
    cloud = np.float32(R.sample_surface(tri, 5000, seed=9) + rng.normal(0.0, 0.3, (5000, 3)))
    cloud[1000] = np.nan
    weights = np.float32(rng.random(5000) * 2.0)
    found = [M.closest_brute(tri, M.transform_points(cloud, T)) for T in TRANSFORMS]
    return tri, cloud, weights, found


@pytest.mark.parametrize("n", (1, 1023, 1025, 5000))
def test_icp_rows_against_the_twin(n):
    from gelslim_depth_amd.mesh_register import MeshVolume, icp_rows
    tri, cloud, weights, found = icp_case()
    vol = MeshVolume(tri, 1.0, DEV)
    pts, wts = torch.from_numpy(cloud[:n]).to(DEV), torch.from_numpy(weights[:n]).to(DEV)
    ts = torch.tensor(TRANSFORMS, dtype=torch.float64, device=DEV)
    worst = 0.0
    for kind in ("plane", "point"):
        for D in (None, ICP_D):
            for w in (None, wts):
                got = icp_rows(vol, pts, ts, D, kind, w)
                assert got.shape == (3, 30) and got.dtype == torch.float64
                again = icp_rows(vol, pts, ts, D, kind, w, out=torch.empty_like(got))
                assert torch.equal(got.view(torch.int64), again.view(torch.int64))
                for s, T in enumerate(TRANSFORMS):
                    alone = icp_rows(vol, pts, ts[s], D, kind, w)
                    assert torch.equal(alone.view(torch.int64), got[s:s + 1].view(torch.int64)), (kind, D, s)
                    f = tuple(a[:n] for a in found[s])
                    want, sums = M.icp_row(tri, cloud[:n], T, D, kind, None if w is None else weights[:n], found=f)
                    row = got[s].cpu().numpy()
                    assert row[1] == want[1], (kind, D, s, row[1], want[1])
                    bound = n * 2.0 ** -52 * sums
                    assert (np.abs(row - want) <= bound).all(), (kind, D, s, np.nonzero(np.abs(row - want) > bound)[0])
                    worst = max(worst, float((np.abs(row - want) / np.maximum(bound, 1e-300)).max()))
                    if D is not None and n >= 1023:
                        assert 0 < want[1] < n - 1          # the limit bites, and the NaN row is in no count
    print(f"n = {n}: worst |row - twin| / bound = {worst:.3g}")


# ---- the cell lists -----------------------------------------------------------------------------------------------------------
# cells per axis at 1 mm: one cell, then the counts around the multiples 4096 and 8192 of the scan's pass of 2048 counts: one short
# of two passes, exactly two, one count in a third pass, two counts in a fifth (8193 = 3 * 2731 needs an axis of 2731 cells, more
# than the 1024 allowed: 8194 is the nearest count above 8192)
@pytest.mark.parametrize("dims, ncells", (((1, 1, 1), 1), ((15, 13, 21), 4095), ((16, 16, 16), 4096), ((17, 241, 1), 4097),
                                          ((17, 241, 2), 8194)))
def test_cell_lists_across_the_scan_pass_boundary(dims, ncells):
    from gelslim_depth_amd.mesh_register import MeshVolume
    tri = R.cell_list_mesh(dims)
    one = MeshVolume(tri, 1.0, DEV, 1000.0)
    assert one.shape == (1, 1, 1) and one.skipped == 1
    listed = np.sort(one.list.cpu().numpy())
    assert np.array_equal(listed, np.delete(np.arange(len(tri)), R.CELL_LIST_SKIPPED)) and len(tri) == 16
    vol = MeshVolume(tri, 1.0, DEV, 1.0)
    assert vol.shape == dims[::-1] and int(np.prod(dims)) == ncells
    g = vol.volume
    lo, hi = M.volume_cell_ranges(tri, (g.x0, g.y0, g.z0), g.inv_cell, dims)
    R.check_cell_lists(vol.cells.cpu().numpy(), vol.list.cpu().numpy(), vol.pairs, dims, len(tri), listed, lo, hi)


# ---- the damped step's edge rows ------------------------------------------------------------------------------------------------
def icp_spd_row(rng, b_scale=1.0):
    Jm = rng.normal(0, 1, (40, 6)) * np.array([1.0, 0.7, 1.3, 3.0, 2.0, 2.5])
    e = rng.normal(0, 0.1, 40)
    A, b = Jm.T @ Jm, (Jm.T @ e) * b_scale
    return np.concatenate(([e @ e, 40.0, e @ e], b, [A[j, k] for j, k in M.PAIRS])), A


def test_lm_update_edge_rows_equal_the_twin_bit_for_bit():
    """Three starts in one call: (0) an accepted trial whose matrix is singular in one parameter -- the gate gives the step 0 and
    the next trial is the state; (1) a NaN trial cost -- not accepted, the step comes from the old row, unclipped in translation;
    (2) an accepted trial whose right-hand side is so large that the clip binds in every component.  The rotation's clip of
    1e-9 rad keeps |omega| below 1e-8, so exp(xi) takes its series branch and no sine or cosine stands between the device and
    M.lm_update: every output is compared bit for bit."""
    from gelslim_depth_amd import _lib as L
    rng = np.random.Generator(np.random.PCG64(31))
    max_step = (1e-3, 1e-3, 1e-3, 1e-9, 1e-9, 1e-9)
    cur = np.stack([icp_spd_row(rng, s)[0] for s in (1.0, 1e-3, 1.0)])
    trial = np.stack([icp_spd_row(rng, s)[0] for s in (1.0, 1.0, 1e6)])
    trial[0, 0], trial[1, 0], trial[2, 0] = 0.5 * cur[0, 0], np.nan, 0.5 * cur[2, 0]
    for q, (j, k) in enumerate(M.PAIRS):
        if 4 in (j, k):
            trial[0, 9 + q] = 0.0                     # w2 drops out of start 0's trial matrix
    trial[0, 3 + 4] = 0.0
    T0 = np.stack([np.asarray(t, float) for t in TRANSFORMS])
    T1 = T0[[1, 2, 0]].copy()
    lam0 = np.array([1e-3, 0.25, 5e-12])
    free = M.lm_solve(cur[1], lam0[1] * 10.0, (np.inf,) * 6)
    assert (np.abs(free[:3]) < 1e-3).all() and free[:3].all()
    free = M.lm_solve(trial[2], 1e-12, (np.inf,) * 6)
    assert (np.abs(free) > np.asarray(max_step)).all()
    lm = L.gsd_icp_lm()
    lm.down, lm.up, lm.lambda_min, lm.lambda_max, lm.first = 0.1, 10.0, 1e-12, 1e12, 0
    lm.max_step[:] = max_step
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    state, lam, row, t_state, t_row = dev(T0), dev(lam0), dev(cur), dev(T1), dev(trial)
    trace = torch.zeros(3, dtype=torch.float64, device=DEV)
    accepted = torch.full((3,), 5, dtype=torch.int32, device=DEV)
    last = torch.zeros((3, 6), dtype=torch.float64, device=DEV)
    assert L.lib.gsd_mesh_icp_lm_update(C.byref(lm), 3, state.data_ptr(), lam.data_ptr(), row.data_ptr(), t_state.data_ptr(), t_row.data_ptr(),
                                        trace.data_ptr(), accepted.data_ptr(), last.data_ptr(), L.stream_ptr()) == L.GSD_OK
    same = lambda got, want: np.array_equal(got.cpu().numpy().reshape(-1).view(np.int64), np.asarray(want, np.float64).reshape(-1).view(np.int64))
    for i in range(3):
        s, nxt, step = M.lm_update({"T": T0[i], "lam": float(lam0[i]), "row": cur[i], "accepted": 5}, T1[i], trial[i], max_step=max_step)
        assert s["accepted"] == int(accepted[i]) == (5 if i == 1 else 6), i
        assert same(state[i], s["T"]) and same(lam[i], s["lam"]) and same(row[i], s["row"]) and same(trace[i], s["row"][0]), i
        assert same(last[i], step) and same(t_state[i], nxt), (i, last[i].cpu().numpy(), step)
        if i == 0:
            assert not step.any() and same(t_state[i], T1[i])
        if i == 2:
            assert np.array_equal(step, max_step)
