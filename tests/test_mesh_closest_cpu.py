"""CPU: the fp64 twins of DESIGN.md section 23 (tests/mesh_closest_ref.py) against hand-computed values, and the host-only part of
the gsd_mesh_volume_* / gsd_mesh_icp_* ABI.  No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np

import mesh_closest_ref as M
import mesh_depth_ref as R
from conftest import REPO


# triangle 0 of box(): a = (-3, -2, -2.5), b = (-3, -2, 2.5), c = (-3, 2, 2.5), in the plane x = -3, the right angle at b.
REGIONS = (            # point, closest point, d^2: small integers and halves, every operation of the twin is exact on them
    ("face, above", (-4.0, -1.0, 1.25), (-3.0, -1.0, 1.25), 1.0),
    ("face, on it", (-3.0, -1.0, 1.25), (-3.0, -1.0, 1.25), 0.0),
    ("vertex a, beyond the corner", (-3.5, -3.0, -4.0), (-3.0, -2.0, -2.5), 3.5),
    ("vertex b, beyond the corner", (-2.0, -4.0, 4.0), (-3.0, -2.0, 2.5), 7.25),
    ("vertex c, beyond the corner", (-3.0, 3.0, 3.5), (-3.0, 2.0, 2.5), 2.0),
    ("vertex a, exactly", (-3.0, -2.0, -2.5), (-3.0, -2.0, -2.5), 0.0),
    ("edge ab, beside", (-3.0, -4.0, 0.0), (-3.0, -2.0, 0.0), 4.0),
    ("edge ab, on it", (-3.0, -2.0, 0.0), (-3.0, -2.0, 0.0), 0.0),
    ("edge bc, beside", (-3.0, 0.0, 4.5), (-3.0, 0.0, 2.5), 4.0),
    ("edge ac, beside", (-3.0, 2.5, -2.0), (-3.0, 0.0, 0.0), 10.25),
    ("edge ac, above and beside", (-5.0, 2.5, -2.0), (-3.0, 0.0, 0.0), 14.25),
)


def test_every_region_of_a_triangle_gives_the_hand_computed_point_exactly():
    v = M.vertices(R.box())
    a, b, c = v[0, 0], v[0, 1], v[0, 2]
    assert np.array_equal(a, (-3, -2, -2.5)) and np.array_equal(b, (-3, -2, 2.5)) and np.array_equal(c, (-3, 2, 2.5))
    for what, p, want, d2 in REGIONS:
        x, got = M.on_triangles(a, b, c, np.asarray(p))
        assert np.array_equal(x, np.asarray(want)) and got == d2, (what, x, got)
        # every labelling of the same triangle finds the same point
        for perm in ((b, c, a), (c, a, b), (a, c, b)):
            x2, got2 = M.on_triangles(*perm, np.asarray(p))
            assert np.array_equal(x2, np.asarray(want)) and got2 == d2, (what, "permuted", x2, got2)


def test_brute_force_on_the_box_picks_the_lowest_id_among_ties_and_pruning_changes_nothing():
    tri = R.box()
    # a corner belongs to several triangles with d^2 = 0: the lowest id wins; the centre of the +x face's diagonal ties its two
    pts = np.array([(-3, -2, -2.5), (3, 2, 2.5), (3, 0, 0), (10, 0, 0), (0, 0, 0), (np.nan, 0, 0), (0, np.inf, 0)], np.float32)
    tid, x, d2, second = M.closest_brute(tri, pts)
    v = M.vertices(tri)
    on = lambda p: [t for t in range(12) if M.on_triangles(v[t, 0], v[t, 1], v[t, 2], np.asarray(p, float))[1] == 0.0]
    assert tid[0] == min(on((-3, -2, -2.5))) == 0 and tid[1] == min(on((3, 2, 2.5))) and tid[2] == min(on((3, 0, 0))) == 2
    assert np.array_equal(d2[:5], (0, 0, 0, 49, 4)) and np.array_equal(x[3], (3, 0, 0)) and np.array_equal(second[:3], (0, 0, 0))
    assert np.array_equal(tid[5:], (-1, -1)) and np.isnan(x[5:]).all() and np.isinf(d2[5:]).all()
    # D: a winner needs d^2 <= D^2, equality included
    assert np.array_equal(M.closest_brute(tri, pts, D=2.0)[0][:5] >= 0, (True, True, True, False, True))
    assert np.array_equal(M.closest_brute(tri, pts, D=0.0)[0][:5] >= 0, (True, True, True, False, False))
    rng = np.random.Generator(np.random.PCG64(5))
    for mesh in (R.sphere(2), R.torus(), R.l_prism()):
        q = (rng.random((400, 3)) - 0.5) * 14
        got, ref = M.closest_brute(mesh, q, prune=True), M.closest_brute(mesh, q, prune=False)
        assert all(np.array_equal(g, r) for g, r in zip(got[:3], ref[:3]))


def test_a_degenerate_triangle_is_skipped():
    tri = R.l_prism()
    v = M.vertices(tri)
    assert np.array_equal(np.nonzero(M.skipped(v))[0], [20])
    far = v[20].mean(axis=0)          # on the degenerate triangle itself
    tid, _, d2, _ = M.closest_brute(tri, far[None])
    assert tid[0] != 20 and tid[0] >= 0 and d2[0] > 1.0
    only = np.repeat(tri[20:21], 3, axis=0)
    tid, x, d2, _ = M.closest_brute(only, far[None])
    assert tid[0] == -1 and np.isnan(x).all() and np.isinf(d2[0])


def face_cloud():
    """Points on the six faces of box(), at least 0.5 mm from every edge, on a lattice of quarters."""
    pts = []
    for axis, half in enumerate((3.0, 2.0, 2.5)):
        others = [k for k in range(3) if k != axis]
        h = [(3.0, 2.0, 2.5)[k] - 0.5 for k in others]
        for s in (-half, half):
            for u in np.arange(-h[0], h[0] + 0.01, 0.75):
                for w in np.arange(-h[1], h[1] + 0.01, 0.75):
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[others[0]], p[others[1]] = s, u, w
                    pts.append(p)
    return np.asarray(pts, np.float32)


def test_one_point_to_plane_step_returns_a_small_translation_along_a_face_normal():
    tri, cloud = R.box(), face_cloud()
    delta = 2.0 ** -7
    T = M.as12(M.rigid((delta, 0.0, 0.0), (0, 0, 1), 0.0))
    row, _ = M.icp_row(tri, cloud, T, kind="plane")
    assert row[1] == len(cloud)
    on_x = int((np.abs(cloud[:, 0]) == 3).sum())
    assert abs(row[0] - on_x * delta * delta) < 1e-15 and abs(row[2] - row[0]) < 1e-15      # only the x faces see the shift
    xi = M.lm_solve(row, 0.0, (1.0,) * 6)
    assert np.abs(xi - (-delta, 0, 0, 0, 0, 0)).max() < 1e-12, xi
    state, trial, step = M.lm_update({"T": T, "lam": 1e-3, "row": None, "accepted": 0}, T, row, first=True, max_step=(1.0,) * 6)
    assert np.abs(trial - M.as12(np.eye(4))).max() < 1e-4 and state["accepted"] == 0 and state["lam"] == 1e-3
    # the point kind's cost is the same function; its step slides along the faces as well and is damped by them
    row_p, _ = M.icp_row(tri, cloud, T, kind="point")
    assert row_p[0] == row[0] and row_p[2] == row[0]
    # the truncation: with D below delta nothing is active and the cost is D^2 per point on the x faces, 0 elsewhere
    row_d, _ = M.icp_row(tri, cloud, T, D=delta / 2, kind="plane")
    assert row_d[1] == len(cloud) - on_x and row_d[0] == on_x * (delta / 2) ** 2 and not row_d[2:9].any()


def test_lm_update_rejects_a_worse_trial_and_a_nan_and_the_twist_composes():
    row = np.zeros(M.ROW)
    row[0] = 2.0
    for q, (j, k) in enumerate(M.PAIRS):
        row[9 + q] = 1.0 if j == k else 0.0
    row[3:9] = (0.5, 0, 0, 0, 0, 0.05)
    s0 = {"T": M.as12(np.eye(4)), "lam": 1e-3, "row": row, "accepted": 2}
    for bad in (2.0, 3.0, np.nan):
        trial_row = row.copy()
        trial_row[0] = bad
        s, nxt, step = M.lm_update(s0, M.as12(M.rigid((9, 9, 9), (1, 0, 0), 1.0)), trial_row)
        assert s["accepted"] == 2 and np.isclose(s["lam"], 1e-2, rtol=1e-15) and np.array_equal(s["T"], s0["T"])
    better = row.copy()
    better[0] = 1.5
    s, nxt, step = M.lm_update(s0, M.as12(np.eye(4)), better)
    assert s["accepted"] == 3 and np.isclose(s["lam"], 1e-4, rtol=1e-15) and np.allclose(step, (0.5 / 1.0001, 0, 0, 0, 0, 0.05 / 1.0001), rtol=1e-14)
    vx, th = -0.5 / 1.0001, -0.05 / 1.0001
    want = M.rigid((vx * np.sin(th) / th, vx * (1 - np.cos(th)) / th, 0), (0, 0, 1), th)
    assert np.abs(M.as44(nxt) - want).max() < 1e-15
    # a twist with translation and rotation: exp against the closed form of a screw about z
    E, u = M.twist_exp((0.3, 0.0, 0.2, 0.0, 0.0, 0.5))
    assert np.abs(E - M.rigid((0, 0, 0), (0, 0, 1), 0.5)[:3, :3]).max() < 1e-15
    assert np.abs(u - (0.3 * np.sin(0.5) / 0.5, 0.3 * (1 - np.cos(0.5)) / 0.5, 0.2)).max() < 1e-15
    E, u = M.twist_exp((0.3, 0.1, 0.2, 1e-9, 0.0, 0.0))          # the series branch
    assert np.abs(u - (0.3, 0.1, 0.2)).max() < 1e-9 and abs(E[2, 1] - 1e-9) < 1e-24
    # a singular system gives no step
    assert not M.lm_solve(np.zeros(M.ROW), 1e-3, (1.0,) * 6).any()


def test_host_only_abi_calls():
    import __graft_entry__ as ge
    ge.build()
    from gelslim_depth_amd import _lib as L
    lib = L.lib
    header = open(os.path.join(REPO, "include", "gsd.h")).read()
    assert L.GSD_ICP_ROW == 30 == M.ROW == int(re.search(r"#define GSD_ICP_ROW (\d+)", header).group(1))
    assert C.sizeof(L.gsd_icp_lm) == 4 * 8 + 6 * 8 + 2 * 4 and L.gsd_icp_lm.max_step.offset == 32 and L.gsd_icp_lm.first.offset == 80
    assert L.gsd_icp_lm.reserved.offset == 84
    assert C.sizeof(L.gsd_mesh_volume) == 8 * 8 + 4 * 4 and L.gsd_mesh_volume.cell.offset == 48 and L.gsd_mesh_volume.nx.offset == 64
    assert L.gsd_mesh_volume.reserved.offset == 76
    q = lib.gsd_mesh_icp_rows_workspace
    assert (q(0, 1), q(1, 0), q(-5, 3), q(1, 1), q(256, 2), q(257, 2), q(5000, 3)) == (0, 0, 0, 30, 60, 120, 20 * 3 * 30)
    assert q(2 ** 31 - 1, 2 ** 9) == 0          # 2^31 blocks or more
    vol = L.gsd_mesh_volume()
    assert lib.gsd_mesh_volume_workspace(None) == 0 and lib.gsd_mesh_volume_workspace(C.byref(vol)) == 0
    box = lambda *v: (C.c_double * 6)(*v)
    assert lib.gsd_mesh_volume_plan(box(-3, -2, -2.5, 3, 2, 2.5), 1.0, C.byref(vol)) == L.GSD_OK
    assert (vol.nx, vol.ny, vol.nz, vol.cell, vol.reserved) == (7, 5, 6, 1.0, 0)
    assert vol.x0 < -3 < 3 < vol.x1 and vol.y0 < -2 < 2 < vol.y1 and vol.z0 < -2.5 < 2.5 < vol.z1 and vol.x1 == vol.x0 + 7.0
    assert lib.gsd_mesh_volume_workspace(C.byref(vol)) == 2 + 2 * 210 + 1
    # the side is enlarged to fit 2^24 cells and 1024 per axis; a flat or a point-like box still has one cell per flat axis
    assert lib.gsd_mesh_volume_plan(box(0, 0, 0, 100, 100, 100), 0.01, C.byref(vol)) == L.GSD_OK
    assert vol.nx * vol.ny * vol.nz <= 1 << 24 and vol.cell > 100 / 257 and max(vol.nx, vol.ny, vol.nz) <= 1024
    assert lib.gsd_mesh_volume_plan(box(0, 0, 0, 1e4, 1, 0), 0.01, C.byref(vol)) == L.GSD_OK
    assert vol.nx <= 1024 and vol.nz == 1 and vol.nx * vol.ny * vol.nz <= 1 << 24
    assert lib.gsd_mesh_volume_plan(box(1, 1, 1, 1, 1, 1), 0.5, C.byref(vol)) == L.GSD_OK and (vol.nx, vol.ny, vol.nz) == (1, 1, 1)
    for bad in (box(0, 0, 0, -1, 1, 1), box(0, 0, 0, 1, float("nan"), 1), box(0, 0, 0, float("inf"), 1, 1)):
        assert lib.gsd_mesh_volume_plan(bad, 1.0, C.byref(vol)) == L.GSD_ERR_BAD_ARG
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.gsd_mesh_volume_plan(box(0, 0, 0, 1, 1, 1), cell, C.byref(vol)) == L.GSD_ERR_BAD_ARG
    assert lib.gsd_mesh_volume_plan(None, 1.0, C.byref(vol)) == L.GSD_ERR_BAD_ARG


def test_the_default_cell_size_model():
    from gelslim_depth_amd.mesh_register import default_cell_mm_3d, triangle_cross
    v = M.vertices(R.sphere(4))
    cell = default_cell_mm_3d(v)
    edge = np.linalg.norm(v[:, 1] - v[:, 0], axis=1).mean()
    assert 0.5 * edge < cell < 2.0 * edge          # about one facet edge: some 8 entries per occupied cell
    assert np.array_equal(triangle_cross(v), M.cross(v))
    flat = np.repeat(R.l_prism()[20:21], 2, axis=0)          # only degenerate triangles: the extent itself
    assert default_cell_mm_3d(M.vertices(flat)) > 0


def test_the_query_cases_have_few_near_ties_and_pruning_changes_nothing_on_them():
    """test_gpu_mesh_closest compares bit for bit.  Should a device division ever round differently, only points whose two best d^2
    lie within 4 ulp without being equal could change their winner (exact ties are resolved by id on both sides).  These are random
    points whose nearest surface point lies on an edge or a vertex that two facets reach by differently rounded routes: 2.5 to 5 %
    of the 700 random points of the torus, depending on the seed, and none of the other points.  The seeds of query_points are
    chosen so that every mesh stays under 1 % of its inputs (torus 19 of 2,366, sphere 14 of 1,856, pattern_32 27 of 7,080).
    The GPU test rests on the pruned twin: on every one of its inputs the pruned and the unpruned brute force must agree in every
    bit (pattern_32: every fourth point)."""
    for name in M.QUERY_MESHES:
        tri, scale = M.query_mesh(name)
        pts = np.concatenate(list(M.query_points(name).values()))
        tid, x, d2, second = M.closest_brute(tri, pts, pc_scale=scale)
        ties = M.near_ties(d2, second)
        print(f"{name}: {len(pts)} points, {int((second == d2).sum())} exact ties, {int(ties.sum())} near ties ({ties.mean():.4f})")
        assert (tid >= 0).all() and (second == d2).sum() >= len(M.query_points(name)["vertices"])
        assert ties.mean() < 0.01, (name, int(ties.sum()), len(pts))
        step = 4 if name == "pattern_32" else 1
        full = M.closest_brute(tri, pts[::step], pc_scale=scale, prune=False)
        assert np.array_equal(full[0], tid[::step]) and np.array_equal(full[1], x[::step]) and np.array_equal(full[2], d2[::step]), name


def test_the_twin_registration_converges_on_the_gpu_cases():
    """The cases of test_gpu_mesh_register, measured here: the twin's recovered-transform error and final rms are the constants
    that file takes its bounds from (mesh_closest_ref.TWIN)."""
    for (name, kind, D, outliers), (want_err, want_rms) in M.TWIN.items():
        tri, cloud = M.case_cloud(name, outliers)
        r = M.register(tri, cloud, None, 20, D, kind)
        err = M.corner_gap(r["matrix"] @ M.T0, np.eye(4), tri)
        print(f"{name} {kind} D={D} outliers={outliers}: error {err:.3e} mm (recorded {want_err:.3e}), rms {r['rms']:.3e} mm (recorded "
              f"{want_rms:.3e}), {r['active']} active, {r['accepted']} accepted, cost {r['trace'][0]:.3e} -> {r['trace'][-1]:.3e}")
        assert (np.diff(r["trace"]) <= 0).all() and (r["active"] == len(cloud)) == (D is None)
        assert 0.5 * want_err <= err <= 2.0 * want_err and 0.5 * want_rms <= r["rms"] <= 2.0 * want_rms
        if kind == "plane" and D is None:
            assert err < 1e-6 and r["rms"] < 1e-6          # the floor is the fp32 rounding of the cloud, some 1e-7 mm
        if D is not None:      # the limit is what recovers the motion: without it the outliers drag the fit five times as far off
            free = M.register(tri, cloud, None, 20, None, kind)
            assert M.corner_gap(free["matrix"] @ M.T0, np.eye(4), tri) > 3 * want_err and err < 0.05


def test_registration_kernels_use_no_scratch():
    """The 6 x 6 system of mesh_icp_lm_update (gsd_lm_solve<6>) is indexed by constants only and the 30 sums of mesh_icp_rows_sum
    stay in registers: neither kernel has scratch or LDS (device-only compile, a few seconds)."""
    import re
    import shutil
    import subprocess
    from gelslim_depth_amd import build as b
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this machine")
    r = subprocess.run([hipcc] + b.CFLAGS + [f"-I{b.INCLUDE}", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(b.CSRC, "gsd_mesh_closest.hip"), "-o", os.devnull], capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(lds)
    got = {}
    for key in ("mesh_icp_lm_update", "mesh_icp_rows_sum", "mesh_volume_scan"):
        hits = [(s, m) for n, s, m in zip(names, scratch, lds) if re.search(rf"\d{key}E", n)]
        assert len(hits) == 1, (key, names)
        got[key] = hits[0]
    assert got == {"mesh_icp_lm_update": (0, 0), "mesh_icp_rows_sum": (0, 0), "mesh_volume_scan": (0, 16 * 8)}, got
