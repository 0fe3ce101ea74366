"""GPU: the refinement past the lattice: gsd_mesh_depth_render_jacobian, gsd_mesh_pose_normal,
gsd_mesh_pose_lm_update, refine_pose and estimate_pose(refine_iterations).

The yardsticks are not the code under test: the Jacobian images are held point by point to the brute-force fp64 twin
(tests/mesh_pose_refine_ref.py) on the points it is certain about, entry 0 and 1 of a normal row to score_poses' bits, the other
14 entries to an fp64 host reduction of the Jacobian images the first test has pinned, the damped step to lm_update_ref.  The
refinements are held to the twin's own error, section 17's rule:

    BOUND = 3 * max(refine_twin's recorded error, delta-equivalent) per axis

with delta = 16 * 2^-23 * coord_max mm (raster_ref's position uncertainty) for the translations and delta / (the mesh's largest
in-plane half-extent) rad for the angle; the margin of 3 because fp32 edge pixels may move an iterate within that scale."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_depth_ref as R
import mesh_pose_ref as P
import mesh_pose_refine_ref as PR
import mesh_pose_width_ref as PW
from test_gpu_mesh_pose import DEV, HEIGHT_MM, grid_of, mesh, problem
from test_gpu_mesh_pose_width import same_bits, widths_of
from test_mesh_pose_refine_cpu import REFINED_TWIN_ERROR, REFINED_TWIN_WIDTH_ERROR, spd_row

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def md():
    from gelslim_depth_amd import mesh_depth
    return mesh_depth


@functools.lru_cache(maxsize=None)
def twin_image(name):
    return PR.image_terms(name)[1]


# ---- 1. the Jacobian image against the twin -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lprism", "sphere4", "ellipsoid"])
def test_jacobian_images_equal_the_twin_point_by_point(name):
    mesh_name, size, pose, flip, invert = PR.IMAGES[name]
    t = twin_image(name)
    grid = grid_of(mesh_name)
    poses = torch.tensor([pose], dtype=torch.float32, device=DEV)
    widths = torch.tensor([P.contact_width(mesh(mesh_name))], dtype=torch.float32, device=DEV)
    J = md().render_depth_jacobian(grid, poses, widths, size, HEIGHT_MM, 0.0, flip, invert)
    assert J.shape == (1, 2, 3, *size) and J.dtype == torch.float64
    J = J[0].cpu().numpy()
    depth = md().render_depth(grid, poses, widths, size, HEIGHT_MM, 0.0, flip, invert)[0].cpu().numpy()
    certain = ~t["uncertain"]
    active = int(t["active"].sum())
    left_out = int((t["uncertain"] & t["active"]).sum())
    assert active >= 80 and left_out <= PR.UNCERTAIN_CAP * active, (active, left_out)
    assert np.array_equal((depth < 0)[certain], t["active"][certain])
    assert not J[np.broadcast_to((depth == 0)[:, None], J.shape)].any()          # every inactive point: exactly 0
    diff, tol = np.abs(J - t["J"]), 64 * EPS * t["mag"]
    mask = np.broadcast_to(certain[:, None], J.shape)
    worst = (diff[mask] / np.maximum(tol[mask], 1e-300)).max() if name != "lprism" else diff[mask].max()
    print(f"{name}: {active} active points, {left_out} left out, largest |J| {np.abs(J).max():.3f}, worst |J - twin| / bound {worst:.3e}")
    assert np.all(diff[mask] <= tol[mask])
    if name == "lprism":          # flat caps: the depth does not depend on the pose where it is not 0
        assert not J.any()
    else:
        assert all(np.abs(J[ch, k]).max() > 0.05 for ch in range(2) for k in range(3))


# ---- 2. entry 0 and 1 are score_poses' bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size,flip,invert", [("lprism", (24, 31), False, False), ("sphere4", (40, 53), True, False),
                                                   ("ellipsoid", (40, 53), False, True), ("ellipsoid", (24, 31), True, True)])
def test_entry_0_is_sum_sq_and_entry_1_n_rendered_bit_for_bit(name, size, flip, invert):
    observed, cand, widths = problem(name, size, flip, invert)
    for stride in (1, 2, 3):
        rows = md().pose_normal_rows(grid_of(name), observed, cand, widths, HEIGHT_MM, 0.0, flip, invert, stride)
        assert rows.shape == (2, 37, 16) and rows.dtype == torch.float64 and bool(torch.isfinite(rows).all())
        score = md().score_poses(grid_of(name), observed, cand, widths, HEIGHT_MM, 0.0, flip, invert, stride, 0.0)
        assert torch.equal(rows[..., 0], score[..., 0]) and torch.equal(rows[..., 1], score[..., 3]), (name, stride)
        assert bool((rows[..., 1] > 0).any()) and bool((rows[..., 0] > 0).all())


def test_one_width_per_candidate():
    name, size = "ellipsoid", (40, 53)
    observed, cand, _ = problem(name, size)
    wg = widths_of(name, 3)          # (2, 3): one column holds a 0, another a width at which nothing touches
    per = wg[:, torch.arange(37, device=DEV) % 3].contiguous()          # (2, 37)
    for stride in (1, 2):
        rows = md().pose_normal_rows(grid_of(name), observed, cand, per, HEIGHT_MM, stride=stride)
        score = md().score_poses_widths(grid_of(name), observed, cand, wg, HEIGHT_MM, stride=stride)
        want = torch.stack([score[:, p, p % 3] for p in range(37)], dim=1)
        assert torch.equal(rows[..., 0], want[..., 0]) and torch.equal(rows[..., 1], want[..., 3])
        assert bool((rows[1, 2::3, 1] == 0).all()) and not bool(rows[1, 2::3, 2:].any())          # nothing touches: no active point, no J
        for k in range(3):          # the columns equal a call with that width for every candidate
            alone = md().pose_normal_rows(grid_of(name), observed, cand, wg[:, k].contiguous(), HEIGHT_MM, stride=stride)
            assert torch.equal(alone[:, k::3], rows[:, k::3])


# ---- 3. entries 2..15 against the host reduction of the pinned images ------------------------------------------------------------
@pytest.mark.parametrize("name,size,flip,invert", [("sphere4", (40, 53), True, False), ("ellipsoid", (40, 53), False, True),
                                                   ("ellipsoid", (24, 31), False, False)])
def test_rows_equal_the_jacobian_images_reduced_in_fp64(name, size, flip, invert):
    """The same terms in another order: per entry |difference| <= 2 n 2^-53 sum |terms|, n the lattice points."""
    observed, cand, widths = problem(name, size, flip, invert)
    b, p = cand.shape[:2]
    flat, w_flat = cand.reshape(-1, 3).contiguous(), widths.repeat_interleave(p).contiguous()
    J = md().render_depth_jacobian(grid_of(name), flat, w_flat, size, HEIGHT_MM, 0.0, flip, invert).reshape(b, p, 2, 3, *size).cpu().numpy()
    depth = md().render_depth(grid_of(name), flat, w_flat, size, HEIGHT_MM, 0.0, flip, invert).reshape(b, p, 2, *size).cpu().numpy()
    seen = observed.cpu().numpy()
    for stride in (1, 2, 3):
        got = md().pose_normal_rows(grid_of(name), observed, cand, widths, HEIGHT_MM, 0.0, flip, invert, stride).cpu().numpy()
        n = P.n_points(size[0], size[1], stride)
        worst = 0.0
        for i in range(b):
            for k in range(p):
                terms = PR.normal_terms(depth[i, k], J[i, k], seen[i], stride)
                assert terms.shape == (16, n)
                want, scale = terms.sum(axis=1), np.abs(terms).sum(axis=1)
                assert got[i, k, 1] == want[1]
                assert np.all(np.abs(got[i, k] - want) <= 2 * n * EPS * scale), (name, stride, i, k)
                worst = max(worst, float((np.abs(got[i, k] - want) / np.maximum(scale, 1e-300)).max()))
        assert np.abs(got[..., 2:5]).max() > 0 and (got[..., 6:9] > 0).any()
        print(f"{name} {size} stride {stride}: worst |row - host| / sum |terms| {worst:.3e} (bound {2 * n * EPS:.3e})")


# ---- 4. batch independence, non-finite input, refusals ----------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch_and_repeat_bitwise():
    for name, size, stride in (("sphere4", (40, 53), 1), ("ellipsoid", (24, 31), 2)):
        observed, cand, widths = problem(name, size)
        rows = lambda o, c, w: md().pose_normal_rows(grid_of(name), o, c, w, HEIGHT_MM, stride=stride)
        full = rows(observed, cand, widths)
        assert torch.equal(full, rows(observed, cand, widths))
        assert torch.equal(rows(observed, cand[:, :5].contiguous(), widths), full[:, :5])
        assert torch.equal(rows(observed, cand[:, 11:12].contiguous(), widths), full[:, 11:12])
        assert torch.equal(rows(observed[1:2].contiguous(), cand[1:2].contiguous(), widths[1:2].contiguous())[0], full[1])


def test_non_finite_pixels_and_refused_widths():
    name, size = "ellipsoid", (24, 31)
    observed, cand, widths = problem(name, size)
    rows = lambda o, w, **kw: md().pose_normal_rows(grid_of(name), o, cand, w, HEIGHT_MM, stride=3, **kw)
    clean = rows(observed, widths)
    on, off = observed.clone(), observed.clone()
    on[0, 1, 10, 13] = float("nan")          # rows and columns 1, 4, 7, 10, 13, ...: on the stride-3 lattice
    on[1, 0, 7, 16] = float("-inf")
    off[0, 1, 11, 14] = float("nan")
    got = rows(on, widths)
    assert bool(got[0, :, 0].isnan().all()) and bool(got[1, :, 0].isinf().all()) and not bool(torch.isfinite(got[..., 2:6]).all())
    assert torch.equal(got[..., 1], clean[..., 1]) and torch.equal(got[..., 6:], clean[..., 6:])          # J does not see D
    assert torch.equal(rows(off, widths), clean)
    bad = widths.clone()
    bad[1] = -1.0
    refused = rows(observed, bad, validate=False)
    assert bool(refused[1].isnan().all()) and torch.equal(refused[0], clean[0])
    per = widths[:, None].expand(2, 37).clone()
    per[0, 5] = float("nan")
    refused = rows(observed, per, validate=False)
    assert bool(refused[0, 5].isnan().all()) and same_bits(refused[0, :5], clean[0, :5]) and torch.equal(refused[0, 6:], clean[0, 6:])
    out = torch.full((2, 37, 16), 7.0, dtype=torch.float64, device=DEV)
    for w in (bad, per, widths[:1], widths.double(), torch.zeros((2, 36), device=DEV)):
        with pytest.raises(md().MeshDepthError):
            rows(observed, w, out=out)
    with pytest.raises(md().MeshDepthError):
        md().pose_normal_rows(grid_of(name), observed, cand, widths, HEIGHT_MM, stride=0, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_the_library_refuses_bad_arguments_before_any_launch():
    from gelslim_depth_amd import _lib as L
    grid = grid_of("lprism")
    observed, cand, _ = problem("lprism", (24, 31))
    widths = torch.full((2, 37), P.contact_width(mesh("lprism")), dtype=torch.float32, device=DEV)
    view = L.gsd_mesh_view()
    view.mpp, view.width_offset, view.swap_axes = HEIGHT_MM / 24, 0.0, grid.swap_axes
    query = L.lib.gsd_mesh_pose_normal_workspace
    need = int(query(2, 37, 24, 31, 2))
    assert L.GSD_POSE_NORMAL_ROW == 16 and need == 2 * 37 * 4 + 2 * 37 * 2 * 16          # pose table | one tile per channel
    rows = torch.full((2, 37, 16), 7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros((need,), dtype=torch.float64, device=DEV)

    def call(b=2, p=37, h=24, w=31, stride=2, elems=need, rows_ptr=None, wid=None):
        return L.lib.gsd_mesh_pose_normal(C.byref(grid.grid), C.byref(view), grid.records.data_ptr(), grid.triangles, grid.cells.data_ptr(),
                                          grid.list.data_ptr(), grid.list.numel(), observed.data_ptr(), b, cand.data_ptr(),
                                          widths.data_ptr() if wid is None else wid, p, h, w, stride, rows.data_ptr() if rows_ptr is None else rows_ptr,
                                          ws.data_ptr(), elems, L.stream_ptr())
    for kw in ({"elems": need - 1}, {"stride": 0}, {"p": 0}, {"b": 0}, {"h": 0}, {"rows_ptr": 0}, {"wid": 0}, {"rows_ptr": rows.data_ptr() + 4},
               {"b": 1 << 15, "p": 1 << 15, "h": 64, "w": 64, "stride": 1}):
        assert call(**kw) == L.GSD_ERR_BAD_ARG, kw
        assert "gsd_mesh_pose_normal" in L.lib.gsd_last_error().decode()
    assert query(2, 37, 24, 31, 0) == 0 and query(0, 37, 24, 31, 2) == 0 and query(1 << 15, 1 << 15, 64, 64, 1) == 0
    jac = torch.full((1, 2, 3, 24, 31), 7.0, dtype=torch.float64, device=DEV)
    tab = torch.zeros((8,), dtype=torch.float32, device=DEV)
    for n, h, elems, code in ((0, 24, 8, L.GSD_ERR_BAD_ARG), (1, 0, 8, L.GSD_ERR_BAD_ARG), (1, 24, 7, L.GSD_ERR_WORKSPACE)):
        assert L.lib.gsd_mesh_depth_render_jacobian(C.byref(grid.grid), C.byref(view), grid.records.data_ptr(), grid.triangles,
                                                    grid.cells.data_ptr(), grid.list.data_ptr(), grid.list.numel(), cand.data_ptr(),
                                                    widths.data_ptr(), n, h, 31, jac.data_ptr(), tab.data_ptr(), elems, L.stream_ptr()) == code
    lm = L.gsd_pose_lm()
    lm.down, lm.up, lm.lambda_min, lm.lambda_max, lm.free_mask = 0.1, 10.0, 1e-12, 1e12, 7
    state = torch.full((64,), 7.0, dtype=torch.float64, device=DEV)
    ptr = state.data_ptr()

    def update(b=1, first=None):
        return L.lib.gsd_mesh_pose_lm_update(C.byref(lm), b, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr if first is None else first,
                                             L.stream_ptr())
    assert update(b=0) == L.GSD_ERR_BAD_ARG and update(first=0) == L.GSD_ERR_BAD_ARG
    for field, value in (("free_mask", 5), ("free_mask", 23), ("down", 0.0), ("down", 2.0), ("up", 0.5), ("lambda_min", -1.0), ("lambda_max", 1e-13)):
        keep = getattr(lm, field)
        setattr(lm, field, value)
        assert update() == L.GSD_ERR_BAD_ARG, (field, value)
        assert "gsd_mesh_pose_lm_update" in L.lib.gsd_last_error().decode()
        setattr(lm, field, keep)
    lm.max_step[2] = -1.0
    assert update() == L.GSD_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((rows == 7.0).all()) and bool((jac == 7.0).all()) and bool((state == 7.0).all())
    assert call() == L.GSD_OK
    assert torch.equal(rows, md().pose_normal_rows(grid, observed, cand, widths, HEIGHT_MM, stride=2))


# ---- 5. the damped step against lm_update_ref ---------------------------------------------------------------------------------------
def test_lm_update_equals_the_twin():
    """Seeded SPD rows; per problem one of: accepted trial, rejected trial (equal cost, higher cost, NaN cost), a failing pivot, and
    a clip that bites; once with the width masked and once with it free.  The accept decision, lambda and the counters are exact;
    the step is within 64 kappa 2^-53 of the twin's in relative norm, kappa the condition number of the damped matrix."""
    from gelslim_depth_amd import _lib as L
    rng = np.random.Generator(np.random.PCG64(21))
    n = 12
    cur = np.stack([spd_row(rng, 1.0 + k)[0] for k in range(n)])
    trial = np.stack([spd_row(rng, 1.0 + k)[0] for k in range(n)])
    trial[:, 0] = cur[:, 0] * np.where(np.arange(n) % 2 == 0, 0.5, 1.5)          # even: accepted, odd: rejected
    trial[3, 0], trial[5, 0] = cur[3, 0], np.nan                                  # equal: rejected, NaN: rejected
    trial[4, 6 + PR.PAIRS.index((2, 2))] = -1.0                                   # accepted, then its pivot fails
    cur[7, 6 + PR.PAIRS.index((0, 0))] = 0.0                                      # rejected, the old row's pivot fails
    pose0 = (rng.uniform(-1, 1, (n, 3)) * np.array([1e-3, 1e-3, 1.0])).astype(np.float32)
    pose1 = (pose0 + rng.uniform(-1, 1, (n, 3)).astype(np.float32) * np.float32(1e-4)).astype(np.float32)
    width0 = rng.uniform(4, 6, n).astype(np.float32)
    width1 = (width0 + np.float32(0.01)).astype(np.float32)
    lam0 = 10.0 ** rng.uniform(-6, 0, n)
    lam0[0], lam0[1] = 5e-12, 5e11                                                 # both bounds bite
    for mask, max_step in ((7, (0.5, 0.5, 0.1, 0.5)), (15, (0.5, 0.5, 0.1, 0.5)), (15, (1e-3, 1e9, 2e-3, 1e-4)), (7, (1e9,) * 4)):
        lm = L.gsd_pose_lm()
        lm.down, lm.up, lm.lambda_min, lm.lambda_max, lm.free_mask, lm.first = 0.1, 10.0, 1e-12, 1e12, mask, 0
        lm.max_step[:] = max_step
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        pose, width, lam, row = dev(pose0), dev(width0), dev(lam0), dev(cur)
        t_pose, t_width, t_row = dev(pose1), dev(width1), dev(trial)
        trace = torch.zeros(n, dtype=torch.float64, device=DEV)
        accepted = torch.full((n,), 3, dtype=torch.int32, device=DEV)
        last = torch.zeros((n, 4), dtype=torch.float64, device=DEV)
        assert L.lib.gsd_mesh_pose_lm_update(C.byref(lm), n, pose.data_ptr(), width.data_ptr(), lam.data_ptr(), row.data_ptr(), t_pose.data_ptr(),
                                             t_width.data_ptr(), t_row.data_ptr(), trace.data_ptr(), accepted.data_ptr(), last.data_ptr(),
                                             L.stream_ptr()) == L.GSD_OK
        got = {k: v.cpu().numpy() for k, v in dict(pose=pose, width=width, lam=lam, row=row, t_pose=t_pose, t_width=t_width, trace=trace,
                                                    accepted=accepted, last=last).items()}
        clipped = failed = 0
        for i in range(n):
            st = {"pose": pose0[i].copy(), "width": width0[i], "lam": float(lam0[i]), "row": cur[i].copy(), "accepted": 3}
            _, _, dl, took = PR.lm_update_ref(st, pose1[i], width1[i], trial[i], mask, max_step=max_step)
            assert took == (i % 2 == 0 and i not in (3, 5)), i
            assert got["accepted"][i] == st["accepted"] and got["lam"][i] == st["lam"], (i, got["lam"][i], st["lam"])
            assert np.array_equal(got["pose"][i], st["pose"]) and got["width"][i] == st["width"]
            assert same_bits(torch.from_numpy(got["row"][i]), torch.from_numpy(st["row"])) and (got["trace"][i] == st["row"][0] or np.isnan(st["row"][0]))
            step = got["last"][i]
            if not dl.any():
                failed += 1
                assert not step.any(), (i, step)
            else:
                _, M = PR.lm_solve(st["row"], st["lam"], mask, (np.inf,) * 4)
                free, _ = PR.lm_solve(st["row"], st["lam"], mask, (np.inf,) * 4)
                hit = np.abs(free) > np.asarray(max_step)
                clipped += int(hit.any())
                assert np.array_equal(step[hit], np.asarray(max_step)[hit]), (i, step)          # a clipped component is the clip, exactly
                kappa = np.linalg.cond(M)
                err = np.linalg.norm((step - np.abs(dl))[~hit]) / np.linalg.norm(dl)
                assert err <= 64 * kappa * EPS, (i, err, kappa)
                if mask == 7:
                    assert step[3] == 0.0
            signed = np.where(dl < 0, -step, step)
            want = np.asarray([np.float32(np.float64(st["pose"][0]) + signed[0] / 1000.0), np.float32(np.float64(st["pose"][1]) + signed[1] / 1000.0),
                               np.float32(np.float64(st["pose"][2]) + signed[2])], np.float32)
            assert np.array_equal(got["t_pose"][i], want) and got["t_width"][i] == np.float32(np.float64(st["width"]) + signed[3]), i
        assert failed >= 2 and (clipped >= 4 or max_step[0] != 1e-3)
    # `first`: the trial becomes the state whatever the costs, the counter restarts, lambda stays
    lm.first = 1
    assert L.lib.gsd_mesh_pose_lm_update(C.byref(lm), n, pose.data_ptr(), width.data_ptr(), lam.data_ptr(), row.data_ptr(), t_pose.data_ptr(),
                                         t_width.data_ptr(), t_row.data_ptr(), trace.data_ptr(), accepted.data_ptr(), last.data_ptr(),
                                         L.stream_ptr()) == L.GSD_OK
    assert same_bits(row, t_row) and not bool(accepted.any()) and torch.equal(lam, torch.from_numpy(got["lam"]).to(DEV))
    assert torch.equal(pose, torch.from_numpy(got["t_pose"]).to(DEV)) and same_bits(trace, t_row[:, 0])


# ---- 6. refine_pose end to end --------------------------------------------------------------------------------------------------------
def ellipsoid_problem():
    case = P.CASES["ellipsoid"]
    grid = grid_of(case["mesh"])
    truth = torch.tensor([P.case_truth(case)], dtype=torch.float32, device=DEV)
    width = torch.tensor([PW.true_width(case)], dtype=torch.float32, device=DEV)
    observed = md().render_depth(grid, truth, width, case["size"], case["height_mm"])
    tri = mesh(case["mesh"])
    delta = PR.default_delta(PR.records(tri), P.case_truth(case), case["size"], case["height_mm"])
    a, b, _, _ = R.prepare(tri, 1.0, P.PLANE)
    half = max(a.max() - a.min(), b.max() - b.min()) / 2
    equivalent = (delta, delta, delta / half)
    bound = tuple(3 * max(e, d) for e, d in zip(REFINED_TWIN_ERROR, equivalent))
    return case, grid, truth, width, observed, bound, delta


def two_steps_off(case):
    step = (1.5e-3 / 27, 1.5e-3 / 27, 0.6 / 64)          # the last level's steps of the three-level search
    return tuple(float(np.float32(t + 2 * s)) for t, s in zip(P.case_truth(case), step))


def test_refine_pose_goes_past_the_lattice():
    case, grid, truth, width, observed, bound, _ = ellipsoid_problem()
    for label, start in (("the lattice twin's end pose", PR.lattice_end(case)), ("two lattice steps off", two_steps_off(case))):
        init = torch.tensor([start], dtype=torch.float32, device=DEV)
        res = md().refine_pose(grid, observed, width, init, 10, image_height_mm=case["height_mm"])
        assert isinstance(res, md().PoseRefinement) and res.pose.shape == (1, 3) and res.pose.dtype == torch.float32
        assert res.width.shape == (1,) and res.cost.shape == (1,) and res.normal_row.shape == (1, 16) and res.trace.shape == (11, 1)
        assert res.accepted.shape == (1,) and res.accepted.dtype == torch.int32 and res.last_step.shape == (1, 4)
        trace = res.trace[:, 0].cpu().numpy()
        err = md().pose_error(res.pose, truth)[0].cpu().numpy()
        print(f"{label}: error (mm, mm, rad) {err.tolist()}, bound {bound}, trace {trace.tolist()}, accepted {int(res.accepted[0])}")
        assert np.all(np.diff(trace) <= 0) and trace[-1] == float(res.cost[0]) <= trace[0]
        start_row = md().score_poses(grid, observed, init.unsqueeze(1), width, case["height_mm"])[0, 0]
        start_cost = md().pose_cost(start_row.unsqueeze(0), "mse", md().lattice_points(case["size"], 1))          # the start's cost, score_poses' bits
        assert trace[0] == float(start_cost[0])
        assert torch.equal(res.normal_row[0, 0], md().score_poses(grid, observed, res.pose.unsqueeze(1), width, case["height_mm"])[0, 0, 0])
        assert torch.equal(res.width, width)
        assert np.all(np.abs(err) <= np.asarray(bound)), (label, err, bound)
        assert int(res.accepted[0]) >= 1


def test_refine_pose_fits_the_width_or_leaves_it_alone():
    case, grid, truth, width, observed, bound, _ = ellipsoid_problem()
    wrong = torch.tensor([PW.start_width(case)], dtype=torch.float32, device=DEV)          # 0.35 mm off
    init = torch.tensor([PR.lattice_end(case)], dtype=torch.float32, device=DEV)
    res = md().refine_pose(grid, observed, wrong, init, 10, fit_width=True, image_height_mm=case["height_mm"])
    err = md().pose_error(res.pose, truth)[0].cpu().numpy()
    w_err = float(res.width[0].double() - width[0].double())
    print(f"width 0.35 mm off, fit_width: error {err.tolist()}, width error {w_err!r} mm (the twin's {REFINED_TWIN_WIDTH_ERROR}), "
          f"trace {res.trace[:, 0].tolist()}")
    assert np.all(np.diff(res.trace[:, 0].cpu().numpy()) <= 0)
    assert np.all(np.abs(err) <= np.asarray(bound)), (err, bound)
    assert abs(w_err) <= 3 * REFINED_TWIN_WIDTH_ERROR, w_err
    fixed = md().refine_pose(grid, observed, wrong, init, 4, fit_width=False, image_height_mm=case["height_mm"])
    assert torch.equal(fixed.width, wrong) and bool((fixed.last_step[:, 3] == 0).all())
    low = md().refine_pose(grid, observed, torch.full((1,), 0.05, device=DEV), init, 4, fit_width=True, image_height_mm=case["height_mm"],
                           max_step=(0.5, 0.5, 0.1, 5.0))
    assert bool((low.width >= 0).all()) and bool(torch.isfinite(low.trace).all())          # a trial below 0 is a NaN row: rejected
    for kw in ({"cost": "l1"}, {"cost": "iou"}, {"iterations": -1}, {"iterations": 2.5}, {"damping": 0.0}, {"damping_up": 0.5}, {"damping_down": 2.0},
               {"max_step": (0.5, 0.5, 0.1)}, {"max_step": (0.5, 0.5, -0.1, 0.5)}):
        with pytest.raises(md().MeshDepthError):
            md().refine_pose(grid, observed, wrong, init, **{"iterations": 2, **kw})
    with pytest.raises(md().MeshDepthError):
        md().refine_pose(grid, observed, -wrong, init, 2)
    with pytest.raises(md().MeshDepthError):
        md().refine_pose(grid, observed, wrong, init[0, :2], 2)


def test_several_starts_give_the_best_single_start():
    case, grid, truth, width, observed, _, _ = ellipsoid_problem()
    starts = torch.tensor([[two_steps_off(case), PR.lattice_end(case), P.case_start(case)]], dtype=torch.float32, device=DEV)          # (1, 3, 3)
    both = md().refine_pose(grid, observed, width, starts, 3, image_height_mm=case["height_mm"])
    single = [md().refine_pose(grid, observed, width, starts[:, k], 3, image_height_mm=case["height_mm"]) for k in range(3)]
    costs = [float(s.cost[0]) for s in single]
    best = single[int(np.argmin(costs))]
    print(f"costs of the three starts after 3 iterations: {costs}")
    assert len(set(costs)) == 3
    for field in ("pose", "width", "cost", "normal_row", "trace", "accepted", "last_step"):
        assert torch.equal(getattr(both, field), getattr(best, field)), field


# ---- 7. estimate_pose(refine_iterations) ------------------------------------------------------------------------------------------------
def test_estimate_pose_refines_its_winner():
    case, grid, truth, width, observed, bound, _ = ellipsoid_problem()
    args = (grid, observed, width, P.case_start(case), case["half_span"], case["counts"], case["levels"], None, case["cost"], case["height_mm"])
    plain = md().estimate_pose(*args)
    fine = md().estimate_pose(*args, refine_iterations=8)
    assert plain.refinement is None and plain.lattice_pose is plain.pose and plain.lattice_cost is plain.cost
    assert torch.equal(fine.lattice_pose, plain.pose) and torch.equal(fine.lattice_cost, plain.cost) and torch.equal(fine.trace, plain.trace)
    assert bool((fine.cost <= fine.lattice_cost).all()) and isinstance(fine.refinement, md().PoseRefinement)
    assert torch.equal(fine.cost, fine.refinement.cost) and torch.equal(fine.pose, fine.refinement.pose) and fine.row.shape == (1, 5)
    assert torch.equal(fine.refinement.trace[0], plain.cost) and torch.equal(fine.width, width)
    e0, e1 = md().pose_error(plain, truth)[0].abs().cpu().numpy(), md().pose_error(fine, truth)[0].abs().cpu().numpy()
    print(f"lattice error {e0.tolist()} cost {float(plain.cost[0])!r}; refined error {e1.tolist()} cost {float(fine.cost[0])!r}")
    assert np.all(e1 <= np.asarray(bound)) and np.all(e1 < e0)
    for bad in (-1, 1.5, True):
        with pytest.raises(md().MeshDepthError):
            md().estimate_pose(*args, refine_iterations=bad)
    wide = md().estimate_pose(grid, observed, torch.tensor([PW.start_width(case)], device=DEV), P.case_start(case), case["half_span"], (5, 5, 7), 2,
                              None, "mse", case["height_mm"], width_half_span=PW.WIDTH_HALF_SPAN, width_count=PW.WIDTH_COUNT, refine_iterations=6)
    assert bool((wide.cost <= wide.lattice_cost).all()) and wide.refinement.last_step.shape == (1, 4)          # the width axis frees the width


def test_lm_update_edge_rows_equal_the_twin_bit_for_bit():
    """Three problems in one call, every parameter free: (0) an accepted trial whose matrix is singular in theta -- the gate gives
    the step 0 and the next trial is the state; (1) a NaN trial cost -- not accepted, the step comes from the old row, unclipped;
    (2) an accepted trial whose right-hand side is so large that the clip binds in every component.  The kernel's arithmetic is
    + - * / and sqrt in lm_update_ref's order: every output is compared bit for bit."""
    from gelslim_depth_amd import _lib as L
    rng = np.random.Generator(np.random.PCG64(33))
    max_step = (0.5, 0.5, 0.1, 0.5)
    cur = np.stack([spd_row(rng)[0] for _ in range(3)])
    trial = np.stack([spd_row(rng)[0] for _ in range(3)])
    cur[1, 2:6] *= 1e-2
    trial[2, 2:6] *= 1e6
    trial[0, 0], trial[1, 0], trial[2, 0] = 0.5 * cur[0, 0], np.nan, 0.5 * cur[2, 0]
    for q, (j, k) in enumerate(PR.PAIRS):
        if 2 in (j, k):
            trial[0, 6 + q] = 0.0
    trial[0, 2 + 2] = 0.0
    lam0 = np.array([1e-3, 0.25, 5e-12])
    free, _ = PR.lm_solve(cur[1], lam0[1] * 10.0, 15, (np.inf,) * 4)
    assert (np.abs(free) < np.asarray(max_step)).all() and free.all()
    free, _ = PR.lm_solve(trial[2], 1e-12, 15, (np.inf,) * 4)
    assert (np.abs(free) > np.asarray(max_step)).all()
    pose0 = (rng.uniform(-1, 1, (3, 3)) * np.array([1e-3, 1e-3, 1.0])).astype(np.float32)
    pose1 = (pose0 + rng.uniform(-1, 1, (3, 3)).astype(np.float32) * np.float32(1e-4)).astype(np.float32)
    width0 = rng.uniform(4, 6, 3).astype(np.float32)
    width1 = (width0 + np.float32(0.01)).astype(np.float32)
    lm = L.gsd_pose_lm()
    lm.down, lm.up, lm.lambda_min, lm.lambda_max, lm.free_mask, lm.first = 0.1, 10.0, 1e-12, 1e12, 15, 0
    lm.max_step[:] = max_step
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pose, width, lam, row = dev(pose0), dev(width0), dev(lam0), dev(cur)
    t_pose, t_width, t_row = dev(pose1), dev(width1), dev(trial)
    trace = torch.zeros(3, dtype=torch.float64, device=DEV)
    accepted = torch.full((3,), 5, dtype=torch.int32, device=DEV)
    last = torch.zeros((3, 4), dtype=torch.float64, device=DEV)
    assert L.lib.gsd_mesh_pose_lm_update(C.byref(lm), 3, pose.data_ptr(), width.data_ptr(), lam.data_ptr(), row.data_ptr(), t_pose.data_ptr(),
                                         t_width.data_ptr(), t_row.data_ptr(), trace.data_ptr(), accepted.data_ptr(), last.data_ptr(),
                                         L.stream_ptr()) == L.GSD_OK
    host = lambda t: t.cpu().numpy()
    same = lambda t, want: same_bits(t.cpu().reshape(-1), torch.from_numpy(np.asarray(want, np.float64).reshape(-1)))
    for i in range(3):
        st = {"pose": pose0[i].copy(), "width": width0[i], "lam": float(lam0[i]), "row": cur[i].copy(), "accepted": 5}
        nxt, nxt_width, dl, took = PR.lm_update_ref(st, pose1[i], width1[i], trial[i], 15, max_step=max_step)
        assert took == (i != 1) and int(accepted[i]) == st["accepted"] == (5 if i == 1 else 6), i
        assert np.array_equal(host(pose[i]), st["pose"]) and host(width[i]) == st["width"] and host(lam[i]) == st["lam"], i
        assert same(row[i], st["row"]) and same(trace[i], st["row"][0]), i
        assert same(last[i], np.abs(dl)), (i, host(last[i]), dl)
        assert np.array_equal(host(t_pose[i]), nxt) and host(t_width[i]) == nxt_width, i
        if i == 0:
            assert not dl.any() and np.array_equal(nxt, st["pose"]) and nxt_width == st["width"]
        if i == 2:
            assert np.array_equal(np.abs(dl), max_step)
