"""GPU: gsd_mesh_pose_score and the pose search of gelslim_depth_amd.mesh_depth.

Rows are held to render_depth of the same poses reduced in fp64 by tests/mesh_pose_ref.py: counts exactly, the two sums to the
reordering of an fp64 sum of identical non-negative terms.  The searches are held to the brute-force twin's own error:

    BOUND = 3 * max(|TWIN_ERROR|, FINAL_STEP) per axis (mm, mm, rad)

TWIN_ERROR is what `python tests/mesh_pose_ref.py` printed for the two cases (rounded up in the last digit kept), FINAL_STEP the
last level's step.  The margin of 3: fp32 edge pixels may move the winner to another member of the same plateau of equal cost,
whose width the twin's own error samples."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import mesh_pose_ref as P

pytestmark = pytest.mark.gpu

# the twin, measured:  lprism    error (-0.0074074, -0.0148148, -0.0093750), cost 0.0 after 4 levels (10 candidates tie at the end)
#                      ellipsoid error ( 0.0333333,  0.0444444, -0.0343750), cost 1.1814e-05 after 3 levels
TWIN_ERROR = {"lprism": (0.0074075, 0.0148149, 0.0093751), "ellipsoid": (0.0333334, 0.0444445, 0.0343751)}
FINAL_STEP = {"lprism": (1.5e-3 / 81 * 1e3, 1.5e-3 / 81 * 1e3, 0.6 / 256), "ellipsoid": (1.5e-3 / 27 * 1e3, 1.5e-3 / 27 * 1e3, 0.6 / 64)}
BOUND = {k: tuple(3 * max(e, s) for e, s in zip(TWIN_ERROR[k], FINAL_STEP[k])) for k in TWIN_ERROR}

HEIGHT_MM = 12.0
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def mesh(name):
    return P.MESHES[name]()


@functools.lru_cache(maxsize=None)
def grid_of(name):
    from gelslim_depth_amd.mesh_depth import MeshGrid
    return MeshGrid(mesh(name), 1.0, P.PLANE, DEV)


@functools.lru_cache(maxsize=None)
def problem(name, size, flip=False, invert=False, b=2, p=37, seed=0):
    """(observed (b, 2, H, W), candidates (b, p, 3), widths (b,)): different widths, seeded candidates around a pose per
    observation, D a render at another pose plus Gaussian noise of 0.05 mm."""
    from gelslim_depth_amd.mesh_depth import render_depth
    rng = np.random.Generator(np.random.PCG64(seed))
    g = P.contact_width(mesh(name))
    widths = torch.tensor([g - 0.3 * k for k in range(b)], dtype=torch.float32, device=DEV)
    base = np.array([[0.4e-3, -0.3e-3, 0.35], [-0.6e-3, 0.5e-3, -1.2]] * b)[:b]
    cand = base[:, None, :] + rng.uniform(-1, 1, (b, p, 3)) * np.array([1.5e-3, 1.5e-3, 0.6])
    cand = torch.from_numpy(cand.astype(np.float32)).to(DEV)
    seen = torch.from_numpy((base + np.array([0.2e-3, -0.15e-3, 0.1])).astype(np.float32)).to(DEV)
    observed = render_depth(grid_of(name), seen, widths, size, HEIGHT_MM, 0.0, flip, invert)
    noise = torch.from_numpy(rng.normal(0.0, 0.05, tuple(observed.shape)).astype(np.float32)).to(DEV)
    return (observed + noise).contiguous(), cand.contiguous(), widths


def score(name, observed, cand, widths, flip=False, invert=False, **kw):
    from gelslim_depth_amd.mesh_depth import score_poses
    return score_poses(grid_of(name), observed, cand, widths, HEIGHT_MM, 0.0, flip, invert, **kw)


@pytest.mark.parametrize("name,size,flip,invert,contact", [("lprism", (24, 31), False, False, 0.0), ("sphere4", (40, 53), True, False, 0.05),
                                                           ("ellipsoid", (40, 53), False, True, 0.0), ("ellipsoid", (24, 31), False, False, 0.1)])
def test_rows_equal_the_render_reduced_in_fp64(name, size, flip, invert, contact):
    from gelslim_depth_amd.mesh_depth import render_depth
    observed, cand, widths = problem(name, size, flip, invert)
    b, p = cand.shape[:2]
    images = render_depth(grid_of(name), cand.reshape(-1, 3), widths.repeat_interleave(p), size, HEIGHT_MM, 0.0, flip, invert)
    images = images.reshape(b, p, 2, *size).cpu().numpy()
    seen = observed.cpu().numpy()
    assert (images < -contact).any() and (seen < -contact).any()
    for stride in (1, 2, 3):
        got = score(name, observed, cand, widths, flip, invert, stride=stride, contact_depth=contact)
        assert got.shape == (b, p, 5) and got.dtype == torch.float64
        got = got.cpu().numpy()
        want = np.stack([np.stack([P.row_ref(images[i, k], seen[i], stride, contact) for k in range(p)]) for i in range(b)])
        n = P.n_points(size[0], size[1], stride)
        assert np.array_equal(got[..., 2:], want[..., 2:]), (name, stride)
        assert want[..., 3].max() > 0 and want[..., 2].max() > 0 and (want[..., 0] > 0).all()
        rel = np.abs(got[..., :2] - want[..., :2]) / want[..., :2]
        print(f"{name} {size} stride {stride} flip={flip} invert={invert}: n = {n}, worst relative difference of the sums "
              f"{rel.max():.3e} (bound {2 * n * 2.0 ** -53:.3e})")
        assert rel.max() <= 2 * n * 2.0 ** -53, (name, stride, rel.max())


@pytest.mark.parametrize("name,size,flip,invert", [("lprism", (24, 31), False, False), ("sphere4", (40, 53), True, False),
                                                   ("ellipsoid", (40, 53), False, True)])
def test_a_candidate_scored_against_its_own_render_is_exactly_zero(name, size, flip, invert):
    from gelslim_depth_amd.mesh_depth import render_depth
    _, cand, widths = problem(name, size, flip, invert)
    k = 11
    own = render_depth(grid_of(name), cand[:, k].contiguous(), widths, size, HEIGHT_MM, 0.0, flip, invert)
    for stride in (1, 2, 3):
        rows = score(name, own, cand, widths, flip, invert, stride=stride).cpu().numpy()
        for i in range(cand.shape[0]):
            row = rows[i, k]
            assert row[0] == 0.0 and row[1] == 0.0 and row[2] == row[3] == row[4] > 0, (name, stride, i, row)


def test_rows_do_not_depend_on_the_batch_and_repeat_bitwise():
    for name, size, stride in (("sphere4", (40, 53), 1), ("lprism", (24, 31), 2), ("ellipsoid", (40, 53), 3)):
        observed, cand, widths = problem(name, size)
        full = score(name, observed, cand, widths, stride=stride)
        assert torch.equal(full, score(name, observed, cand, widths, stride=stride))
        few = score(name, observed, cand[:, :5].contiguous(), widths, stride=stride)
        assert torch.equal(few, full[:, :5]), name
        alone = score(name, observed[1:2].contiguous(), cand[1:2].contiguous(), widths[1:2].contiguous(), stride=stride)
        assert torch.equal(alone[0], full[1]), name
        one = score(name, observed[1:2].contiguous(), cand[1, 36:37].contiguous(), widths[1:2].contiguous(), stride=stride)      # (P, 3)
        assert one.shape == (1, 1, 5) and torch.equal(one[0, 0], full[1, 36])
        # a (P, 3) tensor serves every observation; out is written in place
        out = torch.full((2, 37, 5), 7.0, dtype=torch.float64, device=DEV)
        shared = score(name, observed, cand[0], widths, stride=stride, out=out)
        assert shared is out and torch.equal(shared[0], full[0]) and not torch.equal(shared[1], full[1])


def test_nan_pixels_and_refused_widths():
    from gelslim_depth_amd._lib import GsdError
    from gelslim_depth_amd.mesh_depth import MeshDepthError
    name, size = "ellipsoid", (24, 31)
    observed, cand, widths = problem(name, size)
    clean = score(name, observed, cand, widths, stride=2)
    on, off = observed.clone(), observed.clone()
    on[0, 1, 11, 13] = float("nan")          # odd row, odd column: on the stride-2 lattice
    off[0, 1, 11, 14] = float("nan")
    bad = score(name, on, cand, widths, stride=2)
    assert not bool(torch.isfinite(bad[0, :, :2]).any()) and bool(torch.isfinite(bad[0, :, 2:]).all())
    assert torch.equal(bad[1], clean[1]) and bool((bad[0, :, 4] <= clean[0, :, 4]).all()) and torch.equal(bad[0, :, 3], clean[0, :, 3])
    assert torch.equal(score(name, off, cand, widths, stride=2), clean)
    assert not bool(torch.isfinite(score(name, off, cand, widths, stride=1)[0, :, :2]).any())
    refused = torch.stack((widths[0], -widths[1]))
    got = score(name, observed, cand, refused, stride=2, validate=False)
    assert bool(torch.isnan(got[1]).all()) and torch.equal(got[0], clean[0])
    out = torch.full((2, 37, 5), 7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(MeshDepthError) as e:
        score(name, observed, cand, refused, stride=2, out=out)
    assert isinstance(e.value, ValueError) and isinstance(e.value, GsdError)
    for kw in ({"stride": 0}, {"stride": -2}, {"stride": 1.5}, {"contact_depth": -0.1}, {"contact_depth": float("nan")},
               {"contact_depth": float("inf")}):
        with pytest.raises(MeshDepthError):
            score(name, observed, cand, widths, out=out, **kw)
    with pytest.raises(MeshDepthError):
        score(name, observed, cand[:, :, :2].contiguous(), widths, out=out)
    with pytest.raises(MeshDepthError):
        score(name, observed.cpu(), cand, widths, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_the_library_refuses_bad_arguments_before_any_launch():
    from gelslim_depth_amd import _lib as L
    grid = grid_of("lprism")
    observed, cand, widths = problem("lprism", (24, 31))
    view = L.gsd_mesh_view()
    view.mpp, view.width_offset, view.swap_axes = HEIGHT_MM / 24, 0.0, grid.swap_axes
    need = int(L.lib.gsd_mesh_pose_score_workspace(2, 37, 24, 31, 2))
    assert need == 2 * 37 * 4 + 2 * 37 * 2 * 1 * 1 * 5          # pose table | one tile per channel: 12 x 15 lattice points
    assert L.lib.gsd_mesh_pose_score_workspace(2, 37, 40, 53, 1) == 2 * 37 * 4 + 2 * 37 * 24 * 5
    rows = torch.full((2, 37, 5), 7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros((need,), dtype=torch.float64, device=DEV)

    def call(b=2, p=37, h=24, w=31, stride=2, contact=0.0, elems=need):
        return L.lib.gsd_mesh_pose_score(C.byref(grid.grid), C.byref(view), grid.records.data_ptr(), grid.triangles, grid.cells.data_ptr(),
                                         grid.list.data_ptr(), grid.list.numel(), observed.data_ptr(), b, cand.data_ptr(),
                                         widths.data_ptr(), p, h, w, stride, contact, rows.data_ptr(), ws.data_ptr(), elems,
                                         L.stream_ptr())
    for kw in ({"stride": 0}, {"p": 0}, {"b": 0}, {"contact": -1.0}, {"contact": float("nan")}, {"elems": need - 1},
               {"b": 1 << 15, "p": 1 << 15, "h": 64, "w": 64, "stride": 1}, {"b": 1 << 16, "p": 1 << 16}):
        assert call(**kw) == L.GSD_ERR_BAD_ARG, kw
        assert "gsd_mesh_pose_score" in L.lib.gsd_last_error().decode()
    assert L.lib.gsd_mesh_pose_score_workspace(1 << 15, 1 << 15, 64, 64, 1) == 0 and L.lib.gsd_mesh_pose_score_workspace(2, 37, 24, 31, 0) == 0
    torch.cuda.synchronize()
    assert bool((rows == 7.0).all())
    assert call() == L.GSD_OK
    assert torch.equal(rows, score("lprism", observed, cand, widths, stride=2))


def search(case_name, b=2):
    from gelslim_depth_amd.mesh_depth import PoseEstimate, estimate_pose, lattice_points, pose_cost, pose_error, render_depth, score_poses
    case = P.CASES[case_name]
    grid = grid_of(case["mesh"])
    size = case["size"]
    truth = torch.tensor([P.case_truth(case)] * b, dtype=torch.float32, device=DEV)
    widths = torch.full((b,), P.contact_width(mesh(case["mesh"])), dtype=torch.float32, device=DEV)
    observed = render_depth(grid, truth, widths, size, case["height_mm"])
    est = estimate_pose(grid, observed, widths, P.case_start(case), case["half_span"], case["counts"], case["levels"], None, case["cost"],
                        case["height_mm"])
    assert isinstance(est, PoseEstimate) and est.pose.shape == (b, 3) and est.pose.dtype == torch.float32 and est.pose.is_cuda
    assert est.cost.shape == (b,) and est.row.shape == (b, 5) and est.trace.shape == (case["levels"], b) and est.trace.is_cuda
    trace = est.trace.cpu().numpy()
    assert np.isfinite(trace).all() and np.all(np.diff(trace, axis=0) <= 0), trace
    assert torch.equal(est.trace[-1], est.cost)
    rows = score_poses(grid, observed, est.pose.unsqueeze(1).contiguous(), widths, case["height_mm"])
    assert torch.equal(rows[:, 0], est.row)
    assert torch.equal(pose_cost(rows[:, 0], case["cost"], lattice_points(size, 1)), est.cost)
    assert torch.equal(est.pose[0], est.pose[1]) and torch.equal(est.row[0], est.row[1])          # the same observation twice
    err = pose_error(est, truth).cpu().numpy()
    print(f"{case_name}: pose {est.pose[0].tolist()}, cost {est.cost[0].item():.6e}, trace {trace[:, 0].tolist()}, "
          f"error (mm, mm, rad) {err[0].tolist()}, bound {BOUND[case_name]}")
    assert np.all(np.abs(err) <= np.asarray(BOUND[case_name])), (err, BOUND[case_name])
    return est


def test_search_recovers_the_l_prism_pose_of_the_cpu_twin():
    search("lprism")


def test_search_recovers_the_pose_of_a_smooth_asymmetric_object():
    search("ellipsoid")


def test_search_arguments_strides_and_weighted_costs():
    from gelslim_depth_amd.mesh_depth import MeshDepthError, estimate_pose, pose_error, render_depth
    case = P.CASES["ellipsoid"]
    grid = grid_of("ellipsoid")
    truth = torch.tensor([P.case_truth(case), (-0.5e-3, 0.2e-3, 0.4)], dtype=torch.float32, device=DEV)
    widths = torch.tensor([P.contact_width(mesh("ellipsoid"))] * 2, dtype=torch.float32, device=DEV)
    observed = render_depth(grid, truth, widths, (40, 53), HEIGHT_MM)
    init = truth + torch.tensor([[0.5e-3, -0.4e-3, 0.2], [-0.3e-3, 0.6e-3, -0.25]], device=DEV)
    est = estimate_pose(grid, observed, widths, init, (1.2e-3, 1.2e-3, 0.5), (5, 5, 7), 3, (2, 1, 1), {"mse": 1.0, "iou": 0.01}, HEIGHT_MM,
                        validate=False)
    err = pose_error(est, truth).abs().cpu().numpy()
    # the truth lies inside the first lattice, and every later level reaches one step around its centre: a search that works ends
    # within the FIRST level's step (0.6 mm, 0.6 mm, 0.5 / 3 rad) of the truth, whatever the stride and the cost
    assert est.trace.shape == (3, 2) and np.all(err[:, :2] <= 0.6) and np.all(err[:, 2] <= 0.5 / 3), err
    for kw in ({"counts": (6, 7, 9)}, {"counts": (1, 7, 9)}, {"counts": (7, 7)}, {"strides": (1, 1)}, {"strides": (1, 1, 0)},
               {"contact_depth": -1.0}, {"cost": "rmse"}, {"levels": 0}):
        args = {"counts": (5, 5, 7), "levels": 3, **kw}
        with pytest.raises(MeshDepthError):
            estimate_pose(grid, observed, widths, init, (1.2e-3, 1.2e-3, 0.5), image_height_mm=HEIGHT_MM, **args)
    with pytest.raises(MeshDepthError):
        estimate_pose(grid, observed, widths, init[:1], (1.2e-3, 1.2e-3, 0.5), (5, 5, 7), 3)
    with pytest.raises(MeshDepthError):
        estimate_pose(grid, observed, -widths, init, (1.2e-3, 1.2e-3, 0.5), (5, 5, 7), 3)
