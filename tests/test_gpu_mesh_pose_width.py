"""GPU: gsd_mesh_pose_score_widths and the pose search over an unknown grasp width.

The contract is bits: row (b, p, k) of score_poses_widths equals, in all five entries, the row score_poses gives for observation
b, candidate p and the width widths[b, k] (NaN == NaN counted as equal) -- an oracle that is not the code under test.  The
searches are held to the brute-force twin's own error, section 17's rule with the width as a fourth axis:

    BOUND = 3 * max(|TWIN_ERROR|, FINAL_STEP) per axis (mm, mm, rad, mm)

TWIN_ERROR is what `python tests/mesh_pose_width_ref.py` printed for the two cases (rounded up in the last digit kept), FINAL_STEP
the last level's step.  The margin of 3: fp32 edge pixels may move the winner to another member of the same plateau of equal cost,
whose width the twin's own error samples."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_pose_ref as P
import mesh_pose_width_ref as PW
from test_gpu_mesh_pose import DEV, HEIGHT_MM, grid_of, mesh, problem

pytestmark = pytest.mark.gpu

# the twin, measured (start width = true width + 0.35 mm, width_half_span 0.6 mm, 5 widths):
#   lprism    error ( 0.0111111, -0.0333333,  0.0023438), width error +0.0125 mm, cost 2.1788e-06 after 4 levels (44 candidates tie)
#   ellipsoid error ( 0.0333333,  0.0444444, -0.0343750), width error -0.0250 mm, cost 2.2496e-05 after 3 levels
TWIN_ERROR = {"lprism": (0.0111112, 0.0333334, 0.0023438, 0.0125001), "ellipsoid": (0.0333334, 0.0444445, 0.0343751, 0.0250001)}
FINAL_STEP = {"lprism": (1.5e-3 / 81 * 1e3, 1.5e-3 / 81 * 1e3, 0.6 / 256, 0.6 / 16), "ellipsoid": (1.5e-3 / 27 * 1e3, 1.5e-3 / 27 * 1e3, 0.6 / 64, 0.6 / 8)}
BOUND = {k: tuple(3 * max(e, s) for e, s in zip(TWIN_ERROR[k], FINAL_STEP[k])) for k in TWIN_ERROR}


def same_bits(a, b):
    """Equal entry by entry, NaN == NaN counted as equal."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def widths_of(name, g_count, b=2):
    """(b, G) widths, different per observation: spread around the contact width; with G >= 3, a 0 (the gels meet at the mid-plane)
    in one observation and a width so large that nothing touches in the other."""
    g = P.contact_width(mesh(name))
    w = np.stack([g - 0.3 * i + np.linspace(-0.5, 0.4, g_count) * (g_count > 1) for i in range(b)]).astype(np.float32)
    if g_count >= 3:
        w[0, 1], w[1, g_count - 1] = 0.0, 1.0e3
    else:
        w[1, 0] = 0.0
    return torch.from_numpy(w).to(DEV)


def score(name, observed, cand, widths, flip=False, invert=False, **kw):
    from gelslim_depth_amd.mesh_depth import score_poses
    return score_poses(grid_of(name), observed, cand, widths, HEIGHT_MM, 0.0, flip, invert, **kw)


def score_w(name, observed, cand, widths, flip=False, invert=False, **kw):
    from gelslim_depth_amd.mesh_depth import score_poses_widths
    return score_poses_widths(grid_of(name), observed, cand, widths, HEIGHT_MM, 0.0, flip, invert, **kw)


def columns(name, observed, cand, widths, flip=False, invert=False, **kw):
    """The oracle: one score_poses call per width column, stacked to (B, P, G, 5)."""
    return torch.stack([score(name, observed, cand, widths[:, k].contiguous(), flip, invert, validate=False, **kw)
                        for k in range(widths.shape[1])], dim=2)


@pytest.mark.parametrize("g_count", [1, 3, 5, 32])
@pytest.mark.parametrize("name,size,flip,invert,contact,stride", [("lprism", (24, 31), False, False, 0.0, 1), ("lprism", (24, 31), False, False, 0.0, 3),
                                                                  ("sphere4", (40, 53), True, False, 0.05, 2),
                                                                  ("ellipsoid", (24, 31), False, True, 0.0, 1)])
def test_rows_have_the_bits_of_score_poses(name, size, flip, invert, contact, stride, g_count):
    observed, cand, _ = problem(name, size, flip, invert)
    widths = widths_of(name, g_count)
    got = score_w(name, observed, cand, widths, flip, invert, stride=stride, contact_depth=contact)
    assert got.shape == (2, 37, g_count, 5) and got.dtype == torch.float64 and bool(torch.isfinite(got).all())
    want = columns(name, observed, cand, widths, flip, invert, stride=stride, contact_depth=contact)
    assert same_bits(got, want), (name, stride, g_count, (got != want).nonzero()[:5].tolist())
    assert bool((got[..., 3] > 0).any()) and bool((got[..., 0] > 0).all())
    if g_count >= 3:          # the width at which nothing touches renders no contact; the rows differ from column to column
        assert bool((got[1, :, g_count - 1, 3] == 0).all()) and not torch.equal(got[:, :, 0], got[:, :, 2])


def test_more_than_64_tiles_per_candidate():
    """80 x 106 at stride 1: 2 * 5 * 7 = 70 tiles per candidate, the rows kernel's second trip."""
    name, size = "lprism", (80, 106)
    observed, cand, _ = problem(name, size, False, False, 2, 3)
    widths = widths_of(name, 3)
    from gelslim_depth_amd import _lib as L
    assert L.lib.gsd_mesh_pose_score_widths_workspace(2, 3, 3, 80, 106, 1) == 2 * 3 * 4 + 3 + 2 * 3 * 70 * 3 * 5
    got = score_w(name, observed, cand, widths)
    assert same_bits(got, columns(name, observed, cand, widths)) and bool(torch.isfinite(got).all()) and bool((got[..., 0] > 0).all())


def test_refused_widths_are_nan_columns_and_nothing_else_moves():
    from gelslim_depth_amd._lib import GsdError
    from gelslim_depth_amd.mesh_depth import MeshDepthError
    name, size = "ellipsoid", (24, 31)
    observed, cand, _ = problem(name, size)
    widths = widths_of(name, 5)
    clean = score_w(name, observed, cand, widths, stride=2)
    bad = widths.clone()
    bad[0, 3], bad[1, 0] = -1.0, float("nan")
    got = score_w(name, observed, cand, bad, stride=2, validate=False)
    refused = torch.zeros((2, 37, 5), dtype=torch.bool, device=DEV)
    refused[0, :, 3] = refused[1, :, 0] = True
    assert bool(got[refused].isnan().all()) and torch.equal(got[~refused], clean[~refused]) and bool(torch.isfinite(clean).all())
    assert same_bits(got, columns(name, observed, cand, bad, stride=2))
    out = torch.full((2, 37, 5, 5), 7.0, dtype=torch.float64, device=DEV)
    for w in (bad, widths - 100.0, torch.where(bad.isnan(), torch.full_like(bad, float("inf")), widths)):
        with pytest.raises(MeshDepthError) as e:
            score_w(name, observed, cand, w, stride=2, out=out)
        assert isinstance(e.value, ValueError) and isinstance(e.value, GsdError)
    for kw in ({"stride": 0}, {"stride": 1.5}, {"contact_depth": -0.1}, {"contact_depth": float("nan")}):
        with pytest.raises(MeshDepthError):
            score_w(name, observed, cand, widths, out=out, **kw)
    for w in (widths[0], widths[:1], widths.double(), widths.cpu(), torch.zeros((2, 33), device=DEV), torch.zeros((2, 0), device=DEV)):
        with pytest.raises(MeshDepthError):
            score_w(name, observed, cand, w, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_non_finite_observed_pixels_behave_as_in_score_poses():
    name, size = "ellipsoid", (24, 31)
    observed, cand, _ = problem(name, size)
    widths = widths_of(name, 5)
    clean = score_w(name, observed, cand, widths, stride=3)
    on, off = observed.clone(), observed.clone()
    on[0, 1, 10, 13] = float("nan")          # rows and columns 1, 4, 7, 10, 13, ...: on the stride-3 lattice
    on[1, 0, 7, 16] = float("-inf")
    off[0, 1, 11, 14] = float("nan")
    got = score_w(name, on, cand, widths, stride=3)
    assert same_bits(got, columns(name, on, cand, widths, stride=3))
    assert bool(got[0, :, :, :2].isnan().all()) and bool(got[1, :, :, :2].isinf().all()) and bool(torch.isfinite(got[..., 2:]).all())
    assert torch.equal(got[..., 3], clean[..., 3]) and bool((got[..., 4] <= clean[..., 4]).all())
    assert torch.equal(score_w(name, off, cand, widths, stride=3), clean)
    at_one = score_w(name, off, cand, widths, stride=1)
    assert same_bits(at_one, columns(name, off, cand, widths, stride=1)) and bool(at_one[0, :, :, :2].isnan().all())


def test_rows_do_not_depend_on_the_batch_or_the_other_widths_and_repeat_bitwise():
    for name, size, stride in (("sphere4", (40, 53), 1), ("lprism", (24, 31), 2)):
        observed, cand, _ = problem(name, size)
        widths = widths_of(name, 5)
        full = score_w(name, observed, cand, widths, stride=stride)
        assert torch.equal(full, score_w(name, observed, cand, widths, stride=stride))
        for k in range(5):          # a column scored alone (G = 1)
            assert torch.equal(score_w(name, observed, cand, widths[:, k:k + 1].contiguous(), stride=stride)[:, :, 0], full[:, :, k]), (name, k)
        assert torch.equal(score_w(name, observed, cand, widths[:, 1:3].contiguous(), stride=stride), full[:, :, 1:3])          # G = 2
        assert torch.equal(score_w(name, observed, cand[:, :5].contiguous(), widths, stride=stride), full[:, :5]), name
        alone = score_w(name, observed[1:2].contiguous(), cand[1:2].contiguous(), widths[1:2].contiguous(), stride=stride)
        assert torch.equal(alone[0], full[1]), name
        out = torch.full((2, 37, 5, 5), 7.0, dtype=torch.float64, device=DEV)          # a (P, 3) tensor serves every observation
        shared = score_w(name, observed, cand[0], widths, stride=stride, out=out)
        assert shared is out and torch.equal(shared[0], full[0]) and not torch.equal(shared[1], full[1])


def test_the_library_refuses_bad_arguments_before_any_launch():
    from gelslim_depth_amd import _lib as L
    grid = grid_of("lprism")
    observed, cand, _ = problem("lprism", (24, 31))
    widths = widths_of("lprism", 32)
    view = L.gsd_mesh_view()
    view.mpp, view.width_offset, view.swap_axes = HEIGHT_MM / 24, 0.0, grid.swap_axes
    query = L.lib.gsd_mesh_pose_score_widths_workspace
    need = int(query(2, 37, 3, 24, 31, 2))
    assert L.GSD_POSE_WIDTHS_MAX == 32
    assert need == 2 * 37 * 4 + 3 + 2 * 37 * 2 * 3 * 5          # pose table | 6 half-widths | one tile per channel, 3 rows each
    rows = torch.full((2, 37, 3, 5), 7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros((int(query(2, 37, 32, 24, 31, 1)),), dtype=torch.float64, device=DEV)

    def call(b=2, p=37, g=3, h=24, w=31, stride=2, contact=0.0, elems=need):
        return L.lib.gsd_mesh_pose_score_widths(C.byref(grid.grid), C.byref(view), grid.records.data_ptr(), grid.triangles,
                                                grid.cells.data_ptr(), grid.list.data_ptr(), grid.list.numel(), observed.data_ptr(), b,
                                                cand.data_ptr(), widths.data_ptr(), p, g, h, w, stride, contact, rows.data_ptr(),
                                                ws.data_ptr(), elems, L.stream_ptr())
    for kw in ({"g": 0}, {"g": L.GSD_POSE_WIDTHS_MAX + 1, "elems": ws.numel()}, {"elems": need - 1}, {"stride": 0}, {"p": 0}, {"b": 0},
               {"contact": -1.0}, {"contact": float("nan")}, {"b": 1 << 15, "p": 1 << 15, "h": 64, "w": 64, "stride": 1},
               {"b": 1 << 13, "p": 1 << 13, "g": 32, "h": 4, "w": 4, "stride": 1}):
        assert call(**kw) == L.GSD_ERR_BAD_ARG, kw
        assert "gsd_mesh_pose_score_widths" in L.lib.gsd_last_error().decode()
    assert query(2, 37, 0, 24, 31, 2) == 0 and query(2, 37, L.GSD_POSE_WIDTHS_MAX + 1, 24, 31, 2) == 0 and query(2, 37, 3, 24, 31, 0) == 0
    assert query(1 << 15, 1 << 15, 3, 64, 64, 1) == 0 and query(1 << 13, 1 << 13, 32, 4, 4, 1) == 0 and query(0, 37, 3, 24, 31, 2) == 0
    torch.cuda.synchronize()
    assert bool((rows == 7.0).all())
    assert call() == L.GSD_OK          # the first three of the 32 columns of each observation: widths is read with a row pitch of G
    three = torch.stack((widths.reshape(-1)[:3], widths.reshape(-1)[3:6]))
    assert torch.equal(rows, score_w("lprism", observed, cand, three, stride=2))


def search(case_name, b=2):
    from gelslim_depth_amd.mesh_depth import PoseEstimate, estimate_pose, lattice_points, pose_cost, pose_error, render_depth, score_poses
    case = P.CASES[case_name]
    grid = grid_of(case["mesh"])
    size = case["size"]
    truth = torch.tensor([P.case_truth(case)] * b, dtype=torch.float32, device=DEV)
    widths = torch.full((b,), PW.true_width(case), dtype=torch.float32, device=DEV)
    start = torch.full((b,), PW.start_width(case), dtype=torch.float32, device=DEV)
    observed = render_depth(grid, truth, widths, size, case["height_mm"])
    est = estimate_pose(grid, observed, start, P.case_start(case), case["half_span"], case["counts"], case["levels"], None, case["cost"],
                        case["height_mm"], width_half_span=PW.WIDTH_HALF_SPAN, width_count=PW.WIDTH_COUNT)
    assert isinstance(est, PoseEstimate) and est.pose.shape == (b, 3) and est.pose.dtype == torch.float32 and est.pose.is_cuda
    assert est.width.shape == (b,) and est.width.dtype == torch.float32 and est.width.is_cuda
    assert est.cost.shape == (b,) and est.row.shape == (b, 5) and est.trace.shape == (case["levels"], b) and est.trace.is_cuda
    trace = est.trace.cpu().numpy()
    assert np.isfinite(trace).all() and np.all(np.diff(trace, axis=0) <= 0), trace
    assert torch.equal(est.trace[-1], est.cost)
    rows = score_poses(grid, observed, est.pose.unsqueeze(1).contiguous(), est.width, case["height_mm"])
    assert torch.equal(rows[:, 0], est.row)
    assert torch.equal(pose_cost(rows[:, 0], case["cost"], lattice_points(size, 1)), est.cost)
    assert torch.equal(est.pose[0], est.pose[1]) and torch.equal(est.row[0], est.row[1]) and torch.equal(est.width[0], est.width[1])
    err = np.concatenate((pose_error(est, truth).cpu().numpy(), (est.width.double() - widths.double()).cpu().numpy()[:, None]), axis=1)
    print(f"{case_name}: pose {est.pose[0].tolist()}, width {est.width[0].item()!r}, cost {est.cost[0].item():.6e}, "
          f"trace {trace[:, 0].tolist()}, error (mm, mm, rad, mm) {err[0].tolist()}, bound {BOUND[case_name]}")
    assert np.all(np.abs(err) <= np.asarray(BOUND[case_name])), (err, BOUND[case_name])
    return est


def test_search_recovers_the_l_prism_pose_and_width_of_the_cpu_twin():
    search("lprism")


def test_search_recovers_pose_and_width_of_a_smooth_asymmetric_object():
    search("ellipsoid")


def test_the_width_axis_contains_the_fixed_width_search_and_is_off_by_default():
    from gelslim_depth_amd.mesh_depth import MeshDepthError, estimate_pose, render_depth
    case = P.CASES["ellipsoid"]
    grid = grid_of("ellipsoid")
    truth = torch.tensor([P.case_truth(case), (-0.5e-3, 0.2e-3, 0.4)], dtype=torch.float32, device=DEV)
    widths = torch.tensor([PW.true_width(case), PW.true_width(case) - 0.3], dtype=torch.float32, device=DEV)
    observed = render_depth(grid, truth, widths, (24, 31), HEIGHT_MM)
    init = truth + torch.tensor([[0.5e-3, -0.4e-3, 0.2], [-0.3e-3, 0.6e-3, -0.25]], device=DEV)
    args = (grid, observed, widths, init, (1.2e-3, 1.2e-3, 0.5), (5, 5, 7), 2, (2, 1), "mse", HEIGHT_MM)
    fixed = estimate_pose(*args)
    one = estimate_pose(*args, width_count=1)
    ignored = estimate_pose(*args, width_half_span=0.6, width_count=1)
    for other in (one, ignored):
        assert all(torch.equal(getattr(fixed, k), getattr(other, k)) for k in ("pose", "cost", "row", "trace", "width"))
    assert torch.equal(fixed.width, widths)
    # started at the true width, level 0's lattice holds every candidate of the fixed-width level 0 (the middle width IS the start)
    four = estimate_pose(*args, width_half_span=0.6, width_count=5)
    assert bool((four.trace[0] <= fixed.trace[0]).all()) and bool(torch.isfinite(four.trace).all())
    # a width lattice that reaches below 0 is NaN rows there, +inf in the cost: the search goes on with the rest
    low = estimate_pose(grid, observed, torch.full((2,), 0.2, device=DEV), init, (1.2e-3, 1.2e-3, 0.5), (5, 5, 7), 2, (2, 1), "mse",
                        HEIGHT_MM, width_half_span=0.6, width_count=5)
    assert bool(torch.isfinite(low.trace).all()) and bool((low.width >= 0).all())
    for kw in ({"width_count": 4, "width_half_span": 0.6}, {"width_count": 2, "width_half_span": 0.6},
               {"width_count": 5, "width_half_span": -0.6}, {"width_count": 3, "width_half_span": 0.0}, {"width_count": 3},
               {"width_count": 5, "width_half_span": float("nan")}, {"width_count": 1, "width_half_span": -1.0},
               {"width_count": 0, "width_half_span": 0.6}, {"width_count": 35, "width_half_span": 0.6},
               {"width_count": 5.0, "width_half_span": 0.6}):
        with pytest.raises(MeshDepthError):
            estimate_pose(*args, **kw)
    with pytest.raises(MeshDepthError):          # validate=True checks the STARTING widths once
        estimate_pose(grid, observed, -widths, init, (1.2e-3, 1.2e-3, 0.5), (5, 5, 7), 2, width_half_span=0.6, width_count=5)
