"""CPU: the pose search's definitions without a kernel: tests/mesh_pose_ref.py's rows on hand-made image
pairs, the product's level schedule, cost and tie rule (plain torch and numpy: they run on the host) against that restatement,
and the recovery of a known pose by the brute-force twin of estimate_pose (1,764 fp64 renders, a few seconds)."""
import math

import numpy as np
import pytest
import torch

import mesh_pose_ref as P

H, W = 24, 31          # neither side a multiple of 2 or 3 beyond what the lattice offsets absorb: 31 is prime


def slow_row(r, d, stride, c):
    """The definition, pixel by pixel."""
    out = [0.0, 0.0, 0, 0, 0]
    for ch in range(2):
        for y in range(stride // 2, r.shape[1], stride):
            for x in range(stride // 2, r.shape[2], stride):
                e = float(r[ch, y, x]) - float(d[ch, y, x])
                out[0] += e * e
                out[1] += abs(e)
                cr, cd = r[ch, y, x] < -c, bool(np.isfinite(d[ch, y, x])) and d[ch, y, x] < -c
                out[2] += cr and cd
                out[3] += cr
                out[4] += cd
    return np.array(out, np.float64)


def test_rows_of_hand_made_pairs():
    from gelslim_depth_amd.mesh_depth import lattice_points
    r, d = np.zeros((2, H, W), np.float32), np.zeros((2, H, W), np.float32)
    r[0, 3:9, 4:11] = -0.5          # 42 pixels of contact in the rendered image
    d[0, 5:12, 6:9] = -0.25         # 21 in the observed one, 12 of them shared
    d[1, 20, 30] = 0.125            # a positive value in the last pixel: an error, no contact
    got = P.row_ref(r, d, 1, 0.0)
    # shared 12: e = -0.25; rendered only 30: e = -0.5; observed only 9: e = 0.25; the corner: e = -0.125
    assert got.tolist() == [12 * 0.0625 + 30 * 0.25 + 9 * 0.0625 + 0.015625, 12 * 0.25 + 30 * 0.5 + 9 * 0.25 + 0.125, 12, 42, 21]
    for stride in (1, 2, 3):
        rows, cols = P.lattice(H, W, stride)
        assert rows[0] == cols[0] == stride // 2 and rows[-1] < H <= rows[-1] + stride and cols[-1] < W <= cols[-1] + stride
        assert P.n_points(H, W, stride) == 2 * len(rows) * len(cols) == lattice_points((H, W), stride)
        assert np.array_equal(P.row_ref(r, d, stride, 0.0), slow_row(r, d, stride, 0.0)), stride
    assert (len(P.lattice(H, W, 3)[0]), len(P.lattice(H, W, 3)[1])) == (8, 10) and P.n_points(H, W, 2) == 2 * 12 * 15
    # a seeded pair with more texture, every stride, a threshold inside the values
    rng = np.random.Generator(np.random.PCG64(5))
    r2 = -np.abs(rng.normal(0, 0.3, (2, H, W))).astype(np.float32)
    d2 = (r2 + rng.normal(0, 0.05, (2, H, W))).astype(np.float32)
    for stride in (1, 2, 3):
        a, b = P.row_ref(r2, d2, stride, 0.1), slow_row(r2, d2, stride, 0.1)
        assert np.array_equal(a[2:], b[2:]) and np.allclose(a[:2], b[:2], rtol=1e-13, atol=0)
    # a contact threshold that sits exactly on a value: the comparison is strict
    assert P.row_ref(r, d, 1, 0.25)[2:].tolist() == [0, 42, 0] and P.row_ref(r, d, 1, 0.5)[2:].tolist() == [0, 0, 0]
    assert P.row_ref(r, d, 1, 0.2499)[2:].tolist() == [12, 42, 21]
    # NaN: on the stride-2 lattice (odd row, odd column) it poisons the sums and is not contact; off it, nothing changes
    clean = P.row_ref(r, d, 2, 0.0)
    on, off = d.copy(), d.copy()
    on[0, 7, 7] = np.nan            # was contact in both images
    off[0, 6, 7] = np.nan
    bad = P.row_ref(r, on, 2, 0.0)
    assert np.isnan(bad[:2]).all() and bad[2:].tolist() == [clean[2] - 1, clean[3], clean[4] - 1]
    assert np.array_equal(P.row_ref(r, off, 2, 0.0), clean) and np.isnan(P.row_ref(r, off, 1, 0.0)[:2]).all()
    on[0, 7, 7] = -np.inf           # -inf is below every threshold and still not contact
    bad = P.row_ref(r, on, 2, 0.0)
    assert np.isinf(bad[:2]).all() and bad[2:].tolist() == [clean[2] - 1, clean[3], clean[4] - 1]
    with pytest.raises(Exception):
        lattice_points((H, W), 0)


def test_level_schedule_middle_candidate_and_half_spans():
    from gelslim_depth_amd.mesh_depth import MeshDepthError, search_schedule
    half, counts, levels = (1.5e-3, 1.5e-3, 0.6), (7, 5, 9), 4
    spans, offs = search_schedule(half, counts, levels)
    assert spans.dtype == offs.dtype == np.float32 and spans.shape == (5, 3) and offs.shape == (4, 7 * 5 * 9, 3)
    assert np.array_equal(spans, P.half_spans(half, counts, levels))
    div = np.array([6, 4, 8], np.float32)
    for lvl in range(levels):
        assert np.array_equal(spans[lvl + 1], np.float32(2) * spans[lvl] / div)          # next half-span = this level's step
        assert np.array_equal(offs[lvl], P.offsets(spans[lvl + 1], counts))
    assert abs(float(spans[4, 2]) - 0.6 / 4 ** 4) < 1e-9 and abs(float(spans[4, 0]) - 1.5e-3 / 3 ** 4) < 1e-10
    centre = np.array([0.4e-3 + 0.9e-3, -1.0e-3, 0.65], np.float32)
    middle = (3 * 5 + 2) * 9 + 4
    for lvl in range(levels):
        cand = P.candidates(centre, spans[lvl + 1], counts)
        assert cand.dtype == np.float32 and cand[middle].tobytes() == centre.tobytes()          # bit for bit
        assert np.array_equal(cand, centre[None] + offs[lvl])
        # flat index (i1 * n2 + i2) * n3 + i3, each axis ascending, the corners at -half and (to a rounding) +half
        k = (6 * 5 + 0) * 9 + 8
        assert cand[k, 0] > centre[0] and cand[k, 1] < centre[1] and cand[k, 2] > centre[2]
        assert np.allclose(cand[0], centre - spans[lvl], rtol=0, atol=1e-6 * float(spans[lvl].max()))
        assert np.allclose(cand[-1], centre + spans[lvl], rtol=0, atol=1e-6 * float(spans[lvl].max()))
    for bad in ((6, 7, 9), (1, 7, 9), (7, 7), (7, 7, 9.0), 7):
        with pytest.raises(MeshDepthError):
            search_schedule(half, bad, levels)
    for bad_half in ((1.0, 2.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0)):
        with pytest.raises(MeshDepthError):
            search_schedule(bad_half, counts, levels)
    with pytest.raises(MeshDepthError):
        search_schedule(half, counts, 0)


def test_cost_kinds_and_the_tie_rule():
    from gelslim_depth_amd.mesh_depth import MeshDepthError, first_argmin, pose_cost
    nan = float("nan")
    rows = np.array([[[8.0, 4.0, 3, 4, 5], [2.0, 1.0, 3, 4, 5], [nan] * 5, [2.0, 1.0, 3, 4, 5], [0.5, 9.0, 0, 0, 0],
                      [math.inf, math.inf, 0, 7, 0]],
                     [[nan] * 5] * 6,
                     [[4.0, 2.0, 6, 6, 6]] * 6])
    t = torch.from_numpy(rows)
    kinds = ("mse", "l1", "iou", {"mse": 1.0, "iou": 0.25}, {"l1": 2.0})
    for kind in kinds:
        want = P.pose_cost_ref(rows, kind, 10)
        got = pose_cost(t, kind, 10)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want), kind
        assert not np.isnan(want).any()
        win = first_argmin(got)
        assert win.tolist() == np.argmin(want, axis=1).tolist() == torch.argmin(got, dim=1).tolist(), kind
    mse = pose_cost(t, "mse", 10).numpy()
    assert mse[0].tolist() == [0.8, 0.2, math.inf, 0.2, 0.05, math.inf] and first_argmin(pose_cost(t, "mse", 10)).tolist() == [4, 0, 0]
    iou = pose_cost(t, "iou", 10).numpy()
    assert iou[0].tolist() == [0.5, 0.5, math.inf, 0.5, 0.0, 1.0] and iou[2, 0] == 0.0
    # equal costs: the lowest index; +inf (a NaN row) never beats a finite cost; nothing finite: index 0
    assert first_argmin(pose_cost(t, "l1", 10)).tolist() == [1, 0, 0]
    assert first_argmin(torch.tensor([[math.inf, 3.0, 3.0], [math.inf, math.inf, 7.0]], dtype=torch.float64)).tolist() == [1, 2]
    for bad in ("rmse", {}, {"mse": 1.0, "dice": 1.0}, None):
        with pytest.raises(MeshDepthError):
            pose_cost(t, bad, 10)
    with pytest.raises(MeshDepthError):
        pose_cost(t.float(), "mse", 10)
    with pytest.raises(MeshDepthError):
        pose_cost(t, "mse", 0)


def test_pose_error_is_in_millimetres_and_wraps_the_angle():
    from gelslim_depth_amd.mesh_depth import pose_error
    pose = torch.tensor([[1.5e-3, -2e-3, 3.0], [0.0, 0.0, -3.0], [0.0, 1e-3, 0.25]], dtype=torch.float64)
    truth = torch.tensor([[0.5e-3, -1e-3, -3.0], [0.0, 0.0, 3.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    got = pose_error(pose, truth).numpy()
    want = np.array([[1.0, -1.0, 6.0 - 2 * math.pi], [0.0, 0.0, 2 * math.pi - 6.0], [0.0, 1.0, 0.25]])
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=0, atol=1e-12)
    assert np.allclose(got, P.pose_error_ref(pose.numpy(), truth.numpy()), rtol=0, atol=1e-12)
    edge = pose_error(torch.tensor([[0.0, 0.0, math.pi], [0.0, 0.0, -math.pi]], dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    assert edge[:, 2].tolist() == [math.pi, math.pi]          # (-pi, pi]
    assert pose_error(pose.float(), truth[0]).shape == (3, 3)


def test_the_twin_recovers_the_l_prism_pose():
    """The l-prism case of tests/test_gpu_mesh_pose.py by brute force: the best cost never rises, and the pose error stays within a
    third of the GPU test's bound, that is within max(the recorded twin error, the final step) per axis."""
    from test_gpu_mesh_pose import BOUND, FINAL_STEP, TWIN_ERROR
    res = P.run_case("lprism")
    trace = res["trace"]
    assert res["renders"] == 4 * 441 and len(trace) == 4 and np.all(np.diff(trace) <= 0), trace
    assert res["cost"] == trace[-1] == P.pose_cost_ref(res["row"], "mse", P.n_points(24, 31, 1))
    err = np.abs(res["error"])
    print("twin error (mm, mm, rad):", res["error"].tolist(), "final step:", res["final_step"].tolist())
    step = np.array([1e3 * res["final_step"][0], 1e3 * res["final_step"][1], res["final_step"][2]], np.float64)
    assert np.allclose(step, FINAL_STEP["lprism"], rtol=1e-6, atol=0)
    assert np.all(err <= np.asarray(TWIN_ERROR["lprism"])), (err, TWIN_ERROR["lprism"])
    assert np.all(err <= np.asarray(BOUND["lprism"]) / 3), (err, BOUND["lprism"])
