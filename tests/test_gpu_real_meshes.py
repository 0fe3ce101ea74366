"""GPU: gsd_mesh_depth_* and gsd_mesh_pose_* on the real object meshes of tests/golden/meshes/ (tests/real_mesh_cases.py): metres
and `pc_scale` 1000, 15..80 mm of object against a 12 x 16 mm image, a peg 40 mm off the origin, triangles of zero projected area
by the thousand, open meshes.  The yardsticks are the suite's own, in fp64 on the host, and none of them is the code under test:

  * renders: every value in raster_ref's [lo - slack, hi + slack], finite and <= 0, no pixel excluded -- test_gpu_mesh_depth.check's
    rule.  `slack` is that module's budget for the fp32 interpolation of q, stated in ulps of q: 1e-4 mm while the mesh's largest
    |q| is below 16 mm, doubling with every binade above, so 2e-4 mm for the half-thicknesses of 16..32 mm here
    (real_mesh_cases.slack_mm).  An interval must not hide a failure: per image at most 0.5 % of the pixels may have
    hi - lo > 1e-3 mm (asserted here, and without a GPU in tests/test_real_meshes_cpu.py),
  * Jacobian images: the brute-force twin (mesh_pose_refine_ref.point_terms) on the points it is certain about, 64 * 2^-53 * mag,
  * score and normal rows: fp64 host reductions of the device renders and Jacobian images that the two rules above pin,
    2 n 2^-53 relative to the sum of |terms|, counts exact.

`pytest -s` prints, per mesh, the poses, the contact pixels, the worst excess over [lo, hi], the widest-interval and uncertain
shares and the grid shapes; DESIGN.md section 16 quotes the worst of each."""
import functools
import shutil

import numpy as np
import pytest
import torch

import mesh_depth_ref as R
import mesh_pose_ref as P
import mesh_pose_refine_ref as PR
import real_mesh_cases as M
from test_gpu_mesh_depth import SIZES, hold
from test_gpu_mesh_pose import DEV, HEIGHT_MM
from test_gpu_mesh_pose_refine import EPS, two_steps_off

pytestmark = pytest.mark.gpu

HEX, PEG, P05, P32, KEY, MARBLE = M.NAMES
assert all(SIZES[size] == HEIGHT_MM for size in M.SIZES)


def md():
    from gelslim_depth_amd import mesh_depth
    return mesh_depth


@functools.lru_cache(maxsize=None)
def grid_of(name, plane=M.PLANE, cell=None, scale=None):
    return md().MeshGrid(M.mesh(name), M.pc_scale(name) if scale is None else scale, plane, DEV, cell_mm=cell)


def tensors(batch):
    poses = torch.tensor([pose for _, pose, _ in batch], dtype=torch.float32, device=DEV)
    widths = torch.tensor([g for _, _, g in batch], dtype=torch.float32, device=DEV)
    return poses, widths


def render(grid, batch, size, flip=False, invert=False):
    poses, widths = tensors(batch)
    return md().render_depth(grid, poses, widths, size, HEIGHT_MM, 0.0, flip, invert)


def check(name, plane, size, flip, invert, batch, grid=None, scale=None, what=""):
    """One launch held to raster_ref's intervals (of the mesh at `scale`, default the table's pc_scale).  Returns the images."""
    got = render(grid_of(name, plane, scale=scale) if grid is None else grid, batch, size, flip, invert).cpu().numpy().astype(np.float64)
    assert got.shape == (len(batch), 2, size[0], size[1])
    intervals = [M.interval(name, plane, pose, g, size, invert, scale) for _, pose, g in batch]
    shares = [M.wide_share(lo, hi) for lo, hi in intervals]
    for (label, pose, g), share in zip(batch, shares):
        assert share <= M.WIDE_CAP, (name, plane, size, label, pose, share)
    print(f"{name}{what} {size} {plane} invert={invert}: widest-interval share {max(shares):.4f}")
    hold(got, intervals, flip, M.slack_mm(M.q_max(name, plane)), f"{name}{what} {size} {plane} invert={invert}")
    return got


def check_contact(name, batch, got):
    """(a)..(d) touch, (d) also leaves pixels free, (e) and the width larger than the object are 0 everywhere."""
    for k, (label, pose, g) in enumerate(batch):
        if label in "abcd":
            assert (got[k] < 0).any(), (name, label, pose)
        if label == "d":
            assert (got[k] == 0).any(), (name, label, pose)
        if label in ("e", "wide"):
            assert not got[k].any(), (name, label, pose)


# ---- 1. renders against raster_ref ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.NAMES)
def test_every_pose_of_every_mesh_lies_in_the_fp64_interval(name):
    """(a)..(f) and a width larger than the object as one launch per image size, (b) once more through invert_affine; peg1 also
    with LR_flip.  The hexagonal plate at (a): one flat face under every pixel of both channels, 0.8 mm deep."""
    print(f"{name}: {grid_of(name)!r}")
    for plane, size, flip, invert, batch in M.launches(name):
        if plane != M.PLANE:
            continue
        got = check(name, plane, size, flip, invert, batch)
        check_contact(name, batch, got)
        if name == HEX and not invert:
            k = [label for label, _, _ in batch].index("a")
            assert np.abs(got[k] + M.INDENT_MM).max() <= M.slack_mm(M.q_max(name)), np.abs(got[k] + M.INDENT_MM).max()
    if name == PEG:          # LR_flip swaps the channels, bit for bit
        batch = M.cases(name)
        plain, flipped = render(grid_of(name), batch, M.SIZES[0]), render(grid_of(name), batch, M.SIZES[0], flip=True)
        assert torch.equal(flipped[:, 0], plain[:, 1]) and torch.equal(flipped[:, 1], plain[:, 0])


@pytest.mark.parametrize("plane", [p for p in R.PLANES if p != M.PLANE])
def test_every_other_plane_on_the_three_line_plate(plane):
    """Four of the eleven look at the plate's face (another axis order or sign: the fingers or the image axes swap), eight at its
    60 x 37 and 51 x 37 mm sides, where |q| reaches 30 mm."""
    for pl, size, flip, invert, batch in M.launches(P05):
        if pl == plane:
            got = check(P05, pl, size, flip, invert, batch)
            assert all((got[k] < 0).any() for k in range(len(batch))), plane


# ---- 2. pc_scale ------------------------------------------------------------------------------------------------------------------
def test_scaling_on_the_host_or_in_the_file_gives_the_same_interval():
    """The metre mesh with pc_scale = 1000 and the mesh multiplied by 1000 (rounded to fp32 once more) with pc_scale = 1 are both
    held to the metre mesh's interval: the extra rounding moves a vertex by at most 2^-24 of 40 mm, a fortieth of delta.  The two
    need not be equal bit for bit, and are not asked to be."""
    batch = [M.case(KEY, label) for label in "abd"]
    scaled = (M.mesh(KEY).astype(np.float64) * 1000.0).astype(np.float32)
    check(KEY, M.PLANE, (24, 31), False, False, batch, what=" pc_scale=1000")
    got = check(KEY, M.PLANE, (24, 31), False, False, batch, grid=md().MeshGrid(scaled, 1.0, M.PLANE, DEV), what=" x1000, pc_scale=1")
    check_contact(KEY, batch, got)


def test_a_negative_pc_scale_flips_every_triangle():
    """pc_scale = -1000: the object is reflected through the origin, every triangle's orientation flips (the record's signed area
    changes sign) and the fingers swap sides.  Held to raster_ref(tri, -1000, ...); the poses centre on the reflected centre."""
    assert abs(M.q_max(P05, M.PLANE, -1000.0) - M.q_max(P05)) < 1e-9
    batch = M.reflected_cases(P05)
    for size in M.SIZES:
        got = check(P05, M.PLANE, size, False, False, batch, scale=-1000.0, what=" pc_scale=-1000")
        check_contact(P05, batch, got)
    plain = render(grid_of(P05), [M.case(P05, "a")], (24, 31))
    assert not torch.equal(plain, render(grid_of(P05, scale=-1000.0), batch[:1], (24, 31)))


# ---- 3. grid independence and repeatability -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [KEY, P32])
def test_renders_do_not_depend_on_the_grid_or_the_batch(name):
    batch, size = M.cases(name), (40, 53)
    default = grid_of(name)
    base = render(default, batch, size)
    assert torch.equal(base, render(default, batch, size)) and base.min() < 0
    one, fine = grid_of(name, cell=1e6), grid_of(name, cell=default.cell_mm / 4)
    print(f"{name}: default {default!r}, one cell {one!r}, fine {fine!r}")
    assert one.shape == (1, 1) and fine.shape[0] > default.shape[0] and fine.pairs > default.pairs >= one.pairs
    for grid in (one, fine, md().MeshGrid(M.mesh(name), M.pc_scale(name), M.PLANE, DEV)):          # the last: a second build of the default
        assert torch.equal(base, render(grid, batch, size)), (name, grid)
    for k in range(len(batch)):
        assert torch.equal(render(default, batch[k:k + 1], size)[0], base[k]), (name, k)


# ---- 4. Jacobian images against the twin ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jacobian_image(name, size, label, invert):
    pose, g, _ = M.twin_image(name, size, label, invert)
    poses, widths = tensors([(label, pose, g)])
    J = md().render_depth_jacobian(grid_of(name), poses, widths, size, HEIGHT_MM, 0.0, False, invert)
    depth = md().render_depth(grid_of(name), poses, widths, size, HEIGHT_MM, 0.0, False, invert)
    assert J.shape == (1, 2, 3, *size) and J.dtype == torch.float64
    return J[0].cpu().numpy(), depth[0].cpu().numpy()


def test_jacobian_images_equal_the_twin_point_by_point():
    """test_gpu_mesh_pose_refine's rule on the real meshes.  Every axis of J exceeds 0.05 somewhere in every image; peg1 at (a)
    alone, exempt by name, has no slope along the aligned axis (real_mesh_cases.J_DEAD)."""
    for entry in M.JACOBIANS:
        name, size, label, invert = entry
        _, _, t = M.twin_image(*entry)
        J, depth = jacobian_image(*entry)
        certain = ~t["uncertain"]
        active, left_out = int(t["active"].sum()), int((t["uncertain"] & t["active"]).sum())
        assert active >= M.ACTIVE_MIN and left_out <= PR.UNCERTAIN_CAP * active, (entry, active, left_out)
        assert np.array_equal((depth < 0)[certain], t["active"][certain])
        assert not J[np.broadcast_to((depth == 0)[:, None], J.shape)].any()          # every inactive point: exactly 0
        diff, tol = np.abs(J - t["J"]), 64 * EPS * t["mag"]
        mask = np.broadcast_to(certain[:, None], J.shape)
        worst = (diff[mask] / np.maximum(tol[mask], 1e-300)).max()
        print(f"{entry}: {active} active points, {left_out} left out ({100.0 * left_out / active:.2f} %), largest |J| per axis "
              f"{[float(np.abs(J[:, k]).max()) for k in range(3)]}, worst |J - twin| / bound {worst:.3e}")
        assert np.all(diff[mask] <= tol[mask]), entry
        big = [float(np.abs(J[:, k]).max()) for k in range(3)]
        assert M.live_axes(name, label, big), (entry, big)


def test_a_flat_face_has_a_jacobian_of_exactly_zero():
    for size in M.SIZES:
        poses, widths = tensors([M.case(HEX, "a"), M.case(HEX, "b")])
        J = md().render_depth_jacobian(grid_of(HEX), poses, widths, size, HEIGHT_MM)
        depth = md().render_depth(grid_of(HEX), poses, widths, size, HEIGHT_MM)
        assert bool((depth[0] < 0).all()) and not bool(J.any())


# ---- 5. score and normal rows against the pinned renders ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(name, size=(24, 31), b=2, p=37, seed=0):
    """test_gpu_mesh_pose.problem around pose (a) of a real mesh: (observed (b, 2, H, W), candidates (b, p, 3), widths (b,)), different
    widths, seeded candidates within (1.5 mm, 1.5 mm, 0.1 rad) of (a) -- 0.1 rad swings the peg's centre, 40 mm from the origin, by
    4 mm --, D a render at another pose plus Gaussian noise of 0.05 mm."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = M.contact_width(name)
    widths = torch.tensor([g - 0.3 * k for k in range(b)], dtype=torch.float32, device=DEV)
    base = np.array([M.case(name, "a")[1]] * b)
    cand = base[:, None, :] + rng.uniform(-1, 1, (b, p, 3)) * np.array([1.5e-3, 1.5e-3, 0.1])
    cand = torch.from_numpy(cand.astype(np.float32)).to(DEV)
    seen = torch.from_numpy((base + np.array([[0.2e-3, -0.15e-3, 0.02], [-0.3e-3, 0.25e-3, -0.03]] * b)[:b]).astype(np.float32)).to(DEV)
    observed = md().render_depth(grid_of(name), seen, widths, size, HEIGHT_MM)
    noise = torch.from_numpy(rng.normal(0.0, 0.05, tuple(observed.shape)).astype(np.float32)).to(DEV)
    return (observed + noise).contiguous(), cand.contiguous(), widths


@pytest.mark.parametrize("name", [KEY, PEG])
def test_score_and_normal_rows_equal_the_renders_reduced_in_fp64(name):
    """The rules of test_rows_equal_the_render_reduced_in_fp64 and test_rows_equal_the_jacobian_images_reduced_in_fp64 in one pass
    over the same 74 device renders and Jacobian images."""
    size = (24, 31)
    observed, cand, widths = problem(name)
    b, p = cand.shape[:2]
    grid = grid_of(name)
    flat, w_flat = cand.reshape(-1, 3).contiguous(), widths.repeat_interleave(p).contiguous()
    depth = md().render_depth(grid, flat, w_flat, size, HEIGHT_MM).reshape(b, p, 2, *size).cpu().numpy()
    J = md().render_depth_jacobian(grid, flat, w_flat, size, HEIGHT_MM).reshape(b, p, 2, 3, *size).cpu().numpy()
    seen = observed.cpu().numpy()
    assert (depth < 0).any() and (seen < 0).any()
    for stride in (1, 2, 3):
        n = P.n_points(size[0], size[1], stride)
        score = md().score_poses(grid, observed, cand, widths, HEIGHT_MM, stride=stride)
        rows = md().pose_normal_rows(grid, observed, cand, widths, HEIGHT_MM, stride=stride)
        assert score.shape == (b, p, 5) and rows.shape == (b, p, 16) and score.dtype == rows.dtype == torch.float64
        assert torch.equal(rows[..., 0], score[..., 0]) and torch.equal(rows[..., 1], score[..., 3])
        score, rows = score.cpu().numpy(), rows.cpu().numpy()
        want = np.stack([np.stack([P.row_ref(depth[i, k], seen[i], stride, 0.0) for k in range(p)]) for i in range(b)])
        assert np.array_equal(score[..., 2:], want[..., 2:]), (name, stride)
        assert want[..., 3].max() > 0 and want[..., 2].max() > 0 and (want[..., 0] > 0).all()
        rel = np.abs(score[..., :2] - want[..., :2]) / want[..., :2]
        assert rel.max() <= 2 * n * EPS, (name, stride, rel.max())
        worst = 0.0
        for i in range(b):
            for k in range(p):
                terms = PR.normal_terms(depth[i, k], J[i, k], seen[i], stride)
                assert terms.shape == (16, n)
                total, scale = terms.sum(axis=1), np.abs(terms).sum(axis=1)
                assert rows[i, k, 1] == total[1]
                assert np.all(np.abs(rows[i, k] - total) <= 2 * n * EPS * scale), (name, stride, i, k)
                worst = max(worst, float((np.abs(rows[i, k] - total) / np.maximum(scale, 1e-300)).max()))
        assert np.abs(rows[..., 2:5]).max() > 0 and (rows[..., 6:9] > 0).any()
        print(f"{name} {size} stride {stride}: n = {n}, worst relative difference of the score sums {rel.max():.3e}, worst |normal row - host| / "
              f"sum |terms| {worst:.3e} (bound {2 * n * EPS:.3e})")
        # a candidate scored against its own render: exactly zero
        k = 11
        own = md().render_depth(grid, cand[:, k].contiguous(), widths, size, HEIGHT_MM)
        zero = md().score_poses(grid, own, cand, widths, HEIGHT_MM, stride=stride).cpu().numpy()
        for i in range(b):
            row = zero[i, k]
            assert row[0] == 0.0 and row[1] == 0.0 and row[2] == row[3] == row[4] > 0, (name, stride, i, row)


# ---- 6. a flat face does not break the refinement --------------------------------------------------------------------------------------
def test_refine_pose_on_a_flat_face_stays_where_it_started():
    """J is 0 under every pixel of the hexagonal plate, so the normal matrix is singular: the first pivot fails, the step is 0, every
    trial is the start again and never strictly better."""
    size = (24, 31)
    grid = grid_of(HEX)
    _, pose, g = M.case(HEX, "a")
    truth, width = tensors([("a", pose, g)])
    observed = md().render_depth(grid, truth, width, size, HEIGHT_MM)
    start = two_steps_off({"truth": pose})
    init = torch.tensor([start], dtype=torch.float32, device=DEV)
    assert not torch.equal(init, truth)
    res = md().refine_pose(grid, observed, width, init, 4, image_height_mm=HEIGHT_MM)
    for field in ("pose", "width", "cost", "normal_row", "trace", "last_step"):
        assert bool(torch.isfinite(getattr(res, field)).all()), field
    assert int(res.accepted[0]) == 0 and torch.equal(res.pose, init) and torch.equal(res.width, width)
    trace = res.trace[:, 0]
    assert trace.shape == (5,) and bool((trace == trace[0]).all()) and float(res.cost[0]) == float(trace[0])
    assert not bool(res.normal_row[0, 2:5].any()) and not bool(res.last_step.any())
    fit = md().refine_pose(grid, observed, width, init, 4, fit_width=True, image_height_mm=HEIGHT_MM)          # only the width has a slope
    assert bool(torch.isfinite(fit.trace).all()) and torch.equal(fit.pose, init)


# ---- 7. generate_depth_images_v1 on a real file -------------------------------------------------------------------------------------------
def test_generate_depth_images_v1_on_the_peg(tmp_path):
    import os
    data, meshes = tmp_path / "data", tmp_path / "meshes"
    data.mkdir()
    meshes.mkdir()
    shutil.copy(os.path.join(M.MESH_DIR, PEG + ".stl"), str(meshes / "peg1.stl"))
    g = M.contact_width(PEG)
    poses = torch.tensor([M.case(PEG, label)[1] for label in "abdf"] + [[0.0, 0.0, 0.0]], dtype=torch.float32)
    n = poses.shape[0]
    torch.save({"tactile_image": torch.zeros(n, 6, 24, 31), "base_tactile_image": torch.zeros(n, 6, 24, 31), "in_hand_pose": poses},
               str(data / "peg1_train.pt"))
    (tmp_path / "grasp_widths.txt").write_text(f"peg1: {g!r}\n")
    gen = md().DepthImageGenerator(str(meshes), ["peg1"], 1.0, str(data), str(tmp_path / "grasp_widths.txt"), image_size=(24, 31), batch=2)
    gen.generate_depth_images_v1(prompt=False)
    back = torch.load(str(data / "peg1_train.pt"), map_location="cpu")
    depth = back["depth_image"]
    assert depth.shape == (n, 2, 24, 31) and depth.dtype == torch.float32 and torch.equal(back["in_hand_pose"], poses)
    want = md().render_depth(grid_of(PEG), poses.to(DEV), torch.full((n,), g, device=DEV), (24, 31), HEIGHT_MM)
    assert torch.equal(depth, want.cpu())
    raw = depth[3]          # (f): the pose without the 40 mm offset sees the peg's end, part of the image is empty
    assert bool((raw < 0).any()) and bool((raw == 0).all(dim=0).any())
    assert depth[0].min() < -0.7
