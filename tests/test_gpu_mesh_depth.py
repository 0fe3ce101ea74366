"""GPU: gsd_mesh_depth_* (gelslim_depth_amd.mesh_depth) against DESIGN.md section 16 by brute force (tests/mesh_depth_ref.py).

Every GPU value must lie in raster_ref's [lo - 1e-4 mm, hi + 1e-4 mm]: the interval absorbs sixteen fp32 ulps of position (the
pixel-to-mesh map), the 1e-4 mm the fp32 interpolation of q (|q| < 10 mm: an ulp is 1e-6 mm).  No pixel is excluded."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import mesh_depth_ref as R

pytestmark = pytest.mark.gpu

SLACK_MM = 1e-4
SIZES = {(24, 31): 12.0, (40, 53): 12.0}          # image_size -> image_height_mm: the 5..7 mm objects span 0.4 .. 0.6 of it
THETAS = (0.0, 0.3, math.pi / 2, -2.5)
SHIFTS = ((0.2e-3, -0.1e-3), (6.0e-3, 0.3e-3), (30e-3, -25e-3))       # centred, half off the image, wholly off it (all zeros)


@functools.lru_cache(maxsize=None)
def mesh(name):
    return {"box": lambda: R.box((6.0, 5.0, 7.0), (0.5, 0.25, -0.125)),
            "sphere2": lambda: R.sphere(2, 3.0, (1.0, -0.5, 0.25)),
            "sphere4": lambda: R.sphere(4, 3.0, (1.0, -0.5, 0.25)),
            "torus": lambda: R.torus(2.4, 1.0, 20, 10, axis=1, centre=(0.0, 0.5, -0.25)),
            "lprism": lambda: R.l_prism(3.0, axis=0, centre=(0.25, 0.0, 0.5)),
            "ellipsoid": lambda: R.ellipsoid(2, (3.0, 2.5, 3.5), 0.12, (1.5, 0.75, -0.5))}[name]()


def widths_of(name, plane="+y+z"):
    """g = 0, a contact value (0.8 mm of indentation), larger than the object (all zeros)."""
    _, _, q, _ = R.prepare(mesh(name), 1.0, plane)
    qm = float(q.max())
    return (0.0, 2 * (qm - 0.8), 2 * qm + 1.0)


def product_poses(name):
    g = widths_of(name)
    return [((s[0], s[1], th), w) for th in THETAS for s in SHIFTS for w in g]


def cycled_poses(name, count):
    """`count` poses that run through every theta, shift and width, not the whole product."""
    g = widths_of(name)
    return [((SHIFTS[(i // 2) % 3][0], SHIFTS[(i // 2) % 3][1], THETAS[i % 4]), g[(i + 1) % 3]) for i in range(count)]


@functools.lru_cache(maxsize=None)
def interval(name, plane, pose, g, size, invert):
    tri = mesh(name)
    pose32 = tuple(float(np.float32(p)) for p in pose)           # what the device tensors hold
    return R.raster_ref(tri, 1.0, plane, pose32, float(np.float32(g)), size, SIZES[size], False, invert)


@functools.lru_cache(maxsize=None)
def grid_of(name, plane="+y+z", cell=None):
    from gelslim_depth_amd.mesh_depth import MeshGrid
    return MeshGrid(mesh(name), 1.0, plane, "cuda:0", cell_mm=cell)


def render(name, cases, size, plane="+y+z", flip=False, invert=False, cell=None, **kw):
    from gelslim_depth_amd.mesh_depth import render_depth
    poses = torch.tensor([c[0] for c in cases], dtype=torch.float32, device="cuda:0")
    widths = torch.tensor([c[1] for c in cases], dtype=torch.float32, device="cuda:0")
    return render_depth(grid_of(name, plane, cell), poses, widths, size, SIZES[size], 0.0, flip, invert, **kw)


def hold(got, intervals, flip, slack, what):
    """The rule, for any mesh: image k of `got` (B, 2, H, W) lies in [lo - slack, hi + slack] of intervals[k], every pixel, and is
    finite and <= 0.  Returns (worst excess over [lo, hi], contact pixels)."""
    assert got.shape[0] == len(intervals) and np.isfinite(got).all()
    worst, contact = -np.inf, 0
    for k, (lo, hi) in enumerate(intervals):
        assert got[k].shape == lo.shape == hi.shape
        if flip:
            lo, hi = lo[::-1], hi[::-1]
        over = np.maximum(got[k] - hi, lo - got[k])
        worst = max(worst, float(over.max()))
        contact += int((got[k] < 0).sum())
        assert np.all(got[k] <= 0)
    print(f"{what} flip={flip}: {len(intervals)} poses, {contact} contact pixels, worst excess over [lo, hi] {worst:.3e} mm "
          f"(slack {slack:.0e})")
    assert worst <= slack, (what, flip, worst)
    return worst, contact


def check(name, cases, size, plane="+y+z", flip=False, invert=False):
    got = render(name, cases, size, plane, flip, invert).cpu().numpy().astype(np.float64)
    assert got.shape == (len(cases), 2, size[0], size[1])
    intervals = [interval(name, plane, tuple(pose), g, size, invert) for pose, g in cases]
    _, contact = hold(got, intervals, flip, SLACK_MM, f"{name} {size} {plane} invert={invert}")
    return got, contact


@pytest.mark.parametrize("name", ["box", "lprism"])
def test_few_large_triangles_whole_product_of_poses(name):
    """box: 12 triangles that span many cells; L-prism: vertical walls and a degenerate triangle.  Every theta x shift x width."""
    cases = product_poses(name)
    got, contact = check(name, cases, (24, 31))
    assert contact > 0
    for k, (pose, g) in enumerate(cases):
        if pose[0] == SHIFTS[2][0] or g == widths_of(name)[2]:
            assert not got[k].any(), (pose, g)                  # wholly off the image / fingers wider than the object
    check(name, cases[::3], (40, 53))
    check(name, [(R.inverted_pose(p), g) for p, g in cases[1::3]], (24, 31), invert=True)


def test_icospheres_one_and_five_poses_per_launch():
    five = cycled_poses("sphere2", 12)[:5]
    assert len({c[0] for c in five}) == 5
    _, contact = check("sphere2", five, (40, 53))
    assert contact > 0
    check("sphere2", cycled_poses("sphere2", 12)[5:], (24, 31))
    one = [((0.2e-3, -0.1e-3, 0.3), widths_of("sphere4")[1])]
    got, contact = check("sphere4", one, (40, 53))                           # 5,120 triangles, N = 1
    assert contact > 50 and abs(got.min() + 0.8) < 0.02
    check("sphere4", [((3.0e-3, 0.3e-3, -2.5), 0.0)], (24, 31), invert=True)


def test_torus_takes_the_outer_layer():
    cases = cycled_poses("torus", 7) + [((0.2e-3, -0.1e-3, 0.3), 0.0)]
    got, contact = check("torus", cases, (40, 53))
    assert contact > 0
    # the ring stands on edge (its axis lies in the image plane), so a line of sight crosses up to four layers; with g = 0 each
    # finger must report the outermost one, whose crest is the ring's outer radius 2.4 + 1.0 (an inner layer would give <= 1.4)
    for ch in (0, 1):
        assert -3.4 <= got[-1, ch].min() < -3.3, got[-1, ch].min()


@pytest.mark.parametrize("plane", R.PLANES)
def test_every_plane_flip_and_pose_sense_on_the_ellipsoid(plane):
    g = widths_of("ellipsoid", plane)[1]
    cases = [((0.8e-3, -0.5e-3, 0.4), g), ((-1.5e-3, 1.0e-3, -2.5), 0.5 * g)]
    for flip in (False, True):
        _, contact = check("ellipsoid", cases, (24, 31), plane, flip, False)
        assert contact > 0
        check("ellipsoid", [(R.inverted_pose(p), w) for p, w in cases], (24, 31), plane, flip, True)


def test_renders_are_bitwise_reproducible_and_do_not_depend_on_the_grid():
    from gelslim_depth_amd.mesh_depth import MeshGrid
    for name in ("box", "sphere4", "torus", "lprism"):
        cases = cycled_poses(name, 5)
        base = render(name, cases, (40, 53))
        assert torch.equal(base, render(name, cases, (40, 53)))
        default = grid_of(name)
        cells = (1e6, default.cell_mm / 4)
        one, fine = grid_of(name, cell=cells[0]), grid_of(name, cell=cells[1])
        assert one.shape == (1, 1) and fine.shape[0] > default.shape[0] and fine.pairs > default.pairs >= one.pairs
        print(f"{name}: default {default!r}, fine {fine!r}")
        for cell in cells:
            assert torch.equal(base, render(name, cases, (40, 53), cell=cell)), (name, cell)
        assert base.min() < 0
        # a second build of the same grid (another list order) renders the same bits
        again = MeshGrid(mesh(name), 1.0, "+y+z", "cuda:0")
        from gelslim_depth_amd.mesh_depth import render_depth
        poses = torch.tensor([c[0] for c in cases], dtype=torch.float32, device="cuda:0")
        widths = torch.tensor([c[1] for c in cases], dtype=torch.float32, device="cuda:0")
        assert torch.equal(base, render_depth(again, poses, widths, (40, 53), SIZES[(40, 53)]))


def test_out_is_written_in_place_and_batch_rows_equal_single_renders():
    cases = cycled_poses("sphere2", 5)
    base = render("sphere2", cases, (24, 31))
    out = torch.full((5, 2, 24, 31), 7.0, device="cuda:0")
    ret = render("sphere2", cases, (24, 31), out=out)
    assert ret is out and torch.equal(out, base)
    for k in range(5):
        assert torch.equal(render("sphere2", cases[k:k + 1], (24, 31))[0], base[k]), k
    flipped = render("sphere2", cases, (24, 31), flip=True)
    assert torch.equal(flipped[:, 0], base[:, 1]) and torch.equal(flipped[:, 1], base[:, 0])


def test_cell_size_knob(monkeypatch):
    from gelslim_depth_amd.mesh_depth import MeshGrid
    default = grid_of("sphere4")
    assert 4.0 <= default.pairs / (default.shape[0] * default.shape[1]) <= 24.0, default       # about 8-16 per occupied cell
    monkeypatch.setenv("GSD_MESH_CELL_MM", "0.75")
    forced = MeshGrid(mesh("sphere2"), 1.0, "+y+z", "cuda:0", cell_mm=3.0)
    assert abs(forced.cell_mm - 0.75) < 1e-6


@pytest.mark.parametrize("listed", ["None", "number"])
def test_generate_depth_images_v1_end_to_end(tmp_path, listed):
    from gelslim_depth_amd.dataset import DeviceDataset
    from gelslim_depth_amd.mesh_depth import DepthImageGenerator, MeshGrid, render_depth
    data, meshes = tmp_path / "data", tmp_path / "meshes"
    data.mkdir()
    meshes.mkdir()
    tri = mesh("sphere2")
    R.write_stl_binary(str(meshes / "obj.stl"), tri)
    R.write_stl_ascii(str(meshes / "other.stl"), mesh("box"))
    poses = torch.tensor([[0.2e-3, -0.1e-3, 0.3], [1e-3, 0.5e-3, -2.5], [0.0, 0.0, 0.0], [-2e-3, 1e-3, 1.0]])
    own = torch.tensor([4.0, 4.5, 5.0, 3.5])
    torch.save({"tactile_image": torch.zeros(4, 6, 24, 31), "base_tactile_image": torch.zeros(4, 6, 24, 31), "in_hand_pose": poses,
                "grasp_widths": own}, str(data / "obj_train.pt"))
    torch.save({"untouched": torch.ones(1)}, str(data / "other_train.pt"))
    (tmp_path / "grasp_widths.txt").write_text("other: 1.0\nobj: " + ("None" if listed == "None" else "4.25") + "\n")
    gen = DepthImageGenerator(str(meshes), ["obj"], 1.0, str(data), str(tmp_path / "grasp_widths.txt"), image_size=(24, 31),
                              grasp_width_offset=0.25, batch=3)
    gen.generate_depth_images_v1(prompt=False)
    assert sorted(os.listdir(data)) == ["obj_train.pt", "other_train.pt"]
    assert list(torch.load(str(data / "other_train.pt"))) == ["untouched"]
    back = torch.load(str(data / "obj_train.pt"), map_location="cpu")
    depth = back["depth_image"]
    assert depth.shape == (4, 2, 24, 31) and depth.dtype == torch.float32 and depth.device.type == "cpu"
    assert torch.equal(back["in_hand_pose"], poses) and torch.equal(back["grasp_widths"], own)
    widths = own if listed == "None" else torch.full((4,), 4.25)
    want = render_depth(MeshGrid(tri, 1.0, "+y+z", "cuda:0"), poses.cuda(), widths.cuda(), (24, 31), 12, 0.25)
    assert torch.equal(depth, want.cpu()) and depth.min() < -0.3
    right, left = gen.generate_depth_image(str(meshes / "obj.stl"), poses[1, 0], poses[1, 1], poses[1, 2], widths[1] + 0.25)
    assert torch.equal(right.cpu(), depth[1, 1]) and torch.equal(left.cpu(), depth[1, 0])
    ds = DeviceDataset(directory=str(data), pt_file_list=["obj_train.pt"], device="cuda:0")
    assert tuple(ds.entire_dataset["depth_image"].shape) == (8, 1, 12, 15) and len(ds) == 8
    assert ds.depth_normalization_parameters[0] < 0


def test_refusals_raise_the_package_error_and_write_nothing():
    from gelslim_depth_amd._lib import GsdError
    from gelslim_depth_amd.mesh_depth import DepthImageGenerator, MeshDepthError, MeshGrid, render_depth
    grid = grid_of("box")
    poses = torch.zeros((3, 3), device="cuda:0")
    widths = torch.tensor([4.0, 4.0, -0.5], device="cuda:0")
    out = torch.full((3, 2, 24, 31), 7.0, device="cuda:0")
    with pytest.raises(MeshDepthError) as e:                                   # negative g: a ValueError and the package's error
        render_depth(grid, poses, widths, (24, 31), 12.0, out=out)
    assert isinstance(e.value, ValueError) and isinstance(e.value, GsdError)
    with pytest.raises(GsdError):                                              # ... through the offset as well
        render_depth(grid, poses, widths.abs(), (24, 31), 12.0, grasp_width_offset=-4.5, out=out)
    with pytest.raises(GsdError):                                              # CPU tensors
        render_depth(grid, poses.cpu(), widths.abs().cpu(), (24, 31), 12.0, out=out)
    with pytest.raises(GsdError):
        render_depth(grid, poses, widths.abs().cpu(), (24, 31), 12.0, out=out)
    with pytest.raises(GsdError):                                              # mismatched N
        render_depth(grid, poses, widths.abs()[:2].contiguous(), (24, 31), 12.0, out=out)
    with pytest.raises(GsdError):
        render_depth(grid, poses[:2].contiguous(), widths.abs()[:2].contiguous(), (24, 31), 12.0, out=out)
    with pytest.raises(GsdError):                                              # an empty mesh
        MeshGrid(np.zeros((0, 3, 3), np.float32), 1.0, "+y+z", "cuda:0")
    bad = mesh("box").copy()
    bad[3, 1, 2] = np.inf
    with pytest.raises(GsdError):                                              # a non-finite vertex
        MeshGrid(bad, 1.0, "+y+z", "cuda:0")
    with pytest.raises(GsdError):
        MeshGrid(mesh("box"), 1.0, "+y+z", "cpu")
    with pytest.raises(ValueError, match="Invalid gelslim_plane"):
        MeshGrid(mesh("box"), 1.0, "+x+x", "cuda:0")
    gen = DepthImageGenerator(".", None, 1.0, ".", "none.txt", image_size=(24, 31))
    with pytest.raises(ValueError):
        gen.generate_depth_image(grid, 0.0, 0.0, 0.0, -1.0)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # validate=False never reads the widths back: the refused sample is NaN, the others are rendered
    got = render_depth(grid, poses, widths, (24, 31), 12.0, validate=False)
    assert bool(torch.isnan(got[2]).all()) and bool(torch.isfinite(got[:2]).all()) and got[:2].min() < 0


# ---- the cell lists -----------------------------------------------------------------------------------------------------------
# cells per axis at 1 mm: one cell, then the counts around the multiples 4096 and 8192 of the scan's pass of 2048 counts: one short
# of two passes, exactly two, one count in a third pass, two counts in a fifth (8193 = 3 * 2731 needs an axis of 2731 cells, more
# than the 2048 allowed: 8194 is the nearest count above 8192)
@pytest.mark.parametrize("nx, ny, ncells", ((1, 1, 1), (63, 65, 4095), (64, 64, 4096), (17, 241, 4097), (34, 241, 8194)))
def test_cell_lists_across_the_scan_pass_boundary(nx, ny, ncells, monkeypatch):
    from gelslim_depth_amd.mesh_depth import MeshGrid
    monkeypatch.delenv("GSD_MESH_CELL_MM", raising=False)
    tri = R.cell_list_mesh((4, nx, ny))          # "+y+z": x is the perpendicular axis, the grid's x runs along y, its y along z
    one = MeshGrid(tri, 1.0, "+y+z", "cuda:0", cell_mm=1000.0)
    assert one.shape == (1, 1)
    listed = np.sort(one.list.cpu().numpy())
    # the two faces seen face-on and the three tilted triangles; the eight walls seen edge-on and the degenerate one are skipped
    assert np.array_equal(listed, np.nonzero(one.records[:, 9].cpu().numpy() != 0)[0]) and listed.tolist() == [0, 1, 2, 3, 13, 14, 15]
    grid = MeshGrid(tri, 1.0, "+y+z", "cuda:0", cell_mm=1.0)
    assert grid.shape == (ny, nx) and nx * ny == ncells
    g = grid.grid
    lo, hi = R.grid_cell_ranges(grid.records.cpu().numpy(), g.x0, g.y0, g.inv_cell, nx, ny)
    cells = grid.cells.cpu().numpy()
    R.check_cell_lists(cells, grid.list.cpu().numpy(), grid.pairs, (nx, ny), len(tri), listed, lo, hi)
    assert ncells == 1 or len(np.unique(np.diff(cells[2:2 + ncells + 1]))) >= 3      # the counts differ from cell to cell
