"""GPU: gelslim_depth_amd.touch_fusion against its numpy twin (tests/touch_fusion_ref.py), bit for bit: integration (acc and weight),
extraction (count, order, coordinates), the layouts, the absence of host reads, refusals, and a reconstruction from rendered touches
held to the derived bound of DESIGN.md section 24."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mesh_depth_ref as R
import touch_fusion_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HEIGHT_MM = 12.0
SLACK_MM = 1e-4          # test_gpu_mesh_depth's: the fp32 interpolation of q in render_depth
POSES = ((1.1e-3, -0.7e-3, 0.4), (-0.6e-3, 0.9e-3, -1.3), (0.2e-3, -0.1e-3, 0.0), (0.4e-3, 0.5e-3, 2.2), (-1.0e-3, -0.3e-3, 0.9))
MESHES = {"sphere": lambda: R.sphere(3, 4.0, (0.7, -0.4, 0.3)), "ellipsoid": lambda: R.ellipsoid(3), "l_prism": lambda: R.l_prism()}
WIDTHS = {"sphere": (6.0, 6.5, 5.8, 7.0, 6.2), "ellipsoid": (8.0, 8.5, 9.0, 7.6, 8.2), "l_prism": (2.0, 2.4, 1.6, 2.2, 2.6)}
_CACHE = {}


def rendered(name, size, plane="+y+z"):
    """(tri, grid, depth (5, 2, H, W) on the device, widths, poses): rendered once per (mesh, size, plane)."""
    from gelslim_depth_amd.mesh_depth import MeshGrid, render_depth
    key = (name, size, plane)
    if key not in _CACHE:
        tri = MESHES[name]()
        grid = MeshGrid(tri, 1.0, plane, device=DEV)
        poses = torch.tensor(POSES, device=DEV, dtype=torch.float32)
        widths = torch.tensor(WIDTHS[name], device=DEV, dtype=torch.float32)
        depth = render_depth(grid, poses, widths, image_size=size, image_height_mm=HEIGHT_MM)
        assert float(depth.min()) < -0.2
        _CACHE[key] = (tri, grid, depth, widths, poses)
    return _CACHE[key]


def lattice(tri, dims, h):
    """The origin that centres `dims` voxels of spacing h on the mesh's box."""
    v = tri.reshape(-1, 3).astype(np.float64)
    mid = 0.5 * (v.min(axis=0) + v.max(axis=0))
    return tuple(float(m - 0.5 * h * (n - 1)) for m, n in zip(mid, dims))


def bits(t):
    return t.detach().cpu().numpy().tobytes()


# name, image size, voxels, h, K, LR_flip, weights, carve, offset, contact_depth, transforms, bad pixels
CASES = [
    ("sphere", (24, 31), (21, 18, 14), 0.7, 1, False, False, 1.0, 0.0, 0.0, "pose", False),
    ("sphere", (40, 53), (37, 29, 23), 0.4, 5, False, True, 0.25, 0.0, 0.0, "pose", False),
    ("ellipsoid", (24, 31), (37, 29, 23), 0.55, 2, True, False, 1.0, 0.3, 0.0, "pose", True),
    ("ellipsoid", (40, 53), (21, 18, 14), 0.9, 5, False, True, 0.5, -0.2, 0.05, "se3", False),
    ("l_prism", (24, 31), (21, 18, 14), 0.45, 5, True, True, 2.0, 0.0, 0.02, "se3", True),
    ("l_prism", (40, 53), (37, 29, 23), 0.3, 2, False, False, 1.0, 0.1, 0.0, "edge", False),
    ("sphere", (24, 31), (37, 29, 23), 0.4, 5, False, False, 1.0, 0.0, 0.0, "edge", True),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1][0]}-{c[2][0]}-K{c[4]}-{c[10]}" for c in CASES])
def test_integration_equals_the_twin_bit_for_bit(case):
    """acc and weight of one call with the cull, one without it and a split into two calls, against the twin.  `edge` moves touch 0
    so that its footprint only partly meets the volume and touch 1 so that it misses it; `se3` composes a general rotation and
    shift into every map; bad pixels are NaN, +inf and -inf; a K = 5 case carries one negative width (validate=False)."""
    from gelslim_depth_amd.touch_fusion import TouchVolume, integrate_touches, touch_transforms
    name, size, dims, h, k, flip, weighted, carve, offset, cdepth, kind, bad = case
    tri, grid, depth, widths, poses = rendered(name, size)
    depth, widths = depth[:k].clone(), widths[:k].clone()
    if flip:
        depth = depth.flip(1).contiguous()
    if bad:
        depth[0, 0, size[0] // 2, size[1] // 2] = float("nan")
        depth[0, 1, size[0] // 2 - 2, size[1] // 2 + 1] = float("inf")
        depth[k - 1, 0, size[0] // 2 + 1, size[1] // 2 - 3] = float("-inf")
        depth[k - 1, 1, 3:5, :] = float("nan")
    if k == 5:
        widths[3] = -1.0
    rows = touch_transforms(poses[:k], grid=grid).cpu().numpy()
    if kind == "se3":
        rows = np.stack([T.compose(r, T.rotation((0.3, -1.0, 0.5), 0.2 + 0.3 * j), (0.4, -0.3 * j, 0.2)) for j, r in enumerate(rows)])
    if kind == "edge":
        rows[0, 3] += 0.45 * HEIGHT_MM
        rows[1 % k, 7] += 500.0 if k > 1 else 0.0
    weights = torch.tensor([1.0, 0.5, 2.0, 1.5, 0.75][:k], device=DEV) if weighted else None
    tau = 2.5 * h
    origin = lattice(tri, dims, h)
    kw = dict(image_height_mm=HEIGHT_MM, grasp_width_offset=offset, LR_flip=flip, contact_depth=cdepth, carve_weight=carve, validate=False)
    rows_dev = torch.from_numpy(rows).to(DEV)
    got = {}
    for cull in (True, False):
        vol = TouchVolume(origin, h, dims, tau, device=DEV)
        assert integrate_touches(vol, depth, widths, rows_dev, weights=weights, cull=cull, **kw) is vol
        got[cull] = (bits(vol.acc), bits(vol.weight))
    want = T.integrate(np.zeros(dims[::-1], np.float32), np.zeros(dims[::-1], np.float32), origin, h, tau, depth.cpu().numpy(), widths.cpu().numpy(),
                       rows, HEIGHT_MM, offset, flip, cdepth, carve, None if weights is None else weights.cpu().numpy())
    seen, inside = int((want[1] > 0).sum()), int((want[0] < 0).sum())
    diff = np.abs(np.frombuffer(got[True][0], np.float32).reshape(dims[::-1]) - want[0])
    print(f"{name} {size} {dims}: {seen} observed voxels, {inside} negative; acc differs from the twin in {int((diff > 0).sum())} voxels, by "
          f"{np.nanmax(diff):.3e} at most")
    assert seen > 200 and inside > 10
    assert got[True] == got[False], "the cull changed a bit"
    assert got[True][0] == want[0].tobytes() and got[True][1] == want[1].tobytes()
    if k > 1:
        j = 2 if k == 5 else 1
        vol = TouchVolume(origin, h, dims, tau, device=DEV)
        integrate_touches(vol, depth[:j], widths[:j], rows_dev[:j], weights=None if weights is None else weights[:j], **kw)
        integrate_touches(vol, depth[j:], widths[j:], rows_dev[j:], weights=None if weights is None else weights[j:], **kw)
        assert (bits(vol.acc), bits(vol.weight)) == got[True], f"{k} touches differ from {j} + {k - j}"
    # (K, 4, 4) transforms are the same rows; reset clears the state
    vol = TouchVolume(origin, h, dims, tau, device=DEV)
    m = np.zeros((k, 4, 4))
    m[:, :3, :], m[:, 3, 3] = rows.reshape(k, 3, 4), 1.0
    integrate_touches(vol, depth, widths, m, weights=weights, **kw)
    assert (bits(vol.acc), bits(vol.weight)) == got[True]
    vol.reset()
    assert float(vol.acc.abs().max()) == 0.0 and float(vol.weight.max()) == 0.0


def ulps(a, b):
    """Largest difference of two fp32 arrays in units of the last place (of the bit patterns; equal signs assumed where it matters)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max()) if a.size else 0


def device_volume(acc, weight, origin, h, tau=None):
    from gelslim_depth_amd.touch_fusion import TouchVolume
    nz, ny, nx = acc.shape
    vol = TouchVolume(origin, h, (nx, ny, nz), 2.0 * h if tau is None else tau, device=DEV)
    vol.acc.copy_(torch.from_numpy(np.ascontiguousarray(acc)))
    vol.weight.copy_(torch.from_numpy(np.ascontiguousarray(weight)))
    return vol


def fused_state():
    """The twin's volume of case 1 (sphere, 40 x 53, five weighted touches): weights differ from voxel to voxel."""
    name, size, dims, h, k, flip, _, carve, offset, cdepth, _, _ = CASES[1]
    tri, grid, depth, widths, poses = rendered(name, size)
    from gelslim_depth_amd.touch_fusion import touch_transforms
    rows = touch_transforms(poses, grid=grid).cpu().numpy()
    origin = lattice(tri, dims, h)
    zero = np.zeros(dims[::-1], np.float32)
    acc, weight = T.integrate(zero, zero, origin, h, 2.5 * h, depth.cpu().numpy(), widths.cpu().numpy(), rows, HEIGHT_MM, carve_weight=carve,
                              weights=np.asarray([1.0, 0.5, 2.0, 1.5, 0.75], np.float32))
    return acc, weight, origin, h


@pytest.mark.parametrize("what", ["sphere", "torus", "fused", "fused-min-weight"])
def test_extraction_equals_the_twin_in_count_order_and_bits(what):
    from gelslim_depth_amd import _lib as L
    from gelslim_depth_amd.touch_fusion import extract_surface
    if what in ("sphere", "torus"):
        acc, weight = T.analytic(what)
        origin, h, mw = T.ANALYTIC_ORIGIN, T.ANALYTIC_H, 0.0
    else:
        acc, weight, origin, h = fused_state()
        mw = 1.25 if what == "fused-min-weight" else 0.0
    want, want_cell = T.extract(acc, weight, origin, h, mw)
    vol = device_volume(acc, weight, origin, h)
    got = extract_surface(vol, min_weight=mw, cells=True)
    n = len(want)
    print(f"{what}: {int(got.count)} triangles on the device, {n} in the twin")
    assert n > 500 and int(got.count) == n and tuple(got.triangles.shape) == (n, 3, 3) and got.count.dtype == torch.int64
    tri = got.triangles.cpu().numpy()
    assert np.array_equal(got.cell.cpu().numpy(), want_cell), "order"
    print(f"  coordinates differ by {ulps(tri, want)} ulp at most")
    assert tri.tobytes() == want.tobytes()
    assert got.vertices().shape == (3 * n, 3) and not got.padded
    # a repeated call, and one without `cell`
    again = extract_surface(vol, min_weight=mw)
    assert again.cell is None and bits(again.triangles) == tri.tobytes()
    # padded layouts: below, at and above the count
    for m in (n - 37, n, n + 41):
        pad = extract_surface(vol, min_weight=mw, max_triangles=m, cells=True)
        ptri, pcell = T.padded(want, want_cell, m)
        assert int(pad.count) == n and pad.padded and tuple(pad.triangles.shape) == (m, 3, 3)
        assert bits(pad.triangles) == ptri.tobytes() and np.array_equal(pad.cell.cpu().numpy(), pcell), m
    # a recycled buffer: rows beyond the triangles are rewritten, rows beyond `rows` are left alone
    m = n + 5
    buf = torch.full((m + 3, 3, 3), 7.0, device=DEV)
    cell = torch.full((m + 3,), 7, device=DEV, dtype=torch.int32)
    words = int(L.lib.gsd_touch_extract_workspace(C.byref(vol.volume)))
    ws = torch.empty((words,), device=DEV, dtype=torch.int32)
    total = torch.zeros((1,), device=DEV, dtype=torch.int64)
    L.check(L.lib.gsd_touch_extract_count(C.byref(vol.volume), vol.acc.data_ptr(), vol.weight.data_ptr(), mw, total.data_ptr(), ws.data_ptr(), words,
                                          L.stream_ptr()), "count")
    L.check(L.lib.gsd_touch_extract_write(C.byref(vol.volume), vol.acc.data_ptr(), vol.weight.data_ptr(), mw, m, m, buf.data_ptr(), cell.data_ptr(),
                                          ws.data_ptr(), words, L.stream_ptr()), "write")
    assert int(total) == n and int(ws[:2].view(torch.int64)) == n
    ptri, pcell = T.padded(want, want_cell, m)
    assert bits(buf[:m]) == ptri.tobytes() and np.array_equal(cell[:m].cpu().numpy(), pcell)
    assert float(buf[m:].min()) == 7.0 and float(buf[m:].max()) == 7.0 and int(cell[m:].min()) == 7
    # packed into a buffer that is too short: the row count guards every store
    buf.fill_(7.0)
    L.check(L.lib.gsd_touch_extract_write(C.byref(vol.volume), vol.acc.data_ptr(), vol.weight.data_ptr(), mw, 0, 100, buf.data_ptr(), None,
                                          ws.data_ptr(), words, L.stream_ptr()), "write")
    assert bits(buf[:100]) == want[:100].tobytes() and float(buf[100:].min()) == 7.0
    assert L.lib.gsd_touch_extract_write(C.byref(vol.volume), vol.acc.data_ptr(), vol.weight.data_ptr(), mw, 0, 100, buf.data_ptr(), None,
                                         ws.data_ptr(), words - 1, L.stream_ptr()) == L.GSD_ERR_WORKSPACE


def test_a_volume_without_a_surface_gives_no_triangles():
    from gelslim_depth_amd.touch_fusion import TouchVolume, extract_surface
    vol = TouchVolume((0, 0, 0), 0.5, (9, 8, 7), 1.0, device=DEV)
    assert int(extract_surface(vol).count) == 0          # nothing observed
    vol.acc.fill_(1.0)
    vol.weight.fill_(1.0)
    got = extract_surface(vol, cells=True)
    assert int(got.count) == 0 and tuple(got.triangles.shape) == (0, 3, 3) and tuple(got.cell.shape) == (0,)
    pad = extract_surface(vol, max_triangles=5, cells=True)
    assert int(pad.count) == 0 and bool(torch.isnan(pad.triangles).all()) and bool((pad.cell == -1).all())
    assert bool(torch.isnan(TouchVolume((0, 0, 0), 0.5, (3, 3, 3), 1.0, device=DEV).tsdf()).all()) and float(vol.tsdf().min()) == 1.0


def test_a_scan_of_more_than_one_pass_equals_the_slabs_of_the_same_field():
    """106 x 104 x 102 voxels are 1,092,315 cells: 4267 blocks, more than one pass of the block-total scan.  The order contract
    makes the whole extraction the concatenation of the extractions of z slabs that share one voxel layer.  The spacing and the
    origin are multiples of 1/8, so a slab's voxel coordinates are the whole volume's exactly."""
    from gelslim_depth_amd import _lib as L
    from gelslim_depth_amd.touch_fusion import TouchVolume, extract_surface
    dims, h, origin = (106, 104, 102), 0.125, (-6.625, -6.5, -6.375)
    assert (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1) > L.GSD_TOUCH_EXTRACT_SCAN_PASS * L.GSD_TOUCH_EXTRACT_BLOCK
    ax = [origin[a] + h * torch.arange(dims[a], device=DEV, dtype=torch.float64) for a in range(3)]
    f = torch.sqrt((ax[0][None, None, :] - 0.013) ** 2 + (ax[1][None, :, None] + 0.021) ** 2 + (ax[2][:, None, None] - 0.007) ** 2) - 4.0
    whole = TouchVolume(origin, h, dims, 1.0, device=DEV)
    whole.acc.copy_(f.to(torch.float32))
    whole.weight.fill_(1.0)
    got = extract_surface(whole, cells=True)
    n = int(got.count)
    tris, cells = [], []
    cuts = (0, 30, 50, 51, 70, dims[2] - 1)          # the sphere spans the layers 19 .. 83: every slab holds a part of it
    for z0, z1 in zip(cuts[:-1], cuts[1:]):
        slab = TouchVolume((origin[0], origin[1], origin[2] + h * z0), h, (dims[0], dims[1], z1 - z0 + 1), 1.0, device=DEV)
        slab.acc.copy_(whole.acc[z0:z1 + 1])
        slab.weight.fill_(1.0)
        part = extract_surface(slab, cells=True)
        tris.append(part.triangles)
        cells.append(part.cell + z0 * (dims[0] - 1) * (dims[1] - 1))
    print(f"{n} triangles, {[len(t) for t in tris]} in the slabs")
    assert n > 50000 and sum(len(t) for t in tris) == n
    assert torch.equal(torch.cat(cells), got.cell) and bits(torch.cat(tris)) == bits(got.triangles)
    assert min(len(t) for t in tris) > 0


def test_no_host_reads_with_validate_off_and_a_padded_surface():
    from gelslim_depth_amd.touch_fusion import TouchVolume, extract_surface, integrate_touches, touch_transforms
    tri, grid, depth, widths, poses = rendered("sphere", (24, 31))
    vol = TouchVolume(lattice(tri, (21, 18, 14), 0.7), 0.7, (21, 18, 14), 1.75, device=DEV)
    weights = torch.ones(5, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rows = touch_transforms(poses, grid=grid)
        integrate_touches(vol, depth, widths, rows, image_height_mm=HEIGHT_MM, weights=weights, validate=False)
        got = extract_surface(vol, max_triangles=4000, cells=True)
        field = vol.tsdf()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert 0 < int(got.count) <= 4000 and field.shape == vol.acc.shape and rows.device == poses.device


def test_refusals():
    from gelslim_depth_amd.mesh_depth import MeshDepthError
    from gelslim_depth_amd.touch_fusion import TouchVolume, extract_surface, integrate_touches, touch_transforms
    tri, grid, depth, widths, poses = rendered("sphere", (24, 31))
    rows = touch_transforms(poses, grid=grid)
    vol = TouchVolume((-6, -6, -6), 0.6, (21, 18, 14), 1.5, device=DEV)
    before = bits(vol.acc)
    bad_width = widths.clone()
    bad_width[2] = -0.5
    for args, kw in (((vol, depth.cpu(), widths, rows), {}), ((vol, depth.double(), widths, rows), {}), ((vol, depth[:, :1], widths, rows), {}),
                     ((vol, depth, widths[:4], rows), {}), ((vol, depth, widths, rows[:3]), {}), ((vol, depth, widths, rows[:, :11]), {}),
                     ((vol, depth, bad_width, rows), {}), ((vol, depth, widths, rows), dict(weights=torch.ones(4, device=DEV))),
                     ((vol, depth, widths, rows), dict(contact_depth=-1.0)), ((vol, depth, widths, rows), dict(carve_weight=math.nan)),
                     ((vol, depth, widths, rows), dict(image_height_mm=0.0)), ((object(), depth, widths, rows), {}),
                     ((vol, depth[:, :, :1], widths, rows), {})):
        with pytest.raises(MeshDepthError):
            integrate_touches(*args, **kw)
    assert bits(vol.acc) == before
    for kw in (dict(min_weight=-1.0), dict(max_triangles=0), dict(max_triangles=2.5), dict(min_weight=math.inf)):
        with pytest.raises(MeshDepthError):
            extract_surface(vol, **kw)
    vol.acc = vol.acc[:, :, :-1]
    with pytest.raises(MeshDepthError):
        extract_surface(vol)
    with pytest.raises(MeshDepthError):
        TouchVolume((0, 0, 0), 0.5, (8, 8, 8), 1.0, device="cpu")


def test_end_to_end_a_sphere_from_rendered_touches(tmp_path):
    """render_depth -> integrate_touches -> extract_surface, the sphere of section 21 touched along all three axes (three planes,
    five in-hand poses each).  Every vertex lies within sqrt 3 h + sqrt 2 mpp (+ the render's slack) of the original mesh: the bound
    derived in DESIGN.md section 24.  The result builds a MeshVolume and a MeshGrid.  A fresh touch with a wider grasp indents a
    smaller cap (radius 1.52 mm against 2.65 mm and more): each of its points is farther than sqrt 2 mpp + sqrt 3 h from the border of
    what was fused, where the band of observed cells is complete, so every point finds the reconstruction within the same bound."""
    from gelslim_depth_amd.contact_points import depth_points
    from gelslim_depth_amd.mesh_depth import MeshGrid, read_stl, render_depth
    from gelslim_depth_amd.mesh_register import MeshVolume, closest_points, cloud_mesh_error
    from gelslim_depth_amd.touch_fusion import TouchVolume, extract_surface, integrate_touches, touch_transforms, write_stl
    size, h, tau = (40, 53), 0.25, 1.0
    mpp = HEIGHT_MM / size[0]
    bound = math.sqrt(3.0) * h + math.sqrt(2.0) * mpp + SLACK_MM
    tri = MESHES["sphere"]()
    v = tri.reshape(-1, 3).astype(np.float64)
    vol = TouchVolume.around(v.min(axis=0), v.max(axis=0), h, tau, device=DEV)
    planes = ("+y+z", "+x-y", "+z+x")
    for plane in planes:
        _, grid, depth, widths, poses = rendered("sphere", size, plane)
        integrate_touches(vol, depth, widths, touch_transforms(poses, grid=grid), image_height_mm=HEIGHT_MM)
    surface = extract_surface(vol)
    original = MeshVolume(tri, device=DEV)
    err = cloud_mesh_error(original, surface.vertices())
    print(f"{vol}: {int(surface.count)} triangles; vertices against the mesh: mean {float(err['mean']):.4f}, rms {float(err['rms']):.4f}, "
          f"max {float(err['max']):.4f} mm; bound {bound:.4f}")
    assert int(surface.count) > 5000 and int(err["within"]) == 3 * int(surface.count)
    assert float(err["max"]) <= bound
    rebuilt = MeshVolume(surface.triangles, device=DEV)
    assert rebuilt.triangles == int(surface.count)
    for plane in planes:
        assert MeshGrid(surface.triangles, 1.0, plane, device=DEV).triangles == int(surface.count)
    path = tmp_path / "fused.stl"
    assert write_stl(str(path), surface) == int(surface.count) and read_stl(str(path)).tobytes() == bits(surface.triangles)
    for plane in planes:
        grid = rendered("sphere", size, plane)[1]
        pose = torch.tensor([(0.5e-3, 0.3e-3, 1.7)], device=DEV)
        width = torch.tensor([7.4], device=DEV)
        fresh = render_depth(grid, pose, width, image_size=size, image_height_mm=HEIGHT_MM)
        cloud = depth_points(fresh, width, HEIGHT_MM, frame="object", poses=pose, grid=grid, normals=False, pixels=False)
        hits = closest_points(rebuilt, cloud.points, max_distance_mm=bound)
        found = int((hits.triangle >= 0).sum())
        print(f"  fresh touch on {plane}: {len(cloud.points)} points, {found} within the bound, the farthest at "
              f"{float(hits.distance[hits.triangle >= 0].max()):.4f} mm")
        assert len(cloud.points) > 60 and found == len(cloud.points)
