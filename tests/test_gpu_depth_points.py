"""GPU: gsd_depth_points_* (gelslim_depth_amd.contact_points) against the numpy fp64 twin of DESIGN.md section 21
(tests/depth_points_ref.py) on the same fp32 depth images, which `render_depth` makes from mesh_depth_ref's meshes.

counts, pixel and the order must be equal; every point and normal component must lie within one fp32 ulp of fp32(twin): the
kernel computes in fp64 in the twin's order of operations and rounds once, the ulp absorbs a cos / sin / sqrt / division that
differs in its last fp64 bit across a rounding boundary."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import depth_points_ref as D
import mesh_depth_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HEIGHT_MM = 12.0
SLACK_MM = 1e-4          # test_gpu_mesh_depth's: the fp32 interpolation of q in render_depth
POSES = ((1.1e-3, -0.7e-3, 0.4), (-0.6e-3, 0.9e-3, -1.3), (0.2e-3, -0.1e-3, 0.0), (0.4e-3, 0.5e-3, 2.2), (-1.0e-3, -0.3e-3, 0.9))


@functools.lru_cache(maxsize=None)
def mesh(name):
    return {"sphere": lambda: R.sphere(**D.SPHERE),
            "ellipsoid": lambda: R.ellipsoid(2, (3.0, 2.5, 3.5), 0.12, (1.5, 0.75, -0.5)),
            "lprism": lambda: R.l_prism(3.0, axis=0, centre=(0.25, 0.0, 0.5))}[name]()


@functools.lru_cache(maxsize=None)
def grid_of(name, plane):
    from gelslim_depth_amd.mesh_depth import MeshGrid
    return MeshGrid(mesh(name), 1.0, plane, DEV)


def contact_width(name, plane, indent=0.8):
    _, _, q, _ = R.prepare(mesh(name), 1.0, plane)
    return 2 * (float(q.max()) - indent)


@functools.lru_cache(maxsize=None)
def rendered(name, plane, size, flip=False, invert=False, offset=0.0, count=2):
    """(depth (count, 2, H, W) on the device, poses, widths): `count` poses of POSES at 0.8 and 0.5 mm of indentation."""
    from gelslim_depth_amd.mesh_depth import render_depth
    poses = [R.inverted_pose(POSES[i % 5]) if invert else POSES[i % 5] for i in range(count)]
    widths = [contact_width(name, plane, (0.8, 0.5)[i % 2]) - offset for i in range(count)]
    poses = torch.tensor(poses, dtype=torch.float32, device=DEV)
    widths = torch.tensor(widths, dtype=torch.float32, device=DEV)
    return render_depth(grid_of(name, plane), poses, widths, size, HEIGHT_MM, offset, flip, invert), poses, widths


def within_one_ulp(got, twin, what):
    """`got` (fp32, from the device) against fp32(`twin`): the same NaN pattern, every finite value within one ulp."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == twin.shape, (what, got.dtype, got.shape, twin.shape)
    want = twin.astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
    ulp = np.spacing(np.abs(want[ok])).astype(np.float64)
    worst = float((err / ulp).max()) if err.size else 0.0
    assert worst <= 1.0, (what, worst)
    return worst


def check_cloud(cloud, twin, what):
    p, n, ix, counts = twin
    assert np.array_equal(cloud.counts.cpu().numpy(), counts), what
    assert cloud.pixel.dtype == torch.int32 and np.array_equal(cloud.pixel.cpu().numpy(), ix), what
    return max(within_one_ulp(cloud.points.cpu().numpy(), p, what + " points"),
               within_one_ulp(cloud.normals.cpu().numpy(), n, what + " normals"))


CASES = [("sphere", (24, 31), "+y+z", False, False, 0.0), ("sphere", (40, 53), "+x-y", True, False, 0.25),
         ("ellipsoid", (24, 31), "+z+x", False, True, -0.5), ("ellipsoid", (40, 53), "+y+z", True, True, 0.25),
         ("lprism", (24, 31), "+x-y", False, True, 0.0), ("lprism", (40, 53), "+z+x", True, False, -0.5)]


@pytest.mark.parametrize("name,size,plane,flip,invert,offset", CASES)
def test_every_frame_and_stride_equals_the_twin_on_the_same_depth(name, size, plane, flip, invert, offset):
    from gelslim_depth_amd.contact_points import depth_points
    depth, poses, widths = rendered(name, plane, size, flip, invert, offset)
    grid = grid_of(name, plane)
    host = depth.cpu().numpy()
    total, worst = 0, 0.0
    for stride in (1, 2, 3):
        for frame in ("sensor", "grasp", "object"):
            kw = dict(image_height_mm=HEIGHT_MM, grasp_width_offset=offset, LR_flip=flip, stride=stride, frame=frame, invert_affine=invert)
            twin = D.cloud(host, widths.cpu().numpy(), poses=poses.cpu().numpy(), gelslim_plane=plane, mid=grid.mid, **kw)
            cloud = depth_points(depth, widths, poses=poses, grid=grid, **kw)
            assert cloud.frame == frame and not cloud.padded
            worst = max(worst, check_cloud(cloud, twin, f"{name} {size} {plane} stride {stride} {frame}"))
            total += len(twin[0])
            if stride == 1:
                assert twin[3].min() > 20, twin[3]              # both fingers of both images touch
    print(f"{name} {size} {plane} flip={flip} invert={invert} offset={offset}: {total} points compared, worst {worst:.3f} ulp")


def edge_batch(size):
    """B = 3: no contact (fingers wider than the object), every pixel in contact, and an image of special values."""
    from gelslim_depth_amd.mesh_depth import render_depth
    h, w = size
    grid = grid_of("sphere", "+y+z")
    pose = torch.tensor([POSES[0]], dtype=torch.float32, device=DEV)
    wide = torch.tensor([2 * D.SPHERE["radius"] + 3.0], dtype=torch.float32, device=DEV)
    depth = torch.zeros((3, 2, h, w), dtype=torch.float32, device=DEV)
    depth[0] = render_depth(grid, pose, wide, size, HEIGHT_MM)[0]
    depth[1] = -1.0
    special = np.zeros((2, h, w), np.float32)
    special[0, 0, 0], special[0, 0, 1], special[0, 1, 0] = -0.5, np.nan, np.nan              # a corner: NaN or outside all round
    special[1, h - 1, 1], special[1, h - 1, 0], special[1, h - 1, 2], special[1, h - 2, 1] = -0.25, np.nan, np.nan, np.nan
    special[0, 5, 5], special[0, 5, 6], special[0, 6, 5] = np.nan, np.inf, -0.75            # neither NaN nor +inf is a point
    special[1, 3, 4], special[1, 3, 5] = np.inf, -0.125                                      # ... nor a usable neighbour
    depth[2] = torch.from_numpy(special).to(DEV)
    return depth


def test_edge_batch_no_contact_full_contact_and_non_finite_pixels():
    from gelslim_depth_amd.contact_points import depth_points
    size = (24, 31)
    h, w = size
    depth = edge_batch(size)
    host = depth.cpu().numpy()
    widths = torch.tensor([9.0, 5.0, 5.5], dtype=torch.float32, device=DEV)
    poses = torch.tensor(POSES[:3], dtype=torch.float32, device=DEV)
    for stride in (1, 2):
        for frame in ("sensor", "grasp", "object"):
            kw = dict(image_height_mm=HEIGHT_MM, stride=stride, frame=frame, gelslim_plane="+z+x", mid=0.3)
            twin = D.cloud(host, widths.cpu().numpy(), poses=poses.cpu().numpy(), **kw)
            cloud = depth_points(depth, widths, poses=poses, **kw)
            check_cloud(cloud, twin, f"edge batch stride {stride} {frame}")
            lattice = len(D.lattice(h, stride)) * len(D.lattice(w, stride))
            counts = cloud.counts.cpu().numpy()
            assert counts[0].sum() == 0 and list(counts[1]) == [lattice, lattice]
            assert list(counts[2]) == ([2, 2] if stride == 1 else [0, 2])
    cloud = depth_points(depth, frame="sensor", image_height_mm=HEIGHT_MM)
    pts, nrm, pix = (t.cpu().numpy() for t in cloud.image(2))
    assert list(pix) == [4 * h * w, 4 * h * w + 6 * w + 5, 5 * h * w + 3 * w + 5, 5 * h * w + (h - 1) * w + 1]
    # lonely pixels, beside a NaN or a +inf: no usable neighbour, zero gradient, the normal straight into the gel
    assert np.array_equal(nrm, np.array([[0, 0, -1]] * 4, np.float32))
    assert np.array_equal(pts[:, 2], np.array([-0.5, -0.75, -0.125, -0.25], np.float32))
    full = cloud.finger(1, 0)[1].cpu().numpy()
    assert np.array_equal(full, np.broadcast_to(np.array([0, 0, -1], np.float32), full.shape))          # a flat image


@pytest.mark.parametrize("frame", ["grasp", "object"])
def test_padded_layout_keeps_a_prefix_drops_the_tail_and_fills_with_nan(frame):
    from gelslim_depth_amd.contact_points import depth_points
    size, plane = (24, 31), "+y+z"
    depth, poses, widths = rendered("sphere", plane, size, count=3)
    grid = grid_of("sphere", plane)
    kw = dict(image_height_mm=HEIGHT_MM, frame=frame)
    twin = D.cloud(depth.cpu().numpy(), widths.cpu().numpy(), poses=poses.cpu().numpy(), gelslim_plane=plane, mid=grid.mid, **kw)
    n = twin[3].sum(axis=1)
    assert len(set(n)) > 1 and n.min() > 40, n                    # the images differ in size: one M is below, at and above a count
    for m in (int(n.min()) - 5, int(n.min()), int(n[0]), int(n.max()) + 9, 3000):
        pp, nn, ix = D.padded(*twin, m)
        cloud = depth_points(depth, widths, poses=poses, grid=grid, max_points=m, validate=False, **kw)
        assert cloud.padded and tuple(cloud.points.shape) == (3, m, 3) and tuple(cloud.pixel.shape) == (3, m)
        assert np.array_equal(cloud.counts.cpu().numpy(), twin[3])                  # the true counts: an overflow stays visible
        assert np.array_equal(cloud.pixel.cpu().numpy(), ix)
        within_one_ulp(cloud.points.cpu().numpy(), pp, f"padded {m} points")
        within_one_ulp(cloud.normals.cpu().numpy(), nn, f"padded {m} normals")
        assert np.array_equal(np.isnan(cloud.points.cpu().numpy()).all(axis=2), ix < 0)
    bare = depth_points(depth, widths, poses=poses, grid=grid, max_points=int(n[0]), normals=False, pixels=False, **kw)
    assert bare.normals is None and bare.pixel is None
    within_one_ulp(bare.points.cpu().numpy(), D.padded(*twin, int(n[0]))[0], "points alone")


def bits(cloud):
    return [t.cpu().numpy().view(np.int32) for t in (cloud.points, cloud.normals)] + [cloud.pixel.cpu().numpy()]


def test_an_image_does_not_depend_on_its_batch_and_a_second_call_repeats_the_bits():
    from gelslim_depth_amd.contact_points import depth_points
    size, plane = (40, 53), "+x-y"
    h, w = size
    depth, poses, widths = rendered("ellipsoid", plane, size, count=5)
    grid = grid_of("ellipsoid", plane)
    kw = dict(image_height_mm=HEIGHT_MM, frame="object", grid=grid, stride=1)
    whole = depth_points(depth, widths, poses=poses, **kw)
    again = depth_points(depth, widths, poses=poses, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(bits(whole), bits(again)))
    alone = [depth_points(depth[b:b + 1], widths[b:b + 1], poses=poses[b:b + 1], **kw) for b in range(5)]
    for b in range(5):
        got = [t.cpu().numpy() for t in whole.image(b)]
        want = [t.cpu().numpy() for t in (alone[b].points, alone[b].normals, alone[b].pixel)]
        assert len(want[0]) > 100
        assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
        assert np.array_equal(got[2], want[2] + b * 2 * h * w)
        for ch in (0, 1):
            assert len(whole.finger(b, ch)[0]) == int(alone[b].counts[0, ch])

    # more blocks than one pass of the scan takes: the carry between passes.  The batch repeats the five images.
    from gelslim_depth_amd import _lib as L
    per = -(-(h * w) // L.GSD_DEPTH_POINTS_BLOCK)
    big = L.GSD_DEPTH_POINTS_SCAN_PASS // (2 * per) + 17
    assert 2 * big * per > L.GSD_DEPTH_POINTS_SCAN_PASS
    pick = torch.arange(big, device=DEV) % 5
    packed = depth_points(depth[pick], widths[pick], poses=poses[pick], **kw)
    parts = [alone[b % 5] for b in range(big)]
    assert np.array_equal(packed.counts.cpu().numpy(), np.concatenate([c.counts.cpu().numpy() for c in parts]))
    assert torch.equal(packed.points.view(torch.int32), torch.cat([c.points for c in parts]).view(torch.int32))
    assert torch.equal(packed.normals.view(torch.int32), torch.cat([c.normals for c in parts]).view(torch.int32))
    assert torch.equal(packed.pixel, torch.cat([c.pixel + b * 2 * h * w for b, c in enumerate(parts)]))


def test_a_cloud_of_a_rendered_sphere_lies_on_the_mesh_end_to_end():
    """render_depth -> depth_points(frame='object', grid=...) at the same poses and widths: the CPU file's sphere bound, widened
    by the render's own SLACK_MM."""
    from gelslim_depth_amd.contact_points import depth_points
    tri, centre, radius = mesh("sphere"), np.asarray(D.SPHERE["centre"]), D.SPHERE["radius"]
    sag, _ = D.facet_geometry(tri, centre, radius)
    for plane in D.PLANES:
        for size in D.SIZES:
            for invert in (False, True):
                depth, poses, widths = rendered("sphere", plane, size, False, invert)
                cloud = depth_points(depth, widths, HEIGHT_MM, poses=poses, frame="object", invert_affine=invert, grid=grid_of("sphere", plane))
                p = cloud.points.cpu().numpy().astype(np.float64)
                dist = np.linalg.norm(p - centre, axis=1)
                delta = max(16 * 2.0 ** -23 * R.coord_max(tri, 1.0, plane, pose, size, HEIGHT_MM) for pose in poses.cpu().numpy())
                print(f"{plane} {size} invert={invert}: {len(p)} points, R - |p - c| in [{(radius - dist).min():.5f}, {(radius - dist).max():.5f}]")
                assert len(p) > 150
                assert dist.min() >= radius - sag - delta - SLACK_MM and dist.max() <= radius + delta + SLACK_MM
                n = cloud.normals.cpu().numpy().astype(np.float64)
                assert (np.einsum("nk,nk->n", n, p - centre) > 0).all() and np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6


def test_abi_refusals():
    from gelslim_depth_amd import _lib as L
    lib = L.lib
    b, h, w = 2, 24, 31
    for args in ((0, h, w, 1), (b, 0, w, 1), (b, h, 0, 1), (b, h, w, 0), (1 << 15, 1 << 8, 1 << 7, 1), (1 << 30, 1, 1, 1)):
        assert lib.gsd_depth_points_workspace(*args) == 0, args
    assert lib.gsd_depth_points_workspace((1 << 15) - 1, 1 << 8, 1 << 7, 1) > 0                  # 2 B H W just below 2^31
    words = int(lib.gsd_depth_points_workspace(b, h, w, 1))
    assert words > 0
    depth = torch.full((b, 2, h, w), -1.0, device=DEV)
    widths = torch.full((b,), 5.0, device=DEV)
    poses = torch.zeros((b, 3), device=DEV)
    ws = torch.zeros((words,), dtype=torch.int32, device=DEV)
    counts = torch.full((b, 2), -7, dtype=torch.int32, device=DEV)
    rows = 2 * b * h * w
    points = torch.zeros((rows, 3), device=DEV)

    def view(frame=2, **kw):
        v = L.gsd_depth_points_view()
        v.mpp, v.width_offset, v.contact_depth, v.mid = HEIGHT_MM / h, 0.0, 0.0, 0.0
        v.perp_ind, v.swap_axes, v.multiplier, v.invert_affine, v.lr_flip, v.frame = 0, 0, 1, 0, 0, frame
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    def count(v, widths_ptr=widths.data_ptr(), elems=words, dims=(b, h, w, 1)):
        return lib.gsd_depth_points_count(C.byref(v), depth.data_ptr(), widths_ptr, *dims, counts.data_ptr(), ws.data_ptr(), elems,
                                          L.stream_ptr())

    def write(v, poses_ptr=poses.data_ptr(), elems=words, capacity=0, n=rows, points_ptr=points.data_ptr()):
        return lib.gsd_depth_points_write(C.byref(v), depth.data_ptr(), widths.data_ptr(), poses_ptr, b, h, w, 1, capacity, n, points_ptr,
                                          None, None, ws.data_ptr(), elems, L.stream_ptr())

    assert count(view(), elems=words - 1) == L.GSD_ERR_WORKSPACE and write(view(), elems=words - 1) == L.GSD_ERR_WORKSPACE
    assert b"workspace" in lib.gsd_last_error()
    reserved = view()
    reserved.reserved[1] = 1
    assert count(reserved) == L.GSD_ERR_BAD_ARG and write(reserved) == L.GSD_ERR_BAD_ARG
    assert b"reserved" in lib.gsd_last_error()
    assert write(view(2), poses_ptr=None) == L.GSD_ERR_BAD_ARG and b"poses" in lib.gsd_last_error()
    assert count(view(1), widths_ptr=None) == L.GSD_ERR_BAD_ARG
    for bad in (view(3), view(mpp=0.0), view(mpp=float("nan")), view(contact_depth=-1.0), view(mid=float("inf")), view(multiplier=0),
                view(perp_ind=3), view(lr_flip=2), view(width_offset=float("nan"))):
        assert count(bad) == L.GSD_ERR_BAD_ARG
    assert count(view(), dims=(b, h, w, 0)) == L.GSD_ERR_BAD_ARG
    assert write(view(), points_ptr=None) == L.GSD_ERR_BAD_ARG
    assert write(view(), capacity=-1) == L.GSD_ERR_BAD_ARG and write(view(), n=-1) == L.GSD_ERR_BAD_ARG
    assert write(view(), capacity=h * w, n=b * h * w - 1) == L.GSD_ERR_BAD_ARG          # padded outputs shorter than B x capacity
    torch.cuda.synchronize()
    assert (counts == -7).all() and not points.any()          # every refusal came before any launch
    assert count(view()) == L.GSD_OK and write(view()) == L.GSD_OK and write(view(0), poses_ptr=None) == L.GSD_OK
    torch.cuda.synchronize()
    assert (counts == h * w).all() and int(ws[:2].view(torch.int64).item()) == rows


def test_python_refusals_validate_and_the_cloud_object():
    from gelslim_depth_amd.contact_points import ContactCloud, depth_points
    from gelslim_depth_amd.mesh_depth import MeshDepthError
    depth, poses, widths = rendered("sphere", "+y+z", (24, 31))
    ok = dict(grasp_widths=widths, poses=poses, frame="object")
    for bad in (dict(depth=depth.double()), dict(depth=depth.cpu()), dict(depth=depth[:, :1]), dict(depth=depth[0]), dict(poses=None),
                dict(grasp_widths=None), dict(grasp_widths=widths[:1]), dict(poses=poses[:, :2]), dict(grasp_widths=widths.cpu()),
                dict(stride=0), dict(stride=1.5), dict(stride=True), dict(frame="world"), dict(contact_depth=-0.1),
                dict(contact_depth=float("nan")), dict(image_height_mm=0.0), dict(gelslim_plane="+q+z"), dict(max_points=0),
                dict(mid=float("nan")), dict(grasp_width_offset=float("inf")), dict(grid="a grid")):
        kw = dict(ok, depth=depth)
        kw.update(bad)
        with pytest.raises(MeshDepthError, match="depth_points: "):
            depth_points(**kw)
    negative = widths.clone()
    negative[1] = -1.0
    with pytest.raises(MeshDepthError, match="grasp width"):
        depth_points(depth, negative, frame="grasp")
    silent = depth_points(depth, negative, frame="grasp", validate=False)
    counts = silent.counts.cpu().numpy()
    assert counts[0].min() > 0 and counts[1].sum() == 0 and len(silent.image(1)[0]) == 0
    sensor = depth_points(depth, negative, frame="sensor")                         # reads no widths
    assert sensor.counts.cpu().numpy()[1].min() > 0
    assert isinstance(sensor, ContactCloud) and "packed" in repr(sensor) and "sensor" in repr(sensor)
    deep = depth_points(depth, frame="sensor", contact_depth=0.4)
    assert 0 < int(deep.counts.sum()) < int(sensor.counts.sum()) and float(deep.points[:, 2].max()) < -0.4
    assert "padded to 64" in repr(depth_points(depth, frame="sensor", max_points=64))
    with pytest.raises(MeshDepthError):
        depth_points(depth, frame="sensor", max_points=64).finger(0, 0)
    empty = depth_points(torch.zeros_like(depth), frame="sensor")
    assert tuple(empty.points.shape) == (0, 3) and tuple(empty.pixel.shape) == (0,) and int(empty.counts.sum()) == 0
