"""CPU: the definitions of DESIGN.md section 24 on their numpy twin (tests/touch_fusion_ref.py), and what gelslim_depth_amd.touch_fusion
does without a device: its conventions against the existing forward map, the topology of the marching-tetrahedra table on analytic
fields, split invariance, refusals, and a reconstruction from reference rasters held to a derived bound."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import depth_points_ref as D
import mesh_closest_ref as M
import mesh_depth_ref as R
import touch_fusion_ref as T

HEIGHT_MM = 12.0
SLACK_MM = 1e-4          # test_gpu_mesh_depth's: the fp32 depth of a render


def test_touch_transforms_invert_the_object_frame_of_depth_points():
    """For random object points the twin's projection through `touch_transforms` lands where section 16's forward map
    (depth_points_ref.forward) puts the point: row and column position and the depth of a surface through it, to 1e-9."""
    from gelslim_depth_amd.touch_fusion import touch_transforms
    rng = np.random.default_rng(24)
    size, g, mid = (24, 31), 6.5, 0.37
    mpp = HEIGHT_MM / size[0]
    worst = 0.0
    for plane in ("+y+z", "+x-y", "+z+x"):
        for invert in (False, True):
            poses = np.stack((rng.uniform(-3e-3, 3e-3, 6), rng.uniform(-3e-3, 3e-3, 6), rng.uniform(-3.1, 3.1, 6)), axis=1)
            rows = touch_transforms(torch.from_numpy(poses), plane, mid, invert_affine=invert).numpy()
            assert rows.shape == (6, 12) and rows.dtype == np.float64
            for pose, row in zip(poses, rows):
                for p in rng.uniform(-6.0, 6.0, (5, 3)):
                    for right in (False, True):
                        s = 1.0 if right else -1.0
                        rf, kf, base = T.project(tuple(p), row, s, g, size, HEIGHT_MM)
                        x, y, d = D.forward(p, right, pose, g, plane, mid, invert)
                        worst = max(worst, abs(rf - (x / mpp + size[0] / 2)), abs(kf - (y / mpp + size[1] / 2)), abs(-base - d))
    print(f"touch_transforms against forward: worst difference {worst:.3e}")
    assert worst <= 1e-9
    # fp32 poses are taken as the values they hold; a single pose is one row
    one = touch_transforms(torch.tensor([1.1e-3, -0.7e-3, 0.4]), "+y+z")
    assert one.shape == (1, 12) and one.dtype == torch.float64
    from gelslim_depth_amd.mesh_depth import MeshDepthError
    for bad in (dict(poses=torch.zeros(3, 2)), dict(poses=torch.zeros(1, 3), gelslim_plane="+q+z"), dict(poses=torch.zeros(1, 3), mid=math.nan),
                dict(poses=torch.zeros(1, 3, dtype=torch.int64))):
        with pytest.raises(MeshDepthError):
            touch_transforms(**bad)


def test_the_table_follows_the_rule():
    table = T.tet_table()
    tets = T.tetrahedra()
    assert tets == [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]
    for t_no, rows in enumerate(table):
        for mask, tris in enumerate(rows):
            assert len(tris) == (0, 1, 2, 1, 0)[bin(mask).count("1")]
            inside = {tets[t_no][i] for i in range(4) if mask >> i & 1}
            for tri in tris:
                for lo, hi in tri:
                    assert lo < hi and (lo in inside) != (hi in inside)      # every vertex sits on an edge that the surface crosses
    # complementary masks give the same triangles with the other winding
    for rows in table:
        for mask in range(1, 15):
            a, b = rows[mask], rows[15 - mask]
            assert sorted(sorted(t) for t in a) == sorted(sorted(t) for t in b)


@pytest.mark.parametrize("name,euler,analytic_volume", [("sphere", 2, 4.0 / 3.0 * math.pi * T.SPHERE_RADIUS ** 3),
                                                        ("torus", 0, 2.0 * math.pi ** 2 * T.TORUS_MAJOR * T.TORUS_MINOR ** 2)])
def test_extraction_of_an_analytic_field_is_a_closed_oriented_surface(name, euler, analytic_volume):
    """The field is written straight into acc with weight 1.  Vertices are identified by their fp32 bits, so `open` == 0 also says
    that every copy of a shared vertex has equal bits: a copy that differed in one bit would leave its edges without a reverse."""
    acc, weight = T.analytic(name)
    assert (acc != 0).all(), "the case must not put the surface through a voxel"
    tri, cell = T.extract(acc, weight, T.ANALYTIC_ORIGIN, T.ANALYTIC_H)
    topo = T.topology(tri)
    volume = T.signed_volume(tri)
    print(f"{name}: {len(tri)} triangles, {topo}, volume {volume:.4f} of {analytic_volume:.4f}")
    assert len(tri) > 5000 and topo["degenerate"] == 0
    assert topo["doubled"] == 0, "a directed edge appears twice: inconsistent winding"
    assert topo["open"] == 0, "a directed edge has no reverse: the surface is not closed"
    assert topo["euler"] == euler
    assert 0.0 < volume < analytic_volume and volume > 0.97 * analytic_volume
    assert (np.diff(cell) >= 0).all() and cell.min() >= 0 and cell.max() < (T.ANALYTIC_N - 1) ** 3
    # the vertices lie on lattice edges of their cell
    n = T.ANALYTIC_N - 1
    low = np.stack((cell % n, (cell // n) % n, cell // (n * n)), axis=1) * T.ANALYTIC_H + np.asarray(T.ANALYTIC_ORIGIN)
    rel = tri.astype(np.float64) - low[:, None, :]
    assert rel.min() > -1e-5 and rel.max() < T.ANALYTIC_H + 1e-5
    # min_weight: nothing is observed at or below it
    none, _ = T.extract(acc, weight, T.ANALYTIC_ORIGIN, T.ANALYTIC_H, min_weight=1.0)
    assert len(none) == 0


# ---- fused volumes -------------------------------------------------------------------------------------------------------
SPHERE_CENTRE = (0.7, -0.4, 0.3)
VIEWS = [((0.0, 0.0, 1.0), 0.0), ((0.0, 0.0, 1.0), 1.3), ((0.0, 1.0, 0.0), 0.9), ((0.0, 1.0, 0.0), math.pi / 2), ((0.0, 1.0, 0.0), 2.3),
         ((1.0, 1.0, 0.0), 0.8), ((1.0, -1.0, 0.3), 1.9), ((0.2, 1.0, -0.5), 2.8), ((0.0, 0.0, 1.0), math.pi / 2), ((1.0, 0.0, 1.0), 1.1),
         ((-1.0, 0.4, 0.2), 2.0), ((0.3, -0.2, 1.0), 2.6)]
POSES = [(1.1e-3, -0.7e-3, 0.4), (-0.6e-3, 0.9e-3, -1.3), (0.2e-3, -0.1e-3, 0.0), (0.4e-3, 0.5e-3, 2.2), (-1.0e-3, -0.3e-3, 0.9),
         (0.0, 0.0, 0.0)]
WIDTHS = [6.0, 6.5, 5.8, 7.0, 6.2]


def sphere_touches(size=(24, 31), plane="+y+z"):
    """(tri, depth (K, 2, H, W) float32, widths (K,) float32, rows (K, 12)): the sphere of section 21 turned by each of VIEWS
    before it is rastered (raster_ref midpoints), the turn composed into the touch's map."""
    from gelslim_depth_amd.touch_fusion import touch_transforms
    tri = R.sphere(3, 4.0, SPHERE_CENTRE)
    depth, widths, rows = [], [], []
    for j, (axis, angle) in enumerate(VIEWS):
        rot = T.rotation(axis, angle)
        turned = (tri.astype(np.float64) @ rot.T).astype(np.float32)
        pose = tuple(float(np.float32(v)) for v in POSES[j % len(POSES)])
        g = float(np.float32(WIDTHS[j % len(WIDTHS)]))
        lo, hi = R.raster_ref(turned, 1.0, plane, pose, g, size, HEIGHT_MM)
        depth.append((0.5 * (lo + hi)).astype(np.float32))
        widths.append(g)
        row = touch_transforms(torch.tensor([pose], dtype=torch.float64), plane, D.mesh_mid(turned, plane)).numpy()[0]
        rows.append(T.compose(row, rot))
    return tri, np.stack(depth), np.asarray(widths, np.float32), np.stack(rows)


@pytest.fixture(scope="module")
def touches():
    return sphere_touches()


def lattice_around(tri, h, margin):
    lo, hi = tri.reshape(-1, 3).min(axis=0) - margin, tri.reshape(-1, 3).max(axis=0) + margin
    shape = tuple(int(math.ceil((b - a) / h)) + 1 for a, b in zip(lo, hi))
    return tuple(float(v) for v in lo), shape


def test_split_invariance_and_touches_that_contribute_nothing(touches):
    tri, depth, widths, rows = touches
    h, tau = 0.5, 1.0
    origin, shape = lattice_around(tri, h, 1.5)
    zero = np.zeros(shape[::-1], np.float32)
    kw = dict(image_height_mm=HEIGHT_MM, carve_weight=0.25, contact_depth=0.05, weights=np.asarray([1.0, 0.5, 2.0, 1.5, 0.75], np.float32))
    whole = T.integrate(zero, zero, origin, h, tau, depth[:5], widths[:5], rows[:5], **kw)
    first = T.integrate(zero, zero, origin, h, tau, depth[:2], widths[:2], rows[:2], **dict(kw, weights=kw["weights"][:2]))
    both = T.integrate(first[0], first[1], origin, h, tau, depth[2:5], widths[2:5], rows[2:5], **dict(kw, weights=kw["weights"][2:]))
    assert whole[0].tobytes() == both[0].tobytes() and whole[1].tobytes() == both[1].tobytes()
    assert (whole[1] > 0).sum() > 1000 and (whole[0] < 0).sum() > 50
    # a negative or non-finite width, a touch that looks past the volume, and an all-NaN image change nothing
    for k, (wd, shift) in enumerate(((-1.0, 0.0), (math.nan, 0.0), (math.inf, 0.0), (6.0, 500.0))):
        row = rows[0].copy()
        row[3] += shift
        same = T.integrate(whole[0], whole[1], origin, h, tau, depth[:1], np.asarray([wd], np.float32), row[None], image_height_mm=HEIGHT_MM)
        assert same[0].tobytes() == whole[0].tobytes() and same[1].tobytes() == whole[1].tobytes(), k
    nan = np.full_like(depth[:1], np.nan)
    same = T.integrate(whole[0], whole[1], origin, h, tau, nan, widths[:1], rows[:1], image_height_mm=HEIGHT_MM)
    assert same[0].tobytes() == whole[0].tobytes()
    # LR_flip with swapped channels is the same touch, up to the order of the two fingers' additions: equal where one finger reaches
    plain = T.integrate(zero, zero, origin, h, tau, depth[:1], widths[:1], rows[:1], image_height_mm=HEIGHT_MM)
    flipped = T.integrate(zero, zero, origin, h, tau, depth[:1, ::-1].copy(), widths[:1], rows[:1], image_height_mm=HEIGHT_MM, LR_flip=True)
    assert np.array_equal(plain[1], flipped[1]) and np.allclose(plain[0], flipped[0], atol=1e-6)


def test_refusals_without_a_device():
    """What the Python layer and the library refuse before anything reaches a device: the ABI's checks come before any launch."""
    from gelslim_depth_amd import _lib as L
    from gelslim_depth_amd.mesh_depth import MeshDepthError
    from gelslim_depth_amd.touch_fusion import TouchVolume, write_stl
    for args in (((0, 0, 0), 0.5, (8, 8, 8), 0.9), ((0, 0, 0), 0.5, (1, 8, 8), 1.0), ((0, 0, 0), 0.5, (8, 8, 1025), 1.0), ((0, 0, 0), 0.0, (8, 8, 8), 1.0),
                 ((0, 0, math.nan), 0.5, (8, 8, 8), 1.0), ((0, 0, 0), 0.5, (8, 8), 1.0), ((0, 0, 0), 0.5, (8, 8, 8.5), 1.0),
                 ((0, 0, 0), 0.5, (8, 8, 8), math.inf)):
        with pytest.raises(MeshDepthError):
            TouchVolume(*args)
    with pytest.raises(MeshDepthError):
        TouchVolume.around((0, 0, 0), (1000, 1, 1), 0.5, 1.0)
    with pytest.raises(MeshDepthError):
        write_stl("unused.stl", np.zeros((4, 3)))
    lib = L.lib

    def volume(nx=8, ny=8, nz=8, h=0.5, tau=1.0, x0=0.0, reserved=0):
        v = L.gsd_touch_volume()
        v.x0, v.y0, v.z0, v.voxel, v.truncation, v.nx, v.ny, v.nz, v.reserved = x0, 0.0, 0.0, h, tau, nx, ny, nz, reserved
        return v

    def view(height=12.0, offset=0.0, contact=0.0, carve=1.0, reserved=0):
        v = L.gsd_touch_view()
        v.image_height_mm, v.width_offset, v.contact_depth, v.carve_weight, v.lr_flip, v.cull = height, offset, contact, carve, 0, 1
        v.reserved[1] = reserved
        return v
    p = 4096          # a non-null, aligned address that no refused call reads
    bad, ws_short = L.GSD_ERR_BAD_ARG, L.GSD_ERR_WORKSPACE

    def integrate(vol=None, vw=None, k=1, h=24, w=31, depth=p, widths=p, rows=p, acc=p, weight=p):
        return lib.gsd_touch_integrate(C.byref(vol or volume()), C.byref(vw or view()), depth, widths, rows, None, k, h, w, acc, weight, None)
    cases = [integrate(k=0), integrate(h=1), integrate(w=1), integrate(k=1 << 20, h=32, w=32), integrate(depth=None), integrate(widths=None),
             integrate(rows=None), integrate(acc=None), integrate(weight=None), integrate(rows=p + 4), integrate(vol=volume(nx=1)),
             integrate(vol=volume(nz=1025)), integrate(vol=volume(h=0.0)), integrate(vol=volume(h=math.inf)), integrate(vol=volume(tau=-1.0)),
             integrate(vol=volume(tau=math.nan)), integrate(vol=volume(x0=math.inf)), integrate(vol=volume(reserved=1)),
             integrate(vw=view(height=0.0)), integrate(vw=view(offset=math.nan)), integrate(vw=view(contact=-0.1)), integrate(vw=view(carve=-1.0)),
             integrate(vw=view(carve=math.inf)), integrate(vw=view(reserved=1)),
             lib.gsd_touch_integrate(None, C.byref(view()), p, p, p, None, 1, 24, 31, p, p, None),
             lib.gsd_touch_integrate(C.byref(volume()), None, p, p, p, None, 1, 24, 31, p, p, None)]
    assert cases == [bad] * len(cases), cases
    words = lib.gsd_touch_extract_workspace(C.byref(volume()))
    assert words == 4 + 2 * -(-7 * 7 * 7 // L.GSD_TOUCH_EXTRACT_BLOCK)
    assert lib.gsd_touch_extract_workspace(C.byref(volume(ny=1))) == 0 and lib.gsd_touch_extract_workspace(None) == 0
    count = lambda vol=None, mw=0.0, acc=p, weight=p, total=p, ws=p, n=words: lib.gsd_touch_extract_count(      # noqa: E731
        C.byref(vol or volume()), acc, weight, mw, total, ws, n, None)
    write = lambda cap=0, rows=8, tri=p, ws=p, n=words, mw=0.0: lib.gsd_touch_extract_write(      # noqa: E731
        C.byref(volume()), p, p, mw, cap, rows, tri, None, ws, n, None)
    cases = [count(vol=volume(nx=1)), count(mw=-1.0), count(mw=math.nan), count(acc=None), count(weight=None), count(total=None), count(ws=None),
             count(ws=p + 4), count(total=p + 4), write(cap=-1), write(rows=-1), write(cap=9, rows=8), write(rows=1 << 31), write(tri=None),
             write(ws=None), write(mw=math.inf)]
    assert cases == [bad] * len(cases), cases
    assert count(n=words - 1) == ws_short and write(n=words - 1) == ws_short


def test_write_stl_round_trips_and_skips_nan_rows(tmp_path):
    from gelslim_depth_amd.mesh_depth import read_stl
    from gelslim_depth_amd.touch_fusion import write_stl
    acc, weight = T.analytic("sphere", (12, 12, 12))
    tri, cell = T.extract(acc, weight, T.ANALYTIC_ORIGIN, T.ANALYTIC_H)
    assert len(tri) > 0
    rows, _ = T.padded(tri, cell, len(tri) + 7)
    path = tmp_path / "surface.stl"
    assert write_stl(str(path), torch.from_numpy(rows)) == len(tri)
    back = read_stl(str(path))
    assert back.tobytes() == tri.tobytes()


def test_a_sphere_fused_from_reference_rasters_lies_on_the_mesh(touches):
    """End to end on the twin.  The bound is derived: a vertex lies on a lattice edge of length at most
    sqrt 3 h between a voxel with a negative and one with a non-negative sample; a touch's observed surface is a bilinear patch
    between pixel centres that lie on the mesh, within sqrt 2 mpp of it; distance is 1-Lipschitz.  So every vertex is within
    sqrt 3 h + sqrt 2 mpp of the mesh (plus the slack of an fp32 depth), and no voxel farther than sqrt 2 mpp outside the mesh is
    negative.  Holds for a convex mesh thicker than the truncation along every view axis: the sphere of radius 4 with tau = 1."""
    tri, depth, widths, rows = touches
    h, tau, mpp = 0.25, 1.0, HEIGHT_MM / depth.shape[2]
    origin, shape = lattice_around(tri, h, tau + h)
    zero = np.zeros(shape[::-1], np.float32)
    bound = math.sqrt(3.0) * h + math.sqrt(2.0) * mpp + SLACK_MM
    centre = np.asarray(SPHERE_CENTRE)
    for carve in (1.0, 0.25):
        acc, weight = T.integrate(zero, zero, origin, h, tau, depth, widths, rows, image_height_mm=HEIGHT_MM, carve_weight=carve)
        surface, _ = T.extract(acc, weight, origin, h)
        assert len(surface) > 3000
        verts = np.unique(surface.reshape(-1, 3), axis=0).astype(np.float64)
        _, _, d2, _ = M.closest_brute(tri, verts)
        dist = np.sqrt(d2)
        inside = np.linalg.norm(verts - centre, axis=1) < 4.0
        print(f"carve {carve}: {len(surface)} triangles, {len(verts)} vertices: worst {dist.max():.4f} mm "
              f"({'inside' if inside[dist.argmax()] else 'outside'}), rms {math.sqrt((dist ** 2).mean()):.4f} mm; bound {bound:.4f}")
        assert dist.max() <= bound
        # false surfaces: the negative voxels that lie outside the mesh
        px, py, pz = np.meshgrid(*T.voxel_axes(origin, h, shape), indexing="ij")
        p = np.stack((px, py, pz), axis=3).transpose(2, 1, 0, 3)          # (nz, ny, nx, 3)
        negative = (weight > 0) & (T.field(acc, weight) < 0)
        out = p[negative]
        out = out[np.linalg.norm(out - centre, axis=1) > 4.0]          # the mesh is inscribed: these are outside it
        worst_out = 0.0
        if len(out):
            worst_out = float(np.sqrt(M.closest_brute(tri, out)[2]).max())
        print(f"  {int(negative.sum())} negative voxels, {len(out)} outside the sphere, the farthest {worst_out:.4f} mm from the mesh")
        assert worst_out <= math.sqrt(2.0) * mpp + SLACK_MM


def test_touch_fusion_kernels_use_no_scratch():
    """The four kernels of gsd_touch_fusion.hip are written to need no scratch: the table is read from constant data and a vertex
    reads its two voxels again instead of indexing eight kept values (device-only compile, a few seconds)."""
    import os
    import re
    import shutil
    import subprocess
    from gelslim_depth_amd import build as b
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this machine")
    r = subprocess.run([hipcc] + b.CFLAGS + [f"-I{b.INCLUDE}", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(b.CSRC, "gsd_touch_fusion.hip"), "-o", os.devnull], capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    kernels = {n: s for n, s in zip(names, scratch) if "touch_" in n}
    assert len(kernels) == 4, r.stderr[-2000:]
    assert all(v == 0 for v in kernels.values()), kernels
