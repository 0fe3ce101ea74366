"""CPU: the definition of DESIGN.md section 21 (tests/depth_points_ref.py, the numpy fp64 twin of gsd_depth_points_*) against the
mesh it came from, and `write_ply`.  Depth images are the midpoints of mesh_depth_ref.raster_ref's intervals."""
import functools
import math

import numpy as np
import pytest

import depth_points_ref as D
import mesh_depth_ref as R

RADIUS, CENTRE = D.SPHERE["radius"], D.SPHERE["centre"]


@functools.lru_cache(maxsize=None)
def sphere_cloud(plane, size, invert, centre=CENTRE):
    tri, depth, pose = D.sphere_depth(plane, size, centre, invert)
    mid = D.mesh_mid(tri, plane)
    cloud = D.cloud(depth, [D.WIDTH], D.HEIGHT_MM, frame="object", poses=[pose], invert_affine=invert, gelslim_plane=plane, mid=mid)
    return tri, depth, pose, mid, cloud


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("size", D.SIZES)
@pytest.mark.parametrize("plane", D.PLANES)
def test_object_frame_points_of_a_rendered_sphere_lie_on_its_mesh(plane, size, invert):
    """R - sag - delta <= |p - centre| <= R + delta: a point made from the mesh's own depth image lies between the facets and the
    sphere they are inscribed in.  sag comes from the mesh, delta is raster_ref's position uncertainty."""
    tri, _, pose, _, (p, n, _, counts) = sphere_cloud(plane, size, invert)
    sag, _ = D.facet_geometry(tri, CENTRE, RADIUS)
    delta = 16 * 2.0 ** -23 * R.coord_max(tri, 1.0, plane, pose, size, D.HEIGHT_MM)
    dist = np.linalg.norm(p - np.asarray(CENTRE), axis=1)
    print(f"{plane} {size} invert={invert}: {len(p)} points, R - |p - c| in [{(RADIUS - dist).min():.5f}, {(RADIUS - dist).max():.5f}] mm, "
          f"sag {sag:.6f}, delta {delta:.2e}")
    assert counts[0, 0] > 50 and counts[0, 1] > 50
    assert dist.min() >= RADIUS - sag - delta and dist.max() <= RADIUS + delta
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, rtol=0, atol=1e-15)
    # away from the object: a sphere's outward direction
    assert (np.einsum("nk,nk->n", n, p - np.asarray(CENTRE)) > 0).all()


@pytest.mark.parametrize("size", D.SIZES)
def test_normals_of_a_rendered_sphere_stay_within_the_mesh_s_own_facet_angle(size):
    """Interior points (all four neighbours in contact: a central difference across at most two facets) lie within the largest
    angle between a facet's normal and the radial direction; a border point's one-sided difference is taken half a pixel away,
    which on a sphere adds mpp / (2 R) rad."""
    centre = (0.0, 0.0, 0.0)
    tri, depth, _, _, (p, n, pixel, _) = sphere_cloud("+y+z", size, False, centre)
    _, facet = D.facet_geometry(tri, centre, RADIUS)
    angle = np.radians(D.normal_angles(n, p, centre))
    inner = D.interior(depth[0], pixel, *size)
    mpp = D.HEIGHT_MM / size[0]
    print(f"{size}: interior {inner.sum()} points <= {math.degrees(angle[inner].max()):.2f} deg, all {len(p)} <= "
          f"{math.degrees(angle.max()):.2f} deg; facet angle {math.degrees(facet):.2f}, border bound {math.degrees(facet + mpp / (2 * RADIUS)):.2f}")
    assert inner.sum() > 100 and (~inner).sum() > 20
    assert angle[inner].max() <= facet
    assert angle.max() <= facet + mpp / (2 * RADIUS)


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("plane", D.PLANES)
def test_forward_map_returns_every_point_to_its_own_pixel_and_depth(plane, invert):
    size = D.SIZES[0]
    _, depth, pose, mid, (p, _, pixel, _) = sphere_cloud(plane, size, invert)
    h, w = size
    mpp = D.HEIGHT_MM / h
    worst = 0.0
    for point, px in zip(p, pixel):
        ch, r, k = (px // (h * w)) % 2, (px // w) % h, px % w
        x, y, d = D.forward(point, ch == 1, pose, D.WIDTH, plane, mid, invert)
        worst = max(worst, abs(x - mpp * (r - h / 2)), abs(y - mpp * (k - w / 2)), abs(d - float(depth[0, ch, r, k])))
    assert len(p) > 100 and worst <= 1e-9, worst


def test_frames_flip_stride_and_padding_of_the_twin_agree_with_each_other():
    """The grasp frame is the sensor frame mirrored and shifted per finger; LR_flip swaps which channel is which; a stride keeps
    the lattice's own pixels with unchanged normals; the padded form keeps a prefix."""
    _, depth, _, _, _ = sphere_cloud("+y+z", D.SIZES[0], False)
    h, w = D.SIZES[0]
    ps, ns, ix, counts = D.cloud(depth, frame="sensor")
    pg, ng, ixg, _ = D.cloud(depth, [D.WIDTH], grasp_width_offset=0.5, frame="grasp")
    assert np.array_equal(ix, ixg) and list(ix) == sorted(ix)
    s = np.where((ix // (h * w)) % 2 == 1, 1.0, -1.0)
    assert np.array_equal(pg, np.stack((s * ps[:, 0], ps[:, 1], s * (0.5 * 6.5 - ps[:, 2])), axis=1))
    assert np.array_equal(ng, np.stack((s * ns[:, 0], ns[:, 1], -s * ns[:, 2]), axis=1))
    assert (pg[:, 2] * s > 0).all()                                   # the right finger sits at q > 0
    pf, _, _, cf = D.cloud(depth[:, ::-1].copy(), [D.WIDTH], grasp_width_offset=0.5, frame="grasp", LR_flip=True)
    left = int(counts[0, 0])                                          # channels swapped and declared so: the same cloud, right first
    assert np.array_equal(cf, counts[:, ::-1]) and np.array_equal(pf, np.concatenate((pg[left:], pg[:left])))
    p2, n2, ix2, _ = D.cloud(depth, frame="sensor", stride=2)
    keep = np.isin(ix, ix2)
    assert 0 < len(ix2) < len(ix) and np.array_equal(ps[keep], p2) and np.array_equal(ns[keep], n2)
    assert all(((px // w) % h) % 2 == 1 and (px % w) % 2 == 1 for px in ix2)
    m = int(counts.sum()) - 7
    pp, _, pix = D.padded(ps, ns, ix, counts, m)
    assert np.array_equal(pp[0], ps[:m]) and np.array_equal(pix[0], ix[:m])
    pp, _, pix = D.padded(ps, ns, ix, counts, m + 10)
    assert np.isnan(pp[0, m + 7:]).all() and (pix[0, m + 7:] == -1).all() and np.array_equal(pp[0, :m + 7], ps)
    # a refused width: no points in the grasp frame, the sensor frame does not look at it
    assert D.cloud(depth, [-1.0], frame="grasp")[3].sum() == 0 and D.cloud(depth, [float("nan")], frame="grasp")[3].sum() == 0


def test_write_ply_writes_binary_little_endian_vertices_and_skips_nan_rows(tmp_path):
    from gelslim_depth_amd.contact_points import write_ply
    from gelslim_depth_amd.mesh_depth import MeshDepthError
    rng = np.random.default_rng(0)
    points = rng.standard_normal((2, 5, 3)).astype(np.float32)          # a padded cloud: (B, M, 3)
    normals = rng.standard_normal((2, 5, 3)).astype(np.float32)
    points[0, 3:] = np.nan
    normals[0, 3:] = np.nan
    points[1, 4] = np.nan
    normals[1, 4] = np.nan
    keep = ~np.isnan(points).any(axis=2).reshape(-1)

    def parse(path):
        raw = open(path, "rb").read()
        end = raw.index(b"end_header\n") + len(b"end_header\n")
        return raw[:end].decode("ascii").splitlines(), raw[end:]

    path = tmp_path / "cloud.ply"
    assert write_ply(str(path), points, normals) == 7
    head, body = parse(path)
    assert head == ["ply", "format binary_little_endian 1.0", "element vertex 7"] + \
        [f"property float {n}" for n in ("x", "y", "z", "nx", "ny", "nz")] + ["end_header"]
    assert len(body) == 7 * 6 * 4
    rows = np.frombuffer(body, dtype="<f4").reshape(7, 6)
    assert np.array_equal(rows[:, :3], points.reshape(-1, 3)[keep]) and np.array_equal(rows[:, 3:], normals.reshape(-1, 3)[keep])

    import torch
    assert write_ply(str(path), torch.from_numpy(points)) == 7          # a tensor, no normals
    head, body = parse(path)
    assert head[2] == "element vertex 7" and head[3:] == ["property float x", "property float y", "property float z", "end_header"]
    assert np.array_equal(np.frombuffer(body, dtype="<f4").reshape(7, 3), points.reshape(-1, 3)[keep])

    assert write_ply(str(path), np.full((4, 3), np.nan, np.float32)) == 0
    head, body = parse(path)
    assert head[2] == "element vertex 0" and body == b""
    with pytest.raises(MeshDepthError):
        write_ply(str(path), points, normals[:1])
    with pytest.raises(MeshDepthError):
        write_ply(str(path), points[..., :2])
