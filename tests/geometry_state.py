"""Shared by the tests that ask whether a result of the geometry units (mesh_depth, contact_points, contact_patches, mesh_register,
touch_fusion, and the data path's metrics, blur, statistics, resize and batch gather) depends on anything but its inputs:
test_geometry_state_cpu.py, test_gpu_geometry_list_order.py, test_gpu_geometry_memory.py, test_gpu_geometry_streams.py.  Not
collected; nothing here is product code; torch is imported inside the functions.

WORKLOADS              name -> Workload.  Calling one builds its inputs from fixed seeds, runs one unit's public API and returns a
                       flat dict of named device tensors: every returned tensor and every tensor attribute of the returned objects.
                       Cell lists enter as the cell table plus each cell's segment SORTED, because the raw order inside a segment
                       depends on an atomic cursor and is not a function of the input.  `stage()` / `run(staged, hook)` split a
                       call into making the inputs and using them, for test_gpu_geometry_streams.py.
permute_segments()     the numpy core of permute_lists: every cell's segment of a list reordered, `start` untouched.
permute_lists()        the same on a MeshGrid's or MeshVolume's `list`, in place; returns the old list.
roof()                 eight triangles under "+y+z" whose ridge lies exactly under image row 12 of a 24 x 31 image of
                       ROOF_HEIGHT_MM: every pixel of that row is covered by a left-slope and a right-slope triangle with
                       bit-equal values and opposite Jacobians, and every number involved is dyadic.
tie_box_points()       the cell-corner lattice of the 6 x 4 x 5 box at cell_mm = 1 and the points beside it
                       (test_points_on_the_cell_planes_of_a_box's).
first_in_list_terms()  mesh_pose_refine_ref.finger_terms with a deliberately WRONG tie rule (the first maximum in a given list order
first_in_list_closest()  instead of the lowest id), and the same for mesh_closest_ref.closest_brute: they prove that the stimulus of
                       test_gpu_geometry_list_order.py can see.
"""
import numpy as np

import mesh_closest_ref as MC
import mesh_depth_ref as R
import mesh_pose_ref as P
import mesh_pose_refine_ref as PR

HOWS = ("reversed", "sorted", "sorted_desc", ("shuffle", 1), ("shuffle", 2))
DEV = "cuda:0"
SIZE = (24, 31)


def how_id(how):
    return how if isinstance(how, str) else f"{how[0]}{how[1]}"


# ------------------------------------------------------------------------------------------------------------ list permutations
def permute_segments(start, entries, how):
    """A copy of `entries` in which every segment entries[start[c]:start[c + 1]] is reordered: "reversed", "sorted" (ascending
    ids), "sorted_desc", or ("shuffle", seed) -- numpy's PCG64 seeded with (seed, c), so a cell's order depends on nothing else."""
    start = np.asarray(start, np.int64)
    out = np.array(entries, copy=True)
    assert start.ndim == 1 and start[0] == 0 and (np.diff(start) >= 0).all() and start[-1] <= out.size
    for c in range(start.size - 1):
        seg = out[start[c]:start[c + 1]]
        if how == "reversed":
            seg = seg[::-1]
        elif how == "sorted":
            seg = np.sort(seg)
        elif how == "sorted_desc":
            seg = np.sort(seg)[::-1]
        elif isinstance(how, tuple) and len(how) == 2 and how[0] == "shuffle":
            seg = np.random.Generator(np.random.PCG64([int(how[1]), c])).permutation(seg)
        else:
            raise ValueError(f"permute_segments: how = {how!r}")
        out[start[c]:start[c + 1]] = seg
    return out


def cell_count(owner):
    """Cells of a MeshGrid (nx * ny) or a MeshVolume (nx * ny * nz)."""
    g = owner.grid if hasattr(owner, "grid") else owner.volume
    return int(g.nx) * int(g.ny) * int(getattr(g, "nz", 1))


def list_start(owner):
    """start[ncells + 1] of the owner's cell table as int64 numpy (gsd_cell_lists.h: total (int64) | start | cursor)."""
    n = cell_count(owner)
    return owner.cells[2:2 + n + 1].cpu().numpy().astype(np.int64)


def permute_lists(owner, how):
    """Rewrite owner.list in place (the tensor every later call reads) and return the old list as a device tensor;
    owner.list.copy_(old) puts it back."""
    import torch
    old = owner.list.clone()
    if owner.pairs > 0:
        new = permute_segments(list_start(owner), old.cpu().numpy(), how)
        owner.list.copy_(torch.from_numpy(new).to(owner.list.device))
    return old


def lists_from_ranges(lo, hi, dims, listed):
    """(start, entries) of the cell lists that the index ranges lo, hi (T, len(dims)) inclusive give (x runs fastest), ids of
    `listed` only.  Inside a cell the ascending ids are ROTATED by one ([1, 2, ..., 0]): an order an atomic cursor could leave, and
    one that every `how` of permute_segments changes where a cell holds three or more ids."""
    ncells = int(np.prod(dims))
    per = [[] for _ in range(ncells)]
    for t in listed:
        axes = np.meshgrid(*[np.arange(lo[t, k], hi[t, k] + 1) for k in range(len(dims))][::-1], indexing="ij")      # slowest first
        index = np.zeros_like(axes[0])
        for k, a in zip(range(len(dims) - 1, -1, -1), axes):
            index = index * dims[k] + a
        for c in index.ravel():
            per[int(c)].append(int(t))
    per = [ids[1:] + ids[:1] for ids in per]
    start = np.concatenate(([0], np.cumsum([len(ids) for ids in per]))).astype(np.int64)
    return start, np.array([t for ids in per for t in ids], np.int32)


# ------------------------------------------------------------------------------------------------------------------- the roof
ROOF_PLANE = P.PLANE            # "+y+z": perp x, a = y along the image rows, b = z along the columns, no axis swap
ROOF_HEIGHT_MM = 6.0            # 24 rows: 0.25 mm per pixel, so the 31 columns span b in [-3.875, 3.625], all over the roof
ROOF_POSE = (0.0, 0.0, 0.0)
ROOF_SHIFTED = (0.0, 0.00025, 0.0)      # a2 = one pixel pitch: fp32(1000) * fp32(0.00025) is exactly 0.25 (the CPU test asserts it)
ROOF_SEEN = (0.00025, 0.0, 0.0)         # a1 = one pixel pitch: the pose of the image that the roof's normal rows are scored against
ROOF_G = 0.5
ROOF_ROW = 12                   # u = 0.25 * (12 - 12) = 0: the ridge
ROOF_LEFT, ROOF_RIGHT = (0, 1, 6, 7), (2, 3, 4, 5)      # ids by slope: q rises with a (J[0] = +0.5), q falls with a (J[0] = -0.5)


def roof():
    """(8, 3, 3) fp32.  Eaves at a = -4 and a = +4 with x = 1, the ridge at a = 0 with x = 3 (q = x - 2: -1 .. 1), so the slopes
    are dq/da = +0.5 and -0.5.  Ids 0, 1 (left slope) and 2, 3 (right slope) cover b in [-4, 0]; ids 4, 5 (right slope) and 6, 7
    (left slope) cover b in [0, 4].  Of every slope's two triangles one holds the ridge edge: ids 0, 3, 5 and 6.  On the ridge the
    lowest id is 0 for b < 0 (a left slope) and 5 for b > 0 (a right slope).  Every doubled area is 16, so 1 / area is exact."""
    def slope(a_eave, b0, b1, edge_first):
        e0, e1, r0, r1 = (1.0, a_eave, b0), (1.0, a_eave, b1), (3.0, 0.0, b0), (3.0, 0.0, b1)
        with_edge, corner_only = [e0, r0, r1], [e0, r1, e1]
        return [with_edge, corner_only] if edge_first else [corner_only, with_edge]
    tri = slope(-4.0, -4.0, 0.0, True) + slope(4.0, -4.0, 0.0, False) + slope(4.0, 0.0, 4.0, False) + slope(-4.0, 0.0, 4.0, True)
    return np.ascontiguousarray(np.asarray(tri, np.float32))


def first_in_list_terms(G, order, pose, g, size, height_mm, right, invert=False):
    """finger_terms with the wrong tie rule: among equal values the winner is the first IN `order` (a sequence of all triangle ids:
    the list of a one-cell grid), not the lowest id.  Everything else -- R, J from the winner's slope -- is finger_terms'."""
    order = np.asarray(order, np.int64)
    assert sorted(order.tolist()) == list(range(G["rec"].shape[0]))
    t = PR.finger_terms(dict(G, rec=G["rec"][order]), pose, g, size, height_mm, right, invert)
    t["win"] = np.where(t["win"] >= 0, order[np.maximum(t["win"], 0)], -1)
    return t


# ------------------------------------------------------------------------------------------------------------------- the box
BOX_CELL_MM = 1.0
BOX_DIMS = (7, 5, 6)            # gsd_mesh_volume_plan: ceil((extent + 2 * pad) / cell) with pad = 1e-3 * cell
BOX_ORIGIN = tuple(-0.5 * e - 1e-3 * BOX_CELL_MM for e in (6.0, 4.0, 5.0))


def tie_box_points():
    """(4 * 8 * 6 * 7, 3) fp32: the corners of the cells of MeshVolume(box(), cell_mm=1), the nearest floats on either side of
    them, and the points half a cell along x."""
    x0, y0, z0 = BOX_ORIGIN
    nx, ny, nz = BOX_DIMS
    lattice = np.array([(x0 + i * BOX_CELL_MM, y0 + j * BOX_CELL_MM, z0 + k * BOX_CELL_MM) for i in range(nx + 1) for j in range(ny + 1)
                        for k in range(nz + 1)])
    return np.concatenate([np.float32(lattice), np.nextafter(np.float32(lattice), np.float32(np.inf)),
                           np.nextafter(np.float32(lattice), np.float32(-np.inf)), np.float32(lattice + (0.5, 0.0, 0.0))])


def first_in_list_closest(tri32, order, points):
    """closest_brute with the wrong tie rule: among bit-equal distances the first triangle IN `order` wins."""
    order = np.asarray(order, np.int64)
    assert sorted(order.tolist()) == list(range(len(tri32)))
    tid, x, d2, second = MC.closest_brute(np.asarray(tri32)[order], points)
    return np.where(tid >= 0, order[np.maximum(tid, 0)], -1), x, d2, second




# ------------------------------------------------------------------------------------------------------------------ workloads
class Hook:
    """What a workload calls in front of every unit call: inputs(what, *staged) returns the tensors that the call is to read.  The
    plain hook returns t.clone() + 0 of each -- the same bits in new storage (no staged input holds a -0.0); the hook of
    test_gpu_geometry_streams.py makes them late."""

    def inputs(self, what, *staged):
        return tuple(None if t is None else t.clone() + 0 for t in staged)


class Workload:
    def __init__(self, name, stage, run):
        self.name, self.stage, self._run = name, stage, run

    def run(self, staged, hook=None):
        return self._run(staged, hook or Hook())

    def __call__(self):
        return self.run(self.stage())


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sorted_lists(owner):
    """{cells, list_sorted}: the cell table as built and the list with every cell's segment in ascending id order, on the device."""
    import torch
    n = cell_count(owner)
    if owner.pairs == 0:
        return {"cells": owner.cells, "list_sorted": owner.list}
    start = owner.cells[2:2 + n + 1].to(torch.int64)
    cell_of = torch.repeat_interleave(torch.arange(n, device=owner.cells.device), start[1:] - start[:-1])
    key = cell_of * (1 << 24) + owner.list.to(torch.int64)          # at most 2^24 triangles per mesh
    return {"cells": owner.cells, "list_sorted": (torch.sort(key).values % (1 << 24)).to(torch.int32)}


def _attrs(prefix, obj, names):
    return {f"{prefix}.{n}": getattr(obj, n) for n in names if getattr(obj, n) is not None}


REFINEMENT = ("pose", "width", "cost", "normal_row", "trace", "accepted", "last_step")
ESTIMATE = ("pose", "cost", "row", "trace", "width", "lattice_pose", "lattice_cost")


# ---- mesh_depth
def _mesh_grid_stage():
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(1)
    staged = {}
    # `validate`: the L prism's calls read the smallest width back (the default), the ellipsoid's synchronise nothing
    for name, tri, validate in (("lprism", P.MESHES["lprism"](), True), ("ellipsoid3", R.ellipsoid(3), False)):
        gw = P.contact_width(tri)
        widths = np.asarray([gw, gw - 0.3], np.float32)
        seen = np.asarray([[0.6e-3, -0.45e-3, 0.45], [-0.4e-3, 0.35e-3, -1.1]], np.float32)
        cand = seen[:, None, :] + ((torch.rand((2, 5, 3), generator=g) * 2 - 1) * torch.tensor([1.5e-3, 1.5e-3, 0.6])).numpy()
        many = np.stack([widths, widths - 0.2, widths - 0.4], axis=1)
        staged[name] = dict(tri=tri, validate=validate, widths=_cuda(widths), seen=_cuda(seen), cand=_cuda(cand.astype(np.float32)),
                            many=_cuda(many.astype(np.float32)))
    return staged


def _mesh_grid_run(staged, hook):
    import torch
    from gelslim_depth_amd import mesh_depth as M
    res, height = {}, 12.0
    for name, s in staged.items():
        v = dict(validate=s["validate"])
        hook.inputs(f"MeshGrid {name}")
        grid = M.MeshGrid(s["tri"], 1.0, P.PLANE, DEV)
        res.update({f"{name}.records": grid.records, **{f"{name}.{k}": t for k, t in sorted_lists(grid).items()}})
        seen, widths = hook.inputs("render_depth", s["seen"], s["widths"])
        observed = M.render_depth(grid, seen, widths, SIZE, height, **v)
        out = torch.empty((2, 2) + SIZE, device=DEV, dtype=torch.float32)
        seen, widths = hook.inputs("render_depth out=", s["seen"], s["widths"])
        assert M.render_depth(grid, seen, widths, SIZE, height, out=out, **v) is out
        seen, widths = hook.inputs("render_depth_jacobian", s["seen"], s["widths"])
        jac = M.render_depth_jacobian(grid, seen, widths, SIZE, height, **v)
        obs, cand, widths = hook.inputs("score_poses", observed, s["cand"], s["widths"])
        score = M.score_poses(grid, obs, cand, widths, height, **v)
        obs, cand, many = hook.inputs("score_poses_widths", observed, s["cand"], s["many"])
        score_w = M.score_poses_widths(grid, obs, cand, many, height, **v)
        obs, cand, widths = hook.inputs("pose_normal_rows", observed, s["cand"], s["widths"])
        rows = M.pose_normal_rows(grid, obs, cand, widths, height, **v)
        res.update({f"{name}.render": observed, f"{name}.render_out": out, f"{name}.jacobian": jac, f"{name}.score": score,
                    f"{name}.score_widths": score_w, f"{name}.normal_rows": rows})
        for fit in (False, True):
            obs, widths, init = hook.inputs(f"refine_pose fit_width={fit}", observed, s["widths"], s["cand"][:, :2].contiguous())
            r = M.refine_pose(grid, obs, widths, init, iterations=3, fit_width=fit, image_height_mm=height, **v)
            res.update(_attrs(f"{name}.refine{int(fit)}", r, REFINEMENT))
        obs, widths, init = hook.inputs("estimate_pose", observed, s["widths"], s["cand"][:, 0].contiguous())
        e = M.estimate_pose(grid, obs, widths, init, (1.5e-3, 1.5e-3, 0.6), counts=(3, 3, 3), levels=2, image_height_mm=height, **v)
        res.update(_attrs(f"{name}.estimate", e, ESTIMATE))
    return res


# ---- contact_points, contact_patches
CONTACT_CONNECTIVITY = (4, 8)
CONTACT_FRAMES = ("sensor", "grasp", "object")
CONTACT_LAYOUTS = ("packed", "below", "above")
PATCH_PROPERTIES = ("area_mm2", "centroid_mm", "axis_angle", "axis_lengths_mm", "volume_mm3", "mean_depth", "peak_depth", "peak_rc", "bbox")


def contact_batch():
    """(depth (4, 2, 24, 31) fp32 numpy, widths (4,), poses (4, 3), tri): two images of the L prism (mesh_depth_ref.raster_ref at
    delta = 0: the definition, rendered on the host), one image of zeros, and one of five separate 2 x 3 blobs per plane -- more
    kept patches than max_patches = 2 -- with three NaN pixels and one -inf pixel per plane."""
    tri = P.MESHES["lprism"]()
    gw = float(np.float32(P.contact_width(tri)))
    poses = np.asarray([[0.6e-3, -0.45e-3, 0.45], [-0.4e-3, 0.35e-3, -1.1], [0.0, 0.0, 0.0], [0.2e-3, 0.1e-3, 0.3]], np.float32)
    widths = np.asarray([gw, float(np.float32(gw - 0.3)), gw, gw], np.float32)
    depth = np.zeros((4, 2) + SIZE, np.float32)
    for n in (0, 1):
        lo, _ = R.raster_ref(tri, 1.0, P.PLANE, tuple(float(p) for p in poses[n]), float(widths[n]), SIZE, 12.0, delta=0.0)
        depth[n] = lo.astype(np.float32) + np.float32(0.0)
    for ch in (0, 1):
        for k, (r, c) in enumerate(((2, 3), (2, 20), (10, 11 + ch), (17, 4), (18, 24))):
            depth[3, ch, r:r + 2, c:c + 3] = -0.125 * (k + 1 + ch)
        depth[3, ch, 6, 15:18] = np.nan
        depth[3, ch, 10, 12] = -np.inf          # inside the middle blob
    return depth, widths, poses, tri


def _contact_stage():
    depth, widths, poses, tri = contact_batch()
    with np.errstate(invalid="ignore"):
        counts = [int((depth[b] < 0).sum()) for b in range(depth.shape[0])]
    return dict(depth=_cuda(depth), widths=_cuda(widths), poses=_cuda(poses), tri=tri, counts=counts)


def _contact_run(staged, hook):
    from gelslim_depth_amd.contact_patches import contact_patches
    from gelslim_depth_amd.contact_points import depth_points
    from gelslim_depth_amd.mesh_depth import MeshGrid
    res = {}
    for conn in CONTACT_CONNECTIVITY:
        (depth,) = hook.inputs(f"contact_patches {conn}", staged["depth"])
        p = contact_patches(depth, connectivity=conn, min_area=3, max_patches=2)
        res.update(_attrs(f"patches{conn}", p, ("labels", "counts", "stats")))
        res.update({f"patches{conn}.{n}": getattr(p, n) for n in PATCH_PROPERTIES})
        (depth,) = hook.inputs("filtered_depth", staged["depth"])
        res[f"patches{conn}.filtered"] = p.filtered_depth(depth, keep_largest=1)
    hook.inputs("MeshGrid")
    grid = MeshGrid(staged["tri"], 1.0, P.PLANE, DEV)
    most = max(staged["counts"])
    assert most > 40
    for frame in CONTACT_FRAMES:
        for stride in (1, 2):
            for label, m in zip(CONTACT_LAYOUTS, (None, most // 8, most + 7)):      # (a stride of 2 keeps a quarter of the points)
                depth, widths, poses = hook.inputs(f"depth_points {frame} {stride} {label}", staged["depth"], staged["widths"], staged["poses"])
                c = depth_points(depth, widths, 12.0, stride=stride, frame=frame, poses=poses, grid=grid, normals=True, pixels=True, max_points=m)
                res.update(_attrs(f"points.{frame}.s{stride}.{label}", c, ("points", "normals", "pixel", "counts")))
    return res


# ---- mesh_register
def _mesh_volume_stage():
    rng = np.random.Generator(np.random.PCG64(5))
    pts = ((rng.random((1025, 3)) - 0.5) * 9.0).astype(np.float32)
    pts[7] = np.nan
    weights = (0.5 + rng.random(1025)).astype(np.float32)
    starts = np.stack((np.eye(4), MC.rigid((0.3, -0.2, 0.1), (0, 1, 1), 0.1), MC.rigid((-0.2, 0.1, 0.3), (1, 0.5, 0), -0.15)))
    surface = R.sample_surface(R.l_prism().astype(np.float64)[:20], 600, seed=3).astype(np.float32)      # a cloud that lies on the mesh
    return dict(tri=R.l_prism(), pts=_cuda(pts), weights=_cuda(weights), starts=_cuda(starts), surface=_cuda(surface))


def _mesh_volume_run(staged, hook):
    from gelslim_depth_amd import mesh_register as G
    res = {}
    hook.inputs("MeshVolume")
    vol = G.MeshVolume(staged["tri"], 1.0, DEV)
    res.update({"tri": vol.tri, **sorted_lists(vol)})
    for label, d in (("all", None), ("near", 1.5)):
        (pts,) = hook.inputs(f"closest_points {label}", staged["pts"])
        res.update(_attrs(f"closest.{label}", G.closest_points(vol, pts, d), ("triangle", "closest", "distance", "sq_distance")))
    for kind in ("plane", "point"):
        pts, starts, w = hook.inputs(f"icp_rows {kind}", staged["pts"], staged["starts"], staged["weights"])
        res[f"icp_rows.{kind}"] = G.icp_rows(vol, pts, starts, 2.0, kind, w)
    cloud, starts = hook.inputs("register_cloud", staged["surface"], staged["starts"])
    r = G.register_cloud(vol, cloud, init=starts, iterations=4)
    res.update(_attrs("register", r, ("matrix", "matrices", "cost", "rms", "active", "rows", "trace", "accepted", "last_step", "best")))
    (pts,) = hook.inputs("cloud_mesh_error", staged["pts"])
    res.update({f"error.{k}": t for k, t in G.cloud_mesh_error(vol, pts, 3.0).items()})
    return res


# ---- touch_fusion
TOUCH_DIMS, TOUCH_H = (40, 36, 33), 0.3
TOUCH_POSES = ((1.1e-3, -0.7e-3, 0.4), (-0.6e-3, 0.9e-3, -1.3), (0.2e-3, -0.1e-3, 0.0))
TOUCH_WIDTHS = (6.0, 6.5, 5.8)
TOUCH_LAYOUTS = ("packed", "below", "above")


def _touch_stage():
    tri = R.sphere(3, 4.0, (0.7, -0.4, 0.3))
    depth = np.zeros((3, 2) + SIZE, np.float32)
    for n, (pose, g) in enumerate(zip(TOUCH_POSES, TOUCH_WIDTHS)):
        lo, _ = R.raster_ref(tri, 1.0, P.PLANE, tuple(float(np.float32(p)) for p in pose), g, SIZE, 12.0, delta=0.0)
        depth[n] = lo.astype(np.float32) + np.float32(0.0)
    v = tri.reshape(-1, 3).astype(np.float64)
    mid = 0.5 * (v.min(axis=0) + v.max(axis=0))
    origin = tuple(float(m - 0.5 * TOUCH_H * (n - 1)) for m, n in zip(mid, TOUCH_DIMS))
    perp = v[:, R.plane_table(P.PLANE)[0]]
    return dict(depth=_cuda(depth), widths=_cuda(np.asarray(TOUCH_WIDTHS, np.float32)), poses=_cuda(np.asarray(TOUCH_POSES, np.float32)),
                origin=origin, mid=0.5 * (float(perp.max()) + float(perp.min())))


def _touch_run(staged, hook):
    from gelslim_depth_amd import touch_fusion as F
    res = {}
    vol = F.TouchVolume(staged["origin"], TOUCH_H, TOUCH_DIMS, 2.5 * TOUCH_H, device=DEV)
    (poses,) = hook.inputs("touch_transforms", staged["poses"])
    rows = F.touch_transforms(poses, P.PLANE, staged["mid"])
    res["transforms"] = rows
    for lo, hi in ((0, 2), (2, 3)):
        depth, widths, t = hook.inputs(f"integrate_touches {lo}:{hi}", staged["depth"][lo:hi], staged["widths"][lo:hi], rows[lo:hi])
        F.integrate_touches(vol, depth, widths, t)
    res.update({"acc": vol.acc, "weight": vol.weight})
    hook.inputs("extract_surface packed")
    s = F.extract_surface(vol, cells=True)
    count = int(s.triangles.shape[0])
    assert count > 500
    res.update(_attrs("surface.packed", s, ("triangles", "cell", "count")))
    for label, m in zip(TOUCH_LAYOUTS[1:], (count - 37, count + 41)):
        hook.inputs(f"extract_surface {label}")
        res.update(_attrs(f"surface.{label}", F.extract_surface(vol, max_triangles=m, cells=True), ("triangles", "cell", "count")))
    return res


# ---- metrics, blur, statistics, resize, the batch gather
def _metrics_stage():
    import torch
    from oracle import dataset_ref as dr
    g = torch.Generator(device="cpu")
    g.manual_seed(3)
    out = torch.rand((3, 1) + SIZE, generator=g) * -0.9
    tgt = torch.rand((3, 1) + SIZE, generator=g) * -0.9
    tgt[:, :, : SIZE[0] // 3] = 0.0
    x = torch.rand((2, 3) + SIZE, generator=g) * 255
    base = torch.rand((2, 3) + SIZE, generator=g) * 255
    blur = torch.rand((2, 1, 33, 31), generator=g) * -2
    stats = torch.randn((7, 3, 33, 31), generator=g) * 2 + 3
    return dict(out=out.to(DEV), tgt=tgt.to(DEV), x=x.to(DEV), base=base.to(DEV), blur=blur.to(DEV), stats=stats.to(DEV),
                objects=dr.synthetic_objects(41, [3, 2], h=42, w=54))


def _metrics_run(staged, hook):
    import torch
    from gelslim_depth_amd.dataset import Augment, DeviceDataset, DeviceLoader, channel_stats, gaussian_blur
    from gelslim_depth_amd.metrics import DepthMetrics, depth_metrics
    from gelslim_depth_amd.processing import resize_affine
    res = {}
    out, tgt = hook.inputs("depth_metrics", staged["out"], staged["tgt"])
    res["metrics"] = depth_metrics(out, tgt, DepthMetrics(background=0.0, contact_eps=1e-3))
    (x,) = hook.inputs("gaussian_blur", staged["blur"])
    res["blur"] = gaussian_blur(x, 5)
    (x,) = hook.inputs("channel_stats", staged["stats"])
    res["channel_stats"] = channel_stats(x)
    for mode in ("area", "bilinear"):
        x, base = hook.inputs(f"resize_affine {mode}", staged["x"], staged["base"])
        res[f"resize.{mode}"] = resize_affine(x, (11, 13), [0.5, 1.0, 2.0], [0.0, -1.0, 3.0], base=base, mode=mode)
    hook.inputs("DeviceDataset")
    ds = DeviceDataset(objects=staged["objects"], device="cuda", use_difference_image=True, image_normalization_method="0_255_to_0_1",
                       depth_normalization_method="min_max_to_0_-1", norm_scale=0.9)
    aug = Augment(seed=3, hflip=0.5, vflip=0.5, max_shift=(3, 4), gain=0.1, offset=5.0, noise_std=2.0)
    torch.manual_seed(17)
    hook.inputs("DeviceLoader")
    batch = next(iter(DeviceLoader(ds, 4, shuffle=True, augment=aug)))
    res.update({f"batch.{k}": t for k, t in batch.items() if isinstance(t, torch.Tensor)})
    return res


WORKLOADS = {w.name: w for w in (Workload("mesh_grid", _mesh_grid_stage, _mesh_grid_run), Workload("contact", _contact_stage, _contact_run),
                                 Workload("mesh_volume", _mesh_volume_stage, _mesh_volume_run),
                                 Workload("touch_fusion", _touch_stage, _touch_run), Workload("metrics_data", _metrics_stage, _metrics_run))}
