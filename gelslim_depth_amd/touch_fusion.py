"""Touches fused into a surface, on the device: a truncated signed distance volume and its mesh (libgsd's
gsd_touch_*, include/gsd.h).

`render_depth`, `estimate_pose`, `depth_points` and `register_cloud` all work round an object whose mesh somebody else made.  This
module makes one from touches: depth images of an unknown object (the U-Net's, or rendered labels), each with the rigid map from the
object frame to its grasp frame, are fused into a voxel volume, and the volume's zero level is extracted as triangles that
`MeshVolume` and `MeshGrid` take as they are.

  TouchVolume        the voxel lattice and its state: `acc` = sum w * sample, `weight` = sum w.
  touch_transforms   the object -> grasp map of in-hand poses (t1, t2, theta): the inverse of `depth_points`' object frame.
  integrate_touches  fuses K touches into the volume, in place (gsd_touch_integrate).  Contact pixels give signed distances
                     along the view axis, truncated at `truncation_mm`; a gel that is not indented proves the space above it empty.
  extract_surface    marching tetrahedra over the observed cells (gsd_touch_extract_*): a watertight fp32 mesh in a fixed order.
  write_stl          binary STL of the result, host code.

Both kernels are gathers in a fixed order without float atomics: every voxel looks itself up in every touch.  So K touches in one
call equal any split into consecutive calls bit for bit, and tests/touch_fusion_ref.py holds both to a numpy twin bit for bit.
Colour or normals per voxel, marching cubes, hole filling, simplification, sparse volumes and pose estimation during fusion are out
of scope: poses are inputs, `register_cloud` can refine them beforehand."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib
from .mesh_depth import MeshDepthError, MeshGrid, _check_widths, _need_cuda, plane_convention

AXIS_MAX = 1024      # voxels per axis that the kernels take


def _triple(what: str, name: str, v) -> tuple:
    try:
        out = tuple(float(x) for x in (v.tolist() if isinstance(v, (torch.Tensor, np.ndarray)) else v))
    except (TypeError, ValueError):
        out = ()
    if len(out) != 3 or not all(math.isfinite(x) for x in out):
        raise MeshDepthError(f"{what}: {name} must be three finite numbers, got {v!r}")
    return out


class TouchVolume:
    """A lattice of `shape` = (nx, ny, nz) voxels in the object frame of `depth_points(frame="object")` (mm): voxel (ix, iy, iz) sits
    at origin_mm + voxel_mm * (ix, iy, iz).  `acc` and `weight` are (nz, ny, nx) float32 tensors on the device, zero at first;
    `integrate_touches` updates them, and a caller may fill them with a field of its own (`acc` = f, `weight` = 1).
    `truncation_mm` is the band on either side of the surface inside which a contact sample carries a distance; it must be at least
    2 voxel_mm, since a thinner band leaves no observed voxel inside the object next to the surface."""

    def __init__(self, origin_mm, voxel_mm: float, shape: Sequence[int], truncation_mm: float, device=None) -> None:
        what = "TouchVolume"
        self.origin = _triple(what, "origin_mm", origin_mm)
        try:
            dims = tuple(int(d) for d in shape)
            whole = all(float(d) == int(d) for d in shape)
        except (TypeError, ValueError):
            dims, whole = (), False
        if len(dims) != 3 or not whole or not all(2 <= d <= AXIS_MAX for d in dims):
            raise MeshDepthError(f"{what}: shape must be (nx, ny, nz) with 2..{AXIS_MAX} voxels per axis, got {shape!r}")
        h, tau = float(voxel_mm), float(truncation_mm)
        if not (math.isfinite(h) and h > 0.0 and math.isfinite(tau) and tau > 0.0):
            raise MeshDepthError(f"{what}: voxel_mm and truncation_mm must be finite and positive, got {voxel_mm!r} and {truncation_mm!r}")
        if tau < 2.0 * h:
            raise MeshDepthError(f"{what}: truncation_mm {tau!r} is below 2 voxel_mm = {2.0 * h!r}: no observed voxel would lie inside the object")
        self.voxel_mm, self.truncation_mm, self.dims = h, tau, dims
        self.device = _need_cuda(device)
        self.volume = L.gsd_touch_volume()
        self.volume.x0, self.volume.y0, self.volume.z0 = self.origin
        self.volume.voxel, self.volume.truncation = h, tau
        self.volume.nx, self.volume.ny, self.volume.nz = dims
        self.volume.reserved = 0
        with torch.cuda.device(self.device):
            self.acc = torch.zeros((dims[2], dims[1], dims[0]), device=self.device, dtype=torch.float32)
            self.weight = torch.zeros_like(self.acc)

    @classmethod
    def around(cls, bbox_min, bbox_max, voxel_mm: float, truncation_mm: float, margin_mm: Optional[float] = None, device=None) -> "TouchVolume":
        """The volume whose lattice covers the box bbox_min .. bbox_max (mm) and `margin_mm` around it (default: the truncation plus
        one voxel, so that the band outside the surface is inside the volume)."""
        what = "TouchVolume.around"
        lo, hi = _triple(what, "bbox_min", bbox_min), _triple(what, "bbox_max", bbox_max)
        h, tau = float(voxel_mm), float(truncation_mm)
        if not (math.isfinite(h) and h > 0.0 and math.isfinite(tau) and tau > 0.0):
            raise MeshDepthError(f"{what}: voxel_mm and truncation_mm must be finite and positive, got {voxel_mm!r} and {truncation_mm!r}")
        margin = tau + h if margin_mm is None else float(margin_mm)
        if not (math.isfinite(margin) and margin >= 0.0) or any(b < a for a, b in zip(lo, hi)):
            raise MeshDepthError(f"{what}: margin_mm must be finite and >= 0 and bbox_max not below bbox_min, got {margin_mm!r}, {lo}, {hi}")
        dims = tuple(max(2, int(math.ceil((b - a + 2.0 * margin) / h)) + 1) for a, b in zip(lo, hi))
        if max(dims) > AXIS_MAX:
            raise MeshDepthError(f"{what}: {dims} voxels, at most {AXIS_MAX} per axis: use a larger voxel_mm")
        return cls(tuple(a - margin for a in lo), h, dims, tau, device)

    @property
    def shape(self):
        """(nz, ny, nx), the shape of `acc` and `weight`."""
        return tuple(self.acc.shape)

    def reset(self) -> None:
        self.acc.zero_()
        self.weight.zero_()

    def tsdf(self) -> torch.Tensor:
        """acc / weight in units of the truncation (1: free space, negative: inside), NaN where nothing was observed."""
        return torch.where(self.weight > 0, self.acc / self.weight, torch.full_like(self.acc, float("nan")))

    def _state(self, what: str):
        shape = (self.dims[2], self.dims[1], self.dims[0])
        for name, t in (("acc", self.acc), ("weight", self.weight)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != shape
                    or not t.is_contiguous()):
                raise MeshDepthError(f"{what}: volume.{name} must be a contiguous float32 {shape} tensor on {self.device}")
        return self.acc, self.weight

    def __repr__(self) -> str:
        return (f"TouchVolume({self.dims[0]} x {self.dims[1]} x {self.dims[2]} voxels of {self.voxel_mm:.4g} mm from {self.origin}, "
                f"truncation {self.truncation_mm:.4g} mm)")


def touch_transforms(poses, gelslim_plane: str = "+y+z", mid: float = 0.0, grid: Optional[MeshGrid] = None,
                     invert_affine: bool = False) -> torch.Tensor:
    """(K, 12) float64, on the poses' device: for each in-hand pose (t1 [m], t2 [m], theta [rad]) the row-major 3 x 4 map from the
    object frame (the mesh file's coordinates times pc_scale, mm) to the grasp frame (u unaligned, v aligned, q perpendicular with the
    right finger at q > 0) -- the inverse of `depth_points(frame="object")` and the map that `render_depth` images through.  With
    M = [[cos, -sin, 1000 t1], [sin, cos, 1000 t2]] (M^-1 with `invert_affine`) the in-plane pair in ascending axis order goes through
    M and is named by the plane; q = multiplier * (p[perp] - mid).  `grid` supplies the plane and `mid` of a MeshGrid.  Computed with
    torch in fp64, nothing is read back.  The map is improper (det = -1) for half of the planes; nothing downstream minds."""
    what = "touch_transforms"
    if grid is not None:
        if not isinstance(grid, MeshGrid):
            raise MeshDepthError(f"{what}: grid must be a MeshGrid, got {type(grid).__name__}")
        gelslim_plane, mid = grid.gelslim_plane, grid.mid
    try:
        perp, aligned, unaligned, multiplier = plane_convention(gelslim_plane)
    except ValueError:
        raise MeshDepthError(f"{what}: invalid gelslim_plane {gelslim_plane!r}") from None
    mid = float(mid)
    if not math.isfinite(mid):
        raise MeshDepthError(f"{what}: mid must be finite, got {mid!r}")
    p = torch.as_tensor(poses)
    if p.dim() == 1 and p.shape[0] == 3:
        p = p.unsqueeze(0)
    if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1 or not p.dtype.is_floating_point:
        raise MeshDepthError(f"{what}: poses must be a floating (K, 3) tensor with K >= 1, got {tuple(p.shape)} {p.dtype}")
    p = p.to(torch.float64)
    cs, sn, a1, a2 = torch.cos(p[:, 2]), torch.sin(p[:, 2]), 1000.0 * p[:, 0], 1000.0 * p[:, 1]
    if invert_affine:          # M^-1 = [R^T | -R^T a]
        m = ((cs, sn, -(cs * a1 + sn * a2)), (-sn, cs, -(cs * a2 - sn * a1)))
    else:
        m = ((cs, -sn, a1), (sn, cs, a2))
    lo, hi = sorted((aligned, unaligned))
    zero = torch.zeros_like(cs)

    def row(r):          # the in-plane row r of m over the object's axes
        cols = [zero, zero, zero, r[2]]
        cols[lo], cols[hi] = r[0], r[1]
        return cols
    ra, rb = row(m[0]), row(m[1])
    ru, rv = (rb, ra) if aligned < unaligned else (ra, rb)
    rq = [zero, zero, zero, zero + (-multiplier * mid)]
    rq[perp] = zero + float(multiplier)
    return torch.stack(ru + rv + rq, dim=1).contiguous()


def _rows12(what: str, volume: TouchVolume, transforms, k: int) -> torch.Tensor:
    from .mesh_register import _transforms
    t = _transforms(what, volume, transforms)
    if t.shape[0] == 1 and k > 1:
        t = t.expand(k, 12).contiguous()
    if t.shape[0] != k:
        raise MeshDepthError(f"{what}: {k} touches but {t.shape[0]} transforms")
    return t


def integrate_touches(volume: TouchVolume, depth: torch.Tensor, grasp_widths: torch.Tensor, transforms, image_height_mm: float = 12.0,
                      grasp_width_offset: float = 0.0, LR_flip: bool = False, contact_depth: float = 0.0, carve_weight: float = 1.0,
                      weights: Optional[torch.Tensor] = None, cull: bool = True, validate: bool = True) -> TouchVolume:
    """Fuse the K touches `depth` (K, 2, H, W) fp32 in mm, channels as `render_depth`'s (left, right; swapped by `LR_flip`), into
    `volume`, in place; returns the volume.  `grasp_widths` (K,) fp32; `transforms` (K, 12), (K, 4, 4) or one (4, 4) for all: object
    -> grasp frame (`touch_transforms`, or any rigid map; not checked for orthonormality).

    Every voxel p is mapped into each touch, (u, v, q), and onto the image of either finger (s = +1 right, -1 left) at row
    rf = s u / mpp + H/2, column kf = v / mpp + W/2; the four pixels round (rf, kf) are interpolated to a depth d, and
    phi = s q - g/2 + d is the height of p above the observed gel surface along the view axis.  Where all four pixels are contact
    (d < -contact_depth, `depth_points`' rule) and phi >= -truncation the voxel receives min(phi / truncation, 1) with the touch's
    weight (`weights` (K,) fp32, default 1); where the quad is finite but not contact and phi > 0 it receives +1 with weight
    `carve_weight` times that: free space.  Behind the surface, off the sensor, or at a non-finite pixel: nothing.  Touches are
    applied in order and channel 0 before channel 1, in fp32 onto the stored state, so one call equals any split into consecutive
    calls bit for bit; `cull` (blocks skip touches that cannot reach their brick) never changes a bit.

    `validate=True` reads the smallest grasp width + offset back and raises MeshDepthError for a negative or non-finite one, as
    `render_depth` does; with `validate=False` nothing is read back and such a touch contributes nothing."""
    what = "integrate_touches"
    if not isinstance(volume, TouchVolume):
        raise MeshDepthError(f"{what}: volume must be a TouchVolume, got {type(volume).__name__}")
    acc, weight = volume._state(what)
    dev = volume.device

    def f32(name, t, shape):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev:
            raise MeshDepthError(f"{what}: {name} must be a float32 {shape} tensor on {dev}, got {getattr(t, 'dtype', type(t).__name__)} on "
                                 f"{getattr(t, 'device', 'the host')}")
        return t
    f32("depth", depth, "(K, 2, H, W)")
    if depth.dim() != 4 or depth.shape[1] != 2 or depth.shape[0] < 1 or depth.shape[2] < 2 or depth.shape[3] < 2:
        raise MeshDepthError(f"{what}: depth must be (K, 2, H, W) with K >= 1 and H, W >= 2, got {tuple(depth.shape)}")
    k, _, h, w = (int(d) for d in depth.shape)
    if 2 * k * h * w >= 1 << 31:
        raise MeshDepthError(f"{what}: {k} x 2 x {h} x {w} is more than one call takes (2^31 - 1 pixels): integrate it in parts")
    f32("grasp_widths", grasp_widths, "(K,)")
    if tuple(grasp_widths.shape) != (k,):
        raise MeshDepthError(f"{what}: {k} touches but grasp_widths of shape {tuple(grasp_widths.shape)}")
    if weights is not None:
        f32("weights", weights, "(K,)")
        if tuple(weights.shape) != (k,):
            raise MeshDepthError(f"{what}: {k} touches but weights of shape {tuple(weights.shape)}")
        weights = weights.contiguous()
    rows = _rows12(what, volume, transforms, k)
    height, offset, cdepth, carve = float(image_height_mm), float(grasp_width_offset), float(contact_depth), float(carve_weight)
    if not (math.isfinite(height) and height > 0.0 and math.isfinite(offset)):
        raise MeshDepthError(f"{what}: image_height_mm must be finite and positive and grasp_width_offset finite, got {image_height_mm!r} "
                             f"and {grasp_width_offset!r}")
    if not (math.isfinite(cdepth) and cdepth >= 0.0 and math.isfinite(carve) and carve >= 0.0):
        raise MeshDepthError(f"{what}: contact_depth and carve_weight must be finite and >= 0, got {contact_depth!r} and {carve_weight!r}")
    depth, grasp_widths = depth.contiguous(), grasp_widths.contiguous()
    if validate:
        _check_widths(what, grasp_widths, offset)
    view = L.gsd_touch_view()
    view.image_height_mm, view.width_offset, view.contact_depth, view.carve_weight = height, offset, cdepth, carve
    view.lr_flip, view.cull = int(bool(LR_flip)), int(bool(cull))
    with torch.cuda.device(dev):
        check(lib.gsd_touch_integrate(C.byref(volume.volume), C.byref(view), depth.data_ptr(), grasp_widths.data_ptr(), rows.data_ptr(),
                                      L.ptr(weights), k, h, w, acc.data_ptr(), weight.data_ptr(), L.stream_ptr()), "touch_integrate")
    return volume


class TouchSurface:
    """What `extract_surface` made, all tensors on the device: `triangles` (T, 3, 3) fp32 in mm (triangle, vertex, xyz), normals out
    of the object, ordered by cell, tetrahedron and table; `cell` (T,) int32 = (iz (ny - 1) + iy) (nx - 1) + ix of each triangle's
    cell (or None); `count`, the TRUE number of triangles as a 0-d int64.  Padded (`max_triangles=M`): (M, 3, 3) / (M,), the first
    min(count, M) triangles, then NaN (cell: -1); count > M says that the buffer overflowed."""

    def __init__(self, triangles, cell, count, max_triangles=None) -> None:
        self.triangles, self.cell, self.count, self.max_triangles = triangles, cell, count, max_triangles

    @property
    def padded(self) -> bool:
        return self.max_triangles is not None

    def vertices(self) -> torch.Tensor:
        """(3 T, 3): every triangle's corners, for `cloud_mesh_error` and `closest_points` (NaN rows are ignored there)."""
        return self.triangles.reshape(-1, 3)

    def __repr__(self) -> str:
        layout = f"padded to {self.max_triangles}" if self.padded else f"{self.triangles.shape[0]} triangles packed"
        return f"TouchSurface({layout}{', cell' if self.cell is not None else ''})"


def extract_surface(volume: TouchVolume, min_weight: float = 0.0, max_triangles: Optional[int] = None, cells: bool = False) -> TouchSurface:
    """The zero level of f = acc / weight as triangles, by marching tetrahedra.  A voxel is observed iff
    weight > min_weight and inside iff f < 0; a cell is used iff its eight corners are observed, split into six tetrahedra the same
    way everywhere, and a vertex on a lattice edge is computed in fp64 from the edge's two voxels in ascending linear index, so every
    cell that shares the edge stores the same fp32 bits: the mesh is watertight as it stands wherever the observed region closes.
    Zero-area triangles are kept (`MeshGrid` and `MeshVolume` skip them).

    `max_triangles=None`: packed (T, 3, 3); the call reads the total back once to allocate.  `max_triangles=M`: padded (M, 3, 3),
    NaN beyond the triangles, later triangles dropped, `count` still true; nothing is read back.  `cells=True` adds `cell`."""
    what = "extract_surface"
    if not isinstance(volume, TouchVolume):
        raise MeshDepthError(f"{what}: volume must be a TouchVolume, got {type(volume).__name__}")
    acc, weight = volume._state(what)
    mw = float(min_weight)
    if not (math.isfinite(mw) and mw >= 0.0):
        raise MeshDepthError(f"{what}: min_weight must be finite and >= 0, got {min_weight!r}")
    if max_triangles is not None and (isinstance(max_triangles, bool) or not isinstance(max_triangles, (int, np.integer)) or max_triangles < 1
                                      or int(max_triangles) >= 1 << 31):
        raise MeshDepthError(f"{what}: max_triangles must be None or an integer in 1 .. 2^31 - 1, got {max_triangles!r}")
    dev = volume.device
    words = int(lib.gsd_touch_extract_workspace(C.byref(volume.volume)))
    with torch.cuda.device(dev):
        ws = torch.empty((words,), device=dev, dtype=torch.int32)
        total = torch.empty((1,), device=dev, dtype=torch.int64)
        check(lib.gsd_touch_extract_count(C.byref(volume.volume), acc.data_ptr(), weight.data_ptr(), mw, total.data_ptr(), ws.data_ptr(),
                                          words, L.stream_ptr()), "touch_extract_count")
        if max_triangles is None:
            rows, capacity = int(total.item()), 0          # the one host read: the total to allocate by
            if rows >= 1 << 31:
                raise MeshDepthError(f"{what}: {rows} triangles, at most 2^31 - 1 in one call")
        else:
            rows = capacity = int(max_triangles)
        tri = torch.empty((rows, 3, 3), device=dev, dtype=torch.float32)
        cell = torch.empty((rows,), device=dev, dtype=torch.int32) if cells else None
        if rows > 0:
            check(lib.gsd_touch_extract_write(C.byref(volume.volume), acc.data_ptr(), weight.data_ptr(), mw, capacity, rows, tri.data_ptr(),
                                              L.ptr(cell), ws.data_ptr(), words, L.stream_ptr()), "touch_extract_write")
    return TouchSurface(tri, cell, total[0], None if max_triangles is None else int(max_triangles))


def write_stl(path, triangles) -> int:
    """Write (..., 3, 3) triangles (a tensor, an array or a TouchSurface) as binary STL with unit facet normals (0 for a zero-area
    triangle); a triangle with a NaN is skipped, so a padded surface can be written as it is.  Host code, numpy only; `read_stl`
    reads it back bit for bit.  Returns the number of triangles written."""
    if isinstance(triangles, TouchSurface):
        triangles = triangles.triangles
    if isinstance(triangles, torch.Tensor):
        triangles = triangles.detach().cpu().numpy()
    tri = np.asarray(triangles, dtype=np.float32)
    if tri.ndim < 2 or tri.shape[-2:] != (3, 3):
        raise MeshDepthError(f"write_stl: triangles must be (..., 3, 3), got {tri.shape}")
    tri = tri.reshape(-1, 3, 3)
    tri = tri[~np.isnan(tri).any(axis=(1, 2))]
    if tri.shape[0] >= 1 << 32:
        raise MeshDepthError(f"write_stl: {tri.shape[0]} triangles, a binary STL counts them in 32 bits")
    v = tri.astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    length = np.linalg.norm(n, axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(length > 0.0, n / length, 0.0)
    rec = np.zeros(tri.shape[0], dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    rec["n"], rec["v"] = n, tri
    with open(path, "wb") as fh:
        fh.write(b"gelslim_depth_amd touch fusion".ljust(80, b"\0"))
        fh.write(np.uint32(tri.shape[0]).tobytes())
        fh.write(rec.tobytes())
    return int(tri.shape[0])
