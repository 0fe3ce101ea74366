"""Contact point clouds and normals from depth images, on the device: the inverse of `render_depth`'s pixel -> mesh map
(libgsd's gsd_depth_points_*, include/gsd.h).

The U-Net maps tactile RGB to depth; `depth_points` turns that depth -- or a rendered one -- into geometry in physical
coordinates: every contact pixel becomes a point in mm with a unit normal, in the sensor frame (per finger), the grasp frame (both
fingers in one frame, `grasp_widths` apart) or the object frame (the mesh file's coordinates times pc_scale, given the in-hand
`poses`).  A cloud made from `render_depth(grid, poses, g)` with the same poses and widths lies on the mesh.  The order of the
points is fixed -- image, channel as stored, row, column -- and is part of the contract; `write_ply` stores a cloud for MeshLab,
Open3D or PCL."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib
from .mesh_depth import MeshDepthError, MeshGrid, _check_widths, plane_convention

FRAMES = ("sensor", "grasp", "object")


class ContactCloud:
    """What `depth_points` made, all tensors on the device: `points` fp32 in mm and `normals` fp32 of unit length (or None),
    `pixel` int32 = ((b * 2 + ch) * H + r) * W + k (or None), `counts` (B, 2) int32, the TRUE number of points per (image,
    channel), and `frame`.  Packed (`max_points=None`): (N, 3) / (N,), ordered by image, channel, row, column; `image(b)` and
    `finger(b, ch)` slice it from a host copy of `counts` that the call fetched anyway.  Padded: (B, M, 3) / (B, M), image b's
    first min(n_b, M) points, then NaN (pixel: -1); counts[b].sum() > M says that the image overflowed."""

    def __init__(self, points, normals, pixel, counts, frame, max_points=None, host_counts=None) -> None:
        self.points, self.normals, self.pixel, self.counts, self.frame = points, normals, pixel, counts, frame
        self.max_points = max_points
        self._host = host_counts          # (B, 2) numpy, packed clouds only

    @property
    def padded(self) -> bool:
        return self.max_points is not None

    def _parts(self, sl):
        pick = lambda t: None if t is None else t[sl]
        return pick(self.points), pick(self.normals), pick(self.pixel)

    def _offsets(self) -> np.ndarray:
        if self._host is None:
            self._host = self.counts.cpu().numpy()
        return np.concatenate(([0], np.cumsum(self._host.reshape(-1), dtype=np.int64)))

    def image(self, b: int):
        """(points, normals, pixel) of image b, both channels in order; of a padded cloud its M rows."""
        if self.padded:
            return self._parts(int(b))
        off = self._offsets()
        return self._parts(slice(int(off[2 * b]), int(off[2 * b + 2])))

    def finger(self, b: int, ch: int):
        """(points, normals, pixel) of channel `ch` (as stored) of image b; a packed cloud only -- a padded image may have
        dropped points, so its channels are told apart by `pixel`."""
        if self.padded:
            raise MeshDepthError("ContactCloud.finger: a padded cloud is sliced per image; tell its channels apart by `pixel`")
        off = self._offsets()
        return self._parts(slice(int(off[2 * b + ch]), int(off[2 * b + ch + 1])))

    def __repr__(self) -> str:
        layout = f"padded to {self.max_points} per image" if self.padded else f"{self.points.shape[0]} points packed"
        extras = ", ".join(n for n, t in (("normals", self.normals), ("pixel", self.pixel)) if t is not None)
        return f"ContactCloud({self.counts.shape[0]} images, {layout}, frame {self.frame!r}{', ' + extras if extras else ''})"


def _f32_on(what: str, name: str, t, shape, device) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
        raise MeshDepthError(f"{what}: {name} must be a float32 {shape} tensor on the GPU, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', 'the host')}")
    if device is not None and t.device != device:
        raise MeshDepthError(f"{what}: {name} is on {t.device}, depth on {device}")
    return t


def depth_points(depth: torch.Tensor, grasp_widths: Optional[torch.Tensor] = None, image_height_mm: float = 12.0,
                 grasp_width_offset: float = 0.0, LR_flip: bool = False, stride: int = 1, contact_depth: float = 0.0,
                 frame: str = "grasp", poses: Optional[torch.Tensor] = None, invert_affine: bool = False,
                 gelslim_plane: str = "+y+z", mid: float = 0.0, grid: Optional[MeshGrid] = None, normals: bool = True,
                 pixels: bool = True, max_points: Optional[int] = None, validate: bool = True) -> ContactCloud:
    """The contact points of the depth images `depth` (B, 2, H, W) fp32 in mm, channels as `render_depth`'s (left, right;
    swapped by `LR_flip`), as a `ContactCloud`.

    A pixel of the lattice r = stride // 2 + i * stride, k = stride // 2 + j * stride (`score_poses`') is a point iff its depth
    d < -contact_depth; a NaN is not.  With mpp = image_height_mm / H:
      frame 'sensor': (mpp (r - H/2), mpp (k - W/2), d) per finger, normal (d_x, d_y, -1) normalised: away from the object;
      frame 'grasp':  (s x, y, s (g/2 - d)), s = +1 for the right finger and -1 for the left, g = grasp_widths + offset: both
                      fingers in the frame `render_depth` images, the right finger at positive third coordinate;
      frame 'object': the mesh's own coordinates (times pc_scale) under the in-hand `poses` (B, 3) = (t1 [m], t2 [m], theta
                      [rad]) -- `grid=MeshGrid` supplies `gelslim_plane` and `mid`; clouds of several grasps concatenate.
    d_x, d_y are differences between immediate neighbours that are themselves contact (central, else one-sided, else 0), so
    the background does not bend the normals at a patch's border.  Everything is computed in fp64 and rounded once.

    `max_points=None`: packed (N, 3); the call reads the total back once to allocate, and fetches `counts` with it.
    `max_points=M`: padded (B, M, 3), NaN beyond an image's points, later points dropped, `counts` still true; nothing is read
    back when `validate=False`.  `validate=True` reads the smallest grasp width + offset back and raises MeshDepthError for a
    negative or non-finite one, as `render_depth` does; without it such an image has no points.  `grasp_widths` is not needed,
    and ignored, in the sensor frame."""
    what = "depth_points"
    _f32_on(what, "depth", depth, "(B, 2, H, W)", None)
    if depth.dim() != 4 or depth.shape[1] != 2 or min(depth.shape) < 1:
        raise MeshDepthError(f"{what}: depth must be (B, 2, H, W) with B, H, W >= 1, got {tuple(depth.shape)}")
    b, _, h, w = (int(d) for d in depth.shape)
    if frame not in FRAMES:
        raise MeshDepthError(f"{what}: frame must be one of {FRAMES}, got {frame!r}")
    fr = FRAMES.index(frame)
    if grid is not None:
        if not isinstance(grid, MeshGrid):
            raise MeshDepthError(f"{what}: grid must be a MeshGrid, got {type(grid).__name__}")
        if grid.device != depth.device:
            raise MeshDepthError(f"{what}: depth is on {depth.device}, the mesh on {grid.device}")
        gelslim_plane, mid = grid.gelslim_plane, grid.mid
    try:
        perp, aligned, unaligned, multiplier = plane_convention(gelslim_plane)
    except ValueError:
        raise MeshDepthError(f"{what}: invalid gelslim_plane {gelslim_plane!r}") from None
    if fr >= 1:
        if grasp_widths is None:
            raise MeshDepthError(f"{what}: frame {frame!r} needs grasp_widths")
        _f32_on(what, "grasp_widths", grasp_widths, "(B,)", depth.device)
        if tuple(grasp_widths.shape) != (b,):
            raise MeshDepthError(f"{what}: {b} images but grasp_widths of shape {tuple(grasp_widths.shape)}")
        grasp_widths = grasp_widths.contiguous()
    else:
        grasp_widths = None
    if fr == 2:
        if poses is None:
            raise MeshDepthError(f"{what}: frame 'object' needs poses")
        _f32_on(what, "poses", poses, "(B, 3)", depth.device)
        if tuple(poses.shape) != (b, 3):
            raise MeshDepthError(f"{what}: {b} images but poses of shape {tuple(poses.shape)}")
        poses = poses.contiguous()
    else:
        poses = None
    mpp = float(image_height_mm) / h
    if not (math.isfinite(mpp) and mpp > 0.0):
        raise MeshDepthError(f"{what}: image_height_mm {image_height_mm!r} must be finite and positive")
    offset, mid = float(grasp_width_offset), float(mid)
    if not math.isfinite(offset) or not math.isfinite(mid):
        raise MeshDepthError(f"{what}: grasp_width_offset and mid must be finite, got {grasp_width_offset!r} and {mid!r}")
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1:
        raise MeshDepthError(f"{what}: stride must be an integer >= 1, got {stride!r}")
    cdepth = float(contact_depth)
    if not (math.isfinite(cdepth) and cdepth >= 0.0):
        raise MeshDepthError(f"{what}: contact_depth must be finite and >= 0, got {contact_depth!r}")
    if max_points is not None and (isinstance(max_points, bool) or not isinstance(max_points, (int, np.integer)) or max_points < 1
                                   or b * int(max_points) >= 1 << 31):
        raise MeshDepthError(f"{what}: max_points must be None or an integer >= 1 with B * max_points below 2^31, got {max_points!r}")
    words = int(lib.gsd_depth_points_workspace(b, h, w, int(stride)))
    if words < 1:
        raise MeshDepthError(f"{what}: {b} x 2 x {h} x {w} is more than one call takes (2^31 - 1 pixels): convert it in parts")
    depth = depth.contiguous()
    if validate and fr >= 1:
        _check_widths(what, grasp_widths, offset)
    view = L.gsd_depth_points_view()
    view.mpp, view.width_offset, view.contact_depth, view.mid = mpp, offset, cdepth, mid
    view.perp_ind, view.swap_axes, view.multiplier = perp, int(aligned < unaligned), multiplier
    view.invert_affine, view.lr_flip, view.frame = int(bool(invert_affine)), int(bool(LR_flip)), fr
    dev = depth.device
    with torch.cuda.device(dev):
        ws = torch.empty((words,), device=dev, dtype=torch.int32)
        counts = torch.empty((b, 2), device=dev, dtype=torch.int32)
        check(lib.gsd_depth_points_count(C.byref(view), depth.data_ptr(), L.ptr(grasp_widths), b, h, w, int(stride), counts.data_ptr(),
                                         ws.data_ptr(), words, L.stream_ptr()), "depth_points_count")
        host_counts = None
        if max_points is None:
            host_counts = counts.cpu().numpy()          # the one host read: the total to allocate by, per (image, channel)
            rows, shape, capacity = int(host_counts.sum()), (int(host_counts.sum()),), 0
        else:
            rows, shape, capacity = b * int(max_points), (b, int(max_points)), int(max_points)
        points = torch.empty(shape + (3,), device=dev, dtype=torch.float32)
        nrm = torch.empty(shape + (3,), device=dev, dtype=torch.float32) if normals else None
        pix = torch.empty(shape, device=dev, dtype=torch.int32) if pixels else None
        if rows > 0:
            check(lib.gsd_depth_points_write(C.byref(view), depth.data_ptr(), L.ptr(grasp_widths), L.ptr(poses), b, h, w, int(stride),
                                             capacity, rows, points.data_ptr(), L.ptr(nrm), L.ptr(pix), ws.data_ptr(), words,
                                             L.stream_ptr()), "depth_points_write")
    return ContactCloud(points, nrm, pix, counts, frame, None if max_points is None else int(max_points), host_counts)


def write_ply(path, points, normals=None) -> int:
    """Write a cloud as binary little-endian PLY: `float x y z` per vertex and, with `normals`, `float nx ny nz`.  `points` and
    `normals` are (..., 3) tensors or arrays; a row with a NaN in its point or its normal is skipped, so a padded cloud can be
    written as it is.  Host code, numpy only.  Returns the number of vertices written."""
    def host(a, name):
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        a = np.asarray(a, dtype=np.float32)
        if a.ndim < 1 or a.shape[-1] != 3:
            raise MeshDepthError(f"write_ply: {name} must be (..., 3), got {a.shape}")
        return a.reshape(-1, 3)
    rows = host(points, "points")
    if normals is not None:
        nrm = host(normals, "normals")
        if nrm.shape != rows.shape:
            raise MeshDepthError(f"write_ply: {rows.shape[0]} points but {nrm.shape[0]} normals")
        rows = np.concatenate((rows, nrm), axis=1)
    rows = rows[~np.isnan(rows).any(axis=1)]
    names = ("x", "y", "z", "nx", "ny", "nz")[:rows.shape[1]]
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {rows.shape[0]}\n" + \
        "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(np.ascontiguousarray(rows, dtype="<f4").tobytes())
    return int(rows.shape[0])
