"""Connected contact patches of depth images, on the device (libgsd's gsd_contact_patches_*,
include/gsd.h).

A predicted depth image carries speckle: blobs of a few pixels below the contact threshold, far from the real imprint.
`contact_patches` labels the contact mask of every (image, channel) plane into 4- or 8-connected patches, drops the small ones,
numbers the rest as `scipy.ndimage.label` would, and describes each by integer statistics from which area, centroid, principal
axis, volume and peak follow.  `ContactPatches.filtered_depth` removes what was dropped from the depth image; its output feeds
`depth_points`, `score_poses` and `estimate_pose` unchanged.  Nothing is read back to the host anywhere."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib
from .mesh_depth import MeshDepthError

STAT_COLS = L.GSD_CONTACT_PATCHES_COLS
DQ_SCALE = float(1 << 20)      # the fixed point of column 10: dq = rint(max(d, -1024) * 2^20)


def _int_at_least_one(what: str, name: str, v) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 or v >= 1 << 31:
        raise MeshDepthError(f"{what}: {name} must be an integer >= 1 (below 2^31), got {v!r}")
    return int(v)


def _check_depth(what: str, depth) -> None:
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or not depth.is_cuda:
        raise MeshDepthError(f"{what}: depth must be a float32 (B, 2, H, W) tensor on the GPU, got "
                             f"{getattr(depth, 'dtype', type(depth).__name__)} on {getattr(depth, 'device', 'the host')}")
    if depth.dim() != 4 or depth.shape[1] != 2 or min(depth.shape) < 1:
        raise MeshDepthError(f"{what}: depth must be (B, 2, H, W) with B, H, W >= 1, got {tuple(depth.shape)}")
    if not depth.is_contiguous():
        raise MeshDepthError(f"{what}: depth must be contiguous, got strides {depth.stride()} for shape {tuple(depth.shape)}")


class ContactPatches:
    """What `contact_patches` made, all tensors on the device: `labels` (B, 2, H, W) int32, 0 for background and dropped patches,
    else the patch number (numbers above `max_patches` included); `counts` (B, 2) int32, the TRUE number of kept patches per
    plane, so counts > max_patches says that a plane overflowed; `stats` (B, 2, K, 12) int64 (or None), row j for patch j + 1:
    area, r_min, r_max, k_min, k_max, sum r, sum k, sum r^2, sum k^2, sum r k, sum dq, peak key; rows without a patch are zero.
    The properties derive physical quantities from `stats` in fp64 on the device, (B, 2, K) each, NaN in rows without a patch."""

    def __init__(self, labels, counts, stats, mpp, shape, view) -> None:
        self.labels, self.counts, self.stats, self.mpp, self.shape = labels, counts, stats, float(mpp), tuple(shape)
        self.max_patches = None if stats is None else int(stats.shape[2])
        self._view = view

    # ---- derived quantities -------------------------------------------------------------------------------------------------
    def _need_stats(self, what: str) -> torch.Tensor:
        if self.stats is None:
            raise MeshDepthError(f"ContactPatches.{what}: made with stats=False, there are no statistics")
        return self.stats

    def _col(self, c: int) -> torch.Tensor:
        return self._need_stats("stats")[..., c].to(torch.float64)

    def _used(self) -> torch.Tensor:
        return self._need_stats("stats")[..., 0] > 0

    def _nan_unused(self, t: torch.Tensor) -> torch.Tensor:
        used = self._used()
        while used.dim() < t.dim():
            used = used.unsqueeze(-1)
        return torch.where(used, t, torch.full_like(t, float("nan")))

    @property
    def area_mm2(self) -> torch.Tensor:
        return self._nan_unused(self._col(0) * (self.mpp * self.mpp))

    @property
    def centroid_mm(self) -> torch.Tensor:
        """(B, 2, K, 2): (x, y) = (mpp (mean r - H/2), mpp (mean k - W/2)), `depth_points`' sensor frame."""
        h, w = self.shape[2], self.shape[3]
        n = self._col(0)
        return self._nan_unused(torch.stack((self.mpp * (self._col(5) / n - h / 2), self.mpp * (self._col(6) / n - w / 2)), dim=-1))

    def _central(self):
        """central second moments in pixels^2: mu20 (rows), mu02 (columns), mu11"""
        n = self._col(0)
        mr, mk = self._col(5) / n, self._col(6) / n
        return self._col(7) / n - mr * mr, self._col(8) / n - mk * mk, self._col(9) / n - mr * mk

    @property
    def axis_angle(self) -> torch.Tensor:
        """Angle of the major axis from the row (x) direction towards the column (y) direction, in (-pi/2, pi/2]."""
        m20, m02, m11 = self._central()
        return self._nan_unused(0.5 * torch.atan2(2.0 * m11, m20 - m02))

    @property
    def axis_lengths_mm(self) -> torch.Tensor:
        """(B, 2, K, 2): mpp * sqrt of the eigenvalues of the central second moments, major first (the standard deviations
        along the principal axes)."""
        m20, m02, m11 = self._central()
        half, diff = 0.5 * (m20 + m02), 0.5 * (m20 - m02)
        root = torch.sqrt(diff * diff + m11 * m11)
        major, minor = torch.sqrt(half + root), torch.sqrt(torch.clamp(half - root, min=0.0))
        return self._nan_unused(torch.stack((self.mpp * major, self.mpp * minor), dim=-1))

    @property
    def volume_mm3(self) -> torch.Tensor:
        return self._nan_unused(-self._col(10) / DQ_SCALE * (self.mpp * self.mpp))

    @property
    def mean_depth(self) -> torch.Tensor:
        """Mean depth of the patch in mm (of the depths clamped at -1024 mm), negative."""
        return self._nan_unused(self._col(10) / DQ_SCALE / self._col(0))

    @property
    def peak_depth(self) -> torch.Tensor:
        """fp32: the depth of the deepest pixel, decoded from the key."""
        key = self._need_stats("peak_depth")[..., 11]
        o = key >> 32                                            # ord(d), 0 .. 2^32 - 1
        u = torch.where(o >= (1 << 31), o - (1 << 31), 0xFFFFFFFF - o)      # undo: set sign bit -> ~u, else u | 2^31
        u = torch.where(u >= (1 << 31), u - (1 << 32), u).to(torch.int32)
        return self._nan_unused(u.view(torch.float32))

    @property
    def peak_rc(self) -> torch.Tensor:
        """(B, 2, K, 2) int64: row and column of the deepest pixel, among equals the first in raster order; -1 without a patch."""
        at = self._need_stats("peak_rc")[..., 11] & 0xFFFFFFFF
        w = self.shape[3]
        rc = torch.stack((torch.div(at, w, rounding_mode="floor"), at % w), dim=-1)
        return torch.where(self._used().unsqueeze(-1), rc, torch.full_like(rc, -1))

    @property
    def bbox(self) -> torch.Tensor:
        """(B, 2, K, 4) int64: r_min, r_max, k_min, k_max (inclusive); -1 without a patch."""
        box = self._need_stats("bbox")[..., 1:5]
        return torch.where(self._used().unsqueeze(-1), box, torch.full_like(box, -1))

    # ---- filtering ----------------------------------------------------------------------------------------------------------
    def filtered_depth(self, depth: torch.Tensor, keep_largest: Optional[int] = None) -> torch.Tensor:
        """`depth` bit for bit, except +0.0 where a pixel is contact and its patch is not kept.  A patch is kept when it is
        numbered (it has at least `min_area` pixels); with `keep_largest=n` it must also be among the n largest of its plane
        (on equal areas the lower number wins; patches numbered above `max_patches` are never kept then).  `depth` is the
        tensor the patches were made from."""
        what = "ContactPatches.filtered_depth"
        _check_depth(what, depth)
        if tuple(depth.shape) != self.shape or depth.device != self.labels.device:
            raise MeshDepthError(f"{what}: depth of shape {tuple(depth.shape)} on {depth.device}, the patches are of {self.shape} on "
                                 f"{self.labels.device}")
        b, _, h, w = self.shape
        keep, k = None, 1
        if keep_largest is not None:
            n = _int_at_least_one(what, "keep_largest", keep_largest)
            area = self._need_stats("filtered_depth")[..., 0]
            k = int(area.shape[2])
            # rank by area, largest first; the stable sort leaves equal areas in the order of their numbers
            order = torch.argsort(area, dim=-1, descending=True, stable=True)
            rank = torch.empty_like(order)
            rank.scatter_(-1, order, torch.arange(k, device=area.device).expand_as(order))
            keep = torch.zeros((b, 2, k + 1), device=area.device, dtype=torch.uint8)
            keep[..., 1:] = ((rank < n) & (area > 0)).to(torch.uint8)
        with torch.cuda.device(depth.device):
            out = torch.empty_like(depth)
            check(lib.gsd_contact_patches_filter(C.byref(self._view), depth.data_ptr(), self.labels.data_ptr(), L.ptr(keep), b, h, w, k,
                                                 out.data_ptr(), L.stream_ptr()), "contact_patches_filter")
        return out

    def __repr__(self) -> str:
        b, _, h, w = self.shape
        rows = "no statistics" if self.stats is None else f"statistics of up to {self.max_patches} patches per plane"
        return f"ContactPatches({b} images of 2 x {h} x {w}, connectivity {self._view.connectivity}, min_area {self._view.min_area}, {rows})"


def contact_patches(depth: torch.Tensor, contact_depth: float = 0.0, connectivity: int = 8, min_area: int = 1, max_patches: int = 64,
                    image_height_mm: float = 12.0, stats: bool = True) -> ContactPatches:
    """The connected contact patches of the depth images `depth` (B, 2, H, W) fp32 in mm, contiguous, on the GPU, as a
    `ContactPatches`.

    A pixel is contact iff d < -contact_depth (`depth_points`' rule: a NaN is not, -inf is).  A patch is a maximal 4- or
    8-connected (`connectivity`) set of contact pixels of one (image, channel) plane.  Patches of fewer than `min_area` pixels are
    dropped; the rest are numbered 1, 2, ... per plane in raster order of their first pixel, as `scipy.ndimage.label` numbers them.
    `max_patches=K` sizes the statistics: patches numbered above K keep their labels and are counted, but have no row.
    `image_height_mm` gives mm per pixel for the derived properties.  Everything stays on the device; nothing is read back."""
    what = "contact_patches"
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise MeshDepthError(f"{what}: connectivity must be 4 or 8, got {connectivity!r}")
    min_area = _int_at_least_one(what, "min_area", min_area)
    k = _int_at_least_one(what, "max_patches", max_patches)
    cdepth = float(contact_depth)
    if not (math.isfinite(cdepth) and cdepth >= 0.0):
        raise MeshDepthError(f"{what}: contact_depth must be finite and >= 0, got {contact_depth!r}")
    _check_depth(what, depth)
    b, _, h, w = (int(d) for d in depth.shape)
    if 2 * b * k * STAT_COLS >= 1 << 31:
        raise MeshDepthError(f"{what}: max_patches {k} for {b} images is more than one table holds (2 B K 12 below 2^31)")
    mpp = float(image_height_mm) / h
    if not (math.isfinite(mpp) and mpp > 0.0):
        raise MeshDepthError(f"{what}: image_height_mm {image_height_mm!r} must be finite and positive")
    words = int(lib.gsd_contact_patches_workspace(b, h, w))
    if words < 1:
        raise MeshDepthError(f"{what}: {b} x 2 x {h} x {w} is more than one call takes (2^31 - 1 pixels): label it in parts")
    view = L.gsd_contact_patches_view()
    view.contact_depth, view.connectivity, view.min_area = cdepth, int(connectivity), min_area
    dev = depth.device
    with torch.cuda.device(dev):
        ws = torch.empty((words,), device=dev, dtype=torch.int32)
        labels = torch.empty((b, 2, h, w), device=dev, dtype=torch.int32)
        counts = torch.empty((b, 2), device=dev, dtype=torch.int32)
        check(lib.gsd_contact_patches_label(C.byref(view), depth.data_ptr(), b, h, w, labels.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                            words, L.stream_ptr()), "contact_patches_label")
        table = None
        if stats:
            table = torch.empty((b, 2, k, STAT_COLS), device=dev, dtype=torch.int64)
            check(lib.gsd_contact_patches_stats(C.byref(view), depth.data_ptr(), labels.data_ptr(), b, h, w, k, table.data_ptr(),
                                                L.stream_ptr()), "contact_patches_stats")
    return ContactPatches(labels, counts, table, mpp, (b, 2, h, w), view)
