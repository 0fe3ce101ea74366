"""Closest points on a mesh and 6-DoF registration of contact clouds, on the device.

`depth_points` turns depth images into clouds in millimetres; this module measures such a cloud against its object in 3-D and
registers it under a full rigid motion -- the step that `estimate_pose` / `refine_pose`, which move (t1, t2, theta) in the sensor
plane, cannot make.

  MeshVolume       a 3-D grid of cubic cells over a mesh, built once (gsd_mesh_volume_*), in the object frame of
                   `depth_points(frame="object")`: the file's coordinates times pc_scale, in mm.
  closest_points   the exact nearest surface point of every point of a cloud (gsd_mesh_closest_points).
  icp_rows         the normal-equation rows of a point-to-plane or point-to-point fit over SE(3), fused with that query.
  register_cloud   Levenberg-Marquardt ICP on those rows; nothing is read back from the device.
  cloud_mesh_error mean / rms / max distance of a cloud from the mesh, as device scalars.

Signed distance (inside / outside needs pseudonormals), non-rigid fits and conversions between (t1, t2, theta) and SE(3) beyond
what `depth_points(frame="object")` already does are out of scope."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib
from .mesh_depth import MeshDepthError, _build_cell_lists, _need_cuda, first_argmin

ICP_ROW = L.GSD_ICP_ROW      # columns of a row of `icp_rows`
_KINDS = {"plane": 0, "point": 1}
_LAMBDA_MIN, _LAMBDA_MAX = 1e-12, 1e12      # bounds of the damping in register_cloud


def triangle_cross(v: np.ndarray) -> np.ndarray:
    """(b - a) x (c - a) of (T, 3, 3) fp64 vertices, each component two rounded products and one subtraction: the arithmetic by
    which the kernels decide that a triangle is degenerate (all three exactly 0)."""
    u, w = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    return np.stack((u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]),
                    axis=1)


def default_cell_mm_3d(v: np.ndarray, target: float = 8.0) -> float:
    """Cell size model, the 3-D analogue of `default_cell_mm`.  The cells that a surface of area A crosses number about A / c^2 for
    cells of side c, and a triangle whose box has the footprint s^2 (s^2 = twice the mean triangle area) lands in about
    (s / c + 1)^2 of them, so the mean list of an occupied cell is T (c + s)^2 / A long.  Solving for `target` = 8 entries gives
    c = sqrt(target A / T) - s; it is kept above s / 2 and above 1/512 of the extent.  Nobody has tuned this on the device."""
    ext = float(max((v.max(axis=(0, 1)) - v.min(axis=(0, 1))).max(), 1e-30))
    area = 0.5 * np.sqrt((triangle_cross(v) ** 2).sum(axis=1))
    total = float(area.sum())
    if not (total > 0.0 and math.isfinite(total)):
        return ext
    s = math.sqrt(2.0 * total / v.shape[0])
    return max(math.sqrt(target * total / v.shape[0]) - s, 0.5 * s, ext / 512.0)


class MeshVolume:
    """A mesh prepared for `closest_points`, `icp_rows` and `register_cloud`: the fp32 vertices and the per-cell triangle lists on
    the device, built once.

    triangles: (T, 3, 3) array or tensor (`read_stl`); pc_scale: factor to millimetres; cell_mm: side of a cubic cell, default
    `default_cell_mm_3d` (GSD_MESH_CELL_MM does not apply: it sizes `MeshGrid`).  The vertices are fp32(v * pc_scale), rounded once.
    A triangle whose fp64 cross product is exactly (0, 0, 0) is skipped everywhere (`skipped` counts them).  No result depends on
    the cell size, only the time does.  Building reads one int64 back from the device (the number of (cell, triangle) pairs)."""

    def __init__(self, triangles, pc_scale: float = 1.0, device=None, cell_mm: Optional[float] = None) -> None:
        self.device = _need_cuda(device)
        if isinstance(triangles, torch.Tensor):
            triangles = triangles.detach().cpu().numpy()
        v = np.asarray(triangles, dtype=np.float64)
        if v.ndim != 3 or v.shape[1:] != (3, 3):
            raise MeshDepthError(f"MeshVolume: triangles must be (T, 3, 3), got {v.shape}")
        if v.shape[0] == 0:
            raise MeshDepthError("MeshVolume: the mesh has no triangles")
        if v.shape[0] > 1 << 24:
            raise MeshDepthError(f"MeshVolume: {v.shape[0]} triangles, at most 2^24")
        scale = float(pc_scale)
        if not math.isfinite(scale) or scale == 0.0:
            raise MeshDepthError(f"MeshVolume: pc_scale must be finite and not zero, got {pc_scale!r}")
        with np.errstate(over="ignore", invalid="ignore"):
            tri = (v * scale).astype(np.float32)
        if not np.isfinite(tri).all():
            raise MeshDepthError("MeshVolume: the mesh has a non-finite vertex")
        v = tri.astype(np.float64)
        self.triangles = int(v.shape[0])
        self.skipped = int((triangle_cross(v) == 0.0).all(axis=1).sum())
        cell = default_cell_mm_3d(v) if cell_mm is None else float(cell_mm)
        if not (math.isfinite(cell) and cell > 0.0):
            raise MeshDepthError(f"MeshVolume: cell_mm must be finite and positive, got {cell!r}")
        self.bbox = (v.min(axis=(0, 1)), v.max(axis=(0, 1)))
        self.volume = L.gsd_mesh_volume()
        check(lib.gsd_mesh_volume_plan((C.c_double * 6)(*self.bbox[0], *self.bbox[1]), cell, C.byref(self.volume)), "mesh_volume_plan")
        self.cell_mm = float(self.volume.cell)
        with torch.cuda.device(self.device):
            self.tri = torch.from_numpy(tri.reshape(-1, 9)).to(self.device)
            geometry = (C.byref(self.volume), self.tri.data_ptr(), self.triangles)
            self.cells, self.pairs, self.list = _build_cell_lists(
                "MeshVolume", "mesh_volume", self.device, int(lib.gsd_mesh_volume_workspace(C.byref(self.volume))),
                lambda *ws: lib.gsd_mesh_volume_count(*geometry, *ws), lambda *ws: lib.gsd_mesh_volume_fill(*geometry, *ws))

    @property
    def shape(self):
        """(nz, ny, nx) cells."""
        return int(self.volume.nz), int(self.volume.ny), int(self.volume.nx)

    def _mesh_args(self):
        return (C.byref(self.volume), self.tri.data_ptr(), self.triangles, self.cells.data_ptr(), self.list.data_ptr(), self.list.numel())

    def __repr__(self) -> str:
        return (f"MeshVolume({self.triangles} triangles, {self.skipped} skipped, {self.volume.nx} x {self.volume.ny} x {self.volume.nz} "
                f"cells of {self.cell_mm:.4g} mm, {self.pairs} pairs)")


def _cloud(what: str, volume, points) -> torch.Tensor:
    """`points` as a contiguous float32 (N, 3) tensor on the volume's device; a ContactCloud gives its points (its NaN padding rows
    are non-finite points, which every function here ignores by rule)."""
    if not isinstance(volume, MeshVolume):
        raise MeshDepthError(f"{what}: volume must be a MeshVolume, got {type(volume).__name__}")
    from .contact_points import ContactCloud
    if isinstance(points, ContactCloud):
        points = points.points.reshape(-1, 3)
    if (not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3
            or points.shape[0] < 1):
        raise MeshDepthError(f"{what}: points must be a float32 (N, 3) tensor with N >= 1 or a ContactCloud, got "
                             f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
    if points.device != volume.device:
        raise MeshDepthError(f"{what}: points are on {points.device}, the mesh on {volume.device}")
    return points.contiguous()


def _max_distance(what: str, max_distance_mm) -> float:
    if max_distance_mm is None:
        return math.inf
    try:
        d = float(max_distance_mm)
    except (TypeError, ValueError):
        d = math.nan
    if not d >= 0.0:
        raise MeshDepthError(f"{what}: max_distance_mm must be >= 0 or None, got {max_distance_mm!r}")
    return d


def _out(what: str, name: str, volume: MeshVolume, out, shape, dtype) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, device=volume.device, dtype=dtype)
    if (not isinstance(out, torch.Tensor) or out.dtype != dtype or out.device != volume.device or not out.is_contiguous()
            or tuple(out.shape) != tuple(shape)):
        raise MeshDepthError(f"{what}: {name} must be a contiguous {str(dtype)[6:]} {tuple(shape)} tensor on {volume.device}")
    return out


class ClosestPoints:
    """What `closest_points` found, all tensors on the device: `triangle` (N,) int32 (-1: none), `closest` (N, 3) fp32, `distance`
    (N,) fp32 [mm], `sq_distance` (N,) fp64 [mm^2]."""

    def __init__(self, triangle, closest, distance, sq_distance) -> None:
        self.triangle, self.closest, self.distance, self.sq_distance = triangle, closest, distance, sq_distance

    def __repr__(self) -> str:
        return f"ClosestPoints({self.triangle.shape[0]} points)"


def closest_points(volume: MeshVolume, points, max_distance_mm: Optional[float] = None, out: Optional[ClosestPoints] = None) -> ClosestPoints:
    """The exact nearest surface point of every row of `points` (N, 3) fp32 [mm, object frame]: one libgsd call on torch's current
    stream, nothing synchronises.  Per point the winner is the triangle with the smallest squared distance d^2 (fp64, the region
    method of include/gsd.h), the lowest triangle id among bit-equal ones; `sq_distance` is that d^2, `closest` fp32(x), `distance`
    fp32(sqrt(d^2)).  With `max_distance_mm` = D a winner needs d^2 <= D^2.  No winner, or a point with a non-finite coordinate:
    triangle -1, closest NaN, distance and sq_distance +inf.  The result depends on the point and the mesh alone -- not on the
    volume's cell size, on N or on the point's place in the batch."""
    what = "closest_points"
    pts = _cloud(what, volume, points)
    d = _max_distance(what, max_distance_mm)
    n = int(pts.shape[0])
    if out is not None and not isinstance(out, ClosestPoints):
        raise MeshDepthError(f"{what}: out must be a ClosestPoints, got {type(out).__name__}")
    res = ClosestPoints(_out(what, "out.triangle", volume, out and out.triangle, (n,), torch.int32),
                        _out(what, "out.closest", volume, out and out.closest, (n, 3), torch.float32),
                        _out(what, "out.distance", volume, out and out.distance, (n,), torch.float32),
                        _out(what, "out.sq_distance", volume, out and out.sq_distance, (n,), torch.float64))
    with torch.cuda.device(volume.device):
        check(lib.gsd_mesh_closest_points(*volume._mesh_args(), pts.data_ptr(), n, d, res.triangle.data_ptr(), res.closest.data_ptr(),
                                          res.distance.data_ptr(), res.sq_distance.data_ptr(), L.stream_ptr()), "mesh_closest_points")
    return res


def _transforms(what: str, volume: MeshVolume, transforms) -> torch.Tensor:
    """(S, 12) fp64 on the volume's device from (4, 4), (S, 4, 4), (12,) or (S, 12): the rows [R | t] of each."""
    t = torch.as_tensor(transforms, dtype=torch.float64).to(volume.device)
    if t.dim() == 2 and tuple(t.shape) == (4, 4):
        t = t.unsqueeze(0)
    if t.dim() == 3 and tuple(t.shape[1:]) == (4, 4) and t.shape[0] >= 1:
        return t[:, :3, :].reshape(-1, 12).contiguous()
    if t.dim() == 1 and t.shape[0] == 12:
        t = t.unsqueeze(0)
    if t.dim() == 2 and t.shape[1] == 12 and t.shape[0] >= 1:
        return t.contiguous()
    raise MeshDepthError(f"{what}: transforms must be (4, 4), (S, 4, 4) or (S, 12), got {tuple(t.shape)}")


def _weights(what: str, volume: MeshVolume, weights, n: int) -> Optional[torch.Tensor]:
    if weights is None:
        return None
    if (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or weights.device != volume.device
            or tuple(weights.shape) != (n,)):
        raise MeshDepthError(f"{what}: weights must be a float32 ({n},) tensor on {volume.device}")
    return weights.contiguous()


def _kind(what: str, kind) -> int:
    if kind not in _KINDS:
        raise MeshDepthError(f"{what}: kind must be 'plane' or 'point', got {kind!r}")
    return _KINDS[kind]


def _rows(volume: MeshVolume, pts: torch.Tensor, t: torch.Tensor, d: float, kind: int, w: Optional[torch.Tensor], out: torch.Tensor,
          ws: torch.Tensor) -> None:
    check(lib.gsd_mesh_icp_rows(*volume._mesh_args(), pts.data_ptr(), w.data_ptr() if w is not None else None, int(pts.shape[0]),
                                t.data_ptr(), int(t.shape[0]), d, kind, out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr()),
          "mesh_icp_rows")


def icp_rows(volume: MeshVolume, points, transforms, max_distance_mm: Optional[float] = None, kind: str = "plane",
             weights: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Normal-equation rows (S, 30) float64 of the cloud `points` (N, 3) moved by each of the S rigid `transforms` ((4, 4),
    (S, 4, 4) or (S, 12) row-major [R | t]) against the mesh: with p' = R p + t in fp64, x its closest point, d^2 their squared
    distance and a point active iff it has a winner within D = `max_distance_mm`,

        [0] sum_active w d^2 + D^2 sum_inactive w   [1] #active   [2] sum_active w r^2   [3..8] sum w J^T r   [9..29] sum w J^T J

    (upper triangle, row-major) for the left twist (v, omega), dp' = v + omega x p'.  kind 'plane': r = n.(p' - x) with n the unit
    facet normal of the winner, J = [n, p' x n]; kind 'point': r = p' - x, J = [I, -[p']x].  Entry 0 is the truncated point
    distance whichever kind.  Points with a non-finite coordinate add nothing.  One libgsd call (gsd_mesh_icp_rows): blocks of 256
    points are summed in a fixed tree and a second launch adds the blocks in ascending order, so a row repeats bitwise and start s
    of a batch equals the same start alone.  `weights` (N,) fp32 must be finite and >= 0; the caller guarantees it, nothing here
    reads them back to check."""
    what = "icp_rows"
    pts = _cloud(what, volume, points)
    t = _transforms(what, volume, transforms)
    d, k = _max_distance(what, max_distance_mm), _kind(what, kind)
    w = _weights(what, volume, weights, int(pts.shape[0]))
    s = int(t.shape[0])
    out = _out(what, "out", volume, out, (s, ICP_ROW), torch.float64)
    words = int(lib.gsd_mesh_icp_rows_workspace(int(pts.shape[0]), s))
    if words < 1:
        raise MeshDepthError(f"{what}: {pts.shape[0]} points x {s} starts are more than one launch takes (2^31 - 1 blocks)")
    with torch.cuda.device(volume.device):
        _rows(volume, pts, t, d, k, w, out, torch.empty((words,), device=volume.device, dtype=torch.float64))
    return out


class CloudRegistration:
    """What `register_cloud` found, all tensors on the device: `matrix` (4, 4) fp64, the best start's rigid motion (cloud -> mesh
    frame); `matrices` (S, 4, 4), `cost` (S,) = row entry 0, `rms` (S,) = sqrt(sum_active d^2 / #active) for unit weights (the
    weighted sum over the count otherwise), `active` (S,), `rows` (S, 30), `trace` (iterations + 1, S), the accepted cost after every
    evaluation, `accepted` (S,) int32, `last_step` (S, 6) fp64 (mm x 3, rad x 3), `best` the winning start's index (0-d int64)."""

    def __init__(self, matrix, matrices, cost, rms, active, rows, trace, accepted, last_step, best) -> None:
        self.matrix, self.matrices, self.cost, self.rms, self.active, self.rows = matrix, matrices, cost, rms, active, rows
        self.trace, self.accepted, self.last_step, self.best = trace, accepted, last_step, best

    def apply(self, points: torch.Tensor) -> torch.Tensor:
        """`points` (N, 3) moved by `matrix`, in fp64 and rounded to the points' dtype."""
        p = points.to(torch.float64)
        return (p @ self.matrix[:3, :3].T + self.matrix[:3, 3]).to(points.dtype)

    def __repr__(self) -> str:
        return f"CloudRegistration({self.matrices.shape[0]} starts, {self.trace.shape[0] - 1} iterations)"


def register_cloud(volume: MeshVolume, points, init=None, iterations: int = 20, max_distance_mm: Optional[float] = None,
                   kind: str = "plane", weights: Optional[torch.Tensor] = None, damping: float = 1e-3, damping_up: float = 10.0,
                   damping_down: float = 0.1, max_step: Sequence[float] = (1.0, 1.0, 1.0, 0.1, 0.1, 0.1)) -> CloudRegistration:
    """Rigid registration of a cloud to the mesh by Levenberg-Marquardt ICP over SE(3).  `init` is None (the
    identity), (4, 4), (S, 4, 4) or (S, 12): every start is refined on its own and the lowest final cost wins under
    `first_argmin`'s rule.  Every iteration is one `icp_rows` evaluation of the trials and one gsd_mesh_icp_lm_update: a trial is
    accepted iff its cost -- the truncated point distance, entry 0, whichever `kind` linearised the step -- is STRICTLY below the
    current one (the damping is then multiplied by `damping_down`, otherwise by `damping_up`); the next trial is exp(xi) T with
    (J^T J + damping diag(J^T J)) xi = -J^T r, clipped per component to `max_step` (mm x 3, rad x 3).  So `trace` never rises, and
    a trial cannot win by losing points.  Nothing is read back from the device (an `init` that is not yet a tensor on the volume's
    device is uploaded).  `weights` must be finite and >= 0: they cannot be checked without a read, and a negative or NaN weight
    breaks the semidefiniteness of J^T J that the step relies on."""
    what = "register_cloud"
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise MeshDepthError(f"{what}: iterations must be an integer >= 0, got {iterations!r}")
    try:
        steps = tuple(float(v) for v in max_step)
        damp = tuple(float(v) for v in (damping, damping_up, damping_down))
    except (TypeError, ValueError):
        steps, damp = (), (float("nan"),) * 3
    if len(steps) != 6 or not all(math.isfinite(v) and v >= 0.0 for v in steps):
        raise MeshDepthError(f"{what}: max_step must be six finite values >= 0 (mm x 3, rad x 3), got {max_step!r}")
    if not (all(math.isfinite(v) for v in damp) and _LAMBDA_MIN <= damp[0] <= _LAMBDA_MAX and damp[1] >= 1.0 and 0.0 < damp[2] <= 1.0):
        raise MeshDepthError(f"{what}: need {_LAMBDA_MIN} <= damping <= {_LAMBDA_MAX}, damping_up >= 1 and 0 < damping_down <= 1, got "
                             f"{damping!r}, {damping_up!r}, {damping_down!r}")
    pts = _cloud(what, volume, points)
    d, k = _max_distance(what, max_distance_mm), _kind(what, kind)
    w = _weights(what, volume, weights, int(pts.shape[0]))
    trial = _transforms(what, volume, torch.eye(4, dtype=torch.float64, device=volume.device) if init is None else init).clone()
    s = int(trial.shape[0])
    words = int(lib.gsd_mesh_icp_rows_workspace(int(pts.shape[0]), s))
    if words < 1:
        raise MeshDepthError(f"{what}: {pts.shape[0]} points x {s} starts are more than one launch takes (2^31 - 1 blocks)")
    lm = L.gsd_icp_lm()
    lm.down, lm.up, lm.lambda_min, lm.lambda_max, lm.reserved = damp[2], damp[1], _LAMBDA_MIN, _LAMBDA_MAX, 0
    lm.max_step[:] = steps
    with torch.cuda.device(volume.device):
        dev = volume.device
        state = torch.empty_like(trial)
        lam = torch.full((s,), damp[0], device=dev, dtype=torch.float64)
        row = torch.empty((s, ICP_ROW), device=dev, dtype=torch.float64)
        trial_row = torch.empty_like(row)
        trace = torch.empty((int(iterations) + 1, s), device=dev, dtype=torch.float64)
        accepted = torch.empty((s,), device=dev, dtype=torch.int32)
        last_step = torch.empty((s, 6), device=dev, dtype=torch.float64)
        ws = torch.empty((words,), device=dev, dtype=torch.float64)
        for it in range(int(iterations) + 1):
            _rows(volume, pts, trial, d, k, w, trial_row, ws)
            lm.first = int(it == 0)
            check(lib.gsd_mesh_icp_lm_update(C.byref(lm), s, state.data_ptr(), lam.data_ptr(), row.data_ptr(), trial.data_ptr(),
                                             trial_row.data_ptr(), trace[it].data_ptr(), accepted.data_ptr(), last_step.data_ptr(),
                                             L.stream_ptr()), "mesh_icp_lm_update")
        cost = row[:, 0]
        best = first_argmin(torch.where(torch.isnan(cost), torch.full_like(cost, float("inf")), cost).unsqueeze(0))[0]
        matrices = torch.zeros((s, 4, 4), device=dev, dtype=torch.float64)
        matrices[:, :3, :] = state.view(s, 3, 4)
        matrices[:, 3, 3] = 1.0
        active = row[:, 1]
        # sum_active w d^2: the cost less the truncation term D^2 * sum_inactive w, which icp_rows folds into entry 0 -- so it is
        # measured again from the point kind's entry 2 only where points can be inactive
        if math.isfinite(d):
            sq = torch.empty_like(row)
            _rows(volume, pts, state, d, 1, w, sq, ws)
            sq = sq[:, 2]
        else:
            sq = cost
        rms = torch.sqrt(sq / active)
        # the winner by index_select: indexing with a 0-d device tensor would read it back
        return CloudRegistration(matrices.index_select(0, best.view(1))[0], matrices, cost, rms, active, row, trace, accepted, last_step, best)


def cloud_mesh_error(volume: MeshVolume, points, max_distance_mm: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """The 3-D error of a cloud against its object, as device scalars (nothing is read back): `mean`, `rms` and `max` of the
    distances [mm] of the points that have a closest point within `max_distance_mm`, and `within`, their number (int64).  Points
    with a non-finite coordinate (a ContactCloud's padding) are ignored; with no point within, mean and rms are NaN and max -inf."""
    res = closest_points(volume, points, max_distance_mm)
    ok = res.triangle >= 0
    n = ok.sum()
    dist = torch.sqrt(res.sq_distance)
    zero = torch.zeros_like(dist)
    count = n.to(torch.float64)
    return {"mean": torch.where(ok, dist, zero).sum() / count, "rms": torch.sqrt(torch.where(ok, res.sq_distance, zero).sum() / count),
            "max": torch.where(ok, dist, torch.full_like(dist, float("-inf"))).max(), "within": n}
