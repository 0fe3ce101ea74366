"""Ground-truth depth images from an object's mesh, the recorded in-hand poses and the grasp widths, on the device: the label
maker of the reference (gelslim_depth/mesh_utils/depth_from_mesh.py, driven by scripts/data_scripts/depth_generation.py),
restated exactly instead of sampled.

The reference draws 1e5 random surface points with open3d and runs two scipy Delaunay interpolations per sample.  Here a pixel's
depth is DEFINED by the mesh: the outermost surface under the pixel, `right = -max(0, Qmax - g/2)`,
`left = min(0, Qmin + g/2)`, 0 where no triangle covers it.  libgsd (gsd_mesh_depth_*, include/gsd.h) builds a cell grid over
the mesh once (`MeshGrid`) and renders any number of poses with one launch per batch (`render_depth`); neither open3d nor scipy
is needed, the result does not depend on a random cloud, and it never interpolates across surface layers.

`DepthImageGenerator` keeps the reference's constructor and `generate_depth_images_v1`, so a data-generation script switches by
changing its import."""
from __future__ import annotations

import ctypes as C
import math
import os
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib


class MeshDepthError(L.GsdError, ValueError):
    """What this module refuses: the package's error, and a ValueError where the definition names one (a negative width)."""


# ---- STL ------------------------------------------------------------------------------------------------------------
def _read_stl_ascii(text: str, path: str) -> np.ndarray:
    verts: List[Tuple[float, float, float]] = []
    facets = 0
    for line in text.splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "vertex":
            if len(tok) != 4:
                raise MeshDepthError(f"read_stl: {path}: malformed vertex line {line.strip()!r}")
            try:
                verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
            except ValueError:
                raise MeshDepthError(f"read_stl: {path}: malformed vertex line {line.strip()!r}") from None
        elif tok[0] == "endfacet":
            facets += 1
            if len(verts) != 3 * facets:
                raise MeshDepthError(f"read_stl: {path}: facet {facets} has {len(verts) - 3 * (facets - 1)} vertices, not 3")
    if len(verts) != 3 * facets or "endsolid" not in text:
        raise MeshDepthError(f"read_stl: {path}: truncated ASCII STL ({len(verts)} vertices in {facets} closed facets, "
                             f"{'no ' if 'endsolid' not in text else ''}endsolid)")
    return np.asarray(verts, dtype=np.float32).reshape(-1, 3, 3)


def read_stl(path: str) -> np.ndarray:
    """The triangles of a binary or an ASCII STL file as float32 (T, 3, 3) (triangle, vertex, xyz); normals and attribute
    words are ignored.  numpy only.  A binary file is 80 header bytes, a uint32 count T and T records of 50 bytes: a file
    shorter than 84 bytes, or whose size is not 84 + 50 T, is refused, as is an ASCII file without its `endsolid`."""
    with open(path, "rb") as fh:
        raw = fh.read()
    ascii_form = raw[:512].lstrip().startswith(b"solid")
    if ascii_form and len(raw) >= 84 and len(raw) == 84 + 50 * struct.unpack_from("<I", raw, 80)[0]:
        ascii_form = False      # a binary file whose header happens to start with "solid"
    if ascii_form:
        try:
            return _read_stl_ascii(raw.decode("ascii"), path)
        except UnicodeDecodeError:
            pass            # binary after all: the size check below says what is wrong with it
    if len(raw) < 84:
        raise MeshDepthError(f"read_stl: {path}: {len(raw)} bytes, a binary STL has at least 84 (truncated file)")
    (count,) = struct.unpack_from("<I", raw, 80)
    if len(raw) != 84 + 50 * count:
        raise MeshDepthError(f"read_stl: {path}: header announces {count} triangles = {84 + 50 * count} bytes, the file has "
                             f"{len(raw)} (truncated, or not an STL file)")
    rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=count, offset=84)
    return np.ascontiguousarray(rec["v"], dtype=np.float32)


# ---- conventions (depth_from_mesh.py:85-146) ------------------------------------------------------------------------
def plane_convention(gelslim_plane: str) -> Tuple[int, int, int, int]:
    """(perp_ind, aligned_index, unaligned_index, multiplier) of a `gelslim_plane` string such as '+y+z' (the plane of the
    RIGHT finger's image): the first letter names the unaligned axis (image rows), the second the aligned one (columns), the
    remaining axis is perpendicular, and the right finger looks along multiplier * that axis with
    multiplier = sign1 * sign2 * (+1 if first x second = +perp else -1) -- the reference's twelve-row table in one rule."""
    if not isinstance(gelslim_plane, str):
        raise ValueError("Invalid gelslim_plane")
    axes = [c for c in gelslim_plane if c.isalpha()]
    signs = [c for c in gelslim_plane if c in "+-"]
    pair = next((p for p in ("xy", "xz", "yz") if p[0] in axes and p[1] in axes), None)
    if pair is None or len(signs) < 2 or not axes or axes[0] not in pair:
        raise ValueError("Invalid gelslim_plane")
    first = "xyz".index(axes[0])
    second = "xyz".index(pair[1] if axes[0] == pair[0] else pair[0])
    perp = 3 - first - second
    cyclic = 1 if (second - first) % 3 == 1 else -1          # first x second = cyclic * perp
    same = 1 if signs[0] == signs[1] else -1
    return perp, second, first, same * cyclic


def dataset_key(pt_file: str) -> str:
    """The object a dataset file belongs to (depth_from_mesh.py:51-54, 62-65): `<...>_<object>_{train,val,test}.pt` names it in
    the field before the last underscore, any other name in what precedes the first dot.  The mesh is `<key>.stl`."""
    if "_val" in pt_file or "_test" in pt_file or "_train" in pt_file:
        return pt_file.split("_")[-2]
    return pt_file.split(".")[0]


def select_dataset_files(names: Sequence[str], object_list: Optional[Sequence[str]]) -> List[str]:
    """The `.pt` files among `names` that generate_depth_images_v1 works on (depth_from_mesh.py:26-33): all of them without
    an object list; with one, the name rule is chosen by the FIRST file, as the reference does."""
    files = [f for f in names if f[-3:] == ".pt"]
    if object_list is not None and files:
        first = files[0]
        if "_val" in first or "_test" in first or "_train" in first:
            files = [f for f in files if f.split("_")[-2] in object_list]
        else:
            files = [f for f in files if f.split(".")[0] in object_list]
    return files


def parse_grasp_widths(lines: Sequence[str]) -> Dict[str, Optional[float]]:
    """`object: inter_gelslim_distance` lines (depth_from_mesh.py:38-46): a float, or ` None` for "use the sample's own
    grasp_widths entry"."""
    out: Dict[str, Optional[float]] = {}
    for line in lines:
        part = line.split(":")
        out[part[0]] = None if part[1] in (" None\n", " None") else float(part[1])
    return out


# ---- the mesh on the device -----------------------------------------------------------------------------------------
def _need_cuda(device) -> torch.device:
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise MeshDepthError(f"mesh_depth: the rasteriser runs on the GPU, got device {dev}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def default_cell_mm(a: np.ndarray, b: np.ndarray, target: float = 8.0) -> float:
    """Cell size model.  A triangle whose in-plane bounding box is w x h lands in about (w/c + 1)(h/c + 1) cells of side c,
    the grid has about A / c^2 cells over the mesh's bounding box of area A, so with s^2 the triangles' mean bounding-box
    area the mean list length is T (c + s)^2 / A.  Solving for `target` = 8 entries (two trips of the render's four-entry walk;
    the measured optimum on the 81,920-triangle sphere) gives c = sqrt(target A / T) - s; it is kept above
    s / 2 (finer cells mostly multiply the entries of the triangles; 8.9 entries per cell on that sphere) and above 1/512 of the
    extent."""
    ext_a, ext_b = float(a.max() - a.min()), float(b.max() - b.min())
    ext = max(ext_a, ext_b, 1e-30)
    area = max(ext_a, 1e-3 * ext) * max(ext_b, 1e-3 * ext)
    w = a.max(axis=1) - a.min(axis=1)
    h = b.max(axis=1) - b.min(axis=1)
    s = math.sqrt(max(float(np.mean(w * h)), 0.0))
    return max(math.sqrt(target * area / a.shape[0]) - s, 0.5 * s, ext / 512.0)


def _build_cell_lists(owner: str, entry: str, device, words: int, count, fill):
    """The workspace-to-list tail of MeshGrid and MeshVolume: allocate the `words` int32 of cells, count(cells, words, stream),
    read the int64 total of (cell, triangle) pairs back (the one host read of a mesh), allocate the list and
    fill(cells, words, list, entries, stream).  Returns (cells, pairs, list); with no pair (every triangle is skipped) the list is
    one zero and nothing is filled."""
    cells = torch.empty((words,), device=device, dtype=torch.int32)
    check(count(cells.data_ptr(), words, L.stream_ptr()), f"{entry}_count")
    pairs = int(cells[:2].view(torch.int64).item())
    if pairs >= 1 << 31:
        raise MeshDepthError(f"{owner}: {pairs} (cell, triangle) pairs, at most 2^31 - 1: use larger cells")
    if pairs == 0:
        return cells, pairs, torch.zeros((1,), device=device, dtype=torch.int32)
    lst = torch.empty((pairs,), device=device, dtype=torch.int32)
    check(fill(cells.data_ptr(), words, lst.data_ptr(), lst.numel(), L.stream_ptr()), f"{entry}_fill")
    return cells, pairs, lst


class MeshGrid:
    """A mesh prepared for `render_depth`: the per-triangle records and the per-cell triangle lists on the device, built once.

    triangles: (T, 3, 3) array or tensor (`read_stl`); pc_scale: factor to millimetres (the reference's `pc_scale`);
    gelslim_plane: `plane_convention`; cell_mm: side of a grid cell, default `default_cell_mm`; the environment variable
    GSD_MESH_CELL_MM overrides both.  The image does not depend on the cell size, only the time does.
    Building reads one int64 back from the device (the number of (cell, triangle) pairs, to allocate the list)."""

    def __init__(self, triangles, pc_scale: float = 1.0, gelslim_plane: str = "+y+z", device=None, cell_mm: Optional[float] = None) -> None:
        self.perp_ind, self.aligned_index, self.unaligned_index, self.multiplier = plane_convention(gelslim_plane)
        self.gelslim_plane = gelslim_plane
        self.device = _need_cuda(device)
        if isinstance(triangles, torch.Tensor):
            triangles = triangles.detach().cpu().numpy()
        v = np.asarray(triangles, dtype=np.float64)
        if v.ndim != 3 or v.shape[1:] != (3, 3):
            raise MeshDepthError(f"MeshGrid: triangles must be (T, 3, 3), got {v.shape}")
        if v.shape[0] == 0:
            raise MeshDepthError("MeshGrid: the mesh has no triangles")
        if v.shape[0] > 1 << 24:
            raise MeshDepthError(f"MeshGrid: {v.shape[0]} triangles, at most 2^24")
        scale = float(pc_scale)
        if not math.isfinite(scale) or scale == 0.0:
            raise MeshDepthError(f"MeshGrid: pc_scale must be finite and not zero, got {pc_scale!r}")
        v = v * scale
        if not np.isfinite(v).all():
            raise MeshDepthError("MeshGrid: the mesh has a non-finite vertex")
        perp = v[:, :, self.perp_ind]
        self.mid = 0.5 * (float(perp.max()) + float(perp.min()))
        q = self.multiplier * (perp - self.mid)
        lo, hi = sorted((self.aligned_index, self.unaligned_index))
        a, b = v[:, :, lo], v[:, :, hi]
        self.swap_axes = 1 if self.aligned_index < self.unaligned_index else 0
        env = os.environ.get("GSD_MESH_CELL_MM")
        if env is not None:
            cell = float(env)
        elif cell_mm is not None:
            cell = float(cell_mm)
        else:
            cell = default_cell_mm(a, b)
        if not (math.isfinite(cell) and cell > 0.0):
            raise MeshDepthError(f"MeshGrid: cell_mm must be finite and positive, got {cell!r}")
        self.grid = L.gsd_mesh_grid()
        bbox = (C.c_double * 4)(float(a.min()), float(b.min()), float(a.max()), float(b.max()))
        check(lib.gsd_mesh_depth_plan(bbox, cell, C.byref(self.grid)), "mesh_depth_plan")
        self.cell_mm = float(self.grid.cell)
        self.triangles = int(v.shape[0])
        self.q_range = (float(q.min()), float(q.max()))
        # prepared vertices (a, b, q), relative to the fp32 centre the kernel adds back, rounded to fp32 once
        tri = np.stack((a - float(self.grid.cx), b - float(self.grid.cy), q), axis=2).astype(np.float32)
        # the largest |coordinate| of the mesh in the frame the pixel-to-mesh map works in (for error budgets)
        self.coord_max = float(max(np.abs(a).max(), np.abs(b).max()))
        with torch.cuda.device(self.device):
            self._tri = torch.from_numpy(tri.reshape(-1, 9)).to(self.device)
            self.records = torch.empty((self.triangles, L.GSD_MESH_RECORD_FLOATS), device=self.device, dtype=torch.float32)
            grid, rec, n = C.byref(self.grid), self.records.data_ptr(), self.triangles
            self.cells, self.pairs, self.list = _build_cell_lists(
                "MeshGrid", "mesh_depth", self.device, int(lib.gsd_mesh_depth_workspace(grid)),
                lambda *ws: lib.gsd_mesh_depth_count(grid, self._tri.data_ptr(), n, rec, *ws),
                lambda *ws: lib.gsd_mesh_depth_fill(grid, rec, n, *ws))
            del self._tri

    @property
    def shape(self) -> Tuple[int, int]:
        """(ny, nx) cells."""
        return int(self.grid.ny), int(self.grid.nx)

    def __repr__(self) -> str:
        return (f"MeshGrid({self.triangles} triangles, plane {self.gelslim_plane!r}, {self.grid.nx} x {self.grid.ny} cells of "
                f"{self.cell_mm:.4g} mm, {self.pairs} pairs)")


def _check_tensors(what: str, grid, tensors, contiguous: bool = False) -> None:
    """`grid` is a MeshGrid and every (name, tensor, shape as text) of `tensors` a float32 tensor on its device."""
    if not isinstance(grid, MeshGrid):
        raise MeshDepthError(f"{what}: grid must be a MeshGrid, got {type(grid).__name__}")
    for name, t, shape in tensors:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or (contiguous and not t.is_contiguous()):
            raise MeshDepthError(f"{what}: {name} must be a {'contiguous ' if contiguous else ''}float32 {shape} tensor on the GPU, got "
                                 f"{getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', 'the host')}")
        if t.device != grid.device:
            raise MeshDepthError(f"{what}: {name} is on {t.device}, the mesh on {grid.device}")


def _check_widths(what: str, widths: torch.Tensor, offset: float) -> None:
    """`validate=True`: the smallest width + offset is read back from the device, the call's only synchronisation."""
    g_min = float((widths + offset).min())          # NaN propagates through min
    if not (g_min >= 0.0) or not bool(torch.isfinite(widths).all()):
        raise MeshDepthError(f"{what}: grasp width + offset must be finite and >= 0, the smallest is {g_min!r}")


def _mesh_view(grid: MeshGrid, mpp: float, offset: float, LR_flip: bool, invert_affine: bool) -> "L.gsd_mesh_view":
    view = L.gsd_mesh_view()
    view.mpp, view.width_offset = mpp, offset
    view.swap_axes, view.invert_affine, view.lr_flip, view.reserved = grid.swap_axes, int(bool(invert_affine)), int(bool(LR_flip)), 0
    return view


def _out_tensor(what: str, grid: MeshGrid, out: Optional[torch.Tensor], shape: Tuple[int, ...], dtype: torch.dtype) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, device=grid.device, dtype=dtype)
    if (not isinstance(out, torch.Tensor) or out.dtype != dtype or out.device != grid.device or not out.is_contiguous()
            or tuple(out.shape) != shape):
        raise MeshDepthError(f"{what}: out must be a contiguous {str(dtype)[6:]} {shape} tensor on {grid.device}")
    return out


def render_depth(grid: MeshGrid, poses: torch.Tensor, grasp_widths: torch.Tensor, image_size: Sequence[int] = (320, 427),
                 image_height_mm: float = 12.0, grasp_width_offset: float = 0.0, LR_flip: bool = False,
                 invert_affine: bool = False, out: Optional[torch.Tensor] = None, validate: bool = True) -> torch.Tensor:
    """Depth images (N, 2, H, W) fp32 in mm, channels (left, right), or (right, left) with `LR_flip`, of `grid`'s mesh under
    the N poses `poses` (N, 3) = (t1 [m], t2 [m], theta [rad]) with the inter-finger distances `grasp_widths` (N,) [mm]; both
    are float32 tensors on the grid's device.  One libgsd call, on torch's current stream; `out` is written in place.

    g = grasp_widths + grasp_width_offset must not be negative.  With `validate` (the default) the smallest g is read back
    from the device and a negative or non-finite one raises MeshDepthError (a ValueError) before anything of libgsd runs: this
    is the call's only synchronisation.  `validate=False` promises that the caller has checked (generate_depth_images_v1
    checks the whole file on the host): then nothing is synchronised, and a sample with a bad g comes out as NaN."""
    return _render("render_depth", False, grid, poses, grasp_widths, image_size, image_height_mm, grasp_width_offset, LR_flip, invert_affine,
                   out, validate)


def _render(what: str, jacobian: bool, grid, poses, grasp_widths, image_size, image_height_mm, grasp_width_offset, LR_flip, invert_affine,
            out, validate) -> torch.Tensor:
    """`render_depth` ((N, 2, H, W) fp32, gsd_mesh_depth_render) and, with `jacobian`, `render_depth_jacobian` ((N, 2, 3, H, W)
    fp64, gsd_mesh_depth_render_jacobian): the same checks, view, workspace and call."""
    _check_tensors(what, grid, (("poses", poses, "(N, 3)"), ("grasp_widths", grasp_widths, "(N,)")), contiguous=True)
    if poses.dim() != 2 or poses.shape[1] != 3 or poses.shape[0] < 1:
        raise MeshDepthError(f"{what}: poses must be (N, 3) with N >= 1, got {tuple(poses.shape)}")
    n = int(poses.shape[0])
    if tuple(grasp_widths.shape) != (n,):
        raise MeshDepthError(f"{what}: {n} poses but grasp_widths of shape {tuple(grasp_widths.shape)}")
    h, w = (int(d) for d in image_size)
    mpp = float(image_height_mm) / h if h > 0 else float("nan")
    if h < 1 or w < 1 or not (math.isfinite(mpp) and mpp > 0.0):
        raise MeshDepthError(f"{what}: image_size {tuple(image_size)} and image_height_mm {image_height_mm!r} must be positive")
    offset = float(grasp_width_offset)
    if not math.isfinite(offset):
        raise MeshDepthError(f"{what}: grasp_width_offset must be finite, got {grasp_width_offset!r}")
    out = _out_tensor(what, grid, out, (n, 2, 3, h, w) if jacobian else (n, 2, h, w), torch.float64 if jacobian else torch.float32)
    if validate:
        _check_widths(what, grasp_widths, offset)
    view = _mesh_view(grid, mpp, offset, LR_flip, invert_affine)
    entry = "gsd_mesh_depth_render_jacobian" if jacobian else "gsd_mesh_depth_render"
    with torch.cuda.device(grid.device):
        ws = torch.empty((int(lib.gsd_mesh_depth_render_workspace(n)),), device=grid.device, dtype=torch.float32)
        check(getattr(lib, entry)(C.byref(grid.grid), C.byref(view), grid.records.data_ptr(), grid.triangles,
                                  grid.cells.data_ptr(), grid.list.data_ptr(), grid.list.numel(), poses.data_ptr(),
                                  grasp_widths.data_ptr(), n, h, w, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                  L.stream_ptr()), entry[4:])
    return out


def render_depth_jacobian(grid: MeshGrid, poses: torch.Tensor, grasp_widths: torch.Tensor, image_size: Sequence[int] = (320, 427),
                          image_height_mm: float = 12.0, grasp_width_offset: float = 0.0, LR_flip: bool = False,
                          invert_affine: bool = False, out: Optional[torch.Tensor] = None, validate: bool = True) -> torch.Tensor:
    """(N, 2, 3, H, W) float64: the derivatives of every pixel of `render_depth`'s images with respect to a1 = 1000 t1 [mm],
    a2 = 1000 t2 [mm] and theta [rad] -- the terms that `pose_normal_rows` sums, written out for
    inspection.  0 where the pixel's depth is 0.  The arguments are `render_depth`'s."""
    return _render("render_depth_jacobian", True, grid, poses, grasp_widths, image_size, image_height_mm, grasp_width_offset, LR_flip,
                   invert_affine, out, validate)


# ---- the reference's class ------------------------------------------------------------------------------------------
class DepthImageGenerator:
    """Drop-in for gelslim_depth.mesh_utils.depth_from_mesh.DepthImageGenerator: the same constructor arguments and defaults,
    except that `device` defaults to the GPU (the rasteriser has no CPU form) and that `pc_sampling` is accepted and unused --
    nothing is sampled, the depth comes from the triangles themselves.  `batch` samples are rendered per launch."""

    def __init__(self, mesh_dir, object_list, pc_scale, dataset_dir, grasp_widths_file, gelslim_plane="+y+z", LR_flip=False,
                 image_size=(320, 427), image_height_mm=12, grasp_width_offset=0.0, pc_sampling=1e5, device="cuda",
                 batch: int = 256) -> None:
        self.image_height_mm = image_height_mm
        self.image_size = tuple(int(d) for d in image_size)
        self.mm_per_pixel = image_height_mm / image_size[0]
        self.mesh_dir = mesh_dir
        self.grasp_widths_file = grasp_widths_file
        self.gelslim_plane = gelslim_plane
        self.LR_flip = LR_flip
        self.pc_scale = pc_scale
        self.dataset_dir = dataset_dir
        self.object_list = object_list
        self.plane_axes = [c for c in self.gelslim_plane if c.isalpha()]
        self.pc_sampling = pc_sampling          # unused
        self.device = _need_cuda(device)
        self.grasp_width_offset = grasp_width_offset
        self.batch = int(batch)
        plane_convention(gelslim_plane)         # an invalid plane raises here, not at the first sample
        self._grids: Dict[str, MeshGrid] = {}

    def mesh_grid(self, mesh) -> MeshGrid:
        """`mesh` as a MeshGrid: one is passed through, a path is read with `read_stl` (and kept), triangles are prepared with
        this generator's pc_scale and plane."""
        if isinstance(mesh, MeshGrid):
            return mesh
        if isinstance(mesh, (str, os.PathLike)):
            key = os.fspath(mesh)
            if key not in self._grids:
                self._grids[key] = MeshGrid(read_stl(key), self.pc_scale, self.gelslim_plane, self.device)
            return self._grids[key]
        return MeshGrid(mesh, self.pc_scale, self.gelslim_plane, self.device)

    def generate_depth_image(self, mesh, translation1, translation2, angle, inter_gelslim_distance, invert_affine=False):
        """(right, left) depth images (H, W) on the device for one pose.  `mesh` is a MeshGrid, an STL path or (T, 3, 3)
        triangles in mesh units -- where the reference takes its scaled point cloud.  As there, `inter_gelslim_distance`
        is used as given (generate_depth_images_v1 adds grasp_width_offset before it calls)."""
        grid = self.mesh_grid(mesh)
        g = float(inter_gelslim_distance)
        if not (g >= 0.0 and math.isfinite(g)):
            raise MeshDepthError(f"generate_depth_image: inter_gelslim_distance must be finite and >= 0, got {g!r}")
        pose = torch.tensor([[float(translation1), float(translation2), float(angle)]], dtype=torch.float32, device=grid.device)
        width = torch.tensor([g], dtype=torch.float32, device=grid.device)
        img = render_depth(grid, pose, width, self.image_size, self.image_height_mm, 0.0, False, invert_affine, validate=False)
        return img[0, 1], img[0, 0]

    def generate_depth_images_v1(self, prompt: bool = True) -> None:
        """depth_from_mesh.py:25-78: for every selected `.pt` file of dataset_dir, render the `depth_image` of all its samples
        from `<object>.stl`, its `in_hand_pose` rows and the grasp widths (the file's number, or the samples' own
        `grasp_widths` where the file says None), and write the file back -- through train.atomic_save, so a kill leaves the
        old file.  The tensors are loaded to and saved from the host, as DeviceDataset reads them.  `prompt=False` skips the
        reference's input()."""
        from .train import atomic_save
        dataset_list = select_dataset_files(os.listdir(self.dataset_dir), self.object_list)
        if prompt:
            user_in = input("Generating depth images for " + str(dataset_list) + ", Press enter to continue or q to quit.")
            if user_in == "q":
                return
        with open(self.grasp_widths_file, "r") as f:
            grasp_widths = parse_grasp_widths(f.readlines())
        h, w = self.image_size
        for pt_file in dataset_list:
            path = os.path.join(self.dataset_dir, pt_file)
            dataset_pt = torch.load(path, map_location="cpu")
            n = int(dataset_pt["tactile_image"].shape[0])
            key = dataset_key(pt_file)
            grid = self.mesh_grid(os.path.join(self.mesh_dir, key + ".stl"))
            poses = dataset_pt["in_hand_pose"][:n, :3].to(torch.float32).contiguous()
            distance = grasp_widths[key]
            if distance is None:
                widths = dataset_pt["grasp_widths"].reshape(-1)[:n].to(torch.float32).contiguous()
            else:
                widths = torch.full((n,), float(distance), dtype=torch.float32)
            if poses.shape[0] != n or widths.shape[0] != n:
                raise MeshDepthError(f"{pt_file}: {n} samples but {poses.shape[0]} poses and {widths.shape[0]} grasp widths")
            g = widths + float(self.grasp_width_offset)
            if n and not bool((torch.isfinite(g) & (g >= 0)).all()):          # on the host: the batches below never synchronise
                bad = int((~(torch.isfinite(g) & (g >= 0))).nonzero()[0])
                raise MeshDepthError(f"{pt_file}: sample {bad}: grasp width + offset = {float(g[bad])!r} must be finite and >= 0")
            depth = torch.zeros((n, 2, h, w), dtype=torch.float32)
            poses_d, widths_d = poses.to(self.device), widths.to(self.device)
            for i in range(0, n, max(self.batch, 1)):
                j = min(i + max(self.batch, 1), n)
                img = render_depth(grid, poses_d[i:j], widths_d[i:j], self.image_size, self.image_height_mm,
                                   self.grasp_width_offset, self.LR_flip, False, validate=False)
                depth[i:j] = img.cpu()
            dataset_pt["depth_image"] = depth
            atomic_save(dataset_pt, path)


# ---- in-hand pose from a depth image ----------------------------------------------------------
POSE_ROW = L.GSD_POSE_ROW      # columns of a score row: sum_sq, sum_abs, inter, n_rendered, n_observed


def lattice_points(image_size: Sequence[int], stride: int = 1) -> int:
    """Points that a row of `score_poses` sums over: both channels of the pixel lattice r = stride // 2 + i * stride < H,
    c = stride // 2 + j * stride < W.  What `pose_cost` divides by."""
    h, w = (int(d) for d in image_size)
    s = int(stride)
    if h < 1 or w < 1 or s < 1:
        raise MeshDepthError(f"lattice_points: image_size {tuple(image_size)} and stride {stride!r} must be positive")
    return 2 * len(range(s // 2, h, s)) * len(range(s // 2, w, s))


POSE_WIDTHS_MAX = L.GSD_POSE_WIDTHS_MAX      # widths per observation that one `score_poses_widths` call takes
NORMAL_ROW = L.GSD_POSE_NORMAL_ROW      # columns of a normal row: sum e^2, #active, J^T e (a1, a2, theta, g), upper triangle of J^T J


def _score(what: str, many: bool, grid, observed, candidates, widths, image_height_mm, grasp_width_offset, LR_flip, invert_affine,
           stride, contact_depth, out, validate, normal: bool = False) -> torch.Tensor:
    """`score_poses` (`widths` (B,), rows (B, P, 5), gsd_mesh_pose_score), with `many` `score_poses_widths` (`widths` (B, G),
    rows (B, P, G, 5), gsd_mesh_pose_score_widths) and with `normal` `pose_normal_rows` (`widths` (B,) or (B, P), rows (B, P, 16),
    gsd_mesh_pose_normal): the same checks, view and call, `what` the public name for the messages."""
    _check_tensors(what, grid, (("observed", observed, "(B, 2, H, W)"), ("candidates", candidates, "(B, P, 3) or (P, 3)"),
                                ("widths" if many or normal else "grasp_widths", widths,
                                 "(B, G)" if many else "(B,) or (B, P)" if normal else "(B,)")))
    if observed.dim() != 4 or observed.shape[1] != 2 or min(observed.shape) < 1:
        raise MeshDepthError(f"{what}: observed must be (B, 2, H, W) with B, H, W >= 1, got {tuple(observed.shape)}")
    b, _, h, w = (int(d) for d in observed.shape)
    if candidates.dim() == 2:
        candidates = candidates.unsqueeze(0).expand(b, -1, -1)
    if candidates.dim() != 3 or candidates.shape[0] != b or candidates.shape[2] != 3 or candidates.shape[1] < 1:
        raise MeshDepthError(f"{what}: candidates must be ({b}, P, 3) or (P, 3) with P >= 1, got {tuple(candidates.shape)}")
    p = int(candidates.shape[1])
    if many:
        if widths.dim() != 2 or widths.shape[0] != b or not 1 <= widths.shape[1] <= POSE_WIDTHS_MAX:
            raise MeshDepthError(f"{what}: widths must be ({b}, G) with 1 <= G <= {POSE_WIDTHS_MAX}, got {tuple(widths.shape)}")
    elif normal:
        if tuple(widths.shape) not in ((b,), (b, p)):
            raise MeshDepthError(f"{what}: widths must be ({b},) or ({b}, {p}), one per observation or per candidate, got {tuple(widths.shape)}")
        widths = widths.reshape(b, -1).expand(b, p)
    elif tuple(widths.shape) != (b,):
        raise MeshDepthError(f"{what}: {b} observations but grasp_widths of shape {tuple(widths.shape)}")
    g = tuple(int(d) for d in widths.shape[1:]) if not normal else ()          # (G,) or (): where G stands in the shapes and in the argument lists
    observed, candidates, widths = observed.contiguous(), candidates.contiguous(), widths.contiguous()
    mpp = float(image_height_mm) / h
    if not (math.isfinite(mpp) and mpp > 0.0):
        raise MeshDepthError(f"{what}: image_height_mm {image_height_mm!r} must be finite and positive")
    offset = float(grasp_width_offset)
    if not math.isfinite(offset):
        raise MeshDepthError(f"{what}: grasp_width_offset must be finite, got {grasp_width_offset!r}")
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1:
        raise MeshDepthError(f"{what}: stride must be an integer >= 1, got {stride!r}")
    depth = float(contact_depth)
    if not (math.isfinite(depth) and depth >= 0.0):
        raise MeshDepthError(f"{what}: contact_depth must be finite and >= 0, got {contact_depth!r}")
    out = _out_tensor(what, grid, out, (b, p) + g + (NORMAL_ROW if normal else POSE_ROW,), torch.float64)
    entry = "gsd_mesh_pose_score_widths" if many else "gsd_mesh_pose_normal" if normal else "gsd_mesh_pose_score"          # from the module's `lib`, at every call
    tail = () if normal else (depth,)          # the normal rows take no contact depth
    words = int(getattr(lib, entry + "_workspace")(b, p, *g, h, w, int(stride)))
    if words < 1:
        raise MeshDepthError(f"{what}: {b} x {p} candidates{f' x {g[0]} widths' if many else ''} of {h} x {w} at stride {stride} are "
                             "more than one launch takes (2^31 - 1 blocks or rows): score them in parts")
    if validate:
        _check_widths(what, widths, offset)
    view = _mesh_view(grid, mpp, offset, LR_flip, invert_affine)
    with torch.cuda.device(grid.device):
        ws = torch.empty((words,), device=grid.device, dtype=torch.float64)
        check(getattr(lib, entry)(C.byref(grid.grid), C.byref(view), grid.records.data_ptr(), grid.triangles, grid.cells.data_ptr(),
                                  grid.list.data_ptr(), grid.list.numel(), observed.data_ptr(), b, candidates.data_ptr(),
                                  widths.data_ptr(), p, *g, h, w, int(stride), *tail, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                  L.stream_ptr()), entry[4:])
    return out


def score_poses(grid: MeshGrid, observed: torch.Tensor, candidates: torch.Tensor, grasp_widths: torch.Tensor,
                image_height_mm: float = 12.0, grasp_width_offset: float = 0.0, LR_flip: bool = False, invert_affine: bool = False,
                stride: int = 1, contact_depth: float = 0.0, out: Optional[torch.Tensor] = None, validate: bool = True) -> torch.Tensor:
    """Rows (B, P, 5) float64 that compare the depth images `observed` (B, 2, H, W) fp32 in mm, channels as `render_depth`'s
    (with the same `LR_flip`), with the renders of `grid`'s mesh under the candidate poses `candidates` (B, P, 3) = (t1 [m],
    t2 [m], theta [rad]) -- a (P, 3) tensor serves every observation -- at the widths `grasp_widths` (B,) [mm]:

        sum_sq = sum e^2, sum_abs = sum |e|, inter = #{R < -c and D < -c}, n_rendered = #{R < -c}, n_observed = #{D < -c}

    R the depth `render_depth` gives for that candidate and pixel (the same bits), D the observed one, e = R - D in fp64,
    c = `contact_depth` >= 0, summed over both channels and the pixels r = stride // 2 + i * stride, c = stride // 2 + j * stride
    of the full image (a stride thins the lattice and does not resample).  No image is written: one libgsd call
    (gsd_mesh_pose_score) renders and compares in registers, on torch's current stream.  A row depends on its own observation,
    candidate, stride and image alone, not on B, P or its position, and a repeated call gives the same bits.

    A non-finite D on the lattice makes that row's two sums non-finite and is not contact; off the lattice it changes nothing.
    `validate` is `render_depth`'s: by default the smallest grasp width + offset is read back (the call's only synchronisation)
    and a negative or non-finite one raises MeshDepthError; with `validate=False` nothing is synchronised and such an
    observation's rows are five NaN each."""
    return _score("score_poses", False, grid, observed, candidates, grasp_widths, image_height_mm, grasp_width_offset, LR_flip,
                  invert_affine, stride, contact_depth, out, validate)


def score_poses_widths(grid: MeshGrid, observed: torch.Tensor, candidates: torch.Tensor, widths: torch.Tensor,
                       image_height_mm: float = 12.0, grasp_width_offset: float = 0.0, LR_flip: bool = False,
                       invert_affine: bool = False, stride: int = 1, contact_depth: float = 0.0, out: Optional[torch.Tensor] = None,
                       validate: bool = True) -> torch.Tensor:
    """`score_poses` for G grasp widths per observation at the price of one render per candidate: rows
    (B, P, G, 5) float64 with rows[b, p, k] THE SAME BITS as score_poses(...)[b, p] at the width widths[b, k] -- `widths` is a
    (B, G) float32 tensor on the device, 1 <= G <= POSE_WIDTHS_MAX.  The width enters a pixel's depth in its last step only,
    d = -max(0, m - g/2), so one libgsd call (gsd_mesh_pose_score_widths) finds every lattice point's surface value m once and
    reduces G rows from it.  Every other argument is `score_poses`'.

    `validate=True` reads the smallest width + offset back once and raises MeshDepthError for a negative or non-finite one;
    `validate=False` reads nothing, and such a (b, :, k) column is five NaN per row (+inf for `pose_cost`)."""
    return _score("score_poses_widths", True, grid, observed, candidates, widths, image_height_mm, grasp_width_offset, LR_flip,
                  invert_affine, stride, contact_depth, out, validate)


def pose_normal_rows(grid: MeshGrid, observed: torch.Tensor, candidates: torch.Tensor, widths: torch.Tensor,
                     image_height_mm: float = 12.0, grasp_width_offset: float = 0.0, LR_flip: bool = False, invert_affine: bool = False,
                     stride: int = 1, out: Optional[torch.Tensor] = None, validate: bool = True) -> torch.Tensor:
    """Normal-equation rows (B, P, 16) float64 of the squared error that `score_poses` sums: per candidate

        [0] sum e^2   [1] #active   [2..5] sum J_k e   [6..15] sum J_j J_k, j <= k, row-major   (k over a1, a2, theta, g)

    with J the derivatives of the rendered depth with respect to a1 = 1000 t1 [mm], a2 = 1000 t2 [mm], theta [rad] and the grasp
    width g [mm] -- of the triangle that gives the pixel its depth; 0 where the depth is 0 --, over `score_poses`' lattice, in one
    libgsd call (gsd_mesh_pose_normal) at about the price of a score: the walk over the triangles is the same.  Entry 0 is
    `score_poses`' sum_sq of that candidate, width and stride BIT FOR BIT, entry 1 its n_rendered at contact_depth 0.

    `widths` is (B,) as `score_poses`' or (B, P), one per candidate; the other arguments and `validate` are `score_poses`'.  With
    `validate=False` a candidate whose width + offset is negative or not finite gets 16 NaN."""
    return _score("pose_normal_rows", False, grid, observed, candidates, widths, image_height_mm, grasp_width_offset, LR_flip,
                  invert_affine, stride, 0.0, out, validate, normal=True)


class PoseRefinement:
    """What `refine_pose` found, all tensors on the device: `pose` (B, 3) fp32, `width` (B,) fp32 [mm], `cost` (B,) fp64 = sum e^2 /
    lattice points, `normal_row` (B, 16) fp64 of that pose, `trace` (iterations + 1, B) fp64, the accepted cost after every
    evaluation (entry 0: the start's), `accepted` (B,) int32, the trials that lowered the cost, `last_step` (B, 4) fp64, |step|
    of the last solve (mm, mm, rad, mm)."""

    def __init__(self, pose, width, cost, normal_row, trace, accepted, last_step) -> None:
        self.pose, self.width, self.cost, self.normal_row = pose, width, cost, normal_row
        self.trace, self.accepted, self.last_step = trace, accepted, last_step

    def __repr__(self) -> str:
        return f"PoseRefinement({self.pose.shape[0]} observations, {self.trace.shape[0] - 1} iterations)"


_LAMBDA_MIN, _LAMBDA_MAX = 1e-12, 1e12      # bounds of the damping in refine_pose


def refine_pose(grid: MeshGrid, observed: torch.Tensor, grasp_widths: torch.Tensor, init, iterations: int = 10, fit_width: bool = False,
                stride: int = 1, damping: float = 1e-3, damping_up: float = 10.0, damping_down: float = 0.1,
                max_step: Sequence[float] = (0.5, 0.5, 0.1, 0.5), cost="mse", image_height_mm: float = 12.0,
                grasp_width_offset: float = 0.0, LR_flip: bool = False, invert_affine: bool = False, validate: bool = True) -> PoseRefinement:
    """Continuous refinement of in-hand poses by Levenberg-Marquardt on `score_poses`' mean squared error:
    the step that `estimate_pose`'s lattice cannot make.  `init` is (B, 3) -- or (B, S, 3) for S starts per observation, each
    refined on its own, the lowest final sum e^2 winning under `first_argmin`'s rule.  Every iteration is one `pose_normal_rows`
    evaluation of the trial and one gsd_mesh_pose_lm_update: the trial is accepted iff its sum e^2 is STRICTLY below the current
    one (the damping is then multiplied by `damping_down`, otherwise by `damping_up`), and the next trial solves
    (J^T J + damping diag(J^T J)) step = -J^T e, clipped per component to `max_step` (mm, mm, rad, mm).  So `trace` never rises.

    With `fit_width` the grasp width is a fourth free parameter, started at `grasp_widths`; a trial whose width + offset falls
    below 0 is a NaN row and is rejected.  Without it the width is returned as passed, bit for bit.  Only the 'mse' is
    differentiable here: `cost` 'l1' and 'iou' are refused.  Nothing is read back from the device (with `validate`, the widths
    are checked once, before the first evaluation).  The view arguments are `score_poses`'."""
    if cost != "mse":
        raise MeshDepthError(f"refine_pose: only cost='mse' can be refined ('l1' and 'iou' are not differentiable), got {cost!r}")
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise MeshDepthError(f"refine_pose: iterations must be an integer >= 0, got {iterations!r}")
    try:
        steps = tuple(float(v) for v in max_step)
        damp = tuple(float(v) for v in (damping, damping_up, damping_down))
    except (TypeError, ValueError):
        steps, damp = (), (float("nan"),) * 3
    if len(steps) != 4 or not all(math.isfinite(v) and v >= 0.0 for v in steps):
        raise MeshDepthError(f"refine_pose: max_step must be four finite values >= 0 (mm, mm, rad, mm), got {max_step!r}")
    if not (all(math.isfinite(v) for v in damp) and _LAMBDA_MIN <= damp[0] <= _LAMBDA_MAX and damp[1] >= 1.0 and 0.0 < damp[2] <= 1.0):
        raise MeshDepthError(f"refine_pose: need {_LAMBDA_MIN} <= damping <= {_LAMBDA_MAX}, damping_up >= 1 and 0 < damping_down <= 1, got "
                             f"{damping!r}, {damping_up!r}, {damping_down!r}")
    if not isinstance(grid, MeshGrid):
        raise MeshDepthError(f"refine_pose: grid must be a MeshGrid, got {type(grid).__name__}")
    if not isinstance(observed, torch.Tensor) or observed.dim() != 4:
        raise MeshDepthError("refine_pose: observed must be a (B, 2, H, W) tensor")
    b, _, h, w = (int(d) for d in observed.shape)
    start = torch.as_tensor(init, dtype=torch.float32).to(grid.device)
    if start.dim() == 2:
        start = start.unsqueeze(1)
    if start.dim() != 3 or start.shape[0] != b or start.shape[1] < 1 or start.shape[2] != 3:
        raise MeshDepthError(f"refine_pose: init must be ({b}, 3) or ({b}, S, 3), got {tuple(start.shape)}")
    s = int(start.shape[1])
    if (not isinstance(grasp_widths, torch.Tensor) or grasp_widths.dtype != torch.float32 or grasp_widths.device != grid.device
            or tuple(grasp_widths.shape) != (b,)):
        raise MeshDepthError(f"refine_pose: grasp_widths must be a float32 ({b},) tensor on {grid.device}")
    lm = L.gsd_pose_lm()
    lm.down, lm.up, lm.lambda_min, lm.lambda_max = damp[2], damp[1], _LAMBDA_MIN, _LAMBDA_MAX
    lm.max_step[:] = steps
    lm.free_mask = 15 if fit_width else 7
    n = b * s
    with torch.cuda.device(grid.device):
        dev = grid.device
        trial_pose = start.contiguous().clone()          # (B, S, 3): what the next evaluation scores, rewritten by every update
        trial_width = grasp_widths.unsqueeze(1).expand(b, s).contiguous()
        pose, width = torch.empty_like(trial_pose), torch.empty_like(trial_width)
        lam = torch.full((n,), damp[0], device=dev, dtype=torch.float64)
        row = torch.empty((b, s, NORMAL_ROW), device=dev, dtype=torch.float64)
        trial_row = torch.empty_like(row)
        trace = torch.empty((int(iterations) + 1, b, s), device=dev, dtype=torch.float64)
        accepted = torch.empty((b, s), device=dev, dtype=torch.int32)
        last_step = torch.empty((b, s, 4), device=dev, dtype=torch.float64)
        for it in range(int(iterations) + 1):
            pose_normal_rows(grid, observed, trial_pose, trial_width, image_height_mm, grasp_width_offset, LR_flip, invert_affine, stride,
                             out=trial_row, validate=validate and it == 0)
            lm.first = int(it == 0)
            check(lib.gsd_mesh_pose_lm_update(C.byref(lm), n, pose.data_ptr(), width.data_ptr(), lam.data_ptr(), row.data_ptr(),
                                              trial_pose.data_ptr(), trial_width.data_ptr(), trial_row.data_ptr(), trace[it].data_ptr(),
                                              accepted.data_ptr(), last_step.data_ptr(), L.stream_ptr()), "mesh_pose_lm_update")
        sq = row[..., 0]
        win = first_argmin(torch.where(torch.isnan(sq), torch.full_like(sq, float("inf")), sq))          # (B,): the best start
        pick = lambda t: torch.gather(t, 1, win.view(b, 1, *([1] * (t.dim() - 2))).expand(b, 1, *t.shape[2:])).squeeze(1)
        points = float(lattice_points((h, w), stride))
        best_trace = torch.gather(trace, 2, win.view(1, b, 1).expand(trace.shape[0], b, 1)).squeeze(2)
        return PoseRefinement(pick(pose), pick(width), pick(sq) / points, pick(row), best_trace / points, pick(accepted), pick(last_step))


_COSTS = ("mse", "l1", "iou")


def pose_cost(rows: torch.Tensor, kind="mse", n_points: int = 1) -> torch.Tensor:
    """The cost (...,) float64 of score rows (..., 5), in plain torch on the rows' device:
    'mse' = sum_sq / n_points, 'l1' = sum_abs / n_points (`lattice_points` gives n_points),
    'iou' = 1 - inter / (n_rendered + n_observed - inter), 0 where that union is empty, or a dict of weights over those three
    names, e.g. {"mse": 1.0, "iou": 0.05}.  A NaN cost (a refused width, a NaN observation) becomes +inf, so that it never beats
    a finite one."""
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float64 or rows.dim() < 1 or rows.shape[-1] != POSE_ROW:
        raise MeshDepthError(f"pose_cost: rows must be a float64 (..., {POSE_ROW}) tensor")
    weights = kind if isinstance(kind, dict) else {kind: 1.0}
    if not weights or any(k not in _COSTS for k in weights):
        raise MeshDepthError(f"pose_cost: kind must be one of {_COSTS} or a dict of weights over them, got {kind!r}")
    if not (isinstance(n_points, (int, np.integer)) and n_points >= 1):
        raise MeshDepthError(f"pose_cost: n_points must be a positive integer, got {n_points!r}")
    cost = None
    for name, wt in weights.items():
        if name == "mse":
            part = rows[..., 0] / float(n_points)
        elif name == "l1":
            part = rows[..., 1] / float(n_points)
        else:
            union = rows[..., 3] + rows[..., 4] - rows[..., 2]
            part = torch.where(union > 0, 1.0 - rows[..., 2] / torch.where(union > 0, union, torch.ones_like(union)),
                               torch.zeros_like(union))
            part = torch.where(torch.isnan(union), union, part)          # a NaN row stays NaN here, +inf below
        part = part if isinstance(kind, str) else float(wt) * part
        cost = part if cost is None else cost + part
    return torch.where(torch.isnan(cost), torch.full_like(cost, float("inf")), cost)


def first_argmin(cost: torch.Tensor) -> torch.Tensor:
    """Index (B,) of the smallest entry of every row of `cost` (B, P), THE LOWEST INDEX AMONG EQUAL ONES -- `torch.argmin`'s
    documented rule, spelled out so that the winner of a tie does not depend on how a reduction is scheduled.  A row of +inf
    (nothing finite to choose from) gives index 0; +inf never beats a finite cost."""
    best = cost.min(dim=1, keepdim=True).values
    index = torch.arange(cost.shape[1], device=cost.device).expand_as(cost)
    return torch.where(cost == best, index, torch.full_like(index, cost.shape[1])).min(dim=1).values.clamp_(max=cost.shape[1] - 1)


def _axis_schedule(half: np.float32, n: int, levels: int) -> Tuple[np.ndarray, np.ndarray]:
    """One axis of a search lattice in fp32: (half_spans (levels + 1,), offsets (levels, n)), step = half_spans[l + 1] =
    2 * half_spans[l] / (n - 1), offsets[l, i] = (i - (n - 1) / 2) * step."""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or levels < 1:
        raise MeshDepthError(f"estimate_pose: levels must be an integer >= 1, got {levels!r}")
    spans, offsets = [np.float32(half)], []
    for _ in range(int(levels)):
        step = (np.float32(2.0) * spans[-1]) / np.float32(n - 1)
        offsets.append((np.arange(n, dtype=np.float32) - np.float32((n - 1) // 2)) * step)
        spans.append(step)
    return np.asarray(spans, dtype=np.float32), np.stack(offsets)


def search_schedule(half_span: Sequence[float], counts: Sequence[int] = (7, 7, 9), levels: int = 4) -> Tuple[np.ndarray, np.ndarray]:
    """The lattices of `estimate_pose`, on the host in fp32: (half_spans (levels + 1, 3), offsets (levels, P, 3)).
    Level l has the half-span half_spans[l] and the step half_spans[l + 1] = 2 * half_spans[l] / (n - 1) per axis; its candidate
    with the flat index (i1 * n2 + i2) * n3 + i3 lies offsets[l] = (i - (n - 1) / 2) * step from the centre, so the middle
    candidate's offset is exactly 0.  The schedule depends on no data: it is computed once and uploaded."""
    try:
        counts = tuple(counts)
    except TypeError:
        counts = ()
    if len(counts) != 3 or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 3 or n % 2 == 0 for n in counts):
        raise MeshDepthError(f"estimate_pose: counts must be three odd integers >= 3, got {counts!r}")
    if isinstance(half_span, torch.Tensor):
        half_span = half_span.detach().cpu().numpy()
    half = np.asarray(half_span, dtype=np.float32)
    if half.shape != (3,) or not np.isfinite(half).all() or (half < 0).any():
        raise MeshDepthError(f"estimate_pose: half_span must be three finite values >= 0 (t1 [m], t2 [m], theta [rad]), got {half_span!r}")
    axes = [_axis_schedule(half[a], n, levels) for a, n in enumerate(counts)]
    offsets = [np.stack([m.reshape(-1) for m in np.meshgrid(*(offs[lvl] for _, offs in axes), indexing="ij")], axis=1)
               for lvl in range(int(levels))]
    return np.stack([spans for spans, _ in axes], axis=1), np.stack(offsets)


def width_schedule(width_half_span: float, width_count: int, levels: int = 4) -> Tuple[np.ndarray, np.ndarray]:
    """`search_schedule` for the fourth axis of `estimate_pose`, the grasp width [mm], on the host in fp32: (half_spans
    (levels + 1,), offsets (levels, n)).  Level l has the half-span half_spans[l] and the step half_spans[l + 1] =
    2 * half_spans[l] / (n - 1); its width k lies offsets[l, k] = (k - (n - 1) / 2) * step from the centre, so the middle offset
    is exactly 0.  n = `width_count` is odd and >= 3, `width_half_span` finite and > 0."""
    n = width_count
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 3 or n % 2 == 0 or n > POSE_WIDTHS_MAX:
        raise MeshDepthError(f"estimate_pose: width_count must be 1 or an odd integer in 3..{POSE_WIDTHS_MAX}, got {width_count!r}")
    try:
        half = np.float32(width_half_span)
    except (TypeError, ValueError):
        half = np.float32("nan")
    if half.shape != () or not np.isfinite(half) or not half > 0:
        raise MeshDepthError(f"estimate_pose: width_half_span must be a finite value > 0 [mm] for a width axis, got {width_half_span!r}")
    return _axis_schedule(half, n, levels)


class PoseEstimate:
    """What `estimate_pose` found, all tensors on the device: `pose` (B, 3) fp32 = (t1 [m], t2 [m], theta [rad]), `cost` (B,)
    fp64 and `row` (B, 5) fp64 of that pose at the last level's stride, `trace` (levels, B) fp64, the best cost of every level,
    `width` (B,) fp32 [mm], the grasp width that `row` was scored at: the one passed in, or the width axis' winner.
    `lattice_pose` (B, 3) and `lattice_cost` (B,) are the last level's winner and its cost: `pose` and `cost` themselves unless
    `refine_iterations` > 0 moved them past the lattice; `refinement` is then the `PoseRefinement`, otherwise None."""

    def __init__(self, pose: torch.Tensor, cost: torch.Tensor, row: torch.Tensor, trace: torch.Tensor,
                 width: Optional[torch.Tensor] = None, lattice_pose: Optional[torch.Tensor] = None,
                 lattice_cost: Optional[torch.Tensor] = None, refinement: Optional[PoseRefinement] = None) -> None:
        self.pose, self.cost, self.row, self.trace, self.width = pose, cost, row, trace, width
        self.lattice_pose = pose if lattice_pose is None else lattice_pose
        self.lattice_cost = cost if lattice_cost is None else lattice_cost
        self.refinement = refinement

    def __repr__(self) -> str:
        return f"PoseEstimate({self.pose.shape[0]} observations, {self.trace.shape[0]} levels)"


def estimate_pose(grid: MeshGrid, observed: torch.Tensor, grasp_widths: torch.Tensor, init, half_span: Sequence[float],
                  counts: Sequence[int] = (7, 7, 9), levels: int = 4, strides: Optional[Sequence[int]] = None, cost="mse",
                  image_height_mm: float = 12.0, grasp_width_offset: float = 0.0, LR_flip: bool = False,
                  invert_affine: bool = False, contact_depth: float = 0.0, validate: bool = True, width_half_span: float = 0.0,
                  width_count: int = 1, refine_iterations: int = 0) -> PoseEstimate:
    """The planar pose (t1, t2, theta) of `grid`'s mesh in the hand from depth images `observed` (B, 2, H, W) -- a prediction of the
    net or a label -- and the grasp widths: a coarse-to-fine lattice search, render-and-compare through `score_poses`.

    Level 0 is centred on `init` ((B, 3) or (3,): tensor or sequence) with the half-spans `half_span` (3,) (host values).  Level
    l scores the n1 * n2 * n3 candidates centre + (i - (n - 1) / 2) * step per axis, step = 2 * half / (n - 1), in fp32 (`counts`
    are odd and >= 3, so the middle candidate IS the centre, bit for bit), at `strides[l]` (default: 1 everywhere; at 320 x 427
    something like (4, 2, 1, 1) saves most of the time).  The winner is the candidate of least `pose_cost(rows, cost, ...)`:
    torch.argmin's rule, the LOWEST flat index (i1 * n2 + i2) * n3 + i3 among equal costs (`first_argmin`); NaN costs count as
    +inf, which never beats a finite cost.  The next level is centred on the winner with half-span = this level's step.  Because
    a row does not depend on its batch, the best cost cannot rise from one level to the next at an equal stride.

    An unknown grasp width: `width_count` = n_w odd and >= 3 with `width_half_span` > 0 [mm] adds the width
    as a fourth axis.  `grasp_widths` is then the starting width; level l scores every pose candidate at the n_w widths
    centre_w + (k - (n_w - 1) / 2) * step_w (`width_schedule`; one fp32 add, the middle width IS the centre) through
    `score_poses_widths` -- one render per pose candidate, whatever n_w -- and the winner is the least cost over the flat index
    pose_flat * n_w + k, under the same tie rule.  A lattice width whose g falls below 0 is a NaN row, hence +inf.  The default,
    `width_count` = 1 (`width_half_span` is then ignored), is the fixed-width search above, call for call.  `PoseEstimate.width`
    is the width of the winner.

    `refine_iterations` = K > 0 runs `refine_pose` for K iterations from the last level's winner, at the
    last level's stride, the width free iff there is a width axis.  `pose`, `width` and `cost` are then the refined ones, `row` is
    one `score_poses` call at the refined pose, and `lattice_pose` / `lattice_cost` keep the winner.  The refinement minimises
    the 'mse' whatever `cost` is: it accepts a step only if sum e^2 -- `score_poses`' sum_sq bit for bit -- falls, so for
    cost='mse' `cost` <= `lattice_cost` holds exactly; for another `cost` it need not.  The default 0 is the search alone.

    Everything runs on the device; nothing is read back (with `validate=True`, `score_poses`' one check of the widths is made
    once, before the first level -- of the starting widths, with a width axis).  The view arguments are `score_poses`'."""
    if isinstance(refine_iterations, bool) or not isinstance(refine_iterations, (int, np.integer)) or refine_iterations < 0:
        raise MeshDepthError(f"estimate_pose: refine_iterations must be an integer >= 0, got {refine_iterations!r}")
    spans, offsets = search_schedule(half_span, counts, levels)
    levels = int(levels)
    strides = (1,) * levels if strides is None else tuple(strides)
    if len(strides) != levels or any(isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 1 for s in strides):
        raise MeshDepthError(f"estimate_pose: strides must be {levels} integers >= 1, one per level, got {strides!r}")
    try:
        w_half = float(width_half_span)
    except (TypeError, ValueError):
        w_half = float("nan")
    if not (math.isfinite(w_half) and w_half >= 0.0):
        raise MeshDepthError(f"estimate_pose: width_half_span must be finite and >= 0 [mm], got {width_half_span!r}")
    width_axis = not (isinstance(width_count, (int, np.integer)) and not isinstance(width_count, bool) and width_count == 1)
    if width_axis:
        _, w_offsets = width_schedule(width_half_span, width_count, levels)          # raises for an even count, 2, a zero span
    if not isinstance(grid, MeshGrid):
        raise MeshDepthError(f"estimate_pose: grid must be a MeshGrid, got {type(grid).__name__}")
    if not isinstance(observed, torch.Tensor) or observed.dim() != 4:
        raise MeshDepthError("estimate_pose: observed must be a (B, 2, H, W) tensor")
    b, _, h, w = (int(d) for d in observed.shape)
    centre = torch.as_tensor(init, dtype=torch.float32).to(grid.device)
    if centre.dim() == 1:
        centre = centre.unsqueeze(0).expand(b, -1)
    if tuple(centre.shape) != (b, 3):
        raise MeshDepthError(f"estimate_pose: init must be ({b}, 3) or (3,), got {tuple(centre.shape)}")
    centre = centre.contiguous()
    if width_axis:
        if (not isinstance(grasp_widths, torch.Tensor) or grasp_widths.dtype != torch.float32 or grasp_widths.device != grid.device
                or tuple(grasp_widths.shape) != (b,)):
            raise MeshDepthError(f"estimate_pose: grasp_widths must be a float32 ({b},) tensor on {grid.device}")
        if validate:
            _check_widths("estimate_pose", grasp_widths, float(grasp_width_offset))
    with torch.cuda.device(grid.device):
        offs = torch.from_numpy(offsets).to(grid.device)          # (levels, P, 3)
        trace = torch.empty((levels, b), device=grid.device, dtype=torch.float64)
        best_cost = best_row = None
        if width_axis:
            w_offs = torch.from_numpy(w_offsets).to(grid.device)          # (levels, n_w)
            n_w = int(w_offs.shape[1])
            centre_w = grasp_widths.contiguous()
        for lvl in range(levels):
            cand = (centre.unsqueeze(1) + offs[lvl].unsqueeze(0)).contiguous()          # one fp32 add: the middle one is the centre
            if width_axis:
                cand_w = (centre_w.unsqueeze(1) + w_offs[lvl].unsqueeze(0)).contiguous()          # (B, n_w), the same rule
                rows = score_poses_widths(grid, observed, cand, cand_w, image_height_mm, grasp_width_offset, LR_flip, invert_affine,
                                          strides[lvl], contact_depth, validate=False).reshape(b, -1, POSE_ROW)
            else:
                rows = score_poses(grid, observed, cand, grasp_widths, image_height_mm, grasp_width_offset, LR_flip, invert_affine,
                                   strides[lvl], contact_depth, validate=validate and lvl == 0)
            c = pose_cost(rows, cost, lattice_points((h, w), strides[lvl]))
            win = first_argmin(c)
            best_row = torch.gather(rows, 1, win.view(b, 1, 1).expand(b, 1, POSE_ROW)).squeeze(1)
            best_cost = torch.gather(c, 1, win.view(b, 1)).squeeze(1)
            trace[lvl] = best_cost
            if width_axis:
                centre_w = torch.gather(cand_w, 1, (win % n_w).view(b, 1)).squeeze(1).contiguous()
                win = torch.div(win, n_w, rounding_mode="floor")
            centre = torch.gather(cand, 1, win.view(b, 1, 1).expand(b, 1, 3)).squeeze(1).contiguous()
        width = centre_w if width_axis else grasp_widths
        if refine_iterations == 0:
            return PoseEstimate(centre, best_cost, best_row, trace, width)
        fine = refine_pose(grid, observed, width, centre, int(refine_iterations), width_axis, strides[-1], image_height_mm=image_height_mm,
                           grasp_width_offset=grasp_width_offset, LR_flip=LR_flip, invert_affine=invert_affine, validate=False)
        row = score_poses(grid, observed, fine.pose.unsqueeze(1), fine.width, image_height_mm, grasp_width_offset, LR_flip, invert_affine,
                          strides[-1], contact_depth, validate=False).squeeze(1)
        return PoseEstimate(fine.pose, pose_cost(row, cost, lattice_points((h, w), strides[-1])), row, trace, fine.width, centre,
                            best_cost, fine)


def pose_error(estimate, truth: torch.Tensor) -> torch.Tensor:
    """(B, 3) float64: the translation errors of `estimate` (a PoseEstimate or a (B, 3) pose tensor) against `truth` (B, 3) or
    (3,) -- a dataset file's `in_hand_pose[:, :3]` -- in MILLIMETRES, and the angle error in radians wrapped to (-pi, pi]."""
    pose = estimate.pose if isinstance(estimate, PoseEstimate) else estimate
    if not isinstance(pose, torch.Tensor) or pose.dim() != 2 or pose.shape[1] != 3:
        raise MeshDepthError("pose_error: estimate must be a PoseEstimate or a (B, 3) tensor")
    truth = torch.as_tensor(truth).to(pose.device)
    if truth.shape[-1] != 3 or truth.dim() > 2:
        raise MeshDepthError(f"pose_error: truth must be (B, 3) or (3,), got {tuple(truth.shape)}")
    d = pose.to(torch.float64) - truth.to(torch.float64)
    angle = d[:, 2] - 2.0 * math.pi * torch.ceil((d[:, 2] - math.pi) / (2.0 * math.pi))
    return torch.stack((1000.0 * d[:, 0], 1000.0 * d[:, 1], angle), dim=1)
