"""The times of DESIGN.md section 22: contact_patches (gsd_contact_patches_label / _stats / _filter) at B = 64 images of 2 x 320 x 427

  1. on rendered depth of section 17's icosphere with speckle (the typical case): labelling, statistics and filter separately,
     and the end-to-end call contact_patches(...).filtered_depth(...);
  2. the same on the serpentine (every even row set, joined at alternating ends: one patch per plane whose only path is 68,480
     pixels long), the worst case;
  3. depth_points (padded, sensor frame, no normals) on the same input: the yardstick of a one-read compaction;
  4. where scipy imports: copy to the host, scipy.ndimage.label per plane, copy back -- what a user does today.

Device events, median of `--reps` after `--warmup`, the forms alternating in one process; the host path by the host clock.  Where
scipy imports, the labels of both inputs are also compared with scipy's at min_area = 1 (the numbering is the same by definition).
usage (GPU box): PYTHONPATH=. python profiles/contact_patches_time.py [--b 64] [--reps 10] [--connectivity 8]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import mesh_depth_ref as R  # noqa: E402

from gelslim_depth_amd import _lib as L  # noqa: E402
from gelslim_depth_amd.contact_patches import contact_patches  # noqa: E402
from gelslim_depth_amd.contact_points import depth_points  # noqa: E402
from gelslim_depth_amd.mesh_depth import MeshGrid, render_depth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--b", type=int, default=64)
ap.add_argument("--subdivisions", type=int, default=6)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--connectivity", type=int, default=8)
ap.add_argument("--min-area", type=int, default=4)
ap.add_argument("--max-patches", type=int, default=64)
ap.add_argument("--no-host", action="store_true", help="skip the scipy path and the comparison with it")
a = ap.parse_args()

SIZE, HEIGHT_MM, RADIUS = (320, 427), 12.0, 5.0
H, W = SIZE
K = a.max_patches

try:
    import scipy.ndimage as ndi
except ImportError:
    ndi = None
if a.no_host:
    ndi = None


def rendered_with_speckle():
    grid = MeshGrid(R.sphere(a.subdivisions, RADIUS, (1.0, -0.5, 0.25)), 1.0, "+y+z", "cuda")
    rng = np.random.Generator(np.random.PCG64(0))
    poses = torch.from_numpy((rng.uniform(-1, 1, (a.b, 3)) * np.array([1.5e-3, 1.5e-3, 3.0])).astype(np.float32)).cuda()
    widths = torch.from_numpy((2 * (RADIUS - rng.uniform(0.5, 1.5, a.b))).astype(np.float32)).cuda()
    clean = render_depth(grid, poses, widths, SIZE, HEIGHT_MM)
    gen = torch.Generator(device="cuda").manual_seed(0)
    speckle = (torch.rand(clean.shape, device="cuda", generator=gen) < 2e-3) & (clean == 0)
    return torch.where(speckle, torch.full_like(clean, -0.05), clean).contiguous(), int(speckle.sum())


def serpentine():
    m = np.zeros((H, W), dtype=bool)
    m[0::2] = True
    for r in range(1, H, 2):
        m[r, W - 1 if (r // 2) % 2 == 0 else 0] = True
    plane = np.where(m, np.float32(-1.0), np.float32(0.0)).astype(np.float32)
    return torch.from_numpy(np.broadcast_to(plane, (a.b, 2, H, W)).copy()).cuda()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0), r


def host_path(depth):
    structure = np.ones((3, 3)) if a.connectivity == 8 else None
    mask = (depth < 0).cpu().numpy()
    out = np.empty(mask.shape, dtype=np.int32)
    for b in range(mask.shape[0]):
        for ch in range(2):
            out[b, ch], _ = ndi.label(mask[b, ch], structure=structure)
    return torch.from_numpy(out).cuda()


def measure(name, depth):
    b = depth.shape[0]
    view = L.gsd_contact_patches_view()
    view.contact_depth, view.connectivity, view.min_area = 0.0, a.connectivity, a.min_area
    words = int(L.lib.gsd_contact_patches_workspace(b, H, W))
    ws = torch.empty((words,), device="cuda", dtype=torch.int32)
    labels = torch.empty((b, 2, H, W), device="cuda", dtype=torch.int32)
    counts = torch.empty((b, 2), device="cuda", dtype=torch.int32)
    stats = torch.empty((b, 2, K, 12), device="cuda", dtype=torch.int64)
    out = torch.empty_like(depth)
    st = L.stream_ptr()

    def label():
        L.check(L.lib.gsd_contact_patches_label(C.byref(view), depth.data_ptr(), b, H, W, labels.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                                words, st), "label")

    def table():
        L.check(L.lib.gsd_contact_patches_stats(C.byref(view), depth.data_ptr(), labels.data_ptr(), b, H, W, K, stats.data_ptr(), st), "stats")

    def filt():
        L.check(L.lib.gsd_contact_patches_filter(C.byref(view), depth.data_ptr(), labels.data_ptr(), None, b, H, W, K, out.data_ptr(), st),
                "filter")

    kw = dict(connectivity=a.connectivity, min_area=a.min_area, max_patches=K, image_height_mm=HEIGHT_MM)
    n_max = int(depth_points(depth, frame="sensor", image_height_mm=HEIGHT_MM, normals=False).counts.sum(dim=1).max())
    forms = {"label": label, "stats": table, "filter": filt,
             "contact_patches(...).filtered_depth(...)": lambda: contact_patches(depth, **kw).filtered_depth(depth),
             "depth_points, padded, no normals": lambda: depth_points(depth, frame="sensor", image_height_mm=HEIGHT_MM, normals=False,
                                                                      max_points=n_max, validate=False)}
    runs = {n: [] for n in forms}
    for rep in range(a.warmup + a.reps):
        for n, fn in forms.items():          # alternating
            ms = timed(fn)
            if rep >= a.warmup:
                runs[n].append(ms[:2])
    contact = int((depth < 0).sum())
    print(f"== {name}: B = {b}, 2 x {H} x {W}, {contact} contact pixels of {depth.numel()} ({100.0 * contact / depth.numel():.2f} %), "
          f"connectivity {a.connectivity}, min_area {a.min_area}, K = {K}; patches kept per plane: at most {int(counts.max())}, "
          f"{int(counts.sum())} in all")
    med = {}
    for n in forms:
        med[n] = statistics.median(r[0] for r in runs[n])
        print(f"{name} | {n:42s}: {med[n]:.3f} ms (device events, min {min(r[0] for r in runs[n]):.3f} max {max(r[0] for r in runs[n]):.3f}; "
              f"{statistics.median(r[1] for r in runs[n]):.3f} ms host clock to device idle); median of {a.reps} after {a.warmup}")
    if ndi is not None:
        host = [timed(lambda: host_path(depth))[1] for _ in range(3)]
        print(f"{name} | {'host: copy, scipy.ndimage.label, copy back':42s}: {statistics.median(host):.1f} ms (host clock, median of 3)")
        view.min_area = 1
        label()
        same = torch.equal(labels, host_path(depth))
        print(f"{name} | labels at min_area = 1 equal scipy's: {same}")
        assert same
    return med


px = 2 * a.b * H * W
print(f"bytes per pass at B = {a.b} ({px} pixels): init reads depth and writes parents and areas, {12 * px / 1e6:.1f} MB; merge reads the "
      f"parents twice (own row and the row above), {8 * px / 1e6:.1f} MB + unions; flatten reads and rewrites the parents, {8 * px / 1e6:.1f} "
      f"MB + finds; count and number read parents (areas at roots only), {4 * px / 1e6:.1f} MB each; relabel reads and rewrites the labels, "
      f"{8 * px / 1e6:.1f} MB + the numbers at the roots; stats reads labels and depth, {8 * px / 1e6:.1f} MB; "
      f"filter reads depth and labels and writes depth, {12 * px / 1e6:.1f} MB")
depth, n_speckle = rendered_with_speckle()
print(f"speckle: {n_speckle} pixels at -0.05 mm")
typical = measure("rendered + speckle", depth)
worst = measure("serpentine", serpentine())
for n in ("label", "stats", "filter", "contact_patches(...).filtered_depth(...)"):
    print(f"serpentine / rendered, {n}: {worst[n] / typical[n]:.2f}")
