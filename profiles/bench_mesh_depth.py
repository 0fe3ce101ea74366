"""The times of DESIGN.md section 16: MeshGrid build and render_depth per sample on the subdivision-6 icosphere (81,920
triangles) at 320 x 427, N = 256 poses per launch, device events, median of 10 after 3 warm-ups; beside them the restated
reference (tests/mesh_depth_ref.py: reference_from_points, 1e5 surface points, two scipy griddata calls) per sample on the host.
  --cells 0.5,1,2,4   also render on grids whose cells are these multiples of the default (the cell-size model's check)
usage (GPU box): PYTHONPATH=. python profiles/bench_mesh_depth.py [--n 256] [--subdivisions 6] [--cells ...] [--no-reference]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import mesh_depth_ref as R  # noqa: E402
from cell_list_phases import build_phases  # noqa: E402

from gelslim_depth_amd.mesh_depth import MeshGrid, render_depth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=256)
ap.add_argument("--subdivisions", type=int, default=6)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--cells", default="")
ap.add_argument("--no-reference", action="store_true")
a = ap.parse_args()

SIZE, HEIGHT_MM, RADIUS = (320, 427), 12.0, 5.0
tri = R.sphere(a.subdivisions, RADIUS, (1.0, -0.5, 0.25))
rng = np.random.Generator(np.random.PCG64(0))
poses = np.stack((rng.uniform(-2e-3, 2e-3, a.n), rng.uniform(-2e-3, 2e-3, a.n), rng.uniform(-np.pi, np.pi, a.n)), axis=1)
widths = 2 * (RADIUS - rng.uniform(0.5, 1.5, a.n))            # 0.5 .. 1.5 mm of indentation
poses_d = torch.from_numpy(poses.astype(np.float32)).cuda()
widths_d = torch.from_numpy(widths.astype(np.float32)).cuda()
out = torch.empty((a.n, 2, *SIZE), device="cuda")


def timed(fn):
    """(device ms between two events around fn, host ms until the device is idle)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0), r


def median(fn):
    for _ in range(a.warmup):
        timed(fn)
    runs = [timed(fn)[:2] for _ in range(a.reps)]
    return statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs)


dev_ms, host_ms = median(lambda: MeshGrid(tri, 1.0, "+y+z", "cuda"))
grid = MeshGrid(tri, 1.0, "+y+z", "cuda")
for mult in (1.0, min([float(c) for c in a.cells.split(",") if c] + [0.5])):      # the default cells and the finest grid of --cells
    g = MeshGrid(tri, 1.0, "+y+z", "cuda", cell_mm=grid.cell_mm * mult)
    count_ms, fill_ms = build_phases(lambda: MeshGrid(tri, 1.0, "+y+z", "cuda", cell_mm=grid.cell_mm * mult), "gsd_mesh_depth", a.warmup, a.reps)
    print(f"cell lists, cells x {mult:g} ({g.grid.nx * g.grid.ny} cells, {g.pairs} pairs): records + count + scan {count_ms:.4f} ms, fill "
          f"{fill_ms:.4f} ms (device events; median of {a.reps} after {a.warmup})")
print(f"{grid!r}")
print(f"MeshGrid build, {tri.shape[0]} triangles: {host_ms:.2f} ms on the host clock (numpy preparation, upload, count, the one "
      f"read, fill), {dev_ms:.2f} ms between device events; median of {a.reps} after {a.warmup}")
dev_ms, host_ms = median(lambda: render_depth(grid, poses_d, widths_d, SIZE, HEIGHT_MM, out=out, validate=False))
contact = float((out < 0).float().mean())
print(f"render_depth N={a.n} {SIZE[0]}x{SIZE[1]}: {dev_ms:.3f} ms per launch = {1e3 * dev_ms / a.n:.2f} us per sample (device "
      f"events; {host_ms:.3f} ms host clock), contact fraction {contact:.3f}, deepest {float(out.min()):.4f} mm; median of "
      f"{a.reps} after {a.warmup}")
for mult in [float(c) for c in a.cells.split(",") if c]:
    g = MeshGrid(tri, 1.0, "+y+z", "cuda", cell_mm=grid.cell_mm * mult)
    other = torch.empty_like(out)
    dev_ms, _ = median(lambda: render_depth(g, poses_d, widths_d, SIZE, HEIGHT_MM, out=other, validate=False))
    print(f"  cells x {mult:g}: {g!r}: {dev_ms:.3f} ms per launch, same bits {torch.equal(other, out)}")
if not a.no_reference:
    ms = []
    for k in range(3):
        t0 = time.perf_counter()
        pts = R.sample_surface(tri, 1e5, seed=k)
        R.reference_from_points(pts, "+y+z", poses[k], widths[k], SIZE, HEIGHT_MM)
        ms.append(1e3 * (time.perf_counter() - t0))
    print(f"restated reference (1e5 points, two griddata calls, {os.cpu_count()} CPUs visible, "
          f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')}): {statistics.median(ms):.0f} ms per sample (median of 3: "
          f"{', '.join(f'{m:.0f}' for m in ms)})")
