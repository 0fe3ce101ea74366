"""The times of DESIGN.md section 18: one score_poses_widths call over G widths against G calls of score_poses on the same inputs, on
section 16's mesh, the subdivision-6 icosphere (81,920 triangles), at 320 x 427 with P = 512 candidates for one observation, G = 1,
3, 5, 9, strides 4 and 1; and the wall time of one estimate_pose (counts (7, 7, 9), 4 levels, strides (4, 2, 1, 1)) with and
without a 5-point width axis.  Device events, median of 10 after 3 warm-ups, the two forms alternating in one process; every
measurement is repeated three times and the spread is the max - min of the G calls' three medians.
With --parent-lib PATH the G calls go through gsd_mesh_pose_score of that libgsd.so (the parent commit's build) instead of this
tree's, loaded into the same process beside it and called by the same score_poses.
usage (GPU box): PYTHONPATH=. python profiles/bench_mesh_pose_width.py [--p 512] [--subdivisions 6] [--parent-lib PATH]"""
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
from gelslim_depth_amd import mesh_depth as M  # noqa: E402
from gelslim_depth_amd.mesh_depth import MeshGrid, estimate_pose, pose_error, render_depth, score_poses, score_poses_widths  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--p", type=int, default=512)
ap.add_argument("--subdivisions", type=int, default=6)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--parent-lib", default=None)
a = ap.parse_args()

SIZE, HEIGHT_MM, RADIUS = (320, 427), 12.0, 5.0
tri = R.sphere(a.subdivisions, RADIUS, (1.0, -0.5, 0.25))
grid = MeshGrid(tri, 1.0, "+y+z", "cuda")
print(f"{grid!r}")
rng = np.random.Generator(np.random.PCG64(0))
truth = np.array([[0.4e-3, -0.3e-3, 0.35]])
cand = truth + rng.uniform(-1, 1, (a.p, 3)) * np.array([1.5e-3, 1.5e-3, 0.6])
cand_d = torch.from_numpy(cand.astype(np.float32)).cuda().unsqueeze(0).contiguous()
width = torch.tensor([2 * (RADIUS - 1.0)], dtype=torch.float32, device="cuda")          # 1 mm of indentation
observed = render_depth(grid, torch.from_numpy(truth.astype(np.float32)).cuda(), width, SIZE, HEIGHT_MM)
observed = (observed + 0.02 * torch.randn(observed.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(0))).contiguous()

parent = None
if a.parent_lib:
    parent = C.CDLL(os.path.abspath(a.parent_lib))
    for name in ("gsd_mesh_pose_score_workspace", "gsd_mesh_pose_score"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = L.SIGNATURES[name]
    print(f"the G calls go through {a.parent_lib}")


def one_width(width_1, stride, out):
    """score_poses of this tree, or the same Python through the parent's library: score_poses takes its two entry points from the
    module's `lib`, so both forms pay the same host work between the first event and the first launch."""
    if parent is None:
        return score_poses(grid, observed, cand_d, width_1, HEIGHT_MM, stride=stride, out=out, validate=False)
    M.lib = parent
    try:
        return score_poses(grid, observed, cand_d, width_1, HEIGHT_MM, stride=stride, out=out, validate=False)
    finally:
        M.lib = L.lib


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for stride in (4, 1):
    for g in (1, 3, 5, 9):
        widths = (width[0] + torch.linspace(-0.6, 0.6, g, device="cuda") * (g > 1)).reshape(1, g).contiguous()
        columns = [widths[:, k].contiguous() for k in range(g)]
        fused_rows = torch.empty((1, a.p, g, 5), dtype=torch.float64, device="cuda")
        call_rows = [torch.empty((1, a.p, 5), dtype=torch.float64, device="cuda") for _ in range(g)]
        forms = {"fused": lambda: score_poses_widths(grid, observed, cand_d, widths, HEIGHT_MM, stride=stride, out=fused_rows, validate=False),
                 "calls": lambda: [one_width(columns[k], stride, call_rows[k]) for k in range(g)]}
        medians = {k: [] for k in forms}
        for _ in range(3):
            runs = {k: [] for k in forms}
            for rep in range(a.warmup + a.reps):
                for k, fn in forms.items():          # alternating
                    ms = timed(fn)
                    if rep >= a.warmup:
                        runs[k].append(ms)
            for k in forms:
                medians[k].append(statistics.median(runs[k]))
        same = torch.equal(fused_rows, torch.stack(call_rows, dim=2))
        fused, calls = statistics.median(medians["fused"]), statistics.median(medians["calls"])
        spread = max(medians["calls"]) - min(medians["calls"])
        verdict = (f"within the spread of one call: {abs(fused - calls) <= spread}" if g == 1
                   else f"faster by more than the spread: {calls - fused > spread}")
        print(f"stride {stride} G {g}: fused {fused:.3f} ms (medians {', '.join(f'{m:.3f}' for m in medians['fused'])}), {g} calls "
              f"{calls:.3f} ms (medians {', '.join(f'{m:.3f}' for m in medians['calls'])}; spread {spread:.3f}), ratio {calls / fused:.2f}, "
              f"{1e3 * fused / (a.p * g):.2f} us per scored (candidate, width); {verdict}; rows equal {same}")

init = torch.tensor([0.4e-3 + 0.9e-3, -0.3e-3 - 0.7e-3, 0.35 + 0.3], device="cuda")
half = (1.5e-3, 1.5e-3, 0.6)
start = (width + 0.35).contiguous()
for label, w0, kw in (("fixed width", width, {}), ("5-point width axis, start + 0.35 mm", start, {"width_half_span": 0.6, "width_count": 5}),
                      ("fixed width, 0.35 mm wrong", start, {})):
    walls = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        est = estimate_pose(grid, observed, w0, init, half, strides=(4, 2, 1, 1), image_height_mm=HEIGHT_MM, validate=False, **kw)
        torch.cuda.synchronize()
        if rep >= a.warmup:
            walls.append(1e3 * (time.perf_counter() - t0))
    err = pose_error(est, torch.from_numpy(truth).cuda())[0].tolist()          # a sphere: only the translation is observable
    print(f"estimate_pose counts (7, 7, 9), 4 levels, strides (4, 2, 1, 1), {label}: {statistics.median(walls):.2f} ms wall (host clock to "
          f"device idle; min {min(walls):.2f} max {max(walls):.2f}), translation error (mm, mm) {err[:2]}, width error "
          f"{est.width.item() - width.item():+.4f} mm, cost {est.cost.item():.3e}")
