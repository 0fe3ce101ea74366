"""The times of DESIGN.md section 17: score_poses (the fused render-and-compare kernel) against the unfused form (render_depth of
the same candidates, then the five reductions in torch, fp64) on section 16's mesh, the subdivision-6 icosphere (81,920
triangles), at 320 x 427 with P = 512 candidates for one observation, strides 4, 2 and 1; and the wall time of one default
estimate_pose (counts (7, 7, 9), 4 levels) with strides (4, 2, 1, 1).  Device events, median of 10 after 3 warm-ups, the two
forms alternating in one process.
usage (GPU box): PYTHONPATH=. python profiles/bench_mesh_pose.py [--p 512] [--subdivisions 6]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import mesh_depth_ref as R  # noqa: E402

from gelslim_depth_amd.mesh_depth import MeshGrid, estimate_pose, pose_error, render_depth, score_poses  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--p", type=int, default=512)
ap.add_argument("--subdivisions", type=int, default=6)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
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
rows = torch.empty((1, a.p, 5), dtype=torch.float64, device="cuda")
images = torch.empty((a.p, 2, *SIZE), device="cuda")
widths_p = width.expand(a.p).contiguous()


def unfused(stride):
    render_depth(grid, cand_d[0], widths_p, SIZE, HEIGHT_MM, out=images, validate=False)
    o = stride // 2
    r, d = images[:, :, o::stride, o::stride].double(), observed[:, :, o::stride, o::stride].double()
    e = r - d
    cr, cd = r < 0, torch.isfinite(d) & (d < 0)
    return torch.stack(((e * e).sum((1, 2, 3)), e.abs().sum((1, 2, 3)), (cr & cd).sum((1, 2, 3)).double(), cr.sum((1, 2, 3)).double(),
                        cd.expand_as(cr).sum((1, 2, 3)).double()), dim=1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0), r


for stride in (4, 2, 1):
    forms = {"fused": lambda: score_poses(grid, observed, cand_d, width, HEIGHT_MM, stride=stride, out=rows, validate=False),
             "unfused": lambda: unfused(stride)}
    runs = {k: [] for k in forms}
    for rep in range(a.warmup + a.reps):
        for k, fn in forms.items():          # alternating
            ms = timed(fn)
            if rep >= a.warmup:
                runs[k].append(ms[:2])
    got, want = rows[0].clone(), unfused(stride)
    same_counts = torch.equal(got[:, 2:], want[:, 2:])
    rel = float(((got[:, :2] - want[:, :2]).abs() / want[:, :2]).max())
    for k in forms:
        dev = statistics.median(r[0] for r in runs[k])
        host = statistics.median(r[1] for r in runs[k])
        spread = (min(r[0] for r in runs[k]), max(r[0] for r in runs[k]))
        print(f"stride {stride} {k:8s}: {dev:.3f} ms per {a.p} candidates = {1e3 * dev / a.p:.2f} us per scored candidate (device events, "
              f"min {spread[0]:.3f} max {spread[1]:.3f}; {host:.3f} ms host clock); median of {a.reps} after {a.warmup}")
    print(f"stride {stride}: counts equal {same_counts}, worst relative difference of the sums {rel:.2e}")

init = torch.tensor([0.4e-3 + 0.9e-3, -0.3e-3 - 0.7e-3, 0.35 + 0.3], device="cuda")
half = (1.5e-3, 1.5e-3, 0.6)
for strides in ((4, 2, 1, 1), (1, 1, 1, 1)):
    walls = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        est = estimate_pose(grid, observed, width, init, half, strides=strides, image_height_mm=HEIGHT_MM, validate=False)
        torch.cuda.synchronize()
        if rep >= a.warmup:
            walls.append(1e3 * (time.perf_counter() - t0))
    err = pose_error(est, torch.from_numpy(truth).cuda())[0].tolist()          # a sphere: only the translation is observable
    print(f"estimate_pose counts (7, 7, 9), 4 levels, strides {strides}: {statistics.median(walls):.2f} ms wall (host clock to device "
          f"idle; min {min(walls):.2f} max {max(walls):.2f}), translation error (mm, mm) {err[:2]}, cost {est.cost.item():.3e}")
