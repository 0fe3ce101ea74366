"""The times of DESIGN.md section 19 on section 17's mesh and sizes: the subdivision-6 icosphere (81,920 triangles) at 320 x 427.
  * pose_normal_rows (gsd_mesh_pose_normal: the score's walk plus J^T J and J^T e) against score_poses, P = 512 candidates for one
    observation, strides 1, 2 and 4: device events, median of 10 after 3 warm-ups, the two forms alternating in one process;
  * one estimate_pose at the default 4 levels against 3 levels + refine_iterations=10, both with strides (4, 2, 1[, 1]): wall time
    (host clock to device idle) and pose_error for both -- on the sphere, where only the translation is observable, and on the
    sheared ellipsoid of tests/mesh_depth_ref.py at the same subdivision, where the angle is too.
usage (GPU box): PYTHONPATH=. python profiles/bench_mesh_pose_refine.py [--p 512] [--subdivisions 6]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import mesh_depth_ref as R  # noqa: E402

from gelslim_depth_amd.mesh_depth import MeshGrid, estimate_pose, pose_error, pose_normal_rows, render_depth, score_poses  # noqa: E402

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
normal = torch.empty((1, a.p, 16), dtype=torch.float64, device="cuda")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0), r


for stride in (1, 2, 4):
    forms = {"score": lambda: score_poses(grid, observed, cand_d, width, HEIGHT_MM, stride=stride, out=rows, validate=False),
             "normal": lambda: pose_normal_rows(grid, observed, cand_d, width, HEIGHT_MM, stride=stride, out=normal, validate=False)}
    runs = {k: [] for k in forms}
    for rep in range(a.warmup + a.reps):
        for k, fn in forms.items():          # alternating
            ms = timed(fn)
            if rep >= a.warmup:
                runs[k].append(ms[:2])
    med = {}
    for k in forms:
        med[k] = statistics.median(r[0] for r in runs[k])
        host = statistics.median(r[1] for r in runs[k])
        spread = (min(r[0] for r in runs[k]), max(r[0] for r in runs[k]))
        print(f"stride {stride} {k:6s}: {med[k]:.3f} ms per {a.p} candidates = {1e3 * med[k] / a.p:.2f} us per candidate (device events, "
              f"min {spread[0]:.3f} max {spread[1]:.3f}; {host:.3f} ms host clock); median of {a.reps} after {a.warmup}")
    print(f"stride {stride}: a normal row costs {med['normal'] / med['score']:.2f} scores; entry 0 == sum_sq bitwise "
          f"{torch.equal(normal[..., 0], rows[..., 0])}, entry 1 == n_rendered {torch.equal(normal[..., 1], rows[..., 3])}")


def search(name, grid, observed, width):
    init = torch.tensor([0.4e-3 + 0.9e-3, -0.3e-3 - 0.7e-3, 0.35 + 0.3], device="cuda")
    half = (1.5e-3, 1.5e-3, 0.6)
    forms = {"4 levels": dict(levels=4, strides=(4, 2, 1, 1)), "3 levels + 10 refinements": dict(levels=3, strides=(4, 2, 1), refine_iterations=10)}
    walls, ests = {k: [] for k in forms}, {}
    for rep in range(a.warmup + a.reps):
        for k, kw in forms.items():          # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ests[k] = estimate_pose(grid, observed, width, init, half, image_height_mm=HEIGHT_MM, validate=False, **kw)
            torch.cuda.synchronize()
            if rep >= a.warmup:
                walls[k].append(1e3 * (time.perf_counter() - t0))
    for k in forms:
        est = ests[k]
        err = pose_error(est, torch.from_numpy(truth).cuda())[0].tolist()
        extra = "" if est.refinement is None else (f", lattice cost {est.lattice_cost.item():.6e}, {int(est.refinement.accepted[0])} steps accepted, "
                                                   f"last |step| {est.refinement.last_step[0].tolist()}")
        print(f"{name}: estimate_pose counts (7, 7, 9), {k}: {statistics.median(walls[k]):.2f} ms wall (host clock to device idle; min "
              f"{min(walls[k]):.2f} max {max(walls[k]):.2f}), pose_error (mm, mm, rad) {err}, cost {est.cost.item():.6e}{extra}")


search("icosphere", grid, observed, width)
# the sphere cannot show the angle: tests/mesh_depth_ref.ellipsoid (semi-axes 6, 5, 7 mm, sheared) at the same subdivision, image and noise
tri_e = R.ellipsoid(a.subdivisions)
grid_e = MeshGrid(tri_e, 1.0, "+y+z", "cuda")
print(f"{grid_e!r}")
width_e = torch.tensor([2 * (grid_e.q_range[1] - 1.0)], dtype=torch.float32, device="cuda")          # 1 mm of indentation at the crest
observed_e = render_depth(grid_e, torch.from_numpy(truth.astype(np.float32)).cuda(), width_e, SIZE, HEIGHT_MM)
observed_e = (observed_e + 0.02 * torch.randn(observed_e.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(0))).contiguous()
search("ellipsoid", grid_e, observed_e, width_e)
