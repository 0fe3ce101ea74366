"""The times of DESIGN.md section 21: depth_points (gsd_depth_points_count / _write) against a torch composition of the same
definition (`nonzero`, gathers, the same fp64 arithmetic) on rendered depth of section 17's mesh, the subdivision-6 icosphere
(81,920 triangles, radius 5 mm), B = 64 images of 320 x 427, object frame with normals and pixel indices, strides 1 and 2.
Device events, median of 10 after 3 warm-ups, the forms alternating in one process; the host clock (to device idle) beside them,
because the packed form and the composition both wait for one number from the device in the middle of the call.
usage (GPU box): PYTHONPATH=. python profiles/bench_depth_points.py [--b 64] [--subdivisions 6]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import mesh_depth_ref as R  # noqa: E402

from gelslim_depth_amd.contact_points import depth_points  # noqa: E402
from gelslim_depth_amd.mesh_depth import MeshGrid, render_depth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--b", type=int, default=64)
ap.add_argument("--subdivisions", type=int, default=6)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()

SIZE, HEIGHT_MM, RADIUS = (320, 427), 12.0, 5.0
H, W = SIZE
MPP = HEIGHT_MM / H
grid = MeshGrid(R.sphere(a.subdivisions, RADIUS, (1.0, -0.5, 0.25)), 1.0, "+y+z", "cuda")
print(f"{grid!r}")
rng = np.random.Generator(np.random.PCG64(0))
poses = torch.from_numpy((rng.uniform(-1, 1, (a.b, 3)) * np.array([1.5e-3, 1.5e-3, 3.0])).astype(np.float32)).cuda()
widths = torch.from_numpy((2 * (RADIUS - rng.uniform(0.5, 1.5, a.b))).astype(np.float32)).cuda()          # 0.5 .. 1.5 mm of indentation
depth = render_depth(grid, poses, widths, SIZE, HEIGHT_MM)
print(f"B = {a.b}, {H} x {W}: {int((depth < 0).sum())} contact pixels of {depth.numel()} ({100 * float((depth < 0).float().mean()):.2f} %)")


def composition(stride):
    """Section 21 in torch: object frame of plane '+y+z' (perp 0, unaligned y = axis 1, aligned z = axis 2, multiplier +1)."""
    o = stride // 2
    idx = torch.nonzero(depth[:, :, o::stride, o::stride] < 0)          # image, channel, row, column ascending; waits for the count
    b, ch, r, k = idx[:, 0], idx[:, 1], o + idx[:, 2] * stride, o + idx[:, 3] * stride
    d = depth[b, ch, r, k].double()

    def neighbour(dr, dk):
        rr, kk = r + dr, k + dk
        inside = (rr >= 0) & (rr < H) & (kk >= 0) & (kk < W)
        v = depth[b, ch, rr.clamp(0, H - 1), kk.clamp(0, W - 1)]
        return v.double(), inside & (v < 0)

    def diff(minus, plus):
        (vm, um), (vp, up) = minus, plus
        return torch.where(um & up, (vp - vm) / (2 * MPP), torch.where(up, (vp - d) / MPP, torch.where(um, (d - vm) / MPP, torch.zeros_like(d))))

    dx, dy = diff(neighbour(-1, 0), neighbour(1, 0)), diff(neighbour(0, -1), neighbour(0, 1))
    norm = torch.sqrt(dx * dx + dy * dy + 1.0)
    s = torch.where(ch == 1, 1.0, -1.0).double()
    x, y = MPP * (r.double() - 0.5 * H), MPP * (k.double() - 0.5 * W)
    g = widths.double()[b]
    u, v, q = s * x, y, s * (0.5 * g - d)
    th = poses[:, 2].double()
    cs, sn, a1, a2 = torch.cos(th)[b], torch.sin(th)[b], 1000.0 * poses[:, 0].double()[b], 1000.0 * poses[:, 1].double()[b]
    da, db = u - a1, v - a2
    points = torch.stack((q + grid.mid, cs * da + sn * db, cs * db - sn * da), dim=1).float()
    nu, nv = s * dx, dy
    normals = (torch.stack((s, cs * nu + sn * nv, cs * nv - sn * nu), dim=1) / norm.unsqueeze(1)).float()
    pixel = (((b * 2 + ch) * H + r) * W + k).int()
    return points, normals, pixel


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0), r


for stride in (1, 2):
    kw = dict(image_height_mm=HEIGHT_MM, stride=stride, frame="object", poses=poses, grid=grid, validate=False)
    n_max = int(depth_points(depth, widths, **kw).counts.sum(dim=1).max())
    forms = {"kernel, packed": lambda: depth_points(depth, widths, **kw),
             "kernel, padded": lambda: depth_points(depth, widths, max_points=n_max, **kw),
             "torch composition": lambda: composition(stride)}
    runs = {name: [] for name in forms}
    for rep in range(a.warmup + a.reps):
        for name, fn in forms.items():          # alternating
            ms = timed(fn)
            if rep >= a.warmup:
                runs[name].append(ms[:2])
    cloud, (points, normals, pixel) = forms["kernel, packed"](), composition(stride)
    same = torch.equal(cloud.pixel, pixel)
    worst = max(float((cloud.points - points).abs().max()), float((cloud.normals - normals).abs().max())) if same else float("nan")
    med = {}
    for name in forms:
        dev = med[name] = statistics.median(r[0] for r in runs[name])
        host = statistics.median(r[1] for r in runs[name])
        print(f"stride {stride} {name:17s}: {dev:.3f} ms (device events, min {min(r[0] for r in runs[name]):.3f} max "
              f"{max(r[0] for r in runs[name]):.3f}; {host:.3f} ms host clock to device idle); median of {a.reps} after {a.warmup}")
    print(f"stride {stride}: {cloud.points.shape[0]} points, at most {n_max} per image; pixel indices equal {same}, largest |difference| of "
          f"a component {worst:.2e}; composition / packed = {med['torch composition'] / med['kernel, packed']:.1f}, composition / padded = "
          f"{med['torch composition'] / med['kernel, padded']:.1f}")
