"""Times of closest_points, icp_rows and register_cloud against torch compositions of the same query.

    python profiles/bench_closest_points.py [--out profiles/closest_points_times.txt]

Meshes: `marble` (tests/golden/meshes, 6,440 triangles) and the icosphere of 81,920 triangles, radius 10 mm.  Clouds: 10^4 and
2.6 * 10^6 surface samples with 0.05 mm of noise, shuffled or sorted along x then y (a depth_points cloud is ordered by row and
column; the shuffled one is the worst case for the walk).  Device events, the median of 10 calls after 3 warm-ups.

Compared with
  region: the same region method in torch fp64 over chunked N x T pairs (exact, the result is checked against closest_points);
          only for the 10^4 clouds -- at 2.6 * 10^6 points it would run for minutes;
  cdist:  torch.cdist to the mesh's unique VERTICES in fp32, chunked, min over the vertices: not the answer (a vertex is not the
          nearest surface point), the floor of what a composition that forms N x T distances can cost."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

DEV = "cuda:0"


def timed(fn, warm=3, runs=10):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def region_torch(tri, pts, pairs=1 << 23):
    """(triangle, d2) of every point by the region method over all N x T pairs, fp64, in chunks of about `pairs` pairs."""
    a, b, c = (tri[:, k].unsqueeze(0) for k in range(3))
    ab, ac = b - a, c - a
    dot = lambda u, w: (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]
    ids, best = [], []
    step = max(1, pairs // tri.shape[0])
    for lo in range(0, pts.shape[0], step):
        p = pts[lo:lo + step].double().unsqueeze(1)
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e1, e2 = d4 - d3, d5 - d6
        s = (va + vb) + vc
        x = (a + (vb / s).unsqueeze(-1) * ab) + (vc / s).unsqueeze(-1) * ac
        for cond, val in reversed((((d1 <= 0) & (d2 <= 0), a.expand_as(x)), ((d3 >= 0) & (d4 <= d3), b.expand_as(x)),
                                   ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3)).unsqueeze(-1) * ab),
                                   ((d6 >= 0) & (d5 <= d6), c.expand_as(x)),
                                   ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6)).unsqueeze(-1) * ac),
                                   ((va <= 0) & (e1 >= 0) & (e2 >= 0), b + (e1 / (e1 + e2)).unsqueeze(-1) * (c - b)))):
            x = torch.where(cond.unsqueeze(-1), val, x)
        r = p - x
        dd = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        m = dd.min(dim=1)
        ids.append(m.indices)
        best.append(m.values)
    return torch.cat(ids), torch.cat(best)


def cdist_floor(verts, pts, pairs=1 << 27):
    out = []
    step = max(1, pairs // verts.shape[0])
    for lo in range(0, pts.shape[0], step):
        out.append(torch.cdist(pts[lo:lo + step], verts).min(dim=1).values)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "closest_points_times.txt"))
    ap.add_argument("--no-compositions", action="store_true", help="skip the torch compositions (region, cdist) and the large clouds")
    args = ap.parse_args()
    import mesh_depth_ref as R
    from cell_list_phases import build_phases
    from gelslim_depth_amd.mesh_depth import read_stl
    from gelslim_depth_amd.mesh_register import MeshVolume, closest_points, icp_rows, register_cloud
    meshes = {"marble": (read_stl(os.path.join(os.path.dirname(HERE), "tests", "golden", "meshes", "marble.stl")), 1000.0),
              "icosphere 81,920": (np.float32(R.icosphere(6, 10.0)), 1.0)}
    lines = [f"closest_points against torch compositions, {torch.cuda.get_device_name(0)}; ms, median of 10 after 3 warm-ups",
             f"{'mesh':18s} {'cells':>14s} {'pairs':>9s} {'points':>9s} {'order':>8s} {'closest':>9s} {'icp_rows':>9s} {'region':>9s} "
             f"{'cdist':>9s} {'Mpoints/s':>10s}"]
    for name, (tri, scale) in meshes.items():
        rng = np.random.Generator(np.random.PCG64(1))
        vol = MeshVolume(tri, scale, DEV)
        for mult in (1.0, 0.5):      # the default cells and a grid twice as fine
            v = MeshVolume(tri, scale, DEV, vol.cell_mm * mult)
            count_ms, fill_ms = build_phases(lambda: MeshVolume(tri, scale, DEV, vol.cell_mm * mult), "gsd_mesh_volume")
            lines.append(f"{name:18s} cell lists, cells x {mult:g} ({v.volume.nx * v.volume.ny * v.volume.nz} cells, {v.pairs} pairs): "
                         f"count + scan {count_ms:.4f} ms, fill {fill_ms:.4f} ms")
            print(lines[-1], flush=True)
        tri64 = (vol.tri.view(-1, 3, 3)).double()
        verts = torch.unique(vol.tri.view(-1, 3), dim=0)
        for n in (10 ** 4,) if args.no_compositions else (10 ** 4, 2600000):
            cloud = R.sample_surface(np.float64(tri) * scale, n, seed=3) + rng.normal(0.0, 0.05, (n, 3))
            for order in ("shuffled", "sorted"):
                if order == "sorted":
                    cloud = cloud[np.lexsort((cloud[:, 1], np.round(cloud[:, 0] / 0.3)))]
                pts = torch.from_numpy(np.float32(cloud)).to(DEV)
                out = closest_points(vol, pts)
                t_closest = timed(lambda: closest_points(vol, pts, out=out))
                eye = torch.eye(4, dtype=torch.float64, device=DEV)
                t_rows = timed(lambda: icp_rows(vol, pts, eye))
                t_region = float("nan")
                if n <= 10 ** 4 and not args.no_compositions:
                    ids, d2 = region_torch(tri64, pts)
                    worst = float(((d2 - out.sq_distance).abs() / out.sq_distance.clamp_min(1e-300)).max())
                    lines.append(f"  region method against closest_points, {n} points: {int((d2 != out.sq_distance).sum())} d^2 differ in bits, "
                                 f"largest relative gap {worst:.2e}, {int((ids != out.triangle).sum())} ids differ (torch.min keeps no id rule)")
                    t_region = timed(lambda: region_torch(tri64, pts), warm=1, runs=3 if tri.shape[0] > 10000 else 10)
                t_cdist = float("nan") if args.no_compositions else timed(lambda: cdist_floor(verts, pts), warm=1, runs=3 if n > 10 ** 4 else 10)
                g = vol.volume
                lines.append(f"{name:18s} {f'{g.nx}x{g.ny}x{g.nz}':>14s} {vol.pairs:9d} {n:9d} {order:>8s} {t_closest:9.3f} {t_rows:9.3f} "
                             f"{t_region:9.3f} {t_cdist:9.3f} {n / t_closest / 1e3:10.2f}")
                print(lines[-1], flush=True)
        # one registration: 4,000 points, 20 iterations, one start and eight
        small = torch.from_numpy(np.float32(R.sample_surface(np.float64(tri) * scale, 4000, seed=5))).to(DEV) + 0.2
        for starts in (1, 8):
            init = torch.eye(4, dtype=torch.float64, device=DEV).repeat(starts, 1, 1)
            t = timed(lambda: register_cloud(vol, small, init=init, iterations=20))
            lines.append(f"{name:18s} register_cloud, 4,000 points, 20 iterations, {starts} start(s): {t:9.3f} ms")
            print(lines[-1], flush=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
