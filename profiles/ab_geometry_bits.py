"""A/B of bit-identity between two builds of libgsd.so over the geometry functions whose kernels share gsd_block_prims.h,
gsd_lm_step.h and gsd_cell_lists.h: seeded inputs, the sha256 of every output compared between the two
libraries.  The cases:
  MeshGrid / MeshVolume  cells[2 : 2 + ncells + 1] (the starts) and the lists sorted within each cell, on the three test meshes at
                         their default cells and on the subdivision-6 icosphere at its default cells and at half of them
  depth_points           packed and padded, object frame with normals and pixels, on a batch of more blocks than one scan pass
  contact_patches        labels, counts and statistics at connectivity 4 and 8, min_area 1 and 4, on noisy rendered depth
  extract_surface        triangles, cells and count on the 106 x 104 x 102 field of the multi-pass test, packed and padded
  refine_pose            pose, width, cost, row, trace, accepted and last_step on the test meshes, width fixed and fitted, two starts
  register_cloud         matrices, cost, rms, rows, trace, accepted and last_step, plane and point kind, one start and three

usage (GPU box, repo root): python profiles/ab_geometry_bits.py LIB_A LIB_B [--out profiles/geometry_prims_outputs_equal.txt]
Both libraries are driven by this tree's Python (the ABI is the same).  Each runs in a fresh child process of its own
(GSD_LIB_PATH) under its own time limit; the second starts only if the first succeeded.  Writes one line per output ("equal" /
"DIFFER") and exits non-zero unless all are equal."""
import hashlib
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 240


def child(out_path):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import torch
    import mesh_closest_ref as M
    import mesh_depth_ref as R
    import mesh_pose_ref as P
    from gelslim_depth_amd import _lib as L
    from gelslim_depth_amd.contact_patches import contact_patches
    from gelslim_depth_amd.contact_points import depth_points
    from gelslim_depth_amd.mesh_depth import MeshGrid, refine_pose, render_depth
    from gelslim_depth_amd.mesh_register import MeshVolume, register_cloud
    from gelslim_depth_amd.touch_fusion import TouchVolume, extract_surface
    dev = "cuda:0"
    lines = []

    def emit(case, t):
        torch.cuda.synchronize()
        lines.append(f"{case} {hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()}")

    def emit_lists(case, owner, ncells):
        start = owner.cells[2:2 + ncells + 1]
        emit(f"{case} starts", start)
        cell_of = torch.repeat_interleave(torch.arange(ncells, device=dev), torch.diff(start).long())
        n = int(start[-1])
        emit(f"{case} lists sorted", torch.sort(cell_of * (1 << 24) + owner.list[:n].long()).values)

    meshes = {name: P.MESHES[name]() for name in ("lprism", "sphere4", "ellipsoid")}
    ico = R.sphere(6, 5.0, (1.0, -0.5, 0.25))
    for name, tri, mults in [(k, v, (1.0,)) for k, v in meshes.items()] + [("icosphere6", ico, (1.0, 0.5))]:
        for mult in mults:
            g = MeshGrid(tri, 1.0, P.PLANE, dev)
            g = g if mult == 1.0 else MeshGrid(tri, 1.0, P.PLANE, dev, cell_mm=g.cell_mm * mult)
            emit_lists(f"MeshGrid {name} cells x {mult:g} ({g.grid.nx} x {g.grid.ny}, {g.pairs} pairs)", g, g.grid.nx * g.grid.ny)
            v = MeshVolume(tri, 1.0, dev)
            v = v if mult == 1.0 else MeshVolume(tri, 1.0, dev, v.cell_mm * mult)
            emit_lists(f"MeshVolume {name} cells x {mult:g} ({v.volume.nx} x {v.volume.ny} x {v.volume.nz}, {v.pairs} pairs)", v,
                       v.volume.nx * v.volume.ny * v.volume.nz)

    # rendered depth of the ellipsoid: five images, one with no contact
    rng = np.random.Generator(np.random.PCG64(17))
    tri = meshes["ellipsoid"]
    grid = MeshGrid(tri, 1.0, P.PLANE, dev)
    g0 = P.contact_width(tri)
    size = (40, 53)
    poses = torch.from_numpy((rng.uniform(-1, 1, (5, 3)) * np.array([1.0e-3, 1.0e-3, 3.0])).astype(np.float32)).to(dev)
    widths = torch.from_numpy((g0 + rng.uniform(-1.0, -0.2, 5)).astype(np.float32)).to(dev)
    widths[4] = 1.0e3
    depth = render_depth(grid, poses, widths, size, 12.0)
    per = -(-(size[0] * size[1]) // L.GSD_DEPTH_POINTS_BLOCK)
    big = L.GSD_DEPTH_POINTS_SCAN_PASS // (2 * per) + 17          # more blocks than one pass of the scan
    pick = torch.arange(big, device=dev) % 5
    for stride in (1, 2):
        for cap in (None, 300):
            c = depth_points(depth[pick].contiguous(), widths[pick].contiguous(), 12.0, stride=stride, frame="object",
                             poses=poses[pick].contiguous(), grid=grid, max_points=cap)
            for field in ("points", "normals", "pixel", "counts"):
                emit(f"depth_points B={big} stride {stride} max_points {cap} {field}", getattr(c, field))

    noisy = depth + torch.from_numpy(rng.normal(0, 0.02, tuple(depth.shape)).astype(np.float32)).to(dev)
    noisy = torch.cat([noisy] * 8).contiguous()
    for conn in (4, 8):
        for min_area in (1, 4):
            p = contact_patches(noisy, 0.01, conn, min_area, 16)
            for field in ("labels", "counts", "stats"):
                emit(f"contact_patches connectivity {conn} min_area {min_area} {field}", getattr(p, field))

    dims, h, origin = (106, 104, 102), 0.125, (-6.625, -6.5, -6.375)
    ax = [origin[a] + h * torch.arange(dims[a], device=dev, dtype=torch.float64) for a in range(3)]
    f = torch.sqrt((ax[0][None, None, :] - 0.013) ** 2 + (ax[1][None, :, None] + 0.021) ** 2 + (ax[2][:, None, None] - 0.007) ** 2) - 4.0
    vol = TouchVolume(origin, h, dims, 1.0, device=dev)
    vol.acc.copy_(f.to(torch.float32))
    vol.weight.fill_(1.0)
    for cap in (None, 60000):
        s = extract_surface(vol, max_triangles=cap, cells=True)
        for field in ("triangles", "cell", "count"):
            emit(f"extract_surface 106x104x102 max_triangles {cap} {field}", getattr(s, field))

    for name, tri in meshes.items():
        grid = MeshGrid(tri, 1.0, P.PLANE, dev)
        g0 = P.contact_width(tri)
        truth = torch.tensor([[0.3e-3, -0.2e-3, 0.4], [-0.4e-3, 0.1e-3, -1.1]], dtype=torch.float32, device=dev)
        w = torch.tensor([g0 - 0.8, g0 - 0.5], dtype=torch.float32, device=dev)
        seen = render_depth(grid, truth, w, size, 12.0)
        init = truth[:, None, :] + torch.tensor([[1e-4, -1e-4, 0.02], [-2e-4, 1e-4, -0.03]], dtype=torch.float32, device=dev)[None]
        for fit in (False, True):
            r = refine_pose(grid, seen, w + (0.1 if fit else 0.0), init.contiguous(), iterations=8, fit_width=fit)
            for field in ("pose", "width", "cost", "normal_row", "trace", "accepted", "last_step"):
                emit(f"refine_pose {name} fit_width={fit} {field}", getattr(r, field))

    for name in ("ellipsoid", "l_prism"):
        tri, p = M.case_cloud(name)
        v = MeshVolume(M.case_mesh(name), 1.0, dev)
        pts = torch.from_numpy(p).to(dev)
        starts = torch.eye(4, dtype=torch.float64, device=dev).repeat(3, 1, 1)
        starts[1, 0, 3], starts[2, 1, 3] = 0.3, -0.2
        for kind in ("plane", "point"):
            for init in (None, starts):
                r = register_cloud(v, pts, init=init, iterations=12, kind=kind, max_distance_mm=None if kind == "plane" else 2.0)
                for field in ("matrices", "cost", "rms", "rows", "trace", "accepted", "last_step"):
                    emit(f"register_cloud {name} {kind} starts {1 if init is None else 3} {field}", getattr(r, field))
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def run_child(lib_path, out_path):
    env = dict(os.environ, GSD_LIB_PATH=os.path.abspath(lib_path))
    subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", out_path],
                   env=env, check=True, cwd=REPO)
    with open(out_path) as f:
        return [l.rstrip("\n").rsplit(" ", 1) for l in f if l.strip()]


def main(argv):
    if len(argv) == 3 and argv[1] == "--child":
        return child(argv[2])
    out = os.path.join(REPO, "profiles", "geometry_prims_outputs_equal.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    if len(argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        a = run_child(argv[1], os.path.join(tmp, "a"))      # check=True: a failure of the first run stops here, before the second starts
        b = run_child(argv[2], os.path.join(tmp, "b"))
    assert [c for c, _ in a] == [c for c, _ in b], "the two runs did not produce the same cases"
    differ = 0
    with open(out, "w") as f:
        for (case, ha), (_, hb) in zip(a, b):
            differ += ha != hb
            f.write(f"{'equal ' if ha == hb else 'DIFFER'}  {case}  {ha[:16]}" + ("" if ha == hb else f" != {hb[:16]}") + "\n")
    print(f"{len(a)} cases, {differ} differ -> {out}")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main(list(sys.argv))
