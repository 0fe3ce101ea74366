"""A/B of bit-identity between two builds of libgsd.so over render_depth, score_poses and score_poses_widths (DESIGN.md section 18:
whatever is done to the kernels behind them, no output may change by a bit): seeded inputs, the sha256 of every output compared
between the two libraries.  The cases: the three test meshes at 24 x 31, 40 x 53 and 80 x 106 with both channel
orders and pose senses, widths that include 0, one at which nothing touches, a refused one (validate=False: NaN), score_poses at
strides 1, 2 and 3 with two contact depths on noisy observations with a NaN and a -inf pixel, score_poses_widths on the same
observations, strides and contact depths at G = 1, 2, 3, 5 and 32 with a refused width in one column, and the subdivision-6
icosphere at 320 x 427.

usage (GPU box, repo root): python profiles/ab_mesh_pose_bits.py LIB_A LIB_B [--tree-a DIR] [--out profiles/mesh_pose_width_outputs_equal.txt]
--tree-a: the checkout whose gelslim_depth_amd package and tests/ helpers drive LIB_A (the parent commit's: its library lacks
the symbols that this tree's binding declares; it has to have the three functions, with these arguments).
Each library runs in a fresh child process of its own (GSD_LIB_PATH) under its own time limit; the second starts only if the
first succeeded.  Writes one line per case ("equal" / "DIFFER") and exits non-zero unless all are equal."""
import hashlib
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 180


def child(out_path):
    tree = os.environ.get("GSD_AB_TREE") or REPO
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import numpy as np
    import torch
    import mesh_depth_ref as R
    import mesh_pose_ref as P
    from gelslim_depth_amd.mesh_depth import MeshGrid, render_depth, score_poses, score_poses_widths
    lines = []

    def emit(case, t):
        torch.cuda.synchronize()
        lines.append(f"{case} {hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()}")

    def run(name, tri, sizes, n, p):
        grid = MeshGrid(tri, 1.0, P.PLANE, "cuda")
        rng = np.random.Generator(np.random.PCG64(7))
        g = P.contact_width(tri)
        poses = torch.from_numpy((rng.uniform(-1, 1, (n, 3)) * np.array([1.5e-3, 1.5e-3, 3.0])).astype(np.float32)).cuda()
        widths = torch.from_numpy((g + rng.uniform(-1.0, 0.5, n)).astype(np.float32)).cuda()
        widths[0], widths[1], widths[2] = 0.0, 1.0e3, -1.0
        cand = (poses[:2, None, :] + torch.from_numpy((rng.uniform(-1, 1, (2, p, 3)) * np.array([1e-3, 1e-3, 0.4])).astype(np.float32)).cuda())
        for size in sizes:
            for flip, invert in ((False, False), (True, True)):
                img = render_depth(grid, poses, widths, size, 12.0, 0.0, flip, invert, validate=False)
                emit(f"render_depth {name} {size[0]}x{size[1]} N={n} flip={flip} invert={invert}", img)
                seen = img[3:5] + torch.from_numpy(rng.normal(0, 0.05, (2, 2, *size)).astype(np.float32)).cuda()
                seen[0, 1, 10, 13], seen[1, 0, 7, 16] = float("nan"), float("-inf")
                for w2 in (widths[3:5].contiguous(), widths[1:3].contiguous()):
                    for stride, contact in ((1, 0.0), (2, 0.05), (3, 0.0)):
                        rows = score_poses(grid, seen.contiguous(), cand.contiguous(), w2, 12.0, 0.1, flip, invert, stride, contact,
                                           validate=False)
                        emit(f"score_poses {name} {size[0]}x{size[1]} P={p} widths {w2.tolist()} stride {stride} contact {contact} "
                             f"flip={flip} invert={invert}", rows)
                for g_count in (1, 2, 3, 5, 32):          # the same observations; one refused column (G = 1: one refused observation)
                    wg = widths[3:5, None] + torch.linspace(-0.6, 0.4, g_count, device="cuda")[None, :]
                    if g_count > 1:
                        wg[:, g_count // 2] = -1.0
                    else:
                        wg[1, 0] = -1.0
                    for stride, contact in ((1, 0.0), (2, 0.05), (3, 0.0)):
                        rows = score_poses_widths(grid, seen.contiguous(), cand.contiguous(), wg.contiguous(), 12.0, 0.1, flip, invert,
                                                  stride, contact, validate=False)
                        emit(f"score_poses_widths {name} {size[0]}x{size[1]} P={p} G={g_count} stride {stride} contact {contact} "
                             f"flip={flip} invert={invert}", rows)

    for name in ("lprism", "sphere4", "ellipsoid"):
        run(name, P.MESHES[name](), ((24, 31), (40, 53), (80, 106)), 8, 37)
    run("icosphere6", R.sphere(6, 5.0, (1.0, -0.5, 0.25)), ((320, 427),), 6, 64)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def run_child(lib_path, out_path, tree=None):
    env = dict(os.environ, GSD_LIB_PATH=os.path.abspath(lib_path), GSD_AB_TREE=os.path.abspath(tree or REPO))
    subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", out_path],
                   env=env, check=True, cwd=REPO)
    with open(out_path) as f:
        return [l.rstrip("\n").rsplit(" ", 1) for l in f if l.strip()]


def main(argv):
    if len(argv) == 3 and argv[1] == "--child":
        return child(argv[2])
    out = os.path.join(REPO, "profiles", "mesh_pose_width_outputs_equal.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    tree_a = None
    if "--tree-a" in argv:
        i = argv.index("--tree-a")
        tree_a = argv[i + 1]
        del argv[i:i + 2]
    if len(argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        a = run_child(argv[1], os.path.join(tmp, "a"), tree_a)      # check=True: a failure of the first run stops here, before the second starts
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
