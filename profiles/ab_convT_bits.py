"""A/B of bit-identity between two builds of libgsd.so over the fp32 ConvTranspose2d(k2,s2) entry points: gsd_convT2x2,
gsd_convT2x2_dgrad_as in weight layout modes 7 and 3, gsd_convT2x2_dgrad under both values of GSD_CONVT_DG_DMA,
gsd_convT2x2_dgrad_bnrelu (dz and its partial rows), gsd_convT2x2_wgrad (dW and db) and the weight images of gsd_weight_layout
modes 3, 6 and 7: fixed seeded inputs, the sha256 of every output buffer compared between the two libraries.  The shapes:
CONVT_CASES of tests/tile_cases.py, the shapes of test_convT_fwd_bwd (tests/test_gpu_ops.py) and the four decoder levels at batch 8.

usage (GPU box, repo root): python profiles/ab_convT_bits.py LIB_A LIB_B [--out profiles/ab_convT_bits.txt]
Each library runs in a fresh child process of its own (GSD_LIB_PATH) under its own time limit; the second starts only if the
first succeeded.  Writes one line per case ("equal" / "DIFFER") and exits non-zero unless all are equal."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 180
GUARD = 8       # floats of NaN around every operand: 16-byte alignment kept, and the slack dy declares is there

OPS_CONVT = [(2, 8, 4, 5), (1, 128, 20, 26), (2, 36, 7, 9), (3, 24, 5, 53), (1, 264, 3, 2), (2, 16, 1, 1)]   # (n, ci, h, w), co = ci / 2
LEVELS = [(8, 20, 26, 1024, 512), (8, 40, 53, 512, 256), (8, 80, 106, 256, 128), (8, 160, 213, 128, 64)]   # (n, h, w, ci, co)


def child(out_path):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import tile_cases as T
    from gelslim_depth_amd import _lib as L
    lib, check = L.lib, L.check
    st = L.stream_ptr()
    cpu = torch.Generator().manual_seed(20242)
    lines = []

    def tensor(shape, scale=1.0):
        """Seeded values in a buffer with GUARD floats of NaN either side."""
        numel = 1
        for s in shape:
            numel *= s
        flat = torch.full((GUARD + numel + GUARD,), float("nan"), device="cuda")
        t = flat[GUARD:GUARD + numel].view(shape)
        t.copy_(torch.randn(shape, generator=cpu) * scale)
        return t

    def nan(*shape):
        return torch.full(shape, float("nan"), device="cuda")

    def emit(case, *tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().contiguous().cpu().numpy().tobytes())
        lines.append(f"{case} {h.hexdigest()}")

    def image(mode, w, co, ci):
        wt = nan(lib.gsd_weight_layout_size(mode, co, ci))
        check(lib.gsd_weight_layout(mode, w.data_ptr(), co, ci, wt.data_ptr(), st), f"weight_layout {mode}")
        return wt

    for (n, h, w, ci, co) in T.CONVT_CASES + [(n, h, w, ci, ci // 2) for (n, ci, h, w) in OPS_CONVT] + LEVELS:
        tag = f"{n}x{h}x{w} k{ci} m{co}"
        bn = ci != 36          # as the tests: a deferred BatchNorm + ReLU source, a plain one for Cin = 36
        raw = tensor((n, ci, h, w))
        sc, sh = ((torch.rand(ci, generator=cpu) + 0.5).cuda(), (torch.randn(ci, generator=cpu) * 0.3).cuda()) if bn else (None, None)
        wgt, bias = tensor((ci, co, 2, 2), scale=ci ** -0.5), tensor((co,))
        dy = tensor((n, co, 2 * h, 2 * w))
        sx, sdy = L.make_src(raw, sc, sh, relu=bn), L.make_src(dy, slack=GUARD)
        img = {m: image(m, wgt, co, ci) for m in (3, 6, 7)}
        for m in (3, 6, 7):
            emit(f"weight image mode {m} {tag}", img[m])
        # forward
        y = nan(n, co, 2 * h, 2 * w)
        check(lib.gsd_convT2x2(C.byref(sx), img[6].data_ptr(), bias.data_ptr(), ci, co, C.byref(L.make_dst(y)), n, h, w, st), "convT2x2")
        emit(f"convT2x2 {tag}{' bn' if bn else ''}", y)
        # dX with the image's mode stated, then derived under both values of the switch
        for m in (7, 3):
            dx = nan(n, ci, h, w)
            check(lib.gsd_convT2x2_dgrad_as(m, C.byref(sdy), img[m].data_ptr(), ci, co, C.byref(L.make_dst(dx)), n, h, w, st), "dgrad_as")
            emit(f"convT2x2_dgrad_as mode {m} {tag}", dx)
        for env in ("1", "0"):
            os.environ["GSD_CONVT_DG_DMA"] = env
            m = lib.gsd_convT2x2_dgrad_layout(C.byref(sdy), ci, co, n, h, w)
            dx = nan(n, ci, h, w)
            check(lib.gsd_convT2x2_dgrad(C.byref(sdy), img[m].data_ptr(), ci, co, C.byref(L.make_dst(dx)), n, h, w, st), "dgrad")
            emit(f"convT2x2_dgrad GSD_CONVT_DG_DMA={env} layout {m} {tag}", dx)
            del os.environ["GSD_CONVT_DG_DMA"]
        # dX fused with the backward of the relu(bn(raw)) below: dz and the partial rows
        mean, invstd = (torch.randn(ci, generator=cpu) * 0.2).cuda(), (torch.rand(ci, generator=cpu) * 1.5 + 0.5).cuda()
        bsc, bsh = (sc, sh) if bn else ((torch.rand(ci, generator=cpu) + 0.5).cuda(), (torch.randn(ci, generator=cpu) * 0.3).cuda())
        rows = lib.gsd_convT2x2_dgrad_bnrelu_partial_rows(C.byref(sdy), ci, co, n, h, w)
        dz, part = nan(n, ci, h, w), nan(rows, 2 * (-(-ci // 64) * 64))
        check(lib.gsd_convT2x2_dgrad_bnrelu(C.byref(sdy), img[7].data_ptr(), ci, co, C.byref(L.make_dst(dz)), raw.data_ptr(), bsc.data_ptr(),
                                            bsh.data_ptr(), mean.data_ptr(), invstd.data_ptr(), part.data_ptr(), n, h, w, st), "dgrad_bnrelu")
        emit(f"convT2x2_dgrad_bnrelu rows {rows} {tag}", dz, part)
        # dW and db
        need = lib.gsd_convT2x2_wgrad_workspace(n, h, w, ci, co)
        ws, dw, db = nan(need), nan(ci, co, 2, 2), nan(co)
        check(lib.gsd_convT2x2_wgrad(C.byref(sx), C.byref(sdy), ci, co, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need, n, h, w, st), "wgrad")
        emit(f"convT2x2_wgrad workspace {need} {tag}{' bn' if bn else ''}", dw, db)

    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def run_child(lib_path, out_path):
    env = dict(os.environ, GSD_LIB_PATH=os.path.abspath(lib_path))
    subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", out_path],
                   env=env, check=True, cwd=REPO)
    with open(out_path) as f:
        return [l.rstrip("\n").rsplit(" ", 1) for l in f if l.strip()]


def main(argv):
    if len(argv) == 3 and argv[1] == "--child":
        return child(argv[2])
    out = os.path.join(REPO, "profiles", "ab_convT_bits.txt")
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
