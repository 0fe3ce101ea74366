"""A/B of bit-identity between two builds of libgsd.so over the fp32 weight-gradient entry points (gsd_conv3x3_wgrad in its three
forms, gsd_convT2x2_wgrad with its bias gradient, gsd_sum_planes): fixed seeded inputs, the sha256 of every output buffer compared
between the two libraries.  The cases: every WG_CASES entry of tests/tile_cases.py under its knobs, the shapes of
test_conv3x3_wgrad and test_conv3x3_wgrad_two_segments (tests/test_gpu_ops.py), four layer-sized launches, CONVT_CASES and the
test_convT_fwd_bwd shapes, gsd_sum_planes at K = 1 and K = 12.

usage (GPU box, repo root): python profiles/ab_wgrad_bits.py LIB_A LIB_B [--out profiles/ab_wgrad_bits.txt]
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
GUARD = 8       # floats around every operand: 16-byte alignment kept, and the slack a case declares is there

OPS_WGRAD = [(2, 5, 7, 9, 11), (1, 64, 64, 21, 29), (2, 20, 130, 6, 70), (1, 3, 16, 40, 53), (2, 16, 16, 1, 1), (1, 16, 32, 2, 3),
             (1, 32, 16, 3, 70), (3, 16, 200, 1, 130), (2, 5, 130, 9, 11), (2, 40, 8, 9, 11)]                # (n, ci, co, h, w)
OPS_TWO_SEGMENTS = [(2, 6, 5, 9, 9, 11, 6, 8), (1, 16, 16, 32, 21, 29, 20, 28), (2, 64, 64, 64, 13, 19, 12, 18),
                    (1, 24, 40, 130, 10, 37, 8, 36)]                                                       # (n, c0, c1, co, h, w, uh, uw)
LAYERS = [(2, 64, 64, 37, 53, False), (1, 128, 64, 80, 106, True), (2, 32, 96, 21, 19, False), (4, 256, 128, 40, 53, False)]
OPS_CONVT = [(2, 8, 4, 5), (1, 128, 20, 26), (2, 36, 7, 9), (3, 24, 5, 53), (1, 264, 3, 2), (2, 16, 1, 1)]   # (n, ci, h, w), co = ci / 2


def child(out_path):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import tile_cases as T
    from gelslim_depth_amd import _lib as L
    lib, check = L.lib, L.check
    st = L.stream_ptr()
    cpu = torch.Generator().manual_seed(20241)
    lines = []

    def tensor(shape, pitch=None):
        """Seeded (n, c, h, w) values in a buffer with row pitch `pitch` (pad columns 0) and GUARD floats of NaN either side."""
        n, c, h, w = shape
        p = pitch or w
        flat = torch.full((GUARD + n * c * h * p + GUARD,), float("nan"), device="cuda")
        body = flat[GUARD:GUARD + n * c * h * p].view(n, c, h, p)
        body.zero_()
        t = body[..., :w]
        t.copy_(torch.randn(shape, generator=cpu))
        return t

    def affine(c):
        return (torch.rand(c, generator=cpu) + 0.5).cuda(), (torch.randn(c, generator=cpu) * 0.3).cuda()

    def emit(case, *tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().contiguous().cpu().numpy().tobytes())
        lines.append(f"{case} {h.hexdigest()}")

    def wgrad(case, n, h, w, segs, dy, co, env=()):
        """gsd_conv3x3_wgrad of the gsd_src segments `segs` under the knobs `env`; the form it takes is part of the case's name."""
        for k, v in env:
            os.environ[k] = str(v)
        ci = sum(s.C for s in segs)
        src, sdy = L.src_array(segs), L.make_src(dy)
        form = lib.gsd_conv3x3_wgrad_form(src, len(segs), C.byref(sdy), ci, co, n, h, w)
        need = lib.gsd_conv3x3_wgrad_workspace(n, h, w, ci, co)
        ws = torch.full((max(need, 64),), float("nan"), device="cuda")
        dw = torch.full((co, ci, 3, 3), float("nan"), device="cuda")
        check(lib.gsd_conv3x3_wgrad(src, len(segs), C.byref(sdy), ci, co, dw.data_ptr(), ws.data_ptr(), need, n, h, w, st), case)
        emit(f"{case} form{form}" + "".join(f" {k}={v}" for k, v in env), dw)
        for k, _ in env:
            del os.environ[k]

    # ---- gsd_conv3x3_wgrad: the tile-form cases (operand layouts as tests/test_gpu_tile_forms_fp64.py builds them)
    for c in T.WG_CASES:
        n, h, w = c.n, c.h, c.w
        raw0 = tensor((n, c.c0, h, w))
        sc, sh = affine(c.c0) if c.bn else (None, None)
        segs = [L.make_src(raw0, sc, sh, relu=c.bn, slack=c.slack)]
        if c.c1:
            oh, ow = (1 if h >= 3 else 0), (1 if w >= 3 else 0)
            up = tensor((n, c.c1, h - oh - (1 if h >= 4 else 0), w - ow - (1 if w >= 4 else 0)))
            segs.append(L.make_src(up, off=(oh, ow), slack=c.slack))
        dy = tensor((n, c.co, h, w), pitch=(w + 3) // 4 * 4 if c.pitched else None)
        wgrad(f"wgrad tile case {n}x{h}x{w} c{c.c0}+{c.c1} m{c.co} {'pitched' if c.pitched else 'flat'} slack{c.slack}"
              f"{' bn' if c.bn else ''}", n, h, w, segs, dy, c.co, c.env)
    # ---- the shapes of test_conv3x3_wgrad (one deferred-BatchNorm segment, flat dy, no slack) ...
    for (n, ci, co, h, w) in OPS_WGRAD:
        sc, sh = affine(ci)
        wgrad(f"wgrad {n}x{ci}x{co}x{h}x{w} bn", n, h, w, [L.make_src(tensor((n, ci, h, w)), sc, sh, relu=True)], tensor((n, co, h, w)), co)
    # ---- ... and of test_conv3x3_wgrad_two_segments (a deferred-BatchNorm skip and a plain, smaller segment at its F.pad offset)
    for (n, c0, c1, co, h, w, uh, uw) in OPS_TWO_SEGMENTS:
        sc, sh = affine(c0)
        segs = [L.make_src(tensor((n, c0, h, w)), sc, sh, relu=True), L.make_src(tensor((n, c1, uh, uw)), off=((h - uh) // 2, (w - uw) // 2))]
        wgrad(f"wgrad two segments {n}x{c0}+{c1}x{co}x{h}x{w} up {uh}x{uw}", n, h, w, segs, tensor((n, co, h, w)), co)
    # ---- layer-sized launches: slack around the activation, dy flat
    for (n, ci, co, h, w, plain) in LAYERS:
        sc, sh = (None, None) if plain else affine(ci)
        wgrad(f"wgrad layer {n}x{ci}x{co}x{h}x{w}{' plain' if plain else ' bn'}", n, h, w,
              [L.make_src(tensor((n, ci, h, w)), sc, sh, relu=not plain, slack=L.SLACK)], tensor((n, co, h, w)), co)

    # ---- gsd_convT2x2_wgrad: dW and dbias
    for (n, h, w, ci, co) in T.CONVT_CASES + [(n, h, w, ci, ci // 2) for (n, ci, h, w) in OPS_CONVT]:
        bn = ci != 36
        sc, sh = affine(ci) if bn else (None, None)
        x, dy = tensor((n, ci, h, w)), tensor((n, co, 2 * h, 2 * w))
        sx, sdy = L.make_src(x, sc, sh, relu=bn), L.make_src(dy)
        need = lib.gsd_convT2x2_wgrad_workspace(n, h, w, ci, co)
        ws = torch.full((need,), float("nan"), device="cuda")
        dw, db = torch.full((ci, co, 2, 2), float("nan"), device="cuda"), torch.full((co,), float("nan"), device="cuda")
        check(lib.gsd_convT2x2_wgrad(C.byref(sx), C.byref(sdy), ci, co, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need, n, h, w, st),
              "convT2x2_wgrad")
        emit(f"convT wgrad {n}x{h}x{w} k{ci} m{co}{' bn' if bn else ''}", dw, db)

    # ---- gsd_sum_planes: the 1024-thread form (K <= 8) and the 256-thread one
    for K in (1, 12):
        x = torch.randn((3, K, 37 * 53), generator=cpu).cuda()
        out, ws = torch.full((K,), float("nan"), device="cuda"), torch.zeros(K * 64, device="cuda")
        check(lib.gsd_sum_planes(x.data_ptr(), 3, K, 37 * 53, out.data_ptr(), ws.data_ptr(), st), "sum_planes")
        emit(f"sum_planes K{K}", out)

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
    out = os.path.join(REPO, "profiles", "ab_wgrad_bits.txt")
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
