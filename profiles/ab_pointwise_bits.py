"""A/B of bit-identity between two builds of libgsd.so over the fp32 pointwise entry points (gsd_api.hip, gsd_weight_layout.hip,
gsd_bn.hip, gsd_head.hip, gsd_optim.hip, gsd_area_resize_affine in gsd_resize.hip): every entry point on fixed seeded inputs at
the smallest shapes that reach each of its kernel forms, the sha256 of every output buffer compared between the two libraries.

usage (GPU box, repo root): python profiles/ab_pointwise_bits.py LIB_A LIB_B [--out profiles/ab_pointwise_bits.txt]
Each library runs in a fresh child process of its own (GSD_LIB_PATH) under its own time limit; the second starts only if the
first succeeded.  Writes one line per case ("equal" / "DIFFER") and exits non-zero unless all are equal."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 120


def child(out_path):
    sys.path.insert(0, REPO)
    import torch
    from gelslim_depth_amd import _lib as L
    lib, check = L.lib, L.check
    st = L.stream_ptr()
    cpu = torch.Generator().manual_seed(20240)
    lines = []

    def randn(*shape, scale=1.0):
        return (torch.randn(shape, generator=cpu) * scale).cuda()

    def rand(lo, hi, *shape):
        return (torch.rand(shape, generator=cpu) * (hi - lo) + lo).cuda()

    def nan(*shape, dtype=torch.float32):
        return torch.full(shape, float("nan"), dtype=dtype, device="cuda")

    def emit(case, *tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().contiguous().cpu().numpy().tobytes())
        lines.append(f"{case} {h.hexdigest()}")

    def guard_of(state):
        """state: None (no guard), "raised" (words[0] == tick) or "clear"."""
        if state is None:
            return None, None
        words = torch.tensor([9 if state == "raised" else 4, 2], dtype=torch.int32, device="cuda")
        return words, L.make_guard(words, 9)

    # ---- gsd_api.hip
    a, b, o = randn(16, 4), randn(4, 16), nan(16, 16)
    check(lib.gsd_selftest_mfma(a.data_ptr(), b.data_ptr(), o.data_ptr(), st), "selftest")
    emit("selftest_mfma", o)

    # ---- gsd_weight_layout.hip: every mode at Co = 8, Ci = 5, and the batch entry with three jobs
    Co, Ci = 8, 5
    w = randn(Co * Ci * 9)          # (Co,Ci,3,3) of the conv modes; the ConvT modes read its first Ci*Co*4 floats
    for mode in (m for m in range(10) if m != 2):      # mode 2 is retired
        wt = nan(lib.gsd_weight_layout_size(mode, Co, Ci))
        check(lib.gsd_weight_layout(mode, w.data_ptr(), Co, Ci, wt.data_ptr(), st), f"weight_layout {mode}")
        emit(f"weight_layout mode{mode}", wt)
    jobs = (L.gsd_wl_job * 3)()
    outs = []
    for j, mode in zip(jobs, (8, 9, 4)):
        outs.append(nan(lib.gsd_weight_layout_size(mode, Co, Ci)))
        j.w, j.wt, j.mode, j.Co, j.Ci, j.reserved = w.data_ptr(), outs[-1].data_ptr(), mode, Co, Ci, 0
    check(lib.gsd_weight_layout_batch(jobs, 3, st), "weight_layout_batch")
    emit("weight_layout_batch modes 8,9,4", *outs)

    # ---- gsd_bn.hip: backward reduce / apply at N = 2, C = 5; 6x10 takes the 16-byte forms, 7x9 the scalar ones
    N, Cc = 2, 5
    sc, sh, mean, invstd = rand(0.3, 1.5, Cc), randn(Cc, scale=0.3), randn(Cc, scale=0.3), rand(0.5, 2.0, Cc)
    for (H, W) in ((6, 10), (7, 9)):
        raw, da, dpool = randn(N, Cc, H, W), randn(N, Cc, H, W), randn(N, Cc, H // 2, W // 2)
        rows = lib.gsd_bn_bwd_partial_rows(N, Cc, H, W)
        src = L.make_src(da)
        for mode, K in ((0, 1), (1, 1), (2, 1), (2, 2)):
            dout, wout = randn(N, K, H, W), randn(K, Cc, scale=0.125)
            dz, part = nan(N, Cc, H, W), torch.zeros(rows * 3 * Cc, device="cuda")
            check(lib.gsd_bn_bwd_reduce(mode, raw.data_ptr(), sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                        C.byref(src) if mode != 2 else None, dpool.data_ptr() if mode == 1 else None,
                                        dout.data_ptr() if mode == 2 else None, wout.data_ptr() if mode == 2 else None, K,
                                        dz.data_ptr(), part.data_ptr(), N, Cc, H, W, st), "bn_bwd_reduce")
            emit(f"bn_bwd_reduce {H}x{W} mode{mode} K{K}", dz, part)
        c1, c2 = randn(Cc, scale=0.1), randn(Cc, scale=0.1)
        dz = randn(N, Cc, H, W)
        outp = nan(N, Cc, H, 12)
        check(lib.gsd_bn_bwd_apply(dz.data_ptr(), raw.data_ptr(), sc.data_ptr(), mean.data_ptr(), invstd.data_ptr(), c1.data_ptr(),
                                   c2.data_ptr(), N, Cc, H, W, outp.data_ptr(), 12, st), "bn_bwd_apply pitched")
        emit(f"bn_bwd_apply {H}x{W} pitch12", outp, dz)
        check(lib.gsd_bn_bwd_apply(dz.data_ptr(), raw.data_ptr(), sc.data_ptr(), mean.data_ptr(), invstd.data_ptr(), c1.data_ptr(),
                                   c2.data_ptr(), N, Cc, H, W, None, 0, st), "bn_bwd_apply")
        emit(f"bn_bwd_apply {H}x{W} in place", dz)

    # ---- gsd_bn.hip: finalize, C = 20 (two blocks of the one-launch form, the second partial), 300 partial rows
    Cf, rows, mpad = 20, 300, 64
    part2 = randn(rows, 2 * mpad)
    part2[:, mpad:] = part2[:, mpad:].abs() * 3 + 1
    gamma, beta = rand(0.5, 1.5, Cf), randn(Cf, scale=0.3)
    count = float(rows * 16)
    for running in (True, False):
        for gstate in (None, "raised", "clear"):
            for form in ("one launch", "three launches"):
                rm, rv = (randn(Cf, scale=0.5), rand(0.5, 3.0, Cf)) if running else (None, None)
                o = [nan(Cf) for _ in range(4)]
                sums = torch.zeros(65 * 2 * Cf, dtype=torch.float64, device="cuda")
                words, guard = guard_of(gstate)
                tail = (count, gamma.data_ptr(), beta.data_ptr(), 1e-5, 0.1, L.ptr(rm), L.ptr(rv), o[0].data_ptr(), o[1].data_ptr(),
                        o[2].data_ptr(), o[3].data_ptr(), guard, st)
                if form == "one launch":
                    check(lib.gsd_bn_reduce_finalize(part2.data_ptr(), rows, mpad, Cf, sums.data_ptr(), *tail), form)
                else:
                    check(lib.gsd_bn_reduce_partials(part2.data_ptr(), rows, mpad, Cf, sums.data_ptr(), st), form)
                    check(lib.gsd_bn_finalize(sums.data_ptr(), Cf, *tail), form)
                emit(f"bn forward finalize, {form}, running {running}, guard {gstate}", *o, sums[:2 * Cf],
                     *([rm, rv] if running else []), *([words] if words is not None else []))
    cs_out = nan(7)
    sums = torch.zeros(65 * 2 * Cf, dtype=torch.float64, device="cuda")
    check(lib.gsd_partials_channel_sums(part2.data_ptr(), rows, mpad, Cf, 3, 7, cs_out.data_ptr(), sums.data_ptr(), st), "channel sums")
    emit("partials_channel_sums", cs_out, sums[:Cf])
    part3 = randn(rows, 3 * Cf, scale=1e-2)
    sg = torch.randn(3 * Cf, generator=cpu, dtype=torch.float64).cuda()
    for layout in ("reduce", "epilogue"):
        p, lm = (part3, 0) if layout == "reduce" else (part2, mpad)
        o = [nan(Cf) for _ in range(5)]
        sums = torch.zeros(65 * 3 * Cf, dtype=torch.float64, device="cuda")
        check(lib.gsd_bn_bwd_reduce_finalize(p.data_ptr(), rows, lm, Cf, sums.data_ptr(), count, o[0].data_ptr(), o[1].data_ptr(),
                                             o[2].data_ptr() if layout == "reduce" else None, o[3].data_ptr(), o[4].data_ptr(), st),
              "bn_bwd_reduce_finalize")
        emit(f"bn backward finalize, one launch, {layout} layout", *o, sums[:(3 if layout == "reduce" else 2) * Cf])
        sums = torch.zeros(65 * 3 * Cf, dtype=torch.float64, device="cuda")
        if layout == "reduce":
            check(lib.gsd_bn_bwd_reduce_partials(p.data_ptr(), rows, Cf, sums.data_ptr(), st), "bn_bwd_reduce_partials")
        else:
            check(lib.gsd_bn_reduce_partials(p.data_ptr(), rows, mpad, Cf, sums.data_ptr(), st), "bn_reduce_partials")
        for glob in (None, sg):
            o = [nan(Cf) for _ in range(5)]
            check(lib.gsd_bn_bwd_finalize(sums.data_ptr(), L.ptr(glob), Cf, count, o[0].data_ptr(), o[1].data_ptr(),
                                          o[2].data_ptr() if layout == "reduce" else None, o[3].data_ptr(), o[4].data_ptr(), st),
                  "bn_bwd_finalize")
            emit(f"bn backward finalize, three launches, {layout} layout, global sums {glob is not None}", *o, sums[:3 * Cf])
    rm, rv = randn(Cc, scale=2.0), rand(1e-4, 5.0, Cc)
    o = [nan(Cc) for _ in range(6)]
    check(lib.gsd_bn_eval_coeffs(sc.data_ptr(), sh.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5, Cc, o[0].data_ptr(), o[1].data_ptr(),
                                 st), "bn_eval_coeffs")
    check(lib.gsd_bn_eval_coeffs_bwd(sc.data_ptr(), sh.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5, Cc, o[2].data_ptr(),
                                     o[3].data_ptr(), o[4].data_ptr(), o[5].data_ptr(), st), "bn_eval_coeffs_bwd")
    emit("bn_eval_coeffs", o[0], o[1])
    emit("bn_eval_coeffs_bwd", *o[2:])
    counters = torch.tensor([5, 0, 41], dtype=torch.int64, device="cuda")
    ptrs = (C.c_void_p * 3)(*[counters.data_ptr() + 8 * i for i in range(3)])
    check(lib.gsd_add_counters(ptrs, 3, 2, st), "add_counters")
    emit("add_counters", counters)

    # ---- gsd_head.hip
    H, W = 7, 9
    raw = randn(N, Cc, H, W)
    pooled = nan(N, Cc, H // 2, W // 2)
    s = L.make_src(raw, sc, sh, relu=True)
    check(lib.gsd_maxpool2(C.byref(s), pooled.data_ptr(), N, Cc, H, W, st), "maxpool2")
    emit("maxpool2 7x9", pooled)
    for (H, W) in ((6, 10), (7, 9)):
        raw = randn(N, Cc, H, W)
        s = L.make_src(raw, sc, sh, relu=True)
        for K in (1, 2):
            wk, bk, out = randn(K, Cc, scale=0.2), randn(K), nan(N, K, H, W)
            check(lib.gsd_conv1x1_out(C.byref(s), wk.data_ptr(), bk.data_ptr(), Cc, K, out.data_ptr(), N, H, W, st), "conv1x1_out")
            emit(f"conv1x1_out {H}x{W} K{K}", out)
    K = 2
    dout, dw = randn(N, K, H, W), nan(K, Cc)
    wpart = torch.zeros(lib.gsd_conv1x1_out_wgrad_rows(N, H, W) * K * Cc, device="cuda")
    wsums = torch.zeros(65 * K * Cc, dtype=torch.float64, device="cuda")
    check(lib.gsd_conv1x1_out_wgrad(raw.data_ptr(), sc.data_ptr(), sh.data_ptr(), dout.data_ptr(), Cc, K, dw.data_ptr(), wpart.data_ptr(),
                                    wsums.data_ptr(), N, H, W, st), "conv1x1_out_wgrad")
    emit("conv1x1_out_wgrad K2", dw, wpart, wsums[:K * Cc])

    # ---- gsd_optim.hip: numel = 1027 (a short last group of the gradient norm)
    numel = 1027
    o_, t_ = randn(numel), randn(numel)
    for kind in (0, 1):
        for with_grad in (True, False):
            for gstate in (None, "clear"):
                loss, grad, ws = nan(1), nan(numel), torch.zeros(2048, device="cuda")
                words, guard = guard_of(gstate)
                check(lib.gsd_loss_fwd_bwd(kind, o_.data_ptr(), t_.data_ptr(), numel, 0.5, loss.data_ptr(),
                                           grad.data_ptr() if with_grad else None, ws.data_ptr(), guard, st), "loss")
                emit(f"loss kind{kind} grad {with_grad} guard {gstate}", loss, grad, *([words] if words is not None else []))
    init = {"p": randn(numel, scale=0.05), "g": randn(numel, scale=1e-3), "m": randn(numel, scale=1e-4),
            "v": rand(0.0, 1e-7, numel), "ema": randn(numel, scale=0.05)}
    for with_ema in (True, False):
        for step in (1, 7):
            for gstate in (None, "raised", "clear"):
                for coef in (None, 1.0, 0.25):      # None: gsd_adam_ema; else gsd_adam_ema_clip with clip[1] = coef
                    t = {k: v.clone() for k, v in init.items()}
                    words, guard = guard_of(gstate)
                    args = (t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(),
                            t["ema"].data_ptr() if with_ema else None, numel, step, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.995, 0.5)
                    if coef is None:
                        check(lib.gsd_adam_ema(*args, guard, st), "adam_ema")
                    else:
                        clip = torch.tensor([3.0, coef], device="cuda")
                        check(lib.gsd_adam_ema_clip(*args, clip.data_ptr(), guard, st), "adam_ema_clip")
                    emit(f"adam ema {with_ema} step{step} guard {gstate} clip {coef}", *t.values(),
                         *([words] if words is not None else []))
    arena = randn(numel, scale=1e-2)
    shifted = torch.zeros(numel + 1, device="cuda")
    shifted[1:] = arena
    nws = lib.gsd_grad_norm_workspace(numel)
    for off in (0, 1):          # 16-byte aligned, and offset by 4 bytes: the same values
        gsrc = shifted[1:] if off else arena
        clip, ws = nan(2), torch.zeros(nws, dtype=torch.float64, device="cuda")
        words, guard = guard_of("clear")
        check(lib.gsd_grad_norm(gsrc.data_ptr(), numel, 0.5, 0.01, clip.data_ptr(), ws.data_ptr(), nws, guard, st), "grad_norm")
        emit(f"grad_norm offset {4 * off} B", clip, ws, words)
    live, snap = randn(numel), nan(numel)
    check(lib.gsd_guard_snapshot(live.data_ptr(), snap.data_ptr(), numel, st), "guard_snapshot")
    emit("guard_snapshot", snap)
    for gstate in ("raised", "clear"):
        dst = randn(numel)
        words, guard = guard_of(gstate)
        check(lib.gsd_guard_restore(guard, dst.data_ptr(), snap.data_ptr(), numel, st), "guard_restore")
        emit(f"guard_restore guard {gstate}", dst)

    # ---- gsd_resize.hip: the area form
    x, base = rand(0.0, 255.0, 2, 3, 9, 11), rand(0.0, 255.0, 2, 3, 9, 11)
    A, B = rand(0.5, 2.0, 3), randn(3)
    for with_base in (True, False):
        out = nan(2, 3, 4, 5)
        check(lib.gsd_area_resize_affine(x.data_ptr(), base.data_ptr() if with_base else None, 2, 3, 9, 11, out.data_ptr(), 4, 5,
                                         A.data_ptr(), B.data_ptr(), 3, 255.0, 0.5, st), "area_resize_affine")
        emit(f"area_resize_affine base {with_base}", out)

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
    out = os.path.join(REPO, "profiles", "ab_pointwise_bits.txt")
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
