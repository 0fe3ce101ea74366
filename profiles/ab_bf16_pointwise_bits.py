"""A/B of bit-identity between two builds of libgsd.so over the bf16 pointwise entry points (gsd_bf16_layout.hip, gsd_bf16_bn.hip,
gsd_bf16_head.hip, gsd_bf16_sums.hip) and the MFMA units that share their pack / unpack / statistics pieces (gsd_bf16_conv.hip,
gsd_bf16_c64.hip, gsd_bf16_ctgemm.hip, gsd_bf16_first.hip, gsd_bf16_inc.hip): every entry point on fixed seeded inputs at the shapes
of tests/test_gpu_bf16_pointwise_forms.py and of the small tests of tests/test_gpu_bf16.py, the sha256 of every output buffer
compared between the two libraries.

usage (GPU box, repo root): python profiles/ab_bf16_pointwise_bits.py LIB_A LIB_B [--out profiles/ab_bf16_pointwise_bits.txt]
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
#            C, (N, H, W): cases a-f of tests/test_gpu_bf16_pointwise_forms.py, then the small tests' shapes
APPLY_SHAPES = [(64, (1, 1, 8191)), (64, (1, 1, 8193)), (64, (1, 91, 91)), (128, (1, 1, 4097)), (40, (1, 1, 13108)), (64, (2, 64, 64)),
                (40, (2, 11, 15)), (72, (2, 13, 18))]


def child(out_path):
    sys.path.insert(0, REPO)
    import torch
    from gelslim_depth_amd import _lib as L
    lib, check = L.lib, L.check
    st = L.stream_ptr()
    cpu = torch.Generator().manual_seed(20241)
    lines, keep = [], []

    def randn(*shape, scale=1.0):
        return (torch.randn(shape, generator=cpu) * scale).cuda()

    def rand(lo, hi, *shape):
        return (torch.rand(shape, generator=cpu) * (hi - lo) + lo).cuda()

    def act(*shape, coarse=False):          # (N,H,W,C) bf16
        t = torch.randn(shape, generator=cpu)
        return (torch.round(t * 4) / 4 if coarse else t).to(torch.bfloat16).cuda()

    def nan(*shape, dtype=torch.float32):
        return torch.full(shape, float("nan"), dtype=dtype, device="cuda")

    def nanb(*shape):
        return nan(*shape, dtype=torch.bfloat16)

    def view(t, off=0, c=None):
        keep.append(L.make_nhwc(t, off, c))
        return C.byref(keep[-1])

    def emit(case, *tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else t.dtype).cpu().numpy().tobytes())
        lines.append(f"{case} {h.hexdigest()}")

    def coeffs(c):      # scale, shift, mean, invstd, c1, c2
        return [rand(0.5, 1.5, c), randn(c), randn(c, scale=0.3), rand(0.5, 2.0, c), randn(c, scale=0.1), randn(c, scale=0.1)]

    def image(mode, w, co, ci):
        img = nanb(lib.gsd_bf16_weight_image_size(mode, co, ci))
        check(lib.gsd_bf16_weight_image(mode, w.data_ptr(), co, ci, img.data_ptr(), st), f"weight_image {mode}")
        return img

    # ---- gsd_bf16_layout.hip: all five modes one by one and in one batched launch; the first layer's im2col
    co, ci = 48, 40
    srcs = {0: (randn(co, ci, 3, 3), co, ci), 1: (randn(co, ci, 3, 3), co, ci), 2: (randn(co, 3, 3, 3), co, 3),
            3: (randn(ci, co, 2, 2), co, ci), 4: (randn(ci, co, 2, 2), co, ci)}
    for mode, (w, a, b) in srcs.items():
        emit(f"weight_image mode{mode}", image(mode, w, a, b))
    jobs = (L.gsd_bf16_wimg_job * 5)()
    outs = []
    for j, (mode, (w, a, b)) in zip(jobs, srcs.items()):
        outs.append(nanb(lib.gsd_bf16_weight_image_size(mode, a, b)))
        j.w, j.out, j.mode, j.Cout, j.Cin, j.reserved = w.data_ptr(), outs[-1].data_ptr(), mode, a, b, 0
    check(lib.gsd_bf16_weight_images(jobs, 5, st), "weight_images")
    emit("weight_images modes 0-4 batched", *outs)
    x = rand(0.0, 1.0, 2, 3, 21, 27)
    col = nanb(2, 21, 27, 32)
    check(lib.gsd_bf16_im2col3x3(x.data_ptr(), 2, 3, 21, 27, view(col), st), "im2col")
    emit("im2col3x3 2x3x21x27", col)

    # ---- gsd_bf16_bn.hip: apply (both forms) and backward apply (both forms), tensors as channel slices of wider buffers
    for c, (n, h, w) in APPLY_SHAPES:
        k = coeffs(c)
        ybuf, dz0 = act(n, h, w, c + 16), act(n, h, w, c + 24)
        for relu in (0, 1):
            cat = nanb(n, h, w, c + 24)
            check(lib.gsd_bf16_bn_apply(view(ybuf, 8, c), k[0].data_ptr(), k[1].data_ptr(), view(cat, 0, c), relu, st), "bn_apply")
            emit(f"bn_apply C{c} {n}x{h}x{w} relu{relu}", cat)
        dz = dz0.clone()
        check(lib.gsd_bf16_bn_bwd_apply(view(dz, 0, c), view(ybuf, 8, c), k[0].data_ptr(), k[2].data_ptr(), k[3].data_ptr(), k[4].data_ptr(),
                                        k[5].data_ptr(), st), "bn_bwd_apply")
        emit(f"bn_bwd_apply C{c} {n}x{h}x{w}", dz)

    # apply + pool (with and without the arg-max codes), the stand-alone pool, the backward reduce in every mode and route
    for c, n, h, w in ((40, 3, 11, 15), (40, 3, 12, 16), (72, 2, 13, 18), (64, 2, 13, 18), (64, 2, 12, 17), (48, 3, 9, 11)):
        k = coeffs(c)
        y = act(n, h, w, c, coarse=True)
        cat, pooled, idx = nanb(n, h, w, c + 24), nanb(n, h // 2, w // 2, c), torch.full((n, h // 2, w // 2, c // 8), -1, dtype=torch.int16,
                                                                                         device="cuda")
        check(lib.gsd_bf16_bn_apply_pool_idx(view(y), k[0].data_ptr(), k[1].data_ptr(), view(cat, 0, c), view(pooled), idx.data_ptr(), st),
              "apply_pool_idx")
        emit(f"bn_apply_pool_idx C{c} {n}x{h}x{w}", cat, pooled, idx)
        cat2, pooled2 = nanb(n, h, w, c + 24), nanb(n, h // 2, w // 2, c)
        check(lib.gsd_bf16_bn_apply_pool(view(y), k[0].data_ptr(), k[1].data_ptr(), view(cat2, 0, c), view(pooled2), st), "apply_pool")
        emit(f"bn_apply_pool C{c} {n}x{h}x{w}", cat2, pooled2)
        pooled3 = nanb(n, h // 2, w // 2, c)
        check(lib.gsd_bf16_maxpool2(view(cat, 0, c), view(pooled3), st), "maxpool2")
        emit(f"maxpool2 C{c} {n}x{h}x{w}", pooled3)
        g, dpool = act(n, h, w, c), act(n, h // 2, w // 2, c)
        dout, wout = randn(n, 1, h, w), randn(1, c)
        rows = lib.gsd_bf16_bn_bwd_partial_rows(n, h, w)
        for mode, route in ((0, ""), (1, " a route"), (1, " idx route"), (2, "")):
            dz, part = nanb(n, h, w, c), nan(rows, 3 * c)
            head = (view(y), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(), k[3].data_ptr(), view(g))
            if route == " idx route":
                check(lib.gsd_bf16_bn_bwd_reduce_pool_idx(*head, idx.data_ptr(), view(dpool), view(dz), part.data_ptr(), st), "reduce idx")
            else:
                check(lib.gsd_bf16_bn_bwd_reduce(mode, *head, view(cat, 0, c), view(dpool), dout.data_ptr(), wout.data_ptr(), view(dz),
                                                 part.data_ptr(), st), "reduce")
            emit(f"bn_bwd_reduce mode{mode}{route} C{c} {n}x{h}x{w}", dz, part)

    # ---- gsd_bf16_head.hip
    for n, h, w, c in ((2, 13, 18, 64), (3, 9, 11, 40), (1, 20, 26, 128)):
        k = coeffs(c)
        y = act(n, h, w, c)
        wo, bo = randn(1, c, scale=c ** -0.5), randn(1)
        a, out0, out1 = nanb(n, h, w, c), nan(n, 1, h, w), nan(n, 1, h, w)
        check(lib.gsd_bf16_bn_apply(view(y), k[0].data_ptr(), k[1].data_ptr(), view(a), 1, st), "apply")
        check(lib.gsd_bf16_conv1x1_out(view(a), wo.data_ptr(), bo.data_ptr(), 1, out0.data_ptr(), st), "conv1x1_out")
        check(lib.gsd_bf16_bn_relu_conv1x1_out(view(y), k[0].data_ptr(), k[1].data_ptr(), wo.data_ptr(), bo.data_ptr(), 1, out1.data_ptr(), st),
              "bn_relu_conv1x1_out")
        emit(f"conv1x1_out C{c} {n}x{h}x{w}", out0)
        emit(f"bn_relu_conv1x1_out C{c} {n}x{h}x{w}", out1)

    # ---- gsd_bf16_sums.hip: a window of a channel slice; the ConvT bias gradient with all four pad strips present
    t = act(3, 21, 27, 64)
    nws = lib.gsd_bf16_channel_sums_workspace(3, 20, 26, 32)
    ws, out = nan(nws), nan(32)
    check(lib.gsd_bf16_channel_sums(view(t, 32, 32), 1, 0, 20, 26, out.data_ptr(), ws.data_ptr(), nws, st), "channel_sums")
    emit("channel_sums 3x21x27 C32 window (1,0)+(20,26)", out, ws)
    n, H, W, ctot, cup, oy, ox, hh, ww, kin = 2, 19, 23, 128, 64, 1, 2, 16, 20, 64
    wt = randn(ctot, kin, 3, 3, scale=1.0 / (3.0 * kin ** 0.5))
    img = image(0, wt, ctot, kin)
    xin, gcat = act(n, H, W, kin), nanb(n, H, W, ctot)
    rows, mp = lib.gsd_bf16_conv_partial_rows(n, H, W, ctot), lib.gsd_bf16_conv_mpad(ctot)
    part = nan(rows, 2 * mp)
    check(lib.gsd_bf16_conv3x3(view(xin), img.data_ptr(), view(gcat), kin, ctot, part.data_ptr(), None, st), "conv3x3 + statistics")
    emit("conv3x3 64->128 2x19x23 with partials", gcat, part[:, :ctot], part[:, mp:mp + ctot])
    nws = lib.gsd_bf16_convT_bias_grad_workspace(n, H, W, oy, ox, hh, ww, cup)
    ws, db = nan(nws), nan(cup)
    check(lib.gsd_bf16_convT_bias_grad(part.data_ptr(), rows, 2 * mp, ctot - cup, view(gcat, ctot - cup, cup), oy, ox, hh, ww, db.data_ptr(),
                                       ws.data_ptr(), nws, st), "convT_bias_grad")
    emit("convT_bias_grad 2x19x23 window (1,2)+(16,20), four strips", db, ws)

    # ---- the MFMA units: one small case each, with partials and with the fused BatchNorm-backward pass 1 where the kernel has one
    def bnbwd(yt, k):
        bw = L.gsd_bf16_bnbwd()
        keep.append(L.make_nhwc(yt))
        bw.y = C.pointer(keep[-1])
        bw.scale, bw.shift, bw.mean, bw.invstd = (v.data_ptr() for v in k[:4])
        keep.append(bw)
        return C.byref(bw)

    n, h, w, cin, cout = 2, 19, 37, 96, 64          # conv3x3 dX with the fused backward: M = cin = 96 rows
    wt = randn(cout, cin, 3, 3, scale=1.0 / (3.0 * cin ** 0.5))
    img = image(1, wt, cout, cin)
    dy, y, k = act(n, h, w, cout), act(n, h, w, cin), coeffs(cin)
    rows, mp = lib.gsd_bf16_conv_partial_rows(n, h, w, cin), lib.gsd_bf16_conv_mpad(cin)
    dz, part = nanb(n, h, w, cin), nan(rows, 2 * mp)
    check(lib.gsd_bf16_conv3x3(view(dy), img.data_ptr(), view(dz), cout, cin, part.data_ptr(), bnbwd(y, k), st), "conv3x3 fused dX")
    emit("conv3x3 dX 64->96 2x19x37 fused backward", dz, part[:, :cin], part[:, mp:mp + cin])
    n, h, w, kk, m = 2, 18, 29, 64, 96
    img = image(0, randn(m, kk, 3, 3, scale=1.0 / (3.0 * kk ** 0.5)), m, kk)
    xin, out, k = act(n, h, w, kk), nanb(n, h, w, m), coeffs(m)
    check(lib.gsd_bf16_conv3x3_bnrelu(view(xin), img.data_ptr(), view(out), kk, m, k[0].data_ptr(), k[1].data_ptr(), st), "conv3x3_bnrelu")
    emit("conv3x3_bnrelu 64->96 2x18x29", out)

    n, h, w, m = 2, 19, 70, 64                      # c64: forward with partials, dX with the fused backward
    wt = randn(m, m, 3, 3, scale=0.05)
    a, yb, k = act(n, h, w, m + 32), act(n, h, w, m), coeffs(m)
    rows, mp = lib.gsd_bf16_conv3x3_c64_partial_rows(n, h, w), lib.gsd_bf16_conv_mpad(m)
    for mode, bw in ((0, None), (1, bnbwd(yb, k))):
        img = image(mode, wt, m, m)
        got, part = nanb(n, h, w, m + 16), nan(rows, 2 * mp)
        check(lib.gsd_bf16_conv3x3_c64(view(a, 32, m), img.data_ptr(), view(got, 16, m), part.data_ptr(), bw, st), "conv3x3_c64")
        emit(f"conv3x3_c64 2x19x70 mode{mode} {'fused backward' if bw is not None else 'partials'}", got, part[:, :m], part[:, mp:mp + m])

    n, h, w, kk, m, oy, ox = 2, 8, 16, 64, 128, 1, 0      # ConvT dX on the large-tile kernel, with the fused backward
    wT = randn(m, kk, 2, 2, scale=m ** -0.5)              # (Cin, Cout, 2, 2): dX has M = Cin rows, K = Cout
    img = image(4, wT, kk, m)
    gcat, y, k = act(n, 2 * h + oy, 2 * w + ox, kk), act(n, h, w, m), coeffs(m)
    rows, mp = lib.gsd_bf16_conv_dense_partial_rows(n, h, w, kk, m, 4, 2), lib.gsd_bf16_conv_mpad(m)
    dx, part = nanb(n, h, w, m), nan(rows, 2 * mp)
    ty, tx = L.int_array([oy, oy, oy + 1, oy + 1]), L.int_array([ox, ox + 1, ox, ox + 1])
    check(lib.gsd_bf16_conv_dense(view(gcat), img.data_ptr(), view(dx), kk, m, 4, 2, ty, tx, h, w, 0, 0, 0, None, part.data_ptr(),
                                  bnbwd(y, k), st), "ConvT dX fused")
    emit("conv_dense ConvT dX 64->128 2x8x16 fused backward", dx, part[:, :m], part[:, mp:mp + m])

    n, c, h, w, m = 2, 3, 21, 27, 32                # first layer: partials, eval epilogue, statistics of the fused backward
    x, w0 = rand(0.0, 1.0, n, c, h, w), randn(m, c, 3, 3, scale=0.3)
    img0, mp, k = image(2, w0, m, c), lib.gsd_bf16_conv_mpad(m), coeffs(m)
    rows = lib.gsd_bf16_conv3x3_first_partial_rows(n, h, w, m)
    y1, part = nanb(n, h, w, m), nan(rows, 2 * mp)
    check(lib.gsd_bf16_conv3x3_first(x.data_ptr(), n, c, h, w, img0.data_ptr(), view(y1), m, part.data_ptr(), None, None, st), "first")
    emit("conv3x3_first 2x3x21x27 M32 partials", y1, part[:, :m], part[:, mp:mp + m])
    a1 = nanb(n, h, w, m)
    check(lib.gsd_bf16_conv3x3_first(x.data_ptr(), n, c, h, w, img0.data_ptr(), view(a1), m, None, k[0].data_ptr(), k[1].data_ptr(), st),
          "first eval")
    emit("conv3x3_first 2x3x21x27 M32 eval", a1)
    n, c, h, w, m = 2, 3, 19, 70, 64
    x, w0, w1 = rand(0.0, 1.0, n, c, h, w), randn(m, c, 3, 3, scale=0.3), randn(m, m, 3, 3, scale=0.05)
    img0, img1, mp, k = image(2, w0, m, c), image(0, w1, m, m), lib.gsd_bf16_conv_mpad(m), coeffs(m)
    rows0 = lib.gsd_bf16_conv3x3_first_partial_rows(n, h, w, m)
    da, partb = act(n, h, w, m), nan(rows0, 2 * mp)
    check(lib.gsd_bf16_first_bn_bwd_reduce(x.data_ptr(), n, c, h, w, img0.data_ptr(), view(da), k[0].data_ptr(), k[1].data_ptr(),
                                           k[2].data_ptr(), k[3].data_ptr(), partb.data_ptr(), st), "first_bn_bwd_reduce")
    emit("first_bn_bwd_reduce 2x3x19x70", partb[:, :m], partb[:, mp:mp + m])
    need = lib.gsd_bf16_wgrad_first_workspace(n, h, w, m)
    ws, dw = torch.zeros(need, device="cuda"), nan(m, c, 3, 3)
    check(lib.gsd_bf16_wgrad_first_recompute(x.data_ptr(), n, c, h, w, img0.data_ptr(), view(da), k[0].data_ptr(), k[1].data_ptr(),
                                             k[2].data_ptr(), k[3].data_ptr(), k[4].data_ptr(), k[5].data_ptr(), dw.data_ptr(), ws.data_ptr(),
                                             need, st), "wgrad_first_recompute")
    emit("wgrad_first_recompute 2x3x19x70", dw)
    y0 = nanb(n, h, w, m)
    check(lib.gsd_bf16_conv3x3_first(x.data_ptr(), n, c, h, w, img0.data_ptr(), view(y0), m, None, None, None, st), "first plain")
    dw2 = nan(m, c, 3, 3)
    check(lib.gsd_bf16_wgrad_first(x.data_ptr(), n, c, h, w, view(da), view(y0), k[0].data_ptr(), k[2].data_ptr(), k[3].data_ptr(),
                                   k[4].data_ptr(), k[5].data_ptr(), dw2.data_ptr(), ws.data_ptr(), need, st), "wgrad_first")
    emit("wgrad_first 2x3x19x70 fused backward apply", dw2)
    cat, y1 = nanb(n, h, w, m + 32), nanb(n, h, w, m)
    rowsf = lib.gsd_bf16_inc_conv_partial_rows(n, h, w)
    partf = nan(rowsf, 2 * mp)
    check(lib.gsd_bf16_inc_conv(x.data_ptr(), n, c, h, w, img0.data_ptr(), k[0].data_ptr(), k[1].data_ptr(), img1.data_ptr(), view(cat, 0, m),
                                view(y1), partf.data_ptr(), st), "inc_conv")
    emit("inc_conv 2x3x19x70", cat, y1, partf[:, :m], partf[:, mp:mp + m])

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
    out = os.path.join(REPO, "profiles", "ab_bf16_pointwise_bits.txt")
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
