"""Per-layer cost of the deferred activation at the fp32 U-Net's forward shapes: every conv3x3 whose input is an activated or
pooled tensor (13 + 4 launches per step) in the two-dimensional Winograd form, once the way the engine calls it without
GSD_ACT_ONCE (deferred BatchNorm + ReLU on dense rows; the decoder's first convs as [deferred skip, plain up]; the encoder's
first convs on a dense pooled tensor) and once on ONE plain source with 16-byte aligned, zero-padded rows.  The same for dW.
usage (GPU box): python profiles/act_once_layers.py [batch] [reps] [fwd|dw|both]
Under `rocprofv3 --kernel-trace --stats` the two classes show as conv3x3_w2d_kernel<0, 2, .> / <1, 2, .> against <1, 1, .>."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gelslim_depth_amd import _lib as L

lib, check = L.lib, L.check
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
what = sys.argv[3] if len(sys.argv) > 3 else "both"
DIMS, H0, W0 = [64, 128, 256, 512, 1024], 320, 427
st = L.stream_ptr()
r4 = lambda v: (v + 3) // 4 * 4


def pitched(n, c, h, w):
    """zero-filled (n, c, h, r4(w)) buffer with slack around it, viewed at width w"""
    p = r4(w)
    buf = torch.zeros(n * c * h * p + 2 * L.SLACK, device="cuda")
    return buf[L.SLACK:L.SLACK + n * c * h * p].view(n, c, h, p)[..., :w]


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


layers = []   # (kind, level, cin, cout, h, w): enc0 = first conv of an encoder level (pooled), mid = second conv, dec0 = on the concat
h, w = H0, W0
for lvl, c in enumerate(DIMS):
    if lvl:
        layers.append(("enc0", lvl, c // 2, c, h, w))
    layers.append(("mid", lvl, c, c, h, w))
    if lvl < 4:
        layers.append(("dec0", lvl, 2 * c, c, h, w))
        layers.append(("mid", lvl, c, c, h, w))
    h, w = h // 2, w // 2

ws = torch.empty(max(1, max(lib.gsd_conv3x3_w2d_workspace(B, h, w, ci, co) for _, _, ci, co, h, w in layers)), device="cuda")
tot = {}
print("batch %d, us per launch: deferred / dense sources | one plain pitched source" % B)
for kind, lvl, ci, co, h, w in layers:
    if not lib.gsd_conv3x3_prefers_w2d(B, h, w, ci, co, 1):
        print("%-4s L%d %4d->%4d %3dx%3d  not the 2-D form in train mode" % (kind, lvl, ci, co, h, w))
        continue
    sc, sh = torch.rand(ci, device="cuda") + 0.5, torch.randn(ci, device="cuda") * 0.1
    if kind == "dec0":
        c2 = ci // 2
        skip = L.slack_empty((B, c2, h, w), "cuda").normal_()
        up = L.slack_empty((B, c2, 2 * (h // 2), 2 * (w // 2)), "cuda").normal_()
        old = [L.make_src(skip, sc[:c2].contiguous(), sh[:c2].contiguous(), relu=True, slack=L.SLACK), L.make_src(up, slack=L.SLACK)]
    elif kind == "enc0":
        old = [L.make_src(L.slack_empty((B, ci, h, w), "cuda").normal_(), slack=L.SLACK)]
    else:
        old = [L.make_src(L.slack_empty((B, ci, h, w), "cuda").normal_(), sc, sh, relu=True, slack=L.SLACK)]
    xp = pitched(B, ci, h, w)
    xp.normal_()
    new = [L.make_src(xp, slack=L.SLACK)]
    wt = torch.randn(co, ci, 3, 3, device="cuda") * 0.05
    y = torch.empty(B, co, h, w, device="cuda")
    part = torch.zeros(lib.gsd_conv3x3_w2d_partial_rows(B, h, w, co) * 2 * ((co + 63) // 64 * 64), device="cuda")
    dst = L.dst_array([L.make_dst(y)])
    wl = torch.empty(lib.gsd_weight_layout_size(8, co, ci), device="cuda")
    check(lib.gsd_weight_layout(8, wt.data_ptr(), co, ci, wl.data_ptr(), st), "layout")
    line = "%-4s L%d %4d->%4d %3dx%3d " % (kind, lvl, ci, co, h, w)
    if what in ("fwd", "both"):
        t = []
        for srcs in (old, new):
            arr = L.src_array(srcs)
            t.append(timed(lambda: check(lib.gsd_conv3x3_w2d_ws(arr, len(srcs), wl.data_ptr(), ci, co, dst, 1, part.data_ptr(),
                                                                ws.data_ptr(), ws.numel(), B, h, w, st), "conv")))
        # the pass at the copy rate: read + write; dec0: the pool writes the skip half on the way; enc0: the pool writes pooled anyway
        pass_us = {"mid": 2 * ci, "dec0": ci // 2, "enc0": 0}[kind] * B * h * r4(w) * 4 / 6.3e6
        line += " fwd %8.1f | %8.1f  x%.3f  saves %7.1f  (pass at 6.3 TB/s: %6.1f)" % (t[0], t[1], t[1] / t[0], t[0] - t[1], pass_us)
        k = "fwd " + kind
        tot[k] = [a + b for a, b in zip(tot.get(k, [0, 0]), t)]
    if what in ("dw", "both"):
        dy = pitched(B, co, h, w)
        dy.normal_()
        dys = L.make_src(dy)
        dw = torch.empty(co, ci, 3, 3, device="cuda")
        wws = torch.empty(max(1, lib.gsd_conv3x3_wgrad_workspace(B, h, w, ci, co)), device="cuda")
        t = []
        for srcs in (old, new):
            arr = L.src_array(srcs)
            form = lib.gsd_conv3x3_wgrad_form(arr, len(srcs), dys, ci, co, B, h, w)
            t.append(timed(lambda: check(lib.gsd_conv3x3_wgrad(arr, len(srcs), dys, ci, co, dw.data_ptr(), wws.data_ptr(), wws.numel(),
                                                               B, h, w, st), "wgrad")))
        line += "   dW(form %d) %8.1f | %8.1f  x%.3f" % (form, t[0], t[1], t[1] / t[0])
        k = "dW  " + kind
        tot[k] = [a + b for a, b in zip(tot.get(k, [0, 0]), t)]
    print(line, flush=True)
for k, (a, b) in sorted(tot.items()):
    print("total %-9s %9.1f | %9.1f us   saves %8.1f" % (k, a, b, a - b))
