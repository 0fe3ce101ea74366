"""Per-layer time of the plain two-dimensional Winograd launches at the two deep levels of the fp32 U-Net (40 x 53 and 20 x 26):
every forward ("activate once": one plain pitched source) and every dX shape, as the engine calls them in train mode (K-slab
scratch lent, statistics rows written), with the rectangular tile grid (GSD_W2D_STRIPS=0) and with the band-major flat tile list
(GSD_W2D_STRIPS=1), two rounds interleaved in one process.  In a tree without the strips form both columns time the same kernel:
their difference is that tree's own round-to-round noise.
usage (GPU box): python profiles/w2d_strips_layers.py [batch] [reps] [rounds]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gelslim_depth_amd import _lib as L

lib, check = L.lib, L.check
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
st = L.stream_ptr()
r4 = lambda v: (v + 3) // 4 * 4

# (what, K, M): forward K -> M and the dX launches (K = the layer's output channels) of levels 3 and 4
LAYERS = [(40, 53, [("fwd enc0", 256, 512), ("fwd mid ", 512, 512), ("fwd dec0", 1024, 512), ("dX  enc0", 512, 256), ("dX  dec0", 512, 1024)]),
          (20, 26, [("fwd enc0", 512, 1024), ("fwd mid ", 1024, 1024), ("dX  enc0", 1024, 512)])]


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


print("batch %d, us per launch, %d rounds of (rectangles, strips); mean, strips / rectangles, largest round-to-round difference" % (B, rounds))
tot = {}
for h, w, shapes in LAYERS:
    for what, k, m in shapes:
        if not lib.gsd_conv3x3_prefers_w2d(B, h, w, k, m, 1):
            print("%dx%d %s %4d->%4d  not the 2-D form in train mode at this batch" % (h, w, what, k, m))
            continue
        p = r4(w)
        buf = torch.zeros(B * k * h * p + 2 * L.SLACK, device="cuda")
        x = buf[L.SLACK:L.SLACK + B * k * h * p].view(B, k, h, p)[..., :w]
        x.normal_()
        arr = L.src_array([L.make_src(x, slack=L.SLACK)])
        y = torch.empty(B, m, h, w, device="cuda")
        dst = L.dst_array([L.make_dst(y)])
        part = torch.zeros(lib.gsd_conv3x3_w2d_partial_rows(B, h, w, m) * 2 * ((m + 63) // 64 * 64), device="cuda")
        os.environ["GSD_W2D_STRIPS"] = "1"
        scratch = lib.gsd_conv3x3_w2d_strips_scratch(B, h, w, k, m) if hasattr(lib, "gsd_conv3x3_w2d_strips_scratch") else 0
        ws = torch.empty(max(1, lib.gsd_conv3x3_w2d_workspace(B, h, w, k, m), scratch), device="cuda")   # K slabs, or the strips' per-tile sums
        wl = torch.empty(lib.gsd_weight_layout_size(8, m, k), device="cuda")
        check(lib.gsd_weight_layout(8, (torch.randn(m, k, 3, 3, device="cuda") * 0.05).data_ptr(), m, k, wl.data_ptr(), st), "layout")
        run = lambda: check(lib.gsd_conv3x3_w2d_ws(arr, 1, wl.data_ptr(), k, m, dst, 1, part.data_ptr(), ws.data_ptr(), ws.numel(), B, h, w, st), "conv")
        t = {"0": [], "1": []}
        for _ in range(rounds):
            for sw in ("0", "1"):
                os.environ["GSD_W2D_STRIPS"] = sw
                t[sw].append(timed(run))
        a, b = sum(t["0"]) / rounds, sum(t["1"]) / rounds
        noise = max(max(v) - min(v) for v in t.values())
        key = "%dx%d" % (h, w)
        tot[key] = [u + v for u, v in zip(tot.get(key, [0, 0, 0]), (a, b, noise))]
        print("%dx%d %s %4d->%4d  rect %s  strips %s   %8.1f | %8.1f  x%.3f  (rounds differ by %.1f)" %
              (h, w, what, k, m, " ".join("%8.1f" % v for v in t["0"]), " ".join("%8.1f" % v for v in t["1"]), a, b, b / a, noise), flush=True)
for key, (a, b, noise) in tot.items():
    print("total %s  %9.1f | %9.1f us  x%.3f  saves %8.1f  (sum of the layers' round-to-round differences %.1f)" % (key, a, b, b / a, a - b, noise))
