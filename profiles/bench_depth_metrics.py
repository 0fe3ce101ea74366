"""The metrics launch (gsd_depth_metrics: depth_metrics_stage1 + depth_metrics_stage2) beside the depth-aware loss launch it is
measured against (gsd_depth_loss_fwd_bwd with grad = NULL, grad_scales = 1, contact_weight > 0: depth_loss_stage1<1, false> +
depth_loss_stage2), on the same two (N, 1, 320, 427) tensors, alternating, in one process: the times of DESIGN.md section 15.
  --mode kernels   to be run under rocprofv3 --kernel-trace --stats (the kernel times); also prints device-event times of the
                   two launch pairs, taken with the launches alternating
  --mode pass      a 16-batch validation pass of BASELINE's network (fp32) at that batch with harness.evaluate_loader and with
                   harness.evaluate_metrics, alternating, host clock around passes that end in their one synchronisation
usage (GPU box): PYTHONPATH=. python profiles/bench_depth_metrics.py --mode kernels|pass [--batch 32] [--reps 50]"""
import argparse
import statistics
import time

import numpy as np
import torch

from gelslim_depth_amd import synth
from gelslim_depth_amd.metrics import DepthMetrics, depth_metrics, depth_metrics_workspace
from gelslim_depth_amd.train import DepthLoss, depth_loss_fwd_bwd, depth_loss_workspace

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="kernels", choices=["kernels", "pass"])
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()

SPEC = DepthMetrics(background=0.0, contact_eps=1e-3, unit=-3.2, unit_name="mm")
LOSS = DepthLoss(data="huber", huber_delta=0.05, contact_weight=4.0, contact_eps=1e-3, grad_weight=0.5, grad_kind="l1", grad_scales=1)
x, t = synth.make_batch(a.batch, 320, 427, 1)
t = np.where(np.random.Generator(np.random.PCG64(2)).random(t.shape) < 0.3, t, np.float32(0.0)).astype(np.float32)   # 30 % contact
xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()


def median_ms(fn, reps):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


if a.mode == "kernels":
    od = (td + 0.03 * torch.randn(td.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(3))).contiguous()
    table = torch.empty((a.batch, 16), device="cuda", dtype=torch.float64)
    mws = torch.empty((depth_metrics_workspace(od.shape),), device="cuda", dtype=torch.float64)
    terms = torch.empty((6,), device="cuda")
    lws = torch.empty((depth_loss_workspace(od.shape),), device="cuda", dtype=torch.float64)

    def metrics():
        depth_metrics(od, td, SPEC, table, mws)

    def loss():
        depth_loss_fwd_bwd(LOSS, od, td, None, terms, lws)
    for _ in range(a.warmup):
        metrics(), loss()
    torch.cuda.synchronize()
    res = {"metrics": [], "loss": []}
    for _ in range(a.reps):                      # alternating: both see the same machine
        res["metrics"].append(median_ms(metrics, 1)[0])
        res["loss"].append(median_ms(loss, 1)[0])
    m, l = statistics.median(res["metrics"]), statistics.median(res["loss"])
    print(f"batch {a.batch} ({a.batch}, 1, 320, 427): device events around one launch pair, median of {a.reps}: metrics {1e3 * m:.1f} us, "
          f"depth loss (no grad, 1 scale) {1e3 * l:.1f} us, ratio {m / l:.2f}; contact fraction {float(terms[5]):.3f}, "
          f"table[0, :3] {table[0, :3].tolist()}")
else:
    from gelslim_depth_amd import harness
    from gelslim_depth_amd.models.unet import UNet
    from gelslim_depth_amd.train import TrainStep
    DIMS = [64, 128, 256, 512, 1024]
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=DIMS)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state(3, 1, DIMS, 0, "conditioned").items()}, strict=True)
    step = TrainStep(m.to("cuda").train())
    loader = [{"tactile_image": xd, "depth_image": td}] * 16
    for _ in range(2):
        harness.evaluate_loader(step, loader), harness.evaluate_metrics(step, loader, SPEC)
    res = {"loss": [], "metrics": []}
    for _ in range(max(3, a.reps // 10)):
        t0 = time.perf_counter()
        v = harness.evaluate_loader(step, loader)
        t1 = time.perf_counter()
        v2, s = harness.evaluate_metrics(step, loader, SPEC)
        t2 = time.perf_counter()
        assert v == v2
        res["loss"].append(1e3 * (t1 - t0)), res["metrics"].append(1e3 * (t2 - t1))
    l, mm = statistics.median(res["loss"]), statistics.median(res["metrics"])
    print(f"batch {a.batch}: 16-batch validation pass, fp32 full-size net, median of {len(res['loss'])}: evaluate_loader {l:.1f} ms, "
          f"evaluate_metrics {mm:.1f} ms (+{mm - l:.2f} ms, {100 * (mm - l) / l:.2f} %); loss {v:.6g}, mae {s['mae']:.4g} mm, "
          f"contact_iou {s['contact_iou']:.3f}")
