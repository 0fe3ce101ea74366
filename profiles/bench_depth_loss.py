"""Train steps of BASELINE's network (fp32, batch 32, 3x320x427) with loss="mse" or with a DepthLoss that has every term on
(huber, contact weight, four slope scales), to be run under rocprofv3 --kernel-trace --stats: the kernel times of DESIGN.md
section 14 (depth_loss_stage1<4, true> / depth_loss_stage2 with --loss depth, loss_stage1<0> / loss_stage2 with --loss mse).
With --loss depth the plain MSE kernel is also launched, behind the timed steps, on the very tensors the DepthLoss step left
(its output, its target, a gradient buffer of the same shape): both kernels on the same tensors in one process.
usage (GPU box): PYTHONPATH=. python profiles/bench_depth_loss.py --loss mse|depth [--batch 32] [--steps 8]"""
import argparse
import statistics

import numpy as np
import torch

from gelslim_depth_amd import synth
from gelslim_depth_amd.models.unet import UNet
from gelslim_depth_amd.train import DepthLoss, TrainStep, loss_fwd_bwd

ap = argparse.ArgumentParser()
ap.add_argument("--loss", default="depth", choices=["mse", "depth"])
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()

DIMS = [64, 128, 256, 512, 1024]
FULL = DepthLoss(data="huber", huber_delta=0.05, contact_weight=4.0, contact_eps=1e-3, grad_weight=0.5, grad_kind="l1", grad_scales=4)
m = UNet(n_channels=3, n_classes=1, layer_dimensions=DIMS)
m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state(3, 1, DIMS, 0, "conditioned").items()}, strict=True)
m = m.to("cuda").train()
step = TrainStep(m, loss="mse" if a.loss == "mse" else FULL)
x, t = synth.make_batch(a.batch, 320, 427, 1)
t = np.where(np.random.Generator(np.random.PCG64(2)).random(t.shape) < 0.3, t, np.float32(0.0)).astype(np.float32)   # 30 % contact
xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
for _ in range(a.warmup):
    step(xd, td)
torch.cuda.synchronize()
ms = []
for _ in range(a.steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step(xd, td)
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
line = f"fp32 batch {a.batch} loss {a.loss}: step median {statistics.median(ms):.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}); loss {float(step.last_loss):.6g}"
if a.loss == "depth":
    line += "; terms " + " ".join(f"{v:.5g}" for v in step.last_loss_terms.tolist())
    buf, g = torch.zeros((1,), device="cuda"), torch.empty_like(step._out)
    ws = torch.empty((2048,), device="cuda", dtype=torch.float64)
    for _ in range(a.steps):
        loss_fwd_bwd("mse", step._out, td, g, buf, ws)
    torch.cuda.synchronize()
print(line)
