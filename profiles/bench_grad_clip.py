"""Train steps of BASELINE's network (31.0 M parameters, 3x320x427) with or without TrainStep(max_grad_norm=...), to be run
under rocprofv3 --kernel-trace --stats: the kernel times of DESIGN.md section 13 (grad_norm_stage1 / grad_norm_stage2 /
adam_ema_kernel<true> with --clip on, adam_ema_kernel<false> with --clip off).  Also prints the step time from device events.
usage (GPU box): PYTHONPATH=. python profiles/bench_grad_clip.py --dtype fp32|bf16 --clip on|off [--batch 32] [--steps 8]"""
import argparse
import statistics

import torch

from gelslim_depth_amd import synth
from gelslim_depth_amd.models.unet import UNet
from gelslim_depth_amd.train import TrainStep

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
ap.add_argument("--clip", default="on", choices=["on", "off"])
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()

DIMS = [64, 128, 256, 512, 1024]
m = UNet(n_channels=3, n_classes=1, layer_dimensions=DIMS, precision=a.dtype)
m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state(3, 1, DIMS, 0, "conditioned").items()}, strict=True)
m = m.to("cuda").train()
step = TrainStep(m, max_grad_norm=1.0 if a.clip == "on" else None)
x, t = synth.make_batch(a.batch, 320, 427, 1)
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
line = f"{a.dtype} batch {a.batch} clip {a.clip}: step median {statistics.median(ms):.2f} ms (min {min(ms):.2f}, max {max(ms):.2f})"
if a.clip == "on":
    line += f"; last norm {float(step.last_grad_norm):.4g}, coefficient {float(step.last_clip_coef):.4g}"
print(line)
