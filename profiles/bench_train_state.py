"""What a resumable run pays per state file on BASELINE's network (fp32, 31.0 M parameters): TrainStep.state_dict() (the
device-to-host copies of parameters, buffers, Adam moments and EMA shadow), save_state (that plus the write to disk through
a temporary file, fsync and rename) and load_state (read plus the in-place host-to-device copies).  Median of 5, after one
warm-up of each; host clock around calls that end in a device synchronise.
usage (GPU box): PYTHONPATH=. python profiles/bench_train_state.py [directory for the file]"""
import os
import statistics
import sys
import tempfile
import time

import torch

from gelslim_depth_amd import synth
from gelslim_depth_amd.models.unet import UNet
from gelslim_depth_amd.train import TrainStep

DIMS = [64, 128, 256, 512, 1024]
folder = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp()
os.makedirs(folder, exist_ok=True)
path = os.path.join(folder, "state.pt")
m = UNet(n_channels=3, n_classes=1, layer_dimensions=DIMS)
m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state(3, 1, DIMS, 0, "conditioned").items()}, strict=True)
m = m.to("cuda").train()
step = TrainStep(m)
x, t = synth.make_batch(2, 320, 427, 1)
step(torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda())
torch.cuda.synchronize()


def timed(fn, reps=5):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


rows = [("state_dict", timed(step.state_dict)), ("save_state", timed(lambda: step.save_state(path))),
        ("load_state", timed(lambda: step.load_state(path)))]
size = os.path.getsize(path)
print(f"network {DIMS}, {step.numel} parameters, state file {size / 1e6:.1f} MB")
for name, (med, lo, hi) in rows:
    print(f"{name:11s} median {med * 1e3:8.1f} ms  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
os.remove(path)
