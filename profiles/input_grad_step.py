"""Train steps of the full-size fp32 U-Net with x.requires_grad (module forward + MSE + backward, the input gradient included),
for a kernel trace: the first conv's dX (dgrad3x3_first_kernel) or, with GSD_WGRAD_FIRST=0, the fallback pair
(bn_bwd_apply + the direct-form conv3x3 dX).
usage (GPU box): PYTHONPATH=. rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/input_grad_step.py [batch] [steps]"""
import sys

import torch

from gelslim_depth_amd import synth
from gelslim_depth_amd.models.unet import UNet

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dims = [64, 128, 256, 512, 1024]
st = synth.make_state(3, 1, dims, 2024, "conditioned")
m = UNet(n_channels=3, n_classes=1, layer_dimensions=dims)
m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
m = m.cuda().train()
x = torch.rand(B, 3, 320, 427, device="cuda").requires_grad_(True)
t = torch.rand(B, 1, 320, 427, device="cuda")
for i in range(steps + 1):
    x.grad = None
    loss = torch.mean((m(x=x) - t) ** 2)
    loss.backward()
torch.cuda.synchronize()
u = m._engine.enc[0][0]
print(f"batch {B}: {steps + 1} steps, first layer fused dW/dX {u.plan.fused_dw}, |x.grad| sum {x.grad.abs().sum().item():.6e}")
