"""Generate tests/golden/ginput_grad.npz: the reference U-Net's gradient with respect to its INPUT, in train and in eval mode.

Runs only in the build container, where the reference exists (it does not on the GPU machine); the .npz is committed.  It
imports the reference's own model file the way make_golden.py does
    gelslim_depth/models/unet.py  (UNet:59, forward:79-88)
and differentiates the MSE loss of train_utils/train_unet.py:51-52 with respect to x and every parameter.

  small/*  layer_dimensions [16, 32, 64], N = 3, 3x37x45 (odd sizes: F.pad and floor pooling), the "conditioned" synthetic
           state (running statistics away from (0, 1)).  The state, x and the target are not stored: synth.make_state /
           synth.make_batch rebuild them from small/seed.  Train mode: y and x.grad in full, every parameter gradient as
           checksums (sum, sum |.|, sum of squares) and 64 evenly spaced samples.  Eval mode, from the same initial state:
           the same.
  full/*   the full-size net at 320x427, batch 1, on gfull_b1.npz's seed and state construction: checksums of x.grad
           (sum, sum |.|, sum of squares) and 64 evenly spaced samples, train and eval mode.

Usage: python tests/golden/make_golden_input_grad.py   (from the repository root; writes into tests/golden/)
"""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("GELSLIM_REFERENCE", os.path.join(os.path.dirname(REPO), "reference"))
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
torch.set_num_threads(8)
torch.manual_seed(0)

from gelslim_depth.models.unet import UNet  # noqa: E402  (reference)
from gelslim_depth_amd import synth  # noqa: E402  (build-owned generators)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def build(dims, state):
    net = UNet(n_channels=3, n_classes=1, layer_dimensions=dims, kernel_size=3, maxpool_size=2, upconv_stride=2)
    net.load_state_dict(OrderedDict((k, t(v)) for k, v in state.items()), strict=True)
    return net


def run(net, x, tgt, train):
    """One forward + MSE + backward with x.requires_grad; returns (y, x.grad, parameter gradients)."""
    net.train(train)
    xx = t(x).clone().requires_grad_(True)
    net.zero_grad(set_to_none=True)
    y = net(x=xx)
    loss = torch.mean((y - t(tgt)) ** 2)
    loss.backward()
    grads = OrderedDict((k, p.grad.detach().numpy().copy()) for k, p in net.named_parameters())
    return y.detach().numpy().copy(), xx.grad.detach().numpy().copy(), grads


def checksums(g):
    """(sum, sum |.|, sum of squares) in fp64, the indices of up to 64 evenly spaced elements and their values."""
    d = torch.from_numpy(g).double()
    flat = torch.from_numpy(g).reshape(-1)
    idx = np.linspace(0, flat.numel() - 1, num=min(64, flat.numel())).astype(np.int64)
    return np.array([d.sum().item(), d.abs().sum().item(), d.pow(2).sum().item()]), idx, flat[t(idx)].numpy().copy()


def pack_grads(prefix, grads):
    out = {}
    for k, v in grads.items():
        s, idx, samples = checksums(v)
        out[f"{prefix}/gradsum/{k}"] = s
        out[f"{prefix}/gradidx/{k}"] = idx.astype(np.int32)
        out[f"{prefix}/gradsample/{k}"] = samples
    return out


def main():
    out = {}
    # (a) small network: y and x.grad in full, parameter gradients as checksums and samples
    dims, seed = [16, 32, 64], 31
    st = synth.make_state(3, 1, dims, seed, "conditioned")
    x, tgt = synth.make_batch(3, 37, 45, seed + 1)
    out["small/dims"] = np.array(dims)
    out["small/seed"] = np.array(seed)
    out["small/nhw"] = np.array([3, 37, 45])
    for mode, train in (("train", True), ("eval", False)):
        net = build(dims, st)
        y, gx, grads = run(net, x, tgt, train=train)
        out[f"small/{mode}/y"], out[f"small/{mode}/xgrad"] = y, gx
        out.update(pack_grads(f"small/{mode}", grads))

    # (b) full-size network at batch 1: gfull_b1.npz's construction (make_golden.py g_full)
    dims, seed = [64, 128, 256, 512, 1024], 2024
    st = synth.make_state(3, 1, dims, seed, "conditioned")
    x, tgt = synth.make_batch(1, 320, 427, seed + 1)
    out["full/dims"] = np.array(dims)
    out["full/seed"] = np.array(seed)
    for mode, train in (("train", True), ("eval", False)):
        net = build(dims, st)
        _, gx, _ = run(net, x, tgt, train=train)
        s, idx, samples = checksums(gx)
        out[f"full/{mode}/xgrad_sums"] = s
        out[f"full/{mode}/xgrad_idx"] = idx.astype(np.int32)
        out[f"full/{mode}/xgrad_samples"] = samples
    path = os.path.join(HERE, "ginput_grad.npz")
    np.savez_compressed(path, **out)
    print(f"ginput_grad.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
