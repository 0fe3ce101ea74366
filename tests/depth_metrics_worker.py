"""Worker for tests/test_gpu_depth_metrics.py: one rank of a 2-rank harness.evaluate_metrics pass, fp32 and bf16.
Backend as tests/ddp_worker.py: RCCL with a card per rank where there are two, gloo with both ranks on cuda:0 otherwise.
7 samples at batch 2 per rank give global batches of 4 and 3 (rank 1 scores ONE sample of the tail: a short share, padded by a
repeat that must not be scored); 5 samples give 4 and 1 (rank 1 gets nothing of the tail: an empty share).  Every rank also
walks the unsharded loader alone (no collective): the single-process table.  Writes <outdir>/rank<r>.npz."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


class _TensorSet:
    """What DeviceLoader needs from a DeviceDataset, over two resident tensors."""

    def __init__(self, x, t):
        self.x, self.t, self.device = x, t, x.device

    def __len__(self):
        return self.x.shape[0]

    def batch(self, idx):
        return {"tactile_image": self.x[idx], "depth_image": self.t[idx], "object_index": idx}


def main():
    outdir = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", rank))
    use_rccl = torch.cuda.device_count() >= world and os.environ.get("GSD_DDP_BACKEND", "nccl") == "nccl"
    dev = torch.device("cuda", local if use_rccl else 0)
    torch.cuda.set_device(dev)
    if use_rccl:
        if os.environ.get("NCCL_DEBUG", "").upper() == "VERSION":
            del os.environ["NCCL_DEBUG"]
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from gelslim_depth_amd import harness, synth
    from gelslim_depth_amd.dataset import DeviceLoader
    from gelslim_depth_amd.metrics import SUMMARY_KEYS, DepthMetrics
    from gelslim_depth_amd.models.unet import UNet
    from gelslim_depth_amd.train import TrainStep
    spec = DepthMetrics(background=0.0, contact_eps=1e-3, unit=-3.2, unit_name="mm")
    out = {"backend": dist.get_backend()}
    for precision, dims in (("fp32", [16, 32, 64]), ("bf16", [32, 64, 128])):
        st = synth.make_state(3, 1, dims, 5 + 100 * rank, "conditioned")      # different weights per rank: rank 0's are broadcast
        m = UNet(n_channels=3, n_classes=1, layer_dimensions=dims, precision=precision)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
        m = m.to(dev).train()
        step = TrainStep(m, process_group=dist.group.WORLD)
        for n in (7, 5):
            xe, te = synth.make_batch(n, 37, 53, 9)
            keep = np.random.Generator(np.random.PCG64(70 + n)).random(te.shape) < 0.3      # depth-like: 0 off the patch
            te = np.where(keep, te, np.float32(0.0)).astype(np.float32)
            ds = _TensorSet(torch.from_numpy(xe).to(dev), torch.from_numpy(te).to(dev))
            loader = DeviceLoader(ds, batch_size=2, rank=rank, world_size=world)
            key = f"{precision}/{n}/"
            loss, summary, table = harness.evaluate_metrics(step, loader, spec, per_image=True)
            out[key + "loss"], out[key + "table"] = loss, table.numpy()
            out[key + "summary"] = np.array([float(summary[k]) for k in SUMMARY_KEYS[:-1]])
            out[key + "loss_alone"] = harness.evaluate_loader(step, loader)
            one_loss, one_summary, one_table = harness.evaluate_metrics(step, loader.unsharded(), spec, per_image=True)
            out[key + "one_loss"], out[key + "one_table"] = one_loss, one_table.numpy()
            out[key + "one_summary"] = np.array([float(one_summary[k]) for k in SUMMARY_KEYS[:-1]])
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
