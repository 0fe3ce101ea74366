"""Worker for tests/test_gpu_train_state.py: one rank of a 2-rank data-parallel run that is saved after 2 steps, loaded into
fresh steps and continued for 2 more, next to the same 4 steps uninterrupted.  Backend and device as in tests/ddp_worker.py
(RCCL with a GPU per rank, else gloo on one shared card).  Only rank 0 is given the state file's path; rank 1 is given one
that does not exist, so it can only get the state by broadcast.  Writes <outdir>/rank<r>.npz."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    outdir = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", rank))
    use_rccl = torch.cuda.device_count() >= world and os.environ.get("GSD_DDP_BACKEND", "nccl") == "nccl"
    dev = torch.device("cuda", local if use_rccl else 0)
    torch.cuda.set_device(dev)
    if use_rccl:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from gelslim_depth_amd import synth
    from gelslim_depth_amd.models.unet import UNet
    from gelslim_depth_amd.train import TrainStep
    dims = [16, 32, 64]
    per = 4 // world
    data = []
    for i in range(4):
        x, t = synth.make_batch(4, 37, 53, 30 + i)
        data.append((torch.from_numpy(x[rank * per:(rank + 1) * per]).to(dev), torch.from_numpy(t[rank * per:(rank + 1) * per]).to(dev)))

    def fresh(seed):
        # every rank starts from different weights; the construction broadcast, then the state's, must fix that
        m = UNet(n_channels=3, n_classes=1, layer_dimensions=dims)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.make_state(3, 1, dims, seed + 100 * rank).items()})
        m = m.to(dev).train()
        return m, TrainStep(m, process_group=dist.group.WORLD, sync_bn=True, nan_policy="skip")

    def snapshot(tag, m, step, losses):
        out = {f"{tag}/loss": np.array(losses), f"{tag}/p": step.p_flat.cpu().numpy(), f"{tag}/m": step.m_flat.cpu().numpy(),
               f"{tag}/v": step.v_flat.cpu().numpy(), f"{tag}/ema": step.ema_flat.cpu().numpy(),
               f"{tag}/guard": step.guard_words.cpu().numpy(), f"{tag}/counts": np.array([step.step_count, step.ema_updates])}
        for k, b in m.named_buffers():
            out[f"{tag}/buf/{k}"] = b.cpu().numpy()
        return out

    m, step = fresh(5)
    losses = [step(x, t).item() for x, t in data]
    out = snapshot("straight", m, step, losses)
    m, step = fresh(5)
    losses = [step(x, t).item() for x, t in data[:2]]
    path = os.path.join(outdir, "state.pt")
    step.save_state(path)
    dist.barrier()
    m, step = fresh(9)
    step.load_state(path if rank == 0 else os.path.join(outdir, f"no_such_file_on_rank{rank}.pt"))
    losses += [step(x, t).item() for x, t in data[2:]]
    out.update(snapshot("resumed", m, step, losses))
    out["backend"] = dist.get_backend()
    dist.barrier()
    out["files"] = np.array(sorted(os.listdir(outdir)))
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
