"""Worker for tests/test_gpu_optim_controls.py::test_one_rank_clipped_step_keeps_the_data_parallel_order: ONE rank, backend
"nccl" (RCCL), the collectives forced on (force_sync), max_grad_norm, a schedule and nan_policy="skip" set.  Records the
host-side order of the bucket all-reduces, GradSync.finish, gsd_grad_norm, the guard's MAX all-reduce and the optimiser
launch of the second step (every one of them is issued to, or waited for by, the compute stream, so the host order is the
device order), runs three steps and writes <outdir>/dp.npz."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    outdir, port, max_norm = sys.argv[1], sys.argv[2], float(sys.argv[3])
    torch.cuda.set_device(0)
    if os.environ.get("NCCL_DEBUG", "").upper() == "VERSION":
        del os.environ["NCCL_DEBUG"]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    from gelslim_depth_amd import synth, train
    from gelslim_depth_amd.models.unet import UNet
    dims = [16, 32, 64]
    st = synth.make_state(3, 1, dims, 5, "conditioned")
    x, t = synth.make_batch(2, 21, 27, 6)
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=dims)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    m = m.to("cuda:0").train()
    step = train.TrainStep(m, process_group=dist.group.WORLD, overlap_allreduce=True, force_sync=True, nan_policy="skip",
                           max_grad_norm=max_norm, lr_schedule=train.LRSchedule(warmup_steps=2))
    assert step.sync is not None and step.sync.force, "the collectives must run"
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    losses = [float(step(xd, td).item())]
    events = []

    real_lib, real_reduce, real_finish = train.lib, dist.all_reduce, step.sync.finish

    class Lib:       # libgsd with three entry points reporting when they are called
        def __getattr__(self, name):
            fn = getattr(real_lib, name)
            if name not in ("gsd_grad_norm", "gsd_adam_ema_clip", "gsd_adam_ema"):
                return fn

            def call(*a):
                events.append(name)
                return fn(*a)
            return call

    def all_reduce(tensor, *a, **kw):
        events.append("all_reduce:guard" if tensor.dtype == torch.int32 else "all_reduce:bucket")
        return real_reduce(tensor, *a, **kw)

    def finish():
        real_finish()
        events.append("finish")
    train.lib, dist.all_reduce, step.sync.finish = Lib(), all_reduce, finish
    try:
        losses.append(float(step(xd, td).item()))
    finally:
        train.lib, dist.all_reduce, step.sync.finish = real_lib, real_reduce, real_finish
    losses.append(float(step(xd, td).item()))
    torch.cuda.synchronize()
    out = {"losses": np.array(losses), "events": np.array(events), "p": step.p_flat.cpu().numpy(), "m": step.m_flat.cpu().numpy(),
           "v": step.v_flat.cpu().numpy(), "ema": step.ema_flat.cpu().numpy(), "clip": step.clip_buf.cpu().numpy(),
           "skipped": step.skipped_steps(), "backend": dist.get_backend()}
    np.savez(os.path.join(outdir, "dp.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
