"""GPU: TrainStep.save_state / load_state and harness.fit(state_path=..., resume=True).  A run saved after k steps (epochs)
and continued in a fresh model and step is, bit for bit, the run that was never interrupted: per-step losses, parameters, Adam
moments, EMA shadow, every BatchNorm buffer, the guard's words; fp32 state loads into a bf16 step; mismatches are refused."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from gelslim_depth_amd import synth

pytestmark = pytest.mark.gpu

SMALL = [32, 64, 128]
FULL = [64, 128, 256, 512, 1024]


def _model(dims, seed, precision="fp32"):
    from gelslim_depth_amd.models.unet import UNet
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=dims, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.make_state(3, 1, dims, seed, "conditioned").items()},
                      strict=True)
    return m.to("cuda").train()


def _step(dims, seed, precision="fp32", **kw):
    from gelslim_depth_amd.train import TrainStep
    m = _model(dims, seed, precision)
    return m, TrainStep(m, **kw)


def _batches(k, n, h, w, nan_at=None):
    out = []
    for i in range(k):
        x, t = synth.make_batch(n, h, w, 40 + i)
        if i == nan_at:
            x[0, 0, 3, 5] = np.nan          # non-finite BatchNorm statistics and loss: a skipped step
        out.append((torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()))
    return out


def _snapshot(m, step):
    s = {"p": step.p_flat, "m": step.m_flat, "v": step.v_flat, "ema": step.ema_flat, "guard": step.guard_words}
    s.update({"buf/" + k: b for k, b in m.named_buffers()})
    s = {k: v.detach().cpu().clone() for k, v in s.items() if v is not None}
    s["counts"] = torch.tensor([step.step_count, step.ema_updates])
    return s


def _assert_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _continuation(tmp_path, dims, shape, precision="fp32", nan_at=None, **kw):
    """5 steps straight vs 3 steps, save_state, a fresh model of another init and a fresh step, load_state, 2 steps."""
    data = _batches(5, *shape, nan_at=nan_at)
    m, step = _step(dims, 5, precision, **kw)
    want = [step(x, t).item() for x, t in data]
    ref, ref_skipped = _snapshot(m, step), step.skipped_steps()
    del m, step
    m, step = _step(dims, 5, precision, **kw)
    got = [step(x, t).item() for x, t in data[:3]]
    path = str(tmp_path / "state.pt")
    step.save_state(path)
    del m, step
    torch.cuda.empty_cache()
    m, step = _step(dims, 6, precision, **kw)
    assert not torch.equal(step.p_flat.cpu(), ref["p"])
    step.load_state(path)
    got += [step(x, t).item() for x, t in data[3:]]
    assert np.array_equal(np.array(got), np.array(want), equal_nan=True), (got, want)
    _assert_equal(_snapshot(m, step), ref)
    assert os.listdir(tmp_path) == ["state.pt"]
    return step, ref_skipped


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_continuation_is_bitwise_small(tmp_path, precision):
    _continuation(tmp_path, SMALL, (2, 40, 53), precision)


def test_continuation_is_bitwise_full_size(tmp_path):
    """BASELINE's network at 3x320x427, batch 2: the 124 MB arenas, 4 of them in the file."""
    step, _ = _continuation(tmp_path, FULL, (2, 320, 427))
    assert step.numel == 31037633
    assert os.path.getsize(tmp_path / "state.pt") > 4 * 4 * step.numel


def test_continuation_carries_the_skipped_step(tmp_path):
    step, skipped = _continuation(tmp_path, SMALL, (2, 40, 53), nan_at=1, nan_policy="skip")
    assert skipped == 1 and step.skipped_steps() == 1


def test_fp32_state_loads_into_bf16(tmp_path):
    data = _batches(3, 2, 40, 53)
    m, step = _step(SMALL, 5)
    for x, t in data[:2]:
        step(x, t)
    sd = step.state_dict()
    mb, sb = _step(SMALL, 6, "bf16")
    sb.load_state_dict(sd)
    _assert_equal(_snapshot(mb, sb), _snapshot(m, step))
    assert sb.step_count == 2
    loss = sb(*data[2]).item()
    assert np.isfinite(loss) and sb.step_count == 3


def test_load_is_in_place(tmp_path):
    """Parameter views, the gradient views and a graph captured on the model survive a load."""
    from gelslim_depth_amd.graph import GraphedInference
    data = _batches(3, 2, 40, 53)
    m, step = _step(SMALL, 5)
    for x, t in data:
        step(x, t)
    sd = step.state_dict()
    m2, s2 = _step(SMALL, 6)
    m2.eval()
    graphed = GraphedInference(m2, data[0][0])
    ptrs = [p.data_ptr() for p in m2.parameters()] + [g.data_ptr() for g in m2._grad_views.values()]
    s2.load_state_dict(sd)
    assert ptrs == [p.data_ptr() for p in m2.parameters()] + [g.data_ptr() for g in m2._grad_views.values()]
    m.eval()
    with torch.no_grad():
        want = m(x=data[0][0])
    assert torch.equal(graphed(data[0][0]), want)
    m2.train()
    m.train()
    assert torch.equal(s2(*data[0]), step(*data[0]))


def test_refusals(tmp_path):
    data = _batches(1, 2, 40, 53)
    m, step = _step(SMALL, 5)
    step(*data[0])
    path = str(tmp_path / "state.pt")
    step.save_state(path)
    _, other = _step([16, 32, 64], 6)
    with pytest.raises(ValueError, match=r"'inc\.double_conv\.0\.weight' differs.*layer_dimensions \[32, 64, 128\]"):
        other.load_state(path)
    m2, s2 = _step(SMALL, 6, lr=2e-3)
    before = s2.p_flat.clone()
    with pytest.raises(ValueError, match="lr is 0.001 in the state and 0.002 here"):
        s2.load_state(path)
    assert torch.equal(s2.p_flat, before) and s2.step_count == 0, "a refused load changes nothing"
    s2.load_state(path, strict=False)
    assert s2.lr == 2e-3 and s2.step_count == 1 and torch.equal(s2.p_flat, step.p_flat)
    _, s3 = _step(SMALL, 6, ema_decay=None)
    with pytest.raises(ValueError, match="ema_flat"):
        s3.load_state(path)
    _, s4 = _step(SMALL, 6, nan_policy="skip")
    with pytest.raises(ValueError, match="nan_policy"):
        s4.load_state(path)
    ckpt = str(tmp_path / "unet.pth")
    step.save_checkpoint(ckpt)           # the reference's weights-only layout
    with pytest.raises(ValueError, match=r"weights-only checkpoint.*model\.load_state_dict"):
        s2.load_state(ckpt)


def test_fit_resumed_equals_uninterrupted(tmp_path):
    """harness.fit on a DeviceDataset: 2 epochs with a state file, torch reseeded on purpose, a new model, step and loaders,
    resumed to 4 epochs == 4 epochs straight (H, log lines, checkpoints, final arenas)."""
    from gelslim_depth_amd import harness
    from gelslim_depth_amd.dataset import DeviceDataset, DeviceLoader
    from oracle import dataset_ref as dr
    kw = dict(use_difference_image=True, image_normalization_method="0_255_to_0_1",
              depth_normalization_method="min_max_to_0_-1", norm_scale=0.9)
    dims = [8, 16, 32]
    train_ds = DeviceDataset(objects=dr.synthetic_objects(41, [3, 3], h=42, w=54), device="cuda", **kw)
    val_ds = DeviceDataset(objects=dr.synthetic_objects(42, [2], h=42, w=54), device="cuda",
                           depth_normalization_parameters=train_ds.depth_normalization_parameters, **kw)

    def run(out, seed, max_epochs, **state):
        m, step = _step(dims, seed)
        lines = []
        H = harness.fit(step, DeviceLoader(train_ds, 4, shuffle=True), DeviceLoader(val_ds, 4), DeviceLoader(val_ds, 2),
                        str(out / "weights"), "unet_t", loss_values_path=str(out / "loss.txt"), train_indefinitely=True,
                        save_at_epochs=(0, 2), val_loss_SMA_window=2, validation_loss_count_threshold=0,
                        max_epochs=max_epochs, echo=lines.append, **state)
        return H, [l for l in lines if not l.startswith("Time for epoch") and not l.startswith("Training time")], m, step

    def checkpoints(out):
        d = out / "weights"
        return {f: torch.load(d / f, map_location="cpu") for f in sorted(os.listdir(d))}
    a, b = tmp_path / "straight", tmp_path / "resumed"
    a.mkdir()
    b.mkdir()
    torch.manual_seed(0)
    H0, lines0, m0, s0 = run(a, 4, 4)
    ref = _snapshot(m0, s0)
    del m0, s0
    state = str(b / "state.pt")
    torch.manual_seed(0)
    H1, lines1, _, _ = run(b, 4, 2, state_path=state)
    torch.manual_seed(12345)
    H, lines2, m, step = run(b, 7, 4, state_path=state, resume=True)
    assert lines2[0] == f"Resuming from {state} at epoch 3"
    assert H == H0 and len(H["train_loss"]) == 4
    assert lines1[-1] == "Training complete" and lines1[:-1] + lines2[1:] == lines0
    ca, cb = checkpoints(a), checkpoints(b)
    assert ca.keys() == cb.keys() == {"unet_t.pth", "unet_t_epoch0.pth", "unet_t_epoch2.pth"}
    for f in ca:
        for k in ca[f]:
            assert torch.equal(ca[f][k], cb[f][k]), (f, k)
    _assert_equal(_snapshot(m, step), ref)
    log = [l for l in (b / "loss.txt").read_text().splitlines() if not l.startswith("Time for") and not l.startswith("Training time")]
    assert log == lines1 + lines2[1:] and not os.path.exists(state + ".tmp")


def test_two_ranks_save_once_and_resume_bitwise(tmp_path):
    """Two ranks (gloo on one card, RCCL with a GPU each), SyncBN and the guard on: 2 steps, save, fresh steps, load, 2 more
    == 4 steps straight on both ranks; one file, read by rank 0 only."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29563", os.path.join(REPO, "tests", "train_state_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = [dict(np.load(os.path.join(tmp_path, f"rank{i}.npz"))) for i in range(2)]
    for rr in res:
        keys = [k[len("straight/"):] for k in rr if k.startswith("straight/")]
        assert len(keys) > 8
        for k in keys:
            assert np.array_equal(rr["straight/" + k], rr["resumed/" + k]), k
        assert [f for f in rr["files"] if f.startswith("state") or f.endswith(".tmp")] == ["state.pt"]
    assert np.array_equal(res[0]["resumed/p"], res[1]["resumed/p"])
