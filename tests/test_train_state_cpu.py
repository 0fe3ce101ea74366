"""CPU: resumable training in gelslim_depth_amd/harness.py.  EarlyStopping round-trips its state, and harness.fit saved at
epoch k and resumed gives the run that was never interrupted: the same H, log lines, checkpoints, RNG draws and step state.
The step is a host stand-in with state_dict / load_state_dict; the train pass is the real dataset.train_epoch over a
DeviceLoader on CPU tensors, so the shuffles draw from torch's global generator as they do on the GPU."""
import io

import numpy as np
import pytest
import torch

from gelslim_depth_amd import harness
from gelslim_depth_amd.dataset import DeviceLoader


def _round_trip(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


def _val_sequence(n=40, seed=3):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (1.0 / (1 + t) + 0.002 * np.maximum(t - 12, 0) ** 1.5 + 0.01 * rng.standard_normal(n)).tolist()


@pytest.mark.parametrize("window,threshold,indefinitely", [(10, 5, False), (3, 1, True), (4, 2, False)])
@pytest.mark.parametrize("n_first", [1, 4, 11, 17])
def test_early_stopping_round_trip_equals_straight_run(window, threshold, indefinitely, n_first):
    val = _val_sequence()
    straight = harness.EarlyStopping(window, threshold, indefinitely)
    want = [straight.update(v) for v in val]
    first = harness.EarlyStopping(window, threshold, indefinitely)
    got = [first.update(v) for v in val[:n_first]]
    second = harness.EarlyStopping()          # default settings: the state brings its own
    second.load_state_dict(_round_trip(first.state_dict()))
    got += [second.update(v) for v in val[n_first:]]
    assert got == want
    assert second.state_dict() == straight.state_dict()
    assert any(s[0] or s[1] for s in want[n_first:]), "no stop / stall after the split: the test shows nothing"
    assert any(not s[2] for s in want[n_first:]) and any(s[2] for s in want)


class _Samples:
    """What DeviceLoader needs from a DeviceDataset, over CPU tensors."""

    def __init__(self, x):
        self.x, self.device = x, x.device

    def __len__(self):
        return self.x.shape[0]

    def batch(self, idx):
        return {"tactile_image": self.x[idx], "depth_image": self.x[idx, :1], "object_index": idx}


class _Step:
    """Host stand-in for TrainStep: a weight vector pulled towards every batch's first sample (order-dependent, like SGD)
    and a batch counter; eval passes read both.  Its state is what a resume must carry."""
    rank = 0

    def __init__(self, seed):
        self.w = torch.randn(4, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
        self.n = 0

    def __call__(self, x, t):
        loss = ((x - self.w) ** 2).mean() + 0.0 * t.sum()
        self.w = self.w + 0.3 * (x[0] - self.w)
        self.n += 1
        return loss

    def state_dict(self):
        return {"w": self.w.clone(), "n": self.n}

    def load_state_dict(self, sd):
        self.w, self.n = sd["w"].clone(), int(sd["n"])


def _eval_pass(step, loader):
    # lowest after 12 batches (epoch 3 of 4 batches each): minima, then rises and stalls; w adds the data's noise
    target = 0.5 if loader == "val" else 0.6
    return 0.01 * (step.n / 4 - 3) ** 2 + 0.01 * float(((step.w - target) ** 2).sum())


def _data():
    return _Samples(torch.from_numpy(np.random.default_rng(11).random((10, 4))))


def _fit(tmp_path, step, max_epochs, state_path=None, resume=False, train_pass=None, **kw):
    lines, saves = [], []

    def save(st, path):
        saves.append((path.split("/")[-1], st.w.clone()))
    args = dict(val_loss_SMA_window=2, validation_loss_count_threshold=0, train_indefinitely=True, save_at_epochs=(1, 3))
    args.update(kw)
    H = harness.fit(step, DeviceLoader(_data(), 3, shuffle=True), "val", "test", str(tmp_path / "weights"), "unet_s",
                    loss_values_path=str(tmp_path / "loss.txt"), max_epochs=max_epochs, train_pass=train_pass,
                    eval_pass=_eval_pass, save=save, echo=lines.append, state_path=state_path, resume=resume, **args)
    return H, lines, saves


def _untimed(lines):
    return [l for l in lines if not l.startswith("Time for epoch") and not l.startswith("Training time")]


def _straight(tmp_path, max_epochs, **kw):
    tmp_path.mkdir()
    torch.manual_seed(0)
    step = _Step(1)
    H, lines, saves = _fit(tmp_path, step, max_epochs, **kw)
    return H, lines, saves, step, torch.get_rng_state(), (tmp_path / "loss.txt").read_text().splitlines()


def _same_saves(a, b):
    assert [n for n, _ in a] == [n for n, _ in b]
    assert all(torch.equal(u, v) for (_, u), (_, v) in zip(a, b))


@pytest.mark.parametrize("splits", [(2,), (1, 3), (2, 4)])
def test_fit_resumed_equals_uninterrupted(tmp_path, splits):
    H0, lines0, saves0, step0, rng0, log0 = _straight(tmp_path / "straight", 5)
    assert any("stopped decreasing" in l for l in lines0[-8:]) and lines0.count("Validation loss is at a minimum. Saving the model") >= 2
    run = tmp_path / "split"
    state = str(run / "state.pt")
    run.mkdir()
    torch.manual_seed(0)
    H, lines, saves = _fit(run, _Step(1), splits[0], state_path=state)
    assert lines[-2] == "Training complete"
    lines = lines[:-2]
    for k, stop_at in enumerate(list(splits[1:]) + [5]):
        torch.manual_seed(1000 + k)           # another seed on purpose: the saved generator state must be what is restored
        H, more, s = _fit(run, _Step(77 + k), stop_at, state_path=state, resume=True)
        assert more[0] == f"Resuming from {state} at epoch {splits[k] + 1}"
        saves += s
        lines += more[1:-2] if stop_at < 5 else more[1:]
    assert H == H0
    assert _untimed(lines) == _untimed(lines0)
    _same_saves(saves, saves0)
    assert torch.equal(torch.get_rng_state(), rng0), "the resumed run drew what the uninterrupted one drew"
    log = _untimed((run / "loss.txt").read_text().splitlines())
    closing = [i for i, l in enumerate(log) if l == "Training complete"]
    assert len(closing) == len(splits) + 1 and not any(l.startswith("Resuming") for l in log)
    assert [l for i, l in enumerate(log) if i not in closing[:-1]] == _untimed(log0)
    assert not (run / "state.pt.tmp").exists()


def test_fit_state_every_and_a_killed_run(tmp_path):
    """state_every=2: a run killed in epoch 4 resumes from the file of epoch 2 and repeats epoch 3 exactly."""
    H0, lines0, saves0, step0, rng0, _ = _straight(tmp_path / "straight", 5)
    from gelslim_depth_amd.dataset import train_epoch
    calls = {"n": 0}

    def dies_in_epoch_4(step, loader):
        calls["n"] += 1
        if calls["n"] == 4:
            raise KeyboardInterrupt
        return train_epoch(step, loader)
    run = tmp_path / "split"
    run.mkdir()
    state = str(run / "state.pt")
    torch.manual_seed(0)
    with pytest.raises(KeyboardInterrupt):
        _fit(run, _Step(1), 5, state_path=state, state_every=2, train_pass=dies_in_epoch_4)
    torch.manual_seed(5)
    step = _Step(2)
    H, more, _ = _fit(run, step, 5, state_path=state, resume=True, state_every=2)
    assert more[0] == f"Resuming from {state} at epoch 3"
    assert H == H0 and torch.equal(step.w, step0.w) and step.n == step0.n
    assert _untimed(more[1:]) == _untimed(lines0)[_untimed(lines0).index("[INFO] EPOCH: 2") + 2:]
    assert torch.equal(torch.get_rng_state(), rng0)


def test_fit_resume_after_the_stopping_rule_runs_no_epoch(tmp_path):
    H0, lines0, _, step0, _, _ = _straight(tmp_path / "straight", 30, train_indefinitely=False)
    assert len(H0["validation_loss"]) < 30, "the stopping rule never fired"
    run = tmp_path / "split"
    run.mkdir()
    state = str(run / "state.pt")
    torch.manual_seed(0)
    _fit(run, _Step(1), 30, state_path=state, train_indefinitely=False)
    step = _Step(3)
    H, more, saves = _fit(run, step, 40, state_path=state, resume=True, train_indefinitely=False)
    assert H == H0 and torch.equal(step.w, step0.w) and saves == []
    assert _untimed(more) == [f"Resuming from {state} at epoch {len(H0['validation_loss']) + 1}", "Training complete"]


def test_fit_resume_without_a_file_starts_fresh(tmp_path):
    H0, lines0, saves0, _, _, _ = _straight(tmp_path / "straight", 3)
    run = tmp_path / "fresh"
    run.mkdir()
    torch.manual_seed(0)
    H, lines, saves = _fit(run, _Step(1), 3, state_path=str(run / "state.pt"), resume=True)
    assert H == H0 and _untimed(lines) == _untimed(lines0)
    _same_saves(saves, saves0)
    saved = torch.load(run / "state.pt", weights_only=True)
    assert saved["loop"]["epoch"] == 3 and saved["train_step"]["n"] == 3 * 4


def test_fit_refuses_a_file_that_is_not_a_fit_state(tmp_path):
    torch.save({"w": torch.zeros(3)}, tmp_path / "other.pt")
    with pytest.raises(ValueError, match="not a harness.fit state"):
        _fit(tmp_path, _Step(1), 2, state_path=str(tmp_path / "other.pt"), resume=True)
    with pytest.raises(ValueError, match="state_every"):
        _fit(tmp_path, _Step(1), 2, state_path=str(tmp_path / "s.pt"), state_every=0)
