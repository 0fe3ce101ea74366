"""Epoch loop around the fused step: the reference's training harness without its plotting.

Mirrors /root/reference/train_utils/train_unet.py:312-523:
  * per epoch: train pass (:337-378), validation and test passes in eval mode under the EMA weights with NaN losses
    counted as 0 (:379-458), each loss averaged over the loader's batches;
  * validation-loss smoothing: a ring of the last `val_loss_SMA_window` validation losses, initialised to ZEROS, whose mean
    is compared with the previous epoch's mean; more than `validation_loss_count_threshold` consecutive rises stop the
    run -- or, with `train_indefinitely`, are only logged (:460-474);
  * checkpoint of the EMA-swapped, reference-layout state_dict whenever the raw validation loss reaches a new minimum
    (:475-483), and `_epoch{e}` snapshots at `save_at_epochs` (0-based epoch index, :484-489);
  * the text log: the same lines, in the same order and format, as the reference writes to its loss file (:465,478,
    490-496,520-523).

The device work is libgsd's: TrainStep for the train pass, TrainStep.evaluate (kernels pointed at the EMA arena, no
store/copy/restore) + the fused loss kernel for the other two.  `max_epochs` is an addition: the reference with
train_indefinitely=True only stops when killed.
"""
from __future__ import annotations

import os
import time
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np


class EarlyStopping:
    """The reference's stopping rule as a small state machine (train_unet.py:316-323, 460-474)."""

    def __init__(self, window: int = 10, count_threshold: int = 5, train_indefinitely: bool = False) -> None:
        self.window, self.count_threshold, self.train_indefinitely = window, count_threshold, train_indefinitely
        self.validation_array = np.zeros(window)
        self.prev_validation_loss = 0.0
        self.validation_loss_upward_counter = 0
        self.min_validation_loss = 1000000
        self.e = 0

    def update(self, validation_loss: float):
        """Feed epoch e's validation loss.  Returns (stop, stalled_message_needed, new_minimum)."""
        self.validation_array[self.e % self.window] = validation_loss
        smoothed = float(np.mean(self.validation_array))
        if smoothed > self.prev_validation_loss:
            self.validation_loss_upward_counter += 1
        else:
            self.validation_loss_upward_counter = 0
        stop = stalled = False
        if self.validation_loss_upward_counter > self.count_threshold:
            stop = True
            if self.train_indefinitely:
                stalled, stop = True, False
        self.prev_validation_loss = smoothed
        new_min = validation_loss < self.min_validation_loss
        if new_min:
            self.min_validation_loss = validation_loss
        self.e += 1
        return stop, stalled, new_min

    def state_dict(self) -> Dict[str, object]:
        """Every field, as plain Python values."""
        return {"window": self.window, "count_threshold": self.count_threshold, "train_indefinitely": self.train_indefinitely,
                "validation_array": [float(v) for v in self.validation_array],
                "prev_validation_loss": float(self.prev_validation_loss),
                "validation_loss_upward_counter": self.validation_loss_upward_counter,
                "min_validation_loss": float(self.min_validation_loss), "e": self.e}

    def load_state_dict(self, sd: Dict[str, object]) -> None:
        self.window, self.count_threshold = int(sd["window"]), int(sd["count_threshold"])
        self.train_indefinitely = bool(sd["train_indefinitely"])
        self.validation_array = np.array(sd["validation_array"], dtype=np.float64)
        self.prev_validation_loss = sd["prev_validation_loss"]
        self.validation_loss_upward_counter = int(sd["validation_loss_upward_counter"])
        self.min_validation_loss = sd["min_validation_loss"]
        self.e = int(sd["e"])


def _mean_loss(losses: List[float], n_batches: int) -> float:
    return float(sum(losses) / n_batches) if n_batches else 0.0


def _evaluate_walk(step, loader: Iterable[Dict], loss_kind, metrics, who: str):
    """The one evaluation walk behind evaluate_loader and evaluate_metrics: (mean loss, table, (m, pairs)).  Without
    `metrics` the table is None and nothing but the loss launch follows a forward; with a metrics.DepthMetrics the metrics
    launch reads the same output and target as the loss launch, and the table -- one row per sample of the pass, in walk order,
    float64 on the CPU -- comes back with the batch losses when the pass ends."""
    import torch
    from .train import DepthLoss, depth_loss_fwd_bwd, depth_loss_workspace, loss_fwd_bwd
    depth = isinstance(loss_kind, DepthLoss)
    sharded = getattr(loader, "world_size", 1) > 1 and hasattr(loader, "eval_shares")
    if sharded and (getattr(step, "pg", None) is None or getattr(step, "dist", None) is None):
        raise RuntimeError("%s: the loader is sharded over %d ranks but the step was built without a process_group; "
                           "pass the group to TrainStep or evaluate loader.unsharded()" % (who, loader.world_size))
    if metrics is not None:
        from .metrics import COLS, depth_metrics, depth_metrics_workspace, pairs_per_image
    buf = ws = mws = None
    rows = []          # per (global) batch: device tensor [loss sum over this rank's valid elements, their count]
    tabs = []          # with metrics, per scored share: (its first sample's position in the walk, its (valid, 16) device table)
    seen = 0           # samples of the pass walked so far, over all ranks
    image = (0, 0)     # elements and neighbour pairs of one image
    dev = None
    walk = loader.eval_shares() if sharded else ((data, None, None) for data in loader)
    for data, valid, global_count in walk:
        if data is None:                  # the ragged tail left this rank nothing of this global batch
            rows.append(None)
            seen += global_count
            continue
        x, t = data["tactile_image"], data["depth_image"]
        out = step.evaluate(x, use_ema=True)
        if buf is None:
            dev = out.device
            buf = torch.zeros((6 if depth else 1,), device=dev, dtype=torch.float32)
            ws = torch.empty((2048,), device=dev, dtype=torch.float64)
        t = t.float().contiguous()
        first = seen + (loader.rank * loader.batch_size if sharded else 0)
        seen += global_count if sharded else int(out.shape[0])
        if valid is not None and valid < out.shape[0]:
            out, t = out[:valid], t[:valid]       # leading-dimension slices stay contiguous: the padding is not scored
        if depth:
            if ws.numel() < depth_loss_workspace(out.shape):
                ws = torch.empty((depth_loss_workspace(out.shape),), device=dev, dtype=torch.float64)
            depth_loss_fwd_bwd(loss_kind, out, t, None, buf, ws)       # buf[0] is L; its normalisers are element counts
        else:
            loss_fwd_bwd(loss_kind, out, t, None, buf, ws)
        rows.append((buf[0].double().clone(), float(out.numel())))      # the element counts stay on the host
        if metrics is not None:
            if mws is None or mws.numel() < depth_metrics_workspace(out.shape):
                mws = torch.empty((depth_metrics_workspace(out.shape),), device=dev, dtype=torch.float64)
            tabs.append((first, depth_metrics(out, t, metrics, None, mws)))      # a table of its own per batch: it is kept
            image = (int(out[0].numel()), pairs_per_image(*(int(d) for d in out.shape[1:])))
    if dev is None:
        dev = getattr(getattr(step, "p_flat", None), "device", None) or torch.device("cpu")
    table = None
    if metrics is not None:
        # every sample of the pass has one row; a rank fills in the rows it scored, the rest stay zero, and one all-reduce
        # (adding zeros is exact) leaves every rank with the same complete table.  One more row carries the image size to a
        # rank whose shares were all empty: (m, pairs, 1) from every rank that scored something -- small integers, exact
        table = torch.zeros((seen + (1 if sharded else 0), COLS), device=dev, dtype=torch.float64)
        for first, tab in tabs:
            table[first:first + tab.shape[0]] = tab
        if sharded:
            if tabs:
                table[seen, :3] = torch.tensor([float(image[0]), float(image[1]), 1.0], dtype=torch.float64).to(dev)
            step.dist.all_reduce(table, group=step.pg)
        table = table.cpu()
        if sharded:
            last, table = table[seen].tolist(), table[:seen].contiguous()
            image = (int(last[0] / last[2]), int(last[1] / last[2])) if last[2] > 0 else (0, 0)
    if not rows:
        return 0.0, table, image
    counts = torch.tensor([r[1] if r is not None else 0.0 for r in rows], dtype=torch.float64)
    zero = torch.zeros((), device=dev, dtype=torch.float64)
    losses = torch.stack([r[0] if r is not None else zero for r in rows])
    if not sharded:
        vals = losses.cpu().tolist()                                    # single process: the batch losses themselves
    else:
        tab = torch.stack([losses * counts.to(dev), counts.to(dev)], dim=1)      # one upload, one all-reduce, one download
        step.dist.all_reduce(tab, group=step.pg)
        tab = tab.cpu()
        if bool((tab[:, 1] == 0).any()):
            raise RuntimeError("%s: a global batch was scored by no rank (the ranks' loaders disagree on the batch order)" % who)
        vals = (tab[:, 0] / tab[:, 1]).tolist()
    return _mean_loss([0.0 if v != v else v for v in vals], len(vals)), table, image


def evaluate_loader(step, loader: Iterable[Dict], loss_kind="mse") -> float:
    """Mean over the loader's batches of the loss under the EMA weights, NaN batches counted as 0 (train_unet.py:379-419).
    `loss_kind`: "mse" (the reference's, and what `fit` scores), "l1", or a train.DepthLoss, whose total L is averaged.

    Data parallel (a `DeviceLoader` with world_size > 1): the walk is over the GLOBAL batches, every rank evaluates only its
    contiguous share of each at the per-rank train shape (`DeviceLoader.eval_shares`: no wrap-around padding, no activation
    buffer reallocated, nothing evaluated twice), and ONE all-reduce at the end of the pass sums (loss sum, element count) per
    global batch -- every rank then holds the single-process value of every batch loss, bit for bit the same on all ranks.
    The batch losses stay on the device until the pass ends (one host sync per pass; the reference syncs per batch)."""
    return _evaluate_walk(step, loader, loss_kind, None, "evaluate_loader")[0]


def evaluate_metrics(step, loader: Iterable[Dict], spec, loss_kind="mse", per_image: bool = False):
    """`evaluate_loader`'s walk with the per-image depth metrics of `spec` (a metrics.DepthMetrics) taken on the way: returns
    (loss, summary), or (loss, summary, table) with `per_image`.  `loss` is exactly evaluate_loader(step, loader, loss_kind);
    `summary` is metrics.summarise of the pass; `table` holds one row per sample (the columns of gsd_depth_metrics,
    include/gsd.h; float64, CPU) in walk order -- dataset row order for shuffle=False: the handle for finding the worst samples.

    One forward per batch: the loss launch and the metrics launch read the same output, and nothing is synchronised until the
    pass ends.  Data parallel: every rank scores only the valid leading images of its shares (padded repeats never), places
    their rows by position in the global walk into a zero-filled table of all samples, and one all-reduce (128 bytes per
    sample) gives every rank the complete table; the summary is computed from identical rows in identical order and is
    therefore the same on every rank bit for bit.  A row's bits depend on its image alone, so the table equals the
    single-process one whenever the eval forward's bits do not depend on the batch (the fp32 engine's do not)."""
    from .metrics import DepthMetrics, summarise
    if not isinstance(spec, DepthMetrics):
        raise TypeError(f"evaluate_metrics: spec must be a metrics.DepthMetrics, got {type(spec).__name__}")
    loss, table, image = _evaluate_walk(step, loader, loss_kind, spec, "evaluate_metrics")
    summary = summarise(table, image, spec)
    return (loss, summary, table) if per_image else (loss, summary)


FIT_STATE_FORMAT = "gelslim_depth_amd.harness.fit"


def _save_fit_state(step, path: str, loop: Dict[str, object]) -> None:
    import torch
    from .train import atomic_save
    loop = dict(loop, torch_rng=torch.get_rng_state(),
                cuda_rng=torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    atomic_save({"format": FIT_STATE_FORMAT, "version": 1, "train_step": step.state_dict(), "loop": loop}, path)


def _check_augment_spec(saved: Optional[Dict[str, object]], now: Optional[Dict[str, object]]) -> None:
    """A resumed run continues the SAME augmentation stream: refuse a train loader whose Augment differs from the saved one
    (a state file written before augmentation existed carries no spec and is read as None)."""
    if saved == now:
        return
    if saved is None or now is None:
        raise ValueError("fit(resume=True): augment differs from the saved run's (saved %r, now %r)" % (saved, now))
    for k in sorted(set(saved) | set(now)):
        if saved.get(k) != now.get(k):
            raise ValueError("fit(resume=True): augment field %r differs from the saved run's (saved %r, now %r)"
                             % (k, saved.get(k), now.get(k)))


def _restore_fit_state(step, path: str, is_main: bool, augment_spec: Optional[Dict[str, object]] = None) -> Optional[Dict[str, object]]:
    """The loop's saved state, after the step's and the RNG states have been restored; None when there is no file.  Data
    parallel: rank 0 reads the file, the loop's state goes to every rank with broadcast_object_list, the step's arenas by
    its own broadcast (TrainStep.load_state_dict)."""
    import torch
    from .train import read_state
    blob = read_state(path) if (is_main and os.path.exists(path)) else None
    if blob is not None and (not isinstance(blob, dict) or blob.get("format") != FIT_STATE_FORMAT):
        raise ValueError(f"{path} is not a harness.fit state file (written by fit(..., state_path=...))")
    loop = None if blob is None else blob["loop"]
    if getattr(step, "world", 1) > 1:
        box = [loop]
        step.dist.broadcast_object_list(box, src=0, group=step.pg)
        loop = box[0]
    if loop is None:
        return None
    _check_augment_spec(loop.get("augment"), augment_spec)      # refused before anything is restored
    step.load_state_dict(None if blob is None else blob["train_step"])
    torch.set_rng_state(loop["torch_rng"])
    if loop["cuda_rng"] is not None and torch.cuda.is_available():
        for i, s in enumerate(loop["cuda_rng"][:torch.cuda.device_count()]):
            torch.cuda.set_rng_state(s, i)
    return loop


def fit(step, train_loader, val_loader, test_loader, weights_path: str, weights_name: str, loss_values_path: Optional[str] = None,
        val_loss_SMA_window: int = 10, validation_loss_count_threshold: int = 5, train_indefinitely: bool = False,
        save_at_epochs: Sequence[int] = (), max_epochs: Optional[int] = None,
        train_pass: Optional[Callable] = None, eval_pass: Optional[Callable] = None, save: Optional[Callable] = None,
        echo: Callable[[str], None] = print, state_path: Optional[str] = None, resume: bool = False,
        state_every: int = 1, metrics=None) -> Dict[str, List[float]]:
    """Run epochs until the stopping rule fires (or `max_epochs`).  Returns H = {train_loss, validation_loss, test_loss}.

    `train_pass(step, loader) -> (sum_of_batch_losses, n_batches)`, `eval_pass(step, loader) -> mean_loss` and
    `save(step, path)` default to the libgsd implementations; tests substitute host stubs for them.

    Resumable runs (an addition; off by default): with `state_path`, rank 0 writes one file at the end of every
    `state_every`-th epoch and of the last epoch, after that epoch's log lines and checkpoints -- the step's
    `state_dict()` and the loop's own state: the next epoch, the stopping rule's fields, H, the elapsed training time and
    the torch RNG states (the CPU generator orders DeviceLoader's shuffles) and the train loader's `Augment.spec()` (None
    without augmentation).  Before every train pass the loader is told the epoch (`train_loader.set_epoch(e)`, when it
    has that method): the augmentation stream is a function of (seed, epoch, dataset row), so a resumed run draws what the
    uninterrupted one would; resuming with a loader whose spec differs raises ValueError naming the field.  With `resume=True` and that file present, all
    of it is restored before the first epoch and the run continues at the saved epoch (a run the stopping rule ended
    stays ended); `max_epochs` counts every epoch, the interrupted ones included.  The resumed part writes only the lines of its own epochs to the log file (a one-line
    notice goes to `echo`), so the concatenated log equals an uninterrupted run's apart from the timing lines and the
    first part's closing lines.  Resume is per epoch: a run killed after the last file repeats the epochs since, log lines
    included.

    Data parallel (a build-side addition, the reference is single-process): every rank runs the same epochs on its shard
    of each batch; the epoch losses are averaged over the ranks (`step.mean_across_ranks`) so that all ranks take the
    same stopping and checkpoint decisions, and only rank 0 writes checkpoints, the log file and the echo.  Validation and
    test passes walk the GLOBAL batches with every rank scoring its own share (`evaluate_loader`): the value is the
    single-process one (no wrap-around padding in the loss early stopping reads), identical on every rank, at the per-rank
    train shape; `across()` of it is then the identity up to the last bit.

    `metrics` (a metrics.DepthMetrics; None: everything as without it): H gains `validation_metrics` and `test_metrics`, one
    metrics.summarise dict per epoch, and rank 0 emits one more line per epoch, directly after the `Train loss: ...` line
    (metrics.log_line has the format).  With the default `eval_pass` the validation and test passes become
    `evaluate_metrics` walks -- no second forward over either set; with a caller-supplied `eval_pass` the metrics are a walk
    of their own over the loaders that pass sees.  Both lists are saved with H; a resume from a file without them pads the
    earlier epochs with None.  The stopping rule still reads the validation loss."""
    if state_every < 1:
        raise ValueError(f"state_every must be at least 1, got {state_every}")
    if train_pass is None:
        from .dataset import train_epoch as train_pass
    if metrics is not None:
        from .metrics import DepthMetrics, log_line
        if not isinstance(metrics, DepthMetrics):
            raise TypeError(f"fit: metrics must be a metrics.DepthMetrics or None, got {type(metrics).__name__}")
    fused_metrics = metrics is not None and eval_pass is None
    if eval_pass is None:
        eval_pass = evaluate_loader
    elif getattr(val_loader, "world_size", 1) > 1 and hasattr(val_loader, "unsharded"):
        # a caller-supplied pass does not know about shares: it gets single-process loaders (no wrap-around-padded shards in the
        # loss early stopping reads); the default pass scores every rank's share of the GLOBAL batches instead
        val_loader, test_loader = val_loader.unsharded(), test_loader.unsharded()
    if save is None:
        def save(st, path):
            st.save_checkpoint(path, use_ema=True)
    H: Dict[str, List[float]] = {"train_loss": [], "validation_loss": [], "test_loss": []}
    METRIC_KEYS = ("validation_metrics", "test_metrics")
    stopper = EarlyStopping(val_loss_SMA_window, validation_loss_count_threshold, train_indefinitely)
    is_main = getattr(step, "rank", 0) == 0
    across = getattr(step, "mean_across_ranks", float)
    log = open(loss_values_path, "a") if (loss_values_path and is_main) else None

    def emit(line: str) -> None:
        if not is_main:
            return
        echo(line)
        if log is not None:
            log.write(line + "\n")
    start = time.time()
    try:
        e, done = 0, False
        augment = getattr(train_loader, "augment", None)
        augment_spec = augment.spec() if augment is not None else None
        if resume and state_path is not None:
            saved = _restore_fit_state(step, state_path, is_main, augment_spec)
            if saved is not None:
                e, H = int(saved["epoch"]), {k: list(v) for k, v in saved["H"].items()}
                stopper.load_state_dict(saved["early_stopping"])
                start -= float(saved["elapsed"])
                done = bool(saved["stopped"]) or (max_epochs is not None and e >= max_epochs)
                if is_main:
                    echo(f"Resuming from {state_path} at epoch {e + 1}")
        if metrics is not None:
            for k in METRIC_KEYS:
                H.setdefault(k, [None] * e)      # a fresh run, or a file written without metrics
        while not done:
            t0 = time.time()
            if hasattr(train_loader, "set_epoch"):
                train_loader.set_epoch(e)       # the augmentation stream is keyed by (seed, epoch, dataset row)
            total, nb = train_pass(step, train_loader)
            train_loss = across(total / nb if nb else 0.0)
            H["train_loss"].append(train_loss)
            summaries = [None, None]
            for i, loader in enumerate((val_loader, test_loader)):
                if fused_metrics:
                    raw, summaries[i] = evaluate_metrics(step, loader, metrics)
                else:
                    raw = eval_pass(step, loader)
                    if metrics is not None:
                        summaries[i] = evaluate_metrics(step, loader, metrics)[1]
                if i == 0:
                    validation_loss = across(raw)
                    H["validation_loss"].append(validation_loss)
                else:
                    test_loss = across(raw)
                    H["test_loss"].append(test_loss)
            for k, summary in zip(METRIC_KEYS, summaries):
                if k in H:
                    H[k].append(summary)      # None in a run resumed without `metrics` from a file that has the lists
            stop, stalled, new_min = stopper.update(validation_loss)
            if stalled:
                emit(f"Validation loss stopped decreasing at epoch {e + 1}")
            if new_min:
                emit("Validation loss is at a minimum. Saving the model")
                if is_main:
                    os.makedirs(weights_path, exist_ok=True)
                    save(step, os.path.join(weights_path, weights_name + ".pth"))
            if train_indefinitely and len(save_at_epochs) > 0 and e in save_at_epochs and is_main:
                os.makedirs(weights_path, exist_ok=True)
                save(step, os.path.join(weights_path, weights_name + "_epoch" + str(e) + ".pth"))
            emit("[INFO] EPOCH: {}".format(e + 1))
            emit("Train loss: {:.6f},  Validation loss: {:.6f}, Test loss: {:.6f}".format(train_loss, validation_loss, test_loss))
            if metrics is not None:
                emit(log_line(summaries[0], summaries[1]))
            emit(f"Time for epoch: {time.time() - t0}")
            e += 1
            done = stop or (max_epochs is not None and e >= max_epochs)
            if state_path is not None and is_main and (e % state_every == 0 or done):
                if log is not None:
                    log.flush()              # the log on disk holds every line of the epochs the state has behind it
                _save_fit_state(step, state_path, {"epoch": e, "stopped": stop, "early_stopping": stopper.state_dict(),
                                                   "H": H, "elapsed": time.time() - start, "augment": augment_spec})
        emit("Training complete")
        emit("Training time: {}s".format(time.time() - start))
    finally:
        if log is not None:
            log.close()
    return H
