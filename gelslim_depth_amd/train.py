"""The reference's train-step body as one fused schedule of libgsd kernels.

Reference (paths under /root/reference/):
    optimizer.zero_grad(); output = unet(x=input_image)            train_utils/train_unet.py:346-347
    pred_loss = MSE_loss(input=output, target=output_target)       :370  (def :51-52)
    loss.backward(); optimizer.step(); ema.update()                :374-376
    Adam(lr=1e-3, weight_decay=1e-6) :306, ExponentialMovingAverage(decay=0.995) :309

Here: forward -> loss+grad kernel -> backward -> (RCCL all-reduce of the flat gradient arena, bucketed and
overlapped with the rest of backward) -> one fused Adam+EMA kernel over the flat parameter arena.
No autograd graph, no per-tensor optimiser launches, no host sync inside the step (the loss stays on the
device; call .item() when you want it).

The reference's NaN guard (train_unet.py:371-372) replaces a NaN loss by a constant without grad_fn, after which
loss.backward() raises; it costs a host sync per step.  Here it is a device-side flag (`nan_policy`, gsd_guard in
include/gsd.h): a step whose loss or BatchNorm batch statistics are non-finite leaves parameters, Adam moments and the
EMA shadow untouched and is counted on the device (non-finite batch statistics never reach the running statistics, with
or without a policy).  A skipped step still consumes a tick of the two host-side schedules -- Adam's bias-correction step
count and torch_ema's warm-up count ((1+n)/(10+n)) advance as if the step had been applied, where torch / torch_ema would
not have counted it; either factor changes by less than 1/t from tick t to t+1, so the effect of a skipped step fades with
the step count -- "skip" carries on, "raise" raises GsdError at
the next `check_finite()` (train_epoch calls it once per epoch: one host sync per epoch instead of two per step),
None (default) runs the reference's arithmetic unguarded.

Two additions the reference lacks, both off by default: `max_grad_norm` clips the all-reduced, averaged
gradient by its global L2 norm as torch.nn.utils.clip_grad_norm_ would -- one reduction over the gradient arena
(gsd_grad_norm) whose coefficient stays on the device and is applied inside the optimiser kernel (gsd_adam_ema_clip) --
and `lr_schedule` (LRSchedule: linear warm-up, then constant, linear or cosine decay) makes the learning rate a pure
function of the step count, so a resumed run continues its schedule.

A third: `loss` may be a DepthLoss -- a Huber / L1 / MSE data term, a heavier weight on contact pixels and a
multi-scale slope term on the error image, one libgsd kernel (gsd_depth_loss_fwd_bwd) in the place of the plain loss launch.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, List, Optional, Tuple, Union

import torch

from . import _lib as L
from ._lib import lib, check
from .models.unet import UNet

LOSS_KINDS = {"mse": 0, "l1": 1}

STATE_FORMAT = "gelslim_depth_amd.TrainStep"
STATE_VERSION = 2          # the newest this build reads; a state without max_grad_norm / lr_schedule is still written as 1
STATE_HPARAMS = ("lr", "betas", "eps", "weight_decay", "ema_decay", "loss", "nan_policy", "max_grad_norm", "lr_schedule")

LR_DECAYS = ("constant", "linear", "cosine")


class LRSchedule:
    """Learning rate as a function of the 1-based step count t (an addition: the reference trains at one constant rate):
    a linear warm-up over `warmup_steps` steps, lr * t / warmup_steps, then `decay` from the base rate towards `min_lr`,
    reached at step `total_steps` and held from there on -- "constant" (no decay), "linear" or "cosine" (half a cosine
    wave).  `lr_at` is the formula.  A value class: comparable, hashable, `LRSchedule(**s.spec()) == s`."""

    def __init__(self, warmup_steps: int = 0, decay: str = "constant", total_steps: Optional[int] = None,
                 min_lr: float = 0.0) -> None:
        def whole(name, v):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"LRSchedule: {name} must be a whole number of steps, got {v!r}")
            return int(v)
        self.warmup_steps = whole("warmup_steps", warmup_steps)
        if self.warmup_steps < 0:
            raise ValueError(f"LRSchedule: warmup_steps must not be negative, got {warmup_steps!r}")
        if decay not in LR_DECAYS:
            raise ValueError(f"LRSchedule: decay must be one of {', '.join(repr(d) for d in LR_DECAYS)}, got {decay!r}")
        self.decay = decay
        self.total_steps = None if total_steps is None else whole("total_steps", total_steps)
        if self.total_steps is not None and self.total_steps <= 0:
            raise ValueError(f"LRSchedule: total_steps must be positive, got {total_steps!r}")
        if decay != "constant" and (self.total_steps is None or self.total_steps <= self.warmup_steps):
            raise ValueError(f"LRSchedule: total_steps must exceed warmup_steps ({self.warmup_steps}) for decay={decay!r}, "
                             f"got {total_steps!r}")
        try:
            self.min_lr = float(min_lr)
        except (TypeError, ValueError):
            raise ValueError(f"LRSchedule: min_lr must be a number, got {min_lr!r}") from None
        if not (0.0 <= self.min_lr < math.inf):
            raise ValueError(f"LRSchedule: min_lr must be finite and not negative, got {min_lr!r}")

    def spec(self) -> Dict[str, object]:
        """Every field as a plain Python value (TrainStep.state_dict saves it with the hyperparameters)."""
        return {"warmup_steps": self.warmup_steps, "decay": self.decay, "total_steps": self.total_steps, "min_lr": self.min_lr}

    def __eq__(self, other) -> bool:
        return isinstance(other, LRSchedule) and self.spec() == other.spec()

    def __hash__(self) -> int:
        return hash(tuple(self.spec().items()))

    def __repr__(self) -> str:
        return "LRSchedule(" + ", ".join(f"{k}={v!r}" for k, v in self.spec().items()) + ")"


def lr_at(lr: float, schedule: Optional[LRSchedule], t: int) -> float:
    """The learning rate of the 1-based step t, in float64 on the host:  warm(t) * base(t)  with
        warm = min(1, t / warmup_steps)                         (1 without warm-up)
        q    = clamp((t - warmup_steps) / (total_steps - warmup_steps), 0, 1)
        base = lr | min_lr + (lr - min_lr)(1 - q) | min_lr + (lr - min_lr)(1 + cos(pi q)) / 2     (constant | linear | cosine).
    Without a schedule, and for constant decay behind the warm-up, it is `lr` exactly."""
    lr = float(lr)
    if schedule is None:
        return lr
    w = schedule.warmup_steps
    warm = min(1.0, t / w) if w > 0 else 1.0
    if schedule.decay == "constant":
        base = lr
    else:
        q = min(1.0, max(0.0, (t - w) / (schedule.total_steps - w)))
        shape = 1.0 - q if schedule.decay == "linear" else 0.5 * (1.0 + math.cos(math.pi * q))
        base = schedule.min_lr + (lr - schedule.min_lr) * shape
    return warm * base


DEPTH_DATA_KINDS = {"mse": 0, "l1": 1, "huber": 2}
DEPTH_GRAD_KINDS = {"l1": 0, "l2": 1}
DEPTH_MAX_SCALES = 4


class DepthLoss:
    """A loss for depth maps (an addition: the reference trains on the plain MSE), with e = output - target over M elements:

        L = (1/M) sum w * rho(e)  +  grad_weight * sum_{k < grad_scales} (1/M_k) sum over the grid of step s = 2^k of
                                                  phi(e[h, w+s] - e[h, w]) + phi(e[h+s, w] - e[h, w])

    `data`: rho = e^2 ("mse"), |e| ("l1") or Huber with threshold `huber_delta` ("huber": e^2/2 up to it, linear beyond).
    `contact_weight`: w = 1 + contact_weight where |target - background| > contact_eps, 1 elsewhere (0: off).  `grad_kind`:
    phi = |g| ("l1") or g^2 ("l2"); pairs never wrap around, leave the image or cross images and classes; M_k counts the grid
    points of scale k.  The normalisers are element counts, never sum(w), so the loss of a batch is the mean of the losses of
    its equal shards and data-parallel training needs nothing new.  include/gsd.h (gsd_depth_loss) has the formula in full.
    A value class like LRSchedule: comparable, hashable, `DepthLoss(**d.spec()) == d`."""

    def __init__(self, data: str = "mse", huber_delta: Optional[float] = None, contact_weight: float = 0.0,
                 contact_eps: float = 0.0, background: float = 0.0, grad_weight: float = 0.0, grad_kind: str = "l1",
                 grad_scales: int = 0) -> None:
        def number(name, v, what="finite and not negative", low=0.0):
            try:
                f = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"DepthLoss: {name} must be a number, got {v!r}") from None
            if not (low <= f < math.inf):
                raise ValueError(f"DepthLoss: {name} must be {what}, got {v!r}")
            return f
        if data not in DEPTH_DATA_KINDS:
            raise ValueError(f"DepthLoss: data must be one of {', '.join(repr(d) for d in DEPTH_DATA_KINDS)}, got {data!r}")
        self.data = data
        if data == "huber":
            if huber_delta is None:
                raise ValueError("DepthLoss: huber_delta is required for data='huber'")
            self.huber_delta = number("huber_delta", huber_delta, "finite and positive")
            if not self.huber_delta > 0.0:
                raise ValueError(f"DepthLoss: huber_delta must be finite and positive, got {huber_delta!r}")
        else:
            if huber_delta is not None:
                raise ValueError(f"DepthLoss: huber_delta belongs to data='huber' only, got {huber_delta!r} with data={data!r}")
            self.huber_delta = None
        self.contact_weight = number("contact_weight", contact_weight)
        self.contact_eps = number("contact_eps", contact_eps)
        self.background = number("background", background, "finite", -math.inf)
        if self.background == -math.inf:
            raise ValueError(f"DepthLoss: background must be finite, got {background!r}")
        self.grad_weight = number("grad_weight", grad_weight)
        if grad_kind not in DEPTH_GRAD_KINDS:
            raise ValueError(f"DepthLoss: grad_kind must be one of {', '.join(repr(d) for d in DEPTH_GRAD_KINDS)}, got {grad_kind!r}")
        self.grad_kind = grad_kind
        if isinstance(grad_scales, bool) or not isinstance(grad_scales, int) or not 0 <= grad_scales <= DEPTH_MAX_SCALES:
            raise ValueError(f"DepthLoss: grad_scales must be a whole number from 0 to {DEPTH_MAX_SCALES}, got {grad_scales!r}")
        self.grad_scales = int(grad_scales)
        if self.grad_weight > 0.0 and self.grad_scales == 0:
            raise ValueError(f"DepthLoss: grad_weight {grad_weight!r} needs grad_scales >= 1")

    def spec(self) -> Dict[str, object]:
        """Every field as a plain Python value (TrainStep.state_dict saves it as the `loss` hyperparameter)."""
        return {"data": self.data, "huber_delta": self.huber_delta, "contact_weight": self.contact_weight,
                "contact_eps": self.contact_eps, "background": self.background, "grad_weight": self.grad_weight,
                "grad_kind": self.grad_kind, "grad_scales": self.grad_scales}

    def c_struct(self) -> "L.gsd_depth_loss":
        """The gsd_depth_loss the kernel reads (its weights as fp32)."""
        c = L.gsd_depth_loss()
        c.data_kind, c.grad_kind, c.grad_scales = DEPTH_DATA_KINDS[self.data], DEPTH_GRAD_KINDS[self.grad_kind], self.grad_scales
        c.huber_delta = 0.0 if self.huber_delta is None else self.huber_delta
        c.contact_weight, c.contact_eps, c.background = self.contact_weight, self.contact_eps, self.background
        c.grad_weight = self.grad_weight
        return c

    def __eq__(self, other) -> bool:
        return isinstance(other, DepthLoss) and self.spec() == other.spec()

    def __hash__(self) -> int:
        return hash(tuple(self.spec().items()))

    def __repr__(self) -> str:
        return "DepthLoss(" + ", ".join(f"{k}={v!r}" for k, v in self.spec().items()) + ")"


def as_depth_loss(spec) -> DepthLoss:
    """A DepthLoss from itself or from its `.spec()` dict."""
    return spec if isinstance(spec, DepthLoss) else DepthLoss(**spec)


def atomic_save(obj, path: str) -> None:
    """torch.save to `path + ".tmp"`, flushed to disk, then renamed over `path`: a kill during the write leaves the previous
    file (or none), never a truncated one."""
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        torch.save(obj, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def loss_fwd_bwd(kind: str, out: torch.Tensor, target: torch.Tensor, grad: Optional[torch.Tensor],
                 loss_buf: torch.Tensor, ws: torch.Tensor, grad_scale: float = 1.0, guard=None) -> None:
    """loss_buf[0] = mean((o-t)^2) | mean(|o-t|); grad = d loss / d out * grad_scale (train_unet.py:51-52)."""
    for name, t in (("output", out), ("target", target)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise L.GsdError(f"loss_fwd_bwd: {name} must be a contiguous float32 tensor on the GPU, got {t.dtype} on "
                             f"{t.device} (the kernel reads raw fp32; cast with .float() first)")
    if out.shape != target.shape:
        raise L.GsdError(f"loss_fwd_bwd: output {tuple(out.shape)} and target {tuple(target.shape)} differ in shape")
    check(lib.gsd_loss_fwd_bwd(LOSS_KINDS[kind], out.data_ptr(), target.data_ptr(), out.numel(), grad_scale,
                               loss_buf.data_ptr(), L.ptr(grad), ws.data_ptr(), guard, L.stream_ptr()), "loss_fwd_bwd")


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, target, kind):
        out_c, tgt_c = out.contiguous(), target.contiguous().float()
        loss = torch.empty((1,), device=out.device, dtype=torch.float32)
        grad = torch.empty_like(out_c)
        ws = torch.empty((2048,), device=out.device, dtype=torch.float64)
        loss_fwd_bwd(kind, out_c, tgt_c, grad, loss, ws)
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def mse_loss(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Drop-in for the reference's MSE_loss(input, target) (train_unet.py:51-52), libgsd kernel."""
    return _LossFn.apply(input, target, "mse")


def l1_loss(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return _LossFn.apply(input, target, "l1")


def depth_loss_workspace(shape) -> int:
    """Doubles of scratch depth_loss_fwd_bwd needs for an (N, K, H, W) output: a function of the shape alone."""
    n, k, h, w = (int(d) for d in shape)
    return int(lib.gsd_depth_loss_workspace(n, k, h, w))


def depth_loss_fwd_bwd(spec: DepthLoss, out: torch.Tensor, target: torch.Tensor, grad: Optional[torch.Tensor],
                       terms: torch.Tensor, ws: torch.Tensor, grad_scale: float = 1.0, guard=None) -> None:
    """terms[0:6] = L, L_data, L_grad, mean (o-t)^2, mean |o-t|, contact fraction of the DepthLoss `spec` over the (N, K, H, W)
    output; grad (None: evaluation) = d L / d out * grad_scale.  ws: depth_loss_workspace(out.shape) float64."""
    for name, t in (("output", out), ("target", target)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise L.GsdError(f"depth_loss_fwd_bwd: {name} must be a contiguous float32 tensor on the GPU, got {t.dtype} on "
                             f"{t.device} (the kernel reads raw fp32; cast with .float() first)")
    if out.dim() != 4 or out.shape != target.shape:
        raise L.GsdError(f"depth_loss_fwd_bwd: output {tuple(out.shape)} and target {tuple(target.shape)} must be one "
                         "(N, K, H, W) shape")
    if grad is not None and (grad.dtype != torch.float32 or not grad.is_cuda or not grad.is_contiguous() or grad.shape != out.shape):
        raise L.GsdError("depth_loss_fwd_bwd: grad must be a contiguous float32 GPU tensor of the output's shape")
    if terms.dtype != torch.float32 or not terms.is_cuda or terms.numel() < 6 or ws.dtype != torch.float64 or not ws.is_cuda:
        raise L.GsdError("depth_loss_fwd_bwd: terms must be 6 float32 and ws float64, both on the GPU")
    n, k, h, w = out.shape
    c = spec.c_struct()
    check(lib.gsd_depth_loss_fwd_bwd(C.byref(c), out.data_ptr(), target.data_ptr(), n, k, h, w, grad_scale, terms.data_ptr(),
                                     L.ptr(grad), ws.data_ptr(), ws.numel(), guard, L.stream_ptr()), "depth_loss_fwd_bwd")


class _DepthLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, target, spec):
        out_c, tgt_c = out.contiguous(), target.contiguous().float()
        terms = torch.empty((6,), device=out.device, dtype=torch.float32)
        grad = torch.empty_like(out_c)
        ws = torch.empty((depth_loss_workspace(out_c.shape),), device=out.device, dtype=torch.float64)
        depth_loss_fwd_bwd(spec, out_c, tgt_c, grad, terms, ws)
        ctx.save_for_backward(grad)
        return terms[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def depth_loss(input: torch.Tensor, target: torch.Tensor, spec) -> torch.Tensor:
    """The DepthLoss `spec` (or its `.spec()` dict) of an (N, K, H, W) prediction, differentiable w.r.t. `input`: the autograd
    form of what TrainStep(loss=spec) launches, beside mse_loss / l1_loss."""
    return _DepthLossFn.apply(input, target, as_depth_loss(spec))


class TrainStep:
    """Fused fwd + loss + bwd + Adam + EMA step for a gelslim_depth_amd UNet.

    Parameters live in one flat fp32 arena (the module's parameters become views of it, so state_dict(),
    load_state_dict() and the reference's checkpoint layout keep working); gradients, Adam moments and the EMA
    shadow are arenas of the same size.  With `process_group` set, gradients are summed across ranks with
    RCCL all-reduce (torch.distributed backend "nccl") in per-block buckets launched as soon as a block's
    backward is done, and scaled by 1/world inside the Adam kernel.

    `max_grad_norm`: clip the averaged gradient to this global L2 norm (torch.nn.utils.clip_grad_norm_'s coefficient), behind
    the all-reduce and in front of the optimiser, with no host synchronisation; `last_grad_norm` / `last_clip_coef` are
    device tensors like `last_loss`.  A non-finite norm raises the guard (nan_policy) or, without one, reaches the parameters
    as a NaN -- it is never clipped away.  `lr_schedule`: an LRSchedule; the rate of a step is lr_at(lr, lr_schedule, t) with
    t the step count Adam's bias correction uses (skipped steps count).  Both are saved with the state.

    `loss`: "mse" (the reference's), "l1", or a DepthLoss, whose one launch takes the place of the plain loss kernel; the step
    still returns L, and `last_loss_terms` holds its parts.  Saved with the state as the string or the DepthLoss's spec.
    """

    def __init__(self, model: UNet, lr: float = 1e-3, weight_decay: float = 1e-6, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, ema_decay: Optional[float] = 0.995, loss: Union[str, "DepthLoss"] = "mse",
                 process_group=None, sync_bn: bool = False, overlap_allreduce: bool = True,
                 nan_policy: Optional[str] = None, force_sync: bool = False, time_allreduce: bool = False,
                 max_grad_norm: Optional[float] = None, lr_schedule: Optional[LRSchedule] = None):
        if nan_policy not in (None, "skip", "raise"):
            raise ValueError(f"nan_policy must be None, 'skip' or 'raise', got {nan_policy!r}")
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:
                raise ValueError(f"max_grad_norm must be positive (None: no clipping), got {max_grad_norm!r}")
        if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
            raise ValueError(f"lr_schedule must be an LRSchedule or None, got {type(lr_schedule).__name__}")
        if not isinstance(loss, (str, DepthLoss)):
            raise ValueError(f"loss must be 'mse', 'l1' or a DepthLoss, got {type(loss).__name__}")
        if isinstance(loss, str) and loss not in LOSS_KINDS:
            raise ValueError(f"loss must be 'mse', 'l1' or a DepthLoss, got {loss!r}")
        self.max_grad_norm = max_grad_norm
        self.lr_schedule = lr_schedule
        self.model = model
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.ema_decay = ema_decay
        self.loss_kind = loss
        self.step_count = 0
        self.ema_updates = 0
        self.pg = process_group
        self.world, self.rank = 1, 0
        self.overlap = overlap_allreduce
        self.nan_policy = nan_policy
        if process_group is not None:
            import torch.distributed as dist
            self.dist = dist
            self.world = dist.get_world_size(process_group)
            self.rank = dist.get_rank(process_group)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise L.GsdError("TrainStep needs the model on the GPU")
        names = [n for n, _ in model.named_parameters()]
        sizes = [p.numel() for _, p in model.named_parameters()]
        total = sum(sizes)
        self.numel = total
        self.p_flat = torch.empty((total,), device=dev, dtype=torch.float32)
        self.g_flat = torch.zeros((total,), device=dev, dtype=torch.float32)
        self.m_flat = torch.zeros((total,), device=dev, dtype=torch.float32)
        self.v_flat = torch.zeros((total,), device=dev, dtype=torch.float32)
        self.offsets: Dict[str, Tuple[int, int]] = {}
        off = 0
        gviews: Dict[str, torch.Tensor] = {}
        for (n, p), sz in zip(model.named_parameters(), sizes):
            self.p_flat[off:off + sz].copy_(p.data.reshape(-1))
            p.data = self.p_flat[off:off + sz].view(p.shape)
            gviews[n] = self.g_flat[off:off + sz].view(p.shape)
            self.offsets[n] = (off, sz)
            off += sz
        model._grad_views = gviews
        self.ema_flat = self.p_flat.clone() if ema_decay is not None else None
        # a DepthLoss writes six terms, L first: the step's loss is their first element
        self.terms_buf = torch.zeros((6,), device=dev, dtype=torch.float32) if isinstance(loss, DepthLoss) else None
        self.loss_buf = torch.zeros((1,), device=dev, dtype=torch.float32) if self.terms_buf is None else self.terms_buf[0:1]
        self.loss_ws = torch.empty((2048,), device=dev, dtype=torch.float64)
        # clip = (norm of the averaged gradient before clipping, coefficient in (0, 1]), written by gsd_grad_norm every step
        self.clip_buf = self.norm_ws = None
        if max_grad_norm is not None:
            self.clip_buf = torch.zeros((2,), device=dev, dtype=torch.float32)
            self.norm_ws = torch.empty((lib.gsd_grad_norm_workspace(total),), device=dev, dtype=torch.float64)
        # non-finite guard: words[0] = tick of the last bad step, words[1] = steps skipped (include/gsd.h: gsd_guard)
        self.guard_words = torch.zeros((2,), device=dev, dtype=torch.int32) if nan_policy is not None else None
        # With a nan_policy a skipped step must leave no trace in the BatchNorm running statistics either (layers in front of
        # the first bad one have updated theirs by the time the step is found bad, and every data-parallel rank must end with
        # the same buffers): the float buffers become views of one arena that is snapshotted before the step and put back
        # by a device-side conditional copy behind it.  (num_batches_tracked keeps counting, as it would in the reference,
        # whose forward has run by the time its NaN test fires.)
        self.bn_flat = self.bn_snap = None
        if nan_policy is not None:
            bufs = [b for _, b in model.named_buffers() if b.dtype == torch.float32]
            self.bn_flat = torch.empty((sum(b.numel() for b in bufs),), device=dev, dtype=torch.float32)
            o = 0
            for b in bufs:
                self.bn_flat[o:o + b.numel()].copy_(b.reshape(-1))
                b.data = self.bn_flat[o:o + b.numel()].view(b.shape)
                o += b.numel()
            self.bn_snap = torch.empty_like(self.bn_flat)
        # A later model.to(...) / .float() / .half() re-allocates the module's tensors and silently detaches them from the arenas
        # (the kernels would go on updating arenas nobody reads; the guard's snapshot would cover stale memory): remember where
        # every parameter and arena-backed buffer must live and check it at every step (a host-side pointer compare).
        self._pinned = [(n, p, p.data_ptr()) for n, p in model.named_parameters()]
        if self.bn_flat is not None:
            self._pinned += [(n, b, b.data_ptr()) for n, b in model.named_buffers() if b.dtype == torch.float32]
        self._dout = None
        self._out = None
        eng = model._engine
        eng.world = self.world
        force_sync = process_group is not None and (force_sync or bool(os.environ.get("GSD_FORCE_SYNC")))
        if sync_bn and (self.world > 1 or force_sync):
            eng.sync_fn = lambda t: self.dist.all_reduce(t, group=self.pg)
        self.sync = None
        if self.world > 1 or force_sync:   # 2nd: rehearsal of the collectives with ONE rank
            from .distributed import GradSync, broadcast_state, make_buckets
            broadcast_state(self.p_flat, [b for _, b in model.named_buffers()], group=self.pg)
            if self.ema_flat is not None:
                self.ema_flat.copy_(self.p_flat)
            self.sync = GradSync(self.g_flat, make_buckets(names, self.offsets, eng.L), group=self.pg,
                                 overlap=overlap_allreduce, force=force_sync, timing=time_allreduce)

    def _check_arenas(self) -> None:
        for n, t, ptr in self._pinned:
            if t.data_ptr() != ptr or t.dtype != torch.float32:
                raise L.GsdError(
                    f"TrainStep: '{n}' no longer lives in the step's flat arena (the model was moved or cast -- model.to(...), "
                    ".float(), .half(), load with assign=True -- after TrainStep was built).  Move / cast the model first, then "
                    "construct TrainStep; load_state_dict() and in-place updates keep the arenas.")

    def __call__(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        model = self.model
        eng = model._engine
        self._check_arenas()
        x = x.contiguous()
        target = target.float().contiguous()     # the kernels read raw fp32 (a float64 / uint8 depth target is cast, as _LossFn does)
        if not target.is_cuda:
            raise L.GsdError("TrainStep: the target must be on the GPU")
        guard = L.make_guard(self.guard_words, self.step_count + 1)
        eng.guard = guard
        P = model._tensor_map()
        if self._out is None or self._out.shape != (x.shape[0], model.n_classes, x.shape[2], x.shape[3]):
            self._out = torch.empty((x.shape[0], model.n_classes, x.shape[2], x.shape[3]), device=x.device,
                                    dtype=torch.float32)
            self._dout = torch.empty_like(self._out)
        if self.bn_flat is not None:
            check(lib.gsd_guard_snapshot(self.bn_flat.data_ptr(), self.bn_snap.data_ptr(), self.bn_flat.numel(), L.stream_ptr()),
                  "guard_snapshot")
        try:
            out = eng.forward(x, P, train=True, out=self._out)
            if self.terms_buf is None:
                loss_fwd_bwd(self.loss_kind, out, target, self._dout, self.loss_buf, self.loss_ws, guard=guard)
            else:
                need = depth_loss_workspace(out.shape)
                if self.loss_ws.numel() < need:
                    self.loss_ws = torch.empty((need,), device=out.device, dtype=torch.float64)
                depth_loss_fwd_bwd(self.loss_kind, out, target, self._dout, self.terms_buf, self.loss_ws, guard=guard)
            eng.block_done_cb = self.sync.on_block_done if self.sync is not None else None
            eng.backward(self._dout, P, model._grad_views)
        finally:
            eng.block_done_cb = None
            eng.guard = None
        if self.sync is not None:
            self.sync.finish()
        if self.clip_buf is not None:
            # behind the all-reduce, in front of the guard's MAX: every rank measures the same summed arena, and a non-finite
            # norm found here is part of the skip decision the ranks agree on
            check(lib.gsd_grad_norm(self.g_flat.data_ptr(), self.numel, 1.0 / self.world, self.max_grad_norm,
                                    self.clip_buf.data_ptr(), self.norm_ws.data_ptr(), self.norm_ws.numel(), guard,
                                    L.stream_ptr()), "grad_norm")
        if self.sync is not None and guard is not None:
            # every rank must take the same skip decision: the summed gradient carries any rank's NaN
            self.dist.all_reduce(self.guard_words[0:1], op=self.dist.ReduceOp.MAX, group=self.pg)
        self.step_count += 1
        d = 0.0
        if self.ema_flat is not None:
            # torch_ema 0.3 (requirements.txt:6): decay = min(decay, (1+n)/(10+n)), n counted after increment
            self.ema_updates += 1
            d = min(self.ema_decay, (1.0 + self.ema_updates) / (10.0 + self.ema_updates))
        lr = self.current_lr()
        if self.clip_buf is None:
            check(lib.gsd_adam_ema(self.p_flat.data_ptr(), self.g_flat.data_ptr(), self.m_flat.data_ptr(),
                                   self.v_flat.data_ptr(), L.ptr(self.ema_flat), self.numel, self.step_count, lr,
                                   self.betas[0], self.betas[1], self.eps, self.wd, d, 1.0 / self.world, guard, L.stream_ptr()),
                  "adam_ema")
        else:
            check(lib.gsd_adam_ema_clip(self.p_flat.data_ptr(), self.g_flat.data_ptr(), self.m_flat.data_ptr(),
                                        self.v_flat.data_ptr(), L.ptr(self.ema_flat), self.numel, self.step_count, lr,
                                        self.betas[0], self.betas[1], self.eps, self.wd, d, 1.0 / self.world,
                                        self.clip_buf.data_ptr(), guard, L.stream_ptr()), "adam_ema_clip")
        if self.bn_flat is not None:
            check(lib.gsd_guard_restore(guard, self.bn_flat.data_ptr(), self.bn_snap.data_ptr(), self.bn_flat.numel(), L.stream_ptr()),
                  "guard_restore")
        return self.loss_buf

    def current_lr(self) -> float:
        """The learning rate of the last step taken (of the first one before any): lr_at(lr, lr_schedule, step_count)."""
        return lr_at(self.lr, self.lr_schedule, max(1, self.step_count))

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """L2 norm of the last step's averaged gradient BEFORE clipping: a one-element device tensor that every step
        overwrites (no host sync; .item() when you want it).  None without max_grad_norm."""
        return None if self.clip_buf is None else self.clip_buf[0:1]

    @property
    def last_clip_coef(self) -> Optional[torch.Tensor]:
        """The last step's clip coefficient min(1, max_grad_norm / (norm + 1e-6)), NaN for a non-finite norm; a device tensor
        like last_grad_norm."""
        return None if self.clip_buf is None else self.clip_buf[1:2]

    @property
    def last_loss_terms(self) -> Optional[torch.Tensor]:
        """The last step's six loss terms under a DepthLoss -- L, L_data, L_grad, mean (o-t)^2, mean |o-t|, the fraction of
        contact pixels -- as a device tensor that every step overwrites (no host sync).  None for loss="mse" / "l1"."""
        return self.terms_buf

    def skipped_steps(self) -> int:
        """Optimiser steps the non-finite guard has skipped so far (one host sync; 0 without a nan_policy)."""
        return int(self.guard_words[1].item()) if self.guard_words is not None else 0

    def check_finite(self) -> None:
        """nan_policy="raise": raise if any step since the last check saw a non-finite loss or BatchNorm statistic (the
        reference fails at that step, train_unet.py:371-374; here the arenas were left untouched by the skipped update)."""
        if self.nan_policy != "raise":
            return
        n = self.skipped_steps()
        if n:
            bad = int(self.guard_words[0].item())
            self.guard_words[1].zero_()
            raise L.GsdError(f"non-finite loss or BatchNorm statistics in {n} train step(s), last at step {bad}; those "
                             "updates were skipped (parameters, Adam moments and EMA shadow are intact)")

    def mean_across_ranks(self, value: float) -> float:
        """Mean of a host scalar over the data-parallel ranks (epoch losses: every rank must take the same early-stopping
        and checkpoint decisions)."""
        if self.world == 1:
            return float(value)
        t = torch.tensor([value], device=self.p_flat.device, dtype=torch.float64)
        self.dist.all_reduce(t, group=self.pg)
        return float(t.item()) / self.world

    def evaluate(self, x: torch.Tensor, use_ema: bool = True) -> torch.Tensor:
        """Eval-mode forward under the EMA weights WITHOUT the store / copy-in / restore the reference pays per batch
        (`with ema.average_parameters(): unet(x=...)`, train_unet.py:389-390,428-429): the kernels
        are simply pointed at the shadow arena.  BatchNorm buffers are the live ones, as in the reference."""
        model = self.model
        P = model._tensor_map()
        if use_ema and self.ema_flat is not None:
            for k, (o, sz) in self.offsets.items():
                P[k] = self.ema_flat[o:o + sz].view(P[k].shape)
        with torch.no_grad():
            return model._engine.forward(x.float().contiguous(), P, train=False)

    def save_checkpoint(self, path: str, use_ema: bool = True) -> None:
        """torch.save of the reference-layout state_dict (118 keys), EMA weights swapped in like the reference's
        best-validation save (train_unet.py:480-483); loads into the reference's UNet with strict=True."""
        sd = self.ema_state_dict() if use_ema else self.model.state_dict()
        torch.save({k: v.detach().cpu() for k, v in sd.items()}, path)

    @property
    def last_loss(self) -> torch.Tensor:
        return self.loss_buf

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """state_dict with the EMA shadow in place of the parameters -- what the reference saves at best-val
        under `with ema.average_parameters()` (train_unet.py:480-483); BN buffers are the live ones."""
        sd = self.model.state_dict()
        if self.ema_flat is None:
            return sd
        out = {}
        for k, v in sd.items():
            if k in self.offsets:
                o, s = self.offsets[k]
                out[k] = self.ema_flat[o:o + s].view(v.shape).clone()
            else:
                out[k] = v.clone()
        return out

    # -- the full training state: save, then continue bit for bit ---------------------------------------------------------
    def _arena_table(self) -> List[Tuple[str, int, Tuple[int, ...]]]:
        shapes = {n: tuple(p.shape) for n, p in self.model.named_parameters()}
        return [(n, o, shapes[n]) for n, (o, _) in self.offsets.items()]

    def _loss_hparam(self):
        """The saved form of `loss`: the string, or the DepthLoss's spec dict."""
        return self.loss_kind.spec() if isinstance(self.loss_kind, DepthLoss) else self.loss_kind

    def _hparams(self) -> Dict[str, object]:
        return {"lr": float(self.lr), "betas": tuple(float(b) for b in self.betas), "eps": float(self.eps),
                "weight_decay": float(self.wd), "ema_decay": None if self.ema_decay is None else float(self.ema_decay),
                "loss": self._loss_hparam(), "nan_policy": self.nan_policy, "max_grad_norm": self.max_grad_norm,
                "lr_schedule": None if self.lr_schedule is None else self.lr_schedule.spec()}

    def state_dict(self) -> Dict[str, object]:
        """The whole training state as CPU tensors and host scalars: the model's state_dict (live parameters, BatchNorm
        buffers, num_batches_tracked), the Adam moments and the EMA shadow (None without EMA) as flat fp32 arenas with their
        table of (name, offset, shape), the step and EMA-update counts that drive the bias correction and the EMA warm-up,
        the non-finite guard's words (None without a nan_policy), the constructor's hyperparameters and the architecture.
        `load_state_dict` of it into a TrainStep over the same architecture continues the run bit for bit (same precision,
        same world size).  Unlike `save_checkpoint` (EMA weights, the reference's 118-key layout) this is not a model file."""
        model = self.model

        def cpu(t):
            return None if t is None else t.detach().to("cpu", copy=True)
        # version 2 only when clipping or a schedule is on: a build that knows neither then refuses the state ("newer than
        # this build reads") instead of silently training on unclipped or at the base rate
        version = 1 if self.max_grad_norm is None and self.lr_schedule is None else 2
        return {"format": STATE_FORMAT, "version": version,
                "precision": model.precision, "n_channels": model.n_channels, "n_classes": model.n_classes,
                "layer_dimensions": list(model._dims),
                "model": {k: cpu(v) for k, v in model.state_dict().items()},
                "arena": self._arena_table(),
                "m_flat": cpu(self.m_flat), "v_flat": cpu(self.v_flat), "ema_flat": cpu(self.ema_flat),
                "step_count": self.step_count, "ema_updates": self.ema_updates,
                "guard_words": cpu(self.guard_words),
                "hparams": self._hparams()}

    def load_state_dict(self, sd: Dict[str, object], strict: bool = True) -> None:
        """Continue from a `state_dict()`.  Everything is copied IN PLACE into the existing arenas (parameters, BatchNorm
        buffers, Adam moments, EMA shadow, guard words), so the parameter and gradient views, the arena check of every step
        and a GraphedInference captured on the model stay valid.  fp32 <-> bf16 is allowed: both keep fp32 master state.

        Raises ValueError, naming the field, before anything is copied: another architecture (the first parameter whose
        name, offset or shape differs), EMA on one side only, or -- with strict=True -- another hyperparameter (lr, betas,
        eps, weight_decay, ema_decay, loss, nan_policy, max_grad_norm, lr_schedule -- absent from a state written before the
        last two existed, which reads as None; `loss` is the string or a DepthLoss's spec, and of two specs the first differing
        field is named); strict=False keeps this TrainStep's hyperparameters (the guard's
        skipped-step count then starts at 0 when the state has none).  A weights-only checkpoint is refused.

        Data parallel: a collective.  Rank 0's `sd` is checked and loaded (the other ranks may pass None), then its arenas
        and buffers are broadcast and its host scalars sent with broadcast_object_list."""
        self._load(lambda: sd, strict)

    def save_state(self, path: str) -> None:
        """Write `state_dict()` to `path` (through `path + ".tmp"` and an atomic rename: a kill never leaves a partial
        file).  Data parallel: rank 0 writes, the other ranks return at once."""
        if self.rank == 0:
            atomic_save(self.state_dict(), path)

    def load_state(self, path: str, strict: bool = True) -> None:
        """`load_state_dict` of the file `save_state` wrote.  Data parallel: only rank 0 reads it (the ranks need no shared
        filesystem; `path` is ignored elsewhere)."""
        self._load(lambda: read_state(path), strict)

    def _load(self, get, strict: bool) -> None:
        if self.sync is None:
            self._load_local(get(), strict)
            return
        err = None
        if self.rank == 0:
            try:
                self._load_local(get(), strict)
            except Exception as exc:         # the other ranks wait in the broadcast below: tell them, then raise everywhere
                err = exc
        box = [None if err is None else f"{type(err).__name__}: {err}", self.step_count, self.ema_updates]
        self.dist.broadcast_object_list(box, src=0, group=self.pg)
        if err is not None:
            raise err
        if box[0] is not None:
            raise ValueError(f"TrainStep state: rank 0 could not load it: {box[0]}")
        self.step_count, self.ema_updates = int(box[1]), int(box[2])
        from .distributed import broadcast_state
        broadcast_state(self.p_flat, [b for _, b in self.model.named_buffers()], group=self.pg,
                        extra=[t for t in (self.m_flat, self.v_flat, self.ema_flat, self.guard_words) if t is not None])

    def _load_local(self, sd, strict: bool) -> None:
        _check_state_format(sd)
        model = self.model
        arch = (f"layer_dimensions {list(sd['layer_dimensions'])}, n_channels {sd['n_channels']}, n_classes {sd['n_classes']} "
                f"in the state; {list(model._dims)}, {model.n_channels}, {model.n_classes} here")
        theirs = [(str(n), int(o), tuple(int(d) for d in s)) for n, o, s in sd["arena"]]
        mine = self._arena_table()
        for i in range(max(len(theirs), len(mine))):
            a = theirs[i] if i < len(theirs) else None
            b = mine[i] if i < len(mine) else None
            if a != b:
                desc = [("absent" if t is None else f"'{t[0]}' of shape {t[2]} at offset {t[1]}") for t in (a, b)]
                raise ValueError(f"TrainStep state: parameter '{(a or b)[0]}' differs: {desc[0]} in the state, {desc[1]} here "
                                 f"(another architecture: {arch})")
        here = model.state_dict()
        for k in list(sd["model"]) + [k for k in here if k not in sd["model"]]:
            a, b = sd["model"].get(k), here.get(k)
            if a is None or b is None or tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
                desc = [("absent" if t is None else f"{tuple(t.shape)} {t.dtype}") for t in (a, b)]
                raise ValueError(f"TrainStep state: model entry '{k}' is {desc[0]} in the state, {desc[1]} here ({arch})")
        if (sd["ema_flat"] is None) != (self.ema_flat is None):
            raise ValueError("TrainStep state: ema_flat: " + ("the state has no EMA shadow and this TrainStep keeps one"
                             if sd["ema_flat"] is None else "the state has an EMA shadow and this TrainStep was built with "
                             "ema_decay=None"))
        for key in ("m_flat", "v_flat", "ema_flat"):
            t = sd[key]
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != self.numel):
                raise ValueError(f"TrainStep state: {key} must be {self.numel} float32 values, got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        g = sd["guard_words"]
        if g is not None and (not isinstance(g, torch.Tensor) or g.dtype != torch.int32 or g.numel() != 2):
            raise ValueError("TrainStep state: guard_words must be two int32 words")
        if strict:
            mine_h = self._hparams()
            for k in STATE_HPARAMS:
                v = sd["hparams"].get(k)
                if k == "betas" and v is not None:
                    v = tuple(float(b) for b in v)
                elif k in ("lr", "eps", "weight_decay", "ema_decay", "max_grad_norm") and v is not None:
                    v = float(v)
                elif k == "lr_schedule" and v is not None:
                    v = dict(v)
                elif k == "loss" and isinstance(v, dict) and isinstance(mine_h[k], dict):
                    for f in list(mine_h[k]) + [f for f in v if f not in mine_h[k]]:      # two DepthLoss specs: name the field
                        if f not in v or f not in mine_h[k] or v[f] != mine_h[k][f]:
                            raise ValueError(f"TrainStep state: loss field {f} is {v.get(f)!r} in the state and "
                                             f"{mine_h[k].get(f)!r} here; pass strict=False to continue with this TrainStep's "
                                             "hyperparameters")
                if v != mine_h[k]:
                    raise ValueError(f"TrainStep state: {k} is {v!r} in the state and {mine_h[k]!r} here; pass strict=False "
                                     "to continue with this TrainStep's hyperparameters")
        with torch.no_grad():
            model.load_state_dict(sd["model"], strict=True)
            self.m_flat.copy_(sd["m_flat"])
            self.v_flat.copy_(sd["v_flat"])
            if self.ema_flat is not None:
                self.ema_flat.copy_(sd["ema_flat"])
            if self.guard_words is not None:
                if g is not None:
                    self.guard_words.copy_(g)
                else:
                    self.guard_words.zero_()
        self.step_count = int(sd["step_count"])
        self.ema_updates = int(sd["ema_updates"])
        self._check_arenas()


_STATE_KEYS = ("precision", "n_channels", "n_classes", "layer_dimensions", "model", "arena", "m_flat", "v_flat", "ema_flat",
               "step_count", "ema_updates", "guard_words", "hparams")


def read_state(path: str) -> Dict[str, object]:
    """torch.load of a state file onto the CPU (tensors, numbers, strings and containers only: weights_only)."""
    return torch.load(path, map_location="cpu", weights_only=True)


def _check_state_format(sd) -> None:
    if isinstance(sd, dict) and sd.get("format") == STATE_FORMAT:
        if int(sd.get("version", 0)) > STATE_VERSION:
            raise ValueError(f"TrainStep state: version {sd['version']} is newer than this build reads ({STATE_VERSION})")
        missing = [k for k in _STATE_KEYS if k not in sd]
        if missing:
            raise ValueError(f"TrainStep state: field '{missing[0]}' is missing")
        return
    if isinstance(sd, dict) and sd and all(isinstance(v, torch.Tensor) for v in sd.values()):
        raise ValueError(f"TrainStep state: this is a weights-only checkpoint ({len(sd)} tensors, the model state_dict that "
                         "TrainStep.save_checkpoint and the reference's training script write), with no Adam moments, EMA "
                         "shadow or step counts -- it cannot continue a run.  To start from its weights, call "
                         "model.load_state_dict(torch.load(path)) before building the TrainStep")
    raise ValueError(f"TrainStep state: format: expected a dict tagged '{STATE_FORMAT}' (TrainStep.state_dict / save_state), "
                     f"got {type(sd).__name__}")
