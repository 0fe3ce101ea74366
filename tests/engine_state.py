"""Shared by the tests that ask whether a result depends on anything but its inputs (test_engine_state_cpu.py,
test_gpu_engine_memory.py, test_gpu_engine_history.py).  Not collected; torch is imported inside the functions.

poisoned()   every tensor torch.empty / torch.empty_like / Tensor.new_empty hand out on one device type is filled before the
             caller sees it -- with 0, with a quiet NaN, or with +3.0e4 -- so that "uninitialised" memory is what the test says
             it is instead of whatever the allocator's last owner left (in a fresh test process: usually zeros).
workloads    small functions that build a model from synth.make_state, run one named workload and return {name: tensor}.
same_bits()  equality of integer views (equal NaNs would compare equal) AND every float finite.
"""
import contextlib
import os

ZERO, NAN, BIG = "zero", "nan", "big"
PATTERNS = (ZERO, NAN, BIG)
# BIG is finite in bf16 and its square is finite in fp32; it is positive, so a ReLU or an fmaxf does not swallow it as it swallows a
# NaN (fmaxf(NaN, 0) = 0): a kernel that reads a garbage activation through its fused ReLU shows under BIG and hides under NAN
VALUES = {ZERO: 0.0, NAN: float("nan"), BIG: 3.0e4}
INT_BYTE = 0x5A       # every byte of an integer tensor (int16: 0x5A5A = 23130): non-zero, positive in every signed width


class Poison:
    """What poisoned() returns: the pattern and how many tensors it has filled so far."""

    def __init__(self, pattern, device_type):
        self.pattern, self.device_type, self.value, self.filled = pattern, device_type, VALUES[pattern], 0


def poisoned(monkeypatch, pattern, device_type="cuda"):
    """Patch torch.empty, torch.empty_like and torch.Tensor.new_empty (the whole of that family the package calls: no
    empty_strided, no resize_) through `monkeypatch` so that what they return on `device_type` holds `pattern`.  The originals
    make the allocation; tensors on other devices are left alone.  Undone when the monkeypatch (or its context) unwinds."""
    import torch
    p = Poison(pattern, device_type)

    def fill(t):
        if isinstance(t, torch.Tensor) and t.device.type == device_type and t.numel():
            if t.is_floating_point() or t.is_complex():
                t.fill_(p.value)
            elif t.dtype == torch.bool:
                t.fill_(True)
            else:
                t.fill_(int.from_bytes(bytes([INT_BYTE]) * t.element_size(), "little"))
            p.filled += 1
        return t

    def wrap(orig):
        def patched(*args, **kwargs):
            return fill(orig(*args, **kwargs))
        patched.__name__ = getattr(orig, "__name__", "patched")
        patched.__wrapped__ = orig
        return patched

    monkeypatch.setattr(torch, "empty", wrap(torch.empty))
    monkeypatch.setattr(torch, "empty_like", wrap(torch.empty_like))
    monkeypatch.setattr(torch.Tensor, "new_empty", wrap(torch.Tensor.new_empty))
    return p


@contextlib.contextmanager
def poison(monkeypatch, pattern, device_type="cuda"):
    """poisoned() for the length of a with-block (a test that runs under more than one pattern)."""
    with monkeypatch.context() as mp:
        yield poisoned(mp, pattern, device_type)


@contextlib.contextmanager
def environ(env):
    """os.environ with `env` on top for the length of the block (the library and the engines re-read their switches per call)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------------------------ comparison
def _as_tensor(v):
    import torch
    if isinstance(v, torch.Tensor):
        return v.detach()
    if isinstance(v, bool) or isinstance(v, int):
        return torch.tensor(v, dtype=torch.int64)
    return torch.tensor(v, dtype=torch.float64)


def same_bits(a, b, what, finite=True):
    """a and b (tensors or host scalars) hold the same bits, and -- unless the caller says why not -- every float is finite."""
    import torch
    a, b = _as_tensor(a), _as_tensor(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
    if a.is_floating_point() and finite:
        for t in (a, b):
            bad = int((~torch.isfinite(t)).sum())
            assert bad == 0, f"{what}: {bad} of {t.numel()} values are not finite"
    if a.is_floating_point():
        as_int = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        a, b = a.contiguous().view(as_int), b.contiguous().view(as_int)
    a, b = a.cpu(), b.cpu()
    if not torch.equal(a, b):
        diff = (a != b).reshape(-1)
        first = int(diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ in their bits, the first at flat "
                             f"index {first}")


def same_results(a, b, what, not_finite=()):
    """Two workload results: the same names, each pair the same bits.  not_finite: names exempt from the finiteness check (the
    caller's comment says why)."""
    assert sorted(a) == sorted(b), f"{what}: {sorted(a)} against {sorted(b)}"
    for k in a:
        same_bits(a[k], b[k], f"{what}: {k}", finite=k not in not_finite)


# ------------------------------------------------------------------------------------------------------------------- workloads
class Case:
    """One row of a case table: the network, the batch shape and the library / engine switches it runs under."""

    def __init__(self, name, precision, dims, n, h, w, env=None, n_classes=1):
        self.name, self.precision, self.dims, self.n, self.h, self.w = name, precision, list(dims), n, h, w
        self.env, self.n_classes = dict(env or {}), n_classes

    def __repr__(self):
        return self.name


def snap(t):
    """A host copy that no later launch can change."""
    return None if t is None else t.detach().to("cpu", copy=True)


def make_model(precision, dims, n_classes=1, seed=5, train=True):
    import torch
    from gelslim_depth_amd import synth
    from gelslim_depth_amd.models.unet import UNet
    st = synth.make_state(3, n_classes, dims, seed, "conditioned")
    m = UNet(n_channels=3, n_classes=n_classes, layer_dimensions=dims, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    return m.to("cuda").train(train)


def make_batch(n, h, w, seed=6, n_classes=1):
    import torch
    from gelslim_depth_amd import synth
    x, t = synth.make_batch(n, h, w, seed, n_classes=n_classes)
    return torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()


def buffers_of(model):
    return {"buf." + k: snap(b) for k, b in model.named_buffers()}


def step_state(step, prefix=""):
    """What a TrainStep leaves behind: parameters, Adam moments, EMA shadow, BatchNorm buffers, the guard's count."""
    res = {prefix + "p_flat": snap(step.p_flat), prefix + "m_flat": snap(step.m_flat), prefix + "v_flat": snap(step.v_flat)}
    if step.ema_flat is not None:
        res[prefix + "ema_flat"] = snap(step.ema_flat)
    res.update({prefix + k: v for k, v in buffers_of(step.model).items()})
    res[prefix + "skipped_steps"] = step.skipped_steps()
    return res


def rich_step_kwargs():
    """The TrainStep variant in which the guard, the BatchNorm snapshot, the clip and the norm workspace take part."""
    from gelslim_depth_amd.train import DepthLoss, LRSchedule
    return dict(loss=DepthLoss(data="huber", huber_delta=0.05, contact_weight=2.0, contact_eps=0.01, grad_weight=0.5, grad_scales=2),
                max_grad_norm=0.05, lr_schedule=LRSchedule(warmup_steps=2, decay="cosine", total_steps=8), nan_policy="skip")


def on_device(results):
    """{name: tensor} -> on-device clones taken on the current stream, as an optimiser or a caller would read the results: nothing
    here waits for the device, so a result that another stream has not finished is cloned as it stands."""
    return {k: None if v is None else v.detach().clone() for k, v in results.items()}


def train_steps(case, k=2, rich=False, hook=None, consume=False):
    """k TrainStep steps on one batch.  hook(model, step, i): called in front of step i (the mutation tests).
    consume: nothing synchronises with the device until every result has been cloned on the current stream right behind the
    last step (the per-step loss and clip tensors right behind their step); the host snapshots are made of those clones.  The
    plain form's device-wide synchronise in front of its snapshots would hide a join that is missing at the end of backward."""
    import torch
    from gelslim_depth_amd.train import TrainStep
    with environ(case.env):
        m = make_model(case.precision, case.dims, case.n_classes)
        step = TrainStep(m, **(rich_step_kwargs() if rich else {}))
        x, t = make_batch(case.n, case.h, case.w, n_classes=case.n_classes)
        res = {}
        keep = on_device if consume else (lambda d: {k_: snap(v) for k_, v in d.items()})
        for i in range(k):
            if hook is not None:
                hook(m, step, i)
            loss = step(x, t)
            per_step = {f"loss.{i}": loss}
            if step.last_grad_norm is not None:
                per_step[f"grad_norm.{i}"] = step.last_grad_norm
                per_step[f"clip_coef.{i}"] = step.last_clip_coef
            if step.last_loss_terms is not None:
                per_step[f"loss_terms.{i}"] = step.last_loss_terms
            res.update(keep(per_step))
        if consume:
            arenas = {"out": step._out, "g_flat": step.g_flat, "p_flat": step.p_flat, "m_flat": step.m_flat, "v_flat": step.v_flat}
            if step.ema_flat is not None:
                arenas["ema_flat"] = step.ema_flat
            arenas.update({"buf." + k_: b for k_, b in m.named_buffers()})
            res.update(on_device(arenas))
            torch.cuda.synchronize()
            res = {k_: snap(v) for k_, v in res.items()}
            res["skipped_steps"] = step.skipped_steps()
            return res, m._engine
        torch.cuda.synchronize()
        res["out"] = snap(step._out)
        res["g_flat"] = snap(step.g_flat)
        res.update(step_state(step))
        return res, m._engine


def autograd_step(case, consume=False):
    """model(x) in train mode and backward through torch's autograd, with the input's gradient where the engine has one (fp32).
    consume: as in train_steps -- out, every p.grad, x.grad and the BatchNorm buffers are cloned on the current stream right behind
    backward(), in front of the first synchronise."""
    import torch
    with environ(case.env):
        m = make_model(case.precision, case.dims, case.n_classes)
        x, t = make_batch(case.n, case.h, case.w, n_classes=case.n_classes)
        x.requires_grad_(case.precision == "fp32")
        out = m(x)
        (out * t).sum().backward()
        if consume:
            res = {"out": out}
            res.update({"grad." + k: p.grad for k, p in m.named_parameters()})
            if x.grad is not None:
                res["x.grad"] = x.grad
            res.update({"buf." + k: b for k, b in m.named_buffers()})
            res = on_device(res)
            torch.cuda.synchronize()
            return {k: snap(v) for k, v in res.items()}, m._engine
        torch.cuda.synchronize()
        res = {"out": snap(out)}
        res.update({"grad." + k: snap(p.grad) for k, p in m.named_parameters()})
        if x.grad is not None:
            res["x.grad"] = snap(x.grad)
        res.update(buffers_of(m))
        return res, m._engine


def eval_forward(case):
    import torch
    with environ(case.env):
        m = make_model(case.precision, case.dims, case.n_classes, train=False)
        x, _ = make_batch(case.n, case.h, case.w, n_classes=case.n_classes)
        with torch.no_grad():
            out = m(x=x)
        torch.cuda.synchronize()
        return {"out": snap(out)}, m._engine


def graphed_forward(case):
    """Capture on one batch, replay on another."""
    import torch
    from gelslim_depth_amd.graph import GraphedInference
    with environ(case.env):
        m = make_model(case.precision, case.dims, case.n_classes, train=False)
        x0, _ = make_batch(case.n, case.h, case.w, seed=7, n_classes=case.n_classes)
        x, _ = make_batch(case.n, case.h, case.w, n_classes=case.n_classes)
        fn = GraphedInference(m, x0)
        out = snap(fn(x))
        torch.cuda.synchronize()
        return {"out": out}, m._engine


# the workloads of test_gpu_stream_order.py: three steps, so that a buffer left in use by one step meets the next one
CONSUMING = {"train_steps": lambda case, hook=None: train_steps(case, k=3, hook=hook, consume=True),
             "train_steps_rich": lambda case, hook=None: train_steps(case, k=3, rich=True, hook=hook, consume=True),
             "autograd_step": lambda case, hook=None: autograd_step(case, consume=True)}
WORKLOADS = {"train_steps": train_steps, "train_steps_rich": lambda case: train_steps(case, rich=True),
             "autograd_step": autograd_step, "eval_forward": eval_forward, "graphed_forward": graphed_forward}


# ------------------------------------------------------------------------------------------------- what must still hold zeros
def full_pitch(t):
    """The (N, C, H, pitch) view over a pitched (N, C, H, W) tensor's whole rows."""
    n, c, h, w = t.shape
    return t.as_strided((n, c, h, t.stride(2)), t.stride(), t.storage_offset())


def slack_of(t, slack):
    """The `slack` floats in front of and behind the tensor a _lib.slack_empty / pitched_slack_zeros call returned."""
    n, c, h, w = t.shape
    numel = n * t.stride(0)
    off = t.storage_offset()
    return t.as_strided((slack,), (1,), off - slack), t.as_strided((slack,), (1,), off + numel)


def assert_pads_zero(eng):
    """Every float the engine's contract says nothing writes is still exactly 0: pad columns of the fp32 concat buffers and
    pitched pooled tensors, the part of a concat buffer's up-sampled half the transposed convolution never writes, the slack
    around every slack_empty / pitched_slack_zeros tensor; the F.pad border of the `up` slice of every bf16 concat buffer.
    Returns how many floats it looked at."""
    from gelslim_depth_amd import _lib
    seen = 0

    def zero(t, what):
        nonlocal seen
        seen += t.numel()
        assert not bool((t != 0).any()), f"{what}: {int((t != 0).sum())} of {t.numel()} are not 0"    # (a NaN is != 0)

    if getattr(eng, "precision", "fp32") == "bf16":
        for l, cat in enumerate(eng.cat):
            oy, ox = eng._pad_off(l)
            hu, wu = 2 * eng.hs[l + 1], 2 * eng.ws[l + 1]
            up = cat[..., eng.dims[l]:]
            zero(up[:, :oy], f"bf16 cat[{l}] border rows above")
            zero(up[:, oy + hu:], f"bf16 cat[{l}] border rows below")
            zero(up[:, :, :ox], f"bf16 cat[{l}] border columns left")
            zero(up[:, :, ox + wu:], f"bf16 cat[{l}] border columns right")
        return seen
    slacked = [u.raw for u in eng.units] + [p for p in eng.pooled if p is not None]
    for up in eng.ups:
        hu, wu = 2 * eng.hs[up.level_in], 2 * eng.ws[up.level_in]
        if up.cat is not None:
            full = full_pitch(up.cat)
            w = up.cat.shape[3]
            zero(full[..., w:], f"cat[{up.j}] pad columns")
            zero(full[:, up.cout:, :, wu:], f"cat[{up.j}] columns ConvT never writes")
            zero(full[:, up.cout:, hu:], f"cat[{up.j}] rows ConvT never writes")
            slacked.append(up.cat)
        else:
            slacked.append(up.out)
        if up.dout is not None:
            slacked.append(up.dout)
    for l in range(1, eng.L + 1):
        if eng.plan.pooled_pitched[l]:
            zero(full_pitch(eng.pooled[l])[..., eng.pooled[l].shape[3]:], f"pooled[{l}] pad columns")
    for t in slacked:
        for part in slack_of(t, _lib.SLACK):
            zero(part, f"slack of a {tuple(t.shape)} tensor")
    return seen
