"""GPU: gradient clipping by global norm and learning-rate schedules on the fused train step -- gsd_grad_norm against an
fp64 sum, its handling of a non-finite gradient, gsd_adam_ema_clip against gsd_adam_ema and adam_ema_ref, and TrainStep
with max_grad_norm / lr_schedule: bitwise no-ops when they do not bite, the clipped update, the guard, resume, the order
under data parallelism, and no ATen compute operator."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import fp64_ref as R
from conftest import REPO
from gelslim_depth_amd import synth

pytestmark = pytest.mark.gpu

SENT = -7.25
CONFIGS = [("fp32", [16, 32, 64], (2, 21, 27)), ("bf16", [32, 64, 128], (2, 37, 53))]
IDS = [c[0] for c in CONFIGS]


@pytest.fixture(scope="module")
def L():
    from gelslim_depth_amd import _lib
    return _lib


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def coef_formula(total: torch.Tensor, max_norm: float) -> torch.Tensor:
    """clip_grad_norm_'s clamped coefficient in fp32 on the host, from the fp32 norm the kernel returned."""
    return torch.clamp(f32(max_norm) / (total.cpu() + f32(1e-6)), max=1.0)


def grad_norm(L, g, grad_scale, max_norm, guard=None, ws=None):
    need = L.lib.gsd_grad_norm_workspace(g.numel())
    if ws is None:
        ws = torch.full((need + 8,), SENT, device="cuda", dtype=torch.float64)
    clip = torch.full((2,), SENT, device="cuda")
    L.check(L.lib.gsd_grad_norm(g.data_ptr(), g.numel(), grad_scale, max_norm, clip.data_ptr(), ws.data_ptr(), need, guard,
                                L.stream_ptr()), "grad_norm")
    torch.cuda.synchronize()
    assert bool((ws[need:] == SENT).all()), "gsd_grad_norm wrote past gsd_grad_norm_workspace(numel) doubles"
    return clip, ws[:need].clone()


# ------------------------------------------------------------------------------------------- the reduction against fp64
# 9 * 2048 * 256 * 4 + 5: past the 2048-block cap, nine groups per thread (the loop unrolled by four runs twice, then once)
@pytest.mark.parametrize("numel", [1, 255, 256, 257, 4097, 1000003, 9 * 2048 * 256 * 4 + 5])
def test_grad_norm_against_fp64(L, numel):
    """|got - ref| <= 2^-23 ref with ref = sqrt(sum g^2 in fp64) * grad_scale: the squares are exact in fp64, fewer than 2^25
    fp64 additions contribute less than 2^-28 relative in any order, the one rounding to fp32 2^-24 -- whatever the partition;
    an fp32 accumulation over magnitudes 1e-20 .. 1e18 does not get there.  From a 16-byte aligned base and from views offset
    by 1 and 3 floats (same values: same bits); twice (same bits); nothing written past the workspace; the coefficient is
    the fp32 formula of the returned norm; max_norm = inf gives exactly 1."""
    g0 = gen(2000 + numel % 1000)
    vals = torch.randn(numel, generator=g0, device="cuda") * torch.pow(
        10.0, torch.rand(numel, generator=g0, device="cuda", dtype=torch.float64) * 38.0 - 20.0).float()
    gs = float(f32(1.0 / 3.0))                    # the float the kernel receives
    ref = math.sqrt(float((vals.double() ** 2).sum())) * gs
    assert math.isfinite(ref) and ref > 0
    first = None
    for off in (0, 1, 3):
        base = torch.full((numel + 8,), float("nan"), device="cuda")
        assert base.data_ptr() % 16 == 0
        g = base[off:off + numel]
        g.copy_(vals)
        clip, part = grad_norm(L, g, gs, math.inf)
        total = float(clip[0])
        print(f"numel {numel} offset {off}: norm {total!r} ref {ref!r} rel err {abs(total - ref) / ref:.3g} (bound {2.0 ** -23:.3g})")
        assert abs(total - ref) <= 2.0 ** -23 * ref, (numel, off, total, ref)
        assert float(clip[1]) == 1.0, "max_norm = inf: telemetry only"
        clip2, part2 = grad_norm(L, g, gs, math.inf)
        assert torch.equal(clip, clip2) and torch.equal(part, part2), "two runs differ"
        if first is None:
            first = (clip, part)
        assert torch.equal(clip, first[0]) and torch.equal(part, first[1]), f"the result depends on the alignment (offset {off})"
        for max_norm in (0.37 * total, 2.0 * total, 1.0):
            max_norm = float(f32(max_norm))
            c, _ = grad_norm(L, g, gs, max_norm)
            assert torch.equal(c[0], clip[0])
            want = coef_formula(c[0], max_norm)
            assert float(c[1]) == float(want), (numel, off, max_norm, float(c[1]), float(want))
            assert 0.0 < float(c[1]) <= 1.0
        assert torch.equal(g, vals) and bool(torch.isnan(base[:off]).all()) and bool(torch.isnan(base[off + numel:]).all())


# ------------------------------------------------------------------------------------------------- non-finite gradients
@pytest.mark.parametrize("bad", [math.nan, math.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("pos", [0, 2048, 4096])
def test_non_finite_gradient_is_never_hidden(L, bad, pos):
    numel = 4097
    g0 = gen(2100)
    t = {k: torch.randn(numel, generator=g0, device="cuda") * 1e-2 for k in ("p", "g", "m", "ema")}
    t["v"] = torch.rand(numel, generator=g0, device="cuda") * 1e-6
    t["g"][pos] = bad
    before = {k: v.clone() for k, v in t.items()}
    words = torch.tensor([0, 5], dtype=torch.int32, device="cuda")
    guard = L.make_guard(words, 9)
    clip, _ = grad_norm(L, t["g"], 1.0, 1.0, guard=guard)
    assert not math.isfinite(float(clip[0])) and math.isnan(float(clip[1])), clip.tolist()
    assert words.tolist() == [9, 5]

    def adam(clip, guard):
        L.check(L.lib.gsd_adam_ema_clip(t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(),
                                        t["ema"].data_ptr(), numel, 3, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.995, 1.0, clip.data_ptr(),
                                        guard, L.stream_ptr()), "adam_ema_clip")
        torch.cuda.synchronize()
    adam(clip, guard)
    for k in t:
        assert torch.equal(t[k].view(torch.int32), before[k].view(torch.int32)), f"the skipped step changed {k}"
    assert words.tolist() == [9, 6]
    # without a guard nothing stops the NaN coefficient: it reaches every parameter, as the NaN gradient's norm should
    clip2, _ = grad_norm(L, t["g"], 1.0, 1.0)
    assert not math.isfinite(float(clip2[0])) and math.isnan(float(clip2[1]))
    adam(clip2, None)
    assert bool(torch.isnan(t["p"]).all())


# -------------------------------------------------------------------------------------------- gsd_adam_ema_clip arithmetic
@pytest.mark.parametrize("step", [1, 7])
def test_adam_ema_clip_arithmetic(L, step):
    numel, wd, gs = 100003, 0.1, 0.5
    d = min(0.995, (1.0 + step) / (10.0 + step))
    g0 = gen(2200 + step)
    init = {"p": torch.randn(numel, generator=g0, device="cuda") * 0.05,
            "g": torch.randn(numel, generator=g0, device="cuda") * 1e-3 * torch.rand(numel, generator=g0, device="cuda"),
            "m": torch.randn(numel, generator=g0, device="cuda") * 1e-4,
            "v": torch.rand(numel, generator=g0, device="cuda") * 1e-7}
    init["ema"] = init["p"] + torch.randn(numel, generator=g0, device="cuda") * 1e-3

    def run(coef):
        t = {k: v.clone() for k, v in init.items()}
        args = (t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["ema"].data_ptr(), numel, step,
                1e-3, 0.9, 0.999, 1e-8, wd, d, gs)
        if coef is None:
            L.check(L.lib.gsd_adam_ema(*args, None, L.stream_ptr()), "adam_ema")
        else:
            clip = torch.tensor([123.0, coef], device="cuda")
            L.check(L.lib.gsd_adam_ema_clip(*args, clip.data_ptr(), None, L.stream_ptr()), "adam_ema_clip")
        torch.cuda.synchronize()
        assert torch.equal(t["g"], init["g"])
        return t
    plain, same = run(None), run(1.0)
    for k in ("p", "m", "v", "ema"):
        assert torch.equal(plain[k], same[k]), f"step {step}: clip[1] = 1 changes {k}"
    coef = float(f32(0.37))
    got = run(coef)
    scale = float(f32(gs) * f32(coef))             # the product the kernel forms, in fp32
    ref = R.adam_ema_ref(init["p"], init["g"], init["m"], init["v"], init["ema"], step, 1e-3, weight_decay=wd, ema_decay=d,
                         grad_scale=scale)
    for k in ("p", "m", "v", "ema"):
        worst = R.check_bound(got[k], *ref[k], R.TAU_ADAM, f"step {step} clipped adam {k}", weights=True)
        print(f"step {step} {k}: worst |got-ref|/cond {worst:.3g} (tau {R.TAU_ADAM:.3g})")
    unclipped = R.adam_ema_ref(init["p"], init["g"], init["m"], init["v"], init["ema"], step, 1e-3, weight_decay=wd,
                               ema_decay=d, grad_scale=gs)
    for k in ("p", "m"):
        with pytest.raises(AssertionError):
            R.check_bound(got[k], *unclipped[k], R.TAU_ADAM, f"step {step} {k} against the unclipped reference", weights=True)


# ------------------------------------------------------------------------------------------------------------- TrainStep
def _model(dims, seed, precision):
    from gelslim_depth_amd.models.unet import UNet
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=dims, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.make_state(3, 1, dims, seed, "conditioned").items()},
                      strict=True)
    return m.to("cuda").train()


def _step(cfg, seed=5, **kw):
    from gelslim_depth_amd.train import TrainStep
    m = _model(cfg[1], seed, cfg[0])
    return m, TrainStep(m, **kw)


def _batches(cfg, k, bad_at=None):
    out = []
    for i in range(k):
        x, t = synth.make_batch(*cfg[2], 40 + i)
        if i == bad_at:
            x[1, 2, 3, 5] = np.inf
        out.append((torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()))
    return out


def _snapshot(m, step, counters=True):
    """The arenas and the BatchNorm buffers (counters=False: without num_batches_tracked, which counts skipped steps too)."""
    s = {"p": step.p_flat, "m": step.m_flat, "v": step.v_flat, "ema": step.ema_flat}
    s.update({"buf/" + k: b for k, b in m.named_buffers() if counters or b.dtype == torch.float32})
    return {k: v.detach().clone() for k, v in s.items()}


def _assert_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _first_norm(cfg):
    m, step = _step(cfg, max_grad_norm=math.inf)
    step(*_batches(cfg, 1)[0])
    return float(step.last_grad_norm)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_a_clip_that_never_bites_changes_no_bit(cfg):
    data = _batches(cfg, 3)
    m0, plain = _step(cfg)
    m1, clipped = _step(cfg, max_grad_norm=1e30)
    assert plain.last_grad_norm is None and plain.last_clip_coef is None
    for x, t in data:
        a, b = plain(x, t).clone(), clipped(x, t).clone()
        assert torch.equal(a, b)
        assert float(clipped.last_clip_coef) == 1.0 and 0.0 < float(clipped.last_grad_norm) < 1e30
    _assert_equal(_snapshot(m0, plain), _snapshot(m1, clipped))


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_clipped_step_matches_the_fp64_update(cfg):
    norm0 = _first_norm(cfg)
    m, step = _step(cfg, max_grad_norm=norm0 / 4)
    before = _snapshot(m, step)
    step(*_batches(cfg, 1)[0])
    torch.cuda.synchronize()
    got_norm, coef = float(step.last_grad_norm), float(step.last_clip_coef)
    assert step.last_grad_norm.is_cuda and step.last_grad_norm.shape == (1,) and step.last_clip_coef.shape == (1,)
    ref_norm = math.sqrt(float((step.g_flat.double() ** 2).sum()))
    print(f"{cfg[0]}: norm {got_norm!r} ref {ref_norm!r} coef {coef!r}")
    assert got_norm == norm0, "the same first step measures the same norm"
    assert abs(got_norm - ref_norm) <= 2.0 ** -23 * ref_norm
    assert 0.0 < coef < 1.0 and coef == float(coef_formula(step.last_grad_norm, norm0 / 4))
    ref = R.adam_ema_ref(before["p"], step.g_flat, before["m"], before["v"], before["ema"], 1, 1e-3, weight_decay=1e-6,
                         ema_decay=min(0.995, 2.0 / 11.0), grad_scale=float(f32(1.0) * f32(coef)))
    for k, arena in (("p", step.p_flat), ("m", step.m_flat), ("v", step.v_flat), ("ema", step.ema_flat)):
        R.check_bound(arena, *ref[k], R.TAU_ADAM, f"{cfg[0]} clipped step {k}", weights=True)
    unclipped = R.adam_ema_ref(before["p"], step.g_flat, before["m"], before["v"], before["ema"], 1, 1e-3, weight_decay=1e-6,
                               ema_decay=min(0.995, 2.0 / 11.0))
    with pytest.raises(AssertionError):
        R.check_bound(step.m_flat, *unclipped["m"], R.TAU_ADAM, "m against the unclipped reference", weights=True)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_inf_in_the_batch_skips_the_clipped_step(cfg):
    data = _batches(cfg, 2, bad_at=1)
    m, step = _step(cfg, nan_policy="skip", max_grad_norm=1.0)
    step(*data[0])
    before = _snapshot(m, step, counters=False)
    step(*data[1])
    assert step.skipped_steps() == 1 and step.step_count == 2
    _assert_equal(_snapshot(m, step, counters=False), before)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_step_with_both_controls_dispatches_no_aten_compute_op(cfg):
    """test_gpu_robust.py::test_fused_train_step_dispatches_no_aten_compute_op with max_grad_norm and lr_schedule on."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from gelslim_depth_amd.train import LRSchedule
    m, step = _step(cfg, max_grad_norm=0.5,
                    lr_schedule=LRSchedule(warmup_steps=3, decay="cosine", total_steps=8, min_lr=1e-5))
    xd, td = _batches(cfg, 1)[0]
    step(xd, td)                                   # first call allocates the activation buffers
    seen = []

    class Recorder(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    with Recorder():
        step(xd, td)
    torch.cuda.synchronize()
    harmless = ("aten.empty", "aten.view", "aten._unsafe_view", "aten.slice", "aten.select", "aten.as_strided", "aten.detach",
                "aten.alias", "aten.reshape", "aten.expand", "aten.unsqueeze", "aten.squeeze", "aten.t.", "aten.permute",
                "aten.narrow", "aten.lift_fresh", "aten.new_empty", "aten.empty_like", "aten.empty_strided")
    computing = sorted({f for f in seen if not f.startswith(harmless)})
    assert computing == [], computing
    assert math.isfinite(float(step.last_grad_norm)) and 0.0 < float(step.last_clip_coef) <= 1.0


# --------------------------------------------------------------------------------------------------- schedule in the step
def test_schedule_drives_the_step():
    from gelslim_depth_amd.train import LRSchedule, lr_at
    cfg = CONFIGS[0]
    sched = LRSchedule(warmup_steps=3, decay="cosine", total_steps=8, min_lr=1e-5)
    data = _batches(cfg, 2)
    m, step = _step(cfg, lr=2e-3, lr_schedule=sched)
    for i in range(8):
        step(*data[i % 2])
        assert step.current_lr() == lr_at(2e-3, sched, i + 1), i
        if i == 0:
            first = _snapshot(m, step)
    assert step.current_lr() == 1e-5
    m1, plain = _step(cfg, lr=lr_at(2e-3, sched, 1))
    assert plain.current_lr() == lr_at(2e-3, sched, 1) == pytest.approx(2e-3 / 3, rel=1e-15)
    plain(*data[0])
    _assert_equal(_snapshot(m1, plain), first)
    m2, base = _step(cfg, lr=2e-3)
    base(*data[0])
    assert not torch.equal(base.p_flat, first["p"]), "the warm-up rate must differ from the base rate"


# ------------------------------------------------------------------------------------------------------------------ resume
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_resume_with_clip_and_schedule_is_bitwise(tmp_path, cfg):
    from gelslim_depth_amd.train import LRSchedule, read_state
    kw = dict(max_grad_norm=_first_norm(cfg) / 4, lr_schedule=LRSchedule(warmup_steps=3, decay="linear", total_steps=6, min_lr=1e-4))
    data = _batches(cfg, 4)
    m, step = _step(cfg, **kw)
    want = [step(x, t).item() for x, t in data]
    ref = _snapshot(m, step)
    ref_clip = step.clip_buf.clone()
    m, step = _step(cfg, **kw)
    got = [step(x, t).item() for x, t in data[:2]]
    path = str(tmp_path / "state.pt")
    step.save_state(path)
    assert read_state(path)["version"] == 2
    m, step = _step(cfg, seed=6, **kw)
    step.load_state(path)
    assert step.step_count == 2 and step.current_lr() == pytest.approx(1e-3 * 2 / 3, rel=1e-15)
    got += [step(x, t).item() for x, t in data[2:]]
    assert got == want
    _assert_equal(_snapshot(m, step), ref)
    print(f"{cfg[0]}: clip after four steps {step.clip_buf.tolist()}")
    assert torch.equal(step.clip_buf, ref_clip) and 0.0 < float(step.last_clip_coef) <= 1.0


def test_state_versions_and_refusals(tmp_path):
    from gelslim_depth_amd.train import LRSchedule
    cfg = CONFIGS[0]
    x, t = _batches(cfg, 1)[0]
    _, plain = _step(cfg)
    plain(x, t)
    sd = plain.state_dict()
    assert sd["version"] == 1 and sd["hparams"]["max_grad_norm"] is None and sd["hparams"]["lr_schedule"] is None
    _, other = _step(cfg, seed=6)
    other.load_state_dict(sd)                       # strict
    assert torch.equal(other.p_flat, plain.p_flat)
    old = dict(sd, hparams={k: v for k, v in sd["hparams"].items() if k not in ("max_grad_norm", "lr_schedule")})
    _, other = _step(cfg, seed=6)
    other.load_state_dict(old)                      # a state written before the two fields existed: strict still
    assert torch.equal(other.p_flat, plain.p_flat)
    sched = LRSchedule(warmup_steps=2)
    _, both = _step(cfg, seed=6, max_grad_norm=1.0, lr_schedule=sched)
    before = both.p_flat.clone()
    with pytest.raises(ValueError, match=r"max_grad_norm is None in the state and 1\.0 here; pass strict=False"):
        both.load_state_dict(sd)
    with pytest.raises(ValueError, match=r"max_grad_norm is None in the state"):
        both.load_state_dict(old)
    assert torch.equal(both.p_flat, before)
    both(x, t)
    path = str(tmp_path / "both.pt")
    both.save_state(path)
    for kw, field in ((dict(max_grad_norm=2.0, lr_schedule=sched), "max_grad_norm is 1.0 in the state and 2.0 here"),
                      (dict(max_grad_norm=1.0, lr_schedule=LRSchedule(warmup_steps=3)), "lr_schedule is .*'warmup_steps': 2.* here"),
                      (dict(max_grad_norm=1.0), "lr_schedule is .* in the state and None here"),
                      (dict(lr_schedule=sched), "max_grad_norm is 1.0 in the state and None here")):
        _, s = _step(cfg, seed=6, **kw)
        with pytest.raises(ValueError, match=field):
            s.load_state(path)
        s.load_state(path, strict=False)
        assert s.step_count == 1 and torch.equal(s.p_flat, both.p_flat)
    _, same = _step(cfg, seed=6, max_grad_norm=1.0, lr_schedule=LRSchedule(warmup_steps=2))
    same.load_state(path)
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="max_grad_norm"):
            _step(cfg, max_grad_norm=bad)


# ------------------------------------------------------------------------------------------------------ data-parallel order
def test_one_rank_clipped_step_keeps_the_data_parallel_order(tmp_path):
    """One rank over RCCL with the collectives forced on: three clipped, scheduled, guarded steps equal the same steps without
    a process group bit for bit, and within a step the norm is taken behind every bucket's all-reduce and GradSync.finish,
    in front of the guard's MAX all-reduce and the optimiser."""
    from gelslim_depth_amd.train import LRSchedule
    cfg = CONFIGS[0]
    max_norm = _first_norm(cfg) / 4
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(REPO, "tests", "optim_controls_worker.py"), str(tmp_path), str(port), repr(max_norm)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = dict(np.load(os.path.join(tmp_path, "dp.npz")))
    assert str(res["backend"]) == "nccl" and int(res["skipped"]) == 0
    ev = [str(e) for e in res["events"]]
    n = ev.index("finish")
    assert n >= 2 and set(ev[:n]) == {"all_reduce:bucket"}, ev
    assert ev[n:] == ["finish", "gsd_grad_norm", "all_reduce:guard", "gsd_adam_ema_clip"], ev
    x, t = synth.make_batch(2, 21, 27, 6)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    m, step = _step(cfg, nan_policy="skip", max_grad_norm=max_norm, lr_schedule=LRSchedule(warmup_steps=2))
    losses = [float(step(xd, td).item()) for _ in range(3)]
    assert np.array_equal(np.array(losses), res["losses"])
    for k, arena in (("p", step.p_flat), ("m", step.m_flat), ("v", step.v_flat), ("ema", step.ema_flat), ("clip", step.clip_buf)):
        assert np.array_equal(arena.cpu().numpy(), res[k]), k
    assert 0.0 < float(step.last_clip_coef) < 1.0
