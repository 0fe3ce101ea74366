"""GPU: gsd_depth_loss_fwd_bwd against its fp64 reference (tests/depth_loss_ref.py), what it must leave alone, its guard and
argument checks, and DepthLoss through TrainStep (fp32 and bf16), the autograd path, the saved state and evaluate_loader.

Bounds (derived, not fitted).  Terms: every summand is non-negative and formed in fp64 from fp32 differences that the reference
forms identically, the accumulation is fp64 (fewer than 2^23 additions: below 2^-29 relative) and one store rounds to fp32
(2^-24): relative error at most 2^-20.  Gradient: at most 17 summands of at most four roundings each, so
|g - g_ref| <= 2^-19 * A * grad_scale with A the sum of the summands' magnitudes."""
import ctypes
import math

import numpy as np
import pytest
import torch

import depth_loss_ref as D
from gelslim_depth_amd import synth

pytestmark = pytest.mark.gpu

SENT = -7.25
TERM_BOUND = 2.0 ** -20
GRAD_BOUND = 2.0 ** -19
TERM_NAMES = ("L", "L_data", "L_grad", "mean e^2", "mean |e|", "contact fraction")
BLOCK_CAP = 1024                                  # the kernel's cap on 256-thread blocks (gsd_depth_loss.hip: DL_BLOCKS)
BIG = (8, 1, 160, 213)                            # 272640 elements > 1024 * 256: some threads take two iterations
OP_SHAPES = [(2, 1, 9, 11), (3, 2, 17, 23), (1, 1, 5, 37), (1, 1, 1, 1), BIG]
CONFIGS = [("fp32", [16, 32, 64], (2, 21, 27)), ("bf16", [32, 64, 128], (2, 37, 53))]
IDS = [c[0] for c in CONFIGS]
STEP_SPEC = dict(data="huber", huber_delta=0.05, contact_weight=4.0, contact_eps=1e-3, background=0.0, grad_weight=0.5,
                 grad_kind="l1", grad_scales=2)


def sid(shape):
    return "x".join(map(str, shape))


@pytest.fixture(scope="module")
def L():
    from gelslim_depth_amd import _lib
    return _lib


_CASES = {}
_REFS = {}


def case(shape, seed=None):
    """(o, t) on the CPU and on the GPU, made once per shape."""
    key = (tuple(shape), seed)
    if key not in _CASES:
        o, t = D.make_case(tuple(shape), seed=sum(shape) if seed is None else seed)
        _CASES[key] = (o, t, o.cuda(), t.cuda())
    return _CASES[key]


def ref(shape, spec_id):
    """The reference of a shared case, computed once and never modified (grad_scale 1)."""
    key = (tuple(shape), spec_id)
    if key not in _REFS:
        o, t, _, _ = case(shape)
        _REFS[key] = D.depth_loss_ref(o, t, D.SPECS[spec_id])
    return _REFS[key]


def c_spec(spec):
    from gelslim_depth_amd.train import DepthLoss
    return spec if isinstance(spec, ctypes.Structure) else DepthLoss(**spec).c_struct()


def run_op(L, spec, od, td, with_grad=True, grad_scale=1.0, guard=None):
    """One launch into sentinel-padded buffers; returns (terms, grad or None, the workspace's partial sums)."""
    n, k, h, w = od.shape
    need = L.lib.gsd_depth_loss_workspace(n, k, h, w)
    assert need == 5 * min(BLOCK_CAP, -(-od.numel() // 256))
    ws = torch.full((need + 8,), SENT, device="cuda", dtype=torch.float64)
    terms = torch.full((6 + 4,), SENT, device="cuda")
    gbuf = torch.full((od.numel() + 8,), SENT, device="cuda") if with_grad else None
    o0, t0 = od.clone(), td.clone()
    c = c_spec(spec)
    L.check(L.lib.gsd_depth_loss_fwd_bwd(ctypes.byref(c), od.data_ptr(), td.data_ptr(), n, k, h, w, grad_scale, terms.data_ptr(),
                                         L.ptr(gbuf), ws.data_ptr(), need, guard, L.stream_ptr()), "depth_loss_fwd_bwd")
    torch.cuda.synchronize()
    assert bool((ws[need:] == SENT).all()), "wrote past gsd_depth_loss_workspace doubles"
    assert bool((terms[6:] == SENT).all()), "wrote past the six terms"
    assert gbuf is None or bool((gbuf[od.numel():] == SENT).all()), "wrote past grad"
    assert torch.equal(od.view(torch.int32), o0.view(torch.int32)) and torch.equal(td, t0), "the inputs were written"
    return terms[:6].clone(), None if gbuf is None else gbuf[:od.numel()].view(od.shape).clone(), ws[:need].clone()


def check_terms(got, want, what):
    got, want = got.double().cpu(), want.double().cpu()
    for i, name in enumerate(TERM_NAMES):
        g, r = float(got[i]), float(want[i])
        print(f"{what}: {name} {g!r} ref {r!r} rel err {abs(g - r) / abs(r) if r else abs(g - r):.3g} (bound {TERM_BOUND:.3g})")
        assert abs(g - r) <= TERM_BOUND * abs(r), (what, name, g, r)


def check_grad(got, want, A, grad_scale, what):
    err = (got.double().cpu() - want).abs()
    bound = GRAD_BOUND * A * grad_scale
    worst = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
    print(f"{what}: gradient worst |err| / (2^-19 A) = {worst:.3g}, max |g| {float(want.abs().max()):.3g}")
    assert bool((err <= bound).all()), (what, worst)


# ---------------------------------------------------------------------------------------------- the op against the reference
@pytest.mark.parametrize("spec_id", list(D.SPECS))
@pytest.mark.parametrize("shape", OP_SHAPES, ids=[sid(s) for s in OP_SHAPES])
def test_op_against_fp64(L, shape, spec_id):
    spec = D.SPECS[spec_id]
    _, _, od, td = case(shape)
    if shape == BIG:
        assert od.numel() > BLOCK_CAP * 256 and L.lib.gsd_depth_loss_workspace(*shape) == 5 * BLOCK_CAP
    want, gwant, A = ref(shape, spec_id)
    what = f"{sid(shape)} {spec_id}"
    terms, grad, part = run_op(L, spec, od, td)
    check_terms(terms, want, what)
    check_grad(grad, gwant, A, 1.0, what)
    if spec["grad_scales"] == 0 or max(shape[2], shape[3]) == 1:
        assert float(terms[2]) == 0.0
    terms2, grad2, part2 = run_op(L, spec, od, td)
    assert torch.equal(terms, terms2) and torch.equal(grad, grad2) and torch.equal(part, part2), "two runs differ"
    terms3, none, part3 = run_op(L, spec, od, td, with_grad=False)
    assert none is None and torch.equal(terms, terms3) and torch.equal(part, part3), "the terms depend on whether grad is given"
    terms4, grad4, _ = run_op(L, spec, od, td, grad_scale=0.5)
    assert torch.equal(terms, terms4)
    check_grad(grad4, 0.5 * gwant, A, 0.5, what + " grad_scale 0.5")


@pytest.mark.parametrize("spec_id", list(D.SPECS))
def test_shard_invariance(L, spec_id):
    """The loss of a batch of 4 is the mean of the losses of its halves, and each half's gradient taken with grad_scale = 1/2
    is the matching half of the full-batch gradient: what data parallelism with 1/world in Adam relies on."""
    spec = D.SPECS[spec_id]
    shape = (4, 2, 17, 23)
    o, t, od, td = case(shape, seed=11)
    _, gwant, A = D.depth_loss_ref(o, t, spec)
    full, gfull, _ = run_op(L, spec, od, td)
    halves = [run_op(L, spec, od[i:i + 2].contiguous(), td[i:i + 2].contiguous(), grad_scale=0.5) for i in (0, 2)]
    mean = 0.5 * (float(halves[0][0][0]) + float(halves[1][0][0]))
    print(f"{spec_id}: L {float(full[0])!r}, mean of the halves {mean!r}")
    assert abs(float(full[0]) - mean) <= TERM_BOUND * mean
    for i, (_, g, _) in zip((0, 2), halves):
        # against the reference's half of the full-batch gradient, and against the kernel's own full-batch gradient
        check_grad(g, gwant[i:i + 2], A[i:i + 2], 1.0, f"{spec_id} half {i // 2}")
        assert bool(((g.double() - gfull[i:i + 2].double()).abs().cpu() <= GRAD_BOUND * A[i:i + 2]).all())


# ------------------------------------------------------------------------------------------- does not change what exists
@pytest.mark.parametrize("shape", [(3, 2, 17, 23), BIG], ids=sid)
def test_default_spec_reproduces_the_mse_kernel(L, shape):
    from gelslim_depth_amd.train import DepthLoss, loss_fwd_bwd
    assert DepthLoss().spec()["data"] == "mse"
    _, _, od, td = case(shape)
    terms, grad, _ = run_op(L, DepthLoss().spec(), od, td)
    loss = torch.zeros((1,), device="cuda")
    g_old = torch.empty_like(od)
    loss_fwd_bwd("mse", od, td, g_old, loss, torch.empty((2048,), device="cuda", dtype=torch.float64))
    torch.cuda.synchronize()
    a, b = float(terms[0]), float(loss)
    print(f"{sid(shape)}: DepthLoss() {a!r}, gsd_loss_fwd_bwd {b!r}")
    assert abs(a - b) <= TERM_BOUND * b and torch.equal(terms[0], terms[1]) and torch.equal(terms[0], terms[3])
    assert float(terms[2]) == 0.0
    A = (2.0 * (od.double() - td.double()).abs() / od.numel()).cpu()
    assert bool(((grad.double() - g_old.double()).abs().cpu() <= GRAD_BOUND * A).all())


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


def _batches(cfg, k):
    """Depth-like targets: synth's U(-0.9, 0] on about 30 % of the pixels, exactly 0 elsewhere."""
    out = []
    for i in range(k):
        x, t = synth.make_batch(*cfg[2], 40 + i)
        keep = np.random.Generator(np.random.PCG64(90 + i)).random(t.shape) < 0.3
        out.append((torch.from_numpy(x).cuda(), torch.from_numpy(np.where(keep, t, np.float32(0.0)).astype(np.float32)).cuda()))
    return out


def _depth(**over):
    from gelslim_depth_amd.train import DepthLoss
    return DepthLoss(**dict(STEP_SPEC, **over))


def test_string_losses_never_reach_the_new_entry_point(L, monkeypatch):
    calls = []
    real = L.lib.gsd_depth_loss_fwd_bwd

    def counted(*args):
        calls.append(args)
        return real(*args)
    monkeypatch.setattr(L.lib, "gsd_depth_loss_fwd_bwd", counted)
    cfg = CONFIGS[0]
    x, t = _batches(cfg, 1)[0]
    for kind in ("mse", "l1"):
        _, step = _step(cfg, loss=kind)
        step(x, t)
        assert step.last_loss_terms is None and step.last_loss.shape == (1,)
    torch.cuda.synchronize()
    assert calls == []
    _, step = _step(cfg, loss=_depth())
    step(x, t)
    torch.cuda.synchronize()
    assert len(calls) == 1, "the wrapper sees a DepthLoss step: the two assertions above mean something"


# -------------------------------------------------------------------------------------------------------- guard and errors
@pytest.mark.parametrize("bad", [math.nan, math.inf], ids=["nan", "inf"])
def test_non_finite_output_marks_the_guard(L, bad):
    shape = (3, 2, 17, 23)
    _, _, od, td = case(shape)
    od = od.clone()
    od[1, 1, 4, 7] = bad
    words = torch.tensor([0, 5], dtype=torch.int32, device="cuda")
    terms, grad, _ = run_op(L, D.SPEC_FULL, od, td, guard=L.make_guard(words, 9))
    assert not math.isfinite(float(terms[0])) and words.tolist() == [9, 5]
    # without a guard: the same terms, and run_op's sentinels show nothing else was written
    terms2, _, _ = run_op(L, D.SPEC_FULL, od, td)
    assert not math.isfinite(float(terms2[0]))
    # a finite loss leaves the words alone
    words = torch.tensor([3, 5], dtype=torch.int32, device="cuda")
    run_op(L, D.SPEC_FULL, case(shape)[2], td, guard=L.make_guard(words, 9))
    assert words.tolist() == [3, 5]


def test_bad_arguments_return_before_any_launch(L):
    shape = (2, 1, 9, 11)
    _, _, od, td = case(shape)
    need = L.lib.gsd_depth_loss_workspace(*shape)
    ws = torch.full((need + 2,), SENT, device="cuda", dtype=torch.float64)
    terms = torch.full((6,), SENT, device="cuda")
    grad = torch.full((od.numel(),), SENT, device="cuda")
    words = torch.zeros((2,), dtype=torch.int32, device="cuda")

    def call(spec=D.SPEC_FULL, o=od.data_ptr(), t=td.data_ptr(), dims=shape, terms_p=terms.data_ptr(), ws_p=ws.data_ptr(),
             ws_elems=need, guard=None, **fields):
        c = None
        if spec is not None:
            c = c_spec(spec)
            for k, v in fields.items():
                setattr(c, k, v)
        return L.lib.gsd_depth_loss_fwd_bwd(None if c is None else ctypes.byref(c), o, t, *dims, 1.0, terms_p, grad.data_ptr(),
                                            ws_p, ws_elems, guard, L.stream_ptr())
    no_tick = L.gsd_guard()
    no_tick.words, no_tick.tick = words.data_ptr(), 0
    bad_arg = [dict(spec=None), dict(o=None), dict(t=None), dict(terms_p=None), dict(ws_p=None),
               dict(dims=(0, 1, 9, 11)), dict(dims=(2, -1, 9, 11)), dict(dims=(2, 1, 0, 11)), dict(dims=(2, 1, 9, 0)),
               dict(data_kind=3), dict(data_kind=-1), dict(grad_kind=2), dict(grad_kind=-1), dict(grad_scales=5),
               dict(grad_scales=-1), dict(reserved=1),
               dict(huber_delta=0.0), dict(huber_delta=-0.1), dict(huber_delta=math.nan), dict(huber_delta=math.inf),
               dict(contact_weight=-1.0), dict(contact_weight=math.nan), dict(contact_weight=math.inf),
               dict(contact_eps=-1e-3), dict(contact_eps=math.nan), dict(contact_eps=math.inf),
               dict(background=math.nan), dict(background=math.inf),
               dict(grad_weight=-0.5), dict(grad_weight=math.nan), dict(grad_weight=math.inf),
               dict(ws_p=ws.data_ptr() + 4), dict(guard=ctypes.pointer(no_tick))]
    for kw in bad_arg:
        assert call(**kw) == L.GSD_ERR_BAD_ARG, kw
        assert b"gsd_depth_loss_fwd_bwd" in L.lib.gsd_last_error(), kw
    for elems in (need - 1, 0, -3):
        assert call(ws_elems=elems) == L.GSD_ERR_WORKSPACE, elems
        assert b"workspace" in L.lib.gsd_last_error()
    torch.cuda.synchronize()
    for buf in (ws, terms, grad):
        assert bool((buf == SENT).all()), "a refused call launched something"
    assert words.tolist() == [0, 0]
    assert call() == L.GSD_OK                       # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert bool((terms != SENT).all()) and bool((ws[need:] == SENT).all())
    assert call(huber_delta=0.0, data_kind=0) == L.GSD_OK, "delta is read for huber only"
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ TrainStep, fp32 and bf16
def _flat_grads(model, step):
    """model's p.grad laid out like step's gradient arena."""
    g = torch.zeros_like(step.g_flat)
    for n, p in model.named_parameters():
        o, s = step.offsets[n]
        g[o:o + s] = p.grad.reshape(-1)
    return g


def _autograd_gap(cfg, loss, loss_fn, x, t):
    """max |g_flat - autograd gradient| / max |autograd gradient| after one fused step and one autograd pass from equal weights."""
    m, step = _step(cfg, loss=loss)
    step(x, t)
    m2 = _model(cfg[1], 5, cfg[0])
    loss_fn(m2(x=x), t).backward()
    torch.cuda.synchronize()
    want = _flat_grads(m2, step)
    return float((step.g_flat - want).abs().max()) / float(want.abs().max()), torch.equal(step.g_flat, want)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_train_step_terms_and_gradient(cfg):
    from gelslim_depth_amd.train import depth_loss, mse_loss
    x, t = _batches(cfg, 1)[0]
    spec = _depth()
    m, step = _step(cfg, loss=spec)
    loss = step(x, t)
    torch.cuda.synchronize()
    assert loss.shape == (1,) and step.last_loss_terms.shape == (6,) and step.last_loss_terms.is_cuda
    assert torch.equal(loss, step.last_loss_terms[0:1]) and loss.data_ptr() == step.last_loss.data_ptr()
    want, _, _ = D.depth_loss_ref(step._out, t, spec.spec())
    check_terms(step.last_loss_terms, want, f"{cfg[0]} step")
    assert 0.2 < float(step.last_loss_terms[5]) < 0.4 and float(step.last_loss_terms[2]) > 0
    # the fused step against the autograd path; the bar is what the same comparison gives for loss="mse" on this build
    bar, bar_bits = _autograd_gap(cfg, "mse", lambda o, tt: mse_loss(o, tt), x, t)
    gap, bits = _autograd_gap(cfg, spec, lambda o, tt: depth_loss(o, tt, spec), x, t)
    print(f"{cfg[0]}: fused vs autograd gradient, relative max gap: mse {bar:.3g} (bitwise {bar_bits}), depth loss {gap:.3g} "
          f"(bitwise {bits})")
    assert gap <= bar and (bits or not bar_bits)
    # the spec dict is accepted by the autograd form too
    m3 = _model(cfg[1], 5, cfg[0])
    assert float(depth_loss(m3(x=x), t, spec.spec()).detach()) == float(loss)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_resume_with_a_depth_loss_is_bitwise(tmp_path, cfg):
    from gelslim_depth_amd.train import read_state
    spec = _depth()
    data = _batches(cfg, 4)
    m, step = _step(cfg, loss=spec)
    want = [step(x, t).item() for x, t in data]
    ref_arenas = [a.clone() for a in (step.p_flat, step.m_flat, step.v_flat, step.ema_flat)]
    ref_terms = step.last_loss_terms.clone()
    m, step = _step(cfg, loss=spec)
    got = [step(x, t).item() for x, t in data[:2]]
    path = str(tmp_path / "state.pt")
    step.save_state(path)
    assert read_state(path)["hparams"]["loss"] == spec.spec()
    m, step = _step(cfg, seed=6, loss=_depth())
    step.load_state(path)
    got += [step(x, t).item() for x, t in data[2:]]
    assert got == want
    for a, b in zip(ref_arenas, (step.p_flat, step.m_flat, step.v_flat, step.ema_flat)):
        assert torch.equal(a, b)
    assert torch.equal(step.last_loss_terms, ref_terms)


def test_state_refuses_another_spec_and_names_the_field(tmp_path):
    cfg = CONFIGS[0]
    x, t = _batches(cfg, 1)[0]
    _, step = _step(cfg, loss=_depth())
    step(x, t)
    path = str(tmp_path / "state.pt")
    step.save_state(path)
    for other, msg in ((_depth(grad_weight=0.25), r"loss field grad_weight is 0\.5 in the state and 0\.25 here; pass strict=False"),
                       (_depth(grad_scales=3), r"loss field grad_scales is 2 in the state and 3 here"),
                       (_depth(data="l1", huber_delta=None), r"loss field data is 'huber' in the state and 'l1' here"),
                       ("mse", r"loss is \{.*'grad_weight': 0\.5.*\} in the state and 'mse' here")):
        _, s = _step(cfg, seed=6, loss=other)
        before = s.p_flat.clone()
        with pytest.raises(ValueError, match=msg):
            s.load_state(path)
        assert torch.equal(s.p_flat, before) and s.step_count == 0
        s.load_state(path, strict=False)
        assert s.step_count == 1 and torch.equal(s.p_flat, step.p_flat) and s.loss_kind == other
    # a state written with a string loss: loads into a string step as before, refused by a DepthLoss step
    _, plain = _step(cfg)
    plain(x, t)
    sd = plain.state_dict()
    assert sd["hparams"]["loss"] == "mse" and sd["version"] == 1
    _, s = _step(cfg, seed=6)
    s.load_state_dict(sd)
    _, s = _step(cfg, seed=6, loss=_depth())
    with pytest.raises(ValueError, match=r"loss is 'mse' in the state and \{.*\} here"):
        s.load_state_dict(sd)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_evaluate_loader_takes_a_depth_loss(cfg):
    from gelslim_depth_amd.harness import evaluate_loader
    spec = _depth()
    data = _batches(cfg, 2)
    m, step = _step(cfg, loss=spec)
    step(*data[0])
    loader = [{"tactile_image": x, "depth_image": t} for x, t in data]
    got = evaluate_loader(step, loader, loss_kind=spec)
    refs = [float(D.depth_loss_ref(step.evaluate(x), t, spec.spec())[0][0]) for x, t in data]
    want = sum(refs) / len(refs)
    print(f"{cfg[0]}: evaluate_loader {got!r}, mean of the reference's L {want!r}")
    assert abs(got - want) <= TERM_BOUND * want
    assert evaluate_loader(step, loader) != got, "the default stays the plain MSE"
