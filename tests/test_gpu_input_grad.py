"""The gradient of the fp32 U-Net with respect to its INPUT, in train and in eval mode (reference: unet.py:79-88 is a plain
nn.Module, differentiable w.r.t. x).

  * gsd_conv3x3_dgrad_bn (the first conv's dX with the BatchNorm backward applied on the fly) against an fp64 reference, element
    by element (tests/fp64_ref.py), at 320x427 with N = 2 and 32 and at edge shapes; bitwise run-to-run determinism;
  * the module in train mode against the reference's own x.grad (tests/golden/ginput_grad.npz), and bitwise unchanged outputs,
    parameter gradients and running statistics when x.requires_grad is set;
  * the module in eval mode: x.grad and the parameter gradients against the reference, the output bitwise equal to the no-grad
    eval forward, the running statistics untouched;
  * the engine's x.grad at the full size, teacher-forced from its own dz and coefficients, through the fused kernel and through the
    fallback (n_channels = 4; GSD_WGRAD_FIRST=0), and against the reference's full-size checksums;
  * the error paths that stay.

GSD_INPUT_GRAD_REPORT=<path>: write the measured ratios / errors behind every bound here as JSON.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import fp64_ref as R
from conftest import rel_l1

pytestmark = pytest.mark.gpu

# |got - ref| <= TAU_DF * cond for gsd_conv3x3_dgrad_bn (64 x 9 products per output element plus the d_raw formation terms
# |scale| (|dz| + |c1| + |xhat| |c2|) in cond), at no more than 4x the worst ratio measured on the MI355X and far below
# ceiling(64) = 1.7e-4.
TAU_DF = 5.3e-7          # 1.34e-7 (teacher-forced x.grad, full size, N = 32); kernel cases alone: 8.3e-8 (edge shapes, Cout 16)
# the same check on the fallback (direct-form dX on the materialised d_raw): R.TAU_DIRECT's family, 1.6e-6
TAU_FALLBACK = R.TAU_DIRECT   # 4.51e-7 (n_channels = 4, N = 2)
# module against the reference's fp32 CPU autograd (ginput_grad.npz): relative L1 bounds, <= 4x the measured value
XGRAD_SMALL = 1.9e-5     # x.grad, [16, 32, 64] at 3x37x45: 4.80e-6 (train), 1.74e-6 (eval)
PGRAD_SMALL = 2.3e-5     # worst parameter-gradient checksum / sample error: 5.85e-6 (train), 9.2e-7 (eval)
XGRAD_FULL_SUMS = 1.9e-4  # full size, batch 1: sum |.|, sum of squares, sum / sum |.| of x.grad: 4.69e-5 (train, squares)
XGRAD_FULL = 2e-2         # ... the 64 samples (relative L1): 1.03e-2 (train; BatchNorm at batch 1 amplifies fp32 rounding)

MEASURED = {}
SMALL_DIMS = [16, 32, 64]
FULL_DIMS = [64, 128, 256, 512, 1024]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    path = os.environ.get("GSD_INPUT_GRAD_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(sorted(MEASURED.items())), f, indent=1)


def note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(v))


@pytest.fixture(scope="module")
def lib():
    from gelslim_depth_amd._lib import lib as L
    torch.cuda.set_device(0)
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------ the kernel
def operands(n, h, w, cout, cin=3, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    f = dict(device="cuda", dtype=torch.float32, generator=g)
    dz = torch.randn((n, cout, h, w), **f)
    raw = torch.randn((n, cout, h, w), **f) * 2.0 + 0.5
    scale = torch.rand((cout,), **f) + 0.5
    mean = torch.randn((cout,), **f) * 0.3
    invstd = torch.rand((cout,), **f) + 0.5
    c1 = torch.randn((cout,), **f) * 0.2
    c2 = torch.randn((cout,), **f) * 0.2
    wt = torch.randn((cout, cin, 3, 3), **f) * (2.0 / (9 * cout)) ** 0.5
    return dz, raw, scale, mean, invstd, c1, c2, wt


def launch(lib, ops, bn=True):
    dz, raw, scale, mean, invstd, c1, c2, wt = ops
    n, cout, h, w = dz.shape
    cin = wt.shape[1]
    dx = torch.full((n, cin, h, w), float("nan"), device="cuda")
    p = (lambda t: t.data_ptr()) if bn else (lambda t: None)
    rc = lib.gsd_conv3x3_dgrad_bn(dz.data_ptr(), p(raw), p(scale), p(mean), p(invstd), p(c1), p(c2), wt.data_ptr(), cin, cout,
                                  dx.data_ptr(), n, h, w, stream())
    assert rc == 0, lib.gsd_last_error()
    torch.cuda.synchronize()
    return dx


def draw_ref(dz, raw, scale, mean, invstd, c1, c2, bn=True):
    """(d_raw, formation cond) in fp64 from the same fp32 operands."""
    if not bn:
        return dz.double(), dz.double().abs()
    c = (1, -1, 1, 1)
    v = lambda t: t.double().view(c)   # noqa: E731
    xhat = (raw.double() - v(mean)) * v(invstd)
    d = v(scale) * (dz.double() - v(c1) - xhat * v(c2))
    form = v(scale).abs() * (dz.double().abs() + v(c1).abs() + xhat.abs() * v(c2).abs())
    return d, form


def dx_ref(ops, bn=True, wt=None, i0=0, i1=None):
    dz, raw, scale, mean, invstd, c1, c2, w0 = ops
    wt = w0 if wt is None else wt
    sl = slice(i0, i1)
    d, form = draw_ref(dz[sl], raw[sl], scale, mean, invstd, c1, c2, bn)
    ref, _ = R.conv3x3_dx(d, wt.double())
    cond, _ = R.conv3x3_dx(form, wt.double().abs())
    return ref, cond


def check_kernel(got, ops, bn, what, step=8):
    n = got.shape[0]
    worst = 0.0
    for i in range(0, n, step):
        ref, cond = dx_ref(ops, bn, i0=i, i1=min(n, i + step))
        worst = max(worst, R.check_bound(got[i:i + step], ref, cond, TAU_DF, what, n0=i))
    return worst


EDGE = [(1, 1, 1), (1, 1, 9), (2, 3, 2), (2, 2, 3), (1, 5, 7), (3, 17, 33), (2, 9, 510), (1, 4, 511), (1, 3, 1029)]


@pytest.mark.parametrize("cout", [64, 16])
@pytest.mark.parametrize("nhw", EDGE)
@pytest.mark.parametrize("bn", [True, False])
def test_kernel_edge_shapes_fp64(lib, nhw, cout, bn):
    n, h, w = nhw
    assert lib.gsd_conv3x3_dgrad_bn_supported(n, h, w, 3, cout) == 1
    ops = operands(n, h, w, cout, seed=h * 1000 + w)
    got = launch(lib, ops, bn)
    note(f"tau_edge_cout{cout}", check_kernel(got, ops, bn, f"dgrad_bn {nhw} cout {cout} bn {bn}"))


@pytest.mark.parametrize("n", [2, 32])
def test_kernel_full_size_fp64_and_mutation(lib, n):
    ops = operands(n, 320, 427, 64, seed=n)
    got = launch(lib, ops)
    note("tau_full", check_kernel(got, ops, True, f"dgrad_bn N={n} 320x427"))
    if n == 2:
        got_plain = launch(lib, ops, bn=False)
        note("tau_full_plain", check_kernel(got_plain, ops, False, "dgrad_bn plain N=2"))
    # a weight with one tap flipped (kh, kw) = (0, 0) <-> (2, 2) of one input channel must be rejected
    wm = ops[7].clone()
    wm[:, 1, 0, 0], wm[:, 1, 2, 2] = ops[7][:, 1, 2, 2].clone(), ops[7][:, 1, 0, 0].clone()
    ref, cond = dx_ref(ops, True, wt=wm, i0=0, i1=1)
    with pytest.raises(AssertionError):
        R.check_bound(got[:1], ref, cond, TAU_DF, "mutated tap")


def test_kernel_cin1_cin2(lib):
    for cin in (1, 2):
        ops = operands(2, 19, 45, 32, cin=cin, seed=cin)
        got = launch(lib, ops)
        note("tau_cin12", check_kernel(got, ops, True, f"dgrad_bn cin {cin}"))


def test_kernel_deterministic(lib):
    ops = operands(8, 320, 427, 64, seed=7)
    a = launch(lib, ops)
    b = launch(lib, ops)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ the module
def small_model(g, precision="fp32"):
    """The fixture's small network: its state comes from synth.make_state on the fixture's seed (not stored in the .npz)."""
    from gelslim_depth_amd import synth
    from gelslim_depth_amd.models.unet import UNet
    st = synth.make_state(3, 1, SMALL_DIMS, int(g["small/seed"]), "conditioned")
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=SMALL_DIMS, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    return m.cuda()


def small_batch(g):
    from gelslim_depth_amd import synth
    n, h, w = (int(v) for v in g["small/nhw"])
    x, t = synth.make_batch(n, h, w, int(g["small/seed"]) + 1)
    return torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()


def pgrad_err(grads, g, mode):
    """Worst relative error over every parameter gradient against the fixture's checksums (sum |.|, sum of squares, sum over
    sum |.|) and 64 samples (relative L1)."""
    worst = 0.0
    for k, v in grads.items():
        d = v.double()
        ref = g[f"small/{mode}/gradsum/{k}"]
        samples = v.reshape(-1)[torch.from_numpy(g[f"small/{mode}/gradidx/{k}"]).long().cuda()].cpu().numpy()
        errs = (abs(d.abs().sum().item() - ref[1]) / ref[1], abs(d.pow(2).sum().item() - ref[2]) / ref[2],
                abs(d.sum().item() - ref[0]) / ref[1], rel_l1(samples, g[f"small/{mode}/gradsample/{k}"]))
        worst = max(worst, *errs)
    return worst


def step(m, x, tgt, want_x):
    for p in m.parameters():
        p.grad = None
    xx = x.clone().requires_grad_(want_x)
    y = m(x=xx)
    loss = torch.mean((y - tgt) ** 2)
    loss.backward()
    torch.cuda.synchronize()
    return y.detach(), (xx.grad if want_x else None), {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.fixture(scope="module")
def fixture_ig(golden):
    return golden("ginput_grad.npz")


def test_train_module_input_grad_against_reference(fixture_ig):
    g = fixture_ig
    x, tgt = small_batch(g)
    m = small_model(g).train()
    y, gx, grads = step(m, x, tgt, True)
    assert rel_l1(y.cpu().numpy(), g["small/train/y"]) < 1e-4
    e = rel_l1(gx.cpu().numpy(), g["small/train/xgrad"])
    note("small_train_xgrad_rel_l1", e)
    assert e < XGRAD_SMALL, e
    worst = pgrad_err(grads, g, "train")
    note("small_train_pgrad_rel_l1", worst)
    assert worst < PGRAD_SMALL, worst


def test_train_module_unchanged_by_input_grad(fixture_ig):
    g = fixture_ig
    x, tgt = small_batch(g)
    ma, mb = small_model(g).train(), small_model(g).train()
    ya, _, ga = step(ma, x, tgt, False)
    yb, gxb, gb = step(mb, x, tgt, True)
    assert gxb is not None and bool(torch.isfinite(gxb).all())
    assert torch.equal(ya, yb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    ba, bb = dict(ma.named_buffers()), dict(mb.named_buffers())
    for k in ba:
        assert torch.equal(ba[k], bb[k]), k


def test_eval_module_input_and_parameter_grads(fixture_ig):
    g = fixture_ig
    x, tgt = small_batch(g)
    m = small_model(g).eval()
    before = {k: b.clone() for k, b in m.named_buffers()}
    with torch.no_grad():
        y0 = m(x=x)
    y, gx, grads = step(m, x, tgt, True)
    assert torch.equal(y, y0)                                       # bitwise the no-grad eval forward
    for k, b in m.named_buffers():
        assert torch.equal(b, before[k]), k                         # running stats and num_batches_tracked untouched
    assert rel_l1(y.cpu().numpy(), g["small/eval/y"]) < 1e-4
    e = rel_l1(gx.cpu().numpy(), g["small/eval/xgrad"])
    note("small_eval_xgrad_rel_l1", e)
    assert e < XGRAD_SMALL, e
    worst = pgrad_err(grads, g, "eval")
    note("small_eval_pgrad_rel_l1", worst)
    assert worst < PGRAD_SMALL, worst
    # eval without x.requires_grad: no graph, as before
    y2 = m(x=x)
    assert not y2.requires_grad and torch.equal(y2, y0)


# ------------------------------------------------------------------------------------------------------- full size
def full_model(n_channels=3, seed=2024):
    from gelslim_depth_amd import synth
    from gelslim_depth_amd.models.unet import UNet
    st = synth.make_state(n_channels, 1, FULL_DIMS, seed, "conditioned")
    m = UNet(n_channels=n_channels, n_classes=1, layer_dimensions=FULL_DIMS)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    return m.cuda()


def full_batch(n, c=3, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((n, c, 320, 427), device="cuda", generator=g)
    t = torch.rand((n, 1, 320, 427), device="cuda", generator=g)
    return x, t


@pytest.mark.parametrize("case", ["fused_b2", "fused_b32", "fallback_c4", "fallback_wgrad_first_off"])
def test_full_size_teacher_forced(case, monkeypatch):
    n = 32 if case == "fused_b32" else 2
    c = 4 if case == "fallback_c4" else 3
    if case == "fallback_wgrad_first_off":
        monkeypatch.setenv("GSD_WGRAD_FIRST", "0")
    m = full_model(c).train()
    x, t = full_batch(n, c)
    _, gx, _ = step(m, x, t, True)
    u = m._engine.enc[0][0]
    w = m.inc.double_conv[0].weight.detach()
    assert u.plan.fused_dw == case.startswith("fused")
    worst = 0.0
    for i in range(0, n, 8):
        j = min(n, i + 8)
        if u.plan.fused_dw:   # from the engine's own dz (u.g: the apply pass was skipped) and BatchNorm coefficients
            d, form = draw_ref(u.g[i:j], u.raw[i:j], u.scale, u.mean, u.invstd, u.c1, u.c2)
            ref, _ = R.conv3x3_dx(d, w.double())
            cond, _ = R.conv3x3_dx(form, w.double().abs())
            tau = TAU_DF
        else:            # from the d_raw gsd_bn_bwd_apply materialised
            ref, cond = R.conv3x3_dx(u.dsrc[i:j].double(), w.double())
            tau = TAU_FALLBACK
        worst = max(worst, R.check_bound(gx[i:j], ref, cond, tau, f"x.grad {case}", n0=i))
    note(f"tau_teacher_{case}", worst)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_full_size_against_reference(fixture_ig, mode):
    from gelslim_depth_amd import synth
    g = fixture_ig
    m = full_model().train(mode == "train")
    x, t = synth.make_batch(1, 320, 427, int(g["full/seed"]) + 1)
    _, gx, _ = step(m, torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda(), True)
    d = gx.double()
    sums = np.array([d.sum().item(), d.abs().sum().item(), d.pow(2).sum().item()])
    ref = g[f"full/{mode}/xgrad_sums"]
    e_abs = abs(sums[1] - ref[1]) / ref[1]
    e_sq = abs(sums[2] - ref[2]) / ref[2]
    e_sum = abs(sums[0] - ref[0]) / ref[1]
    samples = gx.reshape(-1)[torch.from_numpy(g[f"full/{mode}/xgrad_idx"]).cuda()].cpu().numpy()
    e_s = rel_l1(samples, g[f"full/{mode}/xgrad_samples"])
    for k, v in (("abs", e_abs), ("sq", e_sq), ("sum", e_sum), ("samples", e_s)):
        note(f"full_{mode}_xgrad_{k}", v)
    assert max(e_abs, e_sq, e_sum) < XGRAD_FULL_SUMS, (e_abs, e_sq, e_sum)
    assert e_s < XGRAD_FULL, e_s


# ------------------------------------------------------------------------------------------------------- error paths
def test_bf16_input_grad_still_refused(fixture_ig):
    from gelslim_depth_amd.models.unet import UNet
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=[32, 64, 128], precision="bf16").cuda().train()
    x = small_batch(fixture_ig)[0].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="fp32-only"):
        m(x=x)
    with torch.no_grad():
        m(x=x)


@pytest.mark.parametrize("train", [True, False])
def test_backward_after_newer_forward_raises(fixture_ig, train):
    m = small_model(fixture_ig).train(train)
    x = small_batch(fixture_ig)[0]
    y1 = m(x=x.clone().requires_grad_(True))
    m(x=x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="saved activations are gone"):
        y1.sum().backward()


def test_engine_backward_after_no_grad_eval_forward_raises(fixture_ig):
    from gelslim_depth_amd._lib import GsdError
    m = small_model(fixture_ig).eval()
    x = small_batch(fixture_ig)[0]
    with torch.no_grad():
        y = m(x=x)
    G = {k: torch.empty_like(p) for k, p in m.named_parameters()}
    with pytest.raises(GsdError, match="needs a preceding"):
        m._engine.backward(torch.ones_like(y), m._tensor_map(), G, dx=torch.empty_like(x))


@pytest.mark.parametrize("train", [True, False])
def test_trainstep_bound_model_refuses_input_grad(fixture_ig, train):
    """A model whose gradients a TrainStep owns (its flat arena) does not take the input-gradient path: TrainStep is outside
    this feature, and the refusal names the input gradient instead of handing back None."""
    from gelslim_depth_amd.train import TrainStep
    m = small_model(fixture_ig).train()
    TrainStep(m)
    m.train(train)
    x = small_batch(fixture_ig)[0].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="gradient with respect to its input"):
        m(x=x)
    with torch.no_grad():
        m(x=x)
