"""GPU parity, network level: the drop-in UNet / TrainStep against (a) golden vectors produced by running
the reference (tests/golden/*.npz) and (b) the oracle on seeded inputs.

Tolerances
  * outputs (depth maps): north-star bound 1e-3 relative L1; we assert 1e-4 (eval) / 2e-4 (train mode).
  * whole-network gradients: 2e-2 relative L1.  Gradients of a ReLU/max-pool net are chaotic in the last
    bits -- one pre-activation that lands on the other side of 0 moves every upstream weight gradient by
    ~1e-3 (measured between two CPU implementations, tests/test_oracle.py) -- so the tight gradient checks
    are the op-level ones in test_gpu_ops.py on identical inputs; this bound catches structural errors.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, sub, rel_l1
from gelslim_depth_amd import synth

pytestmark = pytest.mark.gpu


def make_model(dims, state):
    from gelslim_depth_amd.models.unet import UNet
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=dims, kernel_size=3, maxpool_size=2, upconv_stride=2)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    return m.to("cuda")


def golden_case(name, init):
    g = load_golden(name)
    dims = [int(v) for v in g["meta/dims"]]
    n, h, w = [int(v) for v in g["meta/nhw"]]
    seed = int(g["meta/seed"])
    st = synth.make_state(3, 1, dims, seed, init)
    x, tgt = synth.make_batch(n, h, w, seed + 1)
    return g, dims, st, x, tgt


@pytest.mark.parametrize("name,init", [("gtiny_conditioned.npz", "conditioned"), ("gtiny_refinit.npz", "reference")])
def test_tiny_autograd_path_matches_reference(name, init):
    """The reference's own step body (train_unet.py:346-347,370,374-375) typed against the drop-in module:
    unet(x=...), MSE, loss.backward(), torch.optim.Adam.step()."""
    from gelslim_depth_amd.train import mse_loss
    g, dims, st, x, tgt = golden_case(name, init)
    m = make_model(dims, st)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    m.eval()
    y0 = m(x=xd)
    assert y0.shape == (2, 1, 21, 27) and y0.dtype == torch.float32 and y0.is_cuda
    assert rel_l1(y0.cpu().numpy(), g["y_eval0"]) < 1e-4
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-6)
    losses = []
    for s in range(3):
        opt.zero_grad()
        out = m(x=xd)
        loss = mse_loss(input=out, target=td)
        loss.backward()
        if s == 0:
            assert rel_l1(out.detach().cpu().numpy(), g["y_train0"]) < 2e-4
            tol = 2e-2 if init == "conditioned" else 5e-2
            for k, v in sub(g, "grad0").items():
                got = dict(m.named_parameters())[k].grad.cpu().numpy()
                assert rel_l1(got, v) < tol, k
        opt.step()
        losses.append(loss.item())
        if s == 0:
            sd = m.state_dict()
            for k, v in sub(g, "buf1").items():
                if k.endswith("num_batches_tracked"):
                    assert int(sd[k]) == int(v)
                else:
                    assert rel_l1(sd[k].cpu().numpy(), v) < 1e-4, k
    np.testing.assert_allclose(losses, g["losses"], rtol=2e-4)
    sd = m.state_dict()
    for k, v in sub(g, "param3").items():
        assert rel_l1(sd[k].cpu().numpy(), v) < 2e-3, k
    m.eval()
    assert rel_l1(m(x=xd).cpu().numpy(), g["y_eval3"]) < 2e-3


def test_tiny_fused_trainstep_matches_reference_and_ema():
    from gelslim_depth_amd.train import TrainStep
    g, dims, st, x, tgt = golden_case("gtiny_conditioned.npz", "conditioned")
    m = make_model(dims, st)
    m.train()
    step = TrainStep(m, lr=1e-3, weight_decay=1e-6, ema_decay=0.995)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    losses = [step(xd, td).item() for _ in range(3)]
    np.testing.assert_allclose(losses, g["losses"], rtol=2e-4)
    sd = m.state_dict()
    assert list(sd.keys()) == list(st.keys())
    for k, v in sub(g, "param3").items():
        assert rel_l1(sd[k].cpu().numpy(), v) < 2e-3, k
    for k, v in sub(g, "buf3").items():
        if not k.endswith("num_batches_tracked"):
            assert rel_l1(sd[k].cpu().numpy(), v) < 2e-4, k
        else:
            assert int(sd[k]) == 3
    esd = step.ema_state_dict()
    for k, v in sub(g, "ema3_UNPINNED").items():      # torch_ema rule restated, not reference-pinned
        assert rel_l1(esd[k].cpu().numpy(), v) < 2e-3, k


def test_mid_net_vs_golden_and_oracle():
    from oracle import unet_numpy as on
    g, dims, st, x, tgt = golden_case("gmid_conditioned.npz", "conditioned")
    m = make_model(dims, st)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    m.eval()
    assert rel_l1(m(x=xd).cpu().numpy(), g["y_eval0"]) < 1e-4
    m.train()
    out = m(x=xd)
    assert rel_l1(out.detach().cpu().numpy(), g["y_train0"]) < 2e-4
    loss = torch.mean((out - td) ** 2)      # the reference's literal MSE expression through torch autograd
    loss.backward()
    assert abs(loss.item() - g["losses"][0]) < 2e-4 * g["losses"][0]
    grads = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    for k, v in sub(g, "gradsample0").items():
        flat = grads[k].reshape(-1)
        idx = np.linspace(0, flat.size - 1, num=min(64, flat.size)).astype(np.int64)
        assert rel_l1(flat[idx], v) < 2e-2, k
    # full tensors against the oracle
    net, _, first, _ = on.train_steps(st, x, tgt, 1)
    for k in grads:
        assert rel_l1(grads[k], first["grads"][k]) < 2e-2, k


def _check_stage_statistics(m, want, rtol):
    """Per-stage activation checksums of the HIP path against the reference's forward hooks (tests/golden/make_golden.py:
    mean, mean |.|, L2 norm of the output of inc, down[0..3], up[0..3]).  The engine never stores a normalised activation:
    a stage's output is relu(raw * scale + shift) of its second conv unit, rebuilt here from the engine's buffers."""
    eng = m._engine
    stages = {"inc": eng.enc[0][1]}
    for i in range(eng.L):
        stages[f"down{i}"] = eng.enc[i + 1][1]
        stages[f"up{i}"] = eng.dec[i][1]
    assert set(want) == set(stages)
    for k, u in stages.items():
        a = torch.relu(u.raw.double() * u.scale.double()[None, :, None, None] + u.shift.double()[None, :, None, None])
        got = np.array([a.mean().item(), a.abs().mean().item(), a.pow(2).sum().sqrt().item()])
        np.testing.assert_allclose(got, want[k], rtol=rtol, err_msg=k)


def test_full_size_config1_forward_and_train_step():
    """BASELINE.json configs[0]: one 3x320x427 image through the full-size net, vs the reference's own
    output; then one full train step, gradient checksums vs the reference."""
    g = load_golden("gfull_b1.npz")
    dims = [int(v) for v in g["meta/dims"]]
    seed = int(g["meta/seed"])
    st = synth.make_state(3, 1, dims, seed, "conditioned")
    x, tgt = synth.make_batch(1, 320, 427, seed + 1)
    m = make_model(dims, st)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    m.eval()
    y = m(x=xd)
    assert y.shape == (1, 1, 320, 427)
    err = rel_l1(y.cpu().numpy(), g["y_eval"])
    assert err < 1e-4, err
    _check_stage_statistics(m, sub(g, "act_eval"), 1e-4)
    m.train()
    from gelslim_depth_amd.train import mse_loss
    out = m(x=xd)
    _check_stage_statistics(m, sub(g, "act_train"), 2e-4)
    o64 = out.detach().double()
    np.testing.assert_allclose([o64.sum().item(), o64.abs().sum().item()], g["y_train_sum"], rtol=2e-4)
    assert rel_l1(out.detach().cpu().numpy(), g["y_train"].astype(np.float32)) < 1e-3   # fp16-stored fixture
    loss = mse_loss(out, td)
    loss.backward()
    assert abs(loss.item() - float(g["loss"])) < 2e-4 * float(g["loss"])
    for k, p in m.named_parameters():
        flat = p.grad.reshape(-1)
        idx = torch.from_numpy(np.linspace(0, flat.numel() - 1, num=min(64, flat.numel())).astype(np.int64)).cuda()
        assert rel_l1(flat[idx].cpu().numpy(), g[f"gradsample/{k}"]) < 3e-2, k
        l2 = p.grad.double().pow(2).sum().sqrt().item()
        assert abs(l2 - g[f"gradsum/{k}"][2]) < 2e-2 * g[f"gradsum/{k}"][2], k
    sd = m.state_dict()
    for k, v in sub(g, "bufsum").items():
        d = sd[k].double()
        np.testing.assert_allclose([d.sum().item(), d.abs().sum().item()], v, rtol=1e-3, atol=1e-5)


def test_batch_properties_full_resolution():
    """Size-independent properties at the bench resolution (batch 4 @ 320x427, full-size net):
    run-to-run bitwise determinism of the train step, and eval-mode batch independence
    (image i of a batch == the same image alone)."""
    from gelslim_depth_amd.train import TrainStep
    dims = [64, 128, 256, 512, 1024]
    st = synth.make_state(3, 1, dims, 7, "conditioned")
    x, tgt = synth.make_batch(4, 320, 427, 8)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    m = make_model(dims, st)
    m.eval()
    yb = m(x=xd).clone()
    y1 = m(x=xd[2:3].contiguous())
    assert torch.equal(yb[2:3], y1)
    results = []
    for _ in range(2):
        m2 = make_model(dims, st)
        m2.train()
        step = TrainStep(m2)
        l1 = step(xd, td).item()
        l2 = step(xd, td).item()
        results.append((l1, l2, step.p_flat.clone()))
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1]
    assert torch.equal(results[0][2], results[1][2])
    assert np.isfinite(results[0][0]) and np.isfinite(results[0][1])


@pytest.mark.parametrize("h,w,dims", [(160, 213, [8, 16, 32, 64, 128]), (97, 131, [8, 16, 32]), (64, 64, [16, 32]),
                                      (33, 470, [8, 16])])
def test_other_resolutions_vs_oracle(h, w, dims):
    """The model is fully convolutional: the reference ships 160x213 (config_unet_bigdata.py:29), BASELINE fixes
    320x427.  Other sizes exercise the host-side tile choosers (odd widths, very wide rows, square images)."""
    from oracle import unet_numpy as on
    st = synth.make_state(3, 1, dims, h * 1000 + w, "conditioned")
    x, tgt = synth.make_batch(2, h, w, h + w)
    m = make_model(dims, st)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    m.eval()
    assert rel_l1(m(x=xd).cpu().numpy(), on.UNetOracle(st).forward(x, train=False)) < 1e-4
    m.train()
    out = m(x=xd)
    loss = torch.mean((out - td) ** 2)
    loss.backward()
    net, losses, first, _ = on.train_steps(st, x, tgt, 1)
    assert abs(loss.item() - losses[0]) < 2e-4 * losses[0]
    for k, p in m.named_parameters():
        assert rel_l1(p.grad.cpu().numpy(), first["grads"][k]) < 2e-2, k


@pytest.mark.parametrize("k,h,w,dims", [(3, 37, 53, [8, 16, 32]), (8, 21, 27, [16]), (2, 64, 64, [16, 32])])
def test_more_than_one_output_class_vs_oracle(k, h, w, dims):
    """UNet(n_channels, n_classes > 1) (unet.py:61,77: OutConv(dims[0], n_classes)): forward, loss and EVERY gradient against the
    oracle -- the output conv's dX sums over the classes (gsd_bn_bwd_reduce mode 2, K <= 8) and its dW has K rows
    (gsd_conv1x1_out_wgrad).  No reference config trains with n_classes > 1; the constructor accepts it, so the drop-in does."""
    from oracle import unet_numpy as on
    from gelslim_depth_amd.models.unet import UNet
    st = synth.make_state(3, k, dims, 900 + k, "conditioned")
    x, tgt = synth.make_batch(2, h, w, 17 * k, n_classes=k)
    m = UNet(n_channels=3, n_classes=k, layer_dimensions=dims)
    m.load_state_dict({n_: torch.from_numpy(v.copy()) for n_, v in st.items()}, strict=True)
    m = m.to("cuda")
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    m.eval()
    y = m(x=xd)
    assert tuple(y.shape) == (2, k, h, w)
    assert rel_l1(y.cpu().numpy(), on.UNetOracle(st).forward(x, train=False)) < 1e-4
    m.train()
    out = m(x=xd)
    loss = torch.mean((out - td) ** 2)
    loss.backward()
    net, losses, first, _ = on.train_steps(st, x, tgt, 1)
    assert abs(loss.item() - losses[0]) < 2e-4 * losses[0]
    for name, p_ in m.named_parameters():
        assert p_.grad.shape == p_.shape
        tol = 1e-4 if name.startswith("outc.") else 2e-2     # outc: no upstream error; the rest: test_other_resolutions' bound
        assert rel_l1(p_.grad.cpu().numpy(), first["grads"][name]) < tol, name


@pytest.mark.parametrize("nch", [1, 4, 8])
def test_other_input_channel_counts_vs_oracle(nch):
    """UNet(n_channels != 3) (unet.py:61,67: DoubleConv(n_channels, ...)): the first layer has no Winograd form below 16 input
    channels and no dX; every other count takes the same direct-tap kernels as the RGB difference image.  fp32: loss and every
    gradient against the oracle; bf16 (the first-layer kernels fall back to im2col + dense taps when 9 C > 32): the loss within
    the bf16 bound of the fp32 one."""
    from oracle import unet_numpy as on
    from gelslim_depth_amd.models.unet import UNet
    dims = [32, 64]
    st = synth.make_state(nch, 1, dims, 5 + nch, "conditioned")
    x, tgt = synth.make_batch(2, 40, 52, 3, n_channels=nch)
    net, losses, first, _ = on.train_steps(st, x, tgt, 1)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    for prec in ("fp32", "bf16"):
        m = UNet(n_channels=nch, n_classes=1, layer_dimensions=dims, precision=prec)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
        m = m.to("cuda")
        m.train()
        out = m(x=xd)
        loss = torch.mean((out - td) ** 2)
        loss.backward()
        if prec == "fp32":
            assert abs(loss.item() - losses[0]) < 2e-4 * losses[0]
            for k, p_ in m.named_parameters():
                assert rel_l1(p_.grad.cpu().numpy(), first["grads"][k]) < 2e-2, k
        else:
            assert abs(loss.item() - losses[0]) < 5e-3 * losses[0]
            assert all(bool(torch.isfinite(p_.grad).all()) for p_ in m.parameters())


def test_winograd_and_direct_forms_agree(monkeypatch):
    """The two forms of the fp32 conv3x3 kernels (direct taps / Winograd F(4,3) along rows) through the
    whole network on the same weights and batch.
      * forward: outputs agree to < 1e-5 relative L1 (measured 8e-6; north-star bound 1e-3).
      * backward: F(4,3) is a few ten times noisier per product than direct fp32 accumulation (transform constants up to
        8), and weight/BatchNorm gradients are sums with heavy cancellation (sum dy = 0 per channel after BatchNorm
        backward), so the SAME absolute noise is a larger relative one: measured 4e-5 on the last conv's dW (no upstream
        error), then the backward pass amplifies whatever it is fed by 2-3x per BatchNorm level (the direct form goes
        1e-6 -> 8e-6 against the oracle the same way, the bf16 path 5e-4 -> 0.3): 2.3e-2 at the first layers of this
        net, 1.6e-2 on the full-size net at batch 32.  Bound 5e-2 here, 2e-4 on the last conv."""
    from gelslim_depth_amd.train import mse_loss
    dims = [16, 32, 64, 128]
    st = synth.make_state(3, 1, dims, 11, "conditioned")
    x, tgt = synth.make_batch(3, 72, 101, 12)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    res = {}
    # "0": direct taps; "1": Winograd F(4,3) rows everywhere; "2": the two-dimensional F(2x4,3x3) wherever the shape admits it
    # (Cin a multiple of 4: everything but the 3-channel first layer, which then keeps the row form)
    for algo in ("0", "1", "2"):
        monkeypatch.setenv("GSD_CONV_ALGO", min(algo, "1"))
        monkeypatch.setenv("GSD_WGRAD_ALGO", min(algo, "1"))
        monkeypatch.setenv("GSD_CONV_W2D", "1" if algo == "2" else "0")
        m = make_model(dims, st)
        m.train()
        out = m(x=xd)
        mse_loss(out, td).backward()
        forms = [u.plan.fwd[True].algo for u in m._engine.units]
        if algo == "2":
            assert forms[0] == 1 and all(f == 2 for f in forms[1:]), forms
            assert all(u.plan.dgrad.algo == 2 for u in m._engine.units[1:]), "dX launches too"
        else:
            assert all(f == int(algo) for f in forms), forms     # forcing a form includes the 3-channel first layer
        res[algo] = (out.detach().cpu().numpy(), {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()})
    for algo in ("1", "2"):
        assert rel_l1(res[algo][0], res["0"][0]) < 1e-5
        dev = {k: rel_l1(res[algo][1][k], res["0"][1][k]) for k in res["0"][1]}
        assert dev["up.2.conv.double_conv.3.weight"] < 2e-4, (algo, dev["up.2.conv.double_conv.3.weight"])
        assert max(dev.values()) < 5e-2, (algo, max(dev.values()))


@pytest.mark.parametrize("dims,n,h,w", [([16, 32, 64, 128], 3, 72, 101), ([64, 128, 256], 2, 80, 107)])
def test_side_stream_weight_gradients_are_bit_identical(monkeypatch, dims, n, h, w):
    """The weight-gradient launches run on a side stream next to the dX chain (engine_base.py: _on_side; two d_raw scratch buffers used
    in turn).  Same kernels on the same operands: every gradient must equal the single-stream schedule's bit for bit, over several
    steps.  Both schedules run undisturbed here: a missing dependency between the streams shows only if the GPU happens to run them
    in an unlucky order, which at these shapes it rarely does.  test_gpu_stream_order.py makes one stream late on purpose and holds
    the enforced order."""
    from gelslim_depth_amd.train import mse_loss
    st = synth.make_state(3, 1, dims, 5, "conditioned")
    x, tgt = synth.make_batch(n, h, w, 6)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    res = {}
    for side in ("0", "1"):
        monkeypatch.setenv("GSD_SIDE_DW", side)
        m = make_model(dims, st)
        m.train()
        assert (m._engine.side_dw) == (side == "1")
        grads = []
        for _ in range(3):
            for p_ in m.parameters():
                p_.grad = None
            out = m(x=xd)
            mse_loss(out, td).backward()
            grads.append({k: p_.grad.detach().clone() for k, p_ in m.named_parameters()})
        assert (m._engine.side is not None) == (side == "1")
        res[side] = grads
    for a_, b_ in zip(res["0"], res["1"]):
        for k in a_:
            assert torch.equal(a_[k], b_[k]), k


@pytest.mark.parametrize("dims,h,w", [([64, 128, 256, 512, 1024], 320, 427), ([16, 32, 64], 37, 53)])
def test_backward_teacher_forced_unit_by_unit(dims, h, w):
    """The whole-network gradient bounds above (2e-2 / 3e-2) rest on the argument that a ReLU / max-pool network amplifies
    last-bit differences; this test replaces the argument by a measurement at BASELINE's size (one 3x320x427 image through
    [64..1024]): every unit of the backward pass is checked TIGHTLY against the oracle fed with the HIP path's OWN upstream
    tensors (teacher forcing), so no error can hide behind another unit's amplification:
      forward   raw conv output of every unit vs oracle conv3x3 on the HIP path's input activation (1e-5), BatchNorm statistics;
      BatchNorm backward  d_gamma = sum dz*xhat, d_beta = sum dz from the HIP path's dz (1e-5 of their scale);
      conv dW   vs oracle on (HIP input activation, d_raw rebuilt from the HIP dz)                       (5e-5);
      conv dX   the gradient every producer received (dz of the unit below incl. its ReLU mask, the max-pool routing into the
                skip units, the pooled-gradient buffers, the cropped slice handed to the transposed convolution) vs the
                oracle's dX of the HIP d_raw                                                             (1e-5);
      ConvTranspose2d dW / db / dX and the output conv likewise.
    References: unet.py:7-57 (units), :39-49 (pad / cat), torch autograd's reverse sweep of train_unet.py:374."""
    from gelslim_depth_amd.train import mse_loss
    from oracle import unet_numpy as on
    st = synth.make_state(3, 1, dims, 21, "conditioned")
    x, tgt = synth.make_batch(1, h, w, 22)
    m = make_model(dims, st).train()
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    out = m(x=xd)
    loss = mse_loss(input=out, target=td)
    loss.backward()
    torch.cuda.synchronize()
    eng = m._engine
    G = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}
    npy = lambda t: t.detach().cpu().numpy()          # noqa: E731
    L_ = len(dims) - 1

    def act(u):          # the unit's activation as every consumer forms it on load: relu(raw * scale + shift)
        return np.maximum(npy(u.raw) * npy(u.scale)[None, :, None, None] + npy(u.shift)[None, :, None, None], 0).astype(np.float32)

    def close(got, ref, tol, what):
        scale = float(np.abs(ref).sum()) + 1e-30
        err = float(np.abs(got.astype(np.float64) - ref).sum()) / scale
        assert err < tol, f"{what}: relative L1 {err:.3e} >= {tol}"

    def unit_input(u):
        for lvl, (u0, u1) in enumerate(eng.enc):
            if u is u0:
                return x if lvl == 0 else npy(eng.pooled[lvl])
            if u is u1:
                return act(u0)
        for j, (u0, u1) in enumerate(eng.dec):
            lvl = L_ - 1 - j
            if u is u1:
                return act(u0)
            if u is u0:
                up_p, _ = on.pad_to(npy(eng.ups[j].out), eng.hs[lvl], eng.ws[lvl])
                return np.concatenate([act(eng.enc[lvl][1]), up_p], axis=1)
        raise AssertionError

    d_raw, dx_of = {}, {}
    for u in eng.units:
        a_in = unit_input(u)
        wt = st[u.wname]
        raw = npy(u.raw)
        close(raw, on.conv3x3_fwd(a_in, wt), 1e-5, f"{u.wname} forward")
        mean, invstd = npy(u.mean).astype(np.float64), npy(u.invstd).astype(np.float64)
        r64 = raw.astype(np.float64)
        assert np.allclose(mean, r64.mean(axis=(0, 2, 3)), rtol=1e-5, atol=1e-6), u.gname
        assert np.allclose(invstd, 1.0 / np.sqrt(r64.var(axis=(0, 2, 3)) + 1e-5), rtol=1e-5), u.gname
        xhat = (r64 - mean[None, :, None, None]) * invstd[None, :, None, None]
        g = npy(u.g).astype(np.float64)
        if u.plan.pitched or u.plan.fused_dw:
            # u.g still holds dz (the apply pass wrote d_raw out of place / the first layer's dW formed it on the fly)
            cnt = g.shape[0] * g.shape[2] * g.shape[3]
            dbeta, dgamma = g.sum(axis=(0, 2, 3)), (g * xhat).sum(axis=(0, 2, 3))
            close(G[u.bname], dbeta, 1e-5 + 1e-6 * float(np.abs(g).sum()) / (float(np.abs(dbeta).sum()) + 1e-30), f"{u.bname} grad")
            close(G[u.gname], dgamma, 1e-5 + 1e-6 * float(np.abs(g * xhat).sum()) / (float(np.abs(dgamma).sum()) + 1e-30), f"{u.gname} grad")
            gam = st[u.gname].astype(np.float64)
            dr = (gam * invstd)[None, :, None, None] * (g - dbeta[None, :, None, None] / cnt - xhat * dgamma[None, :, None, None] / cnt)
        else:
            dr = g                # d_raw in place
            mag = np.abs(dr).mean(axis=(0, 2, 3)) * dr.shape[0] * dr.shape[2] * dr.shape[3] + 1e-30
            assert float((np.abs(dr.sum(axis=(0, 2, 3))) / mag).max()) < 1e-4 and float((np.abs((dr * xhat).sum(axis=(0, 2, 3))) / mag).max()) < 1e-4
        d_raw[id(u)] = dr.astype(np.float32)
        dxr, dwr = on.conv3x3_bwd(a_in, wt, d_raw[id(u)], need_dx=u.need_dgrad)
        close(G[u.wname], dwr, 5e-5, f"{u.wname} grad")
        dx_of[id(u)] = dxr

    def masked(u, da):    # dz of unit u from the gradient w.r.t. its activation
        return np.where(act(u) > 0, da, 0).astype(np.float32)

    def dz_of(u):
        assert u.plan.pitched or u.plan.fused_dw, "this check reads dz from u.g"
        return npy(u.g)

    last = eng.dec[-1][1] if L_ > 0 else eng.enc[0][1]
    dout = 2.0 * (npy(out).astype(np.float64) - tgt) / out.numel()
    wout = st["outc.conv.weight"].reshape(1, -1, 1, 1).astype(np.float64)
    if last.plan.pitched:
        close(dz_of(last), masked(last, dout * wout), 1e-5, "output conv dX + ReLU mask")
    close(G["outc.conv.bias"], dout.sum(axis=(0, 2, 3)), 1e-5, "outc bias grad")
    close(G["outc.conv.weight"].reshape(-1), (dout * act(last).astype(np.float64)).sum(axis=(0, 2, 3)), 1e-5, "outc weight grad")
    for pair in list(eng.enc) + list(eng.dec):      # second unit -> first unit of a DoubleConv
        u0, u1 = pair
        if u0.plan.pitched or u0.plan.fused_dw:
            close(dz_of(u0), masked(u0, dx_of[id(u1)]), 1e-5, f"{u1.wname} dX into {u0.gname}")
    for lvl in range(1, L_ + 1):                     # first encoder unit of a level -> the pooled gradient
        close(npy(eng.dpooled[lvl]), dx_of[id(eng.enc[lvl][0])], 1e-5, f"dX into pooled[{lvl}]")
    for j, up in enumerate(eng.ups):
        lvl = L_ - 1 - j
        skip, d0 = eng.enc[lvl][1], eng.dec[j][0]
        dcat = dx_of[id(d0)]
        oy, ox = eng._pad_off(lvl)
        hu, wu = 2 * eng.hs[lvl + 1], 2 * eng.ws[lvl + 1]
        gup = dcat[:, skip.cout:, oy:oy + hu, ox:ox + wu]
        close(npy(up.dout), gup, 1e-5, f"dX slice handed to {up.wname}")
        prev = eng.dec[j - 1][1] if j > 0 else eng.enc[L_][1]
        dxu, dwu, dbu = on.convT_bwd(act(prev), st[up.wname], npy(up.dout))
        close(G[up.wname], dwu, 5e-5, f"{up.wname} grad")
        close(G[up.bname], dbu, 1e-5, f"{up.bname} grad")
        if prev.plan.pitched:
            close(dz_of(prev), masked(prev, dxu), 1e-5, f"{up.wname} dX into {prev.gname}")
        # the skip unit's gradient: its slice of the decoder conv's dX + the max-pool routing of the level below
        if skip.plan.pitched:
            _, idx = on.maxpool2_fwd(act(skip))
            dpool = on.maxpool2_bwd(npy(eng.dpooled[lvl + 1]), idx, act(skip).shape)
            close(dz_of(skip), masked(skip, dcat[:, :skip.cout] + dpool), 1e-5, f"skip + pool gradient into {skip.gname}")


@pytest.mark.parametrize("h,w,dims", [(20, 27, [18, 36]), (41, 53, [20, 40, 80]), (12, 9, [64, 128])])
def test_eval_forward_is_batch_independent_for_any_dims(h, w, dims):
    """Eval-mode batch independence (image i of a batch == the image alone, bitwise) where the two-dimensional Winograd form does
    not serve the channel counts (18: not a multiple of 4) and on small images: the engine decides the conv form from
    N-independent quantities in eval mode and never takes the row form there (it folds rows across images)."""
    st = synth.make_state(3, 1, dims, h + w, "conditioned")
    x, _ = synth.make_batch(5, h, w, 3)
    xd = torch.from_numpy(x).cuda()
    m = make_model(dims, st)
    m.eval()
    yb = m(x=xd).clone()
    for i in (0, 3, 4):
        assert torch.equal(yb[i:i + 1], m(x=xd[i:i + 1].contiguous())), i
    from oracle import unet_numpy as on
    assert rel_l1(yb.cpu().numpy(), on.UNetOracle(st).forward(x, train=False)) < 1e-4
