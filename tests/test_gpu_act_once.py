"""relu(bn(raw)) written once (GSD_ACT_ONCE): the activation pass, the pitched max-pool, and the consumers' bits.

Every comparison here is an equality.  The pass computes max(fmaf(raw, scale, shift), 0) -- fp64_ref.bnrelu_act emulates that
single rounding exactly -- and a conv3x3 or dW launch that reads the written tensor as ONE plain pitched source walks the same
channel chunks, K slabs and tiles as the launch that activates a deferred source on load, so outputs and BatchNorm partial sums
must be torch.equal: a difference needs an explanation, not a tolerance.
"""
import ctypes as C
import os

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu

GUARD = -7.25     # what a kernel must not write stays this value


@pytest.fixture(scope="module")
def gsd():
    from gelslim_depth_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("GSD_ACT_ONCE", "GSD_ACT_ONCE_FORCE", "GSD_CONV_W2D", "GSD_W2D_X4", "GSD_W2D_U4", "GSD_W2D_SPLIT", "GSD_WGRAD_W2D"):
        monkeypatch.delenv(k, raising=False)


def _r4(v):
    return (v + 3) // 4 * 4


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _raw(gsd, g, n, c, h, w):
    t = gsd.slack_empty((n, c, h, w), "cuda")
    t.copy_(torch.randn(n, c, h, w, generator=g))
    return t


def _coef(g, c):
    return (torch.rand(c, generator=g) + 0.5).cuda(), (torch.randn(c, generator=g) * 0.3).cuda()


def _pitched_guarded(n, ctot, h, pitch):
    """(whole buffer with 8 guard floats either side, its (n, ctot, h, pitch) view): 16-byte aligned, everything GUARD."""
    buf = torch.full((n * ctot * h * pitch + 16,), GUARD, device="cuda")
    return buf, buf[8:-8].view(n, ctot, h, pitch)


# ----------------------------------------------------------------------------------------------------------- activation pass
ACT_SHAPES = [(2, 3, 5, 7), (1, 5, 4, 8), (2, 4, 3, 13), (1, 2, 1, 1)]


@pytest.mark.parametrize("extra", [0, 4])
@pytest.mark.parametrize("shape", ACT_SHAPES)
def test_activation_pass(gsd, shape, extra):
    n, c, h, w = shape
    g = _gen(11 + w)
    raw = _raw(gsd, g, n, c, h, w)
    sc, sh = _coef(g, c)
    ref = R.bnrelu_act(raw, sc, sh)
    p = _r4(w) + extra
    buf, full = _pitched_guarded(n, c, h, p)
    src = gsd.make_src(raw, sc, sh, relu=True, slack=gsd.SLACK)
    dst = gsd.make_dst(full[..., :w])
    gsd.check(gsd.lib.gsd_bnrelu_pitched(C.byref(src), C.byref(dst), n, gsd.stream_ptr()), "bnrelu_pitched")
    torch.cuda.synchronize()
    assert torch.equal(full[..., :w].double(), ref), "values: max(fmaf(raw, scale, shift), 0) bit for bit"
    assert bool((full[..., w:] == 0).all()), "pad columns are written 0"
    assert bool((buf[:8] == GUARD).all()) and bool((buf[-8:] == GUARD).all()), "nothing outside the buffer"


def test_activation_pass_into_channel_offset_view(gsd):
    n, c, h, w = 2, 4, 3, 13
    g = _gen(5)
    raw = _raw(gsd, g, n, c, h, w)
    sc, sh = _coef(g, c)
    p = _r4(w)
    buf, full = _pitched_guarded(n, 12, h, p)
    dst = gsd.make_dst(full[:, 4:8, :, :w])
    src = gsd.make_src(raw, sc, sh, relu=True, slack=gsd.SLACK)
    gsd.check(gsd.lib.gsd_bnrelu_pitched(C.byref(src), C.byref(dst), n, gsd.stream_ptr()), "bnrelu_pitched")
    torch.cuda.synchronize()
    assert torch.equal(full[:, 4:8, :, :w].double(), R.bnrelu_act(raw, sc, sh))
    assert bool((full[:, 4:8, :, w:] == 0).all())
    assert bool((full[:, :4] == GUARD).all()) and bool((full[:, 8:] == GUARD).all()), "guard channels untouched"
    assert bool((buf[:8] == GUARD).all()) and bool((buf[-8:] == GUARD).all())


def test_activation_pass_refuses_what_it_cannot_write(gsd):
    raw = _raw(gsd, _gen(1), 1, 2, 3, 5)
    sc, sh = _coef(_gen(2), 2)
    src = gsd.make_src(raw, sc, sh, relu=True)
    dense = torch.empty(1, 2, 3, 5, device="cuda")
    d = gsd.make_dst(dense)                                    # pitch 5
    assert gsd.lib.gsd_bnrelu_pitched(C.byref(src), C.byref(d), 1, gsd.stream_ptr()) == gsd.GSD_ERR_BAD_ARG
    plain = gsd.make_src(raw)
    d = gsd.make_dst(gsd.pitched_empty((1, 2, 3, 5), "cuda"))
    assert gsd.lib.gsd_bnrelu_pitched(C.byref(plain), C.byref(d), 1, gsd.stream_ptr()) == gsd.GSD_ERR_BAD_ARG


# ----------------------------------------------------------------------------------------------------------- max-pool variant
@pytest.mark.parametrize("with_act", [False, True])
@pytest.mark.parametrize("hw", [(5, 7), (6, 8)])
def test_maxpool_pitched(gsd, hw, with_act):
    h, w = hw
    n, c = 2, 3
    g = _gen(3 + h)
    raw = _raw(gsd, g, n, c, h, w)
    sc, sh = _coef(g, c)
    src = gsd.make_src(raw, sc, sh, relu=True, slack=gsd.SLACK)
    hp, wp = h // 2, w // 2
    old = torch.empty(n, c, hp, wp, device="cuda")
    gsd.check(gsd.lib.gsd_maxpool2(C.byref(src), old.data_ptr(), n, c, h, w, gsd.stream_ptr()), "maxpool2")
    pbuf, pfull = _pitched_guarded(n, c, hp, _r4(wp))
    abuf, afull = _pitched_guarded(n, c, h, _r4(w))
    dp = gsd.make_dst(pfull[..., :wp])
    da = gsd.make_dst(afull[..., :w])
    gsd.check(gsd.lib.gsd_maxpool2_pitched(C.byref(src), C.byref(dp), C.byref(da) if with_act else None, n, gsd.stream_ptr()),
              "maxpool2_pitched")
    one = torch.full_like(afull, GUARD)
    d1 = gsd.make_dst(one[..., :w])
    gsd.check(gsd.lib.gsd_bnrelu_pitched(C.byref(src), C.byref(d1), n, gsd.stream_ptr()), "bnrelu_pitched")
    torch.cuda.synchronize()
    assert torch.equal(pfull[..., :wp], old), "pooled: the bits gsd_maxpool2 writes"
    assert bool((pfull[..., wp:] == 0).all())
    assert bool((pbuf[:8] == GUARD).all()) and bool((pbuf[-8:] == GUARD).all())
    if with_act:
        assert torch.equal(afull, one), "the second output: the bits of the activation pass, pad columns included"
        assert torch.equal(afull[..., :w].double(), R.bnrelu_act(raw, sc, sh))
    else:
        assert bool((afull == GUARD).all())
    assert bool((abuf[:8] == GUARD).all()) and bool((abuf[-8:] == GUARD).all())


# ----------------------------------------------------------------------------------------------------------- conv3x3, 2-D form
def _layout(gsd, mode, wt, co, ci):
    out = torch.zeros(gsd.lib.gsd_weight_layout_size(mode, co, ci), device="cuda")
    gsd.check(gsd.lib.gsd_weight_layout(mode, wt.data_ptr(), co, ci, out.data_ptr(), gsd.stream_ptr()), "layout")
    return out


def _conv_w2d(gsd, srcs, wl, ci, co, n, h, w):
    y = torch.full((n, co, h, w), GUARD, device="cuda")
    rows = gsd.lib.gsd_conv3x3_w2d_partial_rows(n, h, w, co)
    part = torch.full((rows * 2 * ((co + 63) // 64 * 64),), GUARD, device="cuda")
    arr = gsd.src_array(srcs)
    gsd.check(gsd.lib.gsd_conv3x3_w2d(arr, len(srcs), wl.data_ptr(), ci, co, gsd.dst_array([gsd.make_dst(y)]), 1, part.data_ptr(),
                                      n, h, w, gsd.stream_ptr()), "conv3x3_w2d")
    torch.cuda.synchronize()
    return y, part


def _activated(gsd, raw, sc, sh):
    """The activation pass's output for `raw` in a fresh zero-filled pitched buffer with slack."""
    n, c, h, w = raw.shape
    t = gsd.pitched_slack_zeros((n, c, h, w), "cuda")
    src, dst = gsd.make_src(raw, sc, sh, relu=True, slack=gsd.SLACK), gsd.make_dst(t)
    gsd.check(gsd.lib.gsd_bnrelu_pitched(C.byref(src), C.byref(dst), n, gsd.stream_ptr()), "bnrelu_pitched")
    return t


@pytest.mark.parametrize("case", [(8, 16, 6, 9), (8, 16, 17, 53)])
def test_conv_w2d_plain_pitched_equals_deferred(gsd, case):
    ci, co, h, w = case
    n = 2
    g = _gen(21 + h)
    raw = _raw(gsd, g, n, ci, h, w)
    sc, sh = _coef(g, ci)
    wl = _layout(gsd, 8, (torch.randn(co, ci, 3, 3, generator=g) * 0.1).cuda(), co, ci)
    y0, p0 = _conv_w2d(gsd, [gsd.make_src(raw, sc, sh, relu=True, slack=gsd.SLACK)], wl, ci, co, n, h, w)
    act = _activated(gsd, raw, sc, sh)
    y1, p1 = _conv_w2d(gsd, [gsd.make_src(act, slack=gsd.SLACK)], wl, ci, co, n, h, w)
    assert bool(torch.isfinite(y0).all()) and not bool((y0 == GUARD).any())
    assert torch.equal(y0, y1), "outputs"
    assert torch.equal(p0, p1), "BatchNorm partial sums"


def _decoder_operands(gsd, g, n, cs, cu, h, w):
    """([deferred skip, plain up] segments, the one concat source) of a decoder's first conv at h x w (up at 2(h/2) x 2(w/2))."""
    hu, wu = 2 * (h // 2), 2 * (w // 2)
    skip = _raw(gsd, g, n, cs, h, w)
    sc, sh = _coef(g, cs)
    up = _raw(gsd, g, n, cu, hu, wu)
    cat = gsd.pitched_slack_zeros((n, cs + cu, h, w), "cuda")
    s, d = gsd.make_src(skip, sc, sh, relu=True, slack=gsd.SLACK), gsd.make_dst(cat[:, :cs])
    gsd.check(gsd.lib.gsd_bnrelu_pitched(C.byref(s), C.byref(d), n, gsd.stream_ptr()), "bnrelu_pitched")
    cat[:, cs:, :hu, :wu].copy_(up)
    two = [gsd.make_src(skip, sc, sh, relu=True, slack=gsd.SLACK), gsd.make_src(up, slack=gsd.SLACK)]
    return two, [gsd.make_src(cat, slack=gsd.SLACK)], (skip, up, cat)


def test_conv_w2d_concat_buffer_equals_two_segments(gsd):
    n, cs, cu, h, w, co = 2, 4, 4, 8, 13, 16
    g = _gen(31)
    two, one, keep = _decoder_operands(gsd, g, n, cs, cu, h, w)
    wl = _layout(gsd, 8, (torch.randn(co, cs + cu, 3, 3, generator=g) * 0.1).cuda(), co, cs + cu)
    y0, p0 = _conv_w2d(gsd, two, wl, cs + cu, co, n, h, w)
    y1, p1 = _conv_w2d(gsd, one, wl, cs + cu, co, n, h, w)
    assert torch.equal(y0, y1) and torch.equal(p0, p1)


# ----------------------------------------------------------------------------------------------------------- dW
@pytest.mark.parametrize("co", [32, 128])
def test_wgrad_concat_buffer_equals_two_segments(gsd, co):
    """64 -> 32 channels on a 32 + 32 concat at 8 x 13, N = 2 (the row form), and 64 -> 128, which gsd_conv3x3_wgrad_form reports as
    the 2-D form; equality holds whichever form runs."""
    n, cs, cu, h, w = 2, 32, 32, 8, 13
    ci = cs + cu
    g = _gen(41)
    two, one, keep = _decoder_operands(gsd, g, n, cs, cu, h, w)
    dy = gsd.pitched_slack_zeros((n, co, h, w), "cuda")
    dy.copy_(torch.randn(n, co, h, w, generator=g))
    dys = gsd.make_src(dy)
    lib = gsd.lib
    assert lib.gsd_conv3x3_wgrad_takes_pitched_act(n, h, w, ci, co) == 1
    forms = [lib.gsd_conv3x3_wgrad_form(gsd.src_array(s), len(s), C.byref(dys), ci, co, n, h, w) for s in (two, one)]
    assert forms[0] == forms[1], forms
    assert forms[0] == (2 if co == 128 else 1), forms
    ws = torch.empty(max(1, lib.gsd_conv3x3_wgrad_workspace(n, h, w, ci, co)), device="cuda")
    out = []
    for s in (two, one):
        dw = torch.full((co, ci, 3, 3), GUARD, device="cuda")
        gsd.check(lib.gsd_conv3x3_wgrad(gsd.src_array(s), len(s), C.byref(dys), ci, co, dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                        n, h, w, gsd.stream_ptr()), "wgrad")
        torch.cuda.synchronize()
        out.append(dw)
    assert bool(torch.isfinite(out[0]).all())
    assert torch.equal(out[0], out[1])


# ----------------------------------------------------------------------------------------------------------- engine
def _two_steps(env):
    from gelslim_depth_amd import synth
    from gelslim_depth_amd.models.unet import UNet
    from gelslim_depth_amd.train import TrainStep
    dims = [16, 32, 64]
    st = synth.make_state(3, 1, dims, 5, "conditioned")
    x, t = synth.make_batch(2, 40, 53, 6)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        m = UNet(n_channels=3, n_classes=1, layer_dimensions=dims)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
        m = m.to("cuda:0").train()
        step = TrainStep(m)
        xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
        losses = [float(step(xd, td)), float(step(xd, td))]
        torch.cuda.synchronize()
        e = m._engine
        plan = (sum(u.plan.act_once for u in e.units), sum(up.plan.cat_on for up in e.ups), sum(e.plan.pooled_pitched))
        cats = [(up.cat, 2 * e.hs[up.level_in], 2 * e.ws[up.level_in]) for up in e.ups if up.cat is not None]
        res = dict(loss=losses, out=step._out.clone(), g=step.g_flat.clone(), p=step.p_flat.clone(),
                   bn=None if step.bn_flat is None else step.bn_flat.clone(),
                   bufs={k: v.clone() for k, v in m.state_dict().items()})
        return res, plan, cats
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("extra", [{}, {"GSD_CONV_W2D": "1"}, {"GSD_CONV_W2D": "1", "GSD_ACT_ONCE_FORCE": "1"}],
                         ids=["default", "w2d", "w2d-forced"])
def test_engine_act_once_equals_deferred(extra):
    """dims [16, 32, 64] at 40 x 53, batch 2: two train steps with GSD_ACT_ONCE=0 against 1, by default (the row form: the plan
    declines everything) and with GSD_CONV_W2D=1 (pitched pooled tensors; the model declines every pass that costs something at
    these sizes).  The third run adds GSD_ACT_ONCE_FORCE=1, which takes a pass wherever the launch admits it, so that the
    concat buffers and the scratch-buffer path are compared too."""
    a, plan_a, _ = _two_steps(dict(extra, GSD_ACT_ONCE="0"))
    b, plan_b, cats = _two_steps(dict(extra, GSD_ACT_ONCE="1"))
    assert plan_a == (0, 0, 0), plan_a
    want = {"default": (0, 0, 0), "w2d": (0, 0, 2), "w2d-forced": (5, 2, 2)}["default" if not extra else "w2d-forced" if len(extra) == 2 else "w2d"]
    assert plan_b == want, f"(second convs on the scratch buffer, concat buffers, pitched pooled tensors) = {plan_b}, expected {want}"
    assert a["loss"] == b["loss"]
    assert torch.equal(a["out"], b["out"]), "prediction"
    assert torch.equal(a["g"], b["g"]), "every gradient"
    assert torch.equal(a["p"], b["p"]), "every parameter"
    assert (a["bn"] is None) == (b["bn"] is None) and (a["bn"] is None or torch.equal(a["bn"], b["bn"]))
    for k in a["bufs"]:
        assert torch.equal(a["bufs"][k], b["bufs"][k]), k
    for cat, hu, wu in cats:   # what no kernel writes is still zero after two steps
        n, c2, h, w = cat.shape
        p = cat.stride(2)
        full = cat.as_strided((n, c2, h, p), cat.stride())
        assert bool((full[..., w:] == 0).all()), "pad columns"
        assert bool((full[:, c2 // 2:, :, wu:] == 0).all()) and bool((full[:, c2 // 2:, hu:] == 0).all()), "the column / row ConvT never writes"
