"""CPU: the depth-aware loss's reference (tests/depth_loss_ref.py) against torch autograd in fp64, its shard invariance,
DepthLoss's validation and spec round trip, and the ctypes layout of gsd_depth_loss.  No kernel is launched.

Scope of the autograd comparison: its inputs are rounded to multiples of 2^-12, so it checks the algebra of the gather-form
gradient and nothing about fp32 rounding; the reference's fp32 formation of e and of the pair differences is exercised by the
GPU tests, which hold the kernel to the same reference on unrounded inputs."""
import ctypes
import math

import pytest
import torch

import depth_loss_ref as D

# Inputs rounded to multiples of 2^-12: every o - t and every pair difference is then exact in fp32, so the reference (which
# forms them in fp32) and the autograd loss (fp64 throughout) are the same function and take the same branches.
QUANTUM = 2.0 ** -12
CPU_SPECS = ["huber_contact_l1x4", "mse_l2x3", "l1_contact"]


@pytest.mark.parametrize("spec_id", CPU_SPECS)
@pytest.mark.parametrize("shape", D.SHAPES, ids=["x".join(map(str, s)) for s in D.SHAPES])
def test_gather_gradient_equals_autograd(shape, spec_id):
    spec = D.SPECS[spec_id]
    o, t = D.make_case(shape, seed=sum(shape), quantum=QUANTUM)
    terms, grad, A = D.depth_loss_ref(o, t, spec)
    o64 = o.double().requires_grad_(True)
    loss = D.depth_loss_autograd(o64, t, spec)
    loss.backward()
    assert abs(float(loss.detach()) - float(terms[0])) <= 1e-14 * abs(float(terms[0]))
    scale = float(o64.grad.abs().max())
    diff = float((grad - o64.grad).abs().max())
    print(f"{shape} {spec_id}: max |gather - autograd| {diff:.3g}, largest gradient element {scale:.3g}")
    assert scale > 0 and diff <= 1e-14 * scale
    assert bool((A >= grad.abs() - 1e-18).all()), "A bounds the gradient it is the summand magnitudes of"
    assert float(terms[0]) == pytest.approx(float(terms[1]) + D.f32(spec["grad_weight"]) * float(terms[2]), rel=1e-15)


@pytest.mark.parametrize("spec_id", list(D.SPECS))
def test_loss_of_a_batch_is_the_mean_of_its_halves(spec_id):
    spec = D.SPECS[spec_id]
    o, t = D.make_case((4, 2, 17, 23), seed=11)
    full, gfull, _ = D.depth_loss_ref(o, t, spec)
    a, ga, _ = D.depth_loss_ref(o[:2], t[:2], spec, grad_scale=0.5)
    b, gb, _ = D.depth_loss_ref(o[2:], t[2:], spec, grad_scale=0.5)
    for i in range(6):
        mean = 0.5 * (float(a[i]) + float(b[i]))
        assert abs(float(full[i]) - mean) <= 1e-14 * abs(mean), (i, float(full[i]), mean)
    assert float((torch.cat([ga, gb]) - gfull).abs().max()) <= 1e-14 * float(gfull.abs().max())


def test_reference_on_a_case_done_by_hand():
    """1x1x2x3, e = [[1, 3, 0], [-2, 0, 0]] / 4, target 0 except one contact pixel; huber(0.5), contact weight 1, l1 slopes, 2 scales."""
    t = torch.tensor([[[[0.0, -0.5, 0.0], [0.0, 0.0, 0.0]]]])
    o = t + torch.tensor([[[[0.25, 0.75, 0.0], [-0.5, 0.0, 0.0]]]])
    spec = dict(data="huber", huber_delta=0.5, contact_weight=1.0, contact_eps=0.1, background=0.0, grad_weight=2.0,
                grad_kind="l1", grad_scales=2)
    terms, grad, A = D.depth_loss_ref(o, t, spec)
    l_data = (0.5 * 0.0625 + 2 * 0.5 * (0.75 - 0.25) + 0.5 * 0.25) / 6
    # scale 0: rows |0.5| + |-0.75| and |0.5| + 0; columns |-0.75| + |-0.75| + 0; over 6.  scale 1: grid (0,0), (0,2): |-0.25|; over 2
    l_grad = (0.5 + 0.75 + 0.5 + 0.75 + 0.75) / 6 + 0.25 / 2
    assert [float(v) for v in terms] == pytest.approx([l_data + 2.0 * l_grad, l_data, l_grad, (0.0625 + 0.5625 + 0.25) / 6,
                                                        1.5 / 6, 1 / 6], rel=1e-15)
    # pixel (0, 0): data 0.25/6; scale 0: right pair -sign(0.5), lower pair -sign(-0.75); scale 1: right pair -sign(-0.25)
    assert float(grad[0, 0, 0, 0]) == pytest.approx(0.25 / 6 + 2.0 / 6 * (-1 + 1) + 2.0 / 2 * (+1), rel=1e-15)
    # pixel (0, 1): contact, |e| beyond delta: 2 * 0.5 / 6; left pair +1, right pair -(-1), lower pair -(-1)
    assert float(grad[0, 0, 0, 1]) == pytest.approx(1.0 / 6 + 2.0 / 6 * 3, rel=1e-15)
    assert float(A[0, 0, 0, 0]) == pytest.approx(0.25 / 6 + 2.0 / 6 * 2 + 1.0, rel=1e-15)


def test_depth_loss_validation_names_the_field():
    from gelslim_depth_amd.train import DepthLoss
    bad = [
        (dict(data="rmse"), "data must be one of 'mse', 'l1', 'huber'"),
        (dict(data="huber"), "huber_delta is required for data='huber'"),
        (dict(data="huber", huber_delta=0.0), "huber_delta must be finite and positive"),
        (dict(data="huber", huber_delta=-1.0), "huber_delta must be finite and positive"),
        (dict(data="huber", huber_delta=math.inf), "huber_delta must be finite and positive"),
        (dict(data="huber", huber_delta="x"), "huber_delta must be a number"),
        (dict(data="mse", huber_delta=0.1), "huber_delta belongs to data='huber' only"),
        (dict(contact_weight=-1.0), "contact_weight must be finite and not negative"),
        (dict(contact_weight=math.nan), "contact_weight must be finite and not negative"),
        (dict(contact_weight=None), "contact_weight must be a number"),
        (dict(contact_eps=-1e-3), "contact_eps must be finite and not negative"),
        (dict(contact_eps=math.inf), "contact_eps must be finite and not negative"),
        (dict(background=math.nan), "background must be finite"),
        (dict(background=-math.inf), "background must be finite"),
        (dict(background="zero"), "background must be a number"),
        (dict(grad_weight=-0.5, grad_scales=1), "grad_weight must be finite and not negative"),
        (dict(grad_weight=math.inf, grad_scales=1), "grad_weight must be finite and not negative"),
        (dict(grad_kind="huber"), "grad_kind must be one of 'l1', 'l2'"),
        (dict(grad_scales=5), "grad_scales must be a whole number from 0 to 4"),
        (dict(grad_scales=-1), "grad_scales must be a whole number from 0 to 4"),
        (dict(grad_scales=2.0), "grad_scales must be a whole number from 0 to 4"),
        (dict(grad_scales=True), "grad_scales must be a whole number from 0 to 4"),
        (dict(grad_weight=0.5), "grad_weight 0.5 needs grad_scales >= 1"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match="DepthLoss: " + msg):
            DepthLoss(**kw)
    DepthLoss(grad_weight=0.0, grad_scales=2)           # the slope term measured (terms[2]) without being trained on
    DepthLoss(background=-1.0, contact_weight=3)


def test_spec_round_trips_through_a_dict():
    from gelslim_depth_amd.train import DepthLoss, as_depth_loss
    d = DepthLoss()
    assert d.spec() == dict(data="mse", huber_delta=None, contact_weight=0.0, contact_eps=0.0, background=0.0, grad_weight=0.0,
                            grad_kind="l1", grad_scales=0)
    for spec in D.SPECS.values():
        d = DepthLoss(**spec)
        assert d.spec() == spec and DepthLoss(**d.spec()) == d and hash(DepthLoss(**d.spec())) == hash(d)
        assert as_depth_loss(spec) == d and as_depth_loss(d) is d
        assert all(v is None or type(v) in (str, float, int) for v in d.spec().values())
        assert "grad_scales=%d" % spec["grad_scales"] in repr(d)
    assert DepthLoss(**D.SPEC_FULL) != DepthLoss(**dict(D.SPEC_FULL, grad_weight=0.25))
    c = DepthLoss(**D.SPEC_FULL).c_struct()
    assert (c.data_kind, c.grad_kind, c.grad_scales, c.reserved) == (2, 0, 4, 0)
    assert (c.huber_delta, c.contact_weight, c.grad_weight) == (D.f32(0.05), 4.0, 0.5)
    assert DepthLoss().c_struct().huber_delta == 0.0


def test_train_step_refuses_a_loss_that_is_neither():
    from gelslim_depth_amd.train import TrainStep
    with pytest.raises(ValueError, match="loss must be 'mse', 'l1' or a DepthLoss, got dict"):
        TrainStep(None, loss=dict(D.SPEC_FULL))
    with pytest.raises(ValueError, match="loss must be 'mse', 'l1' or a DepthLoss, got 'huber'"):
        TrainStep(None, loss="huber")


def test_gsd_depth_loss_layout():
    from gelslim_depth_amd import _lib
    s = _lib.gsd_depth_loss
    assert ctypes.sizeof(s) == 4 * 4 + 5 * 4
    assert s.data_kind.offset == 0 and s.reserved.offset == 12
    assert s.huber_delta.offset == 16 and s.grad_weight.offset == 32
    assert _lib.lib.gsd_depth_loss_workspace(2, 1, 9, 11) == 5 and _lib.lib.gsd_depth_loss_workspace(0, 1, 9, 11) == 0
    assert _lib.lib.gsd_depth_loss_workspace(32, 1, 320, 427) == 5 * 1024
