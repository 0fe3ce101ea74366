"""The depth-aware loss of gsd_depth_loss_fwd_bwd (include/gsd.h), in torch fp64 on the CPU: the reference the tests hold
the kernel to.

What decides a branch is formed in fp32 exactly as the kernel forms it -- e = o - t, the pair differences of the slope term and
the contact test |t - background| > contact_eps; fp32 subtraction is correctly rounded, so the reference takes the kernel's
side of every |e| <= delta, every sign and every contact decision, and no element has to be left out of a comparison.  The
spec's float fields are rounded to fp32 first (the C struct holds floats).  Everything else is fp64.

`depth_loss_ref` returns the six terms, the gradient in gather form, and A, the per-element sum of the absolute values of the
gradient's summands (the scale of its rounding error).  `depth_loss_autograd` is the same loss written straight from the
formula for torch autograd; `make_case` builds the inputs the tests share."""
import torch

DATA_KINDS = {"mse": 0, "l1": 1, "huber": 2}
GRAD_KINDS = {"l1": 0, "l2": 1}

# the specs the tests cross with the shapes (plain dicts, DepthLoss(**spec).spec() == spec)
SPEC_FULL = dict(data="huber", huber_delta=0.05, contact_weight=4.0, contact_eps=1e-3, background=0.0, grad_weight=0.5,
                 grad_kind="l1", grad_scales=4)
SPEC_MSE_L2 = dict(data="mse", huber_delta=None, contact_weight=0.0, contact_eps=0.0, background=0.0, grad_weight=0.25,
                   grad_kind="l2", grad_scales=3)
SPEC_L1_CONTACT = dict(data="l1", huber_delta=None, contact_weight=2.0, contact_eps=1e-3, background=0.0, grad_weight=0.0,
                       grad_kind="l1", grad_scales=0)
SPEC_UNWEIGHTED_SLOPE = dict(data="mse", huber_delta=None, contact_weight=0.0, contact_eps=0.0, background=0.0, grad_weight=0.0,
                             grad_kind="l1", grad_scales=2)
SPECS = {"huber_contact_l1x4": SPEC_FULL, "mse_l2x3": SPEC_MSE_L2, "l1_contact": SPEC_L1_CONTACT,
         "slope_weight0_x2": SPEC_UNWEIGHTED_SLOPE}

SHAPES = [(2, 1, 9, 11), (3, 2, 17, 23), (1, 1, 5, 37), (1, 1, 1, 1), (2, 1, 8, 16)]


def f32(v) -> float:
    """v rounded to fp32, as a Python float."""
    return float(torch.tensor(0.0 if v is None else float(v), dtype=torch.float32))


def make_case(shape, seed: int = 0, quantum: float = 0.0):
    """(o, t) fp32 on the CPU: targets -0.9 * U[0,1) on about 30 % of the pixels and exactly 0 elsewhere, o = t + 0.1 * N(0,1).
    With `quantum` both are rounded to multiples of it (a power of two: every difference is then exact in fp32 and fp64 alike)."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(shape, generator=g) < 0.3
    t = torch.where(mask, -0.9 * torch.rand(shape, generator=g), torch.zeros(shape))
    o = t + 0.1 * torch.randn(shape, generator=g)
    if quantum:
        t, o = torch.round(t / quantum) * quantum, torch.round(o / quantum) * quantum
    return o.float().contiguous(), t.float().contiguous()


def _phi(g, kind):
    return g.abs() if kind == "l1" else g * g


def _dphi(g, kind):
    return torch.sign(g) if kind == "l1" else 2.0 * g


def depth_loss_ref(o: torch.Tensor, t: torch.Tensor, spec: dict, grad_scale: float = 1.0):
    """terms (6 float64), grad (float64, shape of o), A (float64, shape of o; grad_scale not applied)."""
    o32, t32 = o.detach().cpu().float(), t.detach().cpu().float()
    assert o32.dim() == 4 and o32.shape == t32.shape
    M = o32.numel()
    delta, cw, ceps = f32(spec["huber_delta"]), f32(spec["contact_weight"]), f32(spec["contact_eps"])
    bg, gw = f32(spec["background"]), f32(spec["grad_weight"])
    e32 = o32 - t32
    e = e32.double()
    contact = (t32 - torch.tensor(bg, dtype=torch.float32)).abs() > torch.tensor(ceps, dtype=torch.float32)
    w = 1.0 + cw * contact.double()
    if spec["data"] == "mse":
        rho, drho = e * e, 2.0 * e
    elif spec["data"] == "l1":
        rho, drho = e.abs(), torch.sign(e)
    else:
        small = e32.abs() <= torch.tensor(delta, dtype=torch.float32)
        rho = torch.where(small, 0.5 * e * e, delta * (e.abs() - 0.5 * delta))
        drho = torch.where(small, e, delta * torch.sign(e))
    l_data = (w * rho).sum() / M
    grad = w * drho / M
    A = grad.abs()
    l_grad = torch.zeros((), dtype=torch.float64)
    for k in range(int(spec["grad_scales"])):
        s = 1 << k
        sub = e32[:, :, ::s, ::s]                                   # the grid of this scale
        Mk = sub.numel()
        dh = (sub[..., :, 1:] - sub[..., :, :-1]).double()          # e[h, w+s] - e[h, w], formed in fp32
        dv = (sub[..., 1:, :] - sub[..., :-1, :]).double()          # e[h+s, w] - e[h, w]
        l_grad = l_grad + (_phi(dh, spec["grad_kind"]).sum() + _phi(dv, spec["grad_kind"]).sum()) / Mk
        ph, pv = _dphi(dh, spec["grad_kind"]), _dphi(dv, spec["grad_kind"])
        gs = torch.zeros(sub.shape, dtype=torch.float64)
        As = torch.zeros(sub.shape, dtype=torch.float64)
        gs[..., :, 1:] += ph                                        # the pixel is the right end of its left pair
        gs[..., :, :-1] -= ph                                       # ... the left end of its right pair
        gs[..., 1:, :] += pv
        gs[..., :-1, :] -= pv
        As[..., :, 1:] += ph.abs()
        As[..., :, :-1] += ph.abs()
        As[..., 1:, :] += pv.abs()
        As[..., :-1, :] += pv.abs()
        grad[:, :, ::s, ::s] += (gw / Mk) * gs
        A[:, :, ::s, ::s] += (gw / Mk) * As
    terms = torch.stack([l_data + gw * l_grad, l_data, l_grad, (e * e).sum() / M, e.abs().sum() / M,
                         contact.double().sum() / M])
    return terms, grad * float(grad_scale), A


def depth_loss_autograd(o: torch.Tensor, t: torch.Tensor, spec: dict) -> torch.Tensor:
    """L as a differentiable fp64 scalar, written pair by pair from the definition (o: float64, requires_grad).  On inputs whose
    differences are exact in fp32 (make_case with a quantum) it takes the branches depth_loss_ref takes."""
    delta, cw, ceps = f32(spec["huber_delta"]), f32(spec["contact_weight"]), f32(spec["contact_eps"])
    bg, gw = f32(spec["background"]), f32(spec["grad_weight"])
    t = t.double()
    e = o - t
    N, K, H, W = e.shape
    w = 1.0 + cw * ((t - bg).abs() > ceps).double()
    if spec["data"] == "mse":
        rho = e ** 2
    elif spec["data"] == "l1":
        rho = e.abs()
    else:
        rho = torch.where(e.abs() <= delta, 0.5 * e ** 2, delta * (e.abs() - 0.5 * delta))
    loss = (w * rho).sum() / e.numel()
    for k in range(int(spec["grad_scales"])):
        s = 1 << k
        Mk = N * K * (-(-H // s)) * (-(-W // s))
        hs, ws = torch.arange(0, H, s), torch.arange(0, W, s)
        right = e[:, :, hs][:, :, :, ws[ws + s < W] + s] - e[:, :, hs][:, :, :, ws[ws + s < W]]
        down = e[:, :, hs[hs + s < H] + s][:, :, :, ws] - e[:, :, hs[hs + s < H]][:, :, :, ws]
        loss = loss + gw * (_phi(right, spec["grad_kind"]).sum() + _phi(down, spec["grad_kind"]).sum()) / Mk
    return loss
