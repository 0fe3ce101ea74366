"""The per-image table of gsd_depth_metrics (include/gsd.h), in torch fp64 on the CPU: the reference the tests hold the kernel
to.

What decides anything is formed in fp32 exactly as the kernel forms it -- e = o - t, the pair differences of column 11, and
|v - background| of both contact tests and both peaks; fp32 subtraction is correctly rounded, so the reference takes the
kernel's side of every contact decision and finds the same fp32 maxima, and no element has to be left out of a comparison.
The spec's floats are rounded to fp32 first (the C struct holds floats).  Everything else is fp64: |e|, e^2 and the pair
magnitudes are widened exactly and summed in fp64.  A maximum starts from 0 and is never won by a NaN, as in the kernel.

`make_case` builds the inputs the tests share."""
import math

import torch

COLS = 16
SPEC = dict(background=0.0, contact_eps=1e-3)


def f32(v) -> torch.Tensor:
    return torch.tensor(float(v), dtype=torch.float32)


def _max_ignoring_nan(v: torch.Tensor) -> torch.Tensor:
    """Per image: max(0, the largest non-NaN value), what `m = v > m ? v : m` from m = 0 leaves."""
    v = torch.where(torch.isnan(v), torch.zeros_like(v), v)
    return v.reshape(v.shape[0], -1).max(dim=1).values.clamp_min(0.0).double()


def depth_metrics_ref(o: torch.Tensor, t: torch.Tensor, background: float = 0.0, contact_eps: float = 1e-3) -> torch.Tensor:
    """(N, 16) float64 table of fp32 (N, K, H, W) tensors `o`, `t` (moved to the CPU)."""
    o, t = o.detach().cpu().float(), t.detach().cpu().float()
    assert o.dim() == 4 and o.shape == t.shape
    n = o.shape[0]
    bg, eps = f32(background), f32(contact_eps)
    e = o - t                                              # fp32
    dt, dp = (t - bg).abs(), (o - bg).abs()                # fp32
    ct, cp = dt > eps, dp > eps
    ed = e.double()
    ae, sq = ed.abs(), ed * ed
    zero = torch.zeros((), dtype=torch.float64)

    def per_image(v):
        return v.reshape(n, -1).sum(dim=1)
    tab = torch.zeros((n, COLS), dtype=torch.float64)
    tab[:, 0] = per_image(ed)
    tab[:, 1] = per_image(ae)
    tab[:, 2] = per_image(sq)
    tab[:, 3] = _max_ignoring_nan(e.abs())
    tab[:, 4] = per_image(ct.double())
    tab[:, 5] = per_image(cp.double())
    tab[:, 6] = per_image((ct & cp).double())
    tab[:, 7] = per_image(torch.where(ct, ae, zero))       # a select, not a product: a NaN outside the patch stays outside
    tab[:, 8] = per_image(torch.where(ct, sq, zero))
    tab[:, 9] = _max_ignoring_nan(dt)
    tab[:, 10] = _max_ignoring_nan(dp)
    gx = (e[..., :, 1:] - e[..., :, :-1]).double().abs()   # fp32 differences, widened
    gy = (e[..., 1:, :] - e[..., :-1, :]).double().abs()
    tab[:, 11] = per_image(gx) + per_image(gy)
    tab[:, 12] = per_image((~torch.isfinite(e)).double())
    return tab


def next_beyond(v: float, away_from: float) -> float:
    """The fp32 neighbour of `v` on the side away from `away_from`."""
    x = f32(v)
    return float(torch.nextafter(x, f32(math.inf if v > away_from else -math.inf)))


def make_case(shape, seed: int = 0, background: float = 0.0, contact_eps: float = 1e-3):
    """(o, t) fp32 on the CPU.  Every image's target is the background with a paraboloid disc pressed into it, down to -0.9 at
    its centre (centre and radius differ per image and class); image 1, where there is one, has no contact at all.
    o = t + 0.03 * N(0,1): the predicted and the true patch overlap without coinciding.  A few target elements sit exactly at
    background +- contact_eps (not contact: the test is strict) and a few at the next fp32 value beyond (contact)."""
    n, k, h, w = shape
    g = torch.Generator().manual_seed(seed)
    ys = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
    xs = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w)
    cy = (0.25 + 0.5 * torch.rand((n, k, 1, 1), generator=g)) * max(h - 1, 1)
    cx = (0.25 + 0.5 * torch.rand((n, k, 1, 1), generator=g)) * max(w - 1, 1)
    r = (0.2 + 0.15 * torch.rand((n, k, 1, 1), generator=g)) * max(min(h, w), 2)
    d2 = ((ys - cy) ** 2 + (xs - cx) ** 2) / (r * r)
    t = torch.where(d2 < 1.0, -0.9 * (1.0 - d2), torch.zeros(())) + float(background)
    t = t.float().contiguous()
    if n >= 2:
        t[1] = float(background)
    bg, eps = float(f32(background)), float(f32(contact_eps))
    edge = [float(f32(bg) + f32(eps)), float(f32(bg) - f32(eps))]
    edge += [next_beyond(edge[0], bg), next_beyond(edge[1], bg)]
    m = k * h * w
    if m >= 16:
        for img in (i for i in range(n) if i != 1):        # image 1 keeps its bare background
            flat = t[img].view(-1)
            for i, idx in enumerate(torch.randperm(m, generator=g)[:8].tolist()):
                flat[idx] = edge[i % 4]
    o = (t + 0.03 * torch.randn(t.shape, generator=g)).float().contiguous()
    return o, t
