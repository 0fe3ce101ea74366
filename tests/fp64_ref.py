"""fp64 references of the fp32 engine's contractions, with a per-element condition tensor, and the bound check the fp32 kernel
tests hold them to.  A helper module (imported by tests/test_fp64_ref_cpu.py and tests/test_gpu_fp64_bounds.py), not collected.

Every reference is plain torch float64 arithmetic on whatever device its operands live on: a 3x3 convolution is nine shifted-tap
matmuls over a zero-padded copy, a 2x2/s2 transposed convolution four matmuls into the strided output planes.  No F.conv2d (which
backend it takes for double on the GPU is not ours to choose) and nothing from libgsd.  The operands are the exact fp32 values
the kernel reads, widened to fp64 (deferred_act / bnrelu_mask reproduce the kernels' fp32 `fmaf(raw, scale, shift)`).

Each reference returns (ref, cond): cond is the same contraction over absolute values, sum |a||b| per output element.  Any fp32
evaluation of the contraction -- whatever its summation order, tiling, Winograd transform or split-K -- lands within a modest
multiple of 2^-24 * cond of ref, while cond is small exactly where a wrong read shows most: at image borders the zero padding
removes a third of the products from cond, so a halo that reads garbage instead of zeros fails there by orders of magnitude.

check_bound(got, ref, cond, tau) asserts |got - ref| <= tau * cond at every element, and finite outputs everywhere (the tests
NaN-fill outputs before the launch, so an element nobody wrote fails).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

# ---- tolerances: |got - ref| <= TAU * cond, per kernel family.  Each sits at no more than 4x the largest ratio |got-ref|/cond
# measured on the MI355X over tests/test_gpu_fp64_bounds.py (case named beside it).  Forward / dX taus must also stay below
# ceiling(Cin) = 0.1 / (9 Cin): a tenth of the average share of ONE product in cond at the deepest contraction (Cin = 1024).
TAU_WINO = 6.0e-6      # conv3x3 forward / dX, Winograd F(4,3) rows and F(2x4,3x3): 1.52e-6 (up3.c0 dX, N = 32, F(4,3) rows forced)
TAU_DIRECT = 1.6e-6    # conv3x3 forward, direct taps (the first layer): 4.10e-7 (inc.c0 forward, N = 32, train)
TAU_DW = 4.0e-6        # conv3x3 dW (split-K reductions over N*H*W pixels): 1.03e-6 (down3.c1, N = 32)
TAU_CONVT = 1.9e-6     # ConvTranspose2d 2x2/s2 forward, dX, dW, db: 4.80e-7 (up2.up, N = 32)
TAU_1X1 = 8.0e-7       # output 1x1 conv forward / dX / dW / db, MSE loss and gradient: 2.16e-7 (outc forward, N = 32)
TAU_STATS = 3.4e-8     # per-channel sums of a launch's statistics epilogue (vs sum of ref, over sum of cond): 8.51e-9 (inc.c1, N = 8)

# worst |got-ref|/cond seen per key (check_bound(..., key=...)): the GPU module reports them
RATIOS: Dict[str, float] = {}


def ceiling(cin: int) -> float:
    """Largest admissible forward / dX tau for a contraction over `cin` input channels x 9 taps."""
    return 0.1 / (9 * cin)


# ------------------------------------------------------------------------------------------------------------------ operands
def deferred_act(raw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """max(fmaf(raw, scale, shift), 0) as the fp32 kernels load a deferred BatchNorm+ReLU source, widened to fp64.  The fp64
    product of two fp32 values is exact, so this differs from a true fmaf only by a double rounding (at most one fp32 ulp of
    the operand, in rare elements) -- far below every tau."""
    c = (1, -1, 1, 1)
    y = raw.double() * scale.double().view(c) + shift.double().view(c)
    return y.float().double().clamp_min_(0.0)


def bnrelu_mask(raw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """The fused BatchNorm-backward epilogues' mask `fmaf(raw, scale, shift) > 0.f`, exactly: the fp64 product is exact and one
    fp64 rounding of the sum cannot change its sign, the same holds for fmaf's single fp32 rounding."""
    c = (1, -1, 1, 1)
    return (raw.double() * scale.double().view(c) + shift.double().view(c)) > 0


def decoder_src(a0: torch.Tensor, up: torch.Tensor, h: int, w: int) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """cat[skip, F.pad(up)] of a decoder's first conv (unet.py: F.pad(x1, [dX//2, dX-dX//2, dY//2, dY-dY//2])) and the pad
    offset (top, left) the kernels take as the second segment's `off`."""
    uh, uw = up.shape[2], up.shape[3]
    top, left = (h - uh) // 2, (w - uw) // 2
    upp = F.pad(up, [left, w - uw - left, top, h - uh - top])
    return torch.cat([a0, upp], 1), (top, left)


# -------------------------------------------------------------------------------------------------------------- conv3x3
def _taps(x: torch.Tensor, h: int, w: int):
    """(kh, kw, view) of the zero-padded x shifted by every tap, each view flattened to (n, c, h*w)."""
    xp = F.pad(x, [1, 1, 1, 1])
    for kh in range(3):
        for kw in range(3):
            yield kh, kw, xp[:, :, kh:kh + h, kw:kw + w].reshape(x.shape[0], x.shape[1], h * w)


def conv3x3_fwd(a: torch.Tensor, wt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """y[n,co,y,x] = sum_{ci,kh,kw} wt[co,ci,kh,kw] a[n,ci,y+kh-1,x+kw-1] (zero padding 1).  a: (n,ci,h,w), wt: (co,ci,3,3)."""
    n, _, h, w = a.shape
    co = wt.shape[0]
    ref = torch.zeros((n, co, h * w), dtype=torch.float64, device=a.device)
    cond = torch.zeros_like(ref)
    wa = wt.abs()
    for (kh, kw, s), (_, _, sa) in zip(_taps(a, h, w), _taps(a.abs(), h, w)):
        ref += torch.matmul(wt[:, :, kh, kw], s)
        cond += torch.matmul(wa[:, :, kh, kw], sa)
    return ref.view(n, co, h, w), cond.view(n, co, h, w)


def conv3x3_dx(dy: torch.Tensor, wt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """dx[n,ci,y,x] = sum_{co,kh,kw} wt[co,ci,kh,kw] dy[n,co,y-kh+1,x-kw+1].  dy: (n,co,h,w)."""
    n, _, h, w = dy.shape
    ci = wt.shape[1]
    ref = torch.zeros((n, ci, h * w), dtype=torch.float64, device=dy.device)
    cond = torch.zeros_like(ref)
    wtt = wt.transpose(0, 1)
    wta = wtt.abs()
    for (kh, kw, s), (_, _, sa) in zip(_taps(dy, h, w), _taps(dy.abs(), h, w)):
        # tap (kh, kw) of the padded dy is dy[y + kh - 1]: it meets weight (2 - kh, 2 - kw)
        ref += torch.matmul(wtt[:, :, 2 - kh, 2 - kw], s)
        cond += torch.matmul(wta[:, :, 2 - kh, 2 - kw], sa)
    return ref.view(n, ci, h, w), cond.view(n, ci, h, w)


def conv3x3_dw(a: torch.Tensor, dy: torch.Tensor, dy_abs: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """dW[co,ci,kh,kw] = sum_{n,y,x} dy[n,co,y,x] a[n,ci,y+kh-1,x+kw-1].  dy_abs: the bound on |dy| to use in cond (default
    |dy|; a kernel that forms dy itself in fp32 from several terms passes the sum of their magnitudes)."""
    n, ci, h, w = a.shape
    co = dy.shape[1]
    d = dy.reshape(n, co, h * w)
    da = (dy.abs() if dy_abs is None else dy_abs).reshape(n, co, h * w)
    ref = torch.zeros((co, ci, 3, 3), dtype=torch.float64, device=a.device)
    cond = torch.zeros_like(ref)
    for (kh, kw, s), (_, _, sa) in zip(_taps(a, h, w), _taps(a.abs(), h, w)):
        ref[:, :, kh, kw] = torch.matmul(d, s.transpose(1, 2)).sum(0)
        cond[:, :, kh, kw] = torch.matmul(da, sa.transpose(1, 2)).sum(0)
    return ref, cond


def conv3x3_dw_rows(a: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """The contribution of every output row of ONE image to dW: (h, co, ci, 3, 3), summing to conv3x3_dw's ref.  a: (1,ci,h,w)."""
    _, ci, h, w = a.shape
    co = dy.shape[1]
    d = dy[0].transpose(0, 1)                   # (h, co, w)
    ap = F.pad(a, [1, 1, 1, 1])[0]              # (ci, h+2, w+2)
    out = torch.empty((h, co, ci, 3, 3), dtype=torch.float64, device=a.device)
    for kh in range(3):
        for kw in range(3):
            s = ap[:, kh:kh + h, kw:kw + w].transpose(0, 1)     # (h, ci, w)
            out[:, :, :, kh, kw] = torch.matmul(d, s.transpose(1, 2))
    return out


# ------------------------------------------------------------------------------------------- ConvTranspose2d(k=2, s=2)
def convT_fwd(x: torch.Tensor, wt: torch.Tensor, b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """y[n,co,2i+di,2j+dj] = b[co] + sum_ci wt[ci,co,di,dj] x[n,ci,i,j].  x: (n,ci,h,w), wt: (ci,co,2,2)."""
    n, ci, h, w = x.shape
    co = wt.shape[1]
    ref = torch.empty((n, co, 2 * h, 2 * w), dtype=torch.float64, device=x.device)
    cond = torch.empty_like(ref)
    xf, xa = x.reshape(n, ci, h * w), x.abs().reshape(n, ci, h * w)
    for di in range(2):
        for dj in range(2):
            t = wt[:, :, di, dj].transpose(0, 1)
            ref[:, :, di::2, dj::2] = (torch.matmul(t, xf) + b.view(1, co, 1)).view(n, co, h, w)
            cond[:, :, di::2, dj::2] = (torch.matmul(t.abs(), xa) + b.abs().view(1, co, 1)).view(n, co, h, w)
    return ref, cond


def convT_dx(dy: torch.Tensor, wt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """dx[n,ci,i,j] = sum_{co,di,dj} wt[ci,co,di,dj] dy[n,co,2i+di,2j+dj].  dy: (n,co,2h,2w)."""
    n, co, h2, w2 = dy.shape
    h, w = h2 // 2, w2 // 2
    ci = wt.shape[0]
    ref = torch.zeros((n, ci, h * w), dtype=torch.float64, device=dy.device)
    cond = torch.zeros_like(ref)
    for di in range(2):
        for dj in range(2):
            s = dy[:, :, di::2, dj::2].reshape(n, co, h * w)
            ref += torch.matmul(wt[:, :, di, dj], s)
            cond += torch.matmul(wt[:, :, di, dj].abs(), s.abs())
    return ref.view(n, ci, h, w), cond.view(n, ci, h, w)


def convT_dw(x: torch.Tensor, dy: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dW, cond of dW, db, cond of db): dW[ci,co,di,dj] = sum x[n,ci,i,j] dy[n,co,2i+di,2j+dj], db[co] = sum dy[n,co,.,.]."""
    n, ci, h, w = x.shape
    co = dy.shape[1]
    xf, xa = x.reshape(n, ci, h * w), x.abs().reshape(n, ci, h * w)
    dw = torch.empty((ci, co, 2, 2), dtype=torch.float64, device=x.device)
    cw = torch.empty_like(dw)
    for di in range(2):
        for dj in range(2):
            s = dy[:, :, di::2, dj::2].reshape(n, co, h * w)
            dw[:, :, di, dj] = torch.matmul(xf, s.transpose(1, 2)).sum(0)
            cw[:, :, di, dj] = torch.matmul(xa, s.abs().transpose(1, 2)).sum(0)
    return dw, cw, dy.sum(dim=(0, 2, 3)), dy.abs().sum(dim=(0, 2, 3))


# ------------------------------------------------------------------------------------------------ output 1x1 conv + loss
def conv1x1_fwd(a: torch.Tensor, wt: torch.Tensor, b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """out[n,k,p] = b[k] + sum_c wt[k,c] a[n,c,p].  a: (n,c,h,w), wt: (k,c)."""
    n, c, h, w = a.shape
    k = wt.shape[0]
    ref = torch.matmul(wt, a.reshape(n, c, h * w)) + b.view(1, k, 1)
    cond = torch.matmul(wt.abs(), a.abs().reshape(n, c, h * w)) + b.abs().view(1, k, 1)
    return ref.view(n, k, h, w), cond.view(n, k, h, w)


def conv1x1_dx(g: torch.Tensor, wt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """dx[n,c,p] = sum_k wt[k,c] g[n,k,p].  g: (n,k,h,w)."""
    n, k, h, w = g.shape
    c = wt.shape[1]
    ref = torch.matmul(wt.t(), g.reshape(n, k, h * w))
    cond = torch.matmul(wt.abs().t(), g.abs().reshape(n, k, h * w))
    return ref.view(n, c, h, w), cond.view(n, c, h, w)


def conv1x1_dw(a: torch.Tensor, g: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dW, cond, db, cond): dW[k,c] = sum_{n,p} g[n,k,p] a[n,c,p], db[k] = sum g[n,k,p]."""
    n, c, h, w = a.shape
    k = g.shape[1]
    gf, af = g.reshape(n, k, h * w), a.reshape(n, c, h * w)
    dw = torch.matmul(gf, af.transpose(1, 2)).sum(0)
    cw = torch.matmul(gf.abs(), af.abs().transpose(1, 2)).sum(0)
    return dw, cw, g.sum(dim=(0, 2, 3)), g.abs().sum(dim=(0, 2, 3))


def mse_grad(o: torch.Tensor, t: torch.Tensor, numel: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """d mean((o-t)^2) / d o = 2 (o - t) / numel."""
    s = 2.0 / numel
    return (o.double() - t.double()) * s, (o.double().abs() + t.double().abs()) * s


# ------------------------------------------------------------------------------------------------------------ the check
def _pos(flat: int, shape: Sequence[int]) -> Tuple[int, ...]:
    out = []
    for d in reversed(shape):
        out.append(flat % d)
        flat //= d
    return tuple(reversed(out))


def check_bound(got: torch.Tensor, ref: torch.Tensor, cond: torch.Tensor, tau: float, what: str, n0: int = 0,
                image: Optional[int] = None, key: Optional[str] = None, weights: bool = False) -> float:
    """Assert |got - ref| <= tau * cond and isfinite(got) at every element; return the worst ratio |got - ref| / cond.

    got / ref / cond: same shape (n, c, h, w) for activations -- (co, ci, kh, kw) or any shape for weights; n0: index of
    got's first image in the batch (for the report); image: an image whose share of the failures is reported; key: record the
    worst ratio in RATIOS[key]; weights: got is not an activation (no image / tile report).  On failure the message gives the
    worst ratio and its position, the fraction of elements over the bound and, for 4-d activations, how many of those lie on
    an image edge, a tile edge (columns 0 / 3 mod 4, even rows) or in `image`, and the images that hold them."""
    assert got.shape == ref.shape == cond.shape, (what, tuple(got.shape), tuple(ref.shape), tuple(cond.shape))
    g = got.double()
    fin = torch.isfinite(g)
    if not bool(fin.all()):
        bad = (~fin).reshape(-1)
        first = int(bad.nonzero()[0, 0])
        p = _pos(first, got.shape)
        if got.dim() == 4 and not weights:
            p = (p[0] + n0,) + p[1:]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements not finite (unwritten?), first at {p}")
    err = (g - ref).abs()
    ratio = torch.where(cond > 0, err / cond.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst_flat = int(ratio.reshape(-1).argmax())
    worst = float(ratio.reshape(-1)[worst_flat])
    if key is not None:
        RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    over = err > tau * cond
    if not bool(over.any()):
        return worst
    p = _pos(worst_flat, got.shape)
    act = got.dim() == 4 and not weights
    nover = int(over.sum())
    msg = [f"{what}: |got-ref| > {tau:.3g}*cond at {nover} of {over.numel()} elements ({nover / over.numel():.3g}); "
           f"worst ratio {worst:.3g} at {(p[0] + n0,) + p[1:] if act else p}"]
    if act:
        idx = over.nonzero()
        hh, ww = got.shape[2], got.shape[3]
        r, c = idx[:, 2], idx[:, 3]
        edge = (r == 0) | (r == hh - 1) | (c == 0) | (c == ww - 1)
        msg.append(f"image edge {int(edge.sum())}, tile column edge (0 or 3 mod 4) {int(((c % 4 == 0) | (c % 4 == 3)).sum())}, "
                   f"even row {int((r % 2 == 0).sum())}")
        imgs, cnt = torch.unique(idx[:, 0] + n0, return_counts=True)
        top = sorted(zip(cnt.tolist(), imgs.tolist()), reverse=True)[:6]
        msg.append("images (count, n): " + ", ".join(f"({k}, {i})" for k, i in top) + f" of {len(imgs)}")
        if image is not None:
            msg.append(f"in image {image}: {int((idx[:, 0] + n0 == image).sum())}")
        chans = torch.unique(idx[:, 1])
        msg.append(f"channels {chans[:8].tolist()}{' ...' if len(chans) > 8 else ''} ({len(chans)} in all)")
    raise AssertionError("; ".join(msg))


def check_sums(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, tau: float, what: str, key: Optional[str] = None) -> float:
    """Per-channel sums of a launch's statistics epilogue: |got - ref| <= tau * bound (bound: the sum of the per-element cond,
    or of cond^2 for second moments)."""
    return check_bound(got, ref, bound, tau, what, key=key, weights=True)
