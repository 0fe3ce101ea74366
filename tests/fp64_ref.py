"""fp64 references of the fp32 engine's contractions, with a per-element condition tensor, and the bound check the fp32 kernel
tests hold them to.  A helper module (imported by tests/test_fp64_ref_cpu.py and the GPU bound modules), not collected.

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

The bf16 engine (tests/test_gpu_bf16_fp64_bounds.py) stores its results in bf16: check_bound_bf16 allows the RNE rounding of
the result, 2^-8 |ref|, on top of tau * cond; the references of its bf16-only operations (first layer from fp32 x, BatchNorm
apply, max-pool routing, BatchNorm backward, statistics of the stored values) sit at the end of this module.
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
# fp32 pointwise kernels and the optimiser (tests/test_gpu_fp32_pointwise_fp64.py, tests/test_gpu_fp32_step_fp64.py), same rule
TAU_PW = 7.8e-7        # gsd_bn_bwd_apply (in place / pitched), gsd_bn_eval_coeffs[_bwd]: 1.95e-7 (apply, level 2, 16-byte form, N = 32)
TAU_ADAM = 2.3e-7      # gsd_adam_ema, cond of adam_ema_ref (p, m, v, ema): 5.93e-8 (arena of 31 M, step 1, wd 0.1, grad_scale 1/2)
U32 = 2.0 ** -24       # unit roundoff of round-to-nearest fp32: one fp32 rounding of an fp64 value x costs at most U32 |x|

# bf16 engine (tests/test_gpu_bf16_fp64_bounds.py, check_bound_bf16): |got - ref| <= 2^-8 |ref| + TAU * cond.  2^-8 is the unit
# roundoff of the RNE rounding of a stored bf16 result; TAU holds the fp32 accumulation in front of it.  Same rule: each at no
# more than 4x the largest ratio measured on the MI355X (case named beside it); forward / dX taus also below ceiling(Cin).
TAU_BF16_CONV = 2.1e-7     # conv3x3 / c64 / inc_conv forward, dX (plain or with fused BatchNorm-backward pass 1): 5.48e-8 (down2.c1 forward, N = 16)
TAU_BF16_FIRST = 6.4e-8    # conv3x3_first (27 products from fp32 x), with or without BatchNorm+ReLU: 1.81e-8 (inc y0 in the engine step, N = 16)
TAU_BF16_DW = 1.1e-6       # conv3x3 / first-layer / ConvT 4-tap dW (fp32 result, check_bound): 2.79e-7 (inc wgrad_first_recompute, N = 16)
TAU_BF16_CONVT = 1.7e-7    # ConvT forward scattered into the concat buffer, dX, bias gradient: 4.29e-8 (up0.up, N = 7)
TAU_BF16_PW = 5.6e-7       # BatchNorm apply, backward reduce (dz) and apply, 1x1 output conv and its gradients: 1.42e-7 (engine step, N = 16)
TAU_BF16_STATS = 4.2e-6    # per-channel sums of a bf16 statistics epilogue, of the values as stored (each block lane sums its pixels
#                            serially in fp32): 1.05e-6 (up3.c0 dX sum of squares over the concat gradient, N = 32)
U_BF16 = 2.0 ** -8         # unit roundoff of round-to-nearest-even to 8 significant bits (f32_to_bf16 in gsd_bf16_common.h)

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


def fmaf32(x: torch.Tensor, s: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fp32 fmaf(x, s, b) exactly, for fp32-valued operands, as an fp64 tensor.  The product of two fp32 values is exact in fp64;
    TwoSum gives the fp64 sum t and its error e (x*s + b == t + e exactly).  Rounding t to fp32 is then right except when t lies
    exactly on an fp32 midpoint and e != 0: the tie belongs to the side e points to (a double rounding deferred_act accepts)."""
    x, s, b = x.double(), s.double(), b.double()
    p = x * s
    t = p + b
    bb = t - p
    e = (p - (t - bb)) + (b - bb)
    r = t.float()
    rd = r.double()
    up = torch.nextafter(r, torch.full_like(r, math.inf))
    dn = torch.nextafter(r, torch.full_like(r, -math.inf))
    other = torch.where(t > rd, up, dn)
    mid = (2.0 * t == rd + other.double()) & (t != rd)
    fix = mid & (((t > rd) & (e > 0)) | ((t < rd) & (e < 0)))
    return torch.where(fix, other, r).double()


def bnrelu_act(raw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """max(fmaf(raw, scale, shift), 0) bit for bit (fmaf32): the activation gsd_maxpool2 pools and the pool-routed BatchNorm
    backward takes its arg-max of.  Selections and single roundings are compared with torch.equal, so deferred_act's rare
    one-ulp double rounding is not good enough there."""
    c = (1, -1, 1, 1)
    return fmaf32(raw, scale.view(c), shift.view(c)).clamp_min_(0.0)


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


def conv3x3_dx(dy: torch.Tensor, wt: torch.Tensor, dy_abs: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """dx[n,ci,y,x] = sum_{co,kh,kw} wt[co,ci,kh,kw] dy[n,co,y-kh+1,x-kw+1].  dy: (n,co,h,w); dy_abs: the bound on |dy| to use
    in cond (default |dy|), as conv3x3_dw."""
    n, _, h, w = dy.shape
    ci = wt.shape[1]
    ref = torch.zeros((n, ci, h * w), dtype=torch.float64, device=dy.device)
    cond = torch.zeros_like(ref)
    wtt = wt.transpose(0, 1)
    wta = wtt.abs()
    for (kh, kw, s), (_, _, sa) in zip(_taps(dy, h, w), _taps(dy.abs() if dy_abs is None else dy_abs, h, w)):
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
                image: Optional[int] = None, key: Optional[str] = None, weights: bool = False,
                _base: Optional[torch.Tensor] = None) -> float:
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
    if _base is not None:       # check_bound_bf16: the rounding allowance of the stored result comes off before the ratio
        err = (err - _base).clamp_min_(0.0)
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
    lhs = "|got-ref| - 2^-8|ref|" if _base is not None else "|got-ref|"
    msg = [f"{what}: {lhs} > {tau:.3g}*cond at {nover} of {over.numel()} elements ({nover / over.numel():.3g}); "
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


def check_bound_bf16(got: torch.Tensor, ref: torch.Tensor, cond: torch.Tensor, tau: float, what: str, n0: int = 0,
                     image: Optional[int] = None, key: Optional[str] = None, weights: bool = False) -> float:
    """A stored bf16 result: assert |got - ref| <= 2^-8 |ref| + tau * cond and isfinite(got) at every element; return the worst
    ratio (|got - ref| - 2^-8 |ref|)+ / cond.  2^-8 |ref| is what the RNE rounding of the exact result to 8 significant bits may
    cost (half an ulp is 2^-9 of the binade's bottom, i.e. up to 2^-8 relative there); tau * cond holds the fp32 evaluation in
    front of the rounding.  Report and arguments as check_bound."""
    return check_bound(got, ref, cond, tau, what, n0=n0, image=image, key=key, weights=weights,
                       _base=U_BF16 * ref.abs())


# ------------------------------------------------------------------------------------------- bf16 engine: operands, references
def bf16(t: torch.Tensor) -> torch.Tensor:
    """t rounded to bf16 (RNE, as f32_to_bf16) -- via fp32, as every kernel rounds an fp32 value -- widened to fp64."""
    return t.float().to(torch.bfloat16).double()


def nchw(t: torch.Tensor, off: int = 0, c: Optional[int] = None) -> torch.Tensor:
    """Channels [off, off + c) of an NHWC buffer as an (n, c, h, w) fp64 tensor on its device."""
    c = t.shape[3] - off if c is None else c
    return t[..., off:off + c].permute(0, 3, 1, 2).double()


def first_fwd(x: torch.Tensor, wt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The first layer from the fp32 input: the kernels (gsd_bf16_conv3x3_first, gsd_bf16_inc_conv) round x and the weights to
    bf16 themselves, then contract 9 * Cin products in fp32."""
    return conv3x3_fwd(bf16(x), bf16(wt))


def bn_relu_bf16(y: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """BatchNorm apply + ReLU of a stored bf16 raw output as the kernels store it: bf16(max(fmaf(y, scale, shift), 0)).
    Returns (stored, ref, cond): `stored` reproduces the fp32-then-bf16 rounding (the fp64 product of a bf16 and an fp32 value is
    exact; as deferred_act, only a rare double rounding can separate it from a true fmaf) and is the next convolution's operand;
    ref = relu(y*scale + shift) exactly, cond = |y*scale| + |shift| where it is positive (what fmaf's rounding scales with)."""
    c = (1, -1, 1, 1)
    t = y.double() * scale.double().view(c) + shift.double().view(c)
    stored = bf16(t.float().double().clamp_min(0.0))
    pos = t > 0
    cond = torch.where(pos, (y.double() * scale.double().view(c)).abs() + shift.double().abs().view(c), torch.zeros_like(t))
    return stored, t.clamp_min(0.0), cond


def maxpool_route(a: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """2x2/s2 max-pool of the STORED activations (n, c, h, w) and the window position of each maximum, 0..3 in (0,0), (0,1),
    (1,0), (1,1) order, the first maximum winning a tie; an odd last row / column is dropped (floor mode)."""
    hp, wp = a.shape[2] // 2, a.shape[3] // 2
    a = a[:, :, :2 * hp, :2 * wp]
    win = [a[:, :, 0::2, 0::2], a[:, :, 0::2, 1::2], a[:, :, 1::2, 0::2], a[:, :, 1::2, 1::2]]
    best, code = win[0].clone(), torch.zeros(win[0].shape, dtype=torch.int64, device=a.device)
    for q in range(1, 4):
        better = win[q] > best
        code[better] = q
        best = torch.where(better, win[q], best)
    return best, code


def pool_grad(dp: torch.Tensor, code: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """The pooled gradient dp routed to the window position `code` names, zero elsewhere (and in the dropped row / column)."""
    n, c, hp, wp = dp.shape
    out = torch.zeros((n, c, h, w), dtype=torch.float64, device=dp.device)
    for q, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, :, dy:2 * hp:2, dx:2 * wp:2] = torch.where(code == q, dp.double(), torch.zeros((), dtype=torch.float64,
                                                                                               device=dp.device))
    return out


def bn_bwd_dz(y: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, g: torch.Tensor,
              g_abs: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pass 1 of the BatchNorm+ReLU backward, the stored dz: g where fmaf(y, scale, shift) > 0, else 0 (then rounded to bf16).
    g: the gradient w.r.t. the activation in fp64 (a skip gradient plus the routed pooled gradient, the output conv's w * dout,
    or a dX); g_abs: the magnitude its fp32 evaluation in the kernel scales with (default |g|).  Returns (ref, cond)."""
    m = bnrelu_mask(y, scale, shift)
    z = torch.zeros((), dtype=torch.float64, device=g.device)
    return torch.where(m, g.double(), z), torch.where(m, (g.abs() if g_abs is None else g_abs).double(), z)


def bn_bwd_sums(dz: torch.Tensor, y: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Pass 1's per-channel sums over the STORED dz (the kernels sum what they store): (sum dz, sum dz*xhat, sum |dz|,
    sum |dz*xhat|) with xhat = (y - mean) * invstd; the kernels form xhat in fp32 (two roundings, inside the tau)."""
    c = (1, -1, 1, 1)
    xhat = (y.double() - mean.double().view(c)) * invstd.double().view(c)
    p = dz.double() * xhat
    return dz.double().sum((0, 2, 3)), p.sum((0, 2, 3)), dz.double().abs().sum((0, 2, 3)), p.abs().sum((0, 2, 3))


def bn_bwd_apply(dz: torch.Tensor, y: torch.Tensor, scale: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor,
                 c1: torch.Tensor, c2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pass 2: d_raw = scale * (dz - c1 - xhat * c2) (gsd_bf16_bn_bwd_apply; c1 = sum dz / count, c2 = sum dz*xhat / count);
    cond = |scale| (|dz| + |c1| + |xhat * c2|), the magnitude its fp32 evaluation scales with."""
    c = (1, -1, 1, 1)
    xhat = (y.double() - mean.double().view(c)) * invstd.double().view(c)
    t = xhat * c2.double().view(c)
    sc = scale.double().view(c)
    ref = sc * (dz.double() - c1.double().view(c) - t)
    cond = sc.abs() * (dz.double().abs() + c1.double().abs().view(c) + t.abs())
    return ref, cond


def stored_sums(y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """A bf16 statistics epilogue sums the values AS STORED (gsd_bf16_conv.hip: `statistics of the values as stored`):
    (sum y, sum y^2, sum |y|, sum y^2) per channel of the stored (n, c, h, w) output."""
    y = y.double()
    q = y * y
    return y.sum((0, 2, 3)), q.sum((0, 2, 3)), y.abs().sum((0, 2, 3)), q.sum((0, 2, 3))


# ------------------------------------------------------------------------------ fp32 engine: BatchNorm finalize, Adam + EMA
def check_bound_rounded(got: torch.Tensor, ref: torch.Tensor, cond: torch.Tensor, tau: float, what: str,
                        key: Optional[str] = None, weights: bool = True, n0: int = 0) -> float:
    """An fp32 result that a kernel computes in fp64 and rounds once (BatchNorm finalize, running statistics) or in a short fp32
    chain whose last rounding is of the result itself: |got - ref| <= U32 |ref| + tau * cond.  Report as check_bound."""
    return check_bound(got, ref, cond, tau, what, n0=n0, key=key, weights=weights, _base=U32 * ref.abs())


def bn_finalize_ref(s1: torch.Tensor, s2: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor, count: float, gamma: torch.Tensor,
                    beta: torch.Tensor, eps: float = 1e-5, momentum: float = 0.1, running_mean: Optional[torch.Tensor] = None,
                    running_var: Optional[torch.Tensor] = None) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """gsd_bn_finalize / gsd_bn_reduce_finalize from per-channel sums: s1 = sum y, s2 = sum y^2 (fp64 references) and the bounds
    of the kernel's sums, |sum - s1| <= tau b1, |sum of squares - s2| <= tau b2.  Returns name -> (ref, cond) for mean, var
    (biased), invstd, scale, shift and, given the prior buffers, running_mean / running_var (momentum, unbiased variance, as
    BatchNorm2d): each output obeys |got - ref| <= U32 |ref| + tau * cond (check_bound_rounded).

    The kernels take the one-pass variance q / count - mean^2 in fp64, so the sums' errors carry into it as
    (b2 + 2 |mean| b1) / count: relative to var + eps that is (E[y^2] + 2 |mean| E|y|) / (var + eps) times the sums' relative
    bound -- large for a channel whose |mean| / std is large, and the bound grows with it.  invstd = (var + eps)^-1/2 carries
    half the relative error of var + eps; scale, shift and the running statistics are carried from mean and invstd.  A negative
    one-pass variance (rounding, a constant channel) is clamped to 0 before it is used, as the kernels do."""
    f = lambda v: torch.as_tensor(v, dtype=torch.float32).double().item()   # noqa: E731  (the kernels' float eps / momentum)
    eps, mom = f(eps), f(momentum)
    s1, s2, b1, b2 = s1.double(), s2.double(), b1.double(), b2.double()
    g, bt = gamma.double(), beta.double()
    mu = s1 / count
    cmu = b1 / count
    var = s2 / count - mu * mu
    cvar = (b2 + 2.0 * mu.abs() * b1) / count
    istd = 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)
    cis = 0.5 * istd * cvar / (var.clamp_min(0.0) + eps)
    out = {"mean": (mu, cmu), "var": (var, cvar), "invstd": (istd, cis), "scale": (g * istd, g.abs() * cis),
           "shift": (bt - mu * g * istd, g.abs() * (cmu * istd + mu.abs() * cis))}
    if running_mean is not None:
        unb = count / (count - 1.0) if count > 1 else 1.0
        out["running_mean"] = ((1.0 - mom) * running_mean.double() + mom * mu, mom * cmu)
        out["running_var"] = ((1.0 - mom) * running_var.double() + mom * unb * var.clamp_min(0.0), mom * unb * cvar)
    return out


def f32c(v: float) -> float:
    """A host constant as the kernel receives it: rounded to fp32, widened back."""
    return torch.tensor(v, dtype=torch.float32).double().item()


def adam_ema_ref(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, ema: Optional[torch.Tensor], step: int,
                 lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
                 ema_decay: float = 0.0, grad_scale: float = 1.0, kernel_constants: bool = True
                 ) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """One gsd_adam_ema step in fp64 from the fp32 state: torch's single-tensor Adam with coupled L2 (g' = g * grad_scale + wd p,
    m' = m.lerp(g', 1 - b1), v' = b2 v + (1 - b2) g'^2, p' = p - lr / bc1 * m' / (sqrt(v') / sqrt(bc2) + eps)) and torch_ema's
    shadow update ema' = ema - (1 - d) (ema - p').  kernel_constants: use the constants exactly as the kernel holds them (every
    host float rounded to fp32, lr / bc1 and sqrt(bc2) formed in double from the fp32 betas and rounded once, 1 - d in fp32);
    False: plain fp64 constants (torch.optim.Adam in float64).

    Returns name -> (ref, cond) for p, m, v (and ema): cond sums the magnitudes that the fp32 evaluation's roundings scale with
    -- every intermediate once, and the errors of m' and of the denominator carried into the step through their relative
    sizes -- so |got - ref| <= tau * cond with tau a few fp32 unit roundoffs."""
    k = f32c if kernel_constants else float
    b1, b2, ep, wd, lr_, gs = k(beta1), k(beta2), k(eps), k(weight_decay), k(lr), k(grad_scale)
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    lr_bc1, sbc2 = (f32c(lr_ / bc1), f32c(math.sqrt(bc2))) if kernel_constants else (lr_ / bc1, math.sqrt(bc2))
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    omd = f32c(1.0 - k(ema_decay)) if kernel_constants else 1.0 - ema_decay
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gv = g * gs + wd * p
    cg = (g * gs).abs() + (wd * p).abs()
    m1 = m + (gv - m) * omb1
    cm = m.abs() + (gv - m).abs() * omb1 + omb1 * cg + m1.abs()
    v1 = v * b2 + omb2 * gv * gv
    cv = b2 * v.abs() + omb2 * (gv * gv + 2.0 * gv.abs() * cg) + v1.abs()
    sv = torch.sqrt(v1) / sbc2
    csv = torch.where(v1 > 0, sv * (0.5 * cv / v1.clamp_min(1e-300) + 2.0), cv.sqrt() / sbc2)
    den = sv + ep
    cden = csv + den
    q = m1 / den
    cq = cm / den + q.abs() * cden / den + q.abs()
    dp = lr_bc1 * q
    p1 = p - dp
    cp = lr_bc1 * cq + dp.abs() + p1.abs()
    out = {"p": (p1, cp), "m": (m1, cm), "v": (v1, cv)}
    if ema is not None:
        e = ema.double()
        e1 = e - omd * (e - p1)
        out["ema"] = (e1, omd * (2.0 * (e - p1).abs() + cp) + e1.abs())
    return out
