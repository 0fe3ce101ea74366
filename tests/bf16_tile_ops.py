"""Operands and fp64 references of the cases in tests/bf16_tile_cases.py, for the two passes of
tests/test_gpu_bf16_tile_forms_fp64.py.  A helper module, not collected.  Operands are drawn on the CPU from a generator seeded
by the case id and the pass, so tests/test_bf16_tile_form_coverage_cpu.py sees exactly the operands the GPU module launches with
and can prove from the fp64 reference alone that the exact pass is exact.

random pass  normal activations rounded to bf16, weights scaled by 1 / sqrt(fan-in) (rounded to bf16 by the weight image).
exact pass   activations and gradients in {-1, 0, 1}; every OUTPUT ROW's weights (over all taps and K) hold at most NZ = 100
             non-zeros in {+-1, +-2}; biases and eval shifts are integers of magnitude <= 8.  cond = sum |a||w| + |bias| is then
             at most 2 * 100 + 8 = 208 <= 256 at every stored element whatever the activations are: every partial sum in any
             order is an integer of magnitude <= 256, which fp32 and bf16 both hold exactly, so the stored result must EQUAL the
             fp64 reference.  A dW element sums at most N*H*W < 2^24 products of magnitude <= 1: exact in fp32.
             Fused BatchNorm backward: y even integers in [-4, 4], scale in {+-0.5, +-1, 2}, shift a half-integer (y * scale is an
             integer, so the mask argument y * scale + shift is never zero), integer mean, invstd in {1, 2}: xhat and dz * xhat
             are integers.
"""
from __future__ import annotations

import math
import zlib

import torch

import bf16_tile_cases as B
import fp64_ref as R

NZ = 100
LIM_BF16 = 256.0            # integers up to here are bf16 numbers
LIM_F32 = 2.0 ** 24         # ... and up to here fp32 numbers
PASSES = ("random", "exact")


def gen(cid: str, mode: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(f"{cid}/{mode}".encode()))


def acts(g, mode, *shape):
    """(n, c, h, w) activations or gradients as fp64 values that are bf16 numbers."""
    if mode == "exact":
        return torch.randint(-1, 2, shape, generator=g).double()
    return R.bf16(torch.randn(shape, generator=g))


def weights(g, mode, shape, row_dims, fan_in):
    """fp32 master weights; row_dims: the dimensions that index an output row of the contraction."""
    if mode != "exact":
        return torch.randn(shape, generator=g) / fan_in ** 0.5
    rest = [d for d in range(len(shape)) if d not in row_dims]
    perm = list(row_dims) + rest
    rows = math.prod(shape[d] for d in row_dims)
    cols = math.prod(shape[d] for d in rest)
    k = min(NZ, cols)
    idx = torch.rand((rows, cols), generator=g).argsort(1)[:, :k]
    vals = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (rows, k), generator=g)]
    flat = torch.zeros((rows, cols)).scatter_(1, idx, vals)
    inv = [perm.index(d) for d in range(len(shape))]
    return flat.view([shape[d] for d in perm]).permute(inv).contiguous()


def bias(g, mode, c):
    if mode == "exact":
        return torch.randint(-8, 9, (c,), generator=g).float()
    return torch.randn(c, generator=g)


def pick(g, vals, c):
    return torch.tensor(vals)[torch.randint(0, len(vals), (c,), generator=g)].float()


def eval_coeffs(g, mode, c):
    """(scale, shift) of a conv + BatchNorm + ReLU epilogue."""
    if mode == "exact":
        return pick(g, [1.0, -1.0], c), torch.randint(-8, 9, (c,), generator=g).float()
    return torch.rand(c, generator=g) * 1.2 + 0.3, torch.randn(c, generator=g) * 0.3


def bn_coeffs(g, mode, n, c, h, w):
    """y (n, c, h, w) fp64 and the fp32 (scale, shift, mean, invstd) of a fused BatchNorm-backward epilogue."""
    if mode == "exact":
        y = 2.0 * torch.randint(-2, 3, (n, c, h, w), generator=g).double()
        return dict(y=y, sc=pick(g, [0.5, -0.5, 1.0, -1.0, 2.0], c), sh=torch.randint(-3, 3, (c,), generator=g).float() + 0.5,
                    mean=torch.randint(-3, 4, (c,), generator=g).float(), invstd=pick(g, [1.0, 2.0], c))
    return dict(y=acts(g, mode, n, c, h, w), sc=torch.rand(c, generator=g) * 1.2 + 0.3, sh=torch.randn(c, generator=g) * 0.3,
                mean=torch.randn(c, generator=g) * 0.2, invstd=torch.rand(c, generator=g) * 1.5 + 0.5)


def to(o, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in o.items()}


def _masked(o, ref, cond):
    m = R.bnrelu_mask(o["y"], o["sc"], o["sh"])
    return ref * m, cond * m


def _relu_ep(o, ref, cond):
    cv = (1, -1, 1, 1)
    t = ref * o["sc"].double().view(cv) + o["sh"].double().view(cv)
    return t.clamp_min(0.0), cond * o["sc"].double().abs().view(cv) + o["sh"].double().abs().view(cv)


# ----------------------------------------------------------------------------------------------------------------- conv3x3
def conv3_ops(c: B.Conv3, mode: str):
    g = gen(B.conv3_id(c), mode)
    o = dict(a=acts(g, mode, c.n, c.k, c.h, c.w))
    if c.ep == "bnbwd":     # a dX launch: a is dy (K = Cout channels), the weights (Cout, Cin, 3, 3), an output row is a Cin
        o["wt"] = weights(g, mode, (c.k, c.m, 3, 3), (1,), 9 * c.k)
        o.update(bn_coeffs(g, mode, c.n, c.m, c.h, c.w))
    else:
        o["wt"] = weights(g, mode, (c.m, c.k, 3, 3), (0,), 9 * c.k)
        if c.ep == "bnrelu":
            o["sc"], o["sh"] = eval_coeffs(g, mode, c.m)
    return o


def conv3_ref(c: B.Conv3, o):
    """(ref, cond) of the stored output, NCHW fp64 on the operands' device."""
    w64 = R.bf16(o["wt"])
    if c.ep == "bnbwd":
        return _masked(o, *R.conv3x3_dx(o["a"], w64))
    ref, cond = R.conv3x3_fwd(o["a"], w64)
    return _relu_ep(o, ref, cond) if c.ep == "bnrelu" else (ref, cond)


# ------------------------------------------------------------------------------------------- dense / large-tile ConvT cases
def dense_ops(c: B.Dense, mode: str, cid: str):
    g = gen(cid, mode)
    if c.kind in ("1x1", "1x1bnrelu"):
        o = dict(a=acts(g, mode, c.n, c.k, c.h, c.w), wt=weights(g, mode, (c.m, c.k), (0,), c.k))
        if c.kind == "1x1":
            o["b"] = bias(g, mode, c.m)
        else:
            o["sc"], o["sh"] = eval_coeffs(g, mode, c.m)
        return o
    if c.kind == "ctfwd":   # weights (Cin, Cout, 2, 2): an output row is (co, kh, kw)
        return dict(a=acts(g, mode, c.n, c.k, c.h, c.w), wt=weights(g, mode, (c.k, c.cs, 2, 2), (1, 2, 3), c.k), b=bias(g, mode, c.cs))
    # ctdx: the gradient of the upsampled tensor (Cout = K channels), weights (Cin = M, Cout, 2, 2): an output row is a ci
    dy = acts(g, mode, c.n, c.k, 2 * c.h, 2 * c.w)
    if c.crop:              # the buffer ends one row and one column early: what lies beyond reads as zero
        dy[:, :, -1, :] = 0.0
        dy[:, :, :, -1] = 0.0
    o = dict(a=dy, wt=weights(g, mode, (c.m, c.k, 2, 2), (0,), 4 * c.k))
    if c.fused:
        o.update(bn_coeffs(g, mode, c.n, c.m, c.h, c.w))
    return o


def dense_ref(c: B.Dense, o):
    w64 = R.bf16(o["wt"])
    if c.kind == "1x1":
        return R.conv1x1_fwd(o["a"], w64, o["b"].double())
    if c.kind == "1x1bnrelu":
        return _relu_ep(o, *R.conv1x1_fwd(o["a"], w64, torch.zeros(c.m, dtype=torch.float64, device=w64.device)))
    if c.kind == "ctfwd":
        return R.convT_fwd(o["a"], w64, o["b"].double())
    ref, cond = R.convT_dx(o["a"], w64)
    return _masked(o, ref, cond) if c.fused else (ref, cond)


# ---------------------------------------------------------------------------------------------------------------------- dW
def wg_ops(c: B.Wg, mode: str):
    g = gen(B.wg_id(c), mode)
    a = acts(g, mode, c.n, c.m, c.h, c.w)
    if c.taps == 4:
        b = acts(g, mode, c.n, c.ncols, 2 * c.h, 2 * c.w)
        if c.crop:
            b[:, :, -1, :] = 0.0
            b[:, :, :, -1] = 0.0
    else:
        b = acts(g, mode, c.n, c.ncols, c.h, c.w)
    return dict(a=a, b=b)


def wg_ref(c: B.Wg, o):
    """(dW ref, cond) in the kernel's output layout (m, ncols_out, taps), and for 4 taps (db ref, db cond) else None."""
    if c.taps == 9:
        ref, cond = R.conv3x3_dw(o["b"], o["a"])
        return ref.reshape(c.m, c.ncols, 9), cond.reshape(c.m, c.ncols, 9), None
    if c.taps == 1:
        ref, cond, _, _ = R.conv1x1_dw(o["b"], o["a"])
        return ref[:, :c.ncols_out, None].contiguous(), cond[:, :c.ncols_out, None].contiguous(), None
    dw, cw, db, cb = R.convT_dw(o["a"], o["b"])
    return dw.reshape(c.m, c.ncols, 4), cw.reshape(c.m, c.ncols, 4), (db, cb)
