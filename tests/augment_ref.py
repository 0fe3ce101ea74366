"""References for gsd_gather_augment, written from the stream's definition in include/gsd.h (not from the kernel):

  * a numpy uint64 restatement of the random stream -- sample key, flips, shifts, per-channel gain / offset, pixel noise;
  * an fp64 restatement of geometry + photometry that returns (ref, cond) in the style of tests/fp64_ref.py:
        cond = |A| (|gain_c| |x - pivot| + |pivot| + |offset_c| + |noise_std n|) + |B|
    so that the fp32 kernel's five roundings (t, fmaf, + offset, fmaf, fmaf) are bounded by 5 * 2^-24 * cond.

lib_sample / lib_noise are thin wrappers of the library's device-free queries gsd_augment_sample / gsd_augment_noise, returning
what `sample` / `noise` return.

A helper module: no test lives here.  `params` everywhere is a dict with the gsd_augment fields
(seed, p_hflip, p_vflip, max_dy, max_dx, gain, offset, noise_std, pivot); the epoch is passed beside it.
"""
import ctypes as C

import numpy as np

U = np.uint64
GAMMA = U(0x9E3779B97F4A7C15)
NOISE_TAG = U(0x6E6F697365)
NOISE_SCALE = np.float32(np.sqrt(3.0) / 65536.0)
CEILING = 8 * 2.0 ** -24        # TAU_AUG may never exceed this: five fp32 roundings, each bounded by 2^-24 * cond

DEFAULTS = dict(seed=0, p_hflip=0.0, p_vflip=0.0, max_dy=0, max_dx=0, gain=0.0, offset=0.0, noise_std=0.0, pivot=0.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _u64(v):
    """int (any sign, any size) or integer array -> uint64 array, two's complement / modulo 2^64."""
    if isinstance(v, (int, np.integer)):
        return np.array([int(v) & 0xFFFFFFFFFFFFFFFF], dtype=U)
    v = np.asarray(v)
    return v.astype(np.int64).view(U) if v.dtype != U else v


def fin(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def mix(z):
    with np.errstate(over="ignore"):
        return fin(z + GAMMA)


def sample_key(seed, epoch, index):
    """K = mix(mix(mix(seed) ^ epoch) ^ index), one per entry of `index`."""
    return mix(mix(mix(_u64(seed)) ^ _u64(epoch)) ^ _u64(index))


def draw(key, k):
    with np.errstate(over="ignore"):
        return fin(key + U(k + 1) * GAMMA)


def _u_hi(r):
    return (r >> U(40)).astype(np.float64) * 2.0 ** -24


def _u_lo(r):
    return ((r >> U(16)) & U(0xFFFFFF)).astype(np.float64) * 2.0 ** -24


def sample(p, epoch, index, ci):
    """The draws of dataset rows `index` (array): dict of hflip, vflip (bool), dy, dx (int64), gain, offset ((n, ci) float32;
    computed in fp64 and rounded once more to fp32, so a gain may sit 1 ulp from the fmaf the library evaluates)."""
    key = sample_key(p["seed"], epoch, index)
    r0, r1 = draw(key, 0), draw(key, 1)
    my, mx = int(p["max_dy"]), int(p["max_dx"])
    out = {"hflip": _u_hi(r0) < float(np.float32(p["p_hflip"])), "vflip": _u_lo(r0) < float(np.float32(p["p_vflip"])),
           "dy": -my + (((r1 >> U(32)) * U(2 * my + 1)) >> U(32)).astype(np.int64),
           "dx": -mx + (((r1 & U(0xFFFFFFFF)) * U(2 * mx + 1)) >> U(32)).astype(np.int64)}
    g, o = float(np.float32(p["gain"])), float(np.float32(p["offset"]))
    gain, offset = np.empty((key.size, ci), np.float32), np.empty((key.size, ci), np.float32)
    for c in range(ci):
        r = draw(key, 2 + c)
        gain[:, c] = (g * (2.0 * _u_hi(r) - 1.0) + 1.0).astype(np.float32)
        offset[:, c] = (o * (2.0 * _u_lo(r) - 1.0)).astype(np.float32)
    out["gain"], out["offset"] = gain, offset
    return out


def noise(p, epoch, index, first, n):
    """Unit-variance noise of image elements [first, first + n) of ONE dataset row, float32, bit for bit the library's."""
    nk = mix(sample_key(p["seed"], epoch, int(index)) ^ NOISE_TAG)
    with np.errstate(over="ignore"):
        r = fin(nk + (np.arange(first, first + n, dtype=U) + U(1)) * GAMMA)
    s = sum(((r >> U(16 * i)) & U(0xFFFF)).astype(np.int64) for i in range(4))
    return (s - 131070).astype(np.float32) * NOISE_SCALE


def source_index(h, w, dy, dx, hflip, vflip):
    """(hs, ws): the source row of every output row and the source column of every output column."""
    hs = np.clip(np.arange(h) - int(dy), 0, h - 1)
    ws = np.clip(np.arange(w) - int(dx), 0, w - 1)
    if vflip:
        hs = h - 1 - hs
    if hflip:
        ws = w - 1 - ws
    return hs, ws


def gather_augment_ref(src, idx, A, B, p, epoch, photometry=True, draws=None):
    """fp64 (ref, cond), each (len(idx), C, H, W), of one output tensor of gsd_gather_augment: `src` (M, C, H, W) float32 is the
    image arena (photometry=True) or the depth arena (photometry=False: geometry, then A x + B).  `draws` (as `sample` returns
    them, for the rows `idx`) replaces the restatement's own, e.g. by the library's gsd_augment_sample output."""
    src = np.asarray(src)
    idx = np.asarray(idx, dtype=np.int64)
    m, c, h, w = src.shape
    assert idx.min() >= 0 and idx.max() < m
    A = np.asarray(A, np.float32).astype(np.float64)
    B = np.asarray(B, np.float32).astype(np.float64)
    A, B = A[np.minimum(np.arange(c), A.size - 1)], B[np.minimum(np.arange(c), B.size - 1)]
    d = sample(p, epoch, idx, c if photometry else 1) if draws is None else draws
    pivot, ns = float(np.float32(p["pivot"])), float(np.float32(p["noise_std"]))
    on = photometry and (p["gain"] != 0 or p["offset"] != 0 or p["noise_std"] != 0)
    ref, cond = np.empty((idx.size, c, h, w)), np.empty((idx.size, c, h, w))
    a4, b4 = A.reshape(c, 1, 1), B.reshape(c, 1, 1)
    for b, row in enumerate(idx):
        hs, ws = source_index(h, w, d["dy"][b], d["dx"][b], d["hflip"][b], d["vflip"][b])
        x = src[row][:, hs[:, None], ws[None, :]].astype(np.float64)
        if not on:
            ref[b], cond[b] = x * a4 + b4, np.abs(x) * np.abs(a4) + np.abs(b4)
            continue
        g = d["gain"][b].astype(np.float64).reshape(c, 1, 1)
        o = d["offset"][b].astype(np.float64).reshape(c, 1, 1)
        nz = 0.0
        if ns != 0.0:
            nz = ns * noise(p, epoch, row, 0, c * h * w).astype(np.float64).reshape(c, h, w)
        t = x - pivot
        ref[b] = (g * t + pivot + o + nz) * a4 + b4
        cond[b] = np.abs(a4) * (np.abs(g) * np.abs(t) + abs(pivot) + np.abs(o) + np.abs(nz)) + np.abs(b4)
    return ref, cond


def lib_struct(p, epoch):
    from gelslim_depth_amd import _lib as L
    return L.make_augment(p["seed"], epoch, p["p_hflip"], p["p_vflip"], p["max_dy"], p["max_dx"], p["gain"], p["offset"],
                          p["noise_std"], p["pivot"])


def lib_sample(p, epoch, index, ci):
    """gsd_augment_sample over the rows `index`, as the dict `sample` returns."""
    from gelslim_depth_amd import _lib as L
    a, d = lib_struct(p, epoch), L.gsd_augment_draw()
    n = len(index)
    out = {"hflip": np.empty(n, bool), "vflip": np.empty(n, bool), "dy": np.empty(n, np.int64), "dx": np.empty(n, np.int64),
           "gain": np.empty((n, ci), np.float32), "offset": np.empty((n, ci), np.float32)}
    for i, row in enumerate(index):
        assert L.lib.gsd_augment_sample(C.byref(a), int(row), ci, C.byref(d)) == L.GSD_OK
        assert d.hflip in (0, 1) and d.vflip in (0, 1)
        out["hflip"][i], out["vflip"][i], out["dy"][i], out["dx"][i] = d.hflip, d.vflip, d.dy, d.dx
        out["gain"][i], out["offset"][i] = list(d.gain)[:ci], list(d.offset)[:ci]
        assert list(d.gain)[ci:] == [1.0] * (8 - ci) and list(d.offset)[ci:] == [0.0] * (8 - ci)
    return out


def lib_noise(p, epoch, index, first, n):
    from gelslim_depth_amd import _lib as L
    a, out = lib_struct(p, epoch), np.empty(n, np.float32)
    assert L.lib.gsd_augment_noise(C.byref(a), int(index), first, n, out.ctypes.data) == L.GSD_OK
    return out
