"""fp64 restatements of the kernels that feed the network -- gsd_dataset.hip (ingest, Gaussian blur, channel statistics, batch
gather) and the 'area' form at the head of gsd_resize.hip -- written from their definitions, with the per-element condition
numbers and derived bounds the GPU tests hold them to, the mutated references that prove those bounds reject a small local
mistake, and the case tables both test modules walk.  A helper module (imported by tests/test_data_path_ref_cpu.py and
tests/test_gpu_data_path_fp64.py), not collected.  Plain numpy / torch float64: nothing from oracle/, nothing from the product.

As in tests/fp64_ref.py every reference returns (ref, cond, ...): cond is the sum of the magnitudes of the terms the kernel adds,
so an fp32 evaluation with r roundings lands within r * 2^-24 * cond of ref (first order), whatever its order.

  area   out = A[c'] * mean_{window} pre(x) + B[c'],  pre(x) = (x - base + pre_add) * pre_mul with a base, else x;
         window [floor(o*I/O), ceil((o+1)*I/O)) per dimension, n_e terms.  The kernel rounds: the difference image twice per term
         (x - base, + pre_add; * 0.5 is exact), n_e - 1 additions, the division, the fmaf:
             |got - ref| <= (n_e + 4) * 2^-24 * cond_e           (n_e + 3 at first order; one more holds the second order)
  blur   out = sum_{i,j} k2[i][j] * x[reflect(h+i-r)][reflect(w+j-r)]: a chain of K*K fmaf, one rounding each:
             |got - ref| <= (K*K + 1) * 2^-24 * cond
  stats  min, max (selections: bit-equal), mean, unbiased std, with torch's answers for NaN, +-inf and a single element
  gather fmaf(src[idx[b]], A[c'], B[c']), one rounding of an exactly known value: bit-equal; an index outside [0, M): a NaN row
"""
import math

import numpy as np
import torch

from fp64_ref import U32, fmaf32


# ------------------------------------------------------------------------------------------------------------------- area
def windows(n_in, n_out):
    """(n_out, n_in) 0/1 matrix of the adaptive-average-pool windows [floor(o*I/O), ceil((o+1)*I/O))."""
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        m[o, (o * n_in) // n_out:-((-(o + 1) * n_in) // n_out)] = 1.0
    return m


def _pre(x, base, pre_add, pre_mul):
    """(p, mag): the averaged image in fp64 and the magnitude an fp32 evaluation of one of its terms scales with."""
    x = np.asarray(x, np.float64)
    if base is None:
        return x, np.abs(x)
    b = np.asarray(base, np.float64)
    return (x - b + pre_add) * pre_mul, (np.abs(x) + np.abs(b) + pre_add) * pre_mul


def _per_channel(v, c):
    v = np.asarray(v, np.float32).astype(np.float64).reshape(-1)
    return v[np.minimum(np.arange(c), v.size - 1)].reshape(1, c, 1, 1)


def _area(p, mag, wh, ww, A, B):
    n_e = np.outer(wh.sum(1), ww.sum(1))
    a, b = _per_channel(A, p.shape[1]), _per_channel(B, p.shape[1])
    ref = a * ((wh @ p @ ww.T) / n_e) + b
    cond = np.abs(a) * ((wh @ mag @ ww.T) / n_e) + np.abs(b)
    return ref, cond, n_e


def area_ref(x, base, size, A, B, pre_add=255.0, pre_mul=0.5):
    """(ref, cond, n_e) of gsd_area_resize_affine / gsd_ingest_images (A = [1], B = [0]) for x, base (N, C, H, W) of any dtype:
    ref, cond (N, C, OH, OW) fp64, n_e (OH, OW) the number of terms of each window."""
    p, mag = _pre(x, base, pre_add, pre_mul)
    return _area(p, mag, windows(p.shape[2], size[0]), windows(p.shape[3], size[1]), A, B)


def area_bound(cond, n_e):
    return (n_e + 4.0) * U32 * cond


def area_ref_last_column_shifted(x, base, size, A, B, pre_add=255.0, pre_mul=0.5):
    """Mutation: the window of the LAST output column starts and ends one input column early; every other column is right.
    None when the input has one column (there is no other column to read)."""
    p, mag = _pre(x, base, pre_add, pre_mul)
    if p.shape[3] < 2:
        return None
    ww = windows(p.shape[3], size[1])
    ww[-1] = np.roll(ww[-1], -1)
    assert ww[-1, -1] == 0.0 and ww[-1].sum() == windows(p.shape[3], size[1])[-1].sum()
    return _area(p, mag, windows(p.shape[2], size[0]), ww, A, B)[0]


def area_ref_one_term_dropped(x, base, size, A, B, pre_add=255.0, pre_mul=0.5):
    """Mutation: image 0, channel 0, the first element with the largest window sums all its terms but the largest one (and
    still divides by n_e).  Returns (mutated ref, (oh, ow))."""
    p, mag = _pre(x, base, pre_add, pre_mul)
    wh, ww = windows(p.shape[2], size[0]), windows(p.shape[3], size[1])
    ref, _, n_e = _area(p, mag, wh, ww, A, B)
    oh, ow = np.unravel_index(int(n_e.argmax()), n_e.shape)
    win = p[0, 0][np.ix_(wh[oh] > 0, ww[ow] > 0)]
    term = win.reshape(-1)[int(np.abs(win).argmax())]
    ref = ref.copy()
    ref[0, 0, oh, ow] -= _per_channel(A, p.shape[1])[0, 0, 0, 0] * term / n_e[oh, ow]
    return ref, (int(oh), int(ow))


# ------------------------------------------------------------------------------------------------------------------- blur
def gaussian_k2(k):
    """The fp32 K x K kernel of torchvision.transforms.functional.gaussian_blur(img, k) with its default sigma
    0.3 * ((k - 1) * 0.5 - 1) + 0.8, restated from the published definition: normalised fp32 pdf on K points, outer product."""
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / (k * 0.15 + 0.35)).pow(2))
    k1 = pdf / pdf.sum()
    return torch.mm(k1[:, None], k1[None, :])


def _reflect(i, n):
    """Reflect without repeating the edge: -1 -> 1, n -> n - 2."""
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


def _symmetric(i, n):
    """Reflect WITH the edge repeated: -1 -> 0, n -> n - 1."""
    return np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))


def _blur(x, k2, index):
    x = np.asarray(x, np.float64)
    k2 = np.asarray(k2, np.float32).astype(np.float64)
    k, r = k2.shape[0], k2.shape[0] // 2
    h, w = x.shape[-2:]
    ref, cond = np.zeros(x.shape), np.zeros(x.shape)
    for i in range(k):
        rows = x[..., index(np.arange(h) + i - r, h), :]
        for j in range(k):
            t = k2[i, j] * rows[..., index(np.arange(w) + j - r, w)]
            ref += t
            cond += np.abs(t)
    return ref, cond


def blur_ref(x, k2):
    """(ref, cond) of gsd_gaussian_blur on x (..., H, W): the K*K taps with the fp32 k2 the kernel is handed, in fp64."""
    return _blur(x, k2, _reflect)


def blur_bound(cond, k):
    return (k * k + 1.0) * U32 * cond


def blur_ref_edge_repeated(x, k2):
    """Mutation: 'symmetric' padding in place of 'reflect'.  Only pixels within K/2 of a border change."""
    return _blur(x, k2, _symmetric)[0]


def blur_ref_one_pixel_shifted_kernel(x, k2):
    """Mutation: at ONE border pixel (first plane, row 0, last column) every tap meets the weight of its left neighbour, the
    kernel shifted by one tap along its transposed axis (k2 is symmetric: a plain transpose changes nothing).  Returns
    (mutated ref, position)."""
    x = np.asarray(x, np.float64)
    ref = blur_ref(x, k2)[0].copy()
    k2 = np.asarray(k2, np.float32).astype(np.float64)
    k, r = k2.shape[0], k2.shape[0] // 2
    h, w = x.shape[-2:]
    first = (0,) * (x.ndim - 2)
    hh, ww = _reflect(np.arange(k) - r, h), _reflect(w - 1 + np.arange(k) - r, w)
    ref[first + (0, w - 1)] = (np.roll(k2.T, 1, axis=0).T * x[first][np.ix_(hh, ww)]).sum()
    return ref, first + (0, w - 1)


# ------------------------------------------------------------------------------------------------------------------ stats
def stats_ref(x):
    """(C, 4) fp64 {min, max, mean, unbiased std} per channel of x (N, C, H, W), two passes in fp64, answering as torch's
    tensor.min() / .max() / .mean() / .std() do: any NaN makes all four NaN; an infinity makes the mean infinite (NaN when both
    signs occur) and the std NaN; a single element has std NaN."""
    x = np.asarray(x, np.float64)
    out = np.empty((x.shape[1], 4))
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(x.shape[1]):
            v = x[:, c].reshape(-1)
            mean = v.sum() / v.size
            var = ((v - mean) ** 2).sum() / np.float64(v.size - 1)
            out[c] = v.min(), v.max(), mean, np.sqrt(var)
    return out


# ----------------------------------------------------------------------------------------------------------------- gather
def gather_affine_ref(src, idx, A, B):
    """(ref, cond) of gsd_gather_affine, (len(idx), C, H, W) fp64 tensors: ref holds fp32 fmaf(src[idx[b]], A[c'], B[c'])
    exactly, c' = min(c, nab - 1); an index outside [0, M) gives a NaN row."""
    m, c = src.shape[:2]
    idx = torch.as_tensor(idx, dtype=torch.int64)
    ok = (idx >= 0) & (idx < m)
    cc = torch.arange(c).clamp_max(len(A) - 1)
    a = torch.as_tensor(A, dtype=torch.float32)[cc].view(1, c, 1, 1)
    b = torch.as_tensor(B, dtype=torch.float32)[cc].view(1, c, 1, 1)
    rows = src.float()[torch.where(ok, idx, torch.zeros_like(idx))]
    ref = fmaf32(rows, a, b)
    cond = (rows.double() * a.double()).abs() + b.double().abs()
    nan = torch.full((), math.nan, dtype=torch.float64)
    sel = ok.view(-1, 1, 1, 1)
    return torch.where(sel, ref, nan), torch.where(sel, cond, nan)


# ------------------------------------------------------------------------------------------------------------------ cases
# What the GPU module launches, as data: the CPU module proves on exactly these inputs that every mutation exceeds the bound.
AREA_EXTRA = ((64, 86), (2, 3))         # windows of 32 x 29 = 928 and 32 x 30 = 960 terms
AFFINES = (("nab1", [-1 / 40.0], [2.5]), ("nabC", [1 / 40.0, -1 / 50.0, 1 / 60.0], [-3.0, 2.2, -2.1]))
BLUR_SHAPES = ((2, 1, 10, 13, 3), (3, 2, 17, 9, 5), (1, 1, 160, 213, 9), (2, 1, 6, 7, 11), (1, 1, 4, 4, 1))
BLUR_MANY = (65539, 1, 2, 2, 3)         # crosses the 65535-plane launch


def frames(seed, n, c, h, w, dtype=torch.float32):
    """Camera-like frames in [0, 256): uint8, or fp32 with a fractional part so that no rounding is exact by accident."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, c, h, w), generator=g, dtype=torch.int32)
    if dtype == torch.uint8:
        return x.to(torch.uint8)
    return x.float() + torch.rand((n, c, h, w), generator=g)


def resize_cases(shape):
    """(name, x, base or None, size, A, B) of every gsd_area_resize_affine launch at `shape`: N = 2, C = 3, fp32."""
    (h, w), size = shape
    x, base = frames(11, 2, 3, h, w), frames(12, 2, 3, h, w)
    for tag, A, B in AFFINES:
        for b in (None, base):
            yield f"{tag}-{'base' if b is not None else 'plain'}", x, b, size, A, B


def ingest_cases(shape):
    """(name, raw, base or None, c0, size) of every gsd_ingest_images launch at `shape`: the two fingers of a 6-channel
    object, N = 2, fp32 and uint8."""
    (h, w), size = shape
    for dtype, name in ((torch.float32, "f32"), (torch.uint8, "u8")):
        raw, base = frames(13, 2, 6, h, w, dtype), frames(14, 2, 6, h, w, dtype)
        for c0 in (0, 3):
            for b in (None, base):
                yield f"{name}-c{c0}-{'base' if b is not None else 'plain'}", raw, b, c0, size


def blur_input(n, c, h, w, k):
    """Depth-like planes of mixed sign."""
    return torch.randn((n, c, h, w), generator=torch.Generator().manual_seed(1000 * h + 10 * w + k)) * 2.0 + 0.25


def chunk_case():
    """32770 samples of 1x2x2 uint8 with a base, resized to 1x1: crosses ingest_images' chunk of 32768 samples."""
    return frames(15, 32770, 1, 2, 2, torch.uint8), frames(16, 32770, 1, 2, 2, torch.uint8)
