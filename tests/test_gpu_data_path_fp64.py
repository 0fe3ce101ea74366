"""The kernels that feed the network, element by element against fp64: gsd_dataset.hip (gsd_ingest_images, gsd_gaussian_blur,
gsd_channel_stats, gsd_gather_affine) and gsd_area_resize_affine at the head of gsd_resize.hip, 'area' being the default
interp_method and the only one the shipped configuration uses.  References, condition numbers, bounds and case tables are
tests/data_path_ref.py; tests/test_data_path_ref_cpu.py proves on these very inputs that each bound rejects a window one
column off, one dropped term, a repeated edge and a kernel shifted by one tap at one pixel.

Every output starts as NaN in front of a 64-element sentinel tail; what a launch must not read holds NaN (the other finger's
channels of an fp32 object, arena rows no index names).  Nothing is excluded from a comparison.

  area    |got - ref| <= (n_e + 4) * 2^-24 * cond     n_e - 1 additions, two roundings of the difference image, the division and
                                                      the fmaf; the FMA contraction this file allows only removes roundings
          both entry points at every shape of tests/test_gpu_interp.py and 64x86 -> 2x3 (windows of 928 and 960 terms), N = 2
  blur    |got - ref| <= (K*K + 1) * 2^-24 * cond     K*K chained fmaf; K = 1 must copy bit for bit
          the five shapes of tests/test_gpu_dataset.py on inputs of mixed sign, and 65539 planes in one call (two launches)
  ingest  dataset.ingest_images over 32770 samples (two chunks), every sample held to the area bound
  stats   min, max bit-equal; mean, std within 1e-9 relative of the two-pass fp64 reference; NaN and +inf as torch answers
  gather  bit-equal to one fp32 fmaf, vector and scalar forms, misaligned pointers, out-of-range indices -> NaN rows

Largest measured |got - ref| / cond on the MI355X, next to the bound's factor (n_e + 4) * 2^-24 or (K*K + 1) * 2^-24 at that
element -- the largest ratio of a family, then the case that comes closest to its own bound:
  area_resize_affine  3.96e-7 of 5.56e-5 (64x86 -> 2x3, 928 terms, no base);   1.26e-7 of 5.96e-7 (320x427 -> 160x213, 6 terms)
  ingest_images       1.26e-6 of 5.75e-5 (64x86 -> 2x3, 960 terms, f32);       2.14e-7 of 5.96e-7 (320x427 -> 160x213, f32);
                      uint8 at most 5.5e-8 (its sums are exact); the 32770 uint8 samples of the chunk case: 0
  gaussian_blur       3.68e-7 of 4.89e-6 (160x213, K = 9);                     2.31e-7 of 5.96e-7 (65539 planes of 2x2, K = 3)
  channel_stats       mean / std relative error at most 1.15e-11 (normal(100, 0.5), 5x3x16x16) of 1e-9; normal(3, 2): 6.7e-16
No case uses more than 0.39 of its bound.  The module runs in 2.2 s and peaks at 20 MB of device memory.

GSD_DATA_PATH_REPORT=<path>: write the worst |got - ref| / cond per case, the module's wall time and peak device memory there
as JSON.
"""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

import data_path_ref as D
from test_gpu_interp import SHAPES, check_out, nan_out

pytestmark = pytest.mark.gpu

AREA_SHAPES = SHAPES + (D.AREA_EXTRA,)
ids = lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}"       # noqa: E731
RATIOS = {}
T0 = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    torch.cuda.reset_peak_memory_stats()
    T0["t"] = time.time()
    yield
    path = os.environ.get("GSD_DATA_PATH_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"wall_s": time.time() - T0["t"], "max_memory_allocated": torch.cuda.max_memory_allocated(),
                       "ratios": dict(sorted(RATIOS.items()))}, f, indent=1)


@pytest.fixture(scope="module")
def L():
    from gelslim_depth_amd import _lib
    return _lib


def held(got, ref, cond, bound, key):
    """Assert |got - ref| <= bound at every element; record the worst |got - ref| / cond (and the bound's factor there)."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape == cond.shape, key
    assert np.all(np.isfinite(got)), f"{key}: {int((~np.isfinite(got)).sum())} elements not finite"
    err = np.abs(got - ref)
    ratio = np.where(err > 0, err / np.maximum(cond, 1e-300), 0.0)
    i = np.unravel_index(int(ratio.argmax()), ratio.shape)
    factor = float(np.broadcast_to(bound, ref.shape)[i] / max(cond[i], 1e-300))
    if ratio[i] > RATIOS.get(key, {"ratio": -1.0})["ratio"]:
        RATIOS[key] = {"ratio": float(ratio[i]), "bound": factor, "at": [int(v) for v in i]}
    print(f"[data-path] {key}: worst |got-ref|/cond {ratio[i]:.3g} at {i}, bound {factor:.3g}")
    over = err > bound
    assert not over.any(), (f"{key}: {int(over.sum())} of {over.size} elements over the bound, first at "
                            f"{tuple(int(v[0]) for v in np.nonzero(over))}, worst ratio {ratio[i]:.3g} at {i} (bound {factor:.3g})")


# ------------------------------------------------------------------------------------------------------------------- area
@pytest.mark.parametrize("shape", AREA_SHAPES, ids=ids)
def test_area_resize_affine_within_the_derived_bound(L, shape):
    for name, x, base, size, A, B in D.resize_cases(shape):
        n, c, h, w = x.shape
        numel = n * c * size[0] * size[1]
        buf = nan_out(numel)
        a = torch.tensor(A, dtype=torch.float32, device="cuda")
        b = torch.tensor(B, dtype=torch.float32, device="cuda")
        xd = x.cuda().contiguous()
        bd = None if base is None else base.cuda().contiguous()
        L.check(L.lib.gsd_area_resize_affine(xd.data_ptr(), L.ptr(bd), n, c, h, w, buf.data_ptr(), size[0], size[1],
                                             a.data_ptr(), b.data_ptr(), a.numel(), 255.0, 0.5, L.stream_ptr()), name)
        torch.cuda.synchronize()
        got = check_out(buf, numel).reshape(n, c, *size).cpu().numpy()
        ref, cond, n_e = D.area_ref(x, base, size, A, B)
        held(got, ref, cond, D.area_bound(cond, n_e), f"area_resize_affine {ids(shape)} {name}")


@pytest.mark.parametrize("shape", AREA_SHAPES, ids=ids)
def test_ingest_images_finger_split_within_the_derived_bound(L, shape):
    for name, raw, base, c0, size in D.ingest_cases(shape):
        k, c, h, w = raw.shape
        numel = k * 3 * size[0] * size[1]
        buf = nan_out(numel)
        rd = raw.cuda().contiguous()
        bd = None if base is None else base.cuda().contiguous()
        if raw.dtype == torch.float32:          # the other finger is not this launch's to read
            rd[:, 3 - c0:6 - c0] = math.nan
            if bd is not None:
                bd[:, 3 - c0:6 - c0] = math.nan
        L.check(L.lib.gsd_ingest_images(
            rd.data_ptr() + c0 * h * w * rd.element_size(), None if bd is None else bd.data_ptr() + c0 * h * w * bd.element_size(),
            0 if raw.dtype == torch.float32 else 1, k, 3, h, w, c * h * w, h * w, c * h * w, h * w, buf.data_ptr(), size[0],
            size[1], 255.0, 0.5, L.stream_ptr()), name)
        torch.cuda.synchronize()
        got = check_out(buf, numel).reshape(k, 3, *size).cpu().numpy()
        ref, cond, n_e = D.area_ref(raw[:, c0:c0 + 3], None if base is None else base[:, c0:c0 + 3], size, [1.0], [0.0])
        held(got, ref, cond, D.area_bound(cond, n_e), f"ingest_images {ids(shape)} {name}")


def test_ingest_images_across_the_32768_sample_chunk():
    """dataset.ingest_images launches 32768 samples at a time: the second launch's pointers (input, base, output) are offsets
    the Python side computes."""
    from gelslim_depth_amd.dataset import ingest_images
    raw, base = D.chunk_case()
    k = raw.shape[0]
    assert k > 32768
    buf = nan_out(k)
    ingest_images(raw.cuda(), base.cuda(), 0, 1, (1, 1), buf[:k].view(k, 1, 1, 1))
    torch.cuda.synchronize()
    got = check_out(buf, k).reshape(k, 1, 1, 1).cpu().numpy()
    ref, cond, n_e = D.area_ref(raw, base, (1, 1), [1.0], [0.0])
    assert n_e.item() == 4
    held(got, ref, cond, D.area_bound(cond, n_e), "ingest_images 32770 samples")


# ------------------------------------------------------------------------------------------------------------------- blur
@pytest.mark.parametrize("case", D.BLUR_SHAPES + (D.BLUR_MANY,), ids=lambda c: "x".join(map(str, c)))
def test_gaussian_blur_within_the_derived_bound(L, case):
    from gelslim_depth_amd.dataset import gaussian_kernel2d
    n, c, h, w, k = case
    x, k2 = D.blur_input(n, c, h, w, k), D.gaussian_k2(k)
    assert torch.equal(gaussian_kernel2d(k), k2)            # the product hands the kernel these fp32 weights
    numel = x.numel()
    buf = nan_out(numel)
    xd, kd = x.cuda(), k2.cuda()
    L.check(L.lib.gsd_gaussian_blur(xd.data_ptr(), n * c, h, w, kd.data_ptr(), k, buf.data_ptr(), L.stream_ptr()), "blur")
    torch.cuda.synchronize()
    got = check_out(buf, numel).reshape(n, c, h, w).cpu()
    ref, cond = D.blur_ref(x.numpy(), k2.numpy())
    held(got.numpy(), ref, cond, D.blur_bound(cond, k), f"gaussian_blur {'x'.join(map(str, case))}")
    if k == 1:
        assert torch.equal(got, x)          # fmaf(1, x, 0)


# ------------------------------------------------------------------------------------------------------------------ stats
def run_stats(L, x, fill=math.nan):
    """gsd_channel_stats on x (N, C, H, W) -> (C, 4) fp64 numpy; output and workspace start as `fill` before sentinel tails."""
    n, c, h, w = x.shape
    nws = int(L.lib.gsd_channel_stats_workspace(c))
    out = torch.full((4 * c + 64,), fill, dtype=torch.float64, device="cuda")
    ws = torch.full((nws + 64,), math.nan, dtype=torch.float64, device="cuda")
    out[4 * c:] = 1234.5
    ws[nws:] = 1234.5
    xd = x.cuda().contiguous()
    L.check(L.lib.gsd_channel_stats(xd.data_ptr(), n, c, h * w, out.data_ptr(), ws.data_ptr(), L.stream_ptr()), "channel_stats")
    torch.cuda.synchronize()
    assert bool((out[4 * c:] == 1234.5).all()) and bool((ws[nws:] == 1234.5).all()), "write past the end"
    return out[:4 * c].reshape(c, 4).cpu().numpy()


# normal(100, 0.5) is benign for the kernel's one-pass variance (s2 - s * mean) / (count - 1) in fp64.  One rounding at the
# magnitude of the sum of squares moves std, to first order, by
#     count * 2^-53 * E[x^2] / ((count - 1) * 2 * std)   (E[x^2] = sum x^2 / count)   = 1.1e-16 * 1e4 / (2 * 0.5) = 1.1e-12,
# 2.2e-12 of std.  Each of the 64 * 256 lanes adds at most ceil(count / 16384) squares in a row (65 at count = 2^20 + 3), then
# come 14 levels of pairwise sums: at most some 80 such roundings on any path, 1.8e-10 of std if they all pointed one way,
# under the 1e-9 asked (measured: 1.2e-11).  normal(3, 2) has E[x^2] / std^2 = 3.25 and sits at 1e-16.
@pytest.mark.parametrize("mean,std", [(3.0, 2.0), (100.0, 0.5)], ids=["n3_2", "n100_05"])
@pytest.mark.parametrize("shape", [(7, 3, 33, 31), (1, 2, 1, 5), (1, 1, 1, 1), (5, 3, 16, 16), (1, 1, 2 ** 20 + 3, 1)], ids=str)
def test_channel_stats_vs_fp64(L, shape, mean, std):
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(shape[2]), dtype=torch.float64) * std + mean).float()
    got, ref = run_stats(L, x), D.stats_ref(x.numpy())
    assert np.array_equal(got[:, :2], ref[:, :2]), (got, ref)           # min, max: selections
    if x[:, 0].numel() == 1:
        assert np.isnan(got[0, 3]) and np.isnan(ref[0, 3]) and got[0, 0] == got[0, 1] == got[0, 2] == float(x.reshape(-1)[0])
        got, ref = got[:, :3], ref[:, :3]
    assert np.all(np.isfinite(got))
    rel = np.abs(got[:, 2:] - ref[:, 2:]) / np.abs(ref[:, 2:])
    key = f"channel_stats {shape} normal({mean:g}, {std:g})"
    RATIOS[key] = {"ratio": float(rel.max()), "bound": 1e-9}
    print(f"[data-path] {key}: worst relative error of mean / std {rel.max():.3g}")
    assert np.all(rel <= 1e-9), rel


def test_channel_stats_nan_and_inf_as_torch_answers(L):
    """tensor.min() / .max() / .mean() / .std() of the reference all return NaN when an element is NaN; render_depth(...,
    validate=False) writes such a pixel for a refused width, and a min_max normalisation must not look healthy then."""
    x = (torch.randn((7, 3, 33, 31), generator=torch.Generator().manual_seed(9), dtype=torch.float64) * 2 + 3).float()
    clean = run_stats(L, x)
    for pos in ((3, 1, 17, 5), (0, 1, 0, 0), (6, 1, 32, 30)):           # mid-tensor, first and last element of the channel
        bad = x.clone()
        bad[pos] = math.nan
        got, ref = run_stats(L, bad, fill=-7.0), D.stats_ref(bad.numpy())
        print(f"[data-path] channel_stats NaN at {pos}: channel 1 = {got[1].tolist()}")
        assert np.isnan(ref[1]).all()
        assert np.isnan(got[1]).all(), f"NaN at {pos}: channel 1 = {got[1].tolist()}, every statistic must be NaN"
        assert np.array_equal(got[[0, 2]], clean[[0, 2]])               # the other channels to the bit
    inf = x.clone()
    inf[2, 1, 8, 8] = math.inf
    got, ref = run_stats(L, inf, fill=-7.0), D.stats_ref(inf.numpy())
    assert got[1, 0] == ref[1, 0] == clean[1, 0] and got[1, 1] == math.inf and got[1, 2] == math.inf and np.isnan(got[1, 3])
    assert np.array_equal(got[1], ref[1], equal_nan=True)
    assert np.array_equal(got[[0, 2]], clean[[0, 2]])
    both = inf.clone()
    both[4, 1, 0, 3] = -math.inf                                         # both signs: min -inf, max +inf, mean and std NaN
    got, ref = run_stats(L, both, fill=-7.0), D.stats_ref(both.numpy())
    assert np.array_equal(got[1], ref[1], equal_nan=True) and got[1, 0] == -math.inf and got[1, 1] == math.inf
    assert np.isnan(got[1, 2:]).all() and np.array_equal(got[[0, 2]], clean[[0, 2]])


# ----------------------------------------------------------------------------------------------------------------- gather
def run_gather(L, src, idx, A, B, src_offset=0, out_offset=0):
    """gsd_gather_affine on src (M, C, HW) fp32 (CPU) -> (B, C, HW) fp64 (CPU).  Rows no valid index names hold NaN on the device;
    src / out start `offset` floats into their buffers (1 breaks the 16-byte alignment of the vector form)."""
    m, c, hw = src.shape
    named = {i for i in idx if 0 <= i < m}
    sbuf = torch.full((src_offset + src.numel(),), math.nan, device="cuda")
    sd = sbuf[src_offset:].view(m, c, hw)
    for i in named:
        sd[i] = src[i].cuda()
    numel = len(idx) * c * hw
    obuf = nan_out(out_offset + numel)
    if out_offset:
        obuf[:out_offset] = 1234.5
    od = obuf[out_offset:]
    assert sbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
    a = torch.tensor(A, dtype=torch.float32, device="cuda")
    b = torch.tensor(B, dtype=torch.float32, device="cuda")
    i64 = torch.tensor(idx, dtype=torch.int64, device="cuda")
    L.check(L.lib.gsd_gather_affine(sd.data_ptr(), i64.data_ptr(), m, len(idx), c, hw, a.data_ptr(), b.data_ptr(), a.numel(),
                                    od.data_ptr(), L.stream_ptr()), "gather_affine")
    torch.cuda.synchronize()
    assert bool((obuf[:out_offset] == 1234.5).all()) and bool((od[numel:] == 1234.5).all()), "write outside the output"
    return od[:numel].reshape(len(idx), c, hw).cpu().double()


def gather_source(m, c, hw):
    return torch.randn((m, c, hw), generator=torch.Generator().manual_seed(hw)) * 3 + 0.5


def same_rows(got, ref, rows):
    return all(torch.equal(got[r], ref[r]) for r in rows)


@pytest.mark.parametrize("hw", [1, 4, 130, 1023, 1024, 1025, 4100, 160 * 213])
def test_gather_affine_is_one_fmaf_bit_for_bit(L, hw):
    src = gather_source(5, 3, hw)
    for idx, A, B in (([3, 0, 3, 1], [0.3, -1.1, 2.5], [-1.7, 0.4, 9.0]), ([4], [-0.7], [0.1]), ([1, 1], [1.0], [0.0])):
        got = run_gather(L, src, idx, A, B)
        ref, _ = D.gather_affine_ref(src.view(5, 3, hw, 1), idx, A, B)
        assert torch.equal(got, ref.view(len(idx), 3, hw)), (hw, idx, float((got - ref.view(len(idx), 3, hw)).abs().max()))
    assert torch.equal(run_gather(L, src, [1, 1], [1.0], [0.0])[1], src[1].double())


@pytest.mark.parametrize("offsets", [(1, 0), (0, 1), (1, 1), (3, 2)], ids=str)
def test_gather_affine_misaligned_pointers_take_the_scalar_form(L, offsets):
    """HW % 4 == 0 with a pointer that is not 16-byte aligned: a vector load or store there is wrong, the scalar form is due."""
    hw = 1024
    src = gather_source(5, 3, hw)
    idx, A, B = [2, 4, 2, 0], [0.3, -1.1, 2.5], [-1.7, 0.4, 9.0]
    got = run_gather(L, src, idx, A, B, src_offset=offsets[0], out_offset=offsets[1])
    assert torch.equal(got, D.gather_affine_ref(src.view(5, 3, hw, 1), idx, A, B)[0].view(4, 3, hw))


@pytest.mark.parametrize("hw", [1024, 1025])
def test_gather_affine_out_of_range_indices_give_nan_rows(L, hw):
    """DeviceDataset.batch raises before it launches; the kernel's own guard answers NaN and reads nothing out of bounds."""
    src = gather_source(4, 3, hw)
    idx = [1, -1, 2, 4, 0, -2 ** 40, 2 ** 40, 3]
    got = run_gather(L, src, idx, [0.3, -1.1], [-1.7, 0.4])
    ref = D.gather_affine_ref(src.view(4, 3, hw, 1), idx, [0.3, -1.1], [-1.7, 0.4])[0].view(len(idx), 3, hw)
    assert torch.isnan(got[[1, 3, 5, 6]]).all() and torch.isnan(ref[[1, 3, 5, 6]]).all()
    assert same_rows(got, ref, [0, 2, 4, 7])
