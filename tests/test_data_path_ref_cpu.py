"""The fp64 restatements of tests/data_path_ref.py against torch's own float64 operators, and the proof -- without a GPU --
that the bounds of tests/test_gpu_data_path_fp64.py reject a small local mistake: on every input that module launches, each
mutated reference leaves the true one by more than the pass bound at one element or more.  The bounds depend only on ref, cond
and the window size, so a kernel that computed a mutated reference would fail there."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import data_path_ref as D
from fp64_ref import U32
from test_gpu_interp import SHAPES

AREA_SHAPES = SHAPES + (D.AREA_EXTRA,)
ids = lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}"       # noqa: E731


def close(a, b, rel=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= rel * np.abs(b)))


@pytest.mark.parametrize("shape", AREA_SHAPES, ids=ids)
def test_area_ref_is_adaptive_avg_pool_and_interpolate_area(shape):
    for name, x, base, size, A, B in D.resize_cases(shape):
        ref, cond, n_e = D.area_ref(x, base, size, A, B)
        p = x.double() if base is None else (x.double() - base.double() + 255.0) * 0.5
        cc = torch.arange(3).clamp_max(len(A) - 1)
        a = torch.tensor(A, dtype=torch.float32).double()[cc].view(1, 3, 1, 1)
        b = torch.tensor(B, dtype=torch.float32).double()[cc].view(1, 3, 1, 1)
        assert close(ref, (a * F.adaptive_avg_pool2d(p, size) + b).numpy()), name
        assert close(ref, (a * F.interpolate(p, size=size, mode="area") + b).numpy()), name
        assert n_e.shape == size and n_e.min() >= 1 and np.all(cond >= np.abs(ref) * (1 - 1e-12)), name
        ones = D.area_ref(torch.ones_like(x), None, size, [1.0], [0.0])[0]
        assert close(ones, np.ones_like(ones)), name                   # every window is divided by its own count
    (h, w), size = shape
    assert n_e[-1, -1] == (h - ((size[0] - 1) * h) // size[0]) * (w - ((size[1] - 1) * w) // size[1])
    if shape == D.AREA_EXTRA:
        assert n_e.min() == 32 * 29 and n_e.max() == 32 * 30       # 86 / 3: the middle window overlaps both neighbours


@pytest.mark.parametrize("shape", AREA_SHAPES, ids=ids)
def test_area_bound_rejects_a_shifted_last_column_and_a_dropped_term(shape):
    cases = [(n, x, b, size, A, B) for n, x, b, size, A, B in D.resize_cases(shape)]
    cases += [(n, raw[:, c0:c0 + 3], None if b is None else b[:, c0:c0 + 3], size, [1.0], [0.0])
              for n, raw, b, c0, size in D.ingest_cases(shape)]
    assert len(cases) == 12
    for name, x, base, size, A, B in cases:
        ref, cond, n_e = D.area_ref(x, base, size, A, B)
        bound = D.area_bound(cond, n_e)
        shifted = D.area_ref_last_column_shifted(x, base, size, A, B)
        if x.shape[3] == 1:
            assert shifted is None          # one input column: there is no neighbouring column a window could take instead
        else:
            over = np.abs(shifted - ref) > bound
            assert over.any() and not over[..., :-1].any(), name       # the last output column fails and only it
        dropped, (oh, ow) = D.area_ref_one_term_dropped(x, base, size, A, B)
        over = np.abs(dropped - ref) > bound
        assert over.sum() == 1 and over[0, 0, oh, ow] and n_e[oh, ow] == n_e.max(), name


@pytest.mark.parametrize("case", D.BLUR_SHAPES + (D.BLUR_MANY,), ids=lambda c: "x".join(map(str, c)))
def test_blur_ref_is_reflect_pad_and_depthwise_conv_and_its_bound_rejects_mutations(case):
    n, c, h, w, k = case
    x, k2 = D.blur_input(n, c, h, w, k), D.gaussian_k2(k)
    assert k2.dtype == torch.float32 and torch.equal(k2, k2.t()) and abs(float(k2.double().sum()) - 1.0) < 1e-6
    ref, cond = D.blur_ref(x.numpy(), k2.numpy())
    r = k // 2
    xp = F.pad(x.double().reshape(n * c, 1, h, w), [r, r, r, r], mode="reflect") if r else x.double().reshape(n * c, 1, h, w)
    want = F.conv2d(xp, k2.double().view(1, 1, k, k)).reshape(n, c, h, w).numpy()
    assert np.all(np.abs(ref - want) <= 1e-12 * cond)
    assert np.all(cond >= np.abs(ref) * (1 - 1e-12))
    bound = D.blur_bound(cond, k)
    if k == 1:
        # no tap leaves the image: both mutations are the identity, and the GPU test asks for a bit-equal copy instead
        assert np.array_equal(ref, x.double().numpy())
        assert np.array_equal(D.blur_ref_edge_repeated(x.numpy(), k2.numpy()), ref)
        return
    over = np.abs(D.blur_ref_edge_repeated(x.numpy(), k2.numpy()) - ref) > bound
    assert over.any() and not over[..., r:h - r, r:w - r].any()         # pixels within r of a border, and only they
    sym = F.conv2d(torch.from_numpy(np.pad(x.double().numpy().reshape(n * c, 1, h, w), ((0, 0), (0, 0), (r, r), (r, r)),
                                           mode="symmetric")), k2.double().view(1, 1, k, k)).reshape(n, c, h, w).numpy()
    assert np.all(np.abs(D.blur_ref_edge_repeated(x.numpy(), k2.numpy()) - sym) <= 1e-12 * cond)
    bent, pos = D.blur_ref_one_pixel_shifted_kernel(x.numpy(), k2.numpy())
    over = np.abs(bent - ref) > bound
    assert over.sum() == 1 and over[pos]


def poke(x, values):
    """x with `values` written over the first elements of the last channel's first row."""
    x = x.clone()
    x[0, -1, 0, :len(values)] = torch.tensor(values, dtype=x.dtype)
    return x


STATS_SPECIAL = {"plain": [], "nan": [math.nan], "+inf": [math.inf], "-inf": [-math.inf], "+-inf": [math.inf, -math.inf]}


@pytest.mark.filterwarnings("ignore:std\\(\\). degrees of freedom")       # torch says so for a single element
@pytest.mark.parametrize("shape,special", [(s, k) for s in ((7, 3, 33, 31), (1, 2, 1, 5), (1, 1, 1, 1), (5, 3, 16, 16))
                                           for k in sorted(STATS_SPECIAL) if len(STATS_SPECIAL[k]) <= s[3]], ids=str)
def test_stats_ref_answers_as_torch_does(shape, special):
    x = poke(torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 2 + 3, STATS_SPECIAL[special])
    got = D.stats_ref(x.numpy())
    for c in range(shape[1]):
        ch = x[:, c]
        want = np.array([ch.min().item(), ch.max().item(), ch.mean().item(), ch.std().item()])
        assert np.array_equal(np.isnan(got[c]), np.isnan(want)), (c, got[c], want)
        assert np.array_equal(got[c, :2], want[:2], equal_nan=True)
        assert np.allclose(got[c, 2:], want[2:], rtol=1e-12, atol=0, equal_nan=True), (c, got[c], want)
    if special == "nan":
        assert np.isnan(got[-1]).all() and np.isfinite(got[:-1]).all()
    if shape == (1, 1, 1, 1) and special == "plain":
        assert got[0, 0] == got[0, 1] == got[0, 2] and np.isnan(got[0, 3])


def test_gather_affine_ref_is_one_fmaf_and_marks_bad_rows():
    g = torch.Generator().manual_seed(5)
    src = torch.randn((4, 3, 5, 7), generator=g) * 3
    for A, B in (([0.3], [-1.7]), ([0.3, -1.1, 2.5], [-1.7, 0.4, 9.0])):
        ref, cond = D.gather_affine_ref(src, [2, -1, 0, 4, 2], A, B)
        assert ref.dtype == torch.float64 and torch.equal(ref.float().double()[[0, 2, 4]], ref[[0, 2, 4]])   # fp32 values
        assert torch.isnan(ref[[1, 3]]).all() and torch.isnan(cond[[1, 3]]).all() and torch.equal(ref[0], ref[4])
        cc = [min(c, len(A) - 1) for c in range(3)]
        a = torch.tensor(A, dtype=torch.float32).double()[cc].view(3, 1, 1)
        b = torch.tensor(B, dtype=torch.float32).double()[cc].view(3, 1, 1)
        exact = src[2].double() * a + b
        assert bool(((ref[0] - exact).abs() <= U32 * exact.abs()).all())           # one correctly rounded fp32 result
        assert bool(((ref[0] - exact).abs() <= (exact.float().double() - exact).abs()).all())     # and the nearest one
