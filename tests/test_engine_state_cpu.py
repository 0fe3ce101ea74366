"""The helper of the state-independence tests (engine_state.py), checked on the CPU: the poison lands, only where it should,
the originals come back, and same_bits() sees one ulp and a NaN."""
import math

import pytest
import torch

import engine_state as S

DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.int16]


def _allocators(dtype):
    like = torch.zeros((3, 5), dtype=dtype)
    return {"empty": lambda: torch.empty((3, 5), dtype=dtype),
            "empty_like": lambda: torch.empty_like(like),
            "new_empty": lambda: like.new_empty((2, 7))}


@pytest.mark.parametrize("pattern", S.PATTERNS)
def test_each_pattern_lands_in_every_dtype_of_all_three_functions(monkeypatch, pattern):
    p = S.poisoned(monkeypatch, pattern, device_type="cpu")
    n = 0
    for dtype in DTYPES:
        for name, make in _allocators(dtype).items():
            t = make()
            n += 1
            assert t.dtype == dtype and p.filled == n, name
            if dtype == torch.int16:
                assert bool((t == 0x5A5A).all()), (name, "every byte 0x5A")
            elif pattern == S.NAN:
                assert bool(torch.isnan(t).all()), (name, dtype)
            else:
                want = {S.ZERO: 0.0, S.BIG: 3.0e4}[pattern]
                assert bool((t.double() == float(torch.tensor(want, dtype=dtype))).all()), (name, dtype)
                assert bool(torch.isfinite(t).all()) and bool(torch.isfinite(t.float() * t.float()).all()), "BIG and its fp32 square are finite"
    # keyword and positional forms reach the original unchanged
    assert torch.empty(2, 3).shape == (2, 3) and torch.empty(size=(4,), dtype=torch.float64).dtype == torch.float64
    assert torch.empty_like(torch.zeros(2, dtype=torch.float64), dtype=torch.float32).dtype == torch.float32
    assert torch.empty((0,)).numel() == 0, "an empty tensor is not filled and does not fail"


def test_other_devices_are_left_alone(monkeypatch):
    p = S.poisoned(monkeypatch, S.NAN, device_type="cuda")         # (no GPU is touched: nothing is allocated there)
    for dtype in DTYPES:
        for make in _allocators(dtype).values():
            make()
    assert p.filled == 0, "CPU tensors under a cuda poison"
    q = S.poisoned(monkeypatch, S.BIG, device_type="cpu")
    m = torch.empty((3,), device="meta")
    assert m.device.type == "meta" and q.filled == 0
    assert bool((torch.empty((3,)) == 3.0e4).all()) and q.filled == 1


def test_the_originals_are_back_after_the_fixture_unwinds(monkeypatch):
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with S.poison(monkeypatch, S.BIG, device_type="cpu") as p:
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
        assert torch.empty.__wrapped__ is before[0]
        assert bool((torch.zeros(2).new_empty((4,)) == 3.0e4).all()) and p.filled == 1
        with S.poison(monkeypatch, S.ZERO, device_type="cpu"):      # the inner pattern fills last
            assert bool((torch.empty((4,)) == 0).all())
        assert bool((torch.empty((4,)) == 3.0e4).all())
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    assert "new_empty" not in torch.Tensor.__dict__ or torch.Tensor.__dict__["new_empty"] is before[2]


def test_same_bits_rejects_one_ulp_and_a_nan():
    a = torch.tensor([1.0, -2.5, 3.0e4], dtype=torch.float32)
    S.same_bits(a, a.clone(), "equal")
    b = a.clone()
    b[1] = torch.nextafter(b[1], torch.tensor(0.0))
    with pytest.raises(AssertionError, match="1 of 3 elements differ"):
        S.same_bits(a, b, "one ulp")
    for dtype in (torch.bfloat16, torch.float64):
        c = a.to(dtype)
        d = c.clone()
        d[0] = 1.0 + (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -52)      # the next number after 1.0 in either format
        with pytest.raises(AssertionError, match="differ in their bits"):
            S.same_bits(c, d, str(dtype))
    n = a.clone()
    n[2] = math.nan
    with pytest.raises(AssertionError, match="not finite"):
        S.same_bits(n, n.clone(), "equal NaNs are still rejected")
    S.same_bits(n, n.clone(), "unless the caller exempts the result", finite=False)
    with pytest.raises(AssertionError, match="differ in their bits"):
        S.same_bits(n, a, "a NaN against a number", finite=False)
    with pytest.raises(AssertionError, match="not finite"):
        S.same_bits(torch.tensor([math.inf]), torch.tensor([math.inf]), "inf")
    z = torch.tensor([0.0])
    with pytest.raises(AssertionError, match="differ in their bits"):
        S.same_bits(z, -z, "+0 against -0")
    with pytest.raises(AssertionError):
        S.same_bits(a, a.double(), "another dtype")
    S.same_bits(3, 3, "host integers")
    S.same_bits(0.5, 0.5, "host floats")
    with pytest.raises(AssertionError):
        S.same_bits(3, 4, "host integers that differ")
    with pytest.raises(AssertionError, match="k"):
        S.same_results({"k": a}, {"k": b}, "results")
    with pytest.raises(AssertionError):
        S.same_results({"k": a}, {"j": a}, "other names")
    S.same_results({"k": n}, {"k": n.clone()}, "exempt", not_finite=("k",))
