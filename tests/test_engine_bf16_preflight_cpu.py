"""UNetEngineBF16.preflight: a train-capable (n, h, w) whose backward the library would refuse -- the last ConvT dX carries the fused
BatchNorm-backward statistics on the large-tile kernel, which holds (N*H*W + 512) * pitch < 2^31 - 1 elements per operand
(gsd_bf16_ctgemm.hip gsd_ctgemm_operands) -- is refused BEFORE anything is launched, allocated or counted, instead of inside
backward() after the forward has updated every running statistic.  On the CPU, with no tensor: the pre-flight asks
gsd_bf16_conv_dense_fused_misfit with extents and pitches only."""
import pytest
import torch

import bf16_tile_cases as B
from gelslim_depth_amd import _lib as L
from gelslim_depth_amd.engine_bf16 import UNetEngineBF16

DIMS = [64, 128, 256, 512, 1024]
KNOBS = ("GSD_BF16_CTGEMM", "GSD_BF16_CT_BM")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def test_admits_122_and_refuses_123_at_320x427_with_the_default_dims():
    eng = UNetEngineBF16(3, 1, DIMS)
    assert (122 * 320 * 427 + 512) * 128 < 2 ** 31 - 1 <= (123 * 320 * 427 + 512) * 128
    eng.preflight(122, 320, 427)
    eng.preflight(1, 320, 427)
    with pytest.raises(L.GsdError) as e:
        eng.preflight(123, 320, 427)
    msg = str(e.value)
    # the operand, the limit and the largest batch that fits
    assert "up.3.up.weight" in msg and "in (the gradient slice of the concat buffer)" in msg and "123 x 136640 pixels at pitch 128" in msg
    assert "(N*H*W + 512) * pitch < 2^31 - 1" in msg and "largest batch that fits is 122" in msg
    with pytest.raises(L.GsdError, match="largest batch that fits is 122"):
        eng.preflight(4096, 320, 427)


def test_a_refused_batch_leaves_the_engine_as_it_was(monkeypatch):
    """_ensure(train) raises before the shape key, the buffer count or a buffer changes; eval-mode shapes are not asked."""
    eng = UNetEngineBF16(3, 1, [64, 128])
    cpu = torch.device("cpu")
    before = dict(vars(eng))
    with pytest.raises(L.GsdError, match="largest batch that fits is 122"):
        eng._ensure(123, 320, 427, cpu, True)
    assert vars(eng) == before and eng._shape is None and eng.buffers_made == 0 and eng.generation == 0 and not hasattr(eng, "cat")
    asked = []
    monkeypatch.setattr(eng, "preflight", lambda n, h, w: asked.append((n, h, w)))
    with pytest.raises(L.GsdError, match="CUDA"):     # (without a device the eval-mode sizing ends at its first gsd_nhwc view)
        eng._ensure(123, 8, 8, cpu, False)
    assert asked == [] and eng.buffers_made == 1          # an eval-mode forward is never asked
    with pytest.raises(L.GsdError, match="CUDA"):
        eng._ensure(2, 8, 8, cpu, True)
    assert asked == [(2, 8, 8)]


def served(dims, n, h, w):
    """The library's arithmetic restated (bf16_tile_cases.py): every ConvT dX of the net, with fused statistics, is served."""
    hs, ws = [h], [w]
    for _ in dims[1:]:
        hs.append(hs[-1] // 2)
        ws.append(ws[-1] // 2)
    for lvl in range(len(dims) - 1):
        cin, cout = dims[lvl + 1], dims[lvl + 1] // 2
        hi, wi = hs[lvl + 1], ws[lvl + 1]
        oy, ox = (hs[lvl] - 2 * hi) // 2, (ws[lvl] - 2 * wi) // 2
        if not B.ctgemm_shape(n, hi, wi, cout, cin, 4, 2, 0):
            continue
        out = B.Buf(n, hi, wi, cin)
        if not B.ctgemm_operands(B.Buf(n, hs[lvl], ws[lvl], dims[lvl] + cout), out, out, 4, [oy, oy, oy + 1, oy + 1], [ox, ox + 1, ox, ox + 1], hi, wi):
            return False
    return True


@pytest.mark.parametrize("d0", [32, 64, 128])
@pytest.mark.parametrize("h,w", [(320, 427), (160, 213), (64, 64), (37, 53)])
def test_agrees_with_the_library_arithmetic_over_a_grid(d0, h, w):
    """Batches 1 .. 700 and a few far beyond (a level of 2^24 pixels or more is no large-tile shape any more: the general kernel
    serves it, so `served` is not monotone in the batch)."""
    dims = [d0, 2 * d0, 4 * d0]
    eng = UNetEngineBF16(3, 1, dims)
    ok = {n: served(dims, n, h, w) for n in list(range(1, 701)) + [1 << 12, 1 << 16, 1 << 20]}
    assert ok[1] and (d0 == 32 or not all(ok.values()) or h * w < 64 * 64)
    first = next((n for n in sorted(ok) if not ok[n]), None)
    for n in sorted({1, 16, 122, 123, 700, 1 << 12, 1 << 16, 1 << 20} | ({first - 1, first, first + 1} if first and first < 700 else set())):
        if ok[n]:
            eng.preflight(n, h, w)
        else:
            largest = max((m for m in range(1, min(n, 701)) if ok[m]), default=0) if n <= 701 else None
            with pytest.raises(L.GsdError, match="largest batch that fits is " + (f"{largest}$" if largest is not None else r"\d+$")):
                eng.preflight(n, h, w)
