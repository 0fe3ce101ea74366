"""The 2-D dW planner ignores a GSD_WG2D_KX that names no k-step shape (gsd_wgrad_w2d.hip: plan_wg2d).  Only 1, 2 and 4 tiles
across are k-step shapes; any other value used to leave the shape unset and the planner divided by whatever was there.  Host
logic only: the queries read no device memory."""
import pytest

from gelslim_depth_amd import _lib as L

lib = L.lib
SHAPES = [(8, 80, 106, 256, 256), (3, 37, 53, 64, 64)]   # (N, H, W, Cin, Cout): both block forms, even and odd sizes


def plan(n, h, w, ci, co):
    return lib.gsd_conv3x3_wgrad_workspace(n, h, w, ci, co), lib.gsd_conv3x3_wgrad_mfma_count(2, n, h, w, ci, co)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("kx", ["3", "8"])
def test_invalid_kx_plans_as_unset(monkeypatch, shape, kx):
    monkeypatch.delenv("GSD_WG2D_KX", raising=False)
    want = plan(*shape)
    assert want[0] > 0 and want[1] > 0
    monkeypatch.setenv("GSD_WG2D_KX", kx)
    assert plan(*shape) == want


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_valid_kx_still_forces_the_shape(monkeypatch, shape):
    n, h, w, ci, co = shape
    per = 24 * (co // 16) * (ci // 16)
    for kx in (1, 2, 4):
        monkeypatch.setenv("GSD_WG2D_KX", str(kx))
        ksteps = n * -(-((h + 1) // 2) // (4 // kx)) * -(-((w + 3) // 4) // kx)
        assert lib.gsd_conv3x3_wgrad_mfma_count(2, n, h, w, ci, co) == ksteps * per
