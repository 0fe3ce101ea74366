"""CPU-side checks of the input-gradient feature: what gsd_conv3x3_dgrad_bn says it serves, the reference fixture, and the module's
CPU refusal (the kernels and the module's gradients themselves: tests/test_gpu_input_grad.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def test_dgrad_bn_supported_reports_its_shapes():
    from gelslim_depth_amd._lib import lib
    for n in (1, 2, 32, 64):
        assert lib.gsd_conv3x3_dgrad_bn_supported(n, 320, 427, 3, 64) == 1
    assert lib.gsd_conv3x3_dgrad_bn_supported(3, 37, 45, 3, 16) == 1       # the small test network's first layer
    assert lib.gsd_conv3x3_dgrad_bn_supported(1, 1, 1, 1, 1) == 1
    assert lib.gsd_conv3x3_dgrad_bn_supported(2, 320, 427, 4, 64) == 0     # Cin * 9 > 32: the direct-form fallback
    assert lib.gsd_conv3x3_dgrad_bn_supported(2, 320, 427, 3, 65536) == 0
    for bad in ((0, 8, 8, 3, 64), (1, 0, 8, 3, 64), (1, 8, 0, 3, 64), (1, 8, 8, 0, 64), (1, 8, 8, 3, 0)):
        assert lib.gsd_conv3x3_dgrad_bn_supported(*bad) == 0


def test_dgrad_bn_refuses_what_it_does_not_serve():
    from gelslim_depth_amd._lib import lib
    rc = lib.gsd_conv3x3_dgrad_bn(8, None, None, None, None, None, None, 8, 4, 64, 8, 2, 8, 8, None)   # (never launched)
    assert rc == -2 and b"Cin" in lib.gsd_last_error()


def test_input_grad_fixture_keys_finite():
    d = np.load(os.path.join(GOLDEN, "ginput_grad.npz"))
    keys = set(d.files)
    for k in ("small/seed", "small/nhw", "small/train/y", "small/train/xgrad", "small/eval/y", "small/eval/xgrad",
              "full/train/xgrad_sums", "full/train/xgrad_samples", "full/eval/xgrad_sums", "full/eval/xgrad_samples"):
        assert k in keys, k
    from gelslim_depth_amd.models.unet import UNet
    names = [n for n, _ in UNet(3, 1, layer_dimensions=[int(v) for v in d["small/dims"]]).named_parameters()]
    for mode in ("train", "eval"):
        for n in names:
            for part in ("gradsum", "gradidx", "gradsample"):
                assert f"small/{mode}/{part}/{n}" in keys, (mode, part, n)
    assert d["small/train/xgrad"].shape == tuple(int(v) for v in (d["small/nhw"][0], 3, d["small/nhw"][1], d["small/nhw"][2]))
    for k in d.files:
        if d[k].dtype.kind == "f":
            assert np.isfinite(d[k]).all(), k
    # train and eval differ (eval-mode BatchNorm uses the running statistics)
    assert not np.allclose(d["small/train/xgrad"], d["small/eval/xgrad"])


def test_module_refuses_cpu_tensors_with_input_grad():
    from gelslim_depth_amd.models.unet import UNet
    m = UNet(3, 1, layer_dimensions=[4, 8])
    x = torch.zeros(1, 3, 8, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU"):
        m(x=x)
    with pytest.raises(RuntimeError, match="GPU"):
        m.eval()(x=x)
