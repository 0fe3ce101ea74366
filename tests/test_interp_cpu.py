"""CPU: interp_method validation (processing, DeviceDataset) and the argument checks of gsd_resize_affine /
gsd_ingest_images_interp.  Every call here is refused before anything touches a device."""
import ctypes

import pytest
import torch

ACCEPTED = ("area", "nearest", "nearest-exact", "bilinear", "bicubic")


def test_interp_mode_codes_match_the_header():
    import os
    import re
    from conftest import REPO
    from gelslim_depth_amd import processing as pp
    hdr = open(os.path.join(REPO, "include", "gsd.h")).read()
    codes = {m.lower().replace("_", "-"): int(v) for m, v in re.findall(r"GSD_INTERP_([A-Z_]+) = (\d+)", hdr)}
    assert codes == pp.INTERP_MODES
    assert tuple(pp.INTERP_MODES) == ACCEPTED
    for m in ACCEPTED:
        assert pp.interp_mode(m) == pp.INTERP_MODES[m]


@pytest.mark.parametrize("bad", ["linear", "trilinear", "Bilinear", "bilinear ", "", None, 3])
def test_unknown_mode_raises_naming_the_accepted_ones(bad):
    from gelslim_depth_amd import processing as pp
    from gelslim_depth_amd.dataset import DeviceDataset
    from oracle import dataset_ref as dr
    x = torch.zeros(1, 3, 8, 8)
    calls = [lambda: pp.interp_mode(bad),
             lambda: pp.sample_multi_channel_image_to_desired_size(x, (4, 4), interp_method=bad),
             lambda: pp.resize_affine(x, (4, 4), [1.0], [0.0], mode=bad)]
    if bad is not None:     # None is DeviceDataset's default: 'area'
        calls.append(lambda: DeviceDataset(objects=dr.synthetic_objects(1, [1]), interp_method=bad, device="cuda"))
    for call in calls:
        with pytest.raises(NotImplementedError) as e:
            call()
        for m in ACCEPTED:
            assert repr(m) in str(e.value)


def test_predict_depth_validates_config_interp_method():
    import types
    from gelslim_depth_amd import processing as pp
    cfg = types.SimpleNamespace(input_tactile_image_size=(4, 4), interp_method="linear",
                                image_normalization_method="0_255_to_0_1", norm_scale=0.9,
                                depth_normalization_method="min_max_to_0_-1", depth_normalization_parameters=(-1.0, 0.0))
    with pytest.raises(NotImplementedError, match="'bicubic'"):
        pp.predict_depth_from_RGB(torch.zeros(1, 3, 8, 8), None, (8, 8), cfg)


def test_accepted_modes_still_refuse_cpu_tensors():
    from gelslim_depth_amd import _lib as L
    from gelslim_depth_amd import processing as pp
    for m in ACCEPTED:
        with pytest.raises(L.GsdError, match="needs GPU tensors"):
            pp.sample_multi_channel_image_to_desired_size(torch.zeros(1, 3, 8, 8), (4, 4), interp_method=m)


def test_abi_refuses_bad_mode_and_bad_sizes():
    """Return codes of the two entry points for arguments they refuse before any launch (fake, never dereferenced
    pointers where a pointer must be non-null)."""
    from gelslim_depth_amd._lib import lib
    P = 4096
    BAD, UNSUP = -1, -2
    # gsd_resize_affine(mode, in, base, N, C, H, W, out, OH, OW, A, B, nab, pre_add, pre_mul, stream)
    ok = dict(mode=3, inp=P, base=None, N=2, C=3, H=8, W=8, out=P, OH=4, OW=4, A=P, B=P, nab=1)

    def ra(**kw):
        a = dict(ok, **kw)
        return lib.gsd_resize_affine(a["mode"], a["inp"], a["base"], a["N"], a["C"], a["H"], a["W"], a["out"], a["OH"],
                                     a["OW"], a["A"], a["B"], a["nab"], 255.0, 0.5, None)
    for mode in (-1, 5, 99):
        assert ra(mode=mode) == BAD
        assert b"unknown mode" in lib.gsd_last_error()
    for mode in range(5):       # area forwards to gsd_area_resize_affine, which refuses the same way
        assert ra(mode=mode, inp=None) == BAD
        assert ra(mode=mode, OH=0) == BAD
        assert ra(mode=mode, W=-3) == BAD
        assert ra(mode=mode, nab=0) == BAD
        assert ra(mode=mode, N=70000) == UNSUP
    assert ra(H=1 << 16, W=1 << 16) == UNSUP

    def ing(mode=3, inp=P, dtype=1, N=2, C=3, H=8, W=8, cs=64, out=P, OH=4, OW=4):
        return lib.gsd_ingest_images_interp(mode, inp, None, dtype, N, C, H, W, C * cs, cs, 0, 0, out, OH, OW, 255.0, 0.5,
                                            None)
    for mode in (-1, 5):
        assert ing(mode=mode) == BAD
    for mode in range(5):
        assert ing(mode=mode, out=None) == BAD
        assert ing(mode=mode, OW=0) == BAD
        assert ing(mode=mode, cs=63) == BAD            # channel stride smaller than a plane
        assert ing(mode=mode, dtype=2) == UNSUP
        assert ing(mode=mode, C=70000) == UNSUP
    assert isinstance(lib.gsd_last_error(), (bytes, ctypes.c_char_p))
