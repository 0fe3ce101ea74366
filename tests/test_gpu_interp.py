"""GPU parity for interp_method beyond 'area' (gsd_resize.hip): gsd_resize_affine / gsd_ingest_images_interp against
F.interpolate on the CPU (the reference's own call, image_utils.py:12-15), then predict_depth_from_RGB and DeviceDataset
with config.interp_method / interp_method set.

Nearest modes copy a pixel: bit-equal.  Bilinear and bicubic are checked element by element,
    |got - ref| <= TAU * (|A| * sum_k |w_k| |v_k| + |B|),   |v| = (|x| + |base| + 255) / 2 with a base, else |x|,
ref = A * sum_k w_k pre(x)_k + B in fp64 (difference image, taps and affine), with the fp32 weights w_k that F.interpolate
uses, read off it by resizing one-hot rows.  (F.interpolate in fp64 is no reference for them: it places the source
coordinate in fp64, which moves a weight by up to ~1e-5 -- far more than the fp32 rounding this bound is about.)
For a plain resize whose output has OH + OW > 128 (ATen's generic NCHW kernel) the result is also bit-equal to
F.interpolate in fp32: gsd_resize.hip restates that kernel's arithmetic, FMA contractions included."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l1
from gelslim_depth_amd import synth

pytestmark = pytest.mark.gpu

MODES = ("nearest", "nearest-exact", "bilinear", "bicubic")
CODE = {"area": 0, "nearest": 1, "nearest-exact": 2, "bilinear": 3, "bicubic": 4}
# (H, W) -> (OH, OW): the shipped config, the depth back to the camera, non-integer ratios both ways, identity, 1-pixel
# edges, an exact 2x upscale
SHAPES = (((320, 427), (160, 213)), ((160, 213), (320, 427)), ((21, 27), (40, 53)), ((80, 107), (40, 53)),
          ((33, 50), (20, 31)), ((17, 23), (17, 23)), ((1, 1), (3, 4)), ((5, 1), (1, 7)), ((40, 53), (80, 106)))
# largest measured |got - ref| / (|A| sum|w| |v| + |B|) over every case of this file: 2.3e-7 (bicubic, 160x213 -> 320x427)
TAU = 8e-7
SENTINEL = 1234.5


def weights(mode, n, m):
    """(m, n) fp64 matrix of the fp32 weights F.interpolate gives each input pixel (taps that clamp to the same pixel
    add up), read off ATen by resizing one-hot rows."""
    eye = torch.eye(n, dtype=torch.float32).reshape(n, 1, 1, n)
    return F.interpolate(eye, size=(1, m), mode=mode)[:, 0, 0, :].double().numpy().T


def taps64(mode, p, size, absolute=False):
    """sum_k w_k v_k (or sum_k |w_k v_k|) per output element in fp64 for p (N, C, H, W): the separable weights of F.interpolate
    applied as (OH, H) and (OW, W) matrices."""
    wh, ww = weights(mode, p.shape[2], size[0]), weights(mode, p.shape[3], size[1])
    if absolute:
        wh, ww, p = np.abs(wh), np.abs(ww), np.abs(p)
    return wh @ p @ ww.T


def pre64(x, base):
    x = x.double()
    return x if base is None else (x - base.double() + 255.0) * 0.5


def nan_out(numel):
    buf = torch.full((numel + 64,), float("nan"), device="cuda")
    buf[numel:] = SENTINEL
    return buf


def check_out(buf, numel):
    assert torch.all(buf[numel:] == SENTINEL), "write past the end of the output"
    out = buf[:numel]
    assert not torch.isnan(out).any(), "an output element was not written"
    return out


def run_resize_affine(mode, x, base, size, A, B):
    from gelslim_depth_amd import _lib as L
    n, c, h, w = x.shape
    numel = n * c * size[0] * size[1]
    buf = nan_out(numel)
    a = torch.tensor(A, dtype=torch.float32, device="cuda")
    b = torch.tensor(B, dtype=torch.float32, device="cuda")
    xd = x.cuda().contiguous()
    bd = None if base is None else base.cuda().contiguous()
    L.check(L.lib.gsd_resize_affine(CODE[mode], xd.data_ptr(), L.ptr(bd), n, c, h, w, buf.data_ptr(), size[0], size[1],
                                    a.data_ptr(), b.data_ptr(), a.numel(), 255.0, 0.5, L.stream_ptr()), "resize_affine")
    torch.cuda.synchronize()
    return check_out(buf, numel).reshape(n, c, *size).cpu()


def run_ingest(mode, raw, base, c0, c1, size):
    """The finger split of DeviceDataset: channels [c0, c1) of a 6-channel object, passed by stride."""
    from gelslim_depth_amd import _lib as L
    k, c, h, w = raw.shape
    numel = k * (c1 - c0) * size[0] * size[1]
    buf = nan_out(numel)
    rd = raw.cuda().contiguous()
    bd = None if base is None else base.cuda().contiguous()
    L.check(L.lib.gsd_ingest_images_interp(
        CODE[mode], rd.data_ptr() + c0 * h * w * rd.element_size(),
        None if bd is None else bd.data_ptr() + c0 * h * w * bd.element_size(), 0 if raw.dtype == torch.float32 else 1,
        k, c1 - c0, h, w, c * h * w, h * w, c * h * w, h * w, buf.data_ptr(), size[0], size[1], 255.0, 0.5,
        L.stream_ptr()), "ingest_images_interp")
    torch.cuda.synchronize()
    return check_out(buf, numel).reshape(k, c1 - c0, *size).cpu()


def bound_ratio(mode, got, x, base, size, A, B):
    """max |got - ref| / (|A| sum|w| |v| + |B|) with ref in fp64; A, B per channel.  With a base the magnitude of a tap is
    that of the terms of its difference image, (|x| + |base| + 255) / 2: the fp32 difference image cancels."""
    a = np.array(A, np.float64)[None, :, None, None]
    b = np.array(B, np.float64)[None, :, None, None]
    p = pre64(x, base).numpy()
    mag = np.abs(p) if base is None else (x.double().abs() + base.double().abs() + 255.0).numpy() * 0.5
    ref = a * taps64(mode, p, size) + b
    scale = np.abs(a) * taps64(mode, mag, size, absolute=True) + np.abs(b)
    err = np.abs(got.double().numpy() - ref)
    assert np.all(np.isfinite(err))
    return float((err / np.maximum(scale, 1e-300)).max()), ref, scale


def images(seed, n, c, h, w, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, c, h, w), generator=g, dtype=torch.int32)
    if dtype == torch.uint8:
        return x.to(torch.uint8)
    return x.float() + torch.rand((n, c, h, w), generator=g)     # not integer-valued: every weight shows


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_resize_affine_vs_torch_cpu(mode, shape):
    (h, w), size = shape
    x, base = images(1, 2, 3, h, w), images(2, 2, 3, h, w)
    # plain resize: nearest modes copy, the generic-kernel sizes of bilinear / bicubic reproduce ATen's fp32 bits
    got = run_resize_affine(mode, x, None, size, [1.0], [0.0])
    ref32 = F.interpolate(x, size=size, mode=mode)
    if mode.startswith("nearest") or size[0] + size[1] > 128:
        assert torch.equal(got, ref32), float((got - ref32).abs().max())
    ratio, _, _ = bound_ratio(mode, got, x, None, size, [1.0] * 3, [0.0] * 3)
    assert ratio <= TAU, ratio
    # difference image + resize + per-channel affine (the inference pre step; the post step is the 1-channel form)
    A, B = [1 / 40.0, 1 / 50.0, 1 / 60.0], [-3.0, -2.2, -2.1]
    got = run_resize_affine(mode, x, base, size, A, B)
    ratio, _, _ = bound_ratio(mode, got, x, base, size, A, B)
    assert ratio <= TAU, ratio
    print(f"[interp] resize_affine {mode} {shape}: max ratio {ratio:.3g}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_ingest_finger_split_vs_torch_cpu(mode, dtype, shape):
    (h, w), size = shape
    raw, base = images(3, 2, 6, h, w, dtype), images(4, 2, 6, h, w, dtype)
    for c0 in (0, 3):
        for b in (None, base):
            got = run_ingest(mode, raw, b, c0, c0 + 3, size)
            p32 = raw[:, c0:c0 + 3].float()
            if b is not None:
                p32 = (p32 - b[:, c0:c0 + 3].float() + 255.0) / 2.0      # the oracle's fp32 difference image
            ref32 = F.interpolate(p32, size=size, mode=mode)
            if mode.startswith("nearest") or size[0] + size[1] > 128:
                assert torch.equal(got, ref32), (c0, b is None, float((got - ref32).abs().max()))
            ratio, _, _ = bound_ratio(mode, got, raw[:, c0:c0 + 3], None if b is None else b[:, c0:c0 + 3], size,
                                      [1.0] * 3, [0.0] * 3)
            assert ratio <= TAU, (c0, b is None, ratio)
            print(f"[interp] ingest {mode} {raw.dtype} {shape} c0={c0} base={b is not None}: max ratio {ratio:.3g}")


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_bound_rejects_one_tap_and_one_weight_mutations(mode):
    """The element-wise bound is tight enough to see a kernel that reads one wrong tap or gets one weight wrong by the
    amount that separates ATen's FMA source coordinate from a plain multiply-add (~1e-5)."""
    (h, w), size = (320, 427), (160, 213)
    x = images(5, 1, 2, h, w)
    got = run_resize_affine(mode, x, None, size, [1.0], [0.0])
    p = x.double().numpy()
    ratio, ref, scale = bound_ratio(mode, got, x, None, size, [1.0] * 2, [0.0] * 2)
    assert ratio <= TAU
    ww = weights(mode, w, size[1])
    wh = weights(mode, h, size[0])
    ow = 57
    taps = np.nonzero(ww[ow])[0]
    # one tap: output column ow reads its last tap one pixel further right
    moved = ww.copy()
    moved[ow, taps[-1] + 1] += moved[ow, taps[-1]]
    moved[ow, taps[-1]] = 0.0
    # one weight: the largest tap of column ow off by 1e-5 relative, a neighbour compensating (taps still sum to 1)
    bent = ww.copy()
    i = taps[np.argmax(np.abs(ww[ow, taps]))]
    d = 1e-5 * abs(bent[ow, i])
    bent[ow, i] += d
    bent[ow, i + 1 if i + 1 in taps else i - 1] -= d
    for name, wm in (("tap", moved), ("weight", bent)):
        mutated = wh @ p @ wm.T
        bad = np.abs(mutated - ref) / scale
        assert bad.max() > TAU, (name, bad.max())
        assert np.all(bad[..., np.arange(size[1]) != ow] <= TAU)       # only the mutated column fails


def test_area_mode_forwards_to_the_area_kernels():
    from gelslim_depth_amd import processing as pp
    x, base = images(6, 2, 3, 40, 53), images(7, 2, 3, 40, 53)
    want = pp.area_resize_affine(x.cuda(), (21, 27), [0.5, 0.25, 2.0], [1.0, 0.0, -1.0], base=base.cuda()).cpu()
    assert torch.equal(run_resize_affine("area", x, base, (21, 27), [0.5, 0.25, 2.0], [1.0, 0.0, -1.0]), want)
    assert torch.equal(pp.resize_affine(x.cuda(), (21, 27), [0.5, 0.25, 2.0], [1.0, 0.0, -1.0], base=base.cuda(),
                                        mode="area").cpu(), want)
    raw = images(8, 2, 6, 40, 53, torch.uint8)
    got = run_ingest("area", raw, None, 3, 6, (20, 26))
    assert torch.equal(got, F.interpolate(raw[:, 3:6].float(), size=(20, 26), mode="area"))


@pytest.mark.parametrize("mode", MODES)
def test_sample_multi_channel_image_to_desired_size(mode):
    from gelslim_depth_amd import processing as pp
    x = images(9, 2, 3, 160, 213)
    got = pp.sample_multi_channel_image_to_desired_size(x.cuda(), (320, 427), interp_method=mode).cpu()
    assert torch.equal(got, F.interpolate(x, size=(320, 427), mode=mode))


@pytest.mark.parametrize("mode", ["bilinear", "bicubic", "nearest"])
def test_predict_depth_from_rgb_follows_config_interp_method(mode):
    """predict_depth_from_RGB with cfg.interp_method: both resizes follow it (test_depth_estimation.py:14-20)."""
    from gelslim_depth_amd import processing as pp
    from gelslim_depth_amd.models.unet import UNet
    from oracle import processing_ref as pr
    from oracle import unet_numpy as on
    dims = [8, 16, 32]
    st = synth.make_state(3, 1, dims, 21, "conditioned")
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=dims)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    m = m.to("cuda").eval()
    dparams = (-1.9180814027786255, 0.0)
    cfg = types.SimpleNamespace(input_tactile_image_size=(40, 53), interp_method=mode,
                                image_normalization_method="0_255_to_0_1", image_normalization_parameters=None,
                                depth_normalization_method="min_max_to_0_-1", depth_normalization_parameters=dparams,
                                norm_scale=0.9)
    rng = np.random.default_rng(5)
    img = rng.uniform(0, 255, (2, 3, 80, 107)).astype(np.float32)
    base = rng.uniform(0, 255, (2, 3, 80, 107)).astype(np.float32)
    got = pp.predict_depth_from_RGB(torch.from_numpy(img).cuda(), m, (80, 107), cfg,
                                    base_images=torch.from_numpy(base).cuda()).cpu().numpy()

    def resize(a, size):
        return F.interpolate(torch.from_numpy(np.ascontiguousarray(a)), size=size, mode=mode).numpy()
    x = pr.normalize_tactile(resize(pr.difference_image(img, base), (40, 53)), "0_255_to_0_1", 0.9)
    d = on.UNetOracle(st).forward(x.astype(np.float32), train=False)
    ref = resize(pr.denormalize_depth(d, "min_max_to_0_-1", 0.9, dparams), (80, 107))
    assert rel_l1(got, ref) < 1e-4, rel_l1(got, ref)
    area = pp.predict_depth_from_RGB(torch.from_numpy(img).cuda(), m, (80, 107),
                                     types.SimpleNamespace(**{**vars(cfg), "interp_method": "area"}),
                                     base_images=torch.from_numpy(base).cuda()).cpu().numpy()
    assert rel_l1(area, ref) > 1e-3           # the mode is visible in the answer


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kw", [dict(separate_fingers=True, depth_image_blur_kernel=3, use_difference_image=True),
                                dict(separate_fingers=False, depth_image_blur_kernel=1, use_difference_image=False)],
                         ids=["split-blur3-diff", "whole"])
def test_device_dataset_interp_method_vs_oracle(mode, kw, monkeypatch):
    from gelslim_depth_amd.dataset import DeviceDataset
    from oracle import dataset_ref as dr
    kw = dict(kw, image_normalization_method="0_255_to_0_1", depth_normalization_method="min_max_to_0_-1", norm_scale=0.9)
    objs = dr.synthetic_objects(41, [3, 2], h=42, w=54)
    ds = DeviceDataset(objects=objs, device="cuda", interp_method=mode, **kw)
    monkeypatch.setattr(dr, "resize", lambda x, size: F.interpolate(x, size=size, mode=mode))
    ref = dr.DatasetOracle(objs, **kw)
    assert ds.input_tactile_image_size == ref.input_tactile_image_size == (21, 27)
    t_got, t_ref = ds.entire_dataset["tactile_image"].cpu(), ref.entire_dataset["tactile_image"]
    d_got, d_ref = ds.entire_dataset["depth_image"].cpu(), ref.entire_dataset["depth_image"]
    if mode.startswith("nearest"):
        assert torch.equal(t_got, t_ref)
    assert (t_got - t_ref).abs().max() <= 1e-4          # 0..255 images: a few fp32 ulps
    assert (d_got - d_ref).abs().max() <= 2e-6          # depth in [-2, 0], blurred after the resize
    assert np.allclose(np.array(ds.depth_normalization_parameters), np.array(ref.depth_normalization_parameters),
                       rtol=2e-6, atol=1e-6)
    for i in (0, len(ds) - 1):
        a, b = ds[i], ref[i]
        assert np.abs(a["tactile_image"].cpu().numpy() - b["tactile_image"].numpy()).max() <= 2e-6
        assert np.abs(a["depth_image"].cpu().numpy() - b["depth_image"].numpy()).max() <= 2e-6
