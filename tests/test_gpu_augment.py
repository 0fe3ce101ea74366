"""GPU: gsd_gather_augment, the batch gather with on-device augmentation, and what is built on it (DeviceDataset.batch,
DeviceLoader(augment=...), harness.fit).

Every launch here writes into NaN-filled outputs, and every row of the source arenas that the index vector does not name is
NaN: a skipped element or a stray read shows in the output.  Identity and geometry-only launches are held BITWISE to
gsd_gather_affine's batch (moved on the CPU with torch.flip / F.pad(mode="replicate") and the draws of gsd_augment_sample);
photometry and noise are held element-wise to the fp64 restatement of tests/augment_ref.py, |got - ref| <= TAU_AUG * cond.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as AR
from gelslim_depth_amd import synth

pytestmark = pytest.mark.gpu

# |got - ref| <= TAU_AUG * cond: no more than 4x the largest ratio measured on the MI355X, and below the ceiling 8 * 2^-24
# = 4.77e-7 (the chain has five fp32 roundings, each bounded by 2^-24 * cond).
# Largest ratio measured: 1.30e-7 (32x(3+1)x320x427, 0_255_to_-1_1, gain 0.2, offset 12, noise_std 3; with mean_std 1.24e-7, the
# odd shapes 3.0e-8 .. 1.0e-7).  4x that would pass the ceiling, so the ceiling decides: 3.5x the measured ratio.
TAU_AUG = 4.5e-7

#          B  Ci Cd  H    W   max_shift
SHAPES = [(32, 3, 1, 320, 427, (6, 9)),
          (5, 3, 1, 21, 27, (3, 4)),         # H*W % 4 != 0
          (3, 6, 2, 9, 11, (2, 3)),          # both fingers in one sample
          (2, 3, 1, 4, 5, (8, 8))]           # the clamp saturates
IDS = ["32x(3+1)x320x427", "5x(3+1)x21x27", "3x(6+2)x9x11", "2x(3+1)x4x5"]

MEAN_STD = ([1 / 41.3, 1 / 38.9, 1 / 45.2, 1 / 40.1, 1 / 37.7, 1 / 44.4], [-121.7 / 41.3, -130.2 / 38.9, -117.5 / 45.2,
                                                                           -119.9 / 40.1, -128.8 / 37.7, -123.1 / 44.4])
TO_PM1 = ([2.0 / 255.0], [-1.0])              # 0_255_to_-1_1: one (A, B) pair broadcast over the channels
DEPTH = ([-0.9 / 1.93], [-0.9 * 0.02 / 1.93])   # min_max_to_0_-1 with norm_scale 0.9


def _arena(b, ci, cd, h, w, seed, extra=8):
    """(img, dep, idx) on the GPU: M = b + extra rows, the b rows idx names hold data (raw image values in [0, 255), depth
    in [-2, 0]), every other row is NaN."""
    rng = np.random.default_rng(seed)
    m = b + extra
    idx = rng.permutation(m)[:b]
    img = np.full((m, ci, h, w), np.nan, np.float32)
    dep = np.full((m, cd, h, w), np.nan, np.float32)
    img[idx] = (255.0 * rng.random((b, ci, h, w))).astype(np.float32)
    dep[idx] = (-2.0 * rng.random((b, cd, h, w))).astype(np.float32)
    return torch.from_numpy(img).cuda(), torch.from_numpy(dep).cuda(), torch.from_numpy(idx).cuda()


def _dev(ab, n=None):
    a, b = (torch.tensor(v[:n] if n is not None and len(v) > 1 else v, dtype=torch.float32, device="cuda") for v in ab)
    return a, b


def _launch(img, dep, idx, ab_i, ab_d, augment, epoch=0):
    """gather_augment into NaN-filled outputs."""
    from gelslim_depth_amd.dataset import gather_augment
    out = (torch.full((idx.numel(), img.shape[1], *img.shape[2:]), float("nan"), device="cuda"),
           torch.full((idx.numel(), dep.shape[1], *img.shape[2:]), float("nan"), device="cuda"))
    got = gather_augment(img, dep, idx, *ab_i, *ab_d, augment, epoch, out=out)
    torch.cuda.synchronize()
    assert got[0] is out[0] and got[1] is out[1]
    return out


def _plain(img, dep, idx, ab_i, ab_d):
    from gelslim_depth_amd.dataset import gather_affine
    return gather_affine(img, idx, *ab_i), gather_affine(dep, idx, *ab_d)


def _params(augment, epoch_pivot=0.0):
    s = augment.spec()
    return AR.params(seed=s["seed"], p_hflip=s["hflip"], p_vflip=s["vflip"], max_dy=s["max_shift"][0], max_dx=s["max_shift"][1],
                     gain=s["gain"], offset=s["offset"], noise_std=s["noise_std"],
                     pivot=epoch_pivot if s["pivot"] is None else s["pivot"])


def _moved(batch, draws):
    """shift(flip(batch)) with edge replication, on the CPU with torch ops: batch (B, C, H, W), one draw per sample."""
    out = torch.empty_like(batch)
    h, w = batch.shape[2:]
    for b in range(batch.shape[0]):
        x = batch[b:b + 1]
        dims = [d for d, on in ((2, draws["vflip"][b]), (3, draws["hflip"][b])) if on]
        if dims:
            x = torch.flip(x, dims)
        dy, dx = int(draws["dy"][b]), int(draws["dx"][b])
        py, px = abs(dy), abs(dx)
        x = F.pad(x, (px, px, py, py), mode="replicate")
        out[b] = x[0, :, py - dy:py - dy + h, px - dx:px - dx + w]
    return out


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_identity_is_the_two_plain_gathers(shape):
    from gelslim_depth_amd.dataset import Augment
    b, ci, cd, h, w, _ = shape
    img, dep, idx = _arena(b, ci, cd, h, w, 1)
    for ab_i in (_dev(MEAN_STD, ci), _dev(TO_PM1)):
        want = _plain(img, dep, idx, ab_i, _dev(DEPTH))
        got = _launch(img, dep, idx, ab_i, _dev(DEPTH), Augment())
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_geometry_only_is_a_bitwise_permutation(shape):
    from gelslim_depth_amd.dataset import Augment
    b, ci, cd, h, w, shift = shape
    img, dep, idx = _arena(b, ci, cd, h, w, 2)
    ab_i, ab_d = _dev(MEAN_STD, ci), _dev(DEPTH)
    want = _plain(img, dep, idx, ab_i, ab_d)
    seen = {"hflip": set(), "vflip": set(), "dy": set(), "dx": set()}
    for seed, epoch in ((3, 0), (3, 1), (11, 5)):
        aug = Augment(seed=seed, hflip=0.5, vflip=0.5, max_shift=shift)
        draws = AR.lib_sample(_params(aug), epoch, idx.cpu().numpy(), ci)
        for k in seen:
            seen[k] |= set(draws[k].tolist())
        got = _launch(img, dep, idx, ab_i, ab_d, aug, epoch)
        assert _same_bits(got[0].cpu(), _moved(want[0].cpu(), draws)), (seed, epoch, "image")
        assert _same_bits(got[1].cpu(), _moved(want[1].cpu(), draws)), (seed, epoch, "depth")
    assert seen["hflip"] == seen["vflip"] == {False, True} and len(seen["dy"]) > 1 and len(seen["dx"]) > 1
    if b == 32:
        assert seen["dy"] == set(range(-shift[0], shift[0] + 1)) and len(seen["dx"]) > shift[1]
    # each knob alone
    for kw in (dict(hflip=1.0), dict(vflip=1.0), dict(max_shift=(shift[0], 0)), dict(max_shift=(0, shift[1]))):
        aug = Augment(seed=4, **kw)
        draws = AR.lib_sample(_params(aug), 2, idx.cpu().numpy(), ci)
        got = _launch(img, dep, idx, ab_i, ab_d, aug, 2)
        assert _same_bits(got[0].cpu(), _moved(want[0].cpu(), draws)) and _same_bits(got[1].cpu(), _moved(want[1].cpu(), draws)), kw


WORST = {}


def _check_photometry(shape, name, ab, aug, epoch, seed):
    b, ci, cd, h, w, _ = shape
    img, dep, idx = _arena(b, ci, cd, h, w, seed)
    ab_i, ab_d = _dev(ab, ci), _dev(DEPTH)
    got = _launch(img, dep, idx, ab_i, ab_d, aug, epoch)
    p, rows = _params(aug), idx.cpu().numpy()
    draws = AR.lib_sample(p, epoch, rows, ci)
    ref, cond = AR.gather_augment_ref(img.cpu().numpy(), rows, ab_i[0].cpu().numpy(), ab_i[1].cpu().numpy(), p, epoch, draws=draws)
    g = got[0].cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all() and np.isfinite(ref).all() and (cond > 0).all()
    ratio = np.abs(g - ref) / cond
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    key = f"{IDS[SHAPES.index(shape)]} {name} gain={aug.gain} offset={aug.offset} noise_std={aug.noise_std}"
    WORST[key] = float(ratio.max())
    print(f"TAU_AUG ratio {ratio.max():.4e} at {at}: {key}")
    assert ratio.max() <= TAU_AUG, (key, float(ratio.max()), at)
    # the augmentation is really there: far from the plain batch, and the noise has the asked standard deviation
    plain = _moved(_plain(img, dep, idx, ab_i, ab_d)[0].cpu(), draws).numpy().astype(np.float64)
    assert np.abs(g - plain).max() > 1e3 * TAU_AUG * cond.max()
    # depth: the same geometry as a geometry-only launch of the same (seed, epoch), untouched by the photometry
    from gelslim_depth_amd.dataset import Augment
    geo = Augment(seed=aug.seed, hflip=aug.hflip, vflip=aug.vflip, max_shift=aug.max_shift)
    assert _same_bits(got[1], _launch(img, dep, idx, ab_i, ab_d, geo, epoch)[1])


@pytest.mark.parametrize("norm", ["mean_std", "0_255_to_-1_1"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_photometry_and_noise_within_fp64_bound(shape, norm):
    from gelslim_depth_amd.dataset import Augment
    assert TAU_AUG < AR.CEILING
    ab = MEAN_STD if norm == "mean_std" else TO_PM1
    shift = shape[5]
    full = Augment(seed=21, hflip=0.5, vflip=0.5, max_shift=shift, gain=0.2, offset=12.0, noise_std=3.0, pivot=127.5)
    _check_photometry(shape, norm, ab, full, 3, 5)
    if shape[0] != 32:
        _check_photometry(shape, norm, ab, Augment(seed=22, max_shift=shift, gain=0.3, offset=5.0), 1, 6)      # no noise hash
        _check_photometry(shape, norm, ab, Augment(seed=23, hflip=0.5, noise_std=1.5), 0, 7)                  # noise alone
        _check_photometry(shape, norm, ab, Augment(seed=24, gain=0.1, pivot=0.0), 2, 8)                       # identity geometry


def test_keying_by_seed_epoch_and_row():
    from gelslim_depth_amd.dataset import Augment
    b, ci, cd, h, w = 32, 3, 1, 21, 27
    img, dep, idx = _arena(b, ci, cd, h, w, 9)
    ab_i, ab_d = _dev(MEAN_STD, ci), _dev(DEPTH)
    aug = Augment(seed=7, hflip=0.5, vflip=0.5, max_shift=(3, 4), gain=0.2, offset=8.0, noise_std=2.0, pivot=127.5)
    a = _launch(img, dep, idx, ab_i, ab_d, aug, 4)
    again = _launch(img, dep, idx, ab_i, ab_d, aug, 4)
    assert _same_bits(a[0], again[0]) and _same_bits(a[1], again[1])
    # neither the position in the batch nor the batch size matters
    perm = torch.randperm(b, generator=torch.Generator().manual_seed(3)).cuda()
    moved = _launch(img, dep, idx[perm], ab_i, ab_d, aug, 4)
    assert _same_bits(moved[0], a[0][perm]) and _same_bits(moved[1], a[1][perm])
    for k in range(b):
        one = _launch(img, dep, idx[k:k + 1], ab_i, ab_d, aug, 4)
        assert _same_bits(one[0][0], a[0][k]) and _same_bits(one[1][0], a[1][k]), k
    # another epoch, another seed: other bits, in every sample
    for other in (_launch(img, dep, idx, ab_i, ab_d, aug, 5),
                  _launch(img, dep, idx, ab_i, ab_d, Augment(**{**aug.spec(), "seed": 8}), 4)):
        assert all(not _same_bits(other[0][k], a[0][k]) for k in range(b))
        assert not _same_bits(other[1], a[1])


def test_out_of_range_index_gives_nan_rows():
    from gelslim_depth_amd.dataset import Augment
    b, ci, cd, h, w = 6, 3, 1, 21, 27
    img, dep, idx = _arena(b, ci, cd, h, w, 10, extra=0)          # every row holds data: only the bad indices may give NaN
    bad = idx.clone()
    bad[1], bad[4] = -1, img.shape[0]
    for aug in (Augment(), Augment(seed=1, hflip=0.5, max_shift=(2, 2)), Augment(seed=1, vflip=0.5, gain=0.1, noise_std=1.0)):
        got = _launch(img, dep, bad, _dev(MEAN_STD, ci), _dev(DEPTH), aug, 1)
        good = _launch(img, dep, idx, _dev(MEAN_STD, ci), _dev(DEPTH), aug, 1)
        for t, g in zip(got, good):
            for k in range(b):
                if k in (1, 4):
                    assert torch.isnan(t[k]).all(), k
                else:
                    assert torch.isfinite(t[k]).all() and _same_bits(t[k], g[k]), k


DS_KW = dict(use_difference_image=True, image_normalization_method="0_255_to_0_1", depth_normalization_method="min_max_to_0_-1",
             norm_scale=0.9)


def _datasets():
    from gelslim_depth_amd.dataset import DeviceDataset
    from oracle import dataset_ref as dr
    train = DeviceDataset(objects=dr.synthetic_objects(41, [3, 3], h=42, w=54), device="cuda", **DS_KW)
    val = DeviceDataset(objects=dr.synthetic_objects(42, [2], h=42, w=54), device="cuda",
                        depth_normalization_parameters=train.depth_normalization_parameters, **DS_KW)
    return train, val


def test_loader_shards_shuffle_and_default_pivot():
    from gelslim_depth_amd.dataset import Augment, DeviceLoader, gather_augment
    ds, _ = _datasets()
    assert len(ds) == 12
    aug = Augment(seed=5, hflip=0.5, vflip=0.5, max_shift=(2, 3), gain=0.2, offset=6.0, noise_std=2.0)
    keys = ("tactile_image", "depth_image", "object_index")

    def passes(loader, n=2):
        torch.manual_seed(17)
        return [[{k: v.clone() for k, v in batch.items()} for batch in loader] for _ in range(n)], torch.get_rng_state()
    whole, rng = passes(DeviceLoader(ds, 6, shuffle=True, augment=aug))
    ranks = [passes(DeviceLoader(ds, 3, shuffle=True, rank=r, world_size=2, augment=aug))[0] for r in (0, 1)]
    for e in range(2):
        assert len(whole[e]) == len(ranks[0][e]) == len(ranks[1][e]) == 2
        for i, batch in enumerate(whole[e]):
            for k in keys:
                assert _same_bits(torch.cat([ranks[0][e][i][k], ranks[1][e][i][k]]).float(), batch[k].float()), (e, i, k)
    # the second pass is another epoch: the same rows come out differently
    assert not _same_bits(torch.cat([b["tactile_image"] for b in whole[0]]), torch.cat([b["tactile_image"] for b in whole[1]]))
    # augmentation draws nothing from torch: same sample order, same generator state as the plain loader
    plain, rng_plain = passes(DeviceLoader(ds, 6, shuffle=True))
    assert torch.equal(rng, rng_plain)
    order = lambda run: [b["object_index"].tolist() for p in run for b in p]       # noqa: E731
    assert order(whole) == order(plain)
    # set_epoch overrides the epoch: a batch is ds.batch(its rows, aug, that epoch)
    torch.manual_seed(17)
    loader = DeviceLoader(ds, 6, shuffle=True, augment=aug)
    loader.set_epoch(1)
    torch.manual_seed(17)
    perm = DeviceLoader(ds, 6, shuffle=True).order().cuda()
    torch.manual_seed(17)
    for i, batch in enumerate(loader):
        direct = ds.batch(perm[6 * i:6 * i + 6], aug, 1)
        assert all(_same_bits(batch[k].float(), direct[k].float()) for k in keys)
        assert not _same_bits(batch["tactile_image"], whole[0][i]["tactile_image"])       # the same rows as epoch 0
        assert batch["object_index"].tolist() == whole[0][i]["object_index"].tolist()
    assert loader.epoch == 2
    # pivot=None on a difference-image dataset is 127.5
    tA, tB, dA, dB = ds._affines()
    idx = torch.arange(4, device="cuda")
    got = ds.batch(idx, aug, 3)
    want = gather_augment(ds.entire_dataset["tactile_image"], ds.entire_dataset["depth_image"], idx, tA, tB, dA, dB,
                          Augment(**{**aug.spec(), "pivot": 127.5}), 3)
    assert _same_bits(got["tactile_image"], want[0]) and _same_bits(got["depth_image"], want[1])
    other = gather_augment(ds.entire_dataset["tactile_image"], ds.entire_dataset["depth_image"], idx, tA, tB, dA, dB, aug, 3)
    assert not _same_bits(got["tactile_image"], other[0])                                  # pivot 0 there
    # ds.batch without augment is the code as it stands
    b0 = ds.batch(idx)
    assert _same_bits(b0["tactile_image"], ds.batch(idx, Augment(), 0)["tactile_image"])
    # evaluation walks are never augmented
    ev = DeviceLoader(ds, 3, rank=1, world_size=2, augment=aug)
    for (batch, valid, _), s in zip(ev.eval_shares(), (0, 6)):
        assert _same_bits(batch["tactile_image"], ds.batch(torch.arange(s + 3, s + 6))["tactile_image"])
    for batch, s in zip(ev.unsharded(), (0, 6)):
        assert _same_bits(batch["tactile_image"], ds.batch(torch.arange(s, s + 6))["tactile_image"])


def _step(dims, seed):
    from gelslim_depth_amd.models.unet import UNet
    from gelslim_depth_amd.train import TrainStep
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=dims, precision="fp32")
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.make_state(3, 1, dims, seed, "conditioned").items()},
                      strict=True)
    m = m.to("cuda").train()
    return m, TrainStep(m)


def _snapshot(m, step):
    s = {"p": step.p_flat, "m": step.m_flat, "v": step.v_flat, "ema": step.ema_flat}
    s.update({"buf/" + k: b for k, b in m.named_buffers()})
    return {k: v.detach().cpu().clone() for k, v in s.items() if v is not None}


def test_fit_with_augmentation_resumes_bit_for_bit(tmp_path):
    """harness.fit, tiny fp32 net, shuffle and every augmentation kind on: 4 epochs straight == 2 epochs + a resume for 2 more
    (parameters, Adam moments, EMA shadow, BatchNorm buffers, loss history); another Augment.seed changes the losses; a changed
    spec is refused on resume."""
    from gelslim_depth_amd import harness
    from gelslim_depth_amd.dataset import Augment, DeviceLoader
    train_ds, val_ds = _datasets()
    aug = Augment(seed=31, hflip=0.5, vflip=0.5, max_shift=(2, 3), gain=0.2, offset=6.0, noise_std=2.0)

    def run(out, seed, max_epochs, augment=aug, **state):
        m, step = _step([8, 16, 32], seed)
        H = harness.fit(step, DeviceLoader(train_ds, 4, shuffle=True, augment=augment), DeviceLoader(val_ds, 4),
                        DeviceLoader(val_ds, 2), str(out / "weights"), "unet_t", train_indefinitely=True,
                        val_loss_SMA_window=2, validation_loss_count_threshold=0, max_epochs=max_epochs,
                        echo=lambda line: None, **state)
        return H, m, step
    a, b, c = tmp_path / "straight", tmp_path / "resumed", tmp_path / "other"
    for d in (a, b, c):
        d.mkdir()
    torch.manual_seed(0)
    H0, m0, s0 = run(a, 4, 4)
    ref = _snapshot(m0, s0)
    del m0, s0
    state = str(b / "state.pt")
    torch.manual_seed(0)
    H1, _, _ = run(b, 4, 2, state_path=state)
    assert H1["train_loss"] == H0["train_loss"][:2]
    torch.manual_seed(12345)
    with pytest.raises(ValueError, match="noise_std"):
        run(b, 7, 4, augment=Augment(**{**aug.spec(), "noise_std": 1.0}), state_path=state, resume=True)
    H, m, step = run(b, 7, 4, state_path=state, resume=True)
    assert H == H0 and len(H["train_loss"]) == 4
    got = _snapshot(m, step)
    assert got.keys() == ref.keys()
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    # the augmentation reaches the step: another seed, and no augmentation, give other train losses from the first epoch on
    torch.manual_seed(0)
    H2, _, _ = run(c, 4, 1, augment=Augment(**{**aug.spec(), "seed": 32}))
    torch.manual_seed(0)
    H3, _, _ = run(c, 4, 1, augment=None)
    assert H2["train_loss"][0] != H0["train_loss"][0] and H3["train_loss"][0] != H0["train_loss"][0]
    assert H2["train_loss"][0] != H3["train_loss"][0]
