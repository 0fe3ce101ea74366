"""CPU: the augmentation stream of gsd_gather_augment without a GPU.  The library's two device-free queries
(gsd_augment_sample, gsd_augment_noise) run the very code the kernel runs; they are held here to the numpy restatement of
the stream's definition (tests/augment_ref.py) and to the exact distributions the definition implies.  Then the argument
checks of the launch entry point, Augment's validation, and the epoch / spec bookkeeping of DeviceLoader and harness.fit
over host stand-ins."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import augment_ref as AR
from conftest import REPO
from gelslim_depth_amd import _lib as L
from gelslim_depth_amd import harness
from gelslim_depth_amd.dataset import Augment, DeviceLoader

SEEDS, EPOCHS, ROWS = (0, 1, 12345), (0, 1, 7), 4096
P = AR.params(p_hflip=0.5, p_vflip=0.5, max_dy=8, max_dx=8, gain=0.25, offset=10.0, noise_std=2.0, pivot=127.5)


lib_sample, lib_noise = AR.lib_sample, AR.lib_noise


def _ordered(x):
    """float32 -> int64 that orders like the floats and steps by 1 per ulp, across zero too."""
    i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


@pytest.fixture(scope="module")
def draws():
    """The library's draws of rows 0..4095 for every (seed, epoch) pair."""
    return {(s, e): lib_sample(dict(P, seed=s), e, range(ROWS), 3) for s in SEEDS for e in EPOCHS}


def test_sample_equals_the_restatement(draws):
    for (s, e), got in draws.items():
        want = AR.sample(dict(P, seed=s), e, np.arange(ROWS), 3)
        for k in ("hflip", "vflip", "dy", "dx"):
            assert np.array_equal(got[k], want[k]), (s, e, k)
        # an fp64 emulation of fmaf can double-round: 1 fp32 ulp
        for k in ("gain", "offset"):
            assert np.abs(_ordered(got[k]) - _ordered(want[k])).max() <= 1, (s, e, k)
        assert np.abs(got["gain"] - 1).max() <= 0.25 and np.abs(got["offset"]).max() <= 10.0
        assert got["gain"].std() > 0.1 and got["offset"].std() > 4.0


def test_sample_extremes_and_large_keys():
    """p = 0 never flips, p = 1 always does; max_shift 0 never shifts; seeds / epochs / rows beyond 32 bits agree too."""
    idx = np.array([0, 1, 2 ** 31, 2 ** 40 + 3, 2 ** 62])
    for seed, epoch in ((2 ** 64 - 1, 2 ** 40), (0x1234567890ABCDEF, 3)):
        p = dict(P, seed=seed, max_dy=1 << 20, max_dx=3)
        got, want = lib_sample(p, epoch, idx, 8), AR.sample(p, epoch, idx, 8)
        for k in ("hflip", "vflip", "dy", "dx"):
            assert np.array_equal(got[k], want[k]), k
        assert np.abs(_ordered(got["gain"]) - _ordered(want["gain"])).max() <= 1
    never = lib_sample(AR.params(seed=5), 0, range(256), 3)
    assert not never["hflip"].any() and not never["vflip"].any() and not never["dy"].any() and not never["dx"].any()
    assert (never["gain"] == 1).all() and (never["offset"] == 0).all()
    always = lib_sample(AR.params(seed=5, p_hflip=1.0, p_vflip=1.0), 0, range(256), 3)
    assert always["hflip"].all() and always["vflip"].all()


def test_noise_equals_the_restatement_bit_for_bit():
    n = 3 * 320 * 427
    for s, e, row in ((0, 0, 0), (1, 7, 17), (12345, 1, 4095), (2 ** 63 + 1, 2 ** 33, 2 ** 35)):
        p = dict(P, seed=s)
        assert np.array_equal(lib_noise(p, e, row, 0, n).view(np.int32), AR.noise(p, e, row, 0, n).view(np.int32)), (s, e, row)
    p = dict(P, seed=9)
    whole = lib_noise(p, 2, 3, 0, 5000)
    assert np.array_equal(lib_noise(p, 2, 3, 1234, 777), whole[1234:1234 + 777])       # element e, not position in the call
    assert np.abs(whole).max() <= 131070 * np.sqrt(3) / 65536 + 1e-6
    assert not np.array_equal(lib_noise(p, 2, 4, 0, 5000), whole) and not np.array_equal(lib_noise(p, 3, 3, 0, 5000), whole)


def test_flip_and_shift_distributions(draws):
    """5 standard deviations of the exact distributions: Binomial(4096, 1/2) for the flips (sd 32), Binomial(4096, 1/17) per
    shift bin.  Restated with numpy, the worst cases over these seeds and epochs are 49 (flips) and 3.05 sd (a shift bin)."""
    sd_bin = np.sqrt(ROWS * (1 / 17) * (16 / 17))
    for (s, e), d in draws.items():
        for k in ("hflip", "vflip"):
            assert abs(int(d[k].sum()) - ROWS // 2) <= 160, (s, e, k, int(d[k].sum()))
        for k in ("dy", "dx"):
            assert d[k].min() == -8 and d[k].max() == 8
            counts = np.bincount(d[k] + 8, minlength=17)
            assert np.abs(counts - ROWS / 17).max() <= 5 * sd_bin, (s, e, k, counts)
        # the four choices of a sample are separate draws / separate bit fields: no two coincide
        assert 0.35 < np.mean(d["hflip"] == d["vflip"]) < 0.65 and np.mean(d["dy"] == d["dx"]) < 0.12


def test_noise_distribution():
    """Over one 3 x 320 x 427 image: mean within 5 / sqrt(N) of 0, variance within 5 sqrt(1.7 / N) of 1 (a sum of four uniforms
    has kurtosis 2.7, so n^2 has variance 1.7)."""
    n = 3 * 320 * 427
    for s in SEEDS:
        for e in EPOCHS:
            z = lib_noise(dict(P, seed=s), e, 0, 0, n).astype(np.float64)
            assert abs(z.mean()) <= 5 / np.sqrt(n), (s, e, z.mean())
            assert abs(z.var() - 1.0) <= 5 * np.sqrt(1.7 / n), (s, e, z.var())
            assert 2.6 < ((z - z.mean()) ** 4).mean() / z.var() ** 2 < 2.8


def test_epochs_and_seeds_draw_differently(draws):
    for s in SEEDS:
        a, b = draws[(s, 0)], draws[(s, 1)]
        for k in ("hflip", "vflip", "dy", "dx"):
            assert not np.array_equal(a[k], b[k]), (s, k)
        assert 0.35 < np.mean(a["hflip"] == b["hflip"]) < 0.65           # independent, not merely different
        assert not np.array_equal(a["gain"], b["gain"])
    assert not np.array_equal(draws[(0, 0)]["dy"], draws[(1, 0)]["dy"])


def _header_struct(name):
    """[(type, field), ...] of `typedef struct <name> { ... }` in include/gsd.h, arrays as (type, field, length)."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gsd.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for f in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", f)
            fields.append((ctype, m.group(1), int(m.group(2) or 1)))
    return fields


def test_struct_layouts_match_the_header():
    ctypes_of = {"uint64_t": C.c_uint64, "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    for name, cls, size in (("gsd_augment", L.gsd_augment, 48), ("gsd_augment_draw", L.gsd_augment_draw, 80)):
        fields = _header_struct(name)
        assert [f for _, f, _ in fields] == [f for f, _ in cls._fields_], name
        off = 0
        for ctype, f, n in fields:
            t = ctypes_of[ctype]
            off = -(-off // C.sizeof(t)) * C.sizeof(t)          # natural alignment, as the C compiler lays it out
            assert getattr(cls, f).offset == off and getattr(cls, f).size == C.sizeof(t) * n, (name, f)
            off += C.sizeof(t) * n
        align = max(C.sizeof(ctypes_of[ctype]) for ctype, _, _ in fields)
        assert C.sizeof(cls) == size == -(-off // align) * align, name
    assert L.gsd_augment.epoch.offset == 8 and L.gsd_augment.max_dy.offset == 24 and L.gsd_augment.pivot.offset == 44
    assert L.gsd_augment_draw.gain.offset == 16 and L.gsd_augment_draw.offset.offset == 48


def test_gather_augment_refuses_bad_arguments_without_a_device():
    """Every refusal comes before any launch: the pointers below are host memory that is never read."""
    buf = (C.c_float * 16)()
    ptr = C.addressof(buf)

    def call(aug=None, **kw):
        a = dict(img=ptr, dep=ptr, idx=ptr, M=4, B=2, Ci=3, Cd=1, H=2, W=2, Ai=ptr, Bi=ptr, nabi=3, Ad=ptr, Bd=ptr, nabd=1,
                 out_img=ptr, out_dep=ptr)
        a.update(kw)
        aug = C.byref(aug) if aug is not None else None
        rc = L.lib.gsd_gather_augment(a["img"], a["dep"], a["idx"], a["M"], a["B"], a["Ci"], a["Cd"], a["H"], a["W"], a["Ai"],
                                      a["Bi"], a["nabi"], a["Ad"], a["Bd"], a["nabd"], aug, a["out_img"], a["out_dep"], None)
        return rc, L.lib.gsd_last_error().decode()
    ok = L.make_augment(seed=1, p_hflip=0.5, max_dy=2, gain=0.1, offset=1.0, noise_std=1.0)
    for k in ("img", "dep", "idx", "Ai", "Bi", "Ad", "Bd", "out_img", "out_dep"):
        assert call(ok, **{k: None})[0] == L.GSD_ERR_BAD_ARG, k
    assert call(None)[0] == L.GSD_ERR_BAD_ARG
    for k in ("M", "B", "Ci", "Cd", "H", "W", "nabi", "nabd"):
        for v in (0, -1):
            assert call(ok, **{k: v})[0] == L.GSD_ERR_BAD_ARG, (k, v)
    rc, msg = call(ok, Ci=9)
    assert rc == L.GSD_ERR_UNSUPPORTED and "Ci" in msg
    inf, nan = float("inf"), float("nan")
    bad = [dict(p_hflip=-0.01), dict(p_hflip=1.5), dict(p_hflip=nan), dict(p_vflip=-1.0), dict(p_vflip=inf), dict(p_vflip=nan),
           dict(max_dy=-1), dict(max_dx=-3), dict(max_dy=(1 << 20) + 1), dict(gain=-0.1), dict(gain=1.0), dict(gain=nan),
           dict(offset=-1.0), dict(offset=inf), dict(noise_std=-0.5), dict(noise_std=nan), dict(pivot=inf)]
    for kw in bad:
        assert call(L.make_augment(**kw))[0] == L.GSD_ERR_BAD_ARG, kw
        d = L.gsd_augment_draw()
        assert L.lib.gsd_augment_sample(C.byref(L.make_augment(**kw)), 0, 3, C.byref(d)) == L.GSD_ERR_BAD_ARG, kw
    d = L.gsd_augment_draw()
    assert L.lib.gsd_augment_sample(C.byref(ok), 0, 9, C.byref(d)) == L.GSD_ERR_UNSUPPORTED
    assert L.lib.gsd_augment_sample(C.byref(ok), 0, 0, C.byref(d)) == L.GSD_ERR_BAD_ARG
    assert L.lib.gsd_augment_sample(None, 0, 3, C.byref(d)) == L.GSD_ERR_BAD_ARG
    assert L.lib.gsd_augment_sample(C.byref(ok), 0, 3, None) == L.GSD_ERR_BAD_ARG
    assert L.lib.gsd_augment_noise(C.byref(ok), 0, 0, 4, None) == L.GSD_ERR_BAD_ARG
    assert L.lib.gsd_augment_noise(C.byref(ok), 0, -1, 4, ptr) == L.GSD_ERR_BAD_ARG


def test_augment_validation_names_the_field():
    bad = [("hflip", dict(hflip=1.2)), ("hflip", dict(hflip=-0.1)), ("vflip", dict(vflip=2.0)), ("vflip", dict(vflip=float("nan"))),
           ("max_shift", dict(max_shift=(-1, 0))), ("max_shift", dict(max_shift=(0, -2))), ("max_shift", dict(max_shift=(1.5, 0))),
           ("max_shift", dict(max_shift=(1, 2, 3))), ("gain", dict(gain=1.0)), ("gain", dict(gain=-0.2)),
           ("offset", dict(offset=-1.0)), ("noise_std", dict(noise_std=-0.1)), ("noise_std", dict(noise_std=float("inf"))),
           ("pivot", dict(pivot=float("nan")))]
    for field, kw in bad:
        with pytest.raises(ValueError, match=field):
            Augment(**kw)
    a = Augment(seed=3, hflip=0.5, max_shift=(4, 6), gain=0.1, offset=2, noise_std=1.5)
    assert a.spec() == {"seed": 3, "hflip": 0.5, "vflip": 0.0, "max_shift": [4, 6], "gain": 0.1, "offset": 2.0, "noise_std": 1.5,
                        "pivot": None}
    assert all(type(v) in (int, float, list, type(None)) for v in a.spec().values())
    assert a == Augment(**{**a.spec(), "max_shift": (4, 6)}) and a != Augment(seed=4, hflip=0.5) and a != "a"
    assert Augment().spec() == {"seed": 0, "hflip": 0.0, "vflip": 0.0, "max_shift": [0, 0], "gain": 0.0, "offset": 0.0,
                                "noise_std": 0.0, "pivot": None}, "everything is off by default, the flips included"
    assert "flips are off by default" in " ".join(Augment.__doc__.lower().split())
    s = a.struct(5, default_pivot=127.5)
    assert (s.seed, s.epoch, s.p_hflip, s.max_dy, s.max_dx, s.pivot) == (3, 5, 0.5, 4, 6, 127.5)
    assert Augment(pivot=3.0).struct(0, default_pivot=127.5).pivot == 3.0


class _Recorder:
    """What DeviceLoader needs from a DeviceDataset, over CPU tensors; records how `batch` is called."""

    def __init__(self, n=10):
        self.x, self.device, self.calls = torch.arange(float(n)).view(n, 1).repeat(1, 4), torch.device("cpu"), []

    def __len__(self):
        return self.x.shape[0]

    def batch(self, idx, *args, **kw):
        self.calls.append((idx.tolist(), args, kw))
        return {"tactile_image": self.x[idx], "depth_image": self.x[idx, :1], "object_index": idx}


def _augs(ds):
    """(augment, epoch) of every recorded batch call, (None, None) for a plain one; clears the record."""
    out = [(c[1][0], c[1][1]) if c[1] else (None, None) for c in ds.calls]
    assert all(not c[2] for c in ds.calls)
    ds.calls.clear()
    return out


def test_loader_epoch_bookkeeping():
    aug, ds = Augment(seed=1, max_shift=(2, 2)), _Recorder()
    loader = DeviceLoader(ds, 3, shuffle=True, augment=aug)
    torch.manual_seed(0)
    for want in (0, 1, 2):
        assert len(list(loader)) == 4
        assert _augs(ds) == [(aug, want)] * 4           # one epoch for the whole pass, then it advances
    loader.set_epoch(7)
    list(loader)
    assert _augs(ds) == [(aug, 7)] * 4
    list(loader)
    assert _augs(ds) == [(aug, 8)] * 4
    # the shuffle order does not depend on the augmentation: nothing is drawn from torch's generators
    torch.manual_seed(5)
    list(loader), list(loader)
    with_aug, state = [c[0] for c in ds.calls], torch.get_rng_state()
    ds.calls.clear()
    torch.manual_seed(5)
    plain = DeviceLoader(ds, 3, shuffle=True)
    list(plain), list(plain)
    assert [c[0] for c in ds.calls] == with_aug and torch.equal(torch.get_rng_state(), state)
    assert _augs(ds) == [(None, None)] * 8
    # evaluation never augments
    for rank in (0, 1):
        sharded = DeviceLoader(ds, 2, shuffle=False, rank=rank, world_size=2, augment=aug)
        assert sum(1 for _ in sharded.eval_shares()) == 3
        assert set(_augs(ds)) == {(None, None)}
        un = sharded.unsharded()
        assert un.augment is None and un.world_size == 1 and un.batch_size == 4
        list(un)
        assert set(_augs(ds)) == {(None, None)}
        list(sharded)
        assert set(_augs(ds)) == {(aug, 0)}
    un = loader.unsharded()
    assert un is not loader and un.augment is None and un.batch_size == 3 and un.shuffle
    assert plain.unsharded() is plain
    with pytest.raises(TypeError):
        DeviceLoader(ds, 3, augment={"seed": 1})


class _Step:
    rank = 0

    def __init__(self):
        self.n = 0

    def state_dict(self):
        return {"n": self.n}

    def load_state_dict(self, sd):
        self.n = int(sd["n"])


class _EpochLoader:
    """A train loader that only records what fit tells it."""

    def __init__(self, augment=None):
        self.augment, self.epochs = augment, []

    def set_epoch(self, e):
        self.epochs.append(e)


def _fit(tmp_path, loader, max_epochs, **kw):
    seen = []

    def train_pass(step, ld):
        seen.append(ld.epochs[-1] if getattr(ld, "epochs", None) else None)
        step.n += 1
        return 1.0 / step.n, 1
    H = harness.fit(_Step(), loader, "val", "test", str(tmp_path / "w"), "unet", max_epochs=max_epochs, train_indefinitely=True,
                    train_pass=train_pass, eval_pass=lambda st, ld: 1.0 / (1 + st.n), save=lambda st, path: None,
                    echo=lambda line: None, **kw)
    return H, seen


def test_fit_sets_the_epoch_and_guards_the_spec(tmp_path):
    aug = Augment(seed=2, hflip=0.5, noise_std=1.0)
    state = str(tmp_path / "state.pt")
    loader = _EpochLoader(aug)
    _, seen = _fit(tmp_path, loader, 3, state_path=state)
    assert loader.epochs == [0, 1, 2] and seen == [0, 1, 2]          # set before each train pass
    assert torch.load(state, weights_only=True)["loop"]["augment"] == aug.spec()
    # after a resume the first epoch is the saved one
    loader = _EpochLoader(Augment(**{**aug.spec(), "max_shift": (0, 0)}))
    H, seen = _fit(tmp_path, loader, 5, state_path=state, resume=True)
    assert loader.epochs == [3, 4] and seen == [3, 4] and len(H["train_loss"]) == 5
    # a changed spec is refused, naming the field
    for field, kw in (("seed", dict(seed=3)), ("noise_std", dict(noise_std=2.0)), ("max_shift", dict(max_shift=(1, 0)))):
        with pytest.raises(ValueError, match=field):
            _fit(tmp_path, _EpochLoader(Augment(**{**aug.spec(), "max_shift": (0, 0), **kw})), 7, state_path=state, resume=True)
    with pytest.raises(ValueError, match="augment"):
        _fit(tmp_path, _EpochLoader(None), 7, state_path=state, resume=True)
    # a loader without set_epoch (a plain iterable) is left alone, and its state carries augment None ...
    plain = str(tmp_path / "plain.pt")
    _fit(tmp_path, "train", 2, state_path=plain)
    blob = torch.load(plain, weights_only=True)
    assert blob["loop"]["augment"] is None
    with pytest.raises(ValueError, match="augment"):
        _fit(tmp_path, _EpochLoader(aug), 4, state_path=plain, resume=True)
    # ... and a state file written before the key existed reads as None
    del blob["loop"]["augment"]
    torch.save(blob, plain)
    H, _ = _fit(tmp_path, "train", 4, state_path=plain, resume=True)
    assert len(H["train_loss"]) == 4
    with pytest.raises(ValueError, match="augment"):
        _fit(tmp_path, _EpochLoader(aug), 6, state_path=plain, resume=True)


def test_gather_augment_kernels_use_no_scratch():
    """The three instantiations of the kernel (plain / gain+offset / noise) keep their eight loads in registers: no scratch
    (device-only compile of the one source, a few seconds)."""
    import shutil
    import subprocess
    from gelslim_depth_amd import build as b
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this machine")
    assert "gsd_augment.hip" in b.SOURCES
    r = subprocess.run([hipcc] + b.CFLAGS + [f"-I{b.INCLUDE}", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(b.CSRC, "gsd_augment.hip"), "-o", os.devnull], capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    kernels = {n: (s, l) for n, s, l in zip(names, scratch, lds) if "gather_augment_kernel" in n}
    assert len(kernels) == 3, r.stderr[-2000:]
    assert all(s == 0 and l <= 64 for s, l in kernels.values()), kernels      # LDS: the block's draws only
