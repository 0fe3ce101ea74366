"""CPU: the per-image depth metrics without a kernel launch -- the reference (tests/depth_metrics_ref.py) against a case worked
out by hand, DepthMetrics' validation and its derivation from a depth normalisation, `summarise` on hand-made tables, the
workspace query, the ctypes layout, and harness.fit(metrics=...) with host stubs for the passes."""
import ctypes
import math

import pytest
import torch

import depth_metrics_ref as R


# ------------------------------------------------------------------------------------------------------------ the reference
def test_reference_against_a_case_worked_by_hand():
    """One 2 x 3 image, background 0, contact_eps 2^-10; every value is a short binary fraction, so every figure below is exact.
        t = [[0, -0.5, -0.25], [0, 2^-10, -0.75]]      contact: -0.5, -0.25, -0.75 (2^-10 is AT the threshold: not contact)
        o = [[0.125, -0.25, -0.25], [0, -0.5, -1]]     contact: all but the 0
        e = [[0.125, 0.25, 0], [0, -0.5 - 2^-10, -0.25]]"""
    q = 2.0 ** -10
    t = torch.tensor([[0.0, -0.5, -0.25], [0.0, q, -0.75]]).view(1, 1, 2, 3)
    o = torch.tensor([[0.125, -0.25, -0.25], [0.0, -0.5, -1.0]]).view(1, 1, 2, 3)
    big = 0.5 + q
    want = [0.125 + 0.25 - big - 0.25,                       # sum e
            0.125 + 0.25 + big + 0.25,                       # sum |e|
            0.125 ** 2 + 0.25 ** 2 + big ** 2 + 0.25 ** 2,   # sum e^2
            big,                                             # max |e|
            3.0, 5.0, 3.0,                                   # n_t, n_p, n_tp
            0.25 + 0.0 + 0.25,                               # sum |e| over the target's patch: (0,1), (0,2), (1,2)
            0.25 ** 2 + 0.25 ** 2,
            0.75, 1.0,                                       # peaks of t and o
            # right neighbours, row 0 then row 1; then lower neighbours, column by column
            0.125 + 0.25 + big + (big - 0.25) + 0.125 + (big + 0.25) + 0.25,
            0.0, 0.0, 0.0, 0.0]
    got = R.depth_metrics_ref(o, t, 0.0, q)
    assert got.shape == (1, 16) and got.dtype == torch.float64
    assert got[0].tolist() == want
    # a NaN never wins a maximum, is counted, and makes the sums it belongs to non-finite
    o2 = o.clone()
    o2[0, 0, 0, 0] = math.nan
    bad = R.depth_metrics_ref(o2, t, 0.0, q)[0]
    assert bad[12] == 1 and bad[3] == big and bad[10] == 1.0 and math.isnan(float(bad[0])) and math.isnan(float(bad[11]))
    assert bad[7] == 0.5 and bad[4:7].tolist() == [3.0, 4.0, 3.0], "the NaN lies outside the target's patch"


def test_make_case_has_what_the_tests_rely_on():
    o, t = R.make_case((3, 2, 17, 23), seed=1)
    tab = R.depth_metrics_ref(o, t, **R.SPEC)
    eps = float(R.f32(R.SPEC["contact_eps"]))
    assert tab[1, 4] == 0 and bool((t[1] == 0).all()), "image 1 has no contact"
    assert tab[0, 4] > 20 and tab[2, 4] > 20 and 0 < tab[0, 6] < tab[0, 5], "patches overlap without coinciding"
    for img in (0, 2):
        at, beyond = (t[img].abs() == eps), (t[img].abs() == R.next_beyond(eps, 0.0))
        assert int(at.sum()) == 4 and int(beyond.sum()) == 4
        assert not bool((t[img].abs() > R.f32(eps))[at].any()) and bool((t[img].abs() > R.f32(eps))[beyond].all())
    assert float(t.min()) >= -0.9 and float(t.min()) < -0.6


# ------------------------------------------------------------------------------------------------------------- DepthMetrics
def test_depth_metrics_validation_names_the_field():
    from gelslim_depth_amd.metrics import DepthMetrics
    d = DepthMetrics()
    assert d.spec() == {"background": 0.0, "contact_eps": 1e-3, "unit": 1.0, "unit_name": ""}
    assert DepthMetrics(**d.spec()) == d and hash(DepthMetrics(**d.spec())) == hash(d) and d != DepthMetrics(unit=2.0)
    for kw, msg in ((dict(background=math.nan), "background must be finite"), (dict(background=math.inf), "background must be finite"),
                    (dict(background="x"), "background must be a number"),
                    (dict(contact_eps=-1e-3), "contact_eps must be finite and not negative"),
                    (dict(contact_eps=math.inf), "contact_eps must be finite and not negative"),
                    (dict(contact_eps=None), "contact_eps must be a number"),
                    (dict(unit=0.0), "unit must be finite and not zero"), (dict(unit=math.nan), "unit must be finite and not zero"),
                    (dict(unit_name=3), "unit_name must be a string")):
        with pytest.raises(ValueError, match="DepthMetrics: " + msg):
            DepthMetrics(**kw)
    assert DepthMetrics(contact_eps=0.0).contact_eps == 0.0 and DepthMetrics(unit=-2.5).unit == -2.5


def test_c_struct_layout_and_values():
    from gelslim_depth_amd import _lib
    from gelslim_depth_amd.metrics import COLS, DepthMetrics
    assert ctypes.sizeof(_lib.gsd_depth_metrics) == 16 and _lib.gsd_depth_metrics.contact_eps.offset == 4
    assert _lib.gsd_depth_metrics.reserved.offset == 8 and COLS == 16 == R.COLS
    c = DepthMetrics(background=0.25, contact_eps=1e-3, unit=-7.0).c_struct()
    assert c.background == 0.25 and c.contact_eps == float(R.f32(1e-3)) and list(c.reserved) == [0, 0]


@pytest.mark.parametrize("method,params", [("min_max_to_0_-1", (0.0, 3.2, 0.4, 0.7)), ("mean_std", (0.0, 3.2, 0.4, 0.7)),
                                           ("min_max_to_0_1", (0.0, 3.2, 0.4, 0.7))])
def test_from_normalization_follows_the_denormalisation(method, params):
    from gelslim_depth_amd.metrics import DepthMetrics
    from gelslim_depth_amd.processing import depth_denorm_affine
    a, b = depth_denorm_affine(method, 1.0, params)
    d = DepthMetrics.from_normalization(method, 1.0, params, contact_depth=0.05)
    assert d.unit == a and d.unit_name == "mm"
    assert a * d.background + b == pytest.approx(0.0, abs=1e-15), "the background is the network value of physical depth 0"
    assert d.contact_eps == 0.05 / abs(a) and abs(a) * d.contact_eps == pytest.approx(0.05, rel=1e-15)
    if method == "min_max_to_0_-1":
        assert a == -3.2 and d.background == 0.0, "deeper is more negative; the undeformed gel is 0"
    if method == "mean_std":
        assert a == 0.7 and d.background == -0.4 / 0.7

    class Dataset:
        depth_normalization_method, norm_scale, depth_normalization_parameters = method, 1.0, params
    assert DepthMetrics.from_dataset(Dataset(), 0.05, unit_name="um") == DepthMetrics(d.background, d.contact_eps, a, "um")
    with pytest.raises(ValueError, match="contact_depth must be finite and not negative"):
        DepthMetrics.from_normalization(method, 1.0, params, contact_depth=-1.0)


# ---------------------------------------------------------------------------------------------------------------- summarise
def _row(sum_e=0.0, sum_abs=0.0, sum_sq=0.0, max_abs=0.0, n_t=0.0, n_p=0.0, n_tp=0.0, c_abs=0.0, c_sq=0.0, peak_t=0.0, peak_p=0.0,
         slope=0.0, bad=0.0):
    return [sum_e, sum_abs, sum_sq, max_abs, n_t, n_p, n_tp, c_abs, c_sq, peak_t, peak_p, slope, bad, 0.0, 0.0, 0.0]


M, PAIRS = 100, 180          # a 10 x 10 image: 10*9 + 9*10 pairs


def test_summarise_pools_sums_and_means_ratios():
    from gelslim_depth_amd.metrics import SUMMARY_KEYS, DepthMetrics, pairs_per_image, summarise
    assert pairs_per_image(1, 10, 10) == PAIRS and pairs_per_image(2, 1, 7) == 12 and pairs_per_image(1, 1, 1) == 0
    rows = [_row(-2.0, 4.0, 1.0, 0.5, 20, 10, 5, 2.0, 0.8, 0.9, 0.7, 18.0),
            _row(1.0, 2.0, 3.0, 0.25, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 9.0),                 # no contact, empty union
            _row(0.0, 6.0, 4.0, 1.5, 10, 30, 10, 1.0, 0.1, 0.5, 0.75, 27.0),
            _row(math.nan, math.nan, math.inf, 9.0, 7, 7, 7, 1.0, 1.0, 0.5, 8.0, math.nan, bad=2.0)]   # excluded, counted
    s = summarise(torch.tensor(rows, dtype=torch.float64), (M, PAIRS), DepthMetrics(unit=2.0, unit_name="mm"))
    assert tuple(s) == SUMMARY_KEYS
    assert (s["images"], s["nonfinite_images"], s["images_without_contact"], s["unit_name"]) == (3, 1, 1, "mm")
    assert s["mae"] == 2.0 * 12.0 / 300 and s["rmse"] == 2.0 * math.sqrt(8.0 / 300) and s["bias"] == 2.0 * -1.0 / 300
    assert s["max_abs"] == 3.0
    assert s["contact_mae"] == 2.0 * 3.0 / 30 and s["contact_rmse"] == 2.0 * math.sqrt(0.9 / 30)
    assert s["contact_iou"] == 15.0 / (25 + 30) and s["contact_iou_mean"] == (5.0 / 25 + 10.0 / 30) / 2
    assert s["contact_precision"] == 15.0 / 40 and s["contact_recall"] == 15.0 / 30
    assert s["peak_mae"] == pytest.approx(2.0 * (0.2 + 0.0 + 0.25) / 3, rel=1e-15) and s["peak_max"] == 2.0 * 0.25
    assert s["slope_mae"] == 2.0 * 54.0 / (3 * PAIRS)
    # a negative unit flips the sign of the bias and of nothing else
    neg = summarise(torch.tensor(rows, dtype=torch.float64), (M, PAIRS), DepthMetrics(unit=-2.0, unit_name="mm"))
    assert neg["bias"] == -s["bias"] and all(neg[k] == s[k] for k in SUMMARY_KEYS if k != "bias")


def test_summarise_without_contact_and_without_images():
    from gelslim_depth_amd.metrics import SUMMARY_KEYS, DepthMetrics, summarise
    spec = DepthMetrics()
    s = summarise(torch.tensor([_row(1.0, 2.0, 3.0, 0.25, slope=9.0)], dtype=torch.float64), (M, PAIRS), spec)
    assert s["images"] == 1 and s["images_without_contact"] == 1 and s["mae"] == 0.02 and s["peak_mae"] == 0.0
    for k in ("contact_mae", "contact_rmse", "contact_iou", "contact_iou_mean", "contact_precision", "contact_recall"):
        assert math.isnan(s[k]), k
    # predicted contact where there is none: a union, no intersection, no recall
    s = summarise(torch.tensor([_row(n_p=4.0)], dtype=torch.float64), (M, PAIRS), spec)
    assert s["contact_iou"] == 0.0 and s["contact_iou_mean"] == 0.0 and s["contact_precision"] == 0.0 and math.isnan(s["contact_recall"])
    for table in (torch.zeros((0, 16), dtype=torch.float64), torch.tensor([_row(bad=1.0)], dtype=torch.float64)):
        s = summarise(table, (M, PAIRS), spec)
        assert s["images"] == 0 and s["nonfinite_images"] == table.shape[0] and s["images_without_contact"] == 0
        assert s["unit_name"] == ""
        for k in SUMMARY_KEYS[3:-1]:
            assert math.isnan(s[k]), k


def test_workspace_query_depends_on_the_image_size_alone():
    """No launch: gsd_depth_metrics_workspace is N x (blocks per image) x 16 with one block per 2048 elements of an image, at
    most 64 (gsd_depth_metrics.hip: DM_BLOCK_ELEMS, DM_MAX_BLOCKS)."""
    from gelslim_depth_amd.metrics import depth_metrics_workspace
    for shape in ((2, 1, 9, 11), (1, 1, 1, 1), (3, 1, 41, 53), (32, 1, 320, 427), (16, 1, 320, 427), (5, 2, 64, 16), (1, 2, 64, 16)):
        n, k, h, w = shape
        assert depth_metrics_workspace(shape) == n * min(64, -(-k * h * w // 2048)) * 16, shape
    assert depth_metrics_workspace((0, 1, 9, 11)) == 0 and depth_metrics_workspace((2, 1, -9, 11)) == 0


# ------------------------------------------------------------------------------------------------------- fit(metrics=...)
class _Step:
    """What fit's state file needs from a step."""
    rank = 0

    def state_dict(self):
        return {"stub": 1}

    def load_state_dict(self, sd):
        assert sd == {"stub": 1}


TRAIN, VAL, TEST = [0.5, 0.375], [0.25, 0.3125], [0.125, 0.0625]


def _summary(tag, e):
    from gelslim_depth_amd.metrics import SUMMARY_KEYS
    s = {k: float(i) + e + (0.5 if tag == "test" else 0.0) for i, k in enumerate(SUMMARY_KEYS)}
    s.update(images=4, nonfinite_images=0, images_without_contact=1, unit_name="mm", contact_iou=math.nan if tag == "test" else 0.75)
    return s


def _fit(tmp_path, monkeypatch, fused, lines, epochs=2, **kw):
    """Two epochs of harness.fit over host stubs.  `fused`: the default eval_pass, which turns into evaluate_metrics walks when
    `metrics` is given (evaluate_loader / evaluate_metrics are stubbed in the module); else a caller-supplied eval_pass."""
    from gelslim_depth_amd import harness
    state = {"e": kw.pop("first_epoch", 0) - 1}
    calls = []

    def train_pass(step, loader):
        state["e"] += 1                          # the stubs learn the epoch from the train pass that opens it
        return TRAIN[state["e"]] * 7, 7

    def eval_pass(step, loader, loss_kind="mse"):
        calls.append(("loss", loader))
        return VAL[state["e"]] if loader == "val" else TEST[state["e"]]

    def metrics_pass(step, loader, spec, loss_kind="mse", per_image=False):
        calls.append(("metrics", loader))
        return (VAL[state["e"]] if loader == "val" else TEST[state["e"]]), _summary(loader, state["e"])

    def save(step, path):
        open(path, "w").write("x")
    monkeypatch.setattr(harness, "evaluate_loader", eval_pass)
    monkeypatch.setattr(harness, "evaluate_metrics", metrics_pass)
    H = harness.fit(_Step(), "train", "val", "test", str(tmp_path / "weights"), "unet_x", max_epochs=epochs,
                    train_pass=train_pass, eval_pass=None if fused else eval_pass, save=save, echo=lines.append, **kw)
    return H, calls


def _untimed(lines):
    return [l for l in lines if not l.startswith("Time for epoch") and not l.startswith("Training time")]


PARENT_LINES = ["Validation loss is at a minimum. Saving the model",
                "[INFO] EPOCH: 1",
                "Train loss: 0.500000,  Validation loss: 0.250000, Test loss: 0.125000",
                "[INFO] EPOCH: 2",
                "Train loss: 0.375000,  Validation loss: 0.312500, Test loss: 0.062500",
                "Training complete"]


@pytest.mark.parametrize("fused", [True, False], ids=["default_pass", "own_pass"])
def test_fit_without_metrics_is_what_it_was(tmp_path, monkeypatch, fused):
    """The lines and the keys of H of the same stubbed run on the parent's fit, written out."""
    from gelslim_depth_amd.train import read_state
    lines = []
    path = str(tmp_path / "fit.pt")
    H, calls = _fit(tmp_path, monkeypatch, fused, lines, state_path=path)
    assert _untimed(lines) == PARENT_LINES
    assert list(H.keys()) == ["train_loss", "validation_loss", "test_loss"]
    assert H == {"train_loss": TRAIN, "validation_loss": VAL, "test_loss": TEST}
    assert calls == [("loss", "val"), ("loss", "test")] * 2, "no metrics walk without the keyword"
    loop = read_state(path)["loop"]
    assert sorted(loop) == sorted(["epoch", "stopped", "early_stopping", "H", "elapsed", "augment", "torch_rng", "cuda_rng"])
    assert list(loop["H"].keys()) == ["train_loss", "validation_loss", "test_loss"]


@pytest.mark.parametrize("fused", [True, False], ids=["default_pass", "own_pass"])
def test_fit_with_metrics_adds_two_lists_and_one_line(tmp_path, monkeypatch, fused):
    from gelslim_depth_amd.metrics import DepthMetrics
    from gelslim_depth_amd.train import read_state
    lines = []
    path = str(tmp_path / "fit.pt")
    H, calls = _fit(tmp_path, monkeypatch, fused, lines, state_path=path, metrics=DepthMetrics(unit=-3.2, unit_name="mm"))
    assert list(H.keys()) == ["train_loss", "validation_loss", "test_loss", "validation_metrics", "test_metrics"]
    assert (H["train_loss"], H["validation_loss"], H["test_loss"]) == (TRAIN, VAL, TEST), "the losses are what they were"
    for k, tag in (("validation_metrics", "val"), ("test_metrics", "test")):
        assert len(H[k]) == 2
        for e in range(2):
            want = _summary(tag, e)
            assert {a: b for a, b in H[k][e].items() if b == b} == {a: b for a, b in want.items() if b == b}
    if fused:
        assert calls == [("metrics", "val"), ("metrics", "test")] * 2, "one walk per set: the metrics ride on the loss's"
    else:
        assert calls == [("loss", "val"), ("metrics", "val"), ("loss", "test"), ("metrics", "test")] * 2
    extra = ["Metrics [mm]: Validation mae 3.000000, rmse 4.000000, contact_mae 7.000000, contact_iou 0.750000, peak_mae 13.000000, "
             "slope_mae 15.000000; Test mae 3.500000, rmse 4.500000, contact_mae 7.500000, contact_iou nan, peak_mae 13.500000, "
             "slope_mae 15.500000",
             "Metrics [mm]: Validation mae 4.000000, rmse 5.000000, contact_mae 8.000000, contact_iou 0.750000, peak_mae 14.000000, "
             "slope_mae 16.000000; Test mae 4.500000, rmse 5.500000, contact_mae 8.500000, contact_iou nan, peak_mae 14.500000, "
             "slope_mae 16.500000"]
    assert _untimed(lines) == PARENT_LINES[:3] + extra[:1] + PARENT_LINES[3:5] + extra[1:] + PARENT_LINES[5:]
    saved = read_state(path)["loop"]["H"]
    assert list(saved.keys()) == list(H.keys()) and saved["validation_metrics"][1]["mae"] == 4.0
    with pytest.raises(TypeError, match="metrics must be a metrics.DepthMetrics"):
        _fit(tmp_path, monkeypatch, fused, [], metrics={"background": 0.0})


def test_fit_resumes_with_metrics_from_a_state_without_them(tmp_path, monkeypatch):
    from gelslim_depth_amd.metrics import DepthMetrics
    from gelslim_depth_amd.train import read_state
    path = str(tmp_path / "fit.pt")
    H, _ = _fit(tmp_path, monkeypatch, True, [], epochs=1, state_path=path)
    assert "validation_metrics" not in read_state(path)["loop"]["H"]
    lines = []
    H, calls = _fit(tmp_path, monkeypatch, True, lines, epochs=2, first_epoch=1, state_path=path, resume=True, metrics=DepthMetrics())
    assert (H["train_loss"], H["validation_loss"], H["test_loss"]) == (TRAIN, VAL, TEST)
    assert H["validation_metrics"][0] is None and H["test_metrics"][0] is None, "the epochs before the keyword are padded"
    assert H["validation_metrics"][1]["mae"] == _summary("val", 1)["mae"] and len(H["test_metrics"]) == 2
    assert calls == [("metrics", "val"), ("metrics", "test")]
    assert [l for l in _untimed(lines) if l.startswith("Metrics")] == [l for l in _untimed(lines) if "mae 4.000000" in l] != []
    # ... and the round trip of a state that has them: a third epoch's worth of resume changes nothing
    saved = read_state(path)["loop"]["H"]
    assert saved["validation_metrics"][0] is None and saved["test_metrics"][1]["rmse"] == _summary("test", 1)["rmse"]
    H2, calls = _fit(tmp_path, monkeypatch, True, [], epochs=2, first_epoch=2, state_path=path, resume=True, metrics=DepthMetrics())
    assert calls == [] and H2["validation_metrics"][0] is None and H2["validation_metrics"][1]["mae"] == H["validation_metrics"][1]["mae"]
