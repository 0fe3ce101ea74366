"""GPU: gsd_depth_metrics against its fp64 reference (tests/depth_metrics_ref.py), what it must leave alone, its independence
of the batch and its argument checks; harness.evaluate_metrics in fp32 and bf16, fit(metrics=...), and two ranks.

Bounds (derived, not fitted).  Counts (columns 4-6, 12) are integers and the maxima (3, 9, 10) are fp32 values the reference
finds by the same fp32 comparisons: equal.  The summands of columns 1, 2, 7, 8 and 11 are exact in fp64, or fp32 values the
reference forms identically, and are non-negative; an image has fewer than 2^21 fp64 additions in either order of summation,
each within 2^-53 of the running sum: within 2^-32 of the sum, relative.  Column 0 adds signed terms, so its error is held
against the sum of their magnitudes, column 1.  Columns 13-15 are 0."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_metrics_ref as R
from conftest import REPO
from gelslim_depth_amd import synth

pytestmark = pytest.mark.gpu

SENT = -7.25
BOUND = 2.0 ** -32
EQUAL_COLS = (3, 4, 5, 6, 9, 10, 12)
SUM_COLS = (1, 2, 7, 8, 11)
# gsd_depth_metrics.hip: an image gets one 256-thread block per DM_BLOCK_ELEMS elements, at most DM_MAX_BLOCKS; a block owns
# ceil(m / blocks) consecutive elements of its image
BLOCK_ELEMS, MAX_BLOCKS, THREADS = 2048, 64, 256
# 41 * 53 = 2173 elements: two blocks of 1087 = 20 rows + 27 columns (the block boundary lies inside row 20), five iterations per
# thread; 2049 elements is the least that gives two blocks, and no H x W nearer to it has odd sides and a boundary inside a row
BIG = (3, 1, 41, 53)
OP_SHAPES = [(2, 1, 9, 11), (3, 2, 17, 23), (1, 1, 5, 37), (1, 1, 1, 1), (1, 1, 1, 7), (1, 1, 7, 1), BIG]
CONFIGS = [("fp32", [16, 32, 64], (2, 21, 27)), ("bf16", [32, 64, 128], (2, 37, 53))]
IDS = [c[0] for c in CONFIGS]


def sid(shape):
    return "x".join(map(str, shape))


def blocks_per_image(m):
    return min(MAX_BLOCKS, -(-m // BLOCK_ELEMS))


@pytest.fixture(scope="module")
def L():
    from gelslim_depth_amd import _lib
    return _lib


_CASES = {}
_REFS = {}


def case(shape):
    """(o, t) on the CPU and on the GPU, made once per shape."""
    key = tuple(shape)
    if key not in _CASES:
        o, t = R.make_case(key, seed=sum(key), **R.SPEC)
        _CASES[key] = (o, t, o.cuda(), t.cuda())
    return _CASES[key]


def ref(shape):
    """The reference table of a shared case, computed once and never modified."""
    key = tuple(shape)
    if key not in _REFS:
        o, t, _, _ = case(key)
        _REFS[key] = R.depth_metrics_ref(o, t, **R.SPEC)
    return _REFS[key]


def c_spec(**over):
    c = _lib().gsd_depth_metrics()
    c.background, c.contact_eps = R.SPEC["background"], R.SPEC["contact_eps"]
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _lib():
    from gelslim_depth_amd import _lib as lib
    return lib


def run_op(L, od, td, spec=None):
    """One launch into sentinel-padded buffers; returns (table, the workspace's partial rows)."""
    n, k, h, w = od.shape
    need = L.lib.gsd_depth_metrics_workspace(n, k, h, w)
    assert need == n * blocks_per_image(k * h * w) * 16
    ws = torch.full((need + 8,), SENT, device="cuda", dtype=torch.float64)
    table = torch.full((n * 16 + 8,), SENT, device="cuda", dtype=torch.float64)
    o0, t0 = od.clone(), td.clone()
    c = c_spec() if spec is None else spec
    L.check(L.lib.gsd_depth_metrics(ctypes.byref(c), od.data_ptr(), td.data_ptr(), n, k, h, w, table.data_ptr(), ws.data_ptr(), need,
                                    L.stream_ptr()), "depth_metrics")
    torch.cuda.synchronize()
    assert bool((ws[need:] == SENT).all()), "wrote past gsd_depth_metrics_workspace doubles"
    assert bool((table[n * 16:] == SENT).all()), "wrote past the N x 16 table"
    assert torch.equal(od.view(torch.int32), o0.view(torch.int32)) and torch.equal(td.view(torch.int32), t0.view(torch.int32)), \
        "the inputs were written"
    return table[:n * 16].view(n, 16).clone(), ws[:need].clone()


def bits(t):
    return t.contiguous().view(torch.int64)


def check_table(got, want, what):
    """Every row of `got` (device or CPU) against the reference's at the module's bounds, each figure printed first."""
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape
    for i in range(got.shape[0]):
        g, r = got[i].tolist(), want[i].tolist()
        rel = {c: (abs(g[c] - r[c]) / r[c] if r[c] else abs(g[c] - r[c])) for c in SUM_COLS}
        print(f"{what} image {i}: sums rel err " + " ".join(f"{c}:{v:.2g}" for c, v in rel.items())
              + f"; col 0 {g[0]!r} ref {r[0]!r} err/col1 {abs(g[0] - r[0]) / r[1] if r[1] else abs(g[0] - r[0]):.2g}"
              + f"; counts {g[4]:.0f} {g[5]:.0f} {g[6]:.0f} bad {g[12]:.0f}; maxima {g[3]!r} {g[9]!r} {g[10]!r}")
        for c in EQUAL_COLS:
            assert g[c] == r[c], (what, i, c, g[c], r[c])
        for c in SUM_COLS:
            assert abs(g[c] - r[c]) <= BOUND * r[c], (what, i, c, g[c], r[c])
        assert abs(g[0] - r[0]) <= BOUND * r[1], (what, i, 0, g[0], r[0])
        assert g[13:] == [0.0, 0.0, 0.0], (what, i, g[13:])


# ---------------------------------------------------------------------------------------------- the op against the reference
@pytest.mark.parametrize("shape", OP_SHAPES, ids=[sid(s) for s in OP_SHAPES])
def test_op_against_fp64(L, shape):
    n, k, h, w = shape
    m = k * h * w
    if shape == BIG:
        chunk = -(-m // blocks_per_image(m))
        assert blocks_per_image(m) == 2 and chunk % w != 0 and chunk > 2 * THREADS
    else:
        assert blocks_per_image(m) == 1
    _, _, od, td = case(shape)
    want = ref(shape)
    table, part = run_op(L, od, td)
    check_table(table, want, sid(shape))
    if n >= 2:
        assert float(table[1, 4]) == 0.0 and float(table[1, 9]) == 0.0, "image 1 has no contact"
    if m >= 16:
        assert float(table[0, 6]) > 0 and float(table[0, 6]) < float(table[0, 4] + table[0, 5] - table[0, 6]), \
            "the patches overlap without coinciding"
    if w == 1 or h == 1:
        o, t, _, _ = case(shape)
        e = (o - t).view(-1)
        assert float(want[0, 11]) == float((e[1:] - e[:-1]).double().abs().sum()), "only one pair direction exists"
    table2, part2 = run_op(L, od, td)
    assert torch.equal(bits(table), bits(table2)) and torch.equal(bits(part), bits(part2)), "two runs differ"


def test_python_entry_point(L):
    from gelslim_depth_amd.metrics import DepthMetrics, depth_metrics, depth_metrics_workspace
    shape = (3, 2, 17, 23)
    _, _, od, td = case(shape)
    spec = DepthMetrics(**R.SPEC)
    table = depth_metrics(od, td, spec)
    assert table.shape == (3, 16) and table.dtype == torch.float64 and table.is_cuda
    torch.cuda.synchronize()
    assert torch.equal(bits(table), bits(run_op(L, od, td)[0]))
    mine = torch.empty((3, 16), device="cuda", dtype=torch.float64)
    ws = torch.empty((depth_metrics_workspace(shape),), device="cuda", dtype=torch.float64)
    assert depth_metrics(od, td, spec, mine, ws) is mine and torch.equal(bits(mine), bits(table))
    for o, t, msg in ((od.transpose(2, 3), td.transpose(2, 3), "contiguous"), (od.double(), td, "float32"), (od.cpu(), td, "on the GPU"),
                      (od, td.half(), "float32"), (od, td[:2], "must be one"), (od[0], td[0], "must be one")):
        with pytest.raises(L.GsdError, match=msg):
            depth_metrics(o, t, spec)
    with pytest.raises(L.GsdError, match="table must be"):
        depth_metrics(od, td, spec, torch.empty((3, 15), device="cuda", dtype=torch.float64))
    with pytest.raises(L.GsdError, match="workspace"):
        depth_metrics(od, td, spec, None, torch.empty((15,), device="cuda", dtype=torch.float64))


# -------------------------------------------------------------------------------------------------- independence, isolation
@pytest.mark.parametrize("shape", [(3, 2, 17, 23), BIG], ids=sid)
def test_a_row_does_not_depend_on_the_batch(L, shape):
    _, _, od, td = case(shape)
    full, _ = run_op(L, od, td)
    for i in range(shape[0]):
        alone, _ = run_op(L, od[i:i + 1].contiguous(), td[i:i + 1].contiguous())
        lead, _ = run_op(L, od[:i + 1].contiguous(), td[:i + 1].contiguous())
        assert torch.equal(bits(alone[0]), bits(full[i])), f"image {i} alone differs from image {i} of the batch"
        assert torch.equal(bits(lead), bits(full[:i + 1])), f"the leading {i + 1} images differ from the batch's"
    # ... nor on its position: the batch reversed gives the rows reversed
    back, _ = run_op(L, od.flip(0).contiguous(), td.flip(0).contiguous())
    assert torch.equal(bits(back.flip(0)), bits(full))


def test_a_non_finite_image_stays_alone(L):
    shape = (3, 2, 17, 23)
    o, t, od, td = case(shape)
    clean, _ = run_op(L, od, td)
    o2 = o.clone()
    o2[1, 1, 4, 7] = math.nan
    o2[1, 0, 16, 22] = math.inf               # the last element of a plane: no right and no lower neighbour
    o2[1, 0, 3, 3] = -math.inf
    table, _ = run_op(L, o2.cuda(), td)
    want = R.depth_metrics_ref(o2, t, **R.SPEC)
    row = table[1].cpu()
    print("non-finite image:", row.tolist())
    assert float(row[12]) == 3.0 == float(want[1, 12])
    for i in (0, 2):
        assert torch.equal(bits(table[i]), bits(clean[i])), f"image {i} changed"
    for c in (3, 9, 10):
        assert not math.isnan(float(row[c])) and float(row[c]) == float(want[1, c]), c
    assert float(row[3]) == math.inf and float(row[10]) == math.inf and float(row[9]) == 0.0
    assert [float(row[c]) for c in (4, 5, 6)] == [float(want[1, c]) for c in (4, 5, 6)]
    assert all(not math.isfinite(float(row[c])) for c in (0, 1, 2, 11)), "its own sums are non-finite, as they naturally are"
    # a NaN alone: the maxima are those of the finite elements
    o3 = o.clone()
    o3[1, 1, 4, 7] = math.nan
    table, _ = run_op(L, o3.cuda(), td)
    want = R.depth_metrics_ref(o3, t, **R.SPEC)
    for c in EQUAL_COLS:
        assert float(table[1, c]) == float(want[1, c]) and math.isfinite(float(table[1, c])), c
    assert float(table[1, 12]) == 1.0


def test_bad_arguments_return_before_any_launch(L):
    shape = (2, 1, 9, 11)
    _, _, od, td = case(shape)
    need = L.lib.gsd_depth_metrics_workspace(*shape)
    ws = torch.full((need + 2,), SENT, device="cuda", dtype=torch.float64)
    table = torch.full((2 * 16,), SENT, device="cuda", dtype=torch.float64)

    def call(spec=True, o=od.data_ptr(), t=td.data_ptr(), dims=shape, table_p=table.data_ptr(), ws_p=ws.data_ptr(), ws_elems=need,
             reserved=(0, 0), **fields):
        c = c_spec(**fields)
        c.reserved[0], c.reserved[1] = reserved
        return L.lib.gsd_depth_metrics(ctypes.byref(c) if spec else None, o, t, *dims, table_p, ws_p, ws_elems, L.stream_ptr())
    bad_arg = [dict(spec=False), dict(o=None), dict(t=None), dict(table_p=None), dict(ws_p=None),
               dict(dims=(0, 1, 9, 11)), dict(dims=(2, -1, 9, 11)), dict(dims=(2, 1, 0, 11)), dict(dims=(2, 1, 9, 0)),
               dict(reserved=(1, 0)), dict(reserved=(0, -1)),
               dict(contact_eps=-1e-3), dict(contact_eps=math.nan), dict(contact_eps=math.inf),
               dict(background=math.nan), dict(background=math.inf), dict(background=-math.inf)]
    for kw in bad_arg:
        assert call(**kw) == L.GSD_ERR_BAD_ARG, kw
        assert b"gsd_depth_metrics" in L.lib.gsd_last_error(), kw
    for elems in (need - 1, 0, -3):
        assert call(ws_elems=elems) == L.GSD_ERR_WORKSPACE, elems
        assert b"workspace" in L.lib.gsd_last_error()
    torch.cuda.synchronize()
    for buf in (ws, table):
        assert bool((buf == SENT).all()), "a refused call launched something"
    assert call() == L.GSD_OK                       # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert bool((table != SENT).all()) and bool((ws[need:] == SENT).all())
    assert call(contact_eps=0.0) == L.GSD_OK, "a threshold of 0 is legal"
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- end to end
def _model(dims, seed, precision):
    from gelslim_depth_amd.models.unet import UNet
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=dims, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.make_state(3, 1, dims, seed, "conditioned").items()},
                      strict=True)
    return m.to("cuda").train()


def _step(cfg, seed=5, **kw):
    from gelslim_depth_amd.train import TrainStep
    m = _model(cfg[1], seed, cfg[0])
    return m, TrainStep(m, **kw)


def _batches(cfg, k):
    """Depth-like targets: synth's U(-0.9, 0] on about 30 % of the pixels, exactly 0 elsewhere."""
    out = []
    for i in range(k):
        x, t = synth.make_batch(*cfg[2], 40 + i)
        keep = np.random.Generator(np.random.PCG64(90 + i)).random(t.shape) < 0.3
        out.append((torch.from_numpy(x).cuda(), torch.from_numpy(np.where(keep, t, np.float32(0.0)).astype(np.float32)).cuda()))
    return out


def same(a, b, tol=0.0, scale=None):
    """a == b, NaN == NaN, or within tol * (scale or |b|)."""
    if isinstance(b, str) or isinstance(b, int):
        return a == b
    if math.isnan(b):
        return math.isnan(a)
    return abs(a - b) <= tol * (abs(b) if scale is None else scale)


def check_summary(got, want, what):
    """A summary against summarise of the reference's tables.  Counts, ratios of counts, maxima and the peak figures come from
    columns that are equal: equal.  A figure that divides one sum by a count inherits the sum's 2^-32 (a square root halves
    it; the scaling by the unit rounds once more, 2^-53); `bias` is held against `mae`, as column 0 is against column 1."""
    for k in want:
        print(f"{what}: {k} {got[k]!r} ref {want[k]!r}")
    assert list(got) == list(want)
    for k in ("images", "nonfinite_images", "images_without_contact", "max_abs", "contact_iou", "contact_iou_mean", "contact_precision",
              "contact_recall", "peak_mae", "peak_max", "unit_name"):
        assert same(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("mae", "rmse", "contact_mae", "contact_rmse", "slope_mae"):
        assert same(got[k], want[k], 2.0 ** -31), (what, k, got[k], want[k])
    assert same(got["bias"], want["bias"], 2.0 ** -31, want["mae"]), (what, got["bias"], want["bias"])


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_evaluate_metrics_walks_once(cfg, monkeypatch):
    from gelslim_depth_amd.harness import evaluate_loader, evaluate_metrics
    from gelslim_depth_amd.metrics import DepthMetrics, depth_metrics, pairs_per_image, summarise
    spec = DepthMetrics(background=0.0, contact_eps=1e-3, unit=-3.2, unit_name="mm")
    data = _batches(cfg, 3)
    m, step = _step(cfg)
    step(*data[0])
    loader = [{"tactile_image": x, "depth_image": t} for x, t in data]
    want_loss = evaluate_loader(step, loader)
    seen = []
    real = step.evaluate

    def counted(x, **kw):
        out = real(x, **kw)
        assert kw == {"use_ema": True}
        seen.append(out.clone())                    # the engine reuses its output buffer
        return out
    monkeypatch.setattr(step, "evaluate", counted)
    loss, summary, table = evaluate_metrics(step, loader, spec, per_image=True)
    assert len(seen) == len(loader), "one forward per batch"
    assert loss == want_loss and isinstance(loss, float), (loss, want_loss)
    two = evaluate_metrics(step, loader, spec)
    assert len(two) == 2 and two[0] == loss and len(seen) == 2 * len(loader)
    for k in summary:
        assert same(two[1][k], summary[k]), k
    n, k_, h, w = seen[0].shape
    want_table = torch.cat([R.depth_metrics_ref(o, t, spec.background, spec.contact_eps) for o, (_, t) in zip(seen, data)])
    assert table.shape == (3 * n, 16) and table.dtype == torch.float64 and not table.is_cuda
    check_table(table, want_table, f"{cfg[0]} walk")
    # walk order: row i is image i of the pass, bit for bit what the op gives for that batch
    own = torch.cat([depth_metrics(o, t, spec) for o, (_, t) in zip(seen, data)]).cpu()
    assert torch.equal(bits(table), bits(own))
    want = summarise(want_table, (k_ * h * w, pairs_per_image(k_, h, w)), spec)
    check_summary(summary, want, cfg[0])
    assert summary["images"] == 3 * n and summary["nonfinite_images"] == 0 and summary["unit_name"] == "mm"
    assert 0.0 < summary["contact_recall"] <= 1.0 and summary["mae"] > 0 and summary["slope_mae"] > 0
    with pytest.raises(TypeError, match="DepthMetrics"):
        evaluate_metrics(step, loader, spec.spec())
    empty = evaluate_metrics(step, [], spec, per_image=True)
    assert empty[0] == 0.0 and empty[1]["images"] == 0 and math.isnan(empty[1]["mae"]) and empty[2].shape == (0, 16)


def test_fit_with_metrics(tmp_path):
    from gelslim_depth_amd import harness
    from gelslim_depth_amd.metrics import LOG_KEYS, DepthMetrics
    cfg = CONFIGS[0]
    data = [{"tactile_image": x, "depth_image": t} for x, t in _batches(cfg, 3)]
    m, step = _step(cfg)
    lines = []
    H = harness.fit(step, data[:2], data[2:], data[1:2], str(tmp_path / "weights"), "unet_x", max_epochs=2, echo=lines.append,
                    metrics=DepthMetrics(unit=-3.2, unit_name="mm"))
    assert list(H) == ["train_loss", "validation_loss", "test_loss", "validation_metrics", "test_metrics"]
    extra = [l for l in lines if l.startswith("Metrics [mm]: Validation mae ")]
    assert len(extra) == 2 and all(lines[lines.index(l) - 1].startswith("Train loss: ") for l in extra), lines
    for key in ("validation_metrics", "test_metrics"):
        assert len(H[key]) == 2
        for s in H[key]:
            assert s["images"] == cfg[2][0] and s["nonfinite_images"] == 0
            assert all(math.isfinite(s[k]) for k in LOG_KEYS), s
    assert "mae {:.6f}, rmse {:.6f}".format(H["validation_metrics"][1]["mae"], H["validation_metrics"][1]["rmse"]) in extra[1]
    assert len(H["validation_loss"]) == 2 and all(math.isfinite(v) for v in H["validation_loss"])


# ------------------------------------------------------------------------------------------------------------------ two ranks
def test_two_ranks_hold_the_single_process_table(tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29577", os.path.join(REPO, "tests", "depth_metrics_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = [dict(np.load(os.path.join(tmp_path, f"rank{i}.npz"))) for i in range(2)]
    want = "nccl" if (torch.cuda.device_count() >= 2 and os.environ.get("GSD_DDP_BACKEND", "nccl") == "nccl") else "gloo"
    assert all(str(r["backend"]) == want for r in res), "two GPUs or more: the ranks must have met over RCCL"
    for precision in ("fp32", "bf16"):
        for n in (7, 5):
            a, b = ({k[len(f"{precision}/{n}/"):]: v for k, v in r.items() if k.startswith(f"{precision}/{n}/")} for r in res)
            what = f"{precision} {n} samples"
            assert a["table"].shape == (n, 16), "one row per sample: the padded repeat of a short share is not scored"
            assert a["table"].tobytes() == b["table"].tobytes(), what + ": the ranks' tables differ"
            assert a["summary"].tobytes() == b["summary"].tobytes(), what + ": the ranks' summaries differ"
            assert float(a["loss"]) == float(b["loss"]) == float(a["loss_alone"]) == float(b["loss_alone"])
            assert a["summary"][0] == n and a["summary"][1] == 0
            assert a["one_table"].tobytes() == b["one_table"].tobytes()
            differ = int((a["table"].view(np.int64) != a["one_table"].view(np.int64)).any(axis=1).sum())
            print(f"{what}: rows that differ from the single-process table: {differ} of {n}")
            # what only the target decides does not depend on the forward at all
            assert np.array_equal(a["table"][:, [4, 9]], a["one_table"][:, [4, 9]]) and (a["table"][:, 4] > 0).all()
            if precision == "fp32":                 # the fp32 eval forward's bits do not depend on the batch
                assert differ == 0, what
                assert a["summary"].tobytes() == a["one_summary"].tobytes()
                # the loss is evaluate_loader's: a share's loss is rounded to fp32 before the shares of a batch are recombined
                assert abs(float(a["loss"]) - float(a["one_loss"])) <= 2.0 ** -22 * float(a["one_loss"])
