"""Results do not depend on what memory held.

Every buffer the package takes from torch.empty / empty_like / new_empty is handed out filled with 0, with NaN and with +3.0e4
(engine_state.poisoned), and every result of every workload must be the same bits under all three -- and finite.  A launch
that reads a partial row, a pad column, a workspace tail or a halo it did not write gives different numbers under at least
one of them.  The case tables take the smallest shapes that still switch every buffer class of the two engines on; the module
checks that they do (test_every_plan_flag_was_seen_both_ways) and prints what each case reached.

Two mutations prove that the comparison can see: a concat buffer that is not zeroed, and one dirty element in a border that
nothing writes, are both rejected.
"""
import pytest
import torch

import engine_state as S
from engine_state import Case

pytestmark = pytest.mark.gpu

F32 = [16, 32, 64]
W2D = {"GSD_CONV_W2D": "1"}
FORCED = {"GSD_CONV_W2D": "1", "GSD_ACT_ONCE_FORCE": "1"}
FP32_CASES = [
    # the three environments of test_engine_act_once_equals_deferred (plans (0, 0, 0), (0, 0, 2), (5, 2, 2)) ...
    Case("fp32-default", "fp32", F32, 2, 40, 53),
    Case("fp32-w2d", "fp32", F32, 2, 40, 53, W2D),
    Case("fp32-w2d-forced", "fp32", F32, 2, 40, 53, FORCED),
    # ... and at 37 x 45, where level 0 is odd by odd: the up-sampled tensor is one row and one column short of its level
    Case("fp32-default-37x45", "fp32", F32, 2, 37, 45),
    Case("fp32-w2d-37x45", "fp32", F32, 2, 37, 45, W2D),
    Case("fp32-w2d-forced-37x45", "fp32", F32, 2, 37, 45, FORCED),
    # K slabs (test_gpu_kslabs.py's switches, forced to two slabs): the 64-channel launches of levels 1 and 2 sum through conv_ws,
    # in the row form (with the 2-D form off: by default it takes exactly these launches) and in the 2-D form
    Case("fp32-kslabs", "fp32", F32, 2, 40, 53, {"GSD_CONV_W2D": "0", "GSD_W43_SPLIT": "2"}),
    Case("fp32-kslabs-w2d", "fp32", F32, 2, 40, 53, {"GSD_CONV_W2D": "1", "GSD_W2D_SPLIT": "2"}),
    Case("fp32-two-classes", "fp32", F32, 2, 40, 53, n_classes=2),         # outw_partials / outw_sums
    Case("fp32-one-stream", "fp32", F32, 2, 40, 53, {"GSD_SIDE_DW": "0"}),
    Case("fp32-first-unfused", "fp32", F32, 2, 40, 53, {"GSD_WGRAD_FIRST": "0"}),   # the first layer's d_raw is materialised
    # BatchNorm's column sums and finalize as separate launches in both directions, staged through u.sums: the form full-size
    # layers (more than 4096 partial rows) and SyncBN take, which no shape this small reaches on its own
    Case("fp32-bn-three-launch", "fp32", F32, 2, 40, 53, {"GSD_BN_ONE_LAUNCH_ROWS": "0"}),
]
B16 = [32, 64, 128]
BF16_CASES = [
    Case("bf16-21x27", "bf16", B16, 2, 21, 27),
    Case("bf16-inc-c64", "bf16", [64, 128], 2, 20, 26),                    # fused `inc` block and the weights-resident 64 -> 64 kernel
    Case("bf16-im2col", "bf16", [64, 128], 2, 20, 26, {"GSD_BF16_FIRST": "0"}),       # the first layer through col0
    Case("bf16-one-stream", "bf16", B16, 2, 21, 27, {"GSD_BF16_SIDE_DW": "0"}),
    Case("bf16-19x23", "bf16", B16, 2, 19, 23),                            # odd by odd at both levels: a border on every concat buffer
    # the remaining engine switches, so that every plan flag is seen off as well
    Case("bf16-unfused", "bf16", [64, 128], 2, 20, 26, {"GSD_BF16_APPLY_POOL": "0", "GSD_BF16_C64": "0", "GSD_BF16_FUSED_OUT": "0",
                                                       "GSD_BF16_FUSED_INC": "0"}),
]
CASES = FP32_CASES + BF16_CASES
BY_NAME = {c.name: c for c in CASES}
FLAGS = {"fp32": ("act_once", "cat_on", "pooled_pitched", "pitched", "fused_dw", "conv_ws", "side", "bn_one_launch"),
         "bf16": ("first_direct", "fused_inc", "apply_pool", "c64", "fused_out", "side_dw")}
SWITCHES = sorted({k for c in CASES for k in c.env})

_FLAGS_SEEN = {}          # case name -> {flag: set of values over the engine (and, for per-unit flags, over its units)}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in SWITCHES + ["GSD_ACT_ONCE", "GSD_W2D_X4", "GSD_W2D_U4", "GSD_WGRAD_W2D"]:
        monkeypatch.delenv(k, raising=False)


def engine_flags(eng):
    """The plan flags of an engine whose buffers a train-mode forward has sized."""
    if getattr(eng, "precision", "fp32") == "bf16":
        c64 = any(eng._use_c64(u.cin, u.cout) for u in eng.units if not u.first)
        return {"first_direct": {eng.first_direct}, "fused_inc": {eng.fused_inc}, "apply_pool": {eng.apply_pool}, "c64": {c64},
                "fused_out": {eng.fused_out}, "side_dw": {eng.side_dw}}
    return {"act_once": {u.plan.act_once for u in eng.units}, "cat_on": {up.plan.cat_on for up in eng.ups},
            "pooled_pitched": set(eng.plan.pooled_pitched[1:]), "pitched": {u.plan.pitched for u in eng.units},
            "fused_dw": {u.plan.fused_dw for u in eng.units}, "conv_ws": {eng.conv_ws is not None}, "side": {eng.side is not None},
            "bn_one_launch": {eng.one_launch_rows > 0}}      # (no layer of these cases has more than a few hundred partial rows)


def run_patterns(monkeypatch, workload, case):
    out = {}
    for pattern in S.PATTERNS:
        with S.poison(monkeypatch, pattern) as p:
            res, eng = S.WORKLOADS[workload](case)
            assert p.filled > 0, "the workload allocated nothing through the patched functions"
        out[pattern] = res
        if workload.startswith("train_steps"):
            _FLAGS_SEEN[case.name] = engine_flags(eng)
    return out


@pytest.mark.parametrize("workload", list(S.WORKLOADS))
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_results_do_not_depend_on_what_memory_held(monkeypatch, case, workload):
    res = run_patterns(monkeypatch, workload, case)
    for pattern in (S.NAN, S.BIG):
        S.same_results(res[S.ZERO], res[pattern], f"{case.name} {workload}: {S.ZERO} against {pattern}")


def test_every_plan_flag_was_seen_both_ways(monkeypatch, capsys):
    """A case that stops reaching its path fails here instead of passing vacuously.  Per-unit flags (act_once, pitched, fused_dw)
    and per-level ones (cat_on, pooled_pitched) count a value as seen when any unit / level of any case has it."""
    for case in CASES:
        if case.name not in _FLAGS_SEEN:      # (this test selected alone: one step per case sizes the buffers)
            _, eng = S.train_steps(case, k=1)
            _FLAGS_SEEN[case.name] = engine_flags(eng)
    lines = []
    for precision, names in FLAGS.items():
        lines.append(f"{precision:<24}" + "".join(f"{n:>15}" for n in names))
        for case in CASES:
            if case.precision == precision:
                f = _FLAGS_SEEN[case.name]
                lines.append(f"{case.name:<24}" + "".join(f"{'/'.join('01'[v] for v in sorted(f[n])):>15}" for n in names))
    with capsys.disabled():
        print("\nplan flags reached (0: seen off, 1: seen on, 0/1: both among the case's units or levels)\n" + "\n".join(lines))
    for precision, names in FLAGS.items():
        for n in names:
            seen = set().union(*[_FLAGS_SEEN[c.name][n] for c in CASES if c.precision == precision])
            assert seen == {False, True}, f"{precision} {n}: only {sorted(seen)} over the whole case table"
    forced = _FLAGS_SEEN["fp32-w2d-forced"]
    assert forced["act_once"] == {False, True} and forced["cat_on"] == {True} and forced["pooled_pitched"] == {True}, forced
    assert _FLAGS_SEEN["fp32-kslabs"]["conv_ws"] == {True} and _FLAGS_SEEN["fp32-kslabs-w2d"]["conv_ws"] == {True}
    assert _FLAGS_SEEN["bf16-inc-c64"]["fused_inc"] == {True} and _FLAGS_SEEN["bf16-inc-c64"]["c64"] == {True}
    assert _FLAGS_SEEN["bf16-im2col"]["first_direct"] == {False}


# ------------------------------------------------------------------------------------- proof that the comparison can see
def test_an_unzeroed_concat_buffer_is_rejected(monkeypatch):
    """fp32, forced plan: pitched_slack_zeros hands out poisoned memory instead of zeros.  The conv3x3 and dW launches read the
    pad columns of the concat buffers and of the pitched pooled tensors as their zero padding: wrong numbers from readable
    memory under NaN and under +3.0e4, so both comparisons must fail."""
    from gelslim_depth_amd import _lib

    def unzeroed(shape, device):
        n, c, h, w = shape
        p = -(-w // 4) * 4
        numel = n * c * h * p
        buf = torch.empty((numel + 2 * _lib.SLACK,), device=device, dtype=torch.float32)
        return buf[_lib.SLACK:_lib.SLACK + numel].view(n, c, h, p)[..., :w]

    monkeypatch.setattr(_lib, "pitched_slack_zeros", unzeroed)
    case = BY_NAME["fp32-w2d-forced"]
    res = {}
    for pattern in S.PATTERNS:
        with S.poison(monkeypatch, pattern):
            res[pattern], eng = S.train_steps(case)
        assert sum(up.plan.cat_on for up in eng.ups) == 2 and sum(eng.plan.pooled_pitched) == 2
    with pytest.raises(AssertionError, match="differ in their bits"):      # finite, and wrong
        S.same_results(res[S.ZERO], res[S.BIG], "unzeroed concat buffers: zero against big")
    with pytest.raises(AssertionError):       # (different bits or non-finite, as far as an fmaxf on the way swallows the NaN)
        S.same_results(res[S.ZERO], res[S.NAN], "unzeroed concat buffers: zero against nan")


def test_one_dirty_border_element_is_rejected(monkeypatch):
    """bf16 at 19 x 23: after the first step, +3.0e4 in one element of the F.pad border of the `up` slice of cat[0] (the last
    row: the transposed convolution writes 18 of the 19).  Nothing writes it back to 0, the decoder's first convolution and its
    dW read it: the second step's results differ from the clean run's."""
    case = BY_NAME["bf16-19x23"]

    def dirty(model, step, i):
        if i == 1:
            eng = model._engine
            assert eng._pad_off(0) == (0, 0) and 2 * eng.hs[1] == eng.hs[0] - 1
            eng.cat[0][0, -1, 3, eng.dims[0] + 1] = S.VALUES[S.BIG]

    with S.poison(monkeypatch, S.ZERO):
        clean, _ = S.train_steps(case)
        again, _ = S.train_steps(case)
        mutated, _ = S.train_steps(case, hook=dirty)
    S.same_results(clean, again, "the clean run repeats")
    with pytest.raises(AssertionError, match="differ in their bits"):
        S.same_results(clean, mutated, "one dirty border element")


# ------------------------------------------------------------------------------------- the other users of torch.empty
def _three(monkeypatch, fn, what, not_finite=()):
    res = {}
    for pattern in S.PATTERNS:
        with S.poison(monkeypatch, pattern) as p:
            res[pattern] = {k: S.snap(v) for k, v in fn().items()}
            assert p.filled > 0, what
    for pattern in (S.NAN, S.BIG):
        S.same_results(res[S.ZERO], res[pattern], f"{what}: {S.ZERO} against {pattern}", not_finite=not_finite)


def _pair(n=2, k=1, h=24, w=31, seed=3):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    out = (torch.rand((n, k, h, w), generator=g) * -0.9).cuda()
    tgt = (torch.rand((n, k, h, w), generator=g) * -0.9).cuda()
    tgt[:, :, : h // 3] = 0.0       # background rows: the contact masks have both classes
    return out, tgt


@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_loss_fwd_bwd(monkeypatch, kind):
    from gelslim_depth_amd import train
    out, tgt = _pair()

    def run():
        grad = torch.empty_like(out)
        loss = torch.empty((1,), device="cuda")
        ws = torch.empty((2048,), device="cuda", dtype=torch.float64)
        train.loss_fwd_bwd(kind, out, tgt, grad, loss, ws)
        o = out.clone().requires_grad_(True)
        auto = (train.mse_loss if kind == "mse" else train.l1_loss)(o, tgt)
        auto.backward()
        return {"loss": loss, "grad": grad, "autograd.loss": auto, "autograd.grad": o.grad}
    _three(monkeypatch, run, f"loss_fwd_bwd {kind}")


def test_depth_loss_fwd_bwd(monkeypatch):
    from gelslim_depth_amd import train
    out, tgt = _pair(k=2)
    spec = S.rich_step_kwargs()["loss"]

    def run():
        grad = torch.empty_like(out)
        terms = torch.empty((6,), device="cuda")
        ws = torch.empty((train.depth_loss_workspace(out.shape),), device="cuda", dtype=torch.float64)
        train.depth_loss_fwd_bwd(spec, out, tgt, grad, terms, ws)
        o = out.clone().requires_grad_(True)
        auto = train.depth_loss(o, tgt, spec)
        auto.backward()
        return {"terms": terms, "grad": grad, "autograd.loss": auto, "autograd.grad": o.grad}
    _three(monkeypatch, run, "depth_loss_fwd_bwd")


def test_depth_metrics(monkeypatch):
    from gelslim_depth_amd.metrics import DepthMetrics, depth_metrics
    out, tgt = _pair(n=3)
    spec = DepthMetrics(background=0.0, contact_eps=1e-3)
    _three(monkeypatch, lambda: {"table": depth_metrics(out, tgt, spec)}, "depth_metrics")


def test_gather_augment(monkeypatch):
    from gelslim_depth_amd.dataset import Augment, gather_affine, gather_augment
    g = torch.Generator(device="cpu")
    g.manual_seed(9)
    img = (torch.rand((5, 3, 24, 31), generator=g) * 255).cuda()
    dep = (torch.rand((5, 1, 24, 31), generator=g) * -2).cuda()
    idx = torch.tensor([4, 0, 2], dtype=torch.int64).cuda()
    ai, bi = torch.tensor([0.5, 0.25, 2.0]).cuda(), torch.tensor([-1.0, 0.5, 0.0]).cuda()
    ad, bd = torch.tensor([0.5]).cuda(), torch.tensor([0.1]).cuda()
    aug = Augment(seed=3, hflip=0.5, vflip=0.5, max_shift=(3, 4), gain=0.1, offset=5.0, noise_std=2.0)

    def run():
        a, b = gather_augment(img, dep, idx, ai, bi, ad, bd, aug, epoch=2)
        return {"image": a, "depth": b, "plain": gather_affine(img, idx, ai, bi)}
    _three(monkeypatch, run, "gather_augment")


def test_device_loader_batches_with_augmentation(monkeypatch):
    """DeviceLoader's batch gather with every augmentation kind on, the dataset's ingest (resize, blur, statistics) included."""
    from gelslim_depth_amd.dataset import Augment, DeviceDataset, DeviceLoader
    from oracle import dataset_ref as dr
    objects = dr.synthetic_objects(41, [3, 2], h=42, w=54)
    aug = Augment(seed=3, hflip=0.5, vflip=0.5, max_shift=(3, 4), gain=0.1, offset=5.0, noise_std=2.0)

    def run():
        ds = DeviceDataset(objects=objects, device="cuda", use_difference_image=True, image_normalization_method="0_255_to_0_1",
                           depth_normalization_method="min_max_to_0_-1", norm_scale=0.9)
        torch.manual_seed(17)
        res = {}
        for i, batch in enumerate(DeviceLoader(ds, 4, shuffle=True, augment=aug)):     # (a full batch and a ragged one)
            res.update({f"{i}.{k}": v for k, v in batch.items() if isinstance(v, torch.Tensor)})
        return res
    _three(monkeypatch, run, "DeviceLoader(augment=...)")


@pytest.mark.parametrize("mode", ["area", "bilinear"])
def test_resize_affine(monkeypatch, mode):
    from gelslim_depth_amd.processing import resize_affine
    g = torch.Generator(device="cpu")
    g.manual_seed(4)
    x = (torch.rand((2, 3, 24, 31), generator=g) * 255).cuda()
    base = (torch.rand((2, 3, 24, 31), generator=g) * 255).cuda()
    _three(monkeypatch, lambda: {"out": resize_affine(x, (11, 13), [0.5, 1.0, 2.0], [0.0, -1.0, 3.0], base=base, mode=mode)},
           f"resize_affine {mode}")


def test_mesh_depth_calls(monkeypatch):
    """render_depth, score_poses, score_poses_widths, pose_normal_rows and refine_pose on the sphere2 mesh at 24 x 31; the grid
    (records, cell table, triangle lists) is built under the pattern too."""
    import mesh_depth_ref as R
    import mesh_pose_ref as P
    from gelslim_depth_amd import mesh_depth as M
    size, height = (24, 31), 12.0
    tri = R.sphere(2, 3.0, (1.0, -0.5, 0.25))        # test_gpu_mesh_depth.py's sphere2
    gw = P.contact_width(tri)
    widths = torch.tensor([gw, gw - 0.3], dtype=torch.float32).cuda()
    seen = torch.tensor([[0.6e-3, -0.45e-3, 0.45], [-0.4e-3, 0.35e-3, -1.1]], dtype=torch.float32).cuda()
    g = torch.Generator(device="cpu")
    g.manual_seed(1)
    cand = (seen.cpu()[:, None, :] + (torch.rand((2, 7, 3), generator=g) * 2 - 1) * torch.tensor([1.5e-3, 1.5e-3, 0.6])).cuda().contiguous()
    many = torch.stack([widths, widths - 0.2, widths - 0.4], dim=1).contiguous()

    def run():
        grid = M.MeshGrid(tri, 1.0, P.PLANE, "cuda:0")
        observed = M.render_depth(grid, seen, widths, size, height)
        res = {"render": observed,
               "score": M.score_poses(grid, observed, cand, widths, height),
               "score_widths": M.score_poses_widths(grid, observed, cand, many, height),
               "normal_rows": M.pose_normal_rows(grid, observed, cand, widths, height)}
        r = M.refine_pose(grid, observed, widths, cand[:, :2].contiguous(), iterations=3, fit_width=True, image_height_mm=height)
        res.update({"refine." + k: getattr(r, k) for k in ("pose", "width", "cost", "normal_row", "trace", "accepted", "last_step")})
        return res
    _three(monkeypatch, run, "mesh_depth")
