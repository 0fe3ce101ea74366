"""GPU: the geometry units and the data path write what they return -- results do not depend on what memory held.

mesh_depth, contact_points, contact_patches, mesh_register, touch_fusion, metrics, dataset and processing take some sixty buffers
from torch.empty / empty_like / new_empty: cell tables and lists, scan offsets stored in place in a workspace, partial rows, count
tables, padded outputs whose tail a fill loop shared out over the blocks writes, LM states and traces.  Every workload of
geometry_state.WORKLOADS runs with all of them handed out full of 0, of NaN and of +3.0e4 (engine_state.poison; integers: 0x5A
bytes), and every tensor it returns -- every output and every tensor attribute of the returned objects, the cell lists with their
segments sorted -- must hold the same bits under all three, and the bits of a run that poisons nothing.

No region of any output is left out of the comparison: neither a docstring nor DESIGN.md calls any part of them unspecified.
NOT_FINITE names the outputs that hold NaN or an infinity by contract, each with the sentence that says so; they are compared bit
for bit like the rest and only exempt from same_bits' finiteness check.

test_a_dirty_row_behind_the_image_is_rejected proves that the comparison sees: render_depth is handed, as `out=`, the front of a
buffer one image row longer than the images; the row behind them is never written, the workload returns the whole buffer, and the
comparison fails under both patterns.  The dirty border is the test's own, nothing of the package is changed.

Buffers poisoned per run (the same number under every pattern): mesh_grid 84, contact 105, mesh_volume 25, touch_fusion 12,
metrics_data 17; tensors compared: 60, 98, 27, 12, 8.  Measured on an MI355X: 17 tests in 3.5 s; the first run of a workload takes
0.6 s (mesh_grid), 0.4 s (contact) and 0.2 s (the others) for its four runs, every other test 0.01 s.  No difference was found.
"""
import pytest
import torch

import engine_state as E
import geometry_state as S

pytestmark = pytest.mark.gpu

POINTS = [f"points.{f}.s{s}.{l}" for f in S.CONTACT_FRAMES for s in (1, 2) for l in S.CONTACT_LAYOUTS]
NOT_FINITE = {
    "mesh_grid": (),
    "contact": tuple(
        # ContactPatches: "The properties derive physical quantities from `stats` in fp64 on the device, (B, 2, K) each, NaN in rows
        # without a patch" -- the image of zeros has no patch, and no plane fills more rows than it has patches; peak_depth is "the
        # depth of the deepest pixel", -inf for the blob that holds the -inf pixel
        [f"patches{c}.{n}" for c in S.CONTACT_CONNECTIVITY for n in S.PATCH_PROPERTIES if n not in ("peak_rc", "bbox")]
        # filtered_depth: "`depth` bit for bit, except +0.0 where a pixel is contact and its patch is not kept": the input's NaN
        # pixels pass through, its -inf pixel where the blob is kept
        + [f"patches{c}.filtered" for c in S.CONTACT_CONNECTIVITY]
        # depth_points, padded: "NaN beyond an image's points"; every layout: the -inf pixel is a point ("a pixel ... is a point iff
        # its depth d < -contact_depth; a NaN is not") whose third coordinate and whose neighbours' normals are made of that -inf
        + [f"{p}.{n}" for p in POINTS for n in ("points", "normals")]),
    # closest_points: "No winner, or a point with a non-finite coordinate: triangle -1, closest NaN, distance and sq_distance +inf"
    # (row 7 of the cloud is NaN; with a limit most points have no winner)
    "mesh_volume": tuple(f"closest.{l}.{n}" for l in ("all", "near") for n in ("closest", "distance", "sq_distance")),
    # TouchSurface: "Padded (`max_triangles=M`): (M, 3, 3) / (M,), the first min(count, M) triangles, then NaN (cell: -1)"
    "touch_fusion": ("surface.above.triangles",),
    "metrics_data": (),
}
CLEAN = "clean"
_STAGED, _RUNS, _FILLED = {}, {}, {}


def staged(name):
    if name not in _STAGED:
        _STAGED[name] = S.WORKLOADS[name].stage()
    return _STAGED[name]


def run(name, monkeypatch, pattern):
    """The workload's results under one pattern (CLEAN: nothing is poisoned), as host copies; made once per process."""
    if (name, pattern) not in _RUNS:
        inputs = staged(name)
        if pattern == CLEAN:
            res = S.WORKLOADS[name].run(inputs)
        else:
            with E.poison(monkeypatch, pattern) as p:
                res = S.WORKLOADS[name].run(inputs)
            _FILLED[name, pattern] = p.filled
        torch.cuda.synchronize()
        _RUNS[name, pattern] = {k: E.snap(v) for k, v in res.items()}
    return _RUNS[name, pattern]


@pytest.mark.parametrize("pattern", [E.NAN, E.BIG])
@pytest.mark.parametrize("name", list(S.WORKLOADS))
def test_results_do_not_depend_on_what_memory_held(monkeypatch, capsys, name, pattern):
    zero, other = run(name, monkeypatch, E.ZERO), run(name, monkeypatch, pattern)
    with capsys.disabled():
        print(f"\n{name}: {len(zero)} tensors compared, {_FILLED[name, E.ZERO]} buffers poisoned under {E.ZERO}, {_FILLED[name, pattern]} under {pattern}")
    assert _FILLED[name, E.ZERO] > 0 and _FILLED[name, pattern] == _FILLED[name, E.ZERO]
    E.same_results(zero, other, f"{name}: {E.ZERO} against {pattern}", not_finite=NOT_FINITE[name])


@pytest.mark.parametrize("name", list(S.WORKLOADS))
def test_zeroed_memory_gives_the_unpoisoned_result(monkeypatch, name):
    E.same_results(run(name, monkeypatch, CLEAN), run(name, monkeypatch, E.ZERO), f"{name}: unpoisoned against {E.ZERO}", not_finite=NOT_FINITE[name])


def test_the_workloads_reach_what_they_are_meant_to(monkeypatch):
    """A workload that stops reaching its path fails here instead of passing vacuously."""
    c = run("contact", monkeypatch, CLEAN)
    for conn in S.CONTACT_CONNECTIVITY:
        counts, stats = c[f"patches{conn}.counts"], c[f"patches{conn}.stats"]
        assert int(counts.max()) > stats.shape[2] == 2, "a plane holds more patches than max_patches"
        assert int(counts[2].max()) == 0 and not bool(stats[2].any()), "rows without a patch are zero"
        assert int((stats[..., 0] > 0).sum()) >= 6 and bool((stats[..., 0][stats[..., 0] > 0] >= 3).all())
    for frame in S.CONTACT_FRAMES:
        for stride in (1, 2):
            packed, below, above = (c[f"points.{frame}.s{stride}.{l}.points"] for l in S.CONTACT_LAYOUTS)
            per_image = c[f"points.{frame}.s{stride}.packed.counts"].sum(dim=1)
            assert packed.shape[0] == int(per_image.sum()) and below.shape[1] < int(per_image.max()) < above.shape[1]
            assert bool(torch.isnan(above[2]).all()), "the image of zeros is all padding"
    v = run("mesh_volume", monkeypatch, CLEAN)
    assert int(v["closest.all.triangle"][7]) == -1 and int((v["closest.all.triangle"] < 0).sum()) == 1
    assert 100 < int((v["closest.near.triangle"] < 0).sum()) < 1000 and int(v["register.accepted"].sum()) >= 2
    t = run("touch_fusion", monkeypatch, CLEAN)
    n = int(t["surface.packed.count"])
    assert t["surface.below.triangles"].shape[0] == n - 37 and t["surface.above.triangles"].shape[0] == n + 41
    assert bool(torch.isnan(t["surface.above.triangles"][n:]).all()) and bool((t["surface.above.cell"][n:] == -1).all())
    g = run("mesh_grid", monkeypatch, CLEAN)
    for mesh in ("lprism", "ellipsoid3"):
        assert E.snap(g[f"{mesh}.render"]).equal(g[f"{mesh}.render_out"]) and int((g[f"{mesh}.render"] < 0).sum()) > 100
    # (the L prism's caps are flat, its Jacobian is zero and no step is ever taken: the ellipsoid is the one that moves)
    assert int(g["ellipsoid3.refine0.accepted"].sum()) + int(g["ellipsoid3.refine1.accepted"].sum()) >= 1


# ------------------------------------------------------------------------------------- proof that the comparison can see
def test_a_dirty_row_behind_the_image_is_rejected(monkeypatch):
    from gelslim_depth_amd import mesh_depth as M
    import mesh_pose_ref as P
    s = staged("mesh_grid")["lprism"]
    h, w = S.SIZE
    grid = M.MeshGrid(s["tri"], 1.0, P.PLANE, S.DEV)
    res = {}
    for pattern in E.PATTERNS:
        with E.poison(monkeypatch, pattern):
            buf = torch.empty((2 * 2 * h * w + w,), device=S.DEV, dtype=torch.float32)
            out = buf[:2 * 2 * h * w].view(2, 2, h, w)
            assert M.render_depth(grid, s["seen"], s["widths"], S.SIZE, 12.0, out=out) is out
            res[pattern] = {"images": E.snap(out), "buffer": E.snap(buf)}
    for pattern in (E.NAN, E.BIG):
        E.same_results({"images": res[E.ZERO]["images"]}, {"images": res[pattern]["images"]}, f"the images themselves: {pattern}")
    with pytest.raises(AssertionError, match="differ in their bits"):
        E.same_results(res[E.ZERO], res[E.BIG], "a dirty row behind the images: zero against big")
    with pytest.raises(AssertionError, match="not finite"):
        E.same_results(res[E.ZERO], res[E.NAN], "a dirty row behind the images: zero against nan")
