"""CPU: the pose search over an unknown grasp width without a kernel: the identity that lets one render
serve every width, the width axis' level schedule against its restatement, the 4-D brute-force twin of estimate_pose, and the
register budget of the two new kernels."""
import os

import numpy as np
import pytest

import mesh_depth_ref as R
import mesh_pose_ref as P
import mesh_pose_width_ref as PW


@pytest.mark.parametrize("name,pose", [("lprism", (0.4e-3, -0.3e-3, 0.35)), ("sphere4", (-0.6e-3, 0.5e-3, -1.2)), ("ellipsoid", (0.3e-3, -0.4e-3, -0.25))])
def test_one_render_at_width_zero_gives_every_width_bitwise(name, pose):
    """min(0, d_0 + g / 2) is raster_ref(..., g, delta=0) bit for bit, on both channels, for widths from 0 to beyond the crest."""
    tri = P.MESHES[name]()
    g_touch = P.contact_width(tri, indent=0.0)
    for flip, invert in ((False, False), (True, True)):
        d0, _ = R.raster_ref(tri, 1.0, P.PLANE, pose, 0.0, (24, 31), 12.0, flip, invert, delta=0.0)
        assert (d0 < 0).any()
        for g in (0.0, float(np.float32(0.35)), g_touch - 1.6, float(np.float32(g_touch - 0.8)), g_touch + 1.0):
            want, _ = R.raster_ref(tri, 1.0, P.PLANE, pose, g, (24, 31), 12.0, flip, invert, delta=0.0)
            got = PW.depth_at_width(d0, g)
            assert got.tobytes() == want.tobytes(), (name, g, flip)
        assert not PW.depth_at_width(d0, g_touch + 1.0).any() and PW.depth_at_width(d0, g_touch - 0.8).any()


def test_width_schedule_middle_offset_and_half_spans():
    from gelslim_depth_amd.mesh_depth import MeshDepthError, width_schedule
    spans, offs = width_schedule(0.6, 5, 4)
    assert spans.dtype == offs.dtype == np.float32 and spans.shape == (5,) and offs.shape == (4, 5)
    assert np.array_equal(spans, PW.width_half_spans(0.6, 5, 4)) and spans[0] == np.float32(0.6)
    for lvl in range(4):
        assert spans[lvl + 1] == np.float32(2) * spans[lvl] / np.float32(4)          # next half-span = this level's step
        assert np.array_equal(offs[lvl], PW.width_offsets(spans[lvl + 1], 5))
        assert offs[lvl, 2] == 0.0 and np.all(np.diff(offs[lvl]) > 0)
        assert offs[lvl, 0] == -spans[lvl] and offs[lvl, 4] == spans[lvl]          # n = 5: (n - 1) / 2 * step is exact
        centre = np.float32(7.75)
        assert (centre + offs[lvl]).astype(np.float32)[2].tobytes() == centre.tobytes()
    assert abs(float(spans[4]) - 0.6 / 16) < 1e-8
    spans9, offs9 = width_schedule(np.float32(1.0), 9, 2)
    assert offs9.shape == (2, 9) and offs9[0, 4] == 0.0 and np.array_equal(spans9, np.float32([1.0, 0.25, 0.0625]))
    for count in (4, 2, 1, 0, -3, 5.0, True, 33, None):
        with pytest.raises(MeshDepthError):
            width_schedule(0.6, count, 4)
    for half in (0.0, -0.6, float("nan"), float("inf"), (0.6, 0.6), None):
        with pytest.raises(MeshDepthError):
            width_schedule(half, 5, 4)
    with pytest.raises(MeshDepthError):
        width_schedule(0.6, 5, 0)


def check_twin(name, res, levels):
    trace = res["trace"]
    assert len(trace) == levels and np.all(np.diff(trace) <= 0), trace
    assert res["cost"] == trace[-1] == P.pose_cost_ref(res["row"], "mse", P.n_points(24, 31, 1))
    step = float(res["final_width_step"])
    assert step == float(PW.width_half_spans(PW.WIDTH_HALF_SPAN, PW.WIDTH_COUNT, levels)[-1])
    print(f"{name}: twin error (mm, mm, rad) {res['error'].tolist()}, width error {res['width_error']!r} mm, final width step {step!r} mm, "
          f"cost {res['cost']!r}")
    assert abs(res["width_error"]) <= step, (res["width_error"], step)
    assert abs(res["width_error"]) < PW.START_WIDTH_ERROR / 4          # the 0.35 mm of the start are gone


def test_the_twin_recovers_the_l_prism_pose_and_width():
    """The l-prism case of tests/test_gpu_mesh_pose_width.py by brute force (1,764 fp64 renders at width 0, 8,820 rows): the width
    error ends within the final width step, the best cost never rises, and the figures are the ones the GPU test holds."""
    from test_gpu_mesh_pose_width import BOUND, FINAL_STEP, TWIN_ERROR
    res = PW.run_case("lprism", verbose=False)
    assert res["renders"] == 4 * 441
    check_twin("lprism", res, 4)
    err = np.abs(np.append(res["error"], res["width_error"]))
    step = np.array([1e3 * res["final_step"][0], 1e3 * res["final_step"][1], res["final_step"][2], float(res["final_width_step"])])
    assert np.allclose(step, FINAL_STEP["lprism"], rtol=1e-6, atol=0)
    assert np.all(err <= np.asarray(TWIN_ERROR["lprism"])), (err, TWIN_ERROR["lprism"])
    assert np.all(err <= np.asarray(BOUND["lprism"]) / 3)


def test_the_twin_recovers_the_width_of_a_smooth_asymmetric_object():
    """The ellipsoid with the counts (5, 5, 7) (525 renders; the case's own (7, 7, 9) take 45 s and are run by
    `python tests/mesh_pose_width_ref.py`, whose figures the GPU test holds)."""
    res = PW.run_case("ellipsoid", counts=(5, 5, 7), verbose=False)
    assert res["renders"] == 3 * 175
    check_twin("ellipsoid", res, 3)


def test_width_kernels_use_no_scratch():
    """The loop over the widths of mesh_pose_score_widths keeps its per-width values in registers (groups of at most four, fully
    unrolled): no private array, no scratch, in every instantiation, none in mesh_pose_score, and none in the one rows kernel that
    serves them all (device-only compile, ~5 s)."""
    import re
    import shutil
    import subprocess
    from gelslim_depth_amd import build as b
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this machine")
    r = subprocess.run([hipcc] + b.CFLAGS + [f"-I{b.INCLUDE}", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(b.CSRC, "gsd_mesh_depth.hip"), "-o", os.devnull], capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(lds)
    score = {n: (s, m) for n, s, m in zip(names, scratch, lds) if "mesh_pose_score" in n}
    rows = {n: (s, m) for n, s, m in zip(names, scratch, lds) if "mesh_pose_rows" in n}
    assert len(score) == 3 and len(rows) == 1, r.stderr[-2000:]          # one width, CH = 2, CH = 4; one rows kernel for every G
    # four waves' partials: of 32 widths (5 KiB) in the kernel for several, of the one width in mesh_pose_score
    assert all(v == (0, 4 * 32 * 5 * 8 if "widths" in n else 4 * 5 * 8) for n, v in score.items()), score
    assert all(v == (0, 0) for v in rows.values()), rows
