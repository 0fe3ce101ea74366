"""CPU: the refinement past the lattice without a kernel: the twin's Jacobian against difference quotients of
the twin's own depth, the damped step, the refinement of the lattice twin's end poses, the share of points the GPU tests leave
out, and the resources of the new kernels.

    the lattice twin (tests/mesh_pose_ref.py), ellipsoid, 3 levels:  error ( 0.0333333,  0.0444444, -0.0343750), cost 1.1814e-05
    refine_twin from that pose, 10 iterations (`python tests/mesh_pose_refine_ref.py`):
                                                                     error (-8.8e-08, -5.9e-08, 7.5e-08), cost 1.75e-16, 4 accepted
    the same with the width 0.35 mm off and fit_width:               error (0, 0, 1.5e-08), width error 0.0 mm, cost 1.38e-16"""
import os

import numpy as np
import pytest

import mesh_pose_ref as P
import mesh_pose_refine_ref as PR
import mesh_pose_width_ref as PW

# what refine_twin leaves of the lattice twin's error on the ellipsoid, rounded up (mm, mm, rad, and the width in mm)
REFINED_TWIN_ERROR = (1.0e-7, 1.0e-7, 1.0e-7)
REFINED_TWIN_WIDTH_ERROR = 1.0e-7


@pytest.mark.parametrize("plane,flip,invert", [("+y+z", False, False), ("+y+z", True, True), ("+z+x", False, True), ("+z+x", True, False)])
def test_the_jacobian_is_the_derivative_of_the_depth(plane, flip, invert):
    """Central differences of the twin's own R, everything in fp64 (`exact`).  Inside one triangle R is linear in (x, y), and (x, y)
    are linear in a1 and a2 and trigonometric in theta, so the quotient (R(+h) - R(-h)) / 2h differs from J by
      * the rounding of the two R values, 64 * 2^-53 * rscale each (rscale: the magnitudes that enter q), divided by h,
      * for theta the truncation h^2 / 6 * |d^3 R / d theta^3| <= h^2 / 6 * mag (x''' = -x'), nothing for a1 and a2,
      * J's own rounding, 64 * 2^-53 * mag.
    Points: active, not uncertain, and the same winner, still not uncertain, at both probes.  Both channels are both fingers."""
    tri = P.MESHES["ellipsoid"]()
    G = PR.records(tri, plane)
    g = P.contact_width(tri, plane)
    pose = (0.3, -0.4, -0.25)          # a1 [mm], a2 [mm], theta
    size, h = (24, 31), 1e-5
    base = PR.point_terms(G, pose, g, size, 12.0, flip, invert, exact=True)
    checked = np.zeros(2, int)
    for k in range(3):
        up, dn = list(pose), list(pose)
        up[k] += h
        dn[k] -= h
        tu, td = (PR.point_terms(G, p, g, size, 12.0, flip, invert, exact=True) for p in (up, dn))
        ok = base["active"] & ~base["uncertain"] & ~tu["uncertain"] & ~td["uncertain"] & (tu["win"] == base["win"]) & (td["win"] == base["win"])
        ok &= tu["active"] & td["active"]
        quotient = (tu["R"] - td["R"]) / (2 * h)
        tol = 2 * 64 * 2.0 ** -53 * base["rscale"] / (2 * h) + (h * h / 6 * base["mag"][:, k] if k == 2 else 0.0) + 64 * 2.0 ** -53 * base["mag"][:, k]
        diff = np.abs(quotient - base["J"][:, k])
        print(f"{plane} flip={flip} invert={invert} k={k}: {int(ok.sum())} points, worst |quotient - J| {diff[ok].max():.3e} "
              f"(its bound {tol[ok][np.argmax(diff[ok])]:.3e}), largest |J| {np.abs(base['J'][:, k][ok]).max():.3f}")
        assert np.all(diff[ok] <= tol[ok]), (plane, k, float((diff[ok] / tol[ok]).max()))
        assert np.abs(base["J"][:, k][ok]).max() > 0.05          # slopes are there to be wrong about
        checked += ok.reshape(2, -1).sum(axis=1)
    assert np.all(checked >= 3 * 40), checked          # both fingers
    assert not base["J"][np.broadcast_to(~base["active"][:, None], base["J"].shape)].any()          # inactive: exactly 0


def test_normal_row_of_a_rendered_candidate():
    """Entry 0 and 1 are the score row's sum_sq and n_rendered at contact depth 0; the matrix part is symmetric positive."""
    G, t = PR.image_terms("ellipsoid")
    rng = np.random.Generator(np.random.PCG64(3))
    seen = t["R"] + rng.normal(0, 0.05, t["R"].shape)
    for stride in (1, 2, 3):
        row = PR.normal_row(t["R"], t["J"], seen, stride)
        want = P.row_ref(t["R"], seen, stride, 0.0)
        n = P.n_points(40, 53, stride)          # the same non-negative terms in another order
        assert row.shape == (16,) and abs(row[0] - want[0]) <= 2 * n * 2.0 ** -53 * want[0] and row[1] == want[3]
        A = np.zeros((4, 4))
        for n, (j, k) in enumerate(PR.PAIRS):
            A[j, k] = A[k, j] = row[6 + n]
        assert np.all(np.linalg.eigvalsh(A) > 0) and A[3, 3] == 0.25 * row[1]


def spd_row(rng, scale=1.0):
    Jm = rng.normal(0, 1, (40, 4)) * np.array([1.0, 0.7, 3.0, 0.5]) * scale
    e = rng.normal(0, 0.1, 40)
    A, b = Jm.T @ Jm, Jm.T @ e
    return np.concatenate(([e @ e, 40.0], b, [A[j, k] for j, k in PR.PAIRS])), A, b


def test_lm_step():
    rng = np.random.Generator(np.random.PCG64(11))
    row, A, b = spd_row(rng)
    big = (1e9,) * 4
    # lambda -> 0: the Newton step of the normal equations
    dl, _ = PR.lm_solve(row, 0.0, 15, big)
    assert np.allclose(dl, np.linalg.solve(A, -b), rtol=1e-12, atol=0)
    dl3, _ = PR.lm_solve(row, 0.0, 7, big)
    assert dl3[3] == 0.0 and np.allclose(dl3[:3], np.linalg.solve(A[:3, :3], -b[:3]), rtol=1e-12, atol=0)          # a masked width never moves
    lam = 0.3
    dl, M = PR.lm_solve(row, lam, 15, big)
    assert np.allclose(dl, np.linalg.solve(A + lam * np.diag(np.diag(A)), -b), rtol=1e-12, atol=0) and np.allclose(M, A + lam * np.diag(np.diag(A)))
    # the clip, per component
    ms = (1e-3, 1e9, 2e-3, 1e9)
    dc, _ = PR.lm_solve(row, lam, 15, ms)
    assert abs(dc[0]) == 1e-3 and abs(dc[2]) == 2e-3 and dc[1] == dl[1] and dc[3] == dl[3]
    # a pivot that is not positive: no step
    bad = row.copy()
    bad[6 + PR.PAIRS.index((1, 1))] = -1.0
    assert not PR.lm_solve(bad, lam, 15, big)[0].any()
    flat = row.copy()
    flat[6:] = 0.0
    assert not PR.lm_solve(flat, lam, 15, big)[0].any()
    nan = row.copy()
    nan[3] = np.nan
    assert not PR.lm_solve(nan, lam, 15, big)[0].any()


def test_lm_update_accepts_strictly_and_moves_the_damping():
    rng = np.random.Generator(np.random.PCG64(12))
    row, _, _ = spd_row(rng)
    F = np.float32
    state = {"pose": None, "width": None, "lam": 1e-3, "row": None, "accepted": 0}
    start = np.asarray([0.3e-3, -0.4e-3, 0.2], F)
    nxt, nw, dl, _ = PR.lm_update_ref(state, start, F(7.0), row, 7, first=True)
    assert state["lam"] == 1e-3 and state["accepted"] == 0 and np.array_equal(state["pose"], start) and nw == F(7.0)
    assert nxt[0] == F(np.float64(start[0]) + dl[0] / 1000) and nxt[2] == F(np.float64(start[2]) + dl[2])
    for trial0, took in ((row[0], False), (np.nan, False), (np.nextafter(row[0], 0.0), True)):          # equal: no; NaN: no; one ulp less: yes
        st = dict(state, row=state["row"].copy())
        trial = row.copy()
        trial[0] = trial0
        _, _, _, got = PR.lm_update_ref(st, nxt, F(7.5), trial, 7)
        assert got is took and st["accepted"] == int(took) and st["lam"] == (1e-3 * 0.1 if took else 1e-3 * 10.0)
        assert np.array_equal(st["pose"], nxt if took else start) and st["width"] == (F(7.5) if took else F(7.0))
    st = dict(state, row=state["row"].copy(), lam=5e11)
    PR.lm_update_ref(st, nxt, F(7.0), row, 7)
    assert st["lam"] == 1e12          # the bounds hold
    st = dict(state, row=state["row"].copy(), lam=5e-12)
    better = row.copy()
    better[0] *= 0.5
    PR.lm_update_ref(st, nxt, F(7.0), better, 7)
    assert st["lam"] == 1e-12


def test_refinement_beats_the_lattice_on_the_ellipsoid():
    """The feature's point: from the pose the three-level lattice twin ends on, every axis error shrinks and the cost does not rise."""
    res = PR.run_ellipsoid()
    lattice = np.abs(PR.ELLIPSOID_LATTICE_ERROR)
    err = np.abs(res["error"])
    print(f"ellipsoid: lattice error {lattice.tolist()}, refined {res['error'].tolist()}, cost {res['trace'][0]!r} -> {res['cost']!r}, "
          f"{res['accepted']} accepted")
    assert np.all(err < lattice) and np.all(err <= np.asarray(REFINED_TWIN_ERROR))
    assert np.all(np.diff(res["trace"]) <= 0) and res["cost"] == res["trace"][-1] <= res["trace"][0]
    assert abs(res["trace"][0] - 1.1814e-05) < 1e-9          # the start IS the lattice twin's end: its recorded cost
    assert res["accepted"] >= 1 and res["width_error"] == 0.0          # the width was not free


def test_refinement_recovers_a_wrong_width():
    res = PR.run_ellipsoid(fit_width=True, width_error=PW.START_WIDTH_ERROR)
    print(f"ellipsoid, width 0.35 mm off: refined error {res['error'].tolist()}, width error {res['width_error']!r}")
    assert np.all(np.abs(res["error"]) <= np.asarray(REFINED_TWIN_ERROR)) and abs(res["width_error"]) <= REFINED_TWIN_WIDTH_ERROR
    assert np.all(np.diff(res["trace"]) <= 0)


def test_refinement_stays_put_on_the_l_prism_plateau():
    """Seen along its axis the L-prism's caps are flat: every slope is 0, and at the lattice twin's end pose the cost is exactly 0."""
    import mesh_depth_ref as R
    case = P.CASES["lprism"]
    tri = P.MESHES["lprism"]()
    truth, g = P.case_truth(case), PW.true_width(case)
    end = tuple(float(np.float32(t + e)) for t, e in zip(truth, (-0.0074074e-3, -0.0148148e-3, -0.0093750)))
    observed, _ = R.raster_ref(tri, 1.0, P.PLANE, truth, g, case["size"], case["height_mm"], delta=0.0)
    res = PR.refine_twin(tri, P.PLANE, observed, np.float32(g), end, 5)
    assert res["trace"][0] == 0.0 and not res["trace"].any() and res["accepted"] == 0 and not res["last_step"].any()
    assert np.array_equal(res["pose"], np.asarray(end, np.float32))


@pytest.mark.parametrize("name", sorted(PR.IMAGES))
def test_the_uncertain_points_are_few(name):
    """A share condition of the GPU tests, checked here: the mask leaves out at most 2 % of an image's active points."""
    _, t = PR.image_terms(name)
    active = int(t["active"].sum())
    out = int((t["uncertain"] & t["active"]).sum())
    print(f"{name}: {active} active points, {out} uncertain ({100.0 * out / active:.3f} %)")
    assert active >= 80 and out <= PR.UNCERTAIN_CAP * active


def test_refinement_kernels_use_no_scratch():
    """The 15 sums of mesh_pose_normal stay in registers through the four md_wave_sums<4> groups, its four waves meet in 4 x 16
    doubles of LDS, the 4 x 4 system of mesh_pose_lm_update is indexed by constants only (device-only compile, ~5 s)."""
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
    got = {}
    for key in ("mesh_pose_normal_sum", "mesh_pose_normal", "mesh_render_jacobian", "mesh_pose_lm_update"):
        hits = [(s, m) for n, s, m in zip(names, scratch, lds) if re.search(rf"\d{key}E", n)]
        assert len(hits) == 1, (key, names)
        got[key] = hits[0]
    assert got == {"mesh_pose_normal": (0, 4 * 16 * 8), "mesh_pose_normal_sum": (0, 0), "mesh_render_jacobian": (0, 0),
                   "mesh_pose_lm_update": (0, 0)}, got
