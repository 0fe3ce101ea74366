"""Test helpers for the pose refinement of gelslim_depth_amd.mesh_depth (numpy, fp64, no GPU; nothing here is product code),
DESIGN.md section 19 restated by brute force over all triangles:

  * `records`: the fp32 triangle records as gsd_mesh_depth_count forms them (vertices relative to the fp32 grid centre, sorted
    lexicographically, 1 / doubled area from two rounded products),
  * `frame`: a pixel's point in the mesh frame; u, v, pa, pb, da, db in np.float32 with the kernel's expressions, so that the
    derivatives of x and y see the floats the kernel sees (`exact=True`: everything in fp64 from fp64 parameters, for difference
    quotients),
  * `point_terms`: per point the winner (largest sg * q among the covering triangles, THE LOWEST ID among equal values), R, the
    Jacobian J (a1 [mm], a2 [mm], theta [rad]) and the `uncertain` mask: within delta = 16 * 2^-23 * coord_max
    (mesh_depth_ref.raster_ref's) either the winner can change -- the winner is not delta inside its own triangle, or another
    covering or nearly covering triangle's value is within the slope * delta slack of the winner's -- or the active state can,
    |m - g/2| within that slack,
  * `normal_row`: the 16 doubles of a candidate, `lm_update_ref`: the damped step with the kernel's Cholesky order,
    `refine_twin`: refine_pose for one observation.

`python tests/mesh_pose_refine_ref.py` runs the twin on the cases and prints the figures the tests hold as constants."""
import math

import numpy as np

import mesh_depth_ref as R
import mesh_pose_ref as P
import mesh_pose_width_ref as PW

NROW = 16          # sum e^2, #active, sum J_k e (a1, a2, theta, g), sum J_j J_k (j <= k, row-major upper triangle)
PAIRS = [(j, k) for j in range(4) for k in range(j, 4)]
F = np.float32


# ---- the records ------------------------------------------------------------------------------------------------------------
def records(tri, plane=P.PLANE, pc_scale=1.0):
    """dict: rec (T, 10) fp32 = x0, y0, x1, y1, x2, y2, q0, q1, q2, inv (0: skipped); cx, cy fp32; swap_axes; coord_max."""
    a, b, q, aligned_first = R.prepare(tri, pc_scale, plane)
    cx, cy = F(0.5 * (a.min() + a.max())), F(0.5 * (b.min() + b.max()))
    v = np.stack((a - float(cx), b - float(cy), q), axis=2).astype(F)          # (T, 3, 3): the prepared vertices, rounded once
    order = np.lexsort((v[:, :, 1], v[:, :, 0]), axis=1)                        # by x, then y
    v = np.take_along_axis(v, order[:, :, None], axis=1)
    ax, ay, bx, by, cxx, cyy = v[:, 0, 0], v[:, 0, 1], v[:, 1, 0], v[:, 1, 1], v[:, 2, 0], v[:, 2, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        area = (bx - ax) * (cyy - ay) - (by - ay) * (cxx - ax)                  # fp32: two rounded products, one difference
        inv = F(1.0) / area
    ok = (area != 0) & np.isfinite(area) & np.isfinite(inv) & (inv != 0) & np.isfinite(v[:, :, 2]).all(axis=1)
    rec = np.stack((ax, ay, bx, by, cxx, cyy, v[:, 0, 2], v[:, 1, 2], v[:, 2, 2], np.where(ok, inv, F(0))), axis=1).astype(F)
    return {"rec": rec, "cx": cx, "cy": cy, "swap_axes": bool(aligned_first), "coord_max": float(max(np.abs(a).max(), np.abs(b).max()))}


# ---- pixel -> mesh frame ----------------------------------------------------------------------------------------------------
def frame(G, pose, size, height_mm, right, invert, exact=False):
    """Arrays (H, W) fp64 for one finger: cs, sn, pa, pb, da, db, x, y.  `pose` = (t1 [m], t2 [m], theta); with `exact` it is
    (a1 [mm], a2 [mm], theta) in fp64 and nothing is rounded to fp32."""
    h, w = size
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if exact:
        a1, a2, th = (float(p) for p in pose)
        cs, sn, mpp = math.cos(th), math.sin(th), height_mm / h
        u, v = mpp * (r - 0.5 * h), mpp * (c - 0.5 * w)
        t1, t2 = a1, a2
    else:
        t1m, t2m, th = (F(p) for p in pose)
        cs, sn, mpp = F(np.cos(np.float64(th))), F(np.sin(np.float64(th))), F(height_mm / h)
        u = mpp * (r.astype(F) - F(0.5) * F(h))
        v = mpp * (c.astype(F) - F(0.5) * F(w))
        t1, t2 = F(1000) * t1m, F(1000) * t2m
    uu = u if right else -u
    pa, pb = (v, uu) if G["swap_axes"] else (uu, v)
    da, db = pa - t1, pb - t2                                                  # fp32 unless exact
    d = np.float64
    cs, sn, t1, t2, pa, pb, da, db = d(cs), d(sn), d(t1), d(t2), pa.astype(d), pb.astype(d), da.astype(d), db.astype(d)
    if invert:
        x, y = cs * pa - sn * pb + (t1 - d(G["cx"])), sn * pa + cs * pb + (t2 - d(G["cy"]))
    else:
        x, y = cs * da + sn * db - d(G["cx"]), cs * db - sn * da - d(G["cy"])
    return {"cs": cs, "sn": sn, "pa": pa, "pb": pb, "da": da, "db": db, "x": x, "y": y}


def default_delta(G, pose, size, height_mm, exact=False):
    h, w = size
    mpp = height_mm / h
    t = (abs(float(pose[0])), abs(float(pose[1]))) if exact else (abs(1000 * float(pose[0])), abs(1000 * float(pose[1])))
    return 16 * 2.0 ** -23 * max(mpp * h / 2, mpp * w / 2, t[0], t[1], G["coord_max"])


# ---- winner, R, J, uncertain ------------------------------------------------------------------------------------------------
def finger_terms(G, pose, g, size, height_mm, right, invert, exact=False, delta=None):
    rec = G["rec"].astype(np.float64)
    x0, y0, x1, y1, x2, y2, q0, q1, q2, inv = (rec[:, k][:, None, None] for k in range(10))
    fr = frame(G, pose, size, height_mm, right, invert, exact)
    x, y = fr["x"][None], fr["y"][None]
    delta = default_delta(G, pose, size, height_mm, exact) if delta is None else delta
    sg = 1.0 if right else -1.0
    hg = float(g) / 2 if exact else float(F(0.5) * F(g))
    f01 = (x1 - x0) * (y - y0) - (y1 - y0) * (x - x0)
    f02 = (x2 - x0) * (y - y0) - (y2 - y0) * (x - x0)
    f12 = (x2 - x1) * (y - y1) - (y2 - y1) * (x - x1)
    l2, l1, l0 = f01 * inv, -(f02 * inv), f12 * inv
    live = inv != 0
    cover = live & (l0 >= 0) & (l1 >= 0) & (l2 >= 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = 1.0 / np.abs(inv)                                              # |doubled area|
        d2 = l2 * scale / np.hypot(x1 - x0, y1 - y0)                           # inward distances to the three edges
        d1 = l1 * scale / np.hypot(x2 - x0, y2 - y0)
        d0 = l0 * scale / np.hypot(x2 - x1, y2 - y1)
    dmin = np.where(live, np.minimum(d0, np.minimum(d1, d2)), -np.inf)
    near, inside = dmin >= -delta, dmin >= delta
    a, b = q1 - q0, q2 - q0
    qx = (a * (y2 - y0) - b * (y1 - y0)) * inv                                 # (T, 1, 1)
    qy = (b * (x1 - x0) - a * (x2 - x0)) * inv
    q = q0 + l1 * a + l2 * b
    q = np.clip(q, np.minimum(q0, np.minimum(q1, q2)), np.maximum(q0, np.maximum(q1, q2)))
    val = sg * q
    slack = np.hypot(qx, qy) * delta * math.sqrt(2) + 4 * 2.0 ** -23 * np.maximum(np.abs(q0), np.maximum(np.abs(q1), np.abs(q2)))
    cval = np.where(cover, val, -np.inf)
    win = np.argmax(cval, axis=0)                                              # the first maximum: the lowest id among equal values
    m = np.take_along_axis(cval, win[None], axis=0)[0]
    has = m > -np.inf
    win = np.where(has, win, -1)
    pick = lambda arr: np.take_along_axis(np.broadcast_to(arr, cval.shape), np.maximum(win, 0)[None], axis=0)[0]
    wslack, wqx, wqy, winside = pick(slack), pick(qx), pick(qy), pick(inside)
    ids = np.arange(rec.shape[0])[:, None, None]
    rival = near & (ids != win[None]) & (val + slack >= (m - wslack)[None])
    uncertain = np.where(has, rival.any(axis=0) | ~winside | (np.abs(m - hg) <= wslack), near.any(axis=0))
    with np.errstate(invalid="ignore"):
        Rv = np.where(has, -np.maximum(0.0, m - hg), 0.0) + 0.0
    active = Rv < 0
    cs, sn = fr["cs"], fr["sn"]
    if invert:
        xk = (np.ones_like(x[0]), np.zeros_like(x[0]), -sn * fr["pa"] - cs * fr["pb"])
        yk = (np.zeros_like(x[0]), np.ones_like(x[0]), cs * fr["pa"] - sn * fr["pb"])
    else:
        xk = (np.full_like(x[0], -cs), np.full_like(x[0], -sn), -sn * fr["da"] + cs * fr["db"])
        yk = (np.full_like(x[0], sn), np.full_like(x[0], -cs), -sn * fr["db"] - cs * fr["da"])
    J = np.stack([np.where(active, -sg * (wqx * xk[k] + wqy * yk[k]), 0.0) for k in range(3)])
    mag = np.stack([np.where(active, np.abs(wqx) * np.abs(xk[k]) + np.abs(wqy) * np.abs(yk[k]), 0.0) for k in range(3)])
    # the scale of R's own fp64 rounding: q = q0 + l1 a + l2 b with l = (products of coordinate differences) * inv
    ext = np.maximum(np.abs(x[0]), np.abs(y[0])) + pick(np.maximum.reduce([np.abs(v) for v in (x0, y0, x1, y1, x2, y2)]))
    rscale = pick(np.abs(q0)) + pick((np.abs(a) + np.abs(b)) * np.abs(inv)) * ext * ext + abs(hg)
    return {"R": Rv, "J": J + 0.0, "mag": mag, "win": win, "active": active, "uncertain": uncertain, "rscale": rscale}


def point_terms(G, pose, g, size, height_mm=12.0, LR_flip=False, invert=False, exact=False, delta=None):
    """dict of per-point arrays, channels as render_depth's: R (2, H, W), J and mag (2, 3, H, W) -- mag = |qx| |x_k| + |qy| |y_k|,
    the scale of J's rounding --, win, active, uncertain (2, H, W)."""
    per = {}
    for finger in (0, 1):                                                      # 0 left (mirrored), 1 right
        per[finger if not LR_flip else 1 - finger] = finger_terms(G, pose, g, size, height_mm, finger == 1, invert, exact, delta)
    return {k: np.stack((per[0][k], per[1][k])) for k in per[0]}


def normal_terms(Rv, J, observed, stride=1):
    """(16, points) fp64: what every lattice point of both channels adds to the 16 entries, from a candidate's R (2, H, W) and J
    (2, 3, H, W) and the observed images; J_g = 0.5 at active points."""
    Rv, J = np.asarray(Rv, np.float64), np.asarray(J, np.float64)
    rows, cols = P.lattice(Rv.shape[1], Rv.shape[2], stride)
    Rl, Dl = Rv[:, rows][:, :, cols], np.asarray(observed, np.float64)[:, rows][:, :, cols]
    Jl = J[:, :, rows][:, :, :, cols]
    active = Rl < 0
    J4 = [Jl[:, 0], Jl[:, 1], Jl[:, 2], np.where(active, 0.5, 0.0)]
    with np.errstate(invalid="ignore", over="ignore"):
        e = Rl - Dl
        out = [e * e, active.astype(np.float64)] + [J4[k] * e for k in range(4)] + [J4[j] * J4[k] for j, k in PAIRS]
    return np.stack([t.reshape(-1) for t in out])


def normal_row(Rv, J, observed, stride=1):
    """The 16 doubles of one candidate."""
    with np.errstate(invalid="ignore", over="ignore"):
        return normal_terms(Rv, J, observed, stride).sum(axis=1)


# ---- the damped step --------------------------------------------------------------------------------------------------------
def lm_solve(row, lam, mask, max_step):
    """delta (4,) of (A + lam diag(A)) delta = -b on the parameters of `mask`, Cholesky in the order a1, a2, theta, g; a parameter
    that is not free has the identity's row and column and the right-hand side 0.  A pivot <= 0 or not finite, or a solution
    that is not finite, gives 0; the step is clipped per component."""
    A = np.zeros((4, 4))
    for n, (j, k) in enumerate(PAIRS):
        A[j, k] = A[k, j] = row[6 + n]
    rhs = -np.asarray(row[2:6], np.float64)
    free = [(mask >> k) & 1 == 1 for k in range(4)]
    M = np.zeros((4, 4))
    for j in range(4):
        for k in range(4):
            if free[j] and free[k]:
                M[j, k] = A[j, k] + lam * A[j, j] if j == k else A[j, k]
            else:
                M[j, k] = 1.0 if j == k else 0.0
        if not free[j]:
            rhs[j] = 0.0
    L = np.zeros((4, 4))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(4):
            d = M[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            if not (d > 0 and np.isfinite(d)):
                return np.zeros(4), M
            L[j, j] = math.sqrt(d)
            for i in range(j + 1, 4):
                s = M[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        z = np.zeros(4)
        for i in range(4):
            s = rhs[i]
            for k in range(i):
                s = s - L[i, k] * z[k]
            z[i] = s / L[i, i]
        dl = np.zeros(4)
        for i in range(3, -1, -1):
            s = z[i]
            for k in range(i + 1, 4):
                s = s - L[k, i] * dl[k]
            dl[i] = s / L[i, i]
    if not np.isfinite(dl).all():
        return np.zeros(4), M
    ms = np.asarray(max_step, np.float64)
    return np.minimum(np.maximum(dl, -ms), ms), M


def lm_update_ref(state, trial_pose, trial_width, trial_row, mask=7, down=0.1, up=10.0, lam_min=1e-12, lam_max=1e12,
                  max_step=(0.5, 0.5, 0.1, 0.5), first=False):
    """gsd_mesh_pose_lm_update for one problem.  `state`: dict pose (3,) fp32, width fp32, lam, row (16,), accepted; updated in
    place.  Returns (next trial pose (3,) fp32, next trial width fp32, delta (4,), accepted this call)."""
    took = False
    if first:
        state.update(pose=np.asarray(trial_pose, F).copy(), width=F(trial_width), row=np.asarray(trial_row, np.float64).copy(), accepted=0)
    elif trial_row[0] < state["row"][0]:                                        # strict; a NaN never wins
        state.update(pose=np.asarray(trial_pose, F).copy(), width=F(trial_width), row=np.asarray(trial_row, np.float64).copy())
        state["accepted"] += 1
        state["lam"] = max(state["lam"] * down, lam_min)
        took = True
    else:
        state["lam"] = min(state["lam"] * up, lam_max)
    dl, _ = lm_solve(state["row"], state["lam"], mask, max_step)
    p = state["pose"]
    nxt = np.asarray([F(np.float64(p[0]) + dl[0] / 1000.0), F(np.float64(p[1]) + dl[1] / 1000.0), F(np.float64(p[2]) + dl[2])], F)
    return nxt, F(np.float64(state["width"]) + dl[3]), dl, took


def refine_twin(tri, plane, observed, g, init, iterations=10, fit_width=False, stride=1, damping=1e-3, damping_up=10.0,
                damping_down=0.1, max_step=(0.5, 0.5, 0.1, 0.5), image_height_mm=12.0, LR_flip=False, invert_affine=False):
    """refine_pose for one observation (2, H, W) and one start."""
    G = records(tri, plane)
    size = observed.shape[1:]
    state = {"pose": None, "width": None, "lam": float(damping), "row": None, "accepted": 0}
    pose, width, trace = np.asarray(init, F), F(g), []
    for it in range(iterations + 1):
        if float(width) >= 0:
            t = point_terms(G, pose, width, size, image_height_mm, LR_flip, invert_affine)
            row = normal_row(t["R"], t["J"], observed, stride)
        else:
            row = np.full(NROW, np.nan)
        pose, width, dl, _ = lm_update_ref(state, pose, width, row, 15 if fit_width else 7, damping_down, damping_up,
                                           max_step=max_step, first=it == 0)
        trace.append(state["row"][0])
    n = P.n_points(size[0], size[1], stride)
    return {"pose": state["pose"], "width": state["width"], "cost": state["row"][0] / n, "row": state["row"], "trace": np.asarray(trace) / n,
            "accepted": state["accepted"], "last_step": dl}


# ---- the cases of tests/test_mesh_pose_refine_cpu.py and tests/test_gpu_mesh_pose_refine.py -----------------------------------
# name -> (mesh, size, pose, LR_flip, invert_affine): the images the Jacobian is compared on
IMAGES = {"lprism": ("lprism", (24, 31), (0.4e-3, -0.3e-3, 0.35), False, False),
          "sphere4": ("sphere4", (40, 53), (-0.6e-3, 0.5e-3, -1.2), True, False),
          "ellipsoid": ("ellipsoid", (40, 53), (0.3e-3, -0.4e-3, -0.25), False, True)}
UNCERTAIN_CAP = 0.02          # of the active points of an image

# the lattice twin's end pose on the ellipsoid case (tests/mesh_pose_ref.py: truth + its error) and what refine_twin makes of it
ELLIPSOID_LATTICE_ERROR = (0.0333333, 0.0444444, -0.0343750)          # mm, mm, rad


def lattice_end(case):
    """The fp32 pose the three-level lattice twin ends on: the truth plus its recorded error."""
    t = P.case_truth(case)
    e = ELLIPSOID_LATTICE_ERROR
    return tuple(float(F(v)) for v in (t[0] + e[0] * 1e-3, t[1] + e[1] * 1e-3, t[2] + e[2]))


def image_terms(name):
    mesh, size, pose, flip, invert = IMAGES[name]
    tri = P.MESHES[mesh]()
    G = records(tri)
    return G, point_terms(G, pose, F(P.contact_width(tri)), size, 12.0, flip, invert)


def run_ellipsoid(start=None, fit_width=False, width_error=0.0, iterations=10):
    case = P.CASES["ellipsoid"]
    tri = P.MESHES[case["mesh"]]()
    truth, g = P.case_truth(case), PW.true_width(case)
    observed, _ = R.raster_ref(tri, 1.0, P.PLANE, truth, g, case["size"], case["height_mm"], delta=0.0)
    res = refine_twin(tri, P.PLANE, observed, F(F(g) + F(width_error)), lattice_end(case) if start is None else start, iterations, fit_width)
    res["error"] = P.pose_error_ref(res["pose"], truth)
    res["width_error"] = float(res["width"]) - g
    return res


if __name__ == "__main__":
    for image in IMAGES:
        _, t = image_terms(image)
        n_act = int(t["active"].sum())
        print(f"{image}: {n_act} active points, {int((t['uncertain'] & t['active']).sum())} of them uncertain "
              f"({100.0 * (t['uncertain'] & t['active']).sum() / max(n_act, 1):.3f} %), {int(t['uncertain'].sum())} uncertain in all")
    for label, kw in (("from the lattice end", {}), ("width 0.35 mm off, fit_width", {"fit_width": True, "width_error": PW.START_WIDTH_ERROR})):
        res = run_ellipsoid(**kw)
        print(f"ellipsoid {label}: error (mm, mm, rad) {res['error'].tolist()}, width error {res['width_error']!r} mm, cost {res['cost']!r}, "
              f"accepted {res['accepted']}, trace {res['trace'].tolist()}")
