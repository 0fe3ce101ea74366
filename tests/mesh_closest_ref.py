"""fp64 numpy twins of gsd_mesh_closest_points, gsd_mesh_icp_rows and gsd_mesh_icp_lm_update; not a test.

The closest point of p on a triangle is computed in the kernel's order of operations (include/gsd.h), elementwise: numpy's fp64
`+ - * /` round as the device's do, so `closest_brute` is meant to agree with the kernel BIT FOR BIT, ties included.  The twin
evaluates every triangle of the mesh for every point (`prune=False`), or -- the default, because the registration twins run it some
10^5 times -- only the triangles that an exact bounding-sphere test cannot rule out; `test_mesh_closest_cpu` holds the two equal."""
import math

import numpy as np

ROW = 30
PAIRS = [(j, k) for j in range(6) for k in range(j, 6)]


def vertices(tri32, pc_scale=1.0):
    """(T, 3, 3) fp64 of the fp32 vertices fp32(v * pc_scale), the floats MeshVolume uploads."""
    return (np.asarray(tri32, np.float64) * float(pc_scale)).astype(np.float32).astype(np.float64)


def cross(v):
    """(b - a) x (c - a), each component two rounded products and one subtraction."""
    u, w = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    return np.stack((u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]),
                    axis=1)


def skipped(v):
    return (cross(v) == 0.0).all(axis=1)


def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def on_triangles(a, b, c, p):
    """Closest points x and d^2 of the points p (..., 3) on the triangles (a, b, c) (..., 3), broadcast: the region method."""
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e1, e2 = d4 - d3, d5 - d6
    with np.errstate(divide="ignore", invalid="ignore"):
        tab, tac, tbc = (d1 / (d1 - d3))[..., None], (d2 / (d2 - d6))[..., None], (e1 / (e1 + e2))[..., None]
        s = (va + vb) + vc
        fv, fw = (vb / s)[..., None], (vc / s)[..., None]
        shape = np.broadcast(a, p).shape
        full = lambda t: np.broadcast_to(t, shape)
        regions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                   (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e1 >= 0) & (e2 >= 0)]
        values = [full(a), full(b), a + tab * ab, full(c), a + tac * ac, b + tbc * (c - b)]
        x = np.select([r[..., None] for r in regions], values, default=(a + fv * ab) + fw * ac)
    r = p - x
    return x, (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]


def closest_brute(tri32, points, D=None, pc_scale=1.0, prune=True, chunk=256):
    """The winner of every point: (triangle (N,) int64, x (N, 3) fp64, d2 (N,) fp64, second (N,) fp64).  The smallest d^2, the
    lowest id among bit-equal ones; skipped triangles never win; with D a winner needs d^2 <= D * D; no winner or a non-finite
    point: -1, NaN, +inf.  `second` is the next smallest d^2 among the other triangles (+inf where the pruning dropped them all:
    they are far off then), for counting near-ties.  `points` may be fp32 or fp64; they are used as fp64."""
    v = vertices(tri32, pc_scale)
    keep = np.nonzero(~skipped(v))[0]
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = p.shape[0]
    tid, x, d2, second = np.full(n, -1, np.int64), np.full((n, 3), np.nan), np.full(n, np.inf), np.full(n, np.inf)
    finite = np.isfinite(p).all(axis=1)
    if keep.size:
        a, b, c = v[keep, 0], v[keep, 1], v[keep, 2]
        ctr = (a + b + c) / 3.0
        rad = np.sqrt(np.maximum(np.maximum(((a - ctr) ** 2).sum(1), ((b - ctr) ** 2).sum(1)), ((c - ctr) ** 2).sum(1))) * (1 + 1e-9)
        for lo in range(0, n, chunk):
            idx = np.nonzero(finite[lo:lo + chunk])[0] + lo
            if not idx.size:
                continue
            q = p[idx]
            if prune:      # a triangle lies within [dc - rad, dc + rad] of the point, dc the distance to its bounding sphere's centre
                dc = np.sqrt(((q[:, None, :] - ctr[None]) ** 2).sum(2))
                upper = (dc + rad).min(axis=1) * (1 + 1e-9) + 1e-300
                pi, ti = np.nonzero((dc - rad) * (1 - 1e-9) <= upper[:, None])
            else:
                pi, ti = np.divmod(np.arange(q.shape[0] * keep.size), keep.size)
            xs, ds = on_triangles(a[ti], b[ti], c[ti], q[pi])
            first = np.concatenate(([0], np.nonzero(np.diff(pi))[0] + 1))      # pairs are sorted by point, then by triangle id
            best = np.minimum.reduceat(ds, first)
            hit = np.nonzero(ds == best[pi])[0]
            _, where = np.unique(pi[hit], return_index=True)
            win = hit[where]
            tid[idx], x[idx], d2[idx] = keep[ti[win]], xs[win], ds[win]
            rest = ds.copy()
            rest[win] = np.inf
            second[idx] = np.minimum.reduceat(rest, first)
    if D is not None:
        far = ~(d2 <= float(D) * float(D))
        tid[far], x[far], d2[far] = -1, np.nan, np.inf
    return tid, x, d2, second


def ulp_gap(a, b):
    """|a - b| in units of the last place of the larger (fp64 arrays); inf where either is not finite."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(a) & np.isfinite(b), np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))), np.inf)


# ---- normal-equation rows ---------------------------------------------------------------------------------------------------
def transform_points(points32, T):
    """p' = R p + t in fp64, x' = ((R00 px + R01 py) + R02 pz) + t0; T: 12 doubles, row-major [R | t]."""
    p, m = np.asarray(points32, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(T, np.float64).reshape(3, 4)
    return np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], axis=1)


def icp_terms(tri32, points32, T, D=None, kind="plane", weights=None, pc_scale=1.0, found=None):
    """(terms (N, 30), active (N,) bool): what each point adds to the row, in the kernel's order of operations.  `found` may pass
    closest_brute(tri32, transform_points(points32, T)) of an earlier call (it does not depend on D, kind or weights)."""
    v = vertices(tri32, pc_scale)
    pp = transform_points(points32, T)
    n = pp.shape[0]
    w = np.ones(n) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    tid, x, d2, _ = found if found is not None else closest_brute(tri32, pp, None, pc_scale)
    finite = np.isfinite(pp).all(axis=1)
    D2 = np.inf if D is None else float(D) * float(D)
    active = finite & (tid >= 0) & (d2 <= D2)
    t = np.zeros((n, ROW))
    if math.isfinite(D2):
        t[finite & ~active, 0] = (w * D2)[finite & ~active]
    i = np.nonzero(active)[0]
    if i.size:
        p, r3, wi = pp[i], pp[i] - x[i], w[i]
        t[i, 0], t[i, 1] = wi * d2[i], 1.0
        if kind == "plane":
            nrm = cross(v[tid[i]])
            length = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
            nrm = nrm / length[:, None]
            r = _dot(nrm, r3)
            J = np.stack((nrm[:, 0], nrm[:, 1], nrm[:, 2], p[:, 1] * nrm[:, 2] - p[:, 2] * nrm[:, 1],
                          p[:, 2] * nrm[:, 0] - p[:, 0] * nrm[:, 2], p[:, 0] * nrm[:, 1] - p[:, 1] * nrm[:, 0]), axis=1)
            t[i, 2] = wi * (r * r)
            for j in range(6):
                t[i, 3 + j] = wi * (J[:, j] * r)
            for q, (j, k) in enumerate(PAIRS):
                t[i, 9 + q] = wi * (J[:, j] * J[:, k])
        elif kind == "point":
            z, o = np.zeros(i.size), np.ones(i.size)
            J = np.stack((np.stack((o, z, z, z, p[:, 2], -p[:, 1]), 1), np.stack((z, o, z, -p[:, 2], z, p[:, 0]), 1),
                          np.stack((z, z, o, p[:, 1], -p[:, 0], z), 1)), axis=1)          # (n, 3, 6): rows of [I, -[p']x]
            t[i, 2] = wi * d2[i]
            for j in range(6):
                t[i, 3 + j] = wi * ((J[:, 0, j] * r3[:, 0] + J[:, 1, j] * r3[:, 1]) + J[:, 2, j] * r3[:, 2])
            for q, (j, k) in enumerate(PAIRS):
                t[i, 9 + q] = wi * ((J[:, 0, j] * J[:, 0, k] + J[:, 1, j] * J[:, 1, k]) + J[:, 2, j] * J[:, 2, k])
        else:
            raise ValueError(kind)
    return t, active


def icp_row(tri32, points32, T, D=None, kind="plane", weights=None, pc_scale=1.0, found=None):
    """(row (30,), abs_sums (30,)): every entry summed with math.fsum, and the sums of the terms' magnitudes (the error bound of any
    other summation order is n * 2^-52 * abs_sums)."""
    t, _ = icp_terms(tri32, points32, T, D, kind, weights, pc_scale, found)
    return (np.array([math.fsum(t[:, q]) for q in range(ROW)]), np.array([math.fsum(np.abs(t[:, q])) for q in range(ROW)]))


# ---- the cells of MeshVolume ------------------------------------------------------------------------------------------------
CELL_EPS = 1e-6      # of a cell: how far a triangle's index range is widened on either side


def volume_cell_ranges(tri32, origin, inv_cell, dims, pc_scale=1.0):
    """mc_cell_range in numpy, fp64: (T, 3) lowest and highest (ix, iy, iz) of every triangle's widened box."""
    v = vertices(tri32, pc_scale)

    def cell(x, eps):
        f = np.floor((x - np.asarray(origin, float)) * float(inv_cell) + eps)
        return np.clip(f, 0, np.asarray(dims) - 1).astype(np.int64)
    return cell(v.min(axis=1), -CELL_EPS), cell(v.max(axis=1), CELL_EPS)


# ---- the damped step --------------------------------------------------------------------------------------------------------
def lm_solve(row, lam, max_step):
    """(A + lam diag A) xi = -b by Cholesky in the order v1 v2 v3 w1 w2 w3; a bad pivot or a non-finite solution gives 0."""
    M = np.zeros((6, 6))
    for q, (j, k) in enumerate(PAIRS):
        M[j, k] = M[k, j] = row[9 + q] + lam * row[9 + q] if j == k else row[9 + q]
    Lc, ok = np.zeros((6, 6)), True
    with np.errstate(all="ignore"):
        for j in range(6):
            piv = M[j, j]
            for k in range(j):
                piv = piv - Lc[j, k] * Lc[j, k]
            ok = ok and bool(piv > 0.0) and math.isfinite(piv)
            Lc[j, j] = np.sqrt(piv)
            for r in range(j + 1, 6):
                s = M[r, j]
                for k in range(j):
                    s = s - Lc[r, k] * Lc[j, k]
                Lc[r, j] = s / Lc[j, j]
        z, d = np.zeros(6), np.zeros(6)
        for r in range(6):
            s = -row[3 + r]
            for k in range(r):
                s = s - Lc[r, k] * z[k]
            z[r] = s / Lc[r, r]
        for r in range(5, -1, -1):
            s = z[r]
            for k in range(r + 1, 6):
                s = s - Lc[k, r] * d[k]
            d[r] = s / Lc[r, r]
    ok = ok and bool(np.isfinite(d).all())
    return np.clip(d, -np.asarray(max_step, float), np.asarray(max_step, float)) if ok else np.zeros(6)


def twist_exp(xi):
    """(E (3, 3), u (3,)) of the left twist xi = (v, omega): Rodrigues' formula, the series below |omega| = 1e-8."""
    v, w = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = math.sqrt(th2)
    if th < 1e-8:
        A, B, Cc = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        A, B, Cc = math.sin(th) / th, (1.0 - math.cos(th)) / th2, (th - math.sin(th)) / (th2 * th)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    K2 = np.outer(w, w) - th2 * np.eye(3)
    E, V = (np.eye(3) + A * K) + B * K2, (np.eye(3) + B * K) + Cc * K2
    return E, np.array([(V[r, 0] * v[0] + V[r, 1] * v[1]) + V[r, 2] * v[2] for r in range(3)])


def compose(xi, T):
    """exp(xi) T as 12 doubles: R' = E R, t' = E t + u."""
    E, u = twist_exp(xi)
    m, out = np.asarray(T, float).reshape(3, 4), np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            out[r, c] = (E[r, 0] * m[0, c] + E[r, 1] * m[1, c]) + E[r, 2] * m[2, c]
        out[r, 3] = out[r, 3] + u[r]
    return out.reshape(12)


def lm_update(state, trial_T, trial_row, first=False, down=0.1, up=10.0, lam_min=1e-12, lam_max=1e12,
              max_step=(1.0, 1.0, 1.0, 0.1, 0.1, 0.1)):
    """One gsd_mesh_icp_lm_update for one start.  state: dict(T, lam, row, accepted) (row may be None before the first);
    returns (state, next trial T, |step|)."""
    take = bool(first) or bool(trial_row[0] < state["row"][0])
    s = dict(state)
    if first:
        s["accepted"] = 0
    if take:
        s["T"], s["row"] = np.array(trial_T, float), np.array(trial_row, float)
    if not first:
        s["lam"] = max(s["lam"] * down, lam_min) if take else min(s["lam"] * up, lam_max)
        s["accepted"] += int(take)
    d = lm_solve(s["row"], s["lam"], max_step)
    return s, compose(d, s["T"]), np.abs(d)


def as12(m):
    m = np.asarray(m, float)
    return m[:3, :].reshape(12) if m.shape == (4, 4) else m.reshape(12)


def as44(T):
    out = np.eye(4)
    out[:3, :] = np.asarray(T, float).reshape(3, 4)
    return out


def register(tri32, points32, init=None, iterations=20, D=None, kind="plane", weights=None, damping=1e-3, damping_up=10.0,
             damping_down=0.1, max_step=(1.0, 1.0, 1.0, 0.1, 0.1, 0.1), pc_scale=1.0):
    """register_cloud for one start: dict(matrix (4, 4), cost, rms, active, trace (iterations + 1,), accepted, last_step)."""
    trial = as12(np.eye(4) if init is None else init)
    state = {"T": trial.copy(), "lam": float(damping), "row": None, "accepted": 0}
    trace, step = [], np.zeros(6)
    for it in range(int(iterations) + 1):
        row, _ = icp_row(tri32, points32, trial, D, kind, weights, pc_scale)
        state, trial, step = lm_update(state, trial, row, it == 0, damping_down, damping_up, max_step=max_step)
        trace.append(state["row"][0])
    t, active = icp_terms(tri32, points32, state["T"], D, "point", weights, pc_scale)
    sq = math.fsum(t[active, 2])
    return {"matrix": as44(state["T"]), "cost": state["row"][0], "rms": math.sqrt(sq / max(int(active.sum()), 1)), "active": int(active.sum()),
            "trace": np.array(trace), "accepted": state["accepted"], "last_step": step, "row": state["row"]}


# ---- the query cases of tests/test_gpu_mesh_closest.py ------------------------------------------------------------------------
QUERY_MESHES = ("box", "sphere", "torus", "l_prism", "peg1", "pattern_32")


def query_mesh(name):
    """(tri32 in the file's units, pc_scale)."""
    import mesh_depth_ref as R
    if name in ("peg1", "pattern_32"):
        import real_mesh_cases as P
        return P.mesh(name), P.pc_scale(name)
    return {"box": R.box, "sphere": lambda: R.sphere(2), "torus": R.torus, "l_prism": R.l_prism}[name](), 1.0


def query_points(name):
    """dict label -> fp32 (N, 3) in mm: 700 random points in 1.5 x the bounding box, 500 surface samples, every vertex, every edge
    midpoint (exact ties between the triangles that share them) and 14 points 10 x the extent away."""
    import mesh_depth_ref as R
    tri, scale = query_mesh(name)
    v = vertices(tri, scale)
    seed = QUERY_MESHES.index(name)
    rng = np.random.Generator(np.random.PCG64(1002 + seed))
    lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
    mid, ext = 0.5 * (lo + hi), hi - lo
    dirs = np.array([d for d in np.ndindex(3, 3, 3) if sum(abs(c - 1) for c in d) in (1, 3)], float) - 1.0
    mids = np.concatenate([0.5 * (v[:, i] + v[:, (i + 1) % 3]) for i in range(3)])
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    return {"random": f32(mid + (rng.random((700, 3)) - 0.5) * 1.5 * ext), "surface": f32(R.sample_surface(v, 500, seed=200 + seed)),
            "vertices": np.unique(f32(v.reshape(-1, 3)), axis=0), "midpoints": np.unique(f32(mids), axis=0),
            "far": f32(mid + 10.0 * ext.max() * dirs)}


def near_ties(d2, second, ulps=4.0):
    """Points whose two best d^2 differ, but by at most `ulps` units of the last place: where a division that rounds differently
    could change the winner.  Exact ties are not counted: the lowest id resolves them on either side."""
    d2, second = np.asarray(d2), np.asarray(second)
    return np.isfinite(d2) & (second != d2) & (ulp_gap(d2, second) <= ulps)


# ---- the registration cases of tests/test_gpu_mesh_register.py ---------------------------------------------------------------
def rigid(translation, axis, angle):
    """(4, 4) fp64: rotation by `angle` about `axis` (normalised here), then `translation`."""
    k = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)
    m[:3, 3] = translation
    return m


T0 = rigid((0.4, -0.4, 0.2), (1.0, 2.0, -2.0), 0.08)      # |t| = 0.6 mm, 0.08 rad about a skew axis
CLOUD_POINTS = 4000


def case_mesh(name):
    import mesh_depth_ref as R
    return {"ellipsoid": lambda: R.ellipsoid(3), "l_prism": lambda: R.l_prism()}[name]()


def case_cloud(name, outliers=0.0):
    """(tri32, cloud fp32 (N, 3)): CLOUD_POINTS surface samples moved by T0 -- register_cloud should return T0^-1 --, with a share
    `outliers` of them thrown 3 to 6 mm off along a fixed direction pattern."""
    import mesh_depth_ref as R
    tri = case_mesh(name)
    p = R.sample_surface(tri, CLOUD_POINTS, seed=7)
    if outliers:
        rng = np.random.Generator(np.random.PCG64(11))
        bad = rng.choice(p.shape[0], size=int(outliers * p.shape[0]), replace=False)
        d = rng.normal(size=(bad.size, 3))
        p[bad] += d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(3.0, 6.0, size=(bad.size, 1))
    return tri, (p @ T0[:3, :3].T + T0[:3, 3]).astype(np.float32)


def corners(tri32):
    v = np.asarray(tri32, np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    return np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])


def corner_gap(m1, m2, tri32):
    """The largest distance [mm] between the images of the bounding box's corners under two (4, 4) motions."""
    c = corners(tri32)
    a, b = c @ m1[:3, :3].T + m1[:3, 3], c @ m2[:3, :3].T + m2[:3, 3]
    return float(np.sqrt(((a - b) ** 2).sum(axis=1)).max())


# What the twin's own registration reaches on those cases (test_mesh_closest_cpu measures them again and holds them to these
# figures within a factor of two; the GPU test takes its bounds from here).  ERROR is corner_gap(matrix @ T0, identity) in mm.
TWIN = {
    # (case, kind, D, outliers): (ERROR mm, final rms mm), 20 iterations from the identity
    ("ellipsoid", "plane", None, 0.0): (5.907e-08, 1.234e-07),
    ("l_prism", "plane", None, 0.0): (1.142e-08, 5.084e-08),
    # point to point creeps along the tangents: after 20 iterations it is still this far off
    ("ellipsoid", "point", None, 0.0): (5.916e-01, 3.287e-02),
    ("l_prism", "point", None, 0.0): (1.071e-02, 1.455e-03),
    # 10 % of the points thrown 3 to 6 mm off, D = 1.5 mm: the outliers that stay within D of some facet bias the fit this much
    ("ellipsoid", "plane", 1.5, 0.1): (4.185e-02, 1.662e-01),
    ("l_prism", "plane", 1.5, 0.1): (1.463e-02, 1.543e-01),
}
OUTLIER_D = 1.5
