"""Test helper for gelslim_depth_amd.touch_fusion (numpy, fp64, vectorised over voxels and cells; nothing here is product code): the
twin of DESIGN.md section 24.

  * `project` / `integrate`: one sample per (voxel, touch, channel) in the order of operations the kernel uses, the update in fp32
    with products and sums rounded separately, touches in order and channel 0 before channel 1,
  * `tet_table`: the marching-tetrahedra table generated from the rule (six Kuhn tetrahedra, triangles by edges, winding from the
    undeformed lattice), which the kernel has written out,
  * `extract`: the triangles in contract order (cell, tetrahedron, table order), vertices on edges from the lower to the higher
    linear index, rounded to fp32 once,
  * `topology`, `signed_volume`: what the tests ask of a closed surface,
  * `python tests/touch_fusion_ref.py` prints the table as the kernel holds it."""
import itertools
import math

import numpy as np

CORNER = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]      # cube corner c = dx + 2 dy + 4 dz


def voxel_axes(origin, h, shape):
    """The voxel coordinates per axis, origin + h * i: one product and one sum per component.  shape = (nx, ny, nz)."""
    return [float(origin[a]) + float(h) * np.arange(shape[a], dtype=np.float64) for a in range(3)]


def voxel_points(origin, h, shape):
    """(px, py, pz), each broadcastable to (nz, ny, nx)."""
    x, y, z = voxel_axes(origin, h, shape)
    return x[None, None, :], y[None, :, None], z[:, None, None]


def project(p, row, s, g, image_size, image_height_mm):
    """(rf, kf, s q - g/2) of the object-frame points p = (px, py, pz) under the touch `row` (12 doubles) for the finger s."""
    px, py, pz = p
    h, w = image_size
    t = [float(v) for v in row]
    u = ((t[0] * px + t[1] * py) + t[2] * pz) + t[3]
    v = ((t[4] * px + t[5] * py) + t[6] * pz) + t[7]
    q = ((t[8] * px + t[9] * py) + t[10] * pz) + t[11]
    mpp = float(image_height_mm) / h
    inv_mpp = 1.0 / mpp
    rf = (s * u) * inv_mpp + 0.5 * h
    kf = v * inv_mpp + 0.5 * w
    return rf, kf, s * q - 0.5 * g


def integrate(acc, weight, origin, h, tau, depth, widths, transforms, image_height_mm=12.0, grasp_width_offset=0.0, LR_flip=False,
              contact_depth=0.0, carve_weight=1.0, weights=None):
    """(acc, weight) float32 (nz, ny, nx) after the K touches `depth` (K, 2, H, W) float32; the inputs are not changed."""
    acc, weight = np.array(acc, np.float32), np.array(weight, np.float32)
    depth = np.asarray(depth)
    assert depth.dtype == np.float32 and depth.ndim == 4 and depth.shape[1] == 2 and acc.shape == weight.shape
    k_n, _, hh, ww = depth.shape
    nz, ny, nx = acc.shape
    p = voxel_points(origin, h, (nx, ny, nz))
    transforms = np.asarray(transforms, np.float64).reshape(k_n, 12)
    inv_tau = 1.0 / float(tau)
    thr = -np.float32(contact_depth)
    carve = np.float32(carve_weight)
    with np.errstate(all="ignore"):
        for k in range(k_n):
            g = float(np.float32(widths[k])) + float(grasp_width_offset)
            if not (g >= 0.0 and math.isfinite(g)):
                continue
            w = np.float32(1.0 if weights is None else weights[k])
            wc = np.float32(w * carve)
            for ch in (0, 1):
                s = 1.0 if (ch == 1) != bool(LR_flip) else -1.0
                rf, kf, base = project(p, transforms[k], s, g, (hh, ww), image_height_mm)
                rf, kf, base = (np.broadcast_to(a, acc.shape) for a in (rf, kf, base))
                r0, k0 = np.floor(rf), np.floor(kf)
                inside = (r0 >= 0.0) & (r0 <= hh - 2.0) & (k0 >= 0.0) & (k0 <= ww - 2.0)
                ri, ki = np.where(inside, r0, 0.0).astype(np.int64), np.where(inside, k0, 0.0).astype(np.int64)
                img = depth[k, ch]
                d00, d01, d10, d11 = img[ri, ki], img[ri, ki + 1], img[ri + 1, ki], img[ri + 1, ki + 1]
                usable = inside & np.isfinite(d00) & np.isfinite(d01) & np.isfinite(d10) & np.isfinite(d11)
                contact = usable & (d00 < thr) & (d01 < thr) & (d10 < thr) & (d11 < thr)
                a, b = rf - r0, kf - k0
                e00, e01, e10, e11 = (d.astype(np.float64) for d in (d00, d01, d10, d11))
                top = e00 + b * (e01 - e00)
                bot = e10 + b * (e11 - e10)
                dbar = top + a * (bot - top)
                phi = base + dbar
                surf = contact & (phi >= -float(tau))
                free = usable & ~contact & (phi > 0.0)
                val = np.minimum(phi * inv_tau, 1.0).astype(np.float32)
                acc = np.where(surf, acc + w * val, np.where(free, acc + wc, acc)).astype(np.float32)
                weight = np.where(surf, weight + w, np.where(free, weight + wc, weight)).astype(np.float32)
    return acc, weight


# ---- marching tetrahedra --------------------------------------------------------------------------------------------
def tetrahedra():
    """The six Kuhn tetrahedra around the diagonal (0,0,0)-(1,1,1) as cube corner ids (c0, c1, c2, c3), permutations in
    lexicographic order."""
    return [(0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7) for p in itertools.permutations(range(3))]


def _triangles_of_mask(mask):
    """Triangles of a tetrahedron whose corners in `mask` are inside, as edges (i, j) of tetrahedron corner numbers."""
    ins = [i for i in range(4) if mask >> i & 1]
    out = [i for i in range(4) if not mask >> i & 1]
    if len(ins) == 1:
        i, (j, k, l) = ins[0], out
        return [[(i, j), (i, k), (i, l)]]
    if len(ins) == 3:
        (i, j, k), o = ins, out[0]
        return [[(i, o), (j, o), (k, o)]]
    if len(ins) == 2:
        (i, j), (k, l) = ins, out
        return [[(i, k), (i, l), (j, l)], [(i, k), (j, l), (j, k)]]
    return []


def tet_table():
    """table[tet][mask] = list of triangles, each three edges (lo, hi) of CUBE corner ids with lo < hi (ascending linear index:
    the order of corner ids is the order of linear indices for nx, ny >= 2), wound so that the normal leaves the inside."""
    table = []
    for tet in tetrahedra():
        pos = np.array([CORNER[c] for c in tet], np.float64)
        rows = []
        for mask in range(16):
            tris = []
            for tri in _triangles_of_mask(mask):
                mid = [0.5 * (pos[i] + pos[j]) for i, j in tri]
                ins = np.mean([pos[i] for i in range(4) if mask >> i & 1], axis=0)
                out = np.mean([pos[i] for i in range(4) if not mask >> i & 1], axis=0)
                turn = float(np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), out - ins))
                assert turn != 0.0
                if turn < 0.0:
                    tri = [tri[0], tri[2], tri[1]]
                tris.append([(min(tet[i], tet[j]), max(tet[i], tet[j])) for i, j in tri])
            rows.append(tris)
        table.append(rows)
    return table


def field(acc, weight):
    with np.errstate(all="ignore"):
        return np.asarray(acc, np.float32).astype(np.float64) / np.asarray(weight, np.float32).astype(np.float64)


def extract(acc, weight, origin, h, min_weight=0.0):
    """(triangles (T, 3, 3) float32, cell (T,) int64) of the volume in contract order."""
    acc, weight = np.asarray(acc, np.float32), np.asarray(weight, np.float32)
    nz, ny, nx = acc.shape
    f = field(acc, weight)
    observed = weight > np.float32(min_weight)
    with np.errstate(invalid="ignore"):
        inside = f < 0.0
    ax = voxel_axes(origin, h, (nx, ny, nz))
    cz, cy, cx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")

    def at(arr, c):
        dx, dy, dz = CORNER[c]
        return arr[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        valid &= at(observed, c)
    cell_index = (cz * (ny - 1) + cy) * (nx - 1) + cx
    table = tet_table()
    tris, keys = [], []
    for t_no, tet in enumerate(tetrahedra()):
        mask = np.zeros(valid.shape, np.int64)
        for i, c in enumerate(tet):
            mask |= at(inside, c).astype(np.int64) << i
        for m in range(1, 15):
            sel = valid & (mask == m)
            if not sel.any():
                continue
            ix, iy, iz, cells = cx[sel], cy[sel], cz[sel], cell_index[sel]
            for n_no, tri in enumerate(table[t_no][m]):
                verts = np.empty((len(cells), 3, 3), np.float32)
                for v_no, (lo, hi) in enumerate(tri):
                    (lx, ly, lz), (hx, hy, hz) = CORNER[lo], CORNER[hi]
                    f_lo, f_hi = f[iz + lz, iy + ly, ix + lx], f[iz + hz, iy + hy, ix + hx]
                    with np.errstate(all="ignore"):
                        t = f_lo / (f_lo - f_hi)
                        for a, (il, ih) in enumerate(((ix + lx, ix + hx), (iy + ly, iy + hy), (iz + lz, iz + hz))):
                            p_lo, p_hi = ax[a][il], ax[a][ih]
                            verts[:, v_no, a] = (p_lo + (p_hi - p_lo) * t).astype(np.float32)
                tris.append(verts)
                keys.append((cells * 6 + t_no) * 2 + n_no)
    if not tris:
        return np.zeros((0, 3, 3), np.float32), np.zeros((0,), np.int64)
    tris, keys = np.concatenate(tris), np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    return tris[order], keys[order] // 12


def padded(triangles, cell, m):
    """The padded layout: the first min(T, M) rows, then NaN / -1."""
    tri, ce = np.full((m, 3, 3), np.nan, np.float32), np.full((m,), -1, np.int64)
    keep = min(len(triangles), m)
    tri[:keep], ce[:keep] = triangles[:keep], cell[:keep]
    return tri, ce


# ---- what a closed surface has to satisfy ---------------------------------------------------------------------------
def topology(triangles):
    """dict of V, E, F, euler, the number of directed edges that appear twice (`doubled`), of directed edges without their reverse
    (`open`) and of zero-area triangles; vertices are identified by their fp32 bits."""
    tri = np.ascontiguousarray(triangles, np.float32)
    bits = tri.reshape(-1, 3).view(np.uint32).astype(np.uint64)
    # +0.0 and -0.0 are one place
    bits = np.where(bits == 0x80000000, 0, bits)
    _, ids = np.unique(bits, axis=0, return_inverse=True)
    ids = ids.reshape(-1, 3)
    nondeg = (ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 0] != ids[:, 2])
    idn = ids[nondeg]
    n = int(ids.max()) + 1 if ids.size else 0
    a = np.concatenate((idn[:, 0], idn[:, 1], idn[:, 2])).astype(np.int64)
    b = np.concatenate((idn[:, 1], idn[:, 2], idn[:, 0])).astype(np.int64)
    directed = a * n + b
    uniq, counts = np.unique(directed, return_counts=True)
    reverse = np.unique(b * n + a)
    undirected = np.unique(np.minimum(a, b) * n + np.maximum(a, b))
    v = len(np.unique(idn))
    return {"V": v, "E": len(undirected), "F": int(nondeg.sum()), "euler": v - len(undirected) + int(nondeg.sum()),
            "doubled": int((counts > 1).sum()), "open": int(len(np.setdiff1d(uniq, reverse))), "degenerate": int((~nondeg).sum())}


def signed_volume(triangles):
    t = np.asarray(triangles, np.float64)
    return float(np.einsum("tk,tk->t", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


# ---- analytic fields and the cases the CPU and GPU tests share -------------------------------------------------------
def sphere_field(shape, origin, h, centre, radius):
    """acc (nz, ny, nx) float32 = |p - centre| - radius, weight 1."""
    px, py, pz = voxel_points(origin, h, shape)
    f = np.sqrt((px - centre[0]) ** 2 + (py - centre[1]) ** 2 + (pz - centre[2]) ** 2) - radius
    return f.astype(np.float32), np.ones(f.shape, np.float32)


def torus_field(shape, origin, h, centre, major, minor):
    """The ring in the x-y plane."""
    px, py, pz = voxel_points(origin, h, shape)
    ring = np.sqrt((px - centre[0]) ** 2 + (py - centre[1]) ** 2) - major
    f = np.sqrt(ring ** 2 + (pz - centre[2]) ** 2) - minor
    return np.broadcast_to(f, (shape[2], shape[1], shape[0])).astype(np.float32), np.ones((shape[2], shape[1], shape[0]), np.float32)


ANALYTIC_H, ANALYTIC_N = 0.37, 30
ANALYTIC_ORIGIN = tuple(-0.5 * ANALYTIC_H * (ANALYTIC_N - 1) for _ in range(3))
SPHERE_CENTRE, SPHERE_RADIUS = (0.13, -0.21, 0.07), 4.0
TORUS_CENTRE, TORUS_MAJOR, TORUS_MINOR = (0.13, -0.21, 0.07), 3.0, 1.2


def analytic(name, shape=(ANALYTIC_N,) * 3):
    if name == "sphere":
        return sphere_field(shape, ANALYTIC_ORIGIN, ANALYTIC_H, SPHERE_CENTRE, SPHERE_RADIUS)
    return torus_field(shape, ANALYTIC_ORIGIN, ANALYTIC_H, TORUS_CENTRE, TORUS_MAJOR, TORUS_MINOR)


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * k + (1 - math.cos(angle)) * (k @ k)


def compose(rows12, rot, shift=(0.0, 0.0, 0.0)):
    """The touch rows for an object that was moved by p' = rot p + shift before it was imaged with `rows12`: the map
    p -> rows12(rot p + shift)."""
    t = np.asarray(rows12, np.float64).reshape(3, 4)
    a = t[:, :3] @ np.asarray(rot, np.float64)
    b = t[:, :3] @ np.asarray(shift, np.float64) + t[:, 3]
    return np.concatenate((a, b[:, None]), axis=1).reshape(12)


def c_table():
    """The table as the kernel holds it: per (tetrahedron, mask) six bytes lo | hi << 4, 0xff where there is no triangle."""
    lines = []
    for rows in tet_table():
        cells = []
        for tris in rows:
            b = [lo | hi << 4 for tri in tris for lo, hi in tri]
            b += [0xff] * (6 - len(b))
            cells.append("{" + ", ".join(f"0x{x:02x}" for x in b) + "}")
        lines.append("  {" + ", ".join(cells) + "},")
    return "\n".join(lines)


if __name__ == "__main__":
    print(c_table())
