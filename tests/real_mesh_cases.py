"""Test helpers: the real object meshes under tests/golden/meshes/ (STL files of the objects the depth labels are made for, data
only) and the poses that tests/test_real_meshes_cpu.py and tests/test_gpu_real_meshes.py render them at.  Not a test, no product code.

The files differ from the procedural meshes of tests/mesh_depth_ref.py in what matters to the kernels: most are in metres
(`pc_scale` 1000), they are 15..80 mm across against a 12 x 16 mm image, `peg1` lies 40 mm off the origin, up to half of the
triangles have zero projected area, and four of the six are not closed.

One table serves both test files.  Per mesh: `pc_scale`; `bbox`, the bounding box in mm after scaling (lo, hi per axis, rounded to
1e-3 mm: a check of the reader, not an input of any pose); `centre`, the in-plane centre (a, b) in mm under '+y+z' -- the
coordinates in ascending axis order, here (y, z) -- which `centre_of` recomputes from `bbox` for any plane; `edge`, the offset in
mm from the centred pose that puts an outer edge of the object across the image, and the width that pose is rendered with; `raw`,
whether the pose of a user who forgot the offset is a case; `skip_differs`, the triangles that the record's fp32 rule skips and
raster_ref's fp64 rule keeps (walls that lean by 1e-7 mm; tests/test_real_meshes_cpu.py says why that is harmless).

Poses (t1 [m], t2 [m], theta [rad]), every number rounded to fp32 here, so that a device tensor holds exactly what the fp64
yardsticks are given:

  (a) centred on the object: the transformed centre R(theta) c + 1000 t lands on (0.2, -0.1) mm, theta = 0
  (b) the same at theta = 0.3          (c) the same at theta = -2.5
  (d) (a) + `edge`: an outer edge of the object crosses the image.  peg1 and the hexagonal plate touch the fingers up to their
      rim, so the contact width shows it.  The four 50..79 mm plates touch with a raised feature, and their rim lies millimetres below
      it: the rim is rendered with g = 0, where every covered pixel of the left finger is in contact
  (e) wholly off the image: (a) moved by the half-extent + (30, -25) mm
  (f) `raw` meshes only: (0.2, -0.1) mm, theta = 0.3, no offset; the image is partly or wholly empty"""
import functools
import math
import os

import numpy as np

import mesh_depth_ref as R

MESH_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes")
PLANE = "+y+z"
INDENT_MM = 0.8
SHIFT_MM = (0.2, -0.1)
THETAS = (0.0, 0.3, -2.5)          # poses (a), (b), (c)
OFF_MM = (30.0, -25.0)             # pose (e): beyond the half-extent by this much

MESHES = {
    "pattern_18_hex_1": dict(pc_scale=1000.0, triangles=12, bbox=((-25.0, -7.5, -10.0), (25.0, 7.5, 10.0)), centre=(0.0, 0.0),
                             edge=((7.07, 0.0), "contact"), raw=False),
    "peg1": dict(pc_scale=1.0, triangles=146, bbox=((-10.704, -10.700, 0.0), (10.661, 10.683, 80.0)), centre=(-0.009, 40.0),
                 edge=((0.0, 39.07), "contact"), raw=True),
    "pattern_05_3_lines_angle_2": dict(pc_scale=1000.0, triangles=932, bbox=((-22.5, -30.0, -29.731), (14.5, 29.731, 21.495)),
                                       centre=(-0.135, -4.118), edge=((28.93, 3.04), "zero"), raw=False,
                                       skip_differs=(223, 233, 264, 653)),
    "pattern_32": dict(pc_scale=1000.0, triangles=2932, bbox=((-22.498, -7.5, -30.0), (14.499, 21.495, 14.330)), centre=(6.998, -7.835),
                       edge=((13.5, 2.0), "zero"), raw=True, skip_differs=(2442, 2450, 2452, 2458, 2463, 2464, 2479, 2496, 2501, 2842)),
    "hex_key": dict(pc_scale=1000.0, triangles=3432, bbox=((-18.619, -39.5, -39.5), (10.619, 39.5, 39.5)), centre=(0.0, 0.0),
                    edge=((38.0, -37.5), "zero"), raw=False),
    "marble": dict(pc_scale=1000.0, triangles=6440, bbox=((-18.985, -39.5, -39.5), (10.985, 39.5, 39.5)), centre=(0.0, 0.0),
                   edge=((-38.43, 5.0), "zero"), raw=False),
}
NAMES = tuple(MESHES)


def f32(x):
    return float(np.float32(x))


@functools.lru_cache(maxsize=None)
def mesh(name):
    """The triangles of a fixture, float32 (T, 3, 3) in the file's units, through the package's reader."""
    from gelslim_depth_amd.mesh_depth import read_stl
    return read_stl(os.path.join(MESH_DIR, name + ".stl"))


def pc_scale(name):
    return MESHES[name]["pc_scale"]


def centre_of(name, plane=PLANE):
    """The in-plane centre (a, b) in mm, ascending axis order, of the table's bounding box."""
    perp, _, _, _ = R.plane_table(plane)
    lo, hi = MESHES[name]["bbox"]
    return tuple(0.5 * (lo[k] + hi[k]) for k in range(3) if k != perp)


def half_extent_of(name, plane=PLANE):
    perp, _, _, _ = R.plane_table(plane)
    lo, hi = MESHES[name]["bbox"]
    return tuple(0.5 * (hi[k] - lo[k]) for k in range(3) if k != perp)


@functools.lru_cache(maxsize=None)
def q_max(name, plane=PLANE, scale=None):
    """The half-thickness in mm: the largest |q| of the mesh."""
    _, _, q, _ = R.prepare(mesh(name), pc_scale(name) if scale is None else scale, plane)
    return float(q.max())


def contact_width(name, plane=PLANE):
    """g for 0.8 mm of indentation at the crest, as test_gpu_mesh_depth.widths_of's middle entry; fp32."""
    return f32(2 * (q_max(name, plane) - INDENT_MM))


def wide_width(name, plane=PLANE):
    """Fingers further apart than the object is thick: every image is 0."""
    return f32(2 * q_max(name, plane) + 1.0)


def centred_pose(name, theta, plane=PLANE, offset_mm=(0.0, 0.0), centre=None):
    """The fp32 pose that carries the in-plane centre (`centre_of`, or `centre`) onto SHIFT_MM + offset_mm at the angle theta."""
    ca, cb = centre_of(name, plane) if centre is None else centre
    c, s = math.cos(theta), math.sin(theta)
    t1 = SHIFT_MM[0] + offset_mm[0] - (c * ca - s * cb)
    t2 = SHIFT_MM[1] + offset_mm[1] - (s * ca + c * cb)
    return (f32(t1 * 1e-3), f32(t2 * 1e-3), f32(theta))


def cases(name, plane=PLANE):
    """[(label, pose, g)]: (a)..(e), and (f) for the `raw` meshes; pose and g hold fp32 values."""
    g = contact_width(name, plane)
    out = [(label, centred_pose(name, th, plane), g) for label, th in zip("abc", THETAS)]
    offset, kind = MESHES[name]["edge"]
    out.append(("d", centred_pose(name, 0.0, plane, offset), g if kind == "contact" else 0.0))
    ha, hb = half_extent_of(name, plane)
    out.append(("e", centred_pose(name, 0.0, plane, (ha + OFF_MM[0], -hb + OFF_MM[1])), g))
    if MESHES[name]["raw"]:
        out.append(("f", (f32(SHIFT_MM[0] * 1e-3), f32(SHIFT_MM[1] * 1e-3), f32(0.3)), g))
    return out


def case(name, label, plane=PLANE):
    return next(c for c in cases(name, plane) if c[0] == label)


def slack_mm(qmax):
    """The budget of tests/test_gpu_mesh_depth.py for the fp32 interpolation of q, 1e-4 mm, stated in ulps of q: it holds while
    the mesh's largest |q| is below 16 mm and doubles with every binade above (2e-4 mm for 16 <= |q| < 32)."""
    return 1e-4 * max(1.0, 2.0 ** (math.floor(math.log2(qmax)) - 3))


WIDE_MM = 1e-3          # an interval wider than this says little about the pixel
WIDE_CAP = 0.005        # at most this share of an image's pixels may be so wide


@functools.lru_cache(maxsize=None)
def interval(name, plane, pose, g, size, invert=False, scale=None, height_mm=12.0):
    """raster_ref's (lo, hi) of one image, channels (left, right); cached, and shared by the CPU and the GPU tests."""
    return R.raster_ref(mesh(name), pc_scale(name) if scale is None else scale, plane, tuple(pose), g, size, height_mm, False, invert)


def wide_share(lo, hi):
    return float((hi - lo > WIDE_MM).mean())


# ---- what the GPU module renders, stated once so that the CPU module can check the yardsticks' preconditions without a GPU -----
SIZES = ((24, 31), (40, 53))          # at 12 mm of height, as tests/test_gpu_mesh_depth.py


def inverted(pose):
    """The fp32 pose whose invert_affine=True picture is `pose`'s plain one (up to the rounding of the inverted numbers)."""
    return tuple(f32(v) for v in R.inverted_pose(pose))


def launches(name):
    """[(plane, size, LR_flip, invert_affine, [(label, pose, g)])]: one render_depth call each.  Every mesh: (a)..(f) and (a) at a
    width larger than the object, at both sizes, and (b) through invert_affine; peg1 once more with LR_flip; pattern_05 (a), (b),
    (c) and the inverted (b) under the other eleven planes of mesh_depth_ref.PLANES -- eight of them look at the plate edge-on,
    where 0.8 mm of indentation at the bounding box's centre touches nothing: those are rendered with g = 0."""
    wide = ("wide", case(name, "a")[1], wide_width(name))
    out = []
    for size in SIZES:
        out.append((PLANE, size, False, False, cases(name) + [wide]))
        out.append((PLANE, size, False, True, [("b", inverted(case(name, "b")[1]), contact_width(name))]))
    if name == "peg1":
        out.append((PLANE, SIZES[0], True, False, cases(name)))
    if name == "pattern_05_3_lines_angle_2":
        for plane in R.PLANES:
            if plane != PLANE:
                edge_on = R.plane_table(plane)[0] != 0          # the plate's thickness runs along x
                abc = [(label, pose, 0.0 if edge_on else g) for label, pose, g in cases(name, plane)[:3]]
                out.append((plane, SIZES[0], False, False, abc))
                out.append((plane, SIZES[0], False, True, [("b", inverted(abc[1][1]), abc[1][2])]))
    return out


def reflected_cases(name):
    """(a), (b), (c) for the mesh under pc_scale = -|pc_scale|: the object is reflected through the origin, and so is its centre."""
    centre = tuple(-c for c in centre_of(name))
    return [(label, centred_pose(name, th, centre=centre), contact_width(name)) for label, th in zip("abc", THETAS)]


# (name, size, pose label, invert_affine): the images whose Jacobian is held to the fp64 twin.  The two large meshes at 24 x 31: the
# twin costs a second there and four at 40 x 53.  peg1 twice: at (a) the peg lies along the aligned axis at theta = 0 and has no slope
# along it (largest |dR/da2| 0.0012, the facets' noise), so only (b) can tell a wrong a2 column from a right one.
JACOBIANS = (("hex_key", (24, 31), "b", False), ("pattern_05_3_lines_angle_2", (40, 53), "b", True), ("peg1", (40, 53), "a", False),
             ("peg1", (40, 53), "b", False), ("pattern_32", (24, 31), "a", False))
ACTIVE_MIN = 40
J_MIN = 0.05          # every axis of J exceeds this somewhere in every image ...
J_DEAD = {("peg1", "a"): 1}          # ... but this one, by name: (mesh, pose label) -> the axis of J that has no slope there


def live_axes(name, label, big):
    """Whether the largest |J| per axis of one image, `big` (3,), exceeds J_MIN on every axis that is not exempt by name."""
    return all(big[k] > J_MIN for k in range(3) if J_DEAD.get((name, label)) != k)


@functools.lru_cache(maxsize=None)
def twin_records(name, plane=PLANE):
    import mesh_pose_refine_ref as PR
    return PR.records(mesh(name), plane, pc_scale(name))


@functools.lru_cache(maxsize=None)
def twin_image(name, size, label, invert):
    """(pose, g, point_terms) of a JACOBIANS entry; the pose is the inverted one where the entry says invert_affine."""
    import mesh_pose_refine_ref as PR
    _, pose, g = case(name, label)
    pose = inverted(pose) if invert else pose
    return pose, g, PR.point_terms(twin_records(name), pose, np.float32(g), size, 12.0, False, invert)
