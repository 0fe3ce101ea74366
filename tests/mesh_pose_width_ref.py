"""Test helpers for the pose search with an unknown grasp width (numpy, fp64, no GPU; nothing here is product code), DESIGN.md
section 18 restated on top of tests/mesh_pose_ref.py:

  * `depth_at_width`: the depth images of any width g >= 0 from ONE render at width 0, d_g = min(0, d_0 + g / 2) -- in fp64
    bitwise what mesh_depth_ref.raster_ref(..., g, delta=0) gives,
  * `width_half_spans`, `width_offsets`: the fourth axis' level schedule in fp32, as the product builds it,
  * `estimate_width_twin`: the 4-D coarse-to-fine search; every pose candidate is rendered once, at width 0, and each of its
    widths is derived from that render,
  * the cases the CPU and the GPU tests share: mesh_pose_ref.CASES with the true width unknown.

`python tests/mesh_pose_width_ref.py` runs the twin on both cases and prints the errors that the tests hold as constants."""
import numpy as np

import mesh_depth_ref as R
import mesh_pose_ref as P

START_WIDTH_ERROR = 0.35      # mm: the search starts at the true width + this
WIDTH_HALF_SPAN = 0.6         # mm
WIDTH_COUNT = 5


def depth_at_width(d0, g):
    """(2, H, W) fp64 at the width g >= 0 [mm] from the images d0 at width 0: right -max(0, Q - g/2) = min(0, -Q + g/2), left
    min(0, Q + g/2), and a pixel that is 0 at width 0 stays 0.  + 0.0 removes the sign of a zero."""
    assert float(g) >= 0.0
    return np.minimum(0.0, np.asarray(d0, np.float64) + float(g) / 2) + 0.0


def width_half_spans(half_span, count, levels):
    """(levels + 1,) fp32: entry l the half-span of level l, entry l + 1 = level l's step = 2 * half / (n - 1), in fp32."""
    out = [np.float32(half_span)]
    for _ in range(levels):
        out.append((np.float32(2.0) * out[-1]) / np.float32(count - 1))
    return np.asarray(out, np.float32)


def width_offsets(step, count):
    """(n,) fp32: (k - (n - 1) / 2) * step."""
    return ((np.arange(count, dtype=np.float32) - np.float32((count - 1) // 2)) * np.float32(step)).astype(np.float32)


def estimate_width_twin(tri, plane, observed, g_start, init, half_span, counts, levels, width_half_span, width_count, strides=None,
                        cost="mse", image_height_mm=12.0, contact_depth=0.0, LR_flip=False, invert_affine=False, verbose=True):
    """estimate_pose(..., width_half_span, width_count) for one observation (2, H, W): flat index pose_flat * n_w + k, the lowest
    among equal costs; a width below 0 is a row of NaN, hence +inf."""
    assert width_count >= 3 and width_count % 2 == 1 and width_half_span > 0
    size = observed.shape[1:]
    strides = (1,) * levels if strides is None else tuple(strides)
    spans = P.half_spans(half_span, counts, levels)
    w_spans = width_half_spans(width_half_span, width_count, levels)
    centre, centre_w = np.asarray(init, np.float32), np.float32(g_start)
    trace, renders = [], 0
    for lvl in range(levels):
        cand = P.candidates(centre, spans[lvl + 1], counts)
        cand_w = (centre_w + width_offsets(w_spans[lvl + 1], width_count)).astype(np.float32)
        rows = np.full((len(cand), width_count, P.ROW), np.nan)
        for k, pose in enumerate(cand):
            d0, _ = R.raster_ref(tri, 1.0, plane, tuple(float(p) for p in pose), 0.0, size, image_height_mm, LR_flip, invert_affine,
                                 delta=0.0)
            for j, g in enumerate(cand_w):
                if g >= 0:
                    rows[k, j] = P.row_ref(depth_at_width(d0, g), observed, strides[lvl], contact_depth)
        renders += len(cand)
        c = P.pose_cost_ref(rows, cost, P.n_points(size[0], size[1], strides[lvl])).reshape(-1)
        best = int(np.argmin(c))                      # the lowest flat index among equal costs
        ties = int((c == c[best]).sum())
        centre, centre_w = cand[best // width_count], cand_w[best % width_count]
        row, best_cost = rows.reshape(-1, P.ROW)[best], float(c[best])
        trace.append(best_cost)
        if verbose:
            print(f"  level {lvl}: step {spans[lvl + 1]}, width step {w_spans[lvl + 1]}, best {best} of {len(c)} ({ties} equal), "
                  f"width {centre_w}, cost {best_cost:.6e}", flush=True)
    return {"pose": centre, "width": centre_w, "cost": best_cost, "row": row, "trace": np.asarray(trace), "final_step": spans[levels],
            "final_width_step": w_spans[levels], "renders": renders}


def true_width(case):
    """The width of a case's observation, as the fp32 value the GPU renders it with."""
    return float(np.float32(P.contact_width(P.MESHES[case["mesh"]]())))


def start_width(case):
    return float(np.float32(np.float32(true_width(case)) + np.float32(START_WIDTH_ERROR)))


def run_case(name, counts=None, verbose=True):
    case = P.CASES[name]
    tri = P.MESHES[case["mesh"]]()
    truth, g = P.case_truth(case), true_width(case)
    observed, _ = R.raster_ref(tri, 1.0, P.PLANE, truth, g, case["size"], case["height_mm"], delta=0.0)
    got = estimate_width_twin(tri, P.PLANE, observed, start_width(case), P.case_start(case), case["half_span"],
                              case["counts"] if counts is None else counts, case["levels"], WIDTH_HALF_SPAN, WIDTH_COUNT, None,
                              case["cost"], case["height_mm"], verbose=verbose)
    got["error"] = P.pose_error_ref(got["pose"], truth)
    got["width_error"] = float(got["width"]) - g
    return got


if __name__ == "__main__":
    import time
    for case_name in P.CASES:
        t0 = time.time()
        print(case_name)
        res = run_case(case_name)
        print(f"{case_name}: {res['renders']} renders in {time.time() - t0:.0f} s, cost {res['cost']!r}, trace {res['trace'].tolist()}")
        print(f"{case_name}: error (mm, mm, rad) = {res['error'].tolist()}, width error (mm) = {res['width_error']!r}")
        print(f"{case_name}: final step (m, m, rad) = {res['final_step'].tolist()}, final width step (mm) = {float(res['final_width_step'])!r}")
