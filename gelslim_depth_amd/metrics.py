"""Per-image depth metrics (an addition: the reference reports one mean loss per pass): errors in the dataset's depth unit, the
error inside the contact patch, the overlap of the predicted and the true patch, the peak indentation and the slope error.

One libgsd launch (gsd_depth_metrics, include/gsd.h) writes a row of sums, counts and maxima per image of a batch, in the
network's normalised units; `summarise` turns the rows of a whole pass into figures on the host, where the conversion to
physical units is one factor.  harness.evaluate_metrics drives both over a loader."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import torch

from . import _lib as L
from ._lib import check, lib

COLS = L.GSD_DM_COLS
# columns of a row (include/gsd.h)
SUM_E, SUM_ABS, SUM_SQ, MAX_ABS, N_T, N_P, N_TP, C_ABS, C_SQ, PEAK_T, PEAK_P, SLOPE, NONFINITE = range(13)


class DepthMetrics:
    """What the metrics kernel and `summarise` need to know about the depth maps, in the network's units:

    `background`: the value of the undeformed gel (0 under min_max_to_0_-1); `contact_eps`: a pixel v is contact when
    |v - background| > contact_eps, tested in fp32 -- DepthLoss's test; `unit`: physical depth = unit * v + const, so a
    magnitude in network units times |unit| is one in `unit_name` (1.0: report network units).  `from_normalization` and
    `from_dataset` derive all three from a depth normalisation.  A value class like DepthLoss: comparable, hashable,
    `DepthMetrics(**d.spec()) == d`."""

    def __init__(self, background: float = 0.0, contact_eps: float = 1e-3, unit: float = 1.0, unit_name: str = "") -> None:
        def number(name, v, what, ok):
            try:
                f = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"DepthMetrics: {name} must be a number, got {v!r}") from None
            if not (math.isfinite(f) and ok(f)):
                raise ValueError(f"DepthMetrics: {name} must be {what}, got {v!r}")
            return f
        self.background = number("background", background, "finite", lambda f: True)
        self.contact_eps = number("contact_eps", contact_eps, "finite and not negative", lambda f: f >= 0.0)
        self.unit = number("unit", unit, "finite and not zero", lambda f: f != 0.0)
        if not isinstance(unit_name, str):
            raise ValueError(f"DepthMetrics: unit_name must be a string, got {unit_name!r}")
        self.unit_name = unit_name

    @classmethod
    def from_normalization(cls, method: str, norm_scale: float, params, contact_depth: float, unit_name: str = "mm") -> "DepthMetrics":
        """The spec of a depth normalisation (processing.depth_denorm_affine: physical = A*v + B): unit = A, background = the
        network value of physical depth 0, -B/A, and contact_eps = contact_depth/|A| -- `contact_depth` is the indentation, in
        physical units, beyond which a pixel counts as contact."""
        from .processing import depth_denorm_affine
        a, b = (float(v) for v in depth_denorm_affine(method, norm_scale, params))
        if not math.isfinite(a) or a == 0.0:
            raise ValueError(f"DepthMetrics.from_normalization: {method!r} gives the degenerate scale {a!r}")
        try:
            depth = float(contact_depth)
        except (TypeError, ValueError):
            raise ValueError(f"DepthMetrics: contact_depth must be a number, got {contact_depth!r}") from None
        if not (math.isfinite(depth) and depth >= 0.0):
            raise ValueError(f"DepthMetrics: contact_depth must be finite and not negative, got {contact_depth!r}")
        return cls(background=-b / a, contact_eps=depth / abs(a), unit=a, unit_name=unit_name)

    @classmethod
    def from_dataset(cls, device_dataset, contact_depth: float, unit_name: str = "mm") -> "DepthMetrics":
        """`from_normalization` with the depth normalisation a DeviceDataset applies."""
        d = device_dataset
        return cls.from_normalization(d.depth_normalization_method, d.norm_scale, d.depth_normalization_parameters,
                                      contact_depth, unit_name)

    def spec(self) -> Dict[str, object]:
        """Every field as a plain Python value."""
        return {"background": self.background, "contact_eps": self.contact_eps, "unit": self.unit, "unit_name": self.unit_name}

    def c_struct(self) -> "L.gsd_depth_metrics":
        """The gsd_depth_metrics the kernel reads (its two floats as fp32; the unit stays on the host)."""
        c = L.gsd_depth_metrics()
        c.background, c.contact_eps = self.background, self.contact_eps
        c.reserved[0] = c.reserved[1] = 0
        return c

    def __eq__(self, other) -> bool:
        return isinstance(other, DepthMetrics) and self.spec() == other.spec()

    def __hash__(self) -> int:
        return hash(tuple(self.spec().items()))

    def __repr__(self) -> str:
        return "DepthMetrics(" + ", ".join(f"{k}={v!r}" for k, v in self.spec().items()) + ")"


def depth_metrics_workspace(shape) -> int:
    """Doubles of scratch depth_metrics needs for an (N, K, H, W) output: N times a function of K*H*W."""
    n, k, h, w = (int(d) for d in shape)
    return int(lib.gsd_depth_metrics_workspace(n, k, h, w))


def depth_metrics(out: torch.Tensor, target: torch.Tensor, spec: DepthMetrics, table: Optional[torch.Tensor] = None,
                  ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (N, 16) float64 table of the (N, K, H, W) prediction `out` against `target`, one row per image (include/gsd.h has
    the columns), on the device; nothing is synchronised.  `table` and `ws` (depth_metrics_workspace(out.shape) float64) are
    allocated when not given; a row's bits depend on its image alone."""
    for name, t in (("output", out), ("target", target)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise L.GsdError(f"depth_metrics: {name} must be a contiguous float32 tensor on the GPU, got {t.dtype} on "
                             f"{t.device} (the kernel reads raw fp32; cast with .float() first)")
    if out.dim() != 4 or out.shape != target.shape:
        raise L.GsdError(f"depth_metrics: output {tuple(out.shape)} and target {tuple(target.shape)} must be one (N, K, H, W) shape")
    n, k, h, w = out.shape
    if table is None:
        table = torch.empty((n, COLS), device=out.device, dtype=torch.float64)
    elif table.dtype != torch.float64 or not table.is_cuda or not table.is_contiguous() or tuple(table.shape) != (n, COLS):
        raise L.GsdError(f"depth_metrics: table must be a contiguous ({n}, {COLS}) float64 tensor on the GPU")
    if ws is None:
        ws = torch.empty((depth_metrics_workspace(out.shape),), device=out.device, dtype=torch.float64)
    elif ws.dtype != torch.float64 or not ws.is_cuda or not ws.is_contiguous():
        raise L.GsdError("depth_metrics: ws must be a contiguous float64 tensor on the GPU")
    c = spec.c_struct()
    check(lib.gsd_depth_metrics(C.byref(c), out.data_ptr(), target.data_ptr(), n, k, h, w, table.data_ptr(), ws.data_ptr(),
                                ws.numel(), L.stream_ptr()), "depth_metrics")
    return table


def pairs_per_image(k: int, h: int, w: int) -> int:
    """Neighbour pairs column 11 sums over in one (K, H, W) image."""
    return k * (h * (w - 1) + (h - 1) * w)


SUMMARY_KEYS = ("images", "nonfinite_images", "images_without_contact", "mae", "rmse", "bias", "max_abs", "contact_mae",
                "contact_rmse", "contact_iou", "contact_iou_mean", "contact_precision", "contact_recall", "peak_mae", "peak_max",
                "slope_mae", "unit_name")


def summarise(table, counts: Sequence[int], spec: DepthMetrics) -> Dict[str, object]:
    """The figures of a pass from its rows (host code).  `table`: (images, 16) float64 on the CPU; `counts` = (m, pairs), the
    elements and the neighbour pairs of one image (K*H*W and pairs_per_image).  Images with a non-finite error (column 12 > 0)
    are counted in `nonfinite_images` and left out of everything else; over the remaining images I:

      images, nonfinite_images, images_without_contact (n_t = 0)                                      counts
      mae, rmse, bias, max_abs      sum |e| / sum m, sqrt(sum e^2 / sum m), sum e / sum m (signed), max |e|       x unit
      contact_mae, contact_rmse     sum |e| and sqrt(sum e^2) over the target's contact pixels / sum n_t          x |unit|
      contact_iou                   pooled: sum n_tp / sum (n_t + n_p - n_tp)
      contact_iou_mean              mean, over the images with a non-empty union, of their own IoU
      contact_precision, _recall    sum n_tp / sum n_p, sum n_tp / sum n_t
      peak_mae, peak_max            mean and max over I of |max |o - background| - max |t - background||          x |unit|
      slope_mae                     sum of column 11 / sum pairs: a difference of neighbouring pixels in depth units, not
                                    divided by a pixel pitch                                                      x |unit|

    Magnitudes are multiplied by |unit|, `bias` by unit, ratios by nothing; a ratio without a denominator is NaN, and an empty
    pass gives images = 0 and NaN for the rest."""
    tab = torch.as_tensor(table, dtype=torch.float64).reshape(-1, COLS)
    m, pairs = float(counts[0]), float(counts[1])
    bad = tab[:, NONFINITE] > 0
    rows = tab[~bad]
    n = int(rows.shape[0])
    nan = float("nan")
    out: Dict[str, object] = {"images": n, "nonfinite_images": int(bad.sum()), "images_without_contact": int((rows[:, N_T] == 0).sum())}
    scale, unit = abs(spec.unit), spec.unit

    def ratio(a: float, b: float) -> float:
        return a / b if b > 0 else nan
    col = rows.sum(dim=0).tolist() if n else [0.0] * COLS
    out["mae"] = scale * ratio(col[SUM_ABS], n * m)
    out["rmse"] = scale * math.sqrt(ratio(col[SUM_SQ], n * m)) if n else nan
    out["bias"] = unit * ratio(col[SUM_E], n * m)
    out["max_abs"] = scale * float(rows[:, MAX_ABS].max()) if n else nan
    out["contact_mae"] = scale * ratio(col[C_ABS], col[N_T])
    out["contact_rmse"] = scale * math.sqrt(ratio(col[C_SQ], col[N_T])) if col[N_T] > 0 else nan
    union = rows[:, N_T] + rows[:, N_P] - rows[:, N_TP]
    out["contact_iou"] = ratio(col[N_TP], float(union.sum()))
    has = union > 0
    out["contact_iou_mean"] = float((rows[has, N_TP] / union[has]).mean()) if bool(has.any()) else nan
    out["contact_precision"] = ratio(col[N_TP], col[N_P])
    out["contact_recall"] = ratio(col[N_TP], col[N_T])
    peak = (rows[:, PEAK_P] - rows[:, PEAK_T]).abs()
    out["peak_mae"] = scale * float(peak.mean()) if n else nan
    out["peak_max"] = scale * float(peak.max()) if n else nan
    out["slope_mae"] = scale * ratio(col[SLOPE], n * pairs)
    out["unit_name"] = spec.unit_name
    return out


LOG_KEYS = ("mae", "rmse", "contact_mae", "contact_iou", "peak_mae", "slope_mae")


def log_line(validation: Dict[str, object], test: Dict[str, object]) -> str:
    """The line harness.fit(metrics=...) emits per epoch, directly after the `Train loss: ...` line:

        Metrics [<unit_name>]: Validation mae <v>, rmse <v>, contact_mae <v>, contact_iou <v>, peak_mae <v>, slope_mae <v>; Test mae <v>, ...

    every value as {:.6f} (a NaN prints as nan); the unit name is the validation summary's, `[]` when empty."""
    def part(name, s):
        return name + " " + ", ".join("{} {:.6f}".format(k, float(s[k])) for k in LOG_KEYS)
    return "Metrics [{}]: {}; {}".format(validation["unit_name"], part("Validation", validation), part("Test", test))
