"""What one step of the fp32 engine (engine.UNetEngine) launches at a batch shape, decided without a device.

plan_step() asks the library's host-side queries (they read no device memory; the library reads its environment switches as it
does at launch) and returns a frozen StepPlan: per conv unit and per transposed convolution the form, the weight-image mode, the
partial rows and K slabs of every launch class, the flags that route tensors (pitched, fused_dw, act_once, cat_on,
pooled_pitched), the dW form the train-mode operands get, and the size of every shape-dependent buffer for a train-capable and for
an eval-only engine.  The engine turns the sizes into tensors and reads every decision from here; nothing in this module takes
a tensor.

    python -m gelslim_depth_amd.engine_plan N H W [--dims 64 128 ...] [--classes K]     prints the plan (no GPU needed)
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, fields
from typing import List, Optional, Sequence, Tuple

from . import _lib as L
from ._lib import lib

# per conv3x3 form (0 direct taps, 1 Winograd F(4,3) along rows, 2 two-dimensional Winograd F(2x4,3x3)):
WEIGHT_MODES = ((0, 1), (4, 5), (8, 9))     # gsd_weight_layout modes of the forward and of the dX image
PARTIAL_ROWS = (lib.gsd_conv3x3_partial_rows, lib.gsd_conv3x3_w43_partial_rows, lib.gsd_conv3x3_w2d_partial_rows)
# K-slab scratch the form would like for a shape (the two Winograd forms; 0: the shape runs unsplit)
WORKSPACE = (lambda *a: 0, lib.gsd_conv3x3_w43_workspace, lib.gsd_conv3x3_w2d_workspace)


def _r64(c: int) -> int:
    return (c + 63) // 64 * 64


def _r4(w: int) -> int:
    return (w + 3) // 4 * 4


@dataclass(frozen=True)
class ConvLaunch:
    """One conv3x3 forward or dX launch class.  Sizes are (Cin, Cout) of the LAUNCH: a dX launch reads Cout and writes Cin of its unit."""
    algo: int            # 0, 1 or 2
    weight_mode: int     # gsd_weight_layout mode of the weight image the launch reads
    partial_rows: int    # rows its statistics epilogue writes into `partials`
    workspace: int       # K-slab floats the form asks for (train mode; 0: unsplit, the direct form, every eval-mode launch)


@dataclass(frozen=True)
class UnitPlan:
    cin: int
    c0: int              # channels of the first source segment (the decoder's first convs: the skip tensor's)
    cout: int
    level: int
    need_dgrad: bool     # False: the first layer
    fwd: Tuple[ConvLaunch, ConvLaunch]   # indexed by `train`: fwd[False] the eval-mode launch, fwd[True] the train-mode one
    dgrad: Optional[ConvLaunch]
    wt_f_size: int       # serves both modes' images
    wt_d_size: int       # the first layer: the mode-1 image its input gradient reads (allocated with the backward buffers)
    bn_bwd_rows: int     # partial rows of the stand-alone gsd_bn_bwd_reduce
    bn_bwd_fused: bool   # dz and its partial sums come from a dX epilogue: the conv dX of the unit above, or the fused ConvT dX
    bn_bwd_fused_rows: int   # ... and the rows that launch writes (0 when not fused)
    pitched: bool        # gsd_bn_bwd_apply writes d_raw out of place into the pitched scratch buffer
    fused_dw: bool       # first layer: no dX, so dW forms d_raw itself (gsd_conv3x3_wgrad_bn) and the apply pass is skipped
    act_once: bool       # train-mode forward: relu(bn(.)) of the input is written once, pitched, and read as a plain source
    wgrad_workspace: int
    wgrad_bn_workspace: int  # of the fused first-layer dW (0 when fused_dw is off)
    dw_form: Optional[int]   # gsd_conv3x3_wgrad_form for the operands the train-mode step hands dW; None under fused_dw


@dataclass(frozen=True)
class UpPlan:
    cin: int
    cout: int
    level_in: int
    mode_d: int          # gsd_weight_layout mode of wt_d (gsd_convT2x2_dgrad_layout)
    bn_rows: int         # > 0: the dX launch also does pass 1 of the BatchNorm backward of the unit below (partial rows)
    wt_f_size: int
    wt_d_size: int
    cat_on: bool         # the decoder reads one concat buffer [activated skip | up]; the ConvT output is a view of it
    wgrad_workspace: int


@dataclass(frozen=True)
class BufferSizes:
    """Floats (db_sums, outw_sums: doubles) of the engine's shape-dependent scratch; 0: the buffer is not made."""
    partials: int
    conv_ws: int
    gp: int              # one pitched d_raw scratch buffer (the engine makes two when dW runs on a side stream)
    act_buf: int
    wgrad_ws: int
    wgrad_ws_side: int   # made only with a side stream
    db_sums: int
    outw_partials: int
    outw_sums: int


@dataclass(frozen=True)
class StepPlan:
    n: int
    h: int
    w: int
    hs: Tuple[int, ...]
    ws: Tuple[int, ...]
    units: Tuple[UnitPlan, ...]      # in the engine's `units` order: encoder pairs top down, then decoder pairs bottom up
    ups: Tuple[UpPlan, ...]
    pooled_pitched: Tuple[bool, ...]  # per level (index 0 unused): the max-pool output is row-pitched
    sizes: Tuple[BufferSizes, BufferSizes]   # indexed by `train`: an eval-only and a train-capable engine


def desc(c: int, h: int, w: int, pitch: int, deferred: bool = False, slack: int = L.SLACK, off: Tuple[int, int] = (0, 0)) -> L.gsd_src:
    """A gsd_src for the library's host-side queries (they read no device memory): a (c, h, w) segment with rows of `pitch`."""
    s = L.gsd_src()
    s.ptr = 256
    s.scale = s.shift = 256 if deferred else None
    s.C, s.H, s.W, s.relu, s.w_stride, s.slack = c, h, w, int(deferred), pitch, slack
    s.off_h, s.off_w = off
    s.c_stride = h * pitch
    s.n_stride = c * h * pitch
    return s


def conv_launch(algo: int, n: int, h: int, w: int, cin: int, cout: int, dgrad: bool = False, slabs: bool = True) -> ConvLaunch:
    """The launch class of form `algo` at a shape.  slabs=False: the launch gets no K-slab scratch (eval mode)."""
    return ConvLaunch(algo, WEIGHT_MODES[algo][int(dgrad)], PARTIAL_ROWS[algo](n, h, w, cout),
                      WORKSPACE[algo](n, h, w, cin, cout) if slabs else 0)


def choose_algo(n: int, h: int, w: int, cin: int, c0: int, cout: int, train: bool) -> int:
    """The library's preference for a launch shape (include/gsd.h: gsd_conv3x3_algo, gsd_conv3x3_prefers_w2d).  c0: channels
    of the first source segment.  Eval mode gets the forms whose bits do not depend on the batch (no row folding, no K slabs)."""
    if not train:
        # decided from N-independent quantities only: the one-image plan says direct or Winograd; Winograd means the 2-D form (no
        # row folding, no K slabs: image i of a batch gets the bits the image alone gets); where the 2-D form does not serve
        # the channel counts the direct form does (its tiles never span images either) -- never the row form, which folds rows
        # across images
        algo = lib.gsd_conv3x3_algo(1, h, w, cin, cout)
        if algo == 1:
            algo = 2 if lib.gsd_conv3x3_w2d_supported(cin, c0) else 0
        return algo
    algo = lib.gsd_conv3x3_algo(n, h, w, cin, cout)
    if algo == 1 and lib.gsd_conv3x3_w2d_supported(cin, c0) and lib.gsd_conv3x3_prefers_w2d(n, h, w, cin, cout, 1):
        algo = 2
    return algo


def choose(n: int, h: int, w: int, cin: int, c0: int, cout: int, train: bool, dgrad: bool = False) -> ConvLaunch:
    return conv_launch(choose_algo(n, h, w, cin, c0, cout, train), n, h, w, cin, cout, dgrad, slabs=train)


def plan_step(n_channels: int, n_classes: int, dims: Sequence[int], n: int, h: int, w: int) -> StepPlan:
    dims = list(dims)
    nl = len(dims) - 1
    hs, ws = [h], [w]
    for _ in range(nl):
        hs.append(hs[-1] // 2)
        ws.append(ws[-1] // 2)
    assert hs[-1] >= 1 and ws[-1] >= 1, "input too small for this many max-pools"
    pad_off = lambda lvl: ((hs[lvl] - 2 * hs[lvl + 1]) // 2, (ws[lvl] - 2 * ws[lvl + 1]) // 2)   # of F.pad around the up-sampled tensor
    # (cin, c0, cout, level) of every unit, in the engine's order
    shapes = [(n_channels, n_channels, dims[0], 0), (dims[0], dims[0], dims[0], 0)]
    for i in range(nl):
        shapes += [(dims[i], dims[i], dims[i + 1], i + 1), (dims[i + 1], dims[i + 1], dims[i + 1], i + 1)]
    for i in range(nl, 0, -1):      # cat[skip, up]: the skip tensor comes first
        shapes += [(dims[i], dims[i - 1], dims[i - 1], i - 1), (dims[i - 1], dims[i - 1], dims[i - 1], i - 1)]
    enc = lambda lvl: 2 * lvl                  # index of the first unit of encoder pair `lvl` / decoder pair j
    dec = lambda j: 2 * (nl + 1) + 2 * j

    # ---- forms: direct taps, Winograd F(4,3) rows or two-dimensional Winograd, per layer shape, per direction and per mode
    fwd, dgrad, pitched = [], [], []
    for i, (cin, c0, cout, lvl) in enumerate(shapes):
        lh, lw = hs[lvl], ws[lvl]
        fwd.append((choose(n, lh, lw, cin, c0, cout, False), choose(n, lh, lw, cin, c0, cout, True)))
        dgrad.append(choose(n, lh, lw, cout, cout, cin, True, dgrad=True) if i > 0 else None)
        # d_raw goes to a row-pitched scratch buffer (16-byte aligned rows) when both of its readers -- dW and dX of this unit --
        # are the Winograd kernels, which then move it as aligned 16-byte LDS-DMA pieces
        pitched.append(bool(lib.gsd_conv3x3_wgrad_takes_pitched_dy(n, lh, lw, cin, cout)) and (i == 0 or dgrad[i].algo >= 1))

    def dw_form(i: int, segs: List[L.gsd_src]) -> int:
        cin, _, cout, lvl = shapes[i]
        dy = desc(cout, hs[lvl], ws[lvl], _r4(ws[lvl]) if pitched[i] else ws[lvl], slack=0)
        return lib.gsd_conv3x3_wgrad_form(L.src_array(segs), len(segs), C.byref(dy), cin, cout, n, hs[lvl], ws[lvl])

    # ---- which tensors a train-mode forward writes activated and pitched (GSD_ACT_ONCE, default 1; 0: the deferred schedule).
    # The buffers serve both modes, so a tensor goes pitched only where the eval-mode forward reads it through the 2-D form too
    on = os.environ.get("GSD_ACT_ONCE", "1") != "0"
    w2d = lambda i: fwd[i][0].algo == 2 and fwd[i][1].algo == 2
    pays = lambda i, ca, pack: bool(lib.gsd_act_once_pays(n, hs[shapes[i][3]], ws[shapes[i][3]], ca, shapes[i][0], shapes[i][2], 0, 0, pack))
    takes_pitched = lambda i: bool(lib.gsd_conv3x3_wgrad_takes_pitched_act(n, hs[shapes[i][3]], ws[shapes[i][3]], shapes[i][0], shapes[i][2]))
    pooled_pitched = [False] * (nl + 1)
    cat_on = [False] * nl
    act_once = [False] * len(shapes)
    dw_segs: List[Optional[list]] = [None] * len(shapes)   # the activation operand of every unit's dW, as the train-mode step lays it out
    for i, (cin, c0, cout, lvl) in enumerate(shapes):
        lh, lw = hs[lvl], ws[lvl]
        if i % 2 == 1:       # second unit of a pair: the first's deferred output (dW keeps it where the forward reads an activated copy)
            act_once[i] = on and fwd[i][1].algo == 2 and pays(i, cin, 0)
            dw_segs[i] = [desc(cin, lh, lw, lw, deferred=True)]
        elif i == 0:         # the network's input: a plain tensor of the caller's, no slack around it
            dw_segs[i] = [desc(cin, lh, lw, lw, slack=0)]
        elif i < dec(0):     # the max-pool output
            plain, pitch = [desc(cin, lh, lw, lw)], [desc(cin, lh, lw, _r4(lw))]
            pooled_pitched[lvl] = on and w2d(i) and pays(i, cin, 2) and takes_pitched(i) and dw_form(i, plain) == dw_form(i, pitch)
            dw_segs[i] = pitch if pooled_pitched[lvl] else plain
        else:                # [skip | up]: two segments, or the level's concat buffer
            j = (i - dec(0)) // 2
            hu, wu = 2 * hs[lvl + 1], 2 * ws[lvl + 1]
            two = [desc(c0, lh, lw, lw, deferred=True), desc(cin - c0, hu, wu, wu, off=pad_off(lvl))]
            one = [desc(cin, lh, lw, _r4(lw))]
            cat_on[j] = on and pad_off(lvl) == (0, 0) and w2d(i) and pays(i, c0, 1) and takes_pitched(i) and \
                dw_form(i, two) == dw_form(i, one)
            dw_segs[i] = one if cat_on[j] else two

    # ---- transposed convolutions.  The dX queries read only slack and n_stride of dy (a contiguous tensor with slack)
    ups = []
    for j in range(nl):
        li = nl - j
        cin, cout = dims[li], dims[li] // 2
        dy = desc(cout, 2 * hs[li], 2 * ws[li], 2 * ws[li])
        mode_d = lib.gsd_convT2x2_dgrad_layout(C.byref(dy), cin, cout, n, hs[li], ws[li])
        # the LDS-DMA dX kernel can leave dz of the unit below and its per-channel sums (gsd_convT2x2_dgrad_bnrelu)
        bn_rows = lib.gsd_convT2x2_dgrad_bnrelu_partial_rows(C.byref(dy), cin, cout, n, hs[li], ws[li]) if mode_d == 7 else 0
        ups.append(UpPlan(cin, cout, li, mode_d, bn_rows, lib.gsd_weight_layout_size(6, cout, cin),
                          lib.gsd_weight_layout_size(mode_d, cout, cin), cat_on[j],
                          lib.gsd_convT2x2_wgrad_workspace(n, hs[li], ws[li], cin, cout)))

    # ---- units
    units = []
    for i, (cin, c0, cout, lvl) in enumerate(shapes):
        lh, lw = hs[lvl], ws[lvl]
        if i % 2 == 0:       # dz comes from the dX of the pair's second unit, always
            fused_rows = dgrad[i + 1].partial_rows
        elif i == enc(nl) + 1:       # the bottom unit: from the first ConvT dX
            fused_rows = ups[0].bn_rows if nl > 0 else 0
        elif i > dec(0) and (i - dec(0)) // 2 < nl - 1:      # a decoder's second unit: from the ConvT dX of the level above
            fused_rows = ups[(i - dec(0)) // 2 + 1].bn_rows
        else:                # from the max-pool backward or the output conv: the stand-alone reduce
            fused_rows = 0
        fused_dw = i == 0 and bool(lib.gsd_conv3x3_wgrad_bn_supported(n, lh, lw, cin, cout))
        wt_d_size = lib.gsd_weight_layout_size(dgrad[i].weight_mode if i > 0 else 1, cout, cin)
        units.append(UnitPlan(
            cin, c0, cout, lvl, i > 0, fwd[i], dgrad[i],
            max(lib.gsd_weight_layout_size(f.weight_mode, cout, cin) for f in fwd[i]), wt_d_size,
            lib.gsd_bn_bwd_partial_rows(n, cout, lh, lw), i % 2 == 0 or fused_rows > 0, fused_rows, pitched[i], fused_dw, act_once[i],
            lib.gsd_conv3x3_wgrad_workspace(n, lh, lw, cin, cout),
            lib.gsd_conv3x3_wgrad_bn_workspace(n, lh, lw, cin, cout) if fused_dw else 0,
            None if fused_dw else dw_form(i, dw_segs[i])))

    # ---- buffers: the maxima over the launches above.  An eval-only engine makes what its forward touches: `partials` sized
    # for the forward and dX epilogues, no backward scratch
    def sizes(train: bool) -> BufferSizes:
        part = [1] + [max(f.partial_rows for f in u.fwd) * 2 * _r64(u.cout) for u in units] + \
            [u.dgrad.partial_rows * 2 * _r64(u.cin) for u in units if u.dgrad]
        if not train:
            return BufferSizes(max(part), 0, 0, 0, 0, 0, 0, 0, 0)
        part += [u.bn_bwd_rows * 3 * u.cout for u in units] + [up.bn_rows * 2 * _r64(up.cin) for up in ups]
        ws_ = max([1] + [max(u.wgrad_workspace, u.wgrad_bn_workspace) for u in units] + [up.wgrad_workspace for up in ups])
        kc = n_classes * dims[0]
        return BufferSizes(
            partials=max(part),
            # K slabs for the launches that would leave most of the chip idle: train mode only -- an eval-mode forward keeps the
            # one summation order whatever the batch (image i of a batch == the image alone)
            conv_ws=max(max(u.fwd[True].workspace, u.dgrad.workspace if u.dgrad else 0) for u in units),
            gp=max([n * u.cout * hs[u.level] * _r4(ws[u.level]) for u in units if u.pitched] + [0]),
            # relu(bn(raw)) of a unit's input, pitched: ONE recycled scratch (the forward conv is its only reader)
            act_buf=max([n * u.cin * hs[u.level] * _r4(ws[u.level]) for u in units if u.act_once] + [0]),
            wgrad_ws=max(ws_, 64 * max(1, n_classes)), wgrad_ws_side=max(ws_, 64),
            # fp64 column sums of a dX launch's statistics (ConvT bias gradients): gsd_bn_reduce_partials wants (1 + 64) x 2 C doubles
            db_sums=65 * 2 * max(u.cin for u in units),
            # dW of the output conv for K > 1 (gsd_conv1x1_out_wgrad)
            outw_partials=lib.gsd_conv1x1_out_wgrad_rows(n, hs[0], ws[0]) * kc if n_classes > 1 else 0,
            outw_sums=65 * kc if n_classes > 1 else 0)

    return StepPlan(n, h, w, tuple(hs), tuple(ws), tuple(units), tuple(ups), tuple(pooled_pitched), (sizes(False), sizes(True)))


def format_plan(p: StepPlan) -> str:
    form = lambda c: "-" if c is None else f"{'dir w43 w2d'.split()[c.algo]}/{c.partial_rows}r/{c.workspace}"
    flags = lambda o, names: ",".join(nm for nm in names if getattr(o, nm)) or "-"
    out = [f"N={p.n} H={p.h} W={p.w}   launch columns: form/partial rows/K-slab floats",
           f"{'unit':>4} {'lvl':>3} {'HxW':>9} {'Cin':>5} {'Cout':>5} {'fwd eval':>18} {'fwd train':>22} {'dX':>22} {'bn bwd rows':>12} {'dW':>4}  flags"]
    for i, u in enumerate(p.units):
        rows = f"{u.bn_bwd_fused_rows} (dX)" if u.bn_bwd_fused else str(u.bn_bwd_rows)
        dw = "fus" if u.dw_form is None else "dir w43 w2d".split()[u.dw_form]
        out.append(f"{i:>4} {u.level:>3} {p.hs[u.level]:>4}x{p.ws[u.level]:<4} {u.cin:>5} {u.cout:>5} {form(u.fwd[False]):>18} "
                   f"{form(u.fwd[True]):>22} {form(u.dgrad):>22} {rows:>12} {dw:>4}  {flags(u, ('pitched', 'fused_dw', 'act_once'))}")
    for j, up in enumerate(p.ups):
        out.append(f"up{j:>2} {up.level_in:>3} {p.hs[up.level_in]:>4}x{p.ws[up.level_in]:<4} {up.cin:>5} {up.cout:>5} dX mode {up.mode_d} "
                   f"bn_rows {up.bn_rows} dW workspace {up.wgrad_workspace}  {flags(up, ('cat_on',))}")
    out.append("pooled_pitched " + " ".join(str(l) for l, v in enumerate(p.pooled_pitched) if v))
    for train in (False, True):
        out.append(("train " if train else "eval  ") + " ".join(f"{f.name}={getattr(p.sizes[train], f.name)}" for f in fields(BufferSizes)))
    return "\n".join(out)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="Print what one fp32 step launches at a batch shape (no GPU needed).")
    ap.add_argument("n", type=int)
    ap.add_argument("h", type=int)
    ap.add_argument("w", type=int)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 128, 256, 512, 1024])
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--classes", type=int, default=1)
    a = ap.parse_args()
    print(format_plan(plan_step(a.channels, a.classes, a.dims, a.n, a.h, a.w)))
