"""Host-side schedule of the U-Net hot path over libgsd's C ABI.

Mirrors the control flow of the reference model
(/root/reference/gelslim_depth/models/unet.py:79-88 forward; autograd's reverse sweep for backward)
but every arithmetic step is a libgsd kernel launch on torch's current HIP stream.  torch is used
for device memory (buffers) and, in data-parallel runs, for the RCCL collectives; no torch op
computes any part of the path (tests/test_gpu_robust.py checks that a fused train step dispatches no ATen compute op).

Data layout in HBM (all fp32 NCHW):
  raw[u]    raw conv3x3 output of every conv unit (pre-BN); ConvT, the head, dW and every eval-mode consumer apply
            (scale, shift, relu) on load.  In a train-mode forward relu(bn(raw)) is written ONCE where the model says it
            pays (GSD_ACT_ONCE, gsd_act_once_pays): row-pitched, so that the conv3x3 that reads it is the plain aligned
            launch the dX convs are -- into a recycled scratch buffer, or (skip tensors) into the level's concat buffer
  g[u]      gradient buffer of the same shape: da -> dz -> d_raw in place         -- 18 tensors
  pooled[l] max-pool output feeding encoder level l (l>=1);  dpooled[l] its gradient
  up[j]     transposed-conv output (+bias) of decoder j at (2h,2w), unpadded;  dup[j] its gradient
  cat[j]    (GSD_ACT_ONCE) concat buffer (N, 2C', H, pitch) of decoder j, zero-filled once: the activated skip tensor in
            channels [0,C'), up[j] is the view of channels [C',2C') -- the decoder's first conv and its dW read ONE plain source
  wt_*      per-step re-laid-out weights (k-major, out-channel contiguous)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib as L
from ._lib import lib, check
from .engine_base import BN_EPS, ConvUnit, EngineBase, UpUnit
from .engine_plan import PARTIAL_ROWS, WEIGHT_MODES, WORKSPACE, StepPlan, UnitPlan, UpPlan, choose_algo, plan_step


def _r64(c: int) -> int:
    return (c + 63) // 64 * 64


def _r4(w: int) -> int:
    return (w + 3) // 4 * 4


class _ConvForm:
    """One of the three conv3x3 forms -- 0 direct taps, 1 Winograd F(4,3) along rows, 2 two-dimensional Winograd F(2x4,3x3): its
    launches, without and with the engine's K-slab scratch (the direct form never splits K), and the library's queries about it.
    Which form a launch takes, and with how many rows and slabs, is the plan's matter (engine_plan.ConvLaunch)."""
    _CONV = ((lib.gsd_conv3x3, None), (lib.gsd_conv3x3_w43, lib.gsd_conv3x3_w43_ws), (lib.gsd_conv3x3_w2d, lib.gsd_conv3x3_w2d_ws))
    _DGRAD_BNRELU = ((lib.gsd_conv3x3_dgrad_bnrelu, None), (lib.gsd_conv3x3_w43_dgrad_bnrelu, lib.gsd_conv3x3_w43_dgrad_bnrelu_ws),
                     (lib.gsd_conv3x3_w2d_dgrad_bnrelu, lib.gsd_conv3x3_w2d_dgrad_bnrelu_ws))

    def __init__(self, algo: int):
        self.algo = algo
        self.mode_f, self.mode_d = WEIGHT_MODES[algo]
        self.partial_rows, self.workspace = PARTIAL_ROWS[algo], WORKSPACE[algo]

    @staticmethod
    def choose(n: int, h: int, w: int, cin: int, c0: int, cout: int, train: bool) -> "_ConvForm":
        return _FORMS[choose_algo(n, h, w, cin, c0, cout, train)]

    def run(self, ws, src, nsrc, wt, cin, cout, dst, ndst, part, n, h, w, st):
        """conv3x3 forward / dX; `ws`: the engine's K-slab scratch (train mode) or None."""
        plain, with_ws = self._CONV[self.algo]
        if with_ws is not None and ws is not None:
            return with_ws(src, nsrc, wt, cin, cout, dst, ndst, part, ws.data_ptr(), ws.numel(), n, h, w, st)
        return plain(src, nsrc, wt, cin, cout, dst, ndst, part, n, h, w, st)

    def run_bnrelu(self, ws, src, wt, cin, cout, dst, raw, scale, shift, mean, invstd, part, n, h, w, st):
        plain, with_ws = self._DGRAD_BNRELU[self.algo]
        if with_ws is not None and ws is not None:
            return with_ws(src, wt, cin, cout, dst, raw, scale, shift, mean, invstd, part, ws.data_ptr(), ws.numel(), n, h, w, st)
        return plain(src, wt, cin, cout, dst, raw, scale, shift, mean, invstd, part, n, h, w, st)


_FORMS = tuple(_ConvForm(algo) for algo in range(3))


def _of_plan(name: str) -> property:
    """A read-only view of one field of the owner's plan under the name the decision had as an attribute: nothing is copied."""
    return property(lambda self: getattr(self.plan, name))


class _Unit(ConvUnit):
    def __init__(self, prefix: str, conv_idx: int, bn_idx: int, cin: int, cout: int, level: int):
        super().__init__(prefix, conv_idx, bn_idx, cin, cout, level)
        self.plan: Optional[UnitPlan] = None   # every decision about this unit's launches at the current shape (engine_plan)
        self.raw = None
        self.dsrc = None  # d_raw as the dW / dX kernels read it: g itself, or the pitched scratch buffer (engine.gp)
        self.srcs = None  # gsd_src array kept for wgrad

    pitched, fused_dw, act_once = _of_plan("pitched"), _of_plan("fused_dw"), _of_plan("act_once")
    # the form of the train-mode forward launch and of the dX launch (None: the first layer)
    form_f = property(lambda self: _FORMS[self.plan.fwd[True].algo])
    form_d = property(lambda self: None if self.plan.dgrad is None else _FORMS[self.plan.dgrad.algo])


class _Up(UpUnit):
    def __init__(self, j: int, cin: int, level_in: int):
        super().__init__(j, cin, level_in)
        self.plan: Optional[UpPlan] = None
        self.out = self.dout = None
        self.cat = None            # the level's concat buffer when `out` is a view of it (GSD_ACT_ONCE)

    mode_d, bn_rows = _of_plan("mode_d"), _of_plan("bn_rows")


class UNetEngine(EngineBase):
    Unit, Up = _Unit, _Up

    def __init__(self, n_channels: int, n_classes: int, layer_dimensions: Sequence[int]):
        super().__init__(n_channels, n_classes, layer_dimensions)
        self.plan: Optional[StepPlan] = None   # what a step launches at the current shape; units and ups hold their part of it
        self._saved = False        # the last forward kept what a backward needs (train mode, or eval mode with keep=True)
        self._saved_eval = False   # ... and ran in eval mode: BatchNorm normalised with the running statistics
        # partial-row count up to which BatchNorm's column sums and finalize run as ONE launch (gsd_bn_[bwd_]reduce_finalize)
        self.one_launch_rows = int(os.environ.get("GSD_BN_ONE_LAUNCH_ROWS", "4096"))
        # weight gradients on a side stream: dW of a unit runs beside its dX and the BatchNorm backward of the unit below (they only
        # share d_raw as an input).  A dW block owns its CU (8 waves x 240 registers, 96 KiB of LDS), so the two streams interleave CU
        # by CU: dX keeps its stand-alone speed and dW fills the CUs dX's tails and the chain's small launches leave idle
        self.side_dw = os.environ.get("GSD_SIDE_DW", "1") != "0"
        # bench hooks.  kernel_log (EngineBase): every conv3x3 forward / dX launch appends the row _log_end builds
        self.wgrad_log: Optional[list] = None      # conv3x3 dW launches (+ slab reducer), same rows as kernel_log

    # per decoder / per level (index 0 unused), as lists: views of the plan
    cat_on = property(lambda self: [up.plan.cat_on for up in self.ups])
    pooled_pitched = property(lambda self: list(self.plan.pooled_pitched))

    # ------------------------------------------------------------------ buffers
    # Library switches that change the plan (the form a launch takes, tile shapes, partial-row and slab counts, weight-image modes,
    # which tensors go pitched): they are part of the shape key, so a switch flipped between two steps (a test's monkeypatch, a
    # sweep in one process) re-plans and re-sizes the buffers instead of running a stale plan.  tests/test_engine_plan_cpu.py
    # holds the list complete: every library switch that moves a plan must be named here
    _SIZING_ENV = ("GSD_W2D_TW", "GSD_W2D_TW8_PCT", "GSD_W43_TW", "GSD_W43_FOLD", "GSD_CONV_W2D", "GSD_CONV_ALGO", "GSD_W43_SPLIT",
                   "GSD_WGRAD_ALGO", "GSD_WGRAD_W2D", "GSD_WG2D_KX", "GSD_WG2D_BLOCKS", "GSD_WGRAD_BLOCKS", "GSD_WG43_TW",
                   "GSD_ACT_ONCE", "GSD_ACT_ONCE_FORCE", "GSD_W2D_X4", "GSD_W2D_SPLIT", "GSD_CONVT_DG_DMA", "GSD_WGRAD_FIRST")

    def _ensure(self, n: int, h: int, w: int, dev: torch.device, train: bool) -> None:
        key = (n, h, w, str(dev), self._env_key())
        if self._shape == key and (not train or self.units[0].g is not None):
            return
        self.buffers_made += 1     # past the early return: pooled, partials and the workspaces are re-made every time
        if self._shape != key:
            for u in self.units:
                u.raw = u.g = None
            for up in self.ups:
                up.out = up.dout = up.cat = None
            self.plan = plan_step(self.n_channels, self.n_classes, self.dims, n, h, w)
            for u, p in zip(self.units + self.ups, self.plan.units + self.plan.ups):
                u.plan = p
        self._shape = key
        self._set_pyramid(h, w)
        self._allocate(dev, train)

    @staticmethod
    def _strips_scratch(u: "_Unit", n: int, lh: int, lw: int) -> int:
        """Floats of conv_ws the train-mode forward and dX launches of unit u want for the strip list's statistics (0: rectangles)."""
        need = 0
        if u.plan.fwd[True].algo == 2:
            need = lib.gsd_conv3x3_w2d_strips_scratch(n, lh, lw, u.cin, u.cout)
        if u.plan.dgrad is not None and u.plan.dgrad.algo == 2:
            need = max(need, lib.gsd_conv3x3_w2d_strips_scratch(n, lh, lw, u.cout, u.cin))
        return int(need)

    def _allocate(self, dev: torch.device, train: bool) -> None:
        """self.plan's sizes and flags as tensors and streams; train: also what a backward needs."""
        plan, size = self.plan, self.plan.sizes[train]
        n, hs, ws = plan.n, plan.hs, plan.ws
        f32 = dict(device=dev, dtype=torch.float32)

        def fit(t: Optional[torch.Tensor], numel: int) -> torch.Tensor:
            return t if t is not None and t.numel() == numel and t.device == dev else torch.empty((numel,), **f32)

        for u in self.units:
            lh, lw = hs[u.level], ws[u.level]
            if u.raw is None:
                u.raw = L.slack_empty((n, u.cout, lh, lw), dev)   # dW reads it as 16-byte window pieces
            if train and u.g is None:
                u.g = torch.empty((n, u.cout, lh, lw), **f32)
            self._alloc_bn(u, dev)
            u.wt_f = fit(u.wt_f, u.plan.wt_f_size)
            # the first layer's dX runs only for an input gradient; where gsd_conv3x3_dgrad_bn does not take over (fused_dw off) it
            # is the direct form on the materialised d_raw (_input_dgrad)
            if u.need_dgrad or train:
                u.wt_d = fit(u.wt_d, u.plan.wt_d_size)
        self.act_buf = torch.empty((size.act_buf,), **f32) if size.act_buf else None
        for up in self.ups:
            li = up.level_in
            if up.out is None and up.plan.cat_on:
                # the level's concat buffer, zero-filled ONCE: nothing ever writes its pad columns or, where 2w = W - 1, the last
                # column of the up-sampled half -- the zero padding the plain aligned conv3x3 and dW launches read there
                up.cat = L.pitched_slack_zeros((n, 2 * up.cout, hs[li - 1], ws[li - 1]), dev)
                up.out = up.cat[:, up.cout:, :2 * hs[li], :2 * ws[li]]
            if up.out is None:
                up.out = L.slack_empty((n, up.cout, 2 * hs[li], 2 * ws[li]), dev)
            if train and up.dout is None:
                up.dout = L.slack_empty((n, up.cout, 2 * hs[li], 2 * ws[li]), dev)   # ConvT dX reads pixel PAIRS: 2 floats past odd rows
            up.wt_f = fit(up.wt_f, up.plan.wt_f_size)
            if train:
                up.wt_d = fit(up.wt_d, up.plan.wt_d_size)
        self.pooled = [None] + [(L.pitched_slack_zeros if plan.pooled_pitched[l] else L.slack_empty)((n, self.dims[l - 1], hs[l], ws[l]), dev)
                                for l in range(1, self.L + 1)]
        self.dpooled = [None] + ([torch.empty((n, self.dims[l - 1], hs[l], ws[l]), **f32)
                                 for l in range(1, self.L + 1)] if train else [None] * self.L)
        # pitched d_raw scratch: one unit at a time on one stream; with dW on the side stream two, used in turn (dW of a unit may
        # still read its buffer while the BatchNorm backward of the next unit writes the other)
        side = train and self.side_dw
        self.side = torch.cuda.Stream(device=dev) if side else None   # (a high-priority side stream measured the same)
        self.gps = [torch.empty((size.gp,), **f32) for _ in range(2 if side else 1)] if size.gp else None
        self.gp_turn = 0
        self.gp_free: List[Optional[torch.cuda.Event]] = [None, None]   # recorded on the side stream behind a buffer's last reader
        self.partials = torch.empty((size.partials,), **f32)
        # K-slab scratch; an unsplit deep-level launch on the strip list leaves its per-tile statistics there (never both at once)
        conv_ws = max([size.conv_ws] + ([self._strips_scratch(u, n, hs[u.level], ws[u.level]) for u in self.units] if train else []))
        self.conv_ws = torch.empty((conv_ws,), **f32) if conv_ws else None
        self.db_sums = torch.empty((size.db_sums,), device=dev, dtype=torch.float64) if train else None
        self.wgrad_ws = torch.empty((size.wgrad_ws,), **f32) if train else None
        self.wgrad_ws_side = torch.empty((size.wgrad_ws_side,), **f32) if side else None
        self.outw_partials = torch.empty((size.outw_partials,), **f32) if size.outw_partials else None
        self.outw_sums = torch.empty((size.outw_sums,), device=dev, dtype=torch.float64) if size.outw_sums else None

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _layouts(jobs, st: int) -> None:
        """gsd_weight_layout_batch over (mode, weights, Co, Ci, image) tuples."""
        arr = (L.gsd_wl_job * len(jobs))()
        for i, (mode, w, co, ci, wt) in enumerate(jobs):
            arr[i].w, arr[i].wt, arr[i].mode, arr[i].Co, arr[i].Ci = w.data_ptr(), wt.data_ptr(), mode, co, ci
        check(lib.gsd_weight_layout_batch(arr, len(jobs), st), "weight_layout_batch")

    @staticmethod
    def _act_src(u: _Unit) -> L.gsd_src:
        return L.make_src(u.raw, u.scale, u.shift, relu=True, slack=L.SLACK)

    def _activate(self, prev: _Unit, dst_t: torch.Tensor, st: int) -> None:
        """relu(bn(prev.raw)) into the pitched tensor dst_t (gsd_bnrelu_pitched)."""
        s, d = self._act_src(prev), L.make_dst(dst_t)
        check(lib.gsd_bnrelu_pitched(C.byref(s), C.byref(d), prev.raw.shape[0], st), "bnrelu_pitched")

    def _run_unit(self, u: _Unit, srcs: List[L.gsd_src], P: Dict[str, torch.Tensor], train: bool, st: int,
                  keep: bool = False, prev: Optional[_Unit] = None) -> None:
        """prev: the unit whose deferred output `srcs` describes.  Where the plan says so (act_once, train mode) it is written
        activated into the scratch buffer first and the conv reads that as a plain source; dW keeps the deferred one (u.srcs)."""
        n = u.raw.shape[0]
        lh, lw = self.hs[u.level], self.ws[u.level]
        form = u.plan.fwd[train]
        u.srcs = L.src_array(srcs)
        arr = u.srcs
        if train and prev is not None and u.plan.act_once:
            p = _r4(lw)
            act = self.act_buf[:n * u.cin * lh * p].view(n, u.cin, lh, p)[..., :lw]
            self._activate(prev, act, st)
            srcs = [L.make_src(act)]
            arr = L.src_array(srcs)
        dst = L.dst_array([L.make_dst(u.raw)])
        part = self.partials.data_ptr() if train else None
        ev = self._log_begin()
        check(_FORMS[form.algo].run(self.conv_ws if train else None, arr, len(srcs), u.wt_f.data_ptr(), u.cin, u.cout, dst, 1, part,
                                    n, lh, lw, st), "conv3x3")
        self._log_end(ev, u.cout, u.cin, n, lh, lw, form.algo, arr, len(srcs), train)
        if train:
            rows = form.partial_rows
            self._bn_stats(u, rows, _r64(u.cout), float(n * lh * lw), P, st,
                           one_launch=self.sync_fn is None and rows <= self.one_launch_rows)
        elif keep:   # a backward follows: also the running statistics as mean / invstd (same scale / shift bits)
            check(lib.gsd_bn_eval_coeffs_bwd(P[u.gname].data_ptr(), P[u.bname].data_ptr(), P[u.rmname].data_ptr(),
                                             P[u.rvname].data_ptr(), BN_EPS, u.cout, u.scale.data_ptr(), u.shift.data_ptr(),
                                             u.mean.data_ptr(), u.invstd.data_ptr(), st),
                  "bn_eval_coeffs_bwd")
        else:
            check(lib.gsd_bn_eval_coeffs(P[u.gname].data_ptr(), P[u.bname].data_ptr(), P[u.rmname].data_ptr(),
                                         P[u.rvname].data_ptr(), BN_EPS, u.cout, u.scale.data_ptr(), u.shift.data_ptr(), st),
                  "bn_eval_coeffs")

    def _log_begin(self):
        if self.kernel_log is None and self.region_log is None:
            return None
        return self._event()

    def _log_end(self, ev, m: int, k_ch: int, n: int, lh: int, lw: int, algo: int = 0, src=None, nsrc: int = 0,
                 with_ws: bool = True) -> None:
        """(kernel, ALGORITHMIC flops of the convolution = 2*9*M*K*pixels, events, shape, flops the MFMAs executed).
        src, nsrc: the launch's sources -- their class decides whether a two-dimensional Winograd launch ran the strip list."""
        if ev is None or self.kernel_log is None:
            return
        e = self._event()
        flops = 2.0 * m * k_ch * 9 * n * lh * lw
        if algo == 2:
            variant = "conv3x3_w2d_kernel"
            cls = lib.gsd_conv3x3_w2d_source_class(src, nsrc) if src is not None else 0
            executed = 2048.0 * lib.gsd_conv3x3_w2d_mfma_count_class(n, lh, lw, k_ch, m, cls, int(with_ws and self.conv_ws is not None))
        elif algo:
            variant = "conv3x3_w43_kernel"
            executed = 2048.0 * lib.gsd_conv3x3_w43_mfma_count(n, lh, lw, k_ch, m)   # one v_mfma_f32_16x16x4_f32 = 2048 flops
        else:
            variant = "conv3x3_dma_kernel<1,4>" if m <= 64 else "conv3x3_dma_kernel<2,2>"
            executed = flops
        self.kernel_log.append((variant, flops, ev, e, (m, k_ch, lh, lw), executed))

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor, P: Dict[str, torch.Tensor], train: bool, out: Optional[torch.Tensor] = None,
                keep: bool = False) -> torch.Tensor:
        """P: name -> tensor for every state_dict entry (reference names). Returns (N, n_classes, H, W).
        keep (eval mode): also keep what a backward() needs -- the launches and output bits are those of the plain eval forward
        (the eval forms, scale / shift from the running statistics; nothing updates the running statistics), the backward
        buffers are allocated and every unit's mean / invstd hold the running statistics."""
        keep = keep and not train
        x = self._begin_forward(x, train or keep)
        n, _, h, w = x.shape
        st = L.stream_ptr()
        self._saved = train or keep
        self._saved_eval = keep
        # every forward-mode weight layout of the pass: the 2-D Winograd images in one launch
        self._layouts([(u.plan.fwd[train].weight_mode, P[u.wname], u.cout, u.cin, u.wt_f) for u in self.units] +
                      [(6, P[up.wname], up.cout, up.cin, up.wt_f) for up in self.ups], st)
        region = self._log_begin() if self.region_log is not None else None
        for lvl in range(self.L + 1):
            u0, u1 = self.enc[lvl]
            if lvl == 0:
                srcs = [L.make_src(x)]
            else:
                if lvl == 1 and region is not None:       # bench hook: the `inc` double-conv forward (2 convs + BN statistics)
                    self.region_log.append(("inc_forward", region, self._event()))
                prev = self.enc[lvl - 1][1]
                s = self._act_src(prev)
                # train mode with a concat buffer at the level above: the pool also leaves the skip tensor activated in its channels
                above = self.ups[self.L - lvl]
                cat = above.cat if train and above.plan.cat_on else None
                skip_t = None if cat is None else cat[:, :prev.cout]
                if self.plan.pooled_pitched[lvl]:
                    dp = L.make_dst(self.pooled[lvl])
                    da = None if skip_t is None else C.byref(L.make_dst(skip_t))
                    check(lib.gsd_maxpool2_pitched(C.byref(s), C.byref(dp), da, n, st), "maxpool2_pitched")
                else:
                    check(lib.gsd_maxpool2(C.byref(s), self.pooled[lvl].data_ptr(), n, prev.cout, self.hs[lvl - 1],
                                           self.ws[lvl - 1], st), "maxpool2")
                    if skip_t is not None:
                        self._activate(prev, skip_t, st)
                srcs = [L.make_src(self.pooled[lvl], slack=L.SLACK)]
            self._run_unit(u0, srcs, P, train, st, keep)
            self._run_unit(u1, [self._act_src(u0)], P, train, st, keep, prev=u0)
        if self.L == 0 and region is not None:          # a one-level network (profiles/inc_block.py): the block ends here
            self.region_log.append(("inc_forward", region, self._event()))
        cur = self.enc[self.L][1]
        for j in range(self.L):
            up = self.ups[j]
            lvl = self.L - 1 - j
            s = self._act_src(cur)
            d = L.make_dst(up.out)
            check(lib.gsd_convT2x2(C.byref(s), up.wt_f.data_ptr(), P[up.bname].data_ptr(), up.cin, up.cout, C.byref(d), n,
                                   self.hs[lvl + 1], self.ws[lvl + 1], st), "convT2x2")
            skip = self.enc[lvl][1]
            u0, u1 = self.dec[j]
            if train and up.plan.cat_on:     # [activated skip | up]: one plain pitched source, for the conv and for its dW
                self._run_unit(u0, [L.make_src(up.cat, slack=L.SLACK)], P, train, st, keep)
            else:
                self._run_unit(u0, [self._act_src(skip), L.make_src(up.out, off=self._pad_off(lvl), slack=L.SLACK)], P, train, st,
                               keep)
            self._run_unit(u1, [self._act_src(u0)], P, train, st, keep, prev=u0)
            cur = u1
        self._flush_counters()
        if out is None:
            out = torch.empty((n, self.n_classes, h, w), device=x.device, dtype=torch.float32)
        s = self._act_src(cur)
        check(lib.gsd_conv1x1_out(C.byref(s), P["outc.conv.weight"].data_ptr(), P["outc.conv.bias"].data_ptr(), cur.cout,
                                  self.n_classes, out.data_ptr(), n, h, w, st), "conv1x1_out")
        return out

    # ------------------------------------------------------------------ backward
    def _bn_bwd_tail(self, u: _Unit, P, G, st: int, dwout: Optional[torch.Tensor] = None) -> None:
        """u.g holds dz and self.partials its per-block sums: finish BN backward, then dW.
        u.plan.bn_bwd_fused: the partials come from a dX epilogue (conv layout) instead of gsd_bn_bwd_reduce."""
        n = u.raw.shape[0]
        lh, lw = self.hs[u.level], self.ws[u.level]
        fused = u.plan.bn_bwd_fused
        rows = u.fused_rows if fused else u.plan.bn_bwd_rows   # fused: of the dX launch that wrote them
        # the one-launch form takes the output conv's dW row only from stand-alone rows
        self._bn_bwd_sums(u, rows, _r64(u.cout) if fused else 0, float(n * lh * lw), G, dwout, st,
                          one_launch=self.sync_fn is None and rows <= self.one_launch_rows and (dwout is None or not fused))
        if self._saved_eval:
            # eval-mode BatchNorm is the affine map raw * scale + shift: d_raw = scale * dz, i.e. the train-mode expression with
            # c1 = c2 = 0 (dgamma = sum dz * xhat and dbeta = sum dz above hold as they are, xhat from the running statistics)
            u.c1.zero_()
            u.c2.zero_()
        if u.plan.fused_dw:
            self._on_side(lambda sst, ws: check(
                lib.gsd_conv3x3_wgrad_bn(u.srcs, u.g.data_ptr(), u.raw.data_ptr(), u.scale.data_ptr(), u.mean.data_ptr(),
                                         u.invstd.data_ptr(), u.c1.data_ptr(), u.c2.data_ptr(), u.cin, u.cout,
                                         G[u.wname].data_ptr(), ws.data_ptr(), ws.numel(), n, lh, lw, sst), "conv3x3_wgrad_bn"))
            return
        turn = None
        if u.plan.pitched:
            p = _r4(lw)
            turn = self.gp_turn = (self.gp_turn + 1) % len(self.gps)
            if self.gp_free[turn] is not None:     # the dW launch that read this buffer two units ago
                torch.cuda.current_stream().wait_event(self.gp_free[turn])
                self.gp_free[turn] = None
            u.dsrc = self.gps[turn][:n * u.cout * lh * p].view(n, u.cout, lh, p)[..., :lw]
            out_ptr = u.dsrc.data_ptr()
        else:
            p, u.dsrc, out_ptr = 0, u.g, None
        check(lib.gsd_bn_bwd_apply(u.g.data_ptr(), u.raw.data_ptr(), u.scale.data_ptr(), u.mean.data_ptr(),
                                   u.invstd.data_ptr(), u.c1.data_ptr(), u.c2.data_ptr(), n, u.cout, lh, lw, out_ptr, p, st),
              "bn_bwd_apply")
        dy = L.make_src(u.dsrc)
        ev0 = self._log_begin() if self.wgrad_log is not None else None
        on_side = self._on_side(lambda sst, ws: check(
            lib.gsd_conv3x3_wgrad(u.srcs, len(u.srcs), C.byref(dy), u.cin, u.cout, G[u.wname].data_ptr(), ws.data_ptr(), ws.numel(),
                                  n, lh, lw, sst), "conv3x3_wgrad"))
        if ev0 is not None and not on_side:
            ev1 = self._event()
            form = u.plan.dw_form
            name = ("wgrad3x3_kernel", "wgrad3x3_w43_kernel", "wgrad3x3_w2d_kernel")[form]
            flops = 2.0 * u.cout * u.cin * 9 * n * lh * lw
            executed = 2048.0 * lib.gsd_conv3x3_wgrad_mfma_count(form, n, lh, lw, u.cin, u.cout) if form else flops
            self.wgrad_log.append((name, flops, ev0, ev1, (u.cout, u.cin, lh, lw), executed))
        if on_side and turn is not None:
            self.gp_free[turn] = self.side.record_event()

    def _join_side(self) -> None:
        super()._join_side()
        self.gp_free = [None, None]

    def _reduce(self, mode: int, u: _Unit, st: int, dpool: Optional[torch.Tensor] = None,
                dout: Optional[torch.Tensor] = None, wout: Optional[torch.Tensor] = None) -> None:
        n = u.raw.shape[0]
        lh, lw = self.hs[u.level], self.ws[u.level]
        da = L.make_src(u.g)
        check(lib.gsd_bn_bwd_reduce(mode, u.raw.data_ptr(), u.scale.data_ptr(), u.shift.data_ptr(), u.mean.data_ptr(),
                                    u.invstd.data_ptr(), C.byref(da), L.ptr(dpool), L.ptr(dout), L.ptr(wout),
                                    self.n_classes, u.g.data_ptr(), self.partials.data_ptr(), n, u.cout, lh, lw, st),
              "bn_bwd_reduce")

    def _dgrad(self, u: _Unit, P, dsts: List[L.gsd_dst], st: int, stats: bool = False) -> int:
        """dX of unit u into the destination segments.  stats: the launch also leaves per-channel partial sums of what it
        stored in self.partials (the conv epilogue's BatchNorm-statistics path); returns their row count."""
        n = u.raw.shape[0]
        lh, lw = self.hs[u.level], self.ws[u.level]
        s = L.src_array([L.make_src(u.dsrc)])
        ev = self._log_begin()
        check(u.form_d.run(self.conv_ws, s, 1, u.wt_d.data_ptr(), u.cout, u.cin, L.dst_array(dsts), len(dsts),
                           self.partials.data_ptr() if stats else None, n, lh, lw, st), "conv3x3 dgrad")
        self._log_end(ev, u.cin, u.cout, n, lh, lw, u.plan.dgrad.algo, s, 1)
        return u.plan.dgrad.partial_rows if stats else 0

    def _dgrad_fused(self, u: _Unit, prev: _Unit, P, st: int) -> None:
        """dX of unit u straight into prev.g as dz of prev's relu(bn(.)) (+ partial sums): u's input is prev's output."""
        n = u.raw.shape[0]
        lh, lw = self.hs[u.level], self.ws[u.level]
        s = L.make_src(u.dsrc)
        d = L.make_dst(prev.g)
        prev.fused_rows = u.plan.dgrad.partial_rows
        ev = self._log_begin()
        check(u.form_d.run_bnrelu(self.conv_ws, C.byref(s), u.wt_d.data_ptr(), u.cout, u.cin, C.byref(d), prev.raw.data_ptr(),
                                  prev.scale.data_ptr(), prev.shift.data_ptr(), prev.mean.data_ptr(),
                                  prev.invstd.data_ptr(), self.partials.data_ptr(), n, lh, lw, st),
              "conv3x3_dgrad_bnrelu")
        self._log_end(ev, u.cin, u.cout, n, lh, lw, u.plan.dgrad.algo, C.byref(s), 1)

    def _input_dgrad(self, u: _Unit, P, dx: torch.Tensor, st: int) -> None:
        """dX of the first conv (the gradient w.r.t. the network's input) into dx, after u's BatchNorm backward is final.
        fused_dw: d_raw was never stored, gsd_conv3x3_dgrad_bn forms it from dz and raw.  Otherwise gsd_bn_bwd_apply has left it
        in u.dsrc and the general direct-form dX runs on it."""
        n = u.raw.shape[0]
        lh, lw = self.hs[u.level], self.ws[u.level]
        if u.plan.fused_dw:
            check(lib.gsd_conv3x3_dgrad_bn(u.g.data_ptr(), u.raw.data_ptr(), u.scale.data_ptr(), u.mean.data_ptr(),
                                           u.invstd.data_ptr(), u.c1.data_ptr(), u.c2.data_ptr(), P[u.wname].data_ptr(), u.cin,
                                           u.cout, dx.data_ptr(), n, lh, lw, st), "conv3x3_dgrad_bn")
            return
        check(lib.gsd_weight_layout(1, P[u.wname].data_ptr(), u.cout, u.cin, u.wt_d.data_ptr(), st), "weight_layout")
        s = L.src_array([L.make_src(u.dsrc)])
        rc = lib.gsd_conv3x3(s, 1, u.wt_d.data_ptr(), u.cout, u.cin, L.dst_array([L.make_dst(dx)]), 1, None, n, lh, lw, st)
        if rc == L.GSD_ERR_UNSUPPORTED:
            raise NotImplementedError(f"gelslim_depth_amd.UNet: no kernel computes the input gradient of the first conv3x3 at "
                                      f"N={n} H={lh} W={lw} Cin={u.cin} Cout={u.cout}: "
                                      + lib.gsd_last_error().decode("utf-8", "replace"))
        check(rc, "conv3x3 dgrad (input)")

    def input_grad_supported(self, n: int, h: int, w: int) -> bool:
        """Whether backward(..., dx=...) has a kernel for an (n, n_channels, h, w) input: gsd_conv3x3_dgrad_bn when the first
        layer's fused dW is on (it serves every shape that one does), else the direct-form dX (any shape the direct form serves)."""
        u = self.enc[0][0]
        if lib.gsd_conv3x3_wgrad_bn_supported(n, h, w, u.cin, u.cout):
            return bool(lib.gsd_conv3x3_dgrad_bn_supported(n, h, w, u.cin, u.cout))
        return h < 32768 and w < 32768

    def backward(self, dout: torch.Tensor, P: Dict[str, torch.Tensor], G: Dict[str, torch.Tensor],
                 dx: Optional[torch.Tensor] = None) -> None:
        """dout: (N, n_classes, H, W) gradient of the loss w.r.t. the output.
        G: name -> tensor to receive every parameter's gradient (overwritten, not accumulated).
        dx: optional contiguous fp32 (N, n_channels, H, W) tensor to receive the gradient w.r.t. the input (overwritten).
        After an eval-mode forward(keep=True) the gradients are those of eval-mode BatchNorm (an affine map with the running
        statistics); nothing is all-reduced there, so a data-parallel engine (sync_fn set) refuses that case."""
        if not self._saved:
            raise L.GsdError("backward() needs a preceding train-mode forward()")
        if self._saved_eval and self.sync_fn is not None:
            raise NotImplementedError("UNetEngine.backward after an eval-mode forward is single-process only (sync_fn is set)")
        if dx is not None:
            x = self._x
            if dx.shape != x.shape or dx.dtype != torch.float32 or not dx.is_contiguous() or dx.device != x.device:
                raise L.GsdError(f"backward(dx=...): expected a contiguous float32 {tuple(x.shape)} tensor on {x.device}")
            u = self.enc[0][0]
            if u.plan.fused_dw and not self.input_grad_supported(x.shape[0], x.shape[2], x.shape[3]):
                raise NotImplementedError(f"gelslim_depth_amd.UNet: no kernel computes the input gradient at input shape "
                                          f"{tuple(x.shape)} with {u.cout} first-layer channels")
        dout = dout.contiguous()
        st = L.stream_ptr()
        n = dout.shape[0]
        # the dX-mode weight layouts (the weights have not changed since the forward)
        self._layouts([(u.plan.dgrad.weight_mode, P[u.wname], u.cout, u.cin, u.wt_d) for u in self.units if u.need_dgrad] +
                      [(up.plan.mode_d, P[up.wname], up.cout, up.cin, up.wt_d) for up in self.ups], st)
        last = self._last_unit()
        self._reduce(2, last, st, dout=dout, wout=P["outc.conv.weight"])
        check(lib.gsd_sum_planes(dout.data_ptr(), n, self.n_classes, dout.shape[2] * dout.shape[3],
                                 G["outc.conv.bias"].data_ptr(), self.wgrad_ws.data_ptr(), st), "sum_planes")
        dwout = G["outc.conv.weight"]
        if self.n_classes > 1:
            # K > 1: the reduce above leaves only row 0 of dW_out among its sums; all K rows come from a pass of their own
            # (aten::convolution_backward of unet.py:54; no reference config uses it, so it is not on the tuned path)
            lh, lw = self.hs[last.level], self.ws[last.level]
            check(lib.gsd_conv1x1_out_wgrad(last.raw.data_ptr(), last.scale.data_ptr(), last.shift.data_ptr(), dout.data_ptr(),
                                            last.cout, self.n_classes, dwout.data_ptr(), self.outw_partials.data_ptr(),
                                            self.outw_sums.data_ptr(), n, lh, lw, st), "conv1x1_out_wgrad")
            dwout = None
        for j in reversed(range(self.L)):
            u0, u1 = self.dec[j]
            up = self.ups[j]
            lvl = self.L - 1 - j
            # dz of u1 came from the output conv (j = L-1) or from the ConvT dX of the level above -- with its sums when fused
            self._bn_bwd_tail(u1, P, G, st, dwout)
            dwout = None
            self._dgrad_fused(u1, u0, P, st)
            self._bn_bwd_tail(u0, P, G, st)
            skip = self.enc[lvl][1]
            # the ConvT bias gradient is the per-channel sum of up.dout: the Winograd dX launch that writes up.dout leaves it
            # as statistics of its second (cropped) destination -- no second pass over up.dout
            db_fused = u0.plan.dgrad.algo >= 1
            rows = self._dgrad(u0, P, [L.make_dst(skip.g), L.make_dst(up.dout, off=self._pad_off(lvl))], st, stats=db_fused)
            if db_fused:
                check(lib.gsd_partials_channel_sums(self.partials.data_ptr(), rows, _r64(u0.cin), u0.cin, skip.cout, up.cout,
                                                    G[up.bname].data_ptr(), self.db_sums.data_ptr(), st), "partials_channel_sums")
            prev = self.dec[j - 1][1] if j > 0 else self.enc[self.L][1]
            hi, wi = self.hs[lvl + 1], self.ws[lvl + 1]
            xs = self._act_src(prev)
            dys = L.make_src(up.dout, slack=L.SLACK)
            self._on_side(lambda sst, ws, up=up, xs=xs, dys=dys, db_fused=db_fused, hi=hi, wi=wi: check(
                lib.gsd_convT2x2_wgrad(C.byref(xs), C.byref(dys), up.cin, up.cout, G[up.wname].data_ptr(),
                                       None if db_fused else G[up.bname].data_ptr(), ws.data_ptr(), ws.numel(), n, hi, wi, sst),
                "convT2x2_wgrad"))
            d = L.make_dst(prev.g)
            if up.plan.bn_rows:
                check(lib.gsd_convT2x2_dgrad_bnrelu(C.byref(dys), up.wt_d.data_ptr(), up.cin, up.cout, C.byref(d), prev.raw.data_ptr(),
                                                    prev.scale.data_ptr(), prev.shift.data_ptr(), prev.mean.data_ptr(),
                                                    prev.invstd.data_ptr(), self.partials.data_ptr(), n, hi, wi, st),
                      "convT2x2_dgrad_bnrelu")
                prev.fused_rows = up.plan.bn_rows
            else:
                check(lib.gsd_convT2x2_dgrad_as(up.plan.mode_d, C.byref(dys), up.wt_d.data_ptr(), up.cin, up.cout, C.byref(d), n, hi, wi, st),
                      "convT2x2_dgrad")
                self._reduce(0, prev, st)
            self._announce(f"dec{j}")      # up.{j}.* (and outc with the last decoder) are final
        for lvl in reversed(range(self.L + 1)):
            u0, u1 = self.enc[lvl]
            if lvl < self.L:
                self._reduce(1, u1, st, dpool=self.dpooled[lvl + 1])
            # the bottom unit's dz came from the first ConvT dX -- with its sums when that launch was the fused one
            self._bn_bwd_tail(u1, P, G, st, dwout)
            dwout = None
            self._dgrad_fused(u1, u0, P, st)
            self._bn_bwd_tail(u0, P, G, st)
            if lvl == 0 and dx is not None:
                self._input_dgrad(u0, P, dx, st)   # c1 / c2 are final; the first layer's dW runs beside it on the side stream
            self._announce(f"enc{lvl}")
            if lvl > 0:
                self._dgrad(u0, P, [L.make_dst(self.dpooled[lvl])], st)
        self._join_side()
