"""What the fp32 (engine.UNetEngine) and the bf16 (engine_bf16.UNetEngineBF16) host-side schedules share: the network's topology
under the reference's parameter names, the level pyramid, the BatchNorm statistics launches of both directions, the side stream
of the weight gradients and the hand-off of finished gradient blocks.

Nothing here asks which engine it serves: what differs between the two (the partial-row layout, when the one-launch BatchNorm
forms apply, the workspaces' sizes) comes in as an argument or as an attribute the engine's own _ensure sets
(partials, wgrad_ws, wgrad_ws_side, side).
"""
from __future__ import annotations

import os
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from ._lib import lib, check

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


class ConvUnit:
    """conv3x3(no bias) + BatchNorm2d + ReLU (unet.py:11-13 / :14-16)."""

    def __init__(self, prefix: str, conv_idx: int, bn_idx: int, cin: int, cout: int, level: int):
        self.cin, self.cout, self.level = cin, cout, level
        self.wname = f"{prefix}.double_conv.{conv_idx}.weight"
        bn = f"{prefix}.double_conv.{bn_idx}."
        self.gname, self.bname = bn + "weight", bn + "bias"
        self.rmname, self.rvname, self.nbtname = bn + "running_mean", bn + "running_var", bn + "num_batches_tracked"
        self.need_dgrad = True
        # device buffers (filled by the engine)
        self.wt_f = self.wt_d = None
        self.scale = self.shift = self.mean = self.invstd = self.c1 = self.c2 = None
        self.sums = None
        self.g = None
        self.fused_rows = 0         # partial rows written by the dX launch whose epilogue did pass 1 of this unit's BatchNorm backward


class UpUnit:
    """ConvTranspose2d(cin, cin//2, 2, 2) (unet.py:36)."""

    def __init__(self, j: int, cin: int, level_in: int):
        self.j, self.cin, self.cout, self.level_in = j, cin, cin // 2, level_in
        self.wname, self.bname = f"up.{j}.up.weight", f"up.{j}.up.bias"
        self.wt_f = self.wt_d = None


class EngineBase:
    Unit = ConvUnit     # the engine's own unit classes
    Up = UpUnit
    # library switches that change launch plans, so that the engine's buffers are sized from them (see the engines)
    _SIZING_ENV: Tuple[str, ...] = ()

    def __init__(self, n_channels: int, n_classes: int, layer_dimensions: Sequence[int]):
        dims = list(layer_dimensions)
        self.n_channels, self.n_classes, self.dims = n_channels, n_classes, dims
        self.L = len(dims) - 1
        Unit, Up = self.Unit, self.Up
        self.enc: List[Tuple[ConvUnit, ConvUnit]] = []
        self.dec: List[Tuple[ConvUnit, ConvUnit]] = []
        self.ups: List[UpUnit] = []
        self.enc.append((Unit("inc", 0, 1, n_channels, dims[0], 0), Unit("inc", 3, 4, dims[0], dims[0], 0)))
        self.enc[0][0].need_dgrad = False
        for i in range(self.L):
            p = f"down.{i}.maxpool_conv.1"
            self.enc.append((Unit(p, 0, 1, dims[i], dims[i + 1], i + 1), Unit(p, 3, 4, dims[i + 1], dims[i + 1], i + 1)))
        for j, i in enumerate(range(self.L, 0, -1)):
            cin, cout = dims[i], dims[i - 1]
            # Up(cin, cout): ConvTranspose2d(cin, cin//2) then DoubleConv(cin, cout) on cat[skip, up] (unet.py:36-37,48):
            # the reference only runs when skip channels + cin//2 == cin.
            if dims[i - 1] + cin // 2 != cin:
                raise ValueError(f"layer_dimensions {dims}: level {i} needs dims[i-1] + dims[i]//2 == dims[i] "
                                 "(the reference model fails at torch.cat/conv otherwise)")
            self.ups.append(Up(j, cin, i))
            p = f"up.{j}.conv"
            # DoubleConv(in_channels=cin, out=cout): input = cat[skip (dims[i-1]), up (cin//2)]
            self.dec.append((Unit(p, 0, 1, cin, cout, i - 1), Unit(p, 3, 4, cout, cout, i - 1)))
        self.units: List[ConvUnit] = [u for pair in self.enc for u in pair] + [u for pair in self.dec for u in pair]
        self._shape = None
        # times the engine's _ensure has (re)made its buffers: whatever holds raw pointers into them (graph.GraphedInference)
        # is stale once this moves
        self.buffers_made = 0
        self.sync_fn: Optional[Callable[[torch.Tensor], None]] = None   # SyncBN hook: all-reduce fp64 sums in place
        self.world = 1
        self.block_done_cb: Optional[Callable[[str], None]] = None   # data-parallel hook: a block's grads are final
        self._nbt: list = []   # num_batches_tracked buffers of the current train-mode forward
        self.guard = None          # non-finite guard of the current step (_lib.make_guard), set by TrainStep per step
        self.generation = 0        # forwards so far: a backward belongs to exactly one (models/unet.py checks it)
        self.side: Optional[torch.cuda.Stream] = None       # weight gradients (_on_side); the engine's _ensure makes it
        self._handoff: Optional[torch.cuda.Stream] = None   # bucket hand-off to the all-reduce (see _announce)
        self.kernel_log: Optional[list] = None     # bench hook: when a list, the engine's timed launches append a row each
        self.region_log: Optional[list] = None     # bench hook: (region name, start event, end event)

    # ------------------------------------------------------------------ buffers
    def _env_key(self) -> tuple:
        """The environment's part of the shape key: a sizing switch flipped between two steps (a test's monkeypatch, a sweep in
        one process) re-sizes the buffers instead of overrunning them."""
        return tuple(os.environ.get(k) for k in self._SIZING_ENV)

    def _set_pyramid(self, h: int, w: int) -> Tuple[List[int], List[int]]:
        hs, ws = [h], [w]
        for _ in range(self.L):
            hs.append(hs[-1] // 2)
            ws.append(ws[-1] // 2)
        assert hs[-1] >= 1 and ws[-1] >= 1, "input too small for this many max-pools"
        self.hs, self.ws = hs, ws
        return hs, ws

    @staticmethod
    def _alloc_bn(u: ConvUnit, dev: torch.device) -> bool:
        """The unit's BatchNorm coefficient vectors and fp64 sums; True when they were (re)made."""
        if u.scale is not None and u.scale.device == dev:
            return False
        for nm in ("scale", "shift", "mean", "invstd", "c1", "c2"):
            setattr(u, nm, torch.empty((u.cout,), device=dev, dtype=torch.float32))
        u.sums = torch.empty((65 * 3 * u.cout,), device=dev, dtype=torch.float64)
        return True

    # ------------------------------------------------------------------ helpers
    def _pad_off(self, lvl: int) -> Tuple[int, int]:
        # F.pad(x1, [dX//2, dX-dX//2, dY//2, dY-dY//2]) (unet.py:43-47)
        dy = self.hs[lvl] - 2 * self.hs[lvl + 1]
        dx = self.ws[lvl] - 2 * self.ws[lvl + 1]
        return dy // 2, dx // 2

    def _last_unit(self) -> ConvUnit:
        return self.dec[-1][1] if self.L > 0 else self.enc[0][1]

    @staticmethod
    def _event() -> torch.cuda.Event:
        """A timing event recorded on the current stream (the bench hooks build their log rows from two of them)."""
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    # ------------------------------------------------------------------ forward
    def _begin_forward(self, x: torch.Tensor, backward_follows: bool) -> torch.Tensor:
        """Refuse what the kernels do not take, size the buffers (the engine's _ensure) and open a new generation."""
        if x.dtype != torch.float32 or not x.is_cuda:
            raise L.GsdError(f"{type(self).__name__}.forward needs a float32 tensor on the GPU (no CPU fallback)")
        x = x.contiguous()
        n, c, h, w = x.shape
        assert c == self.n_channels, f"expected {self.n_channels} input channels, got {c}"
        self._ensure(n, h, w, x.device, backward_follows)
        self._nbt = []
        self._x = x
        self.generation += 1       # every forward overwrites the saved activations
        return x

    def _bn_stats(self, u: ConvUnit, rows: int, mpad: int, count: float, P, st: int, one_launch: bool) -> None:
        """self.partials holds `rows` BatchNorm partial rows (2 * mpad floats each) of unit u's raw output: batch statistics ->
        (mean, invstd, scale, shift), running statistics, the batch counter.
        one_launch (a few hundred partial rows, no SyncBN exchange in between): column sums + finalize in ONE launch instead
        of three."""
        if one_launch:
            check(lib.gsd_bn_reduce_finalize(self.partials.data_ptr(), rows, mpad, u.cout, u.sums.data_ptr(), count,
                                             P[u.gname].data_ptr(), P[u.bname].data_ptr(), BN_EPS, BN_MOMENTUM,
                                             P[u.rmname].data_ptr(), P[u.rvname].data_ptr(), u.mean.data_ptr(),
                                             u.invstd.data_ptr(), u.scale.data_ptr(), u.shift.data_ptr(), self.guard, st),
                  "bn_reduce_finalize")
        else:
            check(lib.gsd_bn_reduce_partials(self.partials.data_ptr(), rows, mpad, u.cout, u.sums.data_ptr(), st),
                  "bn_reduce_partials")
            if self.sync_fn is not None:     # SyncBN: the fp64 sums are all-reduced between the two halves
                self.sync_fn(u.sums[:2 * u.cout])
                count *= self.world
            check(lib.gsd_bn_finalize(u.sums.data_ptr(), u.cout, count, P[u.gname].data_ptr(), P[u.bname].data_ptr(),
                                      BN_EPS, BN_MOMENTUM, P[u.rmname].data_ptr(), P[u.rvname].data_ptr(),
                                      u.mean.data_ptr(), u.invstd.data_ptr(), u.scale.data_ptr(), u.shift.data_ptr(),
                                      self.guard, st),
                  "bn_finalize")
        self._nbt.append(P[u.nbtname])   # int64 counter buffers (BatchNorm2d.num_batches_tracked): one add for all, below

    def _flush_counters(self) -> None:
        if self._nbt:
            L.add_counters(self._nbt, 1)        # one libgsd launch for every BatchNorm layer's counter
            self._nbt = []

    # ------------------------------------------------------------------ backward
    def _bn_bwd_sums(self, u: ConvUnit, rows: int, mpad: int, count: float, G, dwout: Optional[torch.Tensor], st: int,
                     one_launch: bool) -> None:
        """self.partials holds `rows` partial rows of unit u's dz: dgamma, dbeta (and with dwout the output conv's dW row that
        rides among the sums) into G, the coefficients c1 / c2 of the apply pass into u.
        mpad > 0: the rows come from a dX launch's epilogue (conv partial layout, 2 * mpad floats each); 0: from the
        stand-alone reduce kernels.  Without SyncBN the finalize of the three-launch form gets no global sums (NULL)."""
        dw_ptr = None if dwout is None else dwout.data_ptr()
        if one_launch:
            check(lib.gsd_bn_bwd_reduce_finalize(self.partials.data_ptr(), rows, mpad, u.cout, u.sums.data_ptr(), count,
                                                 G[u.gname].data_ptr(), G[u.bname].data_ptr(), dw_ptr, u.c1.data_ptr(),
                                                 u.c2.data_ptr(), st), "bn_bwd_reduce_finalize")
            return
        if mpad:
            check(lib.gsd_bn_reduce_partials(self.partials.data_ptr(), rows, mpad, u.cout, u.sums.data_ptr(), st),
                  "bn_reduce_partials")
        else:
            check(lib.gsd_bn_bwd_reduce_partials(self.partials.data_ptr(), rows, u.cout, u.sums.data_ptr(), st),
                  "bn_bwd_reduce_partials")
        gsum = None
        if self.sync_fn is not None:
            gsum = u.sums[:2 * u.cout].clone()
            self.sync_fn(gsum)
            count *= self.world
        check(lib.gsd_bn_bwd_finalize(u.sums.data_ptr(), L.ptr(gsum), u.cout, count, G[u.gname].data_ptr(),
                                      G[u.bname].data_ptr(), dw_ptr, u.c1.data_ptr(), u.c2.data_ptr(), st), "bn_bwd_finalize")

    def _on_side(self, launch) -> bool:
        """Run launch(stream pointer, workspace tensor) -- one weight-gradient launch -- behind everything issued so far: on the
        side stream when there is one (True), else on the current stream."""
        if self.side is None or self.kernel_log is not None:    # (a per-kernel timing pass wants every kernel alone on the chip)
            launch(L.stream_ptr(), self.wgrad_ws)
            return False
        self.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            launch(L.stream_ptr(), self.wgrad_ws_side)
        return True

    def _join_side(self) -> None:
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)

    def _announce(self, tag: str) -> None:
        """A block of gradients is final once BOTH streams have finished what was issued so far.  The callback (the bucket's
        all-reduce: RCCL orders itself behind the stream that is current when it is called) therefore runs under a hand-off
        stream that waits for the two -- the main stream does NOT: the dX chain of the next unit does not depend on this
        block's weight gradients and used to stall behind them nine times per step.

        The contract for a callback: it runs under a stream that has waited for the main and the side stream, and the main
        stream does not wait for that stream.  Work it launches there is therefore not ordered before the main stream's next
        launches or the optimiser, so it must leave its caller something to wait on (as GradSync.finish() does: it waits for
        the collectives' work handles).  With a kernel_log installed, or without a side stream, everything is on the main
        stream and the callback is called directly."""
        if self.block_done_cb is None:
            return
        if self.side is None or self.kernel_log is not None:
            self.block_done_cb(tag)
            return
        if self._handoff is None:
            self._handoff = torch.cuda.Stream(device=self.side.device)
        h = self._handoff
        h.wait_stream(torch.cuda.current_stream())
        h.wait_stream(self.side)
        with torch.cuda.stream(h):
            self.block_done_cb(tag)
