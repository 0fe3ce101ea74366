"""GPU: the geometry units and the data path run on the caller's stream, all of them, launch by launch.

Every entry point of libgsd takes torch's current stream (L.stream_ptr()), and gsd_cell_count also issues a hipMemsetAsync.  A
launch or a memset that went to the null stream instead would pass every test that runs on the default stream.  Here every
workload of geometry_state.WORKLOADS runs under a stream of the caller's:

  1. undisturbed (the side stream waits for the current one, the results are cloned on the side stream, the streams join): the
     bits are the default-stream run's;
  2. with the null stream made to matter.  In front of every unit call the hook fills new input tensors with NaN on the side
     stream, enqueues a sleep there (stream_delays.sleep_ms; delay_for: twice the workload's own unperturbed time between two
     events, within 1 .. 20 ms), and behind the sleep, still on the side stream, produces the inputs: a copy of the staged tensors
     plus + 0.  Then the unit is called.  Whatever it issued to another stream would run in front of its inputs and read NaN (or
     find its cell table not yet zeroed).  The results must still be the default-stream bits.

Two streams are not always two queues (test_gpu_stream_order.py): the side stream is probed with stream_delays.independent and
drawn again, ATTEMPTS times at the most, until it can run beside the default stream.

test_a_call_on_the_default_stream_is_seen proves that the stimulus sees: the same late inputs with the unit called under the
default stream give other bits.  It reads memory that stays allocated; nothing faults.  One process, no graphs.

Measured on an MI355X: 11 tests in 3.5 s, none above 0.6 s.  Unperturbed workload times and delays: mesh_grid 5.4 ms / 10.8 ms in
front of 20 unit calls, contact 4.7 / 9.3 ms (23 calls), mesh_volume 1.9 / 3.8 ms (7), touch_fusion 0.6 / 1.2 ms (6), metrics_data
1.7 / 3.5 ms (7).
"""
import pytest
import torch

import engine_state as E
import geometry_state as S
import stream_delays as D
from test_gpu_geometry_memory import NOT_FINITE

pytestmark = pytest.mark.gpu

ATTEMPTS = 8
_STAGED, _REFERENCE, _MS = {}, {}, {}


def staged(name):
    if name not in _STAGED:
        _STAGED[name] = S.WORKLOADS[name].stage()
        torch.cuda.synchronize()
    return _STAGED[name]


def reference(name):
    """(results, milliseconds) of the workload on the default stream, unperturbed; the second of two runs is timed (everything is
    loaded and warm) between two events."""
    if name not in _REFERENCE:
        w, inputs = S.WORKLOADS[name], staged(name)
        first = {k: E.snap(v) for k, v in w.run(inputs).items()}
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = w.run(inputs)
        e1.record()
        torch.cuda.synchronize()
        _REFERENCE[name], _MS[name] = {k: E.snap(v) for k, v in res.items()}, e0.elapsed_time(e1)
        E.same_results(first, _REFERENCE[name], f"{name}: the default-stream run repeats", not_finite=NOT_FINITE[name])
    return _REFERENCE[name], _MS[name]


def side_stream():
    """A stream that can run while the default stream is busy."""
    current = torch.cuda.current_stream()
    for _ in range(ATTEMPTS):
        s = torch.cuda.Stream()
        if D.independent(current, s):
            return s
    raise AssertionError(f"{ATTEMPTS} streams in a row share the default stream's hardware queue")


class Late(S.Hook):
    """inputs(): NaN into new tensors, a sleep, then the real values -- all on the side stream, which must be the current one."""

    def __init__(self, side, ms):
        self.side, self.ms, self.calls = side, ms, 0

    def inputs(self, what, *tensors):
        assert torch.cuda.current_stream().cuda_stream == self.side.cuda_stream, what
        assert (self.calls + 1) * self.ms <= D.BUDGET_MS, f"{self.calls + 1} delays of {self.ms} ms: too large a workload for this test"
        out = [None if t is None else torch.full_like(t, float("nan")) for t in tensors]
        self.side.synchronize()          # the NaN are in memory before anything behind the sleep is issued
        D.sleep_ms(self.side, self.ms)
        self.calls += 1
        for o, t in zip(out, tensors):
            if o is not None:
                o.copy_(t)
                o += 0
        return tuple(out)


def run_on(side, name, hook=None):
    """The workload under `side`, its results cloned there; then the streams join."""
    current = torch.cuda.current_stream()
    side.wait_stream(current)
    with torch.cuda.stream(side):
        res = E.on_device(S.WORKLOADS[name].run(staged(name), hook))
    current.wait_stream(side)
    torch.cuda.synchronize()
    return {k: E.snap(v) for k, v in res.items()}


@pytest.mark.parametrize("name", list(S.WORKLOADS))
def test_results_on_a_callers_stream_equal_the_default_streams(name):
    ref, _ = reference(name)
    got = run_on(side_stream(), name)
    E.same_results(ref, got, f"{name}: the default stream against a caller's stream", not_finite=NOT_FINITE[name])


@pytest.mark.parametrize("name", list(S.WORKLOADS))
def test_results_do_not_change_when_the_inputs_arrive_late_on_the_callers_stream(capsys, name):
    ref, ms = reference(name)
    side = side_stream()
    hook = Late(side, D.delay_for(ms))
    got = run_on(side, name, hook)
    with capsys.disabled():
        print(f"\n{name:<14} unperturbed {ms:7.3f} ms  delay {hook.ms:6.3f} ms  in front of {hook.calls} unit calls")
    assert hook.calls >= 5 and D.independent(torch.cuda.current_stream(), side)
    E.same_results(ref, got, f"{name}: the default stream against late inputs on a caller's stream", not_finite=NOT_FINITE[name])


# ------------------------------------------------------------------------------------- proof that the stimulus can see
def test_a_call_on_the_default_stream_is_seen():
    """render_depth and closest_points with late inputs, once called as they should be and once under the default stream -- what a
    launch that ignored the caller's stream amounts to.  The second reads its inputs while they still hold NaN."""
    from gelslim_depth_amd import mesh_depth as M
    from gelslim_depth_amd import mesh_register as G
    import mesh_pose_ref as P
    s = staged("mesh_grid")["lprism"]
    v = staged("mesh_volume")
    grid, vol = M.MeshGrid(s["tri"], 1.0, P.PLANE, S.DEV), G.MeshVolume(v["tri"], 1.0, S.DEV)
    want = {"render": E.snap(M.render_depth(grid, s["seen"], s["widths"], S.SIZE, 12.0, validate=False)),
            "triangle": E.snap(G.closest_points(vol, v["pts"]).triangle)}
    default = torch.cuda.current_stream()
    got = {}
    for label, under in (("caller", None), ("default", default)):
        side = side_stream()
        hook = Late(side, D.MAX_MS)
        side.wait_stream(default)
        with torch.cuda.stream(side):
            seen, widths, pts = hook.inputs("render_depth, closest_points", s["seen"], s["widths"], v["pts"])
            with torch.cuda.stream(side if under is None else under):
                res = {"render": M.render_depth(grid, seen, widths, S.SIZE, 12.0, validate=False), "triangle": G.closest_points(vol, pts).triangle}
                res = E.on_device(res)
        default.wait_stream(side)
        torch.cuda.synchronize()
        got[label] = {k: E.snap(t) for k, t in res.items()}
    E.same_results(want, got["caller"], "late inputs, the unit on the caller's stream")
    for k in want:
        with pytest.raises(AssertionError):       # (other bits, or NaN images)
            E.same_bits(want[k], got["default"][k], f"late inputs, the unit on the default stream: {k}")
