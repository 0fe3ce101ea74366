"""Every place where the package crosses from one stream to another is known to a test that makes one of the streams late.

test_gpu_stream_order.py perturbs the schedule through torch.cuda.Stream.wait_stream; it proves something only about the
crossings it reaches.  So the package's source is walked here: every call of wait_stream, wait_event, record_event,
torch.cuda.Stream(...) and torch.cuda.stream(...) must stand in the table below, next to the GPU test that exercises it (or
the reason why none does).  A new crossing that nobody added to the table fails here, without a GPU.

The second half checks the policy logic of stream_delays.delays on stub streams: which stream gets the sleep, what passes
through, what is counted.
"""
import ast
import os

import pytest

import stream_delays as D
from conftest import REPO

PACKAGE = os.path.join(REPO, "gelslim_depth_amd")
ORDER = "test_gpu_stream_order.py"
LATE = f"{ORDER}::test_results_do_not_depend_on_which_stream_is_late"
HANDOFF = f"{ORDER}::test_hand_off_callback_sees_final_gradients"
M1 = f"{ORDER}::test_m1_a_missing_join_is_rejected"
M2 = f"{ORDER}::test_m2_unguarded_scratch_buffers_are_rejected"
M3 = f"{ORDER}::test_m3_a_hand_off_that_skips_the_side_stream_is_rejected"
RCCL = "test_gpu_ddp.py::test_one_rank_rccl_step_is_bit_equal"
NOT_DELAYED = "not delayed: "

# (module, enclosing function, call) -> the tests that make a stream late across it, or NOT_DELAYED and the reason
CROSSINGS = {
    ("engine.py", "UNetEngine._allocate", "Stream"): [LATE],                 # the fp32 side stream
    ("engine.py", "UNetEngine._bn_bwd_tail", "wait_event"): [LATE, M2],      # gp_free: the d_raw scratch buffers used in turn
    ("engine.py", "UNetEngine._bn_bwd_tail", "record_event"): [LATE, M2],
    ("engine_bf16.py", "UNetEngineBF16._ensure", "Stream"): [LATE],          # the bf16 side stream
    ("engine_base.py", "EngineBase._on_side", "wait_stream"): [LATE],        # the fork of every weight-gradient launch
    ("engine_base.py", "EngineBase._on_side", "stream"): [LATE],
    ("engine_base.py", "EngineBase._join_side", "wait_stream"): [LATE, M1],  # the join at the end of backward
    ("engine_base.py", "EngineBase._announce", "Stream"): [HANDOFF, RCCL],   # the hand-off stream
    ("engine_base.py", "EngineBase._announce", "wait_stream"): [HANDOFF, M3, RCCL],
    ("engine_base.py", "EngineBase._announce", "stream"): [HANDOFF, RCCL],
    # the warm-up in front of a graph capture: an eval forward on a stream of its own that is joined and followed by a device-wide
    # synchronise before anything reads its output; the capture itself is not perturbed (delays() injects nothing into one)
    ("graph.py", "GraphedInference.__init__", "Stream"): NOT_DELAYED + "capture (the warm-up in front of it)",
    ("graph.py", "GraphedInference.__init__", "wait_stream"): NOT_DELAYED + "capture (the warm-up in front of it)",
    ("graph.py", "GraphedInference.__init__", "stream"): NOT_DELAYED + "capture (the warm-up in front of it)",
    # GradSync's instrumented path exists for the benchmark's collective timing; the production path issues the all-reduce under
    # the hand-off stream (above) and waits on the work handles
    ("distributed.py", "GradSync.set_timing", "Stream"): NOT_DELAYED + "bench only (timing=True)",
    ("distributed.py", "GradSync._reduce", "wait_stream"): NOT_DELAYED + "bench only (timing=True)",
    ("distributed.py", "GradSync._reduce", "stream"): NOT_DELAYED + "bench only (timing=True)",
    ("distributed.py", "GradSync.finish", "wait_stream"): NOT_DELAYED + "bench only (timing=True)",
}
METHODS = ("wait_stream", "wait_event", "record_event")


def dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    if isinstance(node, ast.Name):
        parts.append(node.id)
    return ".".join(reversed(parts))


class Crossings(ast.NodeVisitor):
    def __init__(self):
        self.scope, self.found = [], set()

    def _scoped(self, node):
        self.scope.append(node.name)
        self.generic_visit(node)
        self.scope.pop()

    visit_ClassDef = visit_FunctionDef = visit_AsyncFunctionDef = _scoped

    def visit_Call(self, node):
        name = dotted(node.func) if isinstance(node.func, ast.Attribute) else ""
        kind = None
        if name in ("torch.cuda.Stream", "torch.cuda.stream"):
            kind = name.rsplit(".", 1)[1]
        elif isinstance(node.func, ast.Attribute) and node.func.attr in METHODS:
            kind = node.func.attr
        if kind is not None:
            self.found.add((".".join(self.scope) or "<module>", kind))
        self.generic_visit(node)


def crossings_of(source):
    v = Crossings()
    v.visit(ast.parse(source))
    return v.found


def package_crossings():
    found = set()
    for root, _, files in os.walk(PACKAGE):
        for f in sorted(files):
            if f.endswith(".py"):
                path = os.path.join(root, f)
                with open(path) as fh:
                    found |= {(os.path.relpath(path, PACKAGE),) + c for c in crossings_of(fh.read())}
    return found


def test_the_walker_sees_every_kind_of_crossing():
    src = ("import torch\n"
           "class E:\n"
           "    def fork(self):\n"
           "        s = torch.cuda.Stream(device=0)\n"
           "        s.wait_stream(torch.cuda.current_stream())\n"
           "        with torch.cuda.stream(s):\n"
           "            e = s.record_event()\n"
           "        def inner():\n"
           "            torch.cuda.current_stream().wait_event(e)\n"
           "x = torch.cuda.Event()\n")
    assert crossings_of(src) == {("E.fork", "Stream"), ("E.fork", "wait_stream"), ("E.fork", "stream"), ("E.fork", "record_event"),
                                 ("E.fork.inner", "wait_event")}


def test_every_stream_crossing_is_in_the_table():
    found = package_crossings()
    new = sorted(found - set(CROSSINGS))
    gone = sorted(set(CROSSINGS) - found)
    assert not new, (f"stream crossings that no test makes late: {new} -- add a case to tests/{ORDER} that reaches them (or the reason "
                     "why a delay cannot) and list them in CROSSINGS")
    assert not gone, f"CROSSINGS lists what the package no longer has: {gone}"


def test_the_table_names_tests_that_exist():
    defined = {}
    for entry in CROSSINGS.values():
        if isinstance(entry, str):
            assert entry.startswith(NOT_DELAYED) and len(entry) > len(NOT_DELAYED)
            continue
        assert entry, "a crossing with no test"
        for test in entry:
            module, name = test.split("::")
            if module not in defined:
                with open(os.path.join(REPO, "tests", module)) as fh:
                    defined[module] = {n.name for n in ast.walk(ast.parse(fh.read())) if isinstance(n, ast.FunctionDef)}
            assert name in defined[module], test


# ------------------------------------------------------------------------------------------------ the policies, on stub streams
class StubStream:
    """As much of torch.cuda.Stream as delays() touches."""
    log = []

    def __init__(self, handle):
        self.cuda_stream = handle

    def wait_stream(self, stream):
        StubStream.log.append(("wait", self.cuda_stream, stream.cuda_stream))


class StubBackend:
    stream_cls = StubStream

    def __init__(self, main):
        self.main, self.is_capturing = main, False

    def current_stream(self):
        return StubStream(self.main.cuda_stream)       # a new object per call, as torch.cuda.current_stream() gives

    def capturing(self):
        return self.is_capturing

    def sleep(self, stream, ms):
        StubStream.log.append(("sleep", stream.cuda_stream, ms))


@pytest.fixture
def streams():
    StubStream.log = []
    return StubStream(1), StubStream(2), StubStream(3)


def schedule(main, side, hand):
    """One weight-gradient fork, one announce, the join."""
    side.wait_stream(StubStream(main.cuda_stream))
    hand.wait_stream(main)
    hand.wait_stream(side)
    main.wait_stream(side)


WAITS = [("wait", 2, 1), ("wait", 3, 1), ("wait", 3, 2), ("wait", 1, 2)]


def test_side_late_sleeps_on_the_forked_stream(monkeypatch, streams):
    main, side, hand = streams
    with D.delays(monkeypatch, D.SIDE_LATE, 2.5, backend=StubBackend(main)) as d:
        schedule(main, side, hand)
    assert StubStream.log == [("wait", 2, 1), ("sleep", 2, 2.5), ("wait", 3, 1), ("sleep", 3, 2.5), ("wait", 3, 2), ("wait", 1, 2)]
    assert (d.forks_of(side), d.delayed_of(side), d.slept_on(side)) == (1, 1, 1)
    assert (d.forks_of(hand), d.delayed_of(hand), d.slept_on(hand)) == (1, 1, 1)
    assert (d.forks_of(main), d.delayed_of(main), d.slept_on(main)) == (0, 0, 0)
    assert d.passed == 2 and d.total_forks() == 2 and d.total_delayed() == 2 and d.captured == 0


def test_main_late_sleeps_on_the_main_stream(monkeypatch, streams):
    main, side, hand = streams
    with D.delays(monkeypatch, D.MAIN_LATE, 1.0, backend=StubBackend(main)) as d:
        schedule(main, side, hand)
    assert StubStream.log == [("wait", 2, 1), ("sleep", 1, 1.0), ("wait", 3, 1), ("sleep", 1, 1.0), ("wait", 3, 2), ("wait", 1, 2)]
    assert (d.delayed_of(side), d.delayed_of(hand), d.slept_on(main), d.slept_on(side), d.slept_on(hand)) == (1, 1, 2, 0, 0)
    assert d.passed == 2


def test_none_only_counts(monkeypatch, streams):
    main, side, hand = streams
    with D.delays(monkeypatch, D.NONE, 1.0, backend=StubBackend(main)) as d:
        schedule(main, side, hand)
    assert StubStream.log == WAITS
    assert (d.forks_of(side), d.forks_of(hand), d.total_delayed(), d.passed) == (1, 1, 0, 2)


def test_nothing_is_injected_during_a_capture(monkeypatch, streams):
    main, side, hand = streams
    backend = StubBackend(main)
    backend.is_capturing = True
    with D.delays(monkeypatch, D.SIDE_LATE, 1.0, backend=backend) as d:
        schedule(main, side, hand)
    assert StubStream.log == WAITS
    assert (d.total_forks(), d.total_delayed(), d.captured) == (2, 0, 2)


def test_the_patch_ends_with_the_block(monkeypatch, streams):
    main, side, hand = streams
    orig = StubStream.wait_stream
    with D.delays(monkeypatch, D.SIDE_LATE, 1.0, backend=StubBackend(main)):
        assert StubStream.wait_stream is not orig
    assert StubStream.wait_stream is orig
    schedule(main, side, hand)
    assert StubStream.log == WAITS


def test_a_run_that_would_sleep_too_long_is_refused(monkeypatch, streams):
    main, side, _ = streams
    with D.delays(monkeypatch, D.SIDE_LATE, 20.0, backend=StubBackend(main)) as d:
        d.budget_ms = 45.0
        side.wait_stream(main)
        side.wait_stream(main)
        with pytest.raises(AssertionError, match="too large"):
            side.wait_stream(main)
    assert d.delayed_of(side) == 2 and StubStream.log.count(("sleep", 2, 20.0)) == 2


def test_delay_rule():
    assert D.delay_for(0.1) == 1.0 and D.delay_for(0.5) == 1.0      # a millisecond at the least
    assert D.delay_for(3.0) == 6.0                                   # twice the step
    assert D.delay_for(10.0) == 20.0 and D.delay_for(500.0) == 20.0  # 20 ms at the most
    with pytest.raises(AssertionError):
        D.delays(None, "sideways", 1.0, backend=StubBackend(StubStream(1))).__enter__()
