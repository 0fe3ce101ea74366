"""Make one stream late, on purpose and by a known amount (test_gpu_stream_order.py, test_stream_crossings_cpu.py, nccl_worker.py).
Not collected; torch is imported inside the functions.

The package forks work onto its secondary streams (the weight-gradient side stream, the hand-off stream of _announce, GradSync's
timing stream) through one call only: secondary.wait_stream(main).  delays() patches torch.cuda.Stream.wait_stream so that a
bounded sleep follows every such fork -- on the secondary stream (side_late: what was forked starts late while the main stream
runs on) or on the main stream (main_late: the secondary stream runs ahead of everything the main stream issues next).  An
order between two streams that is only observed, because one of them happens to be quick, then stops holding; an order that
a wait enforces holds whatever the sleep.  Joins (main.wait_stream(secondary)), waits between two secondary streams and
wait_event pass through unchanged, and nothing is injected while the current stream is capturing.

cycles_per_ms()   torch.cuda._sleep's cycles per millisecond, measured once per process
sleep_ms()        a sleep of that many milliseconds on one stream
delay_for()       the delay that goes with a measured step time
delays()          the context manager; it yields a Delays, which counts
independent()     whether two streams can run side by side at all (streams that share a hardware queue cannot be late for each other)
"""
import contextlib

SIDE_LATE, MAIN_LATE, NONE = "side_late", "main_late", "none"
POLICIES = (SIDE_LATE, MAIN_LATE, NONE)
MIN_MS, MAX_MS = 1.0, 20.0
BUDGET_MS = 5000.0       # all the sleeps of one perturbed run together: a case that needs more is too large for these tests

_CYCLES_PER_MS = None


def cycles_per_ms():
    """Spin cycles of torch.cuda._sleep per millisecond: a warm-up sleep, then one timed between two events; the probe grows until
    it lasts a millisecond, so that the events' resolution does not matter."""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        import torch
        cycles = 1_000_000
        for _ in range(4):
            torch.cuda._sleep(cycles)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 1.0:
                break
            cycles *= 10
        assert ms > 0.0, "torch.cuda._sleep took no time at all"
        _CYCLES_PER_MS = cycles / ms
    return _CYCLES_PER_MS


def sleep_ms(stream, ms):
    """Enqueue a sleep of `ms` milliseconds on `stream` (a bounded spin kernel: it ends by itself)."""
    import torch
    assert 0.0 < ms <= MAX_MS, f"a delay of {ms} ms: the tests sleep {MAX_MS} ms at the most"
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * cycles_per_ms()))


def delay_for(step_ms):
    """Twice an unperturbed step, a millisecond at the least, 20 at the most: the other stream can issue and finish the whole rest
    of the step inside one delay.  A stimulus, not a bound -- the mutations of test_gpu_stream_order.py prove it long enough."""
    return min(MAX_MS, max(MIN_MS, 2.0 * step_ms))


class TorchBackend:
    """What delays() needs of torch; test_stream_crossings_cpu.py puts stubs in its place."""

    def __init__(self):
        import torch
        self.stream_cls = torch.cuda.Stream
        self._torch = torch

    def current_stream(self):
        return self._torch.cuda.current_stream()

    def capturing(self):
        return self._torch.cuda.is_current_stream_capturing()

    def sleep(self, stream, ms):
        sleep_ms(stream, ms)


def key(stream):
    """Streams are compared by their handle: torch.cuda.current_stream() makes a new Python object at every call."""
    return stream.cuda_stream


class Delays:
    """What delays() yields.  Per secondary stream (by key()): forks seen and forks delayed; per stream: sleeps enqueued on it."""

    def __init__(self, policy, ms, main, budget_ms=BUDGET_MS):
        assert policy in POLICIES, policy
        self.policy, self.ms, self.main, self.budget_ms = policy, float(ms), main, budget_ms
        self.forks = {}          # secondary stream -> secondary.wait_stream(main) calls
        self.delayed = {}        # secondary stream -> of those, the ones a sleep followed
        self.slept = {}          # stream -> sleeps enqueued on it
        self.passed = 0          # wait_stream calls that are no fork from the main stream: joins, secondary on secondary
        self.captured = 0        # forks seen while the current stream was capturing: nothing injected

    def forks_of(self, stream):
        return 0 if stream is None else self.forks.get(key(stream), 0)

    def delayed_of(self, stream):
        return 0 if stream is None else self.delayed.get(key(stream), 0)

    def slept_on(self, stream):
        return 0 if stream is None else self.slept.get(key(stream), 0)

    def total_delayed(self):
        return sum(self.delayed.values())

    def total_forks(self):
        return sum(self.forks.values())

    def summary(self):
        return (f"{self.policy} {self.ms:.2f} ms: forks per secondary stream {sorted(self.forks.values(), reverse=True)}, "
                f"delayed {sorted(self.delayed.values(), reverse=True)}, passed through {self.passed}")


def _bump(d, k):
    d[k] = d.get(k, 0) + 1


@contextlib.contextmanager
def delays(monkeypatch, policy, ms, backend=None):
    """Patch wait_stream for the length of the block.  The stream that is current on entry is the main stream."""
    backend = backend or TorchBackend()
    main = backend.current_stream()
    d = Delays(policy, ms, main)
    orig = backend.stream_cls.wait_stream

    def wait_stream(self, stream):
        orig(self, stream)
        if key(stream) != key(main) or key(self) == key(main):
            d.passed += 1
            return
        _bump(d.forks, key(self))
        if policy == NONE:
            return
        if backend.capturing():
            d.captured += 1
            return
        assert (d.total_delayed() + 1) * d.ms <= d.budget_ms, \
            f"{d.total_delayed() + 1} delays of {d.ms} ms pass {d.budget_ms} ms: the case is too large for this test"
        target = self if policy == SIDE_LATE else main
        backend.sleep(target, d.ms)
        _bump(d.delayed, key(self))
        _bump(d.slept, key(target))

    with monkeypatch.context() as mp:
        mp.setattr(backend.stream_cls, "wait_stream", wait_stream)
        yield d


def independent(a, b, ms=2.0):
    """Whether work on stream b can run while stream a is busy.  Two streams are not always two queues: the runtime spreads its
    streams over a few hardware queues, and streams that share one run in the order of submission, whatever their waits say --
    no delay makes one of them late for the other.  A sleep goes on a, an event behind it, an event on b; b is independent when
    its event is over while a's is not."""
    a.synchronize()
    b.synchronize()
    sleep_ms(a, ms)
    busy = a.record_event()
    b.record_event().synchronize()
    free = not busy.query()
    busy.synchronize()
    return free
