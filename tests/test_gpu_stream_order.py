"""The order between the engines' streams is enforced, not merely observed.

A train step runs on up to three streams: the caller's, the side stream of the weight gradients (engine_base._on_side) and the
hand-off stream under which _announce calls block_done_cb.  test_side_stream_weight_gradients_are_bit_identical and its bf16
twin compare the two-stream schedule with the one-stream one undisturbed; at their shapes a side launch has usually finished
before the main stream reaches the launch it would conflict with, so a wait that is missing passes there on most runs.  Here
one stream is made late by a known amount at every fork (stream_delays.delays), in both directions, and every result -- cloned
on the device right behind the last call, in front of the first synchronise -- must still be the bits of the one-stream
schedule, which other modules hold to fp64 launch by launch.  Nothing here has a tolerance.

The delay of a case is twice an unperturbed one-stream step of that case (a millisecond at the least): the other stream can issue
and finish the rest of the step inside one delay.  That rule is a stimulus, not a bound; three mutations prove it long enough:
without the join at the end of backward (M1), without the events that guard the two d_raw scratch buffers (M2) and without the
hand-off stream's wait for the side stream (M3) the same comparisons fail.  The mutations read stale values from allocations
that stay alive; none of them leaves one.

Two streams are not always two queues.  The runtime spreads its streams over a few hardware queues (four by default), and two
streams that share one run in the order of submission whatever their waits say: no delay makes one of them late for the other,
and a run on such a pair proves nothing.  Which pair an engine draws depends on how many streams the process has made before.
So every perturbed run is followed by a probe (stream_delays.independent) of the streams it used, and a run whose side stream
turns out to share the main stream's queue is made again with a new model, which draws the next stream.
"""
import pytest
import torch

import engine_state as S
import stream_delays as D
from test_gpu_engine_memory import BY_NAME, SWITCHES

pytestmark = pytest.mark.gpu

TWO_STREAM = ["fp32-default", "fp32-w2d-forced", "fp32-w2d-forced-37x45", "fp32-first-unfused", "fp32-two-classes", "fp32-kslabs-w2d",
              "fp32-bn-three-launch", "bf16-21x27", "bf16-inc-c64", "bf16-im2col", "bf16-unfused"]
CONTROL = ["fp32-one-stream", "bf16-one-stream"]       # no side stream: the context must see no fork at all
ONE_STREAM = {"fp32": {"GSD_SIDE_DW": "0"}, "bf16": {"GSD_BF16_SIDE_DW": "0"}}
FIRST = {"fp32": "fp32-default", "bf16": "bf16-21x27"}
PERTURBED = (D.SIDE_LATE, D.MAIN_LATE)

_REFERENCE = {}      # (case, workload) -> results of the one-stream schedule, unperturbed; made once, never changed
_STEP_MS = {}        # case -> milliseconds of one unperturbed one-stream train step
_FORKS = {}          # (case, workload) -> forks per run of the two-stream schedule (a count-only run)
ATTEMPTS = 8         # models made until one draws streams on queues of their own (a quarter of the streams share the main one's)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in SWITCHES + ["GSD_ACT_ONCE", "GSD_W2D_X4", "GSD_W2D_U4", "GSD_WGRAD_W2D"]:
        monkeypatch.delenv(k, raising=False)


def one_stream(case):
    return S.Case(case.name + "/one-stream", case.precision, case.dims, case.n, case.h, case.w, dict(case.env, **ONE_STREAM[case.precision]),
                  case.n_classes)


def step_ms(case):
    """One unperturbed step of the case's one-stream schedule between two events (the second of three: everything is sized and
    warm); its results are the train_steps reference."""
    if case.name not in _STEP_MS:
        marks = []

        def mark(model, step, i):
            marks.append(torch.cuda.current_stream().record_event(torch.cuda.Event(enable_timing=True)))

        ref, eng = S.CONSUMING["train_steps"](one_stream(case), hook=mark)
        assert eng.side is None, "the reference runs on one stream"
        _REFERENCE[case.name, "train_steps"] = ref
        _STEP_MS[case.name] = marks[1].elapsed_time(marks[2])
    return _STEP_MS[case.name]


def reference(case, workload):
    step_ms(case)
    if (case.name, workload) not in _REFERENCE:
        ref, eng = S.CONSUMING[workload](one_stream(case))
        assert eng.side is None, "the reference runs on one stream"
        _REFERENCE[case.name, workload] = ref
    return _REFERENCE[case.name, workload]


def forks_per_run(monkeypatch, case, workload, ref):
    """The two-stream schedule under the count-only policy: how many forks a perturbed run will delay -- and, since nothing is
    perturbed, the undisturbed comparison of the older tests over again."""
    if (case.name, workload) not in _FORKS:
        with D.delays(monkeypatch, D.NONE, D.MIN_MS) as d:
            res, eng = S.CONSUMING[workload](case)
        assert d.total_delayed() == 0
        S.same_results(ref, res, f"{case.name} {workload}: one stream against two, undisturbed")
        _FORKS[case.name, workload] = d.total_forks()
    return _FORKS[case.name, workload]


def prepare(monkeypatch, case, workload):
    """(reference, delay, forks per run) of one case and workload, all from unperturbed and unmutated runs: a mutation test calls
    this in front of its patches."""
    ref = reference(case, workload)
    return ref, D.delay_for(step_ms(case)), forks_per_run(monkeypatch, case, workload, ref)


def stimulus(case, what, policy, ms, d, eng, attempts):
    return (f"{case.name:<24}{what:<18}{policy:<10} step {step_ms(case):6.3f} ms  delay {ms:6.3f} ms  forks delayed: side "
            f"{d.delayed_of(eng.side):3d}, hand-off {d.delayed_of(eng._handoff):3d}  models made: {attempts}")


def on_queues_of_their_own(main, eng, handoff=False):
    """The engine's side stream can run while the main stream is busy -- and, for the hand-off tests, the hand-off stream while the
    side stream is."""
    if eng.side is None:
        return True
    return D.independent(main, eng.side) and (not handoff or D.independent(eng.side, eng._handoff))


def perturbed(monkeypatch, case, workload, policy, capsys=None):
    """(reference, results under the policy, engine, the context's counters) of one case and workload."""
    ref, ms, forks = prepare(monkeypatch, case, workload)
    assert forks * ms < D.BUDGET_MS, f"{case.name} {workload}: {forks} forks of {ms:.2f} ms: too large a case for this test"
    for attempt in range(1, ATTEMPTS + 1):
        with D.delays(monkeypatch, policy, ms) as d:
            res, eng = S.CONSUMING[workload](case)
        if on_queues_of_their_own(d.main, eng):
            break
    else:
        raise AssertionError(f"{ATTEMPTS} models in a row drew a side stream that shares the main stream's hardware queue")
    if capsys is not None:
        with capsys.disabled():
            print("\n" + stimulus(case, workload, policy, ms, d, eng, attempt))
    return ref, res, eng, d


# ------------------------------------------------------------------------------------------- 1. whichever stream runs late
@pytest.mark.parametrize("policy", PERTURBED)
@pytest.mark.parametrize("workload", list(S.CONSUMING))
@pytest.mark.parametrize("name", TWO_STREAM + CONTROL)
def test_results_do_not_depend_on_which_stream_is_late(monkeypatch, capsys, name, workload, policy):
    case = BY_NAME[name]
    ref, res, eng, d = perturbed(monkeypatch, case, workload, policy, capsys)
    if name in CONTROL:
        assert eng.side is None and d.total_forks() == 0 and d.total_delayed() == 0, d.summary()
    else:
        assert eng.side is not None and d.delayed_of(eng.side) >= 1, d.summary()
        assert d.delayed_of(eng.side) == d.forks_of(eng.side) and d.captured == 0, d.summary()
        assert d.slept_on(eng.side if policy == D.SIDE_LATE else d.main) >= d.delayed_of(eng.side), d.summary()
    S.same_results(ref, res, f"{name} {workload}: one stream against two under {policy}")


# ------------------------------------------------------------------------------------------- 2. the hand-off stream's contract
def handoff_step(case):
    """One forward / backward of the engine itself with a block_done_cb that copies the announced block's range of the gradient
    arena into a snapshot arena, on the device, under whatever stream is current in the callback.  Returns the final arena
    (cloned on the main stream right behind backward), the snapshot arena, the buckets and the tags in the order announced."""
    from gelslim_depth_amd.distributed import make_buckets
    from gelslim_depth_amd.train import TrainStep
    with S.environ(case.env):
        m = S.make_model(case.precision, case.dims, case.n_classes)
        step = TrainStep(m)        # (for its flat gradient arena and the views into it; no step of its own is taken)
        x, t = S.make_batch(case.n, case.h, case.w, n_classes=case.n_classes)
        eng = m._engine
        buckets = make_buckets([n for n, _ in m.named_parameters()], step.offsets, eng.L)
        ranges = {tag: (lo, hi) for tag, lo, hi in buckets}
        snapshot = torch.zeros_like(step.g_flat)
        announced, seen_under = [], []

        def block_done(tag):
            lo, hi = ranges[tag]
            snapshot[lo:hi].copy_(step.g_flat[lo:hi])
            announced.append(tag)
            seen_under.append(torch.cuda.current_stream().cuda_stream)

        P = m._tensor_map()
        out = eng.forward(x, P, train=True)
        eng.block_done_cb = block_done
        try:
            assert t.shape == out.shape
            eng.backward(t, P, m._grad_views)        # (the target as dL/dout: any fixed tensor of that shape serves)
        finally:
            eng.block_done_cb = None
        final = step.g_flat.clone()
        torch.cuda.synchronize()
        return S.snap(final), S.snap(snapshot), buckets, announced, seen_under, eng


def check_handoff(final, snapshot, buckets, announced, what):
    assert sorted(announced) == sorted(tag for tag, _, _ in buckets), f"{what}: announced {announced}"
    covered = 0
    for tag, lo, hi in buckets:
        S.same_bits(snapshot[lo:hi], final[lo:hi], f"{what}: block {tag} as its callback saw it against the final arena")
        covered += hi - lo
    assert covered == final.numel(), "the buckets cover the arena"


def handoff_reference(case):
    if (case.name, "handoff") not in _REFERENCE:
        final, snapshot, buckets, announced, _, eng = handoff_step(one_stream(case))
        assert eng.side is None
        check_handoff(final, snapshot, buckets, announced, f"{case.name}: one stream")
        _REFERENCE[case.name, "handoff"] = final
    return _REFERENCE[case.name, "handoff"]


def handoff_delay(case):
    return D.delay_for(step_ms(case))


def perturbed_handoff(monkeypatch, case, policy, ms):
    """handoff_step under the policy, with a model whose three streams can be late for one another."""
    for attempt in range(1, ATTEMPTS + 1):
        with D.delays(monkeypatch, policy, ms) as d:
            run = handoff_step(case)
        if on_queues_of_their_own(d.main, run[-1], handoff=True):
            return run, d, attempt
    raise AssertionError(f"{ATTEMPTS} models in a row drew side and hand-off streams that share a hardware queue")


@pytest.mark.parametrize("policy", PERTURBED)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_hand_off_callback_sees_final_gradients(monkeypatch, capsys, precision, policy):
    """The contract of engine_base._announce: the callback runs under a stream that has waited for the main and the side stream,
    so the block it is told about is final whichever of them is late."""
    case = BY_NAME[FIRST[precision]]
    ref = handoff_reference(case)
    ms = handoff_delay(case)
    (final, snapshot, buckets, announced, seen_under, eng), d, attempts = perturbed_handoff(monkeypatch, case, policy, ms)
    with capsys.disabled():
        print("\n" + stimulus(case, "hand-off", policy, ms, d, eng, attempts))
    assert eng.side is not None and eng._handoff is not None
    assert set(seen_under) == {eng._handoff.cuda_stream}, "every callback ran under the hand-off stream"
    assert d.delayed_of(eng.side) >= 1 and d.delayed_of(eng._handoff) == len(buckets), d.summary()
    check_handoff(final, snapshot, buckets, announced, f"{case.name} under {policy}")
    S.same_bits(final, ref, f"{case.name} under {policy}: the gradient arena against the one-stream schedule's")


# ------------------------------------------------------------------------------------------- 3. under a caller's stream
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_step_under_a_callers_stream(capsys, precision):
    """Model, batch, TrainStep and three steps under a stream of the caller's, which a sleep in front of every step keeps late:
    whatever the package issued on the default stream instead would run ahead of what it depends on."""
    case = BY_NAME[FIRST[precision]]
    ref = reference(case, "train_steps")
    ms = D.delay_for(step_ms(case))
    for _ in range(ATTEMPTS):       # a stream that shares the default stream's queue could not run behind it
        s = torch.cuda.Stream()
        if D.independent(torch.cuda.current_stream(), s):
            break
    else:
        raise AssertionError(f"{ATTEMPTS} streams in a row share the default stream's hardware queue")
    slept = []

    def late(model, step, i):
        assert torch.cuda.current_stream().cuda_stream == s.cuda_stream
        D.sleep_ms(s, ms)
        slept.append(i)

    with torch.cuda.stream(s):
        res, eng = S.CONSUMING["train_steps"](case, hook=late)
    with capsys.disabled():
        print(f"\n{case.name:<24}{'caller stream':<18}{'':<10} step {step_ms(case):6.3f} ms  delay {ms:6.3f} ms  in front of {len(slept)} steps")
    assert slept == [0, 1, 2] and eng.side is not None and eng.side.cuda_stream != s.cuda_stream
    S.same_results(ref, res, f"{case.name}: the default stream, one-stream schedule, against a caller's stream kept late")


# ------------------------------------------------------------------------------------------- proof that the instrument can see
def differing(ref, res):
    """Names whose bits differ (shapes and names are the same: the mutations change no launch)."""
    assert sorted(ref) == sorted(res)
    out = []
    for k in ref:
        try:
            S.same_bits(ref[k], res[k], k, finite=False)
        except AssertionError:
            out.append(k)
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_m1_a_missing_join_is_rejected(monkeypatch, precision):
    """M1: engine_base._join_side does nothing, so the optimiser and the clones read weight gradients that the late side stream
    has not written yet (the arena's zeros in the first step, the step before's values afterwards)."""
    from gelslim_depth_amd import engine_base
    case = BY_NAME[FIRST[precision]]
    prepare(monkeypatch, case, "train_steps")
    monkeypatch.setattr(engine_base.EngineBase, "_join_side", lambda self: None)
    ref, res, eng, d = perturbed(monkeypatch, case, "train_steps", D.SIDE_LATE)
    torch.cuda.synchronize()
    assert d.delayed_of(eng.side) >= 1
    diff = differing(ref, res)
    assert "g_flat" in diff and "p_flat" in diff, diff
    with pytest.raises(AssertionError, match="g_flat"):
        S.same_results({"g_flat": ref["g_flat"]}, {"g_flat": res["g_flat"]}, "M1")


def test_m2_unguarded_scratch_buffers_are_rejected(monkeypatch):
    """M2: the engine's own Stream.wait_event calls do nothing (wait_stream, which torch builds on wait_event, keeps working), so
    the BatchNorm backward of a unit rewrites gps[turn] while the delayed dW launch of the unit two before still reads it.  Both
    are views of one allocation that lives as long as the engine."""
    case = BY_NAME["fp32-default"]
    prepare(monkeypatch, case, "autograd_step")
    real_wait_event = torch.cuda.Stream.wait_event
    ignored = []
    monkeypatch.setattr(torch.cuda.Stream, "wait_stream", lambda self, stream: real_wait_event(self, stream.record_event()))
    monkeypatch.setattr(torch.cuda.Stream, "wait_event", lambda self, event: ignored.append(event))
    ref, res, eng, d = perturbed(monkeypatch, case, "autograd_step", D.SIDE_LATE)
    torch.cuda.synchronize()
    order = [u for pair in reversed(eng.dec) for u in reversed(pair)] + [u for pair in reversed(eng.enc) for u in reversed(pair)]
    run = best = 0
    for u in order:            # the order of backward
        run = run + 1 if u.plan.pitched and not u.plan.fused_dw else 0
        best = max(best, run)
    assert best >= 3 and len(eng.gps) == 2, f"{best} consecutive pitched units: the scratch buffers are never contended"
    assert len(ignored) >= best - 2, "the engine asked for no event at all"
    diff = differing(ref, res)
    wnames = {"grad." + u.wname for u in order if u.plan.pitched}
    assert wnames & set(diff), f"no pitched unit's weight gradient differs: {diff}"


def test_m3_a_hand_off_that_skips_the_side_stream_is_rejected(monkeypatch):
    """M3: _announce's second wait_stream (hand-off stream on side stream) is dropped, so a callback copies a block whose weight
    gradients the late side stream has not written yet."""
    from gelslim_depth_amd import engine_base
    case = BY_NAME["fp32-default"]
    ref = handoff_reference(case)
    ms = handoff_delay(case)
    real_announce, real_wait_stream = engine_base.EngineBase._announce, torch.cuda.Stream.wait_stream
    state = {"drop": None, "dropped": 0}

    def announce(self, tag):
        state["drop"] = self.side.cuda_stream
        try:
            real_announce(self, tag)
        finally:
            state["drop"] = None

    def wait_stream(self, stream):
        if state["drop"] is not None and stream.cuda_stream == state["drop"]:
            state["dropped"] += 1
            return
        real_wait_stream(self, stream)

    monkeypatch.setattr(engine_base.EngineBase, "_announce", announce)
    monkeypatch.setattr(torch.cuda.Stream, "wait_stream", wait_stream)
    (final, snapshot, buckets, announced, _, eng), d, _ = perturbed_handoff(monkeypatch, case, D.SIDE_LATE, ms)
    torch.cuda.synchronize()
    assert state["dropped"] >= len(buckets) and d.delayed_of(eng.side) >= 1
    S.same_bits(final, ref, "M3 leaves the step itself alone")      # (the join at the end of backward still holds)
    with pytest.raises(AssertionError, match="differ in their bits"):
        check_handoff(final, snapshot, buckets, announced, "M3")

