"""Results do not depend on what ran before.

Both engines keep exactly one shape: any other batch size, image size or mode drops and re-makes their buffers, from memory
the previous shape has just given back.  A long-lived model walks through what harness.fit does in an epoch -- eval, train,
a ragged last batch, validation at other batch sizes, another image size, a skipped step -- with every torch.empty buffer
handed out holding +3.0e4 (engine_state.poisoned), and every call's results must be the bits a FRESH model, loaded with the
state taken in front of that call and given zeroed buffers, computes for that call alone.  Afterwards everything the engines'
contract says nothing writes must still hold 0.

GraphedInference holds raw pointers into the engine's buffers: it must refuse to replay once `engine.buffers_made` has moved
(no test here replays such a graph: the refusal is the behaviour under test).
"""
import copy

import pytest
import torch

import engine_state as S

pytestmark = pytest.mark.gpu

DIMS = {"fp32": [16, 32, 64], "bf16": [32, 64, 128]}
# (precision, switches): the fp32 engine also under the forced act-once plan of test_engine_act_once_equals_deferred, where the
# concat buffers and the pitched pooled tensors exist -- by default the plan declines them at these sizes
FORCED = {"GSD_CONV_W2D": "1", "GSD_ACT_ONCE_FORCE": "1"}
# ... and with BatchNorm's sums and finalize as separate launches (the form of full-size layers and of SyncBN): they stage through
# u.sums, which the engine keeps across shapes
CONFIGS = [("fp32", {}), ("fp32", FORCED), ("fp32", {"GSD_BN_ONE_LAUNCH_ROWS": "0"}), ("bf16", {})]
CONFIG_IDS = ["fp32", "fp32-w2d-forced", "fp32-bn-three-launch", "bf16"]
A, A_RAGGED, V, V1, B = (3, 40, 53), (2, 40, 53), (5, 40, 53), (1, 37, 45), (3, 37, 45)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("GSD_ACT_ONCE", "GSD_ACT_ONCE_FORCE", "GSD_CONV_W2D", "GSD_W2D_X4", "GSD_W2D_U4", "GSD_W2D_SPLIT", "GSD_W43_SPLIT",
              "GSD_WGRAD_W2D", "GSD_SIDE_DW", "GSD_WGRAD_FIRST", "GSD_BN_ONE_LAUNCH_ROWS", "GSD_BF16_FIRST", "GSD_BF16_SIDE_DW", "GSD_BF16_APPLY_POOL",
              "GSD_BF16_C64", "GSD_BF16_FUSED_OUT", "GSD_BF16_FUSED_INC"):
        monkeypatch.delenv(k, raising=False)


def _batch(shape, seed):
    return S.make_batch(*shape, seed=seed)


# ------------------------------------------------------------------------------------------------------- TrainStep sequence
def _new_step(precision):
    from gelslim_depth_amd.train import TrainStep
    m = S.make_model(precision, DIMS[precision])
    return TrainStep(m, nan_policy="skip", max_grad_norm=0.05)


def _train(shape, seed, poison_target=False):
    def call(step):
        x, t = _batch(shape, seed)
        if poison_target:
            t[1, 0, 7, 11] = float("inf")
        loss = step(x, t)
        res = {"loss": S.snap(loss), "out": S.snap(step._out), "grad_norm": S.snap(step.last_grad_norm)}
        res.update(S.step_state(step))
        return res
    return call


def _evaluate(shape, seed):
    def call(step):
        x, _ = _batch(shape, seed)
        res = {"out": S.snap(step.evaluate(x))}
        res.update(S.step_state(step))
        return res
    return call


STEP_SEQUENCE = [
    ("1 eval forward at A", _evaluate(A, 11)),
    ("2 train step at A (eval then train, same key)", _train(A, 12)),
    ("3 train step at A', the ragged last batch", _train(A_RAGGED, 13)),
    ("4 evaluate at V", _evaluate(V, 14)),
    ("5 evaluate at N = 1, 37 x 45", _evaluate(V1, 15)),
    ("6 train step at A, everything re-made", _train(A, 16)),
    ("7 train step at B", _train(B, 17)),
    ("8 skipped step at A (one inf in the target)", _train(A, 18, poison_target=True)),
    ("9 train step at A", _train(A, 19)),
]
# The loss of the skipped step is the mean over a target that holds an inf, and the norm of its gradient is not finite either:
# that is what makes the guard skip it.  Their bits are still compared; everything the step leaves in the model is finite.
NOT_FINITE = {"8 skipped step at A (one inf in the target)": ("loss", "grad_norm")}


@pytest.mark.parametrize("precision,env", CONFIGS, ids=CONFIG_IDS)
def test_train_step_results_do_not_depend_on_what_ran_before(monkeypatch, precision, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with S.poison(monkeypatch, S.BIG):
        live = _new_step(precision)
    skipped = []
    for name, call in STEP_SEQUENCE:
        state = copy.deepcopy(live.state_dict())        # host tensors: parameters, BatchNorm buffers and counters, moments, EMA, guard
        with S.poison(monkeypatch, S.BIG):
            got = call(live)
        with S.poison(monkeypatch, S.ZERO):
            fresh = _new_step(precision)
            fresh.load_state_dict(state)
            want = call(fresh)
        S.same_results(got, want, f"{precision}, call {name}: the long-lived model against a fresh one",
                       not_finite=NOT_FINITE.get(name, ()))
        skipped.append(got["skipped_steps"])
    assert skipped == [0] * 7 + [1, 1], f"exactly call 8 is skipped: {skipped}"
    eng = live.model._engine
    assert eng.buffers_made >= 7, "the sequence re-made the buffers at every change of shape"
    assert precision == "bf16" or (eng.one_launch_rows == 0) == ("GSD_BN_ONE_LAUNCH_ROWS" in env)
    assert S.assert_pads_zero(eng) > 0
    if env == FORCED:
        assert any(up.plan.cat_on for up in eng.ups) and any(eng.plan.pooled_pitched), "the forced plan: concat buffers and pitched pooled tensors"


# --------------------------------------------------------------------------------------------------------- autograd sequence
def _fwd_bwd(model, shape, seed, input_grad):
    x, t = _batch(shape, seed)
    x.requires_grad_(input_grad)
    for p in model.parameters():
        p.grad = None
    out = model(x)
    (out * t).sum().backward()
    res = {"out": S.snap(out)}
    res.update({"grad." + k: S.snap(p.grad) for k, p in model.named_parameters()})
    if input_grad:
        res["x.grad"] = S.snap(x.grad)
    res.update(S.buffers_of(model))
    return res


def _eval(model, shape, seed):
    x, _ = _batch(shape, seed)
    model.eval()
    with torch.no_grad():
        res = {"out": S.snap(model(x=x))}
    model.train()
    res.update(S.buffers_of(model))
    return res


def _forward_then_step(model, input_grad):
    x, _ = _batch(A, 24)
    dropped = model(x)                   # a train-mode forward nobody back-propagates: it still updates the running statistics
    res = _fwd_bwd(model, A_RAGGED, 25, False)
    res["dropped.out"] = S.snap(dropped)
    return res


AUTOGRAD_SEQUENCE = [
    ("1 train forward + backward at A", lambda m, ig: _fwd_bwd(m, A, 21, False)),
    ("2 eval forward under no_grad at V", lambda m, ig: _eval(m, V, 22)),
    ("3 train forward + backward at A with the input's gradient", lambda m, ig: _fwd_bwd(m, A, 23, ig)),
    ("4 a train forward without backward, then forward + backward at A'", _forward_then_step),
    ("5 eval forward at A", lambda m, ig: _eval(m, A, 26)),
]


@pytest.mark.parametrize("precision,env", CONFIGS, ids=CONFIG_IDS)
def test_autograd_results_do_not_depend_on_what_ran_before(monkeypatch, precision, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    input_grad = precision == "fp32"              # (the bf16 engine has no input gradient)
    with S.poison(monkeypatch, S.BIG):
        live = S.make_model(precision, DIMS[precision])
    for name, call in AUTOGRAD_SEQUENCE:
        state = {k: S.snap(v) for k, v in live.state_dict().items()}
        with S.poison(monkeypatch, S.BIG):
            got = call(live, input_grad)
        with S.poison(monkeypatch, S.ZERO):
            fresh = S.make_model(precision, DIMS[precision], seed=9)
            fresh.load_state_dict(state, strict=True)
            want = call(fresh, input_grad)
        S.same_results(got, want, f"{precision}, call {name}: the long-lived model against a fresh one")
    assert S.assert_pads_zero(live._engine) > 0
    if env == FORCED:     # (the last train-mode shape was A')
        assert any(up.cat is not None for up in live._engine.ups), "the forced plan: concat buffers"


# ---------------------------------------------------------------------------------------------------------- GraphedInference
def _eager(model, x):
    was = model.training
    model.eval()
    with torch.no_grad():
        y = model(x=x).clone()
    model.train(was)
    return y


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_inference_refuses_stale_engine_buffers(precision):
    from gelslim_depth_amd._lib import GsdError
    from gelslim_depth_amd.graph import GraphedInference
    m = S.make_model(precision, DIMS[precision], train=False)
    eng = m._engine
    x, _ = _batch((2, 40, 53), 31)
    x2, _ = _batch((2, 40, 53), 32)
    fn = GraphedInference(m, x)
    made = eng.buffers_made
    assert made == 1
    S.same_bits(fn(x2), _eager(m, x2), "replay against eager")
    assert eng.buffers_made == made, "an eager eval forward at the captured shape keeps the buffers"
    S.same_bits(fn(x), _eager(m, x), "replay after an eager forward at the same shape")
    other, _ = _batch((3, 40, 53), 33)
    _eager(m, other)
    assert eng.buffers_made == made + 1
    before = fn.y.clone()
    with pytest.raises(GsdError, match="build a new GraphedInference"):
        fn(x2)
    assert torch.equal(fn.x, x) and torch.equal(fn.y, before), "refused before the input is copied or anything replays"
    _eager(m, x)                    # back at the captured shape: the buffers are new ones all the same
    with pytest.raises(GsdError, match="build a new GraphedInference"):
        fn(x)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_inference_survives_train_steps_once_the_buffers_are_the_train_mode_ones(precision):
    from gelslim_depth_amd._lib import GsdError
    from gelslim_depth_amd.graph import GraphedInference
    from gelslim_depth_amd.train import TrainStep
    m = S.make_model(precision, DIMS[precision])
    eng = m._engine
    step = TrainStep(m)
    x, t = _batch((2, 40, 53), 41)
    xv, _ = _batch((2, 40, 53), 42)
    # captured in front of the first train step: that step re-makes the buffers and the graph must refuse
    m.eval()
    early = GraphedInference(m, xv)
    m.train()
    made = eng.buffers_made
    step(x, t)
    assert eng.buffers_made == made + 1, "the first train-mode forward at the captured shape re-made the buffers"
    with pytest.raises(GsdError, match="build a new GraphedInference"):
        early(xv)
    # captured behind it: valid across further steps at that shape
    m.eval()
    fn = GraphedInference(m, xv)
    m.train()
    made = eng.buffers_made
    for i in range(3):
        step(x, t)
        assert eng.buffers_made == made
        S.same_bits(fn(xv), _eager(m, xv), f"replay against eager after train step {i + 2}")
    ragged, tr = _batch((1, 40, 53), 43)
    step(ragged, tr)
    assert eng.buffers_made == made + 1
    with pytest.raises(GsdError, match="build a new GraphedInference"):
        fn(xv)
