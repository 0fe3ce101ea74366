"""CPU: the host side of gradient-norm clipping and learning-rate schedules -- the argument checks of gsd_grad_norm and
gsd_adam_ema_clip (made before any launch, so they run without a device), the workspace query, the schedule formula at
hand-computed points and the LRSchedule value class."""
import ctypes
import math

import pytest

BAD_ARG, WORKSPACE = -1, -4
ARENA = 31037633        # the full network's parameter count


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from gelslim_depth_amd import _lib
    return _lib


def _guard(L, words, tick):
    g = L.gsd_guard()
    g.words, g.tick = words, tick
    return ctypes.pointer(g)


P = 0x1000          # a non-null, 16-byte aligned address: every call below must return before it is ever touched


def test_grad_norm_workspace_query(L):
    sizes = [L.lib.gsd_grad_norm_workspace(n) for n in (1, 256, 10 ** 6, ARENA)]
    assert sizes[0] >= 1 and sizes == sorted(sizes), sizes
    assert sizes[-1] <= 1 << 16, "a second stage of one block reads them all"
    assert L.lib.gsd_grad_norm_workspace(ARENA) == L.lib.gsd_grad_norm_workspace(ARENA), "a function of numel alone"


def test_grad_norm_refuses_bad_arguments_before_any_launch(L):
    f = L.lib.gsd_grad_norm
    ws = L.lib.gsd_grad_norm_workspace(4097)
    assert f(None, 4097, 1.0, 1.0, P, P, ws, None, None) == BAD_ARG
    assert f(P, 4097, 1.0, 1.0, None, P, ws, None, None) == BAD_ARG
    assert f(P, 4097, 1.0, 1.0, P, None, ws, None, None) == BAD_ARG
    assert f(P, 0, 1.0, 1.0, P, P, ws, None, None) == BAD_ARG
    assert f(P, -5, 1.0, 1.0, P, P, ws, None, None) == BAD_ARG
    for bad in (0.0, -1.0, math.nan):
        assert f(P, 4097, 1.0, bad, P, P, ws, None, None) == BAD_ARG, bad
        assert "max_norm" in L.lib.gsd_last_error().decode()
    assert f(P, 4097, 1.0, 1.0, P, P, ws, _guard(L, P, 0), None) == BAD_ARG, "a guard with tick 0"
    assert f(P, 4097, 1.0, 1.0, P, P, ws, _guard(L, None, 3), None) == BAD_ARG, "a guard without words"
    assert f(P, 4097, 1.0, 1.0, P, P, ws - 1, None, None) == WORKSPACE
    assert f(P, 4097, 1.0, math.inf, P, P, 0, None, None) == WORKSPACE, "max_norm = +inf is legal: the next check answers"
    assert f(P, ARENA, 1.0, 1.0, P, P, L.lib.gsd_grad_norm_workspace(ARENA) - 1, None, None) == WORKSPACE


def test_adam_ema_clip_refuses_bad_arguments_before_any_launch(L):
    f = L.lib.gsd_adam_ema_clip
    tail = (100, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.995, 1.0)

    def call(p=P, g=P, m=P, v=P, ema=P, numel=100, step=1, clip=P, guard=None):
        return f(p, g, m, v, ema, numel, step, *tail[2:], clip, guard, None)
    for name in ("p", "g", "m", "v", "clip"):
        assert call(**{name: None}) == BAD_ARG, name
    assert call(numel=0) == BAD_ARG and call(numel=-1) == BAD_ARG and call(step=0) == BAD_ARG
    assert call(guard=_guard(L, P, 0)) == BAD_ARG and call(guard=_guard(L, None, 2)) == BAD_ARG


# ----------------------------------------------------------------------------------------------------- the schedule formula
def test_lr_at_matches_hand_computed_points():
    from gelslim_depth_amd.train import LRSchedule, lr_at
    lr, lo = 1e-3, 1e-5
    s = LRSchedule(warmup_steps=4, decay="cosine", total_steps=12, min_lr=lo)
    # warm = min(1, t/4); q = clamp((t-4)/8, 0, 1); base = lo + (lr-lo)(1+cos(pi q))/2
    want = {1: 0.25 * lr,                                             # q = 0 (clamped): base = lr
            2: 0.5 * lr,
            4: lr,                                                    # warm-up over, q = 0
            5: lo + (lr - lo) * 0.5 * (1.0 + math.cos(math.pi / 8)),  # q = 1/8
            8: lo + (lr - lo) * 0.5,                                  # q = 1/2: cos = 0 up to 6e-17
            12: lo,                                                   # q = 1
            13: lo, 100: lo}                                          # held behind total_steps
    for t, w in want.items():
        assert lr_at(lr, s, t) == pytest.approx(w, rel=1e-15, abs=0.0), t
    assert lr_at(lr, s, 1) == 0.25 * lr and lr_at(lr, s, 4) == lr and lr_at(lr, s, 12) == lo and lr_at(lr, s, 100) == lo
    assert lr_at(lr, s, 5) == pytest.approx(9.62320369e-4, rel=1e-8)           # by hand: cos(pi/8) = 0.9238795325
    lin = LRSchedule(warmup_steps=2, decay="linear", total_steps=10, min_lr=1e-4)
    assert lr_at(lr, lin, 1) == 0.5 * lr and lr_at(lr, lin, 2) == lr
    assert lr_at(lr, lin, 6) == pytest.approx(1e-4 + 9e-4 * 0.5, rel=1e-15)
    assert lr_at(lr, lin, 10) == 1e-4 and lr_at(lr, lin, 11) == 1e-4
    rates = [lr_at(lr, s, t) for t in range(1, 14)]
    assert rates[:4] == sorted(rates[:4]) and rates[3:] == sorted(rates[3:], reverse=True)


def test_lr_at_constant_returns_lr_exactly():
    from gelslim_depth_amd.train import LRSchedule, lr_at
    for lr in (1e-3, 0.1, 3.3e-4):
        assert lr_at(lr, None, 7) == lr
        for t in (1, 2, 1000, 10 ** 9):
            assert lr_at(lr, LRSchedule(), t) == lr
            assert lr_at(lr, LRSchedule(decay="constant", total_steps=5), t) == lr
        warm = LRSchedule(warmup_steps=10)
        assert lr_at(lr, warm, 5) == 0.5 * lr and lr_at(lr, warm, 10) == lr and lr_at(lr, warm, 11) == lr


# ------------------------------------------------------------------------------------------------------------ LRSchedule
def test_lr_schedule_is_a_validated_value_class():
    from gelslim_depth_amd.train import LRSchedule
    a = LRSchedule(warmup_steps=3, decay="cosine", total_steps=8, min_lr=1e-5)
    spec = a.spec()
    assert spec == {"warmup_steps": 3, "decay": "cosine", "total_steps": 8, "min_lr": 1e-5}
    assert all(v is None or type(v) in (int, float, str) for v in spec.values())
    assert all(v is None or type(v) in (int, float, str) for v in LRSchedule().spec().values())
    assert LRSchedule(**spec) == a and hash(LRSchedule(**spec)) == hash(a) and LRSchedule(**LRSchedule().spec()) == LRSchedule()
    assert a != LRSchedule(warmup_steps=3, decay="cosine", total_steps=9, min_lr=1e-5) and a != spec
    assert "cosine" in repr(a)
    for kw, field in ((dict(warmup_steps=-1), "warmup_steps"), (dict(warmup_steps=1.5), "warmup_steps"),
                      (dict(decay="exp"), "decay"), (dict(decay="linear"), "total_steps"),
                      (dict(decay="cosine", warmup_steps=5, total_steps=5), "total_steps"),
                      (dict(total_steps=0), "total_steps"), (dict(total_steps=2.0), "total_steps"),
                      (dict(min_lr=-1e-3), "min_lr"), (dict(min_lr=math.nan), "min_lr"), (dict(min_lr=math.inf), "min_lr"),
                      (dict(min_lr="x"), "min_lr")):
        with pytest.raises(ValueError, match=field):
            LRSchedule(**kw)


def test_state_keys_name_both_controls():
    from gelslim_depth_amd import train
    assert "max_grad_norm" in train.STATE_HPARAMS and "lr_schedule" in train.STATE_HPARAMS
    assert train.STATE_VERSION == 2
