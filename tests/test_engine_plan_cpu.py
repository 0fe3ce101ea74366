"""engine_plan.plan_step on the CPU: what a step of the fp32 engine launches is a value, computed without a device.

engine_plan_parent.json (beside this file) is what UNetEngine._ensure of the commit before engine_plan.py existed decided, recorded
on a machine without a GPU: that commit's engine was constructed per case under the case's switches and _ensure(n, h, w,
torch.device("meta"), train) run for train and for eval, with _lib._chk_f32 and torch.cuda.Stream stubbed out (nothing else of it
touches a device).  Per unit, up and level the table holds the attributes that _ensure and _plan_act_once left (forms_f, form_d,
pitched, fused_dw, act_once, mode_d, bn_rows, cat_on, pooled_pitched), the numel of every weight image and scratch buffer it
allocated in either mode, the row counts and workspaces that forward / backward asked the library for at launch
(partial_rows, gsd_bn_bwd_partial_rows, the workspace queries), the `fused=` value backward passed to _bn_bwd_tail with the rows
it then read, and that commit's _dw_form for the operand layout each unit's dW is handed in a train step.  The cases: the fp32
table of test_gpu_engine_memory.py, the 5-level network at 3 x 320 x 427 and batches 1, 8, 16, 32, 64, that network with two
classes, and a one-level network."""
import dataclasses
import glob
import json
import os
import re

import pytest

from gelslim_depth_amd import engine_plan as EP
from gelslim_depth_amd.engine import UNetEngine

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "engine_plan_parent.json")) as _f:
    PARENT = json.load(_f)
FLAGSHIP = [64, 128, 256, 512, 1024]
CSRC = os.path.join(os.path.dirname(os.path.abspath(EP.__file__)), "csrc")


def _switches():
    """Every GSD_* environment name the fp32 library sources (and the planner itself) read."""
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) + [EP.__file__]:
        with open(path, errors="replace") as f:
            names |= set(re.findall(r'"(GSD_[A-Z0-9_]+)"', f.read()))
    return sorted(n for n in names if "BF16" not in n)


SWITCHES = _switches()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def plan_of(case):
    p = case["plan"]
    return EP.plan_step(3, case["n_classes"], case["dims"], p["n"], p["h"], p["w"])


@pytest.fixture(params=PARENT, ids=[c["name"] for c in PARENT])
def case_plan(request, monkeypatch):
    for k, v in request.param["env"].items():
        monkeypatch.setenv(k, v)
    return request.param, plan_of(request.param)


def test_table_covers_the_cases():
    import test_gpu_engine_memory as M
    names = {c["name"]: c for c in PARENT}
    for c in M.FP32_CASES:
        t = names[c.name]
        assert (t["dims"], t["plan"]["n"], t["plan"]["h"], t["plan"]["w"], t["env"], t["n_classes"]) == (c.dims, c.n, c.h, c.w, c.env, c.n_classes)
    for b in (1, 8, 16, 32, 64):
        t = names[f"flagship-b{b}"]
        assert (t["dims"], t["plan"]["n"], t["plan"]["h"], t["plan"]["w"], t["n_classes"]) == (FLAGSHIP, b, 320, 427, 1)
    assert names["flagship-b32-two-classes"]["n_classes"] == 2 and names["one-level"]["dims"] == [16]


def test_plan_equals_parent(case_plan):
    case, plan = case_plan
    got = json.loads(json.dumps(dataclasses.asdict(plan)))      # (tuples as lists, as the table holds them)
    want = case["plan"]
    assert sorted(got) == sorted(want)
    for key in ("units", "ups"):
        assert len(got[key]) == len(want[key])
        for i, (a, b) in enumerate(zip(got[key], want[key])):
            assert sorted(a) == sorted(b)
            for f in a:
                assert a[f] == b[f], f"{case['name']}: {key}[{i}].{f} is {a[f]}, the parent had {b[f]}"
    assert got == want


def test_buffer_sizes_are_the_maxima_of_the_plans_launches(case_plan):
    case, p = case_plan
    r64, r4 = (lambda c: (c + 63) // 64 * 64), (lambda w: (w + 3) // 4 * 4)
    k, c0 = case["n_classes"], case["dims"][0]
    fwd_dx = [max(f.partial_rows for f in u.fwd) * 2 * r64(u.cout) for u in p.units] + \
        [u.dgrad.partial_rows * 2 * r64(u.cin) for u in p.units if u.dgrad is not None]
    ev, tr = p.sizes
    assert dataclasses.astuple(ev) == (max(fwd_dx + [1]), 0, 0, 0, 0, 0, 0, 0, 0), "an eval-only engine: partials alone"
    assert tr.partials == max(fwd_dx + [1] + [u.bn_bwd_rows * 3 * u.cout for u in p.units] + [up.bn_rows * 2 * r64(up.cin) for up in p.ups])
    assert tr.conv_ws == max([u.fwd[True].workspace for u in p.units] + [u.dgrad.workspace for u in p.units if u.dgrad is not None])
    assert all(u.fwd[False].workspace == 0 for u in p.units), "an eval-mode launch gets no K slabs"
    assert tr.gp == max([p.n * u.cout * p.hs[u.level] * r4(p.ws[u.level]) for u in p.units if u.pitched] + [0])
    assert tr.act_buf == max([p.n * u.cin * p.hs[u.level] * r4(p.ws[u.level]) for u in p.units if u.act_once] + [0])
    ws = max([1] + [u.wgrad_workspace for u in p.units] + [u.wgrad_bn_workspace for u in p.units] + [up.wgrad_workspace for up in p.ups])
    assert (tr.wgrad_ws, tr.wgrad_ws_side) == (max(ws, 64 * k), max(ws, 64))
    assert tr.db_sums == 65 * 2 * max(u.cin for u in p.units)
    assert (tr.outw_partials > 0, tr.outw_sums) == (k > 1, 65 * k * c0 if k > 1 else 0)
    for u in p.units:
        assert (u.wgrad_bn_workspace > 0) == u.fused_dw and (u.dw_form is None) == u.fused_dw
        assert u.fused_dw <= (not u.need_dgrad) and (u.dgrad is None) == (not u.need_dgrad)


def test_fused_batchnorm_backward_rule(case_plan):
    """bn_bwd_fused is what UNetEngine.backward passed to _bn_bwd_tail as `fused=` before the plan held it."""
    case, p = case_plan
    nl = len(case["dims"]) - 1
    units, ups = p.units, p.ups
    enc = [(units[2 * l], units[2 * l + 1]) for l in range(nl + 1)]
    dec = [(units[2 * (nl + 1) + 2 * j], units[2 * (nl + 1) + 2 * j + 1]) for j in range(nl)]
    assert len(units) == 2 * (2 * nl + 1) and len(ups) == nl
    for lvl, (u0, u1) in enumerate(enc):
        assert u0.level == u1.level == lvl
        assert u0.bn_bwd_fused is True and u0.bn_bwd_fused_rows == u1.dgrad.partial_rows
        assert u1.bn_bwd_fused == (lvl == nl and nl > 0 and ups[0].bn_rows > 0)
        assert u1.bn_bwd_fused_rows == (ups[0].bn_rows if u1.bn_bwd_fused else 0)
    for j, (u0, u1) in enumerate(dec):
        assert u0.level == u1.level == nl - 1 - j == ups[j].level_in - 1
        assert u0.bn_bwd_fused is True and u0.bn_bwd_fused_rows == u1.dgrad.partial_rows
        assert u1.bn_bwd_fused == (j < nl - 1 and ups[j + 1].bn_rows > 0)
        assert u1.bn_bwd_fused_rows == (ups[j + 1].bn_rows if u1.bn_bwd_fused else 0)


GUARD_SHAPES = [(FLAGSHIP, 8, 320, 427), (FLAGSHIP, 32, 320, 427), ([16, 32, 64], 2, 40, 53), ([16, 32, 64], 2, 37, 45)]


def test_every_switch_that_moves_a_plan_is_a_sizing_switch(monkeypatch):
    """The engine keys its plan and buffers on UNetEngine._SIZING_ENV: a library switch outside that list that changes any
    decision would leave a stale plan behind when it is flipped between two steps."""
    assert "GSD_CONV_W2D" in SWITCHES and "GSD_ACT_ONCE" in SWITCHES and len(SWITCHES) > 20, SWITCHES
    plans = lambda: [EP.plan_step(3, 1, dims, n, h, w) for dims, n, h, w in GUARD_SHAPES]
    default = plans()
    moved = {}
    for name in SWITCHES:
        for value in (0, 1, 2, 4, 8, 16, 32, 64):
            with monkeypatch.context() as mp:
                mp.setenv(name, str(value))
                if plans() != default:
                    moved.setdefault(name, []).append(value)
    assert plans() == default
    missing = sorted(set(moved) - set(UNetEngine._SIZING_ENV))
    assert not missing, f"switches that change the plan but are not in UNetEngine._SIZING_ENV: { {k: moved[k] for k in missing} }"
    for name in ("GSD_W2D_SPLIT", "GSD_CONVT_DG_DMA", "GSD_WGRAD_FIRST"):
        assert name in moved, f"{name} no longer moves a plan at these shapes"


def test_plan_is_frozen_and_needs_no_device(monkeypatch):
    import torch

    def refuse(*a, **k):
        raise AssertionError("plan_step touched the device API")

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(torch.cuda, "_lazy_init", refuse)
    monkeypatch.setattr(torch.cuda, "current_stream", refuse)
    p = EP.plan_step(3, 1, [16, 32, 64], 2, 40, 53)
    assert isinstance(p.units, tuple) and isinstance(p.ups, tuple) and isinstance(p.sizes, tuple) and isinstance(p.units[1].fwd, tuple)
    for obj, field in ((p, "n"), (p.units[0], "pitched"), (p.units[1].fwd[True], "algo"), (p.ups[0], "mode_d"), (p.sizes[True], "partials")):
        with pytest.raises(dataclasses.FrozenInstanceError):
            setattr(obj, field, 0)
    assert hash(p) == hash(EP.plan_step(3, 1, [16, 32, 64], 2, 40, 53))
    assert "pooled_pitched" in EP.format_plan(p)
