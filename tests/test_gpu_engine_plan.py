"""The fp32 engine allocates and launches what its plan (engine_plan.plan_step) says: after one train step per case of
test_gpu_engine_memory.py's fp32 table -- the smallest shapes that switch every plan flag both ways -- the buffers have the planned
sizes, and the decisions the planner took from descriptors (the dW form, the ConvT dX weight-image mode, the fused row counts)
are the ones the library gives for the real operands."""
import ctypes as C

import pytest

import engine_state as S
from test_gpu_engine_memory import FP32_CASES, clean_env  # noqa: F401  (clean_env: autouse, the cases' switches cleared)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", FP32_CASES, ids=[c.name for c in FP32_CASES])
def test_engine_runs_its_plan(case):
    from gelslim_depth_amd import _lib as L
    from gelslim_depth_amd.engine_plan import plan_step
    lib = L.lib
    _, e = S.train_steps(case, k=1)
    with S.environ(case.env):
        assert e.plan == plan_step(3, case.n_classes, case.dims, case.n, case.h, case.w)
        n, hs, ws, size = case.n, e.hs, e.ws, e.plan.sizes[True]
        assert (tuple(hs), tuple(ws)) == (e.plan.hs, e.plan.ws)

        numel = lambda t: 0 if t is None else t.numel()
        got = {"partials": numel(e.partials), "conv_ws": numel(e.conv_ws), "act_buf": numel(e.act_buf), "wgrad_ws": numel(e.wgrad_ws),
               "wgrad_ws_side": numel(e.wgrad_ws_side), "db_sums": numel(e.db_sums), "outw_partials": numel(e.outw_partials),
               "outw_sums": numel(e.outw_sums)}
        want = {k: getattr(size, k) for k in got}
        if e.side is None:
            want["wgrad_ws_side"] = 0
        assert got == want
        assert [numel(g) for g in e.gps or []] == ([size.gp] * (2 if e.side is not None else 1) if size.gp else [])
        for u in e.units:
            assert u.plan is e.plan.units[e.units.index(u)]
            assert (u.wt_f.numel(), u.wt_d.numel()) == (u.plan.wt_f_size, u.plan.wt_d_size)
            assert u.raw.shape == u.g.shape == (n, u.cout, hs[u.level], ws[u.level])
        for up in e.ups:
            assert (up.wt_f.numel(), up.wt_d.numel()) == (up.plan.wt_f_size, up.plan.wt_d_size)
            assert (up.cat is not None) == up.plan.cat_on
        # the names the decisions had as attributes read the plan
        for u in e.units:
            assert (u.pitched, u.fused_dw, u.act_once, u.form_f.algo) == (u.plan.pitched, u.plan.fused_dw, u.plan.act_once, u.plan.fwd[True].algo)
            assert (u.form_d is None) == (u.plan.dgrad is None) and (u.form_d is None or u.form_d.algo == u.plan.dgrad.algo)
        assert [(up.mode_d, up.bn_rows) for up in e.ups] == [(p.mode_d, p.bn_rows) for p in e.plan.ups]
        assert e.cat_on == [p.cat_on for p in e.plan.ups] and e.pooled_pitched == list(e.plan.pooled_pitched)
        for l in range(1, e.L + 1):
            assert (e.pooled[l].stride(2) != ws[l]) == (e.plan.pooled_pitched[l] and ws[l] % 4 != 0)

        for u in e.units:
            lh, lw = hs[u.level], ws[u.level]
            if not u.plan.fused_dw:
                dy = L.make_src(u.dsrc)
                assert (dy.w_stride != lw) == (u.plan.pitched and lw % 4 != 0)
                assert lib.gsd_conv3x3_wgrad_form(u.srcs, len(u.srcs), C.byref(dy), u.cin, u.cout, n, lh, lw) == u.plan.dw_form
            if u.plan.bn_bwd_fused:
                assert u.fused_rows == u.plan.bn_bwd_fused_rows > 0
        for up in e.ups:
            li = up.level_in
            dy = L.make_src(up.dout, slack=L.SLACK)
            assert lib.gsd_convT2x2_dgrad_layout(C.byref(dy), up.cin, up.cout, n, hs[li], ws[li]) == up.plan.mode_d
            rows = lib.gsd_convT2x2_dgrad_bnrelu_partial_rows(C.byref(dy), up.cin, up.cout, n, hs[li], ws[li])
            assert up.plan.bn_rows == (rows if up.plan.mode_d == 7 else 0)
