"""Element-wise fp64 bounds for one real fp32 train step (gelslim_depth_amd/engine.py driven by TrainStep, the metric's engine) at
BASELINE's size: UNet(3, 1, [64, 128, 256, 512, 1024]) at 3x320x427, N = 32 (BASELINE configs[2]) and N = 8 (the per-GPU
share of configs[3], which takes other partial-row counts and so other BatchNorm reduction paths).

A module fixture runs two TrainSteps (lr 1e-3, weight decay 1e-6, EMA 0.995, MSE) in the default environment -- weight
gradients on the side stream, pitched d_raw buffers taken in turn behind their gp_free events, K slabs where the planner picks
them, the 2-D Winograd dW, the one-launch and three-launch BatchNorm reductions, the fused ConvT-dX + BatchNorm pass 1, the
first layer's fused dW -- after snapshotting the parameters, Adam moments, EMA and BatchNorm buffers between the two, so that
step 2 has non-trivial prior state and a step-2 bias correction.  test_schedule asserts that this is the schedule covered.

Every tensor the engine keeps from step 2 is then held, per element, to fp64 on the GPU computed from the engine's OWN stored
inputs (teacher forcing, tests/fp64_ref.py):
  forward    every unit's raw output from its real sources (x, pooled[lvl], the deferred BatchNorm+ReLU of the unit before, the
             decoder's [skip, F.pad(up)] at its pad offset); pooled[lvl] bit-equal to the 2x2 max of max(fmaf(raw, scale,
             shift), 0); every ConvT output with its bias; the output conv, the loss and its gradient;
  BatchNorm  mean / invstd / scale / shift from the sums of the stored raw, with their bound (TAU_STATS over sum |raw|,
             sum raw^2) carried through the one-pass finalize, running statistics from the step-1 snapshot (momentum 0.1, unbiased variance), num_batches_tracked + 1;
  backward   every unit's dz rebuilt from its producer's survivors and its exact ReLU mask: the output conv (bit-equal),
             the fused dX of the second conv of its pair, the skip units' decoder-dX segment plus the pooled gradient routed by
             the exact first-maximum rule, the ConvT dX; dpooled, every ConvT's cropped gradient up.dout; c1 / c2 / dgamma /
             dbeta from fp64 sums of dz;
  gradients  every conv3x3 dW (the first layer's fused one included), ConvT dW and db, the output conv's dW and db;
  optimiser  p, m, v and ema after step 2 against fp64 Adam (coupled L2) + torch_ema from the snapshot and the engine's g_flat.
The taus are those the layer kernels are held to, unchanged: a ratio above them here is a difference between how the unit
tests launch a kernel and how the engine does, not a reason to raise one.

Mutation proofs at the real size: normalising the deepest level with the unbiased variance (a relative invstd change of
1/2 (count - 1), about 3e-5 at N = 32), the running variance updated with the biased one, one pooled gradient routed to the
second-largest element of its window, c2 dropped for one channel of a d_raw, the step-1 bias correction used at step 2 and
the EMA decay of the other step must all be rejected.  So must p computed without the step's weight decay: at step 2 of this
network wd * p = 1e-6 * p is of the size of most gradient elements, and the MI355X run puts about 29 M of the 31 M elements of
p over the bound without it (the report records the count).  Coupled L2 where it dominates (weight_decay = 0.1), step 1000,
grad_scale 1/2 and the guard are held in tests/test_gpu_fp32_pointwise_fp64.py.

GSD_FP64_REPORT_STEP=<path>: write the worst ratio per key, the schedule facts, the module's wall time and peak device memory
there as JSON.
"""
import ctypes as C
import json
import os
import time

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu

DIMS = [64, 128, 256, 512, 1024]
H, W = 320, 427
BUDGET = 1 << 26       # fp64 elements per image chunk of a reference tensor (512 MiB)
LR, WD, EMA = 1e-3, 1e-6, 0.995
T0 = {}
SCHED = {}
INFO = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    torch.cuda.reset_peak_memory_stats()
    T0["t"] = time.time()
    yield
    path = os.environ.get("GSD_FP64_REPORT_STEP")
    if path:
        with open(path, "w") as f:
            json.dump({"wall_s": time.time() - T0["t"], "max_memory_allocated": torch.cuda.max_memory_allocated(),
                       "schedule": SCHED, "info": INFO,
                       "ratios": dict(sorted((k, v) for k, v in R.RATIOS.items() if k.startswith("step")))}, f, indent=1)


def chunks(n, per_image):
    step = max(1, BUDGET // per_image)
    for i in range(0, n, step):
        yield i, min(n, i + step)


def rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


class Run:
    """The engine after step 2, and what step 2 started from."""


@pytest.fixture(scope="module", params=(32, 8), ids=("N32", "N8"))
def run(request):
    from gelslim_depth_amd import synth
    from gelslim_depth_amd.models.unet import UNet
    from gelslim_depth_amd.train import TrainStep
    n = request.param
    st_ = synth.make_state(3, 1, DIMS, 31, "conditioned")
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=DIMS)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st_.items()}, strict=True)
    m = m.to("cuda").train()
    step = TrainStep(m, lr=LR, weight_decay=WD, ema_decay=EMA, loss="mse")
    x1, t1 = synth.make_batch(n, H, W, 32)
    step(torch.from_numpy(x1).cuda(), torch.from_numpy(t1).cuda())
    torch.cuda.synchronize()
    r = Run()
    r.snap = {k: getattr(step, f"{k}_flat").clone() for k in ("p", "m", "v", "ema")}
    r.bn = {k: b.clone() for k, b in m.named_buffers()}
    x2, t2 = synth.make_batch(n, H, W, 33)
    r.x, r.t = torch.from_numpy(x2).cuda(), torch.from_numpy(t2).cuda()
    step(r.x, r.t)
    torch.cuda.synchronize()
    r.n, r.m, r.step, r.eng = n, m, step, m._engine
    r.tag = f"step-N{n}"
    r.P = {k: r.snap["p"][o:o + s].view(step.model._grad_views[k].shape) for k, (o, s) in step.offsets.items()}  # step 2's weights
    r.G = m._grad_views
    r.bufs = dict(m.named_buffers())
    e = r.eng
    r.name = {}
    for lvl, (u0, u1) in enumerate(e.enc):
        nm = "inc" if lvl == 0 else f"down{lvl - 1}"
        r.name[id(u0)], r.name[id(u1)] = f"{nm}.c0", f"{nm}.c1"
    for j, (u0, u1) in enumerate(e.dec):
        r.name[id(u0)], r.name[id(u1)] = f"up{j}.c0", f"up{j}.c1"
    yield r
    del r, step, m, e
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------- the engine's wiring
def act_in(r, u, i, j):
    """Unit u's conv3x3 input for images [i, j) as its kernels read it, fp64."""
    e = r.eng
    for lvl, (u0, u1) in enumerate(e.enc):
        if u is u0:
            return e._x[i:j].double() if lvl == 0 else e.pooled[lvl][i:j].double()
        if u is u1:
            return R.deferred_act(u0.raw[i:j], u0.scale, u0.shift)
    for jj, (u0, u1) in enumerate(e.dec):
        lvl = e.L - 1 - jj
        if u is u1:
            return R.deferred_act(u0.raw[i:j], u0.scale, u0.shift)
        if u is u0:
            skip = e.enc[lvl][1]
            a, off = R.decoder_src(R.deferred_act(skip.raw[i:j], skip.scale, skip.shift), e.ups[jj].out[i:j].double(),
                                   e.hs[lvl], e.ws[lvl])
            assert off == e._pad_off(lvl)
            return a
    raise AssertionError("unit not in the engine")


def holds_dz(u):
    """u.g still holds dz: the apply pass wrote d_raw out of place into the pitched buffer (since reused), or the first layer's
    dW formed d_raw itself.  Otherwise u.g holds d_raw in place."""
    return u.plan.pitched or u.plan.fused_dw


def d_raw_of(u, i, j):
    """(d_raw, bound on |d_raw| of its fp32 evaluation or None) of unit u for images [i, j), as its dW / dX kernels read it."""
    if holds_dz(u):
        return R.bn_bwd_apply(u.g[i:j].double(), u.raw[i:j], u.scale, u.mean, u.invstd, u.c1, u.c2)
    return u.g[i:j].double(), None


def dx_tau(u):
    return R.TAU_WINO if u.plan.dgrad.algo else R.TAU_DIRECT


# ----------------------------------------------------------------------------------------------------------- schedule
def test_schedule(run):
    """The schedule these checks cover is the default one: a later default change must not silently drop coverage."""
    from gelslim_depth_amd import _lib as L
    e, n = run.eng, run.n
    assert e.side is not None and e.side_dw, "weight gradients run on the side stream"
    assert e.gps is not None and len(e.gps) == 2, "two pitched d_raw buffers, taken in turn"
    assert e.one_launch_rows == 4096 and e.sync_fn is None
    assert e.enc[0][0].plan.fused_dw, "the first layer's dW forms d_raw itself"
    pitched = [run.name[id(u)] for u in e.units if u.plan.pitched]
    assert pitched, "at least one unit writes d_raw to the pitched buffer"
    forms, fwd, bwd, slabs = {}, {}, {}, []
    for u in e.units:
        lh, lw = e.hs[u.level], e.ws[u.level]
        nm = run.name[id(u)]
        rows = u.plan.fwd[True].partial_rows
        fwd[nm] = "one" if rows <= e.one_launch_rows else "three"
        fused = u.plan.bn_bwd_fused     # (tests/test_engine_plan_cpu.py states the rule)
        rows_b = u.fused_rows if fused else u.plan.bn_bwd_rows
        bwd[nm] = ("one" if rows_b <= e.one_launch_rows else "three") + (" (dX epilogue)" if fused else "")
        if u.plan.fwd[True].workspace or (u.need_dgrad and u.plan.dgrad.workspace):
            slabs.append(nm)
        if not u.plan.fused_dw:
            dy = L.make_src(u.dsrc)
            form = L.lib.gsd_conv3x3_wgrad_form(u.srcs, len(u.srcs), C.byref(dy), u.cin, u.cout, n, lh, lw)
            assert form == u.plan.dw_form, f"{nm}: the plan's dW form against the library's with the real operands"
            forms[nm] = ("direct", "w43", "w2d")[form]
    SCHED[f"N{n}"] = {"pitched": pitched, "fused_dw": [run.name[id(u)] for u in e.units if u.plan.fused_dw], "dw_form": forms,
                      "bn_forward": fwd, "bn_backward": bwd, "k_slabs": slabs,
                      "convT_dx_fused_bn": [up.plan.bn_rows > 0 for up in e.ups],
                      "convT_db_from_dx_stats": [e.dec[j][0].plan.dgrad.algo >= 1 for j in range(e.L)]}
    assert "w2d" in forms.values(), "the 2-D Winograd dW runs somewhere"
    seen_f = {v for s in SCHED.values() for v in s["bn_forward"].values()}
    seen_b = {v.split()[0] for s in SCHED.values() for v in s["bn_backward"].values()}
    assert seen_f == {"one", "three"} and seen_b == {"one", "three"}, (seen_f, seen_b)
    assert any(up.plan.bn_rows > 0 for up in e.ups), "the fused ConvT dX + BatchNorm pass 1 runs"


# ----------------------------------------------------------------------------------------------------------- forward
def test_forward_and_batchnorm(run):
    e, n, P, tag = run.eng, run.n, run.P, run.tag
    for u in e.units:
        lh, lw = e.hs[u.level], e.ws[u.level]
        nm = run.name[id(u)]
        tau = R.TAU_WINO if u.plan.fwd[True].algo else R.TAU_DIRECT
        w64 = P[u.wname].double()
        acc = [torch.zeros(u.cout, dtype=torch.float64, device="cuda") for _ in range(4)]
        for i, j in chunks(n, max(u.cin, u.cout) * lh * lw):
            ref, cond = R.conv3x3_fwd(act_in(run, u, i, j), w64)
            R.check_bound(u.raw[i:j], ref, cond, tau, f"{tag} {nm} raw", n0=i, key=f"{tag}-fwd")
            del ref, cond
            # the statistics epilogue sums the values it stores: the sums of the stored raw, bounded by sum |raw|, sum raw^2
            acc = [a + b for a, b in zip(acc, R.stored_sums(u.raw[i:j]))]
        count = float(n * lh * lw)
        fin = R.bn_finalize_ref(acc[0], acc[1], acc[2], acc[3], count, P[u.gname], P[u.bname],
                                running_mean=run.bn[u.rmname], running_var=run.bn[u.rvname])
        for k, got in (("mean", u.mean), ("invstd", u.invstd), ("scale", u.scale), ("shift", u.shift),
                       ("running_mean", run.bufs[u.rmname]), ("running_var", run.bufs[u.rvname])):
            R.check_bound_rounded(got, *fin[k], R.TAU_STATS, f"{tag} {nm} {k}", key=f"{tag}-bn")
        assert int(run.bufs[u.nbtname]) == int(run.bn[u.nbtname]) + 1, f"{tag} {nm} num_batches_tracked"
        if u is e.enc[e.L][0]:
            # the deepest level normalised with the unbiased variance: invstd off by 1/2 (count - 1) relative
            var = fin["var"][0]
            unb = 1.0 / torch.sqrt(var * count / (count - 1.0) + R.f32c(1e-5))
            rejects(R.check_bound_rounded, unb.float(), *fin["invstd"], R.TAU_STATS, f"{tag} {nm} invstd (unbiased variance)")
            mom = R.f32c(0.1)
            biased = (1.0 - mom) * run.bn[u.rvname].double() + mom * var
            rejects(R.check_bound_rounded, biased.float(), *fin["running_var"], R.TAU_STATS,
                    f"{tag} {nm} running_var (biased variance)")
    # pooled[lvl]: a selection of single fmaf roundings -- bit-equal
    for lvl in range(1, e.L + 1):
        prev = e.enc[lvl - 1][1]
        for i, j in chunks(n, prev.cout * e.hs[lvl - 1] * e.ws[lvl - 1]):
            best, _ = R.maxpool_route(R.bnrelu_act(prev.raw[i:j], prev.scale, prev.shift))
            assert torch.equal(e.pooled[lvl][i:j].double(), best), f"{tag} pooled[{lvl}] (images {i}..{j})"
            del best
    for jj, up in enumerate(e.ups):
        prev = e.dec[jj - 1][1] if jj > 0 else e.enc[e.L][1]
        hi, wi = e.hs[e.L - jj], e.ws[e.L - jj]
        for i, j in chunks(n, max(up.cin * hi * wi, up.cout * 4 * hi * wi)):
            ref, cond = R.convT_fwd(R.deferred_act(prev.raw[i:j], prev.scale, prev.shift), P[up.wname].double(),
                                    P[up.bname].double())
            R.check_bound(up.out[i:j], ref, cond, R.TAU_CONVT, f"{tag} up{jj}.up out", n0=i, key=f"{tag}-convT")
            del ref, cond
    last = e.dec[-1][1]
    out = run.step._out
    wo, bo = P["outc.conv.weight"].double().view(1, -1), P["outc.conv.bias"].double()
    for i, j in chunks(n, last.cout * H * W):
        ref, cond = R.conv1x1_fwd(R.deferred_act(last.raw[i:j], last.scale, last.shift), wo, bo)
        R.check_bound(out[i:j], ref, cond, R.TAU_1X1, f"{tag} output", n0=i, key=f"{tag}-1x1")
        del ref, cond
    lref = ((out.double() - run.t.double()) ** 2).mean().view(1)
    R.check_bound(run.step.loss_buf, lref, lref, R.TAU_1X1, f"{tag} loss", key=f"{tag}-1x1")
    gref, gcond = R.mse_grad(out, run.t, out.numel())
    R.check_bound(run.step._dout, gref, gcond, R.TAU_1X1, f"{tag} loss gradient", key=f"{tag}-1x1")


# ----------------------------------------------------------------------------------------------------------- backward
def test_backward_chain(run):
    """Unit by unit (the map of test_gpu_net.py::test_backward_teacher_forced_unit_by_unit): dz of each unit from its producer's
    survivors and its exact mask; u.g against dz (or d_raw), c1 / c2 / dgamma / dbeta against fp64 sums of dz; dpooled; the
    cropped ConvT gradient up.dout and, where the Winograd dX that writes it leaves it, the ConvT bias gradient."""
    e, n, P, G, tag = run.eng, run.n, run.P, run.G, run.tag
    cv = (1, -1, 1, 1)
    last = e.dec[-1][1]
    wo = P["outc.conv.weight"].double().view(cv)
    dout = run.step._dout
    mutated = {"pool": False, "c2": False}

    def producer(u, i, j, lh, lw):
        """(gradient w.r.t. u's activation, its cond, tau, bit-exact) for images [i, j)."""
        if u is last:
            return (dout[i:j].double() * wo).float().double(), None, R.TAU_1X1, True
        for lvl, (u0, u1) in enumerate(e.enc):
            if u is u0:
                d, da = d_raw_of(u1, i, j)
                g, c = R.conv3x3_dx(d, P[u1.wname].double(), da)
                return g, c, dx_tau(u1), False
            if u is u1 and lvl == e.L:
                up = e.ups[0]
                g, c = R.convT_dx(up.dout[i:j].double(), P[up.wname].double())
                return g, c, R.TAU_CONVT, False
            if u is u1:      # skip unit: first segment of the decoder conv's dX + the routed pooled gradient
                jj = e.L - 1 - lvl
                d0 = e.dec[jj][0]
                d, da = d_raw_of(d0, i, j)
                full, fc = R.conv3x3_dx(d, P[d0.wname].double(), da)
                up = e.ups[jj]
                oy, ox = e._pad_off(lvl)
                hu, wu = up.dout.shape[2], up.dout.shape[3]
                ru, cu = full[:, u.cout:, oy:oy + hu, ox:ox + wu], fc[:, u.cout:, oy:oy + hu, ox:ox + wu]
                R.check_bound(up.dout[i:j], ru, cu, dx_tau(d0), f"{tag} up{jj}.up dout (cropped dX of up{jj}.c0)", n0=i,
                              key=f"{tag}-dx")
                dbacc[jj][0] += ru.sum((0, 2, 3))
                dbacc[jj][1] += cu.sum((0, 2, 3))
                _, code = R.maxpool_route(R.bnrelu_act(u.raw[i:j], u.scale, u.shift))
                routed = R.pool_grad(e.dpooled[lvl + 1][i:j], code, lh, lw)
                codes[id(u)] = (code, e.dpooled[lvl + 1][i:j])
                return full[:, :u.cout] + routed, fc[:, :u.cout] + routed.abs(), dx_tau(d0), False
        for jj, (u0, u1) in enumerate(e.dec):
            if u is u0:
                d, da = d_raw_of(u1, i, j)
                g, c = R.conv3x3_dx(d, P[u1.wname].double(), da)
                return g, c, dx_tau(u1), False
            if u is u1:
                up = e.ups[jj + 1]
                g, c = R.convT_dx(up.dout[i:j].double(), P[up.wname].double())
                return g, c, R.TAU_CONVT, False
        raise AssertionError

    dbacc = [[torch.zeros(up.cout, dtype=torch.float64, device="cuda") for _ in range(2)] for up in e.ups]
    codes = {}
    for u in e.units:
        nm = run.name[id(u)]
        lh, lw = e.hs[u.level], e.ws[u.level]
        acc = [torch.zeros(u.cout, dtype=torch.float64, device="cuda") for _ in range(4)]
        tau_s = R.TAU_STATS
        for i, j in chunks(n, 2 * max(u.cin, u.cout) * lh * lw):
            g, gc, tau, exact = producer(u, i, j, lh, lw)
            m = R.bnrelu_mask(u.raw[i:j], u.scale, u.shift)
            z = torch.zeros((), dtype=torch.float64, device="cuda")
            dz = torch.where(m, g, z)
            dzc = dz.abs() if exact else torch.where(m, gc, z)
            del g, gc
            xhat = (u.raw[i:j].double() - u.mean.double().view(cv)) * u.invstd.double().view(cv)
            if holds_dz(u):
                if exact:
                    assert torch.equal(u.g[i:j].double(), dz), f"{tag} {nm} dz = where(mask, fl32(dout * w), 0)"
                R.check_bound(u.g[i:j], dz, dzc, tau, f"{tag} {nm} dz", n0=i, key=f"{tag}-dz")
                s = u.g[i:j].double()
                acc = [a + b for a, b in zip(acc, (s.sum((0, 2, 3)), (s * xhat).sum((0, 2, 3)), s.abs().sum((0, 2, 3)),
                                                   (s * xhat).abs().sum((0, 2, 3))))]
                if u is e.enc[0][1] and not mutated["c2"]:
                    # c2 dropped for one channel of this unit's d_raw (rebuilt from the stored dz)
                    d, dc = d_raw_of(u, i, j)
                    k = int(u.c2.abs().argmax())
                    bad = d.clone()
                    bad[:, k] += u.scale[k].double() * xhat[:, k] * u.c2[k].double()
                    rejects(R.check_bound, bad.float(), d, dc, tau, f"{tag} {nm} d_raw with c2 dropped in channel {k}")
                    mutated["c2"] = True
                    del d, dc, bad
                if id(u) in codes and not mutated["pool"]:
                    mutated["pool"] = pool_mutation_rejected(u, i, j, *codes[id(u)], dz, dzc, tau, f"{tag} {nm}")
            else:
                ref, cond = R.bn_bwd_apply(dz, u.raw[i:j], u.scale, u.mean, u.invstd, u.c1, u.c2)
                cond += u.scale.double().abs().view(cv) * dzc
                R.check_bound(u.g[i:j], ref, cond, tau, f"{tag} {nm} d_raw (in place)", n0=i, key=f"{tag}-draw")
                acc = [a + b for a, b in zip(acc, (dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3)), dzc.sum((0, 2, 3)),
                                                   (dzc * xhat.abs()).sum((0, 2, 3))))]
                tau_s = tau + R.TAU_STATS
                del ref, cond
            codes.pop(id(u), None)
            del dz, dzc, xhat, m
        count = float(n * lh * lw)
        R.check_bound_rounded(G[u.bname], acc[0], acc[2], tau_s, f"{tag} {nm} dbeta", key=f"{tag}-bnbwd")
        R.check_bound_rounded(G[u.gname], acc[1], acc[3], tau_s, f"{tag} {nm} dgamma", key=f"{tag}-bnbwd")
        R.check_bound_rounded(u.c1, acc[0] / count, acc[2] / count, tau_s, f"{tag} {nm} c1", key=f"{tag}-bnbwd")
        R.check_bound_rounded(u.c2, acc[1] / count, acc[3] / count, tau_s, f"{tag} {nm} c2", key=f"{tag}-bnbwd")
    assert mutated["c2"] and mutated["pool"], mutated
    for lvl in range(1, e.L + 1):
        u0 = e.enc[lvl][0]
        for i, j in chunks(n, 2 * max(u0.cin, u0.cout) * e.hs[lvl] * e.ws[lvl]):
            d, da = d_raw_of(u0, i, j)
            ref, cond = R.conv3x3_dx(d, P[u0.wname].double(), da)
            R.check_bound(e.dpooled[lvl][i:j], ref, cond, dx_tau(u0), f"{tag} dpooled[{lvl}]", n0=i, key=f"{tag}-dx")
            del d, da, ref, cond
    for jj, up in enumerate(e.ups):
        if e.dec[jj][0].plan.dgrad.algo >= 1:     # the bias gradient from the statistics of the dX launch that wrote up.dout
            R.check_sums(G[up.bname], dbacc[jj][0], dbacc[jj][1], R.TAU_STATS, f"{tag} up{jj}.up db (dX statistics)",
                         key=f"{tag}-stats")


def pool_mutation_rejected(u, i, j, code, dpool, dz, dzc, tau, what):
    """One pooled gradient routed to the second-largest element of its window instead of the largest, in a copy of the unit's
    surviving dz (images [i, j)): the bound must reject it.  Returns whether this chunk had a window to mutate (a positive
    second-largest element, strictly below the maximum, and a non-zero pooled gradient)."""
    a = R.bnrelu_act(u.raw[i:j], u.scale, u.shift)
    n_, c_, h, w = a.shape
    hp, wp = h // 2, w // 2
    win = a[:, :, :2 * hp, :2 * wp].reshape(n_, c_, hp, 2, wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(n_, c_, hp, wp, 4)
    srt = win.sort(dim=-1, descending=True, stable=True)
    cand = ((srt.values[..., 1] > 0) & (srt.values[..., 0] > srt.values[..., 1]) & (dpool != 0)).nonzero()
    if len(cand) == 0:
        return False
    ii, cc, yy, xx = cand[len(cand) // 2].tolist()
    q1, q2 = int(code[ii, cc, yy, xx]), int(srt.indices[ii, cc, yy, xx, 1])
    assert q1 == int(srt.indices[ii, cc, yy, xx, 0]) and q1 != q2
    dp = dpool[ii, cc, yy, xx]
    got = u.g[i:j].clone()
    got[ii, cc, 2 * yy + q1 // 2, 2 * xx + q1 % 2] -= dp
    got[ii, cc, 2 * yy + q2 // 2, 2 * xx + q2 % 2] += dp
    rejects(R.check_bound, got, dz, dzc, tau, f"{what} dz with window ({i + ii}, {cc}, {yy}, {xx}) routed to its second-largest")
    return True


# ---------------------------------------------------------------------------------------------------- weight gradients
def test_parameter_gradients(run):
    """Every conv3x3 dW (the first layer's fused one from its stored dz), ConvT dW (and db where the ConvT dW kernel forms it),
    the output conv's dW (the third sum of the mode-2 reduce) and db (gsd_sum_planes)."""
    e, n, P, G, tag = run.eng, run.n, run.P, run.G, run.tag
    for u in e.units:
        nm = run.name[id(u)]
        lh, lw = e.hs[u.level], e.ws[u.level]
        ref = torch.zeros(G[u.wname].shape, dtype=torch.float64, device="cuda")
        cond = torch.zeros_like(ref)
        for i, j in chunks(n, 2 * max(u.cin, u.cout) * lh * lw):
            d, da = d_raw_of(u, i, j)
            r_, c_ = R.conv3x3_dw(act_in(run, u, i, j), d, da)
            ref += r_
            cond += c_
            del d, da, r_, c_
        R.check_bound(G[u.wname], ref, cond, R.TAU_DW, f"{tag} {nm} dW{' (fused first layer)' if u.plan.fused_dw else ''}",
                      key=f"{tag}-dw", weights=True)
    for jj, up in enumerate(e.ups):
        prev = e.dec[jj - 1][1] if jj > 0 else e.enc[e.L][1]
        hi, wi = e.hs[e.L - jj], e.ws[e.L - jj]
        acc = [torch.zeros(G[up.wname].shape, dtype=torch.float64, device="cuda")] * 2 + \
              [torch.zeros(up.cout, dtype=torch.float64, device="cuda")] * 2
        for i, j in chunks(n, max(up.cin * hi * wi, up.cout * 4 * hi * wi)):
            p_ = R.convT_dw(R.deferred_act(prev.raw[i:j], prev.scale, prev.shift), up.dout[i:j].double())
            acc = [a + b for a, b in zip(acc, p_)]
            del p_
        R.check_bound(G[up.wname], acc[0], acc[1], R.TAU_CONVT, f"{tag} up{jj}.up dW", key=f"{tag}-convT", weights=True)
        if e.dec[jj][0].plan.dgrad.algo == 0:     # else from the dX statistics (test_backward_chain)
            R.check_bound(G[up.bname], acc[2], acc[3], R.TAU_CONVT, f"{tag} up{jj}.up db", key=f"{tag}-convT", weights=True)
    last = e.dec[-1][1]
    dout = run.step._dout.double()
    acc = [0.0] * 4
    for i, j in chunks(n, last.cout * H * W):
        p_ = R.conv1x1_dw(R.deferred_act(last.raw[i:j], last.scale, last.shift), dout[i:j])
        acc = [a + b for a, b in zip(acc, p_)]
        del p_
    R.check_bound(G["outc.conv.weight"].view(1, -1), acc[0], acc[1], R.TAU_1X1, f"{tag} outc dW", key=f"{tag}-1x1", weights=True)
    R.check_bound(G["outc.conv.bias"], acc[2], acc[3], R.TAU_1X1, f"{tag} outc db", key=f"{tag}-1x1", weights=True)


# ---------------------------------------------------------------------------------------------------------- optimiser
def test_adam_ema(run):
    """p, m, v and ema after step 2 against fp64 Adam (coupled L2, step-2 bias correction) + torch_ema (the warm-up decay of
    update 2, min(0.995, 3 / 12)) from the step-1 snapshot and the engine's gradient arena, element by element."""
    s, tag = run.step, run.tag
    assert s.step_count == 2 and s.ema_updates == 2
    d2 = min(EMA, 3.0 / 12.0)
    sn = run.snap
    ref = R.adam_ema_ref(sn["p"], s.g_flat, sn["m"], sn["v"], sn["ema"], 2, LR, weight_decay=WD, ema_decay=d2)
    for k in ("p", "m", "v", "ema"):
        R.check_bound(getattr(s, f"{k}_flat"), *ref[k], R.TAU_ADAM, f"{tag} adam {k}", key=f"{tag}-adam", weights=True)
    bad = R.adam_ema_ref(sn["p"], s.g_flat, sn["m"], sn["v"], sn["ema"], 1, LR, weight_decay=WD, ema_decay=d2)
    rejects(R.check_bound, bad["p"][0].float(), *ref["p"], R.TAU_ADAM, f"{tag} p with the bias correction of step 1",
            weights=True)
    d1 = min(EMA, 2.0 / 11.0)
    bad = R.adam_ema_ref(sn["p"], s.g_flat, sn["m"], sn["v"], sn["ema"], 2, LR, weight_decay=WD, ema_decay=d1)
    rejects(R.check_bound, bad["ema"][0].float(), *ref["ema"], R.TAU_ADAM, f"{tag} ema with the decay of update 1",
            weights=True)
    # coupled L2 at 1e-6: wd * p is of the size of most of this network's gradients at step 2, so dropping it shows
    nowd = R.adam_ema_ref(sn["p"], s.g_flat, sn["m"], sn["v"], sn["ema"], 2, LR, weight_decay=0.0, ema_decay=d2)
    rejects(R.check_bound, nowd["p"][0].float(), *ref["p"], R.TAU_ADAM, f"{tag} p without weight decay", weights=True)
    INFO[f"{tag} elements of p over the bound with weight decay dropped"] = int(
        ((nowd["p"][0].float().double() - ref["p"][0]).abs() > R.TAU_ADAM * ref["p"][1] + R.U32 * ref["p"][0].abs()).sum())
    INFO[f"{tag} arena numel"] = s.numel
