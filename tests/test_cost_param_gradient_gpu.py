"""The cost gradient with respect to a trajectory's rows on the GPU (quattro_cost_param_gradient_f32, ops.cost_param_gradient, the
row gradients of autograd.trajectory_cost), built-in models:
   1. grad_phys, grad_cost_rows and grad_ref_rows through the C entry, fed the fp64 reference costate rounded to fp32, against the
      fp64 reference: every set of pgrad_cases.SETS, both integrators, B in param_cases.BATCHES, N in (1, 2, 7, 26, 65) -- 65 crosses a
      64-step pass -- and R in (none, 1, 3, N + 1, N + 3); rows past the horizon and the padding are exactly +0.0;
   2. ops.cost_param_gradient on the device's own costate under heterogeneous weights, targets and phys, alone and together;
   3. bit-for-bit identities: a row of a batch against the B = 1 call, each output alone against all three, NULL rows against
      neutral rows, heterogeneous rows against B calls on model.with_(...), a given costate against the two-launch form, and
      ops.cost_gradient's outputs before and after;
   4. autograd: gradients with respect to tensor rows against ops.cost_param_gradient, upstream weights, and a call in which no row
      requires a gradient against today's path;
   5. the use case: one gradient step on model_phys lowers the fp64 oracle cost of every trajectory against a logged rollout.
The bound of 1 and 2 is pgrad_cases.gpu_bound: the larger of 4 x E (the fp32 restatement's distance from fp64, measured on the CPU)
and the project's fp32 floor 2e-6; every measured value is printed before it is asserted.  Reference, measures, mutants:
tests/pgrad_cases.py, tests/test_cost_param_gradient_cpu.py.

Measured on one MI355X, worst over the shapes of 1: grad_phys 3.1e-7 (quadrotor) and 8.5e-8 (cart-pole), grad_weights 1.8e-7,
grad_targets 1.1e-7; through ops (2): 1.3e-7, 1.7e-7, 1.1e-7.  (With the cart-pole's parameter terms formed in fp32 the skew_barrier
batch at N = 1, B = 9 measured grad_phys 6.3e-6 (Euler) and 2.4e-6 (RK4) against the bound 2e-6: d(theta'')/d(length) cancels
forty-fold at one of its states, csrc/models_generic.h says more; those terms are fp64 now.)"""
import ctypes

import numpy as np
import pytest

import grad_cases as gc
import param_cases as pc
import pgrad_cases as pg
import ref_cases as rc
import weight_cases as wc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BUILTIN = [(model, s, integ) for model in pc.MODELS for s in pg.SETS[model] for integ in pg.INTEGRATORS]
HORIZONS = (1, 2, 7, 26, 65)
KEYS = ("grad_phys", "grad_weights", "grad_targets")


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def host(out):
    return {key: v.double().cpu().numpy() for key, v in out.items()}


def _same(a, b, tag):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b), tag
    assert torch.equal(torch.signbit(a), torch.signbit(b)), tag + " (sign of zero)"


def c_entry(md, x, u, lam, phys=None, rows=None, w=None):
    """quattro_cost_param_gradient_f32 itself, all three outputs pre-filled with NaN -> the raw arrays (B, 8), (B, 40), (B, R, n)."""
    q = _pkg()
    ops = q.ops
    B, N = u.shape[:2]
    xd, ud, ld = dev32(x), dev32(u), dev32(lam)
    pt, rt, ct = ops.model_phys_tensor(md, phys, B, DEV), ops.x_ref_rows_tensor(md, rows, B, DEV), ops.cost_rows_tensor(md, w, B, DEV)
    R = 1 if rt is None else rt.shape[1]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
    gp, gw, gr = nan(B, 8), nan(B, ops.COST_ROW_FLOATS), nan(B, R, md.n)
    p = md.c_params()
    status = q._lib.load_for(md).quattro_cost_param_gradient_f32(
        ctypes.byref(p), ops._ptr(xd), ops._ptr(ud), B, N, ops._ptr(ld), ops._ptr(pt), ops._ptr(rt), 0 if rt is None else R,
        ops._ptr(ct), ops._ptr(gp), ops._ptr(gw), ops._ptr(gr), ops._stream())
    assert status == 0, status
    torch.cuda.synchronize()
    return gp.cpu().numpy(), gw.cpu().numpy(), gr.cpu().numpy()


def _positive_zero(a):
    return bool(np.all(a == 0.0) and not np.any(np.signbit(a)))


# ------------------------------------------------------------------------------------------------ 1. parity through the C entry
@pytest.mark.parametrize("model,set_name,integ", BUILTIN)
def test_c_entry_matches_the_fp64_reference(model, set_name, integ):
    q = _pkg()
    md = pc.device_model(q.models, model, set_name, integ)
    n, m, NP = md.n, md.m, len(md.phys)
    MX = q._lib.MAX_NX
    bound = pg.gpu_bound(model)
    bad = []
    for N in HORIZONS:
        for R in (None, 1, 3, N + 1, N + 3):
            c = pg.case(model, set_name, integ, N, R=R)
            ref = pg.reference(model, c["spec"], c["x"], c["u"], c["lam"], **c["kw"])
            for B in pc.BATCHES[model]:
                gp, gw, gr = c_entry(md, c["x"][:B], c["u"][:B], c["lam"][:B], rows=None if R is None else c["rows"][:B])
                got = dict(grad_phys=gp[:, :NP], grad_weights=np.concatenate([gw[:, :n], gw[:, MX:MX + n], gw[:, 2 * MX:2 * MX + m]], axis=1),
                           grad_targets=gr)
                errs = pg.errors(got, {k: v[:B] for k, v in ref.items()})
                print(f"[pgrad {model} {set_name} {integ}] N={N} R={R} B={B}: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
                bad += [(N, R, B, k, e) for k, e in errs.items() if not e < bound]
                # padding and rows past the horizon: exactly +0.0
                assert _positive_zero(gp[:, NP:]), (N, R, B)
                assert _positive_zero(gw[:, n:MX]) and _positive_zero(gw[:, MX + n:2 * MX]) and _positive_zero(gw[:, 2 * MX + m:]), (N, R, B)
                if R is not None and R > N + 1:
                    assert _positive_zero(gr[:, N + 1:]), (N, R, B)
    assert not bad, (bound, bad)


# ------------------------------------------------------------------------------------------------ 2. parity through ops
@pytest.mark.parametrize("integ", pg.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_ops_rows_match_the_fp64_reference_of_each_trajectory(model, integ):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    N, bound = 7, pg.gpu_bound(model)
    for het in (("weights",), ("targets",), ("phys",), ("weights", "targets", "phys")):
        c = pg.case(model, "skew", integ, N, hetero=het)
        ref = pg.reference(model, c["spec"], c["x"], c["u"], c["lam"], **c["kw"])
        got = q.ops.cost_param_gradient(md, dev32(c["x"]), dev32(c["u"]), targets=c["rows"], weights=c["w"], model_phys=c["phys"])
        assert set(got) == set(KEYS) and all(v.dtype == torch.float64 and v.is_cuda for v in got.values())
        assert tuple(got["grad_phys"].shape) == (c["u"].shape[0], len(md.phys))
        assert tuple(got["grad_weights"].shape) == (c["u"].shape[0], 2 * md.n + md.m)
        assert tuple(got["grad_targets"].shape) == (c["u"].shape[0], 1 if c["rows"] is None else c["rows"].shape[1], md.n)
        errs = pg.errors(host(got), ref)
        print(f"[pgrad rows {model} {integ}] {'+'.join(het)}: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert pg.worst(errs) < bound, (het, errs, bound)


# ------------------------------------------------------------------------------------------------ 3. identities
def _with(md, wrow=None, prow=None, xref=None):
    kw = {}
    if wrow is not None:
        qv, qf, r = wc.split((md.n, md.m), wrow)
        kw.update(q=tuple(map(float, qv)), qf=tuple(map(float, qf)), r=tuple(map(float, r)))
    if prow is not None:
        kw["phys"] = tuple(map(float, prow))
    if xref is not None:
        kw["x_ref"] = tuple(map(float, xref))
    return md.with_(**kw)


@pytest.mark.parametrize("integ", pg.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_identities_bit_for_bit(model, integ):
    q = _pkg()
    pgrad, grad = q.ops.cost_param_gradient, q.ops.cost_gradient
    md = pc.device_model(q.models, model, "skew", integ)
    for N in (7, 65):
        c = pg.case(model, "skew", integ, N, R=3, hetero=("weights", "targets", "phys"))
        B = c["u"].shape[0]
        xd, ud = dev32(c["x"]), dev32(c["u"])
        w, phys, rows = c["w"], c["phys"], c["rows"]
        het = dict(targets=rows, weights=w, model_phys=phys)
        before = grad(md, xd, ud, want_costate=True, **het)
        full = pgrad(md, xd, ud, **het)
        # ops.cost_gradient is what it was, before and after
        after = grad(md, xd, ud, want_costate=True, **het)
        for key in before:
            _same(before[key], after[key], f"cost_gradient {key} after the new call")
        # a given costate against the two-launch form
        given = pgrad(md, xd, ud, costate=before["costate"], **het)
        for key in KEYS:
            _same(given[key], full[key], f"given costate {key}")
        # each output alone against all three together
        for want in ("phys", "weights", "targets"):
            alone = pgrad(md, xd, ud, want=(want,), **het)
            assert set(alone) == {"grad_" + want}
            _same(alone["grad_" + want], full["grad_" + want], f"{want} alone")
        # a row of the batch is the B = 1 call
        for b in sorted({0, B // 2, B - 1}):
            one = pgrad(md, xd[b:b + 1].contiguous(), ud[b:b + 1].contiguous(), targets=rows[b:b + 1], weights=w[b:b + 1],
                        model_phys=phys[b:b + 1])
            for key in KEYS:
                _same(one[key], full[key][b:b + 1], f"row {b} {key}")
        if N != 7:
            continue
        # neutral rows are no rows (R = 1: the model's own x_ref as one row)
        plain = pgrad(md, xd, ud)
        neutral = dict(targets=rc.neutral_rows(md.x_ref, B, 1), weights=np.tile(np.concatenate([md.q, md.qf, md.r]).astype(np.float32), (B, 1)),
                       model_phys=np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1)))
        for keys in (("targets",), ("weights",), ("model_phys",), ("targets", "weights", "model_phys")):
            got = pgrad(md, xd, ud, **{k: neutral[k] for k in keys})
            for key in KEYS:
                _same(got[key], plain[key], f"neutral {keys} {key}")
        # heterogeneous rows against B calls on with_(): one goal per trajectory (R = 1) is with_(x_ref=row)
        goal = rows[:, 2]
        het1 = dict(targets=goal, weights=w, model_phys=phys)
        for keys in (("targets",), ("weights",), ("model_phys",), ("targets", "weights", "model_phys")):
            got = pgrad(md, xd, ud, **{k: het1[k] for k in keys})
            for b in range(B):
                mb = _with(md, w[b] if "weights" in keys else None, phys[b] if "model_phys" in keys else None,
                           goal[b] if "targets" in keys else None)
                one = pgrad(mb, xd[b:b + 1].contiguous(), ud[b:b + 1].contiguous())
                for key in KEYS:
                    _same(one[key], got[key][b:b + 1], f"heterogeneous {keys} b={b} {key}")
        assert not torch.equal(full["grad_phys"], plain["grad_phys"])


# ------------------------------------------------------------------------------------------------ 4. autograd
@pytest.mark.parametrize("integ", pg.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_autograd_row_gradients_are_the_kernel(model, integ):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    N, B = 7, pc.B_FULL[model]
    x0, u = pc.inputs(model, "skew", N)
    w, phys, rows = wc.weight_rows(model, B), gc.phys_rows(model, B), rc.skew_rows(model, B, 4)
    x0d, ud = dev32(x0), dev32(u)
    zK = torch.zeros((B, N, md.m, md.n), device=DEV)
    x, _ = q.ops.track(md, x0d, torch.zeros((B, N + 1, md.n), device=DEV), ud, zK, N, plant_phys=phys, feedback=False)
    ref = q.ops.cost_param_gradient(md, x, ud, targets=rows, weights=w, model_phys=phys)
    base = q.ops.cost_gradient(md, x, ud, targets=rows, weights=w, model_phys=phys)
    up = torch.linspace(0.5, 2.0, B, device=DEV, dtype=torch.float64)
    # device tensors (float32) and host tensors (float64): the gradient takes the tensor's shape, dtype and device
    for make in (lambda a: dev32(a).requires_grad_(True), lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).requires_grad_(True)):
        tw, tp, tr = make(w), make(phys), make(rows)
        xg, ug = dev32(x0).requires_grad_(True), dev32(u).requires_grad_(True)
        J = q.trajectory_cost(md, xg, ug, targets=tr, weights=tw, model_phys=tp)
        _same(J.detach(), q.ops.score(md, x, ud, terminal=True, targets=rows, weights=w, model_phys=phys)[0], "forward value")
        gx, gu, gw, gp, gr = torch.autograd.grad(J.sum(), (xg, ug, tw, tp, tr))
        _same(gu, base["grad_u"], "grad_u")
        _same(gx, base["grad_x0"], "grad_x0")
        for got, like, key in ((gw, tw, "grad_weights"), (gp, tp, "grad_phys"), (gr, tr, "grad_targets")):
            assert got.shape == like.shape and got.dtype == like.dtype and got.device == like.device, key
            _same(got, ref[key].to(device=like.device, dtype=like.dtype), key)
        # per-trajectory upstream weights
        J = q.trajectory_cost(md, xg, ug, targets=tr, weights=tw, model_phys=tp)
        gw2, gp2, gr2 = torch.autograd.grad((J * up).sum(), (tw, tp, tr))
        _same(gw2, (ref["grad_weights"] * up[:, None]).to(device=tw.device, dtype=tw.dtype), "weighted grad_weights")
        _same(gp2, (ref["grad_phys"] * up[:, None]).to(device=tp.device, dtype=tp.dtype), "weighted grad_phys")
        _same(gr2, (ref["grad_targets"] * up[:, None, None]).to(device=tr.device, dtype=tr.dtype), "weighted grad_targets")
    # one row alone, x0 and u constants; the (B, n) form of targets; the padded device forms of the C ABI
    tp = dev32(phys).requires_grad_(True)
    J = q.trajectory_cost(md, x0d, ud, targets=rows, weights=w, model_phys=tp)
    _same(torch.autograd.grad(J.sum(), (tp,))[0], ref["grad_phys"].float(), "phys alone")
    goal = dev32(rows[:, 0]).requires_grad_(True)
    J = q.trajectory_cost(md, x0d, ud, targets=goal)
    x_plain, _ = q.ops.simulate(md, x0d, ud)
    ref_goal = q.ops.cost_param_gradient(md, x_plain, ud, targets=rows[:, 0], want="targets")["grad_targets"]
    _same(torch.autograd.grad(J.sum(), (goal,))[0], ref_goal[:, 0].float(), "targets (B, n)")
    pad_w = q.ops.cost_rows_tensor(md, w, B, DEV).clone().requires_grad_(True)
    pad_p = q.ops.model_phys_tensor(md, phys, B, DEV).clone().requires_grad_(True)
    J = q.trajectory_cost(md, x0d, ud, targets=rows, weights=pad_w, model_phys=pad_p)
    gw, gp = torch.autograd.grad(J.sum(), (pad_w, pad_p))
    MX, n, m = q._lib.MAX_NX, md.n, md.m
    assert tuple(gw.shape) == (B, q.ops.COST_ROW_FLOATS) and tuple(gp.shape) == (B, 8)
    _same(torch.cat([gw[:, :n], gw[:, MX:MX + n], gw[:, 2 * MX:2 * MX + m]], dim=1), ref["grad_weights"].float(), "padded weights")
    _same(gp[:, :len(md.phys)].contiguous(), ref["grad_phys"].float(), "padded phys")
    pad = torch.ones(q.ops.COST_ROW_FLOATS, dtype=torch.bool, device=DEV)
    pad[:n] = pad[MX:MX + n] = pad[2 * MX:2 * MX + m] = False
    assert bool((gw[:, pad] == 0.0).all()) and bool((gp[:, len(md.phys):] == 0.0).all())


@pytest.mark.parametrize("model", pc.MODELS)
def test_autograd_without_row_gradients_is_todays_path(model):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", "euler")
    N, B = 7, pc.B_FULL[model]
    x0, u = pc.inputs(model, "skew", N)
    w, phys, rows = wc.weight_rows(model, B), gc.phys_rows(model, B), rc.skew_rows(model, B, 4)
    forms = (dict(), dict(targets=rows, weights=w, model_phys=phys), dict(targets=dev32(rows), weights=dev32(w), model_phys=dev32(phys)),
             dict(targets=rows, weights=dict(q=torch.as_tensor(w[:, :md.n]).requires_grad_(True))))
    for kw in forms:
        xg, ug = dev32(x0).requires_grad_(True), dev32(u).requires_grad_(True)
        J = q.trajectory_cost(md, xg, ug, **kw)
        assert type(J.grad_fn).__name__.startswith("_TrajectoryCostBackward"), type(J.grad_fn).__name__
        gx, gu = torch.autograd.grad(J.sum(), (xg, ug))
        with torch.no_grad():
            plain = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
            if isinstance(plain.get("weights"), dict):
                plain["weights"] = {k: v.detach() for k, v in plain["weights"].items()}
            if "model_phys" in kw:
                zK = torch.zeros((B, N, md.m, md.n), device=DEV)
                x, _ = q.ops.track(md, xg.detach(), torch.zeros((B, N + 1, md.n), device=DEV), ug.detach(), zK, N,
                                   plant_phys=plain["model_phys"], feedback=False)
            else:
                x, cost = q.ops.simulate(md, xg.detach(), ug.detach())
            if kw:
                _same(J.detach(), q.ops.score(md, x, ug.detach(), terminal=True, **plain)[0], "forward value")
            else:
                _same(J.detach(), cost, "forward value")
            ref = q.ops.cost_gradient(md, x, ug.detach(), **plain)
        _same(gu, ref["grad_u"], "grad_u")
        _same(gx, ref["grad_x0"], "grad_x0")


# ------------------------------------------------------------------------------------------------ 5. system identification
@pytest.mark.parametrize("integ", pg.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_one_gradient_step_on_model_phys_lowers_every_cost(model, integ):
    """pgrad_cases' use case: the log is the oracle's rollout under the true parameters, the loss is the trajectory cost against it
    under q alone, model_phys starts 0.8 .. 1.25 off per entry.  Step rule (pgrad_cases.sysid_descends): theta - s g with
    s = 0.25 min_k |theta_k / g_k|, halved until the fp64 cost of the oracle's rollout falls, at most 30 times; the fp64 reference
    gradient satisfies it on the CPU (tests/test_cost_param_gradient_cpu.py), the other sign never does."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    c = pg.sysid_case(model, integ)
    theta = dev32(c["theta"]).requires_grad_(True)
    J = q.trajectory_cost(md, dev32(c["x0"]), dev32(c["u"]), targets=dev32(c["log"]), weights=c["w"], model_phys=theta)
    g = torch.autograd.grad(J.sum(), (theta,))[0]
    assert g.dtype == torch.float32 and tuple(g.shape) == tuple(theta.shape)
    halvings = pg.sysid_descends(model, integ, c, g.double().cpu().numpy())
    print(f"[sysid {model} {integ}] halvings {halvings.tolist()}")
    assert np.all(halvings >= 0), halvings
