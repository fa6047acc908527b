"""The row gradients of USER-COMPILED models on the GPU (compile_model(..., param_grad=True): quattro_cost_param_gradient_f32 of the
model's library, ops.cost_param_gradient, the row gradients of autograd.trajectory_cost), the models of tests/upgrad_cases.py:
   1. grad_phys, grad_cost_rows and grad_ref_rows through the C entry (outputs pre-filled with NaN), fed the fp64 reference costate
      rounded to fp32, against the fp64 reference: both integrators, B in (1, 3), N in (1, 2, 9, 63, 64) -- at 63 the 64 slots fill one
      pass exactly, at 64 the terminal slot is alone in a second pass -- and R in (none, 1, 3, N + 1, N + 3), per-trajectory phys and
      weights; rows past the horizon and the padding are exactly +0.0; and through ops on the device's own costate;
   2. the quadrotor typed in again against the built-in quadrotor's ops.cost_param_gradient on the same inputs, within twice the bound;
   3. bit for bit: a row of a batch against the B = 1 call, each output alone against all three, NULL rows against neutral rows,
      heterogeneous rows against B calls on model.with_(...), a given costate against the two-launch form;
   4. the existing entries (simulate, linearize, one solve, cost_gradient) of the opt-in 4 x 4 grid library against the plain 4 x 4
      grid library, bit for bit: no existing behaviour changes;
   5. autograd's row gradients against ops.cost_param_gradient, with upstream weights;
   6. one gradient step on model_phys (upgrad_cases' step rule) lowers the fp64 cost of every trajectory of the (2, 1) model, the
      flipped sign lowers none.
The bound of 1 is upgrad_cases.gpu_bound: max(4 E, 2e-6), E the fp32 restatement's distance measured on the CPU; every measured value
is printed before it is asserted.

Measured on one MI355X, worst over the shapes of 1 (Euler / RK4): grad_phys 1.1e-7 / 2.0e-7 (grid 1 x 1), 1.0e-7 / 8.6e-8 (4 x 4),
7.8e-8 / 1.1e-7 (16 x 8), 4.6e-7 / 2.6e-7 (quadrotor), 1.1e-7 / 1.3e-7 (probe); grad_weights <= 2.5e-7, grad_targets <= 2.6e-7; the
quadrotor typed in again against the built-in kernel: grad_phys <= 4.8e-8, weights and targets equal."""
import ctypes

import numpy as np
import pytest

import upgrad_cases as U
import user_grid_cases as g

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("grad_phys", "grad_weights", "grad_targets")
CASES = [(name, integ) for name in U.NAMES for integ in U.INTEGRATORS]


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


def _positive_zero(a):
    return bool(np.all(a == 0.0) and not np.any(np.signbit(a)))


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
    assert status == 0, status          # QUATTRO_OK
    torch.cuda.synchronize()
    return gp.cpu().numpy(), gw.cpu().numpy(), gr.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name,integ", CASES)
def test_c_entry_matches_the_fp64_reference(name, integ):
    q = _pkg()
    model = U.MODELS[name]
    md = model.device(integ)
    n, m, NP, MX = md.n, md.m, len(md.phys), q._lib.MAX_NX
    bound = U.gpu_bound(name)
    bad, worst = [], {}
    for N in U.HORIZONS:
        for R in U.ref_counts(N):
            c = U.case(name, integ, N, R)
            ref = U.reference(model, c["blks"], integ, c["x"], c["u"], c["lam"], rows=c["rows"])
            P, w, rows = U.row_arrays(c)
            for B in U.BATCHES:
                gp, gw, gr = c_entry(md, c["x"][:B], c["u"][:B], c["lam"][:B], phys=P[:B], rows=None if rows is None else rows[:B], w=w[:B])
                got = dict(grad_phys=gp[:, :NP], grad_weights=np.concatenate([gw[:, :n], gw[:, MX:MX + n], gw[:, 2 * MX:2 * MX + m]], axis=1),
                           grad_targets=gr)
                errs = U.errors(got, {k: v[:B] for k, v in ref.items()})
                worst = {k: max(e, worst.get(k, 0.0)) for k, e in errs.items()}
                bad += [(N, R, B, k, e) for k, e in errs.items() if not e < bound]
                # padding and rows past the horizon: exactly +0.0
                assert _positive_zero(gp[:, NP:]), (N, R, B)
                assert _positive_zero(gw[:, n:MX]) and _positive_zero(gw[:, MX + n:2 * MX]) and _positive_zero(gw[:, 2 * MX + m:]), (N, R, B)
                if R is not None and R > N + 1:
                    assert _positive_zero(gr[:, N + 1:]), (N, R, B)
    print(f"[upgrad {name} {integ}] worst " + " ".join(f"{k} {e:.1e}" for k, e in worst.items()) + f" (bound {bound:.1e})")
    assert not bad, (bound, bad)


@pytest.mark.parametrize("name,integ", CASES)
def test_ops_matches_the_fp64_reference_on_the_devices_own_costate(name, integ):
    q = _pkg()
    model = U.MODELS[name]
    md = model.device(integ)
    bound = U.gpu_bound(name)
    for N, R, hetero in ((9, 3, True), (9, None, False), (64, 65, True)):
        c = U.case(name, integ, N, R, hetero=hetero)
        ref = U.reference(model, c["blks"], integ, c["x"], c["u"], c["lam"], rows=c["rows"])
        P, w, rows = U.row_arrays(c) if hetero else (None, None, None)
        got = q.ops.cost_param_gradient(md, dev32(c["x"]), dev32(c["u"]), targets=rows, weights=w, model_phys=P)
        assert set(got) == set(KEYS) and all(v.dtype == torch.float64 and v.is_cuda for v in got.values())
        B = c["u"].shape[0]
        assert tuple(got["grad_phys"].shape) == (B, model.NP) and tuple(got["grad_weights"].shape) == (B, 2 * md.n + md.m)
        assert tuple(got["grad_targets"].shape) == (B, 1 if rows is None else rows.shape[1], md.n)
        errs = U.errors(host(got), ref)
        print(f"[upgrad ops {name} {integ}] N={N} R={R}: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert U.worst(errs) < bound, (N, R, errs, bound)


# ------------------------------------------------------------------------------------------------ 2. the quadrotor, twice
@pytest.mark.parametrize("integ", U.INTEGRATORS)
def test_the_quadrotor_typed_in_again_agrees_with_the_builtin_kernel(integ):
    import param_cases as pc
    q = _pkg()
    user, builtin = U.MODELS["quad"].device(integ), pc.device_model(q.models, "quadrotor", "skew", integ)
    bound = 2.0 * U.gpu_bound("quad")
    for N, R in ((9, 3), (64, 65), (2, None)):
        c = U.case("quad", integ, N, R)
        ref = U.reference(c["model"], c["blks"], integ, c["x"], c["u"], c["lam"], rows=c["rows"])
        P, w, rows = U.row_arrays(c)
        xd, ud, lam = dev32(c["x"]), dev32(c["u"]), dev32(c["lam"])
        a = q.ops.cost_param_gradient(user, xd, ud, targets=rows, weights=w, model_phys=P, costate=lam)
        b = q.ops.cost_param_gradient(builtin, xd, ud, targets=rows, weights=w, model_phys=P, costate=lam)
        # one against the other under the reference's measure: the built-in result in the place of the reference's values
        errs = U.errors(host(a), dict(ref, **host(b)))
        print(f"[upgrad quad vs built-in {integ}] N={N} R={R}: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert U.worst(errs) < bound, (N, R, errs, bound)


# ------------------------------------------------------------------------------------------------ 3. identities
def _with(md, blk=None, keys=(), xref=None):
    kw = {}
    if "weights" in keys:
        kw.update(q=tuple(map(float, blk["q"])), qf=tuple(map(float, blk["qf"])), r=tuple(map(float, blk["r"])))
    if "model_phys" in keys:
        kw["phys"] = tuple(map(float, blk["P"]))
    if xref is not None:
        kw["x_ref"] = tuple(map(float, xref))
    return md.with_(**kw)


@pytest.mark.parametrize("name,integ", [(name, integ) for name in ("grid4x4", "probe", "grid16x8") for integ in U.INTEGRATORS])
def test_identities_bit_for_bit(name, integ):
    q = _pkg()
    pgrad, grad = q.ops.cost_param_gradient, q.ops.cost_gradient
    md = U.MODELS[name].device(integ)
    for N in (9, 64):
        c = U.case(name, integ, N, 3)
        B = c["u"].shape[0]
        xd, ud = dev32(c["x"]), dev32(c["u"])
        phys, w, rows = U.row_arrays(c)
        het = dict(targets=rows, weights=w, model_phys=phys)
        lam = grad(md, xd, ud, want_costate=True, **het)["costate"]
        full = pgrad(md, xd, ud, **het)
        given = pgrad(md, xd, ud, costate=lam, **het)
        for key in KEYS:
            _same(given[key], full[key], f"given costate {key}")
        for want in ("phys", "weights", "targets"):
            alone = pgrad(md, xd, ud, want=(want,), **het)
            assert set(alone) == {"grad_" + want}
            _same(alone["grad_" + want], full["grad_" + want], f"{want} alone")
        for b in range(B):
            one = pgrad(md, xd[b:b + 1].contiguous(), ud[b:b + 1].contiguous(), targets=rows[b:b + 1], weights=w[b:b + 1],
                        model_phys=phys[b:b + 1])
            for key in KEYS:
                _same(one[key], full[key][b:b + 1], f"row {b} {key}")
        if N != 9:
            continue
        plain = pgrad(md, xd, ud)
        neutral = dict(targets=np.tile(np.asarray(md.x_ref, dtype=np.float32), (B, 1, 1)),
                       weights=np.tile(np.concatenate([md.q, md.qf, md.r]).astype(np.float32), (B, 1)),
                       model_phys=np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1)))
        for keys in (("targets",), ("weights",), ("model_phys",), ("targets", "weights", "model_phys")):
            got = pgrad(md, xd, ud, **{k: neutral[k] for k in keys})
            for key in KEYS:
                _same(got[key], plain[key], f"neutral {keys} {key}")
        goal = rows[:, 2]
        het1 = dict(targets=goal, weights=w, model_phys=phys)
        for keys in (("targets",), ("weights",), ("model_phys",), ("targets", "weights", "model_phys")):
            got = pgrad(md, xd, ud, **{k: het1[k] for k in keys})
            for b in range(B):
                mb = _with(md, c["blks"][b], keys, goal[b] if "targets" in keys else None)
                one = pgrad(mb, xd[b:b + 1].contiguous(), ud[b:b + 1].contiguous())
                for key in KEYS:
                    _same(one[key], got[key][b:b + 1], f"heterogeneous {keys} b={b} {key}")
        assert not torch.equal(full["grad_phys"], plain["grad_phys"])


# ------------------------------------------------------------------------------------------------ 4. nothing else changes
@pytest.mark.parametrize("integ", U.INTEGRATORS)
def test_existing_entries_of_the_opt_in_library_are_the_plain_librarys_bits(integ):
    q = _pkg()
    opt, plain = U.MODELS["grid4x4"].device(integ), g.model(4, 4, "convex", integ)
    assert opt.param_grad and not plain.param_grad and opt.lib_path != plain.lib_path
    assert opt.with_(name=plain.name, lib_path=plain.lib_path, source=plain.source, param_grad=False) == plain    # the same problem
    N, B = 9, 3
    x0, u = U.MODELS["grid4x4"].inputs(N, B)
    x0d, ud = dev32(x0), dev32(u)
    out = {}
    for tag, md in (("opt", opt), ("plain", plain)):
        x, cost = q.ops.simulate(md, x0d, ud)
        lin = q.ops.linearize(md, x, ud)
        lin = lin if isinstance(lin, (tuple, list)) else (lin,)
        gr = q.ops.cost_gradient(md, x, ud, want_costate=True)
        sol = q.QuattroILQR(md, horizon=N, tf_window=4, device=DEV).solve(x0, u, max_iter=1)
        out[tag] = dict(x=x, cost=cost, **{f"lin{i}": t for i, t in enumerate(lin) if isinstance(t, torch.Tensor)},
                        **{"g_" + k: v for k, v in gr.items()},
                        **{"s_" + k: v for k, v in sol.items() if isinstance(v, torch.Tensor)})
    assert set(out["opt"]) == set(out["plain"]) and {"x", "cost", "lin0", "g_grad_u", "g_costate", "s_K", "s_k"} <= set(out["opt"])
    for key in out["opt"]:
        _same(out["opt"][key], out["plain"][key], key)


# ------------------------------------------------------------------------------------------------ 5. autograd
@pytest.mark.parametrize("name,integ", [("probe", "euler"), ("grid4x4", "rk4")])
def test_autograd_row_gradients_are_the_kernel(name, integ):
    q = _pkg()
    model = U.MODELS[name]
    md = model.device(integ)
    N, B = 9, U.B_FULL
    c = U.case(name, integ, N, 4)
    phys, w, rows = U.row_arrays(c)
    x0d, ud = dev32(c["x0"]), dev32(c["u"])
    zK = torch.zeros((B, N, md.m, md.n), device=DEV)
    x, _ = q.ops.track(md, x0d, torch.zeros((B, N + 1, md.n), device=DEV), ud, zK, N, plant_phys=phys, feedback=False)
    ref = q.ops.cost_param_gradient(md, x, ud, targets=rows, weights=w, model_phys=phys)
    base = q.ops.cost_gradient(md, x, ud, targets=rows, weights=w, model_phys=phys)
    up = torch.linspace(0.5, 2.0, B, device=DEV, dtype=torch.float64)
    for make in (lambda a: dev32(a).requires_grad_(True), lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).requires_grad_(True)):
        tw, tp, tr = make(w), make(phys), make(rows)
        xg, ug = dev32(c["x0"]).requires_grad_(True), dev32(c["u"]).requires_grad_(True)
        J = q.trajectory_cost(md, xg, ug, targets=tr, weights=tw, model_phys=tp)
        gx, gu, gw, gp, gr = torch.autograd.grad(J.sum(), (xg, ug, tw, tp, tr))
        _same(gu, base["grad_u"], "grad_u")
        _same(gx, base["grad_x0"], "grad_x0")
        for got, like, key in ((gw, tw, "grad_weights"), (gp, tp, "grad_phys"), (gr, tr, "grad_targets")):
            assert got.shape == like.shape and got.dtype == like.dtype and got.device == like.device, key
            _same(got, ref[key].to(device=like.device, dtype=like.dtype), key)
        J = q.trajectory_cost(md, xg, ug, targets=tr, weights=tw, model_phys=tp)
        gw2, gp2, gr2 = torch.autograd.grad((J * up).sum(), (tw, tp, tr))
        _same(gw2, (ref["grad_weights"] * up[:, None]).to(device=tw.device, dtype=tw.dtype), "weighted grad_weights")
        _same(gp2, (ref["grad_phys"] * up[:, None]).to(device=tp.device, dtype=tp.dtype), "weighted grad_phys")
        _same(gr2, (ref["grad_targets"] * up[:, None, None]).to(device=tr.device, dtype=tr.dtype), "weighted grad_targets")


# ------------------------------------------------------------------------------------------------ 6. the use case
@pytest.mark.parametrize("integ", U.INTEGRATORS)
def test_one_gradient_step_on_model_phys_lowers_every_cost(integ):
    """upgrad_cases' use case on the (2, 1) model: the log is the fp64 rollout under the model's own parameters, the loss the
    trajectory cost against it, model_phys starts 0.8 .. 1.25 off per entry.  theta - s g with s = 0.25 min_k |theta_k / g_k|, halved
    until the fp64 cost of the rollout falls, at most 30 times; the flipped sign never lowers it."""
    q = _pkg()
    md = U.MODELS["probe"].device(integ)
    c = U.sysid_case("probe", integ)
    theta = dev32(c["theta"]).requires_grad_(True)
    J = q.trajectory_cost(md, dev32(c["x0"]), dev32(c["u"]), targets=dev32(c["log"]), model_phys=theta)
    grad = torch.autograd.grad(J.sum(), (theta,))[0]
    assert grad.dtype == torch.float32 and tuple(grad.shape) == tuple(theta.shape)
    gn = grad.double().cpu().numpy()
    down, up = U.sysid_descends(c, integ, gn), U.sysid_descends(c, integ, -gn)
    print(f"[upgrad sysid {integ}] halvings {down.tolist()} flipped {up.tolist()}")
    assert np.all(down >= 0) and np.all(up < 0), (down, up)
