"""The cost gradient on the GPU (quattro_cost_gradient_f32, ops.cost_gradient, autograd.trajectory_cost, solve(want_grad=True)):
   1. grad_u, grad_x0 and costate against the fp64 adjoint, built-in models, both integrators, every set of grad_cases.SETS, B in
      param_cases.BATCHES (the ragged last wave), N in (1, 7, 26) and one below, at and one above the kernel's LDS block length;
   2. the same for user-compiled models at the grid points of grad_cases.USER_POINTS (every lanes-per-item), N in (1, 2, 9), B in (1, 3);
   3. bit-for-bit identities: a row of a batch against the B = 1 call, NULL outputs, neutral rows, heterogeneous rows against
      separate calls on model.with_(...), the row rule step by step against the single row, lambda_0 == costate[:, 0];
   4. heterogeneous weights, targets and model_phys together against the fp64 adjoint of every trajectory's own problem;
   5. autograd: gradients and values of trajectory_cost against ops.cost_gradient / ops.simulate / ops.score, and a descent step;
   6. solve(want_grad=True) against ops.cost_gradient, the fp64 adjoint and the gradient norm at the initial controls.
The bound of 1, 2, 4 and 6 is grad_cases.gpu_bound: the larger of 4 x E (the fp32 restatement's distance from fp64, measured on the
CPU) and the project's fp32 floor 2e-6; every measured value is printed before it is asserted.  Reference, measures, mutants:
tests/grad_cases.py, tests/test_cost_gradient_cpu.py."""
import numpy as np
import pytest

import grad_cases as gc
import param_cases as pc
import ref_cases as rc
import weight_cases as wc
from oracle import linearize as o_lin

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BUILTIN = [(model, s, integ) for model in pc.MODELS for s in gc.SETS[model] for integ in gc.INTEGRATORS]


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def host(out):
    return {key: v.double().cpu().numpy() for key, v in out.items()}


def _same(a, b, tag):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b), tag


def _horizons():
    from quattro_ilqr_amd import _lib
    gb = _lib.GRAD_BLOCK
    return tuple(sorted(set(pc.HORIZONS) | {gb - 1, gb, gb + 1}))        # 7 and 26 span three and nine blocks


# ------------------------------------------------------------------------------------------------ 1. parity, built-in models
@pytest.mark.parametrize("model,set_name,integ", BUILTIN)
def test_gradient_matches_the_fp64_adjoint(model, set_name, integ):
    q = _pkg()
    md = pc.device_model(q.models, model, set_name, integ)
    spec = pc.spec(model, set_name, integ)
    bound = gc.gpu_bound(model)
    bad = []
    for N in _horizons():
        x, u = gc.nominal(model, set_name, integ, N)
        d = gc.blocks(spec, x, u)
        ref = gc.adjoint(d)
        for B in pc.BATCHES[model]:
            got = host(q.ops.cost_gradient(md, dev32(x[:B]), dev32(u[:B]), want_costate=True))
            errs = gc.errors(got, {k: v[:B] for k, v in ref.items()}, {k: v[:B] for k, v in d.items()})
            print(f"[grad {model} {set_name} {integ}] N={N} B={B}: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
            bad += [(N, B, k, e) for k, e in errs.items() if not e < bound]
    assert not bad, (bound, bad)


# ------------------------------------------------------------------------------------------------ 2. parity, user models
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("point", gc.USER_POINTS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_user_model_gradient_matches_the_fp64_adjoint(point, integ):
    import user_grid_cases as g
    q = _pkg()
    n, m = point
    md = g.model(n, m, "convex", integ)
    bound = max(4.0 * gc.USER_E, gc.FLOOR)
    bad = []
    for N in g.HORIZONS:
        for B in g.BATCHES:
            x, u, d, ref = gc.user_reference(n, m, integ, N, B)
            got = host(q.ops.cost_gradient(md, dev32(x), dev32(u), want_costate=True))
            errs = gc.errors(got, ref, d)
            print(f"[grad user {n}x{m} {integ}] N={N} B={B}: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
            bad += [(N, B, k, e) for k, e in errs.items() if not e < bound]
    assert not bad, (bound, bad)


# ------------------------------------------------------------------------------------------------ 3. identities
def _identity_case(name, integ):
    """-> (DeviceModel, x (B, N+1, n), u (B, N, m) fp32 arrays, weights (B, 2n+m), phys (B, len(phys)), base x_ref)."""
    q = _pkg()
    N = 7
    if name == "user":
        import user_grid_cases as g
        n, m = 12, 4
        md = g.model(n, m, "convex", integ)
        B = max(g.BATCHES)
        x = gc.f32(g.evaluate(n, m, "convex", integ, N, B)["sim_x"])
        _, u = g.inputs(n, m, "convex", N, B)
        w = wc.rows_about(np.concatenate([md.q, md.qf, md.r]), B)
        f = np.exp(np.random.default_rng(23).uniform(np.log(0.8), np.log(1.25), (B, len(md.phys))))
        phys = (np.asarray(md.phys)[None, :] * f).astype(np.float32)
        rows = (np.asarray(md.x_ref)[None, None, :] + 0.05 * np.random.default_rng(29).standard_normal((B, N + 1, n))).astype(np.float32)
    else:
        md = pc.device_model(q.models, name, "skew", integ)
        B = pc.B_FULL[name]
        x, u = gc.nominal(name, "skew", integ, N)
        w, phys, rows = wc.weight_rows(name, B), gc.phys_rows(name, B), rc.skew_rows(name, B, N + 1)
    return md, x.astype(np.float32), u.astype(np.float32), w, phys, rows


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


@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("name", ("cartpole", "quadrotor", "user"))
def test_gradient_identities_bit_for_bit(name, integ):
    q = _pkg()
    grad = q.ops.cost_gradient
    md, x, u, w, phys, rows = _identity_case(name, integ)
    B, N = u.shape[:2]
    xd, ud = dev32(x), dev32(u)
    full = grad(md, xd, ud, want_costate=True)
    _same(full["grad_x0"], full["costate"][:, 0].contiguous(), "lambda_0 is costate[:, 0]")
    # NULL outputs
    _same(grad(md, xd, ud, want_x0=False)["grad_u"], full["grad_u"], "grad_u without grad_x0")
    only = grad(md, xd, ud, want_x0=False, want_costate=False)
    assert set(only) == {"grad_u"}
    _same(grad(md, xd, ud, want_x0=True, want_costate=False)["grad_x0"], full["grad_x0"], "grad_x0 without costate")
    # a row of the batch is the B = 1 call
    for b in sorted({0, B // 2, B - 1}):
        one = grad(md, xd[b:b + 1].contiguous(), ud[b:b + 1].contiguous(), want_costate=True)
        for key in full:
            _same(one[key], full[key][b:b + 1], f"row {b} {key}")
    # neutral rows are no rows
    neutral = dict(targets=rc.neutral_rows(md.x_ref, B, 3), weights=np.tile(np.concatenate([md.q, md.qf, md.r]).astype(np.float32), (B, 1)),
                   model_phys=np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1)))
    for keys in (("targets",), ("weights",), ("model_phys",), ("targets", "weights", "model_phys")):
        got = grad(md, xd, ud, want_costate=True, **{k: neutral[k] for k in keys})
        for key in full:
            _same(got[key], full[key], f"neutral {keys} {key}")
    # heterogeneous rows against separate calls on with_(): one goal per trajectory (R = 1) is with_(x_ref=row)
    goal = rows[:, N]
    het = dict(targets=goal, weights=w, model_phys=phys)
    for keys in (("targets",), ("weights",), ("model_phys",), ("targets", "weights", "model_phys")):
        got = grad(md, xd, ud, want_costate=True, **{k: het[k] for k in keys})
        for b in range(B):
            mb = _with(md, w[b] if "weights" in keys else None, phys[b] if "model_phys" in keys else None,
                       goal[b] if "targets" in keys else None)
            one = grad(mb, xd[b:b + 1].contiguous(), ud[b:b + 1].contiguous(), want_costate=True)
            for key in got:
                _same(one[key], got[key][b:b + 1], f"heterogeneous {keys} b={b} {key}")
    # a window of rows: the batch against B = 1 calls with the trajectory's window, and R = 3 rows (the last held) against the
    # N + 1 rows they stand for
    got = grad(md, xd, ud, want_costate=True, targets=rows, weights=w, model_phys=phys)
    for b in range(B):
        one = grad(md, xd[b:b + 1].contiguous(), ud[b:b + 1].contiguous(), want_costate=True, targets=rows[b:b + 1],
                   weights=w[b:b + 1], model_phys=phys[b:b + 1])
        for key in got:
            _same(one[key], got[key][b:b + 1], f"window b={b} {key}")
    # the row rule step by step, against the single row: a window that follows goal A up to step k - 1 and goal B from step k on
    # (R = k + 1 rows, the last one held) must give, from step k on, the costate of the R = 1 call on goal B -- which the loop
    # above showed to be with_(x_ref=B) -- and its grad_u from step k - 1 on (g_t reads lambda_{t+1}); below that they differ
    goal_a = rows[:, 0]
    single = grad(md, xd, ud, want_costate=True, targets=goal)
    for k in range(N + 1):
        win = np.concatenate([np.repeat(goal_a[:, None, :], k, axis=1), goal[:, None, :]], axis=1)
        stepped = grad(md, xd, ud, want_costate=True, targets=win)
        _same(stepped["costate"][:, k:], single["costate"][:, k:], f"rows differ below step {k}: costate from {k} on")
        _same(stepped["grad_u"][:, max(k - 1, 0):], single["grad_u"][:, max(k - 1, 0):], f"rows differ below step {k}: grad_u")
        if k > 0:
            assert not torch.equal(stepped["costate"][:, k - 1], single["costate"][:, k - 1]), k
    short = grad(md, xd, ud, want_costate=True, targets=rows[:, :3])
    held = grad(md, xd, ud, want_costate=True, targets=rc.window(rows[:, :3], N))
    for key in short:
        _same(short[key], held[key], f"held row {key}")
    assert not torch.equal(short["grad_u"], full["grad_u"]) and not torch.equal(got["grad_u"], short["grad_u"])


# ------------------------------------------------------------------------------------------------ 4. rows against fp64
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_rows_match_the_fp64_adjoint_of_each_trajectory(model, integ):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    N, B, R = 7, pc.B_FULL[model], 4
    x0, u = pc.inputs(model, "skew", N)
    w, phys, rows = wc.weight_rows(model, B), gc.phys_rows(model, B), rc.skew_rows(model, B, R)
    win = rc.window(rows.astype(np.float64), N)
    bound = gc.gpu_bound(model)
    for keys in (("weights",), ("targets",), ("model_phys",), ("weights", "targets", "model_phys")):
        specs = [pc.spec_from(model, gc.params_with(model, w[b] if "weights" in keys else None,
                                                    phys[b] if "model_phys" in keys else None), integ) for b in range(B)]
        x = gc.f32(np.concatenate([o_lin.rollout_batched(sp, x0[b:b + 1], u[b:b + 1])[0] for b, sp in enumerate(specs)]))
        d = gc.blocks_per_trajectory(specs, x, u, win if "targets" in keys else None)
        ref = gc.adjoint(d)
        kw = dict(weights=w, targets=rows, model_phys=phys)
        got = host(q.ops.cost_gradient(md, dev32(x), dev32(u), want_costate=True, **{k: kw[k] for k in keys}))
        errs = gc.errors(got, ref, d)
        print(f"[grad rows {model} {integ}] {'+'.join(keys)}: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert gc.worst(errs) < bound, (keys, errs, bound)


# ------------------------------------------------------------------------------------------------ 5. autograd
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_autograd_is_the_gradient_kernel(model, integ):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    N, B = 7, pc.B_FULL[model]
    x0, u = pc.inputs(model, "skew", N)
    w, phys, rows = wc.weight_rows(model, B), gc.phys_rows(model, B), rc.skew_rows(model, B, 4)
    for kw in (dict(), dict(targets=rows, weights=w), dict(targets=rows, weights=w, model_phys=phys)):
        x0d, ud = dev32(x0).requires_grad_(True), dev32(u).requires_grad_(True)
        J = q.trajectory_cost(md, x0d, ud, **kw)
        assert J.dtype == torch.float64 and tuple(J.shape) == (B,)
        gx, gu = torch.autograd.grad(J.sum(), (x0d, ud))
        with torch.no_grad():
            if "model_phys" in kw:
                zK = torch.zeros((B, N, md.m, md.n), device=DEV)
                x, _ = q.ops.track(md, x0d.detach(), torch.zeros((B, N + 1, md.n), device=DEV), ud.detach(), zK, N,
                                   plant_phys=phys, feedback=False)
            else:
                x, cost = q.ops.simulate(md, x0d.detach(), ud.detach())
            if kw:
                _same(J.detach(), q.ops.score(md, x, ud.detach(), terminal=True, **kw)[0], "forward value is ops.score's total")
            else:
                _same(J.detach(), cost, "forward value is ops.simulate's cost")
            ref = q.ops.cost_gradient(md, x, ud.detach(), **kw)
        _same(gu, ref["grad_u"], "autograd grad_u")
        _same(gx, ref["grad_x0"], "autograd grad_x0")
        # per-trajectory upstream weights
        up = torch.linspace(0.5, 2.0, B, device=DEV, dtype=torch.float64)
        J = q.trajectory_cost(md, x0d, ud, **kw)
        gx2, gu2 = torch.autograd.grad((J * up).sum(), (x0d, ud))
        _same(gu2, ref["grad_u"] * up.float()[:, None, None], "weighted grad_u")
        _same(gx2, ref["grad_x0"] * up.float()[:, None], "weighted grad_x0")
        # u alone
        J = q.trajectory_cost(md, x0d.detach(), ud, **kw)
        _same(torch.autograd.grad(J.sum(), (ud,))[0], ref["grad_u"], "grad_u with a constant x0")


@pytest.mark.parametrize("integ", gc.INTEGRATORS)
def test_one_gradient_step_lowers_every_cost(integ):
    """Cart-pole, skew set, N = 26: u - s grad_u with s halved from 1 until the fp64 cost of the oracle's rollout falls, per
    trajectory; a descent direction must get there (within 40 halvings: s >= 1e-12)."""
    q = _pkg()
    md = pc.device_model(q.models, "cartpole", "skew", integ)
    spec = pc.spec("cartpole", "skew", integ)
    x0, u = pc.inputs("cartpole", "skew", 26)
    x0d, ud = dev32(x0), dev32(u).requires_grad_(True)
    g = torch.autograd.grad(q.trajectory_cost(md, x0d, ud).sum(), (ud,))[0].double().cpu().numpy()
    J0 = o_lin.rollout_batched(spec, x0, u)[1]
    for b in range(u.shape[0]):
        s, ok = 1.0, False
        for _ in range(40):
            if o_lin.rollout_batched(spec, x0[b:b + 1], u[b:b + 1] - s * g[b:b + 1])[1][0] < J0[b]:
                ok = True
                break
            s *= 0.5
        print(f"[descent cartpole {integ}] b={b}: step {s:.2e}")
        assert ok, b


# ------------------------------------------------------------------------------------------------ 6. solver
def _solve_case(model, integ):
    """The cases tests/test_cost_gradient_cpu.py checks the oracle's solves on -> (md, spec builder per trajectory, N, x0, u0, kw of
    solve, window or None, weights or None)."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    if model == "cartpole":
        N, B = wc.N, wc.B["cartpole"]
        x0, u0 = rc.inputs(model, N, B)
        rows = wc.weight_rows(model)
        return md, N, x0, u0, dict(weights=rows), None, rows
    from test_ref_rows_cpu import REF_B
    N, B = pc.SOLVE_N, REF_B[model]
    x0, u0 = pc.inputs(model, "skew", N, B)
    rows = rc.skew_rows(model, B, N + 1)
    return md, N, x0, u0, dict(targets=rows), rc.window(rows.astype(np.float64), N), None


@pytest.mark.parametrize("model,integ", [("cartpole", "euler"), ("cartpole", "rk4"), ("quadrotor", "euler"), ("quadrotor", "rk4")])
def test_solve_want_grad(model, integ):
    q = _pkg()
    md, N, x0, u0, kw, win, w = _solve_case(model, integ)
    B = x0.shape[0]
    mk = lambda: q.QuattroILQR(md, N, max_iter=pc.SOLVE_MAX_ITER, tol=pc.SOLVE_TOL, device=DEV, tf_window=0)
    out = mk().solve(x0, u0, want_grad=True, **kw)
    assert int(out["status"].abs().sum()) == 0
    assert tuple(out["grad_u"].shape) == (B, N, md.m) and tuple(out["grad_norm"].shape) == (B,)
    ref = q.ops.cost_gradient(md, out["x"], out["u"], want_x0=False, **kw)
    _same(out["grad_u"], ref["grad_u"], "solve's grad_u is ops.cost_gradient on the returned x, u")
    _same(out["grad_norm"], ref["grad_u"].abs().amax(dim=(1, 2)), "grad_norm")
    # against the fp64 adjoint about the returned point
    x, u = out["x"].double().cpu().numpy(), out["u"].double().cpu().numpy()
    specs = [pc.spec_from(model, gc.params_with(model, None if w is None else w[b]), integ) for b in range(B)]
    d = gc.blocks_per_trajectory(specs, x, u, win)
    errs = gc.errors(dict(grad_u=out["grad_u"].double().cpu().numpy()), gc.adjoint(d), d)
    print(f"[solve grad {model} {integ}] grad_u {errs['grad_u']:.1e}")
    assert errs["grad_u"] < gc.gpu_bound(model), errs
    # the measure: below the norm at the initial controls, every trajectory
    x_init, _ = q.ops.simulate(md, dev32(x0), dev32(u0))
    g0 = q.ops.cost_gradient(md, x_init, dev32(u0), want_x0=False, **kw)["grad_u"].abs().amax(dim=(1, 2))
    print(f"[solve grad {model} {integ}] grad_norm {out['grad_norm'].tolist()} at the initial controls {g0.tolist()}")
    assert bool((out["grad_norm"] < g0).all())
    # without the keyword: the old dict, and the same solve
    plain = mk().solve(x0, u0, **kw)
    assert set(plain) == set(out) - {"grad_u", "grad_norm"}
    for key in plain:
        _same(plain[key], out[key], key)


@pytest.mark.parametrize("model", pc.MODELS)
def test_solve_want_grad_without_rows(model):
    """The host-driven and default paths (no rows): the same identity."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", "euler")
    N = pc.SOLVE_N
    x0, u0 = pc.inputs(model, "skew", N, 3)
    for extra in (dict(), dict(device_loop=False)):
        out = q.QuattroILQR(md, N, max_iter=5, tol=pc.SOLVE_TOL, device=DEV, tf_window=0, **extra).solve(x0, u0, want_grad=True)
        ref = q.ops.cost_gradient(md, out["x"], out["u"], want_x0=False)
        _same(out["grad_u"], ref["grad_u"], f"grad_u {extra}")
        _same(out["grad_norm"], ref["grad_u"].abs().amax(dim=(1, 2)), f"grad_norm {extra}")
