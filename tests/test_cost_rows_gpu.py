"""Per-trajectory cost weights (quattro_ilqr_solve_cost_f32, quattro_mpc_run_cost_f32; `weights=` of QuattroILQR.solve,
BatchedMPC.control_step and BatchedMPC.run) on the GPU:
   5. neutral rows (the model's own q, qf, r in every row) leave what the call without them leaves, bit for bit;
   6. NULL rows are the entry each extends;
   7. heterogeneous rows: B solvers built on model.with_(q=, qf=, r=) through the plain path, bit for bit, log ring too; with
      model_phys, with targets and with both against per-trajectory calls with B = 1;
   8. the closed loop in one launch against B runs of one controller each, bit for bit;
   9. the first iteration of every row against the fp64 oracle on that row's spec;
  10. the converged solve of every trajectory against oracle.ilqr.optimize on its own spec;
  11. the modes without a device-resident loop refuse.
The cart-pole (both integrators, B = 5, N = 20) and the planar user model (its prebuilt RK4 library, B = 3, N = 12): the models whose
persistent kernels take cost rows.  The built-in quadrotor's refuses them (tests/test_cost_rows_cpu.py).
Shapes, inputs, the rows and their well-posedness: tests/weight_cases.py, tests/test_cost_rows_cpu.py."""
import numpy as np
import pytest

import param_cases as pc
import ref_cases as rc
import weight_cases as wc
from conftest import GOLDEN, rel_fro
from test_model_phys_cpu import phys_rows

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SOLVE_KEYS = ("x", "u", "K", "k", "cost", "iters", "alpha", "status")
KW = dict(max_iter=40, tol=1e-3, device=DEV, tf_window=0)
ALL = wc.CASES + [("planar", "rk4")]
RUN_STEPS = 6


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def f64(t):
    return t.double().cpu().numpy()


def _snap(out):
    return {k_: v.clone() for k_, v in out.items()}


def _case(model, integ, N=wc.N):
    """-> (name, DeviceModel, N, x0, u0, solver keywords, rows (B, 2n + m) float32).  The planar user model (n = 6, m = 2; its
    prebuilt RK4 library) runs B = 3, N = 12 through its persistent kernel, which rows take without being asked."""
    q = _pkg()
    if model == "planar":
        from test_user_model_gpu import planar_batch, planar_model
        x0, u0 = planar_batch(wc.B["planar"], wc.N_PLANAR, 5)
        md = planar_model(integ)
        rows = wc.rows_about(np.concatenate([md.q, md.qf, md.r]), wc.B["planar"])
        return "planar", md, wc.N_PLANAR, x0.astype(np.float32).astype(np.float64), u0, dict(device_loop="always"), rows
    x0, u0 = rc.inputs(model, N, wc.B[model])
    return model, pc.device_model(q.models, model, "skew", integ), N, x0, u0, {}, wc.weight_rows(model)


def _own(md, B):
    """(B, 2n + m): the model's own weights in every row."""
    return np.tile(np.concatenate([md.q, md.qf, md.r]).astype(np.float32), (B, 1))


def _with_row(md, row):
    qv, qf, r = wc.split((md.n, md.m), row)
    return md.with_(q=tuple(map(float, qv)), qf=tuple(map(float, qf)), r=tuple(map(float, r)))


def _phys(model, md, B):
    if model == "planar":          # the planar model's free parameters, the mass scaled per trajectory
        phys = np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1))
        phys[:, 0] *= (1.0 + 0.2 * np.sin(1.0 + np.arange(B))).astype(np.float32)
        return phys
    return phys_rows(model, B)


def _equal(a, b, keys=SOLVE_KEYS, tag=()):
    for key in keys:
        assert torch.equal(a[key], b[key]), (*tag, key)


# ------------------------------------------------------------------------------------------------ 5. neutral rows
def _assert_neutral(md, N, x0, u0, max_iter, steps=RUN_STEPS, skw={}):
    q = _pkg()
    B = x0.shape[0]
    kw = dict(KW, max_iter=max_iter, **skw)
    a, b = q.QuattroILQR(md, N, **kw), q.QuattroILQR(md, N, **kw)
    ob = _snap(b.solve(x0, u0))
    own = _own(md, B)
    n = md.n
    for form in (own, {}, dict(q=own[0, :n]), dict(qf=own[:, n:2 * n], r=own[0, 2 * n:]), q.ops.cost_rows_tensor(md, own, B, DEV)):
        _equal(a.solve(x0, u0, weights=form), ob, tag=("solve", type(form).__name__))
    _equal(a.solve(x0, u0), ob, tag=("solve", "afterwards, without"))
    dist = dev32(1e-3 * np.random.default_rng(B + N).standard_normal((steps, B, md.n)))
    kw.pop("device_loop", None)
    mb = q.BatchedMPC(md, N, **kw)
    rb = mb.run(x0.astype(np.float32), steps, disturbance=dist, device_loop="always")
    ma = q.BatchedMPC(md, N, **kw)
    ra = ma.run(x0.astype(np.float32), steps, disturbance=dist, weights=own)
    for key in ("x", "u", "iters"):
        assert tuple(ra[key].shape) == tuple(rb[key].shape) and torch.equal(ra[key], rb[key]), ("run", key)
    assert torch.equal(ma.u_warm, mb.u_warm)
    for name in ("K", "k", "x", "cost", "alpha_idx", "status"):
        assert torch.equal(getattr(ma.solver, name), getattr(mb.solver, name)), ("run", name)


@pytest.mark.parametrize("model,integ", ALL)
def test_neutral_weights_equal_the_call_without_them(model, integ):
    """Every row the model's own q, qf, r -- as the plain array, as dicts with all, some and no keys, as the device tensor -- in
    solve and in run: the COST kernels must leave what the entries without weights leave, and a solve without the keyword
    afterwards gives the old bits again."""
    _, md, N, x0, u0, skw, _ = _case(model, integ)
    _assert_neutral(md, N, x0, u0, 40, skw=skw)


# ------------------------------------------------------------------------------------------------ 6. NULL rows
def test_null_rows_are_the_entry_each_extends():
    """The C entries themselves with cost_rows = NULL (the host package never calls them that way): the ref entries' bits, with and
    without reference rows."""
    q = _pkg()
    from quattro_ilqr_amd import _lib
    ops = q.ops
    name, md, N, x0, u0, _, _ = _case("cartpole", "euler")
    B = x0.shape[0]
    targets = ops.x_ref_rows_tensor(md, rc.ref_rows(name, md.x_ref, B, N + 1), B, DEV)
    for rows in (None, targets):
        a, b = q.QuattroILQR(md, N, **KW), q.QuattroILQR(md, N, **KW)
        ob = _snap(b.solve(x0, u0, targets=rows))
        a.solve(x0, u0, max_iter=0)                                  # allocates, uploads and prepares the call
        ps = a._solve_call
        flags = _lib.SOLVE_SIMULATE | _lib.SOLVE_RESET
        ops.check(ps.lib.quattro_ilqr_solve_cost_f32(*ps.head, float(a.tol), 40, flags, *ps.tail, None, None, ops._ptr(rows),
                                                     0 if rows is None else rows.shape[1], None, ops._stream()),
                  "quattro_ilqr_solve_cost_f32")
        for key, t in (("x", a.x), ("u", a.u), ("K", a.K), ("k", a.k), ("cost", a.cost), ("iters", a.iters), ("status", a.status)):
            assert torch.equal(t, ob[key]), (rows is None, key)
    # the closed loop: ops.mpc_run's arguments through the C entry itself
    steps = 4
    mb = q.BatchedMPC(md, N, **KW)
    rb = mb.run(x0.astype(np.float32), steps, replan_every=2, feedback=True)
    ma = q.BatchedMPC(md, N, **KW)
    sv = ma.solver
    sv._alloc(B)
    sv.u.zero_()
    sv._ws = ops.workspace(md, B, N, DEV)
    x_cur = dev32(x0)
    tx = torch.empty((B, steps + 1, md.n), dtype=torch.float32, device=DEV)
    tu = torch.empty((B, steps, md.m), dtype=torch.float32, device=DEV)
    ti = torch.empty((B, steps // 2), dtype=torch.int32, device=DEV)
    head, keep = ops._mpc_args(md, x_cur, sv.x, sv.u, sv.K, sv.k, sv.cost, sv.tol, sv.max_iter, steps, sv._ws, tx, tu, ti, None,
                               sv.alphas, sv.reg, sv.alpha_idx, sv.active, sv.iters, sv.status)
    ops.check(_lib.load_for(md).quattro_mpc_run_cost_f32(*head, None, None, 2, 1, None, None, 0, 1, None, ops._stream()),
              "quattro_mpc_run_cost_f32")
    assert torch.equal(tx, rb["x"]) and torch.equal(tu, rb["u"]) and torch.equal(ti, rb["iters"].to(ti.dtype))


# ------------------------------------------------------------------------------------------------ 7. heterogeneous rows
def _assert_heterogeneous(model, integ, N):
    q = _pkg()
    name, md, N, x0, u0, skw, rows = _case(model, integ, N)
    B = x0.shape[0]
    n = md.n
    solver = q.QuattroILQR(md, N, **KW, **skw)
    het = _snap(solver.solve(x0, u0, weights=rows))
    assert int(het["iters"].min()) >= 1 and (model == "planar" or int(het["status"].abs().sum()) == 0)
    _equal(solver.solve(x0, u0, weights=dict(q=rows[:, :n], qf=rows[:, n:2 * n], r=rows[:, 2 * n:])), het, tag=("dict",))
    _equal(solver.solve(x0, u0, weights=q.ops.cost_rows_tensor(md, rows, B, DEV)), het, tag=("device tensor",))
    plain = _snap(solver.solve(x0, u0))
    for b in range(B):
        one = q.QuattroILQR(_with_row(md, rows[b]), N, **KW, **skw).solve(x0[b:b + 1], u0[b:b + 1])
        for key in SOLVE_KEYS:
            assert torch.equal(het[key][b:b + 1], one[key]), (b, key)
        assert not torch.equal(het["k"][b], plain["k"][b]) and not torch.equal(het["x"][b], plain["x"][b]), b


@pytest.mark.parametrize("model,integ", ALL)
def test_heterogeneous_weights_equal_solvers_built_on_each_row(model, integ):
    """Trajectory b against the plain path of a solver whose model has q, qf, r = row b.  The rows differ from the model's own
    weights and from each other, so the batch without weights does not give these bits."""
    _assert_heterogeneous(model, integ, wc.N)


@pytest.mark.parametrize("model,integ", wc.CASES)
def test_heterogeneous_weights_fill_the_log_ring_like_each_solver(model, integ):
    q = _pkg()
    _, md, N, x0, u0, _, rows = _case(model, integ)
    B = x0.shape[0]
    log = q.ops.SolveLog(md, N, B, 40, DEV)
    het = _snap(q.QuattroILQR(md, N, **KW).solve(x0, u0, weights=rows, log=log))
    _equal(q.QuattroILQR(md, N, **KW).solve(x0, u0, weights=rows), het, tag=("unlogged",))
    for b in range(B):
        mb = _with_row(md, rows[b])
        log1 = q.ops.SolveLog(mb, N, 1, 40, DEV)
        one = q.QuattroILQR(mb, N, **KW).solve(x0[b:b + 1], u0[b:b + 1], log=log1)
        n_it = int(one["iters"][0])
        assert n_it == int(het["iters"][b]) and 1 <= n_it < log.capacity
        got, want = log.rows(b, n_it + 1), log1.rows(0, n_it + 1)
        for key in ("cost", "alpha_idx", "iteration", "x", "u", "K", "k"):
            assert np.array_equal(got[key], want[key]), (b, key)
        assert not got["stamps"][n_it].any(), b


@pytest.mark.parametrize("model,integ", ALL)
@pytest.mark.parametrize("with_phys,with_targets", [(True, False), (False, True), (True, True)])
def test_heterogeneous_weights_combine_with_model_phys_and_targets(model, integ, with_phys, with_targets):
    """Weights with model_phys only, with targets only (R = N + 1, ref_cases.skew_rows' ramp about the model's x_ref) and with both:
    the one COST kernel that takes either array, against per-trajectory calls with B = 1 and -- where the other arrays allow it --
    against a solver built on the row's weights that is given the same model_phys / targets and runs the PHYS / REF kernels."""
    q = _pkg()
    name, md, N, x0, u0, skw, rows = _case(model, integ)
    B = x0.shape[0]
    phys = _phys(model, md, B) if with_phys else None
    targets = rc.ref_rows(name, md.x_ref, B, N + 1) if with_targets else None
    het = _snap(q.QuattroILQR(md, N, **KW, **skw).solve(x0, u0, weights=rows, model_phys=phys, targets=targets))
    assert int(het["iters"].min()) >= 1 and (model == "planar" or int(het["status"].abs().sum()) == 0)
    only_w = _snap(q.QuattroILQR(md, N, **KW, **skw).solve(x0, u0, weights=rows))
    only_o = _snap(q.QuattroILQR(md, N, **KW, **skw).solve(x0, u0, model_phys=phys, targets=targets))
    for b in range(B):
        sl = slice(b, b + 1)
        kw1 = dict(model_phys=None if phys is None else phys[sl], targets=None if targets is None else targets[sl])
        one = q.QuattroILQR(md, N, **KW, **skw).solve(x0[sl], u0[sl], weights=rows[sl], **kw1)
        built = q.QuattroILQR(_with_row(md, rows[b]), N, **KW, **skw).solve(x0[sl], u0[sl], **kw1)
        for key in SOLVE_KEYS:
            assert torch.equal(het[key][sl], one[key]), ("B = 1", b, key)
            assert torch.equal(het[key][sl], built[key]), ("built on the row", b, key)
        assert not torch.equal(het["k"][b], only_o["k"][b]), b
        # (a phys row that IS the model's own -- test_model_phys_cpu.phys_rows' row 0 -- changes nothing by itself)
        own_phys = phys is None or np.array_equal(phys[b], np.asarray(md.phys, dtype=np.float32)[:phys.shape[1]])
        if targets is not None or not own_phys:
            assert not torch.equal(het["k"][b], only_w["k"][b]), b


# ------------------------------------------------------------------------------------------------ 8. closed loop
def _assert_closed_loop(model, integ, combos, targets_preview=None, with_phys=False):
    q = _pkg()
    name, md, N, x0, _, skw, rows = _case(model, integ)
    B, steps = x0.shape[0], RUN_STEPS
    x0 = x0.astype(np.float32)
    dist = dev32(1e-3 * np.random.default_rng(300 + B).standard_normal((steps, B, md.n)))
    base = np.asarray(md.phys, dtype=np.float64)
    wrong = (base[None, :] * (1.0 + 0.1 * np.sin(2.0 + np.arange(B)[:, None] + 1.3 * np.arange(base.size)[None, :]))).astype(np.float32)
    targets = None if targets_preview is None else rc.ref_rows(name, md.x_ref, B, steps + N + 1)
    tkw = {} if targets_preview is None else dict(preview=targets_preview)
    phys = _phys(model, md, B) if with_phys else None       # (controller b plans with phys[b]; its default plant is that row too)
    for hold, feedback, mismatched in combos:
        pp = wrong if mismatched else None
        free = q.BatchedMPC(md, N, **KW).run(x0, steps, disturbance=dist, device_loop="always", replan_every=hold, feedback=feedback,
                                             plant_phys=pp, targets=targets, model_phys=phys, **tkw)
        mpc = q.BatchedMPC(md, N, **KW)
        dev = mpc.run(x0, steps, disturbance=dist, weights=rows, replan_every=hold, feedback=feedback, plant_phys=pp, targets=targets,
                      model_phys=phys, **tkw)
        assert bool(torch.isfinite(dev["x"]).all()) and int(dev["iters"].min()) >= 1
        assert tuple(dev["iters"].shape) == (B, steps // hold)
        for b in range(B):
            sl = slice(b, b + 1)
            one_mpc = q.BatchedMPC(_with_row(md, rows[b]), N, **KW)
            one = one_mpc.run(x0[sl], steps, disturbance=dist[:, sl].contiguous(), device_loop="always", replan_every=hold,
                              feedback=feedback, plant_phys=None if pp is None else pp[sl],
                              targets=None if targets is None else targets[sl],
                              model_phys=None if phys is None else phys[sl], **tkw)
            for key in ("x", "u", "iters"):
                assert torch.equal(dev[key][sl], one[key]), (hold, feedback, mismatched, b, key)
            assert torch.equal(mpc.u_warm[sl], one_mpc.u_warm), (hold, feedback, mismatched, b)
            assert not torch.equal(dev["x"][b], free["x"][b]), (hold, feedback, mismatched, b)


@pytest.mark.parametrize("model,integ", ALL)
def test_closed_loop_equals_runs_of_one_controller_each(model, integ):
    """Six plant steps with a disturbance: replan_every 1 and 3, feedback on and off, the default plant and per-controller plants
    that are NOT the controllers' model (a mismatched plant_phys): run(weights=) against B runs of one controller built on its row;
    x, u, iters and the warm start left behind, bit for bit."""
    _assert_closed_loop(model, integ, [(1, False, False), (3, True, False), (3, False, True), (1, True, True)])


@pytest.mark.parametrize("model,integ", [("cartpole", "euler"), ("cartpole", "rk4"), ("planar", "rk4")])
def test_closed_loop_with_targets_and_preview_equals_runs_of_one_controller_each(model, integ):
    """The kernel that takes every array, with reference rows and NULL model_phys: once with NULL plant_phys too (hold 1, no
    feedback -- the phys the kernel falls back to is also the default plant), once with a mismatched plant_phys."""
    _assert_closed_loop(model, integ, [(1, False, False), (3, True, True)], targets_preview=True)


@pytest.mark.parametrize("model,integ", ALL)
@pytest.mark.parametrize("with_targets", [False, True])
def test_closed_loop_with_model_phys_equals_runs_of_one_controller_each(model, integ, with_targets):
    """run(weights=, model_phys=): controller b plans with its own row of both, and with NULL plant_phys its plant is its phys row;
    with and without reference rows (NULL x_ref_rows in the kernel that takes every array), once against a mismatched plant."""
    _assert_closed_loop(model, integ, [(1, False, False), (3, True, True)], targets_preview=True if with_targets else None,
                        with_phys=True)


def test_control_step_takes_weights():
    q = _pkg()
    _, md, N, x0, _, _, rows = _case("cartpole", "euler")
    a, b = q.BatchedMPC(md, N, **KW), q.BatchedMPC(md, N, **KW)
    xa, ua, ia = a.control_step(x0.astype(np.float32), weights=rows)
    out = b.solver.solve(x0.astype(np.float32), None, weights=rows)
    assert torch.equal(xa, out["x"]) and torch.equal(ua, out["u"]) and torch.equal(ia, out["iters"])


# ------------------------------------------------------------------------------------------------ 9. first iteration
@pytest.mark.parametrize("model,N", wc.SHAPES)
@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_first_iteration_of_every_row_against_the_oracle(model, N, integ):
    """max_iter = 1 with a log ring: cost of the nominal (relative, param_cases.BOUNDS["sim_cost"] = 2e-6), K and k (rel_fro 5e-6)
    and the accepted step against ref_cases.first_iteration on the row's own spec -- the project's own bounds for these quantities;
    a wrong row or an ignored part of it moves K, k and the cost by 100 x these and more (tests/test_cost_rows_cpu.py)."""
    q = _pkg()
    _, md, N, x0, u0, _, rows = _case(model, integ, N)
    B = x0.shape[0]
    log = q.ops.SolveLog(md, N, B, 2, DEV)
    out = _snap(q.QuattroILQR(md, N, **dict(KW, max_iter=1)).solve(x0, u0, weights=rows, log=log))
    assert int(out["status"].abs().sum()) == 0
    bad = []
    for b in range(B):
        ref = wc.first_iteration(model, integ, rows[b], x0[b:b + 1], u0[b:b + 1])
        rec = log.rows(b, 1)
        eJ = abs(rec["cost"][0, 0] - ref["cost"][0]) / abs(ref["cost"][0])
        eK, ek = rel_fro(f64(out["K"][b]), ref["K"][0]), rel_fro(f64(out["k"][b]), ref["k"][0])
        print(f"[cost rows vs oracle {model} {integ} N={N}] b={b}: cost {eJ:.1e} K {eK:.1e} k {ek:.1e} alpha device "
              f"{float(out['alpha'][b])} oracle {ref['alpha'][0]}")
        if not (eJ < pc.BOUNDS["sim_cost"] and eK < pc.BOUNDS["K"] and ek < pc.BOUNDS["k"]
                and abs(float(out["alpha"][b]) - ref["alpha"][0]) < 1e-7):
            bad.append((b, eJ, eK, ek, float(out["alpha"][b]), ref["alpha"][0]))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 10. converged solve
@pytest.mark.parametrize("model,integ", wc.CASES)
def test_converged_solve_of_every_trajectory_matches_optimize_on_its_own_spec(model, integ):
    """Whole solves at N = 7 (param_cases.SOLVE_N, its inputs) under the rows, through the persistent kernel, against
    oracle.ilqr.optimize on each trajectory's own spec: every trajectory of the batch; iteration count within one of the oracle's,
    and where it is equal cost (relative), x and u (largest absolute difference) within weight_cases.solve_bounds =
    max(param_cases.solve_bounds, 4 x weight_cases.SOLVE_E)."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    N, B = pc.SOLVE_N, wc.B[model]
    x0, u0 = wc.solve_inputs(model)
    rows = wc.weight_rows(model)
    out = q.QuattroILQR(md, N, max_iter=pc.SOLVE_MAX_ITER, tol=pc.SOLVE_TOL, device=DEV, tf_window=0).solve(x0, u0, weights=rows)
    assert int(out["status"].abs().sum()) == 0
    u_dev, x_dev = f64(out["u"]), f64(out["x"])
    it_dev, cost_dev = out["iters"].cpu().numpy(), out["cost"].cpu().numpy()
    bounds = wc.solve_bounds(model)
    bad = []
    for b in range(B):
        ref = pc.solve_optimize(wc.row_spec(model, integ, rows[b]), x0[b], u0[b])
        errs = pc.solve_errors((u_dev[b], x_dev[b], float(cost_dev[b])), ref)
        print(f"[converged, own weights {model} {integ}] b={b}: iterations oracle {ref[3]} device {it_dev[b]}, cost {ref[2]:.6f} vs "
              f"{cost_dev[b]:.6f} ({errs['cost']:.1e}), max|dx| {errs['x']:.1e} max|du| {errs['u']:.1e}")
        assert abs(ref[3] - it_dev[b]) <= 1, (b, ref[3], it_dev[b])
        if ref[3] == it_dev[b]:
            bad += [(b, key, e, bounds[key]) for key, e in errs.items() if not e < bounds[key]]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 11. refusals
def test_modes_without_a_device_resident_loop_refuse_weights():
    """A predictor, device_loop=False and use_graph=True: NotImplementedError before the solver has allocated anything."""
    import os
    q = _pkg()
    from quattro_ilqr_amd import models
    md = models.cartpole_model(dt=0.01, integrator="euler")
    tf = q.TransformerILQR(4, 5, device=DEV).load(os.path.join(GOLDEN, "tf_weights_cartpole.npz"))
    B, N = 3, 30
    x0 = np.zeros((B, 4), dtype=np.float32)
    rows = _own(md, B)
    for kw in (dict(tf=tf), dict(device_loop=False, tf_window=0), dict(use_graph=True, tf_window=0)):
        solver = q.QuattroILQR(md, N, max_iter=3, device=DEV, **kw)
        with pytest.raises(NotImplementedError, match="weights runs only in the device-resident loop"):
            solver.solve(x0, weights=rows)
        assert solver._B is None
        mpc = q.BatchedMPC(md, N, max_iter=3, device=DEV, **{k_: v for k_, v in kw.items() if k_ in ("tf", "tf_window")})
        if "tf" in kw:
            with pytest.raises(NotImplementedError, match="device-resident loop"):
                mpc.run(x0, 2, weights=rows)
            with pytest.raises(NotImplementedError, match="device-resident loop"):
                mpc.control_step(x0, weights=rows)
        with pytest.raises(NotImplementedError, match="device-resident loop"):
            mpc.run(x0, 2, weights=rows, device_loop=False)
        assert mpc.solver._B is None
