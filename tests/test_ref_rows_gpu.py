"""Reference rows (quattro_ilqr_solve_ref_f32, quattro_mpc_run_ref_f32; `targets=` of QuattroILQR.solve, BatchedMPC.control_step and
BatchedMPC.run) on the GPU:
   4. neutral rows (the model's own x_ref in every row) leave what the call without them leaves, bit for bit;
   5. R = 1, a goal per trajectory: B solvers built on model.with_(x_ref=row b) through the plain path, bit for bit, log ring too;
   6. heterogeneous moving references: per-trajectory calls with B = 1, bit for bit, with and without model_phys;
   7. the closed loop in one launch against the host-driven form solve(targets=window of plan c) -> ops.track -> shift, bit for bit;
   8. the first iteration against the composed fp64 blocks, the converged solve against the clock-augmented oracle.ilqr.optimize;
   9. the set-point schedule (preview=False): every plan of a short run against plain oracle.ilqr.optimize on its constant target;
  10. the modes without a device-resident loop refuse.
Shapes, inputs, references and their well-posedness: tests/ref_cases.py, tests/test_ref_rows_cpu.py."""
import dataclasses

import numpy as np
import pytest

import param_cases as pc
import ref_cases as rc
from conftest import GOLDEN, rel_fro
from test_model_phys_cpu import phys_rows
from test_ref_rows_cpu import CASES, REF_B, REF_N, REF_N_LONG, RUN_STEPS, run_row_counts, solve_row_counts

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SOLVE_KEYS = ("x", "u", "K", "k", "cost", "iters", "alpha", "status")
KW = dict(max_iter=40, tol=1e-3, device=DEV, tf_window=0)
ALL = CASES + [("planar", "rk4")]


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def f64(t):
    return t.double().cpu().numpy()


def _snap(out):
    return {k_: v.clone() for k_, v in out.items()}


def _case(model, integ, N=REF_N, B=None):
    """-> (model name for ref_cases, DeviceModel, N, x0, u0, solver keywords).  The planar user model (n = 6, m = 2; its prebuilt RK4
    library) runs B = 3, N = 12 through its persistent kernel, which rows take without being asked."""
    q = _pkg()
    if model == "planar":
        from test_user_model_gpu import planar_batch, planar_model
        x0, u0 = planar_batch(3 if B is None else B, 12, 5)
        return "planar", planar_model(integ), 12, x0.astype(np.float32).astype(np.float64), u0, dict(device_loop="always")
    B = REF_B[model] if B is None else B
    x0, u0 = rc.inputs(model, N, B)
    return model, pc.device_model(q.models, model, "skew", integ), N, x0, u0, {}


def _rows(name, md, B, R):
    return rc.ref_rows(name, md.x_ref, B, R)


def _equal(a, b, keys=SOLVE_KEYS, tag=()):
    for key in keys:
        assert torch.equal(a[key], b[key]), (*tag, key)


# ------------------------------------------------------------------------------------------------ 4. neutral rows
def _assert_neutral(md, N, x0, u0, max_iter, row_counts, steps=RUN_STEPS, skw={}):
    q = _pkg()
    B = x0.shape[0]
    kw = dict(KW, max_iter=max_iter, **skw)
    a, b = q.QuattroILQR(md, N, **kw), q.QuattroILQR(md, N, **kw)
    ob = _snap(b.solve(x0, u0))
    for R in row_counts:
        _equal(a.solve(x0, u0, targets=rc.neutral_rows(md.x_ref, B, R)), ob, tag=("solve", R))
    _equal(a.solve(x0, u0, targets=np.tile(np.asarray(md.x_ref, dtype=np.float32), (B, 1))), ob, tag=("solve", "(B, n)"))
    _equal(a.solve(x0, u0), ob, tag=("solve", "afterwards, without"))
    dist = dev32(1e-3 * np.random.default_rng(B + N).standard_normal((steps, B, md.n)))
    kw.pop("device_loop", None)
    mb = q.BatchedMPC(md, N, **kw)
    rb = mb.run(x0.astype(np.float32), steps, disturbance=dist, device_loop="always")
    for R, preview in ((steps + N + 1, True), (steps + N + 1, False), (4, True), (1, False)):
        ma = q.BatchedMPC(md, N, **kw)
        ra = ma.run(x0.astype(np.float32), steps, disturbance=dist, targets=rc.neutral_rows(md.x_ref, B, R), preview=preview)
        for key in ("x", "u", "iters"):
            assert tuple(ra[key].shape) == tuple(rb[key].shape) and torch.equal(ra[key], rb[key]), ("run", R, preview, key)
        assert torch.equal(ma.u_warm, mb.u_warm), (R, preview)
        for name in ("K", "k", "x", "cost", "alpha_idx", "status"):
            assert torch.equal(getattr(ma.solver, name), getattr(mb.solver, name)), ("run", R, preview, name)


@pytest.mark.parametrize("model,integ", ALL)
def test_neutral_rows_equal_the_call_without_them(model, integ):
    """Every row the model's own x_ref, R = 1, 7, N + 1 and the (B, n) form in solve; R covering the run, R = 4 and R = 1 with
    either preview in run: the REF kernels must leave what the entries without rows leave."""
    _, md, N, x0, u0, skw = _case(model, integ)
    _assert_neutral(md, N, x0, u0, 40, solve_row_counts(N), skw=skw)


def test_neutral_rows_equal_the_call_without_them_at_257_quadrotors():
    """B = 257, N = 50 (two LDS refills of the fused sweep, 129 workgroups, the last one half empty), the default quadrotor."""
    from quattro_ilqr_amd import models
    md = models.quadrotor_model()
    B, N = 257, 50
    rng = np.random.default_rng(B)
    x0 = np.asarray(md.x_ref) + rng.uniform(-1, 1, (B, 12)) * np.array([0.5, 0.5, 0.01, 0, 0, 0, 0.2, 0.2, 0.5, 0, 0, 0])
    u0 = 2.4525 + 0.1 * rng.standard_normal((B, N, 4))
    _assert_neutral(md, N, x0, u0, 4, (N + 1,), steps=3)


def test_null_rows_are_the_entry_each_extends():
    """The C entries themselves with x_ref_rows = NULL (the host package never calls them that way): the phys entries' bits."""
    q = _pkg()
    from quattro_ilqr_amd import _lib
    ops = q.ops
    _, md, N, x0, u0, _ = _case("quadrotor", "euler")
    a, b = q.QuattroILQR(md, N, **KW), q.QuattroILQR(md, N, **KW)
    ob = _snap(b.solve(x0, u0))
    a.solve(x0, u0, max_iter=0)                                  # allocates, uploads and prepares the call
    ps = a._solve_call
    flags = _lib.SOLVE_SIMULATE | _lib.SOLVE_RESET
    ops.check(ps.lib.quattro_ilqr_solve_ref_f32(*ps.head, float(a.tol), 40, flags, *ps.tail, None, None, None, 0, ops._stream()),
              "quattro_ilqr_solve_ref_f32")
    for key, t in (("x", a.x), ("u", a.u), ("K", a.K), ("k", a.k), ("cost", a.cost), ("iters", a.iters), ("status", a.status)):
        assert torch.equal(t, ob[key]), key


# ------------------------------------------------------------------------------------------------ 5. a goal per trajectory
@pytest.mark.parametrize("model,integ", ALL)
def test_goal_per_trajectory_equals_solvers_built_on_each_goal(model, integ):
    """R = 1: trajectory b against the plain path of a solver whose model has x_ref = row b.  The goals differ from the model's
    own x_ref and from each other, so the batch without targets does not give these bits."""
    q = _pkg()
    name, md, N, x0, u0, skw = _case(model, integ)
    B = x0.shape[0]
    goals = _rows(name, md, B, 1)[:, 0]
    solver = q.QuattroILQR(md, N, **KW, **skw)
    het = _snap(solver.solve(x0, u0, targets=goals))
    assert int(het["iters"].min()) >= 1 and (model == "planar" or int(het["status"].abs().sum()) == 0)
    _equal(solver.solve(x0, u0, targets=dev32(goals[:, None])), het, tag=("device tensor",))
    plain = _snap(solver.solve(x0, u0))
    for b in range(B):
        one = q.QuattroILQR(md.with_(x_ref=tuple(map(float, goals[b]))), N, **KW, **skw).solve(x0[b:b + 1], u0[b:b + 1])
        for key in SOLVE_KEYS:
            assert torch.equal(het[key][b:b + 1], one[key]), (b, key)
        assert not torch.equal(het["k"][b], plain["k"][b]) and not torch.equal(het["x"][b], plain["x"][b]), b


@pytest.mark.parametrize("model,integ", [("quadrotor", "rk4"), ("cartpole", "euler")])
def test_goal_per_trajectory_fills_the_log_ring_like_each_solver(model, integ):
    q = _pkg()
    name, md, N, x0, u0, _ = _case(model, integ)
    B = x0.shape[0]
    goals = _rows(name, md, B, 1)[:, 0]
    log = q.ops.SolveLog(md, N, B, 40, DEV)
    het = _snap(q.QuattroILQR(md, N, **KW).solve(x0, u0, targets=goals, log=log))
    _equal(q.QuattroILQR(md, N, **KW).solve(x0, u0, targets=goals), het, tag=("unlogged",))
    for b in range(B):
        mb = md.with_(x_ref=tuple(map(float, goals[b])))
        log1 = q.ops.SolveLog(mb, N, 1, 40, DEV)
        one = q.QuattroILQR(mb, N, **KW).solve(x0[b:b + 1], u0[b:b + 1], log=log1)
        n_it = int(one["iters"][0])
        assert n_it == int(het["iters"][b]) and 1 <= n_it < log.capacity
        got, want = log.rows(b, n_it + 1), log1.rows(0, n_it + 1)
        for key in ("cost", "alpha_idx", "iteration", "x", "u", "K", "k"):
            assert np.array_equal(got[key], want[key]), (b, key)
        assert not got["stamps"][n_it].any(), b


# ------------------------------------------------------------------------------------------------ 6. moving references
def _assert_moving(model, integ, N, with_phys):
    q = _pkg()
    name, md, N, x0, u0, _ = _case(model, integ, N)
    B = x0.shape[0]
    phys = None
    if with_phys and model == "planar":          # the planar model's free parameters, the mass scaled per trajectory
        phys = np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1))
        phys[:, 0] *= (1.0 + 0.2 * np.sin(1.0 + np.arange(B))).astype(np.float32)
    elif with_phys:
        phys = phys_rows(model, B)
    plain = _snap(q.QuattroILQR(md, N, **KW).solve(x0, u0, model_phys=phys))
    for R in solve_row_counts(N)[1:]:
        rows = _rows(name, md, B, R)
        het = _snap(q.QuattroILQR(md, N, **KW).solve(x0, u0, targets=rows, model_phys=phys))
        assert int(het["iters"].min()) >= 1 and (model == "planar" or int(het["status"].abs().sum()) == 0)
        for b in range(B):
            one = q.QuattroILQR(md, N, **KW).solve(x0[b:b + 1], u0[b:b + 1], targets=rows[b:b + 1],
                                                   model_phys=None if phys is None else phys[b:b + 1])
            for key in SOLVE_KEYS:
                assert torch.equal(het[key][b:b + 1], one[key]), (R, b, key)
            assert not torch.equal(het["k"][b], plain["k"][b]), (R, b)
        # the rows past R - 1 are never read: the same rows with others appended beyond the horizon give the same bits
        if R == N + 1:
            longer = np.concatenate([rows, 7.0 + rows[:, :3]], axis=1)
            _equal(q.QuattroILQR(md, N, **KW).solve(x0, u0, targets=longer, model_phys=phys), het, tag=("rows beyond N",))
        else:
            held = np.concatenate([rows, np.repeat(rows[:, -1:], N + 1 - R, axis=1)], axis=1)     # the clamp, written out
            _equal(q.QuattroILQR(md, N, **KW).solve(x0, u0, targets=held, model_phys=phys), het, tag=("clamp written out",))


@pytest.mark.parametrize("model,integ", ALL)
@pytest.mark.parametrize("with_phys", [False, True])
def test_moving_references_equal_per_trajectory_solves(model, integ, with_phys):
    """R = 7 (the last row held from step 6 on) and R = N + 1, every trajectory on rows of its own, against B calls with B = 1;
    N = 20 crosses a refill boundary of the RK4 sweep's 12-step batches (quadrotor)."""
    _assert_moving(model, integ, REF_N, with_phys)


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_moving_references_equal_per_trajectory_solves_at_37_steps(integ):
    """N = 37: two refills of the Euler sweep's 25-step batches, four of the RK4 sweep's 12-step ones."""
    _assert_moving("quadrotor", integ, REF_N_LONG, False)


def test_rows_in_a_misaligned_device_tensor_are_realigned():
    """A contiguous float32 device tensor that starts 4 bytes into its storage is not what the C ABI takes (16-byte aligned rows:
    the sweep loads them four floats at a time); ops.x_ref_rows_tensor copies it, and the solve gives the aligned tensor's bits."""
    q = _pkg()
    name, md, N, x0, u0, _ = _case("quadrotor", "euler")
    B = x0.shape[0]
    rows = _rows(name, md, B, N + 1)
    store = torch.zeros(rows.size + 1, dtype=torch.float32, device=DEV)
    view = store[1:].view(B, N + 1, md.n)
    view.copy_(dev32(rows))
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    assert q.ops.x_ref_rows_tensor(md, view, B, DEV).data_ptr() % 16 == 0
    _equal(q.QuattroILQR(md, N, **KW).solve(x0, u0, targets=view), _snap(q.QuattroILQR(md, N, **KW).solve(x0, u0, targets=rows)))


# ------------------------------------------------------------------------------------------------ 7. closed loop
def _host_driven(md, N, x0, rows, steps, hold, feedback, preview, plant_phys, dist, solver_kw):
    """solve(targets=window of plan c) -> ops.track -> shift, as BatchedMPC.run does without a persistent kernel; the window is
    built on the host by the clamp rule (ref_cases.window).  -> the run's dict, the warm start left behind, and the start state
    and warm start of every plan."""
    q = _pkg()
    sv = q.QuattroILQR(md, N, **KW, **solver_kw)
    x, u_warm = dev32(x0), None
    xs, us, its, starts = [x[:, None]], [], [], []
    for c in range(steps // hold):
        win = rc.window(rows, N, s=c * hold, preview=int(preview))
        starts.append((f64(x), None if u_warm is None else f64(u_warm)))
        out = sv.solve(x, u_warm, targets=win)
        xt, ut = q.ops.track(md, x, out["x"], out["u"], out["K"], hold, plant_phys=plant_phys, feedback=feedback,
                             disturbance=dist[c * hold:(c + 1) * hold].contiguous())
        u = out["u"]
        u_warm = torch.cat([u[:, hold:]] + [u[:, -1:]] * hold, dim=1).contiguous()
        x = xt[:, -1].contiguous()
        xs.append(xt[:, 1:]); us.append(ut); its.append(out["iters"].clone())
    return dict(x=torch.cat(xs, dim=1), u=torch.cat(us, dim=1), iters=torch.stack(its, dim=1)), u_warm, starts


@pytest.mark.parametrize("model,integ", ALL)
def test_closed_loop_equals_the_host_driven_form(model, integ):
    """Six plant steps with a disturbance: hold 1 and 3, feedback on and off, either preview, R = steps + N + 1 and R = 4 (runs out
    mid-run), with per-controller plants that are NOT the controllers' model (a mismatched plant_phys) and once with the default
    plant; x, u, iters and the warm start left behind, bit for bit."""
    q = _pkg()
    name, md, N, x0, _, _ = _case(model, integ)
    B, steps = x0.shape[0], RUN_STEPS
    x0 = x0.astype(np.float32)
    dist = dev32(1e-3 * np.random.default_rng(200 + B).standard_normal((steps, B, md.n)))
    base = np.asarray(md.phys, dtype=np.float64)
    wrong = (base[None, :] * (1.0 + 0.1 * np.sin(2.0 + np.arange(B)[:, None] + 1.3 * np.arange(base.size)[None, :]))).astype(np.float32)
    solver_kw = dict(device_loop="always") if model == "planar" else {}
    combos = [(hold, fb, pv, R, wrong) for hold in (1, 3) for fb in (False, True) for pv in (True, False) for R in run_row_counts(N)]
    combos.append((3, True, True, run_row_counts(N)[0], None))
    free = q.BatchedMPC(md, N, **KW).run(x0, steps, disturbance=dist, device_loop="always")["x"]
    for hold, feedback, preview, R, plant_phys in combos:
        rows = _rows(name, md, B, R)
        mpc = q.BatchedMPC(md, N, **KW)
        dev = mpc.run(x0, steps, disturbance=dist, targets=rows, preview=preview, replan_every=hold, feedback=feedback,
                      plant_phys=plant_phys)
        assert bool(torch.isfinite(dev["x"]).all()) and int(dev["iters"].min()) >= 1
        host, u_warm, _ = _host_driven(md, N, x0, rows, steps, hold, feedback, preview, plant_phys, dist, solver_kw)
        for key in ("x", "u", "iters"):
            assert tuple(dev[key].shape) == tuple(host[key].shape), (hold, feedback, preview, R, key)
            assert torch.equal(dev[key], host[key].to(dev[key].dtype)), (hold, feedback, preview, R, key)
        assert torch.equal(mpc.u_warm, u_warm), (hold, feedback, preview, R)
        assert not torch.equal(dev["x"], free)


# ------------------------------------------------------------------------------------------------ 8. against the oracle
@pytest.mark.parametrize("model,integ,N", [(m, i, REF_N) for m, i in CASES] + [("quadrotor", i, REF_N_LONG) for i in ("euler", "rk4")])
def test_first_iteration_against_the_composed_oracle_blocks(model, integ, N):
    """max_iter = 1 with a log ring, R = 1, 7, N + 1: cost of the nominal (relative, param_cases.BOUNDS["sim_cost"] = 2e-6), K and
    k (rel_fro 5e-6) and the accepted step against ref_cases.first_iteration -- linearize pieces of the oracle on the window,
    riccati_sweep_batched, the fp64 line search.  The bounds of tests/test_model_params_gpu.py for the same quantities; a wrong
    row moves k and the cost by 17 x 100 x these and more (tests/test_ref_rows_cpu.py)."""
    q = _pkg()
    name, md, N, x0, u0, _ = _case(model, integ, N)
    spec = pc.spec(model, "skew", integ)
    B = x0.shape[0]
    bad = []
    for R in solve_row_counts(N):
        rows = _rows(name, md, B, R)
        log = q.ops.SolveLog(md, N, B, 2, DEV)
        out = _snap(q.QuattroILQR(md, N, **dict(KW, max_iter=1)).solve(x0, u0, targets=rows, log=log))
        assert int(out["status"].abs().sum()) == 0
        ref = rc.first_iteration(spec, rc.window(rows.astype(np.float64), N), x0, u0)
        for b in range(B):
            rec = log.rows(b, 1)
            eJ = abs(rec["cost"][0, 0] - ref["cost"][b]) / abs(ref["cost"][b])
            eK, ek = rel_fro(f64(out["K"][b]), ref["K"][b]), rel_fro(f64(out["k"][b]), ref["k"][b])
            print(f"[ref rows vs oracle {model} {integ} N={N} R={R}] b={b}: cost {eJ:.1e} K {eK:.1e} k {ek:.1e} alpha device "
                  f"{float(out['alpha'][b])} oracle {ref['alpha'][b]}")
            if not (eJ < pc.BOUNDS["sim_cost"] and eK < pc.BOUNDS["K"] and ek < pc.BOUNDS["k"]
                    and abs(float(out["alpha"][b]) - ref["alpha"][b]) < 1e-7):
                bad.append((R, b, eJ, eK, ek, float(out["alpha"][b]), ref["alpha"][b]))
    assert not bad, bad


@pytest.mark.parametrize("model,integ", CASES)
def test_converged_solve_matches_the_augmented_oracle(model, integ):
    """Whole solves at N = 7 (param_cases.SOLVE_N, its inputs) against rows of their own, R = N + 1, through the persistent kernel,
    against oracle.ilqr.optimize on the clock-augmented problem, in the form and to the standard of
    test_converged_solve_matches_oracle_optimize_at_skewed_parameters: every trajectory of the batch; iteration count within one
    of the oracle's, equal on all but at most one, and where it is equal cost (relative), x and u (largest absolute difference)
    within ref_cases.solve_bounds."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    spec = pc.spec(model, "skew", integ)
    N, B = pc.SOLVE_N, REF_B[model]
    x0, u0 = pc.inputs(model, "skew", N, B)
    rows = rc.skew_rows(model, B, N + 1)
    out = q.QuattroILQR(md, N, max_iter=pc.SOLVE_MAX_ITER, tol=pc.SOLVE_TOL, device=DEV, tf_window=0).solve(x0, u0, targets=rows)
    assert int(out["status"].abs().sum()) == 0
    u_dev, x_dev = f64(out["u"]), f64(out["x"])
    it_dev, cost_dev = out["iters"].cpu().numpy(), out["cost"].cpu().numpy()
    bounds = rc.solve_bounds(model)
    same_iters, bad = 0, []
    traj = rc.SOLVE_TRAJ[model]
    for b in traj:
        ref = rc.augmented_optimize(spec, rows[b].astype(np.float64), x0[b], u0[b])
        errs = pc.solve_errors((u_dev[b], x_dev[b], float(cost_dev[b])), ref)
        print(f"[converged, moving target {model} {integ}] b={b}: iterations oracle {ref[3]} device {it_dev[b]}, cost {ref[2]:.6f} vs "
              f"{cost_dev[b]:.6f} ({errs['cost']:.1e}), max|dx| {errs['x']:.1e} max|du| {errs['u']:.1e}")
        assert abs(ref[3] - it_dev[b]) <= 1, (b, ref[3], it_dev[b])
        if ref[3] == it_dev[b]:
            same_iters += 1
            bad += [(b, key, e, bounds[key]) for key, e in errs.items() if not e < bounds[key]]
    assert same_iters >= len(traj) - 1 and not bad, (same_iters, bad)


# ------------------------------------------------------------------------------------------------ 9. set-point schedule
@pytest.mark.parametrize("model,integ", CASES)
def test_set_point_schedule_plans_match_plain_optimize(model, integ):
    """preview=False, six control steps at N = 7, R = 6: the set-point of plan c is row c for the whole solve, so every plan is a
    constant-target problem and the unaugmented oracle.ilqr.optimize on spec with x_ref = that row is its reference.  Start state
    and warm start of every plan come from the host-driven loop, which the one launch equals bit for bit (asserted here again).
    Every plan of the trajectories of ref_cases.SETPOINT_TRAJ against optimize()'s own result: iteration count within one, equal
    on all but at most one, and where it is equal cost (relative), x and u (largest absolute difference) within
    ref_cases.setpoint_bounds."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    spec = pc.spec(model, "skew", integ)
    N, B, steps = pc.SOLVE_N, REF_B[model], rc.SETPOINT_STEPS
    x0, _ = pc.inputs(model, "skew", N, B)
    x0 = x0.astype(np.float32)
    rows = rc.skew_rows(model, B, steps)
    dist = dev32(np.zeros((steps, B, md.n)))
    mpc = q.BatchedMPC(md, N, **KW)
    dev = mpc.run(x0, steps, targets=rows, preview=False, disturbance=dist)
    host, u_warm, starts = _host_driven(md, N, x0, rows, steps, 1, False, False, None, dist, {})
    for key in ("x", "u", "iters"):
        assert torch.equal(dev[key], host[key].to(dev[key].dtype)), key
    # the plans themselves, once more through the solver (the loop above keeps only what the run records)
    sv = q.QuattroILQR(md, N, **KW)
    bounds = rc.setpoint_bounds(model)
    same_iters, total, bad = 0, 0, []
    for c, (xs, uw) in enumerate(starts):
        out = sv.solve(xs, uw, targets=rows[:, c])
        assert torch.equal(out["iters"], dev["iters"][:, c].to(out["iters"].dtype)), c
        u_dev, x_dev, cost_dev, it_dev = f64(out["u"]), f64(out["x"]), out["cost"].cpu().numpy(), out["iters"].cpu().numpy()
        for b in rc.SETPOINT_TRAJ[model]:
            sp = dataclasses.replace(spec, x_ref=rows[b, c].astype(np.float64))
            ref = pc.solve_optimize(sp, xs[b], np.zeros((N, md.m)) if uw is None else uw[b])
            errs = pc.solve_errors((u_dev[b], x_dev[b], float(cost_dev[b])), ref)
            print(f"[set-point schedule {model} {integ}] plan {c} b={b}: iterations oracle {ref[3]} device {it_dev[b]}, cost "
                  f"{errs['cost']:.1e}, max|dx| {errs['x']:.1e} max|du| {errs['u']:.1e}")
            assert abs(ref[3] - it_dev[b]) <= 1, (c, b, ref[3], it_dev[b])
            total += 1
            if ref[3] == it_dev[b]:
                same_iters += 1
                bad += [(c, b, key, e, bounds[key]) for key, e in errs.items() if not e < bounds[key]]
    assert same_iters >= total - 1 and not bad, (same_iters, total, bad)


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_modes_without_a_device_resident_loop_refuse_targets():
    """A predictor, device_loop=False and use_graph=True: NotImplementedError before the solver has allocated anything."""
    import os
    q = _pkg()
    from quattro_ilqr_amd import models
    md = models.cartpole_model(dt=0.01, integrator="euler")
    tf = q.TransformerILQR(4, 5, device=DEV).load(os.path.join(GOLDEN, "tf_weights_cartpole.npz"))
    B, N = 3, 30
    x0 = np.zeros((B, 4), dtype=np.float32)
    rows = rc.neutral_rows(md.x_ref, B, 4)
    for kw in (dict(tf=tf), dict(device_loop=False, tf_window=0), dict(use_graph=True, tf_window=0)):
        solver = q.QuattroILQR(md, N, max_iter=3, device=DEV, **kw)
        with pytest.raises(NotImplementedError, match="targets runs only in the device-resident loop"):
            solver.solve(x0, targets=rows)
        assert solver._B is None
        mpc = q.BatchedMPC(md, N, max_iter=3, device=DEV, **{k_: v for k_, v in kw.items() if k_ in ("tf", "tf_window")})
        if "tf" in kw:
            with pytest.raises(NotImplementedError, match="device-resident loop"):
                mpc.run(x0, 2, targets=rows)
            with pytest.raises(NotImplementedError, match="device-resident loop"):
                mpc.control_step(x0, targets=rows)
        with pytest.raises(NotImplementedError, match="device-resident loop"):
            mpc.run(x0, 2, targets=rows, device_loop=False)
        assert mpc.solver._B is None
