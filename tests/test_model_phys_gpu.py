"""Per-trajectory model parameters (quattro_ilqr_solve_phys_f32, quattro_mpc_run_phys_f32; `model_phys=` of QuattroILQR.solve,
BatchedMPC.run and BatchedMPC.control_step) on the GPU:
  1. a heterogeneous batch equals the per-trajectory solves (each on the unchanged shared-parameter path), bit for bit;
  2. neutral rows (the model's own phys, tiled) leave what the call without them leaves, bit for bit;
  3. the closed loop against per-controller runs, bit for bit, with the default plant and with a wrong plant of its own;
  4. the first iteration of every row against the fp64 oracle at that row's parameters;
  5. the modes without a device-resident loop refuse.
Inputs and their well-posedness: tests/test_model_phys_cpu.py."""
import numpy as np
import pytest

import param_cases as pc
from conftest import GOLDEN, rel_fro
from test_model_phys_cpu import PHYS_B, PHYS_N, oracle_first_iteration, phys_rows

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(model, integ) for model in pc.MODELS for integ in ("euler", "rk4")]
SOLVE_KEYS = ("x", "u", "K", "k", "cost", "iters", "alpha", "status")
KW = dict(max_iter=40, tol=1e-3, device=DEV, tf_window=0)


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def f64(t):
    return t.double().cpu().numpy()


def _snap(out):
    return {k_: v.clone() for k_, v in out.items()}


def _with_row(md, row):
    return md.with_(phys=tuple(map(float, row[:len(md.phys)])))


def _builtin(model, integ, B):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    x0, u0 = pc.inputs(model, "skew", PHYS_N, B)
    return md, PHYS_N, x0, u0, phys_rows(model, B)


def _planar(B=3, N=12, seed=5):
    from test_user_model_gpu import PHYS, planar_batch, planar_model
    md = planar_model("rk4")
    x0, u0 = planar_batch(B, N, seed)
    rows = np.tile(np.asarray(PHYS, dtype=np.float64), (B, 1))
    rows[:, 0] *= 1.0 + 0.2 * np.sin(1.0 + np.arange(B))
    return md, N, x0, u0, rows.astype(np.float32)


def _assert_rows_equal_single_solves(md, N, x0, u0, rows, het, **solver_kw):
    q = _pkg()
    for b in range(rows.shape[0]):
        one = q.QuattroILQR(_with_row(md, rows[b]), N, **KW, **solver_kw).solve(x0[b:b + 1], u0[b:b + 1])
        for key in SOLVE_KEYS:
            assert torch.equal(het[key][b:b + 1], one[key]), (b, key)


# ------------------------------------------------------------------------------------------------ 1. heterogeneous batch
@pytest.mark.parametrize("model,integ", CASES)
def test_heterogeneous_batch_equals_per_trajectory_solves(model, integ):
    """B = 5 quadrotors (workgroups of 2, 2 and 1 trajectories: two parameter sets inside one workgroup) / 9 cart-poles (rows
    4 + 4 + 1), N = 26, every physical parameter different in every row.  Row 0 holds the shared set: it equals the plain
    batch's trajectory 0, and the other rows do not."""
    q = _pkg()
    md, N, x0, u0, rows = _builtin(model, integ, PHYS_B[model])
    solver = q.QuattroILQR(md, N, **KW)
    het = _snap(solver.solve(x0, u0, model_phys=rows))
    assert int(het["status"].abs().sum()) == 0 and int(het["iters"].min()) >= 1
    _assert_rows_equal_single_solves(md, N, x0, u0, rows, het)
    plain = _snap(solver.solve(x0, u0))                      # the same solver, now without: no stale rows
    for key in SOLVE_KEYS:
        assert torch.equal(het[key][:1], plain[key][:1]), key
    assert not torch.equal(het["K"][1:], plain["K"][1:]) and not torch.equal(het["x"][1:], plain["x"][1:])
    again = solver.solve(x0, u0, model_phys=dev32(np.pad(rows, ((0, 0), (0, 8 - rows.shape[1])))))     # the (B, 8) device form
    for key in SOLVE_KEYS:
        assert torch.equal(het[key], again[key]), key


def test_heterogeneous_user_model_batch_equals_per_trajectory_solves():
    """The prebuilt planar RK4 model: the rows are its free parameters P[0..7], the mass scaled per trajectory; the persistent
    kernel is taken without being asked for."""
    q = _pkg()
    md, N, x0, u0, rows = _planar()
    solver = q.QuattroILQR(md, N, **KW)
    het = _snap(solver.solve(x0, u0, model_phys=rows))
    assert int(het["iters"].min()) >= 1
    _assert_rows_equal_single_solves(md, N, x0, u0, rows, het)
    plain = _snap(solver.solve(x0, u0))                      # (no row is the model's own set here: every trajectory moves)
    for b in range(rows.shape[0]):
        assert not torch.equal(het["K"][b], plain["K"][b]), b


def test_heterogeneous_solve_fills_the_log_ring_per_trajectory():
    """RK4 quadrotor with an ops.SolveLog: iters[b] records for trajectory b, numbered in order, the last one holding the gains
    and the cost the solve leaves behind; the logged solve returns what the unlogged one returns."""
    q = _pkg()
    md, N, x0, u0, rows = _builtin("quadrotor", "rk4", PHYS_B["quadrotor"])
    B = rows.shape[0]
    het = _snap(q.QuattroILQR(md, N, **KW).solve(x0, u0, model_phys=rows))
    log = q.ops.SolveLog(md, N, B, 40, DEV)
    out = _snap(q.QuattroILQR(md, N, **KW).solve(x0, u0, model_phys=rows, log=log))
    for key in SOLVE_KEYS:
        assert torch.equal(het[key], out[key]), key
    iters = out["iters"].cpu().numpy()
    for b in range(B):
        n_it = int(iters[b])
        assert 1 <= n_it < log.capacity
        rec = log.rows(b, n_it + 1)
        assert np.array_equal(rec["iteration"][:n_it], np.arange(n_it)), b
        assert not rec["stamps"][n_it].any(), b             # and not one record more
        assert rec["cost"][n_it - 1, 1] == float(out["cost"][b]), b
        assert np.array_equal(rec["K"][n_it - 1], out["K"][b].cpu().numpy()), b
        assert np.array_equal(rec["x"][0, 0], np.asarray(x0[b], dtype=np.float32)), b


# ------------------------------------------------------------------------------------------------ 2. neutral rows
def _assert_neutral(md, N, x0, u0, max_iter, steps, seed):
    q = _pkg()
    B = x0.shape[0]
    neutral = np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1))
    kw = dict(KW, max_iter=max_iter)
    a, b = q.QuattroILQR(md, N, **kw), q.QuattroILQR(md, N, **kw)
    oa, ob = a.solve(x0, u0, model_phys=neutral), b.solve(x0, u0)
    for key in SOLVE_KEYS:
        assert torch.equal(oa[key], ob[key]), ("solve", key)
    dist = dev32(1e-3 * np.random.default_rng(seed).standard_normal((steps, B, md.n)))
    ma, mb = q.BatchedMPC(md, N, **kw), q.BatchedMPC(md, N, **kw)
    for rep, d in enumerate((dist, None)):
        start = x0.astype(np.float32) if rep == 0 else ra["x"][:, -1].clone()
        ra, rb = ma.run(start, steps, disturbance=d, model_phys=neutral), mb.run(start, steps, disturbance=d)
        for key in ("x", "u", "iters"):
            assert tuple(ra[key].shape) == tuple(rb[key].shape) and torch.equal(ra[key], rb[key]), ("run", rep, key)
        assert torch.equal(ma.u_warm, mb.u_warm), rep
        for name in ("K", "k", "x", "cost", "alpha_idx", "status"):
            assert torch.equal(getattr(ma.solver, name), getattr(mb.solver, name)), ("run", rep, name)


@pytest.mark.parametrize("model,integ", CASES)
def test_neutral_rows_equal_the_call_without_them(model, integ):
    """model_phys = the model's own phys for every trajectory goes through the PHYS kernels and must leave what the old entries
    leave, in solve and in run (two runs, the second continuing from the first)."""
    md, N, x0, u0, _ = _builtin(model, integ, PHYS_B[model])
    _assert_neutral(md, N, x0, u0, 40, 3, 11)


def test_neutral_rows_equal_the_call_without_them_at_257_quadrotors():
    """B = 257, N = 50 (two LDS refills of the fused sweep, 129 workgroups, the last one half empty), the default quadrotor."""
    from quattro_ilqr_amd import models
    md = models.quadrotor_model()
    B, N = 257, 50
    rng = np.random.default_rng(B)
    x0 = np.asarray(md.x_ref) + rng.uniform(-1, 1, (B, 12)) * np.array([0.5, 0.5, 0.01, 0, 0, 0, 0.2, 0.2, 0.5, 0, 0, 0])
    u0 = 2.4525 + 0.1 * rng.standard_normal((B, N, 4))
    _assert_neutral(md, N, x0, u0, 4, 3, 12)


# ------------------------------------------------------------------------------------------------ 3. closed loop
def _assert_closed_loop(md, N, x0, rows, other, **run_kw):
    """(a) the default plant: every controller's plant is its own row; (b) a plant of its own on the other integrator whose rows
    are the controllers' rolled by one, replanning every second step with feedback."""
    q = _pkg()
    B, steps = rows.shape[0], 4
    x0 = x0.astype(np.float32)
    dist = dev32(1e-3 * np.random.default_rng(100 + B).standard_normal((steps, B, md.n)))
    rows2 = np.roll(rows, 1, axis=0)
    assert not np.array_equal(rows, rows2)
    plant = md.with_(integrator=other)
    for case, kw in (("a", {}), ("b", dict(plant=plant, replan_every=2, feedback=True))):
        mpc = q.BatchedMPC(md, N, **KW)
        het = mpc.run(x0, steps, model_phys=rows, disturbance=dist, **({} if case == "a" else dict(plant_phys=rows2)), **kw)
        assert bool(torch.isfinite(het["x"]).all()) and int(het["iters"].min()) >= 1
        assert tuple(het["iters"].shape) == (B, steps if case == "a" else steps // 2)
        for b in range(B):
            one_mpc = q.BatchedMPC(_with_row(md, rows[b]), N, **KW)
            extra = {} if case == "a" else dict(kw, plant=_with_row(md, rows[b]).with_(integrator=other), plant_phys=rows2[b:b + 1])
            one = one_mpc.run(x0[b:b + 1], steps, disturbance=dist[:, b:b + 1].contiguous(), **extra, **run_kw)
            for key in ("x", "u", "iters"):
                assert torch.equal(het[key][b:b + 1], one[key].to(het[key].dtype)), (case, b, key)
            assert torch.equal(mpc.u_warm[b:b + 1], one_mpc.u_warm), (case, b)
        if case == "a":
            # the default plant is the controller's row: the first plant step is ops.track on the controller's own first solve
            sol = q.QuattroILQR(md, N, **KW).solve(x0, model_phys=rows)
            xt, ut = q.ops.track(md, dev32(x0), sol["x"], sol["u"], sol["K"], 1, plant_phys=rows, feedback=False,
                                 disturbance=dist[:1].contiguous())
            assert torch.equal(xt[:, 1], het["x"][:, 1]) and torch.equal(ut[:, 0], het["u"][:, 0])
            # ... and not the shared block's, except where the row is the shared set
            xs, _ = q.ops.track(md, dev32(x0), sol["x"], sol["u"], sol["K"], 1, feedback=False, disturbance=dist[:1].contiguous())
            own = np.asarray(md.phys, dtype=np.float32)
            for b in range(B):
                assert torch.equal(xs[b, 1], het["x"][b, 1]) == np.array_equal(rows[b], own), b


@pytest.mark.parametrize("model,integ", CASES)
def test_closed_loop_equals_per_controller_runs(model, integ):
    """Quadrotor B = 3 (a full workgroup and a half-empty one), cart-pole B = 6 (a full row group and half of one), N = 26, four
    plant steps with a disturbance; `x`, `u`, `iters` and the warm start left behind, bit for bit."""
    md, N, x0, _, rows = _builtin(model, integ, 3 if model == "quadrotor" else 6)
    _assert_closed_loop(md, N, x0, rows, "rk4" if integ == "euler" else "euler")


def test_user_model_closed_loop_equals_per_controller_runs():
    md, N, x0, _, rows = _planar(seed=9)
    _assert_closed_loop(md, N, x0, rows, "euler", device_loop="always")


# ------------------------------------------------------------------------------------------------ 4. fp64 oracle
@pytest.mark.parametrize("model,integ", CASES)
def test_first_iteration_of_every_row_against_the_oracle(model, integ):
    """The form of test_solve_against_the_oracle_at_skewed_parameters, for every row at that row's parameters: gains of the first
    iteration against linearize_analytic + riccati_sweep_batched (rel_fro < param_cases.BOUNDS["K"] = 5e-6) and the accepted
    step against the fp64 line search.  The rows move K by 2e-2 and more (tests/test_model_phys_cpu.py): a kernel that reads
    another row, or the shared block, misses the bound by three orders of magnitude."""
    q = _pkg()
    md, N, x0, u0, rows = _builtin(model, integ, PHYS_B[model])
    out = _snap(q.QuattroILQR(md, N, **dict(KW, max_iter=1)).solve(x0, u0, model_phys=rows))
    assert int(out["status"].abs().sum()) == 0
    errs = []
    for b in range(rows.shape[0]):
        ref = oracle_first_iteration(model, integ, rows[b], x0[b:b + 1], u0[b:b + 1])
        eK, ek = rel_fro(f64(out["K"][b]), ref["K"]), rel_fro(f64(out["k"][b]), ref["k"])
        print(f"[model_phys vs oracle {model} {integ}] row {b}: K {eK:.1e} k {ek:.1e} alpha device {float(out['alpha'][b])} "
              f"oracle {ref['alpha']}")
        errs.append((b, eK, ek, float(out["alpha"][b]), ref["alpha"]))
    for b, eK, ek, a_dev, a_ref in errs:
        assert eK < pc.BOUNDS["K"] and ek < pc.BOUNDS["k"], (b, eK, ek)
        assert abs(a_dev - a_ref) < 1e-7, (b, a_dev, a_ref)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_modes_without_a_device_resident_loop_refuse_model_phys():
    """A predictor, device_loop=False and use_graph=True: NotImplementedError before the solver has allocated anything."""
    import os
    q = _pkg()
    from quattro_ilqr_amd import models
    md = models.cartpole_model(dt=0.01, integrator="euler")
    tf = q.TransformerILQR(4, 5, device=DEV).load(os.path.join(GOLDEN, "tf_weights_cartpole.npz"))
    B, N = 3, 30
    x0 = np.zeros((B, 4), dtype=np.float32)
    rows = np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1))
    for kw in (dict(tf=tf), dict(device_loop=False, tf_window=0), dict(use_graph=True, tf_window=0)):
        solver = q.QuattroILQR(md, N, max_iter=3, device=DEV, **kw)
        with pytest.raises(NotImplementedError, match="device-resident loop"):
            solver.solve(x0, model_phys=rows)
        assert solver._B is None
        mpc = q.BatchedMPC(md, N, max_iter=3, device=DEV, **{k_: v for k_, v in kw.items() if k_ in ("tf", "tf_window")})
        if "tf" in kw:
            with pytest.raises(NotImplementedError, match="device-resident loop"):
                mpc.run(x0, 2, model_phys=rows)
        with pytest.raises(NotImplementedError, match="device-resident loop"):
            mpc.run(x0, 2, model_phys=rows, device_loop=False)
        assert mpc.solver._B is None
