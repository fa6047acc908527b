"""The closed loop with a plant of its own and gain feedback between solves (quattro_track_f32, quattro_mpc_run_plant_f32;
ops.track, BatchedMPC.run(plant=, plant_phys=, replan_every=, feedback=)) on the GPU:
  1. the tracked steps against the fp64 oracle's closed-loop rollout, one plant per controller;
  2. the persistent loops against the host-driven loop (solve, ops.track, shift), bit for bit;
  3. neutral options through the new kernels against the old path, bit for bit;
  4. the three C entries of a run, and of a solve, with neutral arguments against each other, bit for bit;
  5. a hybrid controller through the host loop.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_fro

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import linearize as o_lin  # noqa: E402
from oracle import models as o_models  # noqa: E402

DEV = "cuda:0"
QUAD_SPREAD = np.array([0.5, 0.5, 0.01, 0, 0, 0, 0.2, 0.2, 0.5, 0, 0, 0])


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def f64(t):
    return t.double().cpu().numpy()


def _start(model, md, B, N, rng):
    """A random start: states about the reference, controls about hover / zero."""
    if model == "quadrotor":
        return (np.asarray(md.x_ref) + rng.uniform(-1, 1, (B, 12)) * QUAD_SPREAD, 2.4525 + 0.1 * rng.standard_normal((B, N, 4)))
    x0 = np.zeros((B, 4))
    x0[:, 0] = rng.uniform(-0.5, 0.5, B)
    x0[:, 2] = rng.uniform(-0.5, 0.5, B)
    return x0, 0.3 * rng.standard_normal((B, N, 1))


def _plant_phys(model, md, B):
    """Per-controller plants: mass (pole mass) scaled by 1 + 0.2 sin(1 + b), the quadrotor's Ix by 1 + 0.2 cos b."""
    ph = np.tile(np.asarray(md.phys, dtype=np.float64), (B, 1))
    b = np.arange(B)
    ph[:, 0 if model == "quadrotor" else 1] *= 1.0 + 0.2 * np.sin(1.0 + b)
    if model == "quadrotor":
        ph[:, 1] *= 1.0 + 0.2 * np.cos(b)
    return ph.astype(np.float32)


def _nominal(md, x0, u0, N):
    """Nominal and gains of three device iterations from the start."""
    q = _pkg()
    out = q.QuattroILQR(md, N, max_iter=3, device=DEV, tf_window=0).solve(x0, u0, max_iter=3, fixed_iters=True)
    return out["x"].clone(), out["u"].clone(), out["K"].clone()


def _oracle_track(step_ref, B, x0, x_nom, u_nom, K, dist):
    """fp64 reference of the tracked steps, one plant per controller: step_ref(b, x0_b, x_nom_b, u_nom_b, K_b) is the closed-loop
    rollout of controller b's plant over the rows it is given (k = 0, alpha = 1).  Without a disturbance that is one call over
    all rows; with one, one call per step, the disturbance added in between."""
    N = u_nom.shape[1]
    xs = np.zeros((B, N + 1, x0.shape[1]))
    us = np.zeros_like(u_nom)
    for b in range(B):
        if dist is None:
            xs[b], us[b] = step_ref(b, x0[b:b + 1], x_nom[b:b + 1], u_nom[b:b + 1], K[b:b + 1])
            continue
        xs[b, 0] = x0[b]
        for j in range(N):
            nx, nu = step_ref(b, xs[b:b + 1, j], x_nom[b:b + 1, j:j + 2], u_nom[b:b + 1, j:j + 1], K[b:b + 1, j:j + 1])
            xs[b, j + 1] = nx[1] + dist[j, b]
            us[b, j] = nu[0]
    return xs, us


TRACK_CASES = [(model, integ) for model in ("quadrotor", "cartpole") for integ in ("euler", "rk4")]


@pytest.mark.parametrize("model,integ", TRACK_CASES)
def test_track_against_the_oracle_with_one_plant_per_controller(model, integ):
    """ops.track against oracle.linearize.closed_loop_rollout_batched(plant_spec_b, x0, x_nom, u_nom, k = 0, K * feedback,
    alpha = 1), one call per controller with that controller's physical parameters; the plant integrates with the OTHER
    scheme than the model.  B = 19 quadrotors (a full wave of 16 and a ragged one) / 67 cart-poles (a block and three lanes),
    N = 12, 1 / 5 / 12 tracked steps, with and without disturbance, feedback on and off.  Bound: rel_fro < 1e-5 on x and u, the
    bound test_short_and_odd_horizons_against_the_oracle holds the same closed-loop step to.

    Quadrotor, what the gains are for: max|x - x_nom| at step 8, taken over all 19 trajectories, is smaller with feedback than
    with the open-loop hold (fp64 oracle on this configuration: 0.18 against 0.09).  The ordering is asserted on that maximum
    and not on each trajectory alone, because the fp64 oracle itself does not show it on each: trajectories 2 and 18, whose
    plants are within 3 % of the model's mass, leave the nominal by little more than the 1e-2 start offset when held open-loop
    (0.014, 0.017), while the gains trade that position offset for a larger climb rate (0.025, 0.028, both in vz); five seeds,
    two starts and both integrators gave such a trajectory in 35 of 40 oracle runs.  Per trajectory the device must instead
    order the two as the oracle does; the oracle's gap is checked to exceed what the rel_fro bound lets the device move."""
    q = _pkg()
    from quattro_ilqr_amd import models, ops
    N = 12
    B = 19 if model == "quadrotor" else 67
    other = "rk4" if integ == "euler" else "euler"
    md = models.model_by_name(model, integrator=integ)
    plant = md.with_(integrator=other)
    rng = np.random.default_rng(B + (integ == "rk4"))
    x0r, u0r = _start(model, md, B, N, rng)
    x_nom, u_nom, K = _nominal(md, x0r, u0r, N)
    x0 = (x_nom[:, 0] + dev32(1e-2 * rng.standard_normal((B, md.n)))).contiguous()
    phys = _plant_phys(model, md, B)
    dist = dev32(1e-3 * rng.standard_normal((N, B, md.n)))
    make_spec = o_models.quadrotor_spec if model == "quadrotor" else o_models.cartpole_spec
    specs = []
    for b in range(B):
        spec = make_spec(0.01, 1 if other == "rk4" else 0)
        specs.append(dataclasses.replace(spec, phys={k: float(v) for k, v in zip(spec.phys, phys[b])}))
    xn64, un64, K64, x064 = f64(x_nom), f64(u_nom), f64(K), f64(x0)
    worst = 0.0
    dev_x8, ref_x8, slack = {}, {}, 0.0
    for feedback in (True, False):
        def step_ref(b, xs0, xr, ur, Kr):
            nx, nu, _ = o_lin.closed_loop_rollout_batched(specs[b], xs0, xr, ur, np.zeros_like(ur), Kr * float(feedback), 1.0)
            return nx[0], nu[0]
        for d in (None, dist):
            x_ref, u_ref = _oracle_track(step_ref, B, x064, xn64, un64, K64, None if d is None else f64(d))
            assert np.all(np.isfinite(x_ref)) and np.all(np.isfinite(u_ref))
            for steps in (1, 5, 12):
                xt, ut = ops.track(md, x0, x_nom, u_nom, K, steps, plant=plant, plant_phys=phys, feedback=feedback,
                                   disturbance=None if d is None else d[:steps].contiguous())
                assert tuple(xt.shape) == (B, steps + 1, md.n) and tuple(ut.shape) == (B, steps, md.m)
                assert torch.equal(xt[:, 0], x0)
                ex, eu = rel_fro(f64(xt), x_ref[:, :steps + 1]), rel_fro(f64(ut), u_ref[:, :steps])
                worst = max(worst, ex, eu)
                print(f"track {model} {integ}/{other} feedback={feedback} dist={d is not None} steps={steps}: "
                      f"rel_fro x {ex:.2e} u {eu:.2e}")
                assert ex < 1e-5 and eu < 1e-5, (feedback, d is not None, steps, ex, eu)
                if steps == 12:
                    dev_x8[(feedback, d is not None)] = f64((xt[:, 8] - x_nom[:, 8]).abs().max(dim=1).values)
                    ref_x8[(feedback, d is not None)] = np.abs(x_ref[:, 8] - xn64[:, 8]).max(axis=1)
                    slack = max(slack, 1e-5 * float(np.linalg.norm(x_ref)))      # how far the bound lets an element of x move
    print(f"track {model} {integ}: worst rel_fro {worst:.2e}")
    # the plant mismatch is there, and the per-controller rows are used: controller b's plant is not controller 0's
    x_one, _ = ops.track(md, x0, x_nom, u_nom, K, 12, plant=plant, plant_phys=np.tile(phys[:1], (B, 1)), feedback=True)
    x_all, _ = ops.track(md, x0, x_nom, u_nom, K, 12, plant=plant, plant_phys=phys, feedback=True)
    assert torch.equal(x_one[0], x_all[0]) and not torch.equal(x_one[1:], x_all[1:])
    if model == "quadrotor":
        # what the gains are for: feedback holds the plants closer to the nominal than the open-loop hold (see the docstring)
        for has_d in (False, True):
            fb, ol = dev_x8[(True, has_d)], dev_x8[(False, has_d)]
            fb_ref, ol_ref = ref_x8[(True, has_d)], ref_x8[(False, has_d)]
            print(f"max|x - x_nom| at step 8 (dist={has_d}): open loop {ol.max():.3f}, feedback {fb.max():.3f}; feedback closer "
                  f"on {int((fb < ol).sum())} of {B} trajectories, in the oracle on {int((fb_ref < ol_ref).sum())}")
            assert fb.max() < ol.max(), (has_d, fb, ol)
            # the oracle's gap is 1.8e-3 or more on every trajectory, the slack about 1e-4: no ordering is left to round-off
            assert bool((np.abs(fb_ref - ol_ref) > 2.0 * slack).all()), (has_d, fb_ref, ol_ref, slack)
            assert np.array_equal(fb < ol, fb_ref < ol_ref), (has_d, fb, ol, fb_ref, ol_ref)


def test_track_user_model_against_an_fp64_restatement():
    """The prebuilt planar RK4 model (tests/test_user_model_gpu.py), B = 3, whose phys are the model's free parameters: plant
    mass scaled per controller, plant on Euler; the fp64 reference restates the planar rate with phys as an argument."""
    from test_user_model_gpu import DT, PHYS, planar_batch, planar_model
    from quattro_ilqr_amd import ops
    md = planar_model("rk4")
    plant = md.with_(integrator="euler")
    B, N = 3, 12
    x0r, u0r = planar_batch(B, N, 5)
    x_nom, u_nom, K = _nominal(md, x0r, u0r, N)
    rng = np.random.default_rng(17)
    x0 = (x_nom[:, 0] + dev32(1e-2 * rng.standard_normal((B, 6)))).contiguous()
    phys = np.tile(np.asarray(PHYS, dtype=np.float64), (B, 1))
    phys[:, 0] *= 1.0 + 0.2 * np.sin(1.0 + np.arange(B))
    phys = phys.astype(np.float32)
    dist = dev32(1e-3 * rng.standard_normal((N, B, 6)))

    def rate(ph, x, u):
        m, inertia, arm, g = ph
        th = (u[0] + u[1]) / m
        return np.array([x[3], x[4], x[5], -th * np.sin(x[2]), th * np.cos(x[2]) - g, (u[0] - u[1]) * (arm / inertia)])

    xn, un, Kn, x064, d64 = f64(x_nom), f64(u_nom), f64(K), f64(x0), f64(dist)
    for feedback in (True, False):
        for d in (None, d64):
            x_ref, u_ref = np.zeros((B, N + 1, 6)), np.zeros((B, N, 2))
            for b in range(B):
                ph = phys[b].astype(np.float64)
                x = x064[b].copy()
                x_ref[b, 0] = x
                for j in range(N):
                    u = un[b, j] + (Kn[b, j] @ (x - xn[b, j]) if feedback else 0.0)
                    x = x + DT * rate(ph, x, u) + (0.0 if d is None else d[j, b])        # the plant integrates with Euler
                    x_ref[b, j + 1], u_ref[b, j] = x, u
            for steps in (1, 5, 12):
                xt, ut = ops.track(md, x0, x_nom, u_nom, K, steps, plant=plant, plant_phys=phys, feedback=feedback,
                                   disturbance=None if d is None else dist[:steps].contiguous())
                ex, eu = rel_fro(f64(xt), x_ref[:, :steps + 1]), rel_fro(f64(ut), u_ref[:, :steps])
                print(f"track planar feedback={feedback} dist={d is not None} steps={steps}: rel_fro x {ex:.2e} u {eu:.2e}")
                assert ex < 1e-5 and eu < 1e-5, (feedback, d is not None, steps, ex, eu)


# ------------------------------------------------------------------------------------------------ persistent against host-driven
def _loops_agree(md, plant, phys, x0, N, hold, device_loop, dim, **mpc_kw):
    """Two plans with a disturbance and per-controller plants, then a second run that continues from the first, feedback on and
    off: the persistent loop (a) and the host-driven loop (b) leave the same bits everywhere."""
    q = _pkg()
    B, steps = x0.shape[0], 2 * hold
    rng = np.random.default_rng(1000 * N + hold)
    dist = dev32(1e-3 * rng.standard_normal((steps, B, dim)))
    for feedback in (True, False):
        a = q.BatchedMPC(md, N, max_iter=3, tol=1e-3, device=DEV, check_every=1, **mpc_kw)
        b = q.BatchedMPC(md, N, max_iter=3, tol=1e-3, device=DEV, check_every=1, **mpc_kw)
        for rep, d in enumerate((dist, None)):
            start = x0 if rep == 0 else oa["x"][:, -1].clone()
            kw = dict(disturbance=d, plant=plant, plant_phys=phys, replan_every=hold, feedback=feedback)
            oa = a.run(start, steps, device_loop=device_loop, **kw)
            ob = b.run(start, steps, device_loop=False, **kw)
            assert tuple(oa["x"].shape) == (B, steps + 1, dim) and tuple(oa["iters"].shape) == (B, 2)
            for key in ("x", "u", "iters"):
                assert torch.equal(oa[key], ob[key].to(oa[key].dtype)), (feedback, rep, key)
            assert torch.equal(a.u_warm, b.u_warm), (feedback, rep)
            for name in ("K", "k", "x", "cost", "alpha_idx", "status"):
                assert torch.equal(getattr(a.solver, name), getattr(b.solver, name)), (feedback, rep, name)
            assert torch.equal(oa["x"][:, 0], torch.as_tensor(start, device=DEV))
            assert bool(torch.isfinite(oa["x"]).all()) and int(oa["iters"].min()) >= 1
        if feedback:
            x_fb = oa["x"].clone()
        elif hold > 1:
            assert not torch.equal(x_fb, oa["x"])          # the flag does something


@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("N,hold", [(6, 6), (6, 4), (50, 5), (70, 3)])
def test_quadrotor_persistent_plant_loop_equals_host_driven_loop(integ, N, hold):
    """B = 3 leaves a half-empty workgroup; hold = N, hold < N, and N = 70, past the 65 steps the warm start shifts in one pass."""
    from quattro_ilqr_amd import models
    md = models.quadrotor_model(integrator=integ)
    plant = md.with_(integrator="rk4" if integ == "euler" else "euler")
    B = 3
    rng = np.random.default_rng(N + hold)
    x0 = (np.asarray(md.x_ref) + rng.uniform(-1, 1, (B, 12)) * QUAD_SPREAD).astype(np.float32)
    _loops_agree(md, plant, _plant_phys("quadrotor", md, B), x0, N, hold, True, 12, tf_window=0)


@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("N,hold", [(1, 1), (3, 3), (30, 7)])
def test_cartpole_persistent_plant_loop_equals_host_driven_loop(integ, N, hold):
    from quattro_ilqr_amd import models
    md = models.cartpole_model(dt=0.01, integrator=integ)
    plant = md.with_(integrator="rk4" if integ == "euler" else "euler")
    B = 6
    x0, _ = _start("cartpole", md, B, N, np.random.default_rng(3 * N + hold))
    _loops_agree(md, plant, _plant_phys("cartpole", md, B), x0.astype(np.float32), N, hold, True, 4, tf_window=0)


def test_user_model_persistent_plant_loop_equals_host_driven_loop():
    from test_user_model_gpu import PHYS, planar_batch, planar_model
    md = planar_model("rk4")
    plant = md.with_(integrator="euler")
    B, N, hold = 3, 12, 4
    x0, _ = planar_batch(B, N, 9)
    phys = np.tile(np.asarray(PHYS, dtype=np.float64), (B, 1))
    phys[:, 0] *= 1.0 + 0.2 * np.sin(1.0 + np.arange(B))
    _loops_agree(md, plant, phys.astype(np.float32), x0.astype(np.float32), N, hold, "always", 6, tf_window=0)


# ------------------------------------------------------------------------------------------------ neutral options
@pytest.mark.parametrize("model,B,N", [("quadrotor", 257, 50), ("cartpole", 130, 30)])
def test_neutral_plant_options_through_the_new_kernel_equal_the_old_path(model, B, N):
    """run(plant=model, replan_every=1) takes quattro_mpc_run_plant_f32 — the PLANT kernels, one tracked step per plan on a plant
    that is the model — and must leave what run() leaves through quattro_mpc_run_f32, bit for bit."""
    q = _pkg()
    from quattro_ilqr_amd import models
    md = models.model_by_name(model)
    steps = 3
    rng = np.random.default_rng(B)
    x0, _ = _start(model, md, B, N, rng)
    x0 = x0.astype(np.float32)
    dist = dev32(1e-3 * rng.standard_normal((steps, B, md.n)))
    a = q.BatchedMPC(md, N, max_iter=4, tol=1e-3, device=DEV)
    b = q.BatchedMPC(md, N, max_iter=4, tol=1e-3, device=DEV)
    for rep, d in enumerate((dist, None)):
        start = x0 if rep == 0 else oa["x"][:, -1].clone()
        oa = a.run(start, steps, disturbance=d, plant=md, replan_every=1)
        ob = b.run(start, steps, disturbance=d)
        for key in ("x", "u", "iters"):
            assert tuple(oa[key].shape) == tuple(ob[key].shape) and torch.equal(oa[key], ob[key]), (rep, key)
        assert torch.equal(a.u_warm, b.u_warm)
        for name in ("K", "k", "x", "cost", "alpha_idx", "status"):
            assert torch.equal(getattr(a.solver, name), getattr(b.solver, name)), (rep, name)
    # feedback with one step per plan adds exactly nothing: x_cur == x_nom[0]
    c = q.BatchedMPC(md, N, max_iter=4, tol=1e-3, device=DEV)
    oc = c.run(x0, steps, disturbance=dist, feedback=True)
    od = q.BatchedMPC(md, N, max_iter=4, tol=1e-3, device=DEV).run(x0, steps, disturbance=dist)
    assert torch.equal(oc["x"], od["x"]) and torch.equal(oc["u"], od["u"])


# ------------------------------------------------------------------------------------------------ the entries against each other
class _LoopState:
    """Every array a device-resident run reads or writes, freshly zeroed but for the start: three of these, one per C entry, must
    hold the same bits afterwards."""
    OUTPUTS = ("x_cur", "x", "u", "K", "k", "cost", "alpha_idx", "active", "iters", "status", "traj_x", "traj_u", "traj_it")

    def __init__(self, md, x0, u0, steps):
        from quattro_ilqr_amd import ops
        B, N, n, m = x0.shape[0], u0.shape[1], md.n, md.m
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
        self.x0, self.x_cur, self.u = dev32(x0), dev32(x0), dev32(u0)
        self.x, self.K, self.k = z((B, N + 1, n)), z((B, N, m, n)), z((B, N, m))
        self.cost = z((B,), torch.float64)
        self.alpha_idx, self.active, self.iters, self.status = (z((B,), torch.int32) for _ in range(4))
        self.traj_x, self.traj_u, self.traj_it = z((B, steps + 1, n)), z((B, steps, m)), z((B, steps), torch.int32)
        self.ws = ops.workspace(md, B, N, DEV)

    def same_as(self, other):
        return [name for name in self.OUTPUTS if not torch.equal(getattr(self, name), getattr(other, name))]


ENTRY_CASES = [("quadrotor", "euler", 3, 6), ("quadrotor", "rk4", 3, 6), ("cartpole", "euler", 5, 3), ("cartpole", "rk4", 5, 3)]


@pytest.mark.parametrize("model,integ,B,N", ENTRY_CASES)
def test_the_three_entries_of_a_run_and_of_a_solve_leave_the_same_bits(model, integ, B, N):
    """The C entries themselves, below ops: quattro_mpc_run_f32, quattro_mpc_run_plant_f32
    with the neutral arguments (no plant, no rows, hold 1, no feedback) and quattro_mpc_run_phys_f32 with NULL rows on top run
    2 control steps of at most 3 iterations with a disturbance; quattro_ilqr_solve_f32, quattro_ilqr_solve_logged_f32 with a NULL
    log and quattro_ilqr_solve_phys_f32 with NULL rows solve the same start.  Every output of the three must be equal, bit for
    bit.  B = 3 quadrotors leave a half-empty workgroup, B = 5 cart-poles a wave of four rows and a wave of one."""
    from quattro_ilqr_amd import _lib, models, ops
    md = models.model_by_name(model, integrator=integ)
    lib = _lib.load_for(md)
    steps, max_iter, tol = 2, 3, 1e-3
    rng = np.random.default_rng(B + N + (integ == "rk4"))
    x0, u0 = _start(model, md, B, N, rng)
    dist = dev32(1e-3 * rng.standard_normal((steps, B, md.n)))

    def run(entry, *extra):
        t = _LoopState(md, x0, u0, steps)
        head, keep = ops._mpc_args(md, t.x_cur, t.x, t.u, t.K, t.k, t.cost, tol, max_iter, steps, t.ws, t.traj_x, t.traj_u,
                                   t.traj_it, dist, ops.ALPHAS, ops.QUU_REG, t.alpha_idx, t.active, t.iters, t.status)
        assert getattr(lib, entry)(*head, *extra, ops._stream()) == _lib.QUATTRO_OK, entry
        torch.cuda.synchronize()
        return t

    plain = run("quattro_mpc_run_f32")
    assert bool(torch.isfinite(plain.traj_x).all()) and int(plain.traj_it.min()) >= 1      # the run ran
    assert torch.equal(plain.traj_x[:, 0], plain.x0) and torch.equal(plain.traj_x[:, -1], plain.x_cur)
    assert not torch.equal(plain.traj_x[:, 1], plain.traj_x[:, 0]) and not torch.equal(plain.u, dev32(u0))
    assert plain.same_as(run("quattro_mpc_run_plant_f32", None, None, 1, 0)) == []
    assert plain.same_as(run("quattro_mpc_run_phys_f32", None, None, 1, 0, None)) == []

    def solve(entry, *extra):
        t = _LoopState(md, x0, u0, steps)
        arr, na = ops._alphas(ops.ALPHAS)
        p = md.c_params()
        flags = _lib.SOLVE_SIMULATE | _lib.SOLVE_RESET
        rc = getattr(lib, entry)(ctypes.byref(p), ops._ptr(t.x0), ops._ptr(t.x), ops._ptr(t.u), B, N, ops.QUU_REG, arr, na, tol,
                                 max_iter, flags, ops._ptr(t.K), ops._ptr(t.k), ops._ptr(t.cost), ops._ptr(t.alpha_idx),
                                 ops._ptr(t.active), ops._ptr(t.iters), ops._ptr(t.status), ops._ptr(t.ws),
                                 t.ws.numel() * t.ws.element_size(), *extra, ops._stream())
        assert rc == _lib.QUATTRO_OK, entry
        torch.cuda.synchronize()
        return t

    plain = solve("quattro_ilqr_solve_f32")
    assert bool(torch.isfinite(plain.K).all()) and int(plain.iters.min()) >= 1 and float(plain.cost.min()) > 0.0
    assert plain.same_as(solve("quattro_ilqr_solve_logged_f32", None)) == []
    assert plain.same_as(solve("quattro_ilqr_solve_phys_f32", None, None)) == []


# ------------------------------------------------------------------------------------------------ hybrid controller
def test_hybrid_controller_gets_the_plant_loop_through_the_host():
    """With a predictor there is no persistent kernel: the run is solve, ops.track, shift on the host.  One small run completes,
    and the controls applied in its last plan are ops.track on the state the solver holds after it."""
    q = _pkg()
    from quattro_ilqr_amd import models, ops
    tf = q.TransformerILQR(4, 5, device=DEV).load(os.path.join(GOLDEN, "tf_weights_cartpole.npz"))
    md = models.cartpole_model(dt=0.01, integrator="euler")
    plant = md.with_(integrator="rk4")
    B, N, hold, steps = 3, 30, 3, 6
    x0, _ = _start("cartpole", md, B, N, np.random.default_rng(2))
    phys = _plant_phys("cartpole", md, B)
    dist = dev32(1e-3 * np.random.default_rng(4).standard_normal((steps, B, 4)))
    mpc = q.BatchedMPC(md, N, max_iter=3, tol=1e-1, tf=tf, device=DEV, check_every=1)
    out = mpc.run(x0.astype(np.float32), steps, disturbance=dist, plant=plant, plant_phys=phys, replan_every=hold, feedback=True)
    assert tuple(out["x"].shape) == (B, steps + 1, 4) and tuple(out["u"].shape) == (B, steps, 1)
    assert tuple(out["iters"].shape) == (B, steps // hold) and bool(torch.isfinite(out["x"]).all())
    sv = mpc.solver
    xt, ut = ops.track(md, out["x"][:, steps - hold].contiguous(), sv.x, sv.u, sv.K, hold, plant=plant, plant_phys=phys,
                       feedback=True, disturbance=dist[steps - hold:].contiguous())
    assert torch.equal(ut, out["u"][:, steps - hold:]) and torch.equal(xt, out["x"][:, steps - hold:])
    u_last = sv.u
    assert torch.equal(mpc.u_warm, torch.cat([u_last[:, hold:]] + [u_last[:, -1:]] * hold, dim=1))
