"""Reference rows (quattro_ilqr_solve_ref_f32, quattro_mpc_run_ref_f32; `targets=` of QuattroILQR.solve, BatchedMPC.control_step and
BatchedMPC.run): the row rule on the host, the seeded references, and the fp64 reference for a target that moves.  A plain helper
module (like tests/param_cases.py), used by tests/test_ref_rows_cpu.py and tests/test_ref_rows_gpu.py.

The fp64 reference is the UNCHANGED oracle, in two forms.
  * augmented_optimize: oracle.ilqr.optimize on the clock-augmented problem.  The state is (x, tau) with f_aug = (f(x, u), tau + 1);
    the costs read ref[min(round(tau), R - 1)].  The reference's finite differences (eps 1e-5) see a zero derivative in tau, so
    the extra column of K is zero and Q_uu, k and the x part of K are those of the time-varying problem.
  * composed_blocks: oracle.linearize.step_jac / stage_cost_derivs / terminal_derivs on dataclasses.replace(spec, x_ref=...) --
    the stage functions broadcast an (S, n) reference over the time axis -- for oracle.ilqr.riccati_sweep_batched.
The one loop written here, solve_windowed, is param_cases.solve_emulated with these blocks: the CPU tests use it for what the
inputs do over a whole solve (pivots, pitch), never as a reference for the device."""
import dataclasses

import numpy as np

import param_cases as pc
from oracle import ilqr as o_ilqr
from oracle import linearize as o_lin
from oracle import models as o_models

ALPHAS = o_ilqr.LINE_SEARCH_ALPHAS


# ---------------------------------------------------------------------------------------------------------------- the row rule
def row_index(s, t, preview, R):
    """Horizon step t of the plan that starts at plant step s reads row min(s + preview * t, R - 1); a plain solve is s = 0,
    preview = 1."""
    return min(int(s) + int(preview) * int(t), R - 1)


def window(rows, N, s=0, preview=1):
    """rows (B, R, n) -> (B, N + 1, n): the rows horizon steps 0 .. N of the plan that starts at plant step s read."""
    rows = np.asarray(rows)
    return rows[:, [row_index(s, t, preview, rows.shape[1]) for t in range(N + 1)]]


# ---------------------------------------------------------------------------------------------------------------- seeded references
# Per-step increments of the reference (per trajectory b scaled by 1 + 0.3 b) and the offset between the goals of neighbouring
# trajectories: a ramp of a few centimetres per step in position plus a yaw and a velocity component (quadrotor), cart position
# and pole angle (cart-pole), both positions and the pitch (planar user model).  Large enough that a row read one step early or
# late, or from the neighbouring trajectory, moves k and the cost by far more than 100 x the GPU bounds (tests/test_ref_rows_cpu.py
# measures it), small enough that the solves stay where the skew inputs keep them (pitch clear of the singularity).
STEP = {
    "quadrotor": np.array([0.03, -0.02, 0.025, 0.01, 0.0, 0.0, 0.0, 0.0, 0.02, 0.0, 0.0, 0.0]),
    "cartpole": np.array([0.03, 0.0, 0.015, 0.0]),
    "planar": np.array([0.03, 0.02, 0.01, 0.0, 0.0, 0.0]),
}
OFFSET = {
    "quadrotor": np.array([0.05, 0.04, -0.03, 0.0, 0.02, 0.0, 0.0, 0.0, 0.05, 0.0, 0.0, 0.0]),
    "cartpole": np.array([0.05, 0.0, 0.02, 0.0]),
    "planar": np.array([0.05, -0.04, 0.02, 0.0, 0.0, 0.0]),
}


def ref_rows(name, base, B, R):
    """(B, R, n) float32: row t of trajectory b is base + (b + 1) OFFSET + t (1 + 0.3 b) STEP.  base: the model's own x_ref, which
    no row equals."""
    b = np.arange(B, dtype=np.float64)[:, None, None]
    t = np.arange(R, dtype=np.float64)[None, :, None]
    rows = np.asarray(base, dtype=np.float64)[None, None, :] + (b + 1.0) * OFFSET[name] + t * (1.0 + 0.3 * b) * STEP[name]
    return rows.astype(np.float32)


def inputs(model, N, B, seed=pc.SEED):
    """x0 (B, n), u (B, N, m) about the skew set, rounded to fp32 and handed back as fp64 (param_cases.inputs' convention).  The
    quadrotor starts closer to level than param_cases.inputs puts it (angles 0.1, body rates 0.5 rad/s, no control held on the
    barrier): its horizons here are 20 and 37 steps of dt = 0.02, and those starts tumble past the Euler-angle singularity
    within 0.4 s."""
    p = pc.SETS[model]["skew"]
    n, m = pc.DIMS[model]
    rng = np.random.default_rng(seed + N)
    x_ref = np.asarray(p["x_ref"], dtype=np.float64)
    if model == "quadrotor":
        spread = np.array([.3, .3, .3, .3, .3, .3, .1, .1, .3, .5, .5, .5])
        x0 = x_ref + spread * rng.standard_normal((B, n))
        u = p["phys"]["mass"] * p["phys"]["gravity"] / 4.0 + 0.2 * rng.standard_normal((B, N, m))
    else:
        x0 = x_ref + pc.CART_SPREAD * rng.standard_normal((B, n))
        u = pc.CART_U["skew"][0] + pc.CART_U["skew"][1] * rng.standard_normal((B, N, m))
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
    return f32(x0), f32(u)


def neutral_rows(base, B, R):
    return np.tile(np.asarray(base, dtype=np.float32)[None, None, :], (B, R, 1))


def skew_rows(model, B, R):
    return ref_rows(model, pc.SETS[model]["skew"]["x_ref"], B, R)


# ---------------------------------------------------------------------------------------------------------------- composed blocks
def _with_ref(spec, ref):
    return dataclasses.replace(spec, x_ref=np.asarray(ref, dtype=np.float64))


def composed_cost(spec, win, xs, u):
    """Total cost of sequences xs (B, N+1, n), u (B, N, m) against the window win (B, N+1, n): (B,)."""
    N = u.shape[1]
    return (np.sum(o_lin.stage_cost(_with_ref(spec, win[:, :N]), xs[:, :N], u), axis=1)
            + o_lin.terminal_cost(_with_ref(spec, win[:, N]), xs[:, N]))


def composed_blocks(spec, win, xs, u):
    """The derivative blocks oracle.linearize.linearize_analytic returns, with the cost blocks of step t taken against win[:, t]
    and the terminal pair against win[:, N]."""
    N = u.shape[1]
    _, A, Bm = o_lin.step_jac(spec, xs[:, :N], u)
    lx, lu, lxx, luu, lux = o_lin.stage_cost_derivs(_with_ref(spec, win[:, :N]), xs[:, :N], u)
    VxN, VxxN = o_lin.terminal_derivs(_with_ref(spec, win[:, N]), xs[:, N])
    return dict(A=A, B=Bm, lx=lx, lu=lu, lxx=lxx, luu=luu, lux=lux, VxN=VxN, VxxN=VxxN)


def first_iteration(spec, win, x0, u0):
    """fp64: the first iLQR iteration of a batch against its windows: cost of the nominal, gains, Q_uu + reg I of every step, the
    step the line search accepts per trajectory (-1: none) and the relative margin |J_alpha - J_0| / J_0 of every candidate tried
    on the way."""
    xs, _ = o_lin.rollout_batched(spec, x0, u0)
    J0 = composed_cost(spec, win, xs, u0)
    quu = np.zeros(u0.shape[:2] + (spec.m, spec.m))
    k, K = o_ilqr.riccati_sweep_batched(composed_blocks(spec, win, xs, u0), quu_out=quu)
    B = x0.shape[0]
    alpha, margins = np.full(B, -1.0), [[] for _ in range(B)]
    for a in ALPHAS:
        nx, nu, _ = o_lin.closed_loop_rollout_batched(spec, x0, xs, u0, k, K, a)
        Jc = composed_cost(spec, win, nx, nu)
        for b in range(B):
            if alpha[b] < 0:
                margins[b].append(abs(float(Jc[b] - J0[b])) / float(J0[b]))
                if Jc[b] <= J0[b]:
                    alpha[b] = a
    return dict(xs=xs, cost=J0, K=K, k=k, quu=quu, alpha=alpha, margins=margins)


# ---------------------------------------------------------------------------------------------------------------- augmented problem
def augmented(spec, ref):
    """(f_aug, L_aug, Lf_aug) of the clock-augmented problem for ONE trajectory's rows ref (R, n)."""
    ref = np.asarray(ref, dtype=np.float64)
    specs = [_with_ref(spec, r) for r in ref]

    def at(tau):
        return specs[min(int(round(float(tau))), len(specs) - 1)]

    def f(z, u):
        return np.concatenate([o_models.discrete_step(spec, z[:-1], u), [z[-1] + 1.0]])

    def L(z, u):
        return o_models.running_cost(at(z[-1]), z[:-1], u)

    def Lf(z):
        return o_models.final_cost(at(z[-1]), z[:-1])

    return f, L, Lf


def augmented_optimize(spec, ref, x0, u0, tau0=0.0, max_iter=pc.SOLVE_MAX_ITER, tol=pc.SOLVE_TOL):
    """oracle.ilqr.optimize on the clock-augmented problem of one trajectory -> (u (N, m), x (N+1, n), cost, iterations, logs).
    tau0: the clock at the start of the horizon (the plan's plant step under preview)."""
    f, L, Lf = augmented(spec, ref)
    z0 = np.concatenate([np.asarray(x0, dtype=np.float64), [float(tau0)]])
    u, z, logs = o_ilqr.optimize(f, L, Lf, z0, list(u0), u0.shape[0], max_iter=max_iter, tol=tol)
    return np.array(u), z[:, :-1], float(o_ilqr.trajectory_cost(L, Lf, z, u)), len(logs), logs


def solve_windowed(spec, win, x0, u0, dtype=np.float64, max_iter=pc.SOLVE_MAX_ITER, tol=pc.SOLVE_TOL):
    """param_cases.solve_emulated for a batch against its windows (exact derivatives, `dtype` storage): -> u, x, cost, iterations
    per trajectory, the smallest unpivoted pivot ratio of Q_uu + reg I met on the way and the largest |x[..., 7]| (the
    quadrotor's pitch)."""
    r = lambda a: np.asarray(a).astype(dtype).astype(np.float64)
    B = x0.shape[0]
    u = r(u0)
    xs = r(o_lin.rollout_batched(spec, x0, u)[0])
    J = composed_cost(spec, win, xs, u)
    active, its, pivot, pitch = np.ones(B, dtype=bool), np.zeros(B, dtype=int), np.inf, 0.0
    for _ in range(max_iter):
        if not active.any():
            break
        its += active
        blocks = composed_blocks(spec, win, xs, u)
        quu = np.zeros(u.shape[:2] + (spec.m, spec.m))
        k, K = o_ilqr.riccati_sweep_batched({k_: v.astype(dtype) for k_, v in blocks.items()}, dtype=dtype, quu_out=quu)
        k, K = k.astype(np.float64), K.astype(np.float64)
        pivot = min(pivot, pc.unpivoted_pivot_ratio(quu[active]))
        found = np.zeros(B, dtype=bool)
        nxs, nus, nJ = xs.copy(), u.copy(), J.copy()
        for a in ALPHAS:
            cx, cu, _ = o_lin.closed_loop_rollout_batched(spec, x0, xs, u, k, K, a)
            cx, cu = r(cx), r(cu)
            cJ = composed_cost(spec, win, cx, cu)
            take = active & ~found & (cJ <= J)
            nxs[take], nus[take], nJ[take] = cx[take], cu[take], cJ[take]
            found |= take
        dJ = np.abs(J - nJ)
        xs, u, J = nxs, nus, nJ
        active &= found & ~(dJ < tol)
        if spec.n == 12:
            pitch = max(pitch, float(np.max(np.abs(xs[:, :, 7]))))
    return u, xs, J, its, pivot, pitch


# ---------------------------------------------------------------------------------------------------------------- whole solves
# Whole solves are compared with oracle.ilqr.optimize's own result in the form of param_cases' whole-solve comparison, and the bounds
# are made the way param_cases makes its own: E is what the same algorithm with exact derivatives and fp32 storage differs from
# optimize() by on the CPU, worst over both integrators and every compared trajectory (tests/test_ref_rows_cpu.py holds the
# emulation to these figures); asserted on the GPU: the larger of param_cases.solve_bounds and 4 x E.  Every trajectory of the
# batch is compared.
#   SOLVE_E    : the converged solve against rows of its own (R = N + 1, param_cases.SOLVE_N and its inputs), solve_windowed against
#                augmented_optimize.
#   SETPOINT_E : every plan of the set-point schedule (setpoint_loop), param_cases.solve_emulated against optimize().
# Why the cart-pole's SETPOINT_E is large in x and u and not in the cost: r = 0.004 and dt = 0.02 leave Q_uu ~ 1e-2, so the cost is
# flat along u; both solves stop on |dJ| < 1e-3, and the last line search before that often improves the cost by less than fp32
# storage perturbs it (1e-7 of a cost of 100).  Which of its candidates is taken is then decided by rounding, and the results lie
# a last Newton step apart: up to 1.6e-3 in u at costs equal to 4e-8.
SOLVE_TRAJ = {"quadrotor": (0, 1, 2), "cartpole": (0, 1, 2, 3, 4)}
SOLVE_E = {"quadrotor": dict(cost=3.0e-8, x=8.1e-6, u=4.3e-5), "cartpole": dict(cost=5.5e-9, x=1.3e-7, u=2.9e-6)}
SETPOINT_STEPS = 6
SETPOINT_TRAJ = {"quadrotor": (1, 2), "cartpole": (0, 1, 2, 3, 4)}     # (the quadrotor's 0 shares its workgroup with 1)
SETPOINT_E = {"quadrotor": dict(cost=6.0e-8, x=1.2e-5, u=1.6e-4), "cartpole": dict(cost=4.1e-8, x=7.2e-5, u=1.6e-3)}


def solve_bounds(model):
    base = pc.solve_bounds(model)
    return {key: max(base[key], 4.0 * SOLVE_E[model][key]) for key in base}


def setpoint_bounds(model):
    base = pc.solve_bounds(model)
    return {key: max(base[key], 4.0 * SETPOINT_E[model][key]) for key in base}


def setpoint_loop(model, integ, b, steps=SETPOINT_STEPS):
    """The set-point schedule of trajectory b in fp64 on the CPU: plan c is oracle.ilqr.optimize from the current state and the
    shifted warm start against row c of skew_rows (R = steps) for its whole horizon, then u_0 on the model itself.  -> per plan
    (iterations of optimize, iterations of the fp32-storage emulation from the same start, its distance from optimize's result)."""
    spec = pc.spec(model, "skew", integ)
    N, B = pc.SOLVE_N, max(SETPOINT_TRAJ[model]) + 1
    x0, _ = pc.inputs(model, "skew", N, B)
    rows = skew_rows(model, B, steps).astype(np.float64)
    x, u, out = x0[b].astype(np.float32).astype(np.float64), np.zeros((N, spec.m)), []
    for c in range(steps):
        sp = _with_ref(spec, rows[b, c])
        ref = pc.solve_optimize(sp, x, u)
        em = pc.solve_emulated(sp, x, u)
        out.append((ref[3], em[3], pc.solve_errors(em, ref)))
        x, u = sp.f(x, ref[0][0]), np.concatenate([ref[0][1:], ref[0][-1:]])
    return out
