"""The cost gradient (quattro_cost_gradient_f32, ops.cost_gradient, autograd.trajectory_cost, solve(want_grad=True)): the fp64
reference, the error measures, the fp32 restatement, the mutants and the bounds.  A plain helper module (like tests/param_cases.py),
used by tests/test_cost_gradient_cpu.py and tests/test_cost_gradient_gpu.py.

Reference: the adjoint recursion

    lambda_N = Lf_x(x_N);   t = N-1 .. 0:   g_t = l_u(t) + B_t^T lambda_{t+1},   lambda_t = l_x(t) + A_t^T lambda_{t+1}

in fp64 over derivative blocks about the fp32-rounded (x, u) the device is given: oracle.linearize.linearize_analytic for the
built-in models (ref_cases.composed_blocks under reference rows), the fp64 records of user_grid_cases.evaluate for user models.

Error measures (per trajectory, the largest over the batch is reported):
    costate : max_{t,i} |d lambda_{t,i}| / max_{t,i} |lambda_{t,i}|          (grad_x0 = lambda_0 under the same scale)
    grad_u  : max_{t,a} |d g_{t,a}| / (|l_u|_{t,a} + sum_i |B_t|_{ia} Lambda_i),   Lambda_i = max_t |lambda_{t,i}|
The second is deliberately not "relative to the largest entry": with the quadrotor's barrier active (u[:, ::3, 1] = -0.05 in
param_cases.inputs) the barrier's l_u is two orders of magnitude above everything else and would hide the B^T lambda term under a
per-trajectory scale.  The denominator is the size of the terms that are added to form the entry, what fp32 round-off is relative to.
"""
import numpy as np

import param_cases as pc
import ref_cases as rc
from oracle import linearize as o_lin

MUTANTS = ("A not transposed", "lambda_t in g_t", "l_x dropped", "l_u dropped", "A of step t + 1", "B of step t + 1")


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def adjoint(d, dtype=np.float64, mutant=None):
    """Blocks d (A (B,N,n,n), B (B,N,n,m), lx (B,N,n), lu (B,N,m), VxN (B,n)) -> dict(grad_u (B,N,m), grad_x0 (B,n),
    costate (B,N+1,n)) in `dtype` (float32: the blocks rounded to fp32 and the recursion in fp32, the restatement).  mutant: one of
    MUTANTS, a recursion with that mistake."""
    A, Bm, lx, lu, VxN = (np.asarray(d[key]).astype(dtype) for key in ("A", "B", "lx", "lu", "VxN"))
    Bt, N, n, m = Bm.shape
    lam = np.zeros((Bt, N + 1, n), dtype=dtype)
    g = np.zeros((Bt, N, m), dtype=dtype)
    lam[:, N] = VxN
    for t in range(N - 1, -1, -1):
        At = A[:, min(t + 1, N - 1)] if mutant == "A of step t + 1" else A[:, t]
        Bs = Bm[:, min(t + 1, N - 1)] if mutant == "B of step t + 1" else Bm[:, t]
        nxt = lam[:, t + 1]
        AT = At if mutant == "A not transposed" else At.transpose(0, 2, 1)
        lam[:, t] = np.einsum("bij,bj->bi", AT, nxt) + (0 if mutant == "l_x dropped" else lx[:, t])
        src = lam[:, t] if mutant == "lambda_t in g_t" else nxt
        g[:, t] = np.einsum("bia,bi->ba", Bs, src) + (0 if mutant == "l_u dropped" else lu[:, t])
    return dict(grad_u=g, grad_x0=lam[:, 0].copy(), costate=lam)


def errors(got, ref, d):
    """got, ref: dicts of adjoint()'s keys (got may lack grad_x0 / costate); d: the fp64 blocks ref was made from.  -> dict of the
    measures above, the largest over the batch."""
    lam = np.asarray(ref["costate"], dtype=np.float64)
    scale = np.max(np.abs(lam), axis=(1, 2))                                        # (B,)
    Lam = np.max(np.abs(lam), axis=1)                                               # (B, n)
    den = np.abs(d["lu"]) + np.einsum("btia,bi->bta", np.abs(d["B"]), Lam)          # (B, N, m)
    out = dict(grad_u=float(np.max(np.abs(np.asarray(got["grad_u"], dtype=np.float64) - ref["grad_u"]) / den)))
    if got.get("costate") is not None:
        out["costate"] = float(np.max(np.max(np.abs(np.asarray(got["costate"], dtype=np.float64) - lam), axis=(1, 2)) / scale))
    if got.get("grad_x0") is not None:
        out["grad_x0"] = float(np.max(np.max(np.abs(np.asarray(got["grad_x0"], dtype=np.float64) - lam[:, 0]), axis=1) / scale))
    return out


def worst(errs):
    return max(errs.values())


# ---------------------------------------------------------------------------------------------------------------- built-in models
SETS = {"quadrotor": ("skew", "skew_nobarrier"), "cartpole": ("skew", "skew_barrier")}
INTEGRATORS = ("euler", "rk4")


def nominal(model, set_name, integ, N, B=None):
    """x (B, N+1, n), u (B, N, m) of param_cases.inputs: the fp64 rollout rounded to fp32 (what the device is given), as fp64."""
    x0, u = pc.inputs(model, set_name, N, B)
    xs, _ = o_lin.rollout_batched(pc.spec(model, set_name, integ), x0, u)
    return f32(xs), u


def blocks(spec, x, u, win=None):
    """The fp64 blocks about (x, u); win (B, N+1, n): the cost of step t against win[:, t] (reference rows through ref_cases.window)."""
    return o_lin.linearize_analytic(spec, x, u) if win is None else rc.composed_blocks(spec, win, x, u)


def blocks_per_trajectory(specs, x, u, win=None):
    """One spec per trajectory (heterogeneous weights or phys): the blocks of trajectory b under specs[b], stacked."""
    parts = [blocks(sp, x[b:b + 1], u[b:b + 1], None if win is None else win[b:b + 1]) for b, sp in enumerate(specs)]
    return {key: np.concatenate([p[key] for p in parts], axis=0) for key in parts[0]}


def phys_rows(model, B):
    """(B, len(phys)) float32: the skew set's physical parameters scaled per trajectory and entry by 0.8 .. 1.25 (seeded)."""
    base = np.array([pc.SETS[model]["skew"]["phys"][k] for k in pc.PHYS_NAMES[model]], dtype=np.float64)
    f = np.exp(np.random.default_rng(23).uniform(np.log(0.8), np.log(1.25), (B, base.size)))
    return (base[None, :] * f).astype(np.float32)


def params_with(model, weights_row=None, phys_row=None):
    """The skew set's parameter dict with one row of weights [q | qf | r] and / or of physical parameters (the fp32 values)."""
    import weight_cases as wc
    p = pc.params(model, "skew") if weights_row is None else wc.row_params(model, weights_row)
    if phys_row is not None:
        p["phys"] = {k: float(v) for k, v in zip(pc.PHYS_NAMES[model], phys_row)}
    return p


# ---------------------------------------------------------------------------------------------------------------- finite differences
FD_H = 1e-5
FD_DIRECTIONS = 3


def fd_errors(spec, x0, u, seed=5):
    """Central differences of oracle.linearize.rollout_batched's cost along random directions (dx0, du) against the fp64 adjoint
    about the fp64 rollout: the largest relative difference over trajectories and directions."""
    xs, _ = o_lin.rollout_batched(spec, x0, u)
    g = adjoint(o_lin.linearize_analytic(spec, xs, u))
    rng = np.random.default_rng(seed)
    out = 0.0
    for _ in range(FD_DIRECTIONS):
        dx0, du = rng.standard_normal(x0.shape), rng.standard_normal(u.shape)
        Jp = o_lin.rollout_batched(spec, x0 + FD_H * dx0, u + FD_H * du)[1]
        Jm = o_lin.rollout_batched(spec, x0 - FD_H * dx0, u - FD_H * du)[1]
        fd = (Jp - Jm) / (2.0 * FD_H)
        an = np.sum(g["grad_x0"] * dx0, axis=1) + np.sum(g["grad_u"] * du, axis=(1, 2))
        out = max(out, float(np.max(np.abs(fd - an) / np.abs(an))))
    return out


# Measured (param_cases sets, N = 7 and 26, B = B_FULL, both models and integrators): the worst relative difference between the fp64
# adjoint and central differences (h = 1e-5) of the oracle's rollout cost is FD_WORST; asserted: 10 x that.
FD_WORST = 1.8e-8
FD_BOUND = 10.0 * FD_WORST

# ---------------------------------------------------------------------------------------------------------------- bounds
# E: the distance of the fp32 restatement (blocks rounded to fp32, recursion in fp32) from fp64 under the measures above, the worst
# over the sets, N = 7 and 26, both integrators, B = B_FULL, measured on the CPU (tests/test_cost_gradient_cpu.py holds the
# restatement to these figures).  The GPU tests assert the larger of 4 x E and the fp32 floor of the project's rollout comparisons
# (param_cases.BOUNDS["sim_x"] = 2e-6): the device forms its own fp32 tangents, which the restatement does not model.
E = {"quadrotor": 4.5e-7, "cartpole": 4.4e-7}
FLOOR = pc.BOUNDS["sim_x"]


def gpu_bound(model):
    return max(4.0 * E[model], FLOOR)


# Every mutant stands >= 10 x above gpu_bound in the case named here (model -> mutant -> (set, integrator, N)); measured values in
# tests/test_cost_gradient_cpu.py's docstring.
TEETH = {
    "quadrotor": {"A not transposed": ("skew", "rk4", 26), "lambda_t in g_t": ("skew", "euler", 7), "l_x dropped": ("skew", "rk4", 26),
                  "l_u dropped": ("skew", "euler", 7), "A of step t + 1": ("skew", "rk4", 7), "B of step t + 1": ("skew", "rk4", 7)},
    "cartpole": {"A not transposed": ("skew_barrier", "euler", 26), "lambda_t in g_t": ("skew", "euler", 7),
                 "l_x dropped": ("skew", "rk4", 26), "l_u dropped": ("skew_barrier", "euler", 7),
                 "A of step t + 1": ("skew", "euler", 26), "B of step t + 1": ("skew", "euler", 26)},
}

# ---------------------------------------------------------------------------------------------------------------- user models
USER_POINTS = ((1, 1), (4, 4), (12, 4), (13, 4), (16, 8))      # every lanes-per-item (8, 8, 16, 32, 32) and the maximum
USER_E = 2.3e-7                                                 # the restatement's distance on the grid (same measure)


def user_reference(n, m, integ, N, B):
    """-> x (B, N+1, n) fp32-rounded rollout, u, the fp64 records about it, the fp64 adjoint."""
    import user_grid_cases as g
    ev = g.evaluate(n, m, "convex", integ, N, B)
    x = f32(ev["sim_x"])
    about = g.evaluate(n, m, "convex", integ, N, B, about=dict(nom=x, K=ev["K"], k=ev["k"]))
    d = {key: about[key] for key in ("A", "B", "lx", "lu", "VxN")}
    _, u = g.inputs(n, m, "convex", N, B)
    return x, u, d, adjoint(d)
