"""The cost gradient with respect to a trajectory's rows (quattro_cost_param_gradient_f32, ops.cost_param_gradient, the row
gradients of autograd.trajectory_cost): the fp64 reference, the error measures, the fp32 restatement, the mutants and the bounds.  A
plain helper module (like tests/grad_cases.py, on which it builds), used by tests/test_cost_param_gradient_cpu.py and
tests/test_cost_param_gradient_gpu.py.

Reference (fp64, about the fp32-rounded (x, u) the device is given):
    grad_phys[k]    = sum_{t<N} lambda_{t+1}^T df/dtheta_k(x_t, u_t)     lambda: grad_cases.adjoint over the oracle's blocks;
                      df/dtheta_k: central differences of oracle.models.discrete_step in theta_k about the fp32 phys row (two of
                      them, at h and h / 2, combined so that the h^2 error term cancels: step_dtheta says why), relative
                      step REL_STEP (halving it moves no grad_phys entry by more than 1e-9 of its scale: the CPU test measures it)
    grad_weights    = [sum_{t<N} (x_t - ref_t)^2 | (x_N - ref_N)^2 | sum_{t<N} u_t^2]
    grad_targets    : row rho collects -2 q (x_t - ref_rho) over t < N with min(t, R - 1) = rho, and -2 qf (x_N - ref_rho) where
                      min(N, R - 1) = rho; rows past the horizon are zero
Error measures (the largest over the batch and the entries):
    grad_phys       : |d_k| / sum_t sum_i Lambda_i |df_i/dtheta_k(t)|, Lambda_i = max_t |lambda_{t,i}| -- the scale of the terms that
                      are added, as in grad_cases' measure of grad_u
    grad_weights, grad_targets : |d| / sum |terms added| per entry
An entry whose denominator is zero must be exactly +0.0 (its error is then 0, otherwise inf).  Every phys denominator of the inputs
used here is non-zero (the CPU test checks it): k_yaw needs u0 - u1 + u2 - u3 != 0 at some step, which param_cases' random controls
give; the quadrotor's gravity enters v_z at every step.
"""
import dataclasses

import numpy as np

import grad_cases as gc
import param_cases as pc
import ref_cases as rc
import weight_cases as wc
from oracle import linearize as o_lin
from oracle import models as o_models

REL_STEP = 4e-3          # relative step h of the differences in theta_k (recorded: halving it moves no entry by more than 2.5e-10)
MUTANTS = ("lambda_t for lambda_t+1", "df/dtheta of step t + 1", "rate derivative for the step's", "rk4 differentiated at stage 1 only",
           "terminal term left out of targets", "row rule off by one", "q for qf in the terminal partial", "the neighbour's phys row")

f32 = gc.f32


def phys_base(model, set_name="skew"):
    return np.array([pc.SETS[model][set_name]["phys"][k] for k in pc.PHYS_NAMES[model]], dtype=np.float64)


def _spec_with_phys(spec, names, phys):
    """spec with phys (B, NP) as arrays (B, 1): oracle.models broadcasts them over a (n, B, N) state."""
    return dataclasses.replace(spec, phys={k: phys[:, j:j + 1] for j, k in enumerate(names)})


def _step(spec, x, u):
    """oracle.models.discrete_step over a batch: x (B, N, n), u (B, N, m) -> (B, N, n)."""
    return np.moveaxis(o_models.discrete_step(spec, np.moveaxis(x, 2, 0), np.moveaxis(u, 2, 0)), 0, 2)


def _rate(spec, x, u):
    return np.moveaxis(o_models.continuous_rate(spec, np.moveaxis(x, 2, 0), np.moveaxis(u, 2, 0)), 0, 2)


def _central(model, spec, phys, x, u, rel, fn):
    names = pc.PHYS_NAMES[model]
    out = np.zeros(x.shape + (len(names),))
    for k in range(len(names)):
        h = rel * np.abs(phys[:, k])
        hi, lo = phys.copy(), phys.copy()
        hi[:, k] += h
        lo[:, k] -= h
        out[..., k] = (fn(_spec_with_phys(spec, names, hi), x, u) - fn(_spec_with_phys(spec, names, lo), x, u)) / (2.0 * h)[:, None, None]
    return out


def step_dtheta(model, spec, phys, x, u, rel=REL_STEP, fn=_step):
    """Central differences of the step (fn=_rate: of the rate) in every theta_k, at the relative steps rel and rel / 2 with the h^2
    term of their error eliminated ((4 D(h/2) - D(h)) / 3): phys (B, NP), x (B, N, n), u (B, N, m) -> (B, N, n, NP).  (One central
    difference cannot meet 1e-9 here: the step is x + dt rate with dt down to 0.004, so round-off in the difference is relative to x,
    not to the derivative, and grows as the truncation error falls.)"""
    return (4.0 * _central(model, spec, phys, x, u, 0.5 * rel, fn) - _central(model, spec, phys, x, u, rel, fn)) / 3.0


def reference(model, spec, x, u, lam, phys=None, weights=None, rows=None, mutant=None, rel=REL_STEP, terms=None):
    """x (B, N+1, n), u (B, N, m), lam (B, N+1, n) the costate; phys (B, NP), weights (B, 2n+m), rows (B, R, n) per trajectory or None
    (the spec's own).  -> dict(grad_phys (B, NP), grad_weights (B, 2n+m), grad_targets (B, R, n), den_* the measures' denominators).
    mutant: one of MUTANTS.  terms: a function applied to every per-step term before it is added (the fp32 restatement rounds)."""
    B, N, m = u.shape
    n = x.shape[2]
    rnd = (lambda a: a) if terms is None else terms
    # (the fp32 phys row: without rows that is the model's own parameters as the device holds them)
    phys = np.tile(f32([spec.phys[k] for k in pc.PHYS_NAMES[model]]), (B, 1)) if phys is None else np.asarray(phys, dtype=np.float64)
    if weights is None:
        weights = np.tile(f32(np.concatenate([np.diag(spec.Q), np.diag(spec.Qf), np.diag(spec.R)])), (B, 1))
    weights = np.asarray(weights, dtype=np.float64)
    q, qf = weights[:, :n], weights[:, n:2 * n]
    # (without rows the device differences x against the model's x_ref as it holds it, rounded to fp32; x sits within a few tenths
    #  of it, so the 3e-8 relative rounding of x_ref is up to 1e-4 of a difference: the reference starts from the device's number,
    #  as it does for x, u and the rows)
    rows = np.tile(f32(spec.x_ref)[None, None, :], (B, 1, 1)) if rows is None else np.asarray(rows, dtype=np.float64)
    R = rows.shape[1]
    # --- phys
    ph = np.roll(phys, -1, axis=0) if mutant == "the neighbour's phys row" else phys
    if mutant == "rate derivative for the step's":
        df = step_dtheta(model, spec, ph, x[:, :N], u, rel, fn=_rate)
    elif mutant == "rk4 differentiated at stage 1 only":
        df = spec.dt * step_dtheta(model, spec, ph, x[:, :N], u, rel, fn=_rate)
    else:
        df = step_dtheta(model, spec, ph, x[:, :N], u, rel)
    if mutant == "df/dtheta of step t + 1":
        df = df[:, [min(t + 1, N - 1) for t in range(N)]]
    lam_next = lam[:, :N] if mutant == "lambda_t for lambda_t+1" else lam[:, 1:]
    t_phys = rnd(np.einsum("bti,btik->btk", lam_next, df))
    Lam = np.max(np.abs(lam), axis=1)
    out = dict(grad_phys=np.sum(t_phys, axis=1), den_phys=np.einsum("bi,btik->bk", Lam, np.abs(df)))
    # --- weights
    rule = (lambda t: min(t + 1, R - 1)) if mutant == "row rule off by one" else (lambda t: min(t, R - 1))
    idx = [rule(t) for t in range(N + 1)]
    d = rnd(x - rows[:, [min(t, R - 1) for t in range(N + 1)]])
    sq = rnd(d * d)
    gw = np.concatenate([np.sum(sq[:, :N], axis=1), sq[:, N], np.sum(rnd(u * u), axis=1)], axis=1)
    out.update(grad_weights=gw, den_weights=gw.copy())
    # --- targets
    d = rnd(x - rows[:, idx])
    tt = rnd(rnd(-2.0 * q[:, None, :]) * d[:, :N])
    tN = rnd(rnd(-2.0 * (q if mutant == "q for qf in the terminal partial" else qf)) * d[:, N])
    gt, den = np.zeros((B, R, n)), np.zeros((B, R, n))
    for t in range(N):
        gt[:, idx[t]] += tt[:, t]
        den[:, idx[t]] += np.abs(tt[:, t])
    if mutant != "terminal term left out of targets":
        gt[:, idx[N]] += tN
    den[:, min(N, R - 1)] += np.abs(tN)
    out.update(grad_targets=gt, den_targets=den)
    return out


def restatement(model, spec, x, u, lam, **kw):
    """The fp32 restatement: the costate and every per-step term rounded to fp32, the sums in fp64."""
    return reference(model, spec, x, u, f32(lam), terms=f32, **kw)


def errors(got, ref):
    """got: dict with any of grad_phys / grad_weights / grad_targets; ref: reference()'s dict -> the measures above."""
    out = {}
    for key in ("phys", "weights", "targets"):
        if got.get("grad_" + key) is None:
            continue
        g, r, den = np.asarray(got["grad_" + key], dtype=np.float64), ref["grad_" + key], ref["den_" + key]
        assert g.shape == r.shape, (key, g.shape, r.shape)
        zero = den == 0.0
        e = np.abs(g - r) / np.where(zero, 1.0, den)
        e = np.where(zero, np.where((g == 0.0) & ~np.signbit(g), 0.0, np.inf), e)
        out["grad_" + key] = float(np.max(e))
    return out


def worst(errs):
    return max(errs.values())


# ---------------------------------------------------------------------------------------------------------------- cases
SETS, INTEGRATORS = gc.SETS, gc.INTEGRATORS


N_ROLLED = 26            # param_cases.inputs keeps the quadrotor's pitch clear of the singularity up to this horizon


def case(model, set_name, integ, N, R=None, B=None, hetero=()):
    """-> dict(spec(s), x, u, lam, d, kw of reference()) about param_cases' inputs (N > N_ROLLED: their N_ROLLED-step rollout repeated;
    the outputs are defined about any sequences).  R: rows of ref_cases.skew_rows (None: no rows);
    hetero: any of "weights", "targets", "phys" -- rows of weight_cases / ref_cases / grad_cases.phys_rows per trajectory, the rollout
    under each trajectory's own parameters (the skew set only)."""
    B = pc.B_FULL[model] if B is None else B
    x0, u = pc.inputs(model, set_name, min(N, N_ROLLED), B)
    w = wc.weight_rows(model, B) if "weights" in hetero else None
    phys = gc.phys_rows(model, B) if "phys" in hetero else None
    if "targets" in hetero and R is None:
        R = 3
    rows = rc.ref_rows(model, pc.SETS[model][set_name]["x_ref"], B, R) if R is not None else None
    if w is not None or phys is not None:
        assert set_name == "skew"
        specs = [pc.spec_from(model, gc.params_with(model, None if w is None else w[b], None if phys is None else phys[b]), integ)
                 for b in range(B)]
    else:
        specs = [pc.spec(model, set_name, integ)] * B
    x = f32(np.concatenate([o_lin.rollout_batched(sp, x0[b:b + 1], u[b:b + 1])[0] for b, sp in enumerate(specs)]))
    if N > N_ROLLED:           # the rollout of N_ROLLED steps over and over: any sequences serve, and these stay where the inputs keep them
        x, u = x[:, [t % (N_ROLLED + 1) for t in range(N + 1)]], u[:, [t % N_ROLLED for t in range(N)]]
    win = None if rows is None else rc.window(rows.astype(np.float64), N)
    d = gc.blocks_per_trajectory(specs, x, u, win)
    lam = gc.adjoint(d)["costate"]
    kw = dict(phys=None if phys is None else phys.astype(np.float64), weights=None if w is None else w.astype(np.float64),
              rows=None if rows is None else rows.astype(np.float64))
    return dict(spec=specs[0], specs=specs, x=x, u=u, x0=x0, lam=lam, d=d, kw=kw, w=w, phys=phys, rows=rows)


# ---------------------------------------------------------------------------------------------------------------- bounds
# E: the distance of the fp32 restatement from fp64 under the measures above, the worst over grad_cases.SETS, both integrators,
# N = 7 and 26, B = B_FULL, with R = 3 rows, measured on the CPU (tests/test_cost_param_gradient_cpu.py holds the restatement to
# these figures).  The GPU tests assert the larger of 4 x E and the fp32 floor of the project's rollout comparisons: the device forms
# df/dtheta in fp32 itself, which the restatement (fp64 derivative, fp32 terms) does not model.
E = {"quadrotor": 1.8e-7, "cartpole": 1.8e-7}
FLOOR = pc.BOUNDS["sim_x"]


def gpu_bound(model):
    return max(4.0 * E[model], FLOOR)


# Total derivative: the reference against central differences of the oracle's rollout cost (re-rolled from x0, u under the
# perturbed parameter, target entry or weight), relative to the measure's denominator.  FD_WORST: measured over the cases of the CPU
# test; asserted: 10 x that.
FD_H = 1e-5              # relative, in a parameter
FD_H_EXPLICIT = 0.1      # relative, in a weight or a target entry: J is linear in the one and quadratic in the other, so a central
                         # difference is exact at any step and a large one keeps round-off out (J is 1e3 .. 1e4, a term 1e-2)
FD_WORST = 2.5e-9
FD_BOUND = 10.0 * FD_WORST

# Every mutant stands >= 10 x above gpu_bound in the case named here: model -> mutant -> (set, integrator, N, R, hetero).
TEETH = {
    "quadrotor": {
        "lambda_t for lambda_t+1": ("skew", "euler", 7, 3, ()),
        "df/dtheta of step t + 1": ("skew", "euler", 7, 3, ()),
        "rate derivative for the step's": ("skew", "euler", 7, 3, ()),
        "rk4 differentiated at stage 1 only": ("skew", "rk4", 26, 3, ()),
        "terminal term left out of targets": ("skew", "euler", 7, 3, ()),
        "row rule off by one": ("skew", "euler", 7, 3, ()),
        "q for qf in the terminal partial": ("skew", "euler", 7, 3, ()),
        "the neighbour's phys row": ("skew", "euler", 7, 3, ("phys",)),
    },
    "cartpole": {
        "lambda_t for lambda_t+1": ("skew", "euler", 7, 3, ()),
        "df/dtheta of step t + 1": ("skew", "euler", 7, 3, ()),
        "rate derivative for the step's": ("skew", "euler", 7, 3, ()),
        "rk4 differentiated at stage 1 only": ("skew", "rk4", 26, 3, ()),
        "terminal term left out of targets": ("skew", "euler", 7, 3, ()),
        "row rule off by one": ("skew", "euler", 7, 3, ()),
        "q for qf in the terminal partial": ("skew", "euler", 7, 3, ()),
        "the neighbour's phys row": ("skew", "euler", 7, 3, ("phys",)),
    },
}


def rollout_cost(model, integ, x0, u, phys=None, weights=None, rows=None, set_name="skew"):
    """fp64 cost of the oracle's rollout of u from x0 per trajectory, each under its own phys (B, NP) / weights (B, 2n+m) / rows."""
    B, N = u.shape[:2]
    out = np.zeros(B)
    for b in range(B):
        p = pc.params(model, set_name)
        if weights is not None:
            qv, qfv, rv = wc.split(model, weights[b])
            p["q"], p["qf"], p["r"] = tuple(qv), tuple(qfv), tuple(rv)
        if phys is not None:
            p["phys"] = {k: float(v) for k, v in zip(pc.PHYS_NAMES[model], phys[b])}
        sp = pc.spec_from(model, p, integ)
        xs, J = o_lin.rollout_batched(sp, x0[b:b + 1], u[b:b + 1])
        out[b] = J[0] if rows is None else rc.composed_cost(sp, rc.window(rows[b:b + 1], N), xs, u[b:b + 1])[0]
    return out


# ---------------------------------------------------------------------------------------------------------------- system identification
# The use case: the log is the oracle's rollout under the "true" parameters (the skew set's), the loss of trajectory b is its
# trajectory cost against that log (targets = the log, R = N + 1) under q alone (qf = r = 0), as a function of its model_phys row,
# which starts at grad_cases.phys_rows (every entry off by a factor in 0.8 .. 1.25).
# Step rule: theta' = theta - s g with s = SYSID_RHO min_k |theta_k / g_k| (no parameter moves by more than the fraction SYSID_RHO
# of itself), halved until the fp64 cost of the oracle's rollout under theta' is below that under theta, at most SYSID_HALVINGS times.
SYSID_N, SYSID_RHO, SYSID_HALVINGS = 26, 0.25, 30


def sysid_case(model, integ):
    """-> dict(x0, u, log (B, N+1, n) float32, w (B, 2n+m) float32, theta (B, NP) float32)."""
    B, N = pc.B_FULL[model], SYSID_N
    n, m = pc.DIMS[model]
    x0, u = pc.inputs(model, "skew", N, B)
    log = o_lin.rollout_batched(pc.spec(model, "skew", integ), x0, u)[0].astype(np.float32)
    w = np.tile(np.concatenate([pc.SETS[model]["skew"]["q"], np.zeros(n + m)]).astype(np.float32), (B, 1))
    return dict(x0=x0, u=u, log=log, w=w, theta=gc.phys_rows(model, B))


def sysid_cost(model, integ, c, theta):
    return rollout_cost(model, integ, c["x0"], c["u"], phys=np.asarray(theta, dtype=np.float64), weights=c["w"].astype(np.float64),
                        rows=c["log"].astype(np.float64))


def sysid_reference_gradient(model, integ, c):
    """fp64 dJ/dtheta (B, NP) about the fp64 rollouts under theta."""
    B, N = c["u"].shape[:2]
    specs = [pc.spec_from(model, gc.params_with(model, c["w"][b], c["theta"][b]), integ) for b in range(B)]
    x = np.concatenate([o_lin.rollout_batched(sp, c["x0"][b:b + 1], c["u"][b:b + 1])[0] for b, sp in enumerate(specs)])
    d = gc.blocks_per_trajectory(specs, x, c["u"], rc.window(c["log"].astype(np.float64), N))
    ref = reference(model, specs[0], x, c["u"], gc.adjoint(d)["costate"], phys=c["theta"].astype(np.float64),
                    weights=c["w"].astype(np.float64), rows=c["log"].astype(np.float64))
    return ref["grad_phys"]


def sysid_descends(model, integ, c, g):
    """The step rule with gradient g (B, NP) -> per trajectory the number of halvings after which the cost fell, or -1."""
    theta = c["theta"].astype(np.float64)
    g = np.asarray(g, dtype=np.float64)
    J0 = sysid_cost(model, integ, c, theta)
    s = SYSID_RHO * np.min(np.abs(theta) / np.maximum(np.abs(g), 1e-300), axis=1)
    out = np.full(theta.shape[0], -1)
    for h in range(SYSID_HALVINGS + 1):
        J = sysid_cost(model, integ, c, theta - s[:, None] * g)
        out = np.where((out < 0) & (J < J0), h, out)
        if np.all(out >= 0):
            break
        s = s * 0.5
    return out
