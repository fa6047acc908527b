"""Output feedback inside a tracked run (quattro_track_estimate_f32, ops.track_estimate, QuattroILQR.fly): the cases, the fp64 reference,
the error measures, the fp32 restatement, the mutants and the bounds.  A plain helper module (like tests/cov_cases.py, on which it
builds), used by tests/test_track_estimate_cpu.py and tests/test_track_estimate_gpu.py.

Case: policy_cases.case (B = 5, the skew set, the nominal and the fp64 oracle's gains about it rounded to fp32, the start moved off the
nominal, the plant's spec per trajectory) plus, all seeded and rounded to fp32:
    observed    OBSERVED[model][name]: "pose" (the quadrotor's six pose states, the cart-pole's two positions), "all", "single"
    meas_var    R_i = (0.02 x spread[obs_i])^2, shape (p_y,); hetero "meas_var": scaled per trajectory and entry by 0.5 .. 2, (B, p_y)
    cov0, noise cov_cases.cov_inputs (dense positive definite; diag((0.01 x spread)^2))
    xhat0       x0 + L z, L L^T = cov0, z ~ N(0, 1): off x0 by the cov0 spread; plain=True: None
    meas_noise  sqrt(R) N(0, 1) (S, B, p_y);  disturbance  0.01 x spread x N(0, 1) (S, B, n);  plain=True: both None
    hetero      "plant_phys": grad_cases.phys_rows as the plant's rows; "model_phys": rows of the same kind from another seed as the
                estimator's; "meas_var": above
(spread: param_cases' spread of the starts).  case() asserts, on the fp64 reference alone: every innovation variance s >= R_i, the
posterior variance of every observed state is below its prior at every step, and xhat != x at step 0 (unless plain, the None forms:
the estimator then starts informed and only the plant's mismatch drives the innovations).

Reference (fp64): the definition of include/quattro_hip.h, with f the oracle's step under the right spec (the plant's for x, the
estimator's for xhat) and A from oracle.linearize.step_jac's analytic blocks at (xhat, u_t).  P[j][:] stands for g^T in the rank-1
update as on the device (P is read as symmetric); in fp64 the two forms agree to 1e-16.

Error measures (the largest over the batch, the steps and the entries):
    x, xhat : |d| / spread[i]          u : |d| / U_SPREAD[model]      (the spreads param_cases draws its inputs with)
    cov, var, asym : cov_cases.errors' correlation measure (the reference's P)
    nis     : |d| / the reference value
An entry whose denominator is exactly zero must be exactly zero (policy_cases._ratio).
"""
import numpy as np

import cov_cases as cc
import grad_cases as gc
import param_cases as pc
import policy_cases as pol
from oracle import linearize as o_lin

f32 = gc.f32
KEYS = ("x", "u", "xhat", "var", "cov", "nis")
SEED = 83
OBSERVED = {"quadrotor": dict(pose=(0, 1, 2, 6, 7, 8), all=tuple(range(12)), single=(2,)),
            "cartpole": dict(pose=(0, 2), all=(0, 1, 2, 3), single=(0,))}
U_SPREAD = {"quadrotor": 0.4, "cartpole": pc.CART_U["skew"][1]}     # the sigma param_cases.inputs draws the controls with
MUTANTS = ("control from the true state", "control from the estimate before the update", "R left out of s",
           "P not reduced after an update", "innovation sign", "A at the true state", "A from the plant", "A^T P A", "W dropped",
           "W added before the product", "meas_noise dropped", "nis with s without R")
OTHER = {"euler": "rk4", "rk4": "euler"}


# ---------------------------------------------------------------------------------------------------------------- reference
def run(c, dtype=np.float64, mutant=None):
    """The definition on case c -> dict of KEYS (x (B, S+1, n), u (B, S, m), xhat, var (B, S+1, n), cov (B, S+1, n, n), nis (B, S))
    and "aux" (the smallest s / R, whether every observed posterior variance fell).  dtype float32: the restatement -- the step's
    value and A come from the fp64 oracle at the restatement's own (xhat, u) and are rounded; every estimator and gain-law operation
    is a float32 operation, the update in the device's order (1 / s once; xh += g (e / s); P -= g (g^T / s)).  mutant: one of
    MUTANTS, the definition with that mistake."""
    f = dtype
    B, S, obs = c["x0"].shape[0], c["S"], c["observed"]
    n, m = c["x0"].shape[1], c["u_nom"].shape[2]
    R = np.broadcast_to(np.asarray(c["meas_var"]), (B, len(obs))).astype(f)
    out = dict(x=np.zeros((B, S + 1, n), f), u=np.zeros((B, S, m), f), xhat=np.zeros((B, S + 1, n), f), var=np.zeros((B, S + 1, n), f),
               cov=np.zeros((B, S + 1, n, n), f), nis=np.zeros((B, S), f))
    s_over_r, fell = np.inf, True
    one = f(1.0)
    for b in range(B):
        plant, model = c["specs"][b], c["mspecs"][b]
        xt = c["x0"][b].astype(f)
        xh = (c["x0"][b] if c["xhat0"] is None else c["xhat0"][b]).astype(f)
        P = np.zeros((n, n), f) if c["cov0"] is None else c["cov0"][b].astype(f)
        W = np.zeros((n, n), f) if c["noise"] is None or mutant == "W dropped" else c["noise"][b].astype(f)
        out["x"][b, 0] = xt
        for t in range(S):
            before, prior, nis = xh.copy(), np.diag(P).copy(), f(0.0)
            for i, j in enumerate(obs):
                v = f(0.0) if c["meas_noise"] is None or mutant == "meas_noise dropped" else f(c["meas_noise"][t, b, i])
                y = f(xt[j] + v)
                g, grow = P[:, j].copy(), P[j, :].copy()
                s = f(P[j, j] + (f(0.0) if mutant == "R left out of s" else R[b, i]))
                s_over_r = min(s_over_r, float(s) / float(R[b, i]))
                e = f(xh[j] - y) if mutant == "innovation sign" else f(y - xh[j])
                inv = f(one / s)
                w = f(e * inv)
                nis = f(nis + (f(e * f(e / P[j, j])) if mutant == "nis with s without R" else f(e * w)))
                xh = (xh + grow * w).astype(f)
                if mutant != "P not reduced after an update":
                    P = (P - np.outer(g, (grow * inv).astype(f)).astype(f)).astype(f)
            fell = fell and bool(np.all(np.diag(P)[list(obs)] < prior[list(obs)]))
            out["xhat"][b, t], out["cov"][b, t], out["nis"][b, t] = xh, P, nis
            src = xt if mutant == "control from the true state" else (before if mutant == "control from the estimate before the update" else xh)
            u = (c["u_nom"][b, t].astype(f) + (c["K"][b, t].astype(f) @ (src - c["x_nom"][b, t].astype(f)).astype(f)).astype(f)).astype(f)
            out["u"][b, t] = u
            u64, xt64, xh64 = u.astype(np.float64)[None], xt.astype(np.float64)[None], xh.astype(np.float64)[None]
            xn = o_lin.step(plant, xt64, u64)[0].astype(f)
            if c["disturbance"] is not None:
                xn = (xn + c["disturbance"][t, b].astype(f)).astype(f)
            xhn, A, _ = o_lin.step_jac(model, xh64, u64)
            if mutant == "A at the true state":
                A = o_lin.step_jac(model, xt64, u64)[1]
            if mutant == "A from the plant":
                A = o_lin.step_jac(plant, xh64, u64)[1]
            A = A[0].astype(f)
            if mutant == "A^T P A":
                P = (A.T @ (P @ A).astype(f) + W).astype(f)
            elif mutant == "W added before the product":
                P = (A @ ((P + W).astype(f) @ A.T).astype(f)).astype(f)
            else:
                P = (A @ (P @ A.T).astype(f) + W).astype(f)
            xt, xh = xn, xhn[0].astype(f)
            out["x"][b, t + 1] = xt
        out["xhat"][b, S], out["cov"][b, S] = xh, P
    out["var"] = np.einsum("btii->bti", out["cov"]).copy()
    out["aux"] = dict(s_over_r=s_over_r, fell=fell)
    return out


def errors(c, got):
    """got: dict with any of KEYS; c["ref"]: run() in fp64.  -> dict of the measures of the module docstring (and "asym" with cov)."""
    ref, model = c["ref"], c["model"]
    out = {}
    for key, scale in (("x", pol.SPREAD[model]), ("xhat", pol.SPREAD[model]), ("u", np.full(c["u_nom"].shape[2], U_SPREAD[model]))):
        if got.get(key) is not None:
            g = np.asarray(got[key], dtype=np.float64)
            assert g.shape == ref[key].shape, (key, g.shape, ref[key].shape)
            out[key] = float(np.max(np.abs(g - ref[key]) / scale))
    sub = {k: got[k] for k in ("cov", "var") if got.get(k) is not None}
    out.update(cc.errors(sub, ref, c["S"]))
    if got.get("nis") is not None:
        g = np.asarray(got["nis"], dtype=np.float64)
        assert g.shape == ref["nis"].shape
        out["nis"] = pol._ratio(g - ref["nis"], np.abs(ref["nis"]), g)
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
def model_phys_rows(model, B):
    """(B, len(phys)) float32: the estimator's rows, grad_cases.phys_rows' kind from another seed (0.9 .. 1.1 of the skew set)."""
    base = np.array([pc.SETS[model]["skew"]["phys"][k] for k in pc.PHYS_NAMES[model]], dtype=np.float64)
    f = np.exp(np.random.default_rng(SEED + 1).uniform(np.log(0.9), np.log(1.1), (B, base.size)))
    return (base[None, :] * f).astype(np.float32)


def case(model, integ="rk4", plant_integ=None, N=7, S=None, observed="pose", hetero=(), plain=False, B=pol.B_CASE):
    """-> dict: x0, x_nom, u_nom, K, observed, meas_var, xhat0, cov0, noise, meas_noise, disturbance (fp32-rounded fp64 arrays or None),
    plant_phys, model_phys (float32 rows or None), specs / mspecs (the plant's / the estimator's spec per trajectory), N, S, ref."""
    S = N if S is None else S
    pc_ = pol.case(model, "skew", integ, N, S, B=B, plant_integ=plant_integ, hetero=("phys",) if "plant_phys" in hetero else ())
    n = pc.DIMS[model][0]
    spread = pol.SPREAD[model]
    obs = OBSERVED[model][observed]
    rng = np.random.default_rng(SEED)
    full = pc.B_FULL[model]
    scale = np.exp(rng.uniform(np.log(0.5), np.log(2.0), (full, n)))[:B][:, list(obs)]
    z = rng.standard_normal((full, n))[:B]
    vn = rng.standard_normal((26, full, n))[:S, :B][:, :, list(obs)]
    dn = rng.standard_normal((26, full, n))[:S, :B]
    R = (0.02 * spread[list(obs)]) ** 2
    meas_var = f32(R[None, :] * scale) if "meas_var" in hetero else f32(R)
    mphys = model_phys_rows(model, B) if "model_phys" in hetero else None
    mspecs = ([pc.spec(model, "skew", integ)] * B if mphys is None
              else [pc.spec_from(model, gc.params_with(model, None, mphys[b]), integ) for b in range(B)])
    c = dict(model=model, integ=integ, plant_integ=plant_integ, N=N, S=S, observed=obs, meas_var=meas_var, x0=pc_["x0"],
             x_nom=pc_["x_nom"], u_nom=pc_["u_nom"], K=pc_["K"], specs=pc_["specs"], mspecs=mspecs, plant_phys=pc_["phys"],
             model_phys=mphys, xhat0=None, meas_noise=None, disturbance=None, plain=plain)
    cov0, noise = cc.cov_inputs(model, B)
    c.update(cov0=cov0, noise=noise)
    if not plain:
        L = np.linalg.cholesky(cov0)
        c.update(xhat0=f32(c["x0"] + np.einsum("bij,bj->bi", L, z)),
                 meas_noise=f32(np.sqrt(np.broadcast_to(meas_var, (B, len(obs))))[None] * vn), disturbance=f32(0.01 * spread * dn))
    c["ref"] = run(c)
    aux = c["ref"]["aux"]
    assert aux["s_over_r"] >= 1.0, aux
    assert aux["fell"], "the posterior variance of an observed state did not fall"
    if not plain:
        assert np.all(np.max(np.abs(c["ref"]["xhat"][:, 0] - c["ref"]["x"][:, 0]), axis=1) > 0.0)
    return c


def restatement(c):
    return run(c, dtype=np.float32)


def mutant_errors(c, name):
    """How far mutant `name` of the reference stands from the reference, in case c."""
    return errors(c, run(c, mutant=name))


def case_id(kw):
    return "-".join(str(v) if not isinstance(v, tuple) else "+".join(v) for v in kw.values()) or "default"


# The cases the restatement is measured on and the GPU parity test runs: policy_cases.STEPS, every integrator pair, rows per
# trajectory of all three kinds, every choice of `observed`, and the None forms.
def parity_cases(model):
    out = []
    for integ in gc.INTEGRATORS:
        for N, S in pol.STEPS:
            out.append(dict(integ=integ, N=N, S=S))
        out.append(dict(integ=integ, plant_integ=OTHER[integ], N=7, S=7, hetero=("plant_phys", "model_phys", "meas_var")))
        out.append(dict(integ=integ, N=7, S=5, hetero=("plant_phys", "model_phys", "meas_var"), observed="all"))
        out.append(dict(integ=integ, N=7, S=7, observed="single"))
        out.append(dict(integ=integ, plant_integ=OTHER[integ], N=7, S=5, hetero=("plant_phys",), plain=True))
    return out


# ---------------------------------------------------------------------------------------------------------------- bounds
# E: the distance of the fp32 restatement from fp64 per measure, the worst over parity_cases, measured on the CPU
# (tests/test_track_estimate_cpu.py holds the restatement to these figures).  The GPU tests assert, per measure, the larger of 4 x E
# and a floor: for x, xhat and u the bound tests/test_plant_loop_gpu.py asserts for ops.track's x and u (1e-5 = param_cases.BOUNDS["cl_x"]:
# the plant steps are that arithmetic); for cov, var, asym and nis cov_cases.gpu_bound's floor (param_cases.BOUNDS["sim_x"] = 2e-6).
# nis is a sum of e^2 / s with e = y - xh[j] a difference of two nearly equal numbers (sqrt(R) is 2 % of the spread, and smaller still
# where only the model mismatch drives it): its fp32 error relative to ITSELF is that cancellation, which is why its E stands above the
# others' and is kept per measure instead of widening every bound to the worst.
# The worst nis figure of either model comes from the "single" cases: with one observed state a step's nis is ONE e^2 / s, and where a
# trajectory's e happens to pass near zero the relative measure divides by it.
E = {"quadrotor": dict(x=2.2e-6, u=5.4e-5, xhat=1.7e-6, var=3.2e-6, cov=3.2e-6, asym=3.4e-7, nis=2.2e-2),
     "cartpole": dict(x=7.5e-7, u=1.7e-6, xhat=6.7e-7, var=1.2e-6, cov=1.2e-6, asym=1.8e-7, nis=9.9e-4)}
FLOOR = dict(x=pc.BOUNDS["cl_x"], u=pc.BOUNDS["cl_u"], xhat=pc.BOUNDS["cl_x"], var=cc.FLOOR, cov=cc.FLOOR, asym=cc.FLOOR, nis=cc.FLOOR)


def gpu_bound(model, key):
    return max(4.0 * E[model][key], FLOOR[key])


def over_bound(model, errs):
    """The largest ratio of a measure to its GPU bound."""
    return max(e / gpu_bound(model, k) for k, e in errs.items())


# Every mutant stands >= 10 x above the GPU bound of some measure in the case named here (model -> mutant -> keywords of case());
# measured values in tests/test_track_estimate_cpu.py's docstring.
_MIX = dict(integ="rk4", plant_integ="euler", N=7, S=7, hetero=("plant_phys", "model_phys", "meas_var"))
TEETH = {model: {name: (dict(_MIX) if name == "A from the plant" else dict(integ="rk4", N=7, S=7)) for name in MUTANTS}
         for model in pc.MODELS}
