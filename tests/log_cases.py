"""A logged run filtered and smoothed (quattro_estimate_log_f32, ops.estimate_log): the cases, the fp64 reference, the error measures,
the fp32 restatement, the mutants and the bounds.  A plain helper module (like tests/est_cases.py, on which it builds), used by
tests/test_estimate_log_cpu.py and tests/test_estimate_log_gpu.py.

Case: est_cases.case (B = 5, the skew set, the closed loop behind the sensor in fp64) turned into a LOG:
    y_t[i] = x_t[obs_i] + v_t[i] for t < S from that run's x and meas_noise; row S from the run's last state x_S and one more draw of the
    sensor noise (seeded here); u the run's u.  Both rounded to fp32.  shared=True: the log of trajectory 0 for every hypothesis
    pattern     which readings are missing (NaN), per trajectory (PATTERNS): "a" none; "b" the first sensor absent at steps 1 and 2;
                "c" all of step 2 absent; "d" the final row absent; "e" the first sensor at every second step only; "f" everything
                absent.  "mixed": trajectory b takes pattern "abcde"[b % 5], so cart-pole groups of one wave disagree
    xhat0, cov0, noise, meas_var, model_phys : est_cases' (cov0=None with zero_start=True); the filter is the ESTIMATOR of that run
case() asserts, on the fp64 reference alone: every s >= R_i; 0 <= var_s <= var everywhere, 0 < var_s wherever var > 0; var_s < 0.9 var
somewhere on an unobserved state (on any state where all are observed, and in the cart-pole's cases of S <= 7 steps, over which its
velocities gain 13 % at most from later position readings; not asked of a log without a single reading nor of S = 1); the Bryson-Frazier and the Rauch-Tung-Striebel (explicit solve) forms agree to 1e-9 of the correlation measure;
the sequential filter agrees with the batch Kalman update with Joseph covariance on the readings that exist to 1e-12.

Reference (fp64): the definition of include/quattro_hip.h with f the oracle's step and A from oracle.linearize.step_jac.

Error measures (the largest over the batch, the steps and the entries):
    xhat, xs                  : |d| / spread[i]
    cov, var, cov_s, var_s    : cov_cases.errors' correlation measure against the reference's own matrix of that kind
    innov                     : |d| / sqrt(innov_var of the reference)
    innov_var, nis, loglik    : |d| / the reference value; where that is exactly zero, exactly zero is required
A NaN where the reference has a number, or the other way round, is an infinite error.
"""
import math

import numpy as np

import cov_cases as cc
import est_cases as ec
import grad_cases as gc
import param_cases as pc
import policy_cases as pol
from oracle import linearize as o_lin

f32 = gc.f32
FILTER_KEYS = ("xhat", "var", "cov", "innov", "innov_var", "nis", "loglik")
SMOOTH_KEYS = ("xs", "var_s", "cov_s")
KEYS = FILTER_KEYS + SMOOTH_KEYS
SEED = 97
PATTERNS = "abcdef"
MUTANTS = ("u of step t + 1", "a missing reading updates P", "a missing reading is counted", "R left out of s", "loglik without ln s",
           "loglik without 2 pi", "no update at t = S",
           "A r for A^T r", "A_t for A_{t-1}", "updates in forward order", "1 / s dropped from Lambda", "c dropped", "k^T r dropped",
           "sign of e / s", "Lambda not carried through the prediction", "xs from the prior covariance", "cov - cov Lambda")
LN_2PI = math.log(2.0 * math.pi)


def missing_mask(pattern, B, S, p_y):
    """(B, S+1, p_y) bool: True where there is no reading."""
    m = np.zeros((B, S + 1, p_y), dtype=bool)
    for b in range(B):
        k = "abcde"[b % 5] if pattern == "mixed" else pattern
        if k == "b":
            m[b, [min(1, S), min(2, S)], 0] = True
        elif k == "c":
            m[b, min(2, S), :] = True
        elif k == "d":
            m[b, S, :] = True
        elif k == "e":
            m[b, 1::2, 0] = True
        elif k == "f":
            m[b] = True
        else:
            assert k == "a", k
    return m


# ---------------------------------------------------------------------------------------------------------------- reference
def run(c, dtype=np.float64, mutant=None):
    """The definition on case c -> dict of KEYS and "aux".  dtype float32: the restatement -- the step's value and A come from the fp64
    oracle at the restatement's own (xhat, u) and are rounded; every filter and smoother operation is a float32 operation, the update
    in the device's order (1 / s once; xh += g (e / s); P -= g (g^T / s)).  mutant: one of MUTANTS."""
    f = dtype
    y, u, obs = c["y"], c["u"], c["observed"]
    B, S, n, p_y = c["B"], c["S"], c["n"], len(c["observed"])
    R = np.broadcast_to(np.asarray(c["meas_var"]), (B, p_y)).astype(f)
    out = dict(xhat=np.zeros((B, S + 1, n), f), cov=np.zeros((B, S + 1, n, n), f), innov=np.full((B, S + 1, p_y), np.nan, f),
               innov_var=np.full((B, S + 1, p_y), np.nan, f), nis=np.zeros((B, S + 1), f), loglik=np.zeros(B),
               xs=np.zeros((B, S + 1, n), f), cov_s=np.zeros((B, S + 1, n, n), f))
    prior = np.zeros((B, S + 1, n, n), f)
    As = np.zeros((B, S, n, n), f)
    s_over_r = np.inf
    one, zero = f(1.0), f(0.0)
    for b in range(B):
        spec = c["mspecs"][b]
        yb = (y if y.ndim == 2 else y[b]).astype(f)
        ub = (u if u.ndim == 2 else u[b]).astype(f)
        xh = c["xhat0"][b].astype(f)
        P = np.zeros((n, n), f) if c["cov0"] is None else c["cov0"][b].astype(f)
        W = np.zeros((n, n), f) if c["noise"] is None else c["noise"][b].astype(f)
        recs = []
        ll = 0.0
        for t in range(S + 1):
            prior[b, t] = P
            nis, rec = zero, []
            for i, j in enumerate(obs):
                yi = yb[t, i]
                skip = t == S and mutant == "no update at t = S"
                if np.isnan(yi) or skip:
                    if mutant == "a missing reading updates P" and not skip:
                        s = f(P[j, j] + R[b, i])
                        P = (P - np.outer(P[:, j].copy(), (P[j, :] * f(one / s)).astype(f)).astype(f)).astype(f)
                    if mutant == "a missing reading is counted" and not skip:
                        ll += LN_2PI + math.log(float(f(P[j, j] + R[b, i])))
                        nis = f(nis + one)
                    rec.append(None)
                    continue
                g, grow = P[:, j].copy(), P[j, :].copy()
                s = f(P[j, j] + (zero if mutant == "R left out of s" else R[b, i]))
                s_over_r = min(s_over_r, float(s) / float(R[b, i]))
                e = f(yi - xh[j])
                inv = f(one / s)
                w = f(e * inv)
                nis = f(nis + f(e * w))
                xh = (xh + grow * w).astype(f)
                k = (grow * inv).astype(f)
                P = (P - np.outer(g, k).astype(f)).astype(f)
                out["innov"][b, t, i], out["innov_var"][b, t, i] = e, s
                e64, s64 = float(e), float(s)
                if mutant == "loglik without 2 pi":
                    term = math.log(s64)
                elif mutant == "loglik without ln s":
                    term = LN_2PI
                else:
                    term = math.log(2.0 * math.pi * s64)
                ll += term + e64 * e64 / s64
                rec.append((j, k, w, inv))
            recs.append(rec)
            out["xhat"][b, t], out["cov"][b, t], out["nis"][b, t] = xh, P, nis
            if t < S:
                ut = ub[min(t + 1, S - 1)] if mutant == "u of step t + 1" else ub[t]
                xn, A, _ = o_lin.step_jac(spec, xh.astype(np.float64)[None], ut.astype(np.float64)[None])
                A = A[0].astype(f)
                As[b, t] = A
                P = (A @ (P @ A.T).astype(f) + W).astype(f)
                xh = xn[0].astype(f)
        out["loglik"][b] = 0.0 - 0.5 * ll
        # ---- the smoother
        r, Lm = np.zeros(n, f), np.zeros((n, n), f)
        for t in range(S, -1, -1):
            C = out["cov"][b, t]
            Cx = prior[b, t] if mutant == "xs from the prior covariance" else C
            out["xs"][b, t] = (out["xhat"][b, t] + (Cx @ r).astype(f)).astype(f)
            out["cov_s"][b, t] = (C - ((C @ Lm).astype(f) if mutant == "cov - cov Lambda" else (C @ (Lm @ C).astype(f)).astype(f))).astype(f)
            order = recs[t] if mutant == "updates in forward order" else recs[t][::-1]
            for rec in order:
                if rec is None:
                    continue
                j, k, w, inv = rec
                q = (Lm.T @ k).astype(f)
                cq = zero if mutant == "c dropped" else f(k @ q)
                kr = zero if mutant == "k^T r dropped" else f(k @ r)
                rj = f(f(r[j] + (-w if mutant == "sign of e / s" else w)) - kr)
                Lm = Lm.copy()
                Lm[j, :] = (Lm[j, :] - q).astype(f)
                Lm[:, j] = (Lm[:, j] - q).astype(f)
                Lm[j, j] = f(Lm[j, j] + (cq if mutant == "1 / s dropped from Lambda" else f(cq + inv)))
                r = r.copy()
                r[j] = rj
            if t > 0:
                A = As[b, min(t, S - 1)] if mutant == "A_t for A_{t-1}" else As[b, t - 1]
                r = ((A if mutant == "A r for A^T r" else A.T) @ r).astype(f)
                if mutant != "Lambda not carried through the prediction":
                    Lm = (A.T @ (Lm @ A).astype(f)).astype(f)
    out["var"] = np.einsum("btii->bti", out["cov"]).copy()
    out["var_s"] = np.einsum("btii->bti", out["cov_s"]).copy()
    out["aux"] = dict(s_over_r=s_over_r, prior=prior, A=As)
    return out


def rts(c, ref):
    """The Rauch-Tung-Striebel smoother with an explicit solve, in fp64, on the filter of `ref` -> xs, cov_s."""
    B, S = c["B"], c["S"]
    xs, Ps = ref["xhat"].copy(), ref["cov"].copy()
    for b in range(B):
        spec = c["mspecs"][b]
        ub = c["u"] if c["u"].ndim == 2 else c["u"][b]
        for t in range(S - 1, -1, -1):
            A, Pb = ref["aux"]["A"][b, t], ref["aux"]["prior"][b, t + 1]
            xbar = o_lin.step(spec, ref["xhat"][b, t][None], ub[t].astype(np.float64)[None])[0]
            Cg = np.linalg.solve(Pb, A @ ref["cov"][b, t]).T
            xs[b, t] = ref["xhat"][b, t] + Cg @ (xs[b, t + 1] - xbar)
            Ps[b, t] = ref["cov"][b, t] + Cg @ (Ps[b, t + 1] - Pb) @ Cg.T
    return xs, Ps


def batch_update_errors(c, ref):
    """The sequential filter against the batch Kalman update with Joseph covariance on the readings that exist: the largest relative
    difference of the posterior mean and covariance over the batch and the steps."""
    worst, obs, n = 0.0, list(c["observed"]), c["n"]
    R = np.broadcast_to(np.asarray(c["meas_var"], dtype=np.float64), (c["B"], len(obs)))
    for b in range(c["B"]):
        spec = c["mspecs"][b]
        yb = c["y"] if c["y"].ndim == 2 else c["y"][b]
        ub = c["u"] if c["u"].ndim == 2 else c["u"][b]
        for t in range(c["S"] + 1):
            have = ~np.isnan(yb[t])
            P = ref["aux"]["prior"][b, t]
            xbar = c["xhat0"][b] if t == 0 else o_lin.step(spec, ref["xhat"][b, t - 1][None], ub[t - 1].astype(np.float64)[None])[0]
            if not have.any():
                x_b, P_b = xbar, P
            else:
                H = np.eye(n)[[j for j, h in zip(obs, have) if h]]
                Rm = np.diag(R[b][have])
                L = P @ H.T @ np.linalg.inv(H @ P @ H.T + Rm)
                x_b = xbar + L @ (yb[t][have] - H @ xbar)
                J = np.eye(n) - L @ H
                P_b = J @ P @ J.T + L @ Rm @ L.T
            worst = max(worst, np.max(np.abs(ref["xhat"][b, t] - x_b)) / np.max(np.abs(x_b)),
                        np.max(np.abs(ref["cov"][b, t] - P_b)) / max(np.max(np.abs(P_b)), 1e-300))
    return worst


def _nan_ratio(g, r, den):
    """|g - r| / den where both are numbers; inf where only one is NaN; a zero denominator asks for an exact zero."""
    g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
    assert g.shape == r.shape, (g.shape, r.shape)
    if not np.array_equal(np.isnan(g), np.isnan(r)):
        return np.inf
    ok = ~np.isnan(r)
    if not ok.any():
        return 0.0
    return pol._ratio((g - r)[ok], np.broadcast_to(den, r.shape)[ok], g[ok])


def errors(c, got):
    """got: dict with any of KEYS; c["ref"]: run() in fp64.  -> dict of the measures of the module docstring."""
    ref, out = c["ref"], {}
    spread = pol.SPREAD[c["model"]]
    for key in ("xhat", "xs"):
        if got.get(key) is not None:
            out[key] = _nan_ratio(got[key], ref[key], spread)
    for kc, kv in (("cov", "var"), ("cov_s", "var_s")):
        sub = {a: got[b] for a, b in (("cov", kc), ("var", kv)) if got.get(b) is not None}
        e = cc.errors(sub, dict(cov=ref[kc], var=ref[kv]), c["S"])
        e.pop("asym", None)
        out.update({dict(cov=kc, var=kv)[k]: v for k, v in e.items()})
    if got.get("innov") is not None:
        out["innov"] = _nan_ratio(got["innov"], ref["innov"], np.sqrt(ref["innov_var"]))
    for key in ("innov_var", "nis", "loglik"):
        if got.get(key) is not None:
            out[key] = _nan_ratio(got[key], ref[key], np.abs(ref[key]))
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
def case(model, integ="rk4", N=7, S=None, observed="pose", hetero=(), pattern="mixed", shared=False, zero_start=False, B=pol.B_CASE,
         check=True):
    """-> dict: y (B, S+1, p_y) or (S+1, p_y), u (B, S, m) or (S, m), observed, meas_var, xhat0, cov0, noise (fp32-rounded fp64 arrays or
    None), model_phys (float32 rows or None), mspecs (the filter's spec per trajectory), B, S, n, ref."""
    e = ec.case(model, integ=integ, N=N, S=S, observed=observed, hetero=tuple(hetero), B=B)
    S, obs = e["S"], e["observed"]
    n, p_y = e["x0"].shape[1], len(obs)
    x, u = e["ref"]["x"], e["ref"]["u"]
    Rb = np.broadcast_to(np.asarray(e["meas_var"], dtype=np.float64), (B, p_y))
    last = np.random.default_rng(SEED).standard_normal((pc.B_FULL[model], n))[:B][:, list(obs)] * np.sqrt(Rb)
    y = np.concatenate([x[:, :S][:, :, list(obs)] + e["meas_noise"].transpose(1, 0, 2), (x[:, S][:, list(obs)] + last)[:, None]], axis=1)
    y, u = f32(y), f32(u)
    y[missing_mask(pattern, B, S, p_y)] = np.nan
    if shared:
        y, u = y[0].copy(), u[0].copy()
    c = dict(model=model, integ=integ, N=N, S=S, B=B, n=n, observed=obs, meas_var=e["meas_var"], y=y, u=u, xhat0=e["xhat0"],
             cov0=None if zero_start else e["cov0"], noise=e["noise"], model_phys=e["model_phys"], mspecs=e["mspecs"], pattern=pattern)
    c["ref"] = ref = run(c)
    if check:
        assert ref["aux"]["s_over_r"] >= 1.0, ref["aux"]["s_over_r"]
        var, var_s = ref["var"], ref["var_s"]
        assert np.all(var_s >= 0.0) and np.all(var_s <= var * (1.0 + 1e-9)) and np.all(var_s[var > 0.0] > 0.0)
        if not np.all(np.isnan(c["y"])) and S > 1:
            # (the cart-pole's short cases: the velocities hang on later position readings through dt alone, 0.87 .. 0.996 of var)
            un = [i for i in range(n) if i not in obs] if (model == "quadrotor" or S >= 26) else []
            un = un or list(range(n))
            assert np.any(var_s[:, :, un] < 0.9 * var[:, :, un]), "the smoother does nothing"
        xr, Pr = rts(c, ref)
        d = errors(dict(c, ref=dict(ref, xs=xr, cov_s=Pr, var_s=np.einsum("btii->bti", Pr))), dict(xs=ref["xs"], cov_s=ref["cov_s"]))
        assert d["cov_s"] <= 1e-9 and d["xs"] <= 1e-9, d
        assert batch_update_errors(c, ref) <= 1e-12
    return c


def restatement(c):
    return run(c, dtype=np.float32)


def mutant_errors(c, name):
    return errors(c, run(c, mutant=name))


case_id = ec.case_id


# The cases the restatement is measured on and the GPU parity test runs: policy_cases.STEPS with the mixed patterns, every sensor, rows
# per trajectory, a shared log under heterogeneous hypotheses, a log without a single reading, and the zero start.
def parity_cases(model):
    out = []
    for integ in gc.INTEGRATORS:
        for N, S in pol.STEPS:
            out.append(dict(integ=integ, N=N, S=S))
        out.append(dict(integ=integ, N=7, S=7, observed="all", hetero=("model_phys", "meas_var")))
        out.append(dict(integ=integ, N=7, S=7, observed="single", pattern="e"))
        out.append(dict(integ=integ, N=7, S=5, hetero=("model_phys", "meas_var"), pattern="b", shared=True))
        out.append(dict(integ=integ, N=7, S=5, pattern="f"))
        out.append(dict(integ=integ, N=7, S=7, pattern="a", zero_start=True))
    return out


# ---------------------------------------------------------------------------------------------------------------- hypotheses
HYP_B = 8
HYP_S = 26
HYP_MASS = 0.85 * (1.15 / 0.85) ** (np.arange(HYP_B) / (HYP_B - 1.0))      # 0.85 .. 1.15 of the truth, no two equally near it
HYP_NOISE = 0.1                                                              # the sensor's sigma as a fraction of est_cases'


def hypotheses_case():
    """One shared quadrotor pose-sensor log (S = 26) from the skew plant, scored under HYP_B model_phys rows that differ only in the
    mass.  Asserts on the fp64 reference: argmax loglik is the row nearest the truth, and the gap to the second best is >= 100 x the
    GPU bound on loglik."""
    model = "quadrotor"
    e = ec.case(model, integ="rk4", N=HYP_S, S=HYP_S, observed="pose", B=1)
    obs = e["observed"]
    S, n, p_y = HYP_S, e["x0"].shape[1], len(obs)
    R = np.asarray(e["meas_var"], dtype=np.float64) * HYP_NOISE ** 2
    rng = np.random.default_rng(SEED + 1)
    y = f32(e["ref"]["x"][0][:, list(obs)] + np.sqrt(R) * rng.standard_normal((S + 1, p_y)))
    base = np.array([pc.SETS[model]["skew"]["phys"][k] for k in pc.PHYS_NAMES[model]], dtype=np.float64)
    rows = np.repeat(base[None], HYP_B, axis=0)
    im = list(pc.PHYS_NAMES[model]).index("mass")
    rows[:, im] = base[im] * HYP_MASS
    rows = rows.astype(np.float32)
    mspecs = [pc.spec_from(model, gc.params_with(model, None, rows[b]), "rk4") for b in range(HYP_B)]
    c = dict(model=model, integ="rk4", N=S, S=S, B=HYP_B, n=n, observed=obs, meas_var=f32(R), y=y, u=f32(e["ref"]["u"][0]),
             xhat0=np.repeat(e["xhat0"], HYP_B, axis=0), cov0=np.repeat(e["cov0"], HYP_B, axis=0),
             noise=np.repeat(e["noise"], HYP_B, axis=0), model_phys=rows, mspecs=mspecs, pattern="a")
    c["ref"] = run(c)
    ll = c["ref"]["loglik"]
    best = int(np.argmax(ll))
    assert best == int(np.argmin(np.abs(HYP_MASS - 1.0))), (best, ll)
    second = np.sort(ll)[-2]
    assert ll[best] - second >= 100.0 * gpu_bound(model, "loglik") * abs(ll[best]), (ll, gpu_bound(model, "loglik"))
    c["best"] = best
    return c


# ---------------------------------------------------------------------------------------------------------------- bounds
# E: the distance of the fp32 restatement from fp64 per measure, the worst over parity_cases, measured on the CPU and rounded up
# (tests/test_estimate_log_cpu.py holds the restatement to these figures).  The GPU tests assert, per measure, the larger of 4 x E and
# est_cases.FLOOR's floor: 1e-5 for the states, 2e-6 for the rest.
E = {"quadrotor": dict(xhat=2.4e-6, var=3.2e-6, cov=3.2e-6, innov=6.8e-5, innov_var=1.3e-6, nis=4.7e-5, loglik=1.0e-5, xs=2.4e-6,
                       var_s=1.2e-5, cov_s=5.2e-5),
     "cartpole": dict(xhat=6.4e-7, var=1.2e-6, cov=1.2e-6, innov=8.8e-6, innov_var=4.8e-7, nis=3.5e-5, loglik=1.4e-5, xs=6.7e-7,
                      var_s=8.0e-7, cov_s=8.0e-7)}
# (innov and nis carry e = y - xh[j], a difference of two nearly equal numbers, est_cases' note on nis; loglik is worst with the zero
# start, where ln(2 pi s) and e^2 / s nearly cancel in the sum.)  The smoothed covariance loses digits where var_s << var: the smallest
# var_s / var over parity_cases (where var > 0) is 0.062 for the quadrotor (S = 26: its cov_s figure) and 0.31 for the cart-pole.
MIN_VAR_RATIO = {"quadrotor": 0.062, "cartpole": 0.31}
FLOOR = {k: (ec.FLOOR["xhat"] if k in ("xhat", "xs") else ec.FLOOR["var"]) for k in KEYS}


def gpu_bound(model, key):
    return max(4.0 * E[model][key], FLOOR[key])


def over_bound(model, errs):
    """The largest ratio of a measure to its GPU bound."""
    return max(e / gpu_bound(model, k) for k, e in errs.items())


# Every mutant stands >= 10 x above the GPU bound of some measure in the case named here (model -> mutant -> keywords of case());
# measured values in tests/test_estimate_log_cpu.py's docstring.
TEETH = {model: {name: dict(integ="rk4", N=7, S=7) for name in MUTANTS} for model in pc.MODELS}
