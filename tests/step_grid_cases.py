"""The four closed-loop entries (ops.track_gradient, ops.track_covariance, ops.track_estimate, ops.estimate_log) at the run lengths
and batch sizes that policy_cases.STEPS = ((7, 7), (7, 5), (7, 1), (26, 26)) with B = 5 leaves out: the grid, its bounds and its
mutants.  A plain helper module (like tests/policy_cases.py, tests/cov_cases.py, tests/est_cases.py and tests/log_cases.py, whose
builders, references, measures and restatements it uses unchanged), used by tests/test_step_grid_cpu.py and
tests/test_step_grid_gpu.py.

What the old list leaves out.  The kernels work in blocks: track_covariance.hip COV_BLOCK = 4, estimate_log.hip LOG_BLOCK = 4,
track_gradient.hip QUATTRO_GRAD_BLOCK = 3.  S = 7, 5, 1, 26 leaves remainder 3, 1, 1, 2 modulo 4 and 1, 2, 1, 2 modulo 3: never 0.
    covariance : with S % 4 == 0 the last block is full, Sigma_S is parked in slot COV_BLOCK (the one reason SLOTS = COV_BLOCK + 1
                 exists) and the output loop makes a SECOND pass, in which three of the four lane rows redo the slot and must store
                 nothing; that pass writes cov[:, S], var[:, S] and the terminal term of excess and reads K, u at the clamped row S - 1
    log        : the backward pass stages A for LOG_BLOCK steps; with S % 4 != 0 the block at the low end is always partial
    gradient   : t_hi = S, S - 3, ...; the lowest block is partial in every old case, and S = 2 (shorter than a block, not 1) is absent
    batch      : one wave per workgroup, four trajectories per wave where a group has 16 lanes; B = 5 is one full wave and one with
                 three idle groups; B = 4, 8 (no idle group) and more than two waves are absent

The grid.  STEP_GRID (N, S), N > S everywhere so that the rows the run did not read are written too: S = 2 shorter than either block;
3 one full gradient block; 4 one full covariance / log block; 6, 9 multiples of 3 only; 8, 16 of 4 only; 12, 24 of both; 25 the row
after 24.  N is 7 or 26 (param_cases.inputs accepts the quadrotor horizons 1 .. 7 and 26 only) and S <= 26 (est_cases.case draws 26
rows of noise).  BATCH_AT = (26, 12) with B in batches(model) = (4, 8, param_cases.B_FULL[model]) and every kind of per-trajectory
row the family has.  OPTIONS: every option of a family at block-multiple S.  Both models, both integrators, always.

Bounds: the project's rule, per measure max(4 x E_GRID, floor) with the floors of the four modules.  E_GRID is the distance of the
fp32 restatement (policy_cases.reference(dtype=float32), cov_cases.restatement, est_cases.restatement, log_cases.restatement) from the
fp64 reference, the worst over the cases of THIS module, measured on the CPU and rounded up; tests/test_step_grid_cpu.py holds the
restatement to these figures and the figures to within 10 % of what it measures.  Neither side is code under test.  The E tables of
the four modules belong to their own cases and are not used here.

Shape mutants: transformations of the fp64 reference (its outputs, or its inputs) that restate what a kernel would do if the path it
takes ONLY at a block multiple were wrong.  Each is the identity where S is no multiple of its block, so it is invisible on every
case of the family's parity_cases, and stands >= 10 x above the bound in the case SHAPE_TEETH names.  Measured worst-case distances
(the largest measure), quadrotor / cart-pole: in the SHAPE_TEETH case; [the smallest .. the largest over every case of all_cases()
with S a multiple of the block]; the GPU bound:
    covariance "terminal slot stale"                    : 2.4e+1 / 1.1e+0;  [0.61 .. 25] / [0.16 .. 1.1];     bound 7.2e-6 / 9.6e-6
    covariance "second pass stores from every lane row" : 8.9e-1 / 1.7e+0;  [0.34 .. 1.5] / [0.16 .. 1.7]     (an exact zero
                                                          overwritten at the zero start: inf);                 bound 7.2e-6 / 9.6e-6
    log        "full low block"                         : cov_s 4.5e-2 / 3.3e-3 (xs 5.2e-3 / 2.1e-5): 520 x / 960 x the bound of the
                                                          measure; [0 .. 0.16] / [0 .. 0.033], 0 where Sigma_0 = 0 (the zero start)
                                                          or the log has no reading (pattern f): step 0's outputs do not see A_0
    gradient   "full low block"                         : 7.4e-3 / 2.8e-3;  [4.2e-4 .. 3.6e-2] / [6.4e-4 .. 5.0e-3];  bound 2.0e-6 / 3.4e-6
On the old cases the three that transform arrays ARE the reference (its own asymmetry, <= 1.3e-15, is all the cov measures show), and
the log mutant, which restates the smoother's recursion to run it on other A, reproduces the reference's xs, cov_s and var_s exactly
(tests/test_step_grid_cpu.py asserts < 1e-12).
"""
import functools

import numpy as np

import cov_cases as cc
import est_cases as ec
import grad_cases as gc
import log_cases as lc
import param_cases as pc
import policy_cases as pol

FAMILIES = ("gradient", "covariance", "estimate", "log")
BLOCKS = {"gradient": 3, "covariance": 4, "log": 4}           # read from the sources by tests/test_step_grid_cpu.py
STEP_GRID = ((7, 2), (7, 3), (7, 4), (7, 6), (26, 8), (26, 9), (26, 12), (26, 16), (26, 24), (26, 25))
N_OF = {S: N for N, S in STEP_GRID}
BATCH_AT = (26, 12)
OTHER = ec.OTHER


def batches(model):
    return (4, 8, pc.B_FULL[model])


ROWS = {"gradient": dict(hetero=("weights", "phys"), R=4), "covariance": dict(hetero=("weights", "phys")),
        "estimate": dict(hetero=("plant_phys", "model_phys", "meas_var")), "log": dict(hetero=("model_phys", "meas_var"))}
_BUILD = {"gradient": pol.case, "covariance": cc.case, "estimate": ec.case, "log": lc.case}


# ---------------------------------------------------------------------------------------------------------------- cases
def step_cases(family, model, integ):
    """The keywords of the family's case() over STEP_GRID (the skew set, B = policy_cases.B_CASE, every option at its default)."""
    head = dict(set_name="skew") if family in ("gradient", "covariance") else {}
    return [dict(head, integ=integ, N=N, S=S) for N, S in STEP_GRID]


def batch_cases(family, model, integ):
    """BATCH_AT under every kind of row of the family, B in batches(model)."""
    head = dict(set_name="skew") if family in ("gradient", "covariance") else {}
    N, S = BATCH_AT
    return [dict(head, integ=integ, N=N, S=S, B=B, **ROWS[family]) for B in batches(model)]


def option_cases(family, model, integ):
    """A block-multiple S with every option the family has."""
    out = []
    at = lambda S, **kw: dict(integ=integ, N=N_OF[S], S=S, **kw)
    if family == "gradient":
        for S in (3, 6, 12):
            out.append(at(S, set_name="skew", terminal=False))
            out.append(at(S, set_name="skew", hetero=("weights", "phys"), R=4))
            out.append(at(S, set_name="skew", plant_integ=OTHER[integ], hetero=("phys",)))
        for S in (3, 12):
            out += [at(S, set_name=name) for name in gc.SETS[model] if name != "skew"]
    elif family == "covariance":
        for S in (4, 12):
            out.append(at(S, set_name="skew", terminal=False))
            out.append(at(S, set_name="skew", open=True))
            out.append(at(S, set_name="skew", cov="zero_start"))
            out.append(at(S, set_name="skew", hetero=("weights", "phys")))
            out.append(at(S, set_name="skew", plant_integ=OTHER[integ], hetero=("phys",)))
    elif family == "estimate":
        for S in (4, 12):
            out.append(at(S, observed="all"))
            out.append(at(S, observed="single"))
            out.append(at(S, plant_integ=OTHER[integ], hetero=("plant_phys", "model_phys", "meas_var")))
            out.append(at(S, plain=True))
    else:
        assert family == "log", family
        for S in (4, 8):
            out += [at(S, pattern=k) for k in lc.PATTERNS]
        out.append(at(12, hetero=("model_phys", "meas_var"), pattern="b", shared=True))
        out.append(at(8, pattern="a", zero_start=True))
        out.append(at(4, observed="all"))
        out.append(at(4, observed="single"))
    return out


def all_cases(family, model, integ):
    return step_cases(family, model, integ) + option_cases(family, model, integ) + batch_cases(family, model, integ)


def case_id(kw):
    return "-".join(f"{k}={'+'.join(v) if isinstance(v, tuple) else v}" for k, v in kw.items())


@functools.lru_cache(maxsize=None)
def _built(family, model, items, check):
    kw = dict(items)
    if family == "log":
        kw["check"] = check
    return _BUILD[family](model, **kw)


def build(family, model, kw, check=False):
    """The family's case() on the keywords kw, built once per process and shared: the callers leave it unchanged.  check: log_cases'
    assertions on the fp64 reference (the other builders always make theirs)."""
    return _built(family, model, tuple(kw.items()), bool(check) and family == "log")


def reference_errors(family, model, c, got):
    """The family's own measures of `got` against the fp64 reference of case c."""
    if family == "gradient":
        return pol.case_errors(c, got)
    if family == "covariance":
        return cc.case_errors(c, got)
    return (ec if family == "estimate" else lc).errors(c, got)


def restatement(family, c):
    if family == "gradient":
        return pol.reference(c["d"], c["x"], c["x_nom"], c["K"], c["N"], c["terminal"], dtype=np.float32)
    return {"covariance": cc, "estimate": ec, "log": lc}[family].restatement(c)


# ---------------------------------------------------------------------------------------------------------------- bounds
# E_GRID: the restatement's distance from fp64, the worst over all_cases() of both integrators, measured on the CPU and rounded up;
# the case that sets a figure is named beside it (case_id's keywords; skew set, B = 5 where none is given).  gradient and covariance:
# one figure for all measures, as policy_cases.E and cov_cases.E are; estimate and log: per measure, as est_cases.E and log_cases.E.
# Rounded up by 4 .. 7 %: the restatement's products go through the host's BLAS, whose summation order is not the same everywhere.
E_GRID = {
    "gradient": {"quadrotor": 4.7e-7,       # 4.48e-7: costate, euler N=26 S=24
                 "cartpole": 8.6e-7},       # 8.29e-7: costate, rk4 N=26 S=12 terminal=False (4.3e-7 over STEP_GRID alone)
    "covariance": {"quadrotor": 1.8e-6,     # 1.71e-6: var_u, rk4 N=26 S=12 B=19 weights+phys (cov, var: 1.66e-6 at rk4 N=26 S=24)
                   "cartpole": 2.4e-6},     # 2.26e-6: var_u, rk4 N=26 S=12 weights+phys
    "estimate": {
        "quadrotor": dict(x=4.1e-6,         # 3.93e-6: rk4 N=26 S=12 B=8, all three kinds of rows
                          xhat=3.0e-6,      # 2.87e-6: the same case
                          u=6.1e-5,         # 5.85e-5: rk4 N=26 S=12 plant euler, all three kinds of rows
                          var=3.2e-6, cov=3.2e-6,   # 3.07e-6: euler N=7 S=4 plant rk4, all three kinds of rows
                          asym=4.8e-7,      # 4.61e-7: euler N=26 S=12 observed=single
                          nis=2.2e-3),      # 2.09e-3: rk4 N=26 S=12 observed=single (one e^2 / s per step: est_cases' note on nis)
        "cartpole": dict(x=1.6e-6,          # 1.50e-6: euler N=26 S=12 B=9, all three kinds of rows
                         xhat=1.1e-6,       # 1.03e-6: rk4 N=26 S=12 B=8, all three kinds of rows
                         u=2.0e-6,          # 1.86e-6: euler N=26 S=12 B=8, all three kinds of rows
                         var=1.2e-6, cov=1.2e-6,    # 1.15e-6: euler N=7 S=2
                         asym=2.6e-7,       # 2.45e-7: rk4 N=26 S=12 observed=single
                         nis=1.03e-3)},     # 9.83e-4: rk4 N=7 S=4 observed=single
    "log": {
        "quadrotor": dict(xhat=2.3e-6, xs=2.3e-6,   # 2.17e-6: rk4 N=26 S=12 B=19 model_phys+meas_var
                          var=3.2e-6, cov=3.2e-6,   # 3.07e-6: euler N=26 S=12 shared, pattern b, model_phys+meas_var
                          cov_s=7.4e-5,     # 7.09e-5: rk4 N=26 S=24 (var_s << var: log_cases' note on the smoothed covariance)
                          var_s=1.6e-5,     # 1.51e-5: euler N=26 S=24
                          innov=3.7e-5,     # 3.53e-5: euler N=26 S=12 B=19 model_phys+meas_var
                          innov_var=1.35e-6,        # 1.27e-6: euler N=26 S=12 B=4 model_phys+meas_var
                          nis=7.5e-5,       # 7.13e-5: euler N=7 S=4 observed=single
                          loglik=2.55e-6),  # 2.41e-6: rk4 N=26 S=8 pattern a, zero start
        "cartpole": dict(xhat=1.17e-6, xs=1.17e-6,  # 1.11e-6: euler N=26 S=12 B=9 model_phys+meas_var
                         var=1.2e-6, cov=1.2e-6,    # 1.15e-6: euler N=7 S=2
                         cov_s=8.6e-7, var_s=8.6e-7,        # 8.16e-7: rk4 N=26 S=24
                         innov=8.9e-6,      # 8.46e-6: rk4 N=7 S=4 observed=all
                         innov_var=5.2e-7,  # 4.90e-7: rk4 N=7 S=4 pattern a
                         # 4.60e-4: euler N=26 S=12 B=8 (and B=9) model_phys+meas_var, trajectory 6, step 2.  Its pattern is "b": the
                         # first sensor is absent at step 2, so that step's nis is ONE e^2 / s, and the reference's value there is 6.0e-4
                         # (e passes near zero); the relative measure divides by it.  est_cases' cancellation, not a kernel matter; the next
                         # row of that case stands at 7.8e-5.  No other measure is widened for it and the trajectory stays.
                         nis=4.85e-4,
                         loglik=8.8e-7)},   # 8.37e-7: rk4 N=26 S=12 shared, pattern b, model_phys+meas_var
}
FLOOR = {"gradient": pol.FLOOR, "covariance": cc.FLOOR, "estimate": ec.FLOOR, "log": lc.FLOOR}


def e_grid(family, model, key):
    e = E_GRID[family][model]
    return e[key] if isinstance(e, dict) else e


def gpu_bound(family, model, key):
    """What the GPU tests assert for measure `key`: the larger of 4 x E_GRID and the family's floor."""
    floor = FLOOR[family]
    return max(4.0 * e_grid(family, model, key), floor[key] if isinstance(floor, dict) else floor)


def over_bound(family, model, errs):
    """The largest ratio of a measure to its GPU bound."""
    return max(e / gpu_bound(family, model, k) for k, e in errs.items())


# ---------------------------------------------------------------------------------------------------------------- shape mutants
SHAPE_MUTANTS = {"covariance": ("terminal slot stale", "second pass stores from every lane row"), "log": ("full low block",),
                 "gradient": ("full low block",)}


def _smooth(c, ref, As):
    """log_cases.run's Bryson-Frazier backward pass in fp64, restated over the filter of `ref` (its priors, posteriors and
    innovations) with the step Jacobians As (B, S, n, n) -> dict(xs, cov_s, var_s).  With As = ref["aux"]["A"] it is ref's own."""
    B, S, n, obs = c["B"], c["S"], c["n"], c["observed"]
    R = np.broadcast_to(np.asarray(c["meas_var"], dtype=np.float64), (B, len(obs)))
    xs, cov_s = np.zeros((B, S + 1, n)), np.zeros((B, S + 1, n, n))
    for b in range(B):
        yb = c["y"] if c["y"].ndim == 2 else c["y"][b]
        r, Lm = np.zeros(n), np.zeros((n, n))
        for t in range(S, -1, -1):
            C = ref["cov"][b, t]
            xs[b, t] = ref["xhat"][b, t] + C @ r
            cov_s[b, t] = C - C @ (Lm @ C)
            P, recs = ref["aux"]["prior"][b, t].copy(), []
            for i, j in enumerate(obs):                          # the sequential update again, for each reading's k, e / s and 1 / s
                if np.isnan(yb[t, i]):
                    continue
                inv = 1.0 / (P[j, j] + R[b, i])
                k = P[j, :] * inv
                recs.append((j, k, ref["innov"][b, t, i] * inv, inv))
                P = P - np.outer(P[:, j].copy(), k)
            for j, k, w, inv in recs[::-1]:
                q = Lm.T @ k
                cq, rj = k @ q, (r[j] + w) - k @ r
                Lm = Lm.copy()
                Lm[j, :] -= q
                Lm[:, j] -= q
                Lm[j, j] += cq + inv
                r = r.copy()
                r[j] = rj
            if t > 0:
                A = As[b, t - 1]
                r, Lm = A.T @ r, A.T @ (Lm @ A)
    return dict(xs=xs, cov_s=cov_s, var_s=np.einsum("btii->bti", cov_s).copy())


def shape_mutant(family, name, c):
    """Mutant `name` of the fp64 reference of case c -> the outputs it changes, in the shapes of the entry's (the identity where S is
    no multiple of the family's block)."""
    S, ref = c["S"], c["ref"]
    hit = S % BLOCKS[family] == 0
    if family == "covariance":
        got = {k: ref[k].copy() for k in cc.KEYS}
        if hit and name == "terminal slot stale":
            # slot COV_BLOCK still holds what the block before parked there: rows S of cov and var are row S - 4's, and the terminal
            # term of excess is formed from that row
            got["cov"][:, S], got["var"][:, S] = ref["cov"][:, S - 4], ref["var"][:, S - 4]
            if c["terminal"]:
                got["excess"] = ref["excess"] + 0.5 * np.einsum("bii,bi->b", c["d"]["VxxN"], ref["var"][:, S - 4] - ref["var"][:, S])
        elif hit:
            assert name == "second pass stores from every lane row", name
            # lane rows 1 .. 3 of the second pass store the terminal slot where their first-pass slots went: steps S - 3 .. S - 1
            got["cov"][:, S - 3:S], got["var"][:, S - 3:S] = ref["cov"][:, S:S + 1], ref["var"][:, S:S + 1]
        return got
    if family == "gradient":
        assert name == "full low block", name
        d = dict(c["d"])
        if hit and S > 1:
            # the lowest block's stage slot of step 0 still holds step 1's columns of [A | B]
            d["A"], d["B"] = c["d"]["A"].copy(), c["d"]["B"].copy()
            d["A"][:, 0], d["B"][:, 0] = c["d"]["A"][:, 1], c["d"]["B"][:, 1]
        return pol.reference(d, c["x"], c["x_nom"], c["K"], c["N"], c["terminal"])
    assert family == "log" and name == "full low block", (family, name)
    As = ref["aux"]["A"].copy()
    if hit and S > 1:
        As[:, 0] = ref["aux"]["A"][:, 1]                          # the stage slot of step 0 still holds the A of step 1
    return _smooth(c, ref, As)


def shape_mutant_errors(family, model, name, c):
    """How far the mutant stands from the reference in case c, under the family's own measures."""
    return reference_errors(family, model, c, shape_mutant(family, name, c))


# Every shape mutant stands >= 10 x above gpu_bound of some measure in the case named here (all of them cases of all_cases()).
SHAPE_TEETH = {
    "covariance": {model: {"terminal slot stale": dict(set_name="skew", integ="rk4", N=7, S=4),
                           "second pass stores from every lane row": dict(set_name="skew", integ="rk4", N=7, S=4)}
                   for model in pc.MODELS},
    "log": {model: {"full low block": dict(integ="rk4", N=7, S=4)} for model in pc.MODELS},
    "gradient": {model: {"full low block": dict(set_name="skew", integ="rk4", N=7, S=3)} for model in pc.MODELS},
}
