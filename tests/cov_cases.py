"""The first-order covariance of a tracked closed-loop run (quattro_track_covariance_f32, ops.track_covariance, QuattroILQR.tube): the
cases, the fp64 reference, the error measures, the fp32 restatement, the mutants and the bounds.  A plain helper module (like
tests/policy_cases.py, on which it builds), used by tests/test_track_covariance_cpu.py and tests/test_track_covariance_gpu.py.

Case: policy_cases.case as it stands (the realised run x, u of the oracle's closed loop under the plant's spec, rounded to fp32, the
gains K, the fp64 blocks d about the run), B = 5, plus a seeded start covariance and noise:
    cov0  = diag((0.05 x spread)^2) + G G^T,  G = 0.02 x spread[:, None] x N(0, 1) (n x n): dense and positive definite
    noise = diag((0.01 x spread)^2)
(spread: param_cases' spread of the starts), both rounded to fp32.  cov="zero_start": cov0 = None and noise on the velocity states
only, which makes exact zeros in Sigma_0 and Sigma_1.  open=True: K = None (the open loop about the same run).

Reference (fp64): over Acl = policy_cases.compose(d, K)["A"] = A + B K,
    Sigma_0 = cov0,   Sigma_{t+1} = Acl_t Sigma_t Acl_t^T + W,   var_u_t = diag(K_t Sigma_t K_t^T)
    excess = sum_{t<S} [ 1/2 tr(l_xx,t Sigma_t) + 1/2 tr(l_uu,t K_t Sigma_t K_t^T) ] + [terminal] 1/2 tr(V_xx(N) Sigma_S)
with l_xx, l_uu, V_xx(N) the oracle's blocks (diagonal for both models, l_ux = 0: the sum the entry's header states).

Error measures (the largest over the batch, the steps and the entries):
    cov[t][i][j]  : |d| / sqrt(Sigma_t[i][i] Sigma_t[j][j]), the reference's Sigma: the error of a correlation coefficient
    asym          : |got[t][i][j] - got[t][j][i]| under the same scale (the device reads Sigma as symmetric)
    var, var_u    : |d| / the reference entry
    excess        : |d| / the reference value
An entry whose denominator is exactly zero must be exactly zero (its error is then 0, otherwise inf) and is left out of the ratio
(policy_cases._ratio); rows t >= S of var_u must be exactly +0.0.
"""
import numpy as np

import grad_cases as gc
import param_cases as pc
import policy_cases as pol

f32 = gc.f32
KEYS = ("cov", "var", "var_u", "excess")
COV_SEED = 67
VELOCITY = {"quadrotor": (3, 4, 5, 9, 10, 11), "cartpole": (1, 3)}
MUTANTS = ("W added before the product", "Acl of step t + 1", "B K dropped", "Acl^T Sigma Acl", "W dropped", "cov0 dropped",
           "var_u from Sigma_{t+1}", "K of step t + 1 in var_u", "excess without the control term", "excess with 2 q for q",
           "terminal term kept with the flag off")


# ---------------------------------------------------------------------------------------------------------------- inputs
def cov_inputs(model, B, kind="dense"):
    """-> (cov0 (B, n, n) or None, noise (B, n, n)), fp32-rounded fp64 arrays, seeded; a trajectory's pair does not depend on B."""
    n = pc.DIMS[model][0]
    spread = pol.SPREAD[model]
    rng = np.random.default_rng(COV_SEED)
    G = 0.02 * spread[None, :, None] * rng.standard_normal((pc.B_FULL[model], n, n))[:B]
    cov0 = f32(np.diag((0.05 * spread) ** 2)[None] + G @ G.transpose(0, 2, 1))
    cov0 = 0.5 * (cov0 + cov0.transpose(0, 2, 1))               # (exactly symmetric after the rounding)
    w = np.repeat(((0.01 * spread) ** 2)[None, :], B, axis=0)
    if kind == "zero_start":
        keep = np.zeros(n)
        keep[list(VELOCITY[model])] = 1.0
        return None, f32(np.einsum("bi,ij->bij", w * keep[None, :], np.eye(n)))
    assert kind == "dense"
    return cov0, f32(np.einsum("bi,ij->bij", w, np.eye(n)))


# ---------------------------------------------------------------------------------------------------------------- reference
def propagate(d, K, cov0, noise, N, terminal=True, dtype=np.float64, mutant=None):
    """d: the fp64 blocks about the realised run over S steps; K (B, N, m, n) or None; cov0, noise (B, n, n) or None.
    -> dict of KEYS in the shapes of the entry's outputs (cov (B, S+1, n, n), var (B, S+1, n), var_u (B, N, m), excess (B,) fp64).
    dtype float32: the restatement (A, B, K, cov0, noise rounded to fp32; A + B K, the recursion and the products in fp32; the terms
    of excess are fp64 products of the fp32 entries, as on the device).  mutant: one of MUTANTS."""
    Bt, S, n, m = d["B"].shape
    A, Bm = d["A"].astype(dtype), d["B"].astype(dtype)
    Ks = np.zeros((Bt, S, m, n), dtype=dtype) if K is None else np.asarray(K)[:, :S].astype(dtype)
    Acl = A if mutant == "B K dropped" else (A + np.matmul(Bm, Ks)).astype(dtype)
    if mutant == "Acl of step t + 1":
        Acl = Acl[:, [min(t + 1, S - 1) for t in range(S)]]
    W = np.zeros((Bt, n, n), dtype=dtype) if noise is None or mutant == "W dropped" else np.asarray(noise).astype(dtype)
    sig = np.zeros((Bt, S + 1, n, n), dtype=dtype)
    if cov0 is not None and mutant != "cov0 dropped":
        sig[:, 0] = np.asarray(cov0).astype(dtype)
    for t in range(S):
        a, s = Acl[:, t], sig[:, t]
        if mutant == "W added before the product":
            sig[:, t + 1] = np.matmul(a, np.matmul(s + W, a.transpose(0, 2, 1)))
        elif mutant == "Acl^T Sigma Acl":
            sig[:, t + 1] = np.matmul(a.transpose(0, 2, 1), np.matmul(s, a)) + W
        else:
            sig[:, t + 1] = np.matmul(a, np.matmul(s, a.transpose(0, 2, 1))) + W
    var = np.einsum("btii->bti", sig).copy()
    Kv = Ks[:, [min(t + 1, S - 1) for t in range(S)]] if mutant == "K of step t + 1 in var_u" else Ks
    sv = sig[:, 1:] if mutant == "var_u from Sigma_{t+1}" else sig[:, :S]
    vu = np.einsum("btai,btij,btaj->bta", Kv, sv, Kv).astype(dtype)
    var_u = np.zeros((Bt, N, m), dtype=dtype)
    var_u[:, :S] = vu
    f64 = np.float64
    qx = 0.5 * np.einsum("btii->bti", d["lxx"]) * (2.0 if mutant == "excess with 2 q for q" else 1.0)
    term = np.einsum("bti,bti->bt", qx, var[:, :S].astype(f64))
    if mutant != "excess without the control term":
        term = term + 0.5 * np.einsum("btaa,bta->bt", d["luu"], vu.astype(f64))
    excess = np.zeros(Bt)
    for t in range(S):
        excess = excess + term[:, t]
    if terminal or mutant == "terminal term kept with the flag off":
        excess = excess + 0.5 * np.einsum("bii,bi->b", d["VxxN"], var[:, S].astype(f64))
    return dict(cov=sig, var=var, var_u=var_u, excess=excess)


def errors(got, ref, S):
    """got: dict with any of KEYS; ref: propagate() in fp64.  -> dict of the measures of the module docstring (and "asym" with cov)."""
    out = {}
    sd = np.sqrt(np.einsum("btii->bti", ref["cov"]))
    scale = sd[:, :, :, None] * sd[:, :, None, :]
    if got.get("cov") is not None:
        g = np.asarray(got["cov"], dtype=np.float64)
        assert g.shape == ref["cov"].shape, (g.shape, ref["cov"].shape)
        out["cov"] = pol._ratio(g - ref["cov"], scale, g)
        out["asym"] = pol._ratio(g - g.transpose(0, 1, 3, 2), scale, g)
    if got.get("var") is not None:
        g = np.asarray(got["var"], dtype=np.float64)
        assert g.shape == ref["var"].shape, (g.shape, ref["var"].shape)
        out["var"] = pol._ratio(g - ref["var"], np.abs(ref["var"]), g)
    if got.get("var_u") is not None:
        g = np.asarray(got["var_u"], dtype=np.float64)
        assert g.shape == ref["var_u"].shape, (g.shape, ref["var_u"].shape)
        tail = g[:, S:]
        if tail.size and not (np.all(tail == 0.0) and not np.any(np.signbit(tail))):
            out["var_u"] = np.inf
        else:
            out["var_u"] = pol._ratio(g[:, :S] - ref["var_u"][:, :S], np.abs(ref["var_u"][:, :S]), g[:, :S])
    if got.get("excess") is not None:
        g = np.asarray(got["excess"], dtype=np.float64)
        assert g.shape == ref["excess"].shape
        out["excess"] = pol._ratio(g - ref["excess"], np.abs(ref["excess"]), g)
    return out


def worst(errs):
    return max(errs.values())


# ---------------------------------------------------------------------------------------------------------------- cases
def case(model, set_name="skew", integ="rk4", N=7, S=None, terminal=True, plant_integ=None, hetero=(), cov="dense", open=False,
         B=pol.B_CASE):
    """policy_cases.case plus cov0, noise (None or (B, n, n)), Kc (the gains the entry is given: K, or None with open=True) and
    ref = propagate() in fp64."""
    c = pol.case(model, set_name, integ, N, S, B=B, terminal=terminal, plant_integ=plant_integ, hetero=hetero)
    cov0, noise = cov_inputs(model, c["x"].shape[0], cov)
    Kc = None if open else c["K"]
    Nv = c["S"] if open else N                                  # var_u has the gains' rows; without gains, the run's
    c.update(cov0=cov0, noise=noise, Kc=Kc, Nv=Nv, ref=propagate(c["d"], Kc, cov0, noise, Nv, terminal))
    return c


def case_errors(c, got):
    return errors(got, c["ref"], c["S"])


def restatement(c):
    return propagate(c["d"], c["Kc"], c["cov0"], c["noise"], c["Nv"], c["terminal"], dtype=np.float32)


def mutant_errors(c, name):
    """How far mutant `name` of the reference stands from the reference, in case c."""
    return case_errors(c, propagate(c["d"], c["Kc"], c["cov0"], c["noise"], c["Nv"], c["terminal"], mutant=name))


# The cases the restatement is measured on and the GPU parity test runs: both models, both integrators, the skew set, policy_cases.STEPS
# (S = 7, 5, 1, 26: the remainders 3, 1, 1, 2 of a four-step pass, one pass and several; NOT remainder 0, the one length at which the
# terminal slot goes into a second output pass -- tests/step_grid_cases.py has those lengths), rows per trajectory, a plant with the other integrator, the terminal
# flag off, the zero start and the open loop.
def parity_cases(model):
    out = []
    other = {"euler": "rk4", "rk4": "euler"}
    for integ in gc.INTEGRATORS:
        for N, S in pol.STEPS:
            out.append(dict(set_name="skew", integ=integ, N=N, S=S))
        out.append(dict(set_name="skew", integ=integ, N=7, S=5, hetero=("weights", "phys")))
        out.append(dict(set_name="skew", integ=integ, N=7, S=7, plant_integ=other[integ], hetero=("phys",)))
        out.append(dict(set_name="skew", integ=integ, N=7, S=5, terminal=False))
        out.append(dict(set_name="skew", integ=integ, N=7, S=7, cov="zero_start"))
        out.append(dict(set_name="skew", integ=integ, N=7, S=5, open=True))
    return out


case_id = pol.case_id

# ---------------------------------------------------------------------------------------------------------------- bounds
# E: the distance of the fp32 restatement from fp64 under the measures above (cov, var, var_u, excess and the asymmetry), the worst
# over parity_cases, measured on the CPU (tests/test_track_covariance_cpu.py holds the restatement to these figures).  The GPU tests
# assert the larger of 4 x E and the fp32 floor of the project's rollout comparisons (param_cases.BOUNDS["sim_x"] = 2e-6): the device
# forms its own fp32 tangents, which the restatement does not model (policy_cases.gpu_bound's factor, for the same reason).
E = {"quadrotor": 1.9e-6, "cartpole": 1.9e-6}
FLOOR = pc.BOUNDS["sim_x"]


def gpu_bound(model):
    return max(4.0 * E[model], FLOOR)


# Every mutant stands >= 10 x above gpu_bound in the case named here (model -> mutant -> keywords of case()); measured values in
# tests/test_track_covariance_cpu.py's docstring.
def _k(integ, N, S, **kw):
    return dict(set_name="skew", integ=integ, N=N, S=S, **kw)


TEETH = {
    "quadrotor": {
        "W added before the product": _k("euler", 26, 26), "Acl of step t + 1": _k("rk4", 7, 7, plant_integ="euler", hetero=("phys",)),
        "B K dropped": _k("euler", 26, 26), "Acl^T Sigma Acl": _k("rk4", 7, 7, cov="zero_start"),
        "W dropped": _k("euler", 7, 7, cov="zero_start"), "cov0 dropped": _k("euler", 7, 7),
        "var_u from Sigma_{t+1}": _k("euler", 7, 7, plant_integ="rk4", hetero=("phys",)),
        "K of step t + 1 in var_u": _k("euler", 26, 26), "excess without the control term": _k("rk4", 7, 5, terminal=False),
        "excess with 2 q for q": _k("rk4", 7, 5, terminal=False), "terminal term kept with the flag off": _k("euler", 7, 5, terminal=False)},
    "cartpole": {
        "W added before the product": _k("rk4", 26, 26), "Acl of step t + 1": _k("rk4", 26, 26),
        "B K dropped": _k("euler", 26, 26), "Acl^T Sigma Acl": _k("rk4", 7, 7, cov="zero_start"),
        "W dropped": _k("euler", 7, 7, cov="zero_start"), "cov0 dropped": _k("euler", 7, 7),
        "var_u from Sigma_{t+1}": _k("euler", 7, 7, plant_integ="rk4", hetero=("phys",)),
        "K of step t + 1 in var_u": _k("euler", 26, 26), "excess without the control term": _k("euler", 7, 7, cov="zero_start"),
        "excess with 2 q for q": _k("rk4", 7, 5, terminal=False), "terminal term kept with the flag off": _k("euler", 7, 5, terminal=False)},
}

# ---------------------------------------------------------------------------------------------------------------- definition check
# h in units of one standard deviation of the start: the 2n starts are x0 +- h L[:, c], L L^T = cov0.  The distance falls as h^2
# from 1.2e-6 (2.0e-6 for the cart-pole) at h = 0.1 to the figures below at h = 1e-3; halving h again moves the estimate by 1e-10 of
# the scale (far below 1e-3 of the distance that a mutant makes), and from h = 1e-4 on round-off makes it grow.
FD_H = 1e-3
FD_B = 3
# Measured (skew set, N = 7, both models and integrators, a plant with the other integrator included): the worst distance, under the
# cov measure, between the fp64 reference about the fp64 run (W = 0) and sum_c delta_c delta_c^T / h^2, delta_c half the difference of
# the oracle's closed-loop runs from x0 + h L[:, c] and x0 - h L[:, c]; asserted: 10 x that.
FD_WORST = {"quadrotor": 1.3e-10, "cartpole": 2.1e-10}
FD_BOUND = {model: 10.0 * v for model, v in FD_WORST.items()}


def fd_errors(model, integ, plant_integ, N=7, h=FD_H):
    """-> the worst cov-measure distance between the reference recursion and the sigma-point spread of the oracle's own closed loop."""
    from oracle import linearize as o_lin
    c = pol.case(model, "skew", integ, N, B=FD_B, plant_integ=plant_integ, hetero=("phys",))
    cov0, _ = cov_inputs(model, FD_B)
    n = pc.DIMS[model][0]
    run = lambda b, x0: o_lin.closed_loop_rollout_batched(c["specs"][b], x0, np.repeat(c["x_nom"][b:b + 1], x0.shape[0], axis=0),
                                                           np.repeat(c["u_nom"][b:b + 1], x0.shape[0], axis=0),
                                                           np.zeros((x0.shape[0],) + c["u_nom"].shape[1:]),
                                                           np.repeat(c["K"][b:b + 1], x0.shape[0], axis=0), 1.0)
    out = 0.0
    for b in range(FD_B):
        x, u, _ = run(b, c["x0"][b:b + 1])
        d = gc.blocks(c["specs"][b], x, u)
        ref = propagate(d, c["K"][b:b + 1], cov0[b:b + 1], None, N)
        L = np.linalg.cholesky(cov0[b])
        xp = run(b, c["x0"][b][None, :] + h * L.T)[0]           # row c: x0 + h L[:, c]
        xm = run(b, c["x0"][b][None, :] - h * L.T)[0]
        delta = 0.5 * (xp - xm)                                   # (n, N + 1, n)
        est = np.einsum("cti,ctj->tij", delta, delta)[None] / (h * h)
        out = max(out, errors(dict(cov=est), ref, N)["cov"])
    assert n == L.shape[0]
    return out


# ---------------------------------------------------------------------------------------------------------------- the tile mapping
def tile16_step(sig, acl, w):
    """One step of the quadrotor kernel's chain, restated lane by lane for the operand layouts of v_mfma_f32_16x16x4_f32 (lane l:
    A[i = l % 16][k = l // 16], B[k = l // 16][j = l % 16]; C/D register v: [4 (l // 16) + v][l % 16]).  sig, w (16, 16): the
    padded Sigma_t and W; acl (16, 16): the padded Acl_t as it is staged (row-major).  Lane (g, j) holds sig[4 g + v][j] in register v
    and reads acl[j][4 g .. 4 g + 3]; U = Sigma Acl^T takes register v of Sigma as the A operand -- which is Sigma[4 g + v][j] where
    the instruction expects Sigma[j][4 g + v] -- and Sigma' = Acl U + W takes register v of U as the B operand.  -> Sigma' (16, 16)."""
    lanes = np.arange(64)
    g, j = lanes // 16, lanes % 16

    def mfma(a, b, c):
        """a, b (64,): one operand register; c (64, 4) -> d (64, 4) for the k-slice the lanes' groups hold."""
        A = np.zeros((16, 4), dtype=c.dtype)
        Bm = np.zeros((4, 16), dtype=c.dtype)
        A[j, g] = a
        Bm[g, j] = b
        D = A @ Bm
        return c + np.stack([D[4 * g + v, j] for v in range(4)], axis=1)

    reg = lambda M: np.stack([M[4 * g + v, j] for v in range(4)], axis=1)          # a matrix in the C/D layout
    s, wr = reg(sig), reg(w)
    a = np.stack([acl[j, 4 * g + v] for v in range(4)], axis=1)                   # the one staged operand
    U = np.zeros_like(s)
    for v in range(4):
        U = mfma(s[:, v], a[:, v], U)
    out = wr
    for v in range(4):
        out = mfma(a[:, v], U[:, v], out)
    M = np.zeros((16, 16), dtype=sig.dtype)
    for v in range(4):
        M[4 * g + v, j] = out[:, v]
    return M
