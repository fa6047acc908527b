"""The gradient of the tracked closed-loop cost (quattro_track_gradient_f32, ops.track_gradient, autograd.tracking_cost): the cases,
the fp64 reference, the error measures, the fp32 restatement, the mutants and the bounds.  A plain helper module (like
tests/grad_cases.py, on which it builds), used by tests/test_track_gradient_cpu.py and tests/test_track_gradient_gpu.py.

Case: the nominal (x_nom, u_nom) is grad_cases.nominal; the gains K are the fp64 oracle's Riccati gains about it
(oracle.ilqr.riccati_sweep_batched over linearize_analytic's blocks), both rounded to fp32.  The start is x_nom[0] moved by
START_SPREAD x param_cases' spread x N(0, 1) (seeded), so that the tracked run differs from the nominal (case() asserts that
x - x_nom is non-zero at every step after the first).  The run is oracle.linearize.closed_loop_rollout_batched with k = 0, alpha = 1
under the PLANT's spec (its own phys row and integrator where the case has them), cut after S = n_steps steps and rounded to fp32:
what the device is given.

Reference (fp64, about that run): grad_cases.adjoint over the composed blocks
    A_cl = A + B K,   l_x_cl = l_x + K^T l_u,   B and l_u unchanged,   lambda_S = terminal ? Lf_x(x_S) : 0
which is lambda_t = l_x + A^T lambda_{t+1} + K^T g_t with g_t = l_u + B^T lambda_{t+1}; then
    grad_u_nom_t = g_t,   grad_K_t = g_t (x_t - x_nom_t)^T,   grad_x_nom_t = -K_t^T g_t,   rows t >= S zero.

Error measures (the largest over the batch and the entries):
    costate, grad_x0, grad_u_nom : grad_cases.errors' measures with lambda the closed-loop costate:
                                   G_{t,a} = |l_u|_{t,a} + sum_i |B_t|_{ia} Lambda_i is the scale of g_{t,a}, Lambda_i = max_t |lambda_{t,i}|
    grad_K[t][a][j]              : |d| / (G_{t,a} |x_{t,j} - x_nom_{t,j}|)        the sizes of the two factors that form the entry
    grad_x_nom[t][j]             : |d| / sum_a |K_t[a][j]| G_{t,a}                the sizes of the terms that are added
Neither is relative to the array's largest entry: the tracking error of a well-tracked state is orders of magnitude below that of a
badly tracked one, and a per-array scale would hide every entry of the former.  An entry whose denominator is exactly zero must be
exactly zero (its error is then 0, otherwise inf) and is left out of the ratio; rows t >= S must be exactly +0.0.
"""
import numpy as np

import grad_cases as gc
import param_cases as pc
import ref_cases as rc
import weight_cases as wc
from oracle import ilqr as o_ilqr
from oracle import linearize as o_lin

f32 = gc.f32
START_SPREAD = 0.1
START_SEED = 41
MUTANTS = ("feedback dropped from the costate", "K^T l_u dropped", "B K dropped", "K of step t + 1",
           "x - x_nom of step t + 1 in dJ/dK", "x for x - x_nom in dJ/dK", "sign of dJ/dx_nom",
           "terminal term kept with the flag off")
KEYS = ("costate", "grad_x0", "grad_u_nom", "grad_K", "grad_x_nom")


# ---------------------------------------------------------------------------------------------------------------- reference
def compose(d, K, terminal=True, mutant=None):
    """Blocks d over S steps and gains K (B, S, m, n) -> the blocks grad_cases.adjoint runs the closed-loop recursion on."""
    S = d["B"].shape[1]
    Kc = K[:, [min(t + 1, S - 1) for t in range(S)]] if mutant == "K of step t + 1" else K
    A = d["A"] if mutant in ("B K dropped", "feedback dropped from the costate") else d["A"] + np.einsum("btia,btaj->btij", d["B"], Kc)
    lx = d["lx"] if mutant in ("K^T l_u dropped", "feedback dropped from the costate") else d["lx"] + np.einsum("btaj,bta->btj", Kc, d["lu"])
    keep = terminal or mutant == "terminal term kept with the flag off"
    return dict(A=A, B=d["B"], lx=lx, lu=d["lu"], VxN=d["VxN"] if keep else np.zeros_like(d["VxN"]))


def reference(d, x, x_nom, K, N, terminal=True, dtype=np.float64, mutant=None):
    """d: the fp64 blocks about the realised x (B, S+1, n), u over S steps; x_nom (B, N+1, n), K (B, N, m, n) as the run was given.
    -> dict of KEYS in the shapes of the entry's outputs.  dtype float32: the restatement (the composed blocks rounded to fp32, the
    recursion and the products in fp32).  mutant: one of MUTANTS."""
    Bt, S, n, m = d["B"].shape
    Ks = np.asarray(K, dtype=np.float64)[:, :S]
    cb = compose(d, Ks, terminal, mutant)
    adj = gc.adjoint(cb, dtype)
    g = adj["grad_u"]
    xs, xn, Kd = (np.asarray(v).astype(dtype) for v in (x[:, :S], x_nom[:, :S], Ks))
    e = xs - xn
    if mutant == "x - x_nom of step t + 1 in dJ/dK":
        e = (np.asarray(x).astype(dtype) - np.asarray(x_nom[:, :S + 1]).astype(dtype))[:, [min(t + 1, S) for t in range(S)]]
    if mutant == "x for x - x_nom in dJ/dK":
        e = xs
    Kx = Kd[:, [min(t + 1, S - 1) for t in range(S)]] if mutant == "K of step t + 1" else Kd
    gK = (g[:, :, :, None] * e[:, :, None, :]).astype(dtype)
    gxn = -np.einsum("btaj,bta->btj", Kx, g).astype(dtype)
    if mutant == "sign of dJ/dx_nom":
        gxn = -gxn
    out = dict(costate=adj["costate"], grad_x0=adj["grad_x0"], grad_u_nom=np.zeros((Bt, N, m), dtype=dtype),
               grad_K=np.zeros((Bt, N, m, n), dtype=dtype), grad_x_nom=np.zeros((Bt, N + 1, n), dtype=dtype))
    out["grad_u_nom"][:, :S], out["grad_K"][:, :S], out["grad_x_nom"][:, :S] = g, gK, gxn
    return out


def _ratio(diff, den, got):
    zero = den == 0.0
    e = np.abs(diff) / np.where(zero, 1.0, den)
    e = np.where(zero, np.where(got == 0.0, 0.0, np.inf), e)
    return float(np.max(e))


def errors(got, ref, d, x, x_nom, K):
    """got: dict with any of KEYS (arrays in the entry's shapes); ref: reference() in fp64; d, x, x_nom, K: what ref was made from.
    -> dict of the measures of the module docstring.  Rows t >= S of the full-shape outputs must be exactly +0.0."""
    Bt, S, n, m = d["B"].shape
    lam = np.asarray(ref["costate"], dtype=np.float64)
    Lam = np.max(np.abs(lam), axis=1)
    G = np.abs(d["lu"]) + np.einsum("btia,bi->bta", np.abs(d["B"]), Lam)                  # (B, S, m)
    head = {k: np.asarray(got[k], dtype=np.float64) for k in ("costate", "grad_x0") if got.get(k) is not None}
    head["grad_u"] = np.asarray(got["grad_u_nom"], dtype=np.float64)[:, :S]
    out = gc.errors(head, dict(grad_u=ref["grad_u_nom"][:, :S], costate=lam), d)
    out["grad_u_nom"] = out.pop("grad_u")
    e = np.asarray(x, dtype=np.float64)[:, :S] - np.asarray(x_nom, dtype=np.float64)[:, :S]
    Ks = np.abs(np.asarray(K, dtype=np.float64)[:, :S])
    dens = dict(grad_K=G[:, :, :, None] * np.abs(e)[:, :, None, :], grad_x_nom=np.einsum("btaj,bta->btj", Ks, G))
    for key in ("grad_u_nom", "grad_K", "grad_x_nom"):
        if got.get(key) is None:
            continue
        g = np.asarray(got[key], dtype=np.float64)
        assert g.shape == ref[key].shape, (key, g.shape, ref[key].shape)
        tail = g[:, S:]
        if tail.size and not (np.all(tail == 0.0) and not np.any(np.signbit(tail))):
            out[key] = np.inf
        elif key in dens:
            out[key] = _ratio(g[:, :S] - ref[key][:, :S], dens[key], g[:, :S])
    return out


def worst(errs):
    return max(errs.values())


# ---------------------------------------------------------------------------------------------------------------- built-in cases
SPREAD = {"quadrotor": pc.QUAD_SPREAD, "cartpole": pc.CART_SPREAD}
# (N, n_steps): 7 with 7, 5 and 1 hit the remainders of the kernel's block of 3 steps and the cart-pole's three steps per pass
STEPS = ((7, 7), (7, 5), (7, 1), (26, 26))
B_CASE = 5                 # a last wave with idle groups (four trajectories per wave)


def case(model, set_name, integ, N, S=None, B=B_CASE, terminal=True, plant_integ=None, hetero=(), R=None):
    """-> dict(x, u the realised run (B, S+1, n), (B, S, m); x_nom, u_nom, K as the run was given; x0; d the fp64 blocks about the
    run; ref the fp64 reference; specs the plant's spec per trajectory; w, phys, rows the per-trajectory rows or None; win).
    plant_integ: the plant's integrator (None: the controller's).  hetero: any of "weights", "phys" -- rows of weight_cases /
    grad_cases.phys_rows per trajectory (the skew set only).  R: rows of ref_cases.skew_rows, step t against row min(t, R - 1)."""
    S = N if S is None else S
    x_nom, u_nom = gc.nominal(model, set_name, integ, N, B)
    spec = pc.spec(model, set_name, integ)
    _, K = o_ilqr.riccati_sweep_batched(o_lin.linearize_analytic(spec, x_nom, u_nom))
    K = f32(K)
    rng = np.random.default_rng(START_SEED)
    x0 = f32(x_nom[:, 0] + START_SPREAD * SPREAD[model] * rng.standard_normal((pc.B_FULL[model], pc.DIMS[model][0]))[:B])
    w = wc.weight_rows(model, B) if "weights" in hetero else None
    phys = gc.phys_rows(model, B) if "phys" in hetero else None
    pi = integ if plant_integ is None else plant_integ
    if w is not None or phys is not None:
        assert set_name == "skew"
        specs = [pc.spec_from(model, gc.params_with(model, None if w is None else w[b], None if phys is None else phys[b]), pi)
                 for b in range(B)]
    else:
        specs = [pc.spec(model, set_name, pi)] * B
    runs = [o_lin.closed_loop_rollout_batched(sp, x0[b:b + 1], x_nom[b:b + 1], u_nom[b:b + 1], np.zeros_like(u_nom[b:b + 1]),
                                              K[b:b + 1], 1.0) for b, sp in enumerate(specs)]
    x = f32(np.concatenate([r[0] for r in runs]))[:, :S + 1]
    u = f32(np.concatenate([r[1] for r in runs]))[:, :S]
    assert np.all(np.max(np.abs(x[:, 1:] - x_nom[:, 1:S + 1]), axis=2) > 0.0) and np.all(np.abs(x[:, 0] - x_nom[:, 0]).max(axis=1) > 0)
    rows = rc.skew_rows(model, B, R) if R is not None else None
    win = None if rows is None else rc.window(rows.astype(np.float64), S)
    d = gc.blocks_per_trajectory(specs, x, u, win)
    return dict(x=x, u=u, x_nom=x_nom, u_nom=u_nom, K=K, x0=x0, d=d, ref=reference(d, x, x_nom, K, N, terminal), specs=specs, w=w,
                phys=phys, rows=rows, win=win, N=N, S=S, terminal=terminal)


def case_errors(c, got):
    return errors(got, c["ref"], c["d"], c["x"], c["x_nom"], c["K"])


def mutant_errors(c, name):
    """How far mutant `name` of the reference stands from the reference, in case c (a terminal=False case for the terminal mutant)."""
    return case_errors(c, reference(c["d"], c["x"], c["x_nom"], c["K"], c["N"], c["terminal"], mutant=name))


# The cases the restatement is measured on and the GPU parity test runs: both models, both integrators, STEPS, terminal on and off,
# with and without rows, and a plant with the other integrator.
def parity_cases(model):
    out = []
    for set_name in gc.SETS[model]:
        for integ in gc.INTEGRATORS:
            for N, S in STEPS:
                out.append(dict(set_name=set_name, integ=integ, N=N, S=S))
    other = {"euler": "rk4", "rk4": "euler"}
    for integ in gc.INTEGRATORS:
        out.append(dict(set_name="skew", integ=integ, N=7, S=5, terminal=False))
        out.append(dict(set_name="skew", integ=integ, N=7, S=7, terminal=False, hetero=("weights", "phys"), R=4))
        out.append(dict(set_name="skew", integ=integ, N=7, S=5, hetero=("weights", "phys"), R=4))
        out.append(dict(set_name="skew", integ=integ, N=7, S=7, R=3))
        out.append(dict(set_name="skew", integ=integ, N=7, S=7, plant_integ=other[integ], hetero=("phys",)))
    return out


def case_id(kw):
    return "-".join(str(v) if not isinstance(v, tuple) else "+".join(v) for v in kw.values())


# ---------------------------------------------------------------------------------------------------------------- bounds
# E: the distance of the fp32 restatement (the composed blocks rounded to fp32, the recursion and the three products in fp32) from
# fp64 under the measures above, the worst over parity_cases, measured on the CPU (tests/test_track_gradient_cpu.py holds the
# restatement to these figures).  The GPU tests assert the larger of 4 x E and the fp32 floor of the project's rollout comparisons
# (param_cases.BOUNDS["sim_x"] = 2e-6): the device forms its own fp32 tangents, which the restatement does not model.
E = {"quadrotor": 6.2e-7, "cartpole": 4.0e-7}
FLOOR = pc.BOUNDS["sim_x"]


def gpu_bound(model):
    return max(4.0 * E[model], FLOOR)


# Every mutant stands >= 10 x above gpu_bound in the case named here (model -> mutant -> keywords of case()); measured values in
# tests/test_track_gradient_cpu.py's docstring.
_T = dict(set_name="skew", integ="rk4", N=7, S=7)
TEETH = {model: {name: dict(_T, terminal=False) if name.startswith("terminal") else dict(_T) for name in MUTANTS}
         for model in pc.MODELS}

# ---------------------------------------------------------------------------------------------------------------- finite differences
FD_H = 1e-6            # (the quadrotor's barrier makes the truncation error of h = 1e-5 visible: 5e-5 relative, falling as h^2)
FD_DIRECTIONS = 3
FD_B = 3
# Measured (skew sets, N = 7, both models and integrators, a plant with the other integrator included): the worst relative difference
# between the fp64 reference (with pgrad_cases.reference on the closed-loop costate for the plant's phys) and central differences
# (h = 1e-6) of the oracle's closed-loop cost along seeded directions in (x0, u_nom, x_nom, K, plant phys); asserted: 10 x that.
FD_WORST = {"quadrotor": 5.4e-7, "cartpole": 1.6e-9}
FD_BOUND = {model: 10.0 * v for model, v in FD_WORST.items()}


def closed_loop_cost(model, integ, x0, x_nom, u_nom, K, phys):
    """fp64 cost of the oracle's closed-loop run (k = 0, alpha = 1) per trajectory, the plant under phys (B, NP)."""
    out = np.zeros(x0.shape[0])
    for b in range(x0.shape[0]):
        sp = pc.spec_from(model, gc.params_with(model, None, phys[b]), integ)
        out[b] = o_lin.closed_loop_rollout_batched(sp, x0[b:b + 1], x_nom[b:b + 1], u_nom[b:b + 1], np.zeros_like(u_nom[b:b + 1]),
                                                   K[b:b + 1], 1.0)[2][0]
    return out


def fd_errors(model, integ, plant_integ, N=7, seed=5):
    """Central differences of closed_loop_cost along random directions against the fp64 reference about the fp64 run."""
    import pgrad_cases as pgc
    c = case(model, "skew", integ, N, B=FD_B, plant_integ=plant_integ, hetero=("phys",))
    phys = c["phys"].astype(np.float64)
    J = lambda x0, xn, un, K, ph: closed_loop_cost(model, plant_integ, x0, xn, un, K, ph)
    runs = [o_lin.closed_loop_rollout_batched(sp, c["x0"][b:b + 1], c["x_nom"][b:b + 1], c["u_nom"][b:b + 1],
                                              np.zeros_like(c["u_nom"][b:b + 1]), c["K"][b:b + 1], 1.0) for b, sp in enumerate(c["specs"])]
    x, u = np.concatenate([r[0] for r in runs]), np.concatenate([r[1] for r in runs])
    d = gc.blocks_per_trajectory(c["specs"], x, u)
    ref = reference(d, x, c["x_nom"], c["K"], N)
    gphys = pgc.reference(model, c["specs"][0], x, u, ref["costate"], phys=phys)["grad_phys"]
    rng = np.random.default_rng(seed)
    out = 0.0
    for _ in range(FD_DIRECTIONS):
        dx0, dxn, dun = rng.standard_normal(c["x0"].shape), rng.standard_normal(c["x_nom"].shape), rng.standard_normal(c["u_nom"].shape)
        dK, dph = rng.standard_normal(c["K"].shape) * np.abs(c["K"]), rng.standard_normal(phys.shape) * phys
        h = FD_H
        Jp = J(c["x0"] + h * dx0, c["x_nom"] + h * dxn, c["u_nom"] + h * dun, c["K"] + h * dK, phys + h * dph)
        Jm = J(c["x0"] - h * dx0, c["x_nom"] - h * dxn, c["u_nom"] - h * dun, c["K"] - h * dK, phys - h * dph)
        fd = (Jp - Jm) / (2.0 * h)
        an = (np.sum(ref["grad_x0"] * dx0, axis=1) + np.sum(ref["grad_x_nom"] * dxn, axis=(1, 2)) + np.sum(ref["grad_u_nom"] * dun, axis=(1, 2))
              + np.sum(ref["grad_K"] * dK, axis=(1, 2, 3)) + np.sum(gphys * dph, axis=1))
        out = max(out, float(np.max(np.abs(fd - an) / np.abs(an))))
    return out


# ---------------------------------------------------------------------------------------------------------------- user models
USER_POINTS = ((1, 1), (12, 4), (16, 8))       # 8-, 16- and 32-lane groups
USER_STEPS = ((9, 9), (9, 4))
USER_B = 3
USER_E = 1.7e-7                # the restatement's distance on USER_POINTS x USER_STEPS, both integrators (same measures)


def user_case(n, m, integ, N, S, B=USER_B, terminal=True):
    """The user grid's convex problem at (n, m): nominal = the fp64 rollout of its inputs, gains = its fp64 sweep, both rounded to
    fp32; the start moved by START_SPREAD N(0, 1); the run is Problem.closed_loop with k = 0, alpha = 1.  -> case()'s dict."""
    import user_grid_cases as g
    pr = g.Problem(n, m, g.params(n, m, "convex"), integ)
    x0n, u_nom = g.inputs(n, m, "convex", N, B)
    x_nom = f32(pr.rollout(x0n, u_nom)[0])
    _, K = g.sweep(pr.records(x_nom, u_nom))
    K = f32(K)
    x0 = f32(x_nom[:, 0] + START_SPREAD * np.random.default_rng(START_SEED).standard_normal((B, n)))
    xs, us, _ = pr.closed_loop(x0, x_nom, u_nom, np.zeros_like(u_nom), K, 1.0)
    x, u = f32(xs)[:, :S + 1], f32(us)[:, :S]
    assert np.all(np.max(np.abs(x - x_nom[:, :S + 1]), axis=2) > 0.0)
    rec = pr.records(x, u)
    d = {key: rec[key] for key in ("A", "B", "lx", "lu", "VxN")}
    return dict(x=x, u=u, x_nom=x_nom, u_nom=u_nom, K=K, x0=x0, d=d, ref=reference(d, x, x_nom, K, N, terminal), N=N, S=S,
                terminal=terminal)
