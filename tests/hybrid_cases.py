"""One hybrid backward pass (QuattroILQR.backward with a predictor: the last P rows of the gain stack from the Riccati sweep, the rows
below from the predictor) and the line search that follows it, restated in fp64: the cases, the reference, the measures, the mutants
and the bounds.  A plain helper module (like tests/policy_cases.py and tests/task_loss_cases.py), CPU only, NumPy and oracle/ only;
used by tests/test_hybrid_cases_cpu.py and tests/test_hybrid_parity_gpu.py.

Cases (B = 5 each; L = N + 1 + P + T tokens).  `branch` is the code path of QuattroILQR.backward the case takes:
    in_place    fused tail sweep into rows N - P .. N - 1 of the full stacks, the predictor reads its prompt from those rows
    segment     a sweep into K_seg / k_seg, predict_gains with a packed prompt, torch.where for the swept rows that land in the horizon
    batch_only  the same sweep, then a duck-typed predict_batch with _pack_prompt / _unpack_prediction in torch
    name           model, integrator   N   P   T   branch
    cp_L21         cart-pole, Euler    10  2   8   in_place; one-wave predictor
    cp_L61         cart-pole, RK4      30  5   25  in_place; the prompt straddles token 32
    quad_L101      quadrotor, Euler    50  1   49  in_place; the shipped shape (ff 256, 2 layers)
    quad_L25       quadrotor, RK4      12  3   9   segment (the RK4 quadrotor sweeps through records: ops.model_fuses_sweep is False, so
                                                   T + S = N does not make it in_place); a multi-row prompt with m = 4
    quad_long      quadrotor, Euler    12  3   12  segment, T + S > N with T = N: every row of the stack is predicted, the sweep feeds
                                                   the prompt only
    quad_long_T10  quadrotor, Euler    12  3   10  segment, T + S > N with T < N: the first N - T = 2 of the 3 swept rows land at rows 10, 11
    user_7x2       user_grid_cases.model(7, 2, "convex", "rk4")   9  2  7   segment; unfused sweep (records, tile rowpad), fused predictor, c = 16
    cp_batch_only  as cp_L21, the predictor wrapped so that it shows only predict_batch, prompt_len, target_len: batch_only
    cp_fp32        cart-pole, Euler    10  2   8   in_place; d_model 64 / 8 heads: the layer-wise fp32 predictor
Every case has a non-zero state_offset, hands solve() x_ref = model.x_ref + delta with delta != 0 (the predictor's x_ref; the cost keeps
the model's), and starts from controls hover / zero / 0.5 plus seeded noise.  Trajectory 0 starts where one iteration cannot gain 1e-3,
so that it stops after the first: at the goal (the user model, which has no equilibrium there: at a seeded start) under the controls
pure iLQR settles on from hover / zero / 0.5 (_settled_controls; the cart-pole's stay zero: the equilibrium control); trajectory 1 of
the built-in models starts close to that, the others spread out and go on.

Predictor: predictor_cases.random_model(sharp=True) -- random x_mean / x_std -- with u_mean = the mean of the oracle's Riccati rows
about the first nominal (data-set layout, over batch and steps) and u_std = 0.1 x their std + 1e-6, so that predicted gains stay near
usable ones (tests/task_loss_cases.py does the same).

Reference: `compose` restates quattro_ilqr_tf.py:498-518 as oracle.ilqr.optimize does, from oracle.linearize.linearize_analytic,
oracle.ilqr.riccati_sweep_batched (the last S = P rows of the full sweep are the tail; the user model: user_grid_cases' records and
sweep), oracle.ilqr.pack_prompt, the predictor oracle on operand-rounded weights, oracle.ilqr.unpack_prediction and concat[:N].  With
`tail` the prompt is built from those rows instead of the oracle's own: a check of the predicted rows is thereby separated from the
sweep's error.

Measures: the predicted rows regrouped into tokens (B, Tn, c): predictor_cases.quantities (fro, worst token, worst channel); the swept
rows: relative Frobenius error per trajectory, the worst over the batch, for K and for k.

Bounds, none fitted to the device:
    predicted rows   2 x noise, noise measured as predictor_cases.noise does -- the oracle with both operands of every matrix product
                     rounded against the plain oracle, both on rounded weights -- on this case's own inputs (the four draws of
                     `nominals`, each with its neighbours: predictor_noise), per operand type; cp_fp32: 2e-5
                     (test_predictor_shapes_beyond_the_fused_kernel_run_layer_wise_in_fp32)
    swept rows       max(5e-6, 4 E): 5e-6 is test_short_and_odd_horizons_against_the_oracle's, E the distance of the float32 sweep
                     (NumPy float32 on float32 blocks) from the fp64 one on the tail rows, per nominal, quantity and trajectory
                     (sweep_noise)
    line search      max(1e-5, 4 E_cl): E_cl the distance from fp64 of the closed-loop rollout with fp32 storage (x and u rounded at every
                     step; the user model: its float32 emulation) under the oracle's stack at the accepted step size
"""
import functools

import numpy as np

import predictor_cases as prc
import user_grid_cases as ug
from oracle import ilqr as o_ilqr
from oracle import linearize as o_lin
from oracle import models as o_models
from oracle import transformer as o_tf

B = 5
ALPHAS = o_ilqr.LINE_SEARCH_ALPHAS
TOL = 1e-3                       # QuattroILQR's default stop tolerance
FACTOR = prc.FACTOR
QUANTITIES = prc.QUANTITIES
FP32_PREDICTOR_BOUND = 2e-5
SWEEP_START, LS_START = 5e-6, 1e-5
NEIGHBOURS, NEIGHBOUR_STEP = 4, 1e-3   # inputs per draw behind the predictor noise (predictor_noise): the draw and three neighbours of it
SWEEP_DRAWS, LIN_ULPS = 4, 2.0   # restatements of the float32 linearisation behind E, and the error per block entry they carry (sweep_noise)
TEETH = 3.0                      # every mutant moves an asserted measure by at least this multiple of the measure's bound
DECIDABLE_MARGIN = 10.0          # a candidate closer to J than this multiple of the line-search bound x |J| makes the choice undecidable
MIN_DECIDABLE = 4                # of the B = 5 trajectories of a case
FD_TOL = 5e-4                    # the oracle's finite differences against exact derivatives, as the suite uses it

# name -> model, integrator, N, P, T, ff, layers, d_model, heads, branch, seed
SHAPES = {
    "cp_L21":        dict(model="cartpole", integ="euler", N=10, P=2, T=8, ff=64, layers=1, branch="in_place", seed=0),
    "cp_L61":        dict(model="cartpole", integ="rk4", N=30, P=5, T=25, ff=192, layers=2, branch="in_place", seed=0),
    "quad_L101":     dict(model="quadrotor", integ="euler", N=50, P=1, T=49, ff=256, layers=2, branch="in_place", seed=0),
    "quad_L25":      dict(model="quadrotor", integ="rk4", N=12, P=3, T=9, ff=128, layers=1, branch="segment", seed=0),
    "quad_long":     dict(model="quadrotor", integ="euler", N=12, P=3, T=12, ff=128, layers=1, branch="segment", seed=0),
    "quad_long_T10": dict(model="quadrotor", integ="euler", N=12, P=3, T=10, ff=128, layers=1, branch="segment", seed=0),
    "user_7x2":      dict(model="user", integ="rk4", N=9, P=2, T=7, ff=64, layers=1, branch="segment", seed=0),
    "cp_batch_only": dict(model="cartpole", integ="euler", N=10, P=2, T=8, ff=64, layers=1, branch="batch_only", seed=0, like="cp_L21"),
    "cp_fp32":       dict(model="cartpole", integ="euler", N=10, P=2, T=8, ff=128, layers=2, d_model=64, nhead=8, branch="in_place",
                          seed=0),
}
NAMES = tuple(SHAPES)
BRANCHES = ("in_place", "segment", "batch_only")
USER_NM = (7, 2)
NEAR = {"cartpole": 0.02, "quadrotor": 0.005}    # trajectory 1 = trajectory 0 moved by this fraction of the other trajectories' spread


def precisions(name):
    """The operand types a case runs in; "fp32": the layer-wise fp32 predictor, whose weights are not rounded."""
    return ("fp32",) if name == "cp_fp32" else prc.PRECISIONS


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- plants
class BuiltinPlant:
    """The built-in cart-pole / quadrotor at their defaults: oracle.models' spec behind the interface `compose` needs."""

    def __init__(self, model, integ):
        make = o_models.cartpole_spec if model == "cartpole" else o_models.quadrotor_spec
        self.spec = make(integrator=o_models.INTEGRATOR_RK4 if integ == "rk4" else o_models.INTEGRATOR_EULER)
        self.model, self.integ, self.n, self.m, self.x_ref = model, integ, self.spec.n, self.spec.m, self.spec.x_ref
        self.u_base = f32(np.full(self.m, self.spec.phys["mass"] * self.spec.phys["gravity"] / 4.0 if model == "quadrotor" else 0.0))
        self.x_spread = 0.2 if model == "cartpole" else 0.2 * np.array([1, 1, 1, 1, 1, 1, .5, .5, 1, 1, 1, 1.0])
        self.f, self.L, self.Lf = self.spec.f, self.spec.L, self.spec.Lf

    def device_model(self):
        from quattro_ilqr_amd import models
        return models.model_by_name(self.model, integrator=self.integ)

    def rollout(self, x0, u):
        return o_lin.rollout_batched(self.spec, x0, u)

    def blocks(self, x, u):
        return o_lin.linearize_analytic(self.spec, x, u)

    def sweep(self, d, dtype=np.float64):
        if dtype != np.float64:
            d = {key: np.asarray(v).astype(dtype) for key, v in d.items()}
        return o_ilqr.riccati_sweep_batched(d, dtype=dtype)

    def closed_loop(self, x0, x, u, k, K, alpha, fp32=False):
        if not fp32:
            return o_lin.closed_loop_rollout_batched(self.spec, x0, x, u, k, K, alpha)
        sp, N = self.spec, u.shape[1]
        nx, nu, J = np.zeros_like(x), np.zeros_like(u), np.zeros(u.shape[0])
        nx[:, 0] = x0
        for t in range(N):
            du = f32(k[:, t] + np.einsum("bij,bj->bi", K[:, t], f32(nx[:, t] - x[:, t])))
            nu[:, t] = f32(u[:, t] + f32(alpha * du))
            J = J + f32(o_lin.stage_cost(sp, nx[:, t], nu[:, t]))
            nx[:, t + 1] = f32(o_lin.step(sp, nx[:, t], nu[:, t]))
        return nx, nu, J + f32(o_lin.terminal_cost(sp, nx[:, N]))


class UserPlant:
    """user_grid_cases' family at (7, 2), variant convex."""

    def __init__(self, integ):
        n, m = USER_NM
        self.model, self.integ, self.n, self.m = "user", integ, n, m
        self.params = ug.params(n, m, "convex")
        self.pr = ug.Problem(n, m, self.params, integ)
        self.pr32 = ug.Problem(n, m, self.params, integ, np.float32)
        self.x_ref = self.params["x_ref"]
        self.u_base = np.full(m, 0.5)
        self.x_spread = 0.3
        self.f, self.L, self.Lf = self.pr.f1, self.pr.L, self.pr.Lf

    def device_model(self):
        return ug.model(self.n, self.m, "convex", self.integ)

    def rollout(self, x0, u):
        return self.pr.rollout(x0, u)

    def blocks(self, x, u):
        return self.pr.records(x, u)

    def sweep(self, d, dtype=np.float64):
        return ug.sweep(d, dtype=dtype, inverse="linalg" if dtype == np.float64 else "pivot")

    def closed_loop(self, x0, x, u, k, K, alpha, fp32=False):
        xs, us, J = (self.pr32 if fp32 else self.pr).closed_loop(x0, x, u, k, K, alpha)
        return np.asarray(xs, dtype=np.float64), np.asarray(us, dtype=np.float64), np.asarray(J, dtype=np.float64)


def _settled_controls(plant, x0, u, iters=40):
    """Pure iLQR in fp64 (exact derivatives) from (x0, u) for one trajectory, up to the first step that gains less than TOL / 4: the
    controls trajectory 0 starts from.  Deliberately not run to convergence: at the optimum the swept k is zero, and what fp32 leaves
    of it has no digits to compare."""
    x0, u = x0[None], u[None]
    for _ in range(iters):
        x, J = plant.rollout(x0, u)
        k, K = plant.sweep(plant.blocks(x, u))
        for a in ALPHAS:
            _, nu, nJ = plant.closed_loop(x0, x, u, k, K, a)
            if nJ[0] <= J[0]:
                break
        else:
            break
        if abs(J[0] - nJ[0]) < 0.25 * TOL:
            break
        u = nu
    return u[0]


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    pass


def tokens(k, K):
    """(B, R, m), (B, R, m, n) -> (B, R, m (1 + n)): the layout the prediction is unpacked with (and the data set's): [k_i | K_i] per row i."""
    return np.concatenate([k[..., None], K], axis=-1).reshape(k.shape[0], k.shape[1], -1)


def pack_prompt(k, K):
    """oracle.ilqr.pack_prompt per trajectory: [k | K.flat]."""
    return np.stack([o_ilqr.pack_prompt(list(k[b]), list(K[b])) for b in range(k.shape[0])])


@functools.lru_cache(maxsize=None)
def case(name):
    sh = SHAPES[name]
    if "like" in sh:
        base = case(sh["like"])
        cs = Case()
        cs.__dict__.update(base.__dict__)
        cs.name, cs.branch = name, sh["branch"]
        return cs
    cs = Case()
    cs.name, cs.branch = name, sh["branch"]
    plant = UserPlant(sh["integ"]) if sh["model"] == "user" else BuiltinPlant(sh["model"], sh["integ"])
    cs.plant, cs.n, cs.m = plant, plant.n, plant.m
    cs.N, cs.P, cs.T = sh["N"], sh["P"], sh["T"]
    cs.S, cs.Tn, cs.c = cs.P, min(cs.T, cs.N), plant.m * (1 + plant.n)
    cs.keep = min(cs.S, cs.N - cs.Tn)                                      # swept rows that land inside the horizon, at rows Tn .. Tn + keep - 1
    assert cs.T + cs.S >= cs.N
    cs.d_model, cs.nhead = sh.get("d_model", prc.D), sh.get("nhead", prc.NHEAD)
    rng = np.random.default_rng([NAMES.index(name), sh["seed"]])
    n, m, N = cs.n, cs.m, cs.N
    cs.offset = f32(rng.choice([-1.0, 1.0], n) * rng.uniform(0.75, 1.5, n))
    cs.delta = f32(rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n))
    cs.x_ref_arg = f32(plant.x_ref + cs.delta)

    def start(scale):
        x0 = f32(plant.x_ref + scale * plant.x_spread * rng.standard_normal((B, n)))
        u = f32(plant.u_base + scale * 0.3 * rng.standard_normal((B, N, m)))
        if plant.model != "user":
            x0[0] = plant.x_ref                                            # (the user model has no equilibrium at its goal)
        u[0] = f32(_settled_controls(plant, x0[0], np.tile(plant.u_base, (N, 1))))
        if plant.model != "user":                                          # (its cost is too flat there for a decidable line search)
            x0[1] = f32(x0[0] + NEAR[plant.model] * plant.x_spread * rng.standard_normal(n))
            u[1] = f32(u[0] + NEAR[plant.model] * 0.3 * rng.standard_normal((N, m)))
        return x0, u

    cs.x0, cs.u = start(1.0)
    cs.prev_x0, cs.prev_u = start(0.7)                                    # what the solver object solves before: stale rows would show
    cs.prev_x_ref_arg = f32(cs.x_ref_arg + 0.25)
    cs.x = f32(plant.rollout(cs.x0, cs.u)[0])
    k, K = plant.sweep(plant.blocks(cs.x, cs.u))
    rows = tokens(k, K)
    w, norm, hp = prc.random_model(n, cs.c, N + 1, cs.P, cs.T, sh["ff"], sh["layers"], 900 + NAMES.index(name), sharp=True,
                                   d_model=cs.d_model, nhead=cs.nhead)
    norm = dict(norm, u_mean=f32(rows.mean(axis=(0, 1))), u_std=f32(0.1 * rows.std(axis=(0, 1)) + 1e-6))
    cs.w, cs.norm, cs.hp = w, norm, hp
    return cs


@functools.lru_cache(maxsize=None)
def weights(name, precision):
    """The weights both sides of a comparison start from: matrices rounded to the operand type ("fp32": as they are)."""
    cs = case(name)
    if precision == "fp32":
        return {key: np.asarray(v, dtype=np.float64) for key, v in cs.w.items()}
    return prc.round_weights(cs.w, precision)


# ---------------------------------------------------------------------------------------------------------------- the reference
MUTANTS = (
    "x_ref not subtracted",
    "offset with the opposite sign",
    "model.x_ref in place of the argument",
    "prompt in the data-set layout",
    "prompt from rows 0..P-1 of the stack",
    "prompt rows in reverse order",
    "prompt from the previous solve's tail",
    "prediction unpacked as [k | K.flat]",
    "predicted rows shifted by one step",
    "the last N - T swept rows instead of the first",
    "tail rows overwritten by the prediction",
    "a stopped trajectory's rows rewritten",
)
LAYOUT_MUTANTS = ("prompt in the data-set layout", "prediction unpacked as [k | K.flat]")


def predict(cs, w, x, x_err, prompt, operand=None, kernel_norm=None):
    """The predictor oracle, de-normalised (B, T, c).  kernel_norm "shifted": the states are normalised in fp32 from the raw x with the
    fp32 mean x_mean + x_ref - offset, as the kernel does (TransformerILQR.shifted_mean); "torch": x_err is formed in fp32 first, as the
    duck-typed branch does; None: from the fp64 x_err handed over (the mutants)."""
    nm = cs.norm
    s32 = np.float32
    if kernel_norm == "shifted":
        mean = (nm["x_mean"] + (cs.x_ref_arg - cs.offset)).astype(s32)
        xn = (x.astype(s32) - mean) / nm["x_std"].astype(s32)
    elif kernel_norm == "torch":
        xe = (x.astype(s32) - cs.x_ref_arg.astype(s32)) + cs.offset.astype(s32)
        xn = (xe - nm["x_mean"].astype(s32)) / nm["x_std"].astype(s32)
    else:
        xn = ((x_err - nm["x_mean"]) / nm["x_std"]).astype(s32)
    pn = ((prompt - nm["u_mean"]) / nm["u_std"]).astype(s32)
    with prc._one_thread(limits=1):
        y = o_tf.forward(w, xn, pn, cs.nhead, operand=operand)
    return y * nm["u_std"] + nm["u_mean"]


def compose(cs, x, u, precision, tail=None, mutant=None, stale=None, operand=None, kernel_norm=None):
    """One hybrid backward pass in fp64 about the nominal (x, u) -> dict(x_err, prompt, pred, k, K, k_seg, K_seg, k_full, K_full):
    k (B, N, m), K (B, N, m, n) the gain stack, *_seg the swept tail, *_full the oracle's sweep over the whole horizon.
    tail: (k_seg, K_seg) to build the prompt and the swept rows from instead of the oracle's own.  stale: the tail of the previous
    solve (mutant "prompt from the previous solve's tail").  mutant: one of MUTANTS[:-1]."""
    assert mutant is None or mutant in MUTANTS[:-1], mutant
    N, S, T, Tn, m, n, Bt = cs.N, cs.S, cs.T, cs.Tn, cs.m, cs.n, x.shape[0]
    k_full, K_full = cs.plant.sweep(cs.plant.blocks(x, u))
    k_seg, K_seg = (k_full[:, N - S:], K_full[:, N - S:]) if tail is None else (np.asarray(tail[0], dtype=np.float64),
                                                                                  np.asarray(tail[1], dtype=np.float64))
    x_err = x - cs.x_ref_arg + cs.offset
    if mutant == "x_ref not subtracted":
        x_err = x + cs.offset
    elif mutant == "offset with the opposite sign":
        x_err = x - cs.x_ref_arg - cs.offset
    elif mutant == "model.x_ref in place of the argument":
        x_err = x - cs.plant.x_ref + cs.offset
    src = (k_seg, K_seg)
    if mutant == "prompt from rows 0..P-1 of the stack":
        src = (k_full[:, :cs.P], K_full[:, :cs.P])
    elif mutant == "prompt from the previous solve's tail":
        src = stale
    prompt = tokens(*src) if mutant == "prompt in the data-set layout" else pack_prompt(*src)
    if mutant == "prompt rows in reverse order":
        prompt = prompt[:, ::-1].copy()
    pred = predict(cs, weights(cs.name, precision), x, x_err, prompt, operand, kernel_norm if mutant is None else None)
    if mutant == "prediction unpacked as [k | K.flat]":
        pk, pK = pred[..., :m], pred[..., m:].reshape(Bt, T, m, n)
    else:
        pk, pK = (np.stack(a) for a in zip(*(o_ilqr.unpack_prediction(pred[b], m, n) for b in range(Bt))))
    if mutant == "predicted rows shifted by one step":
        idx = [min(t + 1, T - 1) for t in range(T)]
        pk, pK = pk[:, idx], pK[:, idx]
    sk, sK = k_seg, K_seg
    if mutant == "the last N - T swept rows instead of the first" and cs.keep > 0:
        sk, sK = k_seg[:, S - cs.keep:], K_seg[:, S - cs.keep:]
    k = np.concatenate([pk, sk], axis=1)[:, :N].copy()
    K = np.concatenate([pK, sK], axis=1)[:, :N].copy()
    if mutant == "tail rows overwritten by the prediction" and Tn < N:
        k[:, Tn:], K[:, Tn:] = pk[:, Tn - 1:Tn], pK[:, Tn - 1:Tn]
    return dict(x_err=x_err, prompt=prompt, pred=pred, k=k, K=K, k_seg=k_seg, K_seg=K_seg, k_full=k_full, K_full=K_full)


def reference(cs, x, u, precision, tail=None):
    """What the device's stack is compared with: `compose` with the states normalised as the case's branch normalises them."""
    return compose(cs, x, u, precision, tail=tail, kernel_norm="torch" if cs.branch == "batch_only" else "shifted")


def is_noop(mutant, cs, precision=None):
    """True where the mistake cannot show on this case."""
    if mutant in LAYOUT_MUTANTS:
        return cs.m == 1                                                   # the two layouts coincide
    if mutant == "prompt rows in reverse order":
        return cs.P == 1
    if mutant == "the last N - T swept rows instead of the first":
        return not 0 < cs.keep < cs.S                                      # no swept row lands in the horizon, or all of them do
    if mutant == "tail rows overwritten by the prediction":
        return cs.Tn == cs.N
    if mutant == "a stopped trajectory's rows rewritten":
        # a trajectory that stopped because no step was accepted keeps its nominal: recomputing its rows gives the same rows
        it = iteration(cs.name, precision)
        return not np.any(it["stopped"] & it["found"])
    return False


# ---------------------------------------------------------------------------------------------------------------- measures
def _per_trajectory(got, want):
    got, want = (np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1) for a in (got, want))
    den = np.linalg.norm(want, axis=1)
    return np.linalg.norm(got - want, axis=1) / np.where(den > 0, den, 1.0)


def swept_errors(cs, got_k, got_K, ref):
    """Stack rows Tn .. Tn + keep - 1 against the first `keep` rows of the reference's tail -> dict(K, k) of (B,) relative Frobenius
    errors per trajectory (zeros where no swept row lands in the horizon)."""
    if cs.keep == 0:
        return dict(K=np.zeros(got_k.shape[0]), k=np.zeros(got_k.shape[0]))
    r = slice(cs.Tn, cs.Tn + cs.keep)
    return segment_errors(got_k[:, r], got_K[:, r], ref, cs.keep)


def segment_errors(got_k_seg, got_K_seg, ref, rows=None):
    """The first `rows` (default: all S) rows of a swept segment against the reference's tail -> dict(K, k) of (B,)."""
    r = slice(0, rows)
    return dict(K=_per_trajectory(got_K_seg[:, r], ref["K_seg"][:, r]), k=_per_trajectory(got_k_seg[:, r], ref["k_seg"][:, r]))


def predicted_errors(cs, got_k, got_K, ref, rows=None):
    """Stack rows < Tn regrouped into tokens, against the reference's -> predictor_cases.quantities.  rows: trajectories to compare."""
    b = slice(None) if rows is None else rows
    return prc.quantities(tokens(got_k[b, :cs.Tn], got_K[b, :cs.Tn]), tokens(ref["k"][b, :cs.Tn], ref["K"][b, :cs.Tn]))


def linesearch_errors(got, want):
    """(x, u, cost) against (x, u, cost), per trajectory -> the worst of the relative Frobenius errors of x and u and the relative cost
    error, (B,)."""
    ec = np.abs(np.asarray(got[2]) - want[2]) / np.where(np.abs(want[2]) > 0, np.abs(want[2]), 1.0)
    return np.maximum(np.maximum(_per_trajectory(got[0], want[0]), _per_trajectory(got[1], want[1])), ec)


# ---------------------------------------------------------------------------------------------------------------- the line search
def candidates(cs, x0, x, u, k, K, fp32=False):
    """The closed-loop rollout at every step size -> list of (x', u', cost)."""
    return [cs.plant.closed_loop(x0, x, u, k, K, a, fp32=fp32) for a in ALPHAS]


def accept(J, cand):
    """The first step size whose cost does not exceed J, per trajectory -> index (B,), -1: none.  A non-finite cost is never accepted."""
    costs = np.stack([c[2] for c in cand])
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(costs) & (costs <= J[None])
    return np.where(ok.any(axis=0), ok.argmax(axis=0), -1)


def decidable(J, cand, bound):
    """(B,) bool: no candidate's cost lies within DECIDABLE_MARGIN x bound x |J| of J (a non-finite candidate is far from it)."""
    costs = np.stack([c[2] for c in cand])
    with np.errstate(invalid="ignore"):
        near = np.isfinite(costs) & (np.abs(costs - J[None]) <= DECIDABLE_MARGIN * bound * np.abs(J)[None])
    return ~near.any(axis=0)


def committed(x, u, J, cand, idx):
    """x, u, cost after the line search: the accepted candidate's, the nominal's where none was accepted."""
    nx, nu, nJ = x.copy(), u.copy(), J.copy()
    for b, i in enumerate(idx):
        if i >= 0:
            nx[b], nu[b], nJ[b] = cand[i][0][b], cand[i][1][b], cand[i][2][b]
    return nx, nu, nJ


def iterate(cs, x0, u, x, precision):
    """The oracle's iteration from the nominal (x0, u, x) -> dict(ref, J, cand, idx, found, stopped, x, u, cost): `stopped` as the
    solver stops a trajectory (no step accepted, or a gain below TOL); x, u, cost after the line search."""
    ref = reference(cs, x, u, precision)
    J = cs.plant.rollout(x0, u)[1]
    cand = candidates(cs, x0, x, u, ref["k"], ref["K"])
    idx = accept(J, cand)
    nx, nu, nJ = committed(x, u, J, cand, idx)
    found = idx >= 0
    return dict(ref=ref, J=J, cand=cand, idx=idx, found=found, stopped=~found | (np.abs(J - nJ) < TOL), x=nx, u=nu, cost=nJ)


@functools.lru_cache(maxsize=None)
def iteration(name, precision):
    """The oracle's first iteration from the case's start."""
    cs = case(name)
    return iterate(cs, cs.x0, cs.u, cs.x, precision)


def second_nominal(name, precision):
    """The controls after the oracle's first iteration, rounded to fp32: the nominal of the teacher-forced second iteration."""
    return f32(iteration(name, precision)["u"])


@functools.lru_cache(maxsize=None)
def nominals(name, precision):
    """The case's own inputs, as (x0, u, x): 0 the case's start and 1 the teacher-forced second iteration (what the GPU test solves
    from and compares), 2 the nominal the solver object solves before them and 3 the second iteration of that one.  Four draws, as
    predictor_cases.N_DRAWS."""
    cs = case(name)
    roll = lambda x0, u: f32(cs.plant.rollout(x0, u)[0])
    u2 = second_nominal(name, precision)
    px = roll(cs.prev_x0, cs.prev_u)
    pu2 = f32(iterate(cs, cs.prev_x0, cs.prev_u, px, precision)["u"])
    return ((cs.x0, cs.u, cs.x), (cs.x0, u2, roll(cs.x0, u2)), (cs.prev_x0, cs.prev_u, px), (cs.prev_x0, pu2, roll(cs.prev_x0, pu2)))


# ---------------------------------------------------------------------------------------------------------------- bounds
@functools.lru_cache(maxsize=None)
def predictor_noise(name, precision, neighbours=None):
    """predictor_cases.noise on this case's own inputs: the operand-rounded oracle against the plain one, both on rounded weights and
    both normalising as the kernel does, the worst over the four draws of `nominals` and, per draw, over NEIGHBOURS inputs: the draw
    itself and seeded neighbours of it, every state moved by up to NEIGHBOUR_STEP of itself (both oracles are evaluated at the
    neighbour).  Why neighbours: these predictors attend sharply and their prompts are normalised with the statistics of another
    layout (hundreds of standard deviations), so a few tokens sit next to a tie between two keys and carry a rounding error
    tens of times the typical token's.  What one evaluation gives for such a token is a single sample of that error, and the
    worst-token and worst-channel measures are made of exactly those tokens; a neighbour keeps the token next to its tie and draws the
    sample again (tests/test_hybrid_cases_cpu.py prints the spread between the neighbours)."""
    cs = case(name)
    norm = "torch" if cs.branch == "batch_only" else "shifted"
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for i, (x0, u, x) in enumerate(nominals(name, precision)):
        for r in (range(NEIGHBOURS) if neighbours is None else neighbours):
            g = np.random.default_rng([NAMES.index(name), i, r, 17])
            xj = x if r == 0 else f32(x * (1.0 + NEIGHBOUR_STEP * g.uniform(-1.0, 1.0, x.shape)))
            plain = compose(cs, xj, u, precision, kernel_norm=norm)
            noisy = compose(cs, xj, u, precision, operand=precision, kernel_norm=norm)
            q = predicted_errors(cs, noisy["k"], noisy["K"], plain)
            worst = {key: max(worst[key], q[key]) for key in QUANTITIES}
    return worst


def predictor_bound(name, precision):
    if precision == "fp32":
        return dict.fromkeys(QUANTITIES, FP32_PREDICTOR_BOUND)
    return {key: FACTOR * v for key, v in predictor_noise(name, precision).items()}


@functools.lru_cache(maxsize=None)
def sweep_noise(name, precision, which=0, rows=None, draws=None):
    """E -> dict(K, k) of (B,): the float32 sweep (NumPy float32) on float32 blocks against the fp64 sweep on the exact blocks, per
    trajectory, on the first `rows` (default: all S) tail rows about nominal `which` of `nominals`; the worst of 1 + SWEEP_DRAWS
    restatements.  Restatement 0 holds the exact blocks correctly rounded; the others hold them as a float32 evaluation does: every
    entry is the result of a short float32 expression (sines, products, sums), not the rounded exact value, which restatement r models
    as a seeded relative error of up to LIN_ULPS ulp per entry.
    Per nominal, quantity and trajectory, because k = -W (l_u + B^T V_x) is what cancellation leaves: next to the optimum
    (trajectories 0 and 1), and on the swept rows after an accepted full step under those rows' own gains, it is 1e-2 .. 1e-4 of what
    it is elsewhere, and its float32 error relative to itself is as much larger -- and as much a matter of which way a few roundings
    fell: tests/test_hybrid_cases_cpu.py prints the spread between the restatements (several-fold on those rows)."""
    cs = case(name)
    x0, u, x = nominals(name, precision)[which]
    d = cs.plant.blocks(x, u)
    k64, K64 = cs.plant.sweep(d)
    t = slice(cs.N - cs.S, cs.N)
    worst = None
    for r in (range(1 + SWEEP_DRAWS) if draws is None else draws):
        g = np.random.default_rng([NAMES.index(name), which, r])
        d32 = {key: f32(v if r == 0 else v * (1.0 + LIN_ULPS * 2.0 ** -23 * g.uniform(-1.0, 1.0, np.shape(v)))) for key, v in d.items()}
        k32, K32 = cs.plant.sweep(d32, dtype=np.float32)
        e = segment_errors(k32[:, t], K32[:, t], dict(k_seg=k64[:, t], K_seg=K64[:, t]), rows)
        worst = e if worst is None else {key: np.maximum(worst[key], e[key]) for key in e}
    return worst


def sweep_bound(name, precision, which=0, rows=None):
    return {key: np.maximum(SWEEP_START, 4.0 * v) for key, v in sweep_noise(name, precision, which, rows).items()}


@functools.lru_cache(maxsize=None)
def linesearch_noise(name, precision):
    """E_cl: the closed loop with fp32 storage against fp64 under the oracle's stack at the accepted step size, the worst trajectory."""
    cs = case(name)
    it = iteration(name, precision)
    c32 = candidates(cs, cs.x0, cs.x, cs.u, f32(it["ref"]["k"]), f32(it["ref"]["K"]), fp32=True)
    c64 = candidates(cs, cs.x0, cs.x, cs.u, f32(it["ref"]["k"]), f32(it["ref"]["K"]))
    worst = 0.0
    for b, i in enumerate(it["idx"]):
        if i >= 0:
            e = linesearch_errors(tuple(a[b:b + 1] for a in c32[i]), tuple(a[b:b + 1] for a in c64[i]))
            worst = max(worst, float(e[0]))
    return worst


def linesearch_bound(name, precision):
    return max(LS_START, 4.0 * linesearch_noise(name, precision))


# ---------------------------------------------------------------------------------------------------------------- teeth
def mutant_shift(name, mutant, precision):
    """measure -> (shift of that measure by the mutant on the case, the measure's bound): what the GPU test asserts, on the fp64
    composition.  "a stopped trajectory's rows rewritten" moves a bit-for-bit comparison, whose bound is 0."""
    cs = case(name)
    it = iteration(name, precision)
    if mutant == MUTANTS[-1]:
        # the rows of the stopped trajectories, recomputed about the nominal the line search left behind
        first, again = compose(cs, cs.x, cs.u, precision), compose(cs, f32(it["x"]), f32(it["u"]), precision)
        rows = it["stopped"]
        moved = max(np.abs(again["K"][rows] - first["K"][rows]).max(), np.abs(again["k"][rows] - first["k"][rows]).max())
        return {"stopped rows bit for bit": (float(moved), 0.0)}
    base = compose(cs, cs.x, cs.u, precision)              # (both sides normalise the fp64 x_err: a no-op moves nothing at all)
    px = f32(cs.plant.rollout(cs.prev_x0, cs.prev_u)[0])
    pk, pK = cs.plant.sweep(cs.plant.blocks(px, cs.prev_u))
    mut = compose(cs, cs.x, cs.u, precision, mutant=mutant, stale=(pk[:, cs.N - cs.S:], pK[:, cs.N - cs.S:]))
    pb, sb = predictor_bound(name, precision), sweep_bound(name, precision, 0, cs.keep or None)
    q = predicted_errors(cs, mut["k"], mut["K"], base)
    s = swept_errors(cs, mut["k"], mut["K"], base)
    out = {f"predicted {key}": (q[key], pb[key]) for key in QUANTITIES}
    for key in ("K", "k"):
        b = int(np.argmax(s[key] / sb[key]))
        out[f"swept {key}"] = (float(s[key][b]), float(sb[key][b]))
    return out


def mutant_ratio(name, mutant, precision):
    """The largest shift / bound of mutant_shift with the measure's name (inf where a bit-for-bit comparison moves), or None where
    the mutant is a no-op on the case."""
    if is_noop(mutant, case(name), precision):
        return None
    sh = mutant_shift(name, mutant, precision)
    ratios = {key: (v / bd if bd > 0 else (np.inf if v > 0 else 0.0)) for key, (v, bd) in sh.items()}
    key = max(ratios, key=ratios.get)
    return ratios[key], key
