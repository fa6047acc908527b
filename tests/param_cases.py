"""Parameter sets away from the defaults for the built-in cart-pole and quadrotor, the seeded inputs that go with them and the
single-parameter mutants that the tests must be able to tell apart.  A plain helper module (like tests/dual_probe.py), used by

  * tests/golden/make_golden.py (G16: the reference evaluated at the `skew` sets),
  * tests/test_param_cases_cpu.py (oracle pinned to the reference, analytic vs finite differences, teeth, well-posedness),
  * tests/test_model_params_gpu.py (every kernel that reads quattro_model_params against the fp64 oracle).

Why these values: at the defaults Ix == Iy (the yaw gyroscopic coefficient (Ix - Iy) / Iz is exactly 0), r is constant, q and qf
repeat, x_ref is zero in 11 of 12 components, dt is always 0.01, and the barrier branch is taken by the quadrotor only.  Every
value below is pairwise distinct within its vector, so an index slip or a swapped pair changes a number.

Inputs are rounded to fp32 and handed back as fp64: the device and the oracle start from the same numbers.
"""
import copy

import numpy as np

from oracle import ilqr as o_ilqr
from oracle import linearize as o_lin
from oracle import models as o_models

PHYS_NAMES = {
    "quadrotor": ("mass", "Ix", "Iy", "Iz", "arm", "gravity", "k_yaw"),
    "cartpole": ("m_cart", "m_pole", "length", "gravity"),
}
DEFAULT_PHYS = {
    "quadrotor": dict(mass=1.0, Ix=0.02, Iy=0.02, Iz=0.04, arm=0.1, gravity=9.81, k_yaw=0.01),
    "cartpole": dict(m_cart=1.0, m_pole=0.1, length=0.15, gravity=9.81),
}
DEFAULT_DT = 0.01
DEFAULT_BARRIER = {"quadrotor": (1000.0, 10.0), "cartpole": (0.0, 1.0)}       # (alpha, beta)

_QUAD_SKEW = dict(
    dt=0.02,
    phys=dict(mass=1.3, Ix=0.015, Iy=0.03, Iz=0.041, arm=0.13, gravity=9.6, k_yaw=0.017),
    x_ref=(0.3, -0.2, 0.7, 0.1, -0.15, 0.05, 0.08, -0.06, 0.4, 0.2, -0.3, 0.25),
    q=(7.0, 13.0, 41.0, 0.6, 1.7, 2.9, 8.0, 15.0, 33.0, 0.8, 1.9, 3.1),
    r=(0.006, 0.011, 0.017, 0.025),
    qf=(90.0, 140.0, 450.0, 7.0, 12.0, 19.0, 80.0, 160.0, 390.0, 6.0, 14.0, 21.0),
    barrier_alpha=350.0, barrier_beta=6.0)
_CART_SKEW = dict(
    dt=0.02,
    phys=dict(m_cart=1.4, m_pole=0.23, length=0.31, gravity=9.6),
    x_ref=(0.2, -0.1, 0.15, 0.3),
    q=(3.0, 0.4, 12.0, 0.7), r=(0.004,), qf=(40.0, 5.0, 130.0, 0.9),
    barrier_alpha=0.0, barrier_beta=1.0)

SETS = {
    "quadrotor": {
        "skew": _QUAD_SKEW,
        # the branch the quadrotor never takes at its defaults; r alone is l_uu here
        "skew_nobarrier": dict(_QUAD_SKEW, barrier_alpha=0.0, dt=0.004),
    },
    "cartpole": {
        "skew": _CART_SKEW,
        # the branch the cart-pole never takes at its defaults
        "skew_barrier": dict(_CART_SKEW, barrier_alpha=25.0, barrier_beta=3.0, dt=0.004),
    },
}
MODELS = ("quadrotor", "cartpole")
SET_NAMES = {m: tuple(SETS[m]) for m in MODELS}
DIMS = {"quadrotor": (12, 4), "cartpole": (4, 1)}
B_FULL = {"quadrotor": 19, "cartpole": 9}     # quadrotor: one full wave of sixteen four-lane quads plus a ragged one
BATCHES = {"quadrotor": (1, 19), "cartpole": (1, 9)}
HORIZONS = (1, 7, 26)                          # 26 crosses the fused sweep's 24/25-step refill boundary
SEED = 7
THETA_MAX = 1.3                                # |pitch| stays clear of the Euler-angle singularity at pi / 2

# x0 = x_ref + spread * N(0, 1).  Body rates of a few rad/s are what make the gyroscopic terms visible.
QUAD_SPREAD = np.array([.3, .3, .3, .5, .5, .5, .3, .3, .5, 2.5, 2.5, 2.5])
# (set, N) -> (spread of roll and pitch, spread of the three body rates) where the values above carry the pitch past THETA_MAX
# within the horizon.  dt = 0.02, N = 26 is 0.52 s of tumbling: the largest fp64 pitch is 2.06 with (0.3, 0.7) and still 1.34
# with (0.3, 0.0) -- it comes from the start angle and from the torque of the barrier control, u_1 = -0.05 against a hover
# thrust of 3.1 every third step, which also drives the body rates to 5.6 rad/s whatever they start from -- and 1.28 with
# (0.1, 0.7), the values used.
QUAD_SPREAD_OVERRIDE = {("skew", 26): (0.1, 0.7)}
CART_SPREAD = np.array([.3, .3, .3, .5])
CART_U = {"skew": (0.0, 2.0), "skew_barrier": (0.9, 2.0)}      # (centre, sigma): 0.9 / 2.0 puts about a third below zero

# The bounds the GPU tests assert (tests/test_kernels_gpu.py header, test_short_and_odd_horizons_against_the_oracle), by
# compared quantity; the teeth test asks every mutant for 100 x these.
BOUNDS = dict(
    sim_x=2e-6, sim_cost=2e-6, total_cost=2e-6,
    A=1e-5, B=1e-5, lx=1e-5, lu=1e-5, lxx=1e-5, luu=1e-5, A_rates=1e-5, B_rates=1e-5, VxN=1e-6, VxxN=1e-6,
    K=5e-6, k=5e-6, K_barrier=5e-6, k_barrier=5e-6,
    cl_x=1e-5, cl_u=1e-5, cl_cost=1e-5)
FAMILIES = dict(
    rollout=("sim_x", "sim_cost", "total_cost", "cl_x", "cl_u", "cl_cost"),
    records=("A", "B", "lx", "lu", "lxx", "luu", "A_rates", "B_rates", "VxN", "VxxN"),
    gains=("K", "k", "K_barrier", "k_barrier"))
BLOCKS = ("A", "B", "lx", "lu", "lxx", "luu", "lux")


def params(model, set_name):
    return copy.deepcopy(SETS[model][set_name])


def spec_from(model, p, integ):
    """The fp64 oracle's problem description for a parameter dict; integ 'euler' / 'rk4'."""
    n, m = DIMS[model]
    return o_models.ModelSpec(
        model_id=o_models.MODEL_QUADROTOR if model == "quadrotor" else o_models.MODEL_CARTPOLE, n=n, m=m, dt=float(p["dt"]),
        integrator=o_models.INTEGRATOR_RK4 if integ == "rk4" else o_models.INTEGRATOR_EULER,
        x_ref=np.asarray(p["x_ref"], dtype=np.float64), Q=np.diag(p["q"]).astype(np.float64),
        R=np.diag(p["r"]).astype(np.float64), Qf=np.diag(p["qf"]).astype(np.float64),
        barrier_alpha=float(p["barrier_alpha"]), barrier_beta=float(p["barrier_beta"]), phys=dict(p["phys"]))


def spec(model, set_name, integ):
    return spec_from(model, params(model, set_name), integ)


def device_model(models_mod, model, set_name, integ):
    """The DeviceModel of a set: the built-in model with every parameter replaced through with_()."""
    p = SETS[model][set_name]
    return models_mod.model_by_name(model, integrator=integ).with_(
        dt=float(p["dt"]), x_ref=p["x_ref"], q=tuple(p["q"]), r=tuple(p["r"]), qf=tuple(p["qf"]),
        barrier_alpha=float(p["barrier_alpha"]), barrier_beta=float(p["barrier_beta"]),
        phys=tuple(float(p["phys"][k]) for k in PHYS_NAMES[model]))


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def inputs(model, set_name, N, B=None, seed=SEED):
    """x0 (B, n), u (B, N, m): the first B rows of the full batch of B_FULL[model] starts, so that B = 1 is a row of the larger
    case.  Quadrotor: the fp64 rollouts (both integrators) are checked to keep |theta| < THETA_MAX."""
    p = SETS[model][set_name]
    n, m = DIMS[model]
    full = B_FULL[model]
    B = full if B is None else B
    rng = np.random.default_rng(seed)
    x_ref = np.asarray(p["x_ref"], dtype=np.float64)
    if model == "quadrotor":
        spread = QUAD_SPREAD.copy()
        spread[6:8], spread[9:] = QUAD_SPREAD_OVERRIDE.get((set_name, N), (spread[6], spread[9]))
        x0 = x_ref + spread * rng.standard_normal((full, n))
        u = p["phys"]["mass"] * p["phys"]["gravity"] / 4.0 + 0.4 * rng.standard_normal((full, N, m))
        u[:, ::3, 1] = -0.05                       # the barrier is active on one control every third step
    else:
        x0 = x_ref + CART_SPREAD * rng.standard_normal((full, n))
        centre, sigma = CART_U[set_name]
        u = centre + sigma * rng.standard_normal((full, N, m))
    x0, u = _f32(x0), _f32(u)
    if model == "quadrotor":
        for integ in ("euler", "rk4"):
            xs, _ = o_lin.rollout_batched(spec(model, set_name, integ), x0, u)
            worst = float(np.max(np.abs(xs[:, :, 7])))
            assert worst < THETA_MAX, (set_name, N, integ, worst)
    return x0[:B].copy(), u[:B].copy()


# ---------------------------------------------------------------------------------------------------------------- mutants
def _swap(key, i, j):
    def fn(p):
        v = list(p[key]); v[i], v[j] = v[j], v[i]; p[key] = tuple(v)
    return fn


def _phys_swap(a, b):
    def fn(p):
        p["phys"][a], p["phys"][b] = p["phys"][b], p["phys"][a]
    return fn


def _phys_default(model, name):
    def fn(p):
        p["phys"][name] = DEFAULT_PHYS[model][name]
    return fn


def _set(key, value):
    def fn(p):
        p[key] = value
    return fn


def _iy_is_ix(p):
    p["phys"]["Iy"] = p["phys"]["Ix"]


def _xref_zero(i):
    def fn(p):
        v = list(p["x_ref"]); v[i] = 0.0; p["x_ref"] = tuple(v)
    return fn


ALL = ("rollout", "records", "gains")
# (name, edit of the parameter dict, families the parameter enters).  The quadrotor's gravity is a constant acceleration: it
# enters no derivative block and no gain, only the rollouts.  The cart-pole's enters everything.
MUTANTS = {
    "quadrotor": [
        ("Iy:=Ix", _iy_is_ix, ALL),
        ("swap Ix,Iy", _phys_swap("Ix", "Iy"), ALL),
        ("k_yaw->default", _phys_default("quadrotor", "k_yaw"), ALL),
        ("arm->default", _phys_default("quadrotor", "arm"), ALL),
        ("mass->default", _phys_default("quadrotor", "mass"), ALL),
        ("gravity->default", _phys_default("quadrotor", "gravity"), ("rollout",)),
        ("dt->default", _set("dt", DEFAULT_DT), ALL),
        ("barrier_alpha->default", _set("barrier_alpha", DEFAULT_BARRIER["quadrotor"][0]), ALL),
        ("barrier_beta->default", _set("barrier_beta", DEFAULT_BARRIER["quadrotor"][1]), ALL),
        ("swap r0,r3", _swap("r", 0, 3), ALL),
        ("swap q0,q1", _swap("q", 0, 1), ALL),
        ("swap q9,q10", _swap("q", 9, 10), ALL),
        ("swap qf3,qf4", _swap("qf", 3, 4), ALL),
        ("x_ref[11]:=0", _xref_zero(11), ALL),
    ],
    "cartpole": [
        ("swap m_cart,m_pole", _phys_swap("m_cart", "m_pole"), ALL),
        ("length->default", _phys_default("cartpole", "length"), ALL),
        ("gravity->default", _phys_default("cartpole", "gravity"), ALL),
        ("dt->default", _set("dt", DEFAULT_DT), ALL),
        ("barrier_alpha->default", _set("barrier_alpha", DEFAULT_BARRIER["cartpole"][0]), ALL),
        ("barrier_beta->default", _set("barrier_beta", DEFAULT_BARRIER["cartpole"][1]), ALL),
        ("swap q0,q2", _swap("q", 0, 2), ALL),
        ("swap q1,q3", _swap("q", 1, 3), ALL),
        ("swap qf1,qf3", _swap("qf", 1, 3), ALL),
        ("swap qf0,qf2", _swap("qf", 0, 2), ALL),
        ("x_ref[3]:=0", _xref_zero(3), ALL),
    ],
}


def mutate(model, set_name, name):
    """-> (parameter dict of the mutant, families, True where the edit changes nothing in this set: barrier_beta while
    barrier_alpha is 0, or a value that already is the default)."""
    edit, fams = next((e, f) for n_, e, f in MUTANTS[model] if n_ == name)
    p = params(model, set_name)
    edit(p)
    true = params(model, set_name)
    noop = p == true or (name.startswith("barrier_beta") and true["barrier_alpha"] == 0.0)
    return p, fams, noop


# ---------------------------------------------------------------------------------------------------------------- quantities
def sub_blocks(blocks):
    """The sub-blocks the defaults hide: the body-rate rows of A (gyroscopic terms) and of B (torque rows).  Quadrotor only."""
    return dict(A_rates=blocks["A"][..., 9:12, :], B_rates=blocks["B"][..., 9:12, :])


def barrier_rows(K, k):
    """The gain rows of the control the inputs hold at -0.05 every third step (quadrotor).  There the barrier is nearly all of
    Q_uu, so K's row is proportional to 1 / barrier_alpha -- and small: inside the whole K a wrong barrier_alpha moves 5e-5,
    inside these rows 0.65.  The fused sweeps evaluate the barrier derivatives themselves and give out nothing but gains."""
    return dict(K_barrier=K[:, ::3, 1, :], k_barrier=k[:, ::3, 1])


def evaluate(sp, x0, u, nominal=None, gains=None):
    """Every quantity the GPU tests compare, in fp64: the open-loop rollout, the total cost of the nominal, the derivative
    blocks about the nominal, the gains, and the alpha = 1 closed-loop rollout under the gains.  `nominal` / `gains`: take
    these instead of the spec's own (a mutant is evaluated about the true nominal with the true gains, as a wrong kernel is)."""
    xs, J = o_lin.rollout_batched(sp, x0, u)
    nom = xs if nominal is None else nominal
    blocks = o_lin.linearize_analytic(sp, nom, u)
    k, K = o_ilqr.riccati_sweep_batched(blocks)
    kk, KK = (k, K) if gains is None else gains
    nx, nu, nJ = o_lin.closed_loop_rollout_batched(sp, x0, nom, u, kk, KK, 1.0)
    out = dict(sim_x=xs, sim_cost=J, total_cost=total_cost(sp, nom, u), K=K, k=k, cl_x=nx, cl_u=nu, cl_cost=nJ, **blocks)
    if sp.n == 12:
        out.update(sub_blocks(blocks))
        out.update(barrier_rows(K, k))
    return out


def total_cost(sp, xs, u):
    """sum_t L(x_t, u_t) + Lf(x_N) of given sequences xs (B, N+1, n), u (B, N, m): (B,)."""
    return np.sum(o_lin.stage_cost(sp, xs[:, :-1], u), axis=1) + o_lin.terminal_cost(sp, xs[:, -1])


def change(name, got, ref):
    """The error measure of the GPU tests: relative Frobenius norm for arrays, max relative for the costs."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if name.endswith("cost"):
        return float(np.max(np.abs(got - ref) / np.abs(ref)))
    den = np.linalg.norm(ref)
    return float(np.linalg.norm(got - ref) / (den if den > 0 else 1.0))


def unpivoted_pivot_ratio(quu):
    """quu (..., m, m) -> the smallest pivot of an elimination without pivoting, relative to the diagonal entry it started as.
    The TILE16 sweeps eliminate in this order and flag a trajectory whose pivot collapses."""
    a = np.array(quu, dtype=np.float64)
    m = a.shape[-1]
    diag0 = np.abs(np.array([a[..., i, i] for i in range(m)]))
    worst = np.inf
    for p in range(m):
        piv = a[..., p, p]
        worst = min(worst, float(np.min(piv / diag0[p])))
        for r in range(p + 1, m):
            f = a[..., r, p] / piv
            a[..., r, :] = a[..., r, :] - f[..., None] * a[..., p, :]
    return worst


# ---------------------------------------------------------------------------------------------------------------- whole solves
# The converged solve is compared with oracle.ilqr.optimize -- the reference's algorithm in fp64, its derivatives by finite
# differences -- in the form of tests/test_user_model_gpu.py::test_user_model_solve_matches_the_oracle: iteration count within
# one, and where it is equal the cost (relative) and x, u (largest absolute difference).  The comparison starts from that test's
# bounds, SOLVE_START.  Both solves stop on |dJ| < 1e-3, not at the optimum, so what separates them is the unconverged remainder
# seen through a last bit, not fp32 arithmetic alone.  SOLVE_E is therefore measured without the device: the same algorithm with
# exact derivatives and fp32 storage (solve_emulated: nominal, controls and candidates rounded to fp32, the sweep in fp32 NumPy)
# against optimize(), worst over both integrators and the three trajectories of SOLVE_TRAJ; tests/test_param_cases_cpu.py holds
# the emulation to these figures.  Asserted on the GPU: max(SOLVE_START, 4 x SOLVE_E) -- the kernels round in another order.
SOLVE_N, SOLVE_B, SOLVE_TRAJ, SOLVE_MAX_ITER, SOLVE_TOL = 7, 5, (0, 2, 4), 40, 1e-3
SOLVE_ALPHAS = (1.0, 0.5, 0.25, 0.1, 0.05, 0.01)
SOLVE_START = dict(cost=1e-6, x=1e-5, u=3e-5)
SOLVE_E = {"quadrotor": dict(cost=4.8e-8, x=2.7e-6, u=6.6e-5), "cartpole": dict(cost=7.8e-8, x=1.3e-6, u=4.4e-5)}


def solve_bounds(model):
    return {key: max(SOLVE_START[key], 4.0 * SOLVE_E[model][key]) for key in SOLVE_START}


def solve_optimize(sp, x0, u0, reg=o_ilqr.QUU_REG):
    """oracle.ilqr.optimize on the spec's callables for one trajectory -> u (N, m), x (N+1, n), cost, iterations.  reg: the
    Q_uu regularisation of every backward pass (tests/reg_cases.py moves it; the default is the reference's)."""
    u, x, logs = o_ilqr.optimize(sp.f, sp.L, sp.Lf, x0, list(u0), u0.shape[0], max_iter=SOLVE_MAX_ITER, tol=SOLVE_TOL,
                                 reg=reg)
    return np.array(u), x, float(o_ilqr.trajectory_cost(sp.L, sp.Lf, x, u)), len(logs)


def solve_emulated(sp, x0, u0, dtype=np.float32, reg=o_ilqr.QUU_REG):
    """The algorithm of optimize() for one trajectory with exact derivatives and `dtype` storage: x, u and every candidate are
    rounded to dtype, the sweep runs in dtype (at `reg`), costs are summed in fp64 as on the device."""
    r = lambda a: np.asarray(a).astype(dtype).astype(np.float64)
    x0, u = x0[None], r(u0[None])
    xs = r(o_lin.rollout_batched(sp, x0, u)[0])
    J = float(total_cost(sp, xs, u)[0])
    its = 0
    for _ in range(SOLVE_MAX_ITER):
        its += 1
        blocks = o_lin.linearize_analytic(sp, xs, u)
        k, K = o_ilqr.riccati_sweep_batched({k_: v.astype(dtype) for k_, v in blocks.items()}, reg=reg, dtype=dtype)
        k, K = k.astype(np.float64), K.astype(np.float64)
        found = False
        for a in SOLVE_ALPHAS:
            nx, nu, _ = o_lin.closed_loop_rollout_batched(sp, x0, xs, u, k, K, a)
            nx, nu = r(nx), r(nu)
            nJ = float(total_cost(sp, nx, nu)[0])
            if nJ <= J:
                found = True
                break
        if not found:
            break
        dJ, xs, u, J = abs(J - nJ), nx, nu, nJ
        if dJ < SOLVE_TOL:
            break
    return u[0], xs[0], J, its


def solve_errors(got, ref):
    """(u, x, cost, ...) of two solves -> dict(cost=relative, x=largest absolute, u=largest absolute)."""
    return dict(cost=abs(got[2] - ref[2]) / abs(ref[2]), x=float(np.max(np.abs(got[1] - ref[1]))),
                u=float(np.max(np.abs(got[0] - ref[0]))))
