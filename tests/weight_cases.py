"""Per-trajectory cost weights (quattro_ilqr_solve_cost_f32, quattro_mpc_run_cost_f32; `weights=` of QuattroILQR.solve,
BatchedMPC.control_step and BatchedMPC.run): the seeded rows, the problem each row makes, and the mistakes a kernel could make with
them.  A plain helper module (like tests/param_cases.py and tests/ref_cases.py), used by tests/test_cost_rows_cpu.py and
tests/test_cost_rows_gpu.py.

Row b is the skew set's [q | qf | r] (param_cases.SETS[model]["skew"]), each component multiplied by a factor of its own; the
factors are log-uniform in FACTOR_RANGE from default_rng(SEED), rounded to fp32, and the row is rounded to fp32 once more: the
numbers the device holds are the numbers the oracle gets.  States and controls are ref_cases.inputs(model, N, B).  The fp64
reference is the unchanged oracle on param_cases.spec_from with the row's weights: no new reference.

The built-in quadrotor has no kernel that takes cost rows (its entries refuse them), so the cases are the cart-pole's; base_row and
weight_rows still serve the quadrotor's skew set for whoever adds that kernel.
The planar user model (tests/test_user_model_gpu.py) takes rows made the same way about its own q, qf, r.  It is compared bit for
bit only (against solvers built on model.with_), never against the oracle, so the conditions of tests/test_cost_rows_cpu.py on the
inputs (pivots, pitch, line-search margins) are not evaluated for it and its factor range is the built-in models'."""
import numpy as np

import param_cases as pc
import ref_cases as rc

SEED = 11
FACTOR_RANGE = (0.4, 2.5)
# shapes of the GPU tests: B = 5 puts more than four 16-lane rows of the cart-pole into two waves; the planar model has a wave per
# trajectory
B = {"cartpole": 5, "planar": 3}
N, N_PLANAR = 20, 12
MODELS = ("cartpole",)
SHAPES = [("cartpole", N)]
CASES = [(model, integ) for model in MODELS for integ in ("euler", "rk4")]


def factors(d, B_):
    lo, hi = np.log(FACTOR_RANGE[0]), np.log(FACTOR_RANGE[1])
    return np.exp(np.random.default_rng(SEED).uniform(lo, hi, (B_, d))).astype(np.float32)


def base_row(model):
    """[q | qf | r] of the skew set (fp64)."""
    p = pc.SETS[model]["skew"]
    return np.concatenate([p["q"], p["qf"], p["r"]]).astype(np.float64)


def rows_about(base, B_):
    """(B, 2n + m) float32 in the order [q | qf | r]: the plain-array form of `weights=`."""
    base = np.asarray(base, dtype=np.float64)
    return (base[None, :] * factors(base.size, B_).astype(np.float64)).astype(np.float32)


def weight_rows(model, B_=None):
    return rows_about(base_row(model), B[model] if B_ is None else B_)


def split(model_or_dims, row):
    """row (2n + m,) -> (q, qf, r)."""
    n, m = pc.DIMS[model_or_dims] if isinstance(model_or_dims, str) else model_or_dims
    row = np.asarray(row)
    return row[:n], row[n:2 * n], row[2 * n:2 * n + m]


def row_params(model, row):
    """The skew set's parameter dict with the weights of one row (the fp32 values, as the device holds them)."""
    p = pc.params(model, "skew")
    q, qf, r = split(model, row)
    p["q"], p["qf"], p["r"] = tuple(map(float, q)), tuple(map(float, qf)), tuple(map(float, r))
    return p


def row_spec(model, integ, row):
    return pc.spec_from(model, row_params(model, row), integ)


def const_window(model, N_):
    """(1, N + 1, n): the skew set's x_ref at every step, for ref_cases.first_iteration / solve_windowed."""
    return np.tile(np.asarray(pc.SETS[model]["skew"]["x_ref"], dtype=np.float64)[None, None, :], (1, N_ + 1, 1))


def first_iteration(model, integ, row, x0b, u0b):
    """ref_cases.first_iteration of ONE trajectory (x0b (1, n), u0b (1, N, m)) under the weights of `row`."""
    return rc.first_iteration(row_spec(model, integ, row), const_window(model, u0b.shape[1]), x0b, u0b)


# ---------------------------------------------------------------------------------------------------------------- mistakes
def mistakes(model, rows, b):
    """name -> the row a kernel with that mistake would use for trajectory b."""
    n, m = pc.DIMS[model]
    base = base_row(model).astype(np.float32)
    true = rows[b]
    out = {"the row of b + 1": rows[(b + 1) % rows.shape[0]]}
    for name, sl in (("q ignored", slice(0, n)), ("qf ignored", slice(n, 2 * n)), ("r ignored", slice(2 * n, 2 * n + m))):
        w = true.copy()
        w[sl] = base[sl]                       # the shared block's values in place of the row's
        out[name] = w
    w = true.copy()
    w[:n], w[n:2 * n] = true[n:2 * n], true[:n]
    out["q and qf exchanged"] = w
    return out


# ---------------------------------------------------------------------------------------------------------------- whole solves
# The converged solve of every trajectory is compared with oracle.ilqr.optimize on its own spec (row_spec), in the form of
# param_cases' whole-solve comparison at param_cases.SOLVE_N and its inputs, and the bound is made the way param_cases makes its
# own: SOLVE_E is what param_cases.solve_emulated (exact derivatives, fp32 storage) differs from optimize() by on the CPU, worst
# over both integrators and every trajectory of the batch (tests/test_cost_rows_cpu.py holds the emulation to these figures);
# asserted on the GPU: max(param_cases.solve_bounds(model), 4 x SOLVE_E).
SOLVE_E = {"cartpole": dict(cost=9.2e-8, x=5.8e-7, u=2.3e-5)}


def solve_inputs(model):
    return pc.inputs(model, "skew", pc.SOLVE_N, B[model])


def solve_bounds(model):
    base = pc.solve_bounds(model)
    return {key: max(base[key], 4.0 * SOLVE_E[model][key]) for key in base}
