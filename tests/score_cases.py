"""Scoring on the device (quattro_score_f32, ops.score, `score=` of BatchedMPC.run): the seeded sequences, the fp64 reference and the
mistakes a kernel could make.  A plain helper module (like tests/param_cases.py, tests/ref_cases.py and tests/weight_cases.py), used
by tests/test_score_cpu.py and tests/test_score_gpu.py.

Sequences are NOT rollouts (an open-loop quadrotor rollout of the seeded inputs tumbles to |pitch| 1.3 within 65 - 130 steps): they are
a seeded walk about the target rows, x[b, s] = row(b, s) + spread * (BIAS * sign(STEP) + N(0, 1)) with ref_cases.inputs' spreads -- the
bias keeps the walk on one side of a moving target, so that a row read a step early or late moves the TOTAL and not only single
steps -- and seeded controls, all rounded to fp32.  The rows are ref_cases.skew_rows, the weights weight_cases.weight_rows (which serves the quadrotor too).
The fp64 reference is the unchanged oracle: oracle.linearize.stage_cost / terminal_cost on param_cases.spec_from with the row's weights
and a per-step x_ref, as ref_cases.composed_cost does it.
  cartpole            the skew set (no barrier), u ~ N(0, 6): r u^2 is a few per cent of a step's cost, so a wrong r shows in the total
  quadrotor/barrier   the skew set; a third of the controls (seeded, independently) are -0.2 |N(0, 1)|, the barrier term live and about
                      half of a step's cost, the others ~ N(8, 0.4).  (With every control about zero the barrier's alpha = 350 is
                      all of the cost and r could be anything.)
  quadrotor/shortcut  the skew set, u ~ N(8, 0.4): every beta u far above 20, qt_stage_cost's exact shortcut taken by whole waves"""
import dataclasses

import numpy as np

import param_cases as pc
import ref_cases as rc
import weight_cases as wc
from oracle import linearize as o_lin

SEED = 23
BOUND = 2e-6                                        # relative, per step and per total: what test_simulate_and_total_cost asserts for costs
BATCHES = (1, 5)
STEPS = (1, 63, 64, 65, 130)                        # S + 1 = 64 fills one pass exactly; 64, 65 and 130 end in a partial pass
REF_HOLD = 3
CASES = ("cartpole", "quadrotor/barrier", "quadrotor/shortcut")
U_DIST = {"cartpole": (0.0, 6.0), "quadrotor/barrier": (8.0, 0.4), "quadrotor/shortcut": (8.0, 0.4)}      # (centre, sigma)
BIAS = 0.5
X_SPREAD = {"cartpole": pc.CART_SPREAD, "quadrotor": np.array([.3, .3, .3, .3, .3, .3, .1, .1, .3, .5, .5, .5])}


def model_of(case):
    return case.split("/")[0]


def row_index(s, ref_hold, R):
    """THE row rule of scoring: plant step s (s = S: the terminal slot) reads row min((s // ref_hold) * ref_hold, R - 1)."""
    return min((int(s) // int(ref_hold)) * int(ref_hold), R - 1)


def window(rows, S, ref_hold=1):
    """rows (B, R, n) -> (B, S + 1, n): the row every slot 0 .. S reads."""
    rows = np.asarray(rows)
    return rows[:, [row_index(s, ref_hold, rows.shape[1]) for s in range(S + 1)]]


def rows_of(case, B, R):
    return rc.skew_rows(model_of(case), B, R)


def weights_of(case, B):
    return wc.weight_rows(model_of(case), B)


def sequences(case, B, S):
    """x (B, S + 1, n), u (B, S, m): fp32 values as fp64 arrays, a walk about rows_of(case, B, S + 1).  Trajectory b of a smaller batch
    is trajectory b of a larger one."""
    model = model_of(case)
    n, m = pc.DIMS[model]
    rows = rows_of(case, max(BATCHES), S + 1).astype(np.float64)
    rng = np.random.default_rng(SEED + S)
    side = np.where(rc.STEP[model] < 0.0, -1.0, 1.0)
    x = rows + X_SPREAD[model] * (BIAS * side + rng.standard_normal((max(BATCHES), S + 1, n)))
    centre, sigma = U_DIST[case]
    u = centre + sigma * rng.standard_normal((max(BATCHES), S, m))
    if case == "quadrotor/barrier":
        below = rng.random(u.shape) < 1.0 / 3.0
        u = np.where(below, -0.2 * np.abs(rng.standard_normal(u.shape)), u)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return f32(x)[:B].copy(), f32(u)[:B].copy()


def base_params(case):
    return pc.params(model_of(case), "skew")


def oracle_score(case, x, u, win=None, weights=None, terminal=False, exchange_q_qf=False):
    """fp64: stage (B, S + 1) and total (B,) of the sequences.  win (B, S + 1, n): the target of every slot (None: the skew set's
    x_ref); weights (B, 2n + m) rows [q | qf | r] (None: the skew set's).  exchange_q_qf: a mutant (below)."""
    model = model_of(case)
    B, S = u.shape[:2]
    stage = np.zeros((B, S + 1))
    for b in range(B):
        p = base_params(case) if weights is None else wc.row_params(model, weights[b])
        if exchange_q_qf:
            p["q"], p["qf"] = p["qf"], p["q"]
        spec = pc.spec_from(model, p, "euler")                     # (the cost does not read the integrator)
        ref = np.tile(spec.x_ref, (S + 1, 1)) if win is None else np.asarray(win[b], dtype=np.float64)
        stage[b, :S] = o_lin.stage_cost(dataclasses.replace(spec, x_ref=ref[:S]), x[b, :S], u[b])
        if terminal:
            stage[b, S] = o_lin.terminal_cost(dataclasses.replace(spec, x_ref=ref[S]), x[b, S])
    total = np.zeros(B)
    for s in range(S + 1):                                         # in step order, as the device sums
        total = total + stage[:, s]
    return stage, total


# ---------------------------------------------------------------------------------------------------------------- mistakes
# The configuration the mutants are measured in: B = 5, S = 65 (a second, partial pass), targets of R_SHORT rows held REF_HOLD steps,
# heterogeneous weights, the terminal slot on.  With ref_hold = 3 and R = 40 the slots read rows 0, 3, ..., 39 and the run outlasts
# its rows from step 40 on.
TEETH_B, TEETH_S, R_SHORT = 5, 65, 40


def truth(case, x, u):
    B, S = u.shape[:2]
    rows, w = rows_of(case, B, R_SHORT), weights_of(case, B)
    return oracle_score(case, x, u, window(rows, S, REF_HOLD), w, terminal=True)


def mutants(case, x, u):
    """name -> (stage, total) a kernel with that mistake would return for the configuration of truth()."""
    model = model_of(case)
    n, m = pc.DIMS[model]
    B, S = u.shape[:2]
    rows, w = rows_of(case, B, R_SHORT), weights_of(case, B)
    win = window(rows, S, REF_HOLD)
    long_rows = rows_of(case, B, S + 2)                             # the ramp continued: what lies past a row array that is not held
    idx = [row_index(s, REF_HOLD, R_SHORT) for s in range(S + 1)]
    out = {}
    out["row s + 1"] = oracle_score(case, x, u, rows[:, [min(i + 1, R_SHORT - 1) for i in idx]], w, True)
    out["row s - 1"] = oracle_score(case, x, u, rows[:, [max(i - 1, 0) for i in idx]], w, True)
    out["the rows of b + 1"] = oracle_score(case, x, u, np.roll(win, -1, axis=0), w, True)
    out["the weights of b + 1"] = oracle_score(case, x, u, win, np.roll(w, -1, axis=0), True)
    out["ref_hold ignored"] = oracle_score(case, x, u, window(rows, S, 1), w, True)
    out["q and qf exchanged"] = oracle_score(case, x, u, win, w, True, exchange_q_qf=True)
    w_r = w.copy()
    w_r[:, 2 * n:] = wc.base_row(model).astype(np.float32)[2 * n:]  # the shared block's r in place of the row's
    out["r ignored"] = oracle_score(case, x, u, win, w_r, True)
    out["terminal flag ignored"] = oracle_score(case, x, u, win, w, False)
    out["last row not held"] = oracle_score(case, x, u, long_rows[:, [(s // REF_HOLD) * REF_HOLD for s in range(S + 1)]], w, True)
    return out


def moves(got, true):
    """-> (largest relative change of one step's cost, relative change of the total), per trajectory (B,) each.  A slot whose true
    value is zero counts by its absolute change over the trajectory's mean stage cost."""
    (gs, gt), (ts, tt) = got, true
    den = np.where(ts != 0.0, np.abs(ts), np.mean(np.abs(ts), axis=1, keepdims=True))
    return np.max(np.abs(gs - ts) / den, axis=1), np.abs(gt - tt) / np.abs(tt)
