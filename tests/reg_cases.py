"""The Q_uu regularisation away from 1e-6: the values, the sweep with one mistake at a time, and the solves at those values.
A plain helper module on top of tests/param_cases.py (sets, inputs, spec, device_model, change, BOUNDS, barrier_rows,
solve_errors: used from there, not copied), for

  * tests/test_reg_cases_cpu.py (the sweep below equals the oracle's; every mistake stands >= 10 x above the asserted bound in
    every case and >= 100 x somewhere in every (set, integrator); fp32 NumPy stays inside a quarter of the bound; SOLVE_E_REG),
  * tests/test_reg_gpu.py (every sweep kernel, every loop and the hybrid tail sweep of the C ABI at these values).

The contract (include/quattro_hip.h, oracle.ilqr.riccati_sweep): `reg` goes on the diagonal of Q_uu before the inversion and
nowhere else; the V update takes the unregularised Q_uu.  At the reference's 1e-6 the term reg K is below fp32 resolution of
Q_ux for every set of param_cases, so a sweep that states it wrongly passes every comparison made at the default.
"""
import functools

import numpy as np

import param_cases as pc
from oracle import ilqr as o_ilqr
from oracle import linearize as o_lin

QUU_REG = o_ilqr.QUU_REG

# One visible value per parameter set, chosen on the CPU by the rule of test_reg_cases_cpu.py: every mutant outside NOOPS moves
# max(change(K), change(k)) by >= 10 x BOUNDS in every case (integrator x N in {2, 7, 26}, full batch) and by >= 100 x in at
# least one shape of every (set, integrator); K itself moves by > 1e-2 against the sweep at QUU_REG; the condition number of
# Q_uu + reg I is no worse than at QUU_REG.  Next to each: the median diagonal entry of the oracle's Q_uu over both integrators
# and N in {2, 7, 26} (test_reg_cases_cpu.py::test_regs_are_of_the_order_of_quu prints and asserts them).  reg of that order
# is what makes reg K comparable with Q_ux; reg = 1 collapses the gains and with them the V mistakes (the issue's side note).
REGS = {
    ("quadrotor", "skew"): 1e-2,                # median diag Q_uu 0.141
    ("quadrotor", "skew_nobarrier"): 1e-2,      # median diag Q_uu 0.0422
    ("cartpole", "skew"): 1e-2,                 # median diag Q_uu 0.0131
    ("cartpole", "skew_barrier"): 1e-2,         # median diag Q_uu 0.695 (u < 0 rows: up to 51)
}
MEDIAN_QUU = {("quadrotor", "skew"): 0.141, ("quadrotor", "skew_nobarrier"): 0.0422, ("cartpole", "skew"): 0.0131,
              ("cartpole", "skew_barrier"): 0.695}
SWEEP_REGS = {key: (reg, 0.0) for key, reg in REGS.items()}        # the sweeps also run with no regularisation at all
SWEEP_HORIZONS = (2, 7, 26)                                        # the asserted cases of the teeth test (N = 1: see NOOPS)
INTEGRATORS = ("euler", "rk4")

# The mistakes a sweep can make with `reg`, each one sentence.
MUTANTS = {
    "V_reg": "Q_uu + reg I, not Q_uu, in both V updates (equals the short form V_xx' = Q_xx + Q_ux^T K).",
    "V_sign": "Q_uu - reg I in both V updates: the reg K term of the identity Q_uu K + Q_ux = -reg K with the wrong sign.",
    "Vxx_reg": "Q_uu + reg I in the V_xx update only.",
    "Vx_reg": "Q_uu + reg I in the V_x update only.",
    "reg_twice": "2 reg on the diagonal before the inversion.",
    "first_pivot": "reg on entry (0, 0) of Q_uu only.",
    "all_entries": "reg on every entry of Q_uu, not on its diagonal.",
    "fixed_default": "The sweep runs at 1e-6 whatever it is given.",
    "first_step_only": "reg at the first executed step S - 1 only and 0 at every step after it: a hoisting mistake.",
}
V_MUTANTS = ("V_reg", "V_sign", "Vxx_reg", "Vx_reg")


def cases(model=None):
    """(model, set, integrator, N) over N in {1} + SWEEP_HORIZONS."""
    return [(mo, sn, integ, N) for mo in pc.MODELS if model in (None, mo) for sn in pc.SET_NAMES[mo] for integ in INTEGRATORS
            for N in (1,) + SWEEP_HORIZONS]


# (mutant, case) pairs where a mutant cannot show, enumerated:
#   * every V mutant at N = 1: one step, no V update is ever read;
#   * first_step_only at N = 1: the first executed step is the only one;
#   * first_pivot and all_entries for m = 1 (cart-pole): entry (0, 0) is the whole diagonal and the whole matrix.
#   * WEAK, which is no no-op and is listed for this reason: Vx_reg on the cart-pole `skew_barrier` set at N = 2 never reaches
#     10 x the bound, whatever the value -- 6.4 / 7.1 (Euler / RK4) at reg = 5e-3, 8.0 / 8.7 at 1e-2, 8.1 / 8.8 at 1.2e-2 (the
#     peak), 6.6 / 7.1 at 3e-2, 2.8 / 3.0 at 1e-1.  The wrong term reg K_1^T k_1 enters k_0 alone, K_1 = B^T V_xx A / Q_uu is
#     small over one step of dt = 0.004 under a barrier-dominated Q_uu (0.008 ... 51), and the relative Frobenius norm of k is
#     carried by the rows with u < 0.  Changing the set's reg, as the rule asks, cannot lift it; the same mutant reads 1.1e3 x
#     at N = 7 and V_reg, which contains it, 24 x at this very shape.  The CPU test prints it and holds it above `floor` x the
#     bound (it is visible, only not ten-fold).
WEAK_SCAN = (5e-3, 1e-2, 1.2e-2, 3e-2, 1e-1)                      # the values quoted above; the CPU test prints the pair at each
WEAK = {("Vx_reg", ("cartpole", "skew_barrier", integ, 2)): 5.0 for integ in INTEGRATORS}
NOOPS = frozenset(
    [(mu, c) for mu in V_MUTANTS + ("first_step_only",) for c in cases() if c[3] == 1]
    + [(mu, c) for mu in ("first_pivot", "all_entries") for c in cases("cartpole")]
    + list(WEAK))


def sweep(blocks, reg, mutant=None, dtype=np.float64):
    """The recursion of oracle.ilqr.riccati_sweep_batched, statement for statement, with the mistakes of MUTANTS switchable.
    mutant=None returns that function's arrays bit for bit.  -> k (Bt, S, m), K (Bt, S, m, n)."""
    assert mutant is None or mutant in MUTANTS, mutant
    d = blocks
    A = d["A"].astype(dtype); Bm = d["B"].astype(dtype)
    lx = d["lx"].astype(dtype); lu = d["lu"].astype(dtype)
    lxx = d["lxx"].astype(dtype); luu = d["luu"].astype(dtype); lux = d["lux"].astype(dtype)
    Vx = d["VxN"].astype(dtype); Vxx = d["VxxN"].astype(dtype)
    Bt, S, n, m = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3]
    k_out = np.zeros((Bt, S, m), dtype=dtype)
    K_out = np.zeros((Bt, S, m, n), dtype=dtype)
    eye = np.eye(m, dtype=dtype)
    T = lambda M: np.swapaxes(M, -1, -2)
    mv = lambda M, v: np.einsum("bij,bj->bi", M, v)
    e00 = np.zeros((m, m), dtype=dtype); e00[0, 0] = 1
    for s in reversed(range(S)):
        At, Bt_ = T(A[:, s]), T(Bm[:, s])
        Qx = lx[:, s] + mv(At, Vx)
        Qu = lu[:, s] + mv(Bt_, Vx)
        Qxx = lxx[:, s] + At @ Vxx @ A[:, s]
        Qux = lux[:, s] + Bt_ @ Vxx @ A[:, s]
        Quu = luu[:, s] + Bt_ @ Vxx @ Bm[:, s]
        if mutant == "reg_twice":
            Qreg = Quu + dtype(2.0 * reg) * eye
        elif mutant == "first_pivot":
            Qreg = Quu + dtype(reg) * e00
        elif mutant == "all_entries":
            Qreg = Quu + dtype(reg) * np.ones((m, m), dtype=dtype)
        elif mutant == "fixed_default":
            Qreg = Quu + dtype(QUU_REG) * eye
        elif mutant == "first_step_only":
            Qreg = Quu + dtype(reg if s == S - 1 else 0.0) * eye
        else:
            Qreg = Quu + dtype(reg) * eye
        W = np.linalg.inv(Qreg)
        k = -mv(W, Qu)
        K = -(W @ Qux)
        k_out[:, s] = k
        K_out[:, s] = K
        Quu_x = Quu_xx = Quu
        if mutant in ("V_reg", "Vx_reg"):
            Quu_x = Quu + dtype(reg) * eye
        if mutant in ("V_reg", "Vxx_reg"):
            Quu_xx = Quu + dtype(reg) * eye
        if mutant == "V_sign":
            Quu_x = Quu_xx = Quu - dtype(reg) * eye
        Vx = Qx + mv(T(K) @ Quu_x, k) + mv(T(K), Qu) + mv(T(Qux), k)
        Vxx = Qxx + T(K) @ Quu_xx @ K + T(K) @ Qux + T(Qux) @ K
        Vxx = dtype(0.5) * (Vxx + T(Vxx))
    return k_out, K_out


@functools.lru_cache(maxsize=None)
def blocks(model, sn, integ, N):
    """The oracle's derivative blocks about the fp64 nominal of pc.inputs at the full batch (read-only: shared by the tests)."""
    x0, u = pc.inputs(model, sn, N)
    sp = pc.spec(model, sn, integ)
    xs, _ = o_lin.rollout_batched(sp, x0, u)
    out = o_lin.linearize_analytic(sp, xs, u)
    for v in out.values():
        v.setflags(write=False)
    return out


def gain_change(got, ref):
    """max(change(K), change(k)) of two (k, K) pairs: the figure the teeth conditions are stated in."""
    return max(pc.change("K", got[1], ref[1]), pc.change("k", got[0], ref[0]))


def quu(blk, reg):
    """Q_uu + reg I of every step of the fp64 sweep at `reg`: (Bt, S, m, m)."""
    out = np.zeros(blk["B"].shape[:2] + (blk["B"].shape[-1],) * 2)
    o_ilqr.riccati_sweep_batched(blk, reg=reg, quu_out=out)
    return out


# ---------------------------------------------------------------------------------------------------------------- bounds
# K and k on the device are asserted at param_cases.BOUNDS (5e-6) unchanged.  That is licensed by the fp32 NumPy sweep against
# fp64 on the same blocks staying inside a quarter of it (the rule of tests/test_user_grid_cpu.py), worst over every case and
# N in {1, 2, 7, 26}; test_reg_cases_cpu.py::test_fp32_sweep_keeps_a_quarter_of_the_bound asserts these stored figures:
FP32_SWEEP = {                                  # reg -> (K, k), worst over all sets
    "REGS": (8.8e-7, 9.7e-7),
    0.0: (9.3e-7, 1.07e-6),
}

# ---------------------------------------------------------------------------------------------------------------- whole solves
# As param_cases.SOLVE_E, at REGS: the algorithm with exact derivatives and fp32 storage (pc.solve_emulated(reg=...)) against
# oracle.ilqr.optimize(reg=...) on the `skew` set, N = SOLVE_N, worst over both integrators and SOLVE_TRAJ.  Measured on the CPU
# by test_reg_cases_cpu.py::test_solve_bounds_at_regs, which holds the emulation to these figures.  Asserted on the GPU:
# max(SOLVE_START, 4 x SOLVE_E_REG).
SOLVE_E_REG = {"quadrotor": dict(cost=3.7e-8, x=2.9e-6, u=2.0e-5), "cartpole": dict(cost=2.0e-8, x=7.0e-7, u=3.7e-5)}


def solve_bounds(model):
    return {key: max(pc.SOLVE_START[key], 4.0 * SOLVE_E_REG[model][key]) for key in pc.SOLVE_START}


def solve_optimize(sp, x0, u0, reg):
    return pc.solve_optimize(sp, x0, u0, reg=reg)


def solve_emulated(sp, x0, u0, reg, dtype=np.float32):
    return pc.solve_emulated(sp, x0, u0, dtype=dtype, reg=reg)
