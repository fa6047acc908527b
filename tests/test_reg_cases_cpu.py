"""tests/reg_cases.py on the CPU, on the fp64 oracle alone (no GPU marker): what tests/test_reg_gpu.py asserts can tell a sweep
that states `reg` wrongly from a right one, and its bounds are not the kernel's.

  1. reg_cases.sweep(mutant=None) is oracle.ilqr.riccati_sweep_batched bit for bit, and oracle.ilqr.optimize carries `reg`;
  2. teeth: at reg_cases.REGS every mutant outside NOOPS moves max(change(K), change(k)) by >= 10 x the asserted bound in every
     case (set x integrator x N in {2, 7, 26}, full batch) and by >= 100 x in at least one shape of every (set, integrator); the
     same table at QUU_REG is printed, not asserted: what the suite could see before;
  3. the values are visible (K moves by > 1e-2 against QUU_REG), Q_uu + reg I is conditioned no worse than at QUU_REG, and
     Q_uu is positive definite with healthy pivots at reg = 0, so a status bit on the GPU is the kernel's fault;
  4. fp32 NumPy against fp64 at REGS and at 0 stays inside a quarter of the K / k bounds: 5e-6 holds on the device unchanged;
  5. SOLVE_E_REG: fp32-storage emulation against optimize(reg=...), iteration counts within one.
"""
import numpy as np
import pytest

import param_cases as pc
import reg_cases as rc
from oracle import ilqr as o_ilqr

SETS = [(model, sn) for model in pc.MODELS for sn in pc.SET_NAMES[model]]
BOUND = pc.BOUNDS["K"]
assert pc.BOUNDS["k"] == BOUND


# ------------------------------------------------------------------------------------------------ 1. the sweep is the oracle's
@pytest.mark.parametrize("model,sn", SETS)
def test_unmutated_sweep_is_the_oracles_bit_for_bit(model, sn):
    """np.array_equal on k and K, fp64 and fp32, at REGS, 0 and QUU_REG, N = 1 included."""
    for integ in rc.INTEGRATORS:
        for N in (1,) + rc.SWEEP_HORIZONS:
            blk = rc.blocks(model, sn, integ, N)
            for reg in rc.SWEEP_REGS[(model, sn)] + (rc.QUU_REG,):
                for dtype in (np.float64, np.float32):
                    got, ref = rc.sweep(blk, reg, dtype=dtype), o_ilqr.riccati_sweep_batched(blk, reg=reg, dtype=dtype)
                    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (integ, N, reg, dtype)


def test_backward_pass_and_optimize_carry_reg():
    """oracle.ilqr.backward_pass(reg=) is riccati_sweep(reg=) on its own finite differences, the default is QUU_REG, and
    optimize(reg=) hands the value to the backward pass of its first iteration."""
    sp = pc.spec("cartpole", "skew", "euler")
    x0, u0 = pc.inputs("cartpole", "skew", 7, 1)
    xs = o_ilqr.rollout(sp.f, x0[0], list(u0[0]))
    d = o_ilqr.linearize_fd(sp.f, sp.L, sp.Lf, xs, list(u0[0]))
    reg = rc.REGS[("cartpole", "skew")]
    for r in (reg, 0.0):
        k, K = o_ilqr.backward_pass(sp.f, sp.L, sp.Lf, xs, list(u0[0]), reg=r)
        kr, Kr = o_ilqr.riccati_sweep(d, reg=r)
        assert np.array_equal(np.array(k), kr) and np.array_equal(np.array(K), Kr)
    k, K = o_ilqr.backward_pass(sp.f, sp.L, sp.Lf, xs, list(u0[0]))
    kd, Kd = o_ilqr.riccati_sweep(d, reg=o_ilqr.QUU_REG)
    assert np.array_equal(np.array(K), Kd) and not np.array_equal(Kd, Kr)
    _, _, logs = o_ilqr.optimize(sp.f, sp.L, sp.Lf, x0[0], list(u0[0]), 7, max_iter=1, reg=reg)
    kr, Kr = o_ilqr.riccati_sweep(d, reg=reg)
    assert np.array_equal(np.array(logs[0]["K_seq"]), Kr) and np.array_equal(np.array(logs[0]["k_seq"]), kr)


# ------------------------------------------------------------------------------------------------ 2. teeth
def _table(model, sn, integ, reg):
    """{(mutant, N): max(change(K), change(k)) / bound} for every pair outside NOOPS, against the right sweep at the same reg."""
    out = {}
    for N in rc.SWEEP_HORIZONS:
        blk = rc.blocks(model, sn, integ, N)
        ref = rc.sweep(blk, reg)
        for mu in rc.MUTANTS:
            if (mu, (model, sn, integ, N)) not in rc.NOOPS:
                out[(mu, N)] = rc.gain_change(rc.sweep(blk, reg, mu), ref) / BOUND
    return out


def _print_table(tag, table):
    for mu in rc.MUTANTS:
        row = "  ".join(f"N={N}: {table[(mu, N)]:9.3g}" if (mu, N) in table else f"N={N}:         -" for N in rc.SWEEP_HORIZONS)
        print(f"[{tag}] {mu:16s} {row}")


@pytest.mark.parametrize("integ", rc.INTEGRATORS)
@pytest.mark.parametrize("model,sn", SETS)
def test_every_mutant_stands_above_the_bound_at_regs(model, sn, integ):
    """The two conditions of the module docstring, in units of the bound (5e-6).  Measured at REGS = 1e-2, smallest entry of
    each set over both integrators: quadrotor skew 7.1e3 (V_reg, N = 2), skew_nobarrier 1.0e4 (Vxx_reg, N = 2), cart-pole skew
    5.6e3 (V_reg, N = 2), skew_barrier 24 (V_reg, V_sign, Vxx_reg at N = 2; N = 7: 1.1e3); the reg-placement mutants stand at
    2.5e4 ... 2.4e5 everywhere.  At QUU_REG (printed only) the same table reads V_reg / V_sign / Vxx_reg 0.005 ... 8.4, Vx_reg
    0.6 ... 14, reg_twice, first_pivot, all_entries, first_step_only 2.8 ... 24 and fixed_default exactly 0: in fp64, before
    any fp32 round-off is added, the suite could see the placement mistakes at a few times its bound in some cases and a loop
    that ignores the argument not at all.  The pair of reg_cases.WEAK (Vx_reg, cart-pole skew_barrier, N = 2: 8.0 / 8.7) is
    printed and held above its floor."""
    reg = rc.REGS[(model, sn)]
    at_reg, at_default = _table(model, sn, integ, reg), _table(model, sn, integ, rc.QUU_REG)
    _print_table(f"{model} {sn} {integ} reg={reg:g}", at_reg)
    _print_table(f"{model} {sn} {integ} reg={rc.QUU_REG:g} (not asserted)", at_default)
    low = {key: r for key, r in at_reg.items() if not r >= 10.0}
    assert not low, low
    for mu in rc.MUTANTS:
        if all((mu, (model, sn, integ, N)) in rc.NOOPS for N in rc.SWEEP_HORIZONS):
            continue                                            # first_pivot, all_entries with m = 1
        best = max(r for (mu_, _), r in at_reg.items() if mu_ == mu)
        assert best >= 100.0, (mu, best)
    for (mu, case), floor in rc.WEAK.items():
        if case[:3] == (model, sn, integ):
            blk = rc.blocks(*case)
            r = rc.gain_change(rc.sweep(blk, reg, mu), rc.sweep(blk, reg)) / BOUND
            print(f"[{model} {sn} {integ} reg={reg:g}] weak pair {mu} N={case[3]}: {r:.3g} (listed in NOOPS, floor {floor})")
            assert floor <= r < 10.0, (mu, case, r)            # still above the bound, and still rightly on the list


def test_the_weak_pair_is_weak_at_every_reg():
    """reg_cases.WEAK is on the list because no value lifts it, not because 1e-2 is a poor choice: Vx_reg on the cart-pole
    skew_barrier set at N = 2 over reg_cases.WEAK_SCAN stays below 10 x the bound (and above it).  Measured, Euler / RK4:
    6.4 / 7.1 at 5e-3, 8.0 / 8.7 at 1e-2, 8.1 / 8.8 at 1.2e-2, 6.6 / 7.1 at 3e-2, 2.8 / 3.0 at 1e-1."""
    for (mu, case) in rc.WEAK:
        blk = rc.blocks(*case)
        row = {reg: rc.gain_change(rc.sweep(blk, reg, mu), rc.sweep(blk, reg)) / BOUND for reg in rc.WEAK_SCAN}
        print(f"[weak pair {mu} {case}] " + "  ".join(f"reg={reg:g}: {r:.2g}" for reg, r in row.items()))
        assert all(1.0 < r < 10.0 for r in row.values()), (mu, case, row)


def test_noops_are_no_ops_and_nothing_else_is_listed():
    """Every listed pair is an exact no-op (the mutant's gains equal the right ones bit for bit) or a pair of reg_cases.WEAK;
    the list holds the enumerated kinds only."""
    for mu, case in rc.NOOPS:
        model, sn, integ, N = case
        if (mu, case) in rc.WEAK:
            assert mu == "Vx_reg" and (model, sn, N) == ("cartpole", "skew_barrier", 2)
            continue
        assert (N == 1 and mu in rc.V_MUTANTS + ("first_step_only",)) or \
            (model == "cartpole" and mu in ("first_pivot", "all_entries")), (mu, case)
        blk = rc.blocks(*case)
        reg = rc.REGS[(model, sn)]
        got, ref = rc.sweep(blk, reg, mu), rc.sweep(blk, reg)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (mu, case)
    assert set(mu for mu, _ in rc.NOOPS) <= set(rc.MUTANTS)


# ------------------------------------------------------------------------------------------------ 3. visible, well-posed
@pytest.mark.parametrize("model,sn", SETS)
def test_regs_are_visible_and_well_conditioned(model, sn):
    """K at REGS against K at QUU_REG moves by > 1e-2 in every case (measured: 0.17 ... 0.55); the largest condition number of
    Q_uu + reg I is no worse than at QUU_REG (quadrotor skew: 8.8e3 ... 1.2e4 -> 7.2e3 ... 9.3e3, skew_nobarrier: 4.4 -> 3.3; cart-pole: 1, m = 1); REGS is of the order of the
    median diagonal of Q_uu (between 1 % of it and the whole); and at reg = 0 every pivot of an elimination of Q_uu without
    pivoting stays above 1e-3 of the diagonal entry it started as, as test_param_cases_cpu.py checks at QUU_REG: the sets need no
    regularisation, so the sweeps at reg = 0 are compared with the oracle at reg = 0."""
    reg = rc.REGS[(model, sn)]
    diag = []
    for integ in rc.INTEGRATORS:
        for N in (1,) + rc.SWEEP_HORIZONS:
            blk = rc.blocks(model, sn, integ, N)
            q_reg, q_def, q_0 = rc.quu(blk, reg), rc.quu(blk, rc.QUU_REG), rc.quu(blk, 0.0)
            moved = pc.change("K", rc.sweep(blk, reg)[1], rc.sweep(blk, rc.QUU_REG)[1])
            c_reg, c_def = float(np.linalg.cond(q_reg).max()), float(np.linalg.cond(q_def).max())
            ratio = pc.unpivoted_pivot_ratio(q_0)
            print(f"[{model} {sn} {integ} N={N}] K(reg={reg:g}) vs K({rc.QUU_REG:g}): {moved:.2e}; cond {c_reg:.3g} "
                  f"(at {rc.QUU_REG:g}: {c_def:.3g}); smallest unpivoted pivot ratio at reg = 0: {ratio:.3g}")
            assert moved > 1e-2 and c_reg <= c_def, (integ, N, moved, c_reg, c_def)
            assert ratio > 1e-3 and float(np.linalg.eigvalsh(q_0).min()) > 0.0, (integ, N, ratio)
            if N > 1:
                diag.append(np.diagonal(q_0, axis1=-2, axis2=-1).ravel())
    med = float(np.median(np.concatenate(diag)))
    print(f"[{model} {sn}] median diagonal of Q_uu: {med:.3g}, reg {reg:g}")
    assert 0.95 * rc.MEDIAN_QUU[(model, sn)] <= med <= 1.05 * rc.MEDIAN_QUU[(model, sn)]
    assert 0.01 * med <= reg <= med


# ------------------------------------------------------------------------------------------------ 4. fp32 keeps the bound
def test_fp32_sweep_keeps_a_quarter_of_the_bound():
    """The fp32 NumPy sweep against the fp64 one on the same blocks, every case, N in {1, 2, 7, 26}, at REGS and at 0: K and k
    within BOUNDS / 4 = 1.25e-6, the rule of tests/test_user_grid_cpu.py under which the device keeps 5e-6.  The worst figures
    are the ones stored in reg_cases.FP32_SWEEP (measurements: held from both sides)."""
    worst = {"REGS": [0.0, 0.0], 0.0: [0.0, 0.0]}
    for model, sn in SETS:
        for integ in rc.INTEGRATORS:
            for N in (1,) + rc.SWEEP_HORIZONS:
                blk = rc.blocks(model, sn, integ, N)
                for reg, key in zip(rc.SWEEP_REGS[(model, sn)], ("REGS", 0.0)):
                    k64, K64 = rc.sweep(blk, reg)
                    k32, K32 = rc.sweep(blk, reg, dtype=np.float32)
                    eK, ek = pc.change("K", K32, K64), pc.change("k", k32, k64)
                    worst[key] = [max(worst[key][0], eK), max(worst[key][1], ek)]
                    assert eK <= 0.25 * BOUND and ek <= 0.25 * BOUND, (model, sn, integ, N, reg, eK, ek)
    print(f"fp32 NumPy sweep vs fp64: {worst}")
    for key, (eK, ek) in worst.items():
        sK, sk = rc.FP32_SWEEP[key]
        assert 0.5 * sK <= eK <= sK and 0.5 * sk <= ek <= sk, (key, eK, ek)


# ------------------------------------------------------------------------------------------------ 5. whole solves
@pytest.mark.parametrize("model", pc.MODELS)
def test_solve_bounds_at_regs(model):
    """reg_cases.SOLVE_E_REG is what it says: pc.solve_emulated(reg=REGS) (exact derivatives, fp32 storage) against
    oracle.ilqr.optimize(reg=REGS) on the `skew` set, N = 7, both integrators, trajectories SOLVE_TRAJ: both finish inside
    SOLVE_MAX_ITER with iteration counts within one of each other, no trajectory left out, and where the counts are equal cost,
    x, u are within SOLVE_E_REG and no smaller than half of it.  The fp64-storage emulation is printed beside it."""
    reg = rc.REGS[(model, "skew")]
    worst, same = dict(cost=0.0, x=0.0, u=0.0), 0
    for integ in rc.INTEGRATORS:
        sp = pc.spec(model, "skew", integ)
        x0, u0 = pc.inputs(model, "skew", pc.SOLVE_N, pc.SOLVE_B)
        for b in pc.SOLVE_TRAJ:
            ref = rc.solve_optimize(sp, x0[b], u0[b], reg)
            emu = rc.solve_emulated(sp, x0[b], u0[b], reg)
            errs = pc.solve_errors(emu, ref)
            print(f"[{model} {integ} b={b} reg={reg:g}] iterations optimize {ref[3]} emulation {emu[3]}: {errs}")
            assert abs(emu[3] - ref[3]) <= 1 and 1 < ref[3] < pc.SOLVE_MAX_ITER and emu[3] < pc.SOLVE_MAX_ITER, (integ, b, emu[3], ref[3])
            if emu[3] == ref[3]:
                same += 1
                for key, e in errs.items():
                    worst[key] = max(worst[key], e)
    print(f"fp32-storage emulation vs optimize(reg={reg:g}), {model}: {worst}, equal iteration counts on {same} of "
          f"{2 * len(pc.SOLVE_TRAJ)}")
    assert same >= 2 * len(pc.SOLVE_TRAJ) - 1
    for key, e in worst.items():
        assert 0.5 * rc.SOLVE_E_REG[model][key] <= e <= rc.SOLVE_E_REG[model][key], (key, e)
