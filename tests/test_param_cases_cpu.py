"""The parameter sets of tests/param_cases.py on the CPU, all fp64 (no GPU marker):

  1. the oracle (oracle/models.py, oracle/linearize.py) against the reference evaluated at the `skew` sets (G16);
  2. the oracle's analytic derivatives against central differences at every set, which covers what the reference cannot
     vouch for: k_yaw = 0.017 and the cart-pole's barrier;
  3. teeth: every single-parameter mutant moves what tests/test_model_params_gpu.py compares by >= 100 x the bound asserted
     there, in every family of kernels its parameter enters;
  4. well-posedness: no pivot of Q_uu + reg I comes near zero, so a status bit on the GPU is a failure of the kernel;
  5. the figures the GPU test's bounds on the converged solve are derived from: fp32 storage against oracle.ilqr.optimize.
"""
import functools

import numpy as np
import pytest

import param_cases as pc
from conftest import load_golden, rel_fro
from oracle import ilqr as o_ilqr
from oracle import linearize as o_lin

CASES = [(model, sn, integ) for model in pc.MODELS for sn in pc.SET_NAMES[model] for integ in ("euler", "rk4")]


@functools.lru_cache(maxsize=None)
def _true(model, sn, integ, N):
    x0, u = pc.inputs(model, sn, N)
    return x0, u, pc.evaluate(pc.spec(model, sn, integ), x0, u)


# ------------------------------------------------------------------------------------------------ 1. oracle vs reference (G16)
@pytest.mark.parametrize("model", pc.MODELS)
def test_oracle_matches_the_reference_at_the_skewed_parameters(model):
    """The bounds of test_oracle_golden.py::test_dynamics_and_costs_match_reference (G1/G2) on the G16 fixture.  The fixture
    was made with the `skew` set, except k_yaw (a constant of the reference's rate function): checked against what it stores."""
    g = load_golden(f"dyn_cost_params_{model}.npz")
    p = pc.params(model, "skew")
    want_phys = dict(p["phys"], k_yaw=0.01) if model == "quadrotor" else dict(p["phys"])
    assert np.array_equal(g["phys"], [want_phys[k] for k in pc.PHYS_NAMES[model]])
    for key in ("x_ref", "q", "r", "qf"):
        assert np.array_equal(g[key], p[key]), key
    assert float(g["dt"]) == p["dt"] and float(g["barrier_alpha"]) == p["barrier_alpha"]
    assert float(g["barrier_beta"]) == p["barrier_beta"]
    p["phys"] = want_phys
    se, sr = pc.spec_from(model, p, "euler"), pc.spec_from(model, p, "rk4")
    for i in range(g["x"].shape[0]):
        x, u = g["x"][i], g["u"][i]
        assert np.max(np.abs(se.f(x, u) - g["f_euler"][i])) <= 1e-15
        assert np.max(np.abs(sr.f(x, u) - g["f_rk4"][i])) <= 1e-15
        assert se.L(x, u) == g["L"][i]
        assert se.Lf(x) == g["Lf"][i]
    assert np.max(np.abs(o_lin.step(se, g["x"], g["u"]) - g["f_euler"])) < 1e-13
    assert np.max(np.abs(o_lin.step(sr, g["x"], g["u"]) - g["f_rk4"])) < 1e-13
    assert np.max(np.abs(o_lin.stage_cost(se, g["x"], g["u"]) - g["L"]) / np.abs(g["L"])) < 1e-12
    assert np.max(np.abs(o_lin.terminal_cost(se, g["x"]) - g["Lf"]) / np.abs(g["Lf"])) < 1e-12
    if model == "quadrotor":
        assert np.mean(g["u"] < 0) > 0.03           # the barrier is live at some of the points


def test_running_cost_applies_the_barrier_to_either_model():
    """oracle.models.running_cost follows include/quattro_hip.h: the barrier goes with barrier_alpha != 0, cart-pole included."""
    for integ in ("euler",):
        sp = pc.spec("cartpole", "skew_barrier", integ)
        x0, u = pc.inputs("cartpole", "skew_barrier", 7)
        plain = pc.spec_from("cartpole", dict(pc.params("cartpole", "skew_barrier"), barrier_alpha=0.0), integ)
        for b in range(x0.shape[0]):
            L = sp.L(x0[b], u[b, 0])
            assert isinstance(L, float)
            assert abs(L - float(o_lin.stage_cost(sp, x0[b], u[b, 0]))) <= 1e-12 * abs(L)
            assert L > plain.L(x0[b], u[b, 0])


# ------------------------------------------------------------------------------------------------ 2. analytic vs finite differences
FD_H = 1e-6


def _central(fn, z, h=FD_H):
    """d fn / d z by central differences along the last axis of z: (..., out, len z)."""
    cols = []
    for i in range(z.shape[-1]):
        e = np.zeros(z.shape[-1]); e[i] = h
        cols.append((fn(z + e) - fn(z - e)) / (2.0 * h))
    return np.stack(cols, axis=-1)


@pytest.mark.parametrize("model,sn,integ", CASES)
def test_analytic_derivatives_against_central_differences(model, sn, integ):
    """oracle.linearize.linearize_analytic against central differences with step 1e-6, at the states and controls of the N = 7
    nominal of every set (133 quadrotor / 63 cart-pole points), per block, each block against its own norm:

      first derivatives   A, B (and the body-rate rows of each on their own) from step; l_x, l_u from stage_cost; V_x from
                          terminal_cost: 1e-6
      second derivatives  l_xx, l_uu, l_ux, V_xx as central differences of the analytic l_x, l_u, V_x that the lines above have
                          just checked against the cost itself: 1e-4.  (A second difference of the cost with this step has a
                          round-off of 4 eps |L| / (4 h^2) ~ 0.1: it cannot see a Hessian.  The chain cost -> gradient ->
                          Hessian has eps |l_x| / h ~ 1e-8 at each link.)

    Measured: first derivatives <= 1.4e-8 (worst: l_u of skew_nobarrier, whose entries 2 r u are small against the cost's
    round-off divided by h), second derivatives <= 2e-10."""
    x0, u, true = _true(model, sn, integ, 7)
    sp = pc.spec(model, sn, integ)
    xs, n, m = true["sim_x"], sp.n, sp.m
    fd = dict(
        A=_central(lambda z: o_lin.step(sp, z, u), xs[:, :-1]), B=_central(lambda z: o_lin.step(sp, xs[:, :-1], z), u),
        lx=_central(lambda z: o_lin.stage_cost(sp, z, u)[..., None], xs[:, :-1])[..., 0, :],
        lu=_central(lambda z: o_lin.stage_cost(sp, xs[:, :-1], z)[..., None], u)[..., 0, :],
        VxN=_central(lambda z: o_lin.terminal_cost(sp, z)[..., None], xs[:, -1])[..., 0, :],
        lxx=_central(lambda z: o_lin.stage_cost_derivs(sp, z, u)[0], xs[:, :-1]),
        luu=_central(lambda z: o_lin.stage_cost_derivs(sp, xs[:, :-1], z)[1], u),
        lux=_central(lambda z: o_lin.stage_cost_derivs(sp, z, u)[1], xs[:, :-1]),
        VxxN=_central(lambda z: o_lin.terminal_derivs(sp, z)[0], xs[:, -1]))
    if model == "quadrotor":
        fd.update(pc.sub_blocks(fd))
    worst = {1: 0.0, 2: 0.0}
    for key, got in fd.items():
        order = 2 if key in ("lxx", "luu", "lux", "VxxN") else 1
        assert got.shape == true[key].shape, key
        if key == "lux":
            assert not true[key].any() and np.max(np.abs(got)) < 1e-4      # identically zero: nothing to be relative to
            continue
        e = rel_fro(true[key], got)
        worst[order] = max(worst[order], e)
        assert e < (1e-6 if order == 1 else 1e-4), (key, e)
    print(f"analytic vs central differences {model} {sn} {integ}: first {worst[1]:.1e} second {worst[2]:.1e}")


# ------------------------------------------------------------------------------------------------ 3. teeth
@pytest.mark.parametrize("model,sn,integ", CASES)
@pytest.mark.parametrize("N", [7, 26])
def test_every_mutant_is_detected_in_every_family_its_parameter_enters(model, sn, integ, N):
    """For every mutant of param_cases.MUTANTS: simulate x and cost, the total cost of the nominal, every record block (and the
    body-rate rows of A and B), the terminal pair, K, k (and their barrier rows) and the alpha = 1 closed-loop x, u, cost, once
    with the true spec and once with the mutant's, on the inputs of the GPU tests at the full batch.  The mutant is evaluated
    as a kernel with that mistake would be: about the true nominal and with the true gains.  In every family its parameter
    enters -- rollouts, records, gains -- at least one quantity moves by >= 100 x the bound the GPU test asserts on it.

    N = 1 is left out: a one-step horizon's single gain is made of l_u, l_uu, B and V(N) alone, so q does not enter it.  An edit
    that changes nothing in a set (barrier_beta while barrier_alpha is 0) is no mutant there; test_no_mutant_is_idle checks
    that each is one somewhere."""
    x0, u, true = _true(model, sn, integ, N)
    for name, _, _ in pc.MUTANTS[model]:
        p, fams, noop = pc.mutate(model, sn, name)
        if noop:
            continue
        mut = pc.evaluate(pc.spec_from(model, p, integ), x0, u, nominal=true["sim_x"], gains=(true["k"], true["K"]))
        for fam in fams:
            ratio, which = max((pc.change(q, mut[q], true[q]) / pc.BOUNDS[q], q) for q in pc.FAMILIES[fam] if q in true)
            assert ratio >= 100.0, (name, fam, which, ratio)
        if name == "swap r0,r3" and sn == "skew_nobarrier":
            # without the barrier r alone is l_uu (under `skew` the barrier hides this swap: l_uu moves 2.2e-4)
            assert pc.change("luu", mut["luu"], true["luu"]) >= 100.0 * pc.BOUNDS["luu"]


@pytest.mark.parametrize("model", pc.MODELS)
def test_no_mutant_is_idle(model):
    """Every mutant changes its parameters in at least one set of its model, and every quantity has a bound."""
    for name, _, fams in pc.MUTANTS[model]:
        assert any(not pc.mutate(model, sn, name)[2] for sn in pc.SET_NAMES[model]), name
        assert set(fams) <= set(pc.FAMILIES)
    assert all(q in pc.BOUNDS for qs in pc.FAMILIES.values() for q in qs)


# ------------------------------------------------------------------------------------------------ 4. well-posedness
@pytest.mark.parametrize("model,sn,integ", CASES)
def test_quu_pivots_are_healthy(model, sn, integ):
    """Every pivot of an elimination of the fp64 Q_uu + reg I without pivoting (the order of the tile sweeps) stays above 1e-3 of
    the diagonal entry it started as, at every horizon, segment sweeps from t_start = 3 included (a tail of the same sweep)."""
    for N in pc.HORIZONS:
        x0, u, true = _true(model, sn, integ, N)
        blocks = {k_: true[k_] for k_ in pc.BLOCKS + ("VxN", "VxxN")}
        quu = np.zeros((x0.shape[0], N, true["B"].shape[-1], true["B"].shape[-1]))
        o_ilqr.riccati_sweep_batched(blocks, quu_out=quu)
        ratio = pc.unpivoted_pivot_ratio(quu)
        assert ratio > 1e-3, (N, ratio)
        assert np.all(np.isfinite(true["K"])) and np.all(np.isfinite(true["cl_x"]))


# ------------------------------------------------------------------------------------------------ 5. whole solves
@pytest.mark.parametrize("model", pc.MODELS)
def test_converged_solve_bounds_are_what_the_fp32_emulation_needs(model):
    """param_cases.SOLVE_E, from which the GPU test's bounds on the converged solve come, is what it says: the algorithm with
    exact derivatives and fp32 storage against oracle.ilqr.optimize (fp64, finite differences) on the `skew` set, N = 7, both
    integrators, trajectories 0, 2, 4 -- the same iteration counts, and cost, x, u within SOLVE_E and no smaller than half of
    it (the figures are measurements, not allowances).  In fp64 storage the same comparison gives the same x and u to two
    digits: the gap is the unconverged remainder of a solve that stops on |dJ| < 1e-3, not fp32."""
    worst = dict(cost=0.0, x=0.0, u=0.0)
    for integ in ("euler", "rk4"):
        sp = pc.spec(model, "skew", integ)
        x0, u0 = pc.inputs(model, "skew", pc.SOLVE_N, pc.SOLVE_B)
        for b in pc.SOLVE_TRAJ:
            ref = pc.solve_optimize(sp, x0[b], u0[b])
            emu = pc.solve_emulated(sp, x0[b], u0[b])
            assert emu[3] == ref[3] and 1 < ref[3] < pc.SOLVE_MAX_ITER, (integ, b, emu[3], ref[3])
            for key, e in pc.solve_errors(emu, ref).items():
                worst[key] = max(worst[key], e)
    print(f"fp32-storage emulation vs optimize(), {model}: {worst}")
    for key, e in worst.items():
        assert 0.5 * pc.SOLVE_E[model][key] <= e <= pc.SOLVE_E[model][key], (key, e)
