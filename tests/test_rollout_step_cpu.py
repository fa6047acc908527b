"""The teeth of tests/test_rollout_step_gpu.py (part 3), on the CPU: at the shapes that file compares with the fp64 oracle --
B in {1, 17} x N in {1, 2, 3}, quadrotor, both `skew` sets, both integrators -- every single-parameter mutant of
param_cases.MUTANTS whose parameter enters the rollouts moves a compared quantity past the bound asserted on it there."""
import pytest

import param_cases as pc

MODEL = "quadrotor"
CASES = [(sn, integ) for sn in pc.SET_NAMES[MODEL] for integ in ("euler", "rk4")]
ORACLE_SHAPES = [(B, N) for N in (1, 2, 3) for B in (1, 17)]      # test_rollout_step_gpu.ORACLE_SHAPES


@pytest.mark.parametrize("sn,integ", CASES)
def test_every_rollout_mutant_exceeds_the_bounds_at_these_shapes(sn, integ):
    """fp64 oracle alone, no device: at every shape of ORACLE_SHAPES each single-parameter mutant whose parameter enters the
    rollouts moves at least one compared quantity of that family (sim_x, sim_cost, total_cost, cl_x, cl_u, cl_cost) past the
    bound asserted on it above -- about the true nominal and with the true gains, as a kernel with that mistake would."""
    for B, N in ORACLE_SHAPES:
        x0, u = pc.inputs(MODEL, sn, N, B)
        true = pc.evaluate(pc.spec(MODEL, sn, integ), x0, u)
        for name, _, fams in pc.MUTANTS[MODEL]:
            p, _, noop = pc.mutate(MODEL, sn, name)
            if noop or "rollout" not in fams:
                continue
            mut = pc.evaluate(pc.spec_from(MODEL, p, integ), x0, u, nominal=true["sim_x"], gains=(true["k"], true["K"]))
            ratio, which = max((pc.change(q, mut[q], true[q]) / pc.BOUNDS[q], q) for q in pc.FAMILIES["rollout"])
            assert ratio > 1.0, (B, N, name, which, ratio)
