"""tests/hybrid_cases.py on the CPU: its fp64 composition of one hybrid backward pass is the reference's (oracle.ilqr.optimize with a
spying predictor), every named mutant of it moves what tests/test_hybrid_parity_gpu.py asserts by a stated multiple of that
assertion's bound, and the cases are what the GPU test needs them to be (finite closed loops, one trajectory that stops after the first
iteration and one that goes on, decidable line searches).
"""
import numpy as np
import pytest

import hybrid_cases as hc
from conftest import rel_fro
from oracle import ilqr as o_ilqr

CASE_PRECISIONS = [(name, prec) for name in hc.NAMES for prec in hc.precisions(name)]
IDS = [f"{name}-{prec}" for name, prec in CASE_PRECISIONS]


@pytest.mark.parametrize("name", [n for n in hc.NAMES if "like" not in hc.SHAPES[n]])
def test_reference_is_the_oracle_optimizers_first_iteration(name):
    """oracle.ilqr.optimize(max_iter = 1) with a predictor that records what it is handed: the same x_err (1e-12), the same prompt
    and swept rows within the tolerance of its finite differences against exact derivatives, and a stack with the predicted rows in
    the same rows (exactly: the spy answers with the reference's own prediction) and the swept rows in the same rows."""
    cs = hc.case(name)
    prec = hc.precisions(name)[0]
    x = cs.plant.rollout(cs.x0, cs.u)[0]
    ref = hc.compose(cs, x, cs.u, prec)
    stacks = []
    real = o_ilqr.closed_loop_rollout

    def recording(f, L, Lf, x0, x_seq, u_seq, k_seq, K_seq, alpha=1.0):
        stacks.append((np.array(k_seq), np.array(K_seq)))
        return real(f, L, Lf, x0, x_seq, u_seq, k_seq, K_seq, alpha)

    o_ilqr.closed_loop_rollout = recording
    try:
        for b in range(hc.B):
            seen = {}

            def spy(x_err, prompt, b=b, seen=seen):
                seen.update(x_err=np.array(x_err), prompt=np.array(prompt))
                return ref["pred"][b]

            del stacks[:]
            _, _, logs = o_ilqr.optimize(cs.plant.f, cs.plant.L, cs.plant.Lf, cs.x0[b], list(cs.u[b]), cs.N, x_ref=cs.x_ref_arg,
                                         max_iter=1, tf_predict=spy, tf_window=cs.P, state_offset=cs.offset)
            assert len(logs) == 1
            assert np.max(np.abs(seen["x_err"] - ref["x_err"][b])) < 1e-12
            assert seen["prompt"].shape == ref["prompt"][b].shape == (cs.P, cs.c)
            assert rel_fro(seen["prompt"], ref["prompt"][b]) < hc.FD_TOL
            k_st, K_st = stacks[0]
            assert k_st.shape[0] == cs.T + cs.S and len(stacks) >= 1
            assert np.array_equal(k_st[:cs.Tn], ref["k"][b, :cs.Tn]) and np.array_equal(K_st[:cs.Tn], ref["K"][b, :cs.Tn])
            if cs.keep:
                r = slice(cs.Tn, cs.Tn + cs.keep)
                assert rel_fro(K_st[r], ref["K"][b, r]) < hc.FD_TOL
                den = max(np.linalg.norm(ref["k"][b, r]), 1e-2 * np.linalg.norm(ref["k_full"][b]))     # (k is next to zero near the optimum)
                assert np.linalg.norm(k_st[r] - ref["k"][b, r]) <= hc.FD_TOL * den
            # the swept rows of the stack are the tail of the full sweep, and the prompt is built from them
            assert np.array_equal(ref["k"][b, cs.Tn:cs.Tn + cs.keep], ref["k_full"][b, cs.N - cs.S:cs.N - cs.S + cs.keep])
            assert np.array_equal(ref["prompt"][b, :, :cs.m], ref["k_full"][b, cs.N - cs.S:])
    finally:
        o_ilqr.closed_loop_rollout = real


def test_every_mutant_moves_an_asserted_measure_by_three_bounds():
    """Per branch of QuattroILQR.backward: every mutant that can show on some case of the branch reaches TEETH x the bound of a
    measure the GPU test asserts on at least one case of that branch (in at least one operand type; every ratio is printed)."""
    best = {}
    for name, prec in CASE_PRECISIONS:
        cs = hc.case(name)
        for mutant in hc.MUTANTS:
            r = hc.mutant_ratio(name, mutant, prec)
            print(f"RATIO {cs.branch:10s} {name:14s} {prec:5s} {mutant:48s} " + ("no-op" if r is None else f"{r[0]:10.3g}  ({r[1]})"))
            if r is not None:
                key = (cs.branch, mutant)
                best[key] = max(best.get(key, 0.0), r[0])
    for branch in hc.BRANCHES:
        for mutant in hc.MUTANTS:
            if (branch, mutant) in best:
                assert best[(branch, mutant)] >= hc.TEETH, (branch, mutant, best[(branch, mutant)])
    # the mistakes the issue names are caught in the two branches that have a case with m >= 2, and the rest everywhere
    for mutant in hc.MUTANTS:
        want = ("in_place", "segment") if mutant in hc.LAYOUT_MUTANTS else hc.BRANCHES
        if mutant == "the last N - T swept rows instead of the first":
            want = ("segment",)                                                     # the other branches have no T + S > N
        if mutant == "prompt rows in reverse order" or mutant == hc.MUTANTS[-1]:
            want = tuple(br for br in want if (br, mutant) in best)
            assert want
        for branch in want:
            assert (branch, mutant) in best, (branch, mutant)


def test_layout_mutants_are_caught_where_the_layouts_differ():
    for mutant in hc.LAYOUT_MUTANTS:
        caught = [name for name, prec in CASE_PRECISIONS if hc.case(name).m >= 2 and hc.mutant_ratio(name, mutant, prec)[0] >= hc.TEETH]
        assert caught, mutant
        assert all(hc.mutant_ratio(name, mutant, prec) is None for name, prec in CASE_PRECISIONS if hc.case(name).m == 1)


@pytest.mark.parametrize("name,prec", CASE_PRECISIONS, ids=IDS)
def test_a_no_op_moves_nothing(name, prec):
    """is_noop is a statement about the composition, not a list of exemptions: where it says no-op, the mutated stack is the stack."""
    cs = hc.case(name)
    for mutant in hc.MUTANTS:
        if hc.is_noop(mutant, cs, prec):
            assert all(v == 0.0 for v, _ in hc.mutant_shift(name, mutant, prec).values()), mutant


@pytest.mark.parametrize("name,prec", CASE_PRECISIONS, ids=IDS)
def test_cases_are_what_the_gpu_test_needs(name, prec):
    cs = hc.case(name)
    assert np.all(cs.offset != 0) and np.all(cs.delta != 0) and np.all(cs.x_ref_arg != cs.plant.x_ref)
    assert not np.array_equal(cs.prev_u, cs.u) and not np.array_equal(cs.prev_x0, cs.x0)
    it = hc.iteration(name, prec)
    costs = np.stack([c[2] for c in it["cand"]])
    assert np.isfinite(costs).all() and np.isfinite(it["J"]).all()              # every closed loop under the oracle's stack
    assert it["stopped"].any() and (~it["stopped"]).any(), it["stopped"]
    assert it["stopped"][0]
    bound = hc.linesearch_bound(name, prec)
    dec = hc.decidable(it["J"], it["cand"], bound)
    print(f"CASE {name} {prec}: accepted {it['idx']}, stopped {it['stopped'].astype(int)}, decidable {dec.astype(int)}, "
          f"line-search E_cl {hc.linesearch_noise(name, prec):.1e} bound {bound:.1e}")
    assert dec.sum() >= hc.MIN_DECIDABLE
    # the teacher-forced second nominal differs from the first exactly where a step was accepted
    u2 = hc.second_nominal(name, prec)
    assert [not np.array_equal(u2[b], cs.u[b]) for b in range(hc.B)] == list(it["found"])


@pytest.mark.parametrize("name,prec", CASE_PRECISIONS, ids=IDS)
def test_bounds_are_measured_not_fitted(name, prec):
    """The figures behind every bound the GPU test asserts, printed; each bound is its formula of them."""
    cs = hc.case(name)
    pb = hc.predictor_bound(name, prec)
    if prec == "fp32":
        assert pb == dict.fromkeys(hc.QUANTITIES, 2e-5)
    else:
        noise = hc.predictor_noise(name, prec)
        assert all(0 < noise[key] < 0.05 and pb[key] == 2.0 * noise[key] for key in hc.QUANTITIES), noise
        # the spread between the neighbours: the worst token of each input set alone, largest over smallest
        alone = [hc.predictor_noise(name, prec, neighbours=(r,))["token"] for r in range(hc.NEIGHBOURS)]
        assert max(alone) == noise["token"]
        print(f"BOUND {name} {prec} predicted rows: noise " + ", ".join(f"{key} {noise[key]:.2e}" for key in hc.QUANTITIES) +
              f"; worst token per neighbour {' '.join(f'{v:.2e}' for v in alone)} (spread {max(alone) / min(alone):.1f})")
    for which in (0, 1):
        E, bd = hc.sweep_noise(name, prec, which, cs.keep or None), hc.sweep_bound(name, prec, which, cs.keep or None)
        for key in ("K", "k"):
            assert np.array_equal(bd[key], np.maximum(5e-6, 4.0 * E[key]))
        # the spread between the float32 restatements of one and the same sweep: E of each alone, largest over smallest
        alone = np.stack([hc.sweep_noise(name, prec, which, cs.keep or None, draws=(r,))["k"] for r in range(1 + hc.SWEEP_DRAWS)])
        assert np.array_equal(alone.max(axis=0), E["k"])
        with np.errstate(invalid="ignore", divide="ignore"):
            spread = np.where(alone.min(axis=0) > 0, alone.max(axis=0) / alone.min(axis=0), 1.0)
        print(f"BOUND {name} {prec} swept rows, nominal {which}: E(K) {np.array2string(E['K'], precision=1)} "
              f"E(k) {np.array2string(E['k'], precision=1)} spread of E(k) between restatements {np.array2string(spread, precision=1)}")
        assert E["K"].max() < 1e-6                  # K has no cancellation: the 5e-6 of the suite stands for it on every trajectory
