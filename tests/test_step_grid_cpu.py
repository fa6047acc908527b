"""Host-side checks of tests/step_grid_cases.py, the grid of run lengths and batch sizes at which tests/test_step_grid_gpu.py runs
ops.track_gradient, ops.track_covariance, ops.track_estimate and ops.estimate_log.  None of this needs a GPU:
   1. the grid covers what it claims: for each block size (read from the kernels' sources, so that a changed block fails here and
      does not silently move the edge) a length with remainder 0, one shorter than the block and one equal to it; N > S; and
      policy_cases.STEPS has no multiple of either block, which is why this file exists;
   2. every case builds (log_cases' checks of its reference included), the fp32 restatement stays within E_GRID per measure, and
      E_GRID stands at most 10 % above what is measured here: the constant cannot be padded;
   3. the shape mutants: invisible (< 1e-12) on every case of the family's own parity_cases, >= 10 x above the GPU bound in the case
      SHAPE_TEETH names, which is a case the GPU test runs;
   4. cov_cases.case(B=...) at its default is what it was, bit for bit.
Measured figures: the comments of step_grid_cases.E_GRID and its docstring."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import cov_cases as cc
import est_cases as ec
import log_cases as lc
import param_cases as pc
import policy_cases as pol
import step_grid_cases as sg

OLD = {"gradient": pol, "covariance": cc, "estimate": ec, "log": lc}


# ------------------------------------------------------------------------------------------------ 1. the grid
def _source_blocks():
    csrc = os.path.join(entry.PKG_DIR, "csrc")
    read = lambda *p: open(os.path.join(*p)).read()
    return {"gradient": int(re.search(r"#define QUATTRO_GRAD_BLOCK (\d+)\b", read(entry.ROOT, "include", "quattro_hip.h")).group(1)),
            "covariance": int(re.search(r"constexpr int COV_BLOCK = (\d+);", read(csrc, "track_covariance.hip")).group(1)),
            "log": int(re.search(r"constexpr int LOG_BLOCK = (\d+);", read(csrc, "estimate_log.hip")).group(1))}


def test_the_grid_covers_every_block_edge_and_the_old_steps_none():
    blocks = _source_blocks()
    assert blocks == sg.BLOCKS, "a block size changed: move the grid with it"
    assert "GRAD_BLOCK = QUATTRO_GRAD_BLOCK" in open(os.path.join(entry.PKG_DIR, "csrc", "track_gradient.hip")).read()
    lengths = [S for _, S in sg.STEP_GRID]
    assert len(set(lengths)) == len(lengths) == 10 and sg.N_OF == {S: N for N, S in sg.STEP_GRID}
    for block in sorted(set(blocks.values())):
        assert any(S % block == 0 and S > block for S in lengths), f"several full blocks of {block}"
        assert any(1 < S < block for S in lengths), f"shorter than a block of {block}, and not 1"
        assert block in lengths, f"one full block of {block}"
        assert any(S % block == 0 and all(S % o for o in set(blocks.values()) - {block}) for S in lengths), f"a multiple of {block} alone"
        assert not any(S % block == 0 for _, S in pol.STEPS), "the old step list has no multiple of a block: why this file exists"
    assert any(all(S % b == 0 for b in blocks.values()) for S in lengths) and 25 in lengths and 24 in lengths
    assert all(N in (7, 26) and S < N <= 26 for N, S in sg.STEP_GRID), "param_cases.inputs' horizons; rows past S exist"
    assert sg.BATCH_AT in sg.STEP_GRID and all(sg.BATCH_AT[1] % b == 0 for b in blocks.values())
    for model in pc.MODELS:
        assert sg.batches(model) == (4, 8, pc.B_FULL[model]) and pol.B_CASE not in sg.batches(model)
        assert pc.B_FULL[model] > 8 and pc.B_FULL[model] % 4, "more than two waves of four, the last one ragged"


@pytest.mark.parametrize("family", sg.FAMILIES)
def test_the_case_lists_hold_every_length_batch_and_option(family):
    for model in pc.MODELS:
        for integ in sg.gc.INTEGRATORS:
            cases = sg.all_cases(family, model, integ)
            ids = [sg.case_id(kw) for kw in cases]
            assert len(set(ids)) == len(ids) and all(kw["integ"] == integ and kw["S"] < kw["N"] for kw in cases)
            assert [(kw["N"], kw["S"]) for kw in sg.step_cases(family, model, integ)] == list(sg.STEP_GRID)
            bc = sg.batch_cases(family, model, integ)
            assert [kw["B"] for kw in bc] == list(sg.batches(model)) and all((kw["N"], kw["S"]) == sg.BATCH_AT for kw in bc)
            assert all(kw["hetero"] == sg.ROWS[family]["hetero"] for kw in bc)
            opts = sg.option_cases(family, model, integ)
            block = sg.BLOCKS.get(family, 4)
            assert all(kw["S"] % block == 0 for kw in opts)
            has = lambda **want: [kw["S"] for kw in opts if all(kw.get(k) == v for k, v in want.items())]
            other = sg.OTHER[integ]
            if family == "gradient":
                assert has(terminal=False) == has(R=4, hetero=("weights", "phys")) == has(plant_integ=other) == [3, 6, 12]
                for name in sg.gc.SETS[model]:
                    assert name == "skew" or has(set_name=name) == [3, 12]
                assert all(kw.get("R") == 4 for kw in bc)
            elif family == "covariance":
                for want in (dict(terminal=False), dict(open=True), dict(cov="zero_start"), dict(hetero=("weights", "phys")),
                             dict(plant_integ=other, hetero=("phys",))):
                    assert has(**want) == [4, 12], want
            elif family == "estimate":
                for want in (dict(observed="all"), dict(observed="single"), dict(plain=True),
                             dict(plant_integ=other, hetero=("plant_phys", "model_phys", "meas_var"))):
                    assert has(**want) == [4, 12], want
            else:
                for k in lc.PATTERNS:
                    assert has(pattern=k)[:2] == [4, 8], k
                assert has(shared=True, hetero=("model_phys", "meas_var")) == [12] and has(zero_start=True) == [8]
                assert has(observed="all") == has(observed="single") == [4]


# ------------------------------------------------------------------------------------------------ 2. restatement
@pytest.mark.parametrize("model", pc.MODELS)
@pytest.mark.parametrize("family", sg.FAMILIES)
def test_fp32_restatement_stays_within_E_GRID_and_E_GRID_is_not_padded(family, model):
    worst = {}
    for integ in sg.gc.INTEGRATORS:
        for kw in sg.all_cases(family, model, integ):
            c = sg.build(family, model, kw, check=True)
            B = kw.get("B", pol.B_CASE)
            assert c["S"] == kw["S"] and (c["x0"] if "x0" in c else c["xhat0"]).shape[0] == B
            errs = sg.reference_errors(family, model, c, sg.restatement(family, c))
            print(f"[E_GRID {family} {model} {sg.case_id(kw)}] " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
            for k, e in errs.items():
                assert e <= sg.e_grid(family, model, k), (kw, k, e)
                worst[k] = max(worst.get(k, 0.0), e)
            own = sg.reference_errors(family, model, c, c["ref"])
            assert max(v for k, v in own.items() if k != "asym") == 0.0 and own.get("asym", 0.0) < 1e-14
    if isinstance(sg.E_GRID[family][model], dict):
        assert set(worst) == set(sg.E_GRID[family][model])
        for k, e in worst.items():
            assert e <= sg.E_GRID[family][model][k] <= 1.1 * e, (k, e)
    else:
        assert max(worst.values()) <= sg.E_GRID[family][model] <= 1.1 * max(worst.values()), worst
    # the rule: per measure the larger of 4 x E_GRID and the family's own floor
    for k in worst:
        floor = OLD[family].FLOOR[k] if isinstance(OLD[family].FLOOR, dict) else OLD[family].FLOOR
        assert sg.gpu_bound(family, model, k) == max(4.0 * sg.e_grid(family, model, k), floor)


# ------------------------------------------------------------------------------------------------ 3. shape mutants
@pytest.mark.parametrize("model", pc.MODELS)
@pytest.mark.parametrize("family", sorted(sg.SHAPE_MUTANTS))
def test_shape_mutants_are_invisible_on_the_old_cases_and_stand_out_on_the_grid(family, model):
    assert set(sg.SHAPE_TEETH[family][model]) == set(sg.SHAPE_MUTANTS[family])
    old = [(kw, OLD[family].case(model, **kw)) for kw in OLD[family].parity_cases(model)]
    assert not any(c["S"] % sg.BLOCKS[family] == 0 for _, c in old)
    for name in sg.SHAPE_MUTANTS[family]:
        for kw, c in old:
            errs = sg.shape_mutant_errors(family, model, name, c)
            assert max(errs.values()) < 1e-12, (name, kw, errs)
        kw = sg.SHAPE_TEETH[family][model][name]
        assert kw["S"] % sg.BLOCKS[family] == 0
        assert sg.case_id(kw) in [sg.case_id(k) for k in sg.all_cases(family, model, kw["integ"])], "a case the GPU parity test runs"
        errs = sg.shape_mutant_errors(family, model, name, sg.build(family, model, kw, check=True))
        over = sg.over_bound(family, model, errs)
        print(f"[shape teeth {family} {model}] {name} ({sg.case_id(kw)}): " + " ".join(f"{k} {e:.1e}" for k, e in errs.items())
              + f"; {over:.1e} x the bound")
        assert over >= 10.0, (name, errs)
        # and on every other case of the grid with a full last block it is visible too (the batch and option cases included)
        for integ in sg.gc.INTEGRATORS:
            for k in sg.step_cases(family, model, integ):
                if k["S"] % sg.BLOCKS[family] == 0:
                    e = sg.shape_mutant_errors(family, model, name, sg.build(family, model, k, check=True))
                    assert sg.over_bound(family, model, e) >= 10.0, (name, k, e)


# ------------------------------------------------------------------------------------------------ 4. cov_cases.case(B=...)
@pytest.mark.parametrize("model", pc.MODELS)
def test_cov_case_default_batch_is_what_it_was(model):
    kw = dict(set_name="skew", integ="rk4", N=7, S=5, hetero=("weights", "phys"))
    c = cc.case(model, **kw)
    # as the builder stood before it took B: policy_cases.case at ITS default, then the inputs for that many trajectories
    p = pol.case(model, "skew", "rk4", 7, 5, terminal=True, plant_integ=None, hetero=("weights", "phys"))
    cov0, noise = cc.cov_inputs(model, p["x"].shape[0])
    ref = cc.propagate(p["d"], p["K"], cov0, noise, 7, True)
    assert c["x"].shape[0] == pol.B_CASE == 5
    for key in ("x", "u", "K", "x_nom", "u_nom", "x0", "w", "phys"):
        assert np.array_equal(c[key], p[key]), key
    assert np.array_equal(c["cov0"], cov0) and np.array_equal(c["noise"], noise)
    assert all(np.array_equal(c["ref"][k], ref[k]) for k in cc.KEYS)
    assert all(np.array_equal(cc.case(model, B=5, **kw)["ref"][k], ref[k]) for k in cc.KEYS)
    # and a trajectory's case does not depend on the batch it is built in
    big = cc.case(model, B=8, **kw)
    assert big["x"].shape[0] == 8 and all(np.array_equal(big["ref"][k][:5], ref[k]) for k in cc.KEYS)
