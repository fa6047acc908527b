"""Host-side checks of scoring on the device (quattro_score_f32, ops.score, `score=` of BatchedMPC.run).  None of this needs a GPU:
argument errors come back before any HIP call, shape errors before any tensor is placed on the device.
   1. the symbol is declared, bound, exported, and exported by a user-model library; the argument names in header order;
   2. every QUATTRO_ERR_BAD_ARG of the entry against pointer 1 / NULL arguments, the model check first;
   3. every ValueError of ops.score and the `score=` argument handling of BatchedMPC.run;
   4. the sequences are what tests/score_cases.py says, and teeth: every mistake a kernel could make with the rows, the weights, the
      hold, the terminal slot and the end of the rows moves, for every trajectory, one step's cost and the total by >= 100 x the GPU
      bound."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import param_cases as pc
import score_cases as sc

NAME = "quattro_score_f32"


@pytest.fixture(scope="module")
def lib():
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ 1. the symbol
def test_the_entry_is_declared_exported_and_bound(lib):
    from quattro_ilqr_amd import _lib
    assert NAME in entry.declared_symbols() and NAME in _lib.SIGNATURES
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES[NAME] == (I, [ctypes.POINTER(_lib.ModelParams), P, P, I, I, P, P, I, I, P, I, P, P, P])
    text = open(os.path.join(entry.ROOT, "include", "quattro_hip.h")).read()
    assert re.search(r"#define QUATTRO_SCORE_TERMINAL 1\b", text) and _lib.SCORE_TERMINAL == 1
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    assert [a.split()[-1].lstrip("*") for a in args] == ["p", "x", "u", "B", "S", "model_phys", "x_ref_rows", "ref_rows", "ref_hold",
                                                         "cost_rows", "flags", "stage", "total", "stream"]
    # the library's version is what it was: a model library is found by the digest of its sources, which the new entry changes
    assert lib.quattro_version() == 100


def test_user_model_library_exports_and_checks_the_entry(lib):
    from quattro_ilqr_amd import _lib, user_model
    md = user_model.example_planar_model()
    assert hasattr(ctypes.CDLL(md.lib_path), NAME)
    _check_refusals(_lib.load_for(md), md._build_c_params())


# ------------------------------------------------------------------------------------------------ 2. refusals
def _copy(p):
    from quattro_ilqr_amd import _lib
    c = _lib.ModelParams()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(p), ctypes.sizeof(p))
    return c


def _check_refusals(lib, p):
    """Every refusal comes before any launch: `one` (and the aligned `a16`) is never dereferenced."""
    from quattro_ilqr_amd import _lib
    null, one, a16 = ctypes.c_void_p(0), ctypes.c_void_p(1), ctypes.c_void_p(16)

    def call(p=p, x=one, u=one, B=4, S=10, phys=null, rows=null, R=3, hold=1, cost=null, flags=0, stage=one, total=one):
        return lib.quattro_score_f32(None if p is None else ctypes.byref(p), x, u, B, S, phys, rows, R, hold, cost, flags, stage,
                                     total, null)

    bad = _lib.ERR_BAD_ARG
    assert call(x=null) == bad and call(u=null) == bad and call(total=null) == bad
    assert call(B=0) == bad and call(B=-1) == bad and call(S=0) == bad and call(S=-3) == bad
    for flags in (2, 3, 4, -1, 1 << 16):
        assert call(flags=flags) == bad, flags
    for kw in (dict(R=0), dict(R=-1), dict(hold=0), dict(hold=-2), dict(R=0, hold=0)):
        assert call(rows=a16, **kw) == bad, kw
    for kw in (dict(phys=one), dict(rows=one), dict(cost=one), dict(phys=ctypes.c_void_p(8)), dict(rows=ctypes.c_void_p(20)),
               dict(cost=ctypes.c_void_p(36)), dict(phys=a16, rows=a16, cost=one)):
        assert call(**kw) == bad, kw
    # stage may be NULL, total may not; both are refusals of other arguments here
    assert call(stage=null, total=null) == bad and call(stage=null, x=null) == bad
    # the model check comes first, as quattro_total_cost_f32 makes it
    assert call(p=None) == bad
    unknown = _copy(p)
    unknown.model_id = 77
    dims = _copy(p)
    dims.n = p.n + 1
    for q in (unknown, dims):
        for kw in (dict(), dict(x=null), dict(B=0), dict(flags=2), dict(rows=a16, R=0), dict(cost=one)):
            assert call(p=q, **kw) == _lib.ERR_UNSUPPORTED, kw
            assert lib.quattro_total_cost_f32(ctypes.byref(q), one, one, 4, 10, one, null) == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("model", pc.MODELS)
def test_the_entry_refuses_bad_arguments_before_any_launch(lib, model):
    from quattro_ilqr_amd import models
    _check_refusals(lib, models.model_by_name(model)._build_c_params())


def test_the_main_library_has_no_user_model(lib):
    from quattro_ilqr_amd import _lib, user_model
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(1)
    p = user_model.example_planar_model()._build_c_params()
    assert lib.quattro_score_f32(ctypes.byref(p), one, one, 4, 10, null, null, 0, 1, null, 0, one, one, null) == _lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 3. ops.score, run(score=)
@pytest.mark.parametrize("model", pc.MODELS)
def test_ops_score_raises_value_errors_before_anything_touches_the_device(model):
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import models, ops
    md = models.model_by_name(model)
    n, m = md.n, md.m
    B, S = 3, 7
    x, u = torch.zeros((B, S + 1, n)), torch.zeros((B, S, m))
    for bx, bu in ((x[:, :S], u), (x, u[:, :S - 1]), (x[:B - 1], u), (x[..., :n - 1], u), (x, torch.zeros((B, S, m + 1))),
                   (x[0], u[0]), (x, u[..., 0]), (torch.zeros((B, 1, n)), torch.zeros((B, 0, m))),
                   (torch.zeros((0, S + 1, n)), torch.zeros((0, S, m)))):
        with pytest.raises(ValueError, match="x must have shape"):
            ops.score(md, bx, bu)
    w = sc.wc.weight_rows(model, B)
    for bad in (np.ones((B, n + 1)), np.ones((B - 1, 4, n)), np.ones((B, 0, n)), np.ones((n,))):
        with pytest.raises(ValueError, match="targets"):
            ops.score(md, x, u, targets=bad)
    for bad in (w[:, :-1], w[:B - 1], dict(Q=w[:, :n]), dict(q=w[:, :n - 1])):
        with pytest.raises(ValueError, match="weights"):
            ops.score(md, x, u, weights=bad)
    for bad in (np.ones((B, len(md.phys) + 1)), np.ones((B - 1, len(md.phys))), np.ones((len(md.phys),))):
        with pytest.raises(ValueError, match="model_phys"):
            ops.score(md, x, u, model_phys=bad)
    for bad in (0, -1, 1.5, True, 2.5):
        with pytest.raises(ValueError, match="ref_hold"):
            ops.score(md, x, u, ref_hold=bad, targets=np.zeros((B, 4, n), dtype=np.float32))
    # the quadrotor's weights are taken here: the shapes pass and the first thing refused is where the sequences live
    with pytest.raises(ValueError, match="must live on the GPU"):
        ops.score(md, x, u, weights=w, targets=np.zeros((B, 4, n), dtype=np.float32), ref_hold=2, terminal=True)


def test_run_validates_score_before_any_device_use():
    pytest.importorskip("torch")
    from quattro_ilqr_amd import BatchedMPC, models
    md = models.cartpole_model()
    B, N = 3, 10
    x0 = np.tile(np.asarray(md.x_ref, dtype=np.float32), (B, 1))
    mpc = BatchedMPC(md, N, tf_window=0)
    for bad in ("total", 1, 2.0, ["targets"], ("weights",)):
        with pytest.raises(ValueError, match="score must be None, True or a dict"):
            mpc.run(x0, 4, score=bad)
    with pytest.raises(ValueError, match=r"score has unknown keys \['x_ref', 'hold'\]"):
        mpc.run(x0, 4, score=dict(x_ref=None, terminal=True, hold=2))
    with pytest.raises(ValueError, match=r"score\['targets'\]"):
        mpc.run(x0, 4, score=dict(targets=np.ones((B, 3), dtype=np.float32)))
    with pytest.raises(ValueError, match=r"score\['weights'\]"):
        mpc.run(x0, 4, score=dict(weights=np.ones((B, 3), dtype=np.float32)))
    with pytest.raises(ValueError, match=r"score\['model_phys'\]"):
        mpc.run(x0, 4, score=dict(model_phys=np.ones((B, 9), dtype=np.float32)))
    for bad in (0, -2, 1.5, False):
        with pytest.raises(ValueError, match=r"score\['ref_hold'\]"):
            mpc.run(x0, 4, score=dict(ref_hold=bad))
    # the run's own checks keep their place in front of score's
    with pytest.raises(ValueError, match="targets"):
        mpc.run(x0, 4, targets=np.ones((B, 3), dtype=np.float32), score=True)
    with pytest.raises(ValueError, match="replan_every"):
        mpc.run(x0, 4, replan_every=3, score=True)
    with pytest.raises(NotImplementedError, match="weights runs only in the device-resident loop"):
        mpc.run(x0, 4, weights=np.ones((B, 9), dtype=np.float32), device_loop=False, score=dict(ref_hold=0))
    # what one ops.score call is made with
    rows = np.zeros((B, 5, md.n), dtype=np.float32)
    args = mpc._score_args(True, B, None, True, 1)
    assert args == dict(targets=None, weights=None, model_phys=None, terminal=False, ref_hold=1)
    assert mpc._score_args(None, B, rows, True, 1) is None and mpc._score_args(False, B, rows, True, 1) is None
    assert mpc._score_args(True, B, rows, True, 2)["targets"] is rows and mpc._score_args(True, B, rows, True, 2)["ref_hold"] == 1
    assert mpc._score_args(True, B, rows, False, 2)["ref_hold"] == 2
    other = np.ones((B, md.n), dtype=np.float32)
    args = mpc._score_args(dict(targets=other, terminal=1, ref_hold=4), B, rows, False, 2)
    assert args["targets"] is other and args["terminal"] is True and args["ref_hold"] == 4 and args["weights"] is None
    assert mpc._score_args({}, B, rows, False, 2) == mpc._score_args(True, B, rows, False, 2)
    assert mpc._score_args(dict(targets=None), B, rows, True, 1)["targets"] is None
    # the quadrotor's weights pass here (they are refused in solves and runs, not in scoring)
    quad = BatchedMPC(models.quadrotor_model(), N, tf_window=0)
    w = sc.wc.weight_rows("quadrotor", B)
    assert quad._score_args(dict(weights=w), B, None, True, 1)["weights"] is w


# ------------------------------------------------------------------------------------------------ 4. the sequences, teeth
@pytest.mark.parametrize("case", sc.CASES)
def test_the_sequences_are_what_the_module_says(case):
    model = sc.model_of(case)
    n, m = pc.DIMS[model]
    beta = pc.SETS[model]["skew"]["barrier_beta"]
    for S in sc.STEPS:
        x, u = sc.sequences(case, 5, S)
        assert x.shape == (5, S + 1, n) and u.shape == (5, S, m)
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64)) and np.array_equal(u, u.astype(np.float32))
        x1, u1 = sc.sequences(case, 1, S)
        assert np.array_equal(x1, x[:1]) and np.array_equal(u1, u[:1])                 # B = 1 is a row of B = 5; seeded
        if model == "quadrotor":
            assert np.max(np.abs(x[:, :, 7])) < pc.THETA_MAX
        if case == "quadrotor/shortcut":
            assert beta * u.min() > 2 * 20.0
        stage, total = sc.oracle_score(case, x, u, sc.window(sc.rows_of(case, 5, S + 1), S), sc.weights_of(case, 5), terminal=True)
        assert stage.min() > 0.0 and stage.max() < 1e4 and np.all(total > 0.0)
    x, u = sc.sequences(case, 5, 130)
    if case == "quadrotor/barrier":
        assert 0.28 < (u < 0).mean() < 0.39 and all((u[b] < 0).any() for b in range(5))
    # the row rule
    assert [sc.row_index(s, 1, 4) for s in range(7)] == [0, 1, 2, 3, 3, 3, 3]
    assert [sc.row_index(s, 3, 8) for s in range(11)] == [0, 0, 0, 3, 3, 3, 6, 6, 6, 7, 7]
    assert [sc.row_index(s, 3, 100) for s in range(7)] == [0, 0, 0, 3, 3, 3, 6]


@pytest.mark.parametrize("case", sc.CASES)
def test_every_mistake_moves_a_step_and_the_total_by_100_bounds(case):
    """Row s +- 1, the rows or the weights of trajectory b + 1, ref_hold ignored, q and qf exchanged, r ignored (the shared block's in
    its place), the terminal flag ignored, the last row not held (the ramp continued): against the true score of B = 5, S = 65, 40
    rows held 3 steps, heterogeneous weights, terminal on.  For EVERY trajectory the largest relative change of one step's cost and
    the relative change of the total must be >= 100 x score_cases.BOUND = 2e-4.
    Measured (fp64, smallest over trajectories; step / total): cart-pole >= 1.1e-2 / 5.0e-4 (`the weights of b + 1` 5.0e-4 and
    `r ignored` 5.6e-4 in the total are the closest); quadrotor, barrier live >= 7.5e-2 / 3.4e-3; shortcut >= 7.5e-2 / 5.8e-3."""
    x, u = sc.sequences(case, sc.TEETH_B, sc.TEETH_S)
    true = sc.truth(case, x, u)
    found = sc.mutants(case, x, u)
    assert set(found) == {"row s + 1", "row s - 1", "the rows of b + 1", "the weights of b + 1", "ref_hold ignored",
                          "q and qf exchanged", "r ignored", "terminal flag ignored", "last row not held"}
    for name, got in found.items():
        step, total = sc.moves(got, true)
        print(f"[{case}] {name}: step {step.min():.1e} total {total.min():.1e}")
        assert step.min() >= 100.0 * sc.BOUND and total.min() >= 100.0 * sc.BOUND, (name, step, total)
