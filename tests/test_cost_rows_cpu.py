"""Host-side checks of per-trajectory cost weights (quattro_ilqr_solve_cost_f32, quattro_mpc_run_cost_f32; `cost_rows=` of
ops.ilqr_solve / ops.mpc_run, `weights=` of QuattroILQR.solve, BatchedMPC.control_step and BatchedMPC.run).  None of this needs a GPU:
argument errors come back before any HIP call, mode errors before any tensor is placed on the device.
   1. ops.cost_rows_tensor: the forms, the broadcasting, the defaults taken from the model, the 40-float layout, every ValueError;
      the NotImplementedErrors and their order against model_phys's; the two symbols declared, bound, exported and checked;
   2. teeth: every mistake a kernel could make with the rows moves the first iteration's K, k and cost by >= 100 x the GPU bounds;
   3. the inputs of tests/test_cost_rows_gpu.py are well posed (pivots, pitch, line-search margins) over whole fp64 solves;
   4. weight_cases.SOLVE_E: the fp32-storage emulation of the converged solve against oracle.ilqr.optimize."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import param_cases as pc
import ref_cases as rc
import weight_cases as wc

ALPHAS = (1.0, 0.5, 0.25, 0.1, 0.05, 0.01)


# ------------------------------------------------------------------------------------------------ 1. cost_rows_tensor
def _unpack(t, n, m):
    a = t.numpy()
    return a[:, :n], a[:, 16:16 + n], a[:, 32:32 + m]


@pytest.mark.parametrize("model", pc.MODELS)
def test_cost_rows_tensor_forms_broadcasting_defaults_and_layout(model):
    pytest.importorskip("torch")
    import torch
    from quattro_ilqr_amd import _lib, models, ops
    md = models.model_by_name(model)
    n, m = md.n, md.m
    B = 4
    assert ops.COST_ROW_FLOATS == 2 * _lib.MAX_NX + _lib.MAX_NU == 40
    header = open(os.path.join(entry.ROOT, "include", "quattro_hip.h")).read()
    assert re.search(r"#define QUATTRO_COST_ROW_FLOATS \(2 \* QUATTRO_MAX_NX \+ QUATTRO_MAX_NU\)", header)
    rows = wc.rows_about(np.concatenate([md.q, md.qf, md.r]), B)
    q, qf, r = rows[:, :n], rows[:, n:2 * n], rows[:, 2 * n:]
    own = [np.tile(np.asarray(v, dtype=np.float32), (B, 1)) for v in (md.q, md.qf, md.r)]
    assert ops.cost_rows_tensor(md, None, B, "cpu") is None
    # the plain array [q | qf | r], as an array, a list and a tensor
    for form in (rows, rows.tolist(), torch.as_tensor(rows), rows.astype(np.float64)):
        t = ops.cost_rows_tensor(md, form, B, "cpu")
        assert tuple(t.shape) == (B, 40) and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
        got = _unpack(t, n, m)
        assert np.array_equal(got[0], q) and np.array_equal(got[1], qf) and np.array_equal(got[2], r)
        a = t.numpy()
        assert not a[:, n:16].any() and not a[:, 16 + n:32].any() and not a[:, 32 + m:].any()      # (the entries beyond n / m)
    # the dict: all keys, every subset (a missing key takes the model's own values), one vector broadcast over the batch
    full = dict(q=q, qf=qf, r=r)
    assert torch.equal(ops.cost_rows_tensor(md, full, B, "cpu"), ops.cost_rows_tensor(md, rows, B, "cpu"))
    for keys in ((), ("q",), ("qf",), ("r",), ("q", "r"), ("qf", "r"), ("q", "qf")):
        got = _unpack(ops.cost_rows_tensor(md, {k_: full[k_] for k_ in keys}, B, "cpu"), n, m)
        for i, key in enumerate(("q", "qf", "r")):
            assert np.array_equal(got[i], full[key] if key in keys else own[i]), (keys, key)
    got = _unpack(ops.cost_rows_tensor(md, dict(q=q[1], r=torch.as_tensor(r[2])), B, "cpu"), n, m)
    assert np.array_equal(got[0], np.tile(q[1], (B, 1))) and np.array_equal(got[2], np.tile(r[2], (B, 1)))
    assert np.array_equal(got[1], own[1])
    # the model's own weights in every row: the struct's values
    p = md.c_params()
    neutral = ops.cost_rows_tensor(md, {}, B, "cpu").numpy()
    assert np.array_equal(neutral[0, :16], np.asarray(p.q[:], dtype=np.float32))
    assert np.array_equal(neutral[0, 16:32], np.asarray(p.qf[:], dtype=np.float32))
    assert np.array_equal(neutral[0, 32:40], np.asarray(p.r[:], dtype=np.float32))
    # every ValueError: unknown keys, wrong shapes of either form, a wrong batch size
    for bad in (dict(Q=q), dict(q=q, x_ref=q), dict(q=q[:, :n - 1]), dict(q=q[:B - 1]), dict(qf=np.ones((B, n + 1))),
                dict(r=np.ones((B, m + 1))), dict(r=np.ones((m + 1,))), dict(q=np.ones((B, 1, n))), rows[:, :-1], rows[:B - 1],
                rows[0], np.ones((B, 40), dtype=np.float32) if 2 * n + m != 40 else rows[0], np.ones((B, 2, 2 * n + m))):
        with pytest.raises(ValueError, match="weights"):
            ops.cost_rows_tensor(md, bad, B, "cpu")
        with pytest.raises(ValueError, match="cost_rows"):
            ops.check_cost_rows(md, bad, B, name="cost_rows")


class _Predictor:
    prompt_len = 4


def test_solver_and_mpc_validate_weights_before_any_device_use():
    """Wrong shapes and unknown keys are ValueErrors and the modes that have no device-resident loop NotImplementedErrors, with
    model_phys's wording and in its order, all raised before a tensor is placed on the device: on a machine without a GPU anything
    later would fail in another way."""
    pytest.importorskip("torch")
    import dataclasses
    from quattro_ilqr_amd import BatchedMPC, QuattroILQR, models, ops
    md = models.cartpole_model()
    B, N = 3, 10
    x0 = np.tile(np.asarray(md.x_ref, dtype=np.float32), (B, 1))
    good = wc.rows_about(np.concatenate([md.q, md.qf, md.r]), B)
    for bad in (good[:, :-1], good[:B - 1], dict(q=good[:, :3]), dict(R=good[:, 8:]), np.ones((9,), dtype=np.float32)):
        with pytest.raises(ValueError, match="weights"):
            QuattroILQR(md, N, tf_window=0).solve(x0, weights=bad)
        with pytest.raises(ValueError, match="weights"):
            BatchedMPC(md, N, tf_window=0).run(x0, 4, weights=bad)
        with pytest.raises(ValueError, match="weights"):
            BatchedMPC(md, N, tf_window=0).control_step(x0, weights=bad)
    msg = "weights runs only in the device-resident loop"
    phys = np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1))
    for kw, why in ((dict(tf=_Predictor()), "predictor"), (dict(use_graph=True, tf_window=0), "use_graph"),
                    (dict(device_loop=False, tf_window=0), "device_loop=False")):
        for form in (good, dict(r=good[:, 8:])):
            with pytest.raises(NotImplementedError, match=msg) as e:
                QuattroILQR(md, N, **kw).solve(x0, weights=form)
            assert why in str(e.value)
            # the same words as the model_phys refusal, keyword apart
            with pytest.raises(NotImplementedError) as e2:
                QuattroILQR(md, N, **kw).solve(x0, model_phys=phys)
            assert str(e.value) == str(e2.value).replace("model_phys", "weights")
    # order: the predictor is named before use_graph, use_graph before device_loop=False; the mode before the shape
    with pytest.raises(NotImplementedError, match="predictor"):
        QuattroILQR(md, N, tf=_Predictor(), use_graph=True, device_loop=False).solve(x0, weights=good)
    with pytest.raises(NotImplementedError, match="use_graph"):
        QuattroILQR(md, N, use_graph=True, device_loop=False, tf_window=0).solve(x0, weights=good)
    with pytest.raises(NotImplementedError, match="use_graph"):
        QuattroILQR(md, N, use_graph=True, tf_window=0).solve(x0, weights=good[:, :-1])
    with pytest.raises(NotImplementedError, match=msg):
        BatchedMPC(md, N, tf=_Predictor()).run(x0, 4, weights=good)
    with pytest.raises(NotImplementedError, match=msg):
        BatchedMPC(md, N, tf=_Predictor()).control_step(x0, weights=good)
    with pytest.raises(NotImplementedError, match=msg) as e:
        BatchedMPC(md, N, tf_window=0).run(x0, 4, weights=good, device_loop=False)
    with pytest.raises(NotImplementedError) as e2:
        BatchedMPC(md, N, tf_window=0).run(x0, 4, model_phys=phys, device_loop=False)
    assert str(e.value) == str(e2.value).replace("model_phys", "weights")
    # a model without a persistent kernel (here: an integrator the library has none for)
    from quattro_ilqr_amd import models as m_
    m_._INTEGRATORS["midpoint"] = 7
    try:
        odd = dataclasses.replace(md, integrator="midpoint")
        assert not ops.model_can_device_loop(odd)
        sv = QuattroILQR(md, N, tf_window=0)
        sv.model = odd
        with pytest.raises(NotImplementedError, match=msg):
            sv.solve(x0, weights=good)
        assert sv._B is None
        mpc = BatchedMPC(md, N, tf_window=0)
        mpc.model = mpc.solver.model = odd
        with pytest.raises(NotImplementedError, match=msg):
            mpc.run(x0, 4, weights=good)
    finally:
        del m_._INTEGRATORS["midpoint"]
    # the built-in quadrotor: a persistent kernel, but none that takes cost rows -- refused like a model without one, before the shape
    quad = models.quadrotor_model()
    assert ops.model_can_device_loop(quad) and not ops.model_can_cost_rows(quad) and ops.model_can_cost_rows(md)
    qx0 = np.tile(np.asarray(quad.x_ref, dtype=np.float32), (B, 1))
    for w in (wc.weight_rows("quadrotor", B), np.ones((B, 3), dtype=np.float32)):
        sv = QuattroILQR(quad, N, tf_window=0)
        with pytest.raises(NotImplementedError, match=msg + ".*no persistent kernel that takes cost rows"):
            sv.solve(qx0, weights=w)
        assert sv._B is None
        with pytest.raises(NotImplementedError, match="no persistent kernel that takes cost rows"):
            BatchedMPC(quad, N, tf_window=0).run(qx0, 4, weights=w)
        with pytest.raises(NotImplementedError, match="no persistent kernel that takes cost rows"):
            BatchedMPC(quad, N, tf_window=0).control_step(qx0, weights=w)
    # the other keywords keep their own checks next to weights
    with pytest.raises(ValueError, match="plant_phys"):
        BatchedMPC(md, N, tf_window=0).run(x0, 4, weights=good, plant_phys=np.ones((B, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="replan_every"):
        BatchedMPC(md, N, tf_window=0).run(x0, 4, weights=good, replan_every=3)
    with pytest.raises(ValueError, match="model_phys"):
        QuattroILQR(md, N, tf_window=0).solve(x0, weights=good, model_phys=np.ones((B, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="targets"):
        QuattroILQR(md, N, tf_window=0).solve(x0, weights=good, targets=np.ones((B, 3), dtype=np.float32))


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def lib():
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


def _copy(p):
    from quattro_ilqr_amd import _lib
    c = _lib.ModelParams()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(p), ctypes.sizeof(p))
    return c


def _check_entries(lib, p):
    """Both entries of `lib`: every refusal comes before any launch (`one` is never dereferenced)."""
    from quattro_ilqr_amd import _lib
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(1)
    arr6 = (ctypes.c_float * 6)(*ALPHAS)
    B, N = 4, 10
    SIM = _lib.SOLVE_SIMULATE | _lib.SOLVE_RESET

    def solve(p=p, flags=SIM, phys=null, rows=null, R=3, cost=one, n_alpha=6, x_nom=one, iters=one):
        return lib.quattro_ilqr_solve_cost_f32(ctypes.byref(p), one, x_nom, one, B, N, 1e-6, arr6, n_alpha, 1e-3, 5, flags, one, one,
                                               one, one, one, iters, null, one, 1 << 30, None, phys, rows, R, cost, null)

    def solve_ref(p=p, flags=SIM, phys=null, rows=null, R=3, n_alpha=6, x_nom=one, iters=one):
        return lib.quattro_ilqr_solve_ref_f32(ctypes.byref(p), one, x_nom, one, B, N, 1e-6, arr6, n_alpha, 1e-3, 5, flags, one, one,
                                              one, one, one, iters, null, one, 1 << 30, None, phys, rows, R, null)

    def run(p=p, phys=null, rows=null, R=3, preview=1, cost=one, n_steps=10, hold=5, feedback=0, max_iter=5, plant=None,
            plant_phys=null):
        return lib.quattro_mpc_run_cost_f32(ctypes.byref(p), one, one, one, B, N, 1e-6, arr6, 6, 1e-3, max_iter, n_steps, one, one,
                                            one, null, one, one, one, one, one, one, null, one, 1 << 30,
                                            None if plant is None else ctypes.byref(plant), plant_phys, hold, feedback, phys, rows,
                                            R, preview, cost, null)

    def run_ref(p=p, phys=null, rows=null, R=3, preview=1, n_steps=10, hold=5, feedback=0, max_iter=5, plant=None, plant_phys=null):
        return lib.quattro_mpc_run_ref_f32(ctypes.byref(p), one, one, one, B, N, 1e-6, arr6, 6, 1e-3, max_iter, n_steps, one, one,
                                           one, null, one, one, one, one, one, one, null, one, 1 << 30,
                                           None if plant is None else ctypes.byref(plant), plant_phys, hold, feedback, phys, rows,
                                           R, preview, null)

    # (a call whose arguments are all good gets as far as the workspace check -- `one` is not 256-byte aligned -- and stops
    #  there): weights alone and with model_phys, with rows, with both, with and without a plant
    for phys in (null, one):
        for rows in (null, one):
            assert solve(phys=phys, rows=rows) == _lib.ERR_WORKSPACE
            assert run(phys=phys, rows=rows) == _lib.ERR_WORKSPACE
            assert run(phys=phys, rows=rows, plant=_copy(p), plant_phys=one, hold=1, preview=0) == _lib.ERR_WORKSPACE
    # the refusals of the new argument
    for phys in (null, one):
        assert solve(phys=phys, flags=_lib.SOLVE_SIMULATE | _lib.SOLVE_ENQUEUE) == _lib.ERR_BAD_ARG
    assert solve(flags=_lib.SOLVE_SIMULATE | _lib.SOLVE_ENQUEUE, cost=null) == _lib.ERR_WORKSPACE      # (legal without any rows)
    noloop = _copy(p)
    noloop.integrator = 7              # a known problem, but no persistent kernel for it
    assert lib.quattro_model_has_device_loop(ctypes.byref(noloop)) == 0
    assert solve(p=noloop) == _lib.ERR_UNSUPPORTED and run(p=noloop) == _lib.ERR_UNSUPPORTED
    unknown = _copy(p)
    unknown.model_id = 77
    assert solve(p=unknown) == _lib.ERR_UNSUPPORTED and run(p=unknown) == _lib.ERR_UNSUPPORTED
    # the ref entries' own refusals stand with weights
    assert solve(rows=one, R=0) == _lib.ERR_BAD_ARG and run(rows=one, R=0) == _lib.ERR_BAD_ARG
    assert run(rows=one, preview=2) == _lib.ERR_BAD_ARG
    # NULL weights = the entry each extends; with weights, that entry's own verdicts stand
    other = _copy(p)
    other.dt = 2.0 * p.dt
    for phys in (null, one):
        for rows in (null, one):
            for kw in (dict(n_alpha=0), dict(n_alpha=9), dict(x_nom=null), dict(iters=null), dict(),
                       dict(flags=_lib.SOLVE_SIMULATE | _lib.SOLVE_ENQUEUE)):
                want = solve_ref(phys=phys, rows=rows, **kw)
                assert solve(phys=phys, rows=rows, cost=null, **kw) == want, kw
                if "flags" not in kw:
                    assert solve(phys=phys, rows=rows, **kw) == want, kw
            for kw in (dict(hold=0), dict(n_steps=10, hold=3), dict(n_steps=0), dict(feedback=1, max_iter=0), dict(plant=other),
                       dict(hold=N, n_steps=2 * N), dict()):
                want = run_ref(phys=phys, rows=rows, **kw)
                assert run(phys=phys, rows=rows, cost=null, **kw) == want and run(phys=phys, rows=rows, **kw) == want, kw


def test_the_two_entries_are_declared_exported_and_bound(lib):
    from quattro_ilqr_amd import _lib
    for name in ("quattro_ilqr_solve_cost_f32", "quattro_mpc_run_cost_f32"):
        assert name in entry.declared_symbols() and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    # the arguments of the ref entry each extends, in their order, then cost_rows, then stream
    P = ctypes.c_void_p
    for new, old in (("quattro_ilqr_solve_cost_f32", "quattro_ilqr_solve_ref_f32"), ("quattro_mpc_run_cost_f32", "quattro_mpc_run_ref_f32")):
        assert _lib.SIGNATURES[new][1] == _lib.SIGNATURES[old][1][:-1] + [P, P]
    # ... and in the header: the same parameter names in the same order
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(entry.ROOT, "include", "quattro_hip.h")).read(), flags=re.S)
    names = lambda fn: [a.split()[-1].lstrip("*") for a in re.search(fn + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    assert names("quattro_ilqr_solve_cost_f32") == names("quattro_ilqr_solve_ref_f32")[:-1] + ["cost_rows", "stream"]
    assert names("quattro_mpc_run_cost_f32") == names("quattro_mpc_run_ref_f32")[:-1] + ["cost_rows", "stream"]
    # quattro_model_workspace_bytes takes no rows: the library allocates nothing and plans nothing for them
    assert len(_lib.SIGNATURES["quattro_model_workspace_bytes"][1]) == 3


def test_cost_entries_refuse_bad_arguments_before_any_launch(lib):
    from quattro_ilqr_amd import models
    _check_entries(lib, models.model_by_name("cartpole")._build_c_params())


def test_cost_entries_refuse_the_quadrotor_before_any_launch(lib):
    """The quadrotor's persistent kernel has no COST instantiation: QUATTRO_ERR_UNSUPPORTED with rows, whatever else is given, and
    the ref entry's verdict without."""
    from quattro_ilqr_amd import _lib, models
    p = models.model_by_name("quadrotor")._build_c_params()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(1)
    arr6 = (ctypes.c_float * 6)(*ALPHAS)
    B, N = 4, 10
    SIM = _lib.SOLVE_SIMULATE | _lib.SOLVE_RESET
    for phys in (null, one):
        for cost, want in ((one, _lib.ERR_UNSUPPORTED), (null, _lib.ERR_WORKSPACE)):
            assert lib.quattro_ilqr_solve_cost_f32(ctypes.byref(p), one, one, one, B, N, 1e-6, arr6, 6, 1e-3, 5, SIM, one, one, one, one,
                                                   one, one, null, one, 1 << 30, None, phys, null, 0, cost, null) == want
            assert lib.quattro_mpc_run_cost_f32(ctypes.byref(p), one, one, one, B, N, 1e-6, arr6, 6, 1e-3, 5, 10, one, one, one, null,
                                                one, one, one, one, one, one, null, one, 1 << 30, None, null, 5, 0, phys, null, 0, 1,
                                                cost, null) == want


def test_user_model_library_exports_and_checks_the_cost_entries(lib):
    from quattro_ilqr_amd import _lib, user_model
    md = user_model.example_planar_model()
    raw = ctypes.CDLL(md.lib_path)
    assert hasattr(raw, "quattro_ilqr_solve_cost_f32") and hasattr(raw, "quattro_mpc_run_cost_f32")
    _check_entries(_lib.load_for(md), md._build_c_params())


# ------------------------------------------------------------------------------------------------ 2. teeth, 3. the inputs
def test_the_rows_are_what_the_module_says():
    for model in wc.MODELS:
        n, m = pc.DIMS[model]
        rows = wc.weight_rows(model)
        f = rows.astype(np.float64) / wc.base_row(model)
        assert rows.dtype == np.float32 and rows.shape == (wc.B[model], 2 * n + m) and len({r.tobytes() for r in rows}) == len(rows)
        assert f.min() >= wc.FACTOR_RANGE[0] * (1 - 1e-6) and f.max() <= wc.FACTOR_RANGE[1] * (1 + 1e-6)
        assert np.array_equal(wc.weight_rows(model), rows)                 # seeded
        p = wc.row_params(model, rows[1])
        assert p["q"] == tuple(map(float, rows[1, :n])) and p["r"] == tuple(map(float, rows[1, 2 * n:]))
        assert p["x_ref"] == pc.SETS[model]["skew"]["x_ref"] and p["phys"] == pc.SETS[model]["skew"]["phys"]


@pytest.mark.parametrize("model,N", wc.SHAPES)
@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_every_weight_mistake_moves_what_the_gpu_tests_compare(model, N, integ):
    """The row of b + 1, q / qf / r ignored (the shared block's values in their place), q and qf exchanged: against the true row's
    first iteration (ref_cases.first_iteration, a constant window), every trajectory.  K and k must move by >= 100 x their GPU
    bounds (param_cases.BOUNDS: 5e-6 rel_fro -> 5e-4), the nominal's cost by >= 100 x its bound (2e-6 -> 2e-4).
    Measured (fp64, worst over trajectories, both integrators): K and k move by >= 1.0e-2 for every mistake (`r ignored`: K 1.2e-2,
    k 1.0e-2); the cost by >= 2.7e-2 except `r ignored`: 3.1e-4, 1.5 x the requirement: keep the seed."""
    B = wc.B[model]
    rows = wc.weight_rows(model)
    x0, u0 = rc.inputs(model, N, B)
    for b in range(B):
        true = wc.first_iteration(model, integ, rows[b], x0[b:b + 1], u0[b:b + 1])
        for name, w in wc.mistakes(model, rows, b).items():
            assert not np.array_equal(w, rows[b]), (name, b)
            got = wc.first_iteration(model, integ, w, x0[b:b + 1], u0[b:b + 1])
            dK, dk = pc.change("K", got["K"], true["K"]), pc.change("k", got["k"], true["k"])
            dJ = pc.change("cost", got["cost"], true["cost"])
            print(f"[{model} {integ} N={N}] b={b} {name}: K {dK:.1e} k {dk:.1e} cost {dJ:.1e}")
            assert dK >= 100.0 * pc.BOUNDS["K"] and dk >= 100.0 * pc.BOUNDS["k"], (name, b, dK, dk)
            assert dJ >= 100.0 * pc.BOUNDS["sim_cost"], (name, b, dJ)


@pytest.mark.parametrize("model,N", wc.SHAPES)
@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_the_heterogeneous_weights_keep_the_solves_well_posed(model, N, integ):
    """Whole fp64 solves per trajectory (ref_cases.solve_windowed on the row's spec).  Measured, both integrators: smallest
    unpivoted pivot ratio of Q_uu + reg I 1.0 (m = 1); 2 - 3 iterations; smallest relative margin of a first line-search decision
    0.30.  Asserted: pivot ratio >= 0.05, |pitch| < param_cases.THETA_MAX (no pitch here), first margins >= 1e-2."""
    B = wc.B[model]
    rows = wc.weight_rows(model)
    x0, u0 = rc.inputs(model, N, B)
    for b in range(B):
        first = wc.first_iteration(model, integ, rows[b], x0[b:b + 1], u0[b:b + 1])
        assert first["alpha"][0] > 0 and min(first["margins"][0]) >= 1e-2, (b, first["margins"])
        _, _, _, its, pivot, pitch = rc.solve_windowed(wc.row_spec(model, integ, rows[b]), wc.const_window(model, N),
                                                       x0[b:b + 1], u0[b:b + 1])
        print(f"[{model} {integ} N={N}] b={b}: iterations {int(its[0])}, pivot ratio {pivot:.3f}, |pitch| {pitch:.2f}, first "
              f"margins {['%.2f' % v for v in first['margins'][0]]}")
        assert 1 <= int(its[0]) < pc.SOLVE_MAX_ITER
        assert pivot >= 0.05 and pitch < pc.THETA_MAX, (b, pivot, pitch)


# ------------------------------------------------------------------------------------------------ 4. SOLVE_E
@pytest.mark.parametrize("model", wc.MODELS)
def test_fp32_emulation_of_the_converged_solve_stays_within_solve_e(model):
    """param_cases.solve_emulated against param_cases.solve_optimize on every trajectory's own spec, both integrators, at
    param_cases.SOLVE_N and its inputs: equal iteration counts, distances within weight_cases.SOLVE_E (measured: cost 9.2e-8,
    x 5.8e-7, u 2.3e-5) and not far below it: the constants are the measurement, rounded up."""
    x0, u0 = wc.solve_inputs(model)
    rows = wc.weight_rows(model)
    worst = dict(cost=0.0, x=0.0, u=0.0)
    for integ in ("euler", "rk4"):
        for b in range(wc.B[model]):
            sp = wc.row_spec(model, integ, rows[b])
            ref, em = pc.solve_optimize(sp, x0[b], u0[b]), pc.solve_emulated(sp, x0[b], u0[b])
            errs = pc.solve_errors(em, ref)
            print(f"[{model} {integ}] b={b}: iterations {ref[3]} / {em[3]}, {errs}")
            assert ref[3] == em[3], (integ, b, ref[3], em[3])
            worst = {key: max(worst[key], errs[key]) for key in worst}
    for key in worst:
        assert 0.5 * wc.SOLVE_E[model][key] <= worst[key] <= wc.SOLVE_E[model][key], (key, worst[key], wc.SOLVE_E[model][key])
    assert all(wc.solve_bounds(model)[key] >= 4.0 * wc.SOLVE_E[model][key] for key in worst)
