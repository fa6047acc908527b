"""Host-side checks of per-trajectory model parameters (quattro_ilqr_solve_phys_f32, quattro_mpc_run_phys_f32; `model_phys=` of
ops.ilqr_solve / ops.mpc_run, QuattroILQR.solve, BatchedMPC.run / control_step).  Argument errors come back before any HIP call
and the mode errors before any tensor is placed on the device, so none of this needs a GPU.

Also here: the inputs of tests/test_model_phys_gpu.py (`phys_rows`, `row_params`, `oracle_first_iteration`) and the figures that
make them fit for their purpose -- pitch clear of the Euler-angle singularity, no near tie in the first line search, every row
far enough from the shared parameters that a kernel reading the wrong row is seen -- pinned against the fp64 oracle, so that a
later edit of the inputs cannot silently blunt the GPU tests."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import param_cases as pc
from oracle import ilqr as o_ilqr
from oracle import linearize as o_lin

ALPHAS = (1.0, 0.5, 0.25, 0.1, 0.05, 0.01)            # ops.ALPHAS (quattro_ilqr_tf.py:440)
PHYS_N = 26                                           # crosses the fused sweep's 24/25-step refill boundary
PHYS_B = {"quadrotor": 5, "cartpole": 9}              # workgroups of 2 + 2 + 1 trajectories / rows 4 + 4 + 1
CASES = [(model, integ) for model in pc.MODELS for integ in ("euler", "rk4")]


# ------------------------------------------------------------------------------------------------ inputs shared with the GPU tests
def phys_rows(model, B):
    """(B, len(phys)) float32: parameter j of trajectory b is the skew set's times 1 + 0.12 sin(1 + b + 1.7 j); row 0 is the skew
    set itself."""
    base = np.array([float(pc.SETS[model]["skew"]["phys"][k]) for k in pc.PHYS_NAMES[model]], dtype=np.float64)
    b, j = np.arange(B)[:, None], np.arange(base.size)[None, :]
    rows = (base[None, :] * (1.0 + 0.12 * np.sin(1.0 + b + 1.7 * j))).astype(np.float32)
    rows[0] = base.astype(np.float32)
    return rows


def row_params(model, row):
    """The skew set's parameter dict with the physical parameters of one row (the fp32 values, as the device holds them)."""
    p = pc.params(model, "skew")
    p["phys"] = {k: float(v) for k, v in zip(pc.PHYS_NAMES[model], row)}
    return p


def oracle_first_iteration(model, integ, row, x0b, u0b):
    """fp64: the first iLQR iteration of ONE trajectory (x0b (1, n), u0b (1, N, m)) under the parameters of `row`: gains, the
    step the line search accepts, the relative cost margin |J_alpha - J_0| / J_0 of every candidate it tries on the way, and the
    largest |pitch| of the nominal and of the accepted candidate."""
    spec = pc.spec_from(model, row_params(model, row), integ)
    xs, J0 = o_lin.rollout_batched(spec, x0b, u0b)
    kr, Kr = o_ilqr.riccati_sweep_batched(o_lin.linearize_analytic(spec, xs, u0b))
    want, margins, pitch = -1.0, [], float(np.max(np.abs(xs[:, :, 7]))) if model == "quadrotor" else 0.0
    for a in ALPHAS:
        nx, _, Jc = o_lin.closed_loop_rollout_batched(spec, x0b, xs, u0b, kr, Kr, a)
        margins.append(abs(float(Jc[0]) - float(J0[0])) / float(J0[0]))
        if Jc[0] <= J0[0]:
            want = a
            if model == "quadrotor":
                pitch = max(pitch, float(np.max(np.abs(nx[:, :, 7]))))
            break
    return dict(K=Kr[0], k=kr[0], alpha=want, margins=margins, pitch=pitch)


# ------------------------------------------------------------------------------------------------ the inputs are well posed
@pytest.mark.parametrize("model,integ", CASES)
def test_the_heterogeneous_inputs_are_well_posed(model, integ):
    """Measured (fp64 oracle, both integrators): |pitch| <= 0.94; every line-search candidate tried is decided by a relative
    margin |J_alpha - J_0| / J_0 >= 0.35 (quadrotor, accepted steps 1, 0.1, 0.25, 0.25, 0.25) / >= 0.13 (cart-pole, alpha = 1
    throughout); rows 1.. move the first-iteration K by 4.2e-2 .. 1.2e-1 (quadrotor) / 2.2e-2 .. 4.7e-2 (cart-pole) relative
    to the gains under the shared parameters."""
    B = PHYS_B[model]
    rows = phys_rows(model, B)
    assert rows.dtype == np.float32 and len({r.tobytes() for r in rows}) == B
    x0, u0 = pc.inputs(model, "skew", PHYS_N, B)
    shared = [oracle_first_iteration(model, integ, rows[0], x0[b:b + 1], u0[b:b + 1]) for b in range(B)]
    for b in range(B):
        own = oracle_first_iteration(model, integ, rows[b], x0[b:b + 1], u0[b:b + 1])
        move = pc.change("K", shared[b]["K"], own["K"])
        print(f"[{model} {integ}] row {b}: alpha {own['alpha']}, margins {['%.2f' % v for v in own['margins']]}, "
              f"pitch {own['pitch']:.2f}, K moved by {move:.1e}")
        assert own["pitch"] < pc.THETA_MAX
        assert own["alpha"] > 0 and min(own["margins"]) >= 0.1, (b, own["margins"])
        if b > 0:
            assert move >= 100.0 * pc.BOUNDS["K"], (b, move)


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
    """Both entries of `lib`: refusals come before any launch (`one` is never dereferenced)."""
    from quattro_ilqr_amd import _lib
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(1)
    arr6 = (ctypes.c_float * 6)(*ALPHAS)
    B, N = 4, 10

    def solve(p=p, flags=_lib.SOLVE_SIMULATE | _lib.SOLVE_RESET, phys=one, n_alpha=6, x_nom=one, iters=one):
        return lib.quattro_ilqr_solve_phys_f32(ctypes.byref(p), one, x_nom, one, B, N, 1e-6, arr6, n_alpha, 1e-3, 5, flags, one, one,
                                               one, one, one, iters, null, one, 1 << 30, None, phys, null)

    def solve_old(p=p, flags=_lib.SOLVE_SIMULATE | _lib.SOLVE_RESET, n_alpha=6, x_nom=one, iters=one):
        return lib.quattro_ilqr_solve_logged_f32(ctypes.byref(p), one, x_nom, one, B, N, 1e-6, arr6, n_alpha, 1e-3, 5, flags, one,
                                                 one, one, one, one, iters, null, one, 1 << 30, None, null)

    def run(p=p, phys=one, n_steps=10, hold=5, feedback=0, max_iter=5, plant=None):
        return lib.quattro_mpc_run_phys_f32(ctypes.byref(p), one, one, one, B, N, 1e-6, arr6, 6, 1e-3, max_iter, n_steps, one, one,
                                            one, null, one, one, one, one, one, one, null, one, 1 << 30,
                                            None if plant is None else ctypes.byref(plant), null, hold, feedback, phys, null)

    def run_old(p=p, n_steps=10, hold=5, feedback=0, max_iter=5, plant=None):
        return lib.quattro_mpc_run_plant_f32(ctypes.byref(p), one, one, one, B, N, 1e-6, arr6, 6, 1e-3, max_iter, n_steps, one, one,
                                             one, null, one, one, one, one, one, one, null, one, 1 << 30,
                                             None if plant is None else ctypes.byref(plant), null, hold, feedback, null)

    # (a call whose arguments are all good gets as far as the workspace check -- `one` is not 256-byte aligned -- and stops there)
    assert solve() == _lib.ERR_WORKSPACE and run() == _lib.ERR_WORKSPACE
    # the refusals of the new argument
    assert solve(flags=_lib.SOLVE_SIMULATE | _lib.SOLVE_ENQUEUE) == _lib.ERR_BAD_ARG
    assert solve(flags=_lib.SOLVE_SIMULATE | _lib.SOLVE_ENQUEUE, phys=null) == _lib.ERR_WORKSPACE       # (legal without model_phys)
    noloop = _copy(p)
    noloop.integrator = 7              # a known problem, but no persistent kernel for it
    assert lib.quattro_model_has_device_loop(ctypes.byref(noloop)) == 0
    assert solve(p=noloop) == _lib.ERR_UNSUPPORTED and run(p=noloop) == _lib.ERR_UNSUPPORTED
    # the old entries' own verdicts, with and without model_phys, and NULL = the old entry
    for kw in (dict(n_alpha=0), dict(n_alpha=9), dict(x_nom=null), dict(iters=null), dict()):
        want = solve_old(**kw)
        assert solve(**kw) == want and solve(phys=null, **kw) == want, kw
        assert want == (_lib.ERR_WORKSPACE if not kw else _lib.ERR_BAD_ARG)
    other = _copy(p)
    other.dt = 2.0 * p.dt
    for kw in (dict(hold=0), dict(n_steps=10, hold=3), dict(n_steps=0), dict(feedback=1, max_iter=0), dict(plant=other),
               dict(hold=N, n_steps=2 * N), dict()):
        want = run_old(**kw)
        assert run(**kw) == want and run(phys=null, **kw) == want, kw
    assert run(hold=0) == _lib.ERR_BAD_ARG and run(plant=other) == _lib.ERR_BAD_ARG
    unknown = _copy(p)
    unknown.model_id = 77
    assert solve(p=unknown) == _lib.ERR_UNSUPPORTED and run(p=unknown) == _lib.ERR_UNSUPPORTED


def test_the_two_entries_are_declared_exported_and_bound(lib):
    from quattro_ilqr_amd import _lib
    for name in ("quattro_ilqr_solve_phys_f32", "quattro_mpc_run_phys_f32"):
        assert name in entry.declared_symbols() and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the arguments of the entry each extends, in their order, then model_phys, then stream
    old, new = _lib.SIGNATURES["quattro_ilqr_solve_logged_f32"][1], _lib.SIGNATURES["quattro_ilqr_solve_phys_f32"][1]
    assert new == old[:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    old, new = _lib.SIGNATURES["quattro_mpc_run_plant_f32"][1], _lib.SIGNATURES["quattro_mpc_run_phys_f32"][1]
    assert new == old[:-1] + [ctypes.c_void_p, ctypes.c_void_p]


@pytest.mark.parametrize("model", pc.MODELS)
def test_phys_entries_refuse_bad_arguments_before_any_launch(lib, model):
    from quattro_ilqr_amd import models
    _check_entries(lib, models.model_by_name(model)._build_c_params())


def test_user_model_library_exports_and_checks_the_phys_entries(lib):
    from quattro_ilqr_amd import _lib, user_model
    md = user_model.example_planar_model()
    raw = ctypes.CDLL(md.lib_path)
    assert hasattr(raw, "quattro_ilqr_solve_phys_f32") and hasattr(raw, "quattro_mpc_run_phys_f32")
    _check_entries(_lib.load_for(md), md._build_c_params())


# ------------------------------------------------------------------------------------------------ host classes
class _Predictor:
    prompt_len = 4


def test_solver_and_mpc_validate_model_phys_before_any_device_use():
    """Wrong shapes are ValueErrors and the modes that have no device-resident loop NotImplementedErrors, all raised before a
    tensor is placed on the device: on a machine without a GPU anything later would fail in another way."""
    pytest.importorskip("torch")
    from quattro_ilqr_amd import BatchedMPC, QuattroILQR, models, ops
    md = models.quadrotor_model()
    B, N = 3, 10
    x0 = np.tile(np.asarray(md.x_ref, dtype=np.float32), (B, 1))
    good = np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1))
    bad_shapes = (np.ones((B, 5), dtype=np.float32), np.ones((B - 1, 7), dtype=np.float32), np.ones((7,), dtype=np.float32))
    for bad in bad_shapes:
        with pytest.raises(ValueError, match="model_phys"):
            ops.model_phys_tensor(md, bad, B, "cuda:0")
        with pytest.raises(ValueError, match="model_phys"):
            QuattroILQR(md, N, tf_window=0).solve(x0, model_phys=bad)
        with pytest.raises(ValueError, match="model_phys"):
            BatchedMPC(md, N, tf_window=0).run(x0, 4, model_phys=bad)
        with pytest.raises(ValueError, match="model_phys"):
            BatchedMPC(md, N, tf_window=0).control_step(x0, model_phys=bad)
    assert ops.model_phys_tensor(md, None, B, "cuda:0") is None
    msg = "device-resident loop"
    for kw in (dict(tf=_Predictor()), dict(use_graph=True, tf_window=0), dict(device_loop=False, tf_window=0)):
        with pytest.raises(NotImplementedError, match=msg):
            QuattroILQR(md, N, **kw).solve(x0, model_phys=good)
    with pytest.raises(NotImplementedError, match=msg):
        BatchedMPC(md, N, tf=_Predictor()).run(x0, 4, model_phys=good)
    with pytest.raises(NotImplementedError, match=msg):
        BatchedMPC(md, N, tf=_Predictor()).control_step(x0, model_phys=good)
    with pytest.raises(NotImplementedError, match=msg):
        BatchedMPC(md, N, tf_window=0).run(x0, 4, model_phys=good, device_loop=False)
    # a model without a persistent kernel (here: an integrator the library has none for)
    import dataclasses
    from quattro_ilqr_amd import models as m_
    m_._INTEGRATORS["midpoint"] = 7
    try:
        odd = dataclasses.replace(md, integrator="midpoint")
        assert not ops.model_can_device_loop(odd)
        sv = QuattroILQR(md, N, tf_window=0)
        sv.model = odd
        with pytest.raises(NotImplementedError, match=msg):
            sv.solve(x0, model_phys=good)
        mpc = BatchedMPC(md, N, tf_window=0)
        mpc.model = mpc.solver.model = odd
        with pytest.raises(NotImplementedError, match=msg):
            mpc.run(x0, 4, model_phys=good)
    finally:
        del m_._INTEGRATORS["midpoint"]
    # the plant options keep their own checks next to model_phys
    with pytest.raises(ValueError, match="plant_phys"):
        BatchedMPC(md, N, tf_window=0).run(x0, 4, model_phys=good, plant_phys=np.ones((B, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="replan_every"):
        BatchedMPC(md, N, tf_window=0).run(x0, 4, model_phys=good, replan_every=3)
