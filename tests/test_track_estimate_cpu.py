"""Host-side checks of output feedback inside a tracked run (quattro_track_estimate_f32, ops.track_estimate, QuattroILQR.fly).  None
of this needs a GPU:
   1. the sequential scalar updates of the definition equal the batch Kalman update L = P H^T (H P H^T + R)^-1 with the Joseph
      covariance to 1e-12 relative, on the covariances and sensors of the cases;
   2. the fp32 restatement of tests/est_cases.py stays within E of the fp64 reference, measure by measure, on every case;
   3. teeth: every mutant of the reference stands >= 10 x above the bound the GPU tests assert, in the case est_cases.TEETH names;
   4. every ValueError and NotImplementedError of ops.track_estimate and QuattroILQR.fly, before anything touches the device; the
      symbol is declared, bound and exported by the main and a user-model library, and every refusal of the C entry.

Measured (fp64; restatement fp32), the worst over est_cases.parity_cases:
   sequential against batch (the largest difference over the largest entry): xhat <= 1.7e-16, P <= 2.9e-15, nis within 1e-12.
   E (rounded up): quadrotor x 2.2e-6, xhat 1.7e-6, u 5.4e-5, cov 3.2e-6, var 3.2e-6, asym 3.4e-7, nis 2.2e-2 (the "single" sensor,
      where a step's nis is one e^2 / s and an e near zero is the denominator; 3.4e-5 over the other cases);
      cart-pole x 7.5e-7, xhat 6.7e-7, u 1.7e-6, cov 1.2e-6, var 1.2e-6, asym 1.8e-7, nis 9.9e-4 (5.0e-5 over the other cases).
   mutants in their TEETH case, the measure that stands highest above its GPU bound (quadrotor / cart-pole, in bounds):
      control from the true state u 4.7e+4 / 2.5e+4; control from the estimate before the update u 2.8e+4 / 6.6e+4; R left out of s cov
      7.8e+4 / 2.1e+5; P not reduced after an update var 1.0e+7 / cov 5.7e+6; innovation sign xhat 1.5e+6 / nis 1.5e+7; A at the true
      state cov 1.9e+3 / var 2.1e+2; A from the plant var 5.9e+3 / cov 1.5e+4; A^T P A cov 5.7e+5 / 3.7e+5; W dropped cov 5.1e+4 /
      1.5e+5; W added before the product cov 6.1e+3 / var 1.2e+4; meas_noise dropped u 1.3e+4 / 1.7e+4; nis with s without R nis 16 /
      380."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import est_cases as ec
import param_cases as pc

NAME = "quattro_track_estimate_f32"


@pytest.fixture(scope="module")
def lib():
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ 1. sequential = batch
@pytest.mark.parametrize("observed", ("pose", "all", "single"))
@pytest.mark.parametrize("model", pc.MODELS)
def test_sequential_scalar_updates_are_the_batch_kalman_update(model, observed):
    c = ec.case(model, integ="euler", N=7, S=1, observed=observed, hetero=("meas_var",))
    obs, n = list(c["observed"]), c["x0"].shape[1]
    H = np.eye(n)[obs]
    for b in range(c["x0"].shape[0]):
        P, R = c["cov0"][b], np.diag(c["meas_var"][b])
        xh, y = c["xhat0"][b], c["x0"][b][obs] + c["meas_noise"][0, b]
        Sm = H @ P @ H.T + R
        L = P @ H.T @ np.linalg.inv(Sm)
        e = y - H @ xh
        x_batch = xh + L @ e
        J = np.eye(n) - L @ H
        P_batch = J @ P @ J.T + L @ R @ L.T                                  # Joseph form
        nis_batch = e @ np.linalg.solve(Sm, e)
        ref = c["ref"]
        assert np.max(np.abs(ref["xhat"][b, 0] - x_batch)) <= 1e-12 * np.max(np.abs(x_batch))
        assert np.max(np.abs(ref["cov"][b, 0] - P_batch)) <= 1e-12 * np.max(np.abs(P_batch))
        assert abs(ref["nis"][b, 0] - nis_batch) <= 1e-12 * nis_batch
        print(f"[batch {model} {observed} b={b}] x {np.max(np.abs(ref['xhat'][b, 0] - x_batch)) / np.max(np.abs(x_batch)):.1e} "
              f"P {np.max(np.abs(ref['cov'][b, 0] - P_batch)) / np.max(np.abs(P_batch)):.1e}")


# ------------------------------------------------------------------------------------------------ 2. restatement
@pytest.mark.parametrize("model", pc.MODELS)
def test_fp32_restatement_stays_within_E(model):
    kinds = set()
    for kw in ec.parity_cases(model):
        c = ec.case(model, **kw)
        assert c["x0"].shape[0] == 5 and c["ref"]["aux"]["s_over_r"] >= 1.0 and c["ref"]["aux"]["fell"]
        errs = ec.errors(c, ec.restatement(c))
        print(f"[E {model} {ec.case_id(kw)}] " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert set(errs) == set(ec.KEYS) | {"asym"}
        assert all(errs[k] <= ec.E[model][k] for k in errs), (kw, errs)
        own = ec.errors(c, c["ref"])
        assert max(own[k] for k in ec.KEYS) == 0.0 and own["asym"] < 1e-13
        # a trajectory's reference does not depend on the batch it sits in
        one = ec.case(model, B=1, **kw)["ref"]
        assert all(np.array_equal(one[k], c["ref"][k][:1]) for k in ec.KEYS)
        if kw.get("plain"):
            assert c["xhat0"] is None and c["meas_noise"] is None and c["disturbance"] is None
            assert np.array_equal(c["ref"]["xhat"][:, 0], c["ref"]["x"][:, 0]) and not c["ref"]["nis"][:, 0].any()
            assert np.all(c["ref"]["nis"][:, 1:] > 0.0), "the plant's mismatch drives the later innovations"
        kinds.add((len(c["observed"]), np.ndim(c["meas_var"]), kw.get("plant_integ") is not None, bool(kw.get("plain"))))
    n = pc.DIMS[model][0]
    assert {k[0] for k in kinds} == {1, n // 2, n} and {k[1] for k in kinds} == {1, 2} and {k[2] for k in kinds} == {True, False}


# ------------------------------------------------------------------------------------------------ 3. teeth
@pytest.mark.parametrize("model", pc.MODELS)
def test_every_mutant_stands_ten_bounds_above_the_gpu_bound(model):
    assert set(ec.TEETH[model]) == set(ec.MUTANTS) and len(ec.MUTANTS) == 12
    for key in ("x", "u", "xhat"):
        assert ec.gpu_bound(model, key) == max(4.0 * ec.E[model][key], 1e-5)
    for key in ("cov", "var", "asym", "nis"):
        assert ec.gpu_bound(model, key) == max(4.0 * ec.E[model][key], ec.cc.FLOOR) and ec.cc.FLOOR == pc.BOUNDS["sim_x"]
    ids = [ec.case_id(k) for k in ec.parity_cases(model)]
    cache = {}
    for name, kw in ec.TEETH[model].items():
        assert ec.case_id(kw) in ids, "a mutant's case is one the GPU parity test runs"
        c = cache.setdefault(ec.case_id(kw), ec.case(model, **kw))
        if name == "A from the plant":
            assert c["plant_integ"] not in (None, c["integ"]) and c["plant_phys"] is not None and c["model_phys"] is not None
        errs = ec.mutant_errors(c, name)
        over = ec.over_bound(model, errs)
        print(f"[teeth {model}] {name} ({ec.case_id(kw)}): {over:.1e} bounds; " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert over >= 10.0, (name, errs)


# ------------------------------------------------------------------------------------------------ 4. host checks
@pytest.mark.parametrize("model", pc.MODELS)
def test_ops_track_estimate_raises_before_anything_touches_the_device(model):
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import models, ops
    md = models.model_by_name(model)
    n, m = md.n, md.m
    B, N, S = 3, 7, 5
    x0, xn, un, K = torch.zeros((B, n)), torch.zeros((B, N + 1, n)), torch.zeros((B, N, m)), torch.zeros((B, N, m, n))
    obs, mv = (0, 2), np.array([1e-4, 2e-4])
    assert list(inspect.signature(ops.track_estimate).parameters) == [
        "model", "x0", "x_nom", "u_nom", "K", "steps", "observed", "meas_var", "xhat0", "cov0", "noise", "meas_noise", "disturbance",
        "plant", "plant_phys", "model_phys", "want"]
    sig = inspect.signature(ops.track_estimate).parameters
    assert sig["want"].default == ("xhat", "var", "nis")
    assert all(sig[k].default is None for k in ("xhat0", "cov0", "noise", "meas_noise", "disturbance", "plant", "plant_phys", "model_phys"))
    doc = ops.track_estimate.__doc__
    assert "P <- A P A^T + noise[b]" in doc and "AFTER the update" in doc and "CALLER's responsibility" in doc
    call = lambda *a, **k: ops.track_estimate(md, *a, **k)
    for bad in (("sigma",), "variance", ("var", "K")):
        with pytest.raises(ValueError, match="want may name"):
            call(x0, xn, un, K, S, obs, mv, want=bad)
    for bu in (un[0], torch.zeros((B, N, m + 1)), torch.zeros((B, 0, m))):
        with pytest.raises(ValueError, match="u_nom must have shape"):
            call(x0, xn, bu, K, S, obs, mv)
    for steps in (0, -1, N + 1):
        with pytest.raises(ValueError, match="steps must be in 1..N"):
            call(x0, xn, un, K, steps, obs, mv)
    with pytest.raises(ValueError, match="x0 must have shape"):
        call(x0[:, :n - 1], xn, un, K, S, obs, mv)
    with pytest.raises(ValueError, match="x_nom must have shape"):
        call(x0, xn[:, :N], un, K, S, obs, mv)
    with pytest.raises(ValueError, match="K must have shape"):
        call(x0, xn, un, K[:, :N - 1], S, obs, mv)
    for bad in ((), (0, 0), (2, 0), (-1, 2), (0, n), tuple(range(n)) + (n,), (0.5, 2.0), ((0, 2),), 3, None):
        with pytest.raises(ValueError, match="observed must be"):
            call(x0, xn, un, K, S, bad, np.full(max(1, np.size(bad) if bad is not None else 1), 1e-4))
    for bad in (np.ones(3), np.ones((B + 1, 2)), np.ones((B, 3)), 1.0, "r", torch.ones(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="meas_var must"):
            call(x0, xn, un, K, S, obs, bad)
    for bad in ((0.0, 1e-4), (-1e-4, 1e-4), (np.nan, 1e-4), (np.inf, 1e-4), (1e-60, 1e-4), (1e60, 1.0),
                torch.tensor([[1e-4, 1e-4]] * (B - 1) + [[1e-4, 0.0]])):
        with pytest.raises(ValueError, match="meas_var must be finite and > 0"):
            call(x0, xn, un, K, S, obs, bad)
    for key, shape in (("xhat0", (B, n + 1)), ("xhat0", (n,)), ("meas_noise", (S, B, 3)), ("meas_noise", (N, B, 2)),
                       ("disturbance", (S, B, n + 1)), ("disturbance", (B, S, n + 2))):
        with pytest.raises(ValueError, match=key + " must have shape"):
            call(x0, xn, un, K, S, obs, mv, **{key: torch.zeros(shape)})
    for key in ("cov0", "noise"):
        for bad in (np.ones((n + 1,)), np.ones((B + 2, n)), np.ones((B, n, n + 1)), 1.0, torch.ones((B, n), dtype=torch.int32)):
            with pytest.raises(ValueError, match=key):
                call(x0, xn, un, K, S, obs, mv, **{key: bad})
    with pytest.raises(ValueError, match="plant must be the controller's model"):
        call(x0, xn, un, K, S, obs, mv, plant=md.with_(dt=md.dt * 2))
    for key in ("plant_phys", "model_phys"):
        for bad in (np.ones((B, len(md.phys) + 1)), np.ones((B - 1, len(md.phys)))):
            with pytest.raises(ValueError, match=key):
                call(x0, xn, un, K, S, obs, mv, **{key: bad})
    # well-formed calls pass every check, in every form of the optional arguments; the first thing refused is then where they live
    ph = np.ones((B, len(md.phys)))
    for kw in (dict(), dict(want=()), dict(want="cov", plant=md.with_(integrator="rk4")),
               dict(xhat0=torch.zeros((B, n)), cov0=np.ones(n), noise=np.ones((B, n)), meas_noise=torch.zeros((S, B, 2)),
                    disturbance=torch.zeros((S, B, n)), plant_phys=ph, model_phys=ph, want=ec.KEYS[2:]),
               dict(cov0=np.eye(n), noise=torch.ones((B, n, n)))):
        with pytest.raises(ValueError, match="must live on the GPU"):
            call(x0, xn, un, K, S, obs, mv, **kw)
    with pytest.raises(ValueError, match="must live on the GPU"):
        call(x0, xn, un, K, S, [1], np.full((B, 1), 0.5))


def test_a_user_model_is_refused_before_its_library_is_loaded(monkeypatch):
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import QuattroILQR, _lib, ops, user_model
    md = user_model.example_planar_model()
    sv = QuattroILQR(md, 8, tf_window=0)
    loads = []
    monkeypatch.setattr(_lib, "load_for", lambda *a, **k: loads.append(1))
    B, N = 2, 4
    args = (torch.zeros((B, md.n)), torch.zeros((B, N + 1, md.n)), torch.zeros((B, N, md.m)), torch.zeros((B, N, md.m, md.n)), N)
    with pytest.raises(NotImplementedError, match="built-in models"):
        ops.track_estimate(md, *args, (0,), (1e-4,))
    with pytest.raises(ValueError, match="observed must be"):
        ops.track_estimate(md, *args, (md.n,), (1e-4,))
    with pytest.raises(NotImplementedError, match="built-in models"):
        sv.fly((0,), (1e-4,))
    assert not loads and sv._B is None


def test_fly_is_checked_before_anything_touches_the_device():
    """QuattroILQR.fly, the solve's side of the feature.  It is a method and not a keyword of solve(): the argument list of solve()
    is pinned by tests/test_cost_gradient_cpu.py and stays what it was."""
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import QuattroILQR, models
    md = models.cartpole_model()
    B, N, n = 3, 10, 4
    assert list(inspect.signature(QuattroILQR.fly).parameters) == [
        "self", "observed", "meas_var", "steps", "xhat0", "cov0", "noise", "meas_noise", "disturbance", "plant", "plant_phys", "want"]
    assert "fly" not in inspect.signature(QuattroILQR.solve).parameters and "observed" not in inspect.signature(QuattroILQR.solve).parameters
    assert "ops.track_estimate" in QuattroILQR.fly.__doc__ and "QuattroILQR.fly" in QuattroILQR.solve.__doc__
    sv = QuattroILQR(md, N, tf_window=0)
    with pytest.raises(RuntimeError, match="call solve\\(\\) first"):
        sv.fly((0, 2), (1e-4, 1e-4))
    # as after a solve of B trajectories whose arrays are never looked at: everything is refused first
    sv._B, sv._solved_rows = B, dict(model_phys=None, targets=None, weights=None)
    for kw, match in ((dict(observed=(2, 0)), "observed must be"), (dict(observed=(0, 4)), "observed must be"),
                      (dict(meas_var=(1e-4, 0.0)), "meas_var must be finite"), (dict(meas_var=np.ones((B + 1, 2))), "meas_var must have"),
                      (dict(cov0=np.ones(n + 1)), "cov0 must be"), (dict(noise=np.ones((B + 2, n))), "noise must be"),
                      (dict(steps=0), "steps must be"), (dict(steps=N + 1), "steps must be"),
                      (dict(xhat0=torch.zeros((B, n + 1))), "xhat0 must have shape"),
                      (dict(meas_noise=torch.zeros((N, B, 3))), "meas_noise must have shape"),
                      (dict(steps=4, disturbance=torch.zeros((5, B, n))), "disturbance must have shape"),
                      (dict(plant=md.with_(dt=0.5)), "plant must be"), (dict(plant_phys=np.ones((B, 9))), "plant_phys")):
        args = dict(observed=(0, 2), meas_var=(1e-4, 1e-4))
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            sv.fly(**args)


# ------------------------------------------------------------------------------------------------ ABI
ARGS = ["p", "plant", "x0", "x_nom", "u_nom", "K", "B", "N", "n_steps", "observed", "p_y", "meas_var", "meas_var_rows", "xhat0", "cov0",
        "noise", "meas_noise", "disturbance", "plant_phys", "model_phys", "x", "u", "xhat", "var", "cov", "nis", "stream"]


def test_the_entry_is_declared_exported_and_bound(lib):
    from quattro_ilqr_amd import _lib
    assert NAME in entry.declared_symbols() and NAME in _lib.SIGNATURES
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    P, I, M = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_lib.ModelParams)
    assert _lib.SIGNATURES[NAME] == (I, [M, M, P, P, P, P, I, I, I, ctypes.POINTER(ctypes.c_int32), I, P, I] + [P] * 14)
    text = open(os.path.join(entry.ROOT, "include", "quattro_hip.h")).read()
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int " + NAME, text, flags=re.S).group(1)
    assert "no counterpart" in comment and "P <- A P A^T + W[b]" in comment and "READ AS SYMMETRIC" in comment
    assert "AFTER the update" in comment and "QUATTRO_ERR_UNSUPPORTED" in comment
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    make = open(os.path.join(entry.PKG_DIR, "csrc", "Makefile")).read()
    assert "track_estimate.hip" in make and "FLAGS_track_estimate := -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form=1" in make


def _copy(p):
    from quattro_ilqr_amd import _lib
    c = _lib.ModelParams()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(p), ctypes.sizeof(p))
    return c


def _caller(lib, p):
    """-> call(**overrides): the entry with device pointers that are never dereferenced (`one`) and a valid host `observed`."""
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(1)

    def call(p=p, plant=None, x0=one, xn=one, un=one, K=one, B=4, N=10, S=7, obs=(0, 2), p_y=None, mv=one, rows=0, xh0=null, c0=null,
             w=null, v=null, d=null, pphys=null, mphys=null, x=one, u=one, xhat=one, var=null, cov=null, nis=one):
        arr = None if obs is None else (ctypes.c_int32 * max(1, len(obs)))(*obs)
        return getattr(lib, NAME)(None if p is None else ctypes.byref(p), None if plant is None else ctypes.byref(plant), x0, xn, un, K,
                                  B, N, S, arr, (0 if obs is None else len(obs)) if p_y is None else p_y, mv, rows, xh0, c0, w, v, d,
                                  pphys, mphys, x, u, xhat, var, cov, nis, null)
    return call


def _check_refusals(lib, p):
    """Every refusal comes before any launch: `one` (and the aligned `a16`) is never dereferenced."""
    from quattro_ilqr_amd import _lib
    null, one, a16 = ctypes.c_void_p(0), ctypes.c_void_p(1), ctypes.c_void_p(16)
    call = _caller(lib, p)
    bad, n = _lib.ERR_BAD_ARG, p.n
    for key in ("x0", "xn", "un", "K", "mv", "x", "u"):
        assert call(**{key: null}) == bad, key
    assert call(obs=None, p_y=2) == bad
    for kw in (dict(B=0), dict(B=-1), dict(N=0), dict(N=-3), dict(S=0), dict(S=-1), dict(S=11), dict(N=6)):
        assert call(**kw) == bad, kw
    for kw in (dict(obs=(), p_y=0), dict(p_y=-1), dict(obs=tuple(range(n)) + (n,)), dict(p_y=n + 1), dict(obs=(0, n)), dict(obs=(-1, 2)),
               dict(obs=(2, 2)), dict(obs=(2, 0)), dict(obs=(0, 2, 1)), dict(rows=2), dict(rows=-1)):
        assert call(**kw) == bad, kw
    for kw in (dict(pphys=one), dict(mphys=one), dict(pphys=ctypes.c_void_p(8)), dict(mphys=ctypes.c_void_p(36)), dict(pphys=a16, mphys=one)):
        assert call(**kw) == bad, kw
    for field, value in (("dt", p.dt * 2), ("n", p.n + 1), ("model_id", 77)):
        other = _copy(p)
        setattr(other, field, value)
        assert call(plant=other) == bad, field
    other = _copy(p)
    other.integrator = 5
    assert call(plant=other) == _lib.ERR_UNSUPPORTED
    # the optional arguments may be NULL; these are refusals of other arguments
    assert call(xhat=null, nis=null, x=null) == bad and call(xhat=null, nis=null, S=0) == bad
    # the model check comes first, as quattro_total_cost_f32 makes it
    assert call(p=None) == bad
    unknown = _copy(p)
    unknown.model_id = 77
    dims = _copy(p)
    dims.n = p.n + 1
    for q in (unknown, dims):
        for kw in (dict(), dict(x0=null), dict(B=0), dict(S=11), dict(obs=(2, 0)), dict(pphys=one), dict(rows=3)):
            assert call(p=q, **kw) == _lib.ERR_UNSUPPORTED, kw
            assert lib.quattro_total_cost_f32(ctypes.byref(q), one, one, 4, 10, one, null) == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("model", pc.MODELS)
def test_the_entry_refuses_bad_arguments_before_any_launch(lib, model):
    from quattro_ilqr_amd import models
    _check_refusals(lib, models.model_by_name(model)._build_c_params())


def test_user_model_library_exports_the_entry_and_answers_unsupported(lib):
    from quattro_ilqr_amd import _lib, models, user_model
    md = user_model.example_planar_model()
    assert hasattr(ctypes.CDLL(md.lib_path), NAME)
    ulib = _lib.load_for(md)
    null = ctypes.c_void_p(0)
    p = md._build_c_params()
    # its own model: unsupported whatever else is passed; through the main library the block is an unknown model
    assert _caller(ulib, p)() == _lib.ERR_UNSUPPORTED and _caller(ulib, p)(x0=null) == _lib.ERR_UNSUPPORTED
    assert _caller(ulib, p)(obs=(3, 1)) == _lib.ERR_UNSUPPORTED
    assert _caller(lib, p)() == _lib.ERR_UNSUPPORTED
    assert _caller(ulib, p)(p=None) == _lib.ERR_BAD_ARG
    # the kernel unit is the main library's alone: the build list of a user-model library is what it was
    assert "track_estimate" not in user_model._all_units()
    # a built-in model's block given to a user-model library: checked like any call, then refused without a launch
    q = models.cartpole_model()._build_c_params()
    assert _caller(ulib, q)(x0=null) == _lib.ERR_BAD_ARG and _caller(ulib, q)(obs=(2, 0)) == _lib.ERR_BAD_ARG
    assert _caller(ulib, q)() == _lib.ERR_UNSUPPORTED
