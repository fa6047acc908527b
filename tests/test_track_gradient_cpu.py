"""Host-side checks of the gradient of the tracked closed-loop cost (quattro_track_gradient_f32, ops.track_gradient,
autograd.tracking_cost).  None of this needs a GPU:
   1. the fp64 reference of tests/policy_cases.py against central differences of the oracle's closed-loop cost along seeded
      directions in (x0, u_nom, x_nom, K, plant phys), a plant with the other integrator included;
   2. the fp32 restatement's distance E from fp64, and teeth: every mutant of the reference stands >= 10 x above the bound the GPU
      tests assert, in the case policy_cases.TEETH names, for each model;
   3. every ValueError and NotImplementedError of ops.track_gradient and autograd.tracking_cost, before anything touches the device;
   4. the symbol is declared, bound and exported by the main and a user-model library, and every refusal of the C entry.

Measured (fp64; restatement fp32):
   finite differences (h = 1e-6, skew sets, N = 7, B = 3; controller / plant integrator): quadrotor 7.1e-8 (euler / euler), 5.3e-7
   (rk4 / rk4), 6.7e-8 (euler / rk4), 3.4e-7 (rk4 / euler); cart-pole 9.1e-11, 1.5e-10, 1.5e-10, 1.6e-9.  The quadrotor's figure is
   truncation on its most nonlinear trajectory: the same differences at h = 1e-5 give 5.3e-5, a hundred times more.
   E, worst over policy_cases.parity_cases: quadrotor costate 6.11e-7, grad_x0 5.37e-7, grad_u_nom 1.63e-7, grad_K 1.99e-7, grad_x_nom
   1.10e-7; cart-pole 3.90e-7, 3.90e-7, 2.65e-7, 2.76e-7, 3.02e-7; user points (N = 9, S = 9 and 4, B = 3): <= 1.63e-7.
   mutants in their TEETH case (skew, rk4, N = S = 7; the largest measure), quadrotor / cart-pole, against bounds of 2.5e-6 / 2.0e-6:
   feedback dropped from the costate 1.8e+0 / 1.1e+0, K^T l_u dropped 9.1e-1 / 4.8e-2, B K dropped 1.8e+0 / 1.1e+0, K of step t + 1
   4.9e+0 / 2.5e-1, x - x_nom of step t + 1 in dJ/dK 1.6e+2 / 1.4e+0, x for x - x_nom in dJ/dK 1.0e+4 / 1.8e+2, sign of dJ/dx_nom
   1.5e+0 / 1.8e+0, terminal term kept with the flag off 4.8e+0 / 5.9e+0."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import param_cases as pc
import policy_cases as pol

NAME = "quattro_track_gradient_f32"
OTHER = {"euler": "rk4", "rk4": "euler"}


@pytest.fixture(scope="module")
def lib():
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ 1. finite differences
@pytest.mark.parametrize("integ", pol.gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_reference_matches_central_differences_of_the_closed_loop_cost(model, integ):
    for plant_integ in (integ, OTHER[integ]):
        e = pol.fd_errors(model, integ, plant_integ)
        print(f"[fd {model} {integ} plant {plant_integ}] {e:.1e}")
        assert e < pol.FD_BOUND[model], (plant_integ, e)


# ------------------------------------------------------------------------------------------------ 2. restatement, teeth
@pytest.mark.parametrize("model", pc.MODELS)
def test_fp32_restatement_stays_within_E(model):
    for kw in pol.parity_cases(model):
        c = pol.case(model, **kw)
        r32 = pol.reference(c["d"], c["x"], c["x_nom"], c["K"], c["N"], c["terminal"], dtype=np.float32)
        errs = pol.case_errors(c, r32)
        print(f"[E {model} {pol.case_id(kw)}] " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert set(errs) == set(pol.KEYS) and pol.worst(errs) <= pol.E[model], (kw, errs)
        # the reference against itself is exact, and a trajectory's reference does not depend on the batch it sits in
        assert pol.worst(pol.case_errors(c, c["ref"])) == 0.0
        one = pol.reference({k: v[:1] for k, v in c["d"].items()}, c["x"][:1], c["x_nom"][:1], c["K"][:1], c["N"], c["terminal"])
        assert all(np.array_equal(one[k], c["ref"][k][:1]) for k in pol.KEYS)
        # the tracked run is not the nominal: every entry of x - x_nom after the start carries information
        assert np.all(np.max(np.abs(c["x"] - c["x_nom"][:, :c["S"] + 1]), axis=2) > 0.0)


def test_the_restatement_on_the_user_points_stays_within_E():
    for (n, m) in pol.USER_POINTS:
        for integ in pol.gc.INTEGRATORS:
            for N, S in pol.USER_STEPS:
                c = pol.user_case(n, m, integ, N, S)
                assert c["x"].shape == (pol.USER_B, S + 1, n) and c["K"].shape == (pol.USER_B, N, m, n)
                r32 = pol.reference(c["d"], c["x"], c["x_nom"], c["K"], N, True, dtype=np.float32)
                e = pol.worst(pol.case_errors(c, r32))
                print(f"[E user {n}x{m} {integ} N={N} S={S}] {e:.2e}")
                assert e <= pol.USER_E, (n, m, integ, N, S, e)


def test_the_measures_notice_rows_past_the_tracked_steps_and_zero_factors():
    c = pol.case("cartpole", "skew", "euler", 7, 5)
    for key in ("grad_u_nom", "grad_K", "grad_x_nom"):
        for v in (1e-30, -0.0):
            got = {k: a.copy() for k, a in c["ref"].items()}
            got[key][0, 6] = v
            assert pol.case_errors(c, got)[key] == np.inf, (key, v)
    # an entry whose factor is exactly zero must be exactly zero
    x = c["x"].copy()
    x[1, 2, 3] = c["x_nom"][1, 2, 3]
    ref = pol.reference(c["d"], x, c["x_nom"], c["K"], 7)
    assert ref["grad_K"][1, 2, 0, 3] == 0.0
    assert pol.errors(ref, ref, c["d"], x, c["x_nom"], c["K"])["grad_K"] == 0.0
    got = {k: a.copy() for k, a in ref.items()}
    got["grad_K"][1, 2, 0, 3] = 1e-30
    assert pol.errors(got, ref, c["d"], x, c["x_nom"], c["K"])["grad_K"] == np.inf


@pytest.mark.parametrize("model", pc.MODELS)
def test_every_mutant_stands_ten_bounds_above_the_gpu_bound(model):
    assert set(pol.TEETH[model]) == set(pol.MUTANTS) and len(pol.MUTANTS) == 8
    bound = pol.gpu_bound(model)
    assert bound == max(4.0 * pol.E[model], pc.BOUNDS["sim_x"])
    for name, kw in pol.TEETH[model].items():
        c = pol.case(model, **kw)
        assert c["terminal"] == (not name.startswith("terminal"))
        errs = pol.mutant_errors(c, name)
        print(f"[teeth {model}] {name} ({pol.case_id(kw)}): " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert pol.worst(errs) >= 10.0 * bound, (name, errs)


# ------------------------------------------------------------------------------------------------ 3. host checks
@pytest.mark.parametrize("model", pc.MODELS)
def test_ops_track_gradient_raises_value_errors_before_anything_touches_the_device(model):
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import models, ops
    md = models.model_by_name(model)
    n, m = md.n, md.m
    B, N, S = 3, 7, 5
    x, u = torch.zeros((B, S + 1, n)), torch.zeros((B, S, m))
    x_nom, K = torch.zeros((B, N + 1, n)), torch.zeros((B, N, m, n))
    assert list(inspect.signature(ops.track_gradient).parameters) == [
        "model", "x", "u", "x_nom", "K", "plant", "plant_phys", "targets", "weights", "terminal", "want", "want_costate"]
    assert inspect.signature(ops.track_gradient).parameters["want"].default == ("K", "x_nom", "x0")
    for bx, bu in ((x[:, :S], u), (x, u[:, :S - 1]), (x[:B - 1], u), (x[..., :n - 1], u), (x, torch.zeros((B, S, m + 1))),
                   (x[0], u[0]), (torch.zeros((B, 1, n)), torch.zeros((B, 0, m)))):
        with pytest.raises(ValueError, match="x must have shape"):
            ops.track_gradient(md, bx, bu, x_nom, K)
    for bad in (K[:, :S - 1], K[:B - 1], K[..., :n - 1], K[:, :, 0], torch.zeros((B, N, m + 1, n))):
        with pytest.raises(ValueError, match="K must have shape"):
            ops.track_gradient(md, x, u, x_nom, bad)
    for bad in (None, x_nom[:, :N], x_nom[:B - 1], x_nom[..., :n - 1]):
        with pytest.raises(ValueError, match="x_nom must have shape"):
            ops.track_gradient(md, x, u, bad, K)
    for bad in (("k",), "gains", ("K", "u_nom")):
        with pytest.raises(ValueError, match="want may name"):
            ops.track_gradient(md, x, u, x_nom, K, want=bad)
    with pytest.raises(ValueError, match="plant must be the controller's model"):
        ops.track_gradient(md, x, u, x_nom, K, plant=md.with_(dt=md.dt * 2))
    with pytest.raises(ValueError, match="plant must be the controller's model"):
        ops.track_gradient(md, x, u, x_nom, K, plant=models.model_by_name("cartpole" if model == "quadrotor" else "quadrotor"))
    for bad in (np.ones((B, len(md.phys) + 1)), np.ones((B - 1, len(md.phys)))):
        with pytest.raises(ValueError, match="plant_phys"):
            ops.track_gradient(md, x, u, x_nom, K, plant_phys=bad)
    for bad in (np.ones((B, n + 1)), np.ones((B, 0, n))):
        with pytest.raises(ValueError, match="targets"):
            ops.track_gradient(md, x, u, x_nom, K, targets=bad)
    for bad in (np.ones((B, 2 * n + m - 1)), dict(Q=np.ones((B, n)))):
        with pytest.raises(ValueError, match="weights"):
            ops.track_gradient(md, x, u, x_nom, K, weights=bad)
    # well-formed calls pass every shape check, feedback off included; the first thing refused is then where the sequences live
    for kw in (dict(x_nom=x_nom, K=K), dict(), dict(x_nom=x_nom, K=K, plant=md.with_(integrator="rk4"), want=("K",), terminal=False),
               dict(x_nom=x_nom, K=K, plant_phys=np.ones((B, len(md.phys))), targets=np.zeros((B, 3, n)), want_costate=True)):
        with pytest.raises(ValueError, match="must live on the GPU"):
            ops.track_gradient(md, x, u, **kw)


def test_tracking_cost_is_exported_and_refuses_before_anything_touches_the_device():
    torch = pytest.importorskip("torch")
    import quattro_ilqr_amd as q
    assert q.tracking_cost is q.autograd.tracking_cost and "ops.track_gradient" in q.autograd.__doc__
    assert list(inspect.signature(q.tracking_cost).parameters) == [
        "model", "x0", "x_nom", "u_nom", "K", "steps", "plant", "plant_phys", "disturbance", "targets", "weights", "terminal", "feedback"]
    md = q.models.cartpole_model()
    B, N = 3, 7
    x0, x_nom, u_nom, K = torch.zeros((B, 4)), torch.zeros((B, N + 1, 4)), torch.zeros((B, N, 1)), torch.zeros((B, N, 1, 4))
    with pytest.raises(ValueError, match="u_nom must have shape"):
        q.tracking_cost(md, x0, x_nom, u_nom[0], K)
    for steps in (0, N + 1, -1):
        with pytest.raises(ValueError, match="steps must be in 1..N"):
            q.tracking_cost(md, x0, x_nom, u_nom, K, steps=steps)
    with pytest.raises(ValueError, match="disturbance must have shape"):
        q.tracking_cost(md, x0, x_nom, u_nom, K, steps=5, disturbance=torch.zeros((N, B, 4)))
    with pytest.raises(ValueError, match="plant must be the controller's model"):
        q.tracking_cost(md, x0, x_nom, u_nom, K, plant=q.models.quadrotor_model())
    with pytest.raises(ValueError, match="plant_phys"):
        q.tracking_cost(md, x0, x_nom, u_nom, K, plant_phys=np.ones((B, 5)))
    with pytest.raises(ValueError, match="targets"):
        q.tracking_cost(md, x0, x_nom, u_nom, K, targets=np.ones((B, 5)))
    with pytest.raises(ValueError, match="weights"):
        q.tracking_cost(md, x0, x_nom, u_nom, K, weights=np.ones((B, 5)))
    # a row gradient needs the terminal slot
    for kw in (dict(plant_phys=torch.ones((B, 4), requires_grad=True)), dict(weights=torch.ones((B, 9), requires_grad=True)),
               dict(targets=torch.zeros((B, 4), requires_grad=True))):
        with pytest.raises(NotImplementedError, match="terminal=False"):
            q.tracking_cost(md, x0, x_nom, u_nom, K, terminal=False, **kw)
        with pytest.raises(ValueError, match="must live on the GPU"):
            q.tracking_cost(md, x0, x_nom, u_nom, K, **kw)
    with pytest.raises(ValueError, match="must live on the GPU"):
        q.tracking_cost(md, x0, x_nom, u_nom, K, terminal=False, plant_phys=torch.ones((B, 4)))


# ------------------------------------------------------------------------------------------------ 4. ABI
def test_the_entry_is_declared_exported_and_bound(lib):
    from quattro_ilqr_amd import _lib
    assert NAME in entry.declared_symbols() and NAME in _lib.SIGNATURES
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES[NAME] == (I, [ctypes.POINTER(_lib.ModelParams), P, P, I, I, I, P, P, P, P, I, P, I, P, P, P, P, P, P])
    text = open(os.path.join(entry.ROOT, "include", "quattro_hip.h")).read()
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int " + NAME, text, flags=re.S).group(1)
    assert "no counterpart" in comment and "forward_pass" in comment and "quattro_ilqr_tf.py:377-390" in comment
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    assert [a.split()[-1].lstrip("*") for a in args] == ["p", "x", "u", "B", "N", "n_steps", "x_nom", "K", "model_phys", "x_ref_rows",
                                                         "ref_rows", "cost_rows", "flags", "grad_u_nom", "grad_K", "grad_x_nom",
                                                         "grad_x0", "costate", "stream"]
    make = open(os.path.join(entry.PKG_DIR, "csrc", "Makefile")).read()
    assert "track_gradient.hip" in make and "FLAGS_track_gradient := -ffp-contract=off" in make


def _copy(p):
    from quattro_ilqr_amd import _lib
    c = _lib.ModelParams()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(p), ctypes.sizeof(p))
    return c


def _check_refusals(lib, p):
    """Every refusal comes before any launch: `one` (and the aligned `a16`) is never dereferenced."""
    from quattro_ilqr_amd import _lib
    null, one, a16 = ctypes.c_void_p(0), ctypes.c_void_p(1), ctypes.c_void_p(16)

    def call(p=p, x=one, u=one, B=4, N=10, S=7, xn=one, K=one, phys=null, rows=null, R=3, cost=null, flags=1, gu=one, gK=one, gxn=one,
             gx0=one, lam=one):
        return getattr(lib, NAME)(None if p is None else ctypes.byref(p), x, u, B, N, S, xn, K, phys, rows, R, cost, flags, gu, gK, gxn,
                                  gx0, lam, null)

    bad = _lib.ERR_BAD_ARG
    assert call(x=null) == bad and call(u=null) == bad and call(gu=null) == bad
    for kw in (dict(B=0), dict(B=-1), dict(N=0), dict(N=-3), dict(S=0), dict(S=-1), dict(S=11), dict(N=6)):
        assert call(**kw) == bad, kw
    assert call(xn=null) == bad                                            # K without x_nom
    assert call(K=null) == bad and call(K=null, gK=null) == bad and call(K=null, gxn=null) == bad      # grad_K / grad_x_nom without K
    assert call(K=null, xn=null, gxn=null) == bad and call(K=null, xn=null, gK=null) == bad
    for R in (0, -1):
        assert call(rows=a16, R=R) == bad, R
    for kw in (dict(phys=one), dict(rows=one), dict(cost=one), dict(phys=ctypes.c_void_p(8)), dict(rows=ctypes.c_void_p(20)),
               dict(cost=ctypes.c_void_p(36)), dict(phys=a16, rows=a16, cost=one)):
        assert call(**kw) == bad, kw
    for flags in (2, 3, -1, 1 << 30):
        assert call(flags=flags) == bad, flags
    # the optional outputs may be NULL; these are refusals of other arguments
    assert call(gK=null, gxn=null, gx0=null, lam=null, gu=null) == bad and call(gK=null, gxn=null, gx0=null, lam=null, x=null) == bad
    assert call(K=null, xn=null, gK=null, gxn=null, S=0) == bad
    # the model check comes first, as quattro_total_cost_f32 makes it
    assert call(p=None) == bad
    unknown = _copy(p)
    unknown.model_id = 77
    dims = _copy(p)
    dims.n = p.n + 1
    for q in (unknown, dims):
        for kw in (dict(), dict(x=null), dict(B=0), dict(S=11), dict(K=null), dict(rows=a16, R=0), dict(cost=one), dict(flags=2)):
            assert call(p=q, **kw) == _lib.ERR_UNSUPPORTED, kw
            assert lib.quattro_total_cost_f32(ctypes.byref(q), one, one, 4, 10, one, null) == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("model", pc.MODELS)
def test_the_entry_refuses_bad_arguments_before_any_launch(lib, model):
    from quattro_ilqr_amd import models
    _check_refusals(lib, models.model_by_name(model)._build_c_params())


def test_user_model_library_exports_and_checks_the_entry(lib):
    from quattro_ilqr_amd import _lib, user_model
    md = user_model.example_planar_model()
    assert hasattr(ctypes.CDLL(md.lib_path), NAME)
    _check_refusals(_lib.load_for(md), md._build_c_params())
    # the unit is one of those every user-model library is built from, without implicit contraction like the others
    assert "-ffp-contract=off" in user_model._all_units()["track_gradient"] and set(user_model._UNITS) < set(user_model._all_units())
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(1)
    p = md._build_c_params()
    assert getattr(lib, NAME)(ctypes.byref(p), one, one, 4, 10, 7, one, one, null, null, 0, null, 1, one, one, one, one, one,
                              null) == _lib.ERR_UNSUPPORTED
