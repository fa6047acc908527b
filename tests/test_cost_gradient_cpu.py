"""Host-side checks of the cost gradient (quattro_cost_gradient_f32, ops.cost_gradient, autograd.trajectory_cost,
solve(want_grad=True)).  None of this needs a GPU:
   1. the fp64 adjoint of tests/grad_cases.py against central differences of the oracle's rollout cost (N >= 7);
   2. the fp32 restatement's distance E from fp64, and teeth: every mutant of the recursion stands >= 10 x above the bound the GPU
      tests assert, in the case grad_cases.TEETH names, for each model;
   3. ops.cost_gradient's ValueErrors before anything touches the device; solve(want_grad=) leaves the argument order and the
      refusals of the other keywords as they were;
   4. the symbol is declared, bound and exported by the main and a user-model library, and every refusal of the C entry;
   5. the solver measure: the oracle's solves of the cases the GPU test uses end with a gradient norm <= 0.1 x the initial one.

Measured (fp64; restatement fp32), worst over grad_cases.SETS, N in (7, 26), both integrators, B = param_cases.B_FULL:
   finite differences: 7.6e-9 (quadrotor), 1.7e-8 (cart-pole)
   E: 4.45e-7 (quadrotor), 4.31e-7 (cart-pole); user grid points (N = 9, B = 3): <= 2.2e-7
   mutants in their TEETH case, quadrotor / cart-pole: A not transposed 2.1e+0 / 3.2e+1, lambda_t in g_t 1.2e-1 / 2.7e-1, l_x dropped
   8.0e-1 / 9.3e-1, l_u dropped 8.4e-1 / 1.0e+0, A of step t + 1 3.7e-1 / 2.5e-2, B of step t + 1 6.4e-3 / 2.4e-2.  The B shift is the
   weakest where the step's B barely changes: 3.5e-4 on the Euler quadrotor without barrier at N = 7."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import grad_cases as gc
import param_cases as pc
import ref_cases as rc
import weight_cases as wc
from oracle import linearize as o_lin

NAME = "quattro_cost_gradient_f32"
CASES = [(model, s, integ) for model in pc.MODELS for s in gc.SETS[model] for integ in gc.INTEGRATORS]


@pytest.fixture(scope="module")
def lib():
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ 1. finite differences
@pytest.mark.parametrize("model,set_name,integ", CASES)
def test_adjoint_matches_central_differences_of_the_rollout_cost(model, set_name, integ):
    for N in (7, 26):
        x0, u = pc.inputs(model, set_name, N)
        e = gc.fd_errors(pc.spec(model, set_name, integ), x0, u)
        print(f"[fd {model} {set_name} {integ}] N={N}: {e:.1e}")
        assert e < gc.FD_BOUND, (N, e)


# ------------------------------------------------------------------------------------------------ 2. restatement, teeth
@pytest.mark.parametrize("model,set_name,integ", CASES)
def test_fp32_restatement_stays_within_E(model, set_name, integ):
    spec = pc.spec(model, set_name, integ)
    for N in (7, 26):
        x, u = gc.nominal(model, set_name, integ, N)
        d = gc.blocks(spec, x, u)
        errs = gc.errors(gc.adjoint(d, np.float32), gc.adjoint(d), d)
        print(f"[E {model} {set_name} {integ}] N={N}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert gc.worst(errs) <= gc.E[model], (N, errs)
        # a trajectory's reference does not depend on the batch it sits in
        one = gc.adjoint({k: v[:1] for k, v in d.items()})
        assert all(np.array_equal(one[k], v[:1]) for k, v in gc.adjoint(d).items())


def test_the_restatement_on_the_user_grid_stays_within_E():
    for (n, m) in gc.USER_POINTS:
        for integ in gc.INTEGRATORS:
            x, u, d, ref = gc.user_reference(n, m, integ, 9, 3)
            assert x.shape == (3, 10, n) and u.shape == (3, 9, m)
            e = gc.worst(gc.errors(gc.adjoint(d, np.float32), ref, d))
            print(f"[E user {n}x{m} {integ}] {e:.2e}")
            assert e <= gc.USER_E, (n, m, integ, e)


@pytest.mark.parametrize("model", pc.MODELS)
def test_every_mutant_stands_ten_bounds_above_the_gpu_bound(model):
    assert set(gc.TEETH[model]) == set(gc.MUTANTS)
    bound = gc.gpu_bound(model)
    assert bound == max(4.0 * gc.E[model], 2e-6)
    for name, (set_name, integ, N) in gc.TEETH[model].items():
        x, u = gc.nominal(model, set_name, integ, N)
        d = gc.blocks(pc.spec(model, set_name, integ), x, u)
        moved = gc.worst(gc.errors(gc.adjoint(d, mutant=name), gc.adjoint(d), d))
        print(f"[teeth {model}] {name} ({set_name}, {integ}, N={N}): {moved:.1e}")
        assert moved >= 10.0 * bound, (name, moved)


# ------------------------------------------------------------------------------------------------ 3. host checks
@pytest.mark.parametrize("model", pc.MODELS)
def test_ops_cost_gradient_raises_value_errors_before_anything_touches_the_device(model):
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import models, ops
    md = models.model_by_name(model)
    n, m = md.n, md.m
    B, N = 3, 7
    x, u = torch.zeros((B, N + 1, n)), torch.zeros((B, N, m))
    for bx, bu in ((x[:, :N], u), (x, u[:, :N - 1]), (x[:B - 1], u), (x[..., :n - 1], u), (x, torch.zeros((B, N, m + 1))),
                   (x[0], u[0]), (x, u[..., 0]), (torch.zeros((B, 1, n)), torch.zeros((B, 0, m))),
                   (torch.zeros((0, N + 1, n)), torch.zeros((0, N, m)))):
        with pytest.raises(ValueError, match="x must have shape"):
            ops.cost_gradient(md, bx, bu)
    w = wc.weight_rows(model, B)
    for bad in (np.ones((B, n + 1)), np.ones((B - 1, 4, n)), np.ones((B, 0, n)), np.ones((n,))):
        with pytest.raises(ValueError, match="targets"):
            ops.cost_gradient(md, x, u, targets=bad)
    for bad in (w[:, :-1], w[:B - 1], dict(Q=w[:, :n]), dict(q=w[:, :n - 1])):
        with pytest.raises(ValueError, match="weights"):
            ops.cost_gradient(md, x, u, weights=bad)
    for bad in (np.ones((B, len(md.phys) + 1)), np.ones((B - 1, len(md.phys))), np.ones((len(md.phys),))):
        with pytest.raises(ValueError, match="model_phys"):
            ops.cost_gradient(md, x, u, model_phys=bad)
    # every form the solves and ops.score take passes the shape checks (the quadrotor's weights too); the first thing refused is
    # then where the sequences live
    for kw in (dict(weights=w), dict(weights=dict(q=w[:, :n], r=w[0, 2 * n:])), dict(targets=np.zeros((B, n), dtype=np.float32)),
               dict(targets=np.zeros((B, 4, n), dtype=np.float32), weights=w, model_phys=np.ones((B, len(md.phys)))),
               dict(want_x0=False, want_costate=True)):
        with pytest.raises(ValueError, match="must live on the GPU"):
            ops.cost_gradient(md, x, u, **kw)


def test_trajectory_cost_is_exported_and_checks_rows_first():
    torch = pytest.importorskip("torch")
    import quattro_ilqr_amd as q
    assert q.trajectory_cost is q.autograd.trajectory_cost
    q.autograd._PLACEHOLDERS["key"] = object()
    q.autograd.release_placeholders()
    assert q.autograd._PLACEHOLDERS == {} and "release_placeholders" in q.autograd.__doc__
    assert "differentiable" in q.trajectory_cost.__doc__ and "rows or the model's parameters" in q.trajectory_cost.__doc__
    md = q.models.cartpole_model()
    x0, u = torch.zeros((3, 4)), torch.zeros((3, 7, 1))
    with pytest.raises(ValueError, match="targets"):
        q.trajectory_cost(md, x0, u, targets=np.ones((3, 5)))
    with pytest.raises(ValueError, match="weights"):
        q.trajectory_cost(md, x0, u, weights=np.ones((3, 5)))
    with pytest.raises(ValueError, match="model_phys"):
        q.trajectory_cost(md, x0, u, model_phys=np.ones((2, 4)))
    with pytest.raises(ValueError, match="must live on the GPU"):
        q.trajectory_cost(md, x0, u)


def test_solve_keeps_its_arguments_and_refusals():
    pytest.importorskip("torch")
    from quattro_ilqr_amd import QuattroILQR, models
    names = list(inspect.signature(QuattroILQR.solve).parameters)
    assert names == ["self", "x0", "u_init", "x_ref", "max_iter", "fixed_iters", "log", "want_alpha", "upload_guard", "model_phys",
                     "targets", "weights", "want_grad"]
    assert inspect.signature(QuattroILQR.solve).parameters["want_grad"].default is False
    # the refusals of the other keywords come first and are what they were, with or without want_grad
    B, N = 3, 10
    for want in (False, True):
        quad = QuattroILQR(models.quadrotor_model(), N, tf_window=0)
        x0 = np.zeros((B, 12), dtype=np.float32)
        with pytest.raises(NotImplementedError, match="weights runs only in the device-resident loop"):
            quad.solve(x0, weights=np.ones((B, 28), dtype=np.float32), want_grad=want)
        with pytest.raises(ValueError, match="targets"):
            quad.solve(x0, targets=np.ones((B, 3), dtype=np.float32), want_grad=want)
        with pytest.raises(ValueError, match="model_phys"):
            quad.solve(x0, model_phys=np.ones((B, 9), dtype=np.float32), want_grad=want)
        cart = QuattroILQR(models.cartpole_model(), N, tf_window=0, device_loop=False)
        with pytest.raises(NotImplementedError):
            cart.solve(np.zeros((B, 4), dtype=np.float32), weights=np.ones((B, 9), dtype=np.float32), want_grad=want)


# ------------------------------------------------------------------------------------------------ 4. ABI
def test_the_entry_is_declared_exported_and_bound(lib):
    from quattro_ilqr_amd import _lib
    assert NAME in entry.declared_symbols() and NAME in _lib.SIGNATURES
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES[NAME] == (I, [ctypes.POINTER(_lib.ModelParams), P, P, I, I, P, P, I, P, P, P, P, P])
    text = open(os.path.join(entry.ROOT, "include", "quattro_hip.h")).read()
    block = int(re.search(r"#define QUATTRO_GRAD_BLOCK (\d+)\b", text).group(1))
    assert block == _lib.GRAD_BLOCK >= 2
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    assert [a.split()[-1].lstrip("*") for a in args] == ["p", "x", "u", "B", "N", "model_phys", "x_ref_rows", "ref_rows", "cost_rows",
                                                         "grad_u", "grad_x0", "costate", "stream"]
    assert lib.quattro_version() == 100


def _copy(p):
    from quattro_ilqr_amd import _lib
    c = _lib.ModelParams()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(p), ctypes.sizeof(p))
    return c


def _check_refusals(lib, p):
    """Every refusal comes before any launch: `one` (and the aligned `a16`) is never dereferenced."""
    from quattro_ilqr_amd import _lib
    null, one, a16 = ctypes.c_void_p(0), ctypes.c_void_p(1), ctypes.c_void_p(16)

    def call(p=p, x=one, u=one, B=4, N=10, phys=null, rows=null, R=3, cost=null, gu=one, gx0=one, lam=one):
        return getattr(lib, NAME)(None if p is None else ctypes.byref(p), x, u, B, N, phys, rows, R, cost, gu, gx0, lam, null)

    bad = _lib.ERR_BAD_ARG
    assert call(x=null) == bad and call(u=null) == bad and call(gu=null) == bad
    assert call(B=0) == bad and call(B=-1) == bad and call(N=0) == bad and call(N=-3) == bad
    for R in (0, -1):
        assert call(rows=a16, R=R) == bad, R
    for kw in (dict(phys=one), dict(rows=one), dict(cost=one), dict(phys=ctypes.c_void_p(8)), dict(rows=ctypes.c_void_p(20)),
               dict(cost=ctypes.c_void_p(36)), dict(phys=a16, rows=a16, cost=one)):
        assert call(**kw) == bad, kw
    # grad_x0 and costate may be NULL, grad_u may not; both are refusals of other arguments here
    assert call(gx0=null, lam=null, gu=null) == bad and call(gx0=null, lam=null, x=null) == bad
    # the model check comes first, as quattro_total_cost_f32 makes it
    assert call(p=None) == bad
    unknown = _copy(p)
    unknown.model_id = 77
    dims = _copy(p)
    dims.n = p.n + 1
    for q in (unknown, dims):
        for kw in (dict(), dict(x=null), dict(B=0), dict(rows=a16, R=0), dict(cost=one)):
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
    assert "-ffp-contract=off" in user_model._UNITS["cost_gradient"]
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(1)
    p = md._build_c_params()
    assert getattr(lib, NAME)(ctypes.byref(p), one, one, 4, 10, null, null, 0, null, one, one, one, null) == _lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 5. the solver measure
def _norm(d):
    return np.max(np.abs(gc.adjoint(d)["grad_u"]), axis=(1, 2))


@pytest.mark.parametrize("integ", gc.INTEGRATORS)
def test_oracle_solves_of_the_cartpole_weight_cases_reduce_the_gradient_tenfold(integ):
    """weight_cases' cart-pole inputs (B = 5, N = 20) under its weight rows: oracle.ilqr.optimize on each trajectory's own spec."""
    model, N, B = "cartpole", wc.N, wc.B["cartpole"]
    x0, u0 = rc.inputs(model, N, B)
    rows = wc.weight_rows(model)
    for b in range(B):
        spec = wc.row_spec(model, integ, rows[b])
        u, x, _, its = pc.solve_optimize(spec, x0[b], u0[b])
        xs0, _ = o_lin.rollout_batched(spec, x0[b:b + 1], u0[b:b + 1])
        g0 = _norm(gc.blocks(spec, xs0, u0[b:b + 1]))[0]
        g1 = _norm(gc.blocks(spec, np.asarray(x)[None], np.asarray(u)[None]))[0]
        print(f"[measure cartpole {integ}] b={b}: {its} iterations, grad norm {g0:.3e} -> {g1:.3e}")
        assert g1 <= 0.1 * g0, (b, g0, g1)


@pytest.mark.parametrize("integ", gc.INTEGRATORS)
def test_oracle_solves_of_the_quadrotor_ref_cases_reduce_the_gradient_tenfold(integ):
    """ref_cases' quadrotor solve trajectories (param_cases.SOLVE_N and its inputs, rows of their own, R = N + 1):
    oracle.ilqr.optimize on the clock-augmented problem."""
    from test_ref_rows_cpu import REF_B
    model, N = "quadrotor", pc.SOLVE_N
    B = REF_B[model]
    spec = pc.spec(model, "skew", integ)
    x0, u0 = pc.inputs(model, "skew", N, B)
    rows = rc.skew_rows(model, B, N + 1).astype(np.float64)
    win = rc.window(rows, N)
    assert set(rc.SOLVE_TRAJ[model]) == set(range(B))
    for b in rc.SOLVE_TRAJ[model]:
        u, x, _, its, _ = rc.augmented_optimize(spec, rows[b], x0[b], u0[b])
        xs0, _ = o_lin.rollout_batched(spec, x0[b:b + 1], u0[b:b + 1])
        g0 = _norm(gc.blocks(spec, xs0, u0[b:b + 1], win[b:b + 1]))[0]
        g1 = _norm(gc.blocks(spec, np.asarray(x)[None], np.asarray(u)[None], win[b:b + 1]))[0]
        print(f"[measure quadrotor {integ}] b={b}: {its} iterations, grad norm {g0:.3e} -> {g1:.3e}")
        assert g1 <= 0.1 * g0, (b, g0, g1)
