"""Host-side checks of the cost gradient with respect to a trajectory's rows (quattro_cost_param_gradient_f32,
ops.cost_param_gradient, the row gradients of autograd.trajectory_cost).  None of this needs a GPU:
   1. the fp64 reference of tests/pgrad_cases.py is the TOTAL derivative: against central differences of the oracle's rollout cost
      (parameter, target entry or weight perturbed, re-rolled from the same x0, u), and its difference step is fine enough;
   2. the fp32 restatement's distance E from fp64, the non-zero denominators, and teeth: every mutant of the reference stands >= 10 x
      above the bound the GPU tests assert, in the case pgrad_cases.TEETH names;
   3. ops.cost_param_gradient's ValueErrors and NotImplementedError before anything touches the device;
   4. the symbol is declared, bound and exported by the main and a user-model library (which answers QUATTRO_ERR_UNSUPPORTED), and
      every refusal of the C entry;
   5. the system-identification step rule of the GPU test, with the fp64 reference gradient.

Measured (fp64), worst over pgrad_cases.SETS, N in (7, 26), both integrators, B = param_cases.B_FULL:
   halving the difference step 4e-3: <= 2.5e-10 of the measure's denominator (asserted: 1e-9)
   total derivative against central differences of the rollout cost: phys 2.5e-9 (relative step 1e-5), targets 2.4e-10, weights
   3.0e-11 (relative step 0.1: the cost is quadratic in a target entry and linear in a weight, so the difference is exact)
   E: quadrotor phys 3.7e-8, weights 1.75e-7, targets 1.26e-7; cart-pole 2.1e-8, 1.70e-7, 1.18e-7
   mutants in their TEETH case, quadrotor / cart-pole: lambda_t 2.1e-1 / 1.6e-1, df of step t + 1 2.5e-1 / 3.4e-1, rate derivative
   4.7e+1 / 4.1e+1, rk4 at stage 1 only 4.3e-2 / 8.4e-2, terminal left out 8.7e-1 / 8.8e-1, row rule off by one 7.6e+1 / 1.3e+2,
   q for qf 7.8e-1 / 8.0e-1, the neighbour's phys row 3.5e-1 / 2.4e-1."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import grad_cases as gc
import param_cases as pc
import pgrad_cases as pg
import weight_cases as wc

NAME = "quattro_cost_param_gradient_f32"
CASES = [(model, s, integ) for model in pc.MODELS for s in pg.SETS[model] for integ in pg.INTEGRATORS]


@pytest.fixture(scope="module")
def lib():
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


def _reference(model, c, **kw):
    return pg.reference(model, c["spec"], c["x"], c["u"], c["lam"], **c["kw"], **kw)


# ------------------------------------------------------------------------------------------------ 1. total derivative
@pytest.mark.parametrize("model,integ", [(model, integ) for model in pc.MODELS for integ in pg.INTEGRATORS])
def test_reference_is_the_total_derivative_of_the_rollout_cost(model, integ):
    """Perturb, re-roll out from the same x0 and u, difference J: every parameter, one entry of a target row below the last, one of
    the last row (which collects the terminal term at R - 1 <= N), one weight of each kind."""
    n, m = pc.DIMS[model]
    worst = {}
    for N in (7, 26):
        B, R = pc.B_FULL[model], 3
        c = pg.case(model, "skew", integ, N, R=R, hetero=("weights", "targets", "phys"))
        # the reference about the fp64 rollout itself (case() rounds x to fp32: enough to hide 1e-8)
        x = np.concatenate([pg.o_lin.rollout_batched(sp, c["x0"][b:b + 1], c["u"][b:b + 1])[0] for b, sp in enumerate(c["specs"])])
        d = gc.blocks_per_trajectory(c["specs"], x, c["u"], pg.rc.window(c["kw"]["rows"], N))
        ref = pg.reference(model, c["spec"], x, c["u"], gc.adjoint(d)["costate"], **c["kw"])
        J = lambda **kw: pg.rollout_cost(model, integ, c["x0"], c["u"], **{**c["kw"], **kw})

        def fd(key, arr, index):
            h = (pg.FD_H if key == "phys" else pg.FD_H_EXPLICIT) * np.maximum(np.abs(arr[(slice(None),) + index]), 1e-2)
            hi, lo = arr.copy(), arr.copy()
            hi[(slice(None),) + index] += h
            lo[(slice(None),) + index] -= h
            return (J(**{key: hi}) - J(**{key: lo})) / (2.0 * h)

        for k in range(len(pc.PHYS_NAMES[model])):
            e = np.max(np.abs(fd("phys", c["kw"]["phys"], (k,)) - ref["grad_phys"][:, k]) / ref["den_phys"][:, k])
            worst["phys"] = max(worst.get("phys", 0.0), float(e))
        for index in ((0, 0), (1, n - 1), (R - 1, 2), (R - 1, 1)):
            e = np.max(np.abs(fd("rows", c["kw"]["rows"], index) - ref["grad_targets"][(slice(None),) + index])
                       / ref["den_targets"][(slice(None),) + index])
            worst["targets"] = max(worst.get("targets", 0.0), float(e))
        for j in (1, n + 2, 2 * n + m - 1):
            e = np.max(np.abs(fd("weights", c["kw"]["weights"], (j,)) - ref["grad_weights"][:, j]) / ref["den_weights"][:, j])
            worst["weights"] = max(worst.get("weights", 0.0), float(e))
    print(f"[total derivative {model} {integ}] " + " ".join(f"{k} {e:.1e}" for k, e in worst.items()))
    assert max(worst.values()) < pg.FD_BOUND, worst


@pytest.mark.parametrize("model,set_name,integ", CASES)
def test_halving_the_difference_step_moves_nothing(model, set_name, integ):
    for N in (7, 26):
        c = pg.case(model, set_name, integ, N, R=3)
        a, b = _reference(model, c), _reference(model, c, rel=0.5 * pg.REL_STEP)
        e = float(np.max(np.abs(a["grad_phys"] - b["grad_phys"]) / a["den_phys"]))
        print(f"[step {model} {set_name} {integ}] N={N}: {e:.1e}")
        assert e < 1e-9, (N, e)


# ------------------------------------------------------------------------------------------------ 2. restatement, teeth
@pytest.mark.parametrize("model,set_name,integ", CASES)
def test_fp32_restatement_stays_within_E(model, set_name, integ):
    for N in (7, 26):
        for het in ((), ("weights", "targets", "phys")):
            if het and set_name != "skew":
                continue
            c = pg.case(model, set_name, integ, N, R=3, hetero=het)
            ref = _reference(model, c)
            assert np.all(ref["den_phys"] > 0.0), "every parameter must reach some step"
            errs = pg.errors(pg.restatement(model, c["spec"], c["x"], c["u"], c["lam"], **c["kw"]), ref)
            print(f"[E {model} {set_name} {integ}] N={N} {'+'.join(het) or 'no rows'}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
            assert pg.worst(errs) <= pg.E[model], (N, het, errs)
    # a trajectory's reference does not depend on the batch it sits in
    one = pg.reference(model, c["spec"], c["x"][:1], c["u"][:1], c["lam"][:1], **{k: None if v is None else v[:1] for k, v in c["kw"].items()})
    assert all(np.array_equal(one[k], v[:1]) for k, v in ref.items())


def test_the_measure_wants_an_exact_zero_where_nothing_is_added():
    ref = dict(grad_targets=np.array([[[0.0, 1.0]]]), den_targets=np.array([[[0.0, 2.0]]]))
    assert pg.errors(dict(grad_targets=np.array([[[0.0, 1.5]]])), ref) == dict(grad_targets=0.25)
    for bad in (-0.0, 1e-300):
        assert pg.errors(dict(grad_targets=np.array([[[bad, 1.0]]])), ref)["grad_targets"] == np.inf
    # rows past the horizon: the reference leaves them without a term
    c = pg.case("cartpole", "skew", "euler", 2, R=5)
    ref = _reference("cartpole", c)
    assert np.all(ref["den_targets"][:, 3:] == 0.0) and np.all(ref["grad_targets"][:, 3:] == 0.0) and np.all(ref["den_targets"][:, :3] > 0.0)


@pytest.mark.parametrize("model", pc.MODELS)
def test_every_mutant_stands_ten_bounds_above_the_gpu_bound(model):
    assert set(pg.TEETH[model]) == set(pg.MUTANTS)
    bound = pg.gpu_bound(model)
    assert bound == max(4.0 * pg.E[model], pc.BOUNDS["sim_x"])
    for name, (set_name, integ, N, R, het) in pg.TEETH[model].items():
        c = pg.case(model, set_name, integ, N, R=R, hetero=het)
        moved = pg.worst(pg.errors(_reference(model, c, mutant=name), _reference(model, c)))
        print(f"[teeth {model}] {name} ({set_name}, {integ}, N={N}, R={R}, {het}): {moved:.1e}")
        assert moved >= 10.0 * bound, (name, moved)


# ------------------------------------------------------------------------------------------------ 3. host checks
@pytest.mark.parametrize("model", pc.MODELS)
def test_ops_cost_param_gradient_raises_before_anything_touches_the_device(model):
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
            ops.cost_param_gradient(md, bx, bu)
    w = wc.weight_rows(model, B)
    for bad in (np.ones((B, n + 1)), np.ones((B - 1, 4, n)), np.ones((B, 0, n)), np.ones((n,))):
        with pytest.raises(ValueError, match="targets"):
            ops.cost_param_gradient(md, x, u, targets=bad)
    for bad in (w[:, :-1], w[:B - 1], dict(Q=w[:, :n]), dict(q=w[:, :n - 1])):
        with pytest.raises(ValueError, match="weights"):
            ops.cost_param_gradient(md, x, u, weights=bad)
    for bad in (np.ones((B, len(md.phys) + 1)), np.ones((B - 1, len(md.phys))), np.ones((len(md.phys),))):
        with pytest.raises(ValueError, match="model_phys"):
            ops.cost_param_gradient(md, x, u, model_phys=bad)
    for bad in ((), ("phys", "dt"), "barrier", ("Weights",)):
        with pytest.raises(ValueError, match="want must name"):
            ops.cost_param_gradient(md, x, u, want=bad)
    for bad in (torch.zeros((B, N, n)), torch.zeros((B, N + 1, n + 1)), torch.zeros((N + 1, n))):
        with pytest.raises(ValueError, match="costate must have shape"):
            ops.cost_param_gradient(md, x, u, costate=bad)
    # every accepted form passes the shape checks; the first thing refused is then where the sequences live
    for kw in (dict(), dict(want="weights"), dict(weights=w, want=("targets", "weights")), dict(weights=dict(q=w[:, :n], r=w[0, 2 * n:])),
               dict(targets=np.zeros((B, n), dtype=np.float32)), dict(costate=torch.zeros((B, N + 1, n))),
               dict(targets=np.zeros((B, 4, n), dtype=np.float32), weights=w, model_phys=np.ones((B, len(md.phys))))):
        with pytest.raises(ValueError, match="must live on the GPU"):
            ops.cost_param_gradient(md, x, u, **kw)


def test_a_user_compiled_model_is_refused(lib):
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import ops, user_model
    md = user_model.example_planar_model()
    x, u = torch.zeros((2, 6, md.n)), torch.zeros((2, 5, md.m))
    with pytest.raises(NotImplementedError, match="only for the built-in models"):
        ops.cost_param_gradient(md, x, u)
    with pytest.raises(ValueError, match="x must have shape"):         # the shape checks still come first
        ops.cost_param_gradient(md, x[:, :5], u)


def test_trajectory_cost_says_what_is_differentiable():
    pytest.importorskip("torch")
    import quattro_ilqr_amd as q
    doc = q.trajectory_cost.__doc__
    assert "requires a gradient" in doc and "cost_param_gradient" in doc and "cost_param_gradient" in q.autograd.__doc__
    assert "NOTHING is differentiable" not in doc


# ------------------------------------------------------------------------------------------------ 4. ABI
def test_the_entry_is_declared_exported_and_bound(lib):
    from quattro_ilqr_amd import _lib
    assert NAME in entry.declared_symbols() and NAME in _lib.SIGNATURES
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES[NAME] == (I, [ctypes.POINTER(_lib.ModelParams), P, P, I, I, P, P, P, I, P, P, P, P, P])
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(entry.ROOT, "include", "quattro_hip.h")).read(), flags=re.S)
    args = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    assert [a.split()[-1].lstrip("*") for a in args] == ["p", "x", "u", "B", "N", "costate", "model_phys", "x_ref_rows", "ref_rows",
                                                         "cost_rows", "grad_phys", "grad_cost_rows", "grad_ref_rows", "stream"]


def _copy(p):
    from quattro_ilqr_amd import _lib
    c = _lib.ModelParams()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(p), ctypes.sizeof(p))
    return c


def _call(lib, p, x=1, u=1, B=4, N=10, lam=1, phys=0, rows=0, R=3, cost=0, gp=1, gc_=1, gr=1):
    """Every refusal comes before any launch: the pointers 1 and 16 are never dereferenced."""
    P = ctypes.c_void_p
    return getattr(lib, NAME)(None if p is None else ctypes.byref(p), P(x), P(u), B, N, P(lam), P(phys), P(rows), R, P(cost), P(gp),
                              P(gc_), P(gr), P(0))


@pytest.mark.parametrize("model", pc.MODELS)
def test_the_entry_refuses_bad_arguments_before_any_launch(lib, model):
    from quattro_ilqr_amd import _lib, models
    p = models.model_by_name(model)._build_c_params()
    bad = _lib.ERR_BAD_ARG
    assert _call(lib, p, x=0) == bad and _call(lib, p, u=0) == bad
    assert _call(lib, p, gp=0, gc_=0, gr=0) == bad
    assert _call(lib, p, lam=0) == bad and _call(lib, p, lam=0, gc_=0, gr=0) == bad      # grad_phys without the costate
    assert _call(lib, p, B=0) == bad and _call(lib, p, B=-1) == bad and _call(lib, p, N=0) == bad and _call(lib, p, N=-3) == bad
    for R in (0, -1):
        assert _call(lib, p, rows=16, R=R) == bad, R
    for kw in (dict(phys=1), dict(rows=1), dict(cost=1), dict(phys=8), dict(rows=20), dict(cost=36), dict(phys=16, rows=16, cost=1)):
        assert _call(lib, p, **kw) == bad, kw
    # the model check comes first, as quattro_total_cost_f32 makes it
    assert _call(lib, None) == bad
    unknown, dims, user = _copy(p), _copy(p), _copy(p)
    unknown.model_id = 77
    dims.n = p.n + 1
    user.model_id = _lib.MODEL_USER
    P = ctypes.c_void_p
    for q in (unknown, dims, user):
        for kw in (dict(), dict(x=0), dict(B=0), dict(rows=16, R=0), dict(cost=1), dict(gp=0, gc_=0, gr=0)):
            assert _call(lib, q, **kw) == _lib.ERR_UNSUPPORTED, kw
        assert lib.quattro_total_cost_f32(ctypes.byref(q), P(1), P(1), 4, 10, P(1), P(0)) == _lib.ERR_UNSUPPORTED


def test_user_model_library_exports_the_entry_and_answers_unsupported(lib):
    from quattro_ilqr_amd import _lib, user_model
    md = user_model.example_planar_model()
    assert hasattr(ctypes.CDLL(md.lib_path), NAME)
    ulib = _lib.load_for(md)
    p = md._build_c_params()
    for kw in (dict(), dict(x=0), dict(B=0), dict(gp=0, gc_=0, gr=0), dict(lam=0), dict(rows=16, R=0)):
        assert _call(ulib, p, **kw) == _lib.ERR_UNSUPPORTED, kw
    assert _call(ulib, None) == _lib.ERR_BAD_ARG
    assert _call(lib, p) == _lib.ERR_UNSUPPORTED                       # the main library does not know the model at all
    # the kernel unit is not one of those a user-model library is built from
    assert "cost_param_gradient" not in user_model._UNITS


# ------------------------------------------------------------------------------------------------ 5. the use case's step rule
@pytest.mark.parametrize("model,integ", [(model, integ) for model in pc.MODELS for integ in pg.INTEGRATORS])
def test_the_sysid_step_rule_descends_with_the_reference_gradient(model, integ):
    c = pg.sysid_case(model, integ)
    g = pg.sysid_reference_gradient(model, integ, c)
    halvings = pg.sysid_descends(model, integ, c, g)
    print(f"[sysid {model} {integ}] halvings {halvings.tolist()}")
    assert np.all(halvings >= 0), halvings
    assert np.all(pg.sysid_descends(model, integ, c, -g) < 0)          # and the rule can tell: uphill never gets there
