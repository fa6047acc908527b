"""Host-side checks of the row gradients of USER-COMPILED models (compile_model(..., param_grad=True), csrc/user_param_gradient.hip).
None of this needs a GPU:
   1. without the keyword nothing changes: the generated header of the planar example is the parent commit's text (SHA-1), the
      units are the same, and the plain library still answers QUATTRO_ERR_UNSUPPORTED; the opt-in library has another cache key,
      carries `param_grad`, exports the entry and refuses bad arguments as the main library does;
   2. a body that declares a parameter `float` fails compile_model(param_grad=True) with the compiler's message and the rule;
   3. ops.cost_param_gradient still refuses a plain user model, with the old phrase and the name of the keyword;
   4. the fp64 reference of tests/upgrad_cases.py is the TOTAL derivative (complex-step derivatives of the fp64 rollout cost in every
      parameter, a weight of each kind and target entries of both kinds of row), its inputs are well conditioned (no d rate_i /
      d theta_k is a difference that cancels more than four-fold), the fp32 restatement's distance E, and teeth: every mutant stands
      >= 10 x above the GPU bound in the case upgrad_cases.TEETH names;
   5. the step rule of the GPU test's use case, with the fp64 reference gradient and with its sign flipped.

Measured (fp64): total derivative <= 7.8e-15 of the measure's denominator (asserted: 8e-14); cancellation <= 1.14 (the quadrotor's
inertias; 12 with body rates of 0.6 rad/s and unbiased rotors, where the restatement is 2.4e-6 off at N = 1); E: grid1x1 1.84e-7,
grid4x4 1.64e-7, grid16x8 1.72e-7, quad 5.57e-7, probe 2.09e-7; mutants in their TEETH case: lambda_t 6.5e-2, the cost's own partial
dropped 8.4e-1, terminal slot dropped 5.2e-1, closed-form weights 9.1e-1, row rule off by one 1.5, q / qf exchanged 1.3e+1, RK4 at
stage 1 only 3.8e-2, the seed of theta_k+1 1.7e+2."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import grad_cases as gc
import upgrad_cases as U

NAME = "quattro_cost_param_gradient_f32"
PLANAR_HEADER_SHA1 = "7c59652c4b811d987f92041235ca0e5f2d038e64"        # example_planar_model().source at the parent commit


@pytest.fixture(scope="module")
def lib():
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ 1. the option changes nothing else
def test_without_the_option_the_header_and_the_units_are_the_parents(lib):
    from quattro_ilqr_amd import user_model
    md = user_model.example_planar_model()
    assert hashlib.sha1(md.source.encode()).hexdigest() == PLANAR_HEADER_SHA1
    assert md.param_grad is False
    assert tuple(user_model._UNITS) == ("capi", "linearize", "rollout", "cost_gradient", "sweep_generic", "solve_user")
    assert user_model._PARAM_GRAD_UNIT not in user_model._UNITS


def test_the_opt_in_library_has_its_own_cache_key_and_header(lib):
    from quattro_ilqr_amd import user_model
    plain, opt = user_model.example_planar_model(), user_model.example_planar_model(param_grad=True)
    assert opt.param_grad is True and opt.with_(dt=0.01).param_grad is True
    assert opt.lib_path != plain.lib_path and os.path.dirname(opt.lib_path) != os.path.dirname(plain.lib_path)
    assert opt.source != plain.source
    assert "template <class T, class PB = quattro_model_params>" in opt.source and "const auto* P = p.phys;" in opt.source
    assert "class PB" not in plain.source and "const float* P = p.phys;" in plain.source
    # the new unit's source enters the opt-in library's key only
    a = user_model._sources_digest(True)
    assert a != user_model._sources_digest(False)


def test_a_body_that_holds_a_parameter_in_a_float_does_not_compile(lib):
    from quattro_ilqr_amd import _lib, compile_model
    body = "const float k = P[0];\nxd[0] = u[0] - x[0] * k;"
    with pytest.raises(_lib.QuattroError) as err:
        compile_model("pfloat_rule", 1, 1, rate=body, phys=(2.0,), param_grad=True)
    text = str(err.value)
    assert "error:" in text and "user_param_gradient.hip" in text                 # the compiler's message
    assert "declared T or auto, not float" in text and "param_grad=True" in text  # the rule
    assert "float" in U.QUAD_RATE_FLOAT and "const float mass" in U.QUAD_RATE_FLOAT and "const float" not in U.QUAD_RATE_T


def test_a_plain_user_model_is_still_refused_and_told_how(lib):
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import ops, user_model
    md = user_model.example_planar_model()
    x, u = torch.zeros((2, 6, md.n)), torch.zeros((2, 5, md.m))
    with pytest.raises(NotImplementedError, match="only for the built-in models") as err:
        ops.cost_param_gradient(md, x, u)
    assert "param_grad=True" in str(err.value)
    # a model with the option passes that check: the first thing refused is then where the sequences live
    with pytest.raises(ValueError, match="must live on the GPU"):
        ops.cost_param_gradient(user_model.example_planar_model(param_grad=True), x, u)


def test_docstrings_say_which_user_models_have_row_gradients():
    pytest.importorskip("torch")
    import quattro_ilqr_amd as q
    for doc in (q.trajectory_cost.__doc__, q.autograd.__doc__, q.ops.cost_param_gradient.__doc__, q.user_model.__doc__):
        assert "param_grad=True" in doc
    assert "declared `T` or `auto`, not `float`" in q.user_model.__doc__


def _call(lib, p, x=1, u=1, B=4, N=10, lam=1, phys=0, rows=0, R=3, cost=0, gp=1, gc_=1, gr=1):
    """Every refusal comes before any launch: the pointers 1 and 16 are never dereferenced."""
    P = ctypes.c_void_p
    return getattr(lib, NAME)(None if p is None else ctypes.byref(p), P(x), P(u), B, N, P(lam), P(phys), P(rows), R, P(cost), P(gp),
                              P(gc_), P(gr), P(0))


def test_the_opt_in_library_refuses_what_the_main_library_refuses(lib):
    from quattro_ilqr_amd import _lib, models, user_model
    plain, opt = user_model.example_planar_model(), user_model.example_planar_model(param_grad=True)
    assert hasattr(ctypes.CDLL(opt.lib_path), NAME)
    olib, plib = _lib.load_for(opt), _lib.load_for(plain)
    p, builtin = opt._build_c_params(), models.quadrotor_model()._build_c_params()
    bad = _lib.ERR_BAD_ARG
    refusals = (dict(x=0), dict(u=0), dict(gp=0, gc_=0, gr=0), dict(lam=0), dict(lam=0, gc_=0, gr=0), dict(B=0), dict(B=-1), dict(N=0),
                dict(N=-3), dict(rows=16, R=0), dict(rows=16, R=-1), dict(phys=1), dict(rows=1), dict(cost=1), dict(phys=8),
                dict(rows=20), dict(cost=36), dict(phys=16, rows=16, cost=1))
    for kw in refusals:
        assert _call(olib, p, **kw) == bad, kw
        assert _call(lib, builtin, **kw) == bad, kw                     # the main library, for its own model
        assert _call(plib, p, **kw) == _lib.ERR_UNSUPPORTED, kw         # the plain library answers for its model without the kernel
    assert _call(olib, None) == bad
    assert _call(plib, p) == _lib.ERR_UNSUPPORTED and _call(lib, p) == _lib.ERR_UNSUPPORTED
    dims = _lib.ModelParams()
    ctypes.memmove(ctypes.byref(dims), ctypes.byref(p), ctypes.sizeof(p))
    dims.n = p.n + 1
    assert _call(olib, dims) == _lib.ERR_UNSUPPORTED
    assert _call(olib, builtin) == _lib.ERR_UNSUPPORTED                 # the built-in models' kernel is the main library's


# ------------------------------------------------------------------------------------------------ 4. the reference
def _pick(ref, ent, n):
    if ent[0] == "P":
        return ref["grad_phys"][:, ent[1]], ref["den_phys"][:, ent[1]]
    if ent[0] == "row":
        return ref["grad_targets"][:, ent[1], ent[2]], ref["den_targets"][:, ent[1], ent[2]]
    j = {"q": 0, "qf": n, "r": 2 * n}[ent[0]] + ent[1]
    return ref["grad_weights"][:, j], ref["den_weights"][:, j]


@pytest.mark.parametrize("name", U.NAMES)
def test_reference_is_the_total_derivative_of_the_rollout_cost(name):
    """Seed one entry with i h, re-roll out from the same x0 and u in complex arithmetic, take Im J / h: every parameter, a weight of
    each kind, an entry of a target row below the last and of the last row (which collects the terminal term when R - 1 <= N)."""
    model = U.MODELS[name]
    n, m = model.n, model.m
    worst = 0.0
    for integ in U.INTEGRATORS:
        for N, R in ((9, None), (9, 3), (9, 12), (2, 1)):
            blks, rows = model.rows(U.B_FULL, R)
            x0, u = model.inputs(N)
            x = U.rollout(model, blks, integ, x0, u)[0]                  # the fp64 rollout itself (case() rounds x to fp32)
            d = U.blocks(model, blks, integ, x, u, U.window(rows, blks, N))
            ref = U.reference(model, blks, integ, x, u, gc.adjoint(d)["costate"], rows=rows)
            Rr = 1 if rows is None else rows.shape[1]
            ents = [("P", k) for k in range(model.NP)] + [("q", 0), ("q", n - 1), ("qf", 0), ("qf", n - 1), ("r", 0), ("r", m - 1)]
            if rows is not None:
                ents += [("row", 0, 0), ("row", min(1, Rr - 1), n - 1), ("row", Rr - 1, n - 1)]
            td = U.total_derivative(dict(model=model, blks=blks, rows=rows, x0=x0, u=u), integ, ents)
            for ent, v in zip(ents, td):
                got, den = _pick(ref, ent, n)
                if ent[0] == "row" and ent[1] > N:
                    assert np.all(got == 0.0) and np.all(v == 0.0), ent     # a row past the horizon
                    continue
                if name == "grid1x1" and ent == ("P", 4):                  # the coupling of u_0 with the other controls: m = 1 has none
                    assert np.all(den == 0.0) and np.all(got == 0.0) and np.all(v == 0.0)
                    continue
                assert np.all(den > 0), (integ, N, R, ent)
                worst = max(worst, float(np.max(np.abs(got - v) / den)))
    print(f"[upgrad total derivative {name}] {worst:.1e}")
    assert worst < U.FD_BOUND, worst


@pytest.mark.parametrize("name", U.NAMES)
def test_no_parameter_derivative_of_the_rate_cancels_more_than_fourfold(name):
    worst = max(U.cancellation(U.case(name, integ, N, 3), integ) for integ in U.INTEGRATORS for N in U.HORIZONS)
    print(f"[upgrad cancellation {name}] {worst:.3f}")
    assert worst <= U.CANCEL_MAX, worst
    # the additive terms are the rate
    c = U.case(name, "rk4", 9, 3)
    f = c["model"].fns(c["blks"][0], "rk4")
    assert np.allclose(np.sum(f.rate_terms(c["x"][0, :9], c["u"][0]), axis=-1), f.rate(c["x"][0, :9], c["u"][0]), rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("name", U.NAMES)
def test_fp32_restatement_is_within_E(name):
    """Tangents formed in NumPy float32 (complex64: the imaginary part is the dual arithmetic), lambda and every term rounded to
    fp32, the sums in fp64."""
    worst = {}
    for integ in U.INTEGRATORS:
        for N in U.HORIZONS:
            for R in (None, 3, N + 1):
                c = U.case(name, integ, N, R)
                args = (c["model"], c["blks"], integ, c["x"], c["u"], c["lam"])
                errs = U.errors(U.reference(*args, rows=c["rows"], restate=True), U.reference(*args, rows=c["rows"]))
                worst = {k: max(v, worst.get(k, 0.0)) for k, v in errs.items()}
    print(f"[upgrad E {name}] " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert U.worst(worst) <= U.E[name], worst
    assert U.worst(worst) > 0.25 * U.E[name], worst                          # the recorded figure is the measured one


@pytest.mark.parametrize("mutant", U.MUTANTS)
def test_every_mutant_stands_ten_bounds_above(mutant):
    name, integ, N, R = U.TEETH[mutant]
    c = U.case(name, integ, N, R)
    args = (c["model"], c["blks"], integ, c["x"], c["u"], c["lam"])
    err = U.worst(U.errors(U.reference(*args, rows=c["rows"], mutant=mutant), U.reference(*args, rows=c["rows"])))
    print(f"[upgrad mutant {mutant!r} {name} {integ}] {err:.1e}")
    assert err >= 10.0 * U.gpu_bound(name), (err, U.gpu_bound(name))


def test_the_bound_is_the_projects_rule():
    import param_cases as pc
    assert set(U.E) == set(U.NAMES) == set(U.TEETH[m][0] for m in U.MUTANTS) | {"grid1x1", "grid16x8"}
    for name in U.NAMES:
        assert U.gpu_bound(name) == max(4.0 * U.E[name], pc.BOUNDS["sim_x"])


# ------------------------------------------------------------------------------------------------ 5. the use case's step rule
@pytest.mark.parametrize("integ", U.INTEGRATORS)
def test_the_sysid_step_rule_descends_with_the_reference_gradient_only(integ):
    c = U.sysid_case("probe", integ)
    g = U.sysid_reference_gradient(c, integ)
    down, up = U.sysid_descends(c, integ, g), U.sysid_descends(c, integ, -g)
    print(f"[upgrad sysid {integ}] halvings {down.tolist()} flipped {up.tolist()}")
    assert np.all(down >= 0) and np.all(up < 0), (down, up)
