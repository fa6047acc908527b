"""Host-side checks of the closed-loop covariance (quattro_track_covariance_f32, ops.track_covariance, QuattroILQR.tube).  None of this
needs a GPU:
   1. the fp32 restatement of tests/cov_cases.py stays within E of the fp64 reference on every case;
   2. teeth: every mutant of the reference stands >= 10 x above the bound the GPU tests assert, in the case cov_cases.TEETH names;
   3. the definition: the reference recursion against the spread of the oracle's own closed loop from the 2n starts x0 +- h L[:, c];
      and the quadrotor kernel's operand mapping restated lane by lane (cov_cases.tile16_step) against Acl Sigma Acl^T + W;
   4. every ValueError and NotImplementedError of ops.track_covariance and QuattroILQR.tube, before anything touches the device; the
      symbol is declared, bound and exported by the main and a user-model library, and every refusal of the C entry.

Measured (fp64; restatement fp32), the worst over cov_cases.parity_cases:
   E: quadrotor cov 1.83e-6, asym 9.3e-7, var 1.83e-6, var_u 1.29e-6, excess 1.7e-7 (all at N = S = 26; <= 8.3e-7 at N = 7);
      cart-pole cov 8.6e-7, asym 2.4e-7, var 8.6e-7, var_u 1.89e-6, excess 2.6e-7.  Recorded: E = 1.9e-6 for both, GPU bound 7.6e-6.
   definition (h = 1e-3 standard deviations, skew, N = 7, B = 3; controller / plant integrator): quadrotor 1.2e-10 in all four
      pairings, cart-pole 2.0e-10; at h = 1e-2 a hundred times more (1.2e-8 / 2.0e-8), at h = 1e-4 round-off (<= 1.2e-9).
   mutants in their TEETH case (the largest measure), quadrotor / cart-pole: W added before the product 9.9e-1 / 4.1e-1, Acl of step
      t + 1 1.5e+0 / 4.3e-1, B K dropped 4.2e+2 / 6.1e+1, Acl^T Sigma Acl 7.5e+4 / 6.7e+3, W dropped 1.0 / 1.0, cov0 dropped 1.0 / 1.0,
      var_u from Sigma_{t+1} 1.3e+0 / 8.6e-1, K of step t + 1 in var_u 7.7e+7 / 1.5e+0, excess without the control term 1.0e+0 /
      1.4e-1, excess with 2 q for q 7.6e-1 / 9.4e-1, terminal term kept with the flag off 9.8e-1 / 1.6e+0."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import cov_cases as cc
import param_cases as pc

NAME = "quattro_track_covariance_f32"
OTHER = {"euler": "rk4", "rk4": "euler"}


@pytest.fixture(scope="module")
def lib():
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ 1. restatement
@pytest.mark.parametrize("model", pc.MODELS)
def test_fp32_restatement_stays_within_E(model):
    zeros = 0
    for kw in cc.parity_cases(model):
        c = cc.case(model, **kw)
        assert c["x"].shape[0] == 5
        errs = cc.case_errors(c, cc.restatement(c))
        print(f"[E {model} {cc.case_id(kw)}] " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert set(errs) == set(cc.KEYS) | {"asym"} and cc.worst(errs) <= cc.E[model], (kw, errs)
        # the reference against itself is exact, and a trajectory's reference does not depend on the batch it sits in
        own = cc.case_errors(c, c["ref"])
        assert max(own[k] for k in cc.KEYS) == 0.0 and own["asym"] < 1e-14
        one = cc.propagate({k: v[:1] for k, v in c["d"].items()}, None if c["Kc"] is None else c["Kc"][:1],
                           None if c["cov0"] is None else c["cov0"][:1], c["noise"][:1], c["Nv"], c["terminal"])
        assert all(np.array_equal(one[k], c["ref"][k][:1]) for k in cc.KEYS)
        if kw.get("cov") == "zero_start":           # exact zeros: all of Sigma_0, and Sigma_1 = W off the velocity states
            assert c["cov0"] is None and not c["ref"]["cov"][:, 0].any() and np.array_equal(c["ref"]["cov"][:, 1], c["noise"])
            assert not c["ref"]["var_u"][:, 0].any() and (c["ref"]["var"][:, 1] == 0.0).sum() == 5 * (c["x"].shape[2] // 2)
            zeros += 1
        else:
            L = np.linalg.cholesky(c["cov0"])        # dense and positive definite
            assert np.all(c["cov0"] != 0.0) and np.array_equal(c["cov0"], c["cov0"].transpose(0, 2, 1)) and L.shape == c["cov0"].shape
        if kw.get("open"):
            assert c["Kc"] is None and not c["ref"]["var_u"].any() and c["ref"]["var_u"].shape[1] == c["S"] < c["N"]
    assert zeros == 2


def test_the_measures_notice_rows_past_the_tracked_steps_and_exact_zeros():
    c = cc.case("cartpole", "skew", "euler", 7, 5)
    for v in (1e-30, -0.0):
        got = {k: a.copy() for k, a in c["ref"].items()}
        got["var_u"][0, 6] = v
        assert cc.case_errors(c, got)["var_u"] == np.inf, v
    c = cc.case("cartpole", "skew", "euler", 7, 7, cov="zero_start")
    for key, at in (("cov", (1, 1, 0, 2)), ("var", (1, 0, 1)), ("var_u", (2, 0, 0))):
        assert c["ref"][key][at] == 0.0
        got = {k: a.copy() for k, a in c["ref"].items()}
        got[key][at] = 1e-30
        assert cc.case_errors(c, got)[key] == np.inf, key
    got = {k: a.copy() for k, a in c["ref"].items()}
    got["cov"][0, 3, 1, 2] *= 1.0 + 1e-3
    e = cc.case_errors(c, got)
    assert e["asym"] > 1e-5 and e["cov"] > 1e-5 and e["var"] == 0.0


# ------------------------------------------------------------------------------------------------ 2. teeth
@pytest.mark.parametrize("model", pc.MODELS)
def test_every_mutant_stands_ten_bounds_above_the_gpu_bound(model):
    assert set(cc.TEETH[model]) == set(cc.MUTANTS) and len(cc.MUTANTS) == 11
    bound = cc.gpu_bound(model)
    assert bound == max(4.0 * cc.E[model], pc.BOUNDS["sim_x"])
    ids = [cc.case_id(k) for k in cc.parity_cases(model)]
    for name, kw in cc.TEETH[model].items():
        assert cc.case_id(kw) in ids, "a mutant's case is one the GPU parity test runs"
        c = cc.case(model, **kw)
        assert not (name.startswith("terminal") and c["terminal"])
        errs = cc.mutant_errors(c, name)
        print(f"[teeth {model}] {name} ({cc.case_id(kw)}): " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert cc.worst(errs) >= 10.0 * bound, (name, errs)


# ------------------------------------------------------------------------------------------------ 3. definition, mapping
@pytest.mark.parametrize("integ", cc.gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_reference_matches_the_spread_of_the_oracles_closed_loop(model, integ):
    for plant_integ in (integ, OTHER[integ]):
        e = cc.fd_errors(model, integ, plant_integ)
        print(f"[definition {model} {integ} plant {plant_integ}] {e:.2e}")
        assert e < cc.FD_BOUND[model], (plant_integ, e)
    assert cc.FD_BOUND[model] < 1e-3 * cc.gpu_bound(model)


def test_the_tile_mapping_of_the_quadrotor_chain_is_the_recursion():
    c = cc.case("quadrotor", "skew", "rk4", 7, 5)
    acl = c["d"]["A"] + np.matmul(c["d"]["B"], c["K"][:, :5])
    pad = lambda M: np.pad(M, ((0, 4), (0, 4)))
    for b in range(2):
        sig = c["cov0"][b]
        for t in range(5):
            nxt = cc.tile16_step(pad(sig), pad(acl[b, t]), pad(c["noise"][b]))
            assert not nxt[12:].any() and not nxt[:, 12:].any(), "the padding stays exactly zero"
            want = c["ref"]["cov"][b, t + 1]
            assert np.max(np.abs(nxt[:12, :12] - want) / np.sqrt(np.outer(np.diag(want), np.diag(want)))) < 1e-13, (b, t)
            sig = nxt[:12, :12]
    # the A operand is read as if Sigma were symmetric: with a Sigma that is not, the step is Acl Sigma^T Acl^T + W
    rng = np.random.default_rng(1)
    S, A, W = rng.standard_normal((16, 16)), rng.standard_normal((16, 16)), rng.standard_normal((16, 16))
    assert np.allclose(cc.tile16_step(S, A, W), A @ S.T @ A.T + W, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 4. host checks
@pytest.mark.parametrize("model", pc.MODELS)
def test_ops_track_covariance_raises_before_anything_touches_the_device(model):
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import models, ops
    md = models.model_by_name(model)
    n, m = md.n, md.m
    B, N, S = 3, 7, 5
    x, u, K = torch.zeros((B, S + 1, n)), torch.zeros((B, S, m)), torch.zeros((B, N, m, n))
    assert list(inspect.signature(ops.track_covariance).parameters) == [
        "model", "x", "u", "K", "plant", "plant_phys", "weights", "cov0", "noise", "terminal", "want"]
    sig = inspect.signature(ops.track_covariance).parameters
    assert sig["want"].default == ("var", "var_u", "excess") and sig["terminal"].default is True
    doc = ops.track_covariance.__doc__
    assert "Acl_t Sigma_t Acl_t^T + W" in doc and "diag(K_t Sigma_t K_t^T)" in doc and "CALLER's responsibility" in doc
    for bx, bu in ((x[:, :S], u), (x, u[:, :S - 1]), (x[:B - 1], u), (x[..., :n - 1], u), (x, torch.zeros((B, S, m + 1))),
                   (x[0], u[0]), (torch.zeros((B, 1, n)), torch.zeros((B, 0, m)))):
        with pytest.raises(ValueError, match="x must have shape"):
            ops.track_covariance(md, bx, bu, K)
    for bad in (K[:, :S - 1], K[:B - 1], K[..., :n - 1], K[:, :, 0], torch.zeros((B, N, m + 1, n))):
        with pytest.raises(ValueError, match="K must have shape"):
            ops.track_covariance(md, x, u, bad)
    for bad in (("sigma",), "variance", ("var", "K"), ()):
        with pytest.raises(ValueError, match="want must name"):
            ops.track_covariance(md, x, u, K, want=bad)
    with pytest.raises(ValueError, match="plant must be the controller's model"):
        ops.track_covariance(md, x, u, K, plant=md.with_(dt=md.dt * 2))
    for bad in (np.ones((B, len(md.phys) + 1)), np.ones((B - 1, len(md.phys)))):
        with pytest.raises(ValueError, match="plant_phys"):
            ops.track_covariance(md, x, u, K, plant_phys=bad)
    for bad in (np.ones((B, 2 * n + m - 1)), dict(Q=np.ones((B, n)))):
        with pytest.raises(ValueError, match="weights"):
            ops.track_covariance(md, x, u, K, weights=bad)
    for key in ("cov0", "noise"):
        for bad in (np.ones((n + 1,)), np.ones((B + 2, n)), np.ones((B, n, n + 1)), np.ones((n, n, n, n)), 1.0,
                    torch.ones((B, n), dtype=torch.int32)):
            with pytest.raises(ValueError, match=key):
                ops.track_covariance(md, x, u, K, **{key: bad})
    # well-formed calls pass every check, the open loop and every form of cov0 / noise included; the first thing refused is then
    # where the sequences live
    for kw in (dict(K=K), dict(), dict(K=K, plant=md.with_(integrator="rk4"), want=("cov",), terminal=False),
               dict(K=K, plant_phys=np.ones((B, len(md.phys))), weights=dict(q=np.ones(n)), cov0=np.ones(n), noise=np.ones((B, n))),
               dict(K=K, cov0=np.eye(n), noise=torch.ones((B, n, n)), want="excess")):
        with pytest.raises(ValueError, match="must live on the GPU"):
            ops.track_covariance(md, x, u, **kw)


def test_a_user_model_is_refused_before_its_library_is_loaded(monkeypatch):
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import QuattroILQR, _lib, ops, user_model
    md = user_model.example_planar_model()
    sv = QuattroILQR(md, 8, tf_window=0)
    loads = []
    monkeypatch.setattr(_lib, "load_for", lambda *a, **k: loads.append(1))
    B, S = 2, 4
    with pytest.raises(NotImplementedError, match="built-in models"):
        ops.track_covariance(md, torch.zeros((B, S + 1, md.n)), torch.zeros((B, S, md.m)))
    with pytest.raises(ValueError, match="x must have shape"):
        ops.track_covariance(md, torch.zeros((B, S, md.n)), torch.zeros((B, S, md.m)))
    with pytest.raises(NotImplementedError, match="built-in models"):
        sv.tube(noise=np.ones(md.n))
    assert not loads and sv._B is None


def test_tube_is_checked_before_anything_touches_the_device():
    """QuattroILQR.tube, the solve's side of the feature.  It is a method and not a keyword of solve(): the argument list of solve()
    is pinned by tests/test_cost_gradient_cpu.py and stays what it was."""
    pytest.importorskip("torch")
    from quattro_ilqr_amd import QuattroILQR, models
    md = models.cartpole_model()
    B, N, n = 3, 10, 4
    assert list(inspect.signature(QuattroILQR.tube).parameters) == ["self", "cov0", "noise"]
    assert "tube" not in inspect.signature(QuattroILQR.solve).parameters
    assert "ops.track_covariance" in QuattroILQR.tube.__doc__ and "QuattroILQR.tube" in QuattroILQR.solve.__doc__
    sv = QuattroILQR(md, N, tf_window=0)
    with pytest.raises(RuntimeError, match="call solve\\(\\) first"):
        sv.tube(noise=np.ones(n))
    # as after a solve of B trajectories whose arrays are never looked at: the shapes are refused first
    sv._B, sv._solved_rows = B, dict(model_phys=None, targets=None, weights=None)
    for kw in (dict(cov0=np.ones(n + 1)), dict(noise=np.ones((B + 2, n))), dict(cov0=np.ones(n), noise=np.ones((B, n + 1, n))),
               dict(cov0=1.0)):
        with pytest.raises(ValueError, match="(cov0|noise) must be"):
            sv.tube(**kw)


# ------------------------------------------------------------------------------------------------ ABI
def test_the_entry_is_declared_exported_and_bound(lib):
    from quattro_ilqr_amd import _lib
    assert NAME in entry.declared_symbols() and NAME in _lib.SIGNATURES
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES[NAME] == (I, [ctypes.POINTER(_lib.ModelParams), P, P, I, I, I, P, P, P, P, P, I, P, P, P, P, P])
    text = open(os.path.join(entry.ROOT, "include", "quattro_hip.h")).read()
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int " + NAME, text, flags=re.S).group(1)
    assert "no\n * counterpart" in comment or "no counterpart" in comment
    assert "Acl_t Sigma_t Acl_t^T + W" in comment and "READS Sigma AS SYMMETRIC" in comment
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    assert [a.split()[-1].lstrip("*") for a in args] == ["p", "x", "u", "B", "N", "n_steps", "K", "plant_phys", "cost_rows", "cov0",
                                                         "noise", "flags", "cov", "var", "var_u", "excess", "stream"]
    make = open(os.path.join(entry.PKG_DIR, "csrc", "Makefile")).read()
    assert "track_covariance.hip" in make and "FLAGS_track_covariance := -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form=1" in make


def _copy(p):
    from quattro_ilqr_amd import _lib
    c = _lib.ModelParams()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(p), ctypes.sizeof(p))
    return c


def _check_refusals(lib, p):
    """Every refusal comes before any launch: `one` (and the aligned `a16`) is never dereferenced."""
    from quattro_ilqr_amd import _lib
    null, one, a16 = ctypes.c_void_p(0), ctypes.c_void_p(1), ctypes.c_void_p(16)

    def call(p=p, x=one, u=one, B=4, N=10, S=7, K=one, phys=null, cost=null, c0=one, w=one, flags=1, cov=one, var=one, vu=one, ex=one):
        return getattr(lib, NAME)(None if p is None else ctypes.byref(p), x, u, B, N, S, K, phys, cost, c0, w, flags, cov, var, vu, ex,
                                  null)

    bad = _lib.ERR_BAD_ARG
    assert call(x=null) == bad and call(u=null) == bad
    for kw in (dict(B=0), dict(B=-1), dict(N=0), dict(N=-3), dict(S=0), dict(S=-1), dict(S=11), dict(N=6)):
        assert call(**kw) == bad, kw
    assert call(cov=null, var=null, vu=null, ex=null) == bad                # at least one output
    for kw in (dict(phys=one), dict(cost=one), dict(phys=ctypes.c_void_p(8)), dict(cost=ctypes.c_void_p(36)), dict(phys=a16, cost=one)):
        assert call(**kw) == bad, kw
    for flags in (2, 3, -1, 1 << 30):
        assert call(flags=flags) == bad, flags
    # the optional arguments may be NULL; these are refusals of other arguments
    assert call(K=null, c0=null, w=null, cov=null, var=null, vu=null, x=null) == bad
    assert call(K=null, c0=null, w=null, var=null, S=0) == bad
    # the model check comes first, as quattro_total_cost_f32 makes it
    assert call(p=None) == bad
    unknown = _copy(p)
    unknown.model_id = 77
    dims = _copy(p)
    dims.n = p.n + 1
    for q in (unknown, dims):
        for kw in (dict(), dict(x=null), dict(B=0), dict(S=11), dict(K=null), dict(cost=one), dict(flags=2),
                   dict(cov=null, var=null, vu=null, ex=null)):
            assert call(p=q, **kw) == _lib.ERR_UNSUPPORTED, kw
            assert lib.quattro_total_cost_f32(ctypes.byref(q), one, one, 4, 10, one, null) == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("model", pc.MODELS)
def test_the_entry_refuses_bad_arguments_before_any_launch(lib, model):
    from quattro_ilqr_amd import models
    _check_refusals(lib, models.model_by_name(model)._build_c_params())


def test_user_model_library_exports_the_entry_and_answers_unsupported(lib):
    from quattro_ilqr_amd import _lib, user_model
    md = user_model.example_planar_model()
    assert hasattr(ctypes.CDLL(md.lib_path), NAME)
    ulib = _lib.load_for(md)
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(1)
    p = md._build_c_params()
    args = (one, one, 4, 10, 7, one, null, null, one, one, 1, one, one, one, one, null)
    # its own model: unsupported whatever else is passed; through the main library the block is an unknown model
    assert getattr(ulib, NAME)(ctypes.byref(p), *args) == _lib.ERR_UNSUPPORTED
    assert getattr(ulib, NAME)(ctypes.byref(p), null, *args[1:]) == _lib.ERR_UNSUPPORTED
    assert getattr(lib, NAME)(ctypes.byref(p), *args) == _lib.ERR_UNSUPPORTED
    assert getattr(ulib, NAME)(None, *args) == _lib.ERR_BAD_ARG
    # the kernel unit is the main library's alone: the build list of a user-model library is what it was
    assert "track_covariance" not in user_model._all_units()
    # a built-in model's block given to a user-model library: checked like any call, then refused without a launch
    from quattro_ilqr_amd import models
    q = models.cartpole_model()._build_c_params()
    assert getattr(ulib, NAME)(ctypes.byref(q), null, *args[1:]) == _lib.ERR_BAD_ARG
    assert getattr(ulib, NAME)(ctypes.byref(q), *args) == _lib.ERR_UNSUPPORTED
