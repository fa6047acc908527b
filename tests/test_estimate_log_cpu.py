"""Host-side checks of the filter and smoother over a logged run (quattro_estimate_log_f32, ops.estimate_log).  None of this needs a GPU:
   1. the cases stand (log_cases.case asserts on the fp64 reference: s >= R, 0 < var_s <= var, the smoother does something, Bryson-Frazier
      = Rauch-Tung-Striebel to 1e-9, sequential = batch Joseph to 1e-12), and the fp32 restatement stays within E of the fp64
      reference, measure by measure, on every case; a log without a reading is pure prediction, loglik exactly 0.0, xs == xhat;
   2. teeth: every mutant of the reference stands >= 10 x above the bound the GPU tests assert, in the case log_cases.TEETH names; the
      hypotheses case picks the row nearest the truth with a gap of >= 100 GPU bounds;
   3. every ValueError and NotImplementedError of ops.estimate_log, before anything touches the device;
   4. the two symbols are declared, bound and exported by the main and a user-model library, SIGNATURES is pinned, and every refusal
      of the C entry and the workspace query, a short workspace among them, with pointers that are never dereferenced.

Measured (fp64; restatement fp32), the worst over log_cases.parity_cases:
   Bryson-Frazier against Rauch-Tung-Striebel <= 1e-9 (asserted per case), sequential against batch <= 1e-12 (asserted per case).
   E: quadrotor xhat 2.3e-6, xs 2.3e-6, cov 3.1e-6, var 3.1e-6, cov_s 5.1e-5, var_s 1.1e-5, innov 6.7e-5, innov_var 1.2e-6, nis 4.6e-5,
      loglik 9.9e-6; cart-pole xhat 6.3e-7, xs 6.6e-7, cov 1.1e-6, var 1.1e-6, cov_s 7.9e-7, var_s 7.9e-7, innov 8.7e-6, innov_var
      4.7e-7, nis 3.4e-5, loglik 1.3e-5.  The smallest var_s / var: 0.062 (quadrotor, S = 26), 0.31 (cart-pole).
   mutants in their TEETH case, the measure that stands highest above its GPU bound (quadrotor / cart-pole, in bounds): u of step
      t + 1 xhat 3.3e+4 / 2.6e+4; a missing reading updates P var_s 1.6e+5 / cov_s 2.0e+5; a missing reading is counted nis inf / inf
      (a step without a reading has nis exactly 0); R left out of s innov_var 1.7e+5 / nis 1.3e+6; loglik without ln s 3.7e+4 / 2.7e+4;
      loglik without 2 pi 7.5e+3 / 5.3e+3; no update at t = S innov inf / inf (a NaN for a number); A r for A^T r xs 4.6e+4 / 1.7e+5;
      A_t for A_{t-1} var_s 3.5e+3 / cov_s 9.6e+2; updates in forward order var_s 2.2e+3 / cov_s 1.0e+3; 1 / s dropped var_s 1.9e+5 /
      cov_s 6.7e+5; c dropped var_s 1.7e+5 / cov_s 3.5e+5; k^T r dropped xs 8.9e+4 / 4.1e+3; sign of e / s xs 3.8e+4 / 7.0e+3; Lambda
      not carried var_s 1.9e+5 / cov_s 7.8e+4; xs from the prior covariance xs 6.4e+4 / 1.3e+4; cov - cov Lambda var_s 8.8e+8 / 1.3e+10.
   hypotheses: loglik 618.9 .. 676.9 over the eight masses, the best is row 4 (1.010 of the truth), 110 GPU bounds above the second."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import log_cases as lc
import param_cases as pc

NAME, QUERY = "quattro_estimate_log_f32", "quattro_estimate_log_workspace_bytes"


@pytest.fixture(scope="module")
def lib():
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ 1. cases and restatement
@pytest.mark.parametrize("model", pc.MODELS)
def test_fp32_restatement_stays_within_E(model):
    kinds = set()
    for kw in lc.parity_cases(model):
        c = lc.case(model, **kw)                                               # (asserts what the module docstring lists)
        errs = lc.errors(c, lc.restatement(c))
        print(f"[E {model} {lc.case_id(kw)}] " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert set(errs) == set(lc.KEYS)
        assert all(errs[k] <= lc.E[model][k] for k in errs), (kw, errs)
        assert max(lc.errors(c, c["ref"]).values()) == 0.0
        ref = c["ref"]
        assert np.array_equal(np.isnan(ref["innov"]), np.isnan(np.broadcast_to(c["y"], ref["innov"].shape)))
        assert np.array_equal(ref["xs"][:, -1], ref["xhat"][:, -1]) and np.array_equal(ref["cov_s"][:, -1], ref["cov"][:, -1])
        if kw.get("pattern") == "f":
            assert np.all(ref["loglik"] == 0.0) and not ref["nis"].any() and np.array_equal(ref["xs"], ref["xhat"])
            assert np.array_equal(ref["cov_s"], ref["cov"])
        one = lc.case(model, B=1, check=False, **kw)["ref"]
        assert all(np.array_equal(one[k], ref[k][:1], equal_nan=True) for k in lc.KEYS), "a trajectory does not depend on its batch"
        kinds.add((len(c["observed"]), np.ndim(c["meas_var"]), c["y"].ndim, c["cov0"] is None, c["pattern"]))
    n = pc.DIMS[model][0]
    assert {k[0] for k in kinds} == {1, n // 2, n} and {k[1] for k in kinds} == {1, 2} and {k[2] for k in kinds} == {2, 3}
    assert {k[3] for k in kinds} == {True, False} and {k[4] for k in kinds} == {"mixed", "a", "b", "e", "f"}
    m = lc.missing_mask("mixed", 5, 7, 2)
    assert not m[0].any() and m[1, 1:3, 0].all() and m[2, 2].all() and m[3, 7].all() and m[4, 1::2, 0].all() and not m[4, ::2].any()


# ------------------------------------------------------------------------------------------------ 2. teeth
@pytest.mark.parametrize("model", pc.MODELS)
def test_every_mutant_stands_ten_bounds_above_the_gpu_bound(model):
    assert set(lc.TEETH[model]) == set(lc.MUTANTS) and len(lc.MUTANTS) == 17
    for key in lc.KEYS:
        assert lc.gpu_bound(model, key) == max(4.0 * lc.E[model][key], 1e-5 if key in ("xhat", "xs") else 2e-6)
    ids = [lc.case_id(k) for k in lc.parity_cases(model)]
    cache = {}
    for name, kw in lc.TEETH[model].items():
        assert lc.case_id(kw) in ids, "a mutant's case is one the GPU parity test runs"
        c = cache.setdefault(lc.case_id(kw), lc.case(model, check=False, **kw))
        errs = lc.mutant_errors(c, name)
        over = lc.over_bound(model, errs)
        print(f"[teeth {model}] {name}: {over:.1e} bounds; " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert over >= 10.0, (name, errs)


def test_the_hypotheses_case_picks_the_mass_nearest_the_truth():
    c = lc.hypotheses_case()                                                   # (asserts the argmax and the gap)
    assert c["y"].shape == (lc.HYP_S + 1, 6) and c["u"].shape == (lc.HYP_S, 4) and c["model_phys"].shape == (lc.HYP_B, 7)
    assert np.all(c["model_phys"][:, 1:] == c["model_phys"][0, 1:]) and len(set(c["model_phys"][:, 0])) == lc.HYP_B
    assert abs(lc.HYP_MASS[c["best"]] - 1.0) < 0.02 and lc.HYP_MASS[0] == 0.85 and abs(lc.HYP_MASS[-1] - 1.15) < 1e-12


# ------------------------------------------------------------------------------------------------ 3. host checks
@pytest.mark.parametrize("model", pc.MODELS)
def test_ops_estimate_log_raises_before_anything_touches_the_device(model):
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import models, ops
    md = models.model_by_name(model)
    n, m = md.n, md.m
    B, S = 3, 5
    obs, mv = (0, 2), np.array([1e-4, 2e-4])
    y, u, xh0 = torch.zeros((B, S + 1, 2)), torch.zeros((B, S, m)), torch.zeros((B, n))
    sig = inspect.signature(ops.estimate_log).parameters
    assert list(sig) == ["model", "y", "u", "observed", "meas_var", "xhat0", "cov0", "noise", "model_phys", "smooth", "want"]
    assert sig["want"].default == ("xhat", "var", "nis", "loglik") and sig["smooth"].default is False
    assert all(sig[k].default is None for k in ("cov0", "noise", "model_phys"))
    doc = ops.estimate_log.__doc__
    assert "REVERSE order" in doc and "CALLER's responsibility" in doc and "untouched bit for bit" in doc
    call = lambda *a, **k: ops.estimate_log(md, *a, **k)
    for bad in (("sigma",), "variance", ("var", "x"), ()):
        with pytest.raises(ValueError, match="want must name"):
            call(y, u, obs, mv, xh0, want=bad)
    for bad in ("xs", ("xhat", "var_s"), ("cov_s",)):
        with pytest.raises(ValueError, match="need smooth=True"):
            call(y, u, obs, mv, xh0, want=bad)
    for bad in (torch.zeros((B, S, m + 1)), torch.zeros((S,)), torch.zeros((B, 0, m)), torch.zeros((1, B, S, m))):
        with pytest.raises(ValueError, match="u must have shape"):
            call(y, bad, obs, mv, xh0)
    for bad in (torch.zeros((B, S, 2)), torch.zeros((B, S + 1, 3)), torch.zeros((S + 2, 2)), torch.zeros((2,))):
        with pytest.raises(ValueError, match="y must have shape"):
            call(bad, u, obs, mv, xh0)
    for bad in (torch.zeros((B, n + 1)), torch.zeros((n,)), torch.zeros((0, n))):
        with pytest.raises(ValueError, match="xhat0 must have shape"):
            call(y, u, obs, mv, bad)
    with pytest.raises(ValueError, match="y must have 2 trajectories"):
        call(y, u[:2], obs, mv, xh0[:2])
    with pytest.raises(ValueError, match="u must have 4 trajectories"):
        call(y[0], u, obs, mv, torch.zeros((4, n)))
    for bad in ((), (0, 0), (2, 0), (-1, 2), (0, n), (0.5, 2.0), 3, None):
        with pytest.raises(ValueError, match="observed must be"):
            call(y, u, bad, mv, xh0)
    for bad in (np.ones(3), np.ones((B + 1, 2)), 1.0, "r", torch.ones(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="meas_var must"):
            call(y, u, obs, bad, xh0)
    for bad in ((0.0, 1e-4), (-1e-4, 1e-4), (np.nan, 1e-4), (np.inf, 1e-4), (1e-60, 1e-4)):
        with pytest.raises(ValueError, match="meas_var must be finite and > 0"):
            call(y, u, obs, bad, xh0)
    for key in ("cov0", "noise"):
        for bad in (np.ones((n + 1,)), np.ones((B + 2, n)), np.ones((B, n, n + 1)), 1.0, torch.ones((B, n), dtype=torch.int32)):
            with pytest.raises(ValueError, match=key):
                call(y, u, obs, mv, xh0, **{key: bad})
    for bad in (np.ones((B, len(md.phys) + 1)), np.ones((B - 1, len(md.phys)))):
        with pytest.raises(ValueError, match="model_phys"):
            call(y, u, obs, mv, xh0, model_phys=bad)
    with pytest.raises(ValueError, match="y must be a float32 device tensor"):
        call(np.zeros((S + 1, 2), dtype=np.float32), u, obs, mv, xh0)
    # well-formed calls pass every check, in every form of the arguments; the first thing refused is then where they live
    ph = np.ones((B, len(md.phys)))
    for args, kw in (((y, u), dict()), ((y[0], u), dict(want="cov")), ((y, u[0]), dict(smooth=True)),
                     ((y[0], u[0]), dict(smooth=True, want=lc.KEYS, cov0=np.ones(n), noise=np.ones((B, n)), model_phys=ph)),
                     ((y, u), dict(cov0=np.eye(n), noise=torch.ones((B, n, n)), want=("loglik",)))):
        with pytest.raises(ValueError, match="must live on the GPU"):
            call(*args, obs, mv, xh0, **kw)


def test_a_user_model_is_refused_before_its_library_is_loaded(monkeypatch):
    torch = pytest.importorskip("torch")
    from quattro_ilqr_amd import _lib, ops, user_model
    md = user_model.example_planar_model()
    loads = []
    monkeypatch.setattr(_lib, "load_for", lambda *a, **k: loads.append(1))
    B, S = 2, 4
    args = (torch.zeros((B, S + 1, 1)), torch.zeros((B, S, md.m)))
    with pytest.raises(NotImplementedError, match="built-in models"):
        ops.estimate_log(md, *args, (0,), (1e-4,), torch.zeros((B, md.n)))
    with pytest.raises(ValueError, match="observed must be"):
        ops.estimate_log(md, *args, (md.n,), (1e-4,), torch.zeros((B, md.n)))
    assert not loads


# ------------------------------------------------------------------------------------------------ 4. ABI
ARGS = ["p", "y", "y_rows", "u", "u_rows", "B", "n_steps", "observed", "p_y", "meas_var", "meas_var_rows", "xhat0", "cov0", "noise",
        "model_phys", "workspace", "workspace_bytes", "xhat", "var", "cov", "innov", "innov_var", "nis", "loglik", "xs", "var_s", "cov_s",
        "stream"]


def test_the_entries_are_declared_exported_and_bound(lib):
    from quattro_ilqr_amd import _lib
    P, I, M, Z = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_lib.ModelParams), ctypes.c_size_t
    for name in (NAME, QUERY):
        assert name in entry.declared_symbols() and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.SIGNATURES[QUERY] == (Z, [M, I, I, I, I])
    assert _lib.SIGNATURES[NAME] == (I, [M, P, I, P, I, I, I, ctypes.POINTER(ctypes.c_int32), I, P, I, P, P, P, P, P, Z] + [P] * 11)
    text = open(os.path.join(entry.ROOT, "include", "quattro_hip.h")).read()
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*size_t " + QUERY, text, flags=re.S).group(1)
    assert "no counterpart" in comment and "REVERSE order" in comment and "READ AS SYMMETRIC" in comment
    assert "QUATTRO_ERR_WORKSPACE" in comment and "QUATTRO_ERR_UNSUPPORTED" in comment and "untouched bit for bit" in comment
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    make = open(os.path.join(entry.PKG_DIR, "csrc", "Makefile")).read()
    assert "estimate_log.hip" in make and "FLAGS_estimate_log := -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form=1" in make


def _copy(p):
    from quattro_ilqr_amd import _lib
    c = _lib.ModelParams()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(p), ctypes.sizeof(p))
    return c


def _caller(lib, p):
    """-> call(**overrides): the entry with device pointers that are never dereferenced (`a16`) and a valid host `observed`."""
    null, a16 = ctypes.c_void_p(0), ctypes.c_void_p(16)

    def call(p=p, y=a16, yr=1, u=a16, ur=1, B=4, S=7, obs=(0, 2), p_y=None, mv=a16, rows=0, xh0=a16, c0=null, w=null, mphys=null, ws=a16,
             ws_bytes=None, smooth=False, xhat=a16, var=null, cov=null, innov=null, innov_var=null, nis=null, loglik=a16, xs=null, var_s=null,
             cov_s=null):
        arr = None if obs is None else (ctypes.c_int32 * max(1, len(obs)))(*obs)
        py = (0 if obs is None else len(obs)) if p_y is None else p_y
        if smooth:
            xs = a16
        if ws_bytes is None:
            ws_bytes = 1 << 40
        return getattr(lib, NAME)(None if p is None else ctypes.byref(p), y, yr, u, ur, B, S, arr, py, mv, rows, xh0, c0, w, mphys, ws, ws_bytes,
                                  xhat, var, cov, innov, innov_var, nis, loglik, xs, var_s, cov_s, null)
    return call


def _check_refusals(lib, p):
    """Every refusal comes before any launch: the pointers are never dereferenced."""
    from quattro_ilqr_amd import _lib
    null, one, a16 = ctypes.c_void_p(0), ctypes.c_void_p(1), ctypes.c_void_p(16)
    call = _caller(lib, p)
    bad, short, n = _lib.ERR_BAD_ARG, _lib.ERR_WORKSPACE, p.n
    query = lambda *a: int(getattr(lib, QUERY)(ctypes.byref(p), *a))
    for key in ("y", "u", "mv", "xh0"):
        assert call(**{key: null}) == bad, key
    assert call(obs=None, p_y=2) == bad
    for kw in (dict(B=0), dict(B=-1), dict(S=0), dict(S=-3), dict(yr=2), dict(yr=-1), dict(ur=2), dict(ur=-1), dict(rows=2), dict(rows=-1)):
        assert call(**kw) == bad, kw
    for kw in (dict(obs=(), p_y=0), dict(p_y=-1), dict(obs=tuple(range(n)) + (n,)), dict(p_y=n + 1), dict(obs=(0, n)), dict(obs=(-1, 2)),
               dict(obs=(2, 2)), dict(obs=(2, 0)), dict(obs=(0, 2, 1))):
        assert call(**kw) == bad, kw
    for kw in (dict(mphys=one), dict(mphys=ctypes.c_void_p(36)), dict(smooth=True, u=one), dict(smooth=True, xhat=ctypes.c_void_p(24))):
        assert call(**kw) == bad, kw
    assert call(xhat=null, loglik=null) == bad, "no output at all"
    # the workspace: the query's size is enough, a byte less is refused, and so is a NULL or misaligned one; the query grows with smooth
    for smooth in (False, True):
        need = query(4, 7, 2, int(smooth))
        assert need > 0 and need % 16 == 0
        assert call(smooth=smooth, ws_bytes=need - 1) == short and call(smooth=smooth, ws_bytes=0) == short
        assert call(smooth=smooth, ws=null) == short and call(smooth=smooth, ws=ctypes.c_void_p(24)) == short
    np_ = 16 if n > 4 else 4
    rows, readings = 4 * 8, 4 * 8 * 2
    assert query(4, 7, 2, 0) == 4 * 2 * readings
    assert query(4, 7, 2, 1) == 4 * (readings * (np_ + 4) + 2 * readings + rows * n + rows * n * n)
    assert call(smooth=True, ws_bytes=query(4, 7, 2, 0)) == short, "the filter's workspace is too short for the smoother"
    assert query(0, 7, 2, 0) == 0 and query(4, 0, 2, 1) == 0 and query(4, 7, 0, 0) == 0 and query(4, 7, n + 1, 1) == 0
    # refusals of other arguments come before the workspace's
    assert call(B=0, ws=null) == bad and call(obs=(2, 0), ws_bytes=0) == bad
    # the model check comes first, as quattro_total_cost_f32 makes it
    assert call(p=None) == bad
    unknown = _copy(p)
    unknown.model_id = 77
    dims = _copy(p)
    dims.n = p.n + 1
    for q in (unknown, dims):
        for kw in (dict(), dict(y=null), dict(B=0), dict(obs=(2, 0)), dict(mphys=one), dict(ws=null), dict(rows=3)):
            assert call(p=q, **kw) == _lib.ERR_UNSUPPORTED, kw
        assert int(getattr(lib, QUERY)(ctypes.byref(q), 4, 7, 2, 1)) == 0
    other = _copy(p)
    other.integrator = 5
    assert call(p=other) == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("model", pc.MODELS)
def test_the_entry_refuses_bad_arguments_before_any_launch(lib, model):
    from quattro_ilqr_amd import models
    _check_refusals(lib, models.model_by_name(model)._build_c_params())


def test_user_model_library_exports_the_entries_and_answers_unsupported(lib):
    from quattro_ilqr_amd import _lib, models, user_model
    md = user_model.example_planar_model()
    assert hasattr(ctypes.CDLL(md.lib_path), NAME) and hasattr(ctypes.CDLL(md.lib_path), QUERY)
    ulib = _lib.load_for(md)
    null = ctypes.c_void_p(0)
    p = md._build_c_params()
    # its own model: unsupported whatever else is passed; through the main library the block is an unknown model
    assert _caller(ulib, p)() == _lib.ERR_UNSUPPORTED and _caller(ulib, p)(y=null) == _lib.ERR_UNSUPPORTED
    assert _caller(ulib, p)(obs=(3, 1)) == _lib.ERR_UNSUPPORTED and _caller(ulib, p)(ws=null) == _lib.ERR_UNSUPPORTED
    assert _caller(lib, p)() == _lib.ERR_UNSUPPORTED
    assert _caller(ulib, p)(p=None) == _lib.ERR_BAD_ARG
    assert int(getattr(ulib, QUERY)(ctypes.byref(p), 4, 7, 1, 1)) == 0 and int(getattr(lib, QUERY)(ctypes.byref(p), 4, 7, 1, 1)) == 0
    # the kernel unit is the main library's alone: the build list of a user-model library is what it was
    assert "estimate_log" not in user_model._all_units()
    # a built-in model's block given to a user-model library: checked like any call, then refused without a launch
    q = models.cartpole_model()._build_c_params()
    assert _caller(ulib, q)(y=null) == _lib.ERR_BAD_ARG and _caller(ulib, q)(obs=(2, 0)) == _lib.ERR_BAD_ARG
    assert _caller(ulib, q)(ws_bytes=0) == _lib.ERR_WORKSPACE
    assert _caller(ulib, q)() == _lib.ERR_UNSUPPORTED
    assert int(getattr(ulib, QUERY)(ctypes.byref(q), 4, 7, 2, 1)) == int(getattr(lib, QUERY)(ctypes.byref(q), 4, 7, 2, 1)) > 0
