"""The closed-loop covariance on the GPU (quattro_track_covariance_f32, ops.track_covariance, QuattroILQR.tube):
   5. cov, var, var_u, excess and the asymmetry of cov against the fp64 reference on every case of cov_cases.parity_cases: both
      models and integrators, N = 7 with n_steps = 7, 5 and 1, N = 26, B = 5 (a last wave with idle groups for the cart-pole), rows
      per trajectory, a plant with the other integrator, terminal off, the zero start (exact zeros) and the open loop;
   6. bit-for-bit identities: a trajectory of a batch against its own B = 1 call; K = None against K of zeros; cov0 = None and
      noise = None against zeros; var against the diagonal of cov; an output does not depend on which others are asked for; what is
      not asked for is not written (a sentinel arena through the raw entry, guard zones included);
   7. QuattroILQR.tube() against ops.track_covariance on the arrays the solve before it returned, and the keys of that solve.
The bound of 5 is cov_cases.gpu_bound: the larger of 4 x E (the fp32 restatement's distance from fp64, measured on the CPU) and the
project's fp32 floor 2e-6; every measured value is printed before it is asserted.  Reference, measures, mutants: tests/cov_cases.py,
tests/test_track_covariance_cpu.py."""
import ctypes

import numpy as np
import pytest

import cov_cases as cc
import grad_cases as gc
import param_cases as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = ("cov", "var", "var_u", "excess")


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def host(out):
    return {key: v.double().cpu().numpy() for key, v in out.items()}


def _same(a, b, tag):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b), tag


def _call(q, md, c, plant_integ=None, **over):
    """ops.track_covariance on a case of cov_cases -> the dict of device tensors."""
    kw = dict(K=dev32(c["Kc"]), plant=None if plant_integ is None else md.with_(integrator=plant_integ), plant_phys=c.get("phys"),
              weights=c.get("w"), cov0=dev32(c["cov0"]), noise=dev32(c["noise"]), terminal=c["terminal"], want=ALL)
    kw.update(over)
    return q.ops.track_covariance(md, dev32(c["x"]), dev32(c["u"]), **kw)


# ------------------------------------------------------------------------------------------------ 5. parity
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_covariance_matches_the_fp64_reference(model, integ):
    q = _pkg()
    bound = cc.gpu_bound(model)
    bad = []
    for kw in [k for k in cc.parity_cases(model) if k["integ"] == integ]:
        c = cc.case(model, **kw)
        md = pc.device_model(q.models, model, kw["set_name"], integ)
        out = _call(q, md, c, kw.get("plant_integ"))
        assert set(out) == set(ALL) and out["excess"].dtype == torch.float64 and out["cov"].dtype == torch.float32
        errs = cc.case_errors(c, host(out))
        print(f"[track cov {model} {cc.case_id(kw)}] " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert set(errs) == set(ALL) | {"asym"}
        bad += [(cc.case_id(kw), k, e) for k, e in errs.items() if not e < bound]
    assert not bad, (bound, bad)


# ------------------------------------------------------------------------------------------------ 6. identities
def _sub(c, b):
    return {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}


@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_covariance_identities_bit_for_bit(model, integ):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    c = cc.case(model, "skew", integ, 7, 5, hetero=("weights", "phys"))
    B, N, S, n, m = c["x"].shape[0], c["N"], c["S"], md.n, md.m
    full = _call(q, md, c)
    assert tuple(full["cov"].shape) == (B, S + 1, n, n) and tuple(full["var"].shape) == (B, S + 1, n)
    assert tuple(full["var_u"].shape) == (B, N, m) and tuple(full["excess"].shape) == (B,)
    # var is the diagonal of cov; rows the tracked steps did not read are +0.0
    _same(full["var"], torch.diagonal(full["cov"], dim1=2, dim2=3).contiguous(), "var is the diagonal of cov")
    tail = full["var_u"][:, S:]
    assert tail.numel() > 0 and bool((tail == 0).all()) and not bool(torch.signbit(tail).any())
    assert bool((full["var_u"][:, :S] > 0).all()) and bool((full["var"] > 0).all()) and bool((full["excess"] > 0).all())
    # every trajectory is its own B = 1 call
    for b in range(B):
        one = _call(q, md, _sub(c, b))
        for key in ALL:
            _same(one[key], full[key][b:b + 1], f"trajectory {b} {key}")
    # an output does not depend on which others are asked for
    for want in (("var",), "var", ("cov",), ("var_u",), ("excess",), ("var", "excess"), ("cov", "var_u")):
        got = _call(q, md, c, want=want)
        assert set(got) == set((want,) if isinstance(want, str) else want), want
        for key in got:
            _same(got[key], full[key], f"want={want}: {key}")
    default = q.ops.track_covariance(md, dev32(c["x"]), dev32(c["u"]), K=dev32(c["K"]))
    assert set(default) == {"var", "var_u", "excess"}
    # K = None is K of zeros; cov0 / noise = None are zeros
    zero = _call(q, md, c, K=torch.zeros((B, N, m, n), device=DEV))
    none = _call(q, md, c, K=None)
    assert tuple(none["var_u"].shape) == (B, S, m) and not bool(none["var_u"].any())
    for key in ("cov", "var", "excess"):
        _same(none[key], zero[key], f"K=None against zeros: {key}")
    _same(none["var_u"], zero["var_u"][:, :S].contiguous(), "K=None against zeros: var_u")
    zc = torch.zeros((B, n, n), device=DEV)
    for key in ALL:
        _same(_call(q, md, c, cov0=None)[key], _call(q, md, c, cov0=zc)[key], f"cov0=None against zeros: {key}")
        _same(_call(q, md, c, noise=None)[key], _call(q, md, c, noise=zc)[key], f"noise=None against zeros: {key}")
    # the forms of cov0 / noise: a diagonal is the matrix that holds it
    dg = torch.diagonal(dev32(c["noise"]), dim1=1, dim2=2).contiguous()
    _same(_call(q, md, c, noise=dg)["cov"], full["cov"], "noise as (B, n) diagonals")
    _same(_call(q, md, c, noise=dg[0].cpu().numpy())["cov"], full["cov"], "noise as one (n,) diagonal")
    _same(_call(q, md, _sub(c, 2), cov0=c["cov0"][2])["cov"], full["cov"][2:3], "cov0 as one (n, n) matrix")
    # the rows, the gains, the inputs and the terminal flag matter, each of them
    for drop in ("phys", "w", "cov0", "noise"):
        assert not torch.equal(_call(q, md, dict(c, **{drop: None}))["excess"], full["excess"]), drop
    assert not torch.equal(none["cov"], full["cov"])
    off = _call(q, md, dict(c, terminal=False))
    assert bool((off["excess"] < full["excess"]).all())
    _same(off["cov"], full["cov"], "the terminal flag enters excess alone")


@pytest.mark.parametrize("model", pc.MODELS)
def test_what_is_not_asked_for_is_not_written(model):
    """The raw entry on one arena filled with a sentinel: the outputs that are passed are written in full, the ones that are not, and
    the guard zones between and around them, keep the sentinel."""
    q = _pkg()
    from quattro_ilqr_amd import _lib
    md = pc.device_model(q.models, model, "skew", "rk4")
    c = cc.case(model, "skew", "rk4", 7, 5)
    B, N, S, n, m = c["x"].shape[0], 7, 5, md.n, md.m
    x, u, K, c0, w = (dev32(c[k]) for k in ("x", "u", "K", "cov0", "noise"))
    sizes = dict(cov=B * (S + 1) * n * n, var=B * (S + 1) * n, var_u=B * N * m, excess=2 * B)         # in floats
    GUARD, SENT = 64, -777.25
    at, pos = {}, GUARD
    for key in ALL:
        at[key] = pos
        pos += (sizes[key] + GUARD + 3) // 4 * 4
    lib, p = _lib.load_for(md), md.c_params()
    ptr = lambda t, key: ctypes.c_void_p(t.data_ptr() + 4 * at[key])
    ref = None
    for want in (ALL, ("var",), ("cov",), ("var_u", "excess"), ("excess",)):
        arena = torch.full((pos,), SENT, dtype=torch.float32, device=DEV)
        outs = [ptr(arena, key) if key in want else ctypes.c_void_p(0) for key in ALL]
        q.ops.check(lib.quattro_track_covariance_f32(ctypes.byref(p), q.ops._ptr(x), q.ops._ptr(u), B, N, S, q.ops._ptr(K), None, None,
                                                     q.ops._ptr(c0), q.ops._ptr(w), _lib.SCORE_TERMINAL, *outs, q.ops._stream()), "entry")
        torch.cuda.synchronize()
        a = arena.cpu().numpy()
        ref = a if ref is None else ref
        keep = np.ones(pos, dtype=bool)
        for key in want:
            keep[at[key]:at[key] + sizes[key]] = False
            assert np.array_equal(a[at[key]:at[key] + sizes[key]], ref[at[key]:at[key] + sizes[key]]), (want, key)
            assert not np.any(a[at[key]:at[key] + sizes[key]] == SENT) or key == "excess", (want, key)
        assert np.all(a[keep] == SENT), want


# ------------------------------------------------------------------------------------------------ 7. QuattroILQR.tube
@pytest.mark.parametrize("model", pc.MODELS)
def test_tube_is_the_entry_on_the_arrays_the_solve_returned(model):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", "rk4")
    N, B = 7, 5
    x0, u0 = pc.inputs(model, "skew", N, B)
    cov0, noise = cc.cov_inputs(model, B)
    sv = q.QuattroILQR(md, horizon=N, device=DEV, tf_window=0)
    out = sv.solve(x0, u0, max_iter=3)
    assert set(out) == {"K", "k", "x", "u", "cost", "iters", "status", "alpha"}, "a solve returns the keys it always did"
    before = {k: v.clone() for k, v in out.items()}
    tube = sv.tube(cov0=cov0, noise=noise)
    assert set(tube) == {"var", "var_u", "excess"}
    for k in before:
        _same(out[k], before[k], f"tube() leaves the solve's results alone: {k}")
    ref = q.ops.track_covariance(md, out["x"], out["u"], K=out["K"], cov0=cov0, noise=noise)
    for k in ("var", "var_u", "excess"):
        _same(tube[k], ref[k], k)
    assert tuple(tube["var"].shape) == (B, N + 1, md.n) and tuple(tube["var_u"].shape) == (B, N, md.m) and bool((tube["excess"] > 0).all())
    # one argument alone, in another form
    _same(sv.tube(noise=np.diagonal(noise[0]))["var"], q.ops.track_covariance(md, out["x"], out["u"], K=out["K"], noise=noise[0])["var"],
          "noise alone")
    # under the rows of the call: model_phys is the plant's row (the models whose solve takes rows)
    if model == "cartpole":
        phys = gc.phys_rows(model, B)
        rows = sv.solve(x0, u0, max_iter=3, model_phys=phys)
        tube = sv.tube(cov0=cov0)
        ref = q.ops.track_covariance(md, rows["x"], rows["u"], K=rows["K"], plant_phys=phys, cov0=cov0)
        for k in ("var", "var_u", "excess"):
            _same(tube[k], ref[k], f"under model_phys: {k}")
        assert not torch.equal(tube["var"], q.ops.track_covariance(md, rows["x"], rows["u"], K=rows["K"], cov0=cov0)["var"])
        sv.solve(x0, u0, max_iter=3)                    # a later plain solve forgets the rows
        _same(sv.tube(cov0=cov0)["var"], q.ops.track_covariance(md, sv.x, sv.u, K=sv.K, cov0=cov0)["var"], "rows forgotten")
