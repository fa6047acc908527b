"""Output feedback inside a tracked run on the GPU (quattro_track_estimate_f32, ops.track_estimate, QuattroILQR.fly):
   5. x, u, xhat, var, cov, nis and the asymmetry of cov against the fp64 reference on every case of est_cases.parity_cases: both
      models, every integrator pair, N = 7 with 7, 5 and 1 steps, N = 26, B = 5 (a last wave with idle groups for the cart-pole), rows
      per trajectory of all three kinds, every sensor, the None forms;
   6. bit-for-bit identities: a trajectory of a batch against its own B = 1 call under heterogeneous rows; every subset of `want`
      against the full call; what is not asked for is not written (a sentinel arena through the raw entry); None inputs against
      explicit zeros; var against the diagonal of cov;
   7. a perfectly informed estimator stays perfectly informed: xhat == x bit for bit and nis exactly +0.0, with x, u of that call
      against ops.track's;
   8. QuattroILQR.fly() against ops.track_estimate on the arrays the solve before it returned, and the keys of that solve.
The bound of 5 is est_cases.gpu_bound per measure: the larger of 4 x E (the fp32 restatement's distance from fp64, measured on the
CPU) and the floor (1e-5 for x, u, xhat: ops.track's parity bound; 2e-6 for cov, var, nis); every measured value is printed before it
is asserted.  Reference, measures, mutants: tests/est_cases.py, tests/test_track_estimate_cpu.py."""
import ctypes
import itertools

import numpy as np
import pytest

import est_cases as ec
import grad_cases as gc
import param_cases as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = ("xhat", "var", "cov", "nis")
OUT = ("x", "u") + ALL


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def host(out):
    return {key: v.double().cpu().numpy() for key, v in out.items()}


def _same(a, b, tag):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b), tag


def _model(q, c):
    return pc.device_model(q.models, c["model"], "skew", c["integ"])


def _call(q, c, **over):
    """ops.track_estimate on a case of est_cases -> the dict of device tensors."""
    md = _model(q, c)
    kw = dict(xhat0=dev32(c["xhat0"]), cov0=dev32(c["cov0"]), noise=dev32(c["noise"]), meas_noise=dev32(c["meas_noise"]),
              disturbance=dev32(c["disturbance"]), plant=None if c["plant_integ"] is None else md.with_(integrator=c["plant_integ"]),
              plant_phys=c["plant_phys"], model_phys=c["model_phys"], want=ALL)
    kw.update(over)
    meas_var = kw.pop("meas_var", c["meas_var"])
    return q.ops.track_estimate(md, dev32(c["x0"]), dev32(c["x_nom"]), dev32(c["u_nom"]), dev32(c["K"]), c["S"], c["observed"],
                                meas_var, **kw)


# ------------------------------------------------------------------------------------------------ 5. parity
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_estimate_matches_the_fp64_reference(model, integ):
    q = _pkg()
    bad = []
    for kw in [k for k in ec.parity_cases(model) if k["integ"] == integ]:
        c = ec.case(model, **kw)
        out = _call(q, c)
        assert set(out) == set(OUT) and all(v.dtype == torch.float32 for v in out.values())
        errs = ec.errors(c, host(out))
        print(f"[track est {model} {ec.case_id(kw)}] " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert set(errs) == set(OUT) | {"asym"}
        bad += [(ec.case_id(kw), k, e, ec.gpu_bound(model, k)) for k, e in errs.items() if not e < ec.gpu_bound(model, k)]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 6. identities
def _sub(c, b):
    out = dict(c)
    for k in ("x0", "x_nom", "u_nom", "K", "xhat0", "cov0", "noise", "plant_phys", "model_phys"):
        out[k] = None if c[k] is None else c[k][b:b + 1]
    for k in ("meas_noise", "disturbance"):
        out[k] = None if c[k] is None else c[k][:, b:b + 1]
    if np.ndim(c["meas_var"]) == 2:
        out["meas_var"] = c["meas_var"][b:b + 1]
    return out


@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_estimate_identities_bit_for_bit(model, integ):
    q = _pkg()
    c = ec.case(model, integ=integ, plant_integ=ec.OTHER[integ], N=7, S=5, hetero=("plant_phys", "model_phys", "meas_var"))
    B, S, n, m = c["x0"].shape[0], c["S"], c["x0"].shape[1], c["u_nom"].shape[2]
    full = _call(q, c)
    assert tuple(full["x"].shape) == (B, S + 1, n) and tuple(full["u"].shape) == (B, S, m) and tuple(full["nis"].shape) == (B, S)
    assert tuple(full["xhat"].shape) == (B, S + 1, n) == tuple(full["var"].shape) and tuple(full["cov"].shape) == (B, S + 1, n, n)
    _same(full["var"], torch.diagonal(full["cov"], dim1=2, dim2=3).contiguous(), "var is the diagonal of cov")
    _same(full["x"][:, 0].contiguous(), dev32(c["x0"]), "row 0 of x is x0")
    assert bool((full["var"] > 0).all()) and bool((full["nis"] > 0).all())
    # every trajectory is its own B = 1 call, under its own rows
    for b in range(B):
        one = _call(q, _sub(c, b))
        for key in OUT:
            _same(one[key], full[key][b:b + 1], f"trajectory {b} {key}")
    # an output does not depend on which others are asked for: every subset of want
    for r in range(len(ALL)):
        for want in itertools.combinations(ALL, r):
            got = _call(q, c, want=want)
            assert set(got) == {"x", "u"} | set(want), want
            for key in got:
                _same(got[key], full[key], f"want={want}: {key}")
    _same(_call(q, c, want="cov")["cov"], full["cov"], "want as a string")
    md = _model(q, c)
    default = q.ops.track_estimate(md, dev32(c["x0"]), dev32(c["x_nom"]), dev32(c["u_nom"]), dev32(c["K"]), S, c["observed"], c["meas_var"])
    assert set(default) == {"x", "u", "xhat", "var", "nis"}
    # None inputs are explicit zeros (xhat0: x0 itself)
    zeros = dict(cov0=torch.zeros((B, n, n), device=DEV), noise=torch.zeros((B, n, n), device=DEV),
                 meas_noise=torch.zeros((S, B, len(c["observed"])), device=DEV), disturbance=torch.zeros((S, B, n), device=DEV),
                 xhat0=dev32(c["x0"]))
    for key, z in zeros.items():
        a, b_ = _call(q, c, **{key: None}), _call(q, c, **{key: z})
        for out in OUT:
            _same(a[out], b_[out], f"{key}=None against zeros: {out}")
        assert not torch.equal(a["xhat"], full["xhat"]), f"{key} matters"
    # the forms of meas_var, cov0 and noise
    row = np.broadcast_to(c["meas_var"][0], c["meas_var"].shape)
    _same(_call(q, c, meas_var=c["meas_var"][0])["cov"], _call(q, c, meas_var=np.ascontiguousarray(row))["cov"], "meas_var (p_y,) against rows")
    dg = torch.diagonal(dev32(c["noise"]), dim1=1, dim2=2).contiguous()
    _same(_call(q, c, noise=dg)["cov"], full["cov"], "noise as (B, n) diagonals")
    # the rows matter, each of them
    for drop in ("plant_phys", "model_phys"):
        assert not torch.equal(_call(q, dict(c, **{drop: None}))["xhat"], full["xhat"]), drop
    assert not torch.equal(_call(q, c, meas_var=c["meas_var"][0])["var"], full["var"])
    assert not torch.equal(_call(q, dict(c, plant_integ=None))["x"], full["x"])


@pytest.mark.parametrize("model", pc.MODELS)
def test_what_is_not_asked_for_is_not_written(model):
    """The raw entry on one arena filled with a sentinel: the outputs that are passed are written in full, the ones that are not, and
    the guard zones between and around them, keep the sentinel."""
    q = _pkg()
    from quattro_ilqr_amd import _lib
    c = ec.case(model, integ="rk4", N=7, S=5)
    md = _model(q, c)
    B, N, S, n, m = c["x0"].shape[0], 7, 5, md.n, md.m
    x0, xn, un, K, xh0, c0, w, v, d = (dev32(c[k]) for k in ("x0", "x_nom", "u_nom", "K", "xhat0", "cov0", "noise", "meas_noise",
                                                              "disturbance"))
    mv = dev32(c["meas_var"])
    obs = (ctypes.c_int32 * len(c["observed"]))(*c["observed"])
    sizes = dict(x=B * (S + 1) * n, u=B * S * m, xhat=B * (S + 1) * n, var=B * (S + 1) * n, cov=B * (S + 1) * n * n, nis=B * S)
    GUARD, SENT = 64, -777.25
    at, pos = {}, GUARD
    for key in OUT:
        at[key] = pos
        pos += (sizes[key] + GUARD + 3) // 4 * 4
    lib, p = _lib.load_for(md), md.c_params()
    P = q.ops._ptr
    ref = None
    for want in (ALL, (), ("var",), ("cov",), ("xhat", "nis"), ("nis",)):
        arena = torch.full((pos,), SENT, dtype=torch.float32, device=DEV)
        outs = [ctypes.c_void_p(arena.data_ptr() + 4 * at[key]) if key in ("x", "u") + tuple(want) else ctypes.c_void_p(0) for key in OUT]
        q.ops.check(lib.quattro_track_estimate_f32(ctypes.byref(p), None, P(x0), P(xn), P(un), P(K), B, N, S, obs, len(c["observed"]),
                                                   P(mv), 0, P(xh0), P(c0), P(w), P(v), P(d), None, None, *outs, q.ops._stream()), "entry")
        torch.cuda.synchronize()
        a = arena.cpu().numpy()
        ref = a if ref is None else ref
        keep = np.ones(pos, dtype=bool)
        for key in ("x", "u") + tuple(want):
            keep[at[key]:at[key] + sizes[key]] = False
            assert np.array_equal(a[at[key]:at[key] + sizes[key]], ref[at[key]:at[key] + sizes[key]]), (want, key)
            assert not np.any(a[at[key]:at[key] + sizes[key]] == SENT), (want, key)
        assert np.all(a[keep] == SENT), want


# ------------------------------------------------------------------------------------------------ 7. the informed estimator
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_a_perfectly_informed_estimator_stays_perfectly_informed(model, integ):
    """xhat0 = None, no meas_noise, no disturbance, the plant equal to the model (the same rows for both), whatever cov0 and noise:
    every innovation is an exact zero, so xhat[:, :S] equals x[:, :S] bit for bit and nis is +0.0 -- the plant's step and the
    estimator's base step are one statement of the dynamics.  x, u of that call against ops.track's (state feedback: the same
    control law on the same state): the cart-pole's agree bit for bit (ops.track steps it with the same qt_step and the same fmaf
    chain), which is asserted; the quadrotor's ops.track steps on another lane mapping (rollout_quad.hip), and is held to the parity
    bound."""
    q = _pkg()
    c = ec.case(model, integ=integ, N=26, S=26, hetero=("model_phys",))
    md = _model(q, c)
    S = c["S"]
    xt, ut = q.ops.track(md, dev32(c["x0"]), dev32(c["x_nom"]), dev32(c["u_nom"]), dev32(c["K"]), S, plant_phys=c["model_phys"])
    for tag, kw in (("cov0 and noise", dict()), ("cov0 None", dict(cov0=None)), ("noise None", dict(noise=None)),
                    ("diagonals", dict(cov0=np.full(md.n, 1e-2), noise=np.full(md.n, 1e-3)))):
        out = _call(q, c, xhat0=None, meas_noise=None, disturbance=None, plant_phys=c["model_phys"], want=("xhat", "nis", "var"), **kw)
        _same(out["xhat"][:, :S].contiguous(), out["x"][:, :S].contiguous(), f"{tag}: xhat is x")
        assert not bool(out["nis"].any()) and not bool(torch.signbit(out["nis"]).any()), f"{tag}: nis is +0.0"
        assert bool((out["var"][:, 1:] > 0).all())
        ex = float(((out["x"] - xt).abs().double().cpu().numpy() / ec.pol.SPREAD[model]).max())
        eu = float((out["u"] - ut).abs().max()) / ec.U_SPREAD[model]
        print(f"[informed {model} {integ} {tag}] x {ex:.1e} u {eu:.1e} bitwise {torch.equal(out['x'], xt) and torch.equal(out['u'], ut)}")
        if model == "cartpole":
            _same(out["x"], xt, f"{tag}: x is ops.track's")
            _same(out["u"], ut, f"{tag}: u is ops.track's")
        assert ex < ec.gpu_bound(model, "x") and eu < ec.gpu_bound(model, "u"), (tag, ex, eu)
    # an estimator that is NOT informed differs (its start is off), and so does one whose plant is disturbed: the identity is not vacuous
    off = _call(q, c, meas_noise=None, disturbance=None, plant_phys=c["model_phys"], want=("xhat", "nis"))
    assert bool((off["nis"] > 0).all()) and not torch.equal(off["xhat"][:, :S], off["x"][:, :S])
    dis = _call(q, c, xhat0=None, meas_noise=None, plant_phys=c["model_phys"], want=("xhat", "nis"))
    assert bool((dis["nis"][:, 1:] > 0).all()) and not bool(dis["nis"][:, 0].any())


# ------------------------------------------------------------------------------------------------ 8. QuattroILQR.fly
@pytest.mark.parametrize("model", pc.MODELS)
def test_fly_is_the_entry_on_the_arrays_the_solve_returned(model):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", "rk4")
    N, B = 7, 5
    x0, u0 = pc.inputs(model, "skew", N, B)
    c = ec.case(model, integ="rk4", N=N)
    obs, mv = c["observed"], c["meas_var"]
    sv = q.QuattroILQR(md, horizon=N, device=DEV, tf_window=0)
    out = sv.solve(x0, u0, max_iter=3)
    assert set(out) == {"K", "k", "x", "u", "cost", "iters", "status", "alpha"}, "a solve returns the keys it always did"
    before = {k: v.clone() for k, v in out.items()}
    kw = dict(cov0=c["cov0"], noise=c["noise"], meas_noise=dev32(c["meas_noise"]), disturbance=dev32(c["disturbance"]))
    flown = sv.fly(obs, mv, **kw)
    assert set(flown) == {"x", "u", "xhat", "var", "nis"}
    for k in before:
        _same(out[k], before[k], f"fly() leaves the solve's results alone: {k}")
    ref = q.ops.track_estimate(md, out["x"][:, 0].contiguous(), out["x"], out["u"], out["K"], N, obs, mv, **kw)
    for k in flown:
        _same(flown[k], ref[k], k)
    assert tuple(flown["xhat"].shape) == (B, N + 1, md.n) and bool((flown["nis"] > 0).all())
    short = sv.fly(obs, mv, steps=3, want="cov", cov0=c["cov0"])
    assert set(short) == {"x", "u", "cov"} and tuple(short["cov"].shape) == (B, 4, md.n, md.n)
    # under the rows of the call: model_phys is the estimator's row and the plant's default (the models whose solve takes rows)
    if model == "cartpole":
        phys = gc.phys_rows(model, B)
        rows = sv.solve(x0, u0, max_iter=3, model_phys=phys)
        flown = sv.fly(obs, mv, cov0=c["cov0"])
        ref = q.ops.track_estimate(md, rows["x"][:, 0].contiguous(), rows["x"], rows["u"], rows["K"], N, obs, mv, cov0=c["cov0"],
                                   plant_phys=phys, model_phys=phys)
        for k in flown:
            _same(flown[k], ref[k], f"under model_phys: {k}")
        _same(flown["xhat"][:, :N].contiguous(), flown["x"][:, :N].contiguous(), "the plan flown by its own model is informed")
        other = sv.fly(obs, mv, cov0=c["cov0"], plant_phys=ec.model_phys_rows(model, B))
        assert not torch.equal(other["x"], flown["x"]) and bool((other["nis"][:, 1:] > 0).all())
