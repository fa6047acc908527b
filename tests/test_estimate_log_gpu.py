"""The filter and smoother over a logged run on the GPU (quattro_estimate_log_f32, ops.estimate_log):
   5. every output against the fp64 reference on every case of log_cases.parity_cases: both models and integrators, N = 7 with 7, 5 and
      1 steps, N = 26, B = 5 (a last wave with idle groups for the cart-pole), every sensor, rows per trajectory, a shared log, every
      pattern of missing readings (mixed inside one wave), the zero start; NaN positions exactly;
   6. bit-for-bit identities: a trajectory against its own B = 1 call; every subset of `want` against the full call with the smoother
      on and off (the filter's outputs do not change when the smoother runs); a shared log against the same log repeated B times; var /
      var_s against the diagonals of cov / cov_s; the last row of xs and cov_s against xhat and cov; a log without a reading;
   7. one arena with sentinels through the raw entry: what is asked for is written in full, the rest, the guard zones and everything
      beyond workspace_bytes keep the sentinel;
   8. loglik against the fp64 sum, in step and then sensor order, over the returned innov / innov_var, to 1e-12 relative;
   9. against the existing filter: the log built from an ops.track_estimate run (its x, meas_noise and u, the estimator's rows, the final
      row NaN) gives that run's xhat, var, cov and nis bit for bit;
  10. hypotheses: one shared quadrotor pose log scored under eight masses; the device's argmax loglik is the reference's.
The bound of 5 is log_cases.gpu_bound per measure: the larger of 4 x E (the fp32 restatement's distance from fp64, measured on the
CPU) and the floor (1e-5 for xhat and xs, 2e-6 for the rest); every measured value is printed before it is asserted.  Reference,
measures, mutants: tests/log_cases.py, tests/test_estimate_log_cpu.py."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import est_cases as ec
import grad_cases as gc
import log_cases as lc
import param_cases as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = lc.KEYS


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def host(out):
    return {key: v.double().cpu().numpy() for key, v in out.items()}


def _same(a, b, tag):
    """Bit for bit, a NaN equal to a NaN."""
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), tag
    assert torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)) and torch.equal(a.isnan(), b.isnan()), tag


def _model(q, c):
    return pc.device_model(q.models, c["model"], "skew", c["integ"])


def _call(q, c, smooth=True, want=ALL, **over):
    """ops.estimate_log on a case of log_cases -> the dict of device tensors."""
    kw = dict(cov0=dev32(c["cov0"]), noise=dev32(c["noise"]), model_phys=c["model_phys"], smooth=smooth, want=want)
    kw.update(over)
    y, u, xhat0, meas_var = (kw.pop(k, c[k]) for k in ("y", "u", "xhat0", "meas_var"))
    return q.ops.estimate_log(_model(q, c), dev32(y), dev32(u), c["observed"], meas_var, dev32(xhat0), **kw)


# ------------------------------------------------------------------------------------------------ 5. parity
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_estimate_log_matches_the_fp64_reference(model, integ):
    q = _pkg()
    bad = []
    for kw in [k for k in lc.parity_cases(model) if k["integ"] == integ]:
        c = lc.case(model, check=False, **kw)
        out = _call(q, c)
        assert set(out) == set(ALL) and all(v.dtype == (torch.float64 if k == "loglik" else torch.float32) for k, v in out.items())
        errs = lc.errors(c, host(out))
        print(f"[estimate log {model} {lc.case_id(kw)}] " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert set(errs) == set(ALL)
        bad += [(lc.case_id(kw), k, e, lc.gpu_bound(model, k)) for k, e in errs.items() if not e < lc.gpu_bound(model, k)]
        if kw.get("pattern") == "f":
            assert not bool(out["loglik"].any()) and not bool(out["nis"].any()), "a log without a reading: loglik and nis exactly 0.0"
            _same(out["xs"], out["xhat"], "a log without a reading: xs is xhat")
            assert bool(out["innov"].isnan().all()) and bool(out["innov_var"].isnan().all())
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 6. identities
def _sub(c, b):
    out = dict(c)
    for k in ("xhat0", "cov0", "noise", "model_phys"):
        out[k] = None if c[k] is None else c[k][b:b + 1]
    for k in ("y", "u"):
        out[k] = c[k][b:b + 1] if c[k].ndim == 3 else c[k]
    if np.ndim(c["meas_var"]) == 2:
        out["meas_var"] = c["meas_var"][b:b + 1]
    return out


@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_estimate_log_identities_bit_for_bit(model, integ):
    q = _pkg()
    c = lc.case(model, integ=integ, N=7, S=5, hetero=("model_phys", "meas_var"), check=False)
    B, S, n, p_y = c["B"], c["S"], c["n"], len(c["observed"])
    full = _call(q, c)
    for key, shape in (("xhat", (B, S + 1, n)), ("var", (B, S + 1, n)), ("cov", (B, S + 1, n, n)), ("innov", (B, S + 1, p_y)),
                       ("innov_var", (B, S + 1, p_y)), ("nis", (B, S + 1)), ("loglik", (B,)), ("xs", (B, S + 1, n)),
                       ("var_s", (B, S + 1, n)), ("cov_s", (B, S + 1, n, n))):
        assert tuple(full[key].shape) == shape, key
    _same(full["var"], torch.diagonal(full["cov"], dim1=2, dim2=3).contiguous(), "var is the diagonal of cov")
    _same(full["var_s"], torch.diagonal(full["cov_s"], dim1=2, dim2=3).contiguous(), "var_s is the diagonal of cov_s")
    _same(full["xs"][:, S].contiguous(), full["xhat"][:, S].contiguous(), "the last smoothed state is the last estimate")
    _same(full["cov_s"][:, S].contiguous(), full["cov"][:, S].contiguous(), "the last smoothed covariance is the last posterior")
    assert not torch.equal(full["xs"][:, 0], full["xhat"][:, 0]) and bool((full["var_s"] > 0).all())
    assert torch.equal(full["innov"].isnan(), torch.as_tensor(np.isnan(c["y"]), device=DEV)), "a NaN where there is no reading, nowhere else"
    # every trajectory is its own B = 1 call, under its own rows
    for b in range(B):
        one = _call(q, _sub(c, b))
        for key in ALL:
            _same(one[key], full[key][b:b + 1], f"trajectory {b} {key}")
    # an output does not depend on which others are asked for, nor the filter's on the smoother: every subset of want
    for r in range(1, len(ALL) + 1):
        for want in itertools.combinations(ALL, r):
            got = _call(q, c, want=want)
            assert set(got) == set(want), want
            for key in got:
                _same(got[key], full[key], f"want={want}: {key}")
    for r in range(1, len(lc.FILTER_KEYS) + 1):
        for want in itertools.combinations(lc.FILTER_KEYS, r):
            got = _call(q, c, smooth=False, want=want)
            assert set(got) == set(want), want
            for key in got:
                _same(got[key], full[key], f"smooth=False want={want}: {key}")
    _same(_call(q, c, want="cov_s")["cov_s"], full["cov_s"], "want as a string")
    md = _model(q, c)
    args = (dev32(c["y"]), dev32(c["u"]), c["observed"], c["meas_var"], dev32(c["xhat0"]))
    assert set(q.ops.estimate_log(md, *args)) == {"xhat", "var", "nis", "loglik"}
    assert set(q.ops.estimate_log(md, *args, smooth=True)) == {"xhat", "var", "nis", "loglik", "xs", "var_s"}
    # None inputs are explicit zeros; the rows matter
    for key in ("cov0", "noise"):
        a, b_ = _call(q, c, **{key: None}), _call(q, c, **{key: torch.zeros((B, n, n), device=DEV)})
        for out in ALL:
            _same(a[out], b_[out], f"{key}=None against zeros: {out}")
        assert not torch.equal(a["xs"], full["xs"]), f"{key} matters"
    assert not torch.equal(_call(q, dict(c, model_phys=None))["xhat"], full["xhat"])
    assert not torch.equal(_call(q, c, meas_var=c["meas_var"][0])["var"], full["var"])


@pytest.mark.parametrize("model", pc.MODELS)
def test_a_shared_log_is_the_log_repeated(model):
    q = _pkg()
    c = lc.case(model, integ="rk4", N=7, S=5, hetero=("model_phys", "meas_var"), pattern="b", shared=True, check=False)
    B = c["B"]
    shared = _call(q, c)
    rep = dict(y=np.repeat(c["y"][None], B, axis=0), u=np.repeat(c["u"][None], B, axis=0))
    for kw in (rep, dict(y=rep["y"]), dict(u=rep["u"])):
        got = _call(q, c, **kw)
        for key in ALL:
            _same(got[key], shared[key], f"{sorted(kw)} repeated: {key}")
    assert not torch.equal(shared["loglik"][0], shared["loglik"][1]), "the hypotheses differ"


# ------------------------------------------------------------------------------------------------ 7. the arena
@pytest.mark.parametrize("model", pc.MODELS)
def test_what_is_not_asked_for_is_not_written(model):
    """The raw entry on one arena filled with a sentinel: the outputs that are passed are written in full, the ones that are not, the
    guard zones between and around them and everything after workspace_bytes keep the sentinel."""
    q = _pkg()
    from quattro_ilqr_amd import _lib
    c = lc.case(model, integ="rk4", N=7, S=5, pattern="a", check=False)
    md = _model(q, c)
    B, S, n, p_y = c["B"], c["S"], md.n, len(c["observed"])
    y, u, xh0, c0, w, mv = (dev32(c[k]) for k in ("y", "u", "xhat0", "cov0", "noise", "meas_var"))
    obs = (ctypes.c_int32 * p_y)(*c["observed"])
    rows = B * (S + 1)
    sizes = dict(xhat=rows * n, var=rows * n, cov=rows * n * n, innov=rows * p_y, innov_var=rows * p_y, nis=rows, loglik=2 * B,
                 xs=rows * n, var_s=rows * n, cov_s=rows * n * n)
    lib, p = _lib.load_for(md), md.c_params()
    GUARD, SENT = 64, -777.25
    at, pos = {}, GUARD
    for key in ALL:
        at[key] = pos
        pos += (sizes[key] + GUARD + 3) // 4 * 4
    ws_at = pos
    ws_floats = {s: int(lib.quattro_estimate_log_workspace_bytes(ctypes.byref(p), B, S, p_y, s)) // 4 for s in (0, 1)}
    pos += ws_floats[1] + GUARD
    P = q.ops._ptr
    ref = None
    for want in (ALL, ("loglik",), ("nis",), ("xs",), ("var_s", "innov"), ("cov_s", "cov"), ("xhat", "var", "innov_var")):
        smooth = int(any(k in lc.SMOOTH_KEYS for k in want))
        arena = torch.full((pos,), SENT, dtype=torch.float32, device=DEV)
        outs = [ctypes.c_void_p(arena.data_ptr() + 4 * at[key]) if key in want else ctypes.c_void_p(0) for key in ALL]
        q.ops.check(lib.quattro_estimate_log_f32(ctypes.byref(p), P(y), 1, P(u), 1, B, S, obs, p_y, P(mv), 0, P(xh0), P(c0), P(w), None,
                                                 ctypes.c_void_p(arena.data_ptr() + 4 * ws_at), 4 * ws_floats[smooth], *outs,
                                                 q.ops._stream()), "entry")
        torch.cuda.synchronize()
        a = arena.cpu().numpy()
        ref = a if ref is None else ref
        keep = np.ones(pos, dtype=bool)
        keep[ws_at:ws_at + ws_floats[smooth]] = False                          # the workspace's contents are the entry's business
        for key in want:
            keep[at[key]:at[key] + sizes[key]] = False
            assert np.array_equal(a[at[key]:at[key] + sizes[key]], ref[at[key]:at[key] + sizes[key]]), (want, key)
            assert not np.any(a[at[key]:at[key] + sizes[key]] == SENT), (want, key)
        assert np.all(a[keep] == SENT), want
    # a workspace a float short of the query is refused before anything is written
    arena = torch.full((pos,), SENT, dtype=torch.float32, device=DEV)
    outs = [ctypes.c_void_p(arena.data_ptr() + 4 * at[key]) for key in ALL]
    st = lib.quattro_estimate_log_f32(ctypes.byref(p), P(y), 1, P(u), 1, B, S, obs, p_y, P(mv), 0, P(xh0), P(c0), P(w), None,
                                      ctypes.c_void_p(arena.data_ptr() + 4 * ws_at), 4 * ws_floats[1] - 4, *outs, q.ops._stream())
    torch.cuda.synchronize()
    assert st == _lib.ERR_WORKSPACE and bool((arena == SENT).all())


# ------------------------------------------------------------------------------------------------ 8. loglik
@pytest.mark.parametrize("model", pc.MODELS)
def test_loglik_is_the_fp64_sum_over_the_returned_innovations(model):
    q = _pkg()
    for kw in (dict(integ="rk4", N=26, S=26), dict(integ="euler", N=7, S=1), dict(integ="euler", N=7, S=5, pattern="f")):
        c = lc.case(model, check=False, **kw)
        out = _call(q, c, smooth=False, want=("innov", "innov_var", "loglik"))
        e, s, ll = (out[k].double().cpu().numpy() for k in ("innov", "innov_var", "loglik"))
        for b in range(c["B"]):
            acc = 0.0
            for eb, sb in zip(e[b].ravel(), s[b].ravel()):                     # step order, then sensor order
                if not math.isnan(sb):
                    acc += math.log(2.0 * math.pi * sb) + eb * eb / sb
            want = 0.0 - 0.5 * acc
            print(f"[loglik {model} {lc.case_id(kw)} b={b}] {ll[b]:.17g} against {want:.17g}")
            assert abs(ll[b] - want) <= 1e-12 * abs(want), (b, ll[b], want)


# ------------------------------------------------------------------------------------------------ 9. the existing filter
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_the_log_of_a_track_estimate_run_gives_that_runs_filter_bit_for_bit(model, integ):
    """ops.track_estimate's run turned into a log -- y_t = x_t[obs] + meas_noise_t in the device's own fp32 sum, u the run's u, the
    estimator's rows as model_phys, the final row NaN -- and filtered again: the statements (track_item, qt_step, the update), the flags
    and the bits of u are the same, so xhat, var, cov and nis[:, :S] are that run's bit for bit."""
    q = _pkg()
    e = ec.case(model, integ=integ, plant_integ=ec.OTHER[integ], N=7, S=7, hetero=("plant_phys", "model_phys", "meas_var"))
    md = pc.device_model(q.models, model, "skew", integ)
    S, obs = e["S"], list(e["observed"])
    run = q.ops.track_estimate(md, dev32(e["x0"]), dev32(e["x_nom"]), dev32(e["u_nom"]), dev32(e["K"]), S, e["observed"], e["meas_var"],
                               xhat0=dev32(e["xhat0"]), cov0=dev32(e["cov0"]), noise=dev32(e["noise"]), meas_noise=dev32(e["meas_noise"]),
                               disturbance=dev32(e["disturbance"]), plant=md.with_(integrator=ec.OTHER[integ]), plant_phys=e["plant_phys"],
                               model_phys=e["model_phys"], want=("xhat", "var", "cov", "nis"))
    y = run["x"][:, :, obs].clone()
    y[:, :S] += dev32(e["meas_noise"]).transpose(0, 1)
    y[:, S] = float("nan")
    out = q.ops.estimate_log(md, y.contiguous(), run["u"], e["observed"], e["meas_var"], dev32(e["xhat0"]), cov0=dev32(e["cov0"]),
                             noise=dev32(e["noise"]), model_phys=e["model_phys"], want=("xhat", "var", "cov", "nis"))
    for key in ("xhat", "var", "cov"):
        _same(out[key], run[key], key)
    _same(out["nis"][:, :S].contiguous(), run["nis"], "nis")
    assert not bool(out["nis"][:, S].any())


# ------------------------------------------------------------------------------------------------ 10. hypotheses
def test_the_device_scores_the_mass_hypotheses_as_the_reference_does():
    q = _pkg()
    c = lc.hypotheses_case()
    out = _call(q, c, smooth=False, want=("loglik",))
    ll, ref = out["loglik"].cpu().numpy(), c["ref"]["loglik"]
    err = float(np.max(np.abs(ll - ref) / np.abs(ref)))
    print(f"[hypotheses] loglik {ll} against {ref}: {err:.1e}")
    assert err < lc.gpu_bound("quadrotor", "loglik")
    assert int(np.argmax(ll)) == int(np.argmax(ref)) == c["best"]
