"""ops.track_gradient, ops.track_covariance, ops.track_estimate and ops.estimate_log on the GPU at the run lengths and batch sizes of
tests/step_grid_cases.py: S a multiple of the kernels' blocks (COV_BLOCK = LOG_BLOCK = 4, QUATTRO_GRAD_BLOCK = 3), shorter than a
block, one block exactly; B = 4, 8 (no idle group) and param_cases.B_FULL (more than two waves) -- none of which
policy_cases.STEPS with B = 5 reaches.  Per (entry, model, integrator):
   1. parity: every output against the fp64 reference on every case of step_grid_cases.all_cases (the step grid, the options at
      block-multiple S, the batch grid under every kind of row), per measure below step_grid_cases.gpu_bound = max(4 x E_GRID, the
      family's floor); NaN positions of innov and innov_var exactly (log_cases.errors: a NaN on one side alone is an infinite error,
      and the positions are compared with the log's as well);
   2. rows the run did not read (N > S in every case): var_u[:, S:], grad_K[:, S:], grad_u_nom[:, S:] and grad_x_nom[:, S:] are +0.0
      on the bit pattern;
   3. the independence the kernel headers promise: at (26, 12) under heterogeneous rows, B in (4, 8, B_FULL), every trajectory equals
      its own B = 1 call bit for bit, all four entries;
   4. nothing else is written: ops.track_covariance's raw entry at S = 4 and S = 8 on one sentinel-filled arena with guard zones --
      the second output pass, whose lane rows 1 .. 3 redo the terminal slot and must store nothing.
The entries are called through the helpers of tests/test_track_gradient_gpu.py, tests/test_track_covariance_gpu.py,
tests/test_track_estimate_gpu.py and tests/test_estimate_log_gpu.py; every measured distance is printed before it is asserted, and
each item ends with its worst distance per measure and that distance's ratio to the bound."""
import ctypes

import numpy as np
import pytest

import cov_cases as cc
import grad_cases as gc
import log_cases as lc
import param_cases as pc
import policy_cases as pol
import step_grid_cases as sg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_estimate_log_gpu as t_log  # noqa: E402
import test_track_covariance_gpu as t_cov  # noqa: E402
import test_track_estimate_gpu as t_est  # noqa: E402
import test_track_gradient_gpu as t_grad  # noqa: E402

DEV = t_cov.DEV
dev32, host = t_cov.dev32, t_cov.host
OUTPUTS = {"gradient": pol.KEYS, "covariance": t_cov.ALL, "estimate": t_est.OUT, "log": t_log.ALL}
MEASURES = {"gradient": set(pol.KEYS), "covariance": set(t_cov.ALL) | {"asym"}, "estimate": set(t_est.OUT) | {"asym"},
            "log": set(t_log.ALL)}


def _pkg():
    import quattro_ilqr_amd as q
    return q


def _call(q, family, model, c, kw):
    """The entry of `family` on case c (built from the keywords kw) -> the dict of device tensors, every output asked for."""
    if family == "gradient":
        return t_grad._call(q, pc.device_model(q.models, model, kw["set_name"], kw["integ"]), c, kw.get("plant_integ"))
    if family == "covariance":
        return t_cov._call(q, pc.device_model(q.models, model, kw["set_name"], kw["integ"]), c, kw.get("plant_integ"))
    return t_est._call(q, c) if family == "estimate" else t_log._call(q, c)


def _sub(family, c, b):
    """Trajectory b of case c as a B = 1 case, under its own rows."""
    if family == "estimate":
        return t_est._sub(c, b)
    if family == "log":
        return t_log._sub(c, b)
    return {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _plus_zero(t):
    """Every entry of the float32 tensor is +0.0: the bit pattern, so that -0.0 and denormals fail."""
    return bool((t.contiguous().view(torch.int32) == 0).all())


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
@pytest.mark.parametrize("family", sg.FAMILIES)
def test_every_output_matches_the_fp64_reference_on_the_grid(family, model, integ):
    q = _pkg()
    bad, worst = [], {}
    for kw in sg.all_cases(family, model, integ):
        c = sg.build(family, model, kw)
        out = _call(q, family, model, c, kw)
        assert set(out) == set(OUTPUTS[family])
        errs = sg.reference_errors(family, model, c, host(out))
        print(f"[step grid {family} {model} {sg.case_id(kw)}] " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert set(errs) == MEASURES[family]
        if family == "log":
            assert torch.equal(out["innov"].isnan(), out["innov_var"].isnan())
            y = c["y"] if c["y"].ndim == 3 else np.repeat(c["y"][None], c["B"], axis=0)
            assert torch.equal(out["innov"].isnan(), torch.as_tensor(np.isnan(y), device=DEV)), "a NaN where there is no reading, only there"
        for k, e in errs.items():
            if not e < sg.gpu_bound(family, model, k):
                bad.append((sg.case_id(kw), k, e, sg.gpu_bound(family, model, k)))
            if e >= worst.get(k, (-1.0, None))[0]:
                worst[k] = (e, sg.case_id(kw))
    print(f"[step grid worst {family} {model} {integ}] "
          + "; ".join(f"{k} {e:.2e} = {e / sg.gpu_bound(family, model, k):.2f} x bound ({cid})" for k, (e, cid) in worst.items()))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 2. rows the run did not read
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
@pytest.mark.parametrize("family", ("gradient", "covariance"))
def test_rows_the_run_did_not_read_are_plus_zero(family, model, integ):
    q = _pkg()
    keys = ("grad_K", "grad_u_nom", "grad_x_nom") if family == "gradient" else ("var_u",)
    seen = 0
    for kw in sg.all_cases(family, model, integ):
        if kw.get("open"):
            continue                                             # without gains var_u has the run's rows alone: no tail
        c = sg.build(family, model, kw)
        out = _call(q, family, model, c, kw)
        N, S = kw["N"], kw["S"]
        assert N > S
        for key in keys:
            rows = N + 1 if key == "grad_x_nom" else N
            assert out[key].shape[1] == rows and out[key].dtype == torch.float32, (kw, key)
            tail = out[key][:, S:]
            assert tail.numel() > 0 and _plus_zero(tail), (sg.case_id(kw), key)
            assert bool((out[key][:, :S] != 0).any()), (sg.case_id(kw), key)
            seen += 1
    assert seen >= len(keys) * (len(sg.STEP_GRID) + 3)


# ------------------------------------------------------------------------------------------------ 3. independence of B
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
@pytest.mark.parametrize("family", sg.FAMILIES)
def test_a_trajectory_is_its_own_single_call_in_full_waves_and_many(family, model, integ):
    q = _pkg()
    cases = sg.batch_cases(family, model, integ)
    assert [kw["B"] for kw in cases] == [4, 8, pc.B_FULL[model]]
    for kw in cases:
        c = sg.build(family, model, kw)
        full = _call(q, family, model, c, kw)
        for key, v in full.items():
            assert v.shape[0] == kw["B"], (key, tuple(v.shape))
        for b in range(kw["B"]):
            one = _call(q, family, model, _sub(family, c, b), kw)
            assert set(one) == set(full)
            for key in full:
                t_log._same(one[key], full[key][b:b + 1], f"B={kw['B']} trajectory {b} {key}")
    # the rows differ between trajectories, so a trajectory answered with its neighbour's would be seen
    last = {k: v for k, v in full.items() if v.dim() > 1}
    assert all(not torch.equal(torch.nan_to_num(v[0]), torch.nan_to_num(v[1])) for v in last.values())


# ------------------------------------------------------------------------------------------------ 4. nothing else is written
@pytest.mark.parametrize("S", (4, 8))
@pytest.mark.parametrize("model", pc.MODELS)
def test_covariance_second_output_pass_writes_what_is_asked_for_and_nothing_else(model, S):
    """test_track_covariance_gpu.test_what_is_not_asked_for_is_not_written at S % COV_BLOCK == 0: the raw entry on one arena filled
    with a sentinel.  The outputs that are passed are written in full -- rows S of cov and var come from the second output pass --
    and equal the first call's; the ones that are not passed and the guard zones between and around them keep the sentinel."""
    q = _pkg()
    from quattro_ilqr_amd import _lib
    ALL = t_cov.ALL
    md = pc.device_model(q.models, model, "skew", "rk4")
    N = sg.N_OF[S]
    c = sg.build("covariance", model, dict(set_name="skew", integ="rk4", N=N, S=S))
    B, n, m = c["x"].shape[0], md.n, md.m
    assert S % sg.BLOCKS["covariance"] == 0 and c["x"].shape[1] == S + 1 and c["K"].shape[1] == N > S
    x, u, K, c0, w = (dev32(c[k]) for k in ("x", "u", "K", "cov0", "noise"))
    sizes = dict(cov=B * (S + 1) * n * n, var=B * (S + 1) * n, var_u=B * N * m, excess=2 * B)         # in floats
    GUARD, SENT = 64, -777.25
    at, pos = {}, GUARD
    for key in ALL:
        at[key] = pos
        pos += (sizes[key] + GUARD + 3) // 4 * 4
    lib, p = _lib.load_for(md), md.c_params()
    ref = None
    for want, flags in ((ALL, _lib.SCORE_TERMINAL), (("var",), _lib.SCORE_TERMINAL), (("cov",), _lib.SCORE_TERMINAL),
                        (("var_u", "excess"), _lib.SCORE_TERMINAL), (("excess",), _lib.SCORE_TERMINAL), (("cov", "var"), 0)):
        arena = torch.full((pos,), SENT, dtype=torch.float32, device=DEV)
        outs = [ctypes.c_void_p(arena.data_ptr() + 4 * at[key]) if key in want else ctypes.c_void_p(0) for key in ALL]
        q.ops.check(lib.quattro_track_covariance_f32(ctypes.byref(p), q.ops._ptr(x), q.ops._ptr(u), B, N, S, q.ops._ptr(K), None, None,
                                                     q.ops._ptr(c0), q.ops._ptr(w), flags, *outs, q.ops._stream()), "entry")
        torch.cuda.synchronize()
        a = arena.cpu().numpy()
        ref = a if ref is None else ref
        keep = np.ones(pos, dtype=bool)
        for key in want:
            span = slice(at[key], at[key] + sizes[key])
            keep[span] = False
            assert np.array_equal(a[span], ref[span]), (want, key)        # (cov and var do not depend on the terminal flag)
            assert not np.any(a[span] == SENT) or key == "excess", (want, key)
        assert np.all(a[keep] == SENT), want
    # what the first call wrote is the reference's, the rows of the second pass included
    got = dict(cov=ref[at["cov"]:at["cov"] + sizes["cov"]].reshape(B, S + 1, n, n).astype(np.float64),
               var=ref[at["var"]:at["var"] + sizes["var"]].reshape(B, S + 1, n).astype(np.float64),
               var_u=ref[at["var_u"]:at["var_u"] + sizes["var_u"]].reshape(B, N, m).astype(np.float64),
               excess=ref[at["excess"]:at["excess"] + sizes["excess"]].view(np.float64).copy())
    errs = cc.case_errors(c, got)
    print(f"[step grid arena {model} S={S}] " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert all(e < sg.gpu_bound("covariance", model, k) for k, e in errs.items()), errs
