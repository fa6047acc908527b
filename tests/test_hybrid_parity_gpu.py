"""One hybrid iteration of QuattroILQR (a predictor for the rows below the swept tail) against the fp64 composition of
tests/hybrid_cases.py, per case and operand type, through the public API only: QuattroILQR(md, N, max_iter=1, tf=tf, state_offset=off)
with the default use_graph=False, solve(x0, u_nom, x_ref=...), ops.simulate for the nominal states and ops.linearize_sweep for a swept
segment.  No graph is captured and no persistent kernel runs (a predictor makes the solve a host-driven loop).

Per (case, operand type) ONE solver object does every solve, in this order: a different nominal (so that stale rows would show), the
case's start, the teacher-forced second iteration (the controls after the ORACLE's first iteration, rounded to fp32 -- a drifting run is
never compared), and the case's start again with max_iter=2.  What is asserted:
  1. swept rows: the stack rows that hold swept steps against the oracle's tail about the device's nominal, relative Frobenius error per
     trajectory within hybrid_cases.sweep_bound; status 0;
  2. predicted rows: rows < min(T, N) against the composition fed the DEVICE's own swept rows (the predictor check is separated from the
     sweep's error): fro, worst token, worst channel within hybrid_cases.predictor_bound;
  3. row arithmetic: the swept rows that land in the horizon are the first rows of an ops.linearize_sweep segment call bit for bit
     (quad_long_T10: rows 10, 11 are the first 2 of 3); cp_batch_only is held to the same reference as every other case by 1 and 2, and
     whether it equals cp_L21 bit for bit is printed;
  4. 1 and 2 again on the teacher-forced second iteration;
  5. active mask: after solve(max_iter=2) the trajectories with iters == 1 hold the K, k of the one-iteration solve bit for bit; both
     kinds of trajectory exist;
  6. line search on the hybrid stack: fp64 closed-loop rollouts under the DEVICE's stack at every step size; on decidable trajectories
     the accepted step size is the first with cost <= J; the returned x, u, cost are the accepted candidate's within
     hybrid_cases.linesearch_bound; a non-finite candidate is never accepted; at least 4 of 5 trajectories were decidable.
tests/test_hybrid_cases_cpu.py shows what each bound is made of and that every named mistake in the composition exceeds one of them.
"""
import functools

import numpy as np
import pytest

import hybrid_cases as hc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASE_PRECISIONS = [(name, prec) for name in hc.NAMES for prec in hc.precisions(name)]
IDS = [f"{name}-{prec}" for name, prec in CASE_PRECISIONS]
RUNS = ("first", "second")                # nominal `which` of hybrid_cases.nominals: the case's start, the teacher-forced second iteration


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _host(out):
    f = lambda t: t.detach().cpu().numpy().copy()
    return dict(K=f(out["K"]), k=f(out["k"]), x=f(out["x"]), u=f(out["u"]), cost=f(out["cost"]), iters=f(out["iters"]),
                status=f(out["status"]), alpha=f(out["alpha"]))


class _BatchOnly:
    """A predictor that shows the solver only predict_batch, prompt_len and target_len: the duck-typed branch."""

    def __init__(self, tf):
        self._tf, self.prompt_len, self.target_len = tf, tf.prompt_len, tf.target_len

    def predict_batch(self, x_err, prompt):
        return self._tf.predict_batch(x_err.contiguous(), prompt.contiguous())


@functools.lru_cache(maxsize=None)
def _run(name, prec):
    """Every device result of one (case, operand type), downloaded: dict(first=, second=, two=, segment=)."""
    import quattro_ilqr_amd as q
    from quattro_ilqr_amd import ops
    cs = hc.case(name)
    md = cs.plant.device_model()
    tf = q.TransformerILQR(cs.n, cs.c, device=DEV, precision="bf16" if prec == "fp32" else prec).load_arrays(cs.w, cs.norm, cs.hp)
    assert tf.fused_kernel_covers() == (prec != "fp32")
    if cs.branch == "batch_only":
        tf = _BatchOnly(tf)
    fuses = ops.model_fuses_sweep(md)
    branch = "batch_only" if not hasattr(tf, "predict_gains") else "in_place" if fuses and cs.T + cs.S == cs.N else "segment"
    assert branch == cs.branch, (branch, cs.branch)                      # the case takes the code path it is there for
    s = q.QuattroILQR(md, cs.N, max_iter=1, tf=tf, state_offset=cs.offset, device=DEV)
    assert not s.use_graph
    s.solve(cs.prev_x0, cs.prev_u, x_ref=cs.prev_x_ref_arg)
    res = {}
    for tag, u in zip(RUNS, (cs.u, hc.second_nominal(name, prec))):
        x_nom, J = ops.simulate(md, _dev(cs.x0), _dev(u))
        res[tag] = dict(_host(s.solve(cs.x0, u, x_ref=cs.x_ref_arg)), x_nom=x_nom.double().cpu().numpy(), J=J.cpu().numpy(), u_nom=u)
        if fuses:        # the swept segment as one call of its own
            K_seg, k_seg, st = ops.linearize_sweep(md, x_nom, _dev(u), cs.N - cs.S)
            res[tag].update(K_seg=K_seg.cpu().numpy(), k_seg=k_seg.cpu().numpy(), seg_status=st.cpu().numpy())
    res["two"] = _host(s.solve(cs.x0, cs.u, x_ref=cs.x_ref_arg, max_iter=2))
    return res


def _device_tail(cs, r):
    """The device's own swept rows, all S of them: from the stack where all land in the horizon, else the segment call's."""
    if cs.keep == cs.S:
        return r["k"][:, cs.N - cs.S:].astype(np.float64), r["K"][:, cs.N - cs.S:].astype(np.float64)
    return r["k_seg"].astype(np.float64), r["K_seg"].astype(np.float64)


@pytest.mark.parametrize("name,prec", CASE_PRECISIONS, ids=IDS)
def test_swept_rows_against_the_oracle_tail(name, prec):
    cs = hc.case(name)
    for which, tag in enumerate(RUNS):
        r = _run(name, prec)[tag]
        assert not r["status"].any(), (tag, r["status"])
        ref = hc.reference(cs, r["x_nom"], r["u_nom"], prec)
        checks = []
        if cs.keep:
            checks.append(("stack", hc.swept_errors(cs, r["k"], r["K"], ref), hc.sweep_bound(name, prec, which, cs.keep)))
        if cs.keep < cs.S:             # the rows that only feed the prompt: the segment call's, which 3. ties to the stack
            assert not r["seg_status"].any()
            checks.append(("segment", hc.segment_errors(r["k_seg"], r["K_seg"], ref), hc.sweep_bound(name, prec, which)))
        for what, e, bd in checks:
            for key in ("K", "k"):
                print(f"DEVICE {name} {prec} {tag} swept {key} ({what}): " +
                      " ".join(f"{v:.1e}/{b_:.1e}" for v, b_ in zip(e[key], bd[key])))
        for what, e, bd in checks:
            for key in ("K", "k"):
                assert np.all(e[key] <= bd[key]), (tag, what, key, e[key], bd[key])


@pytest.mark.parametrize("name,prec", CASE_PRECISIONS, ids=IDS)
def test_predicted_rows_against_the_composition_on_the_device_tail(name, prec):
    cs = hc.case(name)
    bd = hc.predictor_bound(name, prec)
    worst = []
    for tag in RUNS:
        r = _run(name, prec)[tag]
        ref = hc.reference(cs, r["x_nom"], r["u_nom"], prec, tail=_device_tail(cs, r))
        assert np.isfinite(r["K"]).all() and np.isfinite(r["k"]).all()
        q = hc.predicted_errors(cs, r["k"].astype(np.float64), r["K"].astype(np.float64), ref)
        print(f"DEVICE {name} {prec} {tag} predicted rows: " + ", ".join(f"{key} {q[key]:.2e} (bound {bd[key]:.2e})" for key in hc.QUANTITIES))
        worst.append((tag, q))
    for tag, q in worst:
        for key in hc.QUANTITIES:
            assert q[key] <= bd[key], (tag, key, q, bd)


@pytest.mark.parametrize("name,prec", CASE_PRECISIONS, ids=IDS)
def test_row_arithmetic_of_the_stack(name, prec):
    cs = hc.case(name)
    res = _run(name, prec)
    for tag in RUNS:
        r = res[tag]
        assert r["K"].shape == (hc.B, cs.N, cs.m, cs.n) and r["k"].shape == (hc.B, cs.N, cs.m)
        if "K_seg" in r and cs.keep:
            rows = slice(cs.Tn, cs.Tn + cs.keep)
            assert np.array_equal(r["K"][:, rows], r["K_seg"][:, :cs.keep]) and np.array_equal(r["k"][:, rows], r["k_seg"][:, :cs.keep]), tag
            if cs.keep < cs.S:         # and not the last ones
                assert not np.array_equal(r["K"][:, rows], r["K_seg"][:, cs.S - cs.keep:])
    if name == "cp_batch_only":
        other = _run("cp_L21", prec)
        same = all(np.array_equal(res[tag][key], other[tag][key]) for tag in RUNS for key in ("K", "k"))
        print(f"DEVICE cp_batch_only {prec}: gain stacks equal cp_L21's bit for bit: {same}")


@pytest.mark.parametrize("name,prec", CASE_PRECISIONS, ids=IDS)
def test_stopped_trajectories_keep_their_rows(name, prec):
    res = _run(name, prec)
    one, two = res["first"], res["two"]
    assert np.all(one["iters"] == 1)
    stopped = two["iters"] == 1
    print(f"DEVICE {name} {prec}: iterations of solve(max_iter=2) {two['iters']}")
    assert stopped.any() and (two["iters"] == 2).any() and np.all((two["iters"] == 1) | (two["iters"] == 2))
    assert np.array_equal(two["K"][stopped], one["K"][stopped]) and np.array_equal(two["k"][stopped], one["k"][stopped])
    for key in ("x", "u", "cost", "alpha"):
        assert np.array_equal(two[key][stopped], one[key][stopped]), key
    assert not np.array_equal(two["K"][~stopped], one["K"][~stopped])       # the others were swept and predicted again


@pytest.mark.parametrize("name,prec", CASE_PRECISIONS, ids=IDS)
def test_line_search_on_the_hybrid_stack(name, prec):
    cs = hc.case(name)
    r = _run(name, prec)["first"]
    bound = hc.linesearch_bound(name, prec)
    K, k = r["K"].astype(np.float64), r["k"].astype(np.float64)
    J = cs.plant.rollout(cs.x0, cs.u)[1]
    cand = hc.candidates(cs, cs.x0, r["x_nom"], cs.u, k, K)
    want = hc.accept(J, cand)
    dec = hc.decidable(J, cand, bound)
    got = np.array([int(np.argmin(np.abs(np.array(hc.ALPHAS) - a))) if a > 0 else -1 for a in r["alpha"]])
    print(f"DEVICE {name} {prec} line search: accepted {got}, fp64 {want}, decidable {dec.astype(int)}, bound {bound:.1e}")
    assert np.all(np.abs(r["J"] - J) <= 2e-6 * np.abs(J))                 # the nominal's cost (test_short_and_odd_horizons...'s bound)
    assert dec.sum() >= hc.MIN_DECIDABLE
    assert np.array_equal(got[dec], want[dec])
    errs = np.zeros(hc.B)
    for b in range(hc.B):
        if got[b] < 0:
            assert np.array_equal(r["x"][b].astype(np.float64), r["x_nom"][b]) and np.array_equal(r["u"][b].astype(np.float64), cs.u[b])
            continue
        c = cand[got[b]]
        assert np.isfinite(c[2][b])                                       # a candidate that is non-finite in fp64 is not accepted
        errs[b] = hc.linesearch_errors((r["x"][b:b + 1], r["u"][b:b + 1], r["cost"][b:b + 1]), tuple(a[b:b + 1] for a in c))[0]
    print(f"DEVICE {name} {prec} line search: x, u, cost of the accepted candidate " + " ".join(f"{e:.1e}" for e in errs))
    assert np.all(errs <= bound), (errs, bound)
