"""Scoring on the device (quattro_score_f32, ops.score, `score=` of BatchedMPC.run) on the GPU:
   5. bit-for-bit identities of the kernel with itself and with quattro_total_cost_f32: the cart-pole, the quadrotor (barrier live;
      shortcut taken) and the planar user model, B in {1, 5}, S in {1, 63, 64, 65, 130};
   6. every stage cost and every total against the fp64 oracle (cart-pole and quadrotor), heterogeneous targets and weights together,
      terminal on and off, within score_cases.BOUND = 2e-6 relative;
   7. BatchedMPC.run(score=...) against ops.score on the returned x, u, bit for bit, on every path of run.
Sequences, rows, the reference and the teeth: tests/score_cases.py, tests/test_score_cpu.py."""
import numpy as np
import pytest

import param_cases as pc
import ref_cases as rc
import score_cases as sc
import weight_cases as wc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = sc.CASES + ("planar",)


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


_CACHE = {}


def _case(case, S):
    """-> (DeviceModel, x (5, S + 1, n), u (5, S, m), rows (5, S + 1, n), weights (5, 2n + m)) as fp32 arrays; computed once per
    (case, S) and shared, never written to.  The planar user model (n = 6, m = 2; its prebuilt RK4 library) walks about rows made like
    the built-in models' with planar_batch's spreads."""
    key = (case, S)
    if key not in _CACHE:
        q = _pkg()
        B = max(sc.BATCHES)
        if case == "planar":
            from test_user_model_gpu import PHYS, planar_model
            md = planar_model("rk4")
            rows = rc.ref_rows("planar", md.x_ref, B, S + 1)
            rng = np.random.default_rng(sc.SEED + S)
            side = np.where(rc.STEP["planar"] < 0.0, -1.0, 1.0)
            x = rows + 0.3 * np.array([1, 1, 0.3, 0.5, 0.5, 0.5]) * (sc.BIAS * side + rng.standard_normal((B, S + 1, 6)))
            u = PHYS[0] * PHYS[3] / 2 + 0.2 * rng.standard_normal((B, S, 2))
            w = wc.rows_about(np.concatenate([md.q, md.qf, md.r]), B)
        else:
            md = pc.device_model(q.models, sc.model_of(case), "skew", "euler")
            x, u = sc.sequences(case, B, S)
            rows, w = sc.rows_of(case, B, S + 1), sc.weights_of(case, B)
        _CACHE[key] = (md, x.astype(np.float32), u.astype(np.float32), rows.astype(np.float32), w.astype(np.float32))
    return _CACHE[key]


def _with_row(md, wrow, xref=None):
    qv, qf, r = wc.split((md.n, md.m), wrow)
    kw = dict(q=tuple(map(float, qv)), qf=tuple(map(float, qf)), r=tuple(map(float, r)))
    if xref is not None:
        kw["x_ref"] = tuple(map(float, xref))
    return md.with_(**kw)


def _ordered_sum(stage_row):
    J = 0.0
    for v in stage_row.tolist():          # Python floats are fp64: (double)stage[b][s] added in step order
        J += v
    return J


def _same(a, b, tag):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b), tag


# ------------------------------------------------------------------------------------------------ 5. identities
@pytest.mark.parametrize("S", sc.STEPS)
@pytest.mark.parametrize("case", ALL)
def test_score_identities_bit_for_bit(case, S):
    """What the kernel must equal exactly, whatever the mapping of steps to lanes: quattro_total_cost_f32 (no rows, terminal on); the
    fp64 sum of its own stage costs in step order; itself without the stage array; B calls with B = 1; the call without rows on a
    model built on the row (R = 1); the one-step call on the model built on the row of every slot; ref_hold = 1 on rows expanded on
    the host; rows padded with their last row; and with the terminal flag off a +0.0 in slot S that the total leaves out."""
    ops = _pkg().ops
    md, x5, u5, rows5, w5 = _case(case, S)
    for B in sc.BATCHES:
        x, u, rows, w = dev32(x5[:B]), dev32(u5[:B]), rows5[:B], w5[:B]
        tag = (case, S, B)
        # no rows, terminal on: quattro_total_cost_f32
        total, stage = ops.score(md, x, u, terminal=True)
        assert total.dtype == torch.float64 and tuple(total.shape) == (B,) and stage.dtype == torch.float32
        assert tuple(stage.shape) == (B, S + 1)
        _same(total, ops.total_cost(md, x, u), (*tag, "total_cost"))
        # rows and weights, terminal on: the reference configuration of everything below
        R = min(S + 1, sc.R_SHORT)
        short = np.ascontiguousarray(rows[:, :R])
        total, stage = ops.score(md, x, u, targets=short, weights=w, terminal=True, ref_hold=sc.REF_HOLD)
        st = stage.cpu().numpy()
        for b in range(B):
            assert float(total[b]) == _ordered_sum(st[b]), (*tag, b, "ordered fp64 sum")
        t2, none = ops.score(md, x, u, targets=short, weights=w, terminal=True, ref_hold=sc.REF_HOLD, want_stage=False)
        assert none is None
        _same(t2, total, (*tag, "want_stage=False"))
        # built-in costs do not read phys: rows of it change nothing
        if case != "planar":
            phys = np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1)) * (1.0 + 0.1 * np.arange(1, B + 1, dtype=np.float32))[:, None]
            tp, sp = ops.score(md, x, u, targets=short, weights=w, model_phys=phys, terminal=True, ref_hold=sc.REF_HOLD)
            _same(tp, total, (*tag, "model_phys total")); _same(sp, stage, (*tag, "model_phys stage"))
        # B calls with B = 1 on the row slices
        for b in range(B):
            tb, sb = ops.score(md, x[b:b + 1].contiguous(), u[b:b + 1].contiguous(), targets=short[b:b + 1], weights=w[b:b + 1],
                               terminal=True, ref_hold=sc.REF_HOLD)
            _same(tb, total[b:b + 1], (*tag, b, "B = 1 total")); _same(sb, stage[b:b + 1], (*tag, b, "B = 1 stage"))
        # ref_hold = 3 against ref_hold = 1 on rows expanded on the host; short rows against rows padded with their last row
        expanded = np.ascontiguousarray(sc.window(short, S, sc.REF_HOLD))
        te, se = ops.score(md, x, u, targets=expanded, weights=w, terminal=True, ref_hold=1)
        _same(te, total, (*tag, "expanded total")); _same(se, stage, (*tag, "expanded stage"))
        if R > 1:
            cut = np.ascontiguousarray(expanded[:, :max(1, (S + 1) // 2)])
            padded = np.concatenate([cut, np.repeat(cut[:, -1:], S + 1 - cut.shape[1], axis=1)], axis=1)
            tc, sc_ = ops.score(md, x, u, targets=cut, weights=w, terminal=True)
            tp, sp = ops.score(md, x, u, targets=padded, weights=w, terminal=True)
            _same(tc, tp, (*tag, "held total")); _same(sc_, sp, (*tag, "held stage"))
        # R = 1 targets plus weights: the call without rows on the model built on the row
        one = np.ascontiguousarray(rows[:, S // 2])
        t1, s1 = ops.score(md, x, u, targets=one, weights=w, terminal=True)
        for b in range(B):
            tb, sb = ops.score(_with_row(md, w[b], one[b]), x[b:b + 1].contiguous(), u[b:b + 1].contiguous(), terminal=True)
            _same(tb, t1[b:b + 1], (*tag, b, "R = 1 total")); _same(sb, s1[b:b + 1], (*tag, b, "R = 1 stage"))
        # every slot against the one-step call on the model built on that slot's row (all slots up to S = 65; around the passes'
        # ends beyond); the terminal slot as the second slot of a one-step call
        slots = range(S + 1) if S <= 65 else (0, 1, 62, 63, 64, 65, 66, 127, 128, S - 1, S)
        for b in sorted({0, B - 1}):
            got, want = [], []
            for s in slots:
                mdl = _with_row(md, w[b], expanded[b, s])
                if s < S:
                    t, _ = ops.score(mdl, x[b:b + 1, s:s + 2].contiguous(), u[b:b + 1, s:s + 1].contiguous(), want_stage=False)
                    want.append(t[0])
                else:
                    _, s2 = ops.score(mdl, x[b:b + 1, S - 1:S + 1].contiguous(), u[b:b + 1, S - 1:S].contiguous(), terminal=True)
                    want.append(s2[0, 1].double())
                got.append(stage[b, s].double())
            _same(torch.stack(got), torch.stack(want), (*tag, b, "one-step calls"))
        # terminal off: +0.0 in slot S, and the total leaves it out
        t0, s0 = ops.score(md, x, u, targets=short, weights=w, ref_hold=sc.REF_HOLD)
        _same(s0[:, :S], stage[:, :S], (*tag, "terminal off, stage"))
        last = s0[:, S].cpu().numpy()
        assert not last.any() and not np.signbit(last).any(), (*tag, "slot S is +0.0")
        for b in range(B):
            assert float(t0[b]) == _ordered_sum(st[b, :S]), (*tag, b, "terminal off, total")


# ------------------------------------------------------------------------------------------------ 6. the oracle
@pytest.mark.parametrize("S", sc.STEPS)
@pytest.mark.parametrize("case", sc.CASES)
def test_score_against_the_fp64_oracle(case, S):
    """Heterogeneous targets (min(S + 1, 40) rows held 3 steps) and weights together, terminal on and off, B = 5: every stage[b][s]
    and every total[b] within 2e-6 relative of oracle.linearize.stage_cost / terminal_cost on the row's spec with the slot's target.
    The bound is the one test_simulate_and_total_cost asserts for costs; a NumPy float32 evaluation of the same formulas sits
    <= 3.7e-7 from fp64 on such inputs.
    Measured on an MI355X, worst over the five S, B = 5, terminal on and off; per step / per total:
      cart-pole 2.0e-7 / 6.1e-8; quadrotor with the barrier live 2.9e-7 / 1.9e-7 (the total at S = 1, one term; 6.5e-8 from S = 63 on);
      quadrotor with the shortcut taken 2.7e-7 / 9.8e-8 (S = 1; 5.8e-8 from S = 63 on)."""
    ops = _pkg().ops
    md, x, u, rows, w = _case(case, S)
    B = max(sc.BATCHES)
    R = min(S + 1, sc.R_SHORT)
    short = np.ascontiguousarray(rows[:, :R])
    win = sc.window(short, S, sc.REF_HOLD)
    for terminal in (True, False):
        total, stage = ops.score(md, dev32(x), dev32(u), targets=short, weights=w, terminal=terminal, ref_hold=sc.REF_HOLD)
        ref_stage, ref_total = sc.oracle_score(case, x.astype(np.float64), u.astype(np.float64), win, w, terminal=terminal)
        st, tt = stage.double().cpu().numpy(), total.cpu().numpy()
        live = S + 1 if terminal else S
        assert ref_stage[:, :live].min() > 0.0
        e_step = float(np.max(np.abs(st[:, :live] - ref_stage[:, :live]) / ref_stage[:, :live]))
        e_total = float(np.max(np.abs(tt - ref_total) / ref_total))
        print(f"[{case} S={S} terminal={terminal}] worst step {e_step:.2e} worst total {e_total:.2e} "
              f"(stage costs {ref_stage[:, :live].min():.3g} .. {ref_stage.max():.3g})")
        assert e_step <= sc.BOUND and e_total <= sc.BOUND, (case, S, terminal, e_step, e_total)
        if not terminal:
            assert not st[:, S].any()


# ------------------------------------------------------------------------------------------------ 7. BatchedMPC.run(score=)
RUN_B, RUN_N, RUN_STEPS = 5, 20, 6


def _run_case(model):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", "euler")
    x0, _ = rc.inputs(model, RUN_N, RUN_B)
    return q, md, x0.astype(np.float32)


def _assert_scored(q, md, out, tag, **kw):
    assert set(out) == {"x", "u", "iters", "score", "stage_cost"}, tag
    assert tuple(out["stage_cost"].shape) == (RUN_B, RUN_STEPS + 1) and tuple(out["score"].shape) == (RUN_B,)
    total, stage = q.ops.score(md, out["x"].contiguous(), out["u"].contiguous(), **kw)
    _same(out["score"], total, (*tag, "score")); _same(out["stage_cost"], stage, (*tag, "stage_cost"))
    assert bool((out["score"] > 0).all())
    return total


@pytest.mark.parametrize("model", pc.MODELS)
def test_run_score_equals_ops_score_on_what_the_run_returns(model):
    """score=True on a plain run (persistent kernel and plain host loop), with targets under preview (ref_hold = 1) and as a set-point
    schedule with replan_every = 3 (ref_hold = 3; persistent kernel, and without targets the host-driven plant loop), a dict that
    overrides; score=None leaves the dict's keys what they are."""
    q, md, x0 = _run_case(model)
    kw = dict(max_iter=20, tol=1e-3, device=DEV, tf_window=0)
    mpc = lambda: q.BatchedMPC(md, RUN_N, **kw)
    plain = mpc().run(x0, RUN_STEPS)
    assert set(plain) == {"x", "u", "iters"} and set(mpc().run(x0, RUN_STEPS, score=None)) == {"x", "u", "iters"}
    out = mpc().run(x0, RUN_STEPS, score=True)
    _same(out["x"], plain["x"], (model, "x")); _same(out["u"], plain["u"], (model, "u"))
    _assert_scored(q, md, out, (model, "plain"))
    _assert_scored(q, md, mpc().run(x0, RUN_STEPS, device_loop=False, score=True), (model, "host loop"))
    _assert_scored(q, md, mpc().run(x0, RUN_STEPS, device_loop=False, replan_every=3, feedback=True, score=True), (model, "plant loop"))
    rows = rc.skew_rows(model, RUN_B, RUN_STEPS + RUN_N + 1)
    out = mpc().run(x0, RUN_STEPS, targets=rows, preview=True, score=True)
    t_prev = _assert_scored(q, md, out, (model, "preview"), targets=rows, ref_hold=1)
    assert not torch.equal(t_prev, q.ops.score(md, out["x"].contiguous(), out["u"].contiguous())[0])       # (not against model.x_ref)
    sched = np.ascontiguousarray(rows[:, :RUN_STEPS])
    out = mpc().run(x0, RUN_STEPS, targets=sched, preview=False, replan_every=3, score=True)
    t_hold = _assert_scored(q, md, out, (model, "schedule"), targets=sched, ref_hold=3)
    assert not torch.equal(t_hold, q.ops.score(md, out["x"].contiguous(), out["u"].contiguous(), targets=sched, ref_hold=1)[0])
    # a dict overrides: other targets, a fleet's own weights (the quadrotor's too), the terminal term, a hold of its own
    w = wc.weight_rows(model, RUN_B)
    other = np.ascontiguousarray(rows[:, 3:5])
    out = mpc().run(x0, RUN_STEPS, targets=rows, score=dict(targets=other, weights=w, terminal=True, ref_hold=2))
    _assert_scored(q, md, out, (model, "override"), targets=other, weights=w, terminal=True, ref_hold=2)
    out = mpc().run(x0, RUN_STEPS, targets=rows, score=dict(targets=None))
    _assert_scored(q, md, out, (model, "override, no targets"))


def test_run_scores_weight_candidates_under_the_models_own_weights():
    """A cart-pole run with `weights=` candidates is scored under the model's q, r -- ONE evaluation cost --, not the candidates'."""
    q, md, x0 = _run_case("cartpole")
    w = wc.weight_rows("cartpole", RUN_B)
    out = q.BatchedMPC(md, RUN_N, max_iter=20, tol=1e-3, device=DEV, tf_window=0).run(x0, RUN_STEPS, weights=w, score=True)
    total = _assert_scored(q, md, out, ("cartpole", "candidates"))
    own, _ = q.ops.score(md, out["x"].contiguous(), out["u"].contiguous(), weights=w)
    assert not torch.equal(total, own)
