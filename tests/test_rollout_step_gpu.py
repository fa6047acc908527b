"""The quadrotor rollout step (csrc/rollout_quad_body.h) at the shapes and in the properties the rest of the suite leaves open.
Quadrotor only, Euler and RK4, the `skew` and `skew_nobarrier` sets of tests/param_cases.py (all inertias, weights and controls
distinct; the second set takes the barrier flag's other arm), inputs from param_cases.inputs, B <= 19, N <= 7.

  1. alpha = 0 is simulate, bit for bit: the closed-loop rollout (quad_rollout_closed, unrolled by four) and the open-loop one
     (simulate_quad_body, unrolled by two) are two differently written loops around the same step.  With a zero step size the
     first must reproduce the second: x, u' = u and the cost, by torch.equal, at every tail length of both unrollings, with a
     ragged wave in both lane mappings and idle quads running along.
  2. A trajectory does not see its wave: alone, and at rows 0, 15 and 16 of a batch of 17 whose other rows force the wave onto the
     paths the design calls "same bits" -- an angle of 1 rad (the full range reduction instead of the |angle| <= 0.78 short cut),
     a control of 0.5 at barrier_beta = 10 (vetoes the barrier short cut), an inactive trajectory (line search only).
  3. The fp64 oracle at B in {1, 17} x N in {1, 2, 3} with the assertions and bounds of
     test_model_params_gpu.py::test_simulate_and_total_cost and ::test_all_alpha_rollouts_and_fused_line_search, plus for N = 1 a
     per-component comparison of x[1]: a norm over the state hides a wrong body-rate row.  Its bound is the relative bound of sim_x
     applied per component against max(|reference component|, dt |rate|), the rate being the oracle's increment over dt.
     On the CPU (tests/test_rollout_step_cpu.py): every mutant of the `rollout` family of param_cases.MUTANTS exceeds these
     bounds at these shapes in the fp64 oracle alone.
  4. n_alpha = 1 and 8 through the fused line search at B = 3, N = 5, the assertions of
     test_kernels_gpu.py::test_line_search_with_one_and_with_eight_step_sizes: lane 3's record and the commit copy.
"""
import numpy as np
import pytest

import param_cases as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import linearize as o_lin  # noqa: E402

DEV = "cuda:0"
MODEL = "quadrotor"
CASES = [(sn, integ) for sn in pc.SET_NAMES[MODEL] for integ in ("euler", "rk4")]
ORACLE_SHAPES = [(B, N) for N in (1, 2, 3) for B in (1, 17)]


def _ops():
    from quattro_ilqr_amd import models, ops
    return models, ops


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def f64(t):
    return t.double().cpu().numpy()


def _gains(ops, md, xs, ud):
    layout = ops.model_layout(md)
    rec, VxN, VxxN, _ = ops.linearize(md, xs, ud, layout=layout)
    K, k, st = ops.riccati_sweep(rec, VxN, VxxN, md.n, md.m, layout)
    assert int(st.abs().sum()) == 0
    return K, k


# ---------------------------------------------------------------------------------------------- 1. alpha = 0 is simulate
@pytest.mark.parametrize("sn,integ", CASES)
def test_zero_step_rollout_is_simulate_bit_for_bit(sn, integ):
    """Holds at the parent of round 6 as well (the property was claimed, not pinned).  What it caught on the way: the control
    row of the record read through DPP moves that the compiler had sunk behind the control lane's exec-mask branch (N = 1)."""
    models, ops = _ops()
    md = pc.device_model(models, MODEL, sn, integ)
    rng = np.random.default_rng(11)
    for N in (1, 2, 3, 4, 5, 7):
        for B in (1, 3, 17):
            x0, u = pc.inputs(MODEL, sn, N, B)
            ud = dev32(u)
            xs, cost = ops.simulate(md, dev32(x0), ud)
            assert bool(torch.isfinite(xs).all()) and bool(torch.isfinite(cost).all())
            K = dev32(rng.standard_normal((B, N, md.m, md.n)))           # any finite gains: alpha = 0 multiplies them away
            k = dev32(rng.standard_normal((B, N, md.m)))
            cand, xn, un = ops.rollout(md, xs, ud, K, k, (0.0,), want_traj=True)
            assert torch.equal(xn[0], xs), (B, N, "x", float((xn[0] - xs).abs().max()))
            assert torch.equal(un[0], ud), (B, N, "u")
            assert torch.equal(cand[0], cost), (B, N, "cost", cand[0].tolist(), cost.tolist())


# ---------------------------------------------------------------------------------------------- 2. a trajectory does not see its wave
PLACE_B, PLACE_N, PLACE_ROWS = 17, 7, (0, 15, 16)


def _placed(x0, u, r):
    """The batch of PLACE_B with trajectory 0 of (x0, u) at row r.  The other rows are the rows 1.. of the inputs, by i % 3:
    0 -- a roll angle of 1 rad from step 0 (|angle| <= param_cases.THETA_MAX); 1 -- that and a control of 0.5 on every step;
    2 -- left as it is, and inactive in the line-search call.  -> x0, u, active"""
    others = [i for i in range(PLACE_B) if i != r]
    xb, ub = np.empty_like(x0), np.empty_like(u)
    active = np.ones(PLACE_B, dtype=np.int32)
    xb[r], ub[r] = x0[0], u[0]
    for src, i in enumerate(others, start=1):
        xb[i], ub[i] = x0[src], u[src]
        if i % 3 in (0, 1):
            xb[i, 6] = 1.0
        if i % 3 == 1:
            ub[i, :, 2] = 0.5
        if i % 3 == 2:
            active[i] = 0
    assert abs(xb[:, 7]).max() < pc.THETA_MAX
    return xb, ub, active


@pytest.mark.parametrize("sn,integ", CASES)
def test_a_trajectory_does_not_see_its_wave(sn, integ):
    """Holds at the parent of round 6 as well.  Both placements are compared with the same library, so this test sees a path
    that depends on the wave, not a path that is wrong everywhere (tests 1 and 3 are for that)."""
    models, ops = _ops()
    # barrier_beta = 10: a hover control takes the barrier short cut (beta u > 20), 0.5 and the inputs' -0.05 do not
    md = pc.device_model(models, MODEL, sn, integ).with_(barrier_beta=10.0)
    x0, u = pc.inputs(MODEL, sn, PLACE_N, PLACE_B)
    x0, u = x0.astype(np.float32), u.astype(np.float32)
    u1 = dev32(u[:1])
    xs1, c1 = ops.simulate(md, dev32(x0[:1]), u1)
    K1, k1 = _gains(ops, md, xs1, u1)
    cand1, xn1, un1 = ops.rollout(md, xs1, u1, K1, k1, ops.ALPHAS, want_traj=True)
    xr1, ur1, cr1 = xs1.clone(), u1.clone(), c1.clone()
    idx1 = ops.linesearch(md, xr1, ur1, K1, k1, cr1, 1e-3)
    assert bool(torch.isfinite(cand1).all())
    for r in PLACE_ROWS:
        xb, ub, active = _placed(x0, u, r)
        ud = dev32(ub)
        xs, c = ops.simulate(md, dev32(xb), ud)
        assert torch.equal(xs[r], xs1[0]) and torch.equal(c[r], c1[0]), (r, "simulate")
        assert bool((xs[:, :, 6].abs().amax(dim=1) > 0.78).any())          # the neighbours do leave the short cut's range
        K, k = K1.repeat(PLACE_B, 1, 1, 1), k1.repeat(PLACE_B, 1, 1)
        cand, xn, un = ops.rollout(md, xs, ud, K, k, ops.ALPHAS, want_traj=True)
        assert torch.equal(cand[:, r], cand1[:, 0]), (r, "rollout cost")
        assert torch.equal(xn[:, r], xn1[:, 0]) and torch.equal(un[:, r], un1[:, 0]), (r, "rollout x, u")
        xr, ur, cr = xs.clone(), ud.clone(), c.clone()
        act = torch.as_tensor(active, device=DEV)
        idx = ops.linesearch(md, xr, ur, K, k, cr, 1e-3, active=act)
        assert int(idx[r]) == int(idx1[0]), (r, "alpha index", int(idx[r]), int(idx1[0]))
        assert torch.equal(xr[r], xr1[0]) and torch.equal(ur[r], ur1[0]) and torch.equal(cr[r], cr1[0]), (r, "line search")
        idle = np.nonzero(active == 0)[0]
        assert torch.equal(xr[idle], xs[idle]) and torch.equal(ur[idle], ud[idle])    # an inactive trajectory stays untouched


# ---------------------------------------------------------------------------------------------- 3. the oracle at the new shapes
def _component_errors(spec, x0, got_x1, ref_x):
    """|got - ref| of x[1] per component over max(|ref component|, dt |rate|), dt |rate| being the oracle's increment: (B, 12)."""
    ref1 = ref_x[:, 1]
    scale = np.maximum(np.abs(ref1), np.abs(ref1 - ref_x[:, 0]))
    return np.abs(got_x1 - ref1) / np.where(scale > 0, scale, 1.0)


@pytest.mark.parametrize("sn,integ", CASES)
def test_simulate_and_total_cost_at_one_two_and_three_steps(sn, integ):
    """Bounds: param_cases.BOUNDS sim_x, sim_cost, total_cost = 2e-6; N = 1: x[1] per component at 2e-6 as well.
    Measured on an MI355X (the same figures before and after round 6, whose change keeps every bit): x <= 4.8e-8, cost <= 3.4e-7,
    total cost <= 1.2e-7; per component <= 4.5e-7 (the vertical velocity of a trajectory near hover, thrust against gravity)."""
    from test_model_params_gpu import Figures, _setup
    _lib, ops, md, spec = _setup(MODEL, sn, integ)
    fig = Figures(f"step simulate {sn} {integ}")
    worst_c = 0.0
    for B, N in ORACLE_SHAPES:
        x0, u = pc.inputs(MODEL, sn, N, B)
        xs, cost = ops.simulate(md, dev32(x0), dev32(u))
        x_ref, cost_ref = o_lin.rollout_batched(spec, x0, u)
        assert bool(torch.isfinite(xs).all())
        fig.add((B, N), "sim_x", f64(xs), x_ref)
        fig.add((B, N), "sim_cost", cost.cpu().numpy(), cost_ref)
        fig.add((B, N), "total_cost", ops.total_cost(md, xs, dev32(u)).cpu().numpy(), pc.total_cost(spec, f64(xs), u))
        if N == 1:
            e = _component_errors(spec, x0, f64(xs)[:, 1], x_ref)
            b, c = np.unravel_index(np.argmax(e), e.shape)
            print(f"[step simulate {sn} {integ}] B={B} x[1] per component: worst {e.max():.1e} (trajectory {b}, state {c}, "
                  f"reference {x_ref[b, 1, c]:.3e}, increment {x_ref[b, 1, c] - x_ref[b, 0, c]:.3e})")
            worst_c = max(worst_c, float(e.max()))
    fig.check()
    assert worst_c < pc.BOUNDS["sim_x"], worst_c


@pytest.mark.parametrize("sn,integ", CASES)
def test_rollouts_and_line_search_at_one_two_and_three_steps(sn, integ):
    """Bounds: param_cases.BOUNDS cl_x, cl_u, cl_cost = 1e-5; the line search picks the first acceptable candidate, leaves its bits.
    Measured on an MI355X: x <= 1.8e-7, u <= 1.3e-7, cost <= 6.2e-7."""
    from test_model_params_gpu import Figures, _setup
    _lib, ops, md, spec = _setup(MODEL, sn, integ)
    fig = Figures(f"step rollouts {sn} {integ}")
    for B, N in ORACLE_SHAPES:
        x0, u = pc.inputs(MODEL, sn, N, B)
        ud = dev32(u)
        xs, cost = ops.simulate(md, dev32(x0), ud)
        K, k = _gains(ops, md, xs, ud)
        cand, xn, un = ops.rollout(md, xs, ud, K, k, ops.ALPHAS, want_traj=True)
        for ai, a in enumerate(ops.ALPHAS):
            nx, nu, nc = o_lin.closed_loop_rollout_batched(spec, x0, f64(xs), u, f64(k), f64(K), a)
            fig.add((B, N, a), "cl_x", f64(xn[ai]), nx)
            fig.add((B, N, a), "cl_u", f64(un[ai]), nu)
            fig.add((B, N, a), "cl_cost", cand[ai].cpu().numpy(), nc)
        assert torch.equal(ops.rollout(md, xs, ud, K, k, ops.ALPHAS), cand)
        x_run, u_run, c_run = xs.clone(), ud.clone(), cost.clone()
        idx = ops.linesearch(md, x_run, u_run, K, k, c_run, 1e-3)
        cand_h, idx_h = cand.cpu().numpy(), idx.cpu().numpy()
        for b in range(B):
            acc = np.nonzero(cand_h[:, b] <= float(cost[b]))[0]
            assert idx_h[b] == (acc[0] if acc.size else -1), (B, N, b)
            if acc.size:
                assert torch.equal(x_run[b], xn[acc[0], b]) and torch.equal(u_run[b], un[acc[0], b])
                assert float(c_run[b]) == cand_h[acc[0], b]
            else:
                assert torch.equal(x_run[b], xs[b]) and torch.equal(u_run[b], ud[b])
    fig.check()


# ---------------------------------------------------------------------------------------------- 4. step-size lists
@pytest.mark.parametrize("sn,integ", CASES)
def test_line_search_with_one_and_with_eight_step_sizes_at_skewed_parameters(sn, integ):
    models, ops = _ops()
    md = pc.device_model(models, MODEL, sn, integ)
    B, N = 3, 5
    x0, u = pc.inputs(MODEL, sn, N, B)
    ud = dev32(u)
    xs, cost = ops.simulate(md, dev32(x0), ud)
    K, k = _gains(ops, md, xs, ud)
    for alphas in ((0.3,), (4.0, 2.0, 1.0, 0.5, 0.25, 0.1, 0.05, 0.01)):
        cand, xn, un = ops.rollout(md, xs, ud, K, k, alphas, want_traj=True)
        assert cand.shape == (len(alphas), B)
        x_run, u_run, c_run = xs.clone(), ud.clone(), cost.clone()
        idx = ops.linesearch(md, x_run, u_run, K, k, c_run, 1e-3, alphas).cpu().numpy()
        cand_h = cand.cpu().numpy()
        for b in range(B):
            acc = np.nonzero(cand_h[:, b] <= float(cost[b]))[0]
            assert idx[b] == (acc[0] if acc.size else -1), (alphas, b)
            if acc.size:
                assert torch.equal(x_run[b], xn[acc[0], b]) and torch.equal(u_run[b], un[acc[0], b])
                assert float(c_run[b]) == cand_h[acc[0], b]
            else:
                assert torch.equal(x_run[b], xs[b]) and torch.equal(u_run[b], ud[b])
