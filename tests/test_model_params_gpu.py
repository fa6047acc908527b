"""Every kernel that evaluates the built-in cart-pole or quadrotor takes quattro_model_params by value; the rest of the suite
holds them at the reference's defaults, where a large share of that code cannot be seen: Ix == Iy makes the yaw gyroscopic
coefficient exactly 0, r is constant, q and qf repeat, x_ref is zero in 11 of 12 components, dt is always 0.01 and the barrier
branch is taken by the quadrotor only.  Here every one of them runs, through the C ABI, at the parameter sets of
tests/param_cases.py -- all values pairwise distinct, two step sizes, the barrier on and off for either model -- against the
fp64 oracle built from the same set.  tests/test_param_cases_cpu.py shows on the CPU that each of the single-parameter
mistakes listed there moves what is compared here by >= 100 x the bound asserted here.

Shapes: quadrotor B in {1, 19} (19: one full wave of sixteen four-lane quads plus a ragged one), cart-pole B in {1, 9},
N in {1, 7, 26} (26 crosses the fused sweep's 24 / 25-step refill boundary), both integrators, both sets per model.

Bounds (param_cases.BOUNDS) are the project's own -- tests/test_kernels_gpu.py header and
test_short_and_odd_horizons_against_the_oracle: 2e-6 simulate and cost, 1e-5 derivative blocks and closed-loop rollouts, 1e-6
terminal pair, 5e-6 rel_fro K and k -- each block and each sub-block (body-rate rows of A and B, barrier rows of K and k) against
its own norm.  None had to be widened, so none is derived from an fp32 emulation.  Worst device errors measured on an MI355X,
over all cases (the per-test figures are in the docstrings below; every test prints its own before it asserts):

  simulate x 1.7e-7, cost 4.8e-7, total_cost 1.8e-7                                             (bound 2e-6)
  A 2.9e-8, B 1.4e-7, l_x 1.1e-7, l_u 3.8e-7, l_xx 2.6e-9, l_uu 3.2e-7, rows 9-11 of A 2.6e-8, of B 1.4e-7   (1e-5)
  V_x(N) 1.0e-7, V_xx(N) 1.8e-10                                                                (1e-6)
  K 1.1e-6, k 1.8e-6, barrier rows of K 1.2e-6, of k 1.0e-6                                     (5e-6)
  all-alpha rollouts x 2.9e-7, u 3.1e-7, cost 1.4e-6; track x 8.3e-8, u 3.2e-7                  (1e-5)

That the tests bite was tried once on a scratch build: c3 := 0 in EulerRecord<QUADROTOR>::fill_dynamics turns
test_linearize_blocks_in_every_layout[quadrotor-*-euler] (rows 9-11 of A: 1.5e-2), test_sweeps_against_the_oracle[quadrotor-*-euler]
(K 6.7e-2) and test_solve_against_the_oracle_at_skewed_parameters[quadrotor-euler] red.
"""
import dataclasses

import numpy as np
import pytest

import param_cases as pc
from conftest import rel_fro

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import ilqr as o_ilqr  # noqa: E402
from oracle import linearize as o_lin  # noqa: E402

DEV = "cuda:0"
CASES = [(model, sn, integ) for model in pc.MODELS for sn in pc.SET_NAMES[model] for integ in ("euler", "rk4")]
T_SEG = 3                                       # the segment sweeps start here


def _pkg():
    import quattro_ilqr_amd as q
    return q


def _ops():
    from quattro_ilqr_amd import _lib, models, ops
    return _lib, models, ops


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def f64(t):
    return t.double().cpu().numpy()


class Figures:
    """Collects (label, error, bound), prints every figure, and asserts them together: a failing run still shows all of them."""

    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def add(self, label, name, got, ref, bound=None):
        self.rows.append((label, name, pc.change(name, got, ref), pc.BOUNDS[name] if bound is None else bound))

    def check(self):
        worst = {}
        for label, name, e, bound in self.rows:
            worst[name] = max(worst.get(name, 0.0), e / bound)
        line = "  ".join(f"{name} {max(e for _, n_, e, _ in self.rows if n_ == name):.1e}" for name in worst)
        print(f"[{self.tag}] worst: {line}")
        bad = [(label, name, e, bound) for label, name, e, bound in self.rows if not e < bound]
        assert not bad, (self.tag, bad)


def _setup(model, sn, integ):
    _lib, models, ops = _ops()
    return _lib, ops, pc.device_model(models, model, sn, integ), pc.spec(model, sn, integ)


def _shapes(model):
    return [(B, N) for N in pc.HORIZONS for B in pc.BATCHES[model]]


def _layouts(_lib, ops, md):
    """Every layout linearize produces for the model: its own (TILE16C Euler / TILE16R RK4 quadrotor), ROWMAJOR, and the full
    TILE16 record of the quadrotor."""
    lays = [ops.model_layout(md), _lib.LAYOUT_ROWMAJOR] + ([_lib.LAYOUT_TILE16] if md.n == 12 else [])
    return list(dict.fromkeys(lays))


def _oracle_gains(spec, xs64, u, t_start=0):
    blocks = o_lin.linearize_analytic(spec, xs64, u, t_start=t_start)
    k, K = o_ilqr.riccati_sweep_batched(blocks)
    return blocks, k, K


def _add_gains(fig, label, model, K, k, Kr, kr, t_start=0):
    fig.add(label, "K", f64(K), Kr)
    fig.add(label, "k", f64(k), kr)
    if model == "quadrotor":
        # rows of the swept range that sit on a barrier step of the full horizon (every third, from 0)
        first = (-t_start) % 3
        if first < Kr.shape[1]:
            got, ref = pc.barrier_rows(f64(K)[:, first:], f64(k)[:, first:]), pc.barrier_rows(Kr[:, first:], kr[:, first:])
            fig.add(label, "K_barrier", got["K_barrier"], ref["K_barrier"])
            fig.add(label, "k_barrier", got["k_barrier"], ref["k_barrier"])


# ---------------------------------------------------------------------------------------------- a. simulate, total_cost
@pytest.mark.parametrize("model,sn,integ", CASES)
def test_simulate_and_total_cost(model, sn, integ):
    """quattro_simulate_f32 and quattro_total_cost_f32 against oracle.linearize.rollout_batched: x by rel_fro, cost by the
    largest relative error, bound 2e-6 each.  The total cost is taken along the device's own states.
    Measured: x <= 1.7e-7 (cart-pole skew RK4), cost <= 4.8e-7 (quadrotor skew_nobarrier Euler), total cost <= 1.8e-7."""
    _lib, ops, md, spec = _setup(model, sn, integ)
    fig = Figures(f"simulate {model} {sn} {integ}")
    for B, N in _shapes(model):
        x0, u = pc.inputs(model, sn, N, B)
        xs, cost = ops.simulate(md, dev32(x0), dev32(u))
        x_ref, cost_ref = o_lin.rollout_batched(spec, x0, u)
        assert bool(torch.isfinite(xs).all())
        fig.add((B, N), "sim_x", f64(xs), x_ref)
        fig.add((B, N), "sim_cost", cost.cpu().numpy(), cost_ref)
        Jt = ops.total_cost(md, xs, dev32(u))
        fig.add((B, N), "total_cost", Jt.cpu().numpy(), pc.total_cost(spec, f64(xs), u))
    fig.check()


# ---------------------------------------------------------------------------------------------- b. linearize, every layout
@pytest.mark.parametrize("model,sn,integ", CASES)
def test_linearize_blocks_in_every_layout(model, sn, integ):
    """quattro_linearize_f32 in every layout the model produces, unpacked by quattro_unpack_derivs_f32 and compared PER BLOCK
    with oracle.linearize.linearize_analytic about the same (device-simulated) nominal: A, B, l_x, l_u, l_xx, l_uu at 1e-5, the
    terminal pair at 1e-6, l_ux exactly zero, t_start = 0 and 3.  For the quadrotor also the body-rate rows 9-11 of A (the
    gyroscopic terms, (Ix - Iy) / Iz among them) and of B (arm / Ix, arm / Iy, k_yaw / Iz), each against its own norm: inside a
    whole record a wrong c3 dt w entry hides behind the unit diagonal.
    Measured, worst over layouts and cases: A 2.9e-8, B 1.4e-7, l_x 1.1e-7, l_u 3.8e-7 and l_uu 3.2e-7 (cart-pole with the
    barrier), l_xx 2.6e-9, rows 9-11 of A 2.6e-8, of B 1.4e-7 (RK4, dt = 0.004), V_x 1.0e-7, V_xx 1.8e-10."""
    _lib, ops, md, spec = _setup(model, sn, integ)
    fig = Figures(f"linearize {model} {sn} {integ}")
    for B, N in _shapes(model):
        x0, u = pc.inputs(model, sn, N, B)
        xs, _ = ops.simulate(md, dev32(x0), dev32(u))
        for t_start in (0, T_SEG) if N > T_SEG else (0,):
            blocks = o_lin.linearize_analytic(spec, f64(xs), u, t_start=t_start)
            if model == "quadrotor":
                blocks.update(pc.sub_blocks(blocks))
            for layout in _layouts(_lib, ops, md):
                rec, VxN, VxxN, _ = ops.linearize(md, xs, dev32(u), t_start=t_start, layout=layout)
                got = {k_: f64(v) for k_, v in ops.unpack_derivs(rec, B, md.n, md.m, layout).items()}
                if model == "quadrotor":
                    got.update(pc.sub_blocks(got))
                label = (B, N, t_start, layout)
                for key in got:
                    if key == "lux":
                        assert not got[key].any() and not blocks[key].any(), label
                        continue
                    assert got[key].shape == blocks[key].shape, (label, key)
                    fig.add(label, key, got[key], blocks[key])
                fig.add(label, "VxN", f64(VxN), blocks["VxN"])
                fig.add(label, "VxxN", f64(VxxN), blocks["VxxN"])
    fig.check()


# ---------------------------------------------------------------------------------------------- c. sweeps
@pytest.mark.parametrize("model,sn,integ", CASES)
def test_sweeps_against_the_oracle(model, sn, integ):
    """Gains against oracle.ilqr.riccati_sweep_batched on the oracle's own blocks, rel_fro 5e-6 on K and k (quadrotor: also on
    the rows of the control that sits on the barrier, whose K is proportional to 1 / barrier_alpha), status 0 everywhere:
    quattro_linearize_f32 + quattro_riccati_sweep_f32 in every layout; quattro_linearize_sweep_f32 (the fused Euler and RK4
    quadrotor sweeps, the cart-pole's lane-per-trajectory sweep), which reads the parameter block on its own; the same two as
    segment sweeps from t_start = 3; and quattro_linearize_sweep_rows_f32 writing rows 3 .. N-1 of full gain stacks in place.
    Measured: quadrotor skew K 1.1e-6, k 1.8e-6 (RK4), barrier rows K 1.2e-6, k 1.3e-7; skew_nobarrier K 3.9e-7, k 2.6e-7, the
    same rows 3.9e-7 / 1.0e-6; cart-pole K <= 4.2e-7, k <= 4.2e-7.  (fp32 NumPy on the quadrotor skew blocks, B = 19, N = 7:
    K 2.7e-7, k 4.5e-7, barrier rows 2.7e-7 / 8.7e-8.)"""
    _lib, ops, md, spec = _setup(model, sn, integ)
    assert ops.model_can_fuse_sweep(md)
    fig = Figures(f"sweeps {model} {sn} {integ}")
    for B, N in _shapes(model):
        x0, u = pc.inputs(model, sn, N, B)
        ud = dev32(u)
        xs, _ = ops.simulate(md, dev32(x0), ud)
        for t_start in (0, T_SEG) if N > T_SEG else (0,):
            _, kr, Kr = _oracle_gains(spec, f64(xs), u, t_start)
            for layout in _layouts(_lib, ops, md):
                rec, VxN, VxxN, _ = ops.linearize(md, xs, ud, t_start=t_start, layout=layout)
                K, k, st = ops.riccati_sweep(rec, VxN, VxxN, md.n, md.m, layout)
                assert int(st.abs().sum()) == 0, (B, N, t_start, layout, st)
                _add_gains(fig, (B, N, t_start, "records", layout), model, K, k, Kr, kr, t_start)
            K, k, st = ops.linearize_sweep(md, xs, ud, t_start=t_start)
            assert int(st.abs().sum()) == 0, (B, N, t_start, "fused", st)
            _add_gains(fig, (B, N, t_start, "fused"), model, K, k, Kr, kr, t_start)
            if t_start:
                Kf = torch.full((B, N, md.m, md.n), -7.0, dtype=torch.float32, device=DEV)
                kf = torch.full((B, N, md.m), -7.0, dtype=torch.float32, device=DEV)
                _, _, st = ops.linearize_sweep(md, xs, ud, t_start=t_start, K=Kf, k=kf, in_place=True)
                assert int(st.abs().sum()) == 0
                assert torch.equal(Kf[:, t_start:], K) and torch.equal(kf[:, t_start:], k)
                assert bool((Kf[:, :t_start] == -7.0).all()) and bool((kf[:, :t_start] == -7.0).all())
    fig.check()


# ---------------------------------------------------------------------------------------------- d. rollouts, line search
@pytest.mark.parametrize("model,sn,integ", CASES)
def test_all_alpha_rollouts_and_fused_line_search(model, sn, integ):
    """The assertions of test_short_and_odd_horizons_against_the_oracle: quattro_rollout_f32 against
    oracle.linearize.closed_loop_rollout_batched for every alpha of ops.ALPHAS (x, u by rel_fro, cost by the largest relative
    error, 1e-5), with the device's own gains; quattro_linesearch_f32 picks the first acceptable candidate and leaves its bits.
    Measured: x <= 2.9e-7, u <= 3.1e-7, cost <= 1.4e-6 (quadrotor skew RK4); the quadrotor skew cases accept alpha indices
    0 .. 4, so the line search is exercised beyond its first candidate."""
    _lib, ops, md, spec = _setup(model, sn, integ)
    fig = Figures(f"rollouts {model} {sn} {integ}")
    picked = set()
    for B, N in _shapes(model):
        x0, u = pc.inputs(model, sn, N, B)
        ud = dev32(u)
        xs, cost = ops.simulate(md, dev32(x0), ud)
        layout = ops.model_layout(md)
        rec, VxN, VxxN, _ = ops.linearize(md, xs, ud, layout=layout)
        K, k, st = ops.riccati_sweep(rec, VxN, VxxN, md.n, md.m, layout)
        assert int(st.abs().sum()) == 0
        cand, xn, un = ops.rollout(md, xs, ud, K, k, ops.ALPHAS, want_traj=True)
        for ai, a in enumerate(ops.ALPHAS):
            nx, nu, nc = o_lin.closed_loop_rollout_batched(spec, x0, f64(xs), u, f64(k), f64(K), a)
            fig.add((B, N, a), "cl_x", f64(xn[ai]), nx)
            fig.add((B, N, a), "cl_u", f64(un[ai]), nu)
            fig.add((B, N, a), "cl_cost", cand[ai].cpu().numpy(), nc)
        cost_only = ops.rollout(md, xs, ud, K, k, ops.ALPHAS)
        assert torch.equal(cost_only, cand)
        x_run, u_run, c_run = xs.clone(), ud.clone(), cost.clone()
        idx = ops.linesearch(md, x_run, u_run, K, k, c_run, 1e-3)
        cand_h, idx_h = cand.cpu().numpy(), idx.cpu().numpy()
        for b in range(B):
            acc = np.nonzero(cand_h[:, b] <= float(cost[b]))[0]
            assert idx_h[b] == (acc[0] if acc.size else -1), (B, N, b)
            picked.add(int(idx_h[b]))
            if acc.size:
                assert torch.equal(x_run[b], xn[acc[0], b]) and torch.equal(u_run[b], un[acc[0], b])
                assert float(c_run[b]) == cand_h[acc[0], b]
            else:
                assert torch.equal(x_run[b], xs[b]) and torch.equal(u_run[b], ud[b])
    print(f"[rollouts {model} {sn} {integ}] accepted alpha indices: {sorted(picked)}")
    fig.check()


# ---------------------------------------------------------------------------------------------- e. persistent loops
LOOP_B, LOOP_N = 5, 26
LOOP_CASES = [(model, integ) for model in pc.MODELS for integ in ("euler", "rk4")]
SOLVE_KEYS = ("K", "k", "x", "u", "cost", "iters", "alpha", "status")


def _bitwise(model, integ):
    """The RK4 quadrotor's persistent kernel linearises by forward mode on the matrix pipe, its host-driven loop through TILE16R
    records: two codes, compared to round-off (test_rk4_quadrotor_device_resident_solve_equals_host_driven_loop).  Every
    other loop is the same arithmetic in both forms."""
    return not (model == "quadrotor" and integ == "rk4")


def _roundoff_equal(tag, od, oh, capped, keys=(("x", 1e-4), ("u", 2e-4), ("K", 2e-4), ("k", 5e-4))):
    """The RK4 quadrotor's persistent loop against its host-driven one, the comparison and the bounds of
    test_rk4_quadrotor_device_resident_solve_equals_host_driven_loop; every figure is printed before anything is asserted."""
    same = (od["iters"] == oh["iters"]) & (od["alpha"] == oh["alpha"])
    sel = same.nonzero().flatten()
    errs = {key: rel_fro(f64(od[key][sel]), f64(oh[key][sel])) for key, _ in keys}
    errs["cost"] = rel_fro(od["cost"][sel].cpu().numpy(), oh["cost"][sel].cpu().numpy())
    print(f"[{tag}] persistent vs host-driven: iterations {od['iters'].tolist()} / {oh['iters'].tolist()}, agreeing "
          f"{int(same.sum())} of {same.numel()}, " + "  ".join(f"{key} {e:.1e}" for key, e in errs.items()))
    if capped:
        assert torch.equal(od["iters"], oh["iters"])
    assert int(same.sum()) >= same.numel() - 1
    for key, tol in keys:
        assert errs[key] < tol, (tag, key, errs[key])
    assert errs["cost"] < 1e-5, (tag, errs["cost"])


@pytest.mark.parametrize("model,integ", LOOP_CASES)
def test_device_resident_solve_equals_host_driven_loop_at_skewed_parameters(model, integ):
    """quattro_ilqr_solve_f32 (csrc/solve_quad.hip, csrc/solve_cartpole.hip read the parameter block again on their own) on the
    `skew` set, B = 5, N = 26, against the host-driven loop of the calls tests a-d verify: bit for bit as in
    test_device_resident_solve_equals_host_driven_loop -- real exit tests, capped, fixed iteration counts; the RK4 quadrotor to
    round-off on every run, as test_rk4_quadrotor_device_resident_solve_equals_host_driven_loop does and with its bounds: equal
    iteration counts and accepted steps on all trajectories but at most one (that test's 99 % of 301 leaves three; a near-tie of
    the accept or stop test may fall the other way), exactly equal counts where they are capped or fixed, and on the
    trajectories that agree x 1e-4, u 2e-4, K 2e-4, k 5e-4, cost 1e-5 (measured: all five agree on every run; x 6.3e-7,
    u 9.6e-7, K 1.3e-6, cost 4.5e-7; k 1.2e-6 on the capped runs and 2.1e-4 at convergence, where k itself is nearly zero).
    The quadrotor solves take 10 - 18 iterations from these
    starts, the cart-pole's 2 - 3."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    assert q.ops.model_has_device_loop(md)
    x0, u0 = pc.inputs(model, "skew", LOOP_N, LOOP_B)
    for kw in (dict(), dict(max_iter=3), dict(max_iter=4, fixed_iters=True)):
        dev = q.QuattroILQR(md, LOOP_N, max_iter=20, device=DEV, device_loop=True, tf_window=0)
        host = q.QuattroILQR(md, LOOP_N, max_iter=20, device=DEV, device_loop=False, check_every=1, tf_window=0)
        od = {k_: v.clone() for k_, v in dev.solve(x0, u0, **kw).items()}
        oh = host.solve(x0, u0, **kw)
        assert int(od["status"].abs().sum()) == 0 and bool(torch.isfinite(od["cost"]).all()), (kw, od["status"])
        print(f"[solve {model} {integ} {kw}] iterations {od['iters'].tolist()} cost {[round(c, 3) for c in od['cost'].tolist()]}")
        if _bitwise(model, integ):
            for key in SOLVE_KEYS:
                assert torch.equal(od[key], oh[key]), (kw, key)
            assert torch.equal(dev.active, host.active) and torch.equal(dev.alpha_idx, host.alpha_idx)
        else:
            _roundoff_equal(f"solve quadrotor rk4 {kw}", od, oh, capped=kw.get("fixed_iters", False))


@pytest.mark.parametrize("model,integ", LOOP_CASES)
def test_device_resident_mpc_loop_equals_host_driven_loop_at_skewed_parameters(model, integ):
    """quattro_mpc_run_f32 over 3 control steps on the `skew` set against BatchedMPC's host-driven loop, bit for bit, as in
    test_device_resident_mpc_loop_equals_host_driven_loop.  The RK4 quadrotor (two linearisation codes, see _bitwise) to round-off
    on the first run: status 0, finite, and the controllers whose iteration counts agree at every step -- all but at most one,
    as in the solve test -- have x within 1e-4 and u within 2e-4 (rel_fro, that test's bounds).  Measured: all five agree at
    every step, 2 - 6 iterations each, and x and u come out identical."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    x0, _ = pc.inputs(model, "skew", LOOP_N, LOOP_B)
    x0 = x0.astype(np.float32)
    steps = 3
    rng = np.random.default_rng(5)
    dist = dev32(1e-3 * rng.standard_normal((steps, LOOP_B, md.n)))
    a = q.BatchedMPC(md, LOOP_N, max_iter=6, tol=1e-3, device=DEV, check_every=1, tf_window=0)
    b = q.BatchedMPC(md, LOOP_N, max_iter=6, tol=1e-3, device=DEV, check_every=1, tf_window=0)
    for rep, d in enumerate((dist, None)):
        start = x0 if rep == 0 else oa["x"][:, -1].clone()
        oa = a.run(start, steps, disturbance=d, device_loop=True)
        ob = b.run(start, steps, disturbance=d, device_loop=False)
        if not _bitwise(model, integ):
            assert int(a.solver.status.abs().sum()) == 0 and bool(torch.isfinite(oa["x"]).all()) and int(oa["iters"].min()) >= 1
            same = (oa["iters"] == ob["iters"].to(oa["iters"].dtype)).all(dim=1)
            sel = same.nonzero().flatten()
            ex, eu = rel_fro(f64(oa["x"][sel]), f64(ob["x"][sel])), rel_fro(f64(oa["u"][sel]), f64(ob["u"][sel]))
            print(f"[mpc quadrotor rk4] persistent vs host-driven: iterations {oa['iters'].tolist()} / {ob['iters'].tolist()}, "
                  f"agreeing {int(same.sum())} of {LOOP_B}, x {ex:.1e} u {eu:.1e}")
            assert int(same.sum()) >= LOOP_B - 1 and ex < 1e-4 and eu < 2e-4, (int(same.sum()), ex, eu)
            break                                    # (a second run would start from two different end states)
        for key in ("x", "u", "iters"):
            assert torch.equal(oa[key], ob[key].to(oa[key].dtype)), (rep, key)
        assert torch.equal(a.u_warm, b.u_warm)
        for name in ("K", "k", "x", "cost", "alpha_idx", "status"):
            assert torch.equal(getattr(a.solver, name), getattr(b.solver, name)), (rep, name)
        assert int(oa["iters"].min()) >= 1 and int(a.solver.status.abs().sum()) == 0
        assert bool(torch.isfinite(oa["x"]).all())


@pytest.mark.parametrize("model,integ", LOOP_CASES)
@pytest.mark.parametrize("enqueue", [False, True])
def test_logged_solve_records_at_skewed_parameters(model, integ, enqueue):
    """The device log of quattro_ilqr_solve_logged_f32 on the `skew` set, checked as
    test_solve_log_gpu.py::test_logged_solve_records_equal_the_host_driven_loop checks it (that file's host-driven loop), with
    its rule for the RK4 quadrotor: bit for bit through enqueued iterations; its persistent launch linearises with another
    code, so there the iteration sequence and the order of the stamps are checked."""
    from test_solve_log_gpu import _host_driven_records
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    B, N, max_iter, tol = LOOP_B, LOOP_N, 9, 1e-3
    x0n, u0n = pc.inputs(model, "skew", N, B)
    x0, u0 = dev32(x0n), dev32(u0n)
    ref, fin = _host_driven_records(q, md, N, x0, u0, max_iter, tol)
    sv = q.QuattroILQR(md, N, max_iter=max_iter, tol=tol, device=DEV, device_loop="always", tf_window=0)
    log = q.ops.SolveLog(md, N, B, max_iter, DEV)
    sv._alloc(B)
    sv._upload(x0, u0)
    sv._ws = q.ops.workspace(md, B, N, DEV)
    q.ops.ilqr_solve(md, sv.x, sv.u, sv.K, sv.k, sv.cost, tol, max_iter, sv._ws, x0=sv._x0, alpha_idx=sv.alpha_idx,
                     active=sv.active, iters=sv.iters, status=sv.status, reset=True, log=log, persistent=not enqueue,
                     enqueue=enqueue)
    st = sv.download_state()
    exact = _bitwise(model, integ) or enqueue
    if exact:
        assert np.array_equal(st["iters"], fin["iters"])
        assert np.array_equal(st["u"], fin["u"]) and np.array_equal(st["x"], fin["x"])
    for b in range(B):
        n_it = int(st["iters"][b])
        rows = log.rows(b, n_it)
        assert list(rows["iteration"]) == list(range(n_it))
        stp = rows["stamps"].astype(np.int64)
        assert np.all(np.diff(stp, axis=1) >= 0) and np.all(stp[1:, 0] >= stp[:-1, 3]) and np.all(stp[:, 3] > stp[:, 0])
        if not exact:
            continue
        for i in range(n_it):
            r = ref[i]
            assert r["active"][b] == 1
            assert np.array_equal(rows["x"][i], r["x"][b]) and np.array_equal(rows["u"][i], r["u"][b])
            assert np.array_equal(rows["K"][i], r["K"][b]) and np.array_equal(rows["k"][i], r["k"][b])
            assert rows["cost"][i, 0] == r["cost_pre"][b] and rows["cost"][i, 1] == r["cost_new"][b]
            assert rows["alpha_idx"][i] == r["alpha_idx"][b]
        assert n_it == len(ref) or ref[n_it]["active"][b] == 0


@pytest.mark.parametrize("model,integ", LOOP_CASES)
def test_solve_against_the_oracle_at_skewed_parameters(model, integ):
    """Beside the converged comparison above, the comparison and bound of
    test_full_size_batch_against_oracle_samples_and_permutation on the `skew` set (N = 26): the first
    iteration's gains (rel_fro 5e-6) and accepted step of three trajectories of the solve equal the fp64 oracle's on the same
    inputs (exact derivatives, fp64 sweep, fp64 line search).  Measured: K <= 3.6e-7, k <= 7.9e-7 (RK4 quadrotor)."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    spec = pc.spec(model, "skew", integ)
    x0, u0 = pc.inputs(model, "skew", LOOP_N, LOOP_B)
    out = {k_: v.clone() for k_, v in q.QuattroILQR(md, LOOP_N, max_iter=1, device=DEV, tf_window=0).solve(x0, u0).items()}
    assert int(out["status"].abs().sum()) == 0
    for b in (0, 2, 4):
        xs, J0 = o_lin.rollout_batched(spec, x0[b:b + 1], u0[b:b + 1])
        blocks = o_lin.linearize_analytic(spec, xs, u0[b:b + 1])
        kr, Kr = o_ilqr.riccati_sweep_batched(blocks)
        eK, ek = rel_fro(f64(out["K"][b]), Kr[0]), rel_fro(f64(out["k"][b]), kr[0])
        print(f"[solve vs oracle {model} {integ}] trajectory {b}: K {eK:.1e} k {ek:.1e}")
        assert eK < 5e-6 and ek < 5e-6, (b, eK, ek)
        want = -1.0
        for a in q.ops.ALPHAS:
            _, _, Jc = o_lin.closed_loop_rollout_batched(spec, x0[b:b + 1], xs, u0[b:b + 1], kr, Kr, a)
            if Jc[0] <= J0[0]:
                want = a
                break
        assert abs(float(out["alpha"][b]) - want) < 1e-7, (b, float(out["alpha"][b]), want)


@pytest.mark.parametrize("model,integ", LOOP_CASES)
def test_converged_solve_matches_oracle_optimize_at_skewed_parameters(model, integ):
    """Whole solves on the `skew` set, N = 7, through the persistent kernel, against oracle.ilqr.optimize on spec.f, spec.L,
    spec.Lf -- the reference's algorithm in fp64 with its finite-difference derivatives -- in the form of
    test_user_model_gpu.py::test_user_model_solve_matches_the_oracle: iteration count within one of the oracle's, equal on all
    compared trajectories but at most one, and where it is equal cost (relative), x and u (largest absolute difference) within
    param_cases.solve_bounds: that test's 1e-6 / 1e-5 / 3e-5, or 4 x what the same algorithm with exact derivatives and fp32
    storage differs from optimize() by on the CPU where that is more (tests/test_param_cases_cpu.py measures it; both solves
    stop on |dJ| < 1e-3, and the unconverged remainder, not fp32, is what separates their u): quadrotor 1e-6 / 1.08e-5 /
    2.6e-4, cart-pole 1e-6 / 1e-5 / 1.8e-4.  The quadrotor compares trajectories 0 and 4 (optimize() takes 2 s for each of
    its 11 - 16 iterations' worth of finite differences), the cart-pole 0, 2 and 4.
    Measured: iteration counts equal on every trajectory (quadrotor 11 - 14, cart-pole 2 - 3); cost <= 1.8e-7; quadrotor
    x 2.7e-6, u 6.5e-5, cart-pole x 1.1e-6, u 4.3e-5 -- to two digits the emulation's own distance from optimize()."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    spec = pc.spec(model, "skew", integ)
    assert q.ops.model_has_device_loop(md)
    N, B = pc.SOLVE_N, pc.SOLVE_B
    x0, u0 = pc.inputs(model, "skew", N, B)
    s = q.QuattroILQR(md, N, max_iter=pc.SOLVE_MAX_ITER, tol=pc.SOLVE_TOL, device=DEV, tf_window=0)
    out = s.solve(x0, u0)
    assert int(out["status"].abs().sum()) == 0
    u_dev, x_dev = f64(out["u"]), f64(out["x"])
    it_dev, cost_dev = out["iters"].cpu().numpy(), out["cost"].cpu().numpy()
    bounds = pc.solve_bounds(model)
    traj = (0, 4) if model == "quadrotor" else pc.SOLVE_TRAJ
    same_iters, bad = 0, []
    for b in traj:
        ref = pc.solve_optimize(spec, x0[b], u0[b])
        errs = pc.solve_errors((u_dev[b], x_dev[b], float(cost_dev[b])), ref)
        print(f"[converged {model} {integ}] b={b}: iterations oracle {ref[3]} device {it_dev[b]}, cost {ref[2]:.6f} vs "
              f"{cost_dev[b]:.6f} ({errs['cost']:.1e}), max|dx| {errs['x']:.1e} max|du| {errs['u']:.1e}")
        assert abs(ref[3] - it_dev[b]) <= 1, (b, ref[3], it_dev[b])
        if ref[3] == it_dev[b]:
            same_iters += 1
            bad += [(b, key, e, bounds[key]) for key, e in errs.items() if not e < bounds[key]]
    assert same_iters >= len(traj) - 1 and not bad, (same_iters, bad)


# ---------------------------------------------------------------------------------------------- f. track, every plant parameter
def _plant_rows(model, md, B):
    """Per-controller plants that vary EVERY physical parameter, parameter j of controller b by 1 + 0.12 sin(1 + b + 1.7 j): a
    different factor per parameter and per controller, within 12 % -- the `skew` set's Ix = 0.015 and Iy = 0.03 cannot meet."""
    ph = np.tile(np.asarray(md.phys, dtype=np.float64), (B, 1))
    b, j = np.arange(B)[:, None], np.arange(ph.shape[1])[None, :]
    ph = (ph * (1.0 + 0.12 * np.sin(1.0 + b + 1.7 * j))).astype(np.float32)
    if model == "quadrotor":
        assert np.all(ph[:, 1] != ph[:, 2])
    return ph


@pytest.mark.parametrize("model,integ", LOOP_CASES)
def test_track_with_plants_that_vary_every_parameter(model, integ):
    """quattro_track_f32 (lane_const_plant: a restated copy of the per-lane constants, for the tracked plant alone) with
    plant_phys rows that vary all seven quadrotor / all four cart-pole parameters, on the `skew` set, against the per-controller
    oracle as in test_track_against_the_oracle_with_one_plant_per_controller: B = 19 / 9, N = 7, 5 tracked steps, the plant on
    the other integrator, feedback on and off, with and without disturbance; rel_fro < 1e-5 on x and u.
    Measured: x <= 8.3e-8, u <= 3.2e-7."""
    from test_plant_loop_gpu import _oracle_track
    _lib, ops, md, spec = _setup(model, "skew", integ)
    other = "rk4" if integ == "euler" else "euler"
    plant = md.with_(integrator=other)
    B, N, steps = pc.B_FULL[model], 7, 5
    x0n, u = pc.inputs(model, "skew", N, B)
    ud = dev32(u)
    x_nom, _ = ops.simulate(md, dev32(x0n), ud)
    layout = ops.model_layout(md)
    rec, VxN, VxxN, _ = ops.linearize(md, x_nom, ud, layout=layout)
    K, _, st = ops.riccati_sweep(rec, VxN, VxxN, md.n, md.m, layout)
    assert int(st.abs().sum()) == 0
    rng = np.random.default_rng(B)
    x0 = (x_nom[:, 0] + dev32(1e-2 * rng.standard_normal((B, md.n)))).contiguous()
    dist = dev32(1e-3 * rng.standard_normal((steps, B, md.n)))
    phys = _plant_rows(model, md, B)
    plant_spec = pc.spec(model, "skew", other)
    specs = [dataclasses.replace(plant_spec, phys={k_: float(v) for k_, v in zip(pc.PHYS_NAMES[model], phys[b])})
             for b in range(B)]
    xn64, un64, K64, x064 = f64(x_nom)[:, :steps + 1], u[:, :steps], f64(K)[:, :steps], f64(x0)
    worst = 0.0
    for feedback in (True, False):
        def step_ref(b, xs0, xr, ur, Kr):
            nx, nu, _ = o_lin.closed_loop_rollout_batched(specs[b], xs0, xr, ur, np.zeros_like(ur), Kr * float(feedback), 1.0)
            return nx[0], nu[0]
        for d in (None, dist):
            x_ref, u_ref = _oracle_track(step_ref, B, x064, xn64, un64, K64, None if d is None else f64(d))
            assert np.all(np.isfinite(x_ref))
            xt, ut = ops.track(md, x0, x_nom, ud, K, steps, plant=plant, plant_phys=phys, feedback=feedback, disturbance=d)
            assert torch.equal(xt[:, 0], x0)
            ex, eu = rel_fro(f64(xt), x_ref), rel_fro(f64(ut), u_ref)
            worst = max(worst, ex, eu)
            print(f"[track {model} {integ}/{other}] feedback={feedback} dist={d is not None}: x {ex:.1e} u {eu:.1e}")
            assert ex < 1e-5 and eu < 1e-5, (feedback, d is not None, ex, eu)
    # the rows are used: controller b's plant is not controller 0's, and not the model's own
    x_one, _ = ops.track(md, x0, x_nom, ud, K, steps, plant=plant, plant_phys=np.tile(phys[:1], (B, 1)), feedback=True)
    x_all, _ = ops.track(md, x0, x_nom, ud, K, steps, plant=plant, plant_phys=phys, feedback=True)
    assert torch.equal(x_one[0], x_all[0]) and not torch.equal(x_one[1:], x_all[1:])
