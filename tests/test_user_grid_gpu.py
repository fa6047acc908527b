"""User-compiled models across the (n, m) grid of tests/user_grid_cases.py against its fp64 reference: every kernel of a user
model's library at the dimensions where it takes another compile-time path (lanes per linearisation item, tile or generic sweep,
float4 or scalar rows, the lanes that own gain columns, the warm-start shift), on a problem whose derivative blocks are all dense.

Per grid point, integrator and variant, B in {1, 3} x N in {1, 2, 9}, through ops / QuattroILQR / BatchedMPC:
  (a) simulate / total_cost against the fp64 rollout, per component and per trajectory;
  (b) linearize -> unpack_derivs against exact fp64 derivatives, per entry, t_start > 0 once;
  (c) the first sweep through the model's layout (tile points: the generic kernel as well, flags, repair, the one-call iteration)
      against the fp64 recursion on the device's own records;
  (d) rollouts at every step size with those gains against the fp64 closed loop, and the fused line search;
  (e) device-resident solve and closed loop equal the host-driven ones bit for bit (convex, rk4, B = 3, N = 9);
  (f) one whole solve against oracle.ilqr.optimize on the Python callables.
Bounds: user_grid_cases.BOUNDS, each one the suite's own for that quantity; tests/test_user_grid_cpu.py shows that the reference
formulas in float32 stay within a quarter of them at these inputs, and that every mutant of the reference exceeds them tenfold.
"""
import numpy as np
import pytest

import user_grid_cases as g

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import ilqr as O  # noqa: E402

DEV = "cuda:0"
CASES = g.cases()
IDS = [g.case_id(c) for c in CASES]
POINT_IDS = [f"{n}x{m}" for n, m in g.POINTS]
SHAPES = [(B, N) for N in g.HORIZONS for B in g.BATCHES]


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def f64(t):
    return t.double().cpu().numpy()


class Figures:
    """Collects error / bound per quantity, prints the device maxima of a case, asserts every one at the end."""

    def __init__(self, title):
        self.title, self.worst = title, {}

    def add(self, where, name, got, ref):
        e = g.error(name, got, ref)
        if e >= self.worst.get(name, (-1.0, None))[0]:
            self.worst[name] = (e, where)

    def check(self):
        print(f"[grid device {self.title}]", {k_: f"{v[0]:.1e}" for k_, v in self.worst.items()})
        for name, (e, where) in self.worst.items():
            assert e <= g.BOUNDS[name], (self.title, name, e, g.BOUNDS[name], where)


def _setup(case):
    from quattro_ilqr_amd import _lib, ops
    n, m, variant, integ = case
    md = g.model(n, m, variant, integ)
    return _lib, ops, md, g.Problem(n, m, g.params(n, m, variant), integ)


def _nominal(ops, md, case, B, N):
    x0, u = g.inputs(case[0], case[1], case[2], N, B)
    ud = dev32(u)
    xs, cost = ops.simulate(md, dev32(x0), ud)
    assert bool(torch.isfinite(xs).all()) and bool(torch.isfinite(cost).all())
    return x0, u, ud, xs, cost


def _device_records(_lib, ops, md, xs, ud, t_start=0):
    """-> rec, VxN, VxxN, layout, and the blocks widened to fp64 in the oracle's layout."""
    B = ud.shape[0]
    rec, VxN, VxxN, layout = ops.linearize(md, xs, ud, t_start=t_start)
    blocks = {k_: f64(v) for k_, v in ops.unpack_derivs(rec, B, md.n, md.m, layout, lib=_lib.load_for(md)).items()}
    blocks["VxN"], blocks["VxxN"] = f64(VxN), f64(VxxN)
    return rec, VxN, VxxN, layout, blocks


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_simulate_and_total_cost(case):
    _lib, ops, md, pr = _setup(case)
    fig = Figures(f"simulate {g.case_id(case)}")
    for B, N in SHAPES:
        x0, u, ud, xs, cost = _nominal(ops, md, case, B, N)
        x_ref, cost_ref = pr.rollout(x0, u)
        fig.add((B, N), "sim_x", f64(xs), x_ref)
        fig.add((B, N), "sim_cost", cost.cpu().numpy(), cost_ref)
        fig.add((B, N, "total"), "sim_cost", ops.total_cost(md, xs, ud).cpu().numpy(), pr.total_cost(f64(xs), u))
    fig.check()


# ---------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_derivative_records_entry_by_entry(case):
    _lib, ops, md, pr = _setup(case)
    n, m = md.n, md.m
    want_layout = _lib.LAYOUT_ROWMAJOR_TILE if (n, m) in g.TILE_POINTS else _lib.LAYOUT_ROWMAJOR
    fig = Figures(f"records {g.case_id(case)}")
    for B, N in SHAPES:
        x0, u, ud, xs, cost = _nominal(ops, md, case, B, N)
        ref = pr.records(f64(xs), u)
        for t_start in ((0, 4) if (B, N) == (3, 9) else (0,)):
            rec, VxN, VxxN, layout, blocks = _device_records(_lib, ops, md, xs, ud, t_start)
            assert layout == want_layout
            for name in g.RECORD_NAMES:
                want = ref[name] if name in ("VxN", "VxxN") else ref[name][:, t_start:]
                assert blocks[name].shape == want.shape, (name, blocks[name].shape, want.shape)
                fig.add((B, N, t_start), name, blocks[name], want)
    fig.check()


# ---------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_first_sweep_in_every_kernel_of_the_library(case):
    import quattro_ilqr_amd as q
    _lib, ops, md, pr = _setup(case)
    n, m, variant, integ = case
    lib = _lib.load_for(md)
    tile = (n, m) in g.TILE_POINTS
    bad = _lib.TRAJ_ILLCOND | _lib.TRAJ_SINGULAR
    fig = Figures(f"sweep {g.case_id(case)}")
    for B, N in SHAPES:
        x0, u, ud, xs, cost = _nominal(ops, md, case, B, N)
        rec, VxN, VxxN, layout, blocks = _device_records(_lib, ops, md, xs, ud)
        quu = np.zeros((B, N, m, m))
        k_o, K_o = O.riccati_sweep_batched(blocks, quu_out=quu)
        flagged = g.unpivoted_pivot_ratio(quu).min(axis=1) <= 1e-6          # what the tile sweep reports, from the device's records
        assert flagged.tolist() == [variant == "pivot"] * B
        sweeps = {"generic": (rec.reshape(B, N, -1), _lib.LAYOUT_ROWMAJOR, False)}
        if tile:
            Kt, kt, st = ops.riccati_sweep(rec, VxN, VxxN, n, m, _lib.LAYOUT_ROWMAJOR_TILE, lib=lib)
            assert ((st.cpu().numpy() & _lib.TRAJ_ILLCOND) != 0).tolist() == flagged.tolist(), st
            if variant == "convex":                              # the raw tile sweep is the model's sweep
                assert int(st.abs().sum()) == 0
                fig.add((B, N, "tile"), "K", f64(Kt), K_o); fig.add((B, N, "tile"), "k", f64(kt), k_o)
            sweeps["tile + repair"] = (rec, _lib.LAYOUT_ROWMAJOR_TILE, True)
        for name, (r_, lay, repair) in sweeps.items():
            K, k, st = ops.riccati_sweep(r_, VxN, VxxN, n, m, lay, repair=repair, lib=lib)
            assert not np.any(st.cpu().numpy() & bad) and int(st.abs().sum()) == 0, (name, st)
            fig.add((B, N, name), "K", f64(K), K_o); fig.add((B, N, name), "k", f64(k), k_o)
        if variant == "convex":                                  # a regularisation that is visible (user_grid_cases.REG_BIG)
            k_r, K_r = O.riccati_sweep_batched(blocks, reg=g.REG_BIG)
            for name, (r_, lay, repair) in sweeps.items():
                K, k, st = ops.riccati_sweep(r_, VxN, VxxN, n, m, lay, reg=g.REG_BIG, repair=repair, lib=lib)
                assert int(st.abs().sum()) == 0
                fig.add((B, N, name), "K_reg", f64(K), K_r); fig.add((B, N, name), "k_reg", f64(k), k_r)
        # the one-call iteration from the same nominal hands the line search the same gains
        s = q.QuattroILQR(md, N, max_iter=1, device=DEV, tf_window=0)
        s.solve(x0, u, max_iter=0)
        assert torch.equal(s.x, xs)
        s.iterate()
        assert not np.any(s.status.cpu().numpy() & bad)
        fig.add((B, N, "iterate"), "K", f64(s.K), K_o); fig.add((B, N, "iterate"), "k", f64(s.k), k_o)
    fig.check()


# ---------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rollouts_at_every_step_size_and_the_fused_line_search(case):
    _lib, ops, md, pr = _setup(case)
    n, m = md.n, md.m
    fig = Figures(f"rollouts {g.case_id(case)}")
    for B, N in SHAPES:
        x0, u, ud, xs, cost = _nominal(ops, md, case, B, N)
        rec, VxN, VxxN, layout = ops.linearize(md, xs, ud)
        K, k, st = ops.riccati_sweep(rec, VxN, VxxN, n, m, layout, repair=True, lib=_lib.load_for(md))
        assert int(st.abs().sum()) == 0
        cand, xn, un = ops.rollout(md, xs, ud, K, k, ops.ALPHAS, want_traj=True)
        assert tuple(ops.ALPHAS) == g.ALPHAS
        ref = [pr.closed_loop(x0, f64(xs), u, f64(k), f64(K), a) for a in g.ALPHAS]
        fig.add((B, N), "cl_x", f64(xn), np.stack([r[0] for r in ref]))
        fig.add((B, N), "cl_u", f64(un), np.stack([r[1] for r in ref]))
        fig.add((B, N), "cl_cost", cand.cpu().numpy(), np.stack([r[2] for r in ref]))
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


# ---------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("nm", g.POINTS, ids=POINT_IDS)
def test_device_resident_solve_and_closed_loop_equal_the_host_driven_ones(nm):
    """The device half of the twice-stated tile rule: csrc/solve_user.hip must sweep as quattro_model_layout says, or the two
    loops part.  m = 8, N = 9: the warm-start shift moves (N - 1) m = 64 elements, one full pass; N = 10: a second, partial one."""
    import quattro_ilqr_amd as q
    n, m = nm
    md = g.model(n, m, "convex", "rk4")
    p = g.params(n, m, "convex")
    plant = g.model(n, m, "convex", "euler", p=dict(p, P=g._f32(p["P"] * np.array([1.1, 1.0, 1.0, 1.0, 1.0, 1.0]))))
    assert plant.lib_path == md.lib_path
    B = 3
    for N in ((9, 10) if m == 8 else (9,)):
        x0, u = g.inputs(n, m, "convex", N, B)
        dev = q.QuattroILQR(md, N, max_iter=15, device=DEV, device_loop="always", tf_window=0)
        host = q.QuattroILQR(md, N, max_iter=15, device=DEV, device_loop=False, check_every=1, tf_window=0)
        od = {k_: v.clone() for k_, v in dev.solve(x0, u).items()}
        oh = host.solve(x0, u)
        for key in ("K", "k", "x", "u", "cost", "iters", "alpha"):
            assert torch.equal(od[key], oh[key]), (N, key)
        assert int(od["iters"].min()) >= 1
        for hold in (1, 4):
            a = q.BatchedMPC(md, N, max_iter=4, device=DEV, check_every=1, tf_window=0)
            b = q.BatchedMPC(md, N, max_iter=4, device=DEV, check_every=1, tf_window=0)
            oa = a.run(x0.astype(np.float32), 3 * hold, device_loop="always", plant=plant, replan_every=hold)
            ob = b.run(x0.astype(np.float32), 3 * hold, device_loop=False, plant=plant, replan_every=hold)
            for key in ("x", "u", "iters"):
                assert torch.equal(oa[key], ob[key].to(oa[key].dtype)), (N, hold, key)
            assert torch.equal(a.u_warm, b.u_warm), (N, hold)
            for name in ("K", "k", "x", "cost"):
                assert torch.equal(getattr(a.solver, name), getattr(b.solver, name)), (N, hold, name)


# ---------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("nm", g.POINTS, ids=POINT_IDS)
def test_one_whole_solve_against_the_oracle(nm):
    """The assertions of test_user_model_at_the_largest_dimensions: iteration count within one, and where equal, x within 2e-4.
    (The oracle differentiates by finite differences, one trajectory at a time: two trajectories up to n + m = 12, one above.)"""
    import quattro_ilqr_amd as q
    n, m = nm
    md = g.model(n, m, "convex", "rk4")
    pr = g.Problem(n, m, g.params(n, m, "convex"), "rk4")
    B, N = 3, 9
    x0, u = g.inputs(n, m, "convex", N, B)
    s = q.QuattroILQR(md, N, max_iter=15, tol=1e-3, device=DEV, tf_window=0)
    out = s.solve(x0, u)
    assert int(out["status"].abs().sum()) == 0
    for b in ((0, 2) if n + m <= 12 else (0,)):
        u_o, x_o, logs = O.optimize(pr.f1, pr.L, pr.Lf, x0[b], [v for v in u[b]], N, max_iter=15, tol=1e-3)
        it = int(out["iters"][b])
        ex = float(np.max(np.abs(f64(out["x"][b]) - x_o)))
        print(f"[grid device solve {n}x{m}] b={b}: iterations oracle {len(logs)} device {it}, max|dx| {ex:.1e}")
        assert abs(len(logs) - it) <= 1
        if len(logs) == it:
            assert ex < g.SOLVE_X_BOUND
