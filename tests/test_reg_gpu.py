"""The Q_uu regularisation `reg` of the C ABI away from 1e-6.  Every backward sweep, solve and closed-loop entry takes it; the rest
of the suite runs the built-in models at ops.QUU_REG = 1e-6, where reg K is below fp32 resolution of Q_ux: a sweep that puts
Q_uu + reg I into the V update, flips the sign of the tile sweep's reg K term, regularises one pivot only, or a loop that drops
the argument and sweeps at a constant 1e-6, passes all of it.  Here everything runs at tests/reg_cases.py REGS (1e-2, of the
order of Q_uu) and the sweeps also at 0, on the parameter sets and shapes of tests/param_cases.py, against the fp64 oracle at the
same value.  tests/test_reg_cases_cpu.py shows on the CPU that each mistake of reg_cases.MUTANTS moves what is compared here by
>= 10 x the bound in every case outside reg_cases.NOOPS and by >= 100 x somewhere in every (set, integrator), and that fp32
NumPy stays within a quarter of the bound: K and k keep param_cases.BOUNDS (5e-6) unchanged.

  a. every sweep kernel -- records in every layout (the model's own, ROWMAJOR: sweep_generic_kernel<4,1> / <12,4>, TILE16), the
     fused Euler and RK4 quadrotor sweeps, the cart-pole lane sweep, segment and rows forms -- at REGS and at 0;
  b. the status words follow Q_uu + reg I: hand-built indefinite / singular records clear at a reg that makes them definite;
  c. the loops carry the argument: ilqr_iterate, every quattro_ilqr_solve_* and quattro_mpc_run_* entry, QuattroILQR and BatchedMPC
     leave the same bits at REGS, and their first sweep is the oracle's at REGS, not at 1e-6;
  d. whole solves at REGS against oracle.ilqr.optimize(reg=...);
  e. the hybrid iteration's tail sweep.

That the tests bite was tried once on a scratch build, never committed: see the docstring of test_sweeps_at_visible_reg.
"""
import ctypes

import numpy as np
import pytest

import param_cases as pc
import reg_cases as rc
from conftest import rel_fro

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import ilqr as o_ilqr  # noqa: E402
from oracle import linearize as o_lin  # noqa: E402
from test_model_params_gpu import (DEV, T_SEG, Figures, _add_gains, _bitwise, _layouts, _roundoff_equal,  # noqa: E402
                                   _setup, dev32, f64)

CASES = [(model, sn, integ) for model in pc.MODELS for sn in pc.SET_NAMES[model] for integ in rc.INTEGRATORS]
LOOP_CASES = [(model, integ) for model in pc.MODELS for integ in rc.INTEGRATORS]
SWEEP_HORIZONS = (1, 2, 7, 26)                  # param_cases.HORIZONS plus N = 2, the shortest horizon with a V update
VISIBLE = 1e-2                                  # what the gains at REGS must differ from the same call at QUU_REG by
STATE_KEYS = ("K", "k", "x", "u", "cost", "iters", "alpha_idx", "status")


def _pkg():
    import quattro_ilqr_amd as q
    return q


# ---------------------------------------------------------------------------------------------- a. every sweep kernel
def _print_per_kernel(fig, _lib):
    """The worst K / k of a Figures per kernel: `records` by layout (ROWMAJOR is sweep_generic_kernel, the TILE16 family the tile
    sweep in its record modes), `fused` the sweep that linearises its own trajectory (cart-pole: the lane sweep)."""
    names = {getattr(_lib, a): a[len("LAYOUT_"):] for a in dir(_lib) if a.startswith("LAYOUT_")}
    worst = {}
    for label, name, e, _ in fig.rows:
        kernel = "fused" if label[3] == "fused" else f"records {names.get(label[4], label[4])}"
        worst.setdefault(kernel, {})[name] = max(worst.setdefault(kernel, {}).get(name, 0.0), e)
    for kernel, w in worst.items():
        print(f"[{fig.tag}] {kernel}: " + "  ".join(f"{name} {e:.1e}" for name, e in w.items()))


@pytest.mark.parametrize("model,sn,integ", CASES)
def test_sweeps_at_visible_reg(model, sn, integ):
    """test_model_params_gpu.py::test_sweeps_against_the_oracle with the reg argument moved: gains against
    oracle.ilqr.riccati_sweep_batched(blocks, reg=...) on the oracle's own blocks about the device's nominal, K, k (quadrotor:
    and their barrier rows) at param_cases.BOUNDS = 5e-6, status 0 everywhere, at reg = REGS and reg = 0 (Q_uu is positive
    definite without help at these sets: test_reg_cases_cpu.py), B in {1, 19} / {1, 9}, N in {1, 2, 7, 26}:
    quattro_linearize_f32 + quattro_riccati_sweep_f32 in every layout of the model, quattro_linearize_sweep_f32 (fused Euler,
    fused RK4, cart-pole lane), both again as segment sweeps from t_start = 3, and quattro_linearize_sweep_rows_f32 equal to the
    segment form bit for bit with the rows before t_start untouched.
    Measured on an MI355X: worst over shapes, t_start and both values of reg, per kernel (every test prints its own):
      tile sweep, quadrotor skew     TILE16C / TILE16 / fused Euler K 1.6e-6, k 2.7e-6 (reg = 0; 1.2e-6 / 1.9e-6 at 1e-2), barrier rows
                                     1.5e-6 / 1.4e-7; TILE16R / TILE16 / fused RK4 K 1.3e-6, k 1.6e-6, barrier rows 8.7e-7 / 2.0e-7
      tile sweep, skew_nobarrier     K <= 2.5e-7, k <= 3.1e-7, the same rows 2.7e-7 / 1.7e-6 (fused RK4, reg = 0)
      sweep_generic_kernel<12,4>     K <= 1.0e-6, k <= 1.9e-6, barrier rows 6.8e-7 / 1.6e-6
      cart-pole lane sweep           K <= 4.3e-7, k <= 5.4e-7;  sweep_generic_kernel<4,1>  K <= 4.2e-7, k <= 5.4e-7
    Teeth on the device, tried once on a scratch build and not committed: with fmaf(reg, Kv, q3) for fmaf(-reg, Kv, q3) in
    sweep_tile16_body.h and piv for Q44 in Gj / G4 of cartpole_body.h, every case of this test goes red at reg = 1e-2 -- tile sweep
    in all five modes K 1.3e-1 (skew) / 2.1e-1 (skew_nobarrier), k 1.2e-1 / 1.9e-1, the cart-pole lane sweep K 8.0e-2 / 5.8e-2
    (skew / skew_barrier), k 1.6e-1 / 3.8e-2 -- while the generic kernel's figures in the same runs stay as above (quadrotor
    K <= 9.3e-7, cart-pole K <= 3.2e-7); tests b (both record tests), c (all eight) and e went red with it as well."""
    _lib, ops, md, spec = _setup(model, sn, integ)
    assert ops.model_can_fuse_sweep(md)
    for reg in rc.SWEEP_REGS[(model, sn)]:
        fig = Figures(f"reg sweeps {model} {sn} {integ} reg={reg:g}")
        for N in SWEEP_HORIZONS:
            for B in pc.BATCHES[model]:
                x0, u = pc.inputs(model, sn, N, B)
                ud = dev32(u)
                xs, _ = ops.simulate(md, dev32(x0), ud)
                for t_start in (0, T_SEG) if N > T_SEG else (0,):
                    blocks = o_lin.linearize_analytic(spec, f64(xs), u, t_start=t_start)
                    kr, Kr = o_ilqr.riccati_sweep_batched(blocks, reg=reg)
                    for layout in _layouts(_lib, ops, md):
                        rec, VxN, VxxN, _ = ops.linearize(md, xs, ud, t_start=t_start, layout=layout)
                        K, k, st = ops.riccati_sweep(rec, VxN, VxxN, md.n, md.m, layout, reg=reg)
                        assert int(st.abs().sum()) == 0, (reg, B, N, t_start, layout, st)
                        _add_gains(fig, (B, N, t_start, "records", layout), model, K, k, Kr, kr, t_start)
                    K, k, st = ops.linearize_sweep(md, xs, ud, t_start=t_start, reg=reg)
                    assert int(st.abs().sum()) == 0, (reg, B, N, t_start, "fused", st)
                    _add_gains(fig, (B, N, t_start, "fused"), model, K, k, Kr, kr, t_start)
                    if t_start:
                        Kf = torch.full((B, N, md.m, md.n), -7.0, dtype=torch.float32, device=DEV)
                        kf = torch.full((B, N, md.m), -7.0, dtype=torch.float32, device=DEV)
                        _, _, st = ops.linearize_sweep(md, xs, ud, t_start=t_start, reg=reg, K=Kf, k=kf, in_place=True)
                        assert int(st.abs().sum()) == 0
                        assert torch.equal(Kf[:, t_start:], K) and torch.equal(kf[:, t_start:], k)
                        assert bool((Kf[:, :t_start] == -7.0).all()) and bool((kf[:, :t_start] == -7.0).all())
        _print_per_kernel(fig, _lib)
        fig.check()


# ---------------------------------------------------------------------------------------------- b. flags
def _gain_figures(tag, pairs):
    """pairs: (label, K, k, K_ref, k_ref) -> print and assert K, k at param_cases.BOUNDS."""
    fig = Figures(tag)
    for label, K, k, Kr, kr in pairs:
        fig.add(label, "K", K, Kr)
        fig.add(label, "k", k, kr)
    fig.check()


def test_flags_follow_quu_plus_reg_on_hand_built_quadrotor_records():
    """The records of test_kernels_gpu.py::test_indefinite_and_ill_conditioned_quu_through_pack_derivs (trajectory 1: an
    indefinite l_uu at three steps; trajectory 2: l_uu + 2.5e6 at two steps, condition number ~1e8) through the TILE16 sweep and
    the pivoting ROWMAJOR one.  With today's reg = 1e-6 the flags stay as that test has them.  At reg = 1 the fp64 Q_uu + reg I of
    trajectories 0 and 1 is positive definite with every unpivoted pivot above 0.9 of its diagonal entry (the kernel's threshold:
    1e-6; asserted here from the records): both clear, and their gains meet the oracle at reg = 1 within 5e-6.  Trajectory 2
    keeps a pivot ratio of 6e-7 at reg = 1 -- still under the threshold, nothing asserted -- and needs reg = 1e7, of the order
    of its own entries, where all three are definite (ratio > 0.9), clear and meet the oracle.
    Measured: K <= 1.7e-6, k <= 2.2e-6 over both values, both kernels and the asserted trajectories."""
    from quattro_ilqr_amd import _lib, ops
    from test_kernels_gpu import BLOCKS, _indefinite_and_ill_conditioned_blocks
    blocks, d64 = _indefinite_and_ill_conditioned_blocks()
    args = (dev32(blocks["VxN"]), dev32(blocks["VxxN"]), 12, 4)
    recs = {lay: ops.pack_derivs(*[dev32(blocks[k_]) for k_ in BLOCKS], layout=lay)[0]
            for lay in (_lib.LAYOUT_TILE16, _lib.LAYOUT_ROWMAJOR)}
    bad = _lib.TRAJ_ILLCOND | _lib.TRAJ_SINGULAR
    _, _, st = ops.riccati_sweep(recs[_lib.LAYOUT_TILE16], *args, _lib.LAYOUT_TILE16)
    st = st.cpu().numpy()
    assert st[0] == 0 and (st[1] & _lib.TRAJ_ILLCOND) and (st[2] & _lib.TRAJ_ILLCOND), st
    pairs = []
    for reg, rows in ((1.0, (0, 1)), (1e7, (0, 1, 2))):
        quu = rc.quu(d64, reg)
        for b in rows:
            ratio = pc.unpivoted_pivot_ratio(quu[b:b + 1])
            ev = float(np.linalg.eigvalsh(0.5 * (quu[b] + np.swapaxes(quu[b], -1, -2))).min())
            print(f"[flags quadrotor reg={reg:g}] trajectory {b}: smallest eigenvalue {ev:.3g}, unpivoted pivot ratio {ratio:.3g}")
            assert ev > 0.0 and ratio > 0.9, (reg, b, ev, ratio)
        ko, Ko = o_ilqr.riccati_sweep_batched(d64, reg=reg)
        for lay, rec in recs.items():
            K, k, st = ops.riccati_sweep(rec, *args, lay, reg=reg)
            st = st.cpu().numpy()
            assert not np.any(st[list(rows)] & bad) and not np.any(st[list(rows)]), (reg, lay, st)
            pairs += [((reg, lay, b), f64(K[b]), f64(k[b]), Ko[b], ko[b]) for b in rows]
    _gain_figures("flags quadrotor records", pairs)


def test_flags_follow_quu_plus_reg_on_rowmajor_tile_records():
    """The records of test_kernels_gpu.py::test_tile_sweep_on_rowmajor_records_flags_what_needs_pivoting (l_uu = diag(1, -0.8, 1,
    0.5) at the last step of trajectory 2) through MODE_ROWPAD: flagged ILLCOND at 1e-6, and that trajectory alone, as today; at
    reg = 1 the fp64 Q_uu + reg I is positive definite with every unpivoted pivot above 0.5 of its diagonal entry in all six
    trajectories: status 0, and the gains of the tile sweep and of the generic one meet the oracle at reg = 1 within 5e-6.
    Measured: smallest eigenvalue 0.2, pivot ratio 0.57; K 2.6e-7, k 2.9e-7."""
    from quattro_ilqr_amd import _lib, ops
    from test_kernels_gpu import _indefinite_rowmajor_problem, _rowmajor_records
    n, m = 12, 4
    d = _indefinite_rowmajor_problem(n=n, m=m)
    rec = dev32(_rowmajor_records(d, n, m))
    args = (rec, dev32(d["VxN"]), dev32(d["VxxN"]), n, m)
    _, _, st = ops.riccati_sweep(*args, _lib.LAYOUT_ROWMAJOR_TILE)
    assert int(st[2]) & _lib.TRAJ_ILLCOND and int((st != 0).sum()) == 1
    reg = 1.0
    quu = rc.quu(d, reg)
    ratio, ev = pc.unpivoted_pivot_ratio(quu), float(np.linalg.eigvalsh(0.5 * (quu + np.swapaxes(quu, -1, -2))).min())
    print(f"[flags rowmajor reg={reg:g}] smallest eigenvalue {ev:.3g}, unpivoted pivot ratio {ratio:.3g}")
    assert ev > 0.0 and ratio > 0.5
    ko, Ko = o_ilqr.riccati_sweep_batched(d, reg=reg)
    pairs = []
    for lay in (_lib.LAYOUT_ROWMAJOR_TILE, _lib.LAYOUT_ROWMAJOR):
        K, k, st = ops.riccati_sweep(*args, lay, reg=reg)
        assert int(st.abs().sum()) == 0, (lay, st)
        pairs.append(((reg, lay), f64(K), f64(k), Ko, ko))
    _gain_figures("flags rowmajor records", pairs)


@pytest.mark.parametrize("golden,n,m", [("sweep_cartpole_N30.npz", 4, 1), ("sweep_quadrotor_N50.npz", 12, 4)])
def test_singular_at_reg_and_clean_at_twice_it(golden, n, m):
    """test_kernels_gpu.py::test_sweep_status_flags_singular_and_nonfinite's record with l_uu = -reg I exactly and B = 0, at
    reg = fp32(1e-2): Q_uu + reg I is exactly zero, TRAJ_SINGULAR in every layout; at twice it Q_uu + reg I = reg I: status 0."""
    from quattro_ilqr_amd import _lib, ops
    from test_kernels_gpu import BLOCKS, _zero_quu_blocks
    reg = float(np.float32(1e-2))
    blocks = _zero_quu_blocks(reg, golden)
    layouts = (None, _lib.LAYOUT_ROWMAJOR) + ((_lib.LAYOUT_TILE16,) if n == 12 else ())
    for lay in layouts:
        rec, layout = ops.pack_derivs(*[dev32(blocks[k_]) for k_ in BLOCKS], layout=lay)
        args = (rec, dev32(blocks["VxN"]), dev32(blocks["VxxN"]), n, m, layout)
        _, _, st = ops.riccati_sweep(*args, reg=reg)
        assert int(st.cpu()[0]) & _lib.TRAJ_SINGULAR, (layout, st)
        K, k, st = ops.riccati_sweep(*args, reg=2.0 * reg)
        assert int(st.cpu()[0]) == 0 and bool(torch.isfinite(K).all()) and bool(torch.isfinite(k).all()), (layout, st)


# ---------------------------------------------------------------------------------------------- c. the loops carry the argument
LOOP_TOL, LOOP_MAX_ITER, MPC_STEPS, MPC_MAX_ITER = 1e-3, 6, 3, 4


def _neutral(ops, md, B):
    """The model's own phys / x_ref / weights as per-trajectory rows: what the phys, ref and cost entries take."""
    rows = dict(model_phys=np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1)),
                x_ref_rows=np.tile(np.asarray(md.x_ref, dtype=np.float32), (B, 1)))
    if ops.model_can_cost_rows(md):
        rows["cost_rows"] = dict(q=np.asarray(md.q), qf=np.asarray(md.qf), r=np.asarray(md.r))
    return rows


def _state_of(t):
    return {key: getattr(t, key).clone() for key in STATE_KEYS}


def _solve_forms(q, md, x0, u0, persistent=False):
    """name -> fn(reg, max_iter) -> the STATE_KEYS of one solve of (x0, u0), each through another entry or wrapper.
    Group `host`: the arithmetic of quattro_ilqr_iterate_f32 (one launch sequence per iteration); group `device`: one
    launch for the whole solve.  persistent: ask for the persistent kernel where it is not the model's fastest form."""
    from quattro_ilqr_amd import _lib, ops
    from test_plant_loop_gpu import _LoopState
    B, N = x0.shape[0], u0.shape[1]
    lib = _lib.load_for(md)
    neutral = _neutral(ops, md, B)

    def fresh():
        return _LoopState(md, x0, u0, 1)

    def iterate(reg, max_iter):
        t = fresh()
        ops.simulate(md, t.x0, t.u, x=t.x, cost=t.cost)
        t.active.fill_(1); t.alpha_idx.fill_(-1)
        for _ in range(max_iter):
            ops.ilqr_iterate(md, t.x, t.u, t.K, t.k, t.cost, LOOP_TOL, t.ws, reg=reg, alpha_idx=t.alpha_idx, active=t.active,
                             iters=t.iters, status=t.status)
        return _state_of(t)

    def ops_solve(**kw):
        def fn(reg, max_iter):
            t = fresh()
            extra = dict(kw)
            if extra.pop("log", False):
                extra["log"] = ops.SolveLog(md, N, B, max_iter, DEV)
            ops.ilqr_solve(md, t.x, t.u, t.K, t.k, t.cost, LOOP_TOL, max_iter, t.ws, reg=reg, x0=t.x0, alpha_idx=t.alpha_idx,
                           active=t.active, iters=t.iters, status=t.status, reset=True, **extra)
            return _state_of(t)
        return fn

    def raw(entry, *extra):
        def fn(reg, max_iter):
            t = fresh()
            arr, na = ops._alphas(ops.ALPHAS)
            p = md.c_params()
            flags = _lib.SOLVE_SIMULATE | _lib.SOLVE_RESET | (_lib.SOLVE_PERSISTENT if persistent else 0)
            rc_ = getattr(lib, entry)(ctypes.byref(p), ops._ptr(t.x0), ops._ptr(t.x), ops._ptr(t.u), B, N, float(reg), arr, na,
                                      LOOP_TOL, max_iter, flags, ops._ptr(t.K), ops._ptr(t.k), ops._ptr(t.cost),
                                      ops._ptr(t.alpha_idx), ops._ptr(t.active), ops._ptr(t.iters), ops._ptr(t.status),
                                      ops._ptr(t.ws), t.ws.numel() * t.ws.element_size(), *extra, ops._stream())
            assert rc_ == _lib.QUATTRO_OK, entry
            torch.cuda.synchronize()
            return _state_of(t)
        return fn

    def solver(device_loop, **rows):
        def fn(reg, max_iter):
            s = q.QuattroILQR(md, N, max_iter=max_iter, tol=LOOP_TOL, reg=reg, device=DEV, device_loop=device_loop, check_every=1,
                              tf_window=0)
            s.solve(x0, u0, **rows)
            return {key: getattr(s, key).clone() for key in STATE_KEYS}
        return fn

    pk = dict(persistent=True) if persistent else {}
    dl = "always" if persistent else True
    host = {"ops.ilqr_iterate": iterate, "ops.ilqr_solve(enqueue)": ops_solve(enqueue=True),
            "QuattroILQR(device_loop=False)": solver(False)}
    device = {"ops.ilqr_solve": ops_solve(**pk), "ops.ilqr_solve(log)": ops_solve(log=True, **pk),
              "quattro_ilqr_solve_f32": raw("quattro_ilqr_solve_f32"),
              "quattro_ilqr_solve_logged_f32(NULL)": raw("quattro_ilqr_solve_logged_f32", None),
              "QuattroILQR(device_loop)": solver(dl)}
    wrapper_rows = dict(model_phys="model_phys", x_ref_rows="targets", cost_rows="weights")
    for key, rows in neutral.items():
        device[f"ops.ilqr_solve({key})"] = ops_solve(**{key: rows}, **pk)
        device[f"QuattroILQR.solve({wrapper_rows[key]})"] = solver(dl, **{wrapper_rows[key]: rows})
    return host, device


def _first_sweep_is_the_oracles(tag, forms, reg, Kr, kr, bounds=None):
    """Every form at max_iter = 1: its gains are the oracle's first sweep at `reg` within the bounds of (a), and differ from the
    same call at QUU_REG by more than VISIBLE -- what separates `every path agrees` from `every path ignores the argument`."""
    fig = Figures(tag)
    moved = {}
    for name, fn in forms.items():
        at_reg, at_default = fn(reg, 1), fn(rc.QUU_REG, 1)
        assert int(at_reg["status"].abs().sum()) == 0, (name, at_reg["status"])
        if bounds is None:
            fig.add(name, "K", f64(at_reg["K"]), Kr)
            fig.add(name, "k", f64(at_reg["k"]), kr)
        else:
            fig.rows.append((name, "K", bounds[0]("K_reg", f64(at_reg["K"]), Kr), bounds[1]["K_reg"]))
            fig.rows.append((name, "k", bounds[0]("k_reg", f64(at_reg["k"]), kr), bounds[1]["k_reg"]))
        moved[name] = pc.change("K", f64(at_reg["K"]), f64(at_default["K"]))
    print(f"[{tag}] K at reg={reg:g} against the same call at {rc.QUU_REG:g}: {min(moved.values()):.2e} ... {max(moved.values()):.2e}")
    fig.check()
    assert all(v > VISIBLE for v in moved.values()), moved


def _same_bits(tag, base_name, base, others):
    for name, got in others.items():
        diff = [key for key in STATE_KEYS if not torch.equal(got[key], base[key])]
        assert not diff, (tag, name, "differs from", base_name, "in", diff)


def _as_solve_out(st):
    """STATE_KEYS -> the keys _roundoff_equal reads."""
    return dict(st, alpha=st["alpha_idx"])


@pytest.mark.parametrize("model,integ", LOOP_CASES)
def test_every_solve_entry_carries_reg(model, integ):
    """`skew` set, B = B_FULL (19 / 9), N = SOLVE_N = 7, reg = REGS.  Every way to a solve -- ops.ilqr_iterate driven by hand, the
    enqueued ops.ilqr_solve, QuattroILQR(device_loop=False); the device-resident ops.ilqr_solve, the same with a log ring, with
    neutral model_phys, x_ref_rows and (cart-pole) cost_rows, quattro_ilqr_solve_f32 and quattro_ilqr_solve_logged_f32 called
    directly, QuattroILQR(reg=) and its solve(model_phys= / targets= / weights=) -- leaves the same K, k, x, u, cost, iters,
    alpha_idx and status, bit for bit, after at most 6 iterations with real exit tests.  (RK4 quadrotor: bit for bit inside the
    host-driven and inside the device-resident group, to round-off between them as everywhere: test_model_params_gpu._bitwise.)
    And every one of them at max_iter = 1 leaves the oracle's first sweep at REGS within 5e-6, more than 1e-2 away from what
    the same call leaves at 1e-6.
    Measured: first sweep K <= 4.1e-7, k <= 5.1e-7 (RK4 quadrotor), 0.19 (quadrotor) / 0.43 (cart-pole) away from the call at 1e-6
    in every form; the quadrotor solves are still running at the cap of 6 iterations, the cart-pole's stop after 5 - 6; RK4
    quadrotor between the groups: all 19 agree, x 1.5e-7, u 1.7e-7, K 5.2e-7, k 8.4e-7, cost 4.5e-8."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    assert q.ops.model_has_device_loop(md)
    reg = rc.REGS[(model, "skew")]
    N, B = pc.SOLVE_N, pc.B_FULL[model]
    x0, u0 = pc.inputs(model, "skew", N, B)
    host, device = _solve_forms(q, md, x0, u0)
    tag = f"reg solve entries {model} {integ}"
    kr, Kr = o_ilqr.riccati_sweep_batched(rc.blocks(model, "skew", integ, N), reg=reg)
    _first_sweep_is_the_oracles(tag, {**host, **device}, reg, Kr, kr)
    h = {name: fn(reg, LOOP_MAX_ITER) for name, fn in host.items()}
    d = {name: fn(reg, LOOP_MAX_ITER) for name, fn in device.items()}
    hb, db = h["ops.ilqr_iterate"], d["ops.ilqr_solve"]
    print(f"[{tag}] iterations {db['iters'].tolist()}")
    assert int(db["status"].abs().sum()) == 0 and int(db["iters"].min()) >= 1 and bool(torch.isfinite(db["cost"]).all())
    _same_bits(tag, "ops.ilqr_iterate", hb, h)
    _same_bits(tag, "ops.ilqr_solve", db, d)
    if _bitwise(model, integ):
        _same_bits(tag, "ops.ilqr_iterate", hb, {"ops.ilqr_solve": db})
    else:
        _roundoff_equal(tag, _as_solve_out(db), _as_solve_out(hb), capped=False)


def _mpc_forms(q, md, x0, u0, dist, steps):
    """name -> fn(reg, max_iter, steps) -> every array a device-resident run leaves, through each quattro_mpc_run_* entry."""
    from quattro_ilqr_amd import ops
    from test_plant_loop_gpu import _LoopState
    B = x0.shape[0]
    neutral = _neutral(ops, md, B)

    def run(**extra):
        def fn(reg, max_iter, n_steps=steps):
            t = _LoopState(md, x0, u0, n_steps)
            ops.mpc_run(md, t.x_cur, t.x, t.u, t.K, t.k, t.cost, LOOP_TOL, max_iter, n_steps, t.ws, t.traj_x, t.traj_u, t.traj_it,
                        disturbance=None if dist is None else dist[:n_steps].contiguous(), reg=reg, alpha_idx=t.alpha_idx,
                        active=t.active, iters=t.iters, status=t.status, **extra)
            torch.cuda.synchronize()
            return t
        return fn

    forms = {"quattro_mpc_run_f32": run(), "quattro_mpc_run_plant_f32(plant=model)": run(plant=md)}
    for key, rows in neutral.items():
        forms[f"quattro_mpc_run_{dict(model_phys='phys', x_ref_rows='ref', cost_rows='cost')[key]}_f32"] = run(**{key: rows})
    return forms


@pytest.mark.parametrize("model,integ", LOOP_CASES)
def test_every_closed_loop_entry_carries_reg(model, integ):
    """`skew` set, B = B_FULL, N = 7, reg = REGS, 3 control steps of at most 4 iterations with a disturbance, warm start u0.
    ops.mpc_run through quattro_mpc_run_f32, _plant_f32 (the neutral plant: the model itself), _phys_f32, _ref_f32 and (cart-pole)
    _cost_f32 with neutral rows leaves the same bits in every array of the run; BatchedMPC on a QuattroILQR(reg=REGS) leaves them
    too, and its host-driven control steps (device_loop=False) give the same x, u, iters, warm start and solver state (RK4
    quadrotor: to round-off, as test_device_resident_mpc_loop_equals_host_driven_loop_at_skewed_parameters).  One control step of
    one iteration through every entry leaves the oracle's first sweep at REGS within 5e-6, more than 1e-2 from the same call at
    1e-6.
    Measured: first sweep K <= 4.0e-7, k <= 5.0e-7, 0.19 / 0.43 away from 1e-6; quadrotor 3 - 4 iterations per control step,
    cart-pole 2 - 4; RK4 quadrotor against its host-driven steps: all 19 agree."""
    from test_plant_loop_gpu import _LoopState
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    reg = rc.REGS[(model, "skew")]
    N, B = pc.SOLVE_N, pc.B_FULL[model]
    x0, u0 = pc.inputs(model, "skew", N, B)
    dist = dev32(1e-3 * np.random.default_rng(5).standard_normal((MPC_STEPS, B, md.n)))
    forms = _mpc_forms(q, md, x0, u0, dist, MPC_STEPS)
    tag = f"reg closed loop {model} {integ}"
    kr, Kr = o_ilqr.riccati_sweep_batched(rc.blocks(model, "skew", integ, N), reg=reg)
    one = {name: (lambda r_, it, fn=fn: _state_of(fn(r_, it, 1))) for name, fn in forms.items()}
    _first_sweep_is_the_oracles(tag, one, reg, Kr, kr)
    runs = {name: fn(reg, MPC_MAX_ITER) for name, fn in forms.items()}
    base = runs["quattro_mpc_run_f32"]
    print(f"[{tag}] iterations per control step {base.traj_it.tolist()}")
    assert int(base.status.abs().sum()) == 0 and int(base.traj_it.min()) >= 1 and bool(torch.isfinite(base.traj_x).all())
    for name, t in runs.items():
        assert base.same_as(t) == [], (name, base.same_as(t))

    def mpc():
        c = q.BatchedMPC(md, N, max_iter=MPC_MAX_ITER, tol=LOOP_TOL, device=DEV, check_every=1, tf_window=0)
        c.solver = q.QuattroILQR(md, N, max_iter=MPC_MAX_ITER, tol=LOOP_TOL, reg=reg, device=DEV, check_every=1, tf_window=0)
        c.u_warm = dev32(u0)
        return c
    a, b = mpc(), mpc()
    oa = a.run(x0.astype(np.float32), MPC_STEPS, disturbance=dist, device_loop=True)
    ob = b.run(x0.astype(np.float32), MPC_STEPS, disturbance=dist, device_loop=False)
    assert torch.equal(oa["x"], base.traj_x) and torch.equal(oa["u"], base.traj_u) and torch.equal(oa["iters"], base.traj_it)
    for name in ("K", "k", "x", "cost", "alpha_idx", "status"):
        assert torch.equal(getattr(a.solver, name), getattr(base, name)), name
    assert torch.equal(a.u_warm, base.u)
    if _bitwise(model, integ):
        for key in ("x", "u", "iters"):
            assert torch.equal(oa[key], ob[key].to(oa[key].dtype)), key
        assert torch.equal(a.u_warm, b.u_warm)
        for name in ("K", "k", "x", "cost", "alpha_idx", "status"):
            assert torch.equal(getattr(a.solver, name), getattr(b.solver, name)), name
    else:
        same = (oa["iters"] == ob["iters"].to(oa["iters"].dtype)).all(dim=1)
        sel = same.nonzero().flatten()
        ex, eu = rel_fro(f64(oa["x"][sel]), f64(ob["x"][sel])), rel_fro(f64(oa["u"][sel]), f64(ob["u"][sel]))
        print(f"[{tag}] persistent vs host-driven: iterations {oa['iters'].tolist()} / {ob['iters'].tolist()}, agreeing "
              f"{int(same.sum())} of {B}, x {ex:.1e} u {eu:.1e}")
        assert int(same.sum()) >= B - 1 and ex < 1e-4 and eu < 2e-4, (int(same.sum()), ex, eu)


USER_POINT = (7, 2)                             # NZ = 9: a tile point (MODE_ROWPAD in csrc/solve_user.hip), all scalar paths


def test_user_model_loops_carry_reg():
    """Grid point 7 x 2 of tests/user_grid_cases.py, convex variant, RK4, B = 3, N = 9, reg = REG_BIG = 5e-2 -- until now that value
    reached quattro_riccati_sweep_f32 only.  The host-driven forms (ops.ilqr_iterate, enqueued ops.ilqr_solve,
    QuattroILQR(device_loop=False)) and the persistent kernel of csrc/solve_user.hip (ops.ilqr_solve(persistent=True), with a log
    ring, with neutral model_phys / x_ref_rows / cost_rows, the two plain C entries, QuattroILQR(device_loop="always")) leave the
    same bits after at most 6 iterations, and the closed loop (device_loop="always" against False, 3 steps) does; each form's
    first sweep is the fp64 recursion at REG_BIG on the device's own records within user_grid_cases.BOUNDS (K_reg 2e-5, k_reg 5e-5,
    per step), more than 1e-2 from the same call at 1e-6.
    Measured: first sweep per step K 2.9e-7, k 2.5e-7, 7.0e-2 away from 1e-6; 3 iterations per trajectory."""
    import user_grid_cases as g
    q = _pkg()
    from quattro_ilqr_amd import _lib, ops
    n, m = USER_POINT
    md = g.model(n, m, "convex", "rk4")
    assert ops.model_can_device_loop(md)
    reg, B, N = g.REG_BIG, 3, 9
    x0, u0 = g.inputs(n, m, "convex", N, B)
    ud = dev32(u0)
    xs, _ = ops.simulate(md, dev32(x0), ud)
    rec, VxN, VxxN, layout = ops.linearize(md, xs, ud)
    blocks = {k_: f64(v) for k_, v in ops.unpack_derivs(rec, B, n, m, layout, lib=_lib.load_for(md)).items()}
    blocks["VxN"], blocks["VxxN"] = f64(VxN), f64(VxxN)
    kr, Kr = o_ilqr.riccati_sweep_batched(blocks, reg=reg)
    host, device = _solve_forms(q, md, x0, u0, persistent=True)
    tag = f"reg user model {n}x{m}"
    _first_sweep_is_the_oracles(tag, {**host, **device}, reg, Kr, kr, bounds=(g.error, g.BOUNDS))
    h = {name: fn(reg, LOOP_MAX_ITER) for name, fn in host.items()}
    d = {name: fn(reg, LOOP_MAX_ITER) for name, fn in device.items()}
    print(f"[{tag}] iterations {d['ops.ilqr_solve']['iters'].tolist()}")
    assert int(d["ops.ilqr_solve"]["iters"].min()) >= 1 and int(d["ops.ilqr_solve"]["status"].abs().sum()) == 0
    _same_bits(tag, "ops.ilqr_iterate", h["ops.ilqr_iterate"], {**h, **d})

    def mpc():
        c = q.BatchedMPC(md, N, max_iter=MPC_MAX_ITER, tol=LOOP_TOL, device=DEV, check_every=1, tf_window=0)
        c.solver = q.QuattroILQR(md, N, max_iter=MPC_MAX_ITER, tol=LOOP_TOL, reg=reg, device=DEV, check_every=1, tf_window=0)
        c.u_warm = dev32(u0)
        return c
    a, b = mpc(), mpc()
    oa = a.run(x0.astype(np.float32), MPC_STEPS, device_loop="always")
    ob = b.run(x0.astype(np.float32), MPC_STEPS, device_loop=False)
    for key in ("x", "u", "iters"):
        assert torch.equal(oa[key], ob[key].to(oa[key].dtype)), key
    assert torch.equal(a.u_warm, b.u_warm)
    for name in ("K", "k", "x", "cost"):
        assert torch.equal(getattr(a.solver, name), getattr(b.solver, name)), name
    # ... and the run is not the run at the default
    c = q.BatchedMPC(md, N, max_iter=MPC_MAX_ITER, tol=LOOP_TOL, device=DEV, check_every=1, tf_window=0)
    c.u_warm = dev32(u0)
    c.run(x0.astype(np.float32), MPC_STEPS, device_loop="always")
    moved = pc.change("K", f64(a.solver.K), f64(c.solver.K))
    print(f"[{tag}] closed loop: K at reg={reg:g} against {rc.QUU_REG:g}: {moved:.2e}")
    assert moved > VISIBLE


# ---------------------------------------------------------------------------------------------- d. whole solves
@pytest.mark.parametrize("model,integ", LOOP_CASES)
def test_converged_solve_matches_oracle_optimize_at_visible_reg(model, integ):
    """test_model_params_gpu.py::test_converged_solve_matches_oracle_optimize_at_skewed_parameters at reg = REGS, through the
    device-resident solve of QuattroILQR(reg=): `skew` set, N = 7, against oracle.ilqr.optimize(reg=REGS) on spec.f, spec.L,
    spec.Lf.  Iteration counts within one of the oracle's, equal on all compared trajectories but at most one, and where equal
    cost (relative), x and u (largest absolute difference) within reg_cases.solve_bounds = max(SOLVE_START, 4 x SOLVE_E_REG), the
    CPU-measured distance of the fp32-storage emulation from optimize(reg=REGS): quadrotor 1e-6 / 1.16e-5 / 8e-5, cart-pole
    1e-6 / 1e-5 / 1.48e-4.  Quadrotor: trajectories 0 and 4, cart-pole: 0, 2, 4.
    Measured: iteration counts equal on every trajectory (quadrotor 11 - 13, cart-pole 5 - 7); cost <= 2.5e-7; quadrotor
    x 7.1e-7, u 1.2e-5, cart-pole x 7.1e-7, u 3.5e-5."""
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    spec = pc.spec(model, "skew", integ)
    reg = rc.REGS[(model, "skew")]
    N, B = pc.SOLVE_N, pc.SOLVE_B
    x0, u0 = pc.inputs(model, "skew", N, B)
    s = q.QuattroILQR(md, N, max_iter=pc.SOLVE_MAX_ITER, tol=pc.SOLVE_TOL, reg=reg, device=DEV, tf_window=0)
    out = s.solve(x0, u0)
    assert int(out["status"].abs().sum()) == 0
    u_dev, x_dev = f64(out["u"]), f64(out["x"])
    it_dev, cost_dev = out["iters"].cpu().numpy(), out["cost"].cpu().numpy()
    bounds = rc.solve_bounds(model)
    traj = (0, 4) if model == "quadrotor" else pc.SOLVE_TRAJ
    same_iters, bad = 0, []
    for b in traj:
        ref = rc.solve_optimize(spec, x0[b], u0[b], reg)
        errs = pc.solve_errors((u_dev[b], x_dev[b], float(cost_dev[b])), ref)
        print(f"[converged reg={reg:g} {model} {integ}] b={b}: iterations oracle {ref[3]} device {it_dev[b]}, cost {ref[2]:.6f} vs "
              f"{cost_dev[b]:.6f} ({errs['cost']:.1e}), max|dx| {errs['x']:.1e} max|du| {errs['u']:.1e}")
        assert abs(ref[3] - it_dev[b]) <= 1, (b, ref[3], it_dev[b])
        if ref[3] == it_dev[b]:
            same_iters += 1
            bad += [(b, key, e, bounds[key]) for key, e in errs.items() if not e < bounds[key]]
    assert same_iters >= len(traj) - 1 and not bad, (same_iters, bad)


# ---------------------------------------------------------------------------------------------- e. hybrid tail sweep
HYBRID_CASE = "L61_straddle"                    # n = 4, c = 5 = m (1 + n): a cart-pole gain stack, N = 30 = 25 predicted + 5 swept


@pytest.mark.parametrize("integ", rc.INTEGRATORS)
def test_hybrid_iteration_sweeps_its_tail_at_reg(integ):
    """A stub predictor (predictor_cases L61_straddle through TransformerILQR.load_arrays; the fused kernel covers it) on the
    cart-pole `skew_barrier` set, N = 30, tf_window = 5, B = 9: after ONE hybrid iteration of QuattroILQR(tf=, reg=REGS) the rows
    t >= N - 5 of K and k equal ops.linearize_sweep(..., t_start = N - 5, reg=REGS) about the first nominal by torch.equal, and
    meet the oracle's segment sweep at REGS within 5e-6 (and are more than 1e-2 away from the segment sweep at 1e-6).  The
    predicted rows are not compared with anything.
    Measured: K <= 2.0e-7, k 2.9e-7; 0.54 away from the sweep at 1e-6."""
    import predictor_cases as prc
    q = _pkg()
    from quattro_ilqr_amd import ops
    cs = prc.case(HYBRID_CASE)
    model, sn = "cartpole", "skew_barrier"
    md, spec = pc.device_model(q.models, model, sn, integ), pc.spec(model, sn, integ)
    assert (cs.n, cs.c) == (md.n, md.m * (1 + md.n))
    N, W, B = cs.ns - 1, cs.P, pc.B_FULL[model]
    assert cs.T + W == N
    reg = rc.REGS[(model, sn)]
    tf = q.TransformerILQR(cs.n, cs.c, device=DEV).load_arrays(cs.w, cs.norm, cs.hp)
    assert tf.fused_kernel_covers() and ops.model_fuses_sweep(md)
    x0, u0 = pc.inputs(model, sn, N, B)
    ud = dev32(u0)
    xs, _ = ops.simulate(md, dev32(x0), ud)
    s = q.QuattroILQR(md, N, max_iter=1, tol=LOOP_TOL, tf=tf, reg=reg, device=DEV, check_every=1)
    assert s.tf_window == W
    out = s.solve(x0, u0, x_ref=np.asarray(md.x_ref))
    K, k = out["K"].clone(), out["k"].clone()
    Ks, ks, st = ops.linearize_sweep(md, xs, ud, t_start=N - W, reg=reg)
    assert int(st.abs().sum()) == 0
    assert torch.equal(K[:, N - W:], Ks) and torch.equal(k[:, N - W:], ks)
    blocks = o_lin.linearize_analytic(spec, f64(xs), u0, t_start=N - W)
    kr, Kr = o_ilqr.riccati_sweep_batched(blocks, reg=reg)
    k0, K0 = o_ilqr.riccati_sweep_batched(blocks)
    fig = Figures(f"reg hybrid tail cartpole {integ}")
    fig.add("tail", "K", f64(K[:, N - W:]), Kr)
    fig.add("tail", "k", f64(k[:, N - W:]), kr)
    moved = pc.change("K", f64(K[:, N - W:]), K0)
    print(f"[reg hybrid tail cartpole {integ}] K tail at reg={reg:g} against the oracle at {rc.QUU_REG:g}: {moved:.2e}")
    fig.check()
    assert moved > VISIBLE
