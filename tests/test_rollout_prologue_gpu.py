"""What the quadrotor rollouts do BEFORE and AROUND their step loop (rollout_quad_body.h, round 9): simulate's controls come
through a register ring SIM_RING = 4 steps deep with the loop unrolled to match, its x0 row leaves after the loop's first wait,
and the fused line search requests a trajectory's flag, its cost and the lane constants in one batch ahead of its early exit.

ops.simulate, Euler and RK4, B = 1, 15, 16, 17, 33 (a wave holds 16 trajectories: one quad, a wave short of one, full, one
past, two and a bit) x N = 1 .. 5, 7, 8, 9, 17, 50, 51 (the ring's depth and its tails, the eight steps of a 128-byte line of
controls, the headline):
  * x and cost equal, bit for bit, the alpha = 0 candidate of ops.rollout and of ops.linesearch under zero gains -- those read
    the controls through quad_rollout_closed's per-step buffer loads, so the two forms check each other;
  * x and cost within the simulate tolerance of tests/test_kernels_gpu.py (2e-6) of the fp64 oracle's rollout;
  * the same with u and x as views into larger buffers whose surroundings are NaN (u) or a sentinel (x), and with every
    second trajectory's controls NaN: a load that strays from its trajectory shows as NaN, a store as a changed sentinel
    (bit for bit under Euler; under RK4, whose stage_sincos votes wave-wide, finite and within the simulate tolerance).

ops.linesearch under `active` masks, B = 1, 2, 3, 5 (a wave holds two trajectories), N = 1, 4, 5, 51: every array of an
inactive trajectory keeps its bits; the active ones equal the same trajectories run in a batch of their own -- bit for bit
under Euler, within the simulate tolerance (accepted index, iters and flags exact) under RK4, for the vote's reason."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import linearize as o_lin  # noqa: E402
from oracle import models as o_models  # noqa: E402

DEV = "cuda:0"
BS = (1, 15, 16, 17, 33)
NS = (1, 2, 3, 4, 5, 7, 8, 9, 17, 50, 51)
SIM_TOL = 2e-6                                   # tests/test_kernels_gpu.py: simulate against the oracle


def _ops():
    from quattro_ilqr_amd import models, ops
    return models, ops


def _dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _close(a, b):
    """relative Frobenius distance of two device arrays within the simulate tolerance (and both finite)"""
    a, b = a.double(), b.double()
    return bool(torch.isfinite(a).all()) and float((a - b).norm()) <= SIM_TOL * float(b.norm())


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


_INPUTS = {}


def _inputs(integ):
    """x0 (33, 12), u (33, 51, 4), rounded to fp32, and the oracle's rollouts of every horizon in NS: computed once"""
    if integ not in _INPUTS:
        rng = np.random.default_rng(909)
        x0 = np.zeros(12)
        x0[2] = 0.5
        x0 = _f32(x0 + 0.2 * rng.standard_normal((max(BS), 12)))
        u = _f32(2.4525 + 0.3 * rng.standard_normal((max(BS), max(NS), 4)))
        spec = o_models.quadrotor_spec(0.01, o_models.INTEGRATOR_RK4 if integ == "rk4" else o_models.INTEGRATOR_EULER)
        _INPUTS[integ] = (x0, u, {N: o_lin.rollout_batched(spec, x0, u[:, :N]) for N in NS})
    return _INPUTS[integ]


def _alpha0(md, ops, xs, u, J):
    """the alpha = 0 candidate under zero gains, by the all-alpha rollout and by the fused line search"""
    B, N = u.shape[0], u.shape[1]
    K = torch.zeros((B, N, 4, 12), dtype=torch.float32, device=DEV)
    k = torch.zeros((B, N, 4), dtype=torch.float32, device=DEV)
    c0, xr, ur = ops.rollout(md, xs, u, K, k, (0.0,), want_traj=True)
    # the line search from a nominal whose rows 1 .. N are NOT the rollout's: what it commits is its own candidate
    x_ls = xs.clone()
    x_ls[:, 1:] += 0.25
    u_ls, J_ls = u.clone(), J.clone() + 1.0
    idx = ops.linesearch(md, x_ls, u_ls, K, k, J_ls, 1e-9, alphas=(0.0,))
    return (c0[0], xr[0], ur[0]), (J_ls, x_ls, u_ls, idx)


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_simulate_against_the_per_step_loads_and_the_oracle(integ):
    models, ops = _ops()
    md = models.quadrotor_model(integrator=integ)
    x0_all, u_all, oracle = _inputs(integ)
    worst = 0.0
    for N in NS:
        x_ref, J_ref = oracle[N]
        for B in BS:
            x0, u = _dev32(x0_all[:B]), _dev32(u_all[:B, :N])
            xs, J = ops.simulate(md, x0, u)
            (c0, xr, ur), (J_ls, x_ls, u_ls, idx) = _alpha0(md, ops, xs, u, J)
            torch.cuda.synchronize()
            assert _same(xs[:, 0], x0), (integ, B, N, "row 0 is x0")
            assert _same(xs, xr) and _same(J, c0) and _same(ur, u), (integ, B, N, "ops.rollout, alpha = 0")
            assert bool((idx == 0).all()), (integ, B, N, idx)
            assert _same(xs, x_ls) and _same(J, J_ls) and _same(u, u_ls), (integ, B, N, "ops.linesearch, alpha = 0")
            xe = np.linalg.norm(xs.double().cpu().numpy() - x_ref[:B]) / np.linalg.norm(x_ref[:B])
            Je = np.max(np.abs(J.cpu().numpy() - J_ref[:B]) / np.abs(J_ref[:B]))
            worst = max(worst, xe, Je)
            assert xe < SIM_TOL and Je < SIM_TOL, (integ, B, N, xe, Je)
    print(f"[simulate {integ}] worst relative error against the oracle {worst:.1e}")


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_simulate_stays_inside_its_trajectories(integ):
    """u and x as views into larger buffers: NaN around u, a sentinel around x; for B = 17 every second trajectory's controls are
    NaN as well (the rows past N of trajectory b are the first rows of trajectory b + 1; B = 17 also leaves the second wave a
    buffer resource that reaches 15 trajectories past the end of u)."""
    models, ops = _ops()
    md = models.quadrotor_model(integrator=integ)
    x0_all, u_all, _ = _inputs(integ)
    PAD, SENT = 256, 12345.0
    for B in (1, 17):
        for N in (1, 9):
            x0, u = _dev32(x0_all[:B]), _dev32(u_all[:B, :N])
            xs, J = ops.simulate(md, x0, u)
            ubuf = torch.full((2 * PAD + B * N * 4,), float("nan"), dtype=torch.float32, device=DEV)
            uv = ubuf[PAD:PAD + B * N * 4].view(B, N, 4)
            uv.copy_(u)
            holes = list(range(1, B, 2))
            if holes:
                uv[holes] = float("nan")
            xbuf = torch.full((2 * PAD + B * (N + 1) * 12,), SENT, dtype=torch.float32, device=DEV)
            xv = xbuf[PAD:PAD + B * (N + 1) * 12].view(B, N + 1, 12)
            Jbuf = torch.full((B + 2,), SENT, dtype=torch.float64, device=DEV)
            ops.simulate(md, x0, uv, x=xv, cost=Jbuf[1:B + 1])
            torch.cuda.synchronize()
            keep = [b for b in range(B) if b not in holes]
            if integ == "euler" or not holes:
                assert _same(xv[keep], xs[keep]) and _same(Jbuf[1:B + 1][keep], J[keep]), (integ, B, N)
            else:
                # an RK4 wave that holds a NaN angle takes stage_sincos' full reduction instead of its polynomial (rollout_quad_body.h:
                # a wave-wide vote), which may move its healthy trajectories by an ulp: finite and within the simulate tolerance
                assert _close(xv[keep], xs[keep]) and _close(Jbuf[1:B + 1][keep], J[keep]), (integ, B, N)
            for b in holes:      # (x0 is finite, the first control is not)
                assert _same(xv[b, 0], x0[b]) and bool(torch.isnan(xv[b, 1:]).any()) and bool(torch.isnan(Jbuf[1 + b])), (integ, B, N, b)
            assert bool((xbuf[:PAD] == SENT).all()) and bool((xbuf[-PAD:] == SENT).all()), (integ, B, N, "x written outside")
            assert float(Jbuf[0]) == SENT and float(Jbuf[-1]) == SENT, (integ, B, N, "cost written outside")
            assert bool(torch.isnan(ubuf[:PAD]).all()) and bool(torch.isnan(ubuf[-PAD:]).all())


# ------------------------------------------------------------------------------------------------ line search under masks
def _masks(B):
    on, off = [1] * B, [0] * B
    alt = [(b + 1) % 2 for b in range(B)]                       # one of the two trajectories of every wave
    alt2 = [b % 2 for b in range(B)]                            # ... the other one
    wave0 = [0 if b < 2 else 1 for b in range(B)]               # both trajectories of the first wave off
    wave1 = [1 if b < 2 else 0 for b in range(B)]               # ... of every other wave
    out = []
    for m in (on, off, alt, alt2, wave0, wave1):
        if m not in out:
            out.append(m)
    return out


def _ls_problem(md, ops, B, N, seed):
    """a nominal and gains the line search has something to do with: the backward pass's own"""
    rng = np.random.default_rng(seed)
    x0 = np.asarray(md.x_ref) + 0.2 * rng.standard_normal((B, 12))
    u = 2.4525 + 0.3 * rng.standard_normal((B, N, 4))
    x0, u = _dev32(x0), _dev32(u)
    xs, J = ops.simulate(md, x0, u)
    rec, VxN, VxxN, lay = ops.linearize(md, xs, u)
    K, k, st = ops.riccati_sweep(rec, VxN, VxxN, 12, 4, lay)
    assert int(st.abs().sum()) == 0
    return xs, u, K, k, J


def _run_ls(md, ops, xs, u, K, k, J, active):
    """-> (x, u, cost, alpha_idx, iters, active) after one fused line search, every array preset where the kernel only updates it"""
    B = u.shape[0]
    x_, u_, J_ = xs.clone(), u.clone(), J.clone()
    idx = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    iters = torch.full((B,), 3, dtype=torch.int32, device=DEV)
    act = None if active is None else torch.tensor(active, dtype=torch.int32, device=DEV)
    ops.linesearch(md, x_, u_, K, k, J_, 1e-9, alpha_idx=idx, active=act, iters=iters)
    torch.cuda.synchronize()
    return x_, u_, J_, idx, iters, act


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_line_search_under_active_masks(integ):
    models, ops = _ops()
    md = models.quadrotor_model(integrator=integ)
    accepted = set()
    for B in (1, 2, 3, 5):
        for N in (1, 4, 5, 51):
            xs, u, K, k, J = _ls_problem(md, ops, B, N, 31 * N + B)
            for mask in _masks(B):
                x_, u_, J_, idx, iters, act = _run_ls(md, ops, xs, u, K, k, J, mask)
                on = [b for b in range(B) if mask[b]]
                off = [b for b in range(B) if not mask[b]]
                tag = (integ, B, N, mask)
                if off:
                    assert _same(x_[off], xs[off]) and _same(u_[off], u[off]) and _same(J_[off], J[off]), tag
                    assert bool((idx[off] == -7).all()) and bool((iters[off] == 3).all()) and bool((act[off] == 0).all()), tag
                if on:
                    # the same trajectories in a batch of their own, with flags (all on) and without an array of flags: bit for bit
                    # (RK4: an RK4 candidate's bits may depend on the wave's other trajectory through stage_sincos' wave-wide vote, so
                    #  x, u and cost are held to the simulate tolerance there; the accepted index, iters and flags stay exact)
                    same = _same if integ == "euler" else _close
                    sub = [t[on].contiguous() for t in (xs, u, K, k, J)]
                    for flags in ([1] * len(on), None):
                        xo, uo, Jo, io, ito, ao = _run_ls(md, ops, *sub, flags)
                        assert same(x_[on], xo) and same(u_[on], uo) and same(J_[on], Jo), tag
                        assert torch.equal(idx[on], io) and torch.equal(iters[on], ito) and bool((ito == 4).all()), tag
                        if ao is not None:
                            assert torch.equal(act[on], ao), tag
                accepted |= set(int(v) for v in idx[on].cpu())
    print(f"[line search {integ}] accepted alpha indices {sorted(accepted)}")
    assert any(a >= 0 for a in accepted), "the masks were tested on line searches that commit something"
