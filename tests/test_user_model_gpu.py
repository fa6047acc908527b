"""User-compiled device models (quattro_ilqr_amd.user_model; csrc/user_model.h, csrc/dual.h) against the oracle.

The reference's iLQR_TF accepts any callables f, L, Lf (quattro_ilqr_tf.py:66-84).  Here a problem the reference does not
ship — a planar two-rotor vehicle with a non-diagonal, non-quadratic cost — is written once as C++ bodies, compiled
for the GPU, and compared with the fp64 oracle running the reference's algorithm (finite differences and all) on the
same problem written as Python callables; and the reference's own quadrotor, re-entered as a *user* model, must reproduce
the built-in kernels (which are pinned to the golden vectors elsewhere).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "quattro-transformer-ilqr_amd")]

from oracle import ilqr as O  # noqa: E402

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------- the planar vehicle
PHYS = (1.0, 0.05, 0.2, 9.81)                      # mass, inertia, arm, gravity
Q = np.array([1.0, 1.0, 1.0, 0.1, 0.1, 0.1]); R = np.array([0.01, 0.02]); QF = np.full(6, 10.0)
XREF = np.array([0.0, 1.0, 0.0, 0.0, 0.0, 0.0])
DT = 0.02

PLANAR_RATE = """
T s, c;
sincos(x[2], &s, &c);
const T thrust = (u[0] + u[1]) / P[0];
xd[0] = x[3];  xd[1] = x[4];  xd[2] = x[5];
xd[3] = -(thrust * s);
xd[4] = thrust * c - P[3];
xd[5] = (u[0] - u[1]) * (P[2] / P[1]);
"""
PLANAR_L = "return default_stage_cost<T>(p, x, u) + x[0] * x[2] * 0.3f + exp(u[0] * 0.1f) * 0.01f;"
PLANAR_LF = "return default_final_cost<T>(p, x) + x[0] * x[1] * 0.5f;"


def planar_rate(x, u):
    m, inertia, arm, g = PHYS
    s, c = np.sin(x[2]), np.cos(x[2])
    th = (u[0] + u[1]) / m
    return np.array([x[3], x[4], x[5], -th * s, th * c - g, (u[0] - u[1]) * arm / inertia])


def planar_f(integrator):
    def f(x, u):
        if integrator == "euler":
            return x + DT * planar_rate(x, u)
        k1 = planar_rate(x, u)
        k2 = planar_rate(x + 0.5 * DT * k1, u)
        k3 = planar_rate(x + 0.5 * DT * k2, u)
        k4 = planar_rate(x + DT * k3, u)
        return x + DT / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    return f


def planar_L(x, u):
    d = x - XREF
    return np.sum(Q * d * d) + np.sum(R * u * u) + 0.3 * x[0] * x[2] + 0.01 * np.exp(0.1 * u[0])


def planar_Lf(x):
    d = x - XREF
    return np.sum(QF * d * d) + 0.5 * x[0] * x[1]


def planar_model(integrator):
    import quattro_ilqr_amd as q
    return q.compile_model("planar", 6, 2, rate=PLANAR_RATE, stage_cost=PLANAR_L, final_cost=PLANAR_LF, dt=DT,
                           integrator=integrator, phys=PHYS, q=Q, r=R, qf=QF, x_ref=XREF)


def planar_batch(B, N, seed=0):
    rng = np.random.default_rng(seed)
    x0 = XREF + rng.normal(0, 0.3, (B, 6)) * np.array([1, 1, 0.3, 0.5, 0.5, 0.5])
    u0 = np.full((B, N, 2), PHYS[0] * PHYS[3] / 2) + rng.normal(0, 0.2, (B, N, 2))
    return x0, u0



# ---------------------------------------------------------------------------------------------- planar + slack: an indefinite Q_uu
# The planar vehicle with a third control u[0] that does not enter the dynamics (u[1], u[2] are the thrusts) and a stage cost
# that couples it to them: planar cost + c u0 (u1 - u2) + w/4 u0^4 (bounded below), r = (0, 0.01, 0.02).  Where u0 = 0 the slack's
# own second derivative is exactly 0, so Q_uu + reg I starts with the pivot reg = 1e-6 and is indefinite (eigenvalues of both
# signs, condition number ~40): an elimination without pivoting — the MFMA tile sweep a user model with n <= 12, m <= 4 gets —
# loses ~10 % of the inverse in fp32 and flags the trajectory QUATTRO_TRAJ_ILLCOND, and every user-model loop must then use
# the pivoting sweep, as the reference's np.linalg.inv (quattro_ilqr_tf.py:306) does.  Where |u0| >= 1.6 the 3 w u0^2 term
# makes the block positive definite (not flagged); from u0 = 2 one accepted iteration brings u0 to ~1.3, indefinite again.
SLACK_C, SLACK_W = 0.3, 1.0
SLACK_R = np.array([0.0, 0.01, 0.02])
SLACK_FLAG, SLACK_CLEAR = 0.0, 2.0                 # slack values that make a step flagged / positive definite at the start
SLACK_RATE = PLANAR_RATE.replace("u[0] + u[1]", "u[1] + u[2]").replace("u[0] - u[1]", "u[1] - u[2]")
SLACK_L = ("return default_stage_cost<T>(p, x, u) + x[0] * x[2] * 0.3f + exp(u[1] * 0.1f) * 0.01f"
           f" + u[0] * (u[1] - u[2]) * {SLACK_C}f + u[0] * u[0] * u[0] * u[0] * {0.25 * SLACK_W}f;")


def slack_rate(x, u):
    return planar_rate(x, u[1:])


def slack_f(integrator):
    def f(x, u):
        if integrator == "euler":
            return x + DT * slack_rate(x, u)
        k1 = slack_rate(x, u)
        k2 = slack_rate(x + 0.5 * DT * k1, u)
        k3 = slack_rate(x + 0.5 * DT * k2, u)
        k4 = slack_rate(x + DT * k3, u)
        return x + DT / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    return f


def slack_L(x, u):
    d = x - XREF
    return (np.sum(Q * d * d) + np.sum(SLACK_R * u * u) + 0.3 * x[0] * x[2] + 0.01 * np.exp(0.1 * u[1])
            + SLACK_C * u[0] * (u[1] - u[2]) + 0.25 * SLACK_W * u[0] ** 4)


slack_Lf = planar_Lf


def slack_model(integrator):
    import quattro_ilqr_amd as q
    return q.compile_model("planar_slack", 6, 3, rate=SLACK_RATE, stage_cost=SLACK_L, final_cost=PLANAR_LF, dt=DT,
                           integrator=integrator, phys=PHYS, q=Q, r=SLACK_R, qf=QF, x_ref=XREF)


def slack_batch(slack, N, seed=0):
    """x0 (B, 6), u0 (B, N, 3) in fp32-representable fp64: planar starts, u0[b, t, 0] = slack[b] (a value per trajectory, or a
    row of N values per trajectory)."""
    slack = np.asarray(slack, dtype=np.float64)
    B = slack.shape[0]
    x0, uth = planar_batch(B, N, seed)
    u0 = np.concatenate([np.broadcast_to(slack.reshape(B, -1, 1), (B, N, 1)), uth], axis=2)
    return x0.astype(np.float32).astype(np.float64), u0.astype(np.float32).astype(np.float64)

def complex_step_jac(fun, z, h=1e-30):
    """Exact (to fp64 round-off) Jacobian of an analytic function by complex-step differentiation."""
    z = np.asarray(z, dtype=np.complex128)
    cols = []
    for i in range(z.size):
        zp = z.copy(); zp[i] += 1j * h
        cols.append(np.imag(np.atleast_1d(fun(zp))) / h)
    return np.array(cols).T


# branch-on-real-part versions of the kinked functions, for complex-step differentiation through a model that uses them
# (ties as in csrc/dual.h: fabs(0) = +z, fmax / fmin take the first argument)
def cs_fabs(z):
    return -z if np.real(z) < 0 else z


def cs_fmax(a, b):
    return a if np.real(a) >= np.real(b) else b


def cs_fmin(a, b):
    return a if np.real(a) <= np.real(b) else b


def exact_derivs(f, L, x, u):
    n, m = x.size, u.size
    z = np.concatenate([x, u])
    F = complex_step_jac(lambda zz: f(zz[:n], zz[n:]), z)
    grad = lambda zz: complex_step_jac(lambda w: L(w[:n], w[n:]), zz)[0]
    g = grad(z)
    H = np.zeros((n + m, n + m))
    eps = 1e-6
    for i in range(n + m):
        e = np.zeros(n + m); e[i] = eps
        H[:, i] = (grad(z + e) - grad(z - e)) / (2 * eps)
    return F[:, :n], F[:, n:], g[:n], g[n:], H[:n, :n], H[n:, n:], H[n:, :n]



def exact_records(f, L, Lf, xs, us):
    """fp64 derivative blocks of a batch at the nominal (xs (B, N+1, n), us (B, N, m)) from exact_derivs, in the layout of
    oracle.ilqr.riccati_sweep_batched."""
    B, N, n = us.shape[0], us.shape[1], xs.shape[2]
    names = ("A", "B", "lx", "lu", "lxx", "luu", "lux")
    d = {k: [] for k in names}
    for b in range(B):
        per = [exact_derivs(f, L, xs[b, t], us[b, t]) for t in range(N)]
        for i, k in enumerate(names):
            d[k].append(np.array([p[i] for p in per]))
    d = {k: np.array(v) for k, v in d.items()}
    grad = lambda z: complex_step_jac(Lf, z)[0]
    d["VxN"] = np.array([grad(xs[b, N]) for b in range(B)])
    eps = 1e-6
    d["VxxN"] = np.array([np.array([(grad(xs[b, N] + eps * e) - grad(xs[b, N] - eps * e)) / (2 * eps) for e in np.eye(n)]).T
                          for b in range(B)])
    return d


def exact_sweep(f, L, Lf, xs, us):
    """-> k (B, N, m), K (B, N, m, n), Q_uu + reg I (B, N, m, m): the fp64 oracle sweep on exact derivatives."""
    d = exact_records(f, L, Lf, xs, us)
    quu = np.zeros(us.shape + (us.shape[2],))
    k, K = O.riccati_sweep_batched(d, quu_out=quu)
    return k, K, quu

# ---------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_user_model_derivative_records_are_exact(integrator):
    """Records from forward-mode differentiation on the device vs exact fp64 derivatives of the same problem in Python
    (complex step), and vs the reference's finite differences (oracle) at their own noise level."""
    import torch
    from quattro_ilqr_amd import _lib, ops
    md = planar_model(integrator)
    f = planar_f(integrator)
    B, N = 5, 12
    x0, u0 = planar_batch(B, N, 1)
    dev = torch.device("cuda:0")
    x, cost = ops.simulate(md, torch.as_tensor(x0, dtype=torch.float32, device=dev),
                           torch.as_tensor(u0, dtype=torch.float32, device=dev))
    xs = x.double().cpu().numpy()
    for b in range(B):                                   # rollout + cost of the float instantiation
        xo = O.rollout(f, x0[b], u0[b])
        assert np.max(np.abs(xs[b] - xo)) < 2e-5
        assert abs(cost[b].item() - O.trajectory_cost(planar_L, planar_Lf, xo, u0[b])) < 1e-5 * abs(cost[b].item())
    rec, VxN, VxxN, layout = ops.linearize(md, x, torch.as_tensor(u0, dtype=torch.float32, device=dev))
    assert layout == _lib.LAYOUT_ROWMAJOR_TILE          # ROWMAJOR records, swept by the MFMA tile kernel (n <= 12, m <= 4)
    blocks = {k: v.double().cpu().numpy() for k, v in ops.unpack_derivs(rec, B, 6, 2, layout, lib=_lib.load_for(md)).items()}
    worst = {}
    for b in range(B):
        for t in range(N):
            A, Bm, lx, lu, lxx, luu, lux = exact_derivs(f, planar_L, xs[b, t], u0[b, t].astype(np.float32).astype(np.float64))
            for name, ref in (("A", A), ("B", Bm), ("lx", lx), ("lu", lu), ("lxx", lxx), ("luu", luu), ("lux", lux)):
                err = np.max(np.abs(blocks[name][b, t] - ref)) / max(1.0, np.max(np.abs(ref)))
                worst[name] = max(worst.get(name, 0.0), err)
    print("user-model records vs exact derivatives (max abs / max(1, |ref|)):", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) < 1e-6                    # measured 4e-8
    # terminal pair
    gN = complex_step_jac(lambda w: planar_Lf(w), xs[0, N])[0]
    assert np.max(np.abs(VxN[0].double().cpu().numpy() - gN)) < 1e-5 * max(1.0, np.max(np.abs(gN)))
    HN = VxxN[0].double().cpu().numpy()
    assert np.max(np.abs(HN - HN.T)) < 1e-6 and np.max(np.abs(np.diag(HN) - 2 * QF)) < 1e-5 and abs(HN[0, 1] - 0.5) < 1e-6
    # the reference's own finite differences of the same callables (what its backward pass would consume)
    d = O.linearize_fd(f, planar_L, planar_Lf, xs[0], [u for u in u0[0].astype(np.float32).astype(np.float64)])
    assert np.max(np.abs(blocks["A"][0] - d["A"])) < 1e-5 and np.max(np.abs(blocks["B"][0] - d["B"])) < 1e-5
    assert np.max(np.abs(blocks["lxx"][0] - d["lxx"])) < 5e-4 and np.max(np.abs(blocks["lux"][0] - d["lux"])) < 5e-4


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_user_model_solve_matches_the_oracle(integrator):
    """Whole solves of the planar problem: the reference's algorithm in fp64 (oracle.optimize on Python callables) vs
    QuattroILQR on the compiled model — same accepted step sizes, same iteration count, same optimum."""
    import torch
    import quattro_ilqr_amd as q
    md = planar_model(integrator)
    f = planar_f(integrator)
    B, N = 6, 30
    x0, u0 = planar_batch(B, N, 2)
    s = q.QuattroILQR(md, N, max_iter=40, tol=1e-3, device="cuda:0")
    out = s.solve(torch.as_tensor(x0, dtype=torch.float32), torch.as_tensor(u0, dtype=torch.float32))
    u_dev, x_dev = out["u"].double().cpu().numpy(), out["x"].double().cpu().numpy()
    it_dev, cost_dev = out["iters"].cpu().numpy(), out["cost"].cpu().numpy()
    same_iters = 0
    for b in range(B):
        u_o, x_o, logs = O.optimize(f, planar_L, planar_Lf, x0[b], list(u0[b].astype(np.float32).astype(np.float64)), N,
                                    max_iter=40, tol=1e-3)
        J_o = O.trajectory_cost(planar_L, planar_Lf, x_o, u_o)
        same_iters += int(len(logs) == it_dev[b])
        print(f"planar/{integrator} b={b}: iterations oracle {len(logs)} device {it_dev[b]}, cost {J_o:.6f} vs {cost_dev[b]:.6f}, "
              f"max|dx| {np.max(np.abs(x_dev[b] - x_o)):.2e} max|du| {np.max(np.abs(u_dev[b] - np.array(u_o))):.2e}")
        assert abs(len(logs) - it_dev[b]) <= 1            # the stop test |dJ| < tol sits on fp32-vs-fp64 round-off at the end
        if len(logs) == it_dev[b]:                        # measured: 2e-7 relative cost, 5e-7 in x, 3e-6 in u
            assert abs(J_o - cost_dev[b]) < 1e-6 * abs(J_o)
            assert np.max(np.abs(x_dev[b] - x_o)) < 1e-5 and np.max(np.abs(u_dev[b] - np.array(u_o))) < 3e-5
    assert same_iters >= B - 1
    # first iteration alone, from identical nominals: gains against the reference's FD backward pass
    s2 = q.QuattroILQR(md, N, device="cuda:0")
    s2.solve(torch.as_tensor(x0, dtype=torch.float32), torch.as_tensor(u0, dtype=torch.float32), max_iter=0)
    xs = s2.x.double().cpu().numpy().copy()
    s2.iterate()
    K_dev, k_dev = s2.K.double().cpu().numpy(), s2.k.double().cpu().numpy()
    for b in range(2):
        k_o, K_o = O.backward_pass(f, planar_L, planar_Lf, xs[b], list(u0[b].astype(np.float32).astype(np.float64)))
        K_o, k_o = np.array(K_o), np.array(k_o)
        eK = np.linalg.norm(K_dev[b] - K_o) / np.linalg.norm(K_o)
        ek = np.linalg.norm(k_dev[b] - k_o) / np.linalg.norm(k_o)
        print(f"planar/{integrator} first sweep b={b}: rel-Fro K {eK:.2e} k {ek:.2e}")
        assert eK < 1e-4 and ek < 1e-4                    # measured 1.2e-5 / 1.5e-5: the reference's FD noise on this problem


QUAD_RATE = """
const float mass = P[0], Ix = P[1], Iy = P[2], Iz = P[3], arm = P[4], grav = P[5], kyaw = P[6];
T sph, cph, sth, cth, sps, cps;
sincos(x[6], &sph, &cph);  sincos(x[7], &sth, &cth);  sincos(x[8], &sps, &cps);
const T sec = 1.0f / cth, tth = sth * sec;
const T wp = x[9], wq = x[10], wr = x[11];
const T tm = (u[0] + u[1] + u[2] + u[3]) / mass;
xd[0] = x[3];  xd[1] = x[4];  xd[2] = x[5];
xd[3] = tm * (sps * sph + cps * sth * cph);
xd[4] = tm * (cps * sph - sps * sth * cph);
xd[5] = tm * (cth * cph) - grav;
const T mix = wq * sph + wr * cph;
xd[6] = wp + mix * tth;
xd[7] = wq * cph - wr * sph;
xd[8] = mix * sec;
xd[9] = (wq * wr) * ((Iy - Iz) / Ix) + ((u[1] + u[2]) - (u[0] + u[3])) * (arm / Ix);
xd[10] = (wp * wr) * ((Iz - Ix) / Iy) + ((u[0] + u[1]) - (u[2] + u[3])) * (arm / Iy);
xd[11] = (wp * wq) * ((Ix - Iy) / Iz) + (u[0] - u[1] + u[2] - u[3]) * (kyaw / Iz);
"""


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_quadrotor_reentered_as_user_model_reproduces_the_builtin_kernels(integrator):
    """quadrotor_dynamics.py:63-164 + the barrier cost typed in as a user model (n = 12, m = 4, default cost): differentiated
    automatically and solved by the generic kernels, it must agree with the hand-derived built-in path."""
    import torch
    import quattro_ilqr_amd as q
    from bench import synthetic_batch
    builtin = q.quadrotor_model(integrator=integrator)
    user = q.compile_model("quadrotor_user", 12, 4, rate=QUAD_RATE, dt=builtin.dt, integrator=integrator, phys=builtin.phys,
                           q=builtin.q, r=builtin.r, qf=builtin.qf, x_ref=builtin.x_ref,
                           barrier_alpha=builtin.barrier_alpha, barrier_beta=builtin.barrier_beta)
    B, N = 64, 50
    x0, u0 = synthetic_batch(B, 0)
    x0 = torch.as_tensor(x0, dtype=torch.float32, device="cuda:0"); u0 = torch.as_tensor(u0, dtype=torch.float32, device="cuda:0")
    sb = q.QuattroILQR(builtin, N, device="cuda:0"); su = q.QuattroILQR(user, N, device="cuda:0")
    sb.solve(x0, u0, max_iter=1); su.solve(x0, u0, max_iter=1)
    eK = (torch.linalg.norm((sb.K - su.K).double().reshape(B, -1), dim=1) / torch.linalg.norm(sb.K.double().reshape(B, -1), dim=1)).max().item()
    ek = (torch.linalg.norm((sb.k - su.k).double().reshape(B, -1), dim=1) / torch.linalg.norm(sb.k.double().reshape(B, -1), dim=1)).max().item()
    print(f"user-model quadrotor vs built-in ({integrator}), first sweep: rel-Fro K {eK:.2e} k {ek:.2e}")
    assert eK < 2e-5 and ek < 2e-5
    assert torch.equal(sb.alpha_idx, su.alpha_idx)
    ob = {k: v.clone() for k, v in sb.solve(x0, u0).items()}
    ou = su.solve(x0, u0)
    same = (ob["iters"] == ou["iters"]).float().mean().item()
    rel = ((ob["cost"] - ou["cost"]).abs() / ob["cost"].abs()).max().item()
    print(f"converged solves: same iteration count on {100 * same:.0f} %, max rel cost difference {rel:.2e}, "
          f"max|du| {(ob['u'] - ou['u']).abs().max().item():.2e}")
    assert same >= 0.9 and rel < 1e-4


def test_user_model_through_the_dropin_class_and_the_mpc_loop():
    """iLQR_TF(model=<user model>) — the reference's class surface — and BatchedMPC run on the same compiled problem."""
    import torch
    import quattro_ilqr_amd as q
    md = planar_model("rk4")
    N = 25
    x0, u0 = planar_batch(3, N, 3)
    il = q.iLQR_TF(md, md, md, x0[0], [u for u in u0[0]], N, dt=DT, max_iter=30, tol=1e-3, device="cuda:0")
    u_opt, x_opt = il.optimize(XREF)
    s = q.QuattroILQR(md, N, max_iter=30, tol=1e-3, device="cuda:0")
    out = s.solve(torch.as_tensor(x0[:1], dtype=torch.float32), torch.as_tensor(u0[:1], dtype=torch.float32))
    assert np.max(np.abs(np.array(u_opt) - out["u"][0].double().cpu().numpy())) < 1e-6
    assert len(il.logs) == int(out["iters"][0])
    k_seq, K_seq = il.backward_pass(il.simulate([u for u in u0[0]]), [u for u in u0[0]])
    assert np.array(K_seq).shape == (N, 2, 6) and np.array(k_seq).shape == (N, 2)
    mpc = q.BatchedMPC(md, N, max_iter=30, device="cuda:0")
    run = mpc.run(torch.as_tensor(x0, dtype=torch.float32), 8)
    xs = run["x"].double().cpu().numpy()
    d0 = np.linalg.norm(xs[:, 0, :3] - XREF[:3], axis=1); d1 = np.linalg.norm(xs[:, -1, :3] - XREF[:3], axis=1)
    assert run["x"].shape == (3, 9, 6) and np.all(np.isfinite(xs)) and np.all(d1 < d0)


def test_user_model_is_refused_by_the_stock_library_and_by_bad_dims():
    import ctypes
    import quattro_ilqr_amd as q
    from quattro_ilqr_amd import _lib
    md = planar_model("euler")
    p = md.c_params()
    assert _lib.load().quattro_model_layout(ctypes.byref(p)) == -1               # libquattro_hip.so has no model 3
    assert _lib.load_for(md).quattro_model_layout(ctypes.byref(p)) == _lib.LAYOUT_ROWMAJOR_TILE
    with pytest.raises(ValueError):
        q.compile_model("too_big", 17, 2, rate="xd[0] = x[0];")
    with pytest.raises(_lib.QuattroError):
        q.compile_model("broken", 2, 1, rate="xd[0] = undefined_symbol;")


def test_user_model_whole_workflow_collect_fit_hybrid():
    """The reference's actual use case on a problem it does not ship: iLQR logs of the user model -> training set -> fit a
    gain predictor (state_dim 6, control_dim m (1 + n) = 14: the layer-wise kernels, no fused shape) -> hybrid solves where
    the predictor supplies the first N - P steps' gains (training_data_collection.py:196-214, transformer_ilqr.py:102-208,
    quattro_ilqr_tf.py:476-591)."""
    import torch
    import quattro_ilqr_amd as q
    from quattro_ilqr_amd import datagen
    md = planar_model("rk4")
    N, P, B = 30, 5, 128
    x0, u0 = planar_batch(B, N, 5)
    log = datagen.collect(q.QuattroILQR(md, N, max_iter=6, tol=1e-3, device="cuda:0"), x0, u0)
    assert len(log) > B and log.K_seq.shape[1:] == (N, 2, 6) and log.x_seq.shape[1:] == (N + 1, 6)
    rng = np.random.default_rng(0)
    perm = rng.permutation(len(log))
    n_train = int(0.8 * len(log))
    tf = q.TransformerILQR(6, 14, prompt_len=P, d_model=64, nhead=4, num_decoder_layers=2, dim_feedforward=128, dropout=0.0,
                           max_seq_len=80, device="cuda:0")
    tf.fit(log.select(perm[:n_train]), log.select(perm[n_train:]), num_epochs=20, batch_size=32, learning_rate=1e-3, patience=20)
    assert tf.train_loss_history[-1] < 0.5 * tf.train_loss_history[0]
    hyb = q.QuattroILQR(md, N, max_iter=4, tol=1e-3, tf=tf, device="cuda:0")
    out = hyb.solve(x0[:16], u0[:16])
    _, cost0 = q.ops.simulate(md, torch.as_tensor(x0[:16], dtype=torch.float32, device="cuda:0"),
                              torch.as_tensor(u0[:16], dtype=torch.float32, device="cuda:0"))
    assert bool(torch.isfinite(out["cost"]).all()) and int((out["iters"] >= 1).sum()) == 16
    assert bool((out["cost"] <= cost0).all())               # accepted steps never increase the cost
    # the drop-in class takes the same decisions with the same predictor
    il = q.iLQR_TF(md, md, md, x0[0], [u for u in u0[0]], N, dt=DT, max_iter=4, tol=1e-3, tf=tf, device="cuda:0")
    u_fin, x_fin = il.optimize(XREF)
    assert len(il.logs) == int(out["iters"][0])
    assert np.max(np.abs(x_fin - out["x"][0].double().cpu().numpy())) < 1e-4


@pytest.mark.parametrize("problem,integrator,B,N", [
    pytest.param("planar", "rk4", 1, 30, id="rk4-1-30"), pytest.param("planar", "euler", 37, 25, id="euler-37-25"),
    pytest.param("planar", "rk4", 300, 50, id="rk4-300-50"), pytest.param("planar", "euler", 5, 7, id="euler-5-7"),
    pytest.param("slack", "rk4", 1, 30, id="slack-rk4-1-30"), pytest.param("slack", "euler", 37, 25, id="slack-euler-37-25"),
    pytest.param("slack", "rk4", 300, 50, id="slack-rk4-300-50")])
def test_user_model_device_resident_solve_and_mpc_equal_the_host_driven_loops(problem, integrator, B, N):
    """A user model's library has a persistent kernel of its own (csrc/solve_user.hip: one wave per trajectory, the generic
    device bodies): quattro_ilqr_solve_f32 / quattro_mpc_run_f32 as ONE launch against the host-driven loops of the same
    library, bit for bit — real exit tests, capped and fixed iteration counts, warm and cold starts, a disturbed closed loop
    and a second run that continues from the first one's warm start.  "slack": the planar + slack problem, whose flagged
    trajectories both loops re-sweep with pivoting."""
    import torch
    import quattro_ilqr_amd as q
    if problem == "planar":
        md = planar_model(integrator)
        x0, u0 = planar_batch(B, N, 11 * B + N)
    else:
        md = slack_model(integrator)
        x0, u0 = slack_batch(np.where(np.arange(B) % 2 == 0, SLACK_FLAG, SLACK_CLEAR), N, 11 * B + N)
    assert q.ops.model_can_device_loop(md) and not q.ops.model_has_device_loop(md)     # exists; enqueued iterations are the default
    keys = ("K", "k", "x", "u", "cost", "iters", "alpha", "status")
    tw = 0 if N <= 10 else 10
    for kw in (dict(), dict(max_iter=2), dict(max_iter=3, fixed_iters=True)):
        for u_init in (u0, None):
            dev = q.QuattroILQR(md, N, max_iter=20, device="cuda:0", device_loop="always", tf_window=tw)
            host = q.QuattroILQR(md, N, max_iter=20, device="cuda:0", device_loop=False, check_every=1, tf_window=tw)
            od = {k: v.clone() for k, v in dev.solve(x0, u_init, **kw).items()}
            oh = host.solve(x0, u_init, **kw)
            for key in keys:
                assert torch.equal(od[key], oh[key]), (integrator, B, N, kw, u_init is None, key)
            assert torch.equal(dev.active, host.active) and torch.equal(dev.alpha_idx, host.alpha_idx)
    steps = 3
    rng = np.random.default_rng(B)
    dist = torch.as_tensor(1e-3 * rng.standard_normal((steps, B, 6)), dtype=torch.float32, device="cuda:0")
    a = q.BatchedMPC(md, N, max_iter=6, device="cuda:0", check_every=1, tf_window=tw)
    b = q.BatchedMPC(md, N, max_iter=6, device="cuda:0", check_every=1, tf_window=tw)
    for rep, d in enumerate((dist, None)):
        start = x0.astype(np.float32) if rep == 0 else oa["x"][:, -1].clone()
        oa = a.run(start, steps, disturbance=d, device_loop="always")
        ob = b.run(start, steps, disturbance=d, device_loop=False)
        for key in ("x", "u", "iters"):
            assert torch.equal(oa[key], ob[key].to(oa[key].dtype)), (rep, key)
        assert torch.equal(a.u_warm, b.u_warm)
        for name in ("K", "k", "x", "cost", "alpha_idx", "status"):
            assert torch.equal(getattr(a.solver, name), getattr(b.solver, name)), (rep, name)


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_user_model_against_the_reference_run_on_the_same_problem(integrator):
    """G13 (tests/golden/user_planar.npz): the REFERENCE's iLQR_TF, run in the build container on this problem as plain Python
    callables, against the compiled model on the GPU: iteration counts and accepted step sizes exactly, first-iteration gains
    at the reference's finite-difference noise, trajectories and optimum to fp32 round-off."""
    import torch
    import quattro_ilqr_amd as q
    from conftest import load_golden
    g = load_golden("user_planar.npz")
    assert np.array_equal(g["phys"], PHYS) and np.array_equal(g["Q"], Q) and np.array_equal(g["R"], R) and float(g["dt"]) == DT
    md = planar_model(integrator)
    N, S = int(g["N"]), g["x0"].shape[0]
    s = q.QuattroILQR(md, N, max_iter=int(g["max_iter"]), tol=float(g["tol"]), device="cuda:0", check_every=1)
    out = s.solve(torch.as_tensor(g["x0"], dtype=torch.float32), torch.as_tensor(g["u_init"], dtype=torch.float32))
    for b in range(S):
        key = f"{integrator}_s{b}_"
        n_it = int(g[key + "n_iter"])
        assert int(out["iters"][b]) == n_it
        assert float(out["alpha"][b]) == float(g[key + "alpha"][n_it - 1])          # last accepted step size
        ex = np.max(np.abs(out["x"][b].double().cpu().numpy() - g[key + "x_final"]))
        eu = np.max(np.abs(out["u"][b].double().cpu().numpy() - g[key + "u_final"]))
        print(f"planar/{integrator} b={b} vs the reference: {n_it} iterations, max|dx| {ex:.2e}, max|du| {eu:.2e}")
        assert ex < 1e-5 and eu < 3e-5
    # the whole alpha sequence and the first iteration's gains, through the drop-in class (one trajectory, the reference's loop)
    il = q.iLQR_TF(md, md, md, g["x0"][0], [u for u in g["u_init"][0]], N, dt=DT, max_iter=int(g["max_iter"]), tol=float(g["tol"]),
                   device="cuda:0")
    il.optimize(g["x_ref"])
    key = f"{integrator}_s0_"
    assert len(il.logs) == int(g[key + "n_iter"])
    assert [(-1.0 if lg["alpha"] is None else lg["alpha"]) for lg in il.logs] == list(g[key + "alpha"][:len(il.logs)])
    K0 = np.array(il.logs[0]["K_seq"])
    eK = np.linalg.norm(K0 - g[key + "K"][0]) / np.linalg.norm(g[key + "K"][0])
    print(f"planar/{integrator} first-iteration gains vs the reference: rel-Fro {eK:.2e}")
    assert eK < 1e-4


# ---------------------------------------------------------------------------------------------- the largest dims the header allows
CHAIN_RATE = """
// NU pendulum-like links coupled to their neighbours: x = (angles, rates), u = torques
for (int i = 0; i < NU; ++i) {
  xd[i] = x[NU + i];
  const T left = i > 0 ? x[i - 1] : x[i], right = i < NU - 1 ? x[i + 1] : x[i];
  xd[NU + i] = u[i] - sin(x[i]) * P[0] - x[NU + i] * P[1] + (left + right - x[i] * 2.0f) * P[2];
}
"""


def chain_rate(x, u, P=(2.0, 0.3, 1.5)):
    W = u.shape[0]
    xd = np.zeros(2 * W, dtype=np.result_type(x, u))
    for i in range(W):
        xd[i] = x[W + i]
        left = x[i - 1] if i > 0 else x[i]
        right = x[i + 1] if i < W - 1 else x[i]
        xd[W + i] = u[i] - np.sin(x[i]) * P[0] - x[W + i] * P[1] + (left + right - 2.0 * x[i]) * P[2]
    return xd


@pytest.mark.parametrize("W", [5, 8])
def test_user_model_at_the_largest_dimensions(W):
    """A chain of W links: n = 2 W, m = W.  W = 8 is n = 16, m = 8 (QUATTRO_MAX_NX / QUATTRO_MAX_NU: 32 lanes per linearisation
    item, an 8 x 8 pivoted inverse per sweep step, 128-float gain rows in the rollouts); W = 5 (n = 10, m = 5) is the middle
    case, 16 lanes per item.  Default diagonal cost with a control barrier: records vs complex-step fp64 derivatives, first
    sweep and a whole solve vs the oracle on the same problem as Python callables; the model's own device-resident loop bit
    for bit against its host-driven one."""
    import torch
    import quattro_ilqr_amd as q
    from quattro_ilqr_amd import _lib, ops
    dt, N, B = 0.02, 12, 4
    n, m = 2 * W, W
    qd = np.concatenate([np.full(W, 2.0), np.full(W, 0.2)]); rd = np.full(W, 0.05); qfd = np.concatenate([np.full(W, 20.0), np.full(W, 2.0)])
    xref = np.concatenate([0.2 * np.arange(W) / W, np.zeros(W)])
    md = q.compile_model(f"chain{n}x{m}", n, m, rate=CHAIN_RATE, dt=dt, integrator="rk4", phys=(2.0, 0.3, 1.5), q=qd, r=rd, qf=qfd,
                         x_ref=xref, barrier_alpha=0.5, barrier_beta=4.0)

    def f(x, u):
        k1 = chain_rate(x, u); k2 = chain_rate(x + 0.5 * dt * k1, u); k3 = chain_rate(x + 0.5 * dt * k2, u); k4 = chain_rate(x + dt * k3, u)
        return x + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)

    def softplus(z, beta):
        return np.log1p(np.exp(-np.abs(beta * z))) / beta + np.maximum(z, 0)       # (real arguments only)

    def L(x, u):
        d = x - xref
        return np.sum(qd * d * d) + np.sum(rd * u * u) + 0.5 * np.sum(softplus(-u, 4.0) ** 2)

    def Lf(x):
        d = x - xref
        return np.sum(qfd * d * d)

    rng = np.random.default_rng(4)
    x0 = (xref + 0.3 * rng.standard_normal((B, n))).astype(np.float32).astype(np.float64)
    u0 = (0.4 + 0.3 * rng.standard_normal((B, N, m))).astype(np.float32).astype(np.float64)
    dev = torch.device("cuda:0")
    x, _ = ops.simulate(md, torch.as_tensor(x0, dtype=torch.float32, device=dev), torch.as_tensor(u0, dtype=torch.float32, device=dev))
    xs = x.double().cpu().numpy()
    assert np.max(np.abs(xs[0] - O.rollout(f, x0[0], u0[0]))) < 2e-5
    rec, VxN, VxxN, layout = ops.linearize(md, x, torch.as_tensor(u0, dtype=torch.float32, device=dev))
    blocks = {k: v.double().cpu().numpy() for k, v in ops.unpack_derivs(rec, B, n, m, layout, lib=_lib.load_for(md)).items()}
    A = complex_step_jac(lambda z: f(z[:n], z[n:]), np.concatenate([xs[1, 3], u0[1, 3]]))
    assert np.max(np.abs(blocks["A"][1, 3] - A[:, :n])) < 2e-6 and np.max(np.abs(blocks["B"][1, 3] - A[:, n:])) < 2e-6
    d = O.linearize_fd(f, L, Lf, xs[1], [u for u in u0[1]])                  # the reference's finite differences
    assert np.max(np.abs(blocks["luu"][1] - d["luu"])) < 5e-4 and np.max(np.abs(blocks["lxx"][1] - d["lxx"])) < 5e-4
    assert np.max(np.abs(blocks["lu"][1] - d["lu"])) < 1e-5 * max(1.0, np.max(np.abs(d["lu"])))
    s = q.QuattroILQR(md, N, max_iter=15, tol=1e-3, device="cuda:0", tf_window=0)
    s.solve(x0, u0, max_iter=0)
    s.iterate()
    k_o, K_o = O.backward_pass(f, L, Lf, xs[0], [u for u in u0[0]])
    eK = np.linalg.norm(s.K[0].double().cpu().numpy() - np.array(K_o)) / np.linalg.norm(np.array(K_o))
    print(f"chain {n} x {m} first sweep vs the oracle: rel-Fro K {eK:.2e}")
    assert eK < 2e-4 and int(s.status.abs().sum()) == 0
    out = {k: v.clone() for k, v in s.solve(x0, u0).items()}
    for b in range(2):
        u_o, x_o, logs = O.optimize(f, L, Lf, x0[b], [u for u in u0[b]], N, max_iter=15, tol=1e-3)
        assert abs(len(logs) - int(out["iters"][b])) <= 1
        if len(logs) == int(out["iters"][b]):
            assert np.max(np.abs(out["x"][b].double().cpu().numpy() - x_o)) < 2e-4
    alw = q.QuattroILQR(md, N, max_iter=15, tol=1e-3, device="cuda:0", tf_window=0, device_loop="always")
    oa = alw.solve(x0, u0)
    for key in ("K", "k", "x", "u", "cost", "iters", "alpha"):
        assert torch.equal(oa[key], out[key]), key


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_user_model_runs_on_the_tile_sweep_and_equals_the_generic_one(integrator):
    """A user model with n <= 12, m <= 4 (the planar example: 6, 2) gets the MFMA tile sweep on its own ROWMAJOR records
    (layout ROWMAJOR_TILE, padded inside the kernel) — VERDICT r3 #8.  Against the generic pivoting sweep of the same library
    on the same records: gains per step <= 2e-6; whole solves take the same decisions."""
    import torch
    import quattro_ilqr_amd as q
    from quattro_ilqr_amd import _lib, ops
    md = planar_model(integrator)
    assert ops.model_layout(md) == _lib.LAYOUT_ROWMAJOR_TILE
    B, N = 301, 50
    x0, u0 = planar_batch(B, N, 17)
    x0t, u0t = torch.as_tensor(x0, dtype=torch.float32, device="cuda:0"), torch.as_tensor(u0, dtype=torch.float32, device="cuda:0")
    x, _ = ops.simulate(md, x0t, u0t)
    rec, VxN, VxxN, lay = ops.linearize(md, x, u0t)
    lib = _lib.load_for(md)
    Kt, kt, st = ops.riccati_sweep(rec, VxN, VxxN, 6, 2, _lib.LAYOUT_ROWMAJOR_TILE, lib=lib)
    Kg, kg, sg = ops.riccati_sweep(rec.reshape(B, N, -1), VxN, VxxN, 6, 2, _lib.LAYOUT_ROWMAJOR, lib=lib)
    assert int(st.abs().sum()) == 0 and int(sg.abs().sum()) == 0
    num = (Kt.double() - Kg.double()).flatten(2).norm(dim=2)
    eK = float((num / Kg.double().flatten(2).norm(dim=2)).max())
    # (k passes through zero along a trajectory: relative to the step's norm, floored at 1 % of the largest)
    ek = float(((kt.double() - kg.double()).norm(dim=2) / kg.double().norm(dim=2).clamp_min(1e-2 * float(kg.double().norm(dim=2).max()))).max())
    print(f"planar/{integrator}: tile sweep vs generic sweep on the same records: per-step K {eK:.2e} k {ek:.2e}")
    assert eK < 2e-6 and ek < 2e-5


def test_user_model_of_the_quadrotors_shape_one_sweep_in_all_three_paths():
    """a user model with (n, m) = (12, 4) — the quadrotor typed in again — used to linearise into TILE16 records for
    the host-driven path while its persistent kernel ran the generic sweep on ROWMAJOR records.  Now quattro_model_layout says
    ROWMAJOR_TILE for it and the host-driven loop, the one-call iteration and the persistent kernel run the SAME sweep body on the
    same records: bit for bit."""
    import torch
    import quattro_ilqr_amd as q
    from quattro_ilqr_amd import _lib, ops
    from bench import synthetic_batch
    builtin = q.quadrotor_model()
    user = q.compile_model("quadrotor_user", 12, 4, rate=QUAD_RATE, dt=builtin.dt, integrator="euler", phys=builtin.phys,
                           q=builtin.q, r=builtin.r, qf=builtin.qf, x_ref=builtin.x_ref,
                           barrier_alpha=builtin.barrier_alpha, barrier_beta=builtin.barrier_beta)
    assert ops.model_layout(user) == _lib.LAYOUT_ROWMAJOR_TILE
    B, N = 33, 50
    x0, u0 = synthetic_batch(B, 0)
    dev = q.QuattroILQR(user, N, max_iter=6, device="cuda:0", device_loop="always")
    host = q.QuattroILQR(user, N, max_iter=6, device="cuda:0", device_loop=False, check_every=1)
    od = {k: v.clone() for k, v in dev.solve(x0, u0).items()}
    oh = host.solve(x0, u0)
    for key in ("K", "k", "x", "u", "cost", "iters", "alpha", "status"):
        assert torch.equal(od[key], oh[key]), key
    assert int(od["iters"].max()) >= 2


# ---------------------------------------------------------------------------------------------- planar + slack on the GPU
def _slack_sweeps(md, x, u):
    """At the device nominal (x, u): the raw tile sweep (ROWMAJOR_TILE: flags, never repairs) and the library's generic pivoting
    sweep (ROWMAJOR) on the same records."""
    from quattro_ilqr_amd import _lib, ops
    B, N = u.shape[0], u.shape[1]
    lib = _lib.load_for(md)
    rec, VxN, VxxN, lay = ops.linearize(md, x, u)
    assert lay == _lib.LAYOUT_ROWMAJOR_TILE
    Kt, kt, st = ops.riccati_sweep(rec, VxN, VxxN, 6, 3, _lib.LAYOUT_ROWMAJOR_TILE, lib=lib)
    Kg, kg, sg = ops.riccati_sweep(rec.reshape(B, N, -1), VxN, VxxN, 6, 3, _lib.LAYOUT_ROWMAJOR, lib=lib)
    assert int(sg.abs().sum()) == 0
    return dict(Kt=Kt.cpu().numpy(), kt=kt.cpu().numpy(), st=st.cpu().numpy(), Kg=Kg.cpu().numpy(), kg=kg.cpu().numpy())


def _slack_nominal(md, x0, u0):
    import torch
    from quattro_ilqr_amd import ops
    x0t = torch.as_tensor(x0, dtype=torch.float32, device="cuda:0")
    u0t = torch.as_tensor(u0, dtype=torch.float32, device="cuda:0")
    x, _ = ops.simulate(md, x0t, u0t)
    return x, u0t


def _slack_check(what, K, k, status, sw, ref, flagged, rows=None, tol=1e-5):
    """Gains handed back by an entry point (K (B, N, 3, 6), k (B, N, 3), status (B,) or None) against the fp64 oracle on exact
    derivatives (ref = (k, K) of trajectories `rows`), the generic sweep (flagged trajectories, bit for bit) and the raw tile sweep
    (the others, bit for bit).  -> worst per-step errors (K, k)."""
    from quattro_ilqr_amd import _lib
    from conftest import per_step_rel, per_step_rel_floor
    K, k = np.asarray(K, dtype=np.float32), np.asarray(k, dtype=np.float32)
    B = K.shape[0]
    if status is not None:
        assert not np.any(np.asarray(status) & (_lib.TRAJ_ILLCOND | _lib.TRAJ_SINGULAR)), (what, status)
    for b in range(B):
        want = (sw["Kg"][b], sw["kg"][b]) if flagged[b] else (sw["Kt"][b], sw["kt"][b])
        assert np.array_equal(K[b], want[0]) and np.array_equal(k[b], want[1]), (what, b, bool(flagged[b]))
    eK = ek = 0.0
    rows = range(B) if rows is None else rows
    for i, b in enumerate(rows):
        eK = max(eK, per_step_rel(K[b], ref[1][i]))
        ek = max(ek, per_step_rel_floor(k[b], ref[0][i]))
    print(f"  {what}: per-step K {eK:.2e} k {ek:.2e} vs the fp64 oracle ({int(np.sum(flagged))} of {B} trajectories flagged)")
    assert eK < tol and ek < tol, (what, eK, ek, tol)
    return eK, ek


def _slack_setup(integrator, slack, N, seed=0, ref_rows=None):
    md = slack_model(integrator)
    x0, u0 = slack_batch(slack, N, seed)
    x, ut = _slack_nominal(md, x0, u0)
    sw = _slack_sweeps(md, x, ut)
    flagged = (sw["st"] & 4) != 0
    rows = list(range(len(x0))) if ref_rows is None else ref_rows
    xs = x.double().cpu().numpy()
    k_o, K_o, _ = exact_sweep(slack_f(integrator), slack_L, slack_Lf, xs[rows], u0[rows])
    return md, x0, u0, sw, flagged, (k_o, K_o), rows


def _solver_gains(md, N, x0, u0, max_iter=1, **kw):
    import quattro_ilqr_amd as q
    s = q.QuattroILQR(md, N, max_iter=40, device="cuda:0", tf_window=0, **kw)
    out = s.solve(x0, u0, max_iter=max_iter)
    return out["K"].cpu().numpy(), out["k"].cpu().numpy(), out["status"].cpu().numpy()


SOLVER_PATHS = {"persistent": dict(device_loop="always"), "default": dict(device_loop=True),
                "host": dict(device_loop=False, check_every=1), "graph": dict(use_graph=True, device_loop=False)}


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_slack_first_sweep_every_entry_point_uses_pivoted_gains(integrator):
    """One iteration from identical nominals, a batch of flagged and clear trajectories (an indefinite Q_uu + reg I at every
    step, at one step, nowhere): every entry point of a user model hands back gains within 1e-5 of the fp64 oracle on exact
    derivatives — the generic pivoting sweep's, bit for bit, where the tile sweep flags the trajectory — and no ILLCOND bit."""
    import torch
    import quattro_ilqr_amd as q
    N = 30
    slack = np.full((6, N), SLACK_CLEAR)
    slack[0] = SLACK_FLAG; slack[2, 7] = SLACK_FLAG; slack[4] = SLACK_FLAG; slack[5, N - 1] = SLACK_FLAG
    md, x0, u0, sw, flagged, ref, _ = _slack_setup(integrator, slack, N, 21)
    # the raw tile sweep still reports exactly the trajectories with an indefinite step (so the repair below is what ran)
    assert flagged.tolist() == [True, False, True, False, True, True], sw["st"]
    print(f"slack/{integrator}: raw tile sweep vs oracle on a flagged trajectory: per-step K "
          f"{max(float(np.max(np.abs(sw['Kt'][0][t] - ref[1][0][t])) / np.linalg.norm(ref[1][0][t])) for t in range(N)):.2e}")
    for name, kw in SOLVER_PATHS.items():
        _slack_check(f"QuattroILQR[{name}]", *_solver_gains(md, N, x0, u0, **kw), sw, ref, flagged)
    # the drop-in class: optimize() (the persistent kernel, gains from its log) and backward_pass() (repair=True)
    for b in (0, 1, 2):
        ul = [u for u in u0[b]]
        il = q.iLQR_TF(md, md, md, x0[b], ul, N, dt=DT, max_iter=1, tol=1e-3, device="cuda:0")
        il.optimize(XREF)
        K_opt, k_opt = np.array(il.logs[0]["K_seq"]), np.array(il.logs[0]["k_seq"])
        k_bp, K_bp = il.backward_pass(il.simulate(ul), ul)
        K_bp, k_bp = np.array(K_bp), np.array(k_bp)
        sub = {key: v[b:b + 1] for key, v in sw.items()}
        refb = ([ref[0][b]], [ref[1][b]])
        _slack_check(f"iLQR_TF.optimize b={b}", K_opt[None], k_opt[None], None, sub, refb, flagged[b:b + 1])
        _slack_check(f"iLQR_TF.backward_pass b={b}", K_bp[None], k_bp[None], None, sub, refb, flagged[b:b + 1])
    # BatchedMPC, one control step of one iteration, from the same warm start: both of its loops
    for loop in ("always", False):
        mpc = q.BatchedMPC(md, N, max_iter=1, device="cuda:0", check_every=1)
        mpc.u_warm = torch.as_tensor(u0, dtype=torch.float32, device="cuda:0")
        mpc.run(x0, 1, device_loop=loop)
        _slack_check(f"BatchedMPC[{loop}]", mpc.solver.K.cpu().numpy(), mpc.solver.k.cpu().numpy(), mpc.solver.status.cpu().numpy(),
                     sw, ref, flagged)


@pytest.mark.parametrize("case", ["N1", "steps", "B1", "B257"])
def test_slack_sweep_edges(case):
    """Edges of the repair: N = 1 (the only step is the flagged one); the flagged step first, last or in the middle of the
    horizon; one trajectory; 257 (more than one wave of a 256-wide grid) with flagged and clear ones interleaved."""
    integrator = "rk4" if case in ("N1", "B257") else "euler"
    if case == "N1":
        N, slack, rows = 1, [[SLACK_FLAG], [SLACK_CLEAR]], None
    elif case == "steps":
        N = 30
        slack = np.full((4, N), SLACK_CLEAR)
        slack[0, 0] = slack[1, N - 1] = slack[2, N // 2] = SLACK_FLAG
        rows = None
    elif case == "B1":
        N, slack, rows = 20, [SLACK_FLAG], None
    else:
        N, rows = 12, [0, 1, 2, 127, 128, 255, 256]
        slack = np.where(np.arange(257) % 3 == 0, SLACK_FLAG, SLACK_CLEAR)
    md, x0, u0, sw, flagged, ref, rows = _slack_setup(integrator, slack, N, 5, rows)
    if case == "steps":
        assert flagged.tolist() == [True, True, True, False]
    else:
        assert flagged.tolist() == [s == SLACK_FLAG for s in np.asarray(slack).reshape(len(x0), -1)[:, 0]]
    for name in ("persistent", "host"):
        _slack_check(f"{case} QuattroILQR[{name}]", *_solver_gains(md, N, x0, u0, **SOLVER_PATHS[name]), sw, ref, flagged, rows)


def _cond_tol(quu, sw, K_o):
    """1e-5 x max(1, cond / 100) over the flagged trajectories' Q_uu + reg I; asserts that the raw tile sweep's gains of the
    flagged trajectories are not the generic sweep's (so that bit equality with the latter shows the repair)."""
    from conftest import per_step_rel
    flagged = (sw["st"] & 4) != 0
    cond = float(np.max(np.linalg.cond(quu[flagged])))
    tol = 1e-5 * max(1.0, cond / 100.0)
    raw = max(per_step_rel(sw["Kt"][b], K_o[b]) for b in np.nonzero(flagged)[0])
    print(f"  cond(Q_uu + reg I) <= {cond:.0f}: bound {tol:.1e}; the raw tile sweep is off by {raw:.2e}")
    assert not np.array_equal(sw["Kt"][flagged], sw["Kg"][flagged])
    return tol


def test_slack_flag_that_appears_after_an_accepted_iteration_and_in_a_later_mpc_step():
    """Clear starts (slack 2: positive definite) whose first accepted iteration moves the slack to ~1.3, where Q_uu + reg I is
    indefinite: the second sweep of a solve, and a later control step of an MPC run, must repair what the first did not flag.
    There the block is also nearly singular (it has just crossed from definite to indefinite), so fp32 gains can only be as
    close to the fp64 oracle as its condition number allows (the bound is 1e-5 x max(1, cond / 100)), and the unpivoted
    elimination is not much worse there: what shows that the repair ran is that the gains equal the generic sweep's bit for bit
    where the raw tile sweep's differ."""
    import torch
    import quattro_ilqr_amd as q
    integrator, N = "euler", 30
    md = slack_model(integrator)
    x0, u0 = slack_batch(np.full(3, SLACK_CLEAR), N, 8)
    x, ut = _slack_nominal(md, x0, u0)
    assert not np.any(_slack_sweeps(md, x, ut)["st"] & 4)
    one = q.QuattroILQR(md, N, device="cuda:0", device_loop="always")
    o1 = one.solve(x0, u0, max_iter=1)
    assert bool((o1["alpha"] > 0).all())                   # accepted
    x1, u1 = o1["x"].clone(), o1["u"].clone()
    sw = _slack_sweeps(md, x1, u1)
    flagged = (sw["st"] & 4) != 0
    assert flagged.all(), sw["st"]
    k_o, K_o, quu = exact_sweep(slack_f(integrator), slack_L, slack_Lf, x1.double().cpu().numpy(), u1.double().cpu().numpy())
    tol = _cond_tol(quu, sw, K_o)
    for name in ("persistent", "host", "default"):
        _slack_check(f"second iteration [{name}]", *_solver_gains(md, N, x0, u0, max_iter=2, **SOLVER_PATHS[name]), sw, (k_o, K_o),
                     flagged, tol=tol)
    # MPC: two control steps, then a third from where they left the plant and the warm start
    for loop in ("always", False):
        mpc = q.BatchedMPC(md, N, max_iter=1, device="cuda:0", check_every=1)
        mpc.u_warm = torch.as_tensor(u0, dtype=torch.float32, device="cuda:0")
        run = mpc.run(x0, 2, device_loop=loop)
        x_cur = run["x"][:, -1].contiguous()
        xn, _ = q.ops.simulate(md, x_cur, mpc.u_warm)
        sw = _slack_sweeps(md, xn, mpc.u_warm)
        flagged = (sw["st"] & 4) != 0
        assert flagged.any(), sw["st"]
        k_o, K_o, quu = exact_sweep(slack_f(integrator), slack_L, slack_Lf, xn.double().cpu().numpy(), mpc.u_warm.double().cpu().numpy())
        tol = _cond_tol(quu, sw, K_o)
        mpc.run(x_cur, 1, device_loop=loop)
        _slack_check(f"MPC control step 3 [{loop}]", mpc.solver.K.cpu().numpy(), mpc.solver.k.cpu().numpy(),
                     mpc.solver.status.cpu().numpy(), sw, (k_o, K_o), flagged, tol=tol)


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_slack_solves_match_the_reference_and_the_oracle(integrator):
    """Whole solves on the G15 starts (tests/golden/user_slack.npz: the REFERENCE's iLQR_TF on these callables) with the rules
    of test_user_model_solve_matches_the_oracle, against the reference's run and against oracle.optimize; the drop-in's
    optimize() and backward_pass() agree bit for bit on the first iteration's gains."""
    import torch
    import quattro_ilqr_amd as q
    from conftest import load_golden
    g = load_golden("user_slack.npz")
    assert float(g["c"]) == SLACK_C and float(g["w"]) == SLACK_W and np.array_equal(g["R"], SLACK_R)
    md = slack_model(integrator)
    f = slack_f(integrator)
    N, S, max_iter, tol = int(g["N"]), g["x0"].shape[0], int(g["max_iter"]), float(g["tol"])
    s = q.QuattroILQR(md, N, max_iter=max_iter, tol=tol, device="cuda:0")
    out = s.solve(torch.as_tensor(g["x0"], dtype=torch.float32), torch.as_tensor(g["u_init"], dtype=torch.float32))
    u_dev, x_dev = out["u"].double().cpu().numpy(), out["x"].double().cpu().numpy()
    it_dev, cost_dev = out["iters"].cpu().numpy(), out["cost"].cpu().numpy()
    assert not np.any(out["status"].cpu().numpy() & 6)
    for src in ("reference", "oracle"):
        same = 0
        for b in range(S):
            ul = [u for u in g["u_init"][b]]
            if src == "reference":
                key = f"{integrator}_s{b}_"
                n_it, alphas = int(g[key + "n_iter"]), list(g[key + "alpha"][:int(g[key + "n_iter"])])
                u_r, x_r = g[key + "u_final"], g[key + "x_final"]
            else:
                u_r, x_r, logs = O.optimize(f, slack_L, slack_Lf, g["x0"][b], ul, N, max_iter=max_iter, tol=tol)
                n_it, alphas = len(logs), [(-1.0 if lg["alpha"] is None else lg["alpha"]) for lg in logs]
                u_r = np.array(u_r)
            J_r = O.trajectory_cost(slack_L, slack_Lf, x_r, u_r)
            il = q.iLQR_TF(md, md, md, g["x0"][b], ul, N, dt=DT, max_iter=max_iter, tol=tol, device="cuda:0")
            il.optimize(XREF)
            a_dev = [(-1.0 if lg["alpha"] is None else lg["alpha"]) for lg in il.logs]
            assert len(il.logs) == it_dev[b]
            same += int(n_it == it_dev[b])
            ex, eu = np.max(np.abs(x_dev[b] - x_r)), np.max(np.abs(u_dev[b] - u_r))
            print(f"slack/{integrator} b={b} vs the {src}: iterations {n_it} / device {it_dev[b]}, alphas {alphas} / {a_dev}, "
                  f"cost {J_r:.6f} / {cost_dev[b]:.6f}, max|dx| {ex:.2e} max|du| {eu:.2e}")
            assert abs(n_it - it_dev[b]) <= 1
            if n_it == it_dev[b]:                        # (x: 3e-5 where the planar test has 1e-5 — measured 1.1e-5: the
                assert a_dev == [float(a) for a in alphas]   # reference's finite-difference noise through cond(Q_uu) ~ 250)
                assert abs(J_r - cost_dev[b]) < 1e-6 * abs(J_r)
                assert ex < 3e-5 and eu < 3e-5
            if src == "reference":                       # first-iteration gains: optimize() vs backward_pass(), bit for bit
                k_bp, K_bp = il.backward_pass(il.simulate(ul), ul)
                assert np.array_equal(np.array(il.logs[0]["K_seq"]), np.array(K_bp))
                assert np.array_equal(np.array(il.logs[0]["k_seq"]), np.array(k_bp))
        assert same >= S - 1
