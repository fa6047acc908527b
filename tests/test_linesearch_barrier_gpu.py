"""The barrier term of the stage cost in the line-search candidates (lane_stage_cost, rollout_quad_body.h) against the other
rollouts' -- whichever of them takes the exact wave-uniform short cut and whichever does not, the bits are the same:

  * ops.linesearch commits the x, u, cost and alpha_idx of the candidate that ops.rollout's costs select (first alpha with
    J <= J0, else none and the nominal stays), bit for bit against ops.rollout's own trajectories;
  * a line search whose only alpha is 0 reproduces ops.simulate (simulate keeps the short cut);
  * with barrier_alpha = 0 the same holds.

Three control regimes, made by the feed-forward term (candidate u = u_nom + alpha (k + K dx), K small): every candidate's
controls above the short cut's threshold beta u = 20, all below it, and mixed inside one wave (alpha = 1 below, the small alphas
above).  B = 1, 2, 3 (a wave holds two trajectories), N = 1, 4, 5 (the unroll by four and its tail), 51; Euler and RK4."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BETA = 10.0


def _ops():
    from quattro_ilqr_amd import models, ops
    return models, ops


def _dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _problem(md, regime, B, N, seed):
    """x0, u_nom, K, k with the candidates' controls in the regime"""
    rng = np.random.default_rng(seed)
    x0 = np.asarray(md.x_ref) + 0.1 * rng.standard_normal((B, 12))
    centre = {"above": 26.0, "below": 12.0, "mixed": 26.0}[regime] / BETA
    u = centre + 0.05 * rng.standard_normal((B, N, 4))
    k = 0.02 * rng.standard_normal((B, N, 4))
    if regime == "mixed":
        k[..., 1] -= 1.0                                   # alpha = 1: beta u ~ 16; alpha = 0.01: ~ 25.9
        k[:, ::2, 3] -= 2.0
    K = 0.01 * rng.standard_normal((B, N, 4, 12))
    return _dev32(x0), _dev32(u), _dev32(K), _dev32(k)


def _check(md, regime, B, N, seed):
    _, ops = _ops()
    x0, u, K, k = _problem(md, regime, B, N, seed)
    xs, J0 = ops.simulate(md, x0, u)
    cand, xn, un = ops.rollout(md, xs, u, K, k, ops.ALPHAS, want_traj=True)
    cost_only = ops.rollout(md, xs, u, K, k, ops.ALPHAS)
    x_ls, u_ls, J_ls = xs.clone(), u.clone(), J0.clone()
    idx = ops.linesearch(md, x_ls, u_ls, K, k, J_ls, 1e-9)
    torch.cuda.synchronize()
    assert torch.equal(_bits(cand), _bits(cost_only)), (regime, B, N)          # ArrayStore and NoStore rollouts
    ok = (cand <= J0[None]).cpu().numpy()
    for b in range(B):
        want = int(np.argmax(ok[:, b])) if ok[:, b].any() else -1
        assert int(idx[b]) == want, (regime, B, N, b, cand[:, b], J0[b])
        wx, wu, wJ = (xs[b], u[b], J0[b]) if want < 0 else (xn[want, b], un[want, b], cand[want, b])
        assert torch.equal(_bits(x_ls[b]), _bits(wx)), (regime, B, N, b, want)
        assert torch.equal(_bits(u_ls[b]), _bits(wu)), (regime, B, N, b, want)
        assert torch.equal(_bits(J_ls[b]), _bits(wJ)), (regime, B, N, b, want)
    # alpha = 0: the nominal again, by the line search's rollout and by the all-alpha rollout
    c0, x0n, u0n = ops.rollout(md, xs, u, K, k, (0.0,), want_traj=True)
    x_z, u_z, J_z = xs.clone(), u.clone(), J0.clone()
    idz = ops.linesearch(md, x_z, u_z, K, k, J_z, 1e-9, alphas=(0.0,))
    torch.cuda.synchronize()
    assert torch.equal(_bits(c0[0]), _bits(J0)) and torch.equal(_bits(x0n[0]), _bits(xs)) and torch.equal(_bits(u0n[0]), _bits(u))
    assert bool((idz == 0).all()), idz
    assert torch.equal(_bits(J_z), _bits(J0)) and torch.equal(_bits(x_z), _bits(xs)) and torch.equal(_bits(u_z), _bits(u))
    return set(int(v) for v in idx.cpu())


@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("regime", ["above", "below", "mixed"])
def test_line_search_commits_what_the_rollouts_select(regime, integ):
    models, _ = _ops()
    md = models.quadrotor_model(integrator=integ)
    picked = set()
    for B in (1, 2, 3):
        for N in (1, 4, 5, 51):
            picked |= _check(md, regime, B, N, 1000 * N + B)
    print(f"[{regime} {integ}] accepted alpha indices {sorted(picked)}")


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_line_search_without_a_barrier(integ):
    models, _ = _ops()
    md = models.quadrotor_model(integrator=integ).with_(barrier_alpha=0.0)
    for regime in ("above", "below", "mixed"):
        for B, N in ((1, 5), (3, 51)):
            _check(md, regime, B, N, 77 * N + B)
