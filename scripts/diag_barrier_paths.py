"""Which path do the barrier short cuts take on the benchmark's batch?  CPU only: the fp64 oracle and the device's rules.

For the benchmark's synthetic batch (bench.synthetic_batch, seed 1234; quadrotor, N = 50) and one iteration from its nominal
(analytic derivatives, the fp64 sweep, the six closed-loop rollouts of ops.ALPHAS) this prints

  * the share of line-search wave-steps on the barrier slow path of lane_stage_cost (rollout_quad_body.h): a wave holds the
    six candidates of two consecutive trajectories, 48 control lanes, and takes the short cut only when EVERY one of them has
    beta u > 20 and a barrier bound below half an ulp of its lane's cost -- with every candidate counted (what the kernel did),
    and with the dead candidates left out of the vote;
  * the share of candidate-steps that are dead: the running cost has passed J0 before the step, so the candidate can no longer
    be accepted (every term of the cost is >= 0);
  * the share of refill batches of the fused sweep (25 steps of one trajectory, the nominal's controls) in which
    qt_barrier_derivs_negligible (models_device.h) holds for every control, so that the derivative short cut is taken;
  * the largest |Euler angle| any candidate reaches (qt_sincos_chain's short cut wants <= 0.78).

usage: python scripts/diag_barrier_paths.py [--pairs 128]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402

from bench import HORIZON, synthetic_batch  # noqa: E402
from oracle import ilqr as o_ilqr  # noqa: E402
from oracle import linearize as o_lin  # noqa: E402
from oracle import models as o_models  # noqa: E402

ALPHAS = (1.0, 0.5, 0.25, 0.1, 0.05, 0.01)          # quattro_ilqr_amd.ops.ALPHAS
FUSED_BATCH = 25                                     # sweep_tile16_body.h
f32 = np.float32


def lane_costs(spec, x, u):
    """c of lane_stage_cost before the barrier, per control lane j: the lane's four state terms (axis j; none on lane 3) plus
    r_j u_j^2.  x (..., 12), u (..., 4) -> (..., 4)"""
    q = np.diag(spec.Q)
    d = x - spec.x_ref
    c = np.diag(spec.R) * u * u
    for j in range(3):
        c[..., j] += sum(q[3 * g + j] * d[..., 3 * g + j] ** 2 for g in range(4))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128, help="wave pairs = pairs of consecutive trajectories")
    a = ap.parse_args()
    B, N = 2 * a.pairs, HORIZON
    spec = o_models.quadrotor_spec()
    al, be = spec.barrier_alpha, spec.barrier_beta
    x0, u0 = synthetic_batch(B, 0)
    x0 = x0.astype(f32).astype(np.float64)
    u0 = u0.astype(f32).astype(np.float64)
    xs, J0 = o_lin.rollout_batched(spec, x0, u0)
    k, K = o_ilqr.riccati_sweep_batched(o_lin.linearize_analytic(spec, xs, u0))
    slow = np.zeros((len(ALPHAS), B, N), dtype=bool)        # this candidate's lanes veto the short cut at step t
    dead = np.zeros((len(ALPHAS), B, N), dtype=bool)
    amax = 0.0
    for i, alpha in enumerate(ALPHAS):
        nx, nu, _ = o_lin.closed_loop_rollout_batched(spec, x0, xs, u0, k, K, alpha)
        big = be * nu > 20.0
        tiny = (f32(abs(al)) * f32(4.25e-18) / f32(be) ** 2) < lane_costs(spec, nx[:, :-1], nu).astype(f32) * f32(2.9e-8)
        slow[i] = ~(big & tiny).all(axis=-1)
        run = np.cumsum(o_lin.stage_cost(spec, nx[:, :-1], nu), axis=1)
        dead[i, :, 1:] = run[:, :-1] > J0[:, None]
        amax = max(amax, float(np.abs(nx[:, :, 6:9]).max()))
    wave = lambda m: m.reshape(len(ALPHAS), B // 2, 2, N).any(axis=(0, 2))     # noqa: E731  (candidates x 2 trajectories)
    all_cnt, live_cnt = wave(slow), wave(slow & ~dead)
    # refill batches: the device's predicate in fp32 on the nominal's controls
    r = np.diag(spec.R).astype(f32)
    u = u0.astype(f32)
    z = f32(be) * u
    e40 = f32(abs(al)) * f32(4.25e-18)
    neg = (z > 20) & (z <= np.finfo(f32).max) & (f32(2) * e40 / f32(abs(be)) < np.abs(f32(2) * r * u) * f32(2.9e-8)) & \
          (f32(4) * e40 < np.abs(f32(2) * r) * f32(2.9e-8))
    batches = [neg[:, b0:b0 + FUSED_BATCH].all(axis=(1, 2)) for b0 in range(0, N, FUSED_BATCH)]
    taken = np.concatenate(batches)
    print(f"quadrotor, N = {N}, {B // 2} wave pairs ({B} trajectories), alphas {ALPHAS}")
    print(f"line search, barrier slow path: {all_cnt.mean():.3f} of {all_cnt.size} wave-steps "
          f"({live_cnt.mean():.3f} with dead candidates out of the vote)")
    print(f"dead candidate-steps: {dead.mean():.3f} of {dead.size}; dead at step 1 by alpha: "
          + " ".join(f"{ALPHAS[i]:g}: {dead[i, :, 1].mean():.2f}" for i in range(len(ALPHAS))))
    print(f"refill batches with the derivative short cut: {taken.mean():.3f} of {taken.size} "
          f"(nominal beta u in [{z.min():.1f}, {z.max():.1f}])")
    print(f"largest |Euler angle| over all candidates: {amax:.3f}")


if __name__ == "__main__":
    main()
