"""Timing of ops.cost_gradient: one process, warm, device events around `inner` calls that end in a synchronise,
`rounds` repetitions in which the contenders alternate:
    cost_gradient    the adjoint sweep (quattro_cost_gradient_f32): grad_u and grad_x0
    simulate         the rollout the gradient is taken about (quattro_simulate_f32)
    backward         the model's fastest backward pass: ops.linearize_sweep where ops.model_fuses_sweep says so, otherwise
                     ops.linearize + ops.riccati_sweep
at quadrotor Euler and RK4 (B = 4096, N = 50), cart-pole Euler (B = 1024, N = 50) and the planar user model (B = 4096, N = 50).
x is the rollout of u from a seeded batch of starts about the model's x_ref.  `gradient_not_slower`: in how many rounds the gradient's
time was at most the backward pass's of the same round.  Also: QuattroILQR.solve with and without want_grad=True at the quadrotor's
size (max_iter iterations, stop flags off).  Prints one JSON line; median (min - max) in microseconds per call."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "quattro-transformer-ilqr_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--solve-iters", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import numpy as np
    import torch
    from quattro_ilqr_amd import QuattroILQR, models, ops, user_model
    assert torch.cuda.is_available(), "time_cost_gradient.py needs a GPU"
    dev = args.device
    N = 50
    cases = [("quadrotor euler", models.quadrotor_model(), 4096), ("quadrotor rk4", models.quadrotor_model(integrator="rk4"), 4096),
             ("cartpole euler", models.cartpole_model(), 1024), ("planar user model", user_model.example_planar_model(), 4096)]

    def timed(forms, rounds, inner):
        for f in forms.values():                      # warm: code objects, the allocator's blocks
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(rounds):
            for k, f in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(inner):
                    f()
                b.record()
                torch.cuda.synchronize()
                times[k].append(1e3 * a.elapsed_time(b) / inner)
        return times

    def stats(v):
        return dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))

    out = {}
    for name, md, B in cases:
        n, m = md.n, md.m
        g = torch.Generator(device=dev).manual_seed(B + N)
        ref = torch.as_tensor(np.asarray(md.x_ref, dtype=np.float32), device=dev)
        hover = md.phys[0] * md.phys[5] / 4.0 if md.name == "quadrotor" else 0.0
        scale = 0.05 if md.name == "quadrotor" else 0.2
        x0 = (ref + scale * torch.randn((B, n), generator=g, device=dev)).contiguous()
        u = (hover + 0.1 * torch.randn((B, N, m), generator=g, device=dev)).contiguous()
        x, _ = ops.simulate(md, x0, u)
        layout = ops.model_layout(md)

        def backward():
            if ops.model_fuses_sweep(md):
                return ops.linearize_sweep(md, x, u)
            rec, VxN, VxxN, lay = ops.linearize(md, x, u, layout=layout)
            return ops.riccati_sweep(rec, VxN, VxxN, n, m, lay, lib=ops._lib.load_for(md))

        forms = {"cost_gradient": lambda: ops.cost_gradient(md, x, u), "simulate": lambda: ops.simulate(md, x0, u),
                 "backward": backward}
        times = timed(forms, args.rounds, args.inner)
        wins = sum(1 for a, b in zip(times["cost_gradient"], times["backward"]) if a <= b)
        out[f"{name} B={B} N={N}"] = dict(fused_backward=bool(ops.model_fuses_sweep(md)), gradient_not_slower=f"{wins}/{args.rounds}",
                                          **{k: stats(v) for k, v in times.items()})
    # the extra cost of want_grad in a solve
    md, B = models.quadrotor_model(), 4096
    rng = np.random.default_rng(0)
    x0 = (np.asarray(md.x_ref) + 0.05 * rng.standard_normal((B, md.n))).astype(np.float32)
    u0 = (md.phys[0] * md.phys[5] / 4.0 + 0.1 * rng.standard_normal((B, N, md.m))).astype(np.float32)
    solver = QuattroILQR(md, N, device=dev, tf_window=0)
    x0d, u0d = torch.as_tensor(x0, device=dev), torch.as_tensor(u0, device=dev)
    forms = {"solve": lambda: solver.solve(x0d, u0d, max_iter=args.solve_iters, fixed_iters=True),
             "solve_want_grad": lambda: solver.solve(x0d, u0d, max_iter=args.solve_iters, fixed_iters=True, want_grad=True)}
    times = timed(forms, args.rounds, args.inner)
    out[f"solve quadrotor euler B={B} N={N} iters={args.solve_iters}"] = {k: stats(v) for k, v in times.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
