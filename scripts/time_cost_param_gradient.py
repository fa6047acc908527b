"""Timing of the row gradients: one process, warm, device events around `inner` calls that end in a synchronise,
`rounds` repetitions in which the contenders alternate:
    cost_gradient        the adjoint sweep it sits beside (one quattro_cost_gradient_f32 call, costate output included): the yardstick
    param_gradient       ONE quattro_cost_param_gradient_f32 call, all three outputs, on a given costate
    param_gradient_phys  the same call with grad_phys alone
    param_gradient_ops   the two-launch form: ops.cost_param_gradient without a costate (the sweep, then the call above)
at quadrotor Euler and RK4 (B = 4096, N = 50), cart-pole Euler and RK4 (B = 1024, N = 50) and the user-compiled planar example
(user_model.example_planar_model(param_grad=True), Euler and RK4, B = 4096, N = 50; --only planar runs these alone), under
per-trajectory weights, targets (R = N + 1) and parameters.  x is the rollout of u from a seeded batch of starts about the model's x_ref.  `not_slower`: in how many
rounds the param_gradient's time was at most the cost_gradient's of the same round (the Euler cases are the gated ones: 6 of 7);
`phys_not_slower`: the same for param_gradient_phys (the planar model's gate).
Prints one JSON line; median (min - max) in microseconds per call."""
import argparse
import ctypes
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
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--only", default="", help="run the cases whose name starts with this")
    args = ap.parse_args()
    import numpy as np
    import torch
    from quattro_ilqr_amd import models, ops, user_model
    assert torch.cuda.is_available(), "time_cost_param_gradient.py needs a GPU"
    dev = args.device
    N = 50
    cases = [("quadrotor euler", models.quadrotor_model(), 4096), ("quadrotor rk4", models.quadrotor_model(integrator="rk4"), 4096),
             ("cartpole euler", models.cartpole_model(), 1024), ("cartpole rk4", models.cartpole_model(integrator="rk4"), 1024),
             ("planar euler", user_model.example_planar_model(integrator="euler", param_grad=True), 4096),
             ("planar rk4", user_model.example_planar_model(integrator="rk4", param_grad=True), 4096)]
    cases = [c for c in cases if c[0].startswith(args.only)]

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
        hover = md.phys[0] * md.phys[5] / 4.0 if md.name == "quadrotor" else md.phys[0] * md.phys[3] / 2.0 if name.startswith("planar") else 0.0
        scale = 0.05 if md.name == "quadrotor" else 0.2
        x0 = (ref + scale * torch.randn((B, n), generator=g, device=dev)).contiguous()
        u = (hover + 0.1 * torch.randn((B, N, m), generator=g, device=dev)).contiguous()
        x, _ = ops.simulate(md, x0, u)
        f = lambda *shape: torch.exp(0.2 * torch.randn(shape, generator=g, device=dev))
        base = np.concatenate([md.q, md.qf, md.r]).astype(np.float32)
        rows = dict(weights=ops.cost_rows_tensor(md, (torch.as_tensor(base, device=dev) * f(B, 2 * n + m)).cpu().numpy(), B, dev),
                    targets=(ref + 0.05 * torch.randn((B, N + 1, n), generator=g, device=dev)).contiguous(),
                    model_phys=ops.model_phys_tensor(md, (torch.as_tensor(np.asarray(md.phys, dtype=np.float32), device=dev)
                                                         * f(B, len(md.phys))).cpu().numpy(), B, dev))
        lam = ops.cost_gradient(md, x, u, want_costate=True, **rows)["costate"]
        # the two C entries themselves on outputs allocated once (ops.cost_param_gradient adds two small torch kernels that bring
        # its outputs into the shapes it returns: they are part of the recorded ops form, not of the gated call)
        lib, p, st = ops._lib.load_for(md), md.c_params(), ops._stream()
        P = ops._ptr
        gu, gx0, lam_out = torch.empty_like(u), torch.empty((B, n), device=dev), torch.empty_like(x)
        gp, gw, gr = (torch.empty(shape, dtype=torch.float64, device=dev) for shape in ((B, 8), (B, ops.COST_ROW_FLOATS), (B, N + 1, n)))
        tail = (P(rows["model_phys"]), P(rows["targets"]), N + 1, P(rows["weights"]))

        def c_sweep():
            ops.check(lib.quattro_cost_gradient_f32(ctypes.byref(p), P(x), P(u), B, N, *tail, P(gu), P(gx0), P(lam_out), st), "sweep")

        def c_param():
            ops.check(lib.quattro_cost_param_gradient_f32(ctypes.byref(p), P(x), P(u), B, N, P(lam), *tail, P(gp), P(gw), P(gr), st),
                      "param")

        def c_param_phys():
            ops.check(lib.quattro_cost_param_gradient_f32(ctypes.byref(p), P(x), P(u), B, N, P(lam), *tail, P(gp), None, None, st),
                      "param phys")

        forms = {"cost_gradient": c_sweep, "param_gradient": c_param, "param_gradient_phys": c_param_phys,
                 "param_gradient_ops": lambda: ops.cost_param_gradient(md, x, u, **rows)}
        times = timed(forms, args.rounds, args.inner)
        wins = sum(1 for a, b in zip(times["param_gradient"], times["cost_gradient"]) if a <= b)
        wins_phys = sum(1 for a, b in zip(times["param_gradient_phys"], times["cost_gradient"]) if a <= b)
        out[f"{name} B={B} N={N}"] = dict(not_slower=f"{wins}/{args.rounds}", phys_not_slower=f"{wins_phys}/{args.rounds}",
                                          **{k: stats(v) for k, v in times.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
