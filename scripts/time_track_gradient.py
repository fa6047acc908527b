"""Timing of ops.track_gradient: one process, warm, device events around `inner` calls that end in a synchronise,
`rounds` repetitions in which the contenders alternate.  The C entries themselves on outputs allocated once:
    cost_gradient      quattro_cost_gradient_f32 on the same x, u: the open-loop adjoint sweep, the yardstick
    track_open         quattro_track_gradient_f32 with K = NULL (feedback off): the same quantities through the new kernel
    track_costate      with K, without grad_K / grad_x_nom: grad_u_nom, grad_x0 and the closed-loop costate
    track_full         with K, every output
at quadrotor Euler and RK4 (B = 4096, N = 50) and cart-pole Euler (B = 1024, N = 50), n_steps = N.  The nominal is the rollout of
seeded controls, the gains are those of one backward pass about it (ops.linearize_sweep), the run is ops.track from a start moved off
the nominal.  There is no pass mark.  Prints one JSON line; median (min - max) in microseconds per call."""
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
    args = ap.parse_args()
    import numpy as np
    import torch
    from quattro_ilqr_amd import _lib, models, ops
    assert torch.cuda.is_available(), "time_track_gradient.py needs a GPU"
    dev = args.device
    N = 50
    cases = [("quadrotor euler", models.quadrotor_model(), 4096), ("quadrotor rk4", models.quadrotor_model(integrator="rk4"), 4096),
             ("cartpole euler", models.cartpole_model(), 1024)]

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
        x0n = (ref + scale * torch.randn((B, n), generator=g, device=dev)).contiguous()
        u_nom = (hover + 0.1 * torch.randn((B, N, m), generator=g, device=dev)).contiguous()
        x_nom, _ = ops.simulate(md, x0n, u_nom)
        K, _, _ = ops.linearize_sweep(md, x_nom, u_nom)[:3]
        x0 = (x0n + 0.1 * scale * torch.randn((B, n), generator=g, device=dev)).contiguous()
        x, u = ops.track(md, x0, x_nom, u_nom, K, N)
        assert bool(torch.isfinite(x).all())
        f32 = torch.float32
        gu, gx0 = torch.empty((B, N, m), dtype=f32, device=dev), torch.empty((B, n), dtype=f32, device=dev)
        lam = torch.empty((B, N + 1, n), dtype=f32, device=dev)
        gK, gxn = torch.empty((B, N, m, n), dtype=f32, device=dev), torch.empty((B, N + 1, n), dtype=f32, device=dev)
        lib, p, P = _lib.load_for(md), md.c_params(), ops._ptr
        st = ops._stream()
        tail = (None, None, 0, None)

        def c_sweep():
            ops.check(lib.quattro_cost_gradient_f32(ctypes.byref(p), P(x), P(u), B, N, *tail, P(gu), P(gx0), P(lam), st), "sweep")

        def c_track(with_K, products):
            def call():
                ops.check(lib.quattro_track_gradient_f32(ctypes.byref(p), P(x), P(u), B, N, N, P(x_nom) if with_K else None,
                                                         P(K) if with_K else None, *tail, _lib.SCORE_TERMINAL, P(gu),
                                                         P(gK) if products else None, P(gxn) if products else None, P(gx0), P(lam),
                                                         st), "track gradient")
            return call

        forms = {"cost_gradient": c_sweep, "track_open": c_track(False, False), "track_costate": c_track(True, False),
                 "track_full": c_track(True, True)}
        times = timed(forms, args.rounds, args.inner)
        out[f"{name} B={B} N={N}"] = {k: stats(v) for k, v in times.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
