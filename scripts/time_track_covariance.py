"""Timing of ops.track_covariance: one process, warm, device events around `inner` calls that end in a synchronise,
`rounds` repetitions in which the contenders alternate.  On outputs allocated once:
    covariance_var     quattro_track_covariance_f32 with var, var_u and excess (what ops.track_covariance asks for by default)
    covariance_all     the same with cov too
    covariance_open    K = NULL, var and excess
    torch_route        the only other way to the same Sigma_t on the device: ops.linearize's records, ops.unpack_derivs, A + B K by
                       torch.baddbmm, then S sequential pairs of torch.bmm with the noise added, and var / var_u by einsum over the
                       stacked Sigma (excess is left out of it)
at quadrotor Euler and RK4 (B = 4096, N = S = 50) and cart-pole Euler (B = 1024, N = S = 50).  The nominal is the rollout of seeded
controls, the gains are those of one backward pass about it (ops.linearize_sweep), the run is ops.track from a start moved off the
nominal.  There is no pass mark.  Prints one JSON line; median (min - max) in microseconds per call; --out writes it to a file too."""
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
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--inner-torch", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from quattro_ilqr_amd import _lib, models, ops
    assert torch.cuda.is_available(), "time_track_covariance.py needs a GPU"
    dev = args.device
    N = 50
    cases = [("quadrotor euler", models.quadrotor_model(), 4096), ("quadrotor rk4", models.quadrotor_model(integrator="rk4"), 4096),
             ("cartpole euler", models.cartpole_model(), 1024)]

    def timed(forms, rounds):
        for f, _ in forms.values():                   # warm: code objects, the allocator's blocks
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(rounds):
            for k, (f, inner) in forms.items():
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
        G = 0.01 * torch.randn((B, n, n), generator=g, device=dev)
        cov0 = (1e-4 * torch.eye(n, device=dev) + G @ G.transpose(1, 2)).contiguous()
        noise = (1e-6 * torch.eye(n, device=dev)).expand(B, n, n).contiguous()
        cov = torch.empty((B, N + 1, n, n), dtype=f32, device=dev)
        var = torch.empty((B, N + 1, n), dtype=f32, device=dev)
        var_u = torch.empty((B, N, m), dtype=f32, device=dev)
        excess = torch.empty((B,), dtype=torch.float64, device=dev)
        lib, p, P = _lib.load_for(md), md.c_params(), ops._ptr
        st = ops._stream()

        def c_cov(with_K, with_cov, with_var_u):
            def call():
                ops.check(lib.quattro_track_covariance_f32(ctypes.byref(p), P(x), P(u), B, N, N, P(K) if with_K else None, None, None,
                                                           P(cov0), P(noise), _lib.SCORE_TERMINAL, P(cov) if with_cov else None, P(var),
                                                           P(var_u) if with_var_u else None, P(excess), st), "track covariance")
            return call

        sig = torch.empty((B, N + 1, n, n), dtype=f32, device=dev)

        def torch_route():
            rec, _, _, layout = ops.linearize(md, x, u)
            d = ops.unpack_derivs(rec, B, n, m, layout, lib=lib)
            Acl = torch.baddbmm(d["A"].reshape(B * N, n, n), d["B"].reshape(B * N, n, m), K.reshape(B * N, m, n)).reshape(B, N, n, n)
            sig[:, 0] = cov0
            for t in range(N):
                a = Acl[:, t]
                sig[:, t + 1] = torch.baddbmm(noise, a, torch.bmm(sig[:, t], a.transpose(1, 2)))
            v = torch.diagonal(sig, dim1=2, dim2=3)
            vu = torch.einsum("btai,btij,btaj->bta", K, sig[:, :N], K)
            return v, vu

        # the two routes agree: the kernel's Sigma against torch's, relative to sqrt(S_ii S_jj)
        c_cov(True, True, True)()
        torch_route()
        torch.cuda.synchronize()
        sd = torch.sqrt(torch.diagonal(sig, dim1=2, dim2=3)).double()
        gap = float(((cov.double() - sig.double()).abs() / (sd[..., :, None] * sd[..., None, :])).max())
        forms = {"covariance_var": (c_cov(True, False, True), args.inner), "covariance_all": (c_cov(True, True, True), args.inner),
                 "covariance_open": (c_cov(False, False, False), args.inner), "torch_route": (torch_route, args.inner_torch)}
        times = timed(forms, args.rounds)
        out[f"{name} B={B} N={N}"] = dict({k: stats(v) for k, v in times.items()}, kernel_vs_torch_cov=float(f"{gap:.2e}"))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
