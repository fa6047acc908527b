"""Timing of ops.estimate_log: one process, warm, device events around `inner` calls that end in a synchronise,
`rounds` repetitions in which the contenders alternate.  On outputs and a workspace allocated once:
    filter             quattro_estimate_log_f32 with xhat, var, nis and loglik (what ops.estimate_log asks for by default)
    filter_smoother    the same with xs and var_s (smooth=True's default): the forward and the backward kernel
    track_estimate     quattro_track_estimate_f32 with xhat, var and nis on the same shapes: the run the log was recorded from.  The
                       log filter does strictly less per step (no plant, no gain law) and one more update.  No gate
    torch_filter       the only other way to the same numbers on the device: a Python loop of S + 1 iterations, each the Kalman update
                       in torch (the batch form: one p_y x p_y solve, a handful of bmm, a logdet), ops.track of one step for the
                       estimate, one ops.linearize at (xhat, u_t) for A, and two bmm for A P A^T + W
    torch_smoother     torch_filter and the Rauch-Tung-Striebel pass: per step one torch.linalg.solve against the prior covariance and
                       four bmm
at quadrotor Euler and RK4 (B = 4096, S = 50, the six pose states observed) and cart-pole Euler (B = 1024, S = 50, the two positions).
The log is that of an ops.track_estimate run (its x plus seeded sensor noise, its u); every reading exists, so that the batch update
of the torch route applies.  The two routes must agree within GAP_BOUND and the kernel route must be faster, filter against filter
and smoother against smoother: both are asserted, after the JSON line has been printed and written.  For the comparison the torch
route's matrix algebra runs in float64 (its Rauch-Tung-Striebel pass solves against a prior covariance whose condition number fp32
does not carry to the bounds); it is TIMED in float32.  Median (min - max) in microseconds per call; --out writes the line to a file."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "quattro-transformer-ilqr_amd")]

# 4 x E of tests/log_cases.py (for xhat and xs, measured here relative to the largest entry of the component, the bound
# scripts/time_track_estimate.py holds its states to)
GAP_BOUND = dict(xhat=2.2e-4, var=2.2e-4, xs=2.2e-4, var_s=2.1e-4, loglik=5.6e-5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--inner-torch", type=int, default=2)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from quattro_ilqr_amd import _lib, models, ops
    assert torch.cuda.is_available(), "time_estimate_log.py needs a GPU"
    dev = args.device
    S = 50
    cases = [("quadrotor euler", models.quadrotor_model(), 4096, (0, 1, 2, 6, 7, 8)),
             ("quadrotor rk4", models.quadrotor_model(integrator="rk4"), 4096, (0, 1, 2, 6, 7, 8)),
             ("cartpole euler", models.cartpole_model(), 1024, (0, 2))]

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

    out, failed = {}, []
    for name, md, B, obs in cases:
        n, m, p_y = md.n, md.m, len(obs)
        f32 = torch.float32
        g = torch.Generator(device=dev).manual_seed(B + S)
        ref = torch.as_tensor(np.asarray(md.x_ref, dtype=np.float32), device=dev)
        hover = md.phys[0] * md.phys[5] / 4.0 if md.name == "quadrotor" else 0.0
        scale = 0.05 if md.name == "quadrotor" else 0.2
        x0n = (ref + scale * torch.randn((B, n), generator=g, device=dev)).contiguous()
        u_nom = (hover + 0.1 * torch.randn((B, S, m), generator=g, device=dev)).contiguous()
        x_nom, _ = ops.simulate(md, x0n, u_nom)
        K, _, _ = ops.linearize_sweep(md, x_nom, u_nom)[:3]
        x0 = (x0n + 0.1 * scale * torch.randn((B, n), generator=g, device=dev)).contiguous()
        G = 0.01 * torch.randn((B, n, n), generator=g, device=dev)
        cov0 = (1e-4 * torch.eye(n, device=dev) + G @ G.transpose(1, 2)).contiguous()
        noise = (1e-6 * torch.eye(n, device=dev)).expand(B, n, n).contiguous()
        xhat0 = (x0 + 1e-2 * torch.randn((B, n), generator=g, device=dev)).contiguous()
        mv = torch.full((p_y,), 1e-4, dtype=f32, device=dev)
        v = (1e-2 * torch.randn((S + 1, B, p_y), generator=g, device=dev)).contiguous()
        d = (1e-3 * torch.randn((S, B, n), generator=g, device=dev)).contiguous()
        oi = torch.as_tensor(obs, device=dev)
        # the recorded run and its log
        run = ops.track_estimate(md, x0, x_nom, u_nom, K, S, obs, mv, xhat0=xhat0, cov0=cov0, noise=noise, meas_noise=v[:S].contiguous(),
                                 disturbance=d, want=())
        ylog = (run["x"][:, :, oi] + v.transpose(0, 1)).contiguous()
        ulog = run["u"].contiguous()
        x = torch.empty((B, S + 1, n), dtype=f32, device=dev)
        xhat, var, xs, var_s = (torch.empty_like(x) for _ in range(4))
        nis = torch.empty((B, S + 1), dtype=f32, device=dev)
        loglik = torch.empty((B,), dtype=torch.float64, device=dev)
        tr_x, tr_xhat, tr_var = (torch.empty_like(x) for _ in range(3))
        tr_u, tr_nis = torch.empty_like(ulog), torch.empty((B, S), dtype=f32, device=dev)
        lib, p, P = _lib.load_for(md), md.c_params(), ops._ptr
        st = ops._stream()
        obs_c = (ctypes.c_int32 * p_y)(*obs)
        ws_bytes = int(lib.quattro_estimate_log_workspace_bytes(ctypes.byref(p), B, S, p_y, 1))
        ws = torch.empty((ws_bytes // 4,), dtype=f32, device=dev)

        def c_log(smooth):
            def call():
                ops.check(lib.quattro_estimate_log_f32(ctypes.byref(p), P(ylog), 1, P(ulog), 1, B, S, obs_c, p_y, P(mv), 0, P(xhat0),
                                                       P(cov0), P(noise), None, P(ws), ws_bytes, P(xhat), P(var), None, None, None,
                                                       P(nis), P(loglik), P(xs) if smooth else None, P(var_s) if smooth else None,
                                                       None, st), "estimate log")
            return call

        def c_track():
            ops.check(lib.quattro_track_estimate_f32(ctypes.byref(p), None, P(x0), P(x_nom), P(u_nom), P(K), B, S, S, obs_c, p_y, P(mv),
                                                     0, P(xhat0), P(cov0), P(noise), P(v), P(d), None, None, P(tr_x), P(tr_u),
                                                     P(tr_xhat), P(tr_var), None, P(tr_nis), st), "track estimate")

        z_x, z_K = torch.zeros((B, 2, n), device=dev), torch.zeros((B, 1, m, n), device=dev)
        res_t = {}

        def torch_route(smooth, dt):
            Rm = torch.diag(mv).to(dt).expand(B, p_y, p_y)
            W = noise.to(dt)
            xh, Pm = xhat0.to(dt), cov0.to(dt)
            xhs, Ps, Pbs, xbs, As = [], [], [None], [None], []
            ll = torch.zeros((B,), dtype=dt, device=dev)
            for t in range(S + 1):
                PH = Pm[:, :, oi]                                                # P H^T
                Sm = PH[:, oi, :] + Rm
                e = (ylog[:, t].to(dt) - xh[:, oi]).unsqueeze(2)
                sol = torch.linalg.solve(Sm, torch.cat([PH.transpose(1, 2), e], dim=2))      # S^-1 [H P | e]
                xh = xh + torch.bmm(PH, sol[:, :, n:]).squeeze(2)
                ll = ll - 0.5 * (p_y * math.log(2.0 * math.pi) + torch.logdet(Sm) + (e * sol[:, :, n:]).sum(dim=(1, 2)))
                Pm = Pm - torch.bmm(PH, sol[:, :, :n])
                xhs.append(xh)
                Ps.append(Pm)
                if t < S:
                    ut = ulog[:, t:t + 1].contiguous()
                    x32 = xh.to(f32).contiguous()
                    xhn, _ = ops.track(md, x32, z_x, ut, z_K, 1, feedback=False)
                    rec, _, _, layout = ops.linearize(md, torch.stack([x32, xhn[:, 1]], dim=1).contiguous(), ut)
                    A = ops.unpack_derivs(rec, B, n, m, layout, lib=lib)["A"].reshape(B, n, n).to(dt)
                    Pm = torch.baddbmm(W, A, torch.bmm(Pm, A.transpose(1, 2)))
                    xh = xhn[:, 1].to(dt)
                    As.append(A)
                    Pbs.append(Pm)
                    xbs.append(xh)
            res_t.update(xhat=torch.stack(xhs, dim=1), var=torch.stack([torch.diagonal(q, dim1=1, dim2=2) for q in Ps], dim=1), loglik=ll)
            if smooth:
                sx, sP = xhs[S], Ps[S]
                sxs, svs = [sx], [torch.diagonal(sP, dim1=1, dim2=2)]
                for t in range(S - 1, -1, -1):
                    C = torch.linalg.solve(Pbs[t + 1], torch.bmm(As[t], Ps[t])).transpose(1, 2)
                    sx = xhs[t] + torch.bmm(C, (sx - xbs[t + 1]).unsqueeze(2)).squeeze(2)
                    sP = Ps[t] + torch.bmm(C, torch.bmm(sP - Pbs[t + 1], C.transpose(1, 2)))
                    sxs.append(sx)
                    svs.append(torch.diagonal(sP, dim1=1, dim2=2))
                res_t.update(xs=torch.stack(sxs[::-1], dim=1), var_s=torch.stack(svs[::-1], dim=1))

        # the two routes agree
        c_log(True)()
        torch_route(True, torch.float64)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(xs).all()) and bool(torch.isfinite(res_t["xs"]).all())
        comp = lambda a, b: float(((a - b).abs().amax(dim=(0, 1)) / b.abs().amax(dim=(0, 1))).max())
        rel = lambda a, b: float(((a - b).abs() / b.abs()).max())
        gap = dict(xhat=comp(xhat.double(), res_t["xhat"]), var=rel(var.double(), res_t["var"]), xs=comp(xs.double(), res_t["xs"]),
                   var_s=rel(var_s.double(), res_t["var_s"]), loglik=rel(loglik, res_t["loglik"]))
        forms = {"filter": (c_log(False), args.inner), "filter_smoother": (c_log(True), args.inner), "track_estimate": (c_track, args.inner),
                 "torch_filter": (lambda: torch_route(False, f32), args.inner_torch),
                 "torch_smoother": (lambda: torch_route(True, f32), args.inner_torch)}
        times = timed(forms, args.rounds)
        res = {k: stats(t) for k, t in times.items()}
        r_f = res["torch_filter"]["median_us"] / res["filter"]["median_us"]
        r_s = res["torch_smoother"]["median_us"] / res["filter_smoother"]["median_us"]
        out[f"{name} B={B} S={S} p_y={p_y}"] = dict(res, torch_over_kernel_filter=round(r_f, 1), torch_over_kernel_smoother=round(r_s, 1),
                                                  filter_over_track_estimate=round(res["filter"]["median_us"] / res["track_estimate"]["median_us"], 3),
                                                  kernel_vs_torch={k: float(f"{e:.2e}") for k, e in gap.items()})
        failed += [(name, k, e) for k, e in gap.items() if not e < GAP_BOUND[k]]
        failed += [(name, k, r) for k, r in (("filter", r_f), ("smoother", r_s)) if not r > 1.0]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    assert not failed, failed


if __name__ == "__main__":
    main()
