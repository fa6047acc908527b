"""Timing of the closed loop: the default forms (regression check against another build of the library) and the plant /
gain-feedback forms (recorded, no target).  Quadrotor, B = 4096, N = 50, host clock around work that ends in a synchronise.

  time_closed_loop.py                                   one process, the shipped library: every figure below, one JSON line
  time_closed_loop.py --ab OLD.so [--rounds 5]          regression check on ONE box: alternates OLD.so (e.g. the parent commit's
                                                        build, under build_ab/; it must export the phys entries ops calls) and the
                                                        shipped library, `rounds` child processes each (the QUATTRO_HIP_LIB
                                                        mechanism of scripts/ab_lib.sh), default forms only.  Prints both medians
                                                        and the older build's own spread, and FAILS (exit status 1) if the two
                                                        builds do not compute the same bits, or if a median of the shipped library
                                                        lies above the maximum of the older build's own rounds.

Default forms: BatchedMPC.run of 10 control steps (the README's 5.4 ms) and a converged QuattroILQR.solve (its 2.4 ms); for the
cart-pole the same two at BASELINE configs[1]'s shape (Euler, B = 1024, N = 50).  Bits: a SHA-256 per model and integrator over
a converged solve (K, k, cost, alpha_idx, status) and 3 control steps with a seeded disturbance after it (x, u, iters of the run
and K, k, cost, alpha_idx, status of the solver), quadrotor B = 5, N = 26, cart-pole B = 9, N = 30.
New forms: 50 plant steps with replan_every = 1 and with replan_every = 5 + feedback + per-controller plants; ops.track of 5 steps;
the converged solve and the 10 control steps with per-trajectory model parameters (model_phys: every parameter of every
trajectory within 12 % of the model's) next to the same calls without, and with neutral rows (the PHYS kernels on the default
problem: same work, same iteration counts); the same two calls with reference rows (targets: neutral rows -- the REF kernels on
the default problem -- and a reference that moves 2 cm per step along a per-trajectory heading, with preview over the horizon:
other work, reported with its iterations per trajectory); and, for the cart-pole (the quadrotor's kernel takes no cost rows), the
same two calls with per-trajectory cost weights (weights: no rows, neutral rows -- the COST kernel on the default problem -- and
heterogeneous rows, every component of q, qf and r of every trajectory scaled by a log-uniform factor in [0.4, 2.5]: other work,
reported with its iterations per trajectory).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "quattro-transformer-ilqr_amd")]


def output_hashes(dev):
    """-> {"quadrotor/euler": sha256, ...}: what a build computes on a small fixed problem per model and integrator."""
    import hashlib

    import numpy as np
    import torch
    from quattro_ilqr_amd import BatchedMPC, models
    out = {}
    for model, B, N in (("quadrotor", 5, 26), ("cartpole", 9, 30)):
        for integ in ("euler", "rk4"):
            md = models.model_by_name(model, dt=0.01, integrator=integ)
            rng = np.random.default_rng(B + N + (integ == "rk4"))
            if model == "quadrotor":
                x0 = np.asarray(md.x_ref) + rng.uniform(-1, 1, (B, 12)) * np.array([0.5, 0.5, 0.01, 0, 0, 0, 0.2, 0.2, 0.5, 0, 0, 0])
            else:
                x0 = np.zeros((B, 4))
                x0[:, 0], x0[:, 2] = rng.uniform(-0.5, 0.5, B), rng.uniform(-0.5, 0.5, B)
            x0 = x0.astype(np.float32)
            dist = torch.as_tensor(1e-3 * rng.standard_normal((3, B, md.n)), dtype=torch.float32, device=dev)
            mpc = BatchedMPC(md, N, max_iter=100, tol=1e-3, device=dev)
            sv = mpc.solver
            h = hashlib.sha256()
            solved = sv.solve(x0)
            for t in [solved[k_] for k_ in ("K", "k", "cost", "status")] + [sv.alpha_idx]:
                h.update(t.cpu().numpy().tobytes())
            ran = mpc.run(x0, 3, disturbance=dist)
            for t in [ran[k_] for k_ in ("x", "u", "iters")] + [sv.K, sv.k, sv.cost, sv.alpha_idx, sv.status]:
                h.update(t.cpu().numpy().tobytes())
            out[f"{model}/{integ}"] = h.hexdigest()
    return out


def measure(defaults_only):
    import numpy as np
    import torch
    from quattro_ilqr_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    new_abi = hasattr(raw, "quattro_mpc_run_plant_f32")
    phys_abi = hasattr(raw, "quattro_mpc_run_phys_f32")
    ref_abi = hasattr(raw, "quattro_mpc_run_ref_f32")
    cost_abi = hasattr(raw, "quattro_mpc_run_cost_f32")
    # an older build of the library: bind what it has (the default forms need nothing newer)
    for name in ("quattro_track_f32", "quattro_mpc_run_plant_f32", "quattro_ilqr_solve_phys_f32", "quattro_mpc_run_phys_f32",
                 "quattro_ilqr_solve_ref_f32", "quattro_mpc_run_ref_f32", "quattro_ilqr_solve_cost_f32", "quattro_mpc_run_cost_f32"):
        if not hasattr(raw, name):
            _lib.SIGNATURES.pop(name, None)
    from quattro_ilqr_amd import BatchedMPC, QuattroILQR, cartpole_model, ops, quadrotor_model
    import bench
    dev, B, N = "cuda:0", 4096, 50
    md = quadrotor_model(dt=0.01, integrator="euler")
    x0h, _ = bench.synthetic_batch(B, 0)
    x0 = torch.as_tensor(x0h, dtype=torch.float32, device=dev)

    def timed(fn, reps=7):
        fn(); fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts))

    out = {"lib": os.path.basename(_lib.LIB_PATH), "new_abi": new_abi, "phys_abi": phys_abi, "ref_abi": ref_abi, "cost_abi": cost_abi}
    mpc = BatchedMPC(md, N, max_iter=100, tol=1e-3, device=dev)

    def run(steps, **kw):
        mpc.u_warm = None
        return mpc.run(x0, steps, **kw)

    sv = QuattroILQR(md, N, max_iter=100, tol=1e-3, device=dev)
    for _ in range(10):
        sv.solve(x0, max_iter=20, fixed_iters=True)                  # clocks
    out["solve_default_ms"] = timed(lambda: sv.solve(x0, max_iter=100))
    out["mpc_run_default_10_steps_ms"] = timed(lambda: run(10))
    # the cart-pole's default forms at BASELINE configs[1]'s shape, as bench.py sets that problem up
    cp = cartpole_model(dt=0.01, integrator="euler")
    cx0 = torch.as_tensor(bench.synthetic_cartpole(1024, 0)[0], dtype=torch.float32, device=dev)
    cp_sv = QuattroILQR(cp, 50, max_iter=100, tol=1e-1, device=dev)
    cp_mpc = BatchedMPC(cp, 50, max_iter=100, tol=1e-1, device=dev)

    def cp_run(steps):
        cp_mpc.u_warm = None
        return cp_mpc.run(cx0, steps)

    out["cartpole_solve_default_ms"] = timed(lambda: cp_sv.solve(cx0, max_iter=100))
    out["cartpole_mpc_run_default_10_steps_ms"] = timed(lambda: cp_run(10))
    if defaults_only:
        out["sha256"] = output_hashes(dev)
    if not defaults_only and new_abi:
        phys = np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1))
        phys[:, 0] *= 1.0 + 0.2 * np.sin(1.0 + np.arange(B))
        phys[:, 1] *= 1.0 + 0.2 * np.cos(np.arange(B))
        phys_t = ops.plant_phys_tensor(md, phys, B, dev)
        plant = md.with_(integrator="rk4")
        out["mpc_run_default_50_steps_ms"] = timed(lambda: run(50), reps=5)
        out["mpc_run_plant_50_steps_replan_1_ms"] = timed(lambda: run(50, plant=plant, plant_phys=phys), reps=5)
        out["mpc_run_plant_50_steps_replan_5_feedback_ms"] = timed(
            lambda: run(50, plant=plant, plant_phys=phys, replan_every=5, feedback=True), reps=5)
        out["mpc_run_plant_50_steps_replan_5_open_loop_ms"] = timed(
            lambda: run(50, plant=plant, plant_phys=phys, replan_every=5, feedback=False), reps=5)
        r = sv.solve(x0, max_iter=3, fixed_iters=True)
        xn, un, K = r["x"].clone(), r["u"].clone(), r["K"].clone()
        xs = xn[:, 0].contiguous()
        out["track_5_steps_ms"] = timed(lambda: ops.track(md, xs, xn, un, K, 5, plant=plant, plant_phys=phys_t), reps=21)
        out["track_50_steps_ms"] = timed(lambda: ops.track(md, xs, xn, un, K, 50, plant=plant, plant_phys=phys_t), reps=21)
    if not defaults_only and phys_abi:
        base = np.asarray(md.phys, dtype=np.float64)
        b_, j_ = np.arange(B)[:, None], np.arange(base.size)[None, :]
        rows = ops.model_phys_tensor(md, (base * (1.0 + 0.12 * np.sin(1.0 + b_ + 1.7 * j_))).astype(np.float32), B, dev)
        neutral = ops.model_phys_tensor(md, np.tile(base.astype(np.float32), (B, 1)), B, dev)
        # the three forms of each call alternate, so that clocks and caches treat them alike
        for rnd in range(3):
            for tag, kw in (("shared", {}), ("neutral_rows", dict(model_phys=neutral)), ("model_phys", dict(model_phys=rows))):
                out.setdefault(f"solve_{tag}_ms", []).append(timed(lambda: sv.solve(x0, max_iter=100, **kw), reps=5))
                out.setdefault(f"mpc_run_10_steps_{tag}_ms", []).append(timed(lambda: run(10, **kw), reps=5))
                if rnd == 0:
                    out[f"solve_{tag}_mean_iters"] = float(sv.solve(x0, max_iter=100, **kw)["iters"].float().mean())
    if not defaults_only and ref_abi:
        R = 10 + N + 1
        neutral = ops.x_ref_rows_tensor(md, np.tile(np.asarray(md.x_ref, dtype=np.float32), (B, R, 1)), B, dev)
        heading = 0.7 * np.arange(B)[:, None]
        path = np.tile(np.asarray(md.x_ref, dtype=np.float64), (B, R, 1))
        path[:, :, 0] += 0.02 * np.arange(R)[None, :] * np.cos(heading)
        path[:, :, 1] += 0.02 * np.arange(R)[None, :] * np.sin(heading)
        moving = ops.x_ref_rows_tensor(md, path.astype(np.float32), B, dev)
        for rnd in range(3):
            for tag, kw in (("shared", {}), ("neutral_targets", dict(targets=neutral)), ("moving_targets", dict(targets=moving))):
                out.setdefault(f"ref_solve_{tag}_ms", []).append(timed(lambda: sv.solve(x0, max_iter=100, **kw), reps=5))
                out.setdefault(f"ref_mpc_run_10_steps_{tag}_ms", []).append(timed(lambda: run(10, **kw), reps=5))
                if rnd == 0:
                    out[f"ref_solve_{tag}_mean_iters"] = float(sv.solve(x0, max_iter=100, **kw)["iters"].float().mean())
                    out[f"ref_mpc_run_10_steps_{tag}_mean_iters"] = float(run(10, **kw)["iters"].float().mean())
        # the cart-pole at BASELINE configs[1]'s shape: the same three forms
        cR = 10 + 50 + 1
        c_neutral = ops.x_ref_rows_tensor(cp, np.tile(np.asarray(cp.x_ref, dtype=np.float32), (1024, cR, 1)), 1024, dev)
        c_path = np.tile(np.asarray(cp.x_ref, dtype=np.float64), (1024, cR, 1))
        c_path[:, :, 0] += 0.01 * np.arange(cR)[None, :] * np.cos(0.7 * np.arange(1024))[:, None]
        c_moving = ops.x_ref_rows_tensor(cp, c_path.astype(np.float32), 1024, dev)

        def cp_run_kw(steps, **kw):
            cp_mpc.u_warm = None
            return cp_mpc.run(cx0, steps, **kw)

        for rnd in range(3):
            for tag, kw in (("shared", {}), ("neutral_targets", dict(targets=c_neutral)), ("moving_targets", dict(targets=c_moving))):
                out.setdefault(f"ref_cartpole_solve_{tag}_ms", []).append(timed(lambda: cp_sv.solve(cx0, max_iter=100, **kw), reps=5))
                out.setdefault(f"ref_cartpole_mpc_run_10_steps_{tag}_ms", []).append(timed(lambda: cp_run_kw(10, **kw), reps=5))
                if rnd == 0:
                    out[f"ref_cartpole_solve_{tag}_mean_iters"] = float(cp_sv.solve(cx0, max_iter=100, **kw)["iters"].float().mean())
    if not defaults_only and cost_abi:
        def weight_rows(model, nb):
            own = np.concatenate([model.q, model.qf, model.r]).astype(np.float64)
            lo, hi = np.log(0.4), np.log(2.5)
            f = np.exp(np.random.default_rng(11).uniform(lo, hi, (nb, own.size))).astype(np.float32)
            return (ops.cost_rows_tensor(model, np.tile(own.astype(np.float32), (nb, 1)), nb, dev),
                    ops.cost_rows_tensor(model, (own[None, :] * f).astype(np.float32), nb, dev))

        # (cp_run_kw: the reference-rows block above; a library with the cost entries has the ref entries)
        w_neutral, w_het = weight_rows(cp, 1024)
        for rnd in range(3):
            for tag, kw in (("shared", {}), ("neutral_weights", dict(weights=w_neutral)), ("het_weights", dict(weights=w_het))):
                out.setdefault(f"cost_cartpole_solve_{tag}_ms", []).append(timed(lambda: cp_sv.solve(cx0, max_iter=100, **kw), reps=5))
                out.setdefault(f"cost_cartpole_mpc_run_10_steps_{tag}_ms", []).append(timed(lambda: cp_run_kw(10, **kw), reps=5))
                if rnd == 0:
                    out[f"cost_cartpole_solve_{tag}_mean_iters"] = float(cp_sv.solve(cx0, max_iter=100, **kw)["iters"].float().mean())
                    out[f"cost_cartpole_mpc_run_10_steps_{tag}_mean_iters"] = float(cp_run_kw(10, **kw)["iters"].float().mean())
    print(json.dumps(out), flush=True)


def ab(old, rounds):
    import numpy as np
    res = {"old": [], "new": []}
    for r in range(rounds):
        for tag in (("old", "new") if r % 2 == 0 else ("new", "old")):     # the order alternates: the child that runs second is ~0.4 % slower
            env = dict(os.environ)
            if tag == "old":
                env["QUATTRO_HIP_LIB"] = os.path.realpath(old)
            else:
                env.pop("QUATTRO_HIP_LIB", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--defaults-only"], env=env, capture_output=True,
                               text=True, timeout=400)
            if p.returncode != 0:
                sys.exit(f"child ({tag}, round {r}) failed with status {p.returncode}:\n{p.stderr[-2000:]}")
            d = json.loads(p.stdout.strip().splitlines()[-1])
            res[tag].append(d)
            print(f"round {r} {tag}: solve {d['solve_default_ms']:.3f} ms, run(10) {d['mpc_run_default_10_steps_ms']:.3f} ms; "
                  f"cart-pole solve {d['cartpole_solve_default_ms']:.3f} ms, run(10) {d['cartpole_mpc_run_default_10_steps_ms']:.3f} ms",
                  flush=True)
    summary = {}
    for key in ("solve_default_ms", "mpc_run_default_10_steps_ms", "cartpole_solve_default_ms", "cartpole_mpc_run_default_10_steps_ms"):
        o, n = np.array([d[key] for d in res["old"]]), np.array([d[key] for d in res["new"]])
        summary[key] = {"old_median": float(np.median(o)), "old_min": float(o.min()), "old_max": float(o.max()),
                        "new_median": float(np.median(n)), "new_min": float(n.min()), "new_max": float(n.max()),
                        "new_median_at_or_below_old_max": bool(np.median(n) <= o.max())}
    hashes = {tag: [d["sha256"] for d in res[tag]] for tag in res}
    summary["sha256"] = hashes["new"][0]
    summary["sha256_equal"] = all(h == hashes["new"][0] for tag in hashes for h in hashes[tag])
    print(json.dumps(summary), flush=True)
    if not summary["sha256_equal"]:
        sys.exit(f"the two builds compute different bits: {json.dumps(hashes)}")
    slow = [key for key, v in summary.items() if isinstance(v, dict) and not v.get("new_median_at_or_below_old_max", True)]
    if slow:
        sys.exit(f"slower than the older build's own spread allows: {slow}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", metavar="OLD.so")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--defaults-only", action="store_true")
    a = ap.parse_args()
    if a.ab:
        ab(a.ab, a.rounds)
    else:
        measure(a.defaults_only)
