"""Timings around the tracking loss of the gain predictor, shipped quadrotor predictor shape, batch 256, on one GPU.

  python scripts/time_task_loss.py [--parent-lib build_ab/libquattro_hip_parent.so] [--rounds 3]

Every figure comes from a child process of its own (fresh runtime, fresh allocator):
  step      quattro_tf_train_step_f32 (forward + MSE + backward) through ctypes alone, so that a library built from the parent commit
            (which lacks the new entries) runs the very same child; with --parent-lib the two builds alternate, `rounds` times each, and
            the medians of this build are set beside the parent's spread
  tracking  HipTrainer.tracking_step at N = 50, beside its parts (predictor forward / unpack + track + score + gradient + pack / backward),
            the MSE step, and the same loss through training.tracking_loss under torch autograd on training.forward
Times are host clocks around windows that end in a device synchronise (20 warm-up calls, windows of 50 calls, median window).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "quattro-transformer-ilqr_amd"))
DEV = "cuda:0"
SHAPE = dict(n=12, c=52, d=128, H=4, layers=3, ff=512, NS=51, P=1, T=49)
B, N = 256, 50
WARM, CALLS, WINDOWS = 20, 50, 7


def window_ms(fn):
    import torch
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / CALLS)
    return statistics.median(out), min(out), max(out)


def child_step(lib_path):
    import torch
    from quattro_ilqr_amd import _lib, training
    lib = ctypes.CDLL(lib_path or _lib.LIB_PATH)
    P, s = ctypes.c_void_p, SHAPE
    desc = _lib.TfTrainDesc(s["n"], s["c"], s["d"], s["H"], s["layers"], s["ff"], s["NS"], s["P"], s["T"], 0.0)
    lib.quattro_tf_train_param_count.restype = ctypes.c_size_t
    lib.quattro_tf_train_workspace_bytes.restype = ctypes.c_size_t
    n_params = lib.quattro_tf_train_param_count(ctypes.byref(desc))
    ws_bytes = lib.quattro_tf_train_workspace_bytes(ctypes.byref(desc), B)
    g = torch.Generator().manual_seed(1)
    params = (0.05 * torch.randn(n_params, generator=g)).to(DEV)
    grads = torch.zeros(n_params, device=DEV)
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=DEV)
    base = (ws.data_ptr() + 255) // 256 * 256
    _, buffers = training.init_params(s["n"], s["c"], s["d"], s["H"], s["layers"], s["ff"], 110, s["T"], device=DEV)
    pe = buffers["pos_encoder.pe"][0, :s["NS"] + s["P"] + s["T"]].contiguous()
    x, u, y = (torch.randn(sh, generator=g).to(DEV) for sh in ((B, s["NS"], s["n"]), (B, s["P"], s["c"]), (B, s["T"], s["c"])))
    loss = torch.zeros(1, device=DEV)
    stream = P(torch.cuda.current_stream().cuda_stream)
    lib.quattro_tf_train_step_f32.argtypes = [ctypes.POINTER(_lib.TfTrainDesc), P, P, P, ctypes.c_size_t, P, P, P, P, ctypes.c_int,
                                              ctypes.c_uint64, ctypes.c_int, P, P, P]

    def step():
        rc = lib.quattro_tf_train_step_f32(ctypes.byref(desc), P(params.data_ptr()), P(grads.data_ptr()), P(base), ws_bytes,
                                           P(x.data_ptr()), P(u.data_ptr()), P(y.data_ptr()), P(pe.data_ptr()), B, 0, 1,
                                           P(loss.data_ptr()), None, stream)
        assert rc == 0, rc

    med, lo, hi = window_ms(step)
    print(json.dumps(dict(step_ms=med, lo=lo, hi=hi, loss=float(loss.item()), grad_norm=float(grads.double().norm()))))


def child_tracking():
    import numpy as np
    import torch
    import torch.nn.functional as F
    import quattro_ilqr_amd as q
    from quattro_ilqr_amd import ops, train_hip, training
    s = SHAPE
    md = q.quadrotor_model()
    rng = np.random.default_rng(0)
    x0 = np.asarray(md.x_ref)[None, :] + rng.uniform(-1, 1, (B, 12)) * np.array([0.5, 0.5, 0.01, 0, 0, 0, 0.2, 0.2, 0.5, 0, 0, 0])
    u0 = 2.4525 + 0.1 * rng.standard_normal((B, N, 4))
    out = q.QuattroILQR(md, horizon=N, device=DEV).solve(x0, u0, max_iter=1, want_alpha=False)
    f32 = lambda t: t.detach().float().contiguous()
    u_nom = torch.as_tensor(u0, dtype=torch.float32, device=DEV)
    x_nom, _ = ops.track(md, f32(torch.as_tensor(x0, device=DEV)), torch.zeros((B, N + 1, 12), device=DEV), u_nom,
                         torch.zeros((B, N, 4, 12), device=DEV), N, feedback=False)
    K_log, k_log = f32(out["K"]), f32(out["k"])
    rows = torch.cat([k_log[..., None], K_log], dim=-1).reshape(B, N, s["c"])
    u_mean, u_std = rows.mean(dim=(0, 1)).contiguous(), (0.1 * rows.std(dim=(0, 1)) + 1e-6).contiguous()
    task = train_hip.TrackingTask(md, x_nom, u_nom, K_log, k_log, u_mean, u_std)
    params, buffers = training.init_params(s["n"], s["c"], s["d"], s["H"], s["layers"], s["ff"], 110, s["T"], seed=0, device=DEV)
    tr = train_hip.HipTrainer(s["n"], s["c"], s["d"], s["H"], s["layers"], s["ff"], s["NS"], s["P"], s["T"], 0.0,
                              buffers["pos_encoder.pe"].cpu().numpy(), DEV)
    tr.load_state_dict({k: v.detach() for k, v in params.items()})
    g = torch.Generator().manual_seed(1)
    xn, up, y = (torch.randn(sh, generator=g).to(DEV) for sh in ((B, s["NS"], s["n"]), (B, s["P"], s["c"]), (B, s["T"], s["c"])))
    loss, div = tr.tracking_step(xn, up, task)
    res = dict(loss=float(loss), diverged=int(div.sum()))
    pred = tr.forward(xn, up)
    K, u_ff = train_hip.gains_unpack(pred, task)
    d_pred = torch.zeros_like(pred)

    def middle():
        Kk, uf = train_hip.gains_unpack(pred, task, K, u_ff)
        x, u = ops.track(md, task.x0, task.x_nom, uf, Kk, N)
        cost, _ = ops.score(md, x, u, terminal=True, want_stage=False)
        gg = ops.track_gradient(md, x, u, task.x_nom, Kk, want=("K",))
        train_hip.gains_pack_grad(gg["grad_K"], gg["grad_u_nom"], cost, task, s["T"], out=tr._task_bufs[(B, N)])

    norm = dict(u_mean=u_mean, u_std=u_std)

    def torch_chain():
        for v in params.values():
            v.grad = None
        p = training.forward(params, buffers, xn, up, s["H"])
        training.tracking_loss(md, p, norm, x_nom, u_nom, K_log, k_log).backward()

    def torch_mse():
        for v in params.values():
            v.grad = None
        F.mse_loss(training.forward(params, buffers, xn, up, s["H"]), y).backward()

    for name, fn in (("tracking_step", lambda: tr.tracking_step(xn, up, task)), ("mse_step", lambda: tr.forward_backward(xn, up, y)),
                     ("forward", lambda: tr.forward(xn, up, out=pred)), ("unpack_track_score_gradient_pack", middle),
                     ("backward", lambda: tr.backward(d_pred, xn, up)), ("torch_tracking_loss", torch_chain), ("torch_mse", torch_mse)):
        res[name + "_ms"] = window_ms(fn)
    torch_chain()
    tr.tracking_step(xn, up, task)
    res["grad_rel_diff_hip_vs_torch"] = max(float((tr.view(tr.grads, k).double() - v.grad.double()).norm() / v.grad.double().norm())
                                            for k, v in params.items())
    print(json.dumps(res))


def run_child(mode, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode] + (["--lib", lib] if lib else [])
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--lib")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.child == "step":
        return child_step(a.lib)
    if a.child == "tracking":
        return child_tracking()
    builds = [("this", None)] + ([("parent", os.path.abspath(a.parent_lib))] if a.parent_lib else [])
    rows = {name: [] for name, _ in builds}
    for _ in range(a.rounds):
        for name, lib in builds[::-1]:
            r = run_child("step", lib)
            rows[name].append(r)
            print(f"[step B={B}] {name:6s} {r['step_ms']:.3f} ms (windows {r['lo']:.3f} .. {r['hi']:.3f})  loss {r['loss']:.6f}  "
                  f"|grad| {r['grad_norm']:.6f}", flush=True)
    for name, rs in rows.items():
        ms = [r["step_ms"] for r in rs]
        print(f"[step B={B}] {name:6s} median {statistics.median(ms):.3f} ms, spread {min(ms):.3f} .. {max(ms):.3f}")
    r = run_child("tracking")
    print(f"[tracking B={B} N={N}] loss {r['loss']:.6f}, diverged {r['diverged']}, worst block |hip - torch| / |torch| of the gradient "
          f"{r['grad_rel_diff_hip_vs_torch']:.1e}")
    for k, v in r.items():
        if k.endswith("_ms"):
            print(f"[tracking B={B} N={N}] {k[:-3]:34s} {v[0]:.3f} ms (windows {v[1]:.3f} .. {v[2]:.3f})")


if __name__ == "__main__":
    main()
