"""Timing of ops.score against ops.total_cost: one process, warm, device events around `inner` calls that end in a
synchronise, `rounds` repetitions in which the four forms alternate:
    total_cost               one lane per trajectory, serial over steps (quattro_total_cost_f32)
    score                    no rows, terminal on: the same numbers, a wave per trajectory (quattro_score_f32)
    score, totals only       the same without the stage array
    score, targets + weights the same launch with reference rows (R = S + 1) and cost rows
at (B, S) = (4096, 50), (4096, 2000), (64, 2000) for the quadrotor and the cart-pole.  The sequences are a seeded walk about the
model's x_ref, the quadrotor's controls about hover.  Before timing, score's totals without rows are compared with
total_cost's, bit for bit, at the timed size.  Prints one JSON line; median (min - max) in microseconds per call."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "quattro-transformer-ilqr_amd")]

SHAPES = ((4096, 50), (4096, 2000), (64, 2000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import numpy as np
    import torch
    from quattro_ilqr_amd import models, ops
    assert torch.cuda.is_available(), "time_score.py needs a GPU"
    dev = args.device
    out = {}
    for name in ("quadrotor", "cartpole"):
        md = models.model_by_name(name)
        n, m = md.n, md.m
        hover = md.phys[0] * md.phys[5] / 4.0 if name == "quadrotor" else 0.0
        for B, S in SHAPES:
            g = torch.Generator(device=dev).manual_seed(B + S)
            ref = torch.as_tensor(np.asarray(md.x_ref, dtype=np.float32), device=dev)
            x = (ref + 0.3 * torch.randn((B, S + 1, n), generator=g, device=dev)).contiguous()
            u = (hover + 0.2 * torch.randn((B, S, m), generator=g, device=dev)).contiguous()
            rows = (ref + 0.05 * torch.randn((B, S + 1, n), generator=g, device=dev)).contiguous()
            w = np.tile(np.concatenate([md.q, md.qf, md.r]).astype(np.float32), (B, 1))
            w *= np.exp(np.random.default_rng(B).uniform(np.log(0.4), np.log(2.5), w.shape)).astype(np.float32)
            rows = ops.x_ref_rows_tensor(md, rows, B, dev)
            w = ops.cost_rows_tensor(md, w, B, dev)
            forms = {
                "total_cost": lambda: ops.total_cost(md, x, u),
                "score": lambda: ops.score(md, x, u, terminal=True),
                "score_totals_only": lambda: ops.score(md, x, u, terminal=True, want_stage=False),
                "score_rows": lambda: ops.score(md, x, u, targets=rows, weights=w, terminal=True),
            }
            same = bool(torch.equal(forms["total_cost"](), forms["score"]()[0]))
            for f in forms.values():                      # warm: code objects, the allocator's blocks
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k in forms}
            for _ in range(args.rounds):
                for k, f in forms.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.inner):
                        f()
                    b.record()
                    torch.cuda.synchronize()
                    times[k].append(1e3 * a.elapsed_time(b) / args.inner)
            out[f"{name} B={B} S={S}"] = dict(
                bits_equal_total_cost=same,
                **{k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
                   for k, v in times.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
