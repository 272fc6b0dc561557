#!/usr/bin/env python3
"""Cost of the closed loop's tick: srbd_qp_srbd_rollout_f64 for 65536 robots,
N = 20, BOX_U, each from the reference's cold start, with a full plan over N + ticks - 1 stages
whose arrays repeat the model's constants (the window gather and the PLAN kernels run), and
srbd_qp_srbd_advance_f64 alone.

Prints one JSON line: wall-clock ms per rollout and per tick, the SQP iterations per tick, and
the advance's ms per call between two events on the handle's stream (--advance-calls calls
back to back).  For the per-kernel times run it under the profiler's kernel trace:
    rocprofv3 --kernel-trace --stats -d out -o rollout -- python scripts/rollout_cost.py
A first measurement, not a pass / fail line.

Usage: python scripts/rollout_cost.py [--batch 65536] [--ticks 3] [--runs 2]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402  (import_pkg, NMPC_SETTINGS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--substeps", type=int, default=1)
    ap.add_argument("--advance-calls", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    pkg = bench.import_pkg()
    capi = pkg.capi
    device = torch.device("cuda", 0)
    batch, N, T = args.batch, args.N, args.ticks
    P = N + T - 1
    p = pkg.srbd_model.SrbdParams()
    f = dict(dtype=torch.float64, device=device)
    _, _, dx0 = pkg.srbd_model.sample_trajectories(batch, N, args.seed + 7, p)
    x0_ref = np.zeros(12)
    x0_ref[8] = 1.0
    x0 = torch.from_numpy(x0_ref + dx0).to(device)
    xs0 = torch.zeros(batch, N + 1, 12, **f)
    us0 = torch.full((batch, N, 12), 100.0, **f)
    const = lambda v, n: torch.tensor(v, **f).expand(batch, n, len(v)).contiguous()
    plan = capi.Plan(x_ref=const(p.x_ref, P + 1), foot_r=const(p.foot_r, P), foot_l=const(p.foot_l, P),
                     fz_max=const((p.fmax, p.fmax), P))
    h = capi.Handle(N, 12, 12, 0, True, False, capacity=batch)

    def rollout():
        xs, us, x = xs0.clone(), us0.clone(), x0.clone()
        al = torch.ones(batch, **f)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        logs = capi.srbd_rollout(h, xs, us, x, al, T, "box_u", bench.NMPC_SETTINGS, 15, plan=plan,
                                 substeps=args.substeps, alpha_reset=1.0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, xs, us, x, logs

    rollout()  # allocates the scratch and warms up
    ms, last = [], None
    for _ in range(args.runs):
        t, *last = rollout()
        ms.append(round(t, 2))
    xs, us, x, logs = last
    it = logs[2].float()
    # the advance alone, back to back on the handle's stream (each call shifts the guess again)
    window = capi.Plan(foot_r=const(p.foot_r, N), foot_l=const(p.foot_l, N))
    ext = h.torch_stream()
    capi.srbd_advance(h, xs, us, x=x, plan=window, substeps=args.substeps)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(ext):
        e0.record()
        for _ in range(args.advance_calls):
            capi.srbd_advance(h, xs, us, x=x, plan=window, substeps=args.substeps, stream=h.stream())
        e1.record()
    torch.cuda.synchronize()
    out = {"script": "rollout_cost", "batch": batch, "N": N, "ticks": T, "substeps": args.substeps,
           "rollout_ms": ms, "ms_per_tick_min": round(min(ms) / T, 2),
           "sqp_iters_mean_per_tick": [round(float(v), 3) for v in it.mean(dim=0)],
           "sqp_iters_max_per_tick": [int(v) for v in logs[2].max(dim=0).values],
           "advance_ms_per_call": round(e0.elapsed_time(e1) / args.advance_calls, 4),
           "finite": bool(torch.isfinite(x).all())}
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()
