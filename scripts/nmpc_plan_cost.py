#!/usr/bin/env python3
"""Cost of a plan: the NMPC step of bench.py's nmpc_step_config1 (65536 robots, N = 20, each
from the reference's cold start, up to 15 SQP iterations) run once without a plan
(srbd_qp_srbd_nmpc_f64) and once with a full plan whose arrays repeat the model's constants
(srbd_qp_srbd_nmpc_plan_f64: the PLAN kernels, loading x_ref, both feet and fz_max per robot
and stage).  Both runs do the same arithmetic and end on the same bits; the difference is the
plan's loads.

Same inputs and timing (wall clock around the synchronous call, after one warm call) as
bench.py's nmpc_config1.  The two variants alternate, --runs times each.  Prints one JSON
line: ms per NMPC step for every run, the SQP iteration counts and whether the two variants'
trajectories are equal.  A first measurement, not a pass / fail line.

Usage: python scripts/nmpc_plan_cost.py [--batch 65536] [--runs 3]
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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sqp-max-loop", type=int, default=15)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    pkg = bench.import_pkg()
    capi = pkg.capi
    device = torch.device("cuda", 0)
    batch, N = args.batch, args.N
    p = pkg.srbd_model.SrbdParams()
    f = dict(dtype=torch.float64, device=device)
    _, _, dx0 = pkg.srbd_model.sample_trajectories(batch, N, args.seed + 7, p)
    x0_ref = np.zeros(12)
    x0_ref[8] = 1.0
    x0 = torch.from_numpy(x0_ref + dx0).to(device)
    xs0 = torch.zeros(batch, N + 1, 12, **f)
    us0 = torch.full((batch, N, 12), 100.0, **f)
    const = lambda v, n: torch.tensor(v, **f).expand(batch, n, len(v)).contiguous()
    plans = {"no_plan": None,
             "full_plan": capi.Plan(x_ref=const(p.x_ref, N + 1), foot_r=const(p.foot_r, N),
                                    foot_l=const(p.foot_l, N), fz_max=const((p.fmax, p.fmax), N))}
    h = capi.Handle(N, 12, 12, 0, False, False, capacity=batch)

    def step(plan):
        xs, us = xs0.clone(), us0.clone()
        al = torch.ones(batch, **f)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it, cv = capi.srbd_nmpc(h, xs, us, x0, al, "none", bench.NMPC_SETTINGS, args.sqp_max_loop,
                                plan=plan)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, xs, us, it, cv

    step(None)  # allocates the scratch and warms up
    ms = {k: [] for k in plans}
    last = {}
    for _ in range(args.runs):
        for name, plan in plans.items():
            t, *last[name] = step(plan)
            ms[name].append(round(t, 2))
    it = last["no_plan"][2]
    same = all(torch.equal(a, b) for a, b in zip(last["no_plan"], last["full_plan"]))
    plan_bytes = 8 * (12 * (N + 1) + 8 * N)
    out = {"script": "nmpc_plan_cost", "batch": batch, "N": N, "runs": args.runs, "ms": ms,
           "full_over_none_min": round(min(ms["full_plan"]) / min(ms["no_plan"]), 4),
           "sqp_iters_mean": round(float(it.float().mean()), 3), "sqp_iters_max": int(it.max()),
           "same_bits": bool(same), "plan_bytes_per_robot_per_pass": plan_bytes}
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()
