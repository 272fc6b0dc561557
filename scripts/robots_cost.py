#!/usr/bin/env python3
"""Cost of per-robot parameters: the four kernels that read them --
srbd_lin_stage_kernel, srbd_lin_cost_kernel, srbd_linesearch_kernel, srbd_advance_kernel -- for
65536 robots, N = 20, BOX_U, with the set-up of scripts/rollout_cost.py (the reference's cold
start, a full plan that repeats the model's constants), with and without robots on the handle,
alternating in one process.  The robots repeat the model's constants too, so both variants do
the same work on the same values: the difference is where the constants come from.

For the per-kernel times run it under the profiler's kernel trace, in a run of its own:
    rocprofv3 --kernel-trace --stats -d out -o robots -- python scripts/robots_cost.py
(each instantiation has its own kernel name: <PLAN, ROBOT>).  The script itself prints one JSON
line with the time of each call between two events on the handle's stream, per variant: mean,
min and max over --reps calls.  --plain-only runs the variant without robots alone (a library
built from a commit before srbd_qp_srbd_set_robots_f64: SRBD_QP_LIB=...).
A first measurement, not a pass / fail line.

Usage: python scripts/robots_cost.py [--batch 65536] [--reps 10] [--plain-only]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402  (import_pkg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--plain-only", action="store_true")
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
    x = torch.from_numpy(x0_ref + dx0).to(device)
    xs0 = torch.zeros(batch, N + 1, 12, **f)
    us0 = torch.full((batch, N, 12), 100.0, **f)
    g = torch.Generator(device=device).manual_seed(args.seed + 8)
    dx = 0.05 * torch.randn(batch, N + 1, 12, generator=g, **f)
    du = 2.0 * torch.randn(batch, N, 12, generator=g, **f)
    const = lambda v, n: torch.tensor(v, **f).expand(batch, n, len(v)).contiguous()
    plan = capi.Plan(x_ref=const(p.x_ref, N + 1), foot_r=const(p.foot_r, N), foot_l=const(p.foot_l, N),
                     fz_max=const((p.fmax, p.fmax), N))
    rows = lambda v: torch.tensor(v, **f).expand(batch, *np.shape(v)).contiguous()
    variants = {"plain": None}
    if not args.plain_only:
        variants["robots"] = (capi.Robots(mass=rows(p.mass), Lbody=rows(p.Lbody), mu=rows(p.mu), Q=rows(p.Q),
                                          Qf=rows(p.Qf), R=rows(p.R)),
                              capi.Robots(mass=rows(p.mass), Lbody=rows(p.Lbody)))
    h = capi.Handle(N, 12, 12, 0, True, False, capacity=batch)
    ext = h.torch_stream()
    out_bufs = None
    times = {name: {"linearize": [], "linesearch": [], "advance": []} for name in variants}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(ext):
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    s = h.stream()
    for rep in range(args.reps + 1):  # the first round warms up
        for name, robots in variants.items():
            if robots is not None:
                h.set_robots(model=robots[0], plant=robots[1])
            elif not args.plain_only:
                h.set_robots()
            if out_bufs is None:
                out_bufs, _ = capi.srbd_linearize(h, xs0, us0, "box_u", plan=plan)
            t_lin = timed(lambda: capi.srbd_linearize(h, xs0, us0, "box_u", plan=plan, out=out_bufs, stream=s))
            xs, us, al = xs0.clone(), us0.clone(), torch.ones(batch, **f)
            t_ls = timed(lambda: capi.srbd_linesearch(h, xs, us, dx, du, al, plan=plan, stream=s))
            xs, us, xp = xs0.clone(), us0.clone(), x.clone()
            t_adv = timed(lambda: capi.srbd_advance(h, xs, us, x=xp, plan=plan, stream=s))
            if rep:
                for key, t in (("linearize", t_lin), ("linesearch", t_ls), ("advance", t_adv)):
                    times[name][key].append(t)
    stat = lambda v: {"mean_ms": round(float(np.mean(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    print(json.dumps({"script": "robots_cost", "batch": batch, "N": N, "reps": args.reps,
                      "calls": {name: {k: stat(v) for k, v in d.items()} for name, d in times.items()}}))
    h.close()


if __name__ == "__main__":
    main()
