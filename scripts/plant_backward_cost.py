#!/usr/bin/env python3
"""Cost of the differentiable plant: srbd_qp_srbd_plant_rollout_f64 and
srbd_qp_srbd_plant_rollout_backward_f64 for 65536 robots over T = 100 ticks, substeps 1 and 4,
with feet and a wrench given and the PLANT role set (every robot its own mass and Lbody).  The
robots stand: the state starts at the reference, the feet are under the body and carry the nominal
weight, and inputs, feet and wrench carry small noise, so that 1.5 s without a controller stay
finite (the largest rotation vector is reported: sin and cos of an absurd angle would be timed
on their slow path).

Call times, by device events around the call (the smallest of --runs after a warm-up):
  forward_ms            the open-loop rollout, one launch
  backward_ms           its adjoint, all seven outputs
  backward_robot_ms     its adjoint, mass and Lbody only
  advance_loop_ms       what there was before for the same states: on a handle of N = 1, T calls of
                        srbd_qp_srbd_advance_f64, each after us[:, 0] = u[:, t] (one wave per
                        robot with one lane integrating, T launches); the per-tick feet, wrench
                        and input slices are made contiguous outside the timed region
and the ratios backward / forward and advance loop / forward.  A measurement, not a pass / fail
line.  Written as JSON to --out (default profiles/backward/plant_backward_cost.json) and printed.

Usage: python scripts/plant_backward_cost.py [--batch 65536] [--ticks 100] [--substeps 1 4] [--runs 5]
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402  (import_pkg)


def measure(pkg, B, T, substeps, runs, seed):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    dev = torch.device("cuda", 0)
    p = sm.SrbdParams()
    g = torch.Generator(device=dev).manual_seed(seed)
    rand = lambda *shape: torch.rand(*shape, dtype=torch.float64, device=dev, generator=g)
    const = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)
    around = lambda v, spread, *shape: const(v) * (1.0 + spread * (2 * rand(*shape) - 1))
    shift = lambda v, width, *shape: const(v) + width * (2 * rand(*shape) - 1)
    # a standing robot: x near the reference, each foot carrying about half the weight.  Nothing
    # balances an open-loop plant, so the disturbances are small enough that T ticks of it stay
    # well inside the rotation vector's range (the results are checked to be finite)
    x0 = shift(p.x_ref, 0.002, B, 12)
    hold = [0.0, 0.0, 0.5 * p.mass * 9.8, 0.0, 0.0, 0.0] * 2
    u = shift(hold, 0.1, B, T, 12)
    under = [p.x_ref[6], p.x_ref[7], 0.0]  # the feet under the body: the weight has no lever
    foot_r = shift([a + b for a, b in zip(p.foot_r, under)], 0.002, B, T, 3)
    foot_l = shift([a + b for a, b in zip(p.foot_l, under)], 0.002, B, T, 3)
    wrench = 2 * rand(B, T, 6) - 1
    gx = torch.randn(B, T + 1, 12, dtype=torch.float64, device=dev, generator=g)
    plant = capi.Robots(mass=around(p.mass, 0.2, B), Lbody=around(p.Lbody, 0.2, B, 3))
    mp = capi.model_params(p)
    h = capi.Handle(4, 12, 12, capacity=B)
    h.set_robots(plant=plant)
    args = (x0, u, foot_r, foot_l, wrench, substeps, mp)
    x_traj = capi.srbd_plant_rollout(h, *args)
    every = capi.srbd_plant_rollout_backward(h, *args, x_traj=x_traj, gx=gx)
    robot = {k: every[k] for k in ("mass", "Lbody")}

    # the loop of before: a handle of N = 1, us[:, 0] = u[:, t], then the advance
    h1 = capi.Handle(1, 12, 12, capacity=B)
    h1.set_robots(plant=plant)
    xs1, us1, x1 = torch.zeros(B, 2, 12, dtype=torch.float64, device=dev), torch.zeros(B, 1, 12, dtype=torch.float64, device=dev), x0.clone()
    u_t = [u[:, t].contiguous() for t in range(T)]
    w_t = [wrench[:, t].contiguous() for t in range(T)]
    plan_t = [capi.Plan(foot_r=foot_r[:, t:t + 1].contiguous(), foot_l=foot_l[:, t:t + 1].contiguous()) for t in range(T)]

    def advance_loop():
        x1.copy_(x0)
        for t in range(T):
            us1[:, 0] = u_t[t]
            capi.srbd_advance(h1, xs1, us1, x=x1, plan=plan_t[t], wrench=w_t[t], substeps=substeps, params=mp)

    def timed(fn):
        ms = []
        for _ in range(1 + runs):  # the first run warms up
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        return round(min(ms[1:]), 3)

    res = {"forward_ms": timed(lambda: capi.srbd_plant_rollout(h, *args, out=x_traj)),
           "backward_ms": timed(lambda: capi.srbd_plant_rollout_backward(h, *args, x_traj=x_traj, gx=gx, out=every)),
           "backward_robot_ms": timed(lambda: capi.srbd_plant_rollout_backward(h, *args, x_traj=x_traj, gx=gx,
                                                                               want=("mass", "Lbody"), out=robot)),
           "advance_loop_ms": timed(advance_loop)}
    res["backward_over_forward"] = round(res["backward_ms"] / res["forward_ms"], 2)
    res["advance_loop_over_forward"] = round(res["advance_loop_ms"] / res["forward_ms"], 2)
    h.synchronize()
    h1.synchronize()
    res["advance_loop_max_abs_diff"] = float((x1 - x_traj[:, T]).abs().max())
    res["forward_finite"] = bool(torch.isfinite(x_traj).all())
    res["backward_finite"] = bool(all(torch.isfinite(t).all() for t in every.values()))
    res["max_rotation"] = round(float(x_traj[:, :, 0:3].norm(dim=2).max()), 3)
    h.close()
    h1.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--substeps", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--out", default=str(REPO / "profiles" / "backward" / "plant_backward_cost.json"))
    args = ap.parse_args()
    pkg = bench.import_pkg()
    out = {"script": "plant_backward_cost", "batch": args.batch, "ticks": args.ticks, "runs": args.runs}
    for s in args.substeps:
        out[f"substeps_{s}"] = measure(pkg, args.batch, args.ticks, s, args.runs, args.seed)
    text = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
