#!/usr/bin/env python3
"""Cost of the gait planner, for 65536 robots and N = 20:

  * srbd_qp_srbd_gait_plan_f64 alone: hip events around each launch on the handle's stream,
    after a warm-up, the median (and the smallest) of --repeats launches, with a walking gait
    (period 12, swing 5, per-robot offsets, commands with a yaw rate);
  * the closed loop's tick with a constant plan (srbd_qp_srbd_rollout_f64) against the same
    rollout replanned every tick (srbd_qp_srbd_rollout_gait_f64) with a standing gait, whose
    windows are that constant plan bit for bit, so both run the same SQP iterations: BOX_U,
    each robot from the reference's cold start, alternating, the smallest of --runs each.

With --terrain the planner alone is measured again with a terrain on the
handle, for search 0, 1 and 3, on one 256 x 256 map of random heights and on 16 such maps with
a random map per robot ("planner_terrain_us": median and smallest per case).  --planner-only
skips the ticks.  The planner without terrain also runs on a library built from an older commit
(SRBD_QP_LIB=...), for A/B runs.

Prints one JSON line.  A measurement, not a pass / fail line.

Usage: python scripts/gait_cost.py [--batch 65536] [--N 20] [--ticks 3] [--runs 2] [--repeats 50]
                                   [--terrain] [--planner-only]
"""
import argparse
import json
import statistics
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
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--terrain", action="store_true")
    ap.add_argument("--planner-only", action="store_true")
    args = ap.parse_args()
    import torch
    pkg = bench.import_pkg()
    capi = pkg.capi
    device = torch.device("cuda", 0)
    batch, N, T = args.batch, args.N, args.ticks
    P = N + T - 1
    p = pkg.srbd_model.SrbdParams()
    f = dict(dtype=torch.float64, device=device)
    rng = np.random.default_rng(args.seed)
    h = capi.Handle(N, 12, 12, 0, True, False, capacity=batch)
    xr = np.array(p.x_ref, dtype=np.float64)

    # ---- the planner alone ----
    cmd = torch.from_numpy(np.stack([rng.uniform(-0.5, 0.5, batch), rng.uniform(-0.3, 0.3, batch),
                                     rng.uniform(-1.0, 1.0, batch), np.full(batch, xr[8])], axis=1)).to(device)
    x = torch.from_numpy(xr + 0.05 * rng.normal(size=(batch, 12))).to(device)
    pose = torch.from_numpy(np.tile([xr[6], xr[7], xr[2]], (batch, 1))).to(device)
    feet = torch.from_numpy(np.tile(np.array([p.foot_r, p.foot_l], dtype=np.float64), (batch, 1, 1))).to(device)
    offset = torch.from_numpy(rng.integers(0, 12, size=(batch, 2)).astype(np.int32)).to(device)
    walk = capi.Gait(period=12, swing=(5, 5), offset=offset, k_raibert=0.03, fz_stance=250.0, fz_swing=1.0)
    ext = h.torch_stream()
    win = capi.srbd_gait_plan(h, walk, cmd, x, 0, pose, feet)
    torch.cuda.synchronize()

    def planner_us():
        times = []
        with torch.cuda.stream(ext):
            for r in range(5 + args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                capi.srbd_gait_plan(h, walk, cmd, x, r + 1, pose, feet, stream=h.stream(), out=win)
                e1.record()
                times.append((e0, e1))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) * 1e3 for a, b in times[5:]]

    us = planner_us()
    window_bytes = (12 * (N + 1) + 8 * N) * 8 * batch
    out = {"script": "gait_cost", "batch": batch, "N": N, "ticks": T,
           "planner_us_median": round(statistics.median(us), 1), "planner_us_min": round(min(us), 1),
           "window_MB": round(window_bytes / 1e6, 1),
           "planner_TBps_at_median": round(window_bytes / statistics.median(us) / 1e6, 2)}
    if args.terrain:  # 5 cm cells around the robots: the footholds fall inside the maps
        out["planner_terrain_us"] = {}
        for maps in (1, 16):
            height = torch.from_numpy(rng.uniform(0.0, 0.05, size=(maps, 256, 256))).to(device)
            map_r = torch.from_numpy(rng.integers(0, maps, size=batch).astype(np.int32)).to(device)
            for search in (0, 1, 3):
                h.set_terrain(capi.Terrain(height, xr[6] - 6.4, xr[7] - 6.4, 0.05, map_r=map_r if maps > 1 else None,
                                           search=search, w_rough=10.0))
                t = planner_us()
                out["planner_terrain_us"][f"maps{maps}_search{search}"] = [round(statistics.median(t), 1),
                                                                           round(min(t), 1)]
        h.set_terrain(None)
        t = planner_us()  # cleared again: the planner without terrain
        out["planner_cleared_us"] = [round(statistics.median(t), 1), round(min(t), 1)]
    if args.planner_only:
        print(json.dumps(out))
        h.close()
        return

    # ---- the tick, with a constant plan and replanned ----
    _, _, dx0 = pkg.srbd_model.sample_trajectories(batch, N, args.seed + 7, p)
    x0_ref = np.zeros(12)
    x0_ref[8] = 1.0
    x0 = torch.from_numpy(x0_ref + dx0).to(device)
    xs0 = torch.zeros(batch, N + 1, 12, **f)
    us0 = torch.full((batch, N, 12), 100.0, **f)
    const = lambda v, n: torch.tensor(v, **f).expand(batch, n, len(v)).contiguous()
    plan = capi.Plan(x_ref=const(p.x_ref, P + 1), foot_r=const(p.foot_r, P), foot_l=const(p.foot_l, P),
                     fz_max=const((p.fmax, p.fmax), P))
    stand = capi.Gait(period=4, swing=(0, 0), offset=(0, 2), fz_stance=p.fmax, fz_swing=1.0)
    cmd_t = torch.tensor([0.0, 0.0, 0.0, xr[8]], **f).expand(batch, T, 4).contiguous()

    def rollout(gait):
        xs, us_, xx = xs0.clone(), us0.clone(), x0.clone()
        al = torch.ones(batch, **f)
        ps, ft = pose.clone(), feet.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if gait:
            logs = capi.srbd_rollout_gait(h, stand, cmd_t, xs, us_, xx, al, ps, ft, T, 0, "box_u",
                                          bench.NMPC_SETTINGS, 15, alpha_reset=1.0)
        else:
            logs = capi.srbd_rollout(h, xs, us_, xx, al, T, "box_u", bench.NMPC_SETTINGS, 15, plan=plan,
                                     alpha_reset=1.0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, logs

    pose.copy_(torch.from_numpy(np.tile([xr[6], xr[7], xr[2]], (batch, 1))))  # the planner above moved them
    feet.copy_(torch.from_numpy(np.tile(np.array([p.foot_r, p.foot_l], dtype=np.float64), (batch, 1, 1))))
    rollout(False), rollout(True)  # allocate the scratch and warm up
    ms = {False: [], True: []}
    for _ in range(args.runs):
        for gait in (False, True):
            t, logs = rollout(gait)
            ms[gait].append(round(t, 2))
            ms[("logs", gait)] = logs
    same = all(torch.equal(a, b) for a, b in zip(ms[("logs", False)], ms[("logs", True)][:4]))
    out.update({"rollout_plan_ms": ms[False], "rollout_gait_ms": ms[True],
           "ms_per_tick_plan_min": round(min(ms[False]) / T, 2), "ms_per_tick_gait_min": round(min(ms[True]) / T, 2),
           "sqp_iters_mean_per_tick": [round(float(v), 3) for v in ms[("logs", True)][2].float().mean(dim=0)],
           "gait_rollout_equals_plan_rollout": bool(same)})
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()
