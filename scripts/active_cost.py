#!/usr/bin/env python3
"""Cost of the closed loop's tick with and without an active set:
srbd_qp_srbd_rollout_gait_f64 for 65536 robots, N = 20, BOX_U, a walking gait from perturbed
starts, a contact model with fall detection, and a downward push on half of the robots at a tick
drawn per robot, so that robots fall all over the run (the contact tests' setup scaled up).

The same rollout, from the same start, on one handle, under three settings:

  * "none":          no active set (every SQP iteration over the whole batch);
  * "skip_compact":  Active(skip_fallen=True, compact=True);
  * "compact":       Active(compact=True) alone (fallen robots are still stepped).

and, as "uniform", a batch in which every robot is the same robot and nobody is pushed, so that
all stop at the same iteration and compaction cannot gain anything: "none" against "compact"
there is what the option costs (the selection kernels and one more read-back per step).

Prints one JSON line: per setting the wall-clock ms per tick (the smallest of --runs rollouts
after a warm-up), step_work's (qp_solves, sqp_iterations) of the rollout, ms per 1000 QP solves,
and how many robots had fallen at the end.  A measurement, not a pass / fail line.

Usage: python scripts/active_cost.py [--batch 65536] [--N 20] [--ticks 20] [--runs 2]
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

PUSH, Z_MIN = 3000.0, 0.97  # N downward for one tick; the fall threshold on the body's height


def make_case(sm, p, B, N, T, seed, uniform=False):
    """Host arrays of the rollout's inputs: (xs, us, x, alpha, cmd, ref_pose, foot_now, wrench) and
    the gait's per-robot offsets.  uniform: every robot is the same robot, and nobody is pushed."""
    rng = np.random.default_rng(seed)
    xs, us, dx0 = sm.sample_trajectories(B, N, seed, p)
    x = xs[:, 0] + dx0
    xr = np.array(p.x_ref, dtype=np.float64)
    cmd = np.empty((B, T, 4))
    cmd[:, :, 0:2] = rng.uniform(-0.3, 0.3, size=(B, 1, 2))
    cmd[:, :, 2] = rng.uniform(-0.2, 0.2, size=(B, 1))
    cmd[:, :, 3] = xr[8]
    ref_pose = np.tile(np.array([xr[6], xr[7], xr[2]]), (B, 1))
    foot_now = np.empty((B, 2, 3))
    foot_now[:, 0] = xr[6:9] * np.array([1.0, 1.0, 0.0]) + np.array(p.foot_r)
    foot_now[:, 1] = xr[6:9] * np.array([1.0, 1.0, 0.0]) + np.array(p.foot_l)
    shift = np.arange(B) % 3
    offset = np.stack([shift, shift + 3], axis=1)
    wrench = np.zeros((B, T, 6))
    pushed = np.flatnonzero(rng.uniform(size=B) < 0.5)
    wrench[pushed, rng.integers(0, T, size=pushed.size), 5] = -PUSH
    arrays = [xs, us, x, np.ones(B), cmd, ref_pose, foot_now, wrench, offset]
    if uniform:  # the robot that starts highest: it stands
        wrench[:] = 0.0
        k = int(np.argmax(x[:, 8]))
        arrays = [np.ascontiguousarray(np.broadcast_to(a[k:k + 1], a.shape)) for a in arrays]
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--uniform-ticks", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    pkg = bench.import_pkg()
    capi, sm = pkg.capi, pkg.srbd_model
    device = torch.device("cuda", 0)
    B, N = args.batch, args.N
    p = sm.SrbdParams()
    dev = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
    h = capi.Handle(N, 12, 12, 0, True, False, capacity=B)
    ints = lambda: torch.zeros(B, dtype=torch.int32, device=device)
    state = [ints(), ints(), ints()]

    def measure(case, T, settings):
        xs0, us0, x0, al0, cmd, pose0, feet0, wrench, offset = case
        start = [dev(a) for a in (xs0, us0, x0, al0, pose0, feet0)]
        cmd_t, wrench_t = dev(cmd), dev(wrench)
        gait = capi.Gait(period=6, swing=(3, 3), offset=dev(offset, np.int32), hip=((0.0, -0.1), (0.0, 0.1)),
                         ground_z=0.0, k_raibert=0.03, fz_stance=250.0, fz_swing=1.0)
        h.set_contact(capi.Contact(mu=0.5, Lt=(0.0, 0.05, 0.05), fz_hi=400.0, fz_contact=125.5, z_min=Z_MIN,
                                   cos_tilt_min=0.5, fallen=state[0], alive=state[1], sat=state[2]))
        out = {}
        for name, active in settings:
            h.set_active(active)
            ms = []
            for _ in range(1 + args.runs):  # the first run allocates the scratch and warms up
                v = [a.clone() for a in start]
                for s in state:
                    s.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                logs = capi.srbd_rollout_gait(h, gait, cmd_t, *v, T, 0, "box_u", bench.NMPC_SETTINGS, 15,
                                              wrench=wrench_t, alpha_reset=1.0)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            solves, iters = h.step_work()
            best = min(ms[1:])
            out[name] = {"ms_per_tick": round(best / T, 2), "qp_solves": solves, "sqp_iterations": iters,
                         "ms_per_1000_qp_solves": round(best / solves * 1e3, 4), "fallen": int(state[0].sum()),
                         "sqp_iter_sum": int(logs[2].sum()), "finite": bool(torch.isfinite(v[2]).all())}
        h.set_active(None)
        return out

    none, compact = ("none", None), ("compact", capi.Active(compact=True))
    out = {"script": "active_cost", "batch": B, "N": N, "ticks": args.ticks, "uniform_ticks": args.uniform_ticks}
    out["pushed"] = measure(make_case(sm, p, B, N, args.ticks, args.seed + 7), args.ticks,
                            [none, ("skip_compact", capi.Active(skip_fallen=True, compact=True)), compact])
    out["uniform"] = measure(make_case(sm, p, B, N, args.uniform_ticks, args.seed + 7, uniform=True),
                             args.uniform_ticks, [none, compact])
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()
