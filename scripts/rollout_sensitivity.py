#!/usr/bin/env python3
"""The inputs and the tolerance table of tests/test_gpu_rollout.py's comparison with the host
closed loop, computed on the CPU.

For each case (constraints, alpha_reset) of the test and a seed of rollout_host.walking_case,
through rollout_host.closed_loop:
  * the conditions on the inputs: the host loop's smallest comparison margin over all ticks
    (wanted >= 1e-6) and the SQP iteration counts (wanted: at least two distinct);
  * d_t: the largest change of the host loop's x_log[t] / u_log[t-1] when the loop is rerun with
    x, xs, us perturbed by relative 1e-7 (every entry times 1 +- 1e-7, random signs; the largest
    over --draws draws).  That is the largest device-host gap the step test's tolerance
    (rtol 1e-7) admits after one step, carried through the later ticks.

    python scripts/rollout_sensitivity.py --seed 30            # the table of the test's seed
    python scripts/rollout_sensitivity.py --search 20 40       # seeds that meet the conditions

With --robots the same for tests/test_gpu_robots.py's rollout: per-robot model
parameters from robots_host.draw at seed + 100, the true robots from robots_host.draw_plant at
seed + 200, two plant substeps, through the same loop with model= and plant=; and how far the
mismatch moves x_log (the same loop with plant = model).

    python scripts/rollout_sensitivity.py --robots --seed 30

With --gait the same for tests/test_gpu_gait.py's replanning rollout: the inputs
of gait_host.walking_case through the loop with gait=, which plans every tick from the
measured state, so the perturbation of x reaches the later windows through the feedback.

    python scripts/rollout_sensitivity.py --gait --seed 30

With --gait --terrain the same for tests/test_gpu_terrain.py's rollout up the stairs (DESIGN.md
4.7f): terrain_host.stairs_case through the loop with gait= and terrain= (search 1), with two more
conditions on the inputs: the smallest gap between the best and the second-best foothold cost
over every touchdown of every tick (wanted >= 1e-6 cell^2), and the chosen candidates, which like
the iteration counts must not change under the perturbation; the feet's d_t is printed too.

    python scripts/rollout_sensitivity.py --gait --terrain --seed 30
"""
import argparse
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "oracle"))

import gait_host as GH  # noqa: E402
import helpers  # noqa: E402
import robots_host as BH  # noqa: E402
import rollout_host as RH  # noqa: E402
import terrain_host as TH  # noqa: E402
from srbd_device import NMPC  # noqa: E402

CASES = [(c, a) for c in ("none", "box_u") for a in (0.0, 1.0)]
B, N, T = 4, 10, 4


ROBOTS = None  # --robots: (model list, plant list)
GAIT = False   # --gait: the inputs are gait_host.walking_case's
TERRAIN = None  # --gait --terrain: the SrbdTerrain; the inputs are terrain_host.stairs_case's


def run(sm, oracle, p, case, inputs):
    xs, us, x, alpha = inputs[:4]
    if GAIT:
        gait, cmd, ref_pose, foot_now = inputs[4:]
        features = dict(p=p, gait=gait, cmd=cmd, ref_pose=ref_pose, foot_now=foot_now, terrain=TERRAIN)
    elif ROBOTS:
        features = dict(model=ROBOTS[0], plant=ROBOTS[1], plan=inputs[4], substeps=2)
    else:
        features = dict(p=p, plan=inputs[4])
    return RH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, 15, case[0], alpha_reset=case[1], **features)


def conditions(sm, oracle, p, seed):
    if TERRAIN is not None:
        inputs = TH.stairs_case(sm, p, B, N, T, seed)
    else:
        inputs = (GH if GAIT else RH).walking_case(sm, p, B, N, T, seed)
    out = {}
    for case in CASES:
        h = run(sm, oracle, p, case, inputs)
        out[case] = (h["margin"], sorted(set(h["sqp_iter"].ravel().tolist())), h)
    return inputs, out


def main():
    global ROBOTS, GAIT, TERRAIN
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=30)
    ap.add_argument("--search", type=int, nargs=2, metavar=("FROM", "TO"))
    ap.add_argument("--draws", type=int, default=3)
    ap.add_argument("--robots", action="store_true")
    ap.add_argument("--gait", action="store_true")
    ap.add_argument("--terrain", action="store_true")
    a = ap.parse_args()
    if a.terrain and not a.gait:
        ap.error("--terrain goes with --gait")
    if a.gait and a.robots:
        ap.error("--gait and --robots are separate tables")
    GAIT = a.gait
    sm, oracle = helpers.load_package().srbd_model, helpers.load_oracle()
    p = sm.SrbdParams()
    if a.terrain:
        TERRAIN = TH.stairs_terrain(sm)
        global CASES
        CASES = [(c, 0.0) for c in ("none", "box_u")]  # the terrain test's cases

    def sel(h):  # the selection margin in cell^2
        return h["select_margin"] / TERRAIN.cell ** 2

    def set_robots(seed):
        global ROBOTS
        if a.robots:
            model = BH.draw(p, B, seed + 100)
            ROBOTS = (model, BH.draw_plant(model, seed + 200))
    if a.search:
        for seed in range(a.search[0], a.search[1]):
            set_robots(seed)
            _, c = conditions(sm, oracle, p, seed)
            ok = all(m >= 1e-6 and len(its) >= 2 for m, its, _ in c.values())
            extra = ""
            if a.terrain:
                ok = ok and all(sel(h) >= 1e-6 for _, _, h in c.values())
                extra = {k: f"select {sel(h):.1e}" for k, (_, _, h) in c.items()}
            print(seed, "OK " if ok else "-- ", {k: (f"{m:.1e}", its) for k, (m, its, _) in c.items()}, extra,
                  flush=True)
        return
    set_robots(a.seed)
    inputs, c = conditions(sm, oracle, p, a.seed)
    xs, us, x = inputs[:3]
    for case in CASES:
        margin, its, base = c[case]
        print(f"{case}: margin {margin:.2e}, sqp iterations {its}\n{base['sqp_iter']}")
        dx, du, df = np.zeros(T), np.zeros(T), np.zeros(T)
        if a.terrain:
            print(f"  selection margin {sel(base):.2e} cell^2, chosen candidates of row 0\n{base['q_log']}")
        for d in range(a.draws):
            rng = np.random.default_rng([a.seed, d])
            pert = lambda v: v * (1.0 + 1e-7 * rng.choice([-1.0, 1.0], size=v.shape))
            h = run(sm, oracle, p, case, (pert(xs), pert(us), pert(x)) + tuple(inputs[3:]))
            same = np.array_equal(h["sqp_iter"], base["sqp_iter"])
            dx = np.maximum(dx, np.abs(h["x_log"][:, 1:] - base["x_log"][:, 1:]).max(axis=(0, 2)))
            du = np.maximum(du, np.abs(h["u_log"] - base["u_log"]).max(axis=(0, 2)))
            print(f"  draw {d}: same iteration counts {same}")
            if a.terrain:
                df = np.maximum(df, np.abs(h["foot_log"] - base["foot_log"]).max(axis=(0, 2, 3)))
                print(f"  draw {d}: same chosen candidates {np.array_equal(h['q_log'], base['q_log'])}")
        fmt = lambda v: "(" + ", ".join(f"{e:.1e}" for e in v) + ")"
        print(f"    {case!r}: ({fmt(dx)}, {fmt(du)}" + (f", {fmt(df)}" if a.terrain else "") + "),")
        if ROBOTS:
            both = ROBOTS
            ROBOTS = (both[0], both[0])
            same_plant = run(sm, oracle, p, case, inputs)
            ROBOTS = both
            print(f"    plant != model moves x_log by {np.abs(base['x_log'] - same_plant['x_log']).max():.2e}")


if __name__ == "__main__":
    main()
