"""TEST INFRASTRUCTURE ONLY -- the terrains of the terrain tests, generated from seeds, and the
host closed loop with terrain that the replanning device rollout is compared against: per tick
srbd_model.gait_plan(terrain=...) from the measured state, then the host SQP loop of
tests/nmpc_plan_host.py on that window, then srbd_model.plant_step and srbd_model.shift_guess
(tests/gait_host.py's loop with the terrain under the planner)."""
from __future__ import annotations

import numpy as np

import gait_host as GH
import nmpc_plan_host as PH

__all__ = ["flat0", "plane", "stairs", "rough", "lipschitz", "nominal", "selection", "closed_loop",
           "stairs_terrain", "stairs_level", "stairs_case", "STAIRS"]


# ---- the terrains: height arrays [ny][nx]; sample (j, i) lies at (x0 + i cell, y0 + j cell) ----
def flat0(ny, nx):
    return np.zeros((ny, nx))


def plane(ny, nx, x0, y0, cell, alpha, beta, gamma):
    """H[j][i] = alpha x_i + beta y_j + gamma: the bilinear is exact on it."""
    xs, ys = x0 + cell * np.arange(nx), y0 + cell * np.arange(ny)
    return alpha * xs[None, :] + beta * ys[:, None] + gamma


def stairs(ny, nx, run, rise, first=0):
    """Treads of `run` samples along x, each `rise` above the one before; the riser is the cell
    between the last sample of a tread and the first of the next.  Tread 0 ends at sample `first`."""
    level = np.maximum(0, (np.arange(nx) - first - 1 + run) // run)
    return np.tile(rise * level.astype(np.float64), (ny, 1))


def rough(ny, nx, seed, amplitude=0.03):
    """Uniform random heights in [0, amplitude)."""
    return np.random.default_rng(seed).uniform(0.0, amplitude, size=(ny, nx))


def lipschitz(height, cell):
    """G: the largest difference between adjacent samples over cell.  The bilinear changes by at
    most G (|dx| + |dy|) between two points."""
    H = np.asarray(height, dtype=np.float64)
    H = H[None] if H.ndim == 2 else H
    return max(np.abs(np.diff(H, axis=1)).max(), np.abs(np.diff(H, axis=2)).max()) / cell


# ---- what the planner selected, restated from the planner without terrain ----
def nominal(sm, p, gait, cmd, x, tick, ref_pose, foot_now, N):
    """(n [B][N][2][2], down [B][N][2]): the nominal footholds, which are the feet's xy of the
    planner without terrain, and the rows that hold foot_now instead of a touchdown."""
    B = np.asarray(cmd).shape[0]
    w = sm.gait_plan(p, gait, cmd, x, tick, ref_pose, foot_now, N)[0]
    period, swing, offset = (np.broadcast_to(np.asarray(v, dtype=np.int64), s) for v, s in
                             zip((gait.period, gait.swing, gait.offset), ((B,), (B, 2), (B, 2))))
    down = GH.schedule(period, swing, offset, tick, N)[2]
    return np.stack([w.foot_r[:, :, 0:2], w.foot_l[:, :, 0:2]], axis=2), down


def selection(sm, p, gait, terrain, cmd, x, tick, ref_pose, foot_now, N, map_r=None):
    """(q [B][N][2] the chosen candidate of every row's touchdown, -1 where the row holds
    foot_now; margin: the smallest gap between the best and the second-best cost over all
    touchdowns, inf where nothing is selected; n, down of nominal())."""
    n, down = nominal(sm, p, gait, cmd, x, tick, ref_pose, foot_now, N)
    maps = terrain.map_r if map_r is None else map_r
    maps = np.zeros(n.shape[0], dtype=np.int64) if maps is None else np.asarray(maps, dtype=np.int64)
    _, _, q, margin = sm.foothold_select(terrain, n, maps[:n.shape[0], None, None])
    return np.where(down, -1, q), np.where(down, np.inf, margin).min(initial=np.inf), n, down


# ---- the host closed loop ----
def closed_loop(sm, oracle, p, gait, terrain, cmd, xs, us, x, alpha, ref_pose, foot_now, ticks, settings,
                sqp_max_loop, constraints="none", tick0=0, alpha_reset=0.0):
    """gait_host.closed_loop with the terrain under the planner.  Returns its dict plus q_log
    [B][ticks][2] (the chosen candidate of row 0's touchdown, -1 for a foot that is down),
    select_margin (the smallest best-to-second-best cost gap over every touchdown of every tick)
    and poses / feet (ref_pose and foot_now after each tick's planning step)."""
    B, N = us.shape[0], us.shape[1]
    xs, us, x = xs.copy(), us.copy(), x.copy()
    alpha = np.array(alpha, dtype=np.float64)
    ref_pose, foot_now = np.array(ref_pose, dtype=np.float64), np.array(foot_now, dtype=np.float64)
    x_log = np.empty((B, ticks + 1, 12))
    u_log = np.empty((B, ticks, 12))
    it_log = np.zeros((B, ticks), dtype=np.int32)
    cv_log = np.zeros((B, ticks), dtype=np.int32)
    foot_log = np.empty((B, ticks, 2, 3))
    fz_log = np.empty((B, ticks, 2))
    q_log = np.empty((B, ticks, 2), dtype=np.int64)
    x_log[:, 0] = x
    margin, select_margin, steps, windows, poses, feet = np.inf, np.inf, [], [], [], []
    for t in range(ticks):
        q, m, _, _ = selection(sm, p, gait, terrain, cmd[:, t], x, tick0 + t, ref_pose, foot_now, N)
        q_log[:, t], select_margin = q[:, 0], min(select_margin, m)
        w, ref_pose, foot_now = sm.gait_plan(p, gait, cmd[:, t], x, tick0 + t, ref_pose, foot_now, N,
                                             terrain=terrain)
        windows.append(w)
        poses.append(ref_pose)
        feet.append(foot_now)
        if alpha_reset > 0.0:
            alpha[:] = alpha_reset
        res = [PH.sqp_loop(sm, oracle, p, w.robot(i), xs[i], us[i], x[i], float(alpha[i]), settings,
                           sqp_max_loop, constraints) for i in range(B)]
        steps.append(res)
        xs = np.stack([r[0] for r in res])
        us = np.stack([r[1] for r in res])
        alpha = np.array([r[2] for r in res], dtype=np.float64)
        it_log[:, t] = [r[3] for r in res]
        cv_log[:, t] = [int(r[4]) for r in res]
        margin = min([margin] + [r[5] for r in res])
        foot_log[:, t, 0], foot_log[:, t, 1], fz_log[:, t] = w.foot_r[:, 0], w.foot_l[:, 0], w.fz_max[:, 0]
        u0 = us[:, 0].copy()
        x = sm.plant_step(x, u0, p, w.foot_r[:, 0], w.foot_l[:, 0], None, 1)
        xs, us = sm.shift_guess(xs, us, p, w)
        u_log[:, t] = u0
        x_log[:, t + 1] = x
    return dict(x_log=x_log, u_log=u_log, sqp_iter=it_log, converged=cv_log, xs=xs, us=us, x=x, alpha=alpha,
                margin=margin, steps=steps, foot_log=foot_log, fz_log=fz_log, ref_pose=ref_pose,
                foot_now=foot_now, windows=windows, q_log=q_log, select_margin=select_margin,
                poses=poses, feet=feet)


# the stairs the closed-loop tests walk up: 2 cm cells, treads of three samples (6 cm), 3 cm risers
STAIRS = dict(ny=9, nx=40, x0=0.2, y0=-0.4, cell=0.02, run=3, rise=0.03, first=14)


def stairs_terrain(sm, search=1, w_rough=10.0, map_r=None):
    s = STAIRS
    return sm.SrbdTerrain(height=stairs(s["ny"], s["nx"], s["run"], s["rise"], s["first"]), x0=s["x0"], y0=s["y0"],
                          cell=s["cell"], map_r=map_r, search=search, w_rough=w_rough)


def stairs_level(x):
    """The tread under x (its index; -1 on a riser), from STAIRS' definition and not the sampler."""
    s = STAIRS
    u = (np.asarray(x, dtype=np.float64) - s["x0"]) / s["cell"]  # in samples
    i = np.floor(u).astype(np.int64)
    lo = np.maximum(0, (i - s["first"] - 1 + s["run"]) // s["run"])
    hi = np.maximum(0, (i + 1 - s["first"] - 1 + s["run"]) // s["run"])
    return np.where((lo == hi) | (u == i), lo, -1)


def stairs_case(sm, p, B, N, T, seed, vx=1.0):
    """gait_host.walking_case's robots and gait, commanded straight up the stairs: vx for every
    robot, no lateral velocity and no yaw rate.  Returns walking_case's tuple."""
    xs, us, x, alpha, gait, cmd, ref_pose, foot_now = GH.walking_case(sm, p, B, N, T, seed)
    cmd[:, :, 0], cmd[:, :, 1], cmd[:, :, 2] = vx, 0.0, 0.0
    return xs, us, x, alpha, gait, cmd, ref_pose, foot_now
